// am_options.h -- the opt-in decode options as one value, and the one place that knows their ranges and messages.  Plain C++17,
// no HIP: a host compiler builds it alone (tests/helpers/options_check.cc).
//
// Every handle -- am_ctx, am_pipe, am_spipe -- holds one am_decode_opts, and every am_*set_* call of am_capi.hip goes through
// the function of its option below: it either updates the value and returns null, or returns the message and leaves the value
// as it was.
#ifndef AM_OPTIONS_H
#define AM_OPTIONS_H

#include <cmath>

#include "airmodes_hip.h"

struct am_decode_opts {
    int fix_bits = 0;           // am_set_fix_errors: wrong bits a DF11 / DF17 reply may be repaired of (0: none, the reference's :179-182)
    int long_mask = 0;          // am_set_long_formats: formats beyond the reference's four that are sliced as 112 bits (AM_LF_*)
    int gate_mode = 0;          // am_set_address_gate: 0: off; 1: address/parity replies need a taught address; 2: and reserved formats are dropped
    double gate_ttl_s = 60.0;   // ... how long a taught address lives, seconds
    int gate_repair = 0;        // am_set_address_repair: 0: off; 1: on (inert while gate_mode is 0)
};

inline const char *am_opt_fix_errors(am_decode_opts &o, int max_bits)
{
    if (max_bits < 0 || max_bits > 2) return "fix_errors: max_bits must be 0, 1 or 2";
    o.fix_bits = max_bits;
    return nullptr;
}

inline const char *am_opt_long_formats(am_decode_opts &o, int mask)
{
    if (mask < 0 || mask > (AM_LF_DF18 | AM_LF_DF19)) return "long_formats: mask must be an OR of AM_LF_DF18 and AM_LF_DF19";
    o.long_mask = mask;
    return nullptr;
}

inline const char *am_opt_address_gate(am_decode_opts &o, int mode, double ttl_seconds)
{
    if (mode < 0 || mode > 2) return "address_gate: mode must be 0, 1 or 2";
    if (!std::isfinite(ttl_seconds) || !(ttl_seconds > 0.0)) return "address_gate: ttl must be finite and positive";
    o.gate_mode = mode;
    o.gate_ttl_s = ttl_seconds;
    return nullptr;
}

inline const char *am_opt_address_repair(am_decode_opts &o, int max_bits)
{
    if (max_bits < 0 || max_bits > 1) return "address_repair: max_bits must be 0 or 1";
    o.gate_repair = max_bits;
    return nullptr;
}

#endif
