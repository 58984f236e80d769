// am_options.h on its own, with a host compiler: every accepted value of every option is stored, the first value outside each
// end of a range is refused with a message and leaves the value bytewise as it was (tests/test_options.py builds and runs this).
#include "am_options.h"

#include <initializer_list>
#include <limits>
#include <stdio.h>
#include <string.h>

static int bad = 0;

// a value with known bytes everywhere (padding too), settings that are nobody's default
static void fresh(am_decode_opts &o)
{
    memset(static_cast<void *>(&o), 0x5a, sizeof(o));
    o.fix_bits = 1; o.long_mask = 2; o.gate_mode = 2; o.gate_ttl_s = 0.125; o.gate_repair = 1;
}

// f refuses: a non-empty message, and no byte of the value moves
template <class F>
static void refused(const char *what, double v, F f)
{
    am_decode_opts o, before;
    fresh(o);
    memcpy(&before, &o, sizeof(o));
    const char *msg = f(o);
    if (!msg || !*msg) { printf("%s %g: accepted, or refused without a message\n", what, v); bad++; }
    if (memcmp(&before, &o, sizeof(o)) != 0) { printf("%s %g: refused, but the value changed\n", what, v); bad++; }
}

// f accepts: no message, `member` holds v, every other member is what fresh() left
static void stored(const char *what, double v, const am_decode_opts &o, const char *msg, const am_decode_opts &want)
{
    if (msg) { printf("%s %g: refused (%s)\n", what, v, msg); bad++; return; }
    if (o.fix_bits != want.fix_bits || o.long_mask != want.long_mask || o.gate_mode != want.gate_mode ||
        memcmp(&o.gate_ttl_s, &want.gate_ttl_s, sizeof(double)) != 0 || o.gate_repair != want.gate_repair) {
        printf("%s %g: accepted, but not stored (or another member moved)\n", what, v);
        bad++;
    }
}

int main()
{
    const am_decode_opts d;
    if (d.fix_bits != 0 || d.long_mask != 0 || d.gate_mode != 0 || d.gate_ttl_s != 60.0 || d.gate_repair != 0) {
        printf("the defaults are not 0, 0, 0, 60.0, 0\n");
        bad++;
    }
    am_decode_opts o, want;
    for (int v = 0; v <= 2; v++) {
        fresh(o); fresh(want); want.fix_bits = v;
        stored("fix_errors", v, o, am_opt_fix_errors(o, v), want);
    }
    for (int v : {-1, 3}) refused("fix_errors", v, [v](am_decode_opts &x) { return am_opt_fix_errors(x, v); });

    for (int v = 0; v <= (AM_LF_DF18 | AM_LF_DF19); v++) {
        fresh(o); fresh(want); want.long_mask = v;
        stored("long_formats", v, o, am_opt_long_formats(o, v), want);
    }
    for (int v : {-1, (AM_LF_DF18 | AM_LF_DF19) + 1}) refused("long_formats", v, [v](am_decode_opts &x) { return am_opt_long_formats(x, v); });

    for (int v = 0; v <= 1; v++) {
        fresh(o); fresh(want); want.gate_repair = v;
        stored("address_repair", v, o, am_opt_address_repair(o, v), want);
    }
    for (int v : {-1, 2}) refused("address_repair", v, [v](am_decode_opts &x) { return am_opt_address_repair(x, v); });

    // the gate: every mode with a ttl that is nobody's, the smallest positive double included; a refused mode leaves the ttl
    // alone, a refused ttl the mode
    const double inf = std::numeric_limits<double>::infinity(), tiny = std::numeric_limits<double>::denorm_min();
    for (int v = 0; v <= 2; v++)
        for (double ttl : {60.0, 0.5, tiny, std::numeric_limits<double>::max()}) {
            fresh(o); fresh(want); want.gate_mode = v; want.gate_ttl_s = ttl;
            stored("address_gate mode", v, o, am_opt_address_gate(o, v, ttl), want);
        }
    for (int v : {-1, 3}) refused("address_gate mode", v, [v](am_decode_opts &x) { return am_opt_address_gate(x, v, 7.0); });
    for (double ttl : {std::numeric_limits<double>::quiet_NaN(), inf, -inf, 0.0, -0.0, -1.0, -tiny})
        for (int v = 0; v <= 2; v++) refused("address_gate ttl", ttl, [v, ttl](am_decode_opts &x) { return am_opt_address_gate(x, v, ttl); });

    if (bad) return 1;
    printf("ok\n");
    return 0;
}
