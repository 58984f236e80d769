// am_dispatch.h -- which template instantiation a run-time value selects.  Plain C++17, no HIP: a host compiler builds it alone
// (tests/helpers/dispatch_check.cc).  The launchers pass a generic lambda; it receives the values as std::integral_constant
// and names the kernel with them: am_k_extract_slice<decltype(fix)::value, decltype(gate)::value, decltype(lf)::value>.
#ifndef AM_DISPATCH_H
#define AM_DISPATCH_H

#include <atomic>
#include <type_traits>

// The slicing kernels <FIX, GATE>.  fix_bits: 0, 1, anything else = 2 wrong bits repaired.  gate: 0 = off, 2 = on with the
// address repair, anything else = on.
template <class F>
void am_with_fix_gate(int fix_bits, int gate, F &&f)
{
    using std::integral_constant;
    if (fix_bits == 0) {
        if (gate == 2) f(integral_constant<int, 0>{}, integral_constant<int, 2>{});
        else if (gate) f(integral_constant<int, 0>{}, integral_constant<int, 1>{});
        else f(integral_constant<int, 0>{}, integral_constant<int, 0>{});
    } else if (fix_bits == 1) {
        if (gate == 2) f(integral_constant<int, 1>{}, integral_constant<int, 2>{});
        else if (gate) f(integral_constant<int, 1>{}, integral_constant<int, 1>{});
        else f(integral_constant<int, 1>{}, integral_constant<int, 0>{});
    } else {
        if (gate == 2) f(integral_constant<int, 2>{}, integral_constant<int, 2>{});
        else if (gate) f(integral_constant<int, 2>{}, integral_constant<int, 1>{});
        else f(integral_constant<int, 2>{}, integral_constant<int, 0>{});
    }
}

// The slicing kernels <FIX, GATE, LF>: the same, and long_mask (am_set_long_formats): 0 = LF 0, the kernels as they are without
// the option; anything else = LF 1, which reads the enabled formats from the context's device block.
template <class F>
void am_with_fix_gate_long(int fix_bits, int gate, int long_mask, F &&f)
{
    am_with_fix_gate(fix_bits, gate, [&](auto fix, auto g) {
        if (long_mask) f(fix, g, std::integral_constant<int, 1>{});
        else f(fix, g, std::integral_constant<int, 0>{});
    });
}

// The samples per chip am_k_extract_slice_iq<SPC, ...> is instantiated for: the rates the streaming front ends serve.
// false, and f is not called: no such instantiation.
template <class F>
bool am_with_spc(int spc, F &&f)
{
    using std::integral_constant;
    switch (spc) {
    case 32: f(integral_constant<int, 32>{}); return true;
    case 20: f(integral_constant<int, 20>{}); return true;
    case 16: f(integral_constant<int, 16>{}); return true;
    case 10: f(integral_constant<int, 10>{}); return true;
    case 8: f(integral_constant<int, 8>{}); return true;
    case 4: f(integral_constant<int, 4>{}); return true;
    case 5: f(integral_constant<int, 5>{}); return true;
    case 2: f(integral_constant<int, 2>{}); return true;
    case 1: f(integral_constant<int, 1>{}); return true;
    default: return false;
    }
}

// One small cache per device (a process may hold contexts on several) and per instantiation: every distinct Key -- the kernel
// whose property is cached -- has storage of its own, zero at start.  Devices at or beyond AM_DISPATCH_DEVICES are not cached.
#define AM_DISPATCH_DEVICES 64
template <class Key>
std::atomic<int> *am_device_cache(int dev)
{
    static std::atomic<int> cache[AM_DISPATCH_DEVICES];
    return dev >= 0 && dev < AM_DISPATCH_DEVICES ? &cache[dev] : nullptr;
}

#endif
