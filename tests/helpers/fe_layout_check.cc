// Host-side check of am_fe_plan / am_fe_layout (am_internal.h): the ONE description of the bitmap a streaming front end leaves,
// against the three derivations it replaced -- restated here as they stood (the front-end launchers' grid / steps per workgroup /
// n_long, am_capi.hip's fe_* words, am_launch_refine_seg's short segment) -- and against what any layout must satisfy.
// Built and run by tests/test_fe_layout.py against tests/emu/hip/hip_runtime.h, with am_fe3.hip / am_fe4.hip compiled as C++.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "am_internal.h"

int am_device_cus(void) { return 256; }      // (am_kernels.hip is not linked; the planning function never asks)

namespace {

struct Before {
    // the launchers' out-parameters and launch
    unsigned nsteps, spw, nlong, grid, a_n_long;
    // am_capi.hip's context words
    uint32_t fe_vspan, fe_nv, fe_nlong, fe_wps, fe_lag, fe_wbits, fe_nwg, fe_wpw, fe_nwords;
    // am_launch_refine_seg
    uint32_t rs_n_long, words_short, vspan_short;
    bool rs_invalid;
};

Before before(int spc, long long out_n, unsigned resident, bool asked)
{
    Before b = {};
    unsigned nsteps = 0, spw = 1, nlong = 0;
    unsigned *n_long = asked ? &nlong : nullptr;
    unsigned grid = 0, a_n_long = 0;
    if (spc == 32) {
        // am_launch_fe3 (FE3_LAG * FE3_SPC = 288, FE3_T = 3072)
        const unsigned a_nsteps = (unsigned)((out_n + 9 * 32 + 3072 - 1) / 3072);
        nsteps = a_nsteps;
        spw = 1;
        if (a_nsteps != 0) {
            spw = (a_nsteps + resident - 1) / resident;
            if (spw < 4) spw = 4;
            grid = (a_nsteps + spw - 1) / spw;
            a_n_long = grid;
            if (n_long) {
                unsigned G = a_nsteps / 4u;
                G = G < 1u ? 1u : (G > resident ? resident : G);
                const unsigned lo = a_nsteps / G, r = a_nsteps - lo * G;
                grid = G;
                if (r == 0) { spw = lo; a_n_long = G; }
                else { spw = lo + 1u; a_n_long = r; }
                *n_long = a_n_long;
            }
        }
    } else {
        // am_launch_fe4 + fe4_launch (n_long is not written)
        const long long T = am_fe4_tile(spc);
        const unsigned a_nsteps = T ? (unsigned)((out_n + am_fe4_lag(spc) + T - 1) / T) : 0u;
        nsteps = a_nsteps;
        spw = 1;
        if (a_nsteps != 0) {
            spw = (a_nsteps + resident - 1) / resident;
            if (spw < 4) spw = 4;
            grid = (a_nsteps + spw - 1) / spw;
        }
    }
    b.nsteps = nsteps; b.spw = spw; b.nlong = nlong; b.grid = grid; b.a_n_long = a_n_long;
    // am_capi.hip
    const unsigned wps = am_fe4_words(spc) * am_fe4_waves(spc);
    b.fe_vspan = spw * am_fe4_tile(spc);
    b.fe_nv = (nsteps + spw - 1) / spw;
    b.fe_nlong = 0;
    b.fe_wps = wps;
    if (nlong && spw > 1) {
        const unsigned rest = nsteps > nlong * spw ? nsteps - nlong * spw : 0u;
        b.fe_nv = nlong + (rest + (spw - 1) - 1) / (spw - 1);
        b.fe_nlong = nlong;
    }
    b.fe_lag = am_fe4_lag(spc);
    b.fe_wbits = am_fe4_unit(spc);
    b.fe_nwg = b.fe_nv;
    b.fe_wpw = spw * wps;
    b.fe_nwords = nsteps * wps;
    // am_launch_refine_seg(nwg = fe_nwg, n_long = fe_nlong, words_per_wg = fe_wpw, words_per_step = fe_wps, vspan = fe_vspan)
    {
        const uint32_t nwg = b.fe_nwg, n_long_in = b.fe_nlong, words_per_wg = b.fe_wpw, words_per_step = b.fe_wps, vspan = b.fe_vspan;
        b.rs_n_long = (n_long_in == 0 || n_long_in > nwg) ? nwg : n_long_in;
        b.rs_invalid = b.rs_n_long < nwg && (words_per_step == 0 || words_per_step >= words_per_wg);
        b.words_short = b.rs_n_long < nwg ? words_per_wg - words_per_step : words_per_wg;
        b.vspan_short = (b.rs_n_long < nwg && words_per_wg) ? (uint32_t)((unsigned long long)vspan * b.words_short / words_per_wg) : vspan;
    }
    return b;
}

long long cases = 0;
int bad = 0;

#define WANT(cond)                                                                                                            \
    do {                                                                                                                      \
        if (!(cond)) {                                                                                                        \
            if (bad++ < 20) printf("spc %d out_n %lld resident %u levelled %d: %s\n", spc, out_n, resident, (int)asked, #cond); \
            return;                                                                                                           \
        }                                                                                                                     \
    } while (0)

void check(int spc, long long out_n, unsigned resident, bool asked)
{
    cases++;
    const am_fe_layout l = am_fe_plan(spc, out_n, resident, asked);
    const Before b = before(spc, out_n, resident, asked);
    // every field and accessor against the three earlier derivations
    WANT(l.nsteps == b.nsteps && l.spw == b.spw);
    WANT(l.wbits == b.fe_wbits && l.lag == b.fe_lag && l.wps == b.fe_wps && l.tile == am_fe4_tile(spc));
    WANT(l.nwg == b.grid && l.nwg == b.fe_nwg && l.nv() == b.fe_nv);
    if (spc == 32 && b.nsteps) WANT(l.n_long == b.a_n_long);                  // what am_k_fe3 is told
    WANT((l.alike() ? l.nwg : l.n_long) == b.rs_n_long);                       // what am_k_refine_seg is told
    WANT(asked && spc == 32 ? true : l.alike());                               // levelled only where am_k_fe3 runs and the caller asks
    WANT(l.words_per_wg() == b.fe_wpw && l.nwords() == b.fe_nwords && l.vspan() == b.fe_vspan);
    WANT(!b.rs_invalid);
    WANT(l.words_short() == b.words_short && l.vspan_short() == b.vspan_short);
    // ... and on its own
    WANT(l.tile == l.wps * l.wbits && l.nwords() == l.nsteps * l.wps);
    WANT((l.nsteps == 0) == (l.nwg == 0));
    if (l.nsteps == 0) return;
    WANT(l.spw >= 1 && l.n_long >= 1 && l.n_long <= l.nwg && l.steps_short() >= 1 && l.spw - l.steps_short() <= 1);
    // segments, as the kernels place them (am_k_fe3: sb / mine; am_k_refine_seg: seg_b / seg_w): long ones first, each with a
    // step of its own, together exactly [0, nsteps); only the last segment of an unlevelled grid may be cut by the end
    unsigned long long next = 0, words = 0;
    for (uint32_t g = 0; g < l.nwg; ++g) {
        const bool lng = g < l.n_long;
        const unsigned long long s0 = lng ? (unsigned long long)g * l.spw : (unsigned long long)l.n_long * l.spw + (unsigned long long)(g - l.n_long) * l.steps_short();
        const unsigned long long len = lng ? l.spw : l.steps_short();
        WANT(s0 == next && s0 < l.nsteps);
        unsigned long long s1 = s0 + len;
        if (s1 > l.nsteps) { WANT(g == l.nwg - 1 && l.alike()); s1 = l.nsteps; }
        const unsigned long long w0 = lng ? (unsigned long long)g * l.words_per_wg() : (unsigned long long)l.n_long * l.words_per_wg() + (unsigned long long)(g - l.n_long) * l.words_short();
        WANT(w0 == s0 * l.wps);
        words += (s1 - s0) * l.wps;
        next = s1;
    }
    WANT(next == l.nsteps && words == l.nwords());
}

}   // namespace

int main()
{
    static const int spcs[] = {1, 2, 4, 5, 8, 10, 16, 20, 32};
    static const unsigned residents[] = {1, 2, 3, 256, 1280, 1536, 2048};
    for (int spc : spcs) {
        const long long T = am_fe4_tile(spc), lag = am_fe4_lag(spc);
        if (!am_fe4_supported(spc) || T <= 0) { printf("spc %d has no streaming front end\n", spc); return 1; }
        for (unsigned R : residents)
            for (int lev = 0; lev < 2; ++lev) {
                auto steps = [&](long long k) {
                    if (k < 0) return;
                    // the shortest and the longest out_n with k steps, and one in between
                    check(spc, k * T - lag, R, lev != 0);
                    if (k > 0) { check(spc, (k - 1) * T - lag + 1, R, lev != 0); check(spc, k * T - lag - T / 3, R, lev != 0); }
                };
                for (long long k = 0; k <= 40; ++k) steps(k);
                for (long long m : {4ll, 13ll, 14ll})
                    for (long long d = -2; d <= 2; ++d) steps(m * (long long)R + d);
                check(spc, 64ll << 20, R, lev != 0);
                check(spc, 0, R, lev != 0);
            }
    }
    if (bad) printf("FAILED %d of %lld layouts\n", bad, cases);
    else printf("%lld layouts\nok\n", cases);
    return bad ? 1 : 0;
}
