// am_dispatch.h on its own, with a host compiler: which instantiation every run-time value selects, and that every
// instantiation's per-device cache is its own (tests/test_dispatch.py builds and runs this).
#include "am_dispatch.h"

#include <stdio.h>

template <int A, int B> struct key {};

int main()
{
    int bad = 0;
    // <FIX, GATE>: fix_bits 0 -> 0, 1 -> 1, anything else -> 2; gate 0 -> 0, 2 -> 2, anything else -> 1
    for (int fix_bits = -1; fix_bits <= 4; fix_bits++)
        for (int gate = -1; gate <= 4; gate++) {
            const int want_f = fix_bits == 0 ? 0 : fix_bits == 1 ? 1 : 2;
            const int want_g = gate == 0 ? 0 : gate == 2 ? 2 : 1;
            int calls = 0, got_f = -1, got_g = -1;
            am_with_fix_gate(fix_bits, gate, [&](auto f, auto g) {
                calls++;
                got_f = decltype(f)::value;
                got_g = decltype(g)::value;
            });
            if (calls != 1 || got_f != want_f || got_g != want_g) {
                printf("fix_bits %d gate %d: %d call(s), <%d, %d>, expected <%d, %d>\n", fix_bits, gate, calls, got_f, got_g, want_f, want_g);
                bad++;
            }
        }
    // SPC: the nine rates of the extraction kernel, nothing else
    static const int rates[9] = {1, 2, 4, 5, 8, 10, 16, 20, 32};
    for (int spc = 0; spc <= 64; spc++) {
        bool supported = false;
        for (int r : rates) supported = supported || r == spc;
        int calls = 0, got = -1;
        const bool ret = am_with_spc(spc, [&](auto s) {
            calls++;
            got = decltype(s)::value;
        });
        if (ret != supported || calls != (supported ? 1 : 0) || (supported && got != spc)) {
            printf("spc %d: returned %d, %d call(s), <%d>\n", spc, (int)ret, calls, got);
            bad++;
        }
    }
    // the caches: one per key and device, zero at start, nothing beyond the table
    std::atomic<int> *a = am_device_cache<key<32, 0>>(0), *b = am_device_cache<key<32, 1>>(0), *c = am_device_cache<key<20, 0>>(0);
    if (!a || !b || !c || a == b || a == c || b == c || a != am_device_cache<key<32, 0>>(0) || a + 1 != am_device_cache<key<32, 0>>(1)) {
        printf("two instantiations share a cache, or one has two\n");
        bad++;
    } else {
        if (a->load() != 0 || b->load() != 0) { printf("a cache does not start at zero\n"); bad++; }
        a->store(5);
        am_device_cache<key<32, 0>>(AM_DISPATCH_DEVICES - 1)->store(7);
        if (b->load() != 0 || c->load() != 0 || am_device_cache<key<32, 1>>(AM_DISPATCH_DEVICES - 1)->load() != 0 ||
            am_device_cache<key<32, 0>>(0)->load() != 5) {
            printf("a store into one instantiation's cache shows in another's\n");
            bad++;
        }
    }
    if (am_device_cache<key<32, 0>>(-1) || am_device_cache<key<32, 0>>(AM_DISPATCH_DEVICES)) {
        printf("a device outside the table has a cache entry\n");
        bad++;
    }
    if (bad) return 1;
    printf("ok\n");
    return 0;
}
