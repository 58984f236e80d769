// am_gate.inc -- the address gate (am_set_address_gate; DESIGN.md 14), included by am_kernels.hip.
//
// The reference's slicer checks parity for DF11 and DF17 only (lib/slicer_impl.cc:170-182): in DF0/4/5/16/20/21 the parity is
// overlaid with the aircraft's address, the syndrome IS the address, and every bit pattern "passes".  With the gate on, such a
// reply is handed out only if its address was taught by a parity-clean DF11 / DF17 reply at most ttl item counts before it.
//
// The slicing wave (am_slice_wave<FIX, 1>) leaves one am_gate_rec per hit index in device memory: the packet array is pinned host
// memory and is never read back here.  Hit indices are in stream order, item counts ascend with them.  The kernels of one call:
//
//   (memset)          the call's table and its three counters are zeroed
//   am_k_gate_teach   every teaching record enters the CALL's table under (stream, address, window), window = item count / ttl:
//                     first = min item count (kept as max of the complement, so that zero is "none"), last = max item count + 1
//   am_k_gate_test    a test at item count s in window w passes iff
//                        the call taught the address in window w before s         (first < s: inside one window every teach is fresh)
//                     or the call taught it in window w - 1 and s - last <= ttl    (anything in w - 1 is before s; w - 2 is too old)
//                     or the context's map, taught by EARLIER calls, has it with s - last <= ttl;
//                     what fails, and with mode 2 every reserved format, loses packets[i].reserved[0] (a byte store to pinned
//                     memory, as the slicer's own reject)
//   am_k_gate_repair  only with am_set_address_repair: every address/parity reply the test failed is searched for the one bit whose
//                     flip makes its syndrome an address that is alive (the same three-way lookup); exactly one: the packet is
//                     rewritten and kept, and moves from the dropped counter to the repaired one
//   am_k_gate_ticket  am_k_ticket + the call's three counters for the host (am_k_gate_repair_ticket: five)
//
// and, only once the host has ACCEPTED the scan (a speculative scan that is repeated, or one that timed out, never gets here):
//
//   am_k_gate_commit  the call's teaching records enter the context's map: last[address] = max(last, item count + 1)
//
// so a repeated scan finds the map as the first try found it, and the call's table is rebuilt from nothing.  Order comes from
// the launch boundaries on the context's stream alone: integer atomics on 64-bit words, no fences.
//
// Both tables are open addressing with linear probing.  The call's table has no keys of its own: a slot is claimed with the
// index of the first record that hashed there (compare-and-swap on the owner word) and a key is compared by looking that record up,
// so (stream, address, window) needs no packing into 64 bits.  It has at least twice as many slots as the call can have
// records, so it never fills.  The context's map holds address + 1; when three quarters of its slots are taken a new address is
// not learned (the gate fails closed) and a counter says so.

#if defined(__HIP_MEMORY_SCOPE_AGENT)
#define AM_GATE_SCOPE __HIP_MEMORY_SCOPE_AGENT
#else
#define AM_GATE_SCOPE __HIP_MEMORY_SCOPE_SYSTEM
#endif

__device__ __forceinline__ unsigned long long am_gate_mix(unsigned long long x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// The stream a record belongs to and its item count there (what sort_into_streams does on the host, after the scan); false: the
// host will drop the packet -- it neither teaches nor counts.  K = 0: one stream, the item count is the record's.
__device__ __forceinline__ bool am_gate_locate(const am_gate_args &a, unsigned long long raw, uint32_t &j, unsigned long long &s)
{
    j = 0;
    s = raw;
    if (a.K == 0) return true;
    const unsigned long long pos = raw - a.hist0;
    uint32_t lo = 0, hi = a.K;                               // first offset > pos
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.moff[mid] <= pos) lo = mid + 1; else hi = mid;
    }
    if (lo == 0) return false;
    j = lo - 1;
    const unsigned long long e = pos - a.moff[j];
    if (a.mem[j] < 0 || e > (unsigned long long)a.mem[j]) return false;
    s = e + a.hist0;
    return true;
}

// slot of (j, addr, w) in the call's table, ~0u if it has none; claim = record index + 1: a free slot is taken for it
__device__ __forceinline__ uint32_t am_gate_slot(const am_gate_args &a, uint32_t j, uint32_t addr, unsigned long long w, uint32_t claim)
{
    uint32_t h = (uint32_t)am_gate_mix((((unsigned long long)j << 24) | addr) ^ am_gate_mix(w)) & a.s_mask;
    for (uint32_t probe = 0; probe <= a.s_mask; ++probe, h = (h + 1) & a.s_mask) {
        unsigned long long o = __hip_atomic_load(&a.s_owner[h], __ATOMIC_RELAXED, AM_GATE_SCOPE);
        if (o == 0ull) {
            if (!claim) return ~0u;
            unsigned long long expected = 0ull;
            if (__hip_atomic_compare_exchange_strong(&a.s_owner[h], &expected, (unsigned long long)claim, __ATOMIC_RELAXED,
                                                     __ATOMIC_RELAXED, AM_GATE_SCOPE))
                return h;
            o = expected;                                    // somebody else's record got the slot: is it our key?
        }
        const am_gate_rec r = a.rec[o - 1ull];               // (written by the slicing launch; an owner passed am_gate_locate)
        uint32_t jo;
        unsigned long long so;
        (void)am_gate_locate(a, r.sample, jo, so);
        if (jo == j && r.addr == addr && so / a.ttl == w) return h;
    }
    return ~0u;
}

__global__ void __launch_bounds__(256) am_k_gate_teach(am_gate_args a)
{
    const uint32_t n = a.n_ptr ? *a.n_ptr : a.n;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool taught = false;
    if (i < n) {
        const am_gate_rec r = a.rec[i];
        uint32_t j;
        unsigned long long s;
        if (r.cls == AM_GC_TEACH && am_gate_locate(a, r.sample, j, s)) {
            const uint32_t h = am_gate_slot(a, j, r.addr, s / a.ttl, i + 1u);
            if (h != ~0u) {
                atomicMax(&a.s_first[h], ~s);
                atomicMax(&a.s_last[h], s + 1ull);
            }
            taught = true;
        }
    }
    const unsigned long long m = __ballot(taught);
    if ((threadIdx.x & (AM_WAVE - 1)) == 0 && m) atomicAdd(&a.cnt[0], (unsigned long long)__popcll(m));
}

// Is address addr alive for stream j at item count s (window w = s / ttl)?  The three ways of the header: the call's table in
// window w, the call's table in window w - 1, the context's map.  The gate's own test and the repair's search ask here.
__device__ __forceinline__ bool am_gate_alive(const am_gate_args &a, uint32_t j, uint32_t addr, unsigned long long s)
{
    const unsigned long long w = s / a.ttl;
    uint32_t h = am_gate_slot(a, j, addr, w, 0u);
    if (h != ~0u && ~a.s_first[h] < s) return true;
    if (w > 0ull) {
        h = am_gate_slot(a, j, addr, w - 1ull, 0u);
        if (h != ~0u && s - (a.s_last[h] - 1ull) <= a.ttl) return true;
    }
    uint32_t t = (uint32_t)am_gate_mix(addr) & a.t_mask;     // the context's map: what earlier calls of this stream taught
    for (uint32_t probe = 0; probe <= a.t_mask; ++probe, t = (t + 1) & a.t_mask) {
        const unsigned long long k = a.t_key[t];
        if (k == 0ull) break;
        if (k == (unsigned long long)addr + 1ull) {
            const unsigned long long l = a.t_last[t];
            return l != 0ull && l - 1ull <= s && s - (l - 1ull) <= a.ttl;
        }
    }
    return false;
}

// REPAIR: 1 = the hit index of every address/parity record that fails goes onto the repair's list (am_k_gate_repair below; in any
// order: each entry is looked at on its own); 0 is the test alone.
template <int REPAIR>
__global__ void __launch_bounds__(256) am_k_gate_test(am_gate_args a)
{
    const uint32_t n = a.n_ptr ? *a.n_ptr : a.n;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool passed = false, dropped = false;
    if (i < n) {
        const am_gate_rec r = a.rec[i];
        uint32_t j;
        unsigned long long s;
        if (r.cls >= AM_GC_TEST && am_gate_locate(a, r.sample, j, s)) {
            bool keep;
            if (r.cls == AM_GC_OTHER) {
                keep = a.mode != 2;
            } else {
                keep = am_gate_alive(a, j, r.addr & 0xFFFFFFu, s);
                passed = keep;
                if constexpr (REPAIR > 0)
                    if (!keep) a.rl[AM_GATE_RL_HDR + atomicAdd(&a.rl[0], 1u)] = i;     // (at most n entries: one per record)
            }
            if (!keep) {
                a.packets[i].reserved[0] = 0;
                dropped = true;
            }
        }
    }
    const unsigned long long mp = __ballot(passed), md = __ballot(dropped);
    if ((threadIdx.x & (AM_WAVE - 1)) == 0) {
        if (mp) atomicAdd(&a.cnt[1], (unsigned long long)__popcll(mp));
        if (md) atomicAdd(&a.cnt[2], (unsigned long long)__popcll(md));
    }
}

// Repair of an address/parity reply with one wrong bit (am_set_address_repair; DESIGN.md 15).  The syndrome of such a reply is
// address ^ syn(j) when bit j is wrong, so crc ^ syn(j) is tried for every j = 5 .. nbits - 1 against the addresses that are alive
// where the reply stands; exactly one hit: the reply is that aircraft's with bit j flipped.  One wave per list entry, entries
// wave-strided over a fixed grid; lane l owns bits l and l + 64, as in am_slice_wave.  The record (am_slice_wave<FIX, 2>) carries
// the DF above the syndrome: DF16/20/21 are long.  Lane 0 of a wave that repairs reads the one data byte back from the packet
// array, which the slicing wave wrote in full (the packet was "ok" there); nothing else is ever read from it.
__global__ void __launch_bounds__(256) am_k_gate_repair(am_gate_args a)
{
    const int lane = threadIdx.x & (AM_WAVE - 1);
    const uint32_t nw = gridDim.x * (blockDim.x / AM_WAVE);
    const uint32_t n = a.rl[0];
    for (uint32_t k = blockIdx.x * (blockDim.x / AM_WAVE) + threadIdx.x / AM_WAVE; k < n; k += nw) {      // (wave-uniform)
        const uint32_t i = a.rl[AM_GATE_RL_HDR + k];
        const am_gate_rec r = a.rec[i];
        uint32_t j;
        unsigned long long s;
        (void)am_gate_locate(a, r.sample, j, s);             // (it is on the list: am_k_gate_test located it)
        const uint32_t crc = r.addr & 0xFFFFFFu;
        const int nbits = (r.addr >> 24) & 16u ? 112 : 56;
        const bool h0 = lane >= 5 && lane < nbits && am_gate_alive(a, j, crc ^ a.crc_pow[nbits - 1 - lane], s);
        const bool h1 = lane + 64 < nbits && am_gate_alive(a, j, crc ^ a.crc_pow[nbits - 1 - (lane + 64)], s);
        const unsigned long long f0 = __ballot(h0), f1 = __ballot(h1);
        const int hits = __popcll(f0) + __popcll(f1);
        if (lane != 0 || hits == 0) continue;
        if (hits > 1) {
            atomicAdd(&a.rl[2], 1u);
            continue;
        }
        const int b = f0 ? __ffsll((long long)f0) - 1 : 63 + __ffsll((long long)f1);
        am_packet *p = a.packets + i;
        p->data[b >> 3] = (uint8_t)(p->data[b >> 3] ^ (0x80u >> (b & 7)));
        p->crc = crc ^ a.crc_pow[nbits - 1 - b];
        p->reserved[1] = 1;
        p->reserved[0] = 1;
        atomicAdd(&a.cnt[2], ~0ull);                         // no longer dropped ...
        atomicAdd(&a.rl[1], 1u);                             // ... but repaired
    }
}

// the teaching records of a scan the host has accepted enter the context's map (one stream: never launched for K streams, whose
// maps end with the call).  DEV_N = 1 (am_spipe, DESIGN.md 16): the chunk's records enter the pipe's RUNNING map as soon as the
// chunk's own test and repair are through -- the count is still on the device (a.n is the bound the launch was sized for)
template <int DEV_N>
__global__ void __launch_bounds__(256) am_k_gate_commit(am_gate_args a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (DEV_N > 0) {
        const uint32_t n = *a.n_ptr;
        if (i >= (n < a.n ? n : a.n)) return;
    } else if (i >= a.n) return;
    const am_gate_rec r = a.rec[i];
    if (r.cls != AM_GC_TEACH) return;
    const unsigned long long key = (unsigned long long)r.addr + 1ull;
    uint32_t t = (uint32_t)am_gate_mix(r.addr) & a.t_mask;
    for (uint32_t probe = 0; probe <= a.t_mask; ++probe, t = (t + 1) & a.t_mask) {
        unsigned long long k = __hip_atomic_load(&a.t_key[t], __ATOMIC_RELAXED, AM_GATE_SCOPE);
        if (k == 0ull) {
            if (__hip_atomic_load(&a.t_hdr[0], __ATOMIC_RELAXED, AM_GATE_SCOPE) >= a.t_limit) break;    // full: not learned
            unsigned long long expected = 0ull;
            if (__hip_atomic_compare_exchange_strong(&a.t_key[t], &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, AM_GATE_SCOPE)) {
                atomicAdd(&a.t_hdr[0], 1ull);
                k = key;
            } else {
                k = expected;
            }
        }
        if (k == key) {
            atomicMax(&a.t_last[t], r.sample + 1ull);
            return;
        }
    }
    atomicAdd(&a.t_hdr[1], 1ull);
}

// am_k_ticket for a scan with the gate: the call's counters (taught, passed, dropped) travel with the ticket.
// cnt_dst = the context's pinned block from AM_PW_GATE_TAUGHT on
#define AM_GATE_DST(word) ((word) - AM_PW_GATE_TAUGHT)
__global__ void am_k_gate_ticket(uint32_t *host_word, uint32_t seq, const unsigned long long *cnt, uint32_t *cnt_dst)
{
    cnt_dst[AM_GATE_DST(AM_PW_GATE_TAUGHT)] = (uint32_t)cnt[0];
    cnt_dst[AM_GATE_DST(AM_PW_GATE_PASSED)] = (uint32_t)cnt[1];
    cnt_dst[AM_GATE_DST(AM_PW_GATE_DROPPED)] = (uint32_t)cnt[2];
    __hip_atomic_store(host_word, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ... and with the repair on, two more: repaired, ambiguous
__global__ void am_k_gate_repair_ticket(uint32_t *host_word, uint32_t seq, const unsigned long long *cnt, const uint32_t *rl,
                                        uint32_t *cnt_dst)
{
    cnt_dst[AM_GATE_DST(AM_PW_GATE_TAUGHT)] = (uint32_t)cnt[0];
    cnt_dst[AM_GATE_DST(AM_PW_GATE_PASSED)] = (uint32_t)cnt[1];
    cnt_dst[AM_GATE_DST(AM_PW_GATE_DROPPED)] = (uint32_t)cnt[2];
    cnt_dst[AM_GATE_DST(AM_PW_REPAIRED)] = rl[1];
    cnt_dst[AM_GATE_DST(AM_PW_AMBIGUOUS)] = rl[2];
    __hip_atomic_store(host_word, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ... and for a chunk of am_spipe, with what am_k_ticket carries for the pipe's resolve step: the redo flag and the word in which
// the scan leaves the chunk (rl null: no repair)
__global__ void am_k_gate_pipe_ticket(uint32_t *host_word, uint32_t seq, const unsigned long long *cnt, const uint32_t *rl,
                                      uint32_t *cnt_dst, const uint32_t *flag_src, uint32_t *flag_dst,
                                      const unsigned long long *word_src, unsigned long long *word_dst)
{
    cnt_dst[AM_GATE_DST(AM_PW_GATE_TAUGHT)] = (uint32_t)cnt[0];
    cnt_dst[AM_GATE_DST(AM_PW_GATE_PASSED)] = (uint32_t)cnt[1];
    cnt_dst[AM_GATE_DST(AM_PW_GATE_DROPPED)] = (uint32_t)cnt[2];
    if (rl) {
        cnt_dst[AM_GATE_DST(AM_PW_REPAIRED)] = rl[1];
        cnt_dst[AM_GATE_DST(AM_PW_AMBIGUOUS)] = rl[2];
    }
    if (flag_src) *flag_dst = *flag_src;
    if (word_src) *word_dst = *word_src;
    __hip_atomic_store(host_word, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
#undef AM_GATE_DST

size_t am_gate_scratch_bytes(uint32_t slots) { return ((size_t)4 + (size_t)3 * slots) * sizeof(unsigned long long); }

void am_gate_scratch_layout(am_gate_args &a, void *scratch, uint32_t slots)
{
    unsigned long long *p = static_cast<unsigned long long *>(scratch);
    a.cnt = p;
    a.s_owner = p + 4;
    a.s_first = p + 4 + (size_t)slots;
    a.s_last = p + 4 + (size_t)2 * slots;
    a.s_mask = slots - 1u;
}

hipError_t am_launch_gate(const am_gate_args &a, uint32_t n_max, hipStream_t s)
{
    hipError_t rc = hipMemsetAsync(a.cnt, 0, am_gate_scratch_bytes(a.s_mask + 1u), s);
    if (rc == hipSuccess && a.rl) rc = hipMemsetAsync(a.rl, 0, AM_GATE_RL_HDR * sizeof(uint32_t), s);     // (the ticket reads them)
    if (rc != hipSuccess || n_max == 0) return rc;
    hipLaunchKernelGGL(am_k_gate_teach, dim3(am_grid(n_max, 256)), dim3(256), 0, s, a);
    if (!a.rl) {
        hipLaunchKernelGGL(am_k_gate_test<0>, dim3(am_grid(n_max, 256)), dim3(256), 0, s, a);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(am_k_gate_test<1>, dim3(am_grid(n_max, 256)), dim3(256), 0, s, a);
    // a fixed, modest grid: a scan fails some hundreds of address/parity replies, and each costs one wave a few probes per lane
    const uint32_t waves = n_max < 256u ? n_max : 256u;
    hipLaunchKernelGGL(am_k_gate_repair, dim3(am_grid(waves, 4)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t am_launch_gate_commit(const am_gate_args &a, hipStream_t s)
{
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(am_k_gate_commit<0>, dim3(am_grid(a.n, 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t am_launch_gate_commit_running(const am_gate_args &a, hipStream_t s)
{
    if (a.n == 0 || !a.n_ptr) return hipSuccess;
    hipLaunchKernelGGL(am_k_gate_commit<1>, dim3(am_grid(a.n, 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t am_launch_gate_ticket(uint32_t *pin, uint32_t seq, const unsigned long long *cnt, const uint32_t *rl, hipStream_t s,
                                 const uint32_t *flag_src, const uint64_t *word_src)
{
    uint32_t *host_word = pin + AM_PW_TICKET, *cnt_dst = pin + AM_PW_GATE_TAUGHT;
    if (flag_src || word_src) {
        hipLaunchKernelGGL(am_k_gate_pipe_ticket, dim3(1), dim3(1), 0, s, host_word, seq, cnt, rl, cnt_dst, flag_src, pin + AM_PW_FLAG,
                           reinterpret_cast<const unsigned long long *>(word_src), reinterpret_cast<unsigned long long *>(pin + AM_PW_EXIT));
        return hipGetLastError();
    }
    if (rl) hipLaunchKernelGGL(am_k_gate_repair_ticket, dim3(1), dim3(1), 0, s, host_word, seq, cnt, rl, cnt_dst);
    else hipLaunchKernelGGL(am_k_gate_ticket, dim3(1), dim3(1), 0, s, host_word, seq, cnt, cnt_dst);
    return hipGetLastError();
}
