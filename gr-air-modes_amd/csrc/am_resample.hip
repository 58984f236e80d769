// am_resample.hip -- polyphase arbitrary-ratio interpolator in front of the receive path.
//
// python/radio.py:49-53: input slower than 4 Msps goes through pfb.arb_resampler_ccf(4e6 / rate) before rx_path.
// GNU Radio's block and its tap design are not in the reference tree (PARITY UNPINNED); the DEFINITION of this stage
// is air_modes/resample.py (32 phases x 8 taps, Kaiser-windowed sinc, linear interpolation between neighbouring
// phases), whose arithmetic is written out operation by operation so that this kernel can repeat it bit for bit:
//
//   output m of a block:  t = pos + step * m          (double; step = 1 / ratio, pos = read position carried between calls)
//                         i0 = floor(t), frac = (t - i0) * 32, p = min(floor(frac), 31), a = frac - p
//                         y0 = sum over q = 0..7, in that order, of x[i0 - q] * taps[p][q]      (re and im apart, double)
//                         y1 = the same one phase on (p + 1 = 32: phase 0 of the next sample)
//                         y  = float((1 - a) * y0 + a * y1)
//
// every product and every sum one IEEE double rounding (contraction off).  The taps come from the caller (numpy's
// kaiser / sinc are not reproduced here).  The host part -- how many outputs a block yields, the carried position and
// the last 8 input samples -- repeats resample.py's scalar double arithmetic, including its blocks of 2^17 inputs.
//
// One launch per call (am_k_resample_raw<FMT>), whatever the sample format and however many blocks the call spans: that
// recurrence needs no device data, so the host runs it for the whole call and hands the kernel a table with one entry per
// block (first input, pos, number of outputs, first output).  The kernel reads the samples where they lie, at the width they
// have (cf32, or sc16 / cs8 / cu8 widened by am_raw_iq.h exactly as am_k_unpack would have written them): a block's "history" is
// simply what stands in front of it in the same array, the first block's is the handle's 8 carried samples (a device buffer),
// and an index at or beyond the call's end reads zero -- AM_F_FLUSH: resample.py's work_samples(flush=True).  The carried
// samples are renewed by the same launch, from one device buffer into the other.
//
// Also in this file, the other input-side stages: am_k_unpack (native sample formats sc16 / cs8 / cu8 -> float32, the
// definition is air_modes/formats.py) and the pinned uploader of a host source.
#include "am_internal.h"
#include "am_raw_iq.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <new>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define AM_RS_NPHASE 32
#define AM_RS_TAPS 8
#define AM_RS_BLOCK (1u << 17)            /* inputs per block, as resample.py */
#define AM_RS_WG 256                      /* outputs per workgroup, one per thread */
// Samples a workgroup stages.  Its outputs read x[floor(t) - 7 .. floor(t) + 1] with t = pos + step * m over 256 consecutive m:
// step <= 1 (ratio >= 1) and every t is within one rounding of its exact value, so the floors of the first and the last differ by
// at most 256; with the 9 samples around them, and 1 more when the window starts inside an aligned pair of 8-bit samples: <= 266.
#define AM_RS_WIN 272
#define AM_RS_TAPROW (AM_RS_TAPS + 1)     /* doubles per phase in LDS: rows 18 banks apart, so 32 different phases hit 32 different bank pairs */

// one block of the definition, as the host's recurrence leaves it
struct rs_blk {
    double pos;                           // read position of the block's output 0, relative to its first input
    uint64_t out0;                        // index of that output in the call's output
    uint32_t in0, m_cnt;                  // the block's first input (index in the call's input), its number of outputs
};

struct rs_args {
    const unsigned char *raw;             // the call's samples, aligned to a component
    uint64_t n;                           // how many of them
    const float *hist_in;                 // the 8 samples in front of them (I, Q)
    float *hist_out;                      // where (hist_in ++ the samples)[-8:] goes; null: nowhere (flush)
    const double *taps;                   // [32][8]
    double step;
    float2 *out;
    const rs_blk *tab;                    // one entry per block (blockIdx.y)
};

struct am_resampler {
    int device = 0;
    hipStream_t stream = nullptr, own_stream = nullptr;   // `stream` is own_stream unless am_resampler_set_stream replaced it
    double ratio = 1.0, step = 1.0, pos = 0.0;
    float *hist_dev = nullptr;            // 2 x 8 samples (I, Q): [hist_cur] holds the last 8 input samples of the calls so far,
    int hist_cur = 0;                     // the other one is where the next call writes its own
    double *taps_dev = nullptr;           // [32][8]
    unsigned char *in_dev = nullptr;      // host input, staged at its raw width
    float *out_dev = nullptr;
    size_t in_cap = 0, out_cap = 0;       // bytes
    uint64_t out_n = 0;                   // complex samples in out_dev after the last call
    // the block table: written into one of two pinned buffers in turn, sent to its device twin by one asynchronous copy
    rs_blk *tab_host[2] = {}, *tab_dev = nullptr;
    size_t tab_cap = 0;                   // entries
    hipEvent_t tab_sent[2] = {};          // behind the last copy out of tab_host[k]
    int tab_cur = 0;
    char err[160] = "";
};

// sample g of the call, whatever g: the carried samples in front of the call, zero behind it (and in front of what is carried)
template <int FMT>
__device__ __forceinline__ float2 rs_sample(const unsigned char *raw, long long n, const float *hist, long long g)
{
    float2 v; v.x = 0.0f; v.y = 0.0f;
    if (g < 0) {
        if (g >= -AM_RS_TAPS) { v.x = hist[2 * (AM_RS_TAPS + g)]; v.y = hist[2 * (AM_RS_TAPS + g) + 1]; }
    } else if (g < n) {
        if (FMT == AM_FMT_CF32) {
            const float *p = reinterpret_cast<const float *>(raw) + 2 * g;
            v.x = p[0]; v.y = p[1];
        } else {
            constexpr int CS = unp_fmt<FMT>::CS;
            const unsigned char *p = raw + g * (2 * CS);
            v.x = unp_one<FMT>(p); v.y = unp_one<FMT>(p + CS);
        }
    }
    return v;
}

// One thread per output; blockIdx.y = block of the definition, blockIdx.x = which 256 of its outputs.  The workgroup stages the
// input window of its outputs (about 256 / ratio + 9 samples, widened) and the taps in LDS and computes from there: neighbouring
// outputs share 15 of their 16 samples.  Loads are as wide as the address allows -- a whole sample (sc16: 4 bytes, cf32: 8), a
// pair of samples (cs8 / cu8: 4 bytes) -- where that unit is aligned and lies inside the call's samples; everything else goes one
// component at a time (rs_sample).  Nothing outside [raw, raw + n samples) is read.
template <int FMT>
__global__ void __launch_bounds__(AM_RS_WG)
am_k_resample_raw(const rs_args a)
{
    __shared__ float2 s_x[AM_RS_WIN];
    __shared__ double s_taps[AM_RS_NPHASE * AM_RS_TAPROW];
    constexpr int CS = unp_fmt<FMT>::CS;
    constexpr int SPU = CS == 1 ? 2 : 1;                       // samples per load unit
    const int tid = (int)threadIdx.x;
    const long long n = (long long)a.n;
    if (blockIdx.x == 0 && blockIdx.y == 0 && a.hist_out && tid < AM_RS_TAPS) {
        const float2 v = rs_sample<FMT>(a.raw, n, a.hist_in, n - AM_RS_TAPS + tid);
        a.hist_out[2 * tid] = v.x;
        a.hist_out[2 * tid + 1] = v.y;
    }
    const rs_blk e = a.tab[blockIdx.y];
    const uint32_t m0 = blockIdx.x * AM_RS_WG;
    if (m0 >= e.m_cnt) return;                                 // (the grid is as wide as the call's longest block)
    const uint32_t m1 = e.m_cnt - 1 - m0 < AM_RS_WG - 1 ? e.m_cnt - 1 : m0 + (AM_RS_WG - 1);
    // the window: t is monotone in m (one rounding of the product, one of the sum), so these two bound every output's floor(t)
    long long lo = (long long)e.in0 + (long long)floor(e.pos + a.step * (double)m0) - (AM_RS_TAPS - 1);
    const long long hi = (long long)e.in0 + (long long)floor(e.pos + a.step * (double)m1) + 1;
    const unsigned long long addr = reinterpret_cast<unsigned long long>(a.raw);
    // a unit can be loaded whole if samples lie at multiples of their size (8-bit: of 2, and then every other one at a multiple of 4:
    // the window starts on such a one)
    const bool wide = (addr & (unsigned)(SPU == 2 ? 1 : 2 * CS - 1)) == 0;
    if (SPU == 2 && wide) lo -= (lo + (long long)((addr >> 1) & 1)) & 1;
    int W = (int)(hi - lo + 1);
    if (W > AM_RS_WIN) W = AM_RS_WIN;
    for (int j = tid; j * SPU < W; j += AM_RS_WG) {
        const long long g = lo + (long long)j * SPU;
        if (wide && g >= 0 && g + SPU <= n) {
            if (FMT == AM_FMT_CF32) {
                s_x[j] = reinterpret_cast<const float2 *>(a.raw)[g];
            } else {
                float f[4];
                unp_word<FMT>(*reinterpret_cast<const uint32_t *>(a.raw + g * (2 * CS)), f);
                float2 v; v.x = f[0]; v.y = f[1];
                s_x[j * SPU] = v;
                if (SPU == 2) { v.x = f[2]; v.y = f[3]; s_x[j * SPU + 1] = v; }
            }
        } else {
            s_x[j * SPU] = rs_sample<FMT>(a.raw, n, a.hist_in, g);
            if (SPU == 2 && j * SPU + 1 < W) s_x[j * SPU + 1] = rs_sample<FMT>(a.raw, n, a.hist_in, g + 1);
        }
    }
    s_taps[(tid >> 3) * AM_RS_TAPROW + (tid & 7)] = a.taps[tid];               // (256 threads, 32 x 8 taps)
    __syncthreads();
    const uint32_t m = m0 + (uint32_t)tid;
    if (m > m1) return;
    const double t = e.pos + a.step * (double)m;
    const double fl = floor(t);
    const long long i0 = (long long)fl;
    const double frac = (t - fl) * (double)AM_RS_NPHASE;
    int p = (int)floor(frac);
    if (p > AM_RS_NPHASE - 1) p = AM_RS_NPHASE - 1;
    const double al = frac - (double)p;
    const bool wrap = p + 1 >= AM_RS_NPHASE;
    const double *t0 = s_taps + p * AM_RS_TAPROW, *t1 = s_taps + (wrap ? 0 : p + 1) * AM_RS_TAPROW;
    const float2 *w = s_x + ((long long)e.in0 + i0 + 1 - lo);                  // x[i0 + 1]
    float2 x[AM_RS_TAPS + 1];                                                  // x[j] = sample i0 + 1 - j
#pragma unroll
    for (int j = 0; j <= AM_RS_TAPS; ++j) x[j] = w[-j];
    double y0r = 0.0, y0i = 0.0, y1r = 0.0, y1i = 0.0;
#pragma unroll
    for (int q = 0; q < AM_RS_TAPS; ++q) {
        const float2 u = x[q + 1], v = wrap ? x[q] : x[q + 1];
        const double c0 = t0[q], c1 = t1[q];
        y0r = y0r + (double)u.x * c0;
        y0i = y0i + (double)u.y * c0;
        y1r = y1r + (double)v.x * c1;
        y1i = y1i + (double)v.y * c1;
    }
    const double b = 1.0 - al;
    float2 y;
    y.x = (float)(b * y0r + al * y1r);
    y.y = (float)(b * y0i + al * y1i);
    a.out[e.out0 + m] = y;
}

namespace {

int rs_fail(am_resampler *h, int code, const char *what, hipError_t rc = hipSuccess)
{
    if (h) {
        if (rc != hipSuccess) snprintf(h->err, sizeof(h->err), "%s: %s", what, hipGetErrorString(rc));
        else snprintf(h->err, sizeof(h->err), "%s", what);
    }
    return code;
}

// a device buffer of at least `bytes`; what it held is not kept
template <class T>
int rs_ensure(am_resampler *h, T **p, size_t *cap, size_t bytes)
{
    if (*p && *cap >= bytes) return AM_OK;
    T *q = nullptr;
    const size_t want = bytes + bytes / 4 + 4096;
    hipError_t rc = hipMalloc(reinterpret_cast<void **>(&q), want);
    if (rc != hipSuccess) return rs_fail(h, AM_ENOMEM, "hipMalloc", rc);
    if (*p) {
        (void)hipStreamSynchronize(h->stream);                  // (an earlier call may still read or write the old one)
        (void)hipFree(*p);
    }
    *p = q;
    *cap = want;
    return AM_OK;
}

// room for a table of `entries` blocks in pinned memory (twice) and on the device
int rs_ensure_table(am_resampler *h, size_t entries)
{
    if (h->tab_cap >= entries) return AM_OK;
    (void)hipStreamSynchronize(h->stream);                      // (an earlier call may still read the old ones)
    for (int k = 0; k < 2; ++k) {
        if (h->tab_host[k]) (void)hipHostFree(h->tab_host[k]);
        h->tab_host[k] = nullptr;
    }
    if (h->tab_dev) (void)hipFree(h->tab_dev);
    h->tab_dev = nullptr;
    h->tab_cap = 0;
    const size_t want = entries + entries / 4;
    if (hipHostMalloc(reinterpret_cast<void **>(&h->tab_host[0]), want * sizeof(rs_blk), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&h->tab_host[1]), want * sizeof(rs_blk), hipHostMallocDefault) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&h->tab_dev), want * sizeof(rs_blk)) != hipSuccess)
        return rs_fail(h, AM_ENOMEM, "block table");
    h->tab_cap = want;
    return AM_OK;
}

template <int FMT>
hipError_t rs_launch(const rs_args &a, unsigned gx, unsigned gy, hipStream_t s)
{
    hipLaunchKernelGGL(am_k_resample_raw<FMT>, dim3(gx, gy), dim3(AM_RS_WG), 0, s, a);
    return hipGetLastError();
}

// One call of either kind.  `wait`: return only when the output is complete (am_resampler_work's contract).
int rs_work(am_resampler *h, const void *raw, uint64_t n, int fmt, uint32_t flags, float *out, uint64_t cap, uint64_t *n_out,
            bool wait)
{
    if (!h) return AM_EINVAL;
    if (n_out) *n_out = 0;
    h->out_n = 0;
    const size_t sb = am_sample_bytes(fmt);
    if (!sb) return rs_fail(h, AM_EINVAL, "unknown sample format");
    if (n && !raw) return rs_fail(h, AM_EINVAL, "null input");
    if (n > ((uint64_t)1 << 31)) return rs_fail(h, AM_EINVAL, "chunk larger than 2^31 samples");
    const bool dev_in = (flags & AM_F_DEVICE_IN) != 0, flush = (flags & AM_F_FLUSH) != 0;
    const bool host_out = out && !(flags & AM_F_DEVICE_OUT);
    // flush: eight zero samples follow in the same call (the blocks are cut over both), then a new stream starts
    const uint64_t n_tot = n + (flush ? AM_RS_TAPS : 0);
    if (!n_tot) return AM_OK;
    if (hipSetDevice(h->device) != hipSuccess) return rs_fail(h, AM_EHIP, "hipSetDevice");

    // the table: resample.py's scalar double arithmetic, block by block
    const size_t nblk = (size_t)((n_tot + AM_RS_BLOCK - 1) / AM_RS_BLOCK);
    if (int rc = rs_ensure_table(h, nblk); rc != AM_OK) return rc;
    // (the copy out of this pinned buffer, two calls ago, has to have read it: it stands in front of that call's kernel)
    if (hipEventSynchronize(h->tab_sent[h->tab_cur]) != hipSuccess) return rs_fail(h, AM_EHIP, "hipEventSynchronize");
    rs_blk *tab = h->tab_host[h->tab_cur];
    const double step = h->step;
    double pos = h->pos;
    uint64_t total = 0, m_max = 0;
    for (size_t b = 0; b < nblk; ++b) {
        const uint64_t o = (uint64_t)b * AM_RS_BLOCK;
        const uint64_t n_in = (n_tot - o < AM_RS_BLOCK) ? n_tot - o : AM_RS_BLOCK;
        // outputs that need nothing beyond x[n_in - 1]: t = pos + m step < n_in - 1
        const double span = (double)(n_in - 1) - pos;
        const uint64_t m_cnt = span > 0.0 ? (uint64_t)ceil(span / step) : 0;
        tab[b].pos = pos;
        tab[b].out0 = total;
        tab[b].in0 = (uint32_t)o;
        tab[b].m_cnt = (uint32_t)m_cnt;
        if (m_cnt) {
            const double t_last = pos + step * (double)(m_cnt - 1);
            pos = t_last + step - (double)n_in;
            total += m_cnt;
            if (m_cnt > m_max) m_max = m_cnt;
        } else
            pos -= (double)n_in;
    }
    if (m_max > 0xffffffffull) return rs_fail(h, AM_EINVAL, "more than 2^32 outputs from one block");
    if (n_out) *n_out = total;

    const unsigned char *src = static_cast<const unsigned char *>(raw);
    hipError_t e = hipSuccess;
    if (!dev_in && n) {
        if (int rc = rs_ensure(h, &h->in_dev, &h->in_cap, (size_t)n * sb); rc != AM_OK) return rc;
        e = hipMemcpyAsync(h->in_dev, raw, (size_t)n * sb, hipMemcpyHostToDevice, h->stream);
        if (e != hipSuccess) return rs_fail(h, AM_EHIP, "hipMemcpyAsync", e);
        src = h->in_dev;
    }
    if (int rc = rs_ensure(h, &h->out_dev, &h->out_cap, (size_t)(total + 1) * 2 * sizeof(float)); rc != AM_OK) return rc;
    rs_args a;
    a.raw = src;
    a.n = n;
    a.hist_in = h->hist_dev + 2 * AM_RS_TAPS * h->hist_cur;
    a.hist_out = flush ? nullptr : h->hist_dev + 2 * AM_RS_TAPS * (h->hist_cur ^ 1);
    a.taps = h->taps_dev;
    a.step = step;
    a.out = reinterpret_cast<float2 *>(h->out_dev);
    a.tab = h->tab_dev;
    e = hipMemcpyAsync(h->tab_dev, tab, nblk * sizeof(rs_blk), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipEventRecord(h->tab_sent[h->tab_cur], h->stream);
    if (e != hipSuccess) return rs_fail(h, AM_EHIP, "block table copy", e);
    h->tab_cur ^= 1;
    const unsigned gx = m_max ? (unsigned)((m_max + AM_RS_WG - 1) / AM_RS_WG) : 1u, gy = (unsigned)nblk;
    switch (fmt) {
    case AM_FMT_CF32: e = rs_launch<AM_FMT_CF32>(a, gx, gy, h->stream); break;
    case AM_FMT_SC16: e = rs_launch<AM_FMT_SC16>(a, gx, gy, h->stream); break;
    case AM_FMT_CS8: e = rs_launch<AM_FMT_CS8>(a, gx, gy, h->stream); break;
    default: e = rs_launch<AM_FMT_CU8>(a, gx, gy, h->stream); break;
    }
    if (e != hipSuccess) return rs_fail(h, AM_EHIP, "am_k_resample_raw launch", e);
    // the state after the call (the device's half of it is ordered on the stream)
    h->out_n = total;
    if (flush) {
        h->pos = 0.0;
        e = hipMemsetAsync(h->hist_dev + 2 * AM_RS_TAPS * h->hist_cur, 0, 2 * AM_RS_TAPS * sizeof(float), h->stream);
        if (e != hipSuccess) return rs_fail(h, AM_EHIP, "hipMemsetAsync", e);
    } else {
        h->pos = pos;
        h->hist_cur ^= 1;
    }
    int rc = AM_OK;
    if (out && total > cap) rc = rs_fail(h, AM_ECAPACITY, "output array too small");
    else if (out && total) {
        e = hipMemcpyAsync(out, h->out_dev, (size_t)total * 2 * sizeof(float), host_out ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                           h->stream);
        if (e != hipSuccess) return rs_fail(h, AM_EHIP, "output copy", e);
    }
    // host input has to have left the caller's buffer, host output has to be there; device to device nobody waits
    if ((wait || !dev_in || host_out) && hipStreamSynchronize(h->stream) != hipSuccess)
        return rs_fail(h, AM_EHIP, "hipStreamSynchronize");
    return rc;
}

} // namespace

extern "C" {

am_resampler *am_resampler_create(int device, double ratio, const double *taps, int *err)
{
    int code = AM_OK;
    am_resampler *h = nullptr;
    do {
        if (!(ratio >= 1.0) || !taps) { code = AM_EINVAL; break; }
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { code = AM_ENODEV; break; }
        h = new (std::nothrow) am_resampler();
        if (!h) { code = AM_ENOMEM; break; }
        if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
        if (device >= ndev) { code = AM_ENODEV; break; }
        h->device = device;
        h->ratio = ratio;
        h->step = 1.0 / ratio;
        if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&h->own_stream) != hipSuccess) { code = AM_EHIP; break; }
        h->stream = h->own_stream;
        if (hipMalloc(reinterpret_cast<void **>(&h->taps_dev), AM_RS_NPHASE * AM_RS_TAPS * sizeof(double)) != hipSuccess) { code = AM_ENOMEM; break; }
        if (hipMemcpy(h->taps_dev, taps, AM_RS_NPHASE * AM_RS_TAPS * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) { code = AM_EHIP; break; }
        if (hipMalloc(reinterpret_cast<void **>(&h->hist_dev), 2 * 2 * AM_RS_TAPS * sizeof(float)) != hipSuccess) { code = AM_ENOMEM; break; }
        if (hipMemset(h->hist_dev, 0, 2 * 2 * AM_RS_TAPS * sizeof(float)) != hipSuccess) { code = AM_EHIP; break; }
        for (int k = 0; k < 2 && code == AM_OK; ++k)
            if (hipEventCreateWithFlags(&h->tab_sent[k], hipEventDisableTiming) != hipSuccess) code = AM_EHIP;
    } while (0);
    if (code != AM_OK && h) { am_resampler_destroy(h); h = nullptr; }
    if (err) *err = code;
    return h;
}

void am_resampler_destroy(am_resampler *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->taps_dev) (void)hipFree(h->taps_dev);
    if (h->hist_dev) (void)hipFree(h->hist_dev);
    if (h->in_dev) (void)hipFree(h->in_dev);
    if (h->out_dev) (void)hipFree(h->out_dev);
    for (int k = 0; k < 2; ++k) {
        if (h->tab_host[k]) (void)hipHostFree(h->tab_host[k]);
        if (h->tab_sent[k]) (void)hipEventDestroy(h->tab_sent[k]);
    }
    if (h->tab_dev) (void)hipFree(h->tab_dev);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
}

const char *am_resampler_last_error(const am_resampler *h) { return h ? h->err : "null resampler"; }
const float *am_resampler_device_output(const am_resampler *h) { return h ? h->out_dev : nullptr; }

int am_resampler_set_stream(am_resampler *h, void *hip_stream)
{
    if (!h) return AM_EINVAL;
    if (hipSetDevice(h->device) != hipSuccess) return rs_fail(h, AM_EHIP, "hipSetDevice");
    if (hipStreamSynchronize(h->stream) != hipSuccess) return rs_fail(h, AM_EHIP, "hipStreamSynchronize");   // nothing of ours is left on the old one
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return AM_OK;
}

int am_resampler_reset(am_resampler *h)
{
    if (!h) return AM_EINVAL;
    h->pos = 0.0;
    h->out_n = 0;
    if (hipSetDevice(h->device) != hipSuccess) return rs_fail(h, AM_EHIP, "hipSetDevice");
    // (on the stream: behind a call that may still read the carried samples, in front of the next one)
    hipError_t e = hipMemsetAsync(h->hist_dev + 2 * AM_RS_TAPS * h->hist_cur, 0, 2 * AM_RS_TAPS * sizeof(float), h->stream);
    return e == hipSuccess ? AM_OK : rs_fail(h, AM_EHIP, "hipMemsetAsync", e);
}

int am_resampler_work(am_resampler *h, const float *iq, uint64_t n, uint32_t flags, float *out, uint64_t cap, uint64_t *n_out)
{
    return rs_work(h, iq, n, AM_FMT_CF32, flags & (AM_F_DEVICE_IN | AM_F_DEVICE_OUT), out, cap, n_out, true);
}

int am_resampler_work_samples(am_resampler *h, const void *raw, uint64_t n, int fmt, uint32_t flags, float *out, uint64_t cap,
                              uint64_t *n_out)
{
    return rs_work(h, raw, n, fmt, flags, out, cap, n_out, false);
}

} // extern "C"

/* ---- native sample formats: raw integer I,Q -> float32 I,Q (python/radio.py:164-231) -----------------------------
 * The reference's sources convert on the host before rx_path sees a sample (uhd cpu_format="fc32", osmosdr.source); here the
 * raw bytes cross PCIe and the widening runs on the device: in this kernel, in front of the front end, or -- at 64 Msps -- inside the
 * kernels that read the samples (am_k_fe3<FMT> and what follows it).  The conversion itself, word by word and component by
 * component (unp_word<FMT>, unp_one<FMT>), is am_raw_iq.h's, shared with those kernels.
 * A stream of COMPONENTS, not of samples: the raw pointer is aligned to its component only, so the 16-byte body may begin
 * in the middle of a sample.  Body: 16-byte loads aligned on the RAW side (nt: every raw byte is read once), 16-byte stores at
 * the 4-byte alignment that leaves (plain policy: the front end reads the floats next, and a chunk fits the Infinity Cache).
 * Head and tail (fewer than 16 components each) go one component per thread.  Nothing outside [raw, raw + nc * CS) is read,
 * nothing outside [out, out + nc) written. */
#if defined(__HIP_DEVICE_COMPILE__)
typedef unsigned int unp_u4 __attribute__((ext_vector_type(4)));
typedef float unp_f4a __attribute__((ext_vector_type(4), aligned(4)));
#endif

__device__ __forceinline__ uint4 unp_load16(const unsigned char *p)          // p: 16-byte aligned
{
#if defined(__HIP_DEVICE_COMPILE__)
    const unp_u4 t = __builtin_nontemporal_load(reinterpret_cast<const unp_u4 *>(p));
    uint4 r; r.x = t.x; r.y = t.y; r.z = t.z; r.w = t.w;
    return r;
#else
    uint4 r;
    memcpy(&r, p, 16);
    return r;
#endif
}

__device__ __forceinline__ void unp_store16(float *p, const float *f)        // p: 4-byte aligned
{
#if defined(__HIP_DEVICE_COMPILE__)
    unp_f4a t; t.x = f[0]; t.y = f[1]; t.z = f[2]; t.w = f[3];
    *reinterpret_cast<unp_f4a *>(p) = t;
#else
    memcpy(p, f, 16);
#endif
}

// value of `v` in lane j of the caller's group of four lanes (DPP quad_perm:[j,j,j,j])
template <int J>
__device__ __forceinline__ uint32_t unp_quad_bcast(uint32_t v, int lane)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)lane;
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, J * 0x55, 0xf, 0xf, true);
#else
    return __shfl(v, (lane & ~3) + J, AM_WAVE);
#endif
}

// word q (= lane & 3) of the 16 bytes that lane J of the quad loaded
template <int J>
__device__ __forceinline__ uint32_t unp_quad_word(const uint4 &w, int lane)
{
    const uint32_t t0 = unp_quad_bcast<J>(w.x, lane), t1 = unp_quad_bcast<J>(w.y, lane);
    const uint32_t t2 = unp_quad_bcast<J>(w.z, lane), t3 = unp_quad_bcast<J>(w.w, lane);
    const uint32_t lo = (lane & 1) ? t1 : t0, hi = (lane & 1) ? t3 : t2;        // (two levels of v_cndmask, no branch)
    return (lane & 2) ? hi : lo;
}

// one wave-uniform step of the 8-bit body: lane `lane` loads vector v (if it exists), the quad exchanges words, and store
// j of a lane writes piece q of the vector that the quad's lane j loaded.  FULL: all 64 vectors of the step exist.
template <int FMT, bool FULL>
__device__ __forceinline__ void unp_step8(const unsigned char *vb, float *ob, unsigned long long v, unsigned long long nvec, int lane)
{
    uint4 w; w.x = w.y = w.z = w.w = 0u;
    if (FULL || v < nvec) w = unp_load16(vb + v * 16);
    const uint32_t o0 = unp_quad_word<0>(w, lane), o1 = unp_quad_word<1>(w, lane);
    const uint32_t o2 = unp_quad_word<2>(w, lane), o3 = unp_quad_word<3>(w, lane);
    const int q = lane & 3;
    const unsigned long long vq = v - (unsigned)q;                               // the vector the quad's lane 0 loaded
    float *p = ob + vq * 16 + 4 * q;
    float f[4];
    if (FULL || vq + 0 < nvec) { unp_word<FMT>(o0, f); unp_store16(p, f); }
    if (FULL || vq + 1 < nvec) { unp_word<FMT>(o1, f); unp_store16(p + 16, f); }
    if (FULL || vq + 2 < nvec) { unp_word<FMT>(o2, f); unp_store16(p + 32, f); }
    if (FULL || vq + 3 < nvec) { unp_word<FMT>(o3, f); unp_store16(p + 48, f); }
}

#define AM_UNPACK_THREADS 256
template <int FMT>
__global__ void __launch_bounds__(AM_UNPACK_THREADS)
am_k_unpack(const unsigned char *__restrict__ raw, unsigned long long nc, float *__restrict__ out)
{
    constexpr int CS = unp_fmt<FMT>::CS, CPW = 4 / CS, CPV = 16 / CS;            // bytes per component; components per word / per load
    unsigned long long head = ((16u - (unsigned)(reinterpret_cast<unsigned long long>(raw) & 15u)) & 15u) / CS;
    if (head > nc) head = nc;
    const unsigned long long nvec = (nc - head) / CPV;
    const unsigned long long tail0 = head + nvec * CPV;
    const unsigned long long g = (unsigned long long)blockIdx.x * AM_UNPACK_THREADS + threadIdx.x;
    const unsigned long long stride = (unsigned long long)gridDim.x * AM_UNPACK_THREADS;
    const unsigned char *vb = raw + head * CS;
    float *ob = out + head;
    if (CS == 2) {
        // a lane stores the 32 bytes of floats of its own load
        for (unsigned long long v = g; v < nvec; v += stride) {
            const uint4 w = unp_load16(vb + v * 16);
            float f[CPV];
            unp_word<FMT>(w.x, f);
            unp_word<FMT>(w.y, f + CPW);
            unp_word<FMT>(w.z, f + 2 * CPW);
            unp_word<FMT>(w.w, f + 3 * CPW);
#pragma unroll
            for (int j = 0; j < CPV / 4; ++j) unp_store16(ob + v * CPV + 4 * j, f + 4 * j);
        }
    } else {
        // One load widens to 64 bytes: stored by the lane that loaded them, a store instruction would touch a quarter of 64
        // different 64-byte lines (measured: 7 % slower than a device-to-device copy of the same output, which moves MORE
        // bytes).  So the four lanes of a quad exchange words first: store j of a quad writes, as four adjacent 16-byte pieces,
        // the whole line that the quad's lane j loaded -- 16 whole lines per instruction.  The loop is uniform over the wave
        // (every lane takes part in the exchange); loads and stores past the last vector are masked.
        const int lane = (int)(threadIdx.x & (AM_WAVE - 1));
        for (unsigned long long v0 = g - (unsigned)lane; v0 < nvec; v0 += stride) {
            if (v0 + AM_WAVE <= nvec) unp_step8<FMT, true>(vb, ob, v0 + (unsigned)lane, nvec, lane);
            else unp_step8<FMT, false>(vb, ob, v0 + (unsigned)lane, nvec, lane);
        }
    }
    if (g < head) out[g] = unp_one<FMT>(raw + g * CS);
    if (g < nc - tail0) out[tail0 + g] = unp_one<FMT>(raw + (tail0 + g) * CS);
}

template <int FMT>
static hipError_t unp_launch(const void *raw, uint64_t n, float *out, hipStream_t s)
{
    const unsigned long long nc = 2ull * n;
    const unsigned long long nvec = nc / (16 / unp_fmt<FMT>::CS) + 1;               // (an upper bound: the head may take one away)
    // a grid the chip holds at once (8 workgroups of 4 waves per CU: a 16-byte load per lane = 32 KiB in flight per CU), strided
    unsigned long long blocks = (nvec + AM_UNPACK_THREADS - 1) / AM_UNPACK_THREADS;
    const unsigned long long resident = 8ull * (unsigned long long)am_device_cus();
    if (blocks > resident) blocks = resident;
    hipLaunchKernelGGL(am_k_unpack<FMT>, dim3((unsigned)blocks), dim3(AM_UNPACK_THREADS), 0, s,
                       static_cast<const unsigned char *>(raw), nc, out);
    return hipGetLastError();
}

hipError_t am_launch_unpack(int fmt, const void *raw, uint64_t n, float *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    switch (fmt) {
    case AM_FMT_SC16: return unp_launch<AM_FMT_SC16>(raw, n, out, s);
    case AM_FMT_CS8: return unp_launch<AM_FMT_CS8>(raw, n, out, s);
    case AM_FMT_CU8: return unp_launch<AM_FMT_CU8>(raw, n, out, s);
    default: return hipErrorInvalidValue;
    }
}

extern "C" size_t am_sample_bytes(int fmt)
{
    switch (fmt) {
    case AM_FMT_CF32: return 8;
    case AM_FMT_SC16: return 4;
    case AM_FMT_CS8: case AM_FMT_CU8: return 2;
    default: return 0;
    }
}

/* ---- pinned staging: host samples on their way to the device, several buffers in flight --------------------------
 * A file (or socket) reader fills slot k's pinned buffer and starts its copy while the receive path still works on
 * slot k-1's samples on the device: the PCIe transfer of one chunk overlaps the scan of the one before it. */
#define AM_UP_MAXSLOTS 8
struct am_uploader {
    int device = 0, nslots = 0;
    uint64_t cap = 0;                     // complex samples per slot
    float *host[AM_UP_MAXSLOTS] = {};
    float *dev[AM_UP_MAXSLOTS] = {};
    hipEvent_t done[AM_UP_MAXSLOTS] = {};
    hipStream_t stream = nullptr;
};

extern "C" {

am_uploader *am_uploader_create(int device, uint64_t capacity_complex, int nslots, int *err)
{
    int code = AM_OK;
    am_uploader *u = nullptr;
    do {
        if (nslots < 1 || nslots > AM_UP_MAXSLOTS || capacity_complex == 0) { code = AM_EINVAL; break; }
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { code = AM_ENODEV; break; }
        u = new (std::nothrow) am_uploader();
        if (!u) { code = AM_ENOMEM; break; }
        if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
        if (device >= ndev) { code = AM_ENODEV; break; }
        u->device = device; u->nslots = nslots; u->cap = capacity_complex;
        if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&u->stream) != hipSuccess) { code = AM_EHIP; break; }
        const size_t bytes = (size_t)capacity_complex * 2 * sizeof(float);
        for (int k = 0; k < nslots && code == AM_OK; ++k) {
            if (hipHostMalloc(reinterpret_cast<void **>(&u->host[k]), bytes, hipHostMallocDefault) != hipSuccess) code = AM_ENOMEM;
            else if (hipMalloc(reinterpret_cast<void **>(&u->dev[k]), bytes) != hipSuccess) code = AM_ENOMEM;
            else if (hipEventCreateWithFlags(&u->done[k], hipEventDisableTiming) != hipSuccess) code = AM_EHIP;
        }
    } while (0);
    if (code != AM_OK && u) { am_uploader_destroy(u); u = nullptr; }
    if (err) *err = code;
    return u;
}

void am_uploader_destroy(am_uploader *u)
{
    if (!u) return;
    (void)hipSetDevice(u->device);
    if (u->stream) (void)hipStreamSynchronize(u->stream);
    for (int k = 0; k < AM_UP_MAXSLOTS; ++k) {
        if (u->host[k]) (void)hipHostFree(u->host[k]);
        if (u->dev[k]) (void)hipFree(u->dev[k]);
        if (u->done[k]) (void)hipEventDestroy(u->done[k]);
    }
    if (u->stream) (void)hipStreamDestroy(u->stream);
    delete u;
}

float *am_uploader_host(am_uploader *u, int slot) { return (u && slot >= 0 && slot < u->nslots) ? u->host[slot] : nullptr; }

int am_uploader_start_bytes(am_uploader *u, int slot, uint64_t nbytes)
{
    if (!u || slot < 0 || slot >= u->nslots || nbytes > u->cap * 2 * sizeof(float)) return AM_EINVAL;
    if (hipSetDevice(u->device) != hipSuccess) return AM_EHIP;
    if (nbytes && hipMemcpyAsync(u->dev[slot], u->host[slot], (size_t)nbytes, hipMemcpyHostToDevice, u->stream) != hipSuccess)
        return AM_EHIP;
    return hipEventRecord(u->done[slot], u->stream) == hipSuccess ? AM_OK : AM_EHIP;
}

int am_uploader_start(am_uploader *u, int slot, uint64_t n_complex)
{
    if (!u || n_complex > u->cap) return AM_EINVAL;
    return am_uploader_start_bytes(u, slot, n_complex * 2 * sizeof(float));
}

const float *am_uploader_wait(am_uploader *u, int slot)
{
    if (!u || slot < 0 || slot >= u->nslots) return nullptr;
    if (hipSetDevice(u->device) != hipSuccess || hipEventSynchronize(u->done[slot]) != hipSuccess) return nullptr;
    return u->dev[slot];
}

} // extern "C"
