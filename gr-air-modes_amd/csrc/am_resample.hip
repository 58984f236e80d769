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

struct am_resampler {
    int device = 0;
    hipStream_t stream = nullptr;
    double ratio = 1.0, step = 1.0, pos = 0.0;
    float hist[2 * AM_RS_TAPS] = {};      // the last 8 input samples of the calls so far (I, Q)
    double *taps_dev = nullptr;           // [32][8]
    float *in_dev = nullptr, *out_dev = nullptr;
    size_t in_cap = 0, out_cap = 0;       // floats
    uint64_t out_n = 0;                   // complex samples in out_dev after the last call
    char err[160] = "";
};

// buf = 8 history samples + the block's inputs (x[j] = buf[8 + j]); one thread per output
__global__ void __launch_bounds__(256)
am_k_resample(const float2 *__restrict__ buf, const double *__restrict__ taps, double pos, double step, uint32_t m_cnt,
              float2 *__restrict__ out)
{
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= m_cnt) return;
    const double t = pos + step * (double)m;
    const double fl = floor(t);
    const long long i0 = (long long)fl;
    const double frac = (t - fl) * (double)AM_RS_NPHASE;
    int p = (int)floor(frac);
    if (p > AM_RS_NPHASE - 1) p = AM_RS_NPHASE - 1;
    const double a = frac - (double)p;
    const int wrap = (p + 1 >= AM_RS_NPHASE) ? 1 : 0;
    const double *t0 = taps + p * AM_RS_TAPS, *t1 = taps + (wrap ? 0 : p + 1) * AM_RS_TAPS;
    const float2 *w0 = buf + (AM_RS_TAPS + i0), *w1 = w0 + wrap;
    double y0r = 0.0, y0i = 0.0, y1r = 0.0, y1i = 0.0;
#pragma unroll
    for (int q = 0; q < AM_RS_TAPS; ++q) {
        const float2 u = w0[-q], v = w1[-q];
        const double c0 = t0[q], c1 = t1[q];
        y0r = y0r + (double)u.x * c0;
        y0i = y0i + (double)u.y * c0;
        y1r = y1r + (double)v.x * c1;
        y1i = y1i + (double)v.y * c1;
    }
    const double b = 1.0 - a;
    float2 y;
    y.x = (float)(b * y0r + a * y1r);
    y.y = (float)(b * y0i + a * y1i);
    out[m] = y;
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

int rs_ensure(am_resampler *h, float **p, size_t *cap, size_t floats)
{
    if (*p && *cap >= floats) return AM_OK;
    float *q = nullptr;
    const size_t want = floats + floats / 4 + 1024;
    hipError_t rc = hipMalloc(reinterpret_cast<void **>(&q), want * sizeof(float));
    if (rc != hipSuccess) return rs_fail(h, AM_ENOMEM, "hipMalloc", rc);
    if (*p) {
        // (the output buffer keeps what earlier blocks of this call wrote)
        if (p == &h->out_dev && h->out_n) (void)hipMemcpyAsync(q, *p, h->out_n * 2 * sizeof(float), hipMemcpyDeviceToDevice, h->stream);
        (void)hipStreamSynchronize(h->stream);
        (void)hipFree(*p);
    }
    *p = q;
    *cap = want;
    return AM_OK;
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
        if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&h->stream) != hipSuccess) { code = AM_EHIP; break; }
        if (hipMalloc(reinterpret_cast<void **>(&h->taps_dev), AM_RS_NPHASE * AM_RS_TAPS * sizeof(double)) != hipSuccess) { code = AM_ENOMEM; break; }
        if (hipMemcpy(h->taps_dev, taps, AM_RS_NPHASE * AM_RS_TAPS * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) { code = AM_EHIP; break; }
    } while (0);
    if (code != AM_OK && h) { am_resampler_destroy(h); h = nullptr; }
    if (err) *err = code;
    return h;
}

void am_resampler_destroy(am_resampler *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->taps_dev) (void)hipFree(h->taps_dev);
    if (h->in_dev) (void)hipFree(h->in_dev);
    if (h->out_dev) (void)hipFree(h->out_dev);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

const char *am_resampler_last_error(const am_resampler *h) { return h ? h->err : "null resampler"; }
const float *am_resampler_device_output(const am_resampler *h) { return h ? h->out_dev : nullptr; }

int am_resampler_reset(am_resampler *h)
{
    if (!h) return AM_EINVAL;
    h->pos = 0.0;
    memset(h->hist, 0, sizeof(h->hist));
    h->out_n = 0;
    return AM_OK;
}

int am_resampler_work(am_resampler *h, const float *iq, uint64_t n, uint32_t flags, float *out, uint64_t cap, uint64_t *n_out)
{
    if (!h) return AM_EINVAL;
    if (n_out) *n_out = 0;
    h->out_n = 0;
    if (n && !iq) return rs_fail(h, AM_EINVAL, "null input");
    if (n > ((uint64_t)1 << 31)) return rs_fail(h, AM_EINVAL, "chunk larger than 2^31 samples");
    if (hipSetDevice(h->device) != hipSuccess) return rs_fail(h, AM_EHIP, "hipSetDevice");
    const bool dev_in = (flags & AM_F_DEVICE_IN) != 0;
    const hipMemcpyKind in_kind = dev_in ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const double step = h->step;
    for (uint64_t o = 0; o < n; o += AM_RS_BLOCK) {
        const uint64_t n_in = (n - o < AM_RS_BLOCK) ? n - o : AM_RS_BLOCK;
        // buf = history + block
        if (int rc = rs_ensure(h, &h->in_dev, &h->in_cap, (size_t)(AM_RS_TAPS + n_in) * 2); rc != AM_OK) return rc;
        hipError_t e = hipMemcpyAsync(h->in_dev, h->hist, sizeof(h->hist), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h->in_dev + 2 * AM_RS_TAPS, iq + 2 * o, (size_t)n_in * 2 * sizeof(float), in_kind, h->stream);
        if (e != hipSuccess) return rs_fail(h, AM_EHIP, "hipMemcpyAsync", e);
        // outputs that need nothing beyond x[n_in - 1]: t = pos + m step < n_in - 1   (resample.py, same double arithmetic)
        const double span = (double)(n_in - 1) - h->pos;
        const uint64_t m_cnt = span > 0.0 ? (uint64_t)ceil(span / step) : 0;
        if (m_cnt) {
            if (int rc = rs_ensure(h, &h->out_dev, &h->out_cap, (size_t)(h->out_n + m_cnt) * 2); rc != AM_OK) return rc;
            hipLaunchKernelGGL(am_k_resample, dim3((unsigned)((m_cnt + 255) / 256)), dim3(256), 0, h->stream,
                               reinterpret_cast<const float2 *>(h->in_dev), h->taps_dev, h->pos, step, (uint32_t)m_cnt,
                               reinterpret_cast<float2 *>(h->out_dev) + h->out_n);
            if (hipGetLastError() != hipSuccess) return rs_fail(h, AM_EHIP, "am_k_resample launch");
            const double t_last = h->pos + step * (double)(m_cnt - 1);
            h->pos = t_last + step - (double)n_in;
            h->out_n += m_cnt;
        } else
            h->pos -= (double)n_in;
        // the block's last 8 samples (with the history when it is shorter) become the history
        float nh[2 * AM_RS_TAPS];                              // buf[-8:] (part history, part block when the block is shorter)
        e = hipMemcpyAsync(nh, h->in_dev + 2 * n_in, sizeof(nh), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) return rs_fail(h, AM_EHIP, "history copy", e);
        memcpy(h->hist, nh, sizeof(nh));
    }
    if (n_out) *n_out = h->out_n;
    if (out) {
        if (h->out_n > cap) return rs_fail(h, AM_ECAPACITY, "output array too small");
        if (h->out_n) {
            const hipMemcpyKind k = (flags & AM_F_DEVICE_OUT) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
            hipError_t e = hipMemcpyAsync(out, h->out_dev, (size_t)h->out_n * 2 * sizeof(float), k, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
            if (e != hipSuccess) return rs_fail(h, AM_EHIP, "output copy", e);
        }
    } else if (hipStreamSynchronize(h->stream) != hipSuccess)
        return rs_fail(h, AM_EHIP, "hipStreamSynchronize");
    return AM_OK;
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
