// am_raw_iq.h -- native sample formats on the device: raw integer I,Q -> float32 I,Q, for the kernel that widens a whole stream
// (am_k_unpack, am_resample.hip) and for the kernels that read raw samples themselves (64 Msps: am_k_fe3<FMT>, am_k_refine_seg<PMF, FMT>;
// 2 .. 40 Msps: am_k_fe4<SPC, G, NW, FMT>; both: am_k_extract_slice_iq<..., 1>).  Not part of the public ABI.  DEFINITION: air_modes/formats.py
//
//   sc16  float(x) * 2^-15        cs8  float(x) * 2^-7        cu8  (float(x) - 127.5f) * 2^-7
//
// Every operation is exact in float32 (|x| < 2^16; x - 127.5 has 9 significant bits; a power-of-two scale), so forms that
// are equal over the reals are equal bit for bit, and a kernel picks the cheapest:
//   cu8   v_cvt_f32_ubyteN, then ONE fma: u * 2^-7 - 127.5 * 2^-7 (the exact value is representable, so the single rounding
//         of the fma returns it)
//   cs8   x + 128 = the byte with its top bit flipped, read as unsigned: one v_xor per FOUR components, then the cu8 pair
//         with -1.0 as the addend
//   sc16  sign-extending extract, v_cvt_f32_i32, one multiply
// Whoever reads raw samples through these helpers therefore forms, for every sample, the float32 pair am_k_unpack would have
// written, and |.|^2 = fl(fl(I*I) + fl(Q*Q)) of it is the staged path's, bit for bit.
#ifndef AM_RAW_IQ_H
#define AM_RAW_IQ_H

#include "am_internal.h"

#include <string.h>

template <int FMT> struct unp_fmt;
template <> struct unp_fmt<AM_FMT_CF32> { static constexpr int CS = 4; };
template <> struct unp_fmt<AM_FMT_SC16> { static constexpr int CS = 2; };
template <> struct unp_fmt<AM_FMT_CS8> { static constexpr int CS = 1; };
template <> struct unp_fmt<AM_FMT_CU8> { static constexpr int CS = 1; };

// one component, the definition as written
template <int FMT>
__device__ __forceinline__ float unp_one(const unsigned char *p)
{
    if (FMT == AM_FMT_SC16) return (float)(int)*reinterpret_cast<const int16_t *>(p) * 0x1p-15f;
    if (FMT == AM_FMT_CS8) return (float)(int)*reinterpret_cast<const signed char *>(p) * 0x1p-7f;
    return ((float)(int)*p - 127.5f) * 0x1p-7f;
}

// the 4 / CS components of one 32-bit word
template <int FMT>
__device__ __forceinline__ void unp_word(uint32_t w, float *f)
{
    if (FMT == AM_FMT_SC16) {
        f[0] = (float)(int)(int16_t)(w & 0xffffu) * 0x1p-15f;
        f[1] = (float)((int32_t)w >> 16) * 0x1p-15f;
    } else {
        const float c = FMT == AM_FMT_CS8 ? -1.0f : -127.5f * 0x1p-7f;
        if (FMT == AM_FMT_CS8) w ^= 0x80808080u;
#pragma unroll
        for (int k = 0; k < 4; ++k) f[k] = fmaf((float)((w >> (8 * k)) & 0xffu), 0x1p-7f, c);
    }
}

// ---- what the kernels that read raw samples add ------------------------------------------------------------------------------
// bytes per complex sample (device and host; am_sample_bytes is the exported form)
__host__ __device__ __forceinline__ int raw_sample_bytes(int fmt) { return fmt == AM_FMT_CF32 ? 8 : (fmt == AM_FMT_SC16 ? 4 : 2); }

// |.|^2 of a sample: fl(fl(I*I) + fl(Q*Q)) (a1; the translation units that include this compile with fp contraction off)
__device__ __forceinline__ float raw_mag2(float i, float q)
{
    const float r = i * i, s = q * q;
    return r + s;
}

// |.|^2 of the samples one 32-bit word holds: one (sc16) or two (cs8 / cu8)
template <int FMT>
__device__ __forceinline__ void raw_word_mag2(uint32_t w, float *m)
{
    float f[4];
    unp_word<FMT>(w, f);
    m[0] = raw_mag2(f[0], f[1]);
    if (FMT != AM_FMT_SC16) m[1] = raw_mag2(f[2], f[3]);
}

// |.|^2 of sample idx of the array at `base` (element 0 = sample 0), one sample at a time: stream edges, unaligned input
template <int FMT>
__device__ __forceinline__ float raw_mag2_at(const void *base, long long idx)
{
    if (FMT == AM_FMT_CF32) {
        const float2 t = static_cast<const float2 *>(base)[idx];
        return raw_mag2(t.x, t.y);
    }
    constexpr int CS = unp_fmt<FMT>::CS;
    const unsigned char *p = static_cast<const unsigned char *>(base) + idx * (2 * CS);
    return raw_mag2(unp_one<FMT>(p), unp_one<FMT>(p + CS));
}
// ... with the format as a (wave-uniform) run-time value
__device__ __forceinline__ float raw_mag2_at_rt(int fmt, const void *base, long long idx)
{
    if (fmt == AM_FMT_SC16) return raw_mag2_at<AM_FMT_SC16>(base, idx);
    if (fmt == AM_FMT_CS8) return raw_mag2_at<AM_FMT_CS8>(base, idx);
    if (fmt == AM_FMT_CU8) return raw_mag2_at<AM_FMT_CU8>(base, idx);
    return raw_mag2_at<AM_FMT_CF32>(base, idx);
}

// |.|^2 of the PAIR of samples 2 pair, 2 pair + 1 of the array at `base`, which is aligned to a pair (8 bytes of sc16, 4 of cs8 / cu8):
// the load, and what becomes of the loaded bits -- apart, so that a kernel can keep several loads in flight
struct raw_pair_bits { uint32_t lo, hi; };
template <int FMT>
__device__ __forceinline__ raw_pair_bits raw_pair_load(const void *base, long long pair)
{
    raw_pair_bits b;
#if defined(__HIP_DEVICE_COMPILE__)
    // (device memory, said so: a pointer that went through scalar registers as integers would otherwise be loaded from as flat)
    typedef unsigned raw_u2 __attribute__((ext_vector_type(2)));
    if (FMT == AM_FMT_SC16) {
        const raw_u2 t = reinterpret_cast<const raw_u2 __attribute__((address_space(1))) *>(reinterpret_cast<unsigned long long>(base))[pair];
        b.lo = t.x; b.hi = t.y;
    } else {
        b.lo = reinterpret_cast<const uint32_t __attribute__((address_space(1))) *>(reinterpret_cast<unsigned long long>(base))[pair];
        b.hi = 0u;
    }
#else
    if (FMT == AM_FMT_SC16) {
        const uint2 t = static_cast<const uint2 *>(base)[pair];
        b.lo = t.x; b.hi = t.y;
    } else {
        b.lo = static_cast<const uint32_t *>(base)[pair];
        b.hi = 0u;
    }
#endif
    return b;
}
template <int FMT>
__device__ __forceinline__ float2 raw_pair_mag2(const raw_pair_bits &b)
{
    float m[2];
    float2 r;
    if (FMT == AM_FMT_SC16) {
        raw_word_mag2<FMT>(b.lo, m);
        r.x = m[0];
        raw_word_mag2<FMT>(b.hi, m);
        r.y = m[0];
    } else {
        raw_word_mag2<FMT>(b.lo, m);
        r.x = m[0]; r.y = m[1];
    }
    return r;
}
__device__ __forceinline__ raw_pair_bits raw_pair_load_rt(int fmt, const void *base, long long pair)
{
    return fmt == AM_FMT_SC16 ? raw_pair_load<AM_FMT_SC16>(base, pair) : raw_pair_load<AM_FMT_CS8>(base, pair);
}
__device__ __forceinline__ float2 raw_pair_mag2_rt(int fmt, const raw_pair_bits &b)
{
    if (fmt == AM_FMT_SC16) return raw_pair_mag2<AM_FMT_SC16>(b);
    if (fmt == AM_FMT_CS8) return raw_pair_mag2<AM_FMT_CS8>(b);
    return raw_pair_mag2<AM_FMT_CU8>(b);
}

#endif
