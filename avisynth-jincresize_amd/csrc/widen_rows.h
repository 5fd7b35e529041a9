// widen_rows.h -- one lane's share of one row of the widening pass (kernel_widen.hip widen_samples_kernel; kernels.h WidenGroup),
// as plain inline functions for host and device: a stand-alone host program runs exactly this code lane by lane against exactly
// sized buffers (tests/host_sanitizer/widen_rows_main.cpp).
//
// Integer samples of SB bytes (1: a byte; 2: a little-endian 16-bit word), N per pixel, become fp32 (OB = 4), binary16 (OB = 2) or
// bfloat16 (OB = 2, KIND = kSampleBFloat16: the size no longer says which 16-bit type is meant) samples of up to N dense planes:
// plane c holds float((raw >> shift[c]) & mask) of channel c.  The conversion is exact: every integer below 2^24 is an fp32 value,
// every integer up to 2047 a binary16 value and every integer up to 256 a bfloat16 value (dispatch refuses wider samples into half
// and bfloat16 planes; the bfloat16 form exists for bytes only).
//
// A lane owns 16 / SB whole pixels per step, as in split_samples_kernel: N 16-byte accesses on the source side (consecutive lanes,
// consecutive addresses; 4 N dwords where base, pitch or frame stride is a multiple of 4 only) and, per given plane, OB / SB whole
// 16-byte vectors of converted samples that lie side by side -- a wave's trip stores one piece of 64 x 16 x OB / SB bytes to each
// plane.  The samples are picked out of the loaded dwords with shifts whose amounts are compile-time constants; shift[c] and the
// mask are the same in every lane.  Bytes take neither: src_bits 8 fills the byte, so a byte is its value.
// What is left moves sample by sample under a width guard: a row's tail, groups whose base, pitch or frame stride is no multiple of
// 4 bytes (vec_pixels 0), and the last pixel of a group with a channel missing, whose missing samples may lie behind the end of the
// caller's buffer.  Nothing beyond `width` samples is read from a given channel or stored to a plane; the source is never written.
//
// The scaled form (trailing template parameter Scaled; jinc_filter_process_device_widened_scaled): plane c holds
// s = fl32(fl32(float(value) * scale[c]) + offset[c]) -- one multiply and one add behind the conversion, two fp32 roundings, never an
// FMA -- and 16-bit planes hold s narrowed round-to-nearest-even (binary16: overflow to +-inf, subnormals kept) by the conversions
// the resampling kernels store with (device_common.hpp round_pair_f16 / round_pair_bf16 / half_bits / bf16_bits; on the host the
// same roundings in integer arithmetic).  The rounding is defined, not exact, so words go into bfloat16 planes too.  scale[c] and
// offset[c] are the same in every lane, as shift[c]; the unscaled form reads neither.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "kernels.h"

#if defined(__HIPCC__)
#include "device_common.hpp"
#define JINC_WIDEN_HD __host__ __device__ __forceinline__
#else
#define JINC_WIDEN_HD inline
#endif

namespace jinc {
namespace widen {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // 16 bytes as ONE access

// 16 N bytes of whole pixels: N 16-byte accesses where the group allows them, else 4 N dwords.
template <int N>
JINC_WIDEN_HD void load_pixels(const char* p, uint32_t unit, uint32_t* w) {
    if (unit == 16) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(p + 16 * k);
            w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4 * N; ++k) w[k] = *reinterpret_cast<const uint32_t*>(p + 4 * k);
    }
}
JINC_WIDEN_HD void store16(char* p, const uint32_t* w) {
    u32x4 v;
    v.x = w[0], v.y = w[1], v.z = w[2], v.w = w[3];
    *reinterpret_cast<u32x4*>(p) = v;
}

// The value of a raw sample as fp32 (v_cvt_f32_ubyte0..3 on the bytes of a dword, v_cvt_f32_u32 behind shift and mask on words).
template <int SB>
JINC_WIDEN_HD float value_of(uint32_t raw, uint32_t shift, uint32_t mask) {
    if constexpr (SB == 1) return static_cast<float>(raw);
    else return static_cast<float>((raw >> shift) & mask);
}
// Sample i of a run of SB-byte samples held in dwords (i is a constant once the loops around the calls are unrolled).
template <int SB>
JINC_WIDEN_HD float value_at(const uint32_t* w, int i, uint32_t shift, uint32_t mask) {
    if constexpr (SB == 1) return value_of<1>((w[i >> 2] >> (8 * (i & 3))) & 0xffu, shift, mask);
    else return value_of<2>((w[i >> 1] >> (16 * (i & 1))) & 0xffffu, shift, mask);
}
JINC_WIDEN_HD uint32_t float_bits(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return b;
}
// binary16 of an fp32 value that is an integer in 0 .. 2047: exact, so every rounding mode gives the same bits.
JINC_WIDEN_HD uint32_t half_bits(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    const _Float16 h = static_cast<_Float16>(v);  // v_cvt_f16_f32
    uint16_t b;
    memcpy(&b, &h, 2);
    return b;
#else
    // (host: no half type needed) fp32 is 1.m x 2^(e - 127) with at most 10 significant bits of m here: the exponent moves from
    // bias 127 to bias 15, the mantissa loses 13 bits that are zeros.
    const uint32_t f = float_bits(v);
    return f ? (f >> 13) - ((127u - 15u) << 10) : 0u;
#endif
}

// The 16-bit sample of an fp32 value that the type holds exactly: binary16, or bfloat16 -- the upper half of the fp32 bits, whose
// lower half is zeros for an integer of at most 8 bits, so nothing is rounded.
template <int KIND>
JINC_WIDEN_HD uint32_t narrow_bits(float v) {
    if constexpr (KIND == kSampleBFloat16) return float_bits(v) >> 16;
    else return half_bits(v);
}

// ---- the scaled form ----
// fl32(fl32(v * scale) + offset): a multiply and an add of their own (v_mul_f32, v_add_f32), whatever the build's contraction setting.
JINC_WIDEN_HD float scaled_value(float v, float scale, float offset) {
#pragma clang fp contract(off)
    const float product = v * scale;
    return product + offset;
}
#if !defined(__HIP_DEVICE_COMPILE__)
// fp32 -> binary16, round to nearest even (host: no half type needed): overflow to +-inf, subnormals kept, a NaN stays one.
JINC_WIDEN_HD uint32_t host_half_rne(float v) {
    const uint32_t f = float_bits(v), sign = (f >> 16) & 0x8000u, a = f & 0x7fffffffu;
    if (a >= 0x7f800000u) return sign | 0x7c00u | (a > 0x7f800000u ? 0x200u : 0u);
    if (a < 0x38800000u) {  // below 2^-14: a multiple of 2^-24 -- |v| x 2^24 is exact, nearbyintf rounds half to even (1024 is 2^-14)
        float m;
        memcpy(&m, &a, 4);
        return sign | static_cast<uint32_t>(nearbyintf(m * 16777216.f));
    }
    const uint32_t r = a + 0xfffu + ((a >> 13) & 1u);  // (a carry out of the mantissa raises the exponent; past 65504 that is 0x7c00, inf)
    const uint32_t h = (r - (112u << 23)) >> 13;
    return sign | (h > 0x7c00u ? 0x7c00u : h);
}
// fp32 -> bfloat16, round to nearest even: the upper half of the bits plus the carry of the lower half (+-inf from 0x7f7f8000 on).
JINC_WIDEN_HD uint32_t host_bf16_rne(float v) {
    const uint32_t f = float_bits(v);
    if ((f & 0x7fffffffu) > 0x7f800000u) return (f >> 16) | 0x40u;  // a NaN stays a NaN
    return (f + 0x7fffu + ((f >> 16) & 1u)) >> 16;
}
#endif
// The 16-bit sample of ANY fp32 value, rounded to nearest even.
template <int KIND>
JINC_WIDEN_HD uint32_t rounded_bits(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (KIND == kSampleBFloat16) return jinc::bf16_bits(v);
    else return jinc::half_bits(v);
#else
    if constexpr (KIND == kSampleBFloat16) return host_bf16_rne(v);
    else return host_half_rne(v);
#endif
}
// Two 16-bit samples as one dword, (a) in the low half.
template <int KIND, bool Scaled>
JINC_WIDEN_HD uint32_t pair_bits(float a, float b) {
    if constexpr (!Scaled) {
        return narrow_bits<KIND>(a) | (narrow_bits<KIND>(b) << 16);
    } else {
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (KIND == kSampleBFloat16) return round_pair_bf16(a, b);
        else return round_pair_f16(a, b);
#else
        return rounded_bits<KIND>(a) | (rounded_bits<KIND>(b) << 16);
#endif
    }
}
// Sample i of the loaded dwords as the plane holds it in fp32.
template <int SB, bool Scaled>
JINC_WIDEN_HD float sample_at(const uint32_t* w, int i, uint32_t shift, uint32_t mask, float scale, float offset) {
    if constexpr (Scaled) return scaled_value(value_at<SB>(w, i, shift, mask), scale, offset);
    else return value_at<SB>(w, i, shift, mask);
}

// Lane `lane` of the wave that owns row `row` of frame `frame` of group g.
template <int SB, int N, int OB, int KIND = 0, bool Scaled = false>
JINC_WIDEN_HD void widen_row(const WidenGroup& g, uint32_t mask, uint32_t frame, uint32_t row, uint32_t lane) {
    static_assert((SB == 1 || SB == 2) && N >= 1 && N <= 4 && (OB == 4 || OB == 2), "no such form");
    static_assert(KIND == 0 || KIND == kSampleHalf || (KIND == kSampleBFloat16 && OB == 2 && (SB == 1 || Scaled)), "no such form");
    constexpr uint32_t P = 16 / SB;          // pixels a lane owns per step
    constexpr int kVectors = OB / SB;        // 16-byte vectors of P converted samples
    constexpr int kPerVector = 16 / OB;      // samples in one of them
    const char* __restrict__ packed = g.packed + frame * g.packed_frame_stride + static_cast<size_t>(row) * g.packed_pitch;
    const size_t dense = frame * g.plane_frame_stride + static_cast<size_t>(row) * g.plane_pitch;
    for (uint32_t x = lane * P; x < g.vec_pixels; x += 64 * P) {
        uint32_t in[4 * N];
        load_pixels<N>(packed + static_cast<size_t>(x) * (N * SB), g.unit, in);
#pragma unroll
        for (int c = 0; c < N; ++c) {
            if (!g.plane[c]) continue;
            const uint32_t sh = g.shift[c];
            float sc = 1.f, of = 0.f;
            if constexpr (Scaled) sc = g.scale[c], of = g.offset[c];
            char* out = g.plane[c] + dense + static_cast<size_t>(x) * OB;
#pragma unroll
            for (int v = 0; v < kVectors; ++v) {
                uint32_t o[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int p = v * kPerVector + (OB == 4 ? k : 2 * k);  // the pixel of dword k's (first) sample
                    if constexpr (OB == 4) o[k] = float_bits(sample_at<SB, Scaled>(in, p * N + c, sh, mask, sc, of));
                    else o[k] = pair_bits<KIND, Scaled>(sample_at<SB, Scaled>(in, p * N + c, sh, mask, sc, of), sample_at<SB, Scaled>(in, (p + 1) * N + c, sh, mask, sc, of));
                }
                store16(out + 16 * v, o);
            }
        }
    }
    for (uint32_t x = g.vec_pixels + lane; x < g.width; x += 64) {
#pragma unroll
        for (int c = 0; c < N; ++c) {
            if (!g.plane[c]) continue;
            uint32_t raw;
            if constexpr (SB == 1) raw = reinterpret_cast<const uint8_t*>(packed)[static_cast<size_t>(x) * N + c];
            else raw = reinterpret_cast<const uint16_t*>(packed)[static_cast<size_t>(x) * N + c];
            float v = value_of<SB>(raw, g.shift[c], mask);
            if constexpr (Scaled) v = scaled_value(v, g.scale[c], g.offset[c]);
            if constexpr (OB == 4) reinterpret_cast<float*>(g.plane[c] + dense)[x] = v;
            else if constexpr (Scaled) reinterpret_cast<uint16_t*>(g.plane[c] + dense)[x] = static_cast<uint16_t>(rounded_bits<KIND>(v));
            else reinterpret_cast<uint16_t*>(g.plane[c] + dense)[x] = static_cast<uint16_t>(narrow_bits<KIND>(v));
        }
    }
}

}  // namespace widen
}  // namespace jinc
