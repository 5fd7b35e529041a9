// narrow_rows.h -- one lane's share of one row of the narrowing pass (kernel_narrow.hip narrow_samples_kernel; kernels.h NarrowGroup),
// as plain inline functions for host and device: a stand-alone host program runs exactly this code lane by lane against exactly
// sized buffers (tests/host_sanitizer/narrow_rows_main.cpp).  The mirror image of widen_rows.h.
//
// The results of a float filter -- fp32 (KIND 0), binary16 (kSampleHalf) or bfloat16 (kSampleBFloat16) samples of up to N dense
// planes -- become integer samples of DB bytes (1: a byte; 2: a little-endian 16-bit word), N per pixel: channel c of a pixel is
// lrintf(clamp(r, 0, peak)) << shift[c] with r the plane's sample widened exactly to fp32 (ref JincResize.cpp:582: what the integer
// filters end in).  Round half to even; a NaN, -inf and -0 become 0, +inf becomes peak.  On the device the conversion is
// device_common.hpp's: round_sample_u8 for bytes (peak is 255 then), round_pair_u16 for the word pairs of the vectors, round_sample
// for single words; on the host a plain clamp and nearbyintf with the same values.
//
// A lane owns 16 / DB whole pixels per step: per plane (input bytes / DB) adjacent 16-byte loads from the 256-byte-aligned stand-ins
// (consecutive lanes, consecutive addresses) and N 16-byte stores on the destination side that lie side by side (4 N dwords where
// base, pitch or frame stride is a multiple of 4 only) -- a wave's trip stores one piece of 64 x 16 x N bytes.  The samples are put
// into the dwords with shifts whose amounts are compile-time constants; shift[c] and the peak are the same in every lane.
// What is left moves sample by sample under a width guard: a row's tail, groups whose base, pitch or frame stride is no multiple of
// 4 bytes and groups with a channel missing (vec_pixels 0: only the given channels' samples may be stored to).  Nothing beyond
// `width` samples is read from a plane or stored to a channel; the destination is never read, the planes are never written.
//
// The scaled form (trailing template parameter Scaled; jinc_filter_process_device_narrowed_scaled): channel c of a pixel is
// lrintf(clamp(fl32(fl32(r * scale[c]) + offset[c]), 0, peak)) << shift[c] -- one multiply and one add in front of the same
// conversions, two fp32 roundings, never an FMA, in the vector loop and in the sample-by-sample loop alike.  scale[c] and offset[c]
// are the same in every lane, as shift[c]; the unscaled form reads neither.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "kernels.h"

#if defined(__HIPCC__)
#include "device_common.hpp"
#define JINC_NARROW_HD __host__ __device__ __forceinline__
#else
#define JINC_NARROW_HD inline
#endif

namespace jinc {
namespace narrow {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // 16 bytes as ONE access

constexpr int input_bytes(int kind) { return kind == 0 ? 4 : 2; }

JINC_NARROW_HD void load16(const char* p, uint32_t* w) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(p);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
}
// 16 N bytes of whole pixels: N 16-byte accesses where the group allows them, else 4 N dwords.
template <int N>
JINC_NARROW_HD void store_pixels(char* p, uint32_t unit, const uint32_t* w) {
    if (unit == 16) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            u32x4 v;
            v.x = w[4 * k], v.y = w[4 * k + 1], v.z = w[4 * k + 2], v.w = w[4 * k + 3];
            *reinterpret_cast<u32x4*>(p + 16 * k) = v;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4 * N; ++k) *reinterpret_cast<uint32_t*>(p + 4 * k) = w[k];
    }
}

JINC_NARROW_HD float float_of_bits(uint32_t b) {
    float v;
    memcpy(&v, &b, 4);
    return v;
}
// A 16-bit float sample widened exactly to fp32 (device: v_cvt_f32_f16 / a shift; host: plain integer arithmetic, no half type).
template <int KIND>
JINC_NARROW_HD float value_of16(uint32_t h) {
    if constexpr (KIND == kSampleBFloat16) {
        return float_of_bits(h << 16);
    } else {
#if defined(__HIP_DEVICE_COMPILE__)
        return to_float(__builtin_bit_cast(half_t, static_cast<uint16_t>(h)));
#else
        const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 1023u;
        if (e == 31u) return float_of_bits(sign | 0x7f800000u | (m << 13));                  // infinities and NaNs
        if (e) return float_of_bits(sign | ((e + 127u - 15u) << 23) | (m << 13));             // normal numbers
        const float sub = static_cast<float>(m) * 5.9604644775390625e-8f;                     // m x 2^-24: exact
        return sign ? -sub : sub;
#endif
    }
}
// Sample i of a run of a plane's samples held in dwords (i is a constant once the loops around the calls are unrolled).
template <int KIND>
JINC_NARROW_HD float value_at(const uint32_t* w, int i) {
    if constexpr (KIND == 0) {
        return float_of_bits(w[i]);
    } else if constexpr (KIND == kSampleBFloat16) {
#if defined(__HIP_DEVICE_COMPILE__)
        return (i & 1) ? bf16_hi(w[i >> 1]) : bf16_lo(w[i >> 1]);
#else
        return value_of16<KIND>((w[i >> 1] >> (16 * (i & 1))) & 0xffffu);
#endif
    } else {
        return value_of16<KIND>((w[i >> 1] >> (16 * (i & 1))) & 0xffffu);
    }
}
// Sample x of a plane's row.
template <int KIND>
JINC_NARROW_HD float value_in_row(const char* row, size_t x) {
    if constexpr (KIND == 0) return reinterpret_cast<const float*>(row)[x];
    else return value_of16<KIND>(reinterpret_cast<const uint16_t*>(row)[x]);
}

// lrintf(clamp(r, 0, peak)): device_common.hpp's helpers on the device, the same values in plain C++ on the host (nearbyintf under
// the default rounding mode rounds half to even; !(r > 0) takes NaNs, -0 and everything negative to 0).
#if !defined(__HIP_DEVICE_COMPILE__)
JINC_NARROW_HD uint32_t host_round(float r, float peak) {
    if (!(r > 0.f)) return 0u;
    return static_cast<uint32_t>(nearbyintf(r < peak ? r : peak));
}
#endif
JINC_NARROW_HD uint32_t byte_of(float r) {
#if defined(__HIP_DEVICE_COMPILE__)
    return round_sample_u8(r);
#else
    return host_round(r, 255.f);
#endif
}
JINC_NARROW_HD uint32_t word_of(float r, float peak) {
#if defined(__HIP_DEVICE_COMPILE__)
    return round_sample(r, peak);
#else
    return host_round(r, peak);
#endif
}
JINC_NARROW_HD uint32_t word_pair_of(float a, float b, float peak) {  // (a) in the low half
#if defined(__HIP_DEVICE_COMPILE__)
    return round_pair_u16(a, b, peak);
#else
    return host_round(a, peak) | (host_round(b, peak) << 16);
#endif
}

// fl32(fl32(r * scale) + offset): a multiply and an add of their own (v_mul_f32, v_add_f32), whatever the build's contraction setting.
JINC_NARROW_HD float scaled_value(float r, float scale, float offset) {
#pragma clang fp contract(off)
    const float product = r * scale;
    return product + offset;
}
// Sample i of the loaded dwords / sample x of a row as the conversion takes it.
template <int KIND, bool Scaled>
JINC_NARROW_HD float result_at(const uint32_t* w, int i, float scale, float offset) {
    if constexpr (Scaled) return scaled_value(value_at<KIND>(w, i), scale, offset);
    else return value_at<KIND>(w, i);
}

// Lane `lane` of the wave that owns row `row` of frame `frame` of group g.
template <int KIND, int N, int DB, bool Scaled = false>
JINC_NARROW_HD void narrow_row(const NarrowGroup& g, float peak, uint32_t frame, uint32_t row, uint32_t lane) {
    static_assert((KIND == 0 || KIND == kSampleHalf || KIND == kSampleBFloat16) && N >= 1 && N <= 4 && (DB == 1 || DB == 2), "no such form");
    constexpr int IB = input_bytes(KIND);
    constexpr uint32_t P = 16 / DB;   // pixels a lane owns per step
    constexpr int kLoads = IB / DB;   // 16-byte vectors of P samples of one plane
    char* __restrict__ packed = g.packed + frame * g.packed_frame_stride + static_cast<size_t>(row) * g.packed_pitch;
    const size_t dense = frame * g.plane_frame_stride + static_cast<size_t>(row) * g.plane_pitch;
    for (uint32_t x = lane * P; x < g.vec_pixels; x += 64 * P) {  // (complete groups only: every byte of these pixels is a given sample)
        uint32_t out[4 * N];
#pragma unroll
        for (int k = 0; k < 4 * N; ++k) out[k] = 0u;
#pragma unroll
        for (int c = 0; c < N; ++c) {
            uint32_t in[4 * kLoads];
            const char* plane = g.plane[c] + dense + static_cast<size_t>(x) * IB;
            float sc = 1.f, of = 0.f;
            if constexpr (Scaled) sc = g.scale[c], of = g.offset[c];
#pragma unroll
            for (int k = 0; k < kLoads; ++k) load16(plane + 16 * k, in + 4 * k);
            if constexpr (DB == 1) {  // (a byte takes no shift)
#pragma unroll
                for (int p = 0; p < static_cast<int>(P); ++p) {
                    const int i = p * N + c;
                    out[i >> 2] |= byte_of(result_at<KIND, Scaled>(in, p, sc, of)) << (8 * (i & 3));
                }
            } else {
                const uint32_t sh = g.shift[c];  // (peak << sh stays below 65536: nothing crosses from the low half into the high one)
#pragma unroll
                for (int p = 0; p < static_cast<int>(P); p += 2) {
                    const uint32_t pair = word_pair_of(result_at<KIND, Scaled>(in, p, sc, of), result_at<KIND, Scaled>(in, p + 1, sc, of), peak) << sh;
                    if constexpr (N == 1) {
                        out[p >> 1] = pair;
                    } else {
                        const int i = p * N + c, j = (p + 1) * N + c;
                        out[i >> 1] |= (pair & 0xffffu) << (16 * (i & 1));
                        out[j >> 1] |= (pair >> 16) << (16 * (j & 1));
                    }
                }
            }
        }
        store_pixels<N>(packed + static_cast<size_t>(x) * (N * DB), g.unit, out);
    }
    for (uint32_t x = g.vec_pixels + lane; x < g.width; x += 64) {
#pragma unroll
        for (int c = 0; c < N; ++c) {
            if (!g.plane[c]) continue;
            float r = value_in_row<KIND>(g.plane[c] + dense, x);
            if constexpr (Scaled) r = scaled_value(r, g.scale[c], g.offset[c]);
            if constexpr (DB == 1) reinterpret_cast<uint8_t*>(packed)[static_cast<size_t>(x) * N + c] = static_cast<uint8_t>(byte_of(r));
            else reinterpret_cast<uint16_t*>(packed)[static_cast<size_t>(x) * N + c] = static_cast<uint16_t>(word_of(r, peak) << g.shift[c]);
        }
    }
}

}  // namespace narrow
}  // namespace jinc
