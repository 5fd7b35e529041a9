// device_common.hpp -- helpers shared by the gfx950 kernels of libjincresize_hip.so (included by every
// kernel_*.hip translation unit; everything lives in an anonymous namespace, so each TU has its own copy).
//
// The result of the resampling path is DEFINED by the reference's opt=0 code: per output sample a strictly
// sequential fp32 chain   r = 0; for ly: for lx: r = fl(r + fl(float(src) * coeff))
// (/root/reference/src/JincResize.cpp:570-579) followed by clamp + round-half-even for integer planes
// (ref :581-582).  Therefore, in every kernel:
//   * one lane owns one output sample's whole chain; cross-lane operations move data only;
//   * multiply and add stay un-fused: the kernel files are compiled with -ffp-contract=off AND carry the
//     pragma below; tests/test_build.py greps the ISA for v_fma / v_fmac / v_mad / v_pk_fma / v_mfma;
//   * fp32 denormals are kept (gfx9 default; no -fgpu-flush-denormals-to-zero).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <type_traits>

#include "kernels.h"

#pragma clang fp contract(off)

namespace jinc {
namespace {

#define JINC_CONSTANT __attribute__((address_space(4)))

// IEEE binary16 planes (PlaneIO::sample_kind == kSampleHalf): samples widen exactly to fp32 on load (v_cvt_f32_f16), the fp32 chain
// is the float planes' one, and the result narrows under the default round mode (round to nearest even, v_cvt_f16_f32): overflow
// to +-inf, subnormals and the sign of zero kept, no clamp -- float planes' semantics end to end.  (Never the packed
// round-toward-zero conversion: it saturates at 65504 and rounds differently.)
using half_t = _Float16;

// bfloat16 planes (PlaneIO::sample_kind == kSampleBFloat16): a sample is the upper 16 bits of an fp32 value, so it widens with a
// shift (no conversion instruction; exact for every pattern, subnormals, infinities and NaNs included), the fp32 chain is the float
// planes' one, and the result narrows with round to nearest even (gfx950: v_cvt_pk_bf16_f32, two results per instruction): results
// at or beyond 0x7f7f8000 in magnitude become +-inf, subnormals and the sign of zero are kept, a NaN stays a NaN, no clamp.
using bf16_t = __bf16;

// Float-like samples (fp32, binary16 and bfloat16): no clamp, non-finite samples possible -- no zero-tap elision on frames that
// hold one.
template <typename T>
inline constexpr bool is_float_sample_v = std::is_same_v<T, float> || std::is_same_v<T, half_t> || std::is_same_v<T, bf16_t>;

template <typename T>
__device__ __forceinline__ float to_float(T v) {
    if constexpr (std::is_same_v<T, bf16_t>)
        return __builtin_bit_cast(float, static_cast<uint32_t>(__builtin_bit_cast(uint16_t, v)) << 16);
    else
        return static_cast<float>(v);
}

// Bit 31 set when v is an infinity or a NaN (exponent field all ones: the biased field plus one carries into the sign bit);
// 0 for integer samples.
template <typename T>
__device__ __forceinline__ uint32_t nonfinite_bit(T v) {
    if constexpr (std::is_same_v<T, float>)
        return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) + 0x00800000u;
    else if constexpr (std::is_same_v<T, half_t>)
        return ((static_cast<uint32_t>(__builtin_bit_cast(uint16_t, v)) & 0x7c00u) + 0x0400u) << 16;
    else if constexpr (std::is_same_v<T, bf16_t>)
        return ((static_cast<uint32_t>(__builtin_bit_cast(uint16_t, v)) & 0x7f80u) + 0x0080u) << 16;
    else
        return 0u;
}

__device__ __forceinline__ uint16_t half_bits(float r) { return __builtin_bit_cast(uint16_t, static_cast<half_t>(r)); }
// The two binary16 samples of a dword (low half first) widened to fp32.
__device__ __forceinline__ float half_lo(uint32_t w) { return static_cast<float>(__builtin_bit_cast(half_t, static_cast<uint16_t>(w))); }
__device__ __forceinline__ float half_hi(uint32_t w) { return static_cast<float>(__builtin_bit_cast(half_t, static_cast<uint16_t>(w >> 16))); }
// ... and the two bfloat16 samples of a dword: one shift, one mask.
__device__ __forceinline__ float bf16_lo(uint32_t w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t w) { return __builtin_bit_cast(float, w & 0xffff0000u); }
// The two 2-byte float samples of a dword, by type.
template <typename T>
__device__ __forceinline__ float float16_lo(uint32_t w) {
    if constexpr (std::is_same_v<T, bf16_t>) return bf16_lo(w);
    else return half_lo(w);
}
template <typename T>
__device__ __forceinline__ float float16_hi(uint32_t w) {
    if constexpr (std::is_same_v<T, bf16_t>) return bf16_hi(w);
    else return half_hi(w);
}

// ref :581-582 -- clamp(result, 0, peak) then lrintf (round-half-even).  For every non-NaN input
// v_med3_f32(r, 0, peak) equals the reference's "upper bound first, then lower" clamp; a NaN (only
// reachable through non-finite coefficients) ends as 0 on both sides.
__device__ __forceinline__ uint32_t round_sample(float r, float peak) {
    return static_cast<uint32_t>(__builtin_rintf(__builtin_amdgcn_fmed3f(r, 0.f, peak)));
}

// 8-bit planes (peak is always 255): v_cvt_pk_u8_f32 rounds to nearest even (MODE.fp_round default) and
// saturates to [0, 255] in one instruction -- the same value as clamp + lrintf for every input, NaN -> 0.
// tests/test_gpu_parity.py::test_integer_conversion_ties checks ties, bounds and specials on the device.
__device__ __forceinline__ uint32_t round_sample_u8(float r) { return __builtin_amdgcn_cvt_pk_u8_f32(r, 0u, 0u); }

// Two 9 ... 16-bit samples as one dword, (a) in the low half: clamp as round_sample, then round-half-even by adding 2^23 -- the
// sum of a value in [0, 65535] and 8388608.0f has an ulp of 1, so its low mantissa bits ARE the sample rounded to nearest, ties to
// even (2^23 is even: the tie rule of the sum is the tie rule of the sample) -- and v_perm_b32 picks the two low halves: five
// instructions per pair against seven (v_med3, v_rndne, v_cvt_u32 each and a v_lshl_or).  The same value as round_sample for every
// input (NaN: v_med3 returns 0 first); tests/test_gpu_parity.py::test_integer_conversion_ties runs both forms over ties and bounds.
__device__ __forceinline__ uint32_t round_pair_u16(float a, float b, float peak) {
    const float ca = __builtin_amdgcn_fmed3f(a, 0.f, peak) + 8388608.0f, cb = __builtin_amdgcn_fmed3f(b, 0.f, peak) + 8388608.0f;
    return __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, cb), __builtin_bit_cast(uint32_t, ca), 0x05040100u);
}

// Two binary16 samples as one dword, (a) in the low half: round_pair_u16's analogue for half planes (two v_cvt_f16_f32).
__device__ __forceinline__ uint32_t round_pair_f16(float a, float b) {
    return static_cast<uint32_t>(half_bits(a)) | (static_cast<uint32_t>(half_bits(b)) << 16);
}
// bfloat16: both halves from ONE v_cvt_pk_bf16_f32 (the vector conversion selects it; two scalar casts cost a shift more).
typedef float f32x2_cvt __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_cvt __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t round_pair_bf16(float a, float b) {
    const f32x2_cvt v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_cvt));
}
__device__ __forceinline__ uint16_t bf16_bits(float r) { return __builtin_bit_cast(uint16_t, static_cast<bf16_t>(r)); }
// A pair of samples of type T packed into one dword (2-byte samples only).
template <typename T>
__device__ __forceinline__ uint32_t round_pair16(float a, float b, float peak) {
    if constexpr (std::is_same_v<T, half_t>)
        return round_pair_f16(a, b);
    else if constexpr (std::is_same_v<T, bf16_t>)
        return round_pair_bf16(a, b);
    else
        return round_pair_u16(a, b, peak);
}

template <typename T>
__device__ __forceinline__ T convert_sample(float r, float peak) {
    if constexpr (std::is_same_v<T, float>)
        return r;
    else if constexpr (std::is_same_v<T, half_t>)
        return static_cast<half_t>(r);
    else if constexpr (std::is_same_v<T, bf16_t>)
        return static_cast<bf16_t>(r);
    else if constexpr (std::is_same_v<T, uint8_t>)
        return static_cast<uint8_t>(round_sample_u8(r));
    else
        return static_cast<T>(round_sample(r, peak));
}

template <typename T>
__device__ __forceinline__ void store_sample(T* p, float r, float peak) {
    *p = convert_sample<T>(r, peak);
}

// Store through a buffer resource: per-lane byte offset in a VGPR that never changes, the row offset in
// an SGPR -- no address arithmetic on the VALU (the binding unit of these kernels) per stored sample.
using BufferRsrc = __amdgpu_buffer_rsrc_t;
__device__ __forceinline__ BufferRsrc make_rsrc(void* base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(base, 0, bytes, 0x00020000);
}
template <typename T>
__device__ __forceinline__ void store_sample_buf(BufferRsrc rsrc, uint32_t voffset, uint32_t soffset, float r, float peak) {
    if constexpr (std::is_same_v<T, float>)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, r), rsrc, voffset, soffset, 0);
    else if constexpr (std::is_same_v<T, half_t>)
        __builtin_amdgcn_raw_buffer_store_b16(half_bits(r), rsrc, voffset, soffset, 0);
    else if constexpr (std::is_same_v<T, bf16_t>)
        __builtin_amdgcn_raw_buffer_store_b16(bf16_bits(r), rsrc, voffset, soffset, 0);
    else if constexpr (std::is_same_v<T, uint8_t>)
        __builtin_amdgcn_raw_buffer_store_b8(static_cast<uint8_t>(round_sample_u8(r)), rsrc, voffset, soffset, 0);
    else
        __builtin_amdgcn_raw_buffer_store_b16(static_cast<uint16_t>(round_sample(r, peak)), rsrc, voffset, soffset, 0);
}

// Coefficient rows are padded to a multiple of 4 floats on the device (16-byte aligned rows).
__host__ __device__ constexpr int padded_row(int fs) { return (fs + 3) & ~3; }

// XCD-aware tile order.  Workgroups are dealt round-robin over the 8 XCDs (each with its own L2) in
// linear-id order, so neighbouring linear ids land on different XCDs and every XCD would fetch its own copy
// of the halo rows/columns shared by adjacent tiles.  Re-map the linear id so that each XCD walks a
// contiguous run of tiles of the frame (bijective for any tile count; placement affects speed only).
__device__ __forceinline__ void swizzled_tile(int& tx, int& ty) {
    const int n = gridDim.x * gridDim.y;
    const int lin = blockIdx.y * gridDim.x + blockIdx.x;
    constexpr int kXcds = 8;
    const int q = n / kXcds, rem = n % kXcds;
    const int xcd = lin % kXcds, idx = lin / kXcds;
    // XCD k owns q (+1 if k < rem) consecutive tiles starting at k*q + min(k, rem)
    const int tile_id = xcd * q + (xcd < rem ? xcd : rem) + idx;
    ty = tile_id / gridDim.x;
    tx = tile_id - ty * gridDim.x;
}

}  // namespace
}  // namespace jinc
