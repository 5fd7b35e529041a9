// matrix_rows.h -- one lane's share of one row of the output matrix pass (kernel_matrix.hip output_matrix_kernel; kernels.h
// MatrixArgs), as plain inline functions for host and device: a stand-alone host program runs exactly this code lane by lane against
// exactly sized buffers (tests/host_sanitizer/matrix_rows_main.cpp).  The shape of narrow_rows.h.
//
// Planes 0 .. 2 of a float filter's results -- fp32 (KIND 0), binary16 (kSampleHalf) or bfloat16 (kSampleBFloat16), three planes of
// one size -- are updated IN PLACE: with r0, r1, r2 the three samples of a pixel widened exactly to fp32, plane i gets
//   fl32(fl32(fl32(fl32(m[3i] * r0) + fl32(m[3i+1] * r1)) + fl32(m[3i+2] * r2)) + offset[i])
// -- three multiplies and three adds of their own, in this order, never an FMA -- and a 16-bit filter rounds that to nearest even
// into its sample type by the conversions the resampling kernels store with (device_common.hpp round_pair_f16 / round_pair_bf16 /
// half_bits / bf16_bits; on the host widen_rows.h's integer arithmetic with the same values).
//
// A lane owns 16 bytes per plane per step, 4 fp32 or 8 sixteen-bit pixels: three 16-byte loads, then three 16-byte stores (four
// dwords each where base, pitch or frame stride is a multiple of 4 only); consecutive lanes, consecutive addresses.  What is left
// moves sample by sample under the width guard: a row's tail, and the whole row where even 4-byte alignment fails (vec_pixels 0).
// A lane reads all three samples of its pixels before it stores any of them, and no other lane touches them: in place is safe.
// Nothing beyond `width` samples of a row is read or written.  The matrix and the offset are the same in every lane.
#pragma once
#include "narrow_rows.h"
#include "widen_rows.h"

#if defined(__HIPCC__)
#define JINC_MATRIX_HD __host__ __device__ __forceinline__
#else
#define JINC_MATRIX_HD inline
#endif

namespace jinc {
namespace matrix {

// Row i of the matrix on one pixel: every product and every sum rounded to fp32 on its own, whatever the build's contraction setting.
JINC_MATRIX_HD float mixed(const float* m, float offset, float r0, float r1, float r2) {
#pragma clang fp contract(off)
    const float p0 = m[0] * r0;
    const float p1 = m[1] * r1;
    const float p2 = m[2] * r2;
    const float two = p0 + p1;
    const float three = two + p2;
    return three + offset;
}

JINC_MATRIX_HD void load_lane(const char* p, uint32_t unit, uint32_t* w) { widen::load_pixels<1>(p, unit, w); }
JINC_MATRIX_HD void store_lane(char* p, uint32_t unit, const uint32_t* w) { narrow::store_pixels<1>(p, unit, w); }

// Lane `lane` of the wave that owns row `row` of frame `frame`.
template <int KIND>
JINC_MATRIX_HD void matrix_row(const MatrixArgs& a, uint32_t frame, uint32_t row, uint32_t lane) {
    static_assert(KIND == 0 || KIND == kSampleHalf || KIND == kSampleBFloat16, "no such form");
    constexpr int SB = narrow::input_bytes(KIND);
    constexpr uint32_t P = 16 / SB;  // pixels a lane owns per step
    char* line[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) line[c] = a.plane[c] + static_cast<size_t>(frame) * a.frame_stride[c] + static_cast<size_t>(row) * a.pitch[c];
    for (uint32_t x = lane * P; x < a.vec_pixels; x += 64 * P) {
        const size_t at = static_cast<size_t>(x) * SB;
        uint32_t in[3][4], out[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) load_lane(line[c] + at, a.unit, in[c]);  // (all three before any store)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            float o[P];
#pragma unroll
            for (int p = 0; p < static_cast<int>(P); ++p)
                o[p] = mixed(a.m + 3 * i, a.offset[i], narrow::value_at<KIND>(in[0], p), narrow::value_at<KIND>(in[1], p), narrow::value_at<KIND>(in[2], p));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if constexpr (KIND == 0) out[i][k] = widen::float_bits(o[k]);
                else out[i][k] = widen::pair_bits<KIND, true>(o[2 * k], o[2 * k + 1]);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) store_lane(line[c] + at, a.unit, out[c]);
    }
    for (uint32_t x = a.vec_pixels + lane; x < a.width; x += 64) {
        const float r0 = narrow::value_in_row<KIND>(line[0], x), r1 = narrow::value_in_row<KIND>(line[1], x), r2 = narrow::value_in_row<KIND>(line[2], x);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float o = mixed(a.m + 3 * i, a.offset[i], r0, r1, r2);
            if constexpr (KIND == 0) reinterpret_cast<float*>(line[i])[x] = o;
            else reinterpret_cast<uint16_t*>(line[i])[x] = static_cast<uint16_t>(widen::rounded_bits<KIND>(o));
        }
    }
}

}  // namespace matrix
}  // namespace jinc
