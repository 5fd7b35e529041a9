// kernel_matrix.hip -- the 3x3 output matrix of a float filter (jinc_filter_set_output_matrix): planes 0 .. 2 of the results an
// fp32 / binary16 / bfloat16 filter's kernels have written -- Y', Cb, Cr on one grid, say -- become o = M r + offset in place, R', G',
// B' for a network or a display.  A pass of its own between the resampling kernels and the destination pass of a call
// (stand_ins.cpp apply_output_matrix), so that every device call has it and no other kernel knows of it.
//
// Shape, after narrow_samples_kernel: ONE launch covers every row and frame of a slice (grid = row blocks x frames), a wave owns a
// row, its lanes walk along it, and no access costs a division or a modulo.  The row function is matrix_rows.h: a lane owns 16 bytes
// per plane per step -- three 16-byte loads, 3 x (3 v_mul_f32 + 3 v_add_f32) per pixel with the twelve coefficients in scalar
// registers (-ffp-contract=off and the row function's own pragma keep them apart), three 16-byte stores (dwords where the planes'
// alignment allows no more); tails and planes that are not even 4-byte aligned move sample by sample.  Plain C++: no assembly, no
// LDS, no scratch.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "matrix_rows.h"

namespace jinc {
namespace {

// Row blockIdx.x * 4 + wave of frame blockIdx.y.
template <int KIND>
__global__ __launch_bounds__(256) void output_matrix_kernel(const MatrixArgs a) {
    const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row < a.rows) matrix::matrix_row<KIND>(a, blockIdx.y, row, threadIdx.x & 63u);
}

template <int KIND>
int launch(const MatrixArgs& a, const dim3& grid, hipStream_t s) {
    hipLaunchKernelGGL((output_matrix_kernel<KIND>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace

int launch_output_matrix(const MatrixArgs& a, int kind, int nframes, void* stream) {
    if (kind != 0 && kind != kSampleHalf && kind != kSampleBFloat16) return hipErrorInvalidValue;  // (never a silent skip)
    if (nframes <= 0 || a.rows == 0 || a.width == 0) return hipSuccess;
    if (nframes > 65535) return hipErrorInvalidValue;
    const uint32_t lane_pixels = kind == 0 ? 4u : 8u;
    if (a.unit != 16 && a.unit != 4 && a.unit != 0) return hipErrorInvalidValue;
    if (a.vec_pixels > a.width || a.vec_pixels % lane_pixels || (a.vec_pixels && !a.unit)) return hipErrorInvalidValue;
    for (int c = 0; c < 3; ++c) {
        if (!a.plane[c]) return hipErrorInvalidValue;
        const uintptr_t al = reinterpret_cast<uintptr_t>(a.plane[c]) | a.pitch[c] | (nframes > 1 ? a.frame_stride[c] : 0);
        if (a.vec_pixels && al % a.unit) return hipErrorInvalidValue;  // (the accesses of the vector loop are aligned ones)
    }
    const dim3 grid((a.rows + 3) / 4, static_cast<uint32_t>(nframes));
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (kind) {
        case 0: return launch<0>(a, grid, s);
        case kSampleHalf: return launch<kSampleHalf>(a, grid, s);
        default: return launch<kSampleBFloat16>(a, grid, s);
    }
}

}  // namespace jinc
