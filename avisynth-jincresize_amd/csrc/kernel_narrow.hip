// kernel_narrow.hip -- the dense fp32 / binary16 / bfloat16 planes a float filter's kernels have written -> integer samples, behind
// jinc_filter_process_device_narrowed (dispatch.cpp enqueue_narrowed): the results of a float, half or bfloat16 filter become the
// planes of an encoder's or a display's NV12 / P010 / Y210 surface, packed 8-bit RGB(A) or planar integer frames.  A merge
// (kernel_interleave.hip) that NARROWS: it stores lrintf(clamp(r, 0, peak)) << shift[c] as channel c of N interleaved samples -- the
// step the integer filters end in (ref JincResize.cpp:582), through device_common.hpp's round_sample_u8 / round_pair_u16 /
// round_sample, so a float filter followed by this pass is the integer filter of the same geometry whenever the float planes hold
// integers.  The mirror image of kernel_widen.hip's widen_samples_kernel.
//
// Shape, after merge_samples_kernel and widen_samples_kernel: ONE launch covers every channel group and frame of a slice (grid = row
// blocks x frames x groups; the groups travel as kernel arguments, kernels.h NarrowArgs), a wave owns a row, its lanes walk along it,
// and no access costs a division or a modulo.  The row function is narrow_rows.h: a lane owns 16 / DB whole pixels per step, IB / DB
// 16-byte loads per plane and N 16-byte stores (dwords where the group's alignment allows no more); tails, unaligned groups and
// groups with a channel missing store sample by sample and only their own samples.  The destination is never read.  Plain C++: no
// assembly, no LDS, no scratch.
// The scaled forms (jinc_filter_process_device_narrowed_scaled) are the same kernel with one v_mul_f32 and one v_add_f32 per sample
// in front of the conversion (scale[c], offset[c] of the group's channel in scalar registers; -ffp-contract=off keeps them apart).
//
// Two more destinations whose samples neither a step nor a shift addresses (jinc_filter_process_device_narrowed_packed10 / _v210;
// dispatch.cpp enqueue_narrowed_packed10 / enqueue_narrowed_v210): 10:10:10:2 words -- Y410, R10G10B10A2 and kin -- and v210 blocks.
// narrow_fields_kernel has the shape of pack_fields_kernel and narrow_v210_kernel that of pack_v210_kernel (kernel_interleave.hip):
// one launch over every row and frame of a slice, grid = row blocks x frames, a wave owns a row; they read float samples where those
// read 16-bit integers and convert them -- lrintf(clamp(r, 0, 1023)), behind the scaled forms' multiply and add -- in front of the
// packing.  The row functions are narrow_fields_rows.h and narrow_v210_rows.h; the exchange between the two lanes of a block pair is
// v210_exchange.h's, 10-bit CODES behind the conversion.  Plain C++ and that one DPP builtin: no assembly, no LDS, no scratch.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "narrow_fields_rows.h"
#include "narrow_rows.h"
#include "narrow_v210_rows.h"
#include "v210_exchange.h"

namespace jinc {
namespace {

// Row blockIdx.x * 4 + wave of frame blockIdx.y of group blockIdx.z.
template <int KIND, int N, int DB, bool Scaled>
__global__ __launch_bounds__(256) void narrow_samples_kernel(const NarrowArgs a) {
    const NarrowGroup& g = a.g[blockIdx.z];
    const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row < g.rows) narrow::narrow_row<KIND, N, DB, Scaled>(g, a.peak, blockIdx.y, row, threadIdx.x & 63u);
}

template <int KIND, int N, int DB, bool Scaled>
int launch(const NarrowArgs& a, int nframes, hipStream_t s) {
    uint32_t rows = 0;
    for (int k = 0; k < a.ngroups; ++k) rows = a.g[k].rows > rows ? a.g[k].rows : rows;
    if (a.ngroups <= 0 || nframes <= 0 || rows == 0) return hipSuccess;
    const dim3 grid((rows + 3) / 4, static_cast<uint32_t>(nframes), static_cast<uint32_t>(a.ngroups));
    hipLaunchKernelGGL((narrow_samples_kernel<KIND, N, DB, Scaled>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

template <int KIND, int DB, bool Scaled>
int launch_by_step(const NarrowArgs& a, int step, int nframes, hipStream_t s) {
    switch (step) {
        case 1: return launch<KIND, 1, DB, Scaled>(a, nframes, s);
        case 2: return launch<KIND, 2, DB, Scaled>(a, nframes, s);
        case 3: return launch<KIND, 3, DB, Scaled>(a, nframes, s);
        case 4: return launch<KIND, 4, DB, Scaled>(a, nframes, s);
    }
    return hipErrorInvalidValue;
}

template <int KIND, bool Scaled>
int launch_by_size(const NarrowArgs& a, int step, int dst_bytes, int nframes, hipStream_t s) {
    if (dst_bytes == 1) return launch_by_step<KIND, 1, Scaled>(a, step, nframes, s);
    if (dst_bytes == 2) return launch_by_step<KIND, 2, Scaled>(a, step, nframes, s);
    return hipErrorInvalidValue;
}

template <bool Scaled>
int launch_by_kind(const NarrowArgs& a, int in_kind, int step, int dst_bytes, int nframes, hipStream_t s) {
    switch (in_kind) {
        case 0: return launch_by_size<0, Scaled>(a, step, dst_bytes, nframes, s);
        case kSampleHalf: return launch_by_size<kSampleHalf, Scaled>(a, step, dst_bytes, nframes, s);
        case kSampleBFloat16: return launch_by_size<kSampleBFloat16, Scaled>(a, step, dst_bytes, nframes, s);
    }
    return hipErrorInvalidValue;  // (no kernel for this shape: an error, never a silent skip)
}

// ---- 10:10:10:2 words (kernels.h NarrowFieldArgs; the row function: narrow_fields_rows.h) ----
// Row blockIdx.x * 4 + wave of frame blockIdx.y.
template <int KIND, bool Scaled>
__global__ __launch_bounds__(256) void narrow_fields_kernel(const NarrowFieldArgs a) {
    const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row < a.rows) narrow::narrow_fields_row<KIND, Scaled>(a, blockIdx.y, row, threadIdx.x & 63u);
}

// ---- v210 blocks (kernels.h NarrowV210Args; the row functions: narrow_v210_rows.h, v210_rows.h; the exchange: v210_exchange.h) ----
// Row blockIdx.x * 4 + wave of frame blockIdx.y (the wave's number through a scalar register: the row's addresses are wave-uniform).
template <int KIND, bool Scaled>
__global__ __launch_bounds__(256) void narrow_v210_kernel(const NarrowV210Args a) {
    const uint32_t row = blockIdx.x * 4 + static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
    if (row >= a.rows) return;
    const uint32_t lane = threadIdx.x & 63u, paired = v210::paired_blocks(a), blocks = v210::row_blocks(a);
    const v210::RowOf r = v210::row_of(a, blockIdx.y, row);
    for (uint32_t b = lane; b < paired; b += 64) {
        v210::LaneState s;
        uint32_t y[3];
        v210::narrow_pair_begin<KIND, Scaled>(a, r, b, y, s);  // (codes, not samples, cross the lanes)
        v210::pack_pair_end(a, r, b, y, s, v210::from_partner(s.send));
    }
    for (uint32_t b = paired + lane; b < blocks; b += 64) v210::narrow_tail<KIND, Scaled>(a, r, b);
}

template <int KIND, bool Scaled>
int launch_fields(const NarrowFieldArgs& a, const dim3& grid, hipStream_t s) {
    hipLaunchKernelGGL((narrow_fields_kernel<KIND, Scaled>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}
template <int KIND, bool Scaled>
int launch_v210(const NarrowV210Args& a, const dim3& grid, hipStream_t s) {
    hipLaunchKernelGGL((narrow_v210_kernel<KIND, Scaled>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace

int launch_narrow_fields(const NarrowFieldArgs& a, int in_kind, int nframes, void* stream, bool scaled) {
    if (in_kind != 0 && in_kind != kSampleHalf && in_kind != kSampleBFloat16) return hipErrorInvalidValue;  // (never a silent skip)
    if (nframes <= 0 || a.rows == 0 || a.width == 0) return hipSuccess;
    if ((a.unit != 16 && a.unit != 4) || a.vec_pixels > a.width || a.vec_pixels % 8u) return hipErrorInvalidValue;  // (a word is the smallest access)
    for (int c = 0; c < 3; ++c)
        if (a.offset[c] > 22u || !a.plane[c]) return hipErrorInvalidValue;
    if (!a.packed) return hipErrorInvalidValue;
    const dim3 grid((a.rows + 3) / 4, static_cast<uint32_t>(nframes));
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (in_kind) {
        case 0: return scaled ? launch_fields<0, true>(a, grid, s) : launch_fields<0, false>(a, grid, s);
        case kSampleHalf: return scaled ? launch_fields<kSampleHalf, true>(a, grid, s) : launch_fields<kSampleHalf, false>(a, grid, s);
        default: return scaled ? launch_fields<kSampleBFloat16, true>(a, grid, s) : launch_fields<kSampleBFloat16, false>(a, grid, s);
    }
}

int launch_narrow_v210(const NarrowV210Args& a, int in_kind, int nframes, void* stream, bool scaled) {
    if (in_kind != 0 && in_kind != kSampleHalf && in_kind != kSampleBFloat16) return hipErrorInvalidValue;  // (never a silent skip)
    if (nframes <= 0 || a.rows == 0 || a.width == 0) return hipSuccess;
    if ((a.unit != 16 && a.unit != 4) || a.whole_blocks != a.width / 6 || (a.width & 1u)) return hipErrorInvalidValue;
    if (!a.blocks || !a.plane[0] || !a.plane[1] || !a.plane[2]) return hipErrorInvalidValue;
    const dim3 grid((a.rows + 3) / 4, static_cast<uint32_t>(nframes));
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (in_kind) {
        case 0: return scaled ? launch_v210<0, true>(a, grid, s) : launch_v210<0, false>(a, grid, s);
        case kSampleHalf: return scaled ? launch_v210<kSampleHalf, true>(a, grid, s) : launch_v210<kSampleHalf, false>(a, grid, s);
        default: return scaled ? launch_v210<kSampleBFloat16, true>(a, grid, s) : launch_v210<kSampleBFloat16, false>(a, grid, s);
    }
}

int launch_narrow_samples(const NarrowArgs& a, int in_kind, int step, int dst_bytes, int nframes, void* stream, bool scaled) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a.ngroups > 4 || (dst_bytes != 1 && dst_bytes != 2)) return hipErrorInvalidValue;
    // the peak of a byte is 255 (round_sample_u8 saturates there); a word's lies in 511 .. 65535 and is 2^bits - 1
    if (dst_bytes == 1 ? a.peak != 255.f : !(a.peak >= 511.f && a.peak <= 65535.f)) return hipErrorInvalidValue;
    for (int k = 0; k < a.ngroups; ++k) {
        const NarrowGroup& g = a.g[k];
        const uint32_t lane_pixels = 16u / static_cast<uint32_t>(dst_bytes);
        if (g.vec_pixels > g.width || g.vec_pixels % lane_pixels || (g.vec_pixels && g.unit != 16 && g.unit != 4)) return hipErrorInvalidValue;
        for (int c = 0; c < 4; ++c) {
            if (g.vec_pixels && c < step && !g.plane[c]) return hipErrorInvalidValue;  // (vectors store every channel of a pixel)
            if (dst_bytes == 1 ? g.shift[c] != 0 : (static_cast<uint32_t>(a.peak) << g.shift[c]) > 65535u) return hipErrorInvalidValue;
        }
    }
    return scaled ? launch_by_kind<true>(a, in_kind, step, dst_bytes, nframes, s) : launch_by_kind<false>(a, in_kind, step, dst_bytes, nframes, s);
}

}  // namespace jinc
