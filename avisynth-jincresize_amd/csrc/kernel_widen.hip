// kernel_widen.hip -- integer samples -> the dense fp32 / binary16 / bfloat16 planes the float filters' kernels read, in front of
// jinc_filter_process_device_widened (dispatch.cpp enqueue_widened): the planes of a decoder's NV12 / P010 / Y210 surface, packed
// 8-bit RGB(A) or planar integer frames become the stand-ins of a float or half filter.  A split (kernel_interleave.hip) that WIDENS:
// it picks channel c out of N interleaved samples, drops the bits below and above the sample, (raw >> shift[c]) & mask, and stores
// the value converted exactly -- v_cvt_f32_ubyte0..3 on the bytes of a loaded dword, v_cvt_f32_u32 on words, v_cvt_f16_f32 on top
// for binary16 planes (values up to 2047 only), the upper half of the fp32 bits for bfloat16 planes (bytes only).  No arithmetic beyond that: what the resampling kernels compute from these planes is
// what they compute from any float plane holding the same values.
//
// Shape, after split_samples_kernel: ONE launch covers every channel group and frame of a call (grid = row blocks x frames x groups;
// the groups travel as kernel arguments, kernels.h WidenArgs), a wave owns a row, its lanes walk along it, and no access costs a
// division or a modulo.  The row function is widen_rows.h: a lane owns 16 / SB whole pixels per step, N 16-byte loads (dwords where
// the group's alignment allows no more) and OB / SB 16-byte stores per plane; tails, unaligned groups and the last pixel of a group
// with a channel missing move sample by sample.  The source is read only.
// The scaled forms (jinc_filter_process_device_widened_scaled) are the same kernel with one v_mul_f32 and one v_add_f32 per sample
// behind the conversion (scale[c], offset[c] of the group's channel in scalar registers; -ffp-contract=off keeps them apart) and, for
// 16-bit planes, the round-to-nearest-even conversions the resampling kernels store with: words go into bfloat16 planes there.
//
// Two more sources whose samples neither a step nor a shift addresses (jinc_filter_process_device_widened_packed10 / _v210;
// dispatch.cpp enqueue_widened_packed10 / enqueue_widened_v210): 10:10:10:2 words -- Y410, R10G10B10A2 and kin, three 10-bit fields
// in one 32-bit word per pixel -- and v210 blocks, six pixels of 10-bit 4:2:2 in 16 bytes.  widen_fields_kernel has the shape of
// unpack_fields_kernel and widen_v210_kernel that of unpack_v210_kernel (kernel_interleave.hip): one launch over every row and
// frame of a slice, grid = row blocks x frames, a wave owns a row; they store the field values converted instead of 16-bit
// integers.  The row functions are widen_fields_rows.h and widen_v210_rows.h; the exchange between the two lanes of a block pair
// is v210_exchange.h's, RAW samples in front of the conversion.  Plain C++ and that one DPP builtin: no assembly, no scratch.
// Their scaled forms (jinc_filter_process_device_widened_packed10_scaled / _widened_v210_scaled; kernels.h WidenFieldArgs /
// WidenV210Args) are the same kernels with widen_rows.h's scaled_value behind the conversion and its round-to-nearest-even pair
// conversions for 16-bit planes, bfloat16 among them; the pairs of the three planes are kernel arguments in scalar registers, and
// the v210 lane that stores a pair's chroma row selects between plane 1's and plane 2's pair by the parity of its block.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kernels.h"
#include "v210_exchange.h"
#include "widen_fields_rows.h"
#include "widen_rows.h"
#include "widen_v210_rows.h"

namespace jinc {
namespace {

// Row blockIdx.x * 4 + wave of frame blockIdx.y of group blockIdx.z.
template <int SB, int N, int OB, int KIND, bool Scaled>
__global__ __launch_bounds__(256) void widen_samples_kernel(const WidenArgs a) {
    const WidenGroup& g = a.g[blockIdx.z];
    const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row < g.rows) widen::widen_row<SB, N, OB, KIND, Scaled>(g, a.mask, blockIdx.y, row, threadIdx.x & 63u);
}

template <int SB, int N, int OB, int KIND, bool Scaled>
int launch(const WidenArgs& a, int nframes, hipStream_t s) {
    uint32_t rows = 0;
    for (int k = 0; k < a.ngroups; ++k) rows = a.g[k].rows > rows ? a.g[k].rows : rows;
    if (a.ngroups <= 0 || nframes <= 0 || rows == 0) return hipSuccess;
    const dim3 grid((rows + 3) / 4, static_cast<uint32_t>(nframes), static_cast<uint32_t>(a.ngroups));
    hipLaunchKernelGGL((widen_samples_kernel<SB, N, OB, KIND, Scaled>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

template <int SB, int OB, int KIND = 0, bool Scaled = false>
int launch_by_step(const WidenArgs& a, int step, int nframes, hipStream_t s) {
    switch (step) {
        case 1: return launch<SB, 1, OB, KIND, Scaled>(a, nframes, s);
        case 2: return launch<SB, 2, OB, KIND, Scaled>(a, nframes, s);
        case 3: return launch<SB, 3, OB, KIND, Scaled>(a, nframes, s);
        case 4: return launch<SB, 4, OB, KIND, Scaled>(a, nframes, s);
    }
    return hipErrorInvalidValue;
}

// ---- 10:10:10:2 words (kernels.h FieldArgs / WidenFieldArgs; the row function: widen_fields_rows.h) ----
// Row blockIdx.x * 4 + wave of frame blockIdx.y.  The unscaled forms take FieldArgs as it is; the scaled forms (KIND: the plane's
// type, bfloat16 among them) take the record with the three pairs behind it.
template <int OB, int KIND, bool Scaled>
__global__ __launch_bounds__(256) void widen_fields_kernel(const std::conditional_t<Scaled, WidenFieldArgs, FieldArgs> a) {
    const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row < a.rows) widen::widen_fields_row<OB, KIND, Scaled>(a, blockIdx.y, row, threadIdx.x & 63u);
}

// ---- v210 blocks (kernels.h V210Args / WidenV210Args; the row functions: widen_v210_rows.h) ----
// Row blockIdx.x * 4 + wave of frame blockIdx.y (the wave's number through a scalar register: the row's addresses are wave-uniform).
template <int OB, int KIND, bool Scaled>
__global__ __launch_bounds__(256) void widen_v210_kernel(const std::conditional_t<Scaled, WidenV210Args, V210Args> a) {
    const uint32_t row = blockIdx.x * 4 + static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
    if (row >= a.rows) return;
    const uint32_t lane = threadIdx.x & 63u, paired = v210::paired_blocks(a), blocks = v210::row_blocks(a);
    const v210::RowOf r = v210::row_of(a, blockIdx.y, row);
    for (uint32_t b = lane; b < paired; b += 64) {
        v210::LaneState s;
        v210::widen_pair_begin<OB, KIND, Scaled>(a, r, b, s);
        v210::widen_pair_end<OB, KIND, Scaled>(a, r, b, s, v210::from_partner(s.send));  // (RAW samples cross the lanes; scale and convert behind)
    }
    for (uint32_t b = paired + lane; b < blocks; b += 64) v210::widen_tail<OB, KIND, Scaled>(a, r, b);
}

template <int OB, int KIND, bool Scaled>
int launch_fields(const WidenFieldArgs& a, const dim3& grid, hipStream_t s) {
    if constexpr (Scaled) hipLaunchKernelGGL((widen_fields_kernel<OB, KIND, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((widen_fields_kernel<OB, KIND, false>), grid, dim3(256), 0, s, static_cast<const FieldArgs&>(a));
    return hipGetLastError();
}
template <int OB, int KIND, bool Scaled>
int launch_v210(const WidenV210Args& a, const dim3& grid, hipStream_t s) {
    if constexpr (Scaled) hipLaunchKernelGGL((widen_v210_kernel<OB, KIND, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((widen_v210_kernel<OB, KIND, false>), grid, dim3(256), 0, s, static_cast<const V210Args&>(a));
    return hipGetLastError();
}

}  // namespace

int launch_widen_fields(const WidenFieldArgs& a, int out_kind, int nframes, void* stream, bool scaled) {
    if (out_kind != 0 && out_kind != kSampleHalf && out_kind != kSampleBFloat16) return hipErrorInvalidValue;  // (never a silent skip)
    if (out_kind == kSampleBFloat16 && !scaled) return hipErrorInvalidValue;  // (ten bits are not exact in bfloat16)
    if (nframes <= 0 || a.rows == 0 || a.width == 0) return hipSuccess;
    if ((a.unit != 16 && a.unit != 4) || a.vec_pixels > a.width || a.vec_pixels % 8u) return hipErrorInvalidValue;  // (a word is the smallest access)
    for (int c = 0; c < 3; ++c)
        if (a.offset[c] > 22u) return hipErrorInvalidValue;
    const dim3 grid((a.rows + 3) / 4, static_cast<uint32_t>(nframes));
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (out_kind) {
        case 0: return scaled ? launch_fields<4, 0, true>(a, grid, s) : launch_fields<4, 0, false>(a, grid, s);
        case kSampleHalf: return scaled ? launch_fields<2, kSampleHalf, true>(a, grid, s) : launch_fields<2, 0, false>(a, grid, s);
        default: return launch_fields<2, kSampleBFloat16, true>(a, grid, s);
    }
}

int launch_widen_v210(const WidenV210Args& a, int out_kind, int nframes, void* stream, bool scaled) {
    if (out_kind != 0 && out_kind != kSampleHalf && out_kind != kSampleBFloat16) return hipErrorInvalidValue;  // (never a silent skip)
    if (out_kind == kSampleBFloat16 && !scaled) return hipErrorInvalidValue;  // (ten bits are not exact in bfloat16)
    if (nframes <= 0 || a.rows == 0 || a.width == 0) return hipSuccess;
    if ((a.unit != 16 && a.unit != 4) || a.whole_blocks != a.width / 6 || (a.width & 1u)) return hipErrorInvalidValue;
    const dim3 grid((a.rows + 3) / 4, static_cast<uint32_t>(nframes));
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (out_kind) {
        case 0: return scaled ? launch_v210<4, 0, true>(a, grid, s) : launch_v210<4, 0, false>(a, grid, s);
        case kSampleHalf: return scaled ? launch_v210<2, kSampleHalf, true>(a, grid, s) : launch_v210<2, 0, false>(a, grid, s);
        default: return launch_v210<2, kSampleBFloat16, true>(a, grid, s);
    }
}

int launch_widen_samples(const WidenArgs& a, int src_bytes, int step, int out_bytes, int out_kind, int nframes, void* stream, bool scaled) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a.ngroups > 4) return hipErrorInvalidValue;
    for (int k = 0; k < a.ngroups; ++k) {
        const WidenGroup& g = a.g[k];
        const uint32_t lane_pixels = 16u / static_cast<uint32_t>(src_bytes == 2 ? 2 : 1);
        if (g.vec_pixels > g.width || g.vec_pixels % lane_pixels || (g.vec_pixels && g.unit != 16 && g.unit != 4)) return hipErrorInvalidValue;
        for (int c = 0; c < 4; ++c)
            if (src_bytes == 1 && g.shift[c]) return hipErrorInvalidValue;  // (a byte takes no shift)
    }
    if (scaled) {  // a defined rounding, no claim of exactness: every depth into every type
        if (a.mask > 0xffffu || (src_bytes == 1 && a.mask != 0xffu)) return hipErrorInvalidValue;
        if (out_kind == kSampleBFloat16) {
            if (out_bytes != 2) return hipErrorInvalidValue;
            if (src_bytes == 1) return launch_by_step<1, 2, kSampleBFloat16, true>(a, step, nframes, s);
            if (src_bytes == 2) return launch_by_step<2, 2, kSampleBFloat16, true>(a, step, nframes, s);
            return hipErrorInvalidValue;
        }
        switch (src_bytes * 8 + out_bytes) {
            case 1 * 8 + 4: return launch_by_step<1, 4, 0, true>(a, step, nframes, s);
            case 1 * 8 + 2: return launch_by_step<1, 2, 0, true>(a, step, nframes, s);
            case 2 * 8 + 4: return launch_by_step<2, 4, 0, true>(a, step, nframes, s);
            case 2 * 8 + 2: return launch_by_step<2, 2, 0, true>(a, step, nframes, s);
        }
        return hipErrorInvalidValue;
    }
    if (out_bytes == 2 && a.mask > 2047u) return hipErrorInvalidValue;  // (not exact in binary16)
    if (out_kind == kSampleBFloat16) {  // bytes only: nine bits are not exact in bfloat16
        if (out_bytes != 2 || src_bytes != 1) return hipErrorInvalidValue;
        return launch_by_step<1, 2, kSampleBFloat16>(a, step, nframes, s);
    }
    switch (src_bytes * 8 + out_bytes) {
        case 1 * 8 + 4: return launch_by_step<1, 4>(a, step, nframes, s);
        case 1 * 8 + 2: return launch_by_step<1, 2>(a, step, nframes, s);
        case 2 * 8 + 4: return launch_by_step<2, 4>(a, step, nframes, s);
        case 2 * 8 + 2: return launch_by_step<2, 2>(a, step, nframes, s);
    }
    return hipErrorInvalidValue;  // (no kernel for this shape: an error, never a silent skip)
}

}  // namespace jinc
