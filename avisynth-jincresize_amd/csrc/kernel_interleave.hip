// kernel_interleave.hip -- interleaved samples <-> dense planes around jinc_filter_process_device_strided (dispatch.cpp enqueue_strided): the chroma
// plane of NV12 / P010 / P016 (U and V sample by sample) and packed RGB(A) are SPLIT into the dense planes the resampling kernels
// read, and the dense results are MERGED into the caller's interleaved destination.  Bytes in, the same bytes out: nothing here
// looks at a sample's value, so one instantiation per sample size serves integer, fp32 and binary16 planes.
//
// Shape, after kernel_blit.hip: ONE launch per direction covers every channel group and frame of a call (grid = row blocks x frames
// x groups; the groups travel as kernel arguments, kernels.h InterleaveArgs), a wave owns a row, its lanes walk along it, and no
// access costs a division or a modulo.  A lane owns 16 / B whole pixels per step: N vectors of 16 bytes on the interleaved side
// (consecutive lanes, consecutive addresses) and one vector of 16 bytes per dense plane, rearranged in registers with shifts whose
// amounts are compile-time constants.  Every interleaved byte of those pixels is read once (split) or written once (merge).
// Sample-sized accesses take what is left: a row's tail, groups whose base or pitch is not a multiple of 4 bytes, and the merge of
// an incomplete group -- there only the given channels' samples are stored, the bytes between them are not touched.
//
// SHIFTED forms (jinc_filter_process_device_shifted; 16-bit samples only): P010 / P012 / Y210 keep a sample in the HIGH bits of its
// 16-bit word.  The split then stores raw >> shift, the merge (result << shift) & 0xffff -- padding bits are dropped on the way in
// and written as zeros on the way out.  The shift is a kernel argument per channel (wave-uniform: shift and mask stay in scalar
// registers) and is applied on the dense side to whole dwords of two samples, (w >> s) & mask or (w << s) & mask, two vector
// instructions per dword, in all three access classes; tails and incomplete groups shift sample by sample.  Shifted is a template
// parameter: the unshifted instantiations hold no trace of it.  Only the shifted forms have N = 1, a dense plane to a dense plane
// (the luma of P010): a lane owns 16 contiguous bytes on both sides, a wave's access is 1 KiB in one piece.
//
// FIELD forms (jinc_filter_process_device_packed10): Y410 and R10G10B10A2-style frames keep three 10-bit samples in ONE 32-bit word
// per pixel, at bit offsets that are no byte offsets.  unpack_fields_kernel stores (word >> offset[c]) & 1023 into three dense 16-bit
// planes, pack_fields_kernel builds (r0 << o0) | (r1 << o1) | (r2 << o2) | fill in registers and stores the whole word once; it never
// reads the destination.  Same shape: grid = row blocks x frames, a wave owns a row.  A lane owns 8 pixels per step: two 16-byte
// accesses on the word side (consecutive lanes at consecutive 32-byte pieces, 2 KiB per wave in one piece; eight dwords where base,
// pitch or frame stride is a multiple of 4 only) and one 16-byte access per dense plane.  The offsets and the fill are kernel
// arguments: wave-uniform, in scalar registers.  The rest of a row moves word by word.
//
// V210 forms (jinc_filter_process_device_v210): 10-bit 4:2:2 in 16-byte blocks of six pixels, twelve fields in four words in an
// order that repeats only every 128 bits.  unpack_v210_kernel fills the three dense planes of YUV422P10 from the blocks,
// pack_v210_kernel builds the blocks in registers (bits 30 - 31 and the unused fields of a partial block are zeros by construction)
// and stores them whole; it never reads the destination.  Same shape: grid = row blocks x frames, a wave owns a row.  A lane owns
// ONE block per trip, so a wave's trip is 64 consecutive blocks: 1 KiB in one piece on the block side (one 16-byte access per
// lane; four dwords where base, pitch or frame stride is a multiple of 4 only) and 768 bytes in one piece on the luma plane (one
// 12-byte access per lane, 4-byte aligned).  Chroma: a block holds 3 samples of each plane, 6 bytes -- no aligned access -- so
// lanes l and l ^ 1 swap three samples through one cross-lane move of two dwords (DPP, no LDS) and then the even lane moves the
// pair's 6 Cb samples and the odd lane its 6 Cr samples, 12 bytes each.  Every block byte is read once or written once; block and
// sample indices come from the lane number by additions, shifts and multiplications by constants.  What the pairs leave over
// (the odd whole block, the partial last block) moves sample by sample under a width guard.  The row functions are v210_rows.h:
// plain inline functions that a host program runs lane by lane against exactly sized buffers.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "v210_exchange.h"
#include "v210_rows.h"

namespace jinc {
namespace {

template <int B> struct SampleOf;
template <> struct SampleOf<1> { using type = uint8_t; };
template <> struct SampleOf<2> { using type = uint16_t; };
template <> struct SampleOf<4> { using type = uint32_t; };

// Sample i of a run of B-byte samples held in dwords (i is a constant once the loops around the calls are unrolled).
template <int B>
__device__ __forceinline__ uint32_t get_sample(const uint32_t* w, int i) {
    if constexpr (B == 4) return w[i];
    else if constexpr (B == 2) return (w[i >> 1] >> (16 * (i & 1))) & 0xffffu;
    else return (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
}
template <int B>
__device__ __forceinline__ void put_sample(uint32_t* w, int i, uint32_t v) {  // (w starts as zeros)
    if constexpr (B == 4) w[i] = v;
    else if constexpr (B == 2) w[i >> 1] |= v << (16 * (i & 1));
    else w[i >> 2] |= v << (8 * (i & 3));
}

// 16 N bytes of whole pixels: N 16-byte accesses where the group allows them, else 4 N dwords.
template <int N>
__device__ __forceinline__ void load_packed(const char* p, uint32_t unit, uint32_t* w) {
    if (unit == 16) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const uint4 v = *reinterpret_cast<const uint4*>(p + 16 * k);
            w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4 * N; ++k) w[k] = *reinterpret_cast<const uint32_t*>(p + 4 * k);
    }
}
template <int N>
__device__ __forceinline__ void store_packed(char* p, uint32_t unit, const uint32_t* w) {
    if (unit == 16) {
#pragma unroll
        for (int k = 0; k < N; ++k) *reinterpret_cast<uint4*>(p + 16 * k) = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4 * N; ++k) *reinterpret_cast<uint32_t*>(p + 4 * k) = w[k];
    }
}

// Two 16-bit samples in a dword, both shifted by s (0 .. 15): what crosses from one half into the other is masked away.
__device__ __forceinline__ uint32_t down_mask(uint32_t s) { return (0xffffu >> s) * 0x10001u; }
__device__ __forceinline__ uint32_t up_mask(uint32_t s) { return ((0xffffu << s) & 0xffffu) * 0x10001u; }

// Row blockIdx.x * 4 + wave of frame blockIdx.y of group blockIdx.z.
template <int B, int N, bool Shifted = false>
__global__ __launch_bounds__(256) void split_samples_kernel(const InterleaveArgs a) {
    static_assert(!Shifted || B == 2, "shifted samples are 16-bit words");
    static_assert(Shifted || N > 1, "a dense plane without a shift needs no pass");
    using T = typename SampleOf<B>::type;
    constexpr uint32_t P = 16 / B;  // pixels a lane owns per step
    const InterleaveGroup& g = a.g[blockIdx.z];
    const uint32_t lane = threadIdx.x & 63u, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= g.rows) return;
    const char* __restrict__ packed = g.packed + blockIdx.y * g.packed_frame_stride + static_cast<size_t>(row) * g.packed_pitch;
    const size_t dense = blockIdx.y * g.plane_frame_stride + static_cast<size_t>(row) * g.plane_pitch;
    uint32_t sh[N], mask[N];  // (Shifted only; the same in every lane)
    if constexpr (Shifted) {
#pragma unroll
        for (int c = 0; c < N; ++c) sh[c] = g.shift[c], mask[c] = down_mask(sh[c]);
    }
    for (uint32_t x = lane * P; x < g.vec_pixels; x += 64 * P) {
        uint32_t in[4 * N];
        load_packed<N>(packed + static_cast<size_t>(x) * (N * B), g.unit, in);
#pragma unroll
        for (int c = 0; c < N; ++c) {
            if (!g.plane[c]) continue;
            uint32_t out[4] = {0u, 0u, 0u, 0u};
            if constexpr (N == 1) {
                out[0] = in[0], out[1] = in[1], out[2] = in[2], out[3] = in[3];
            } else {
#pragma unroll
                for (int p = 0; p < static_cast<int>(P); ++p) put_sample<B>(out, p, get_sample<B>(in, p * N + c));
            }
            if constexpr (Shifted) {
#pragma unroll
                for (int k = 0; k < 4; ++k) out[k] = (out[k] >> sh[c]) & mask[c];
            }
            *reinterpret_cast<uint4*>(g.plane[c] + dense + static_cast<size_t>(x) * B) = make_uint4(out[0], out[1], out[2], out[3]);
        }
    }
    for (uint32_t x = g.vec_pixels + lane; x < g.width; x += 64) {
#pragma unroll
        for (int c = 0; c < N; ++c) {
            if (!g.plane[c]) continue;
            T v = reinterpret_cast<const T*>(packed)[static_cast<size_t>(x) * N + c];
            if constexpr (Shifted) v = static_cast<T>(v >> sh[c]);
            reinterpret_cast<T*>(g.plane[c] + dense)[x] = v;
        }
    }
}

template <int B, int N, bool Shifted = false>
__global__ __launch_bounds__(256) void merge_samples_kernel(const InterleaveArgs a) {
    static_assert(!Shifted || B == 2, "shifted samples are 16-bit words");
    static_assert(Shifted || N > 1, "a dense plane without a shift needs no pass");
    using T = typename SampleOf<B>::type;
    constexpr uint32_t P = 16 / B;
    const InterleaveGroup& g = a.g[blockIdx.z];
    const uint32_t lane = threadIdx.x & 63u, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= g.rows) return;
    char* __restrict__ packed = g.packed + blockIdx.y * g.packed_frame_stride + static_cast<size_t>(row) * g.packed_pitch;
    const size_t dense = blockIdx.y * g.plane_frame_stride + static_cast<size_t>(row) * g.plane_pitch;
    uint32_t sh[N], mask[N];  // (Shifted only; the same in every lane)
    if constexpr (Shifted) {
#pragma unroll
        for (int c = 0; c < N; ++c) sh[c] = g.shift[c], mask[c] = up_mask(sh[c]);
    }
    for (uint32_t x = lane * P; x < g.vec_pixels; x += 64 * P) {  // (complete groups only: every byte of these pixels is a given sample)
        uint32_t out[4 * N];
#pragma unroll
        for (int k = 0; k < 4 * N; ++k) out[k] = 0u;
#pragma unroll
        for (int c = 0; c < N; ++c) {
            const uint4 v = *reinterpret_cast<const uint4*>(g.plane[c] + dense + static_cast<size_t>(x) * B);
            uint32_t in[4] = {v.x, v.y, v.z, v.w};
            if constexpr (Shifted) {
#pragma unroll
                for (int k = 0; k < 4; ++k) in[k] = (in[k] << sh[c]) & mask[c];
            }
            if constexpr (N == 1) {
                out[0] = in[0], out[1] = in[1], out[2] = in[2], out[3] = in[3];
            } else {
#pragma unroll
                for (int p = 0; p < static_cast<int>(P); ++p) put_sample<B>(out, p * N + c, get_sample<B>(in, p));
            }
        }
        store_packed<N>(packed + static_cast<size_t>(x) * (N * B), g.unit, out);
    }
    for (uint32_t x = g.vec_pixels + lane; x < g.width; x += 64) {
#pragma unroll
        for (int c = 0; c < N; ++c) {
            if (!g.plane[c]) continue;
            T v = reinterpret_cast<const T*>(g.plane[c] + dense)[x];
            if constexpr (Shifted) v = static_cast<T>(static_cast<uint32_t>(v) << sh[c]);  // (the store keeps the low 16 bits)
            reinterpret_cast<T*>(packed)[static_cast<size_t>(x) * N + c] = v;
        }
    }
}

template <bool Merge, int B, int N, bool Shifted = false>
int launch(const InterleaveArgs& a, int nframes, hipStream_t s) {
    uint32_t rows = 0;
    for (int k = 0; k < a.ngroups; ++k) rows = a.g[k].rows > rows ? a.g[k].rows : rows;
    if (a.ngroups <= 0 || nframes <= 0 || rows == 0) return hipSuccess;
    const dim3 grid((rows + 3) / 4, static_cast<uint32_t>(nframes), static_cast<uint32_t>(a.ngroups));
    if constexpr (Merge) hipLaunchKernelGGL((merge_samples_kernel<B, N, Shifted>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((split_samples_kernel<B, N, Shifted>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

template <bool Merge>
int launch_by_shape(const InterleaveArgs& a, int sample_bytes, int step, int nframes, void* stream, bool* took_shifted) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    bool shifted = false;  // one shifted channel makes the launch a shifted one (its other channels shift by 0)
    for (int k = 0; k < a.ngroups; ++k)
        for (int c = 0; c < 4; ++c) shifted |= a.g[k].shift[c] != 0;
    if (took_shifted) *took_shifted = shifted;
    if (shifted) {
        if (sample_bytes != 2) return hipErrorInvalidValue;
        switch (step) {
            case 1: return launch<Merge, 2, 1, true>(a, nframes, s);
            case 2: return launch<Merge, 2, 2, true>(a, nframes, s);
            case 3: return launch<Merge, 2, 3, true>(a, nframes, s);
            case 4: return launch<Merge, 2, 4, true>(a, nframes, s);
        }
        return hipErrorInvalidValue;
    }
    switch (sample_bytes * 8 + step) {
        case 1 * 8 + 2: return launch<Merge, 1, 2>(a, nframes, s);
        case 1 * 8 + 3: return launch<Merge, 1, 3>(a, nframes, s);
        case 1 * 8 + 4: return launch<Merge, 1, 4>(a, nframes, s);
        case 2 * 8 + 2: return launch<Merge, 2, 2>(a, nframes, s);
        case 2 * 8 + 3: return launch<Merge, 2, 3>(a, nframes, s);
        case 2 * 8 + 4: return launch<Merge, 2, 4>(a, nframes, s);
        case 4 * 8 + 2: return launch<Merge, 4, 2>(a, nframes, s);
        case 4 * 8 + 3: return launch<Merge, 4, 3>(a, nframes, s);
        case 4 * 8 + 4: return launch<Merge, 4, 4>(a, nframes, s);
    }
    return hipErrorInvalidValue;  // (no kernel for this shape: an error, never a silent skip)
}

// ---- 10:10:10:2 words (kernels.h FieldArgs) ----
// 16 bytes as ONE access (a vector type of the compiler's: the access is not taken apart into its elements).
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__host__ __device__ __forceinline__ void load16(const char* p, uint32_t* w) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(p);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
}
__host__ __device__ __forceinline__ void store16(char* p, const uint32_t* w) {
    u32x4 v;
    v.x = w[0], v.y = w[1], v.z = w[2], v.w = w[3];
    *reinterpret_cast<u32x4*>(p) = v;
}
// The 8 words of a lane's pixels: two 16-byte accesses, or eight dwords.
__host__ __device__ __forceinline__ void load_words(const char* p, uint32_t unit, uint32_t* w) {
    if (unit == 16) {
        load16(p, w), load16(p + 16, w + 4);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = *reinterpret_cast<const uint32_t*>(p + 4 * k);
    }
}
__host__ __device__ __forceinline__ void store_words(char* p, uint32_t unit, const uint32_t* w) {
    if (unit == 16) {
        store16(p, w), store16(p + 16, w + 4);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) *reinterpret_cast<uint32_t*>(p + 4 * k) = w[k];
    }
}

// One lane's share of one row.  __host__ too: the index arithmetic can be run lane by lane on the CPU against exactly sized buffers.
__host__ __device__ inline void unpack_fields_row(const FieldArgs& a, uint32_t frame, uint32_t row, uint32_t lane) {
    const char* __restrict__ packed = a.packed + frame * a.packed_frame_stride + static_cast<size_t>(row) * a.packed_pitch;
    const size_t dense = frame * a.plane_frame_stride + static_cast<size_t>(row) * a.plane_pitch;
    for (uint32_t x = lane * 8; x < a.vec_pixels; x += 64 * 8) {
        uint32_t w[8];
        load_words(packed + static_cast<size_t>(x) * 4, a.unit, w);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint32_t out[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) out[k] = ((w[2 * k] >> a.offset[c]) & 1023u) | (((w[2 * k + 1] >> a.offset[c]) & 1023u) << 16);
            store16(a.plane[c] + dense + static_cast<size_t>(x) * 2, out);
        }
    }
    for (uint32_t x = a.vec_pixels + lane; x < a.width; x += 64) {
        const uint32_t w = reinterpret_cast<const uint32_t*>(packed)[x];
#pragma unroll
        for (int c = 0; c < 3; ++c) reinterpret_cast<uint16_t*>(a.plane[c] + dense)[x] = static_cast<uint16_t>((w >> a.offset[c]) & 1023u);
    }
}

__host__ __device__ inline void pack_fields_row(const FieldArgs& a, uint32_t frame, uint32_t row, uint32_t lane) {
    char* __restrict__ packed = a.packed + frame * a.packed_frame_stride + static_cast<size_t>(row) * a.packed_pitch;
    const size_t dense = frame * a.plane_frame_stride + static_cast<size_t>(row) * a.plane_pitch;
    for (uint32_t x = lane * 8; x < a.vec_pixels; x += 64 * 8) {
        uint32_t w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = a.fill;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint32_t in[4];
            load16(a.plane[c] + dense + static_cast<size_t>(x) * 2, in);
#pragma unroll
            for (int k = 0; k < 4; ++k) {  // (results are at most 1023; the mask keeps a field inside its bits whatever the plane holds)
                w[2 * k] |= (in[k] & 1023u) << a.offset[c];
                w[2 * k + 1] |= ((in[k] >> 16) & 1023u) << a.offset[c];
            }
        }
        store_words(packed + static_cast<size_t>(x) * 4, a.unit, w);
    }
    for (uint32_t x = a.vec_pixels + lane; x < a.width; x += 64) {
        uint32_t w = a.fill;
#pragma unroll
        for (int c = 0; c < 3; ++c) w |= (static_cast<uint32_t>(reinterpret_cast<const uint16_t*>(a.plane[c] + dense)[x]) & 1023u) << a.offset[c];
        reinterpret_cast<uint32_t*>(packed)[x] = w;
    }
}

// Row blockIdx.x * 4 + wave of frame blockIdx.y.
__global__ __launch_bounds__(256) void unpack_fields_kernel(const FieldArgs a) {
    const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row < a.rows) unpack_fields_row(a, blockIdx.y, row, threadIdx.x & 63u);
}
__global__ __launch_bounds__(256) void pack_fields_kernel(const FieldArgs a) {
    const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row < a.rows) pack_fields_row(a, blockIdx.y, row, threadIdx.x & 63u);
}

template <bool Pack>
int launch_fields(const FieldArgs& a, int nframes, void* stream) {
    if (nframes <= 0 || a.rows == 0 || a.width == 0) return hipSuccess;
    if (a.unit != 16 && a.unit != 4) return hipErrorInvalidValue;  // (no sample-sized form: a word is the smallest access)
    const dim3 grid((a.rows + 3) / 4, static_cast<uint32_t>(nframes));
    if constexpr (Pack) hipLaunchKernelGGL(pack_fields_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
    else hipLaunchKernelGGL(unpack_fields_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError();
}

// ---- v210 blocks (kernels.h V210Args; the row functions: v210_rows.h; the exchange between lanes l and l ^ 1: v210_exchange.h) ----
using v210::from_partner;

// Row blockIdx.x * 4 + wave of frame blockIdx.y (the wave's number through a scalar register: the row's addresses are wave-uniform).
__global__ __launch_bounds__(256) void unpack_v210_kernel(const V210Args a) {
    const uint32_t row = blockIdx.x * 4 + static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
    if (row >= a.rows) return;
    const uint32_t lane = threadIdx.x & 63u, paired = v210::paired_blocks(a), blocks = v210::row_blocks(a);
    const v210::RowOf r = v210::row_of(a, blockIdx.y, row);
    for (uint32_t b = lane; b < paired; b += 64) {
        v210::LaneState s;
        v210::unpack_pair_begin(a, r, b, s);
        v210::unpack_pair_end(a, r, b, s, from_partner(s.send));
    }
    for (uint32_t b = paired + lane; b < blocks; b += 64) v210::unpack_tail(a, r, b);
}
__global__ __launch_bounds__(256) void pack_v210_kernel(const V210Args a) {
    const uint32_t row = blockIdx.x * 4 + static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
    if (row >= a.rows) return;
    const uint32_t lane = threadIdx.x & 63u, paired = v210::paired_blocks(a), blocks = v210::row_blocks(a);
    const v210::RowOf r = v210::row_of(a, blockIdx.y, row);
    for (uint32_t b = lane; b < paired; b += 64) {
        v210::LaneState s;
        uint32_t y[3];
        v210::pack_pair_begin(a, r, b, y, s);
        v210::pack_pair_end(a, r, b, y, s, from_partner(s.send));
    }
    for (uint32_t b = paired + lane; b < blocks; b += 64) v210::pack_tail(a, r, b);
}

template <bool Pack>
int launch_v210(const V210Args& a, int nframes, void* stream) {
    if (nframes <= 0 || a.rows == 0 || a.width == 0) return hipSuccess;
    if ((a.unit != 16 && a.unit != 4) || a.whole_blocks != a.width / 6 || (a.width & 1u)) return hipErrorInvalidValue;
    const dim3 grid((a.rows + 3) / 4, static_cast<uint32_t>(nframes));
    if constexpr (Pack) hipLaunchKernelGGL(pack_v210_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
    else hipLaunchKernelGGL(unpack_v210_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError();
}

}  // namespace

int launch_unpack_v210(const V210Args& a, int nframes, void* stream) { return launch_v210<false>(a, nframes, stream); }

int launch_pack_v210(const V210Args& a, int nframes, void* stream) { return launch_v210<true>(a, nframes, stream); }

int launch_unpack_fields(const FieldArgs& a, int nframes, void* stream) { return launch_fields<false>(a, nframes, stream); }

int launch_pack_fields(const FieldArgs& a, int nframes, void* stream) { return launch_fields<true>(a, nframes, stream); }

int launch_split_samples(const InterleaveArgs& a, int sample_bytes, int step, int nframes, void* stream, bool* shifted) {
    return launch_by_shape<false>(a, sample_bytes, step, nframes, stream, shifted);
}

int launch_merge_samples(const InterleaveArgs& a, int sample_bytes, int step, int nframes, void* stream, bool* shifted) {
    return launch_by_shape<true>(a, sample_bytes, step, nframes, stream, shifted);
}

}  // namespace jinc
