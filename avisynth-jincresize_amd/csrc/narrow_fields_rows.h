// narrow_fields_rows.h -- one lane's share of one row of the pass that narrows a float filter's results into 10:10:10:2 words
// (kernel_narrow.hip narrow_fields_kernel; kernels.h NarrowFieldArgs), as a plain inline function for host and device: a stand-alone
// host program runs exactly this code lane by lane against exactly sized buffers (tests/host_sanitizer/narrow_fields_rows_main.cpp).
// The mirror image of widen_fields_rows.h; the word side is pack_fields_kernel's.
//
// The samples of three dense planes -- fp32 (KIND 0), binary16 (kSampleHalf) or bfloat16 (kSampleBFloat16) -- become one
// little-endian 32-bit word per pixel: (v0 << offset[0]) | (v1 << offset[1]) | (v2 << offset[2]) | fill with
// v_c = lrintf(clamp(r_c, 0, 1023)), r_c the plane's sample widened exactly to fp32 -- or, in the scaled form,
// fl32(fl32(r_c * value_scale[c]) + value_offset[c]): two fp32 roundings, never an FMA.  Round half to even; a NaN, -inf and -0 become
// 0, +inf becomes 1023.  The conversion is narrow_rows.h's (word_pair_of in the vectors, word_of in the tail) with peak 1023.
//
// A lane owns 8 pixels per step, as in pack_fields_kernel: per plane (input bytes / 2) adjacent 16-byte loads from the
// 256-byte-aligned stand-ins (consecutive lanes, consecutive addresses) and two adjacent 16-byte stores of words (eight dwords where
// base, pitch or frame stride is a multiple of 4 only) -- a wave's trip stores one piece of 2 KiB.  Offsets, fill, scale and offset
// are the same in every lane.  The rest of the row goes word by word under the width guard.  Every word is built in registers and
// stored whole; nothing beyond `width` samples is read from a plane, nothing beyond `width` words is stored; the words are never
// read, the planes never written.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernels.h"
#include "narrow_rows.h"

namespace jinc {
namespace narrow {

constexpr float kFieldPeak = 1023.f;  // ten bits

// Lane `lane` of the wave that owns row `row` of frame `frame`.
template <int KIND, bool Scaled>
JINC_NARROW_HD void narrow_fields_row(const NarrowFieldArgs& a, uint32_t frame, uint32_t row, uint32_t lane) {
    static_assert(KIND == 0 || KIND == kSampleHalf || KIND == kSampleBFloat16, "no such form");
    constexpr int IB = input_bytes(KIND);
    constexpr int kLoads = IB / 2;  // 16-byte vectors of 8 samples of one plane
    char* __restrict__ packed = a.packed + frame * a.packed_frame_stride + static_cast<size_t>(row) * a.packed_pitch;
    const size_t dense = frame * a.plane_frame_stride + static_cast<size_t>(row) * a.plane_pitch;
    for (uint32_t x = lane * 8; x < a.vec_pixels; x += 64 * 8) {
        uint32_t w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = a.fill;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint32_t in[4 * kLoads];
            const char* plane = a.plane[c] + dense + static_cast<size_t>(x) * IB;
            float sc = 1.f, of = 0.f;
            if constexpr (Scaled) sc = a.value_scale[c], of = a.value_offset[c];
#pragma unroll
            for (int k = 0; k < kLoads; ++k) load16(plane + 16 * k, in + 4 * k);
            const uint32_t sh = a.offset[c];
#pragma unroll
            for (int p = 0; p < 8; p += 2) {  // (either half is at most 1023: a field stays inside its bits)
                const uint32_t pair = word_pair_of(result_at<KIND, Scaled>(in, p, sc, of), result_at<KIND, Scaled>(in, p + 1, sc, of), kFieldPeak);
                w[p] |= (pair & 0xffffu) << sh;
                w[p + 1] |= (pair >> 16) << sh;
            }
        }
        store_pixels<2>(packed + static_cast<size_t>(x) * 4, a.unit, w);
    }
    for (uint32_t x = a.vec_pixels + lane; x < a.width; x += 64) {
        uint32_t w = a.fill;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float r = value_in_row<KIND>(a.plane[c] + dense, x);
            if constexpr (Scaled) r = scaled_value(r, a.value_scale[c], a.value_offset[c]);
            w |= word_of(r, kFieldPeak) << a.offset[c];
        }
        reinterpret_cast<uint32_t*>(packed)[x] = w;
    }
}

}  // namespace narrow
}  // namespace jinc
