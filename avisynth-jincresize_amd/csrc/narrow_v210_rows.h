// narrow_v210_rows.h -- one lane's share of one row of the pass that narrows a float 4:2:2 filter's results into v210 blocks
// (kernel_narrow.hip narrow_v210_kernel; kernels.h NarrowV210Args), as plain inline functions for host and device: a stand-alone
// host program runs exactly this code lane by lane and trip by trip against exactly sized buffers, with the cross-lane move
// modelled by indexing (tests/host_sanitizer/narrow_v210_rows_main.cpp).  The mirror image of widen_v210_rows.h: the block side, its
// encoding, the walk and the store are v210_rows.h's, unchanged -- pack_pair_end stores the block of a pair's lane.
//
// `width` luma samples and width / 2 samples of each chroma plane per row -- fp32 (KIND 0), binary16 (kSampleHalf) or bfloat16
// (kSampleBFloat16) -- become the twelve 10-bit fields of the row's blocks: lrintf(clamp(r, 0, 1023)) each with r the sample widened
// exactly to fp32, or, in the scaled form, fl32(fl32(r * value_scale[c]) + value_offset[c]) of its plane c (two fp32 roundings,
// never an FMA).  The conversion is narrow_rows.h's with peak 1023.  On the plane side NarrowV210Args is read with samples of
// input_bytes(KIND) bytes; pitches and frame strides stay in bytes.
//
// A lane owns one block per trip and blocks move in PAIRS (lanes l and l ^ 1), as in pack_v210_kernel: each lane loads its 6 luma
// samples side by side -- 24 bytes at an 8-byte aligned address (fp32) or 12 bytes at a 4-byte aligned address (16-bit types),
// contiguous from lane to lane -- and the pair's 6 samples of ONE chroma plane in the same way, Cb in the even lane, Cr in the odd
// one.  Every sample is converted to its 10-bit code IN FRONT of the exchange (narrow_pair_begin): what crosses the lanes are three
// codes in two dwords, as in the integer pass, and pack_pair_end (v210_rows.h) encodes and stores the block whole behind it.  What
// pairs leave over -- the odd whole block of a row with an odd number of them and the row's partial last block -- goes sample by
// sample under the width guards (narrow_tail): nothing beyond `width` (luma) or `width / 2` (chroma) samples is read from a plane,
// and the block is still stored whole, with zeros in the absent fields.  The planes are never written, the blocks never read.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernels.h"
#include "narrow_rows.h"
#include "v210_rows.h"

namespace jinc {
namespace v210 {

typedef uint32_t u32x2_in __attribute__((ext_vector_type(2)));  // 8 bytes as ONE access

// Six samples side by side as three dwords of code pairs: fp32 -- three 8-byte loads at an 8-byte aligned address; 16-bit types --
// three adjacent dwords at a 4-byte aligned address, as load_six.
template <int KIND, bool Scaled>
JINC_V210_HD void load_six_narrowed(const char* p, float scale, float offset, uint32_t d[3]) {
    if constexpr (KIND == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const u32x2_in v = reinterpret_cast<const u32x2_in*>(p)[k];
            const uint32_t in[2] = {v.x, v.y};
            d[k] = narrow::word_pair_of(narrow::result_at<0, Scaled>(in, 0, scale, offset), narrow::result_at<0, Scaled>(in, 1, scale, offset), 1023.f);
        }
    } else {
        uint32_t in[3];
        load_six(p, in);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            d[k] = narrow::word_pair_of(narrow::result_at<KIND, Scaled>(in, 2 * k, scale, offset), narrow::result_at<KIND, Scaled>(in, 2 * k + 1, scale, offset), 1023.f);
    }
}

// Block b < paired_blocks(a).  Loads and converts the block's luma (y, three dwords of code pairs) and the pair's six samples of one
// chroma plane (Cb if b is even, Cr if odd: they lie at sample 3 * (b & ~1)); s.keep: this block's three codes of them, s.send: the
// three of block b ^ 1.  pack_pair_end(a, r, b, y, s, s.send of the lane of block b ^ 1) stores the block.
template <int KIND, bool Scaled>
JINC_V210_HD void narrow_pair_begin(const NarrowV210Args& a, const RowOf& r, uint32_t b, uint32_t y[3], LaneState& s) {
    static_assert(KIND == 0 || KIND == kSampleHalf || KIND == kSampleBFloat16, "no such form");
    constexpr int IB = narrow::input_bytes(KIND);
    const bool odd = b & 1u;
    float sy = 1.f, oy = 0.f, sc = 1.f, oc = 0.f;
    if constexpr (Scaled) {
        sy = a.value_scale[0], oy = a.value_offset[0];
        sc = odd ? a.value_scale[2] : a.value_scale[1], oc = odd ? a.value_offset[2] : a.value_offset[1];
    }
    uint32_t d[3];
    load_six_narrowed<KIND, Scaled>(a.plane[0] + r.luma + static_cast<size_t>(b) * (6 * IB), sy, oy, y);
    load_six_narrowed<KIND, Scaled>((odd ? a.plane[2] : a.plane[1]) + r.chroma + static_cast<size_t>(b >> 1) * (6 * IB), sc, oc, d);
    Three first, second;
    first.lo = d[0], first.hi = d[1] & 0xffffu;
    second.lo = (d[1] >> 16) | (d[2] << 16), second.hi = d[2] >> 16;
    s.keep = odd ? second : first;
    s.send = odd ? first : second;
}

// Sample x of a row of plane c as its 10-bit code.
template <int KIND, bool Scaled>
JINC_V210_HD uint32_t code_in_row(const NarrowV210Args& a, const char* row, uint32_t x, int c) {
    float v = narrow::value_in_row<KIND>(row, x);
    if constexpr (Scaled) v = narrow::scaled_value(v, a.value_scale[c], a.value_offset[c]);
    return narrow::word_of(v, 1023.f);
}

// Block b in [paired_blocks(a), row_blocks(a)): samples beyond the planes' widths are not read; their fields are zeros.
template <int KIND, bool Scaled>
JINC_V210_HD void narrow_tail(const NarrowV210Args& a, const RowOf& r, uint32_t b) {
    uint32_t w[4], y[6] = {0, 0, 0, 0, 0, 0}, cb[3] = {0, 0, 0}, cr[3] = {0, 0, 0};
    const char* py = a.plane[0] + r.luma;
    const char* pu = a.plane[1] + r.chroma;
    const char* pv = a.plane[2] + r.chroma;
    for (uint32_t i = 0; i < 6; ++i)
        if (b * 6 + i < a.width) y[i] = code_in_row<KIND, Scaled>(a, py, b * 6 + i, 0);
    for (uint32_t i = 0; i < 3; ++i)
        if (b * 3 + i < (a.width >> 1))
            cb[i] = code_in_row<KIND, Scaled>(a, pu, b * 3 + i, 1), cr[i] = code_in_row<KIND, Scaled>(a, pv, b * 3 + i, 2);
    encode_block(y, cb, cr, w);
    store_block(r.blocks + static_cast<size_t>(b) * 16, a.unit, w);
}

}  // namespace v210
}  // namespace jinc
