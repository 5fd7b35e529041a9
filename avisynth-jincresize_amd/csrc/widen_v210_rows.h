// widen_v210_rows.h -- one lane's share of one row of the pass that widens v210 blocks (kernel_widen.hip widen_v210_kernel;
// kernels.h V210Args), as plain inline functions for host and device: a stand-alone host program runs exactly this code lane by
// lane and trip by trip against exactly sized buffers, with the cross-lane move modelled by indexing
// (tests/host_sanitizer/widen_v210_rows_main.cpp).  The block side, its decoding and the walk are v210_rows.h's, unchanged.
//
// The twelve 10-bit fields of a block become fp32 (OB = 4) or binary16 (OB = 2) samples of three dense planes: `width` luma
// samples and width / 2 samples of each chroma plane per row, float(field) each -- exact in either type.  On the plane side
// V210Args is read with samples of OB bytes; pitches and frame strides stay in bytes.
//
// A lane owns one block per trip and blocks move in PAIRS (lanes l and l ^ 1), as in unpack_v210_kernel: each lane loads its
// block as one 16-byte access and stores its 6 converted luma samples side by side -- 24 bytes at an 8-byte aligned address
// (fp32) or 12 bytes at a 4-byte aligned address (binary16), contiguous from lane to lane; the two lanes exchange their three RAW
// chroma samples (two dwords: widen_pair_begin runs in front of that exchange, widen_pair_end behind it, and the conversion happens
// there), then the even lane stores the pair's 6 Cb samples and the odd lane its 6 Cr samples in the same way.  What pairs leave
// over -- the odd whole block of a row with an odd number of them and the row's partial last block -- goes sample by sample under
// the width guards (widen_tail): nothing beyond `width` (luma) or `width / 2` (chroma) samples is stored to a plane.  The blocks
// are never written.
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "kernels.h"
#include "v210_rows.h"
#include "widen_rows.h"

namespace jinc {
namespace v210 {

// The bits of a 10-bit value converted to the plane's type: v_cvt_f32_u32, v_cvt_f16_f32 on top for binary16.
template <int OB>
JINC_V210_HD uint32_t widened_bits(uint32_t value) {
    const float v = static_cast<float>(value);
    if constexpr (OB == 4) return widen::float_bits(v);
    else return widen::half_bits(v);
}

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));  // 8 bytes as ONE access
// Six converted samples side by side: fp32 -- three 8-byte accesses at an 8-byte aligned address; binary16 -- three adjacent dwords
// at a 4-byte aligned address, as store_six.
template <int OB>
JINC_V210_HD void store_six_widened(char* p, const uint32_t s[6]) {
    if constexpr (OB == 4) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            u32x2 v;
            v.x = widened_bits<4>(s[2 * k]), v.y = widened_bits<4>(s[2 * k + 1]);
            reinterpret_cast<u32x2*>(p)[k] = v;
        }
    } else {
        const uint32_t d[3] = {widened_bits<2>(s[0]) | (widened_bits<2>(s[1]) << 16), widened_bits<2>(s[2]) | (widened_bits<2>(s[3]) << 16),
                               widened_bits<2>(s[4]) | (widened_bits<2>(s[5]) << 16)};
        store_six(p, d);
    }
}

// Block b < paired_blocks(a).  Stores the block's converted luma; s.keep: the block's RAW samples of the plane this lane stores (Cb
// if b is even, Cr if odd), s.send: those of the other plane, which the lane of block b ^ 1 stores.
template <int OB>
JINC_V210_HD void widen_pair_begin(const V210Args& a, const RowOf& r, uint32_t b, LaneState& s) {
    static_assert(OB == 4 || OB == 2, "no such form");
    uint32_t w[4], y[6], cb[3], cr[3];
    load_block(r.blocks + static_cast<size_t>(b) * 16, a.unit, w);
    decode_block(w, y, cb, cr);
    store_six_widened<OB>(a.plane[0] + r.luma + static_cast<size_t>(b) * (6 * OB), y);
    const Three u = three_of(cb[0], cb[1], cb[2]), v = three_of(cr[0], cr[1], cr[2]);
    const bool odd = b & 1u;
    s.keep = odd ? v : u;
    s.send = odd ? u : v;
}
// recv: s.send of the lane of block b ^ 1.  The even block's samples come first in the pair's six, which lie at sample
// 3 * (b & ~1) of Cb (even block) or Cr (odd block).
template <int OB>
JINC_V210_HD void widen_pair_end(const V210Args& a, const RowOf& r, uint32_t b, const LaneState& s, const Three& recv) {
    const bool odd = b & 1u;
    const Three first = odd ? recv : s.keep, second = odd ? s.keep : recv;
    const uint32_t six[6] = {sample_of(first, 0), sample_of(first, 1), sample_of(first, 2), sample_of(second, 0), sample_of(second, 1), sample_of(second, 2)};
    store_six_widened<OB>((odd ? a.plane[2] : a.plane[1]) + r.chroma + static_cast<size_t>(b >> 1) * (6 * OB), six);
}
// Block b in [paired_blocks(a), row_blocks(a)): sample by sample, nothing beyond the planes' widths.
template <int OB>
JINC_V210_HD void widen_tail(const V210Args& a, const RowOf& r, uint32_t b) {
    uint32_t w[4], y[6], cb[3], cr[3];
    load_block(r.blocks + static_cast<size_t>(b) * 16, a.unit, w);
    decode_block(w, y, cb, cr);
    typedef typename std::conditional<OB == 4, uint32_t, uint16_t>::type Sample;
    Sample* py = reinterpret_cast<Sample*>(a.plane[0] + r.luma);
    Sample* pu = reinterpret_cast<Sample*>(a.plane[1] + r.chroma);
    Sample* pv = reinterpret_cast<Sample*>(a.plane[2] + r.chroma);
    for (uint32_t i = 0; i < 6; ++i)
        if (b * 6 + i < a.width) py[b * 6 + i] = static_cast<Sample>(widened_bits<OB>(y[i]));
    for (uint32_t i = 0; i < 3; ++i)
        if (b * 3 + i < (a.width >> 1))
            pu[b * 3 + i] = static_cast<Sample>(widened_bits<OB>(cb[i])), pv[b * 3 + i] = static_cast<Sample>(widened_bits<OB>(cr[i]));
}

}  // namespace v210
}  // namespace jinc
