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
//
// The scaled forms (trailing template parameters KIND and Scaled; jinc_filter_process_device_widened_v210_scaled; kernels.h
// WidenV210Args): plane c (0: Y, 1: Cb, 2: Cr) holds s = fl32(fl32(float(field) * value_scale[c]) + value_offset[c]) -- widen_rows.h's
// scaled_value, two fp32 roundings, never an FMA -- and 16-bit planes hold s narrowed round-to-nearest-even by widen_rows.h's
// pair_bits / rounded_bits, the ONE definition of that rounding; bfloat16 planes (KIND = kSampleBFloat16) exist in this form only.
// The exchange stays in front of all that: RAW samples cross the lanes, and the lane that stores the pair's chroma row takes plane
// 1's pair when its block is even and plane 2's when it is odd -- a select between two scalar pairs, as the plane's base is.  The
// unscaled forms read neither array.
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
// A 10-bit value as the fp32 sample the plane holds: the value itself, or widen_rows.h's scaled_value of it.
template <bool Scaled>
JINC_V210_HD float widened_sample(uint32_t value, float scale, float offset) {
    const float v = static_cast<float>(value);
    if constexpr (Scaled) return widen::scaled_value(v, scale, offset);
    else return v;
}
// ... and ONE sample's bits in the plane's type (the tails).
template <int OB, int KIND, bool Scaled>
JINC_V210_HD uint32_t widened_bits(uint32_t value, float scale, float offset) {
    if constexpr (!Scaled) return widened_bits<OB>(value);
    else if constexpr (OB == 4) return widen::float_bits(widened_sample<true>(value, scale, offset));
    else return widen::rounded_bits<KIND>(widened_sample<true>(value, scale, offset));
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
// ... of ONE plane, with that plane's pair in the scaled forms: the same accesses.
template <int OB, int KIND, bool Scaled>
JINC_V210_HD void store_six_widened(char* p, const uint32_t s[6], float scale, float offset) {
    if constexpr (!Scaled) {
        store_six_widened<OB>(p, s);
    } else if constexpr (OB == 4) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            u32x2 v;
            v.x = widen::float_bits(widened_sample<true>(s[2 * k], scale, offset)), v.y = widen::float_bits(widened_sample<true>(s[2 * k + 1], scale, offset));
            reinterpret_cast<u32x2*>(p)[k] = v;
        }
    } else {
        uint32_t d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = widen::pair_bits<KIND, true>(widened_sample<true>(s[2 * k], scale, offset), widened_sample<true>(s[2 * k + 1], scale, offset));
        store_six(p, d);
    }
}

// Block b < paired_blocks(a).  Stores the block's converted luma; s.keep: the block's RAW samples of the plane this lane stores (Cb
// if b is even, Cr if odd), s.send: those of the other plane, which the lane of block b ^ 1 stores.
// Args: V210Args, or WidenV210Args for the scaled forms.
template <int OB, int KIND = 0, bool Scaled = false, class Args>
JINC_V210_HD void widen_pair_begin(const Args& a, const RowOf& r, uint32_t b, LaneState& s) {
    static_assert(OB == 4 || OB == 2, "no such form");
    static_assert(KIND == 0 || (KIND == kSampleHalf && OB == 2) || (KIND == kSampleBFloat16 && OB == 2 && Scaled), "no such form");
    uint32_t w[4], y[6], cb[3], cr[3];
    load_block(r.blocks + static_cast<size_t>(b) * 16, a.unit, w);
    decode_block(w, y, cb, cr);
    float sc = 1.f, of = 0.f;
    if constexpr (Scaled) sc = a.value_scale[0], of = a.value_offset[0];
    store_six_widened<OB, KIND, Scaled>(a.plane[0] + r.luma + static_cast<size_t>(b) * (6 * OB), y, sc, of);
    const Three u = three_of(cb[0], cb[1], cb[2]), v = three_of(cr[0], cr[1], cr[2]);
    const bool odd = b & 1u;
    s.keep = odd ? v : u;
    s.send = odd ? u : v;
}
// recv: s.send of the lane of block b ^ 1.  The even block's samples come first in the pair's six, which lie at sample
// 3 * (b & ~1) of Cb (even block) or Cr (odd block).
template <int OB, int KIND = 0, bool Scaled = false, class Args>
JINC_V210_HD void widen_pair_end(const Args& a, const RowOf& r, uint32_t b, const LaneState& s, const Three& recv) {
    const bool odd = b & 1u;
    const Three first = odd ? recv : s.keep, second = odd ? s.keep : recv;
    const uint32_t six[6] = {sample_of(first, 0), sample_of(first, 1), sample_of(first, 2), sample_of(second, 0), sample_of(second, 1), sample_of(second, 2)};
    float sc = 1.f, of = 0.f;
    if constexpr (Scaled) {  // (the pair of the plane this lane stores: a select between two scalars)
        const float sc_cb = a.value_scale[1], sc_cr = a.value_scale[2], of_cb = a.value_offset[1], of_cr = a.value_offset[2];
        sc = odd ? sc_cr : sc_cb, of = odd ? of_cr : of_cb;
    }
    store_six_widened<OB, KIND, Scaled>((odd ? a.plane[2] : a.plane[1]) + r.chroma + static_cast<size_t>(b >> 1) * (6 * OB), six, sc, of);
}
// Block b in [paired_blocks(a), row_blocks(a)): sample by sample, nothing beyond the planes' widths.
template <int OB, int KIND = 0, bool Scaled = false, class Args>
JINC_V210_HD void widen_tail(const Args& a, const RowOf& r, uint32_t b) {
    uint32_t w[4], y[6], cb[3], cr[3];
    load_block(r.blocks + static_cast<size_t>(b) * 16, a.unit, w);
    decode_block(w, y, cb, cr);
    float sc[3] = {1.f, 1.f, 1.f}, of[3] = {0.f, 0.f, 0.f};
    if constexpr (Scaled) {
#pragma unroll
        for (int c = 0; c < 3; ++c) sc[c] = a.value_scale[c], of[c] = a.value_offset[c];
    }
    typedef typename std::conditional<OB == 4, uint32_t, uint16_t>::type Sample;
    Sample* py = reinterpret_cast<Sample*>(a.plane[0] + r.luma);
    Sample* pu = reinterpret_cast<Sample*>(a.plane[1] + r.chroma);
    Sample* pv = reinterpret_cast<Sample*>(a.plane[2] + r.chroma);
    for (uint32_t i = 0; i < 6; ++i)
        if (b * 6 + i < a.width) py[b * 6 + i] = static_cast<Sample>(widened_bits<OB, KIND, Scaled>(y[i], sc[0], of[0]));
    for (uint32_t i = 0; i < 3; ++i)
        if (b * 3 + i < (a.width >> 1))
            pu[b * 3 + i] = static_cast<Sample>(widened_bits<OB, KIND, Scaled>(cb[i], sc[1], of[1])), pv[b * 3 + i] = static_cast<Sample>(widened_bits<OB, KIND, Scaled>(cr[i], sc[2], of[2]));
}

}  // namespace v210
}  // namespace jinc
