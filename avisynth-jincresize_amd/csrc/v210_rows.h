// v210_rows.h -- one lane's share of one row of the v210 passes (kernel_interleave.hip unpack_v210_kernel / pack_v210_kernel;
// kernels.h V210Args), as plain inline functions for host and device: a stand-alone host program runs exactly this code lane by
// lane and trip by trip against exactly sized buffers, with the cross-lane move modelled by indexing (tests/host_sanitizer).
//
// v210: a row is a run of 16-byte blocks of four little-endian 32-bit words, three 10-bit fields per word at bits 0, 10 and 20
// (bits 30 - 31 unused).  Block b holds luma samples 6b .. 6b+5 and samples 3b .. 3b+2 of each chroma plane:
//   word 0: Cb[3b]   | Y[6b]     << 10 | Cr[3b]   << 20        word 2: Cr[3b+1] | Y[6b+3]   << 10 | Cb[3b+2] << 20
//   word 1: Y[6b+1]  | Cb[3b+1]  << 10 | Y[6b+2]  << 20        word 3: Y[6b+4]  | Cr[3b+2]  << 10 | Y[6b+5]  << 20
//
// A lane owns one block per trip.  Blocks move in PAIRS (lanes l and l ^ 1; the walk starts at block `lane`, so a pair is blocks
// 2k and 2k + 1): each lane moves its block as one 16-byte access and its 6 luma samples as one 12-byte access (4-byte aligned,
// contiguous from lane to lane); the even lane moves the pair's 6 Cb samples, the odd lane the pair's 6 Cr samples, 12 bytes
// each, after the two lanes have exchanged three chroma samples (two dwords) -- *_begin runs in front of that exchange, *_end
// behind it.  What pairs leave over -- the odd whole block of a row with an odd number of them and the row's partial last block --
// goes sample by sample under a width guard (*_tail): nothing beyond `width` (luma) or `width / 2` (chroma) is read from or stored
// to the dense planes.  The block side always moves whole blocks: they belong to the row (jinc_v210_row_bytes).
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernels.h"

#if defined(__HIPCC__)
#define JINC_V210_HD __host__ __device__ __forceinline__
#else
#define JINC_V210_HD inline
#endif

namespace jinc {
namespace v210 {

// Three 16-bit samples in two dwords: s0 | s1 << 16, s2.
struct Three {
    uint32_t lo = 0, hi = 0;
};
JINC_V210_HD uint32_t sample_of(const Three& t, int i) { return i == 0 ? t.lo & 0xffffu : i == 1 ? t.lo >> 16 : t.hi & 0xffffu; }
JINC_V210_HD Three three_of(uint32_t s0, uint32_t s1, uint32_t s2) {
    Three t;
    t.lo = s0 | (s1 << 16), t.hi = s2;
    return t;
}

// What a lane holds between *_begin and *_end: the chroma samples it keeps and those its partner gets.
struct LaneState {
    Three keep, send;
};

// One block's fields.  y[6], cb[3], cr[3]: values 0 .. 1023 (decode masks them out of the words; encode masks what it is given, so
// a field stays inside its bits whatever the planes hold, and bits 30 - 31 are zeros by construction).
JINC_V210_HD void decode_block(const uint32_t w[4], uint32_t y[6], uint32_t cb[3], uint32_t cr[3]) {
    cb[0] = w[0] & 1023u, y[0] = (w[0] >> 10) & 1023u, cr[0] = (w[0] >> 20) & 1023u;
    y[1] = w[1] & 1023u, cb[1] = (w[1] >> 10) & 1023u, y[2] = (w[1] >> 20) & 1023u;
    cr[1] = w[2] & 1023u, y[3] = (w[2] >> 10) & 1023u, cb[2] = (w[2] >> 20) & 1023u;
    y[4] = w[3] & 1023u, cr[2] = (w[3] >> 10) & 1023u, y[5] = (w[3] >> 20) & 1023u;
}
JINC_V210_HD void encode_block(const uint32_t y[6], const uint32_t cb[3], const uint32_t cr[3], uint32_t w[4]) {
    w[0] = (cb[0] & 1023u) | ((y[0] & 1023u) << 10) | ((cr[0] & 1023u) << 20);
    w[1] = (y[1] & 1023u) | ((cb[1] & 1023u) << 10) | ((y[2] & 1023u) << 20);
    w[2] = (cr[1] & 1023u) | ((y[3] & 1023u) << 10) | ((cb[2] & 1023u) << 20);
    w[3] = (y[4] & 1023u) | ((cr[2] & 1023u) << 10) | ((y[5] & 1023u) << 20);
}

// A block as ONE 16-byte access (a vector type of the compiler's: the access is not taken apart) or as four dwords.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
JINC_V210_HD void load_block(const char* p, uint32_t unit, uint32_t w[4]) {
    if (unit == 16) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(p);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else {
        for (int k = 0; k < 4; ++k) w[k] = reinterpret_cast<const uint32_t*>(p)[k];
    }
}
JINC_V210_HD void store_block(char* p, uint32_t unit, const uint32_t w[4]) {
    if (unit == 16) {
        u32x4 v;
        v.x = w[0], v.y = w[1], v.z = w[2], v.w = w[3];
        *reinterpret_cast<u32x4*>(p) = v;
    } else {
        for (int k = 0; k < 4; ++k) reinterpret_cast<uint32_t*>(p)[k] = w[k];
    }
}
// Six 16-bit samples of a dense plane: 12 bytes at a 4-byte aligned address (three adjacent dwords; one 12-byte access on gfx950).
JINC_V210_HD void load_six(const char* p, uint32_t d[3]) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    d[0] = q[0], d[1] = q[1], d[2] = q[2];
}
JINC_V210_HD void store_six(char* p, const uint32_t d[3]) {
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
    q[0] = d[0], q[1] = d[1], q[2] = d[2];
}

struct RowOf {
    char* blocks;  // the row's first block
    size_t luma, chroma;  // byte offsets of the row in the luma plane and in either chroma plane
};
JINC_V210_HD RowOf row_of(const V210Args& a, uint32_t frame, uint32_t row) {
    RowOf r;
    r.blocks = a.blocks + frame * a.block_frame_stride + static_cast<size_t>(row) * a.block_pitch;
    r.luma = frame * a.luma_frame_stride + static_cast<size_t>(row) * a.luma_pitch;
    r.chroma = frame * a.chroma_frame_stride + static_cast<size_t>(row) * a.chroma_pitch;
    return r;
}
JINC_V210_HD uint32_t paired_blocks(const V210Args& a) { return a.whole_blocks & ~1u; }             // blocks that move in pairs
JINC_V210_HD uint32_t row_blocks(const V210Args& a) { return a.whole_blocks + (a.whole_blocks * 6u < a.width ? 1u : 0u); }
// The pair's six samples of ONE chroma plane: Cb for the even block, Cr for the odd one, at sample 3 * (b & ~1).
JINC_V210_HD char* pair_chroma(const V210Args& a, const RowOf& r, uint32_t b) {
    return ((b & 1u) ? a.plane[2] : a.plane[1]) + r.chroma + static_cast<size_t>(b >> 1) * 12;
}

// ---- unpack: blocks -> planes ----
// Block b < paired_blocks(a).  Stores the block's luma; s.keep: the block's samples of the plane this lane stores (Cb if b is
// even, Cr if odd), s.send: those of the other plane, which the lane of block b ^ 1 stores.
JINC_V210_HD void unpack_pair_begin(const V210Args& a, const RowOf& r, uint32_t b, LaneState& s) {
    uint32_t w[4], y[6], cb[3], cr[3];
    load_block(r.blocks + static_cast<size_t>(b) * 16, a.unit, w);
    decode_block(w, y, cb, cr);
    const uint32_t luma[3] = {y[0] | (y[1] << 16), y[2] | (y[3] << 16), y[4] | (y[5] << 16)};
    store_six(a.plane[0] + r.luma + static_cast<size_t>(b) * 12, luma);
    const Three u = three_of(cb[0], cb[1], cb[2]), v = three_of(cr[0], cr[1], cr[2]);
    const bool odd = b & 1u;
    s.keep = odd ? v : u;
    s.send = odd ? u : v;
}
// recv: s.send of the lane of block b ^ 1.  The even block's samples come first in the pair's six.
JINC_V210_HD void unpack_pair_end(const V210Args& a, const RowOf& r, uint32_t b, const LaneState& s, const Three& recv) {
    const bool odd = b & 1u;
    const Three first = odd ? recv : s.keep, second = odd ? s.keep : recv;
    const uint32_t d[3] = {first.lo, (first.hi & 0xffffu) | (second.lo << 16), (second.lo >> 16) | (second.hi << 16)};
    store_six(pair_chroma(a, r, b), d);
}
// Block b in [paired_blocks(a), row_blocks(a)): sample by sample, nothing beyond the planes' widths.
JINC_V210_HD void unpack_tail(const V210Args& a, const RowOf& r, uint32_t b) {
    uint32_t w[4], y[6], cb[3], cr[3];
    load_block(r.blocks + static_cast<size_t>(b) * 16, a.unit, w);
    decode_block(w, y, cb, cr);
    uint16_t* py = reinterpret_cast<uint16_t*>(a.plane[0] + r.luma);
    uint16_t* pu = reinterpret_cast<uint16_t*>(a.plane[1] + r.chroma);
    uint16_t* pv = reinterpret_cast<uint16_t*>(a.plane[2] + r.chroma);
    for (uint32_t i = 0; i < 6; ++i)
        if (b * 6 + i < a.width) py[b * 6 + i] = static_cast<uint16_t>(y[i]);
    for (uint32_t i = 0; i < 3; ++i)
        if (b * 3 + i < (a.width >> 1)) pu[b * 3 + i] = static_cast<uint16_t>(cb[i]), pv[b * 3 + i] = static_cast<uint16_t>(cr[i]);
}

// ---- pack: planes -> blocks ----
// Block b < paired_blocks(a).  Loads the block's luma (y, three dwords) and the pair's six samples of one chroma plane; s.keep:
// this block's three of them, s.send: the three of block b ^ 1.
JINC_V210_HD void pack_pair_begin(const V210Args& a, const RowOf& r, uint32_t b, uint32_t y[3], LaneState& s) {
    uint32_t d[3];
    load_six(a.plane[0] + r.luma + static_cast<size_t>(b) * 12, y);
    load_six(pair_chroma(a, r, b), d);
    Three first, second;
    first.lo = d[0], first.hi = d[1] & 0xffffu;
    second.lo = (d[1] >> 16) | (d[2] << 16), second.hi = d[2] >> 16;
    const bool odd = b & 1u;
    s.keep = odd ? second : first;
    s.send = odd ? first : second;
}
// recv: s.send of the lane of block b ^ 1 -- this block's samples of the other chroma plane.  Stores the whole block.
JINC_V210_HD void pack_pair_end(const V210Args& a, const RowOf& r, uint32_t b, const uint32_t y[3], const LaneState& s, const Three& recv) {
    const bool odd = b & 1u;
    const Three u = odd ? recv : s.keep, v = odd ? s.keep : recv;
    const uint32_t luma[6] = {y[0] & 0xffffu, y[0] >> 16, y[1] & 0xffffu, y[1] >> 16, y[2] & 0xffffu, y[2] >> 16};
    const uint32_t cb[3] = {sample_of(u, 0), sample_of(u, 1), sample_of(u, 2)}, cr[3] = {sample_of(v, 0), sample_of(v, 1), sample_of(v, 2)};
    uint32_t w[4];
    encode_block(luma, cb, cr, w);
    store_block(r.blocks + static_cast<size_t>(b) * 16, a.unit, w);
}
// Block b in [paired_blocks(a), row_blocks(a)): samples beyond the planes' widths are not read; their fields are zeros.
JINC_V210_HD void pack_tail(const V210Args& a, const RowOf& r, uint32_t b) {
    uint32_t w[4], y[6] = {0, 0, 0, 0, 0, 0}, cb[3] = {0, 0, 0}, cr[3] = {0, 0, 0};
    const uint16_t* py = reinterpret_cast<const uint16_t*>(a.plane[0] + r.luma);
    const uint16_t* pu = reinterpret_cast<const uint16_t*>(a.plane[1] + r.chroma);
    const uint16_t* pv = reinterpret_cast<const uint16_t*>(a.plane[2] + r.chroma);
    for (uint32_t i = 0; i < 6; ++i)
        if (b * 6 + i < a.width) y[i] = py[b * 6 + i];
    for (uint32_t i = 0; i < 3; ++i)
        if (b * 3 + i < (a.width >> 1)) cb[i] = pu[b * 3 + i], cr[i] = pv[b * 3 + i];
    encode_block(y, cb, cr, w);
    store_block(r.blocks + static_cast<size_t>(b) * 16, a.unit, w);
}

}  // namespace v210
}  // namespace jinc
