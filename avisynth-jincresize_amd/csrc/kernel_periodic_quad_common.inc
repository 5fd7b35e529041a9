// kernel_periodic_quad_common.inc -- pieces shared by the quad forms of the periodic family (kernel_periodic_quad.hip,
// kernel_periodic_quad2.inc, kernel_periodic_quad2x8.hip); included INSIDE namespace jinc { namespace { of the including translation
// unit, behind kernel_periodic_common.inc.  What only one of the units uses lives in that unit.
//   every quad form            quad_fetch / quad_arrived, quad_fetch10 / quad_arrived10: the coefficient pairs of a kernel row
//   the 8-row supports         kQuad8TrimTap4, quad8_trim_of: the chord pattern TR8 (quad8, quad2x8)
//   two periods per lane       JINC_LO / JINC_HI / JINC_ADD2, store_quad_buf, edge_tile_of, stage_edge_column, quad2_edge_columns
//                              (quad2, quad2x8)

// The 16 coefficient pairs of kernel row LY (q = 0: pairs 0..7, q = 1: pairs 8..15): two s_load_dwordx16.
__device__ __forceinline__ void quad_fetch(f32x2 (&c)[16], const JINC_CONSTANT f32x2* quad, int ly) {
#pragma unroll
    for (int k = 0; k < 16; ++k) c[k] = quad[ly * 16 + k];
}
__device__ __forceinline__ void quad_arrived(f32x2 (&c)[16]) {
#pragma unroll
    for (int k = 0; k < 16; ++k) asm volatile("" : "+s"(c[k]));
}

// Nine taps per kernel row (quad_pixel9, quad2_pixel9): the 2 x 10 coefficient pairs of a kernel row do not fit twice next to
// everything else (2 x 40 SGPRs), so the two phase rows q alternate through two sets of 20 SGPRs: the pairs of (ly, q = 1) are
// requested before the taps of (ly, q = 0) are issued, those of (ly + 1, q = 0) before the taps of (ly, q = 1).  Layout:
// quad[ly][q][10 pairs][p].
__device__ __forceinline__ void quad_fetch10(f32x2 (&c)[10], const JINC_CONSTANT f32x2* quad, int row) {
#pragma unroll
    for (int k = 0; k < 10; ++k) c[k] = quad[row * 10 + k];
}
__device__ __forceinline__ void quad_arrived10(f32x2 (&c)[10]) {
#pragma unroll
    for (int k = 0; k < 10; ++k) asm volatile("" : "+s"(c[k]));
}

// TR8: compile-time pattern of the kernel rows of an 8 x 8 support that run without their first and last t taps (quad_row8_t1 / _t2,
// quad2_row8_t1 / _t2: those taps carry zero coefficients for both phases p of a q), two bits per (kernel row ly, q) at bit
// 2 * (2 * ly + q).  Instantiated for "none" and for the 2x up-scale with tap 4 (blur 1 and 0.98): q = 0 rows 0 / 6 / 7 leave out
// 1 / 1 / 2 taps per side, q = 1 rows 0 / 1 / 7 leave out 2 / 1 / 1 -- 56 instead of 64 taps per sample.  The launcher takes the
// pattern when the plan's rows allow at least it.
constexpr uint32_t kQuad8TrimTap4 = kQuad8TrimTap4Value;
constexpr int quad8_trim_of(uint32_t tr8, int ly, int q) { return static_cast<int>((tr8 >> (2 * (2 * ly + q))) & 3u); }

// The two-periods-per-lane rows (quad2_row6, quad2_row6_inner, quad2_row8) spell their taps with these: the product of a coefficient
// pair with one sample of a window pair, and the adds of the lane's two periods.  (The units that use them undefine them after the
// last use.)
#define JINC_LO(T, W, C) "v_pk_mul_f32 " T ", " W ", " C " op_sel_hi:[0,1]\n\t"                 /* sample = low half of the pair */
#define JINC_HI(T, W, C) "v_pk_mul_f32 " T ", " W ", " C " op_sel:[1,0] op_sel_hi:[1,1]\n\t"   /* sample = high half */
#define JINC_ADD2 "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3\n\t"

// The four (or, for the lane that holds the plane's last odd period, two) samples of one output row of a lane: one store.
template <typename T>
__device__ __forceinline__ void store_quad_buf(BufferRsrc rsrc, uint32_t voffset, uint32_t soffset, f32x2 a, f32x2 b, float peak, bool b_ok) {
    if constexpr (std::is_same_v<T, float>) {
        // two 8-byte stores: the samples start at a 4-byte boundary (odd interior origin), and a 16-byte store that is not
        // 16-byte aligned does not write its four dwords where they belong (measured: dwords 1 and 3 took the values of 0 and 2)
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, a), rsrc, voffset, soffset, 0);
        if (b_ok) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, b), rsrc, voffset + 8u, soffset, 0);
    } else if constexpr (std::is_same_v<T, uint8_t>) {
        uint32_t w = __builtin_amdgcn_cvt_pk_u8_f32(a.x, 0u, 0u);
        w = __builtin_amdgcn_cvt_pk_u8_f32(a.y, 1u, w);
        w = __builtin_amdgcn_cvt_pk_u8_f32(b.x, 2u, w);
        w = __builtin_amdgcn_cvt_pk_u8_f32(b.y, 3u, w);
        if (b_ok) __builtin_amdgcn_raw_buffer_store_b32(w, rsrc, voffset, soffset, 0);
        else __builtin_amdgcn_raw_buffer_store_b16(static_cast<uint16_t>(w), rsrc, voffset, soffset, 0);
    } else {
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        const uint32_t lo = round_pair16<T>(a.x, a.y, peak);
        if (b_ok) {
            const u32x2 v = {lo, round_pair16<T>(b.x, b.y, peak)};
            __builtin_amdgcn_raw_buffer_store_b64(v, rsrc, voffset, soffset, 0);
        } else {
            __builtin_amdgcn_raw_buffer_store_b32(lo, rsrc, voffset, soffset, 0);
        }
    }
}

// The plane's border columns beside this tile's rows (PeriodicArgs::EdgeColumns; integer planes, first / last tile column only) for the
// two-periods-per-lane quad forms (Cfg: Quad2Cfg / Quad2x8Cfg; NR kernel rows = the interior's trimmed rows, NC = the plan's filter size).
// Lane = period-row of the tile, one NR-row x NC-column register window per lane for every column of the side (they share their
// window origin) and both row phases (they share theirs); wave w takes row phase w & 1 of one half of the side's columns, four
// columns at a time: their samples are adjacent in the lane's output row and leave as one store.  Every sample is the reference's
// chain: taps in (ly, lx) order, multiply and add un-fused (ref /root/reference/src/JincResize.cpp:570-579); the kernel rows left
// out carry zero coefficients (checked on the host).
template <typename T>
__device__ __forceinline__ bool edge_tile_of(const PeriodicArgs& a, int tile_x) {
    if constexpr (is_float_sample_v<T>) return false;  // (float and half planes: the border kernels, whatever the samples)
    return a.edge.coeffs != nullptr && ((a.edge.n[0] > 0 && tile_x == a.edge.tile_x[0]) || (a.edge.n[1] > 0 && tile_x == a.edge.tile_x[1]));
}

// An edge window that starts one source column in front of the tile (the left border's, when the interior's support was trimmed by a
// column): that column goes into the word in front of each tile row -- the previous row's last spare word, or for row 0 the word in
// front of the tile (the kernels allocate two).  Call between the staging writes and the barrier, edge tiles only.
template <typename T, typename Cfg>
__device__ __forceinline__ void stage_edge_column(const PeriodicArgs& a, const PlaneIO& io, float* tile, int tile_x, const char* sbase, int gx0, int gy0,
                                                  int wave, int lane) {
    static_assert(Cfg::kLdsPitch >= Cfg::kLdsCols + 1 && Cfg::kLdsRows <= 64, "a spare word per tile row, one tile row per lane");
    const bool in_front = (a.edge.n[0] > 0 && tile_x == a.edge.tile_x[0] && a.edge.lds_col[0] < 0) || (a.edge.n[1] > 0 && tile_x == a.edge.tile_x[1] && a.edge.lds_col[1] < 0);
    if (in_front && wave == 0 && lane < Cfg::kLdsRows && gx0 > 0) {
        int gy = gy0 + lane;
        gy = gy < a.src_h ? gy : a.src_h - 1;
        tile[lane * Cfg::kLdsPitch - 1] = to_float(reinterpret_cast<const T*>(sbase + static_cast<size_t>(gy) * io.src_pitch)[gx0 - 1]);
    }
}

// wave_shl:1 -- lane l takes lane l + 1's value
__device__ __forceinline__ float wave_shl1(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
}
__device__ __forceinline__ f32x2 wave_shl1(f32x2 v) { return f32x2{wave_shl1(v.x), wave_shl1(v.y)}; }
__device__ __forceinline__ float frame_lo(float v) { return v; }
__device__ __forceinline__ float frame_lo(f32x2 v) { return v.x; }
__device__ __forceinline__ float frame_hi(float v) { return v; }
__device__ __forceinline__ float frame_hi(f32x2 v) { return v.y; }

// V: a staged sample -- float, or the f32x2 of the frame-pair tile (quad2_share_body): both frames' chains run in the packed halves
// (v_pk_mul_f32 with the coefficient broadcast, v_pk_add_f32: each half is the per-frame chain, same order, un-fused) and leave to
// drsrc and, when hi_ok, drsrc_hi.  ES: staged samples per tile word of type V (2: one frame's half of the frame-pair tile, read as floats
// with `tile` pointing at that half of the first pair -- the half-tile instance, whose 80 VGPRs do not hold a window of pairs).
// W: the tile's word, V itself or the bf16 pair word of the 8-bit full tiles (quad2_pair_of rebuilds the f32 pair: same bits).
__device__ __forceinline__ float quad2_pair_of(float v) { return v; }
__device__ __forceinline__ f32x2 quad2_pair_of(f32x2 v) { return v; }
__device__ __forceinline__ f32x2 quad2_pair_of(uint32_t v) {  // low half: the low frame's bf16, high half: the high frame's
    return f32x2{__builtin_bit_cast(float, v << 16), __builtin_bit_cast(float, v & 0xffff0000u)};
}
template <typename T, typename Cfg, int NR, int NC, typename V = float, int ES = 1, typename W = V>
__device__ __forceinline__ void quad2_edge_columns(const PeriodicArgs& a, const PlaneIO& io, const W* tile, int tile_x, int j0, int wave, int lane,
                                                   BufferRsrc drsrc, BufferRsrc drsrc_hi, bool hi_ok) {
    constexpr bool kPair = !std::is_same_v<V, float>;
    constexpr int NCP = (NC + 3) & ~3;  // floats per coefficient row
    for (int s = 0; s < 2; ++s) {
        const int n = a.edge.n[s];
        if (n <= 0 || tile_x != a.edge.tile_x[s]) continue;  // workgroup-uniform
        const int q = wave & 1, half = (n + 1) >> 1;
        const int k_begin = (wave >> 1) * half, k_end = k_begin + half < n ? k_begin + half : n;
        if (k_begin >= k_end) continue;  // wave-uniform
        const bool live = lane < Cfg::kTileRows && j0 + lane < a.nj;
        // The window: lane l reads the NC samples of tile row l, rows l + 1 .. l + NR - 1 come over from the lanes above by whole-wave
        // shifts (read from LDS, the lanes' rows lie a pitch apart: four banks for 64 lanes, a 16-way conflict per read.  Measured
        // level with this form all the same -- round5/edge_cols_ab.log -- the chains are what the edge tiles pay for).
        // Tiles of 64 period rows (69 staged rows) have no lane above lane 63 to shift from: every lane reads its NR rows itself (the
        // bf16 pair tile's rows lie 138 words apart, a two-way conflict): NR x NC LDS reads and two VALU instructions per pair to
        // rebuild it, against NC reads and (NR - 1) x NC x 2 shifts.  Not measured on its own: the edge tiles' time is part of the
        // interior kernel's, which was measured whole (profiles/quad2_bf16_tile/).
        static_assert(Cfg::kLdsRows <= 64 || Cfg::kTileRows + NR - 1 <= Cfg::kLdsRows, "one tile row per lane");
        const W* wp = tile + ((lane < Cfg::kLdsRows ? lane : 0) * Cfg::kLdsPitch + a.edge.lds_col[s]) * ES;
        V w[NR][NC];
#pragma unroll
        for (int lx = 0; lx < NC; ++lx) w[0][lx] = quad2_pair_of(wp[lx * ES]);
#pragma unroll
        for (int ly = 1; ly < NR; ++ly)
#pragma unroll
            for (int lx = 0; lx < NC; ++lx) {
                if constexpr (Cfg::kLdsRows <= 64) w[ly][lx] = wave_shl1(w[ly - 1][lx]);
                else w[ly][lx] = quad2_pair_of(wp[(ly * Cfg::kLdsPitch + lx) * ES]);
            }
        const uint32_t row_off = static_cast<uint32_t>(a.iy0 + 2 * (j0 + lane) + q) * static_cast<uint32_t>(io.dst_pitch);
        for (int k0 = k_begin; k0 < k_end; k0 += 4) {  // wave-uniform
            const int nk = k_end - k0 < 4 ? k_end - k0 : 4;
            V r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                r[k] = V{};
                if (k < nk) {  // wave-uniform
                    const JINC_CONSTANT float* cs = (const JINC_CONSTANT float*)(a.edge.coeffs) + ((s * PeriodicArgs::EdgeColumns::kMaxPerSide + k0 + k) * 2 + q) * (NR * NCP);
                    V acc = V{};
#pragma unroll
                    for (int ly = 0; ly < NR; ++ly)
#pragma unroll
                        for (int lx = 0; lx < NC; ++lx) acc = acc + w[ly][lx] * cs[ly * NCP + lx];
                    r[k] = acc;
                }
            }
            if (!live) continue;
            const uint32_t voff = row_off + static_cast<uint32_t>(a.edge.x0[s] + k0) * static_cast<uint32_t>(sizeof(T));
            auto store = [&](BufferRsrc d, auto frame) {
                if (nk == 4) {
                    if constexpr (std::is_same_v<T, uint8_t>) {
                        uint32_t v = __builtin_amdgcn_cvt_pk_u8_f32(frame(r[0]), 0u, 0u);
                        v = __builtin_amdgcn_cvt_pk_u8_f32(frame(r[1]), 1u, v);
                        v = __builtin_amdgcn_cvt_pk_u8_f32(frame(r[2]), 2u, v);
                        v = __builtin_amdgcn_cvt_pk_u8_f32(frame(r[3]), 3u, v);
                        __builtin_amdgcn_raw_buffer_store_b32(v, d, voff, 0, 0);
                    } else {
                        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
                        const u32x2 v = {round_pair_u16(frame(r[0]), frame(r[1]), io.peak), round_pair_u16(frame(r[2]), frame(r[3]), io.peak)};
                        __builtin_amdgcn_raw_buffer_store_b64(v, d, voff, 0, 0);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        if (k < nk) store_sample_buf<T>(d, voff + static_cast<uint32_t>(k * sizeof(T)), 0, frame(r[k]), io.peak);
                }
            };
            store(drsrc, [](V v) { return frame_lo(v); });
            if constexpr (kPair) {
                if (hi_ok) store(drsrc_hi, [](V v) { return frame_hi(v); });
            }
        }
    }
}

