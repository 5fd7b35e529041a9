// kernel_periodic_quad2.inc -- one translation unit of the periodic interior kernel in quad form with two periods per lane on the
// trimmed 6-row support (2x up-scales with tap 3, integer planes and finite float planes): ewa_periodic_quad2_kernel on tiles of
// JINC_QUAD2_RG row groups (kernel_periodic_quad2_rg8.hip: long batches, kernel_periodic_quad2_rg4.hip: short ones), launched by
// JINC_QUAD2_LAUNCH.  Two units because the frame-pair walks are unrolled whole: together they compile longer than all other
// periodic kernels.
//   per-frame body   Quad2Cfg, the 6-tap rows quad2_row6 / quad2_row6_inner, the 7-tap rows quad2_row7 / quad2_row7_span (6 rows x 7
//                    columns: chroma sited as MPEG-2), quad2_load_row, quad2_pixel6
//   frame-pair body  quad2_share_body on Quad2ShareTile: one product per (source sample, symmetry class), strips of 2 / 8 / 16 period
//                    rows (quad2_share_strip; quad2_share_walk16 over the bf16 pair tile of 8-bit planes)
// and launch_periodic_quad2_t.  The four-sample store, the edge columns, the coefficient fetches and the packed-multiply macros are
// shared with kernel_periodic_quad2x8.hip: kernel_periodic_quad_common.inc.  See kernel_periodic.hip for the family,
// device_common.hpp for the parity rules.
#include "device_common.hpp"
#include "kernel_periodic_launch.h"
#include "knobs.h"
#include <utility>

#pragma clang fp contract(off)

namespace jinc {
namespace {

#include "kernel_periodic_common.inc"
#include "kernel_periodic_quad_common.inc"

// ------------------------------------------------------------------------------------------------
// Periodic interior kernel, quad form on a trimmed 6 x 6 support, two periods per lane
// ------------------------------------------------------------------------------------------------
// Integer planes whose coefficient sets carry exact zeros along the window's edge run on the trimmed support (host:
// device_plan.cpp, trim_periodic): the 2x up-scale with tap 3 has filter size 7, but the first kernel row and column of all
// four phase sets are 0.0f (the EWA disc of radius 3.24 spans six samples at these phases), and a tap whose coefficient is
// zero adds +0 to a chain that is never -0 -- leaving it out is exact for finite samples, which integer samples are.
// 36 taps per sample instead of 49.
// The lane mapping changes with it: a lane owns TWO horizontally adjacent periods -- 4 x 2 output samples from ONE
// 6 x 7 register window (the periods' windows are one source column apart).  Against ewa_periodic_quad_kernel, per output
// sample: half the coefficient fetches (one SGPR pair feeds both periods: the scalar cache delivered two s_load_dwordx16
// per 784 issue cycles and wave there, now two per 1152), window rows as four aligned ds_read_b64 per eight samples
// instead of seven ds_read_b32 per four, four independent chains per lane interleaved two by two, and the four 8-bit
// samples of a row leave as one dword store.  Every chain still meets its taps in (ly, lx) order, multiply and add un-fused.
// Coefficient layout: as the fs-7 quad form, quad[ly][q][8 pairs][p] with pairs 6 and 7 unused.
template <int RG>
struct Quad2Cfg {
    static constexpr int FS = 6;
    static constexpr int kPeriodsPerLane = 2;
    static constexpr int kTileCols = 64 * kPeriodsPerLane;  // periods per tile row
    static constexpr int kTileRows = FS * RG;               // period-rows per tile
    static constexpr int kLdsCols = kTileCols + FS;         // lane 63 reads columns 126 .. 133
    static constexpr int kLdsPitch = 136;                   // even: every lane's row segment is 8-byte aligned
    static constexpr int kLdsRows = kTileRows + FS - 1;
};

// One kernel row of one q for both periods of a lane: window pairs w0..w3 = source columns 0..7 of the row (period A
// reads columns 0..5, period B columns 1..6), coefficient pairs c0..c5 = (p = 0, p = 1) of taps 0..5.
__device__ __forceinline__ void quad2_row6(f32x2& acc_a, f32x2& acc_b, f32x2 w0, f32x2 w1, f32x2 w2, f32x2 w3, f32x2 c0, f32x2 c1, f32x2 c2,
                                           f32x2 c3, f32x2 c4, f32x2 c5) {
    f32x2 ta, tb;
    asm(JINC_LO("%2", "%4", "%8") JINC_HI("%3", "%4", "%8") JINC_ADD2      // tap 0: A column 0, B column 1
        JINC_HI("%2", "%4", "%9") JINC_LO("%3", "%5", "%9") JINC_ADD2      // tap 1: A 1, B 2
        JINC_LO("%2", "%5", "%10") JINC_HI("%3", "%5", "%10") JINC_ADD2    // tap 2: A 2, B 3
        JINC_HI("%2", "%5", "%11") JINC_LO("%3", "%6", "%11") JINC_ADD2    // tap 3: A 3, B 4
        JINC_LO("%2", "%6", "%12") JINC_HI("%3", "%6", "%12") JINC_ADD2    // tap 4: A 4, B 5
        JINC_HI("%2", "%6", "%13") JINC_LO("%3", "%7", "%13")              // tap 5: A 5, B 6
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3"
        : "+v"(acc_a), "+v"(acc_b), "=&v"(ta), "=&v"(tb)
        : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "s"(c0), "s"(c1), "s"(c2), "s"(c3), "s"(c4), "s"(c5));
}

// Seven taps per kernel row for both periods of a lane (the 6-row x 7-column support: chroma planes sited as MPEG-2 at 2x): period A
// reads columns 0 .. 6, period B columns 1 .. 7 of the same four register pairs.
__device__ __forceinline__ void quad2_row7(f32x2& acc_a, f32x2& acc_b, f32x2 w0, f32x2 w1, f32x2 w2, f32x2 w3, f32x2 c0, f32x2 c1, f32x2 c2, f32x2 c3, f32x2 c4, f32x2 c5, f32x2 c6) {
    f32x2 ta, tb;
    asm("v_pk_mul_f32 %2, %4, %8 op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %3, %4, %8 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3\n\t"
        "v_pk_mul_f32 %2, %4, %9 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_mul_f32 %3, %5, %9 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3\n\t"
        "v_pk_mul_f32 %2, %5, %10 op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %3, %5, %10 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3\n\t"
        "v_pk_mul_f32 %2, %5, %11 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_mul_f32 %3, %6, %11 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3\n\t"
        "v_pk_mul_f32 %2, %6, %12 op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %3, %6, %12 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3\n\t"
        "v_pk_mul_f32 %2, %6, %13 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_mul_f32 %3, %7, %13 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3\n\t"
        "v_pk_mul_f32 %2, %7, %14 op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %3, %7, %14 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3"
        : "+v"(acc_a), "+v"(acc_b), "=&v"(ta), "=&v"(tb)
        : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "s"(c0), "s"(c1), "s"(c2), "s"(c3), "s"(c4), "s"(c5), "s"(c6));
}

// The same kernel row where tap 0 and tap 5 carry zero coefficients for BOTH phases p of this q (the disc's chord in the box's
// first / last row: host, PeriodicArgs::quad_inner): taps 1 .. 4 only.
__device__ __forceinline__ void quad2_row6_inner(f32x2& acc_a, f32x2& acc_b, f32x2 w0, f32x2 w1, f32x2 w2, f32x2 c1, f32x2 c2, f32x2 c3, f32x2 c4) {
    f32x2 ta, tb;
    asm(JINC_HI("%2", "%4", "%7") JINC_LO("%3", "%5", "%7") JINC_ADD2      // tap 1: A column 1, B column 2
        JINC_LO("%2", "%5", "%8") JINC_HI("%3", "%5", "%8") JINC_ADD2      // tap 2: A 2, B 3
        JINC_HI("%2", "%5", "%9") JINC_LO("%3", "%6", "%9") JINC_ADD2      // tap 3: A 3, B 4
        JINC_LO("%2", "%6", "%10") JINC_HI("%3", "%6", "%10")              // tap 4: A 4, B 5
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3"
        : "+v"(acc_a), "+v"(acc_b), "=&v"(ta), "=&v"(tb)
        : "v"(w0), "v"(w1), "v"(w2), "s"(c1), "s"(c2), "s"(c3), "s"(c4));
}

// quad2_row7 on a span of its taps: the chord of a (kernel row, q) of the 6-row x 7-column support -- form 1 = taps 1 .. 6, 2 = taps
// 1 .. 5, 3 = taps 2 .. 5 (form 0: all seven, quad2_row7) -- for rows whose other taps carry zero coefficients for BOTH phases p.
// Chroma planes sited as MPEG-2 at 2x with tap 3: 36 of the 42 taps per sample (PeriodicArgs::kQuadSpan7Mpeg2).
#define JINC_Q7_EVEN(W, C) /* tap t even: period A = the low half of pair t / 2, B its high half */                         \
    "v_pk_mul_f32 %2, " W ", " C " op_sel_hi:[0,1]\n\tv_pk_mul_f32 %3, " W ", " C " op_sel:[1,0] op_sel_hi:[1,1]\n\t" \
    "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3\n\t"
#define JINC_Q7_ODD(W, WN, C) /* tap t odd: A = the high half of pair t / 2, B the low half of the next pair */             \
    "v_pk_mul_f32 %2, " W ", " C " op_sel:[1,0] op_sel_hi:[1,1]\n\tv_pk_mul_f32 %3, " WN ", " C " op_sel_hi:[0,1]\n\t" \
    "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3\n\t"
template <int FORM>
__device__ __forceinline__ void quad2_row7_span(f32x2& acc_a, f32x2& acc_b, f32x2 w0, f32x2 w1, f32x2 w2, f32x2 w3, f32x2 c0, f32x2 c1, f32x2 c2, f32x2 c3,
                                                f32x2 c4, f32x2 c5, f32x2 c6) {
    static_assert(FORM >= 0 && FORM <= 3, "span forms of the seven-tap row");
    f32x2 ta, tb;
    if constexpr (FORM == 0) {
        quad2_row7(acc_a, acc_b, w0, w1, w2, w3, c0, c1, c2, c3, c4, c5, c6);
    } else if constexpr (FORM == 1) {  // taps 1 .. 6
        asm(JINC_Q7_ODD("%4", "%5", "%8") JINC_Q7_EVEN("%5", "%9") JINC_Q7_ODD("%5", "%6", "%10") JINC_Q7_EVEN("%6", "%11")
            JINC_Q7_ODD("%6", "%7", "%12") JINC_Q7_EVEN("%7", "%13") ""
            : "+v"(acc_a), "+v"(acc_b), "=&v"(ta), "=&v"(tb)
            : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "s"(c1), "s"(c2), "s"(c3), "s"(c4), "s"(c5), "s"(c6));
    } else if constexpr (FORM == 2) {  // taps 1 .. 5
        asm(JINC_Q7_ODD("%4", "%5", "%8") JINC_Q7_EVEN("%5", "%9") JINC_Q7_ODD("%5", "%6", "%10") JINC_Q7_EVEN("%6", "%11")
            JINC_Q7_ODD("%6", "%7", "%12") ""
            : "+v"(acc_a), "+v"(acc_b), "=&v"(ta), "=&v"(tb)
            : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "s"(c1), "s"(c2), "s"(c3), "s"(c4), "s"(c5));
    } else {                           // taps 2 .. 5
        asm(JINC_Q7_EVEN("%4", "%7") JINC_Q7_ODD("%4", "%5", "%8") JINC_Q7_EVEN("%5", "%9") JINC_Q7_ODD("%5", "%6", "%10") ""
            : "+v"(acc_a), "+v"(acc_b), "=&v"(ta), "=&v"(tb)
            : "v"(w1), "v"(w2), "v"(w3), "s"(c2), "s"(c3), "s"(c4), "s"(c5));
    }
}
#undef JINC_Q7_EVEN
#undef JINC_Q7_ODD

#undef JINC_LO
#undef JINC_HI
#undef JINC_ADD2

// Window slot SLOT <- eight source columns of one tile row (four aligned ds_read_b64).
template <int SLOT>
__device__ __forceinline__ void quad2_load_row(f32x2 (&w)[24], const float* p) {
    const f32x2* p2 = reinterpret_cast<const f32x2*>(p);
#pragma unroll
    for (int m = 0; m < 4; ++m) w[4 * SLOT + m] = p2[m];
}

// One output row pair of both periods: acc[0] / acc[1] = period A / B at q = 0, acc[2] / acc[3] at q = 1.  Coefficient pairs of
// kernel row ly + 1 are requested before the taps of row ly are issued, as in quad_pixel7.
template <int U, uint32_t INNER, int NT>
__device__ __forceinline__ void quad2_pixel6(f32x2 (&acc)[4], const f32x2 (&w)[24], const JINC_CONSTANT f32x2* quad) {
    f32x2 ca[16], cb[16];
    quad_fetch(ca, quad, 0);
#define JINC_QUAD2_STEP(LY, CUR, NEXT)                                                                                        \
    if constexpr (LY < 5) quad_fetch(NEXT, quad, LY + 1);                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                                                         \
    quad_arrived(CUR);                                                                                                         \
    {                                                                                                                          \
        constexpr int S = 4 * ((U + LY) % 6);                                                                                  \
        /* INNER: a compile-time mask (a run-time test here, however uniform, cost 8 % of the kernel: round4/quad_inner_ab.log) */ \
        if constexpr (NT == 7) { /* 6 rows x 7 columns: seven taps per kernel row */                                            \
            /* (NT == 7: INNER holds the span form of every (kernel row, q), two bits each) */                              \
            quad2_row7_span<(INNER >> (2 * (2 * LY))) & 3u>(acc[0], acc[1], w[S], w[S + 1], w[S + 2], w[S + 3], CUR[0], CUR[1], CUR[2], CUR[3], CUR[4], CUR[5], CUR[6]); \
            quad2_row7_span<(INNER >> (2 * (2 * LY + 1))) & 3u>(acc[2], acc[3], w[S], w[S + 1], w[S + 2], w[S + 3], CUR[8], CUR[9], CUR[10], CUR[11], CUR[12], CUR[13], CUR[14]); \
        } else {                                                                                                               \
        if constexpr ((INNER >> (2 * LY)) & 1u)                                                                                \
            quad2_row6_inner(acc[0], acc[1], w[S], w[S + 1], w[S + 2], CUR[1], CUR[2], CUR[3], CUR[4]);                        \
        else                                                                                                                   \
            quad2_row6(acc[0], acc[1], w[S], w[S + 1], w[S + 2], w[S + 3], CUR[0], CUR[1], CUR[2], CUR[3], CUR[4], CUR[5]);    \
        if constexpr ((INNER >> (2 * LY + 1)) & 1u)                                                                            \
            quad2_row6_inner(acc[2], acc[3], w[S], w[S + 1], w[S + 2], CUR[9], CUR[10], CUR[11], CUR[12]);                     \
        else                                                                                                                   \
            quad2_row6(acc[2], acc[3], w[S], w[S + 1], w[S + 2], w[S + 3], CUR[8], CUR[9], CUR[10], CUR[11], CUR[12], CUR[13]); \
        }                                                                                                                      \
    }                                                                                                                          \
    __builtin_amdgcn_sched_barrier(0);
    JINC_QUAD2_STEP(0, ca, cb)
    JINC_QUAD2_STEP(1, cb, ca)
    JINC_QUAD2_STEP(2, ca, cb)
    JINC_QUAD2_STEP(3, cb, ca)
    JINC_QUAD2_STEP(4, ca, cb)
    JINC_QUAD2_STEP(5, cb, ca)
#undef JINC_QUAD2_STEP
}

// ------------------------------------------------------------------------------------------------
// The same interior on frame pairs, one product per (source sample, symmetry class) (integer planes, kQuad2InnerTap3)
// ------------------------------------------------------------------------------------------------
// The reference computes every output as its own chain of un-fused acc = acc + sample * coeff in (ly, lx) order.  That fixes each
// chain's adds and the value of each product, not where the product is computed: fl(s * c) depends on the bits of s and c alone, so
// one product added into several chains is bit-identical to a product per chain.  At exactly 2x the outputs sit +-1/4 and +-3/4 of
// a source step from the samples and a coefficient depends on the unordered pair of distance classes (kernels.h quad2_share_class;
// the host checks the plan's four phase sets against it, PeriodicArgs::quad_share): a product sample * w(class) is needed by every
// output at that class's distance, in the period rows above and below the lane's as much as in its own.  A lane owns a strip 2
// periods across and H period rows down = 4 x 2H outputs of TWO frames (the packed halves: frames 2z and 2z + 1, each source sample
// staged as one f32x2) and walks the strip's 7-column x (H + 5)-row source window row by row, left to right: per (sample, class) an
// open chain needs, one v_pk_mul_f32 (the class coefficient broadcast from an SGPR by op_sel), then one v_pk_add_f32 into each chain
// that takes it.  Period row j opens at source row j and is complete after source row j + 5: it is stored there, and its registers
// serve period row j + 6 (the walk is unrolled whole, so at most six period rows = 48 packed accumulators are live).  Every chain
// still meets its taps in (ly, lx) order: ly and lx grow with the source row and column.  Three taps per row phase are zero (leaving
// them out is exact for integer samples, see Quad2Cfg).  The last pair of an odd frame count stages the low frame twice and stores
// it once.  Per output pair the per-frame form above issues 34 multiplies + 34 adds, strips of H = 2 (2 x 2-period blocks)
// 21.9 + 31, strips of H = 8 15.5 + 31; a chain's first product opens it (quad2_share_adds), so one add of the 31 is not issued.
//   Full tiles (RG 8, long batches; 16-bit planes): 128 x 32 periods, one strip of 8 period rows per wave, 37 staged rows of f32 pairs (40.9 KB of
// LDS: four workgroups per CU, as many as the 96 live accumulators leave waves per SIMD).  Its products come one class at a time,
// the adds of each behind the next multiply: all of a sample's products at once would not fit beside the accumulators.
//   Half tiles (RG 4, short batches): 128 x 16 periods, two strips of 2 period rows per wave (23.2 KB, six workgroups per CU), all
// of a sample's products in front of their adds, so that no add waits on the multiply just issued.
//   8-bit full tiles (Bf16): a sample 0 .. 255 is exact in bfloat16, and a bf16 over 16 zero bits is that sample's f32.  The tile
// holds one 32-bit word per pair (the low frame's bf16 in the low half), 128 x 64 periods, one strip of 16 period rows per wave,
// 69 staged rows in 38.1 KB: still four workgroups per CU, and the strip's end rows (their samples serve fewer period rows) are
// paid once per 128 output pairs, 13.4 products per pair.  The walk reads each half with ds_read_u16_d16_hi into a register whose
// low half was zeroed once (quad2_share_walk16): the window arrives as f32 pairs with no VALU instruction per sample.
template <int H, int StripsPerWave, int MulLead, bool Bf16 = false>
struct Quad2ShareTile {
    static constexpr bool kBf16 = Bf16;
    using Word = std::conditional_t<Bf16, uint32_t, f32x2>;  // one staged pair
    using Half = std::conditional_t<Bf16, uint16_t, float>;  // one frame's half of it: the staging writes halves, frame f's at [2 * pair + f]
    static __device__ __forceinline__ Half half_of(float v) {
        if constexpr (Bf16) return static_cast<uint16_t>(__builtin_bit_cast(uint32_t, v) >> 16);
        else return v;
    }
    static constexpr int kTileCols = 128;                    // periods per tile row (Quad2Cfg's: the edge columns' tile_x)
    static constexpr int kStripRows = H;                     // period rows per strip
    static constexpr int kStripsPerWave = StripsPerWave;     // strips per lane, one below the other
    static constexpr int kMulLead = MulLead;                 // multiplies issued ahead of the adds that take them
    static constexpr int kTileRows = 4 * H * StripsPerWave;  // period rows per tile
    static constexpr int kLdsCols = kTileCols + 6;           // (pairs) as Quad2Cfg: the edge columns' windows reach column 133
    static constexpr int kLdsSpare = 4;                      // pairs between the rows: what the staging's dwords hold beside the row,
    static constexpr int kLdsPitch = kLdsCols + kLdsSpare;   // and column -1 of the next row (pairs: rows 16-byte aligned)
    static constexpr int kLdsRows = kTileRows + 5;
    static constexpr int kLdsFloats = (Bf16 ? 1 : 2) * (kLdsSpare + kLdsRows * kLdsPitch);  // the spare pairs in front of row 0 too
    static_assert(kLdsPitch % 2 == 0 && kLdsSpare % 2 == 0, "16-byte aligned rows");
    static_assert(H <= Quad2ShareOuts::kMaxStripRows, "a strip's outputs index one Quad2ShareOuts");
    static_assert(!Bf16 || (StripsPerWave == 1 && MulLead == 1), "quad2_share_walk16");
};
// Full tiles (RG 8) of 8-bit planes take the bf16 pair tile and strips of 16; 16-bit samples do not fit bf16.
template <typename T, int RG>
using Quad2ShareCfg = std::conditional_t<RG == 8, std::conditional_t<sizeof(T) == 1, Quad2ShareTile<16, 1, 1, true>, Quad2ShareTile<8, 1, 1>>,
                                         Quad2ShareTile<2, 2, kQuad2ShareClasses>>;

// Both launcher and kernel: does this launch of the integer kInnerTap3 instance (launched for plans with quad_share only) run the
// frame-pair form?  The full-tile instance (RG 8: long batches) has no other body -- the per-frame form's window and tile would cost
// it registers and LDS; the half-tile one (RG 4) keeps the per-frame form for single frames, where a pair's second half is wasted.
template <int RG>
__host__ __device__ inline bool quad2_share_runs(const PlaneIO& io) { return RG == 8 || io.nframes > 1; }

// The strip's outputs that take sample (r, c) of its window with a coefficient of class k: kernels.h quad2_share_outs.
// The outputs among quad2_share_outs(r, c, k) whose chain sample (r, c) opens: it is their first tap with a non-zero coefficient.
template <int H>
constexpr Quad2ShareOuts quad2_share_opens(int r, int c, int k) {
    const Quad2ShareOuts outs = r < H ? quad2_share_outs<H>(r, c, k) : Quad2ShareOuts{};
    Quad2ShareOuts m;
    for (int o = 8 * r; outs.any() && o < 8 * r + 8; ++o) {  // period row r's outputs: their kernel row 0 is source row r
        if (!outs.has(o)) continue;
        const int p = o & 1, q = (o >> 2) & 1, lx = c - ((o & 3) >> 1);
        bool first = true;
        for (int l = 0; l < lx; ++l) first = first && quad2_share_class(quad2_share_m(p, l), quad2_share_m(q, 0)) < 0;
        if (first) m.set(o);
    }
    return m;
}
constexpr bool quad2_share_row0_opens(int p, int q) {  // kernel row 0 has a non-zero tap: every chain opens in its first source row
    for (int l = 0; l < 6; ++l)
        if (quad2_share_class(quad2_share_m(p, l), quad2_share_m(q, 0)) >= 0) return true;
    return false;
}
static_assert(quad2_share_row0_opens(0, 0) && quad2_share_row0_opens(1, 0) && quad2_share_row0_opens(0, 1) && quad2_share_row0_opens(1, 1),
              "no accumulator is zeroed: the first source row of a period row must open all eight of its chains");

// Sample (R, C) times class K (the high / low half of SGPR pair K / 2, for both frames), where the strip needs that product.
template <int H, int R, int C, int K>
__device__ __forceinline__ void quad2_share_mul(f32x2& t, f32x2 s, const f32x2 (&w)[kQuad2ShareClasses / 2]) {
    if constexpr (quad2_share_outs<H>(R, C, K).any()) {
        if constexpr (K & 1)
            asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(t) : "v"(s), "s"(w[K >> 1]));
        else
            asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(t) : "v"(s), "s"(w[K >> 1]));
    }
}
// ... added into every chain that takes it.  A chain that this product opens takes the product itself: no accumulator is zeroed and
// no 0 + p is added.  The opening chains come last, so the product's register becomes the accumulator of one of them without a move
// (a product that opens several chains is copied for the others).  p and 0 + p differ only for p = -0 (a zero sample times a negative
// coefficient).  A partial sum of -0 behaves as +0 in every later add, except that a chain of nothing but zero products may end as -0
// where it ended as +0: the integer stores (v_cvt_pk_u8_f32, round_pair16) write 0 for both.  Float planes would keep the sign, and
// do not run this body (quad2_share_instance).
template <int H, int R, int C, int K>
__device__ __forceinline__ void quad2_share_adds(f32x2 (&acc)[8 * H], f32x2 t) {
    constexpr Quad2ShareOuts outs = quad2_share_outs<H>(R, C, K), opens = quad2_share_opens<H>(R, C, K);
#pragma unroll
    for (int o = 0; o < 8 * H; ++o)
        if constexpr (outs.any())
            if (outs.has(o) && !opens.has(o)) asm("v_pk_add_f32 %0, %0, %1" : "+v"(acc[o]) : "v"(t));
#pragma unroll
    for (int o = 0; o < 8 * H; ++o)
        if constexpr (opens.any())
            if (opens.has(o)) acc[o] = t;
}
// Step K of a sample: the multiply of class K, then the adds of class K - kMulLead.
template <typename Cfg, int R, int C, int K>
__device__ __forceinline__ void quad2_share_step(f32x2 (&acc)[8 * Cfg::kStripRows], f32x2 (&t)[kQuad2ShareClasses], f32x2 s,
                                                 const f32x2 (&w)[kQuad2ShareClasses / 2]) {
    if constexpr (K < kQuad2ShareClasses) quad2_share_mul<Cfg::kStripRows, R, C, K>(t[K], s, w);
    if constexpr (K >= Cfg::kMulLead) quad2_share_adds<Cfg::kStripRows, R, C, K - Cfg::kMulLead>(acc, t[K - Cfg::kMulLead]);
}
template <typename Cfg, int R, int C, int... K>
__device__ __forceinline__ void quad2_share_sample(f32x2 (&acc)[8 * Cfg::kStripRows], f32x2 s, const f32x2 (&w)[kQuad2ShareClasses / 2],
                                                   std::integer_sequence<int, K...>) {
    f32x2 t[kQuad2ShareClasses];
    (quad2_share_step<Cfg, R, C, K>(acc, t, s, w), ...);
}
// Source row R of the strip's window: pairs row[0 .. 6] = columns 0 .. 6 (row[7] is loaded with them and unused).  Period row R's chains open here (quad2_share_adds).
template <typename Cfg, int R, int... C>
__device__ __forceinline__ void quad2_share_row(f32x2 (&acc)[8 * Cfg::kStripRows], const f32x2* wb, const f32x2 (&w)[kQuad2ShareClasses / 2],
                                                std::integer_sequence<int, C...>) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const f32x4* p4 = reinterpret_cast<const f32x4*>(wb + R * Cfg::kLdsPitch);
    f32x2 row[8];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const f32x4 v = p4[m];
        row[2 * m] = f32x2{v.x, v.y};
        row[2 * m + 1] = f32x2{v.z, v.w};
    }
    (quad2_share_sample<Cfg, R, C>(acc, row[C], w, std::make_integer_sequence<int, kQuad2ShareClasses + Cfg::kMulLead>{}), ...);
}
// The whole strip, source rows 0 .. H + 4: after row R, period row R - 5 is complete and leaves by store(integral_constant<R - 5>).
template <typename Cfg, int... R, typename Store>
__device__ __forceinline__ void quad2_share_strip(f32x2 (&acc)[8 * Cfg::kStripRows], const f32x2* wb, const f32x2 (&w)[kQuad2ShareClasses / 2],
                                                  std::integer_sequence<int, R...>, Store&& store) {
    ((quad2_share_row<Cfg, R>(acc, wb, w, std::make_integer_sequence<int, 7>{}), store(std::integral_constant<int, R - 5>{})), ...);
}

// The same walk over the bf16 pair tile.  Window column C lives in s[C]: two registers whose low halves are zero from the start of the
// strip and stay zero -- ds_read_u16_d16_hi writes the high half and keeps the low one (or, on parts with SRAM ECC, writes zero
// there: the same thing here, and the only value of the low half this code may rely on) -- each register is the sample's f32 as loaded.
// What the compiler does not know: between the load asm and the matching s_waitcnt asm, up to a row later, s[C] is NOT yet defined,
// although the asm's output says so.  A copy, a re-pairing move or a spill of s[C] placed in between would read stale data without any
// warning.  Today's listing has none (the only moves of the walk zero the registers, in front of the first wait; every wait is one of
// these); tests/test_quad2_bf16_tile.py holds the listing to that, and the GPU tests compare every byte.  Sample
// (R + 1, C) is loaded into s[C] behind the last product of sample (R, C), so 14 loads are in flight all the time and sample (R, C)
// waits for its own two only: LDS loads return in order, and the twelve issued behind them are columns C + 1 .. 6 of row R and columns
// 0 .. C - 1 of row R + 1 (none of the latter in the last row).  The compiler does not count loads issued by inline assembly, hence the
// s_waitcnt here; whatever else is in flight on that counter only makes the wait longer.
template <typename Cfg, int R, int C>
__device__ __forceinline__ void quad2_share_load16(float (&s)[2], uint32_t at) {
    constexpr int off = 4 * (R * Cfg::kLdsPitch + C);
    static_assert(off + 2 < 65536, "the offset field");
    asm volatile("ds_read_u16_d16_hi %0, %2 offset:%3\n\tds_read_u16_d16_hi %1, %2 offset:%4"
                 : "+v"(s[0]), "+v"(s[1])
                 : "v"(at), "n"(off), "n"(off + 2)
                 : "memory");
}
template <typename Cfg, int R, int C>
__device__ __forceinline__ void quad2_share_sample16(f32x2 (&acc)[8 * Cfg::kStripRows], float (&s)[7][2], uint32_t at,
                                                     const f32x2 (&w)[kQuad2ShareClasses / 2]) {
    constexpr bool last = R == Cfg::kStripRows + 4;
    constexpr int behind = 2 * ((6 - C) + (last ? 0 : C));
    asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(s[C][0]), "+v"(s[C][1]) : "n"(behind));
    quad2_share_sample<Cfg, R, C>(acc, f32x2{s[C][0], s[C][1]}, w, std::make_integer_sequence<int, kQuad2ShareClasses + Cfg::kMulLead>{});
    if constexpr (!last) quad2_share_load16<Cfg, R + 1, C>(s[C], at);
}
template <typename Cfg, int R, int... C>
__device__ __forceinline__ void quad2_share_row16(f32x2 (&acc)[8 * Cfg::kStripRows], float (&s)[7][2], uint32_t at,
                                                  const f32x2 (&w)[kQuad2ShareClasses / 2], std::integer_sequence<int, C...>) {
    (quad2_share_sample16<Cfg, R, C>(acc, s, at, w), ...);
}
template <typename Cfg, int... C>
__device__ __forceinline__ void quad2_share_open16(float (&s)[7][2], uint32_t at, std::integer_sequence<int, C...>) {
    (quad2_share_load16<Cfg, 0, C>(s[C], at), ...);
}
template <typename Cfg, int... R, typename Store>
__device__ __forceinline__ void quad2_share_walk16(f32x2 (&acc)[8 * Cfg::kStripRows], const uint32_t* wb, const f32x2 (&w)[kQuad2ShareClasses / 2],
                                                   std::integer_sequence<int, R...>, Store&& store) {
    const uint32_t at = static_cast<uint32_t>(reinterpret_cast<uintptr_t>((const __attribute__((address_space(3))) uint32_t*)wb));
    float s[7][2] = {};
    quad2_share_open16<Cfg>(s, at, std::make_integer_sequence<int, 7>{});
    ((quad2_share_row16<Cfg, R>(acc, s, at, w, std::make_integer_sequence<int, 7>{}), store(std::integral_constant<int, R - 5>{})), ...);
}

template <typename T, int RG>
__device__ __forceinline__ void quad2_share_body(const PeriodicArgs& a, const PlaneIO& io, float* lds) {
    using Cfg = Quad2ShareCfg<T, RG>;
    using Word = typename Cfg::Word;
    Word* const tile = reinterpret_cast<Word*>(lds) + Cfg::kLdsSpare;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int tile_x, tile_y;
    swizzled_tile(tile_x, tile_y);
    const int i0 = tile_x * Cfg::kTileCols;
    const int j0 = tile_y * Cfg::kTileRows;
    const size_t f0 = 2 * static_cast<size_t>(blockIdx.z);
    const bool f1_ok = f0 + 1 < static_cast<size_t>(io.nframes);  // the last pair of an odd count: the high half repeats the low frame
    const size_t f1 = f1_ok ? f0 + 1 : f0;
    const bool edge_tile = edge_tile_of<T>(a, tile_x);
    {   // Stage both frames' source tiles as pairs (f32, or the high halves of the f32: Cfg::half_of), all loads in front of the LDS writes (see ewa_periodic_kernel).  A lane loads
        // the aligned dword(s) that hold four samples of a row, through a descriptor over the frame's plane (widened to whole dwords:
        // an aligned dword lies in one page, and a dword past the plane's last one reads as zero), the row's offset in an SGPR.  The
        // dword that holds the tile's first sample starts up to three samples in front of it: the row lands that far to the left in
        // the tile (a wave-uniform shift per row and frame, whatever the pitch), and the samples in front of column 0 or behind
        // column kLdsCols - 1 fall into the spare pairs between the rows.
        const int gx0 = a.min_sx + i0;
        const int gy0 = a.min_sy + j0;
        const char* sb0 = static_cast<const char*>(io.src) + f0 * io.src_frame_stride;
        const char* sb1 = static_cast<const char*>(io.src) + f1 * io.src_frame_stride;
        constexpr int kRowsPerWave = (Cfg::kLdsRows + 3) / 4;
        constexpr int kDwords = static_cast<int>(sizeof(T));              // per lane and row: four samples
        constexpr int kLoadLanes = (Cfg::kLdsCols + 3 + 3) / 4;           // the shifted row's dwords (x kDwords)
        static_assert(kLoadLanes <= 64 && 4 * (kLoadLanes - 1) < Cfg::kLdsPitch - 1 && 4 * (kLoadLanes - 2) + 3 < Cfg::kLdsPitch - 1 && Cfg::kLdsSpare > 3,
                      "the last lane's first sample, the other lanes' four and the three samples in front of a row: spare pairs, not the next row's column -1");
        const uint32_t plane_bytes = static_cast<uint32_t>(a.src_h - 1) * static_cast<uint32_t>(io.src_pitch) + static_cast<uint32_t>(a.src_w) * static_cast<uint32_t>(sizeof(T));
        const uint32_t lead0 = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(sb0)) & 3u, lead1 = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(sb1)) & 3u;
        const BufferRsrc rs0 = make_rsrc(const_cast<char*>(sb0) - lead0, (plane_bytes + lead0 + 3u) & ~3u);  // wave-uniform
        const BufferRsrc rs1 = make_rsrc(const_cast<char*>(sb1) - lead1, (plane_bytes + lead1 + 3u) & ~3u);
        const uint32_t lead[2] = {lead0, lead1};
        const uint32_t voff = static_cast<uint32_t>(lane) * (4u * kDwords);
        uint32_t d[kRowsPerWave][2][kDwords];
        int shift[kRowsPerWave][2];  // samples, wave-uniform
#pragma unroll
        for (int i = 0; i < kRowsPerWave; ++i) {
            int gy = gy0 + wave + 4 * i;
            gy = gy < a.src_h ? gy : a.src_h - 1;
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                const uint32_t so = lead[f] + static_cast<uint32_t>(gy) * static_cast<uint32_t>(io.src_pitch) + static_cast<uint32_t>(gx0) * static_cast<uint32_t>(sizeof(T));
                shift[i][f] = static_cast<int>((so & 3u) / sizeof(T));
#pragma unroll
                for (int k = 0; k < kDwords; ++k) d[i][f][k] = __builtin_amdgcn_raw_buffer_load_b32(f ? rs1 : rs0, voff + 4u * k, so & ~3u, 0);
            }
        }
        // (the lane's first pair as a pointer of its own: what indexes it below is wave-uniform and stays in SGPRs)
        typename Cfg::Half* const tf = reinterpret_cast<typename Cfg::Half*>(tile) + 8 * lane;
        auto sample = [&](int i, int f, int b) {
            if constexpr (sizeof(T) == 1) return static_cast<float>((d[i][f][0] >> (8 * b)) & 0xffu);
            else return static_cast<float>((d[i][f][b >> 1] >> (16 * (b & 1))) & 0xffffu);
        };
        if (lane < kLoadLanes) {
#pragma unroll
            for (int i = 0; i < kRowsPerWave; ++i) {
                const int r = wave + 4 * i;
                if (r >= Cfg::kLdsRows) continue;  // wave-uniform
#pragma unroll
                for (int f = 0; f < 2; ++f) tf[2 * (r * Cfg::kLdsPitch - shift[i][f]) + f] = Cfg::half_of(sample(i, f, 0));
            }
        }
        if (lane < kLoadLanes - 1) {
#pragma unroll
            for (int i = 0; i < kRowsPerWave; ++i) {
                const int r = wave + 4 * i;
                if (r >= Cfg::kLdsRows) continue;  // wave-uniform
#pragma unroll
                for (int f = 0; f < 2; ++f)
#pragma unroll
                    for (int b = 1; b < 4; ++b) tf[2 * (r * Cfg::kLdsPitch - shift[i][f] + b) + f] = Cfg::half_of(sample(i, f, b));
            }
        }
        // The tile column that reaches past the plane's last column: those columns replicate it (the dwords held the pitch's padding, the
        // next row or zero there).  Behind the writes above, by the wave that wrote the row.
        if (gx0 + Cfg::kLdsCols > a.src_w) {  // workgroup-uniform
            typename Cfg::Half* const tr = reinterpret_cast<typename Cfg::Half*>(tile);
#pragma unroll
            for (int i = 0; i < kRowsPerWave; ++i) {
                const int r = wave + 4 * i;
                if (r >= Cfg::kLdsRows) continue;  // wave-uniform
                int gy = gy0 + r;
                gy = gy < a.src_h ? gy : a.src_h - 1;
                const float v0 = to_float(reinterpret_cast<const T*>(sb0 + static_cast<size_t>(gy) * io.src_pitch)[a.src_w - 1]);
                const float v1 = to_float(reinterpret_cast<const T*>(sb1 + static_cast<size_t>(gy) * io.src_pitch)[a.src_w - 1]);
#pragma unroll
                for (int k = 0; k < (Cfg::kLdsCols + 63) / 64; ++k) {
                    const int c = lane + 64 * k;
                    if (gx0 + c >= a.src_w && c < Cfg::kLdsCols) {
                        tr[2 * (r * Cfg::kLdsPitch + c)] = Cfg::half_of(v0);
                        tr[2 * (r * Cfg::kLdsPitch + c) + 1] = Cfg::half_of(v1);
                    }
                }
            }
        }
        // an edge window that starts one column in front of the tile: that column into the pair in front of each row (stage_edge_column)
        const bool in_front = edge_tile && ((a.edge.n[0] > 0 && tile_x == a.edge.tile_x[0] && a.edge.lds_col[0] < 0) ||
                                            (a.edge.n[1] > 0 && tile_x == a.edge.tile_x[1] && a.edge.lds_col[1] < 0));
        constexpr int kFrontWaves = (Cfg::kLdsRows + 63) / 64;  // a lane per tile row: wave 0 alone up to 64 staged rows
        const int fr = kFrontWaves == 1 ? lane : lane + 64 * wave;
        if (in_front && (kFrontWaves == 1 ? wave == 0 : wave < kFrontWaves) && fr < Cfg::kLdsRows && gx0 > 0) {
            int gy = gy0 + fr;
            gy = gy < a.src_h ? gy : a.src_h - 1;
            typename Cfg::Half* const tc = reinterpret_cast<typename Cfg::Half*>(tile + fr * Cfg::kLdsPitch - 1);
            tc[0] = Cfg::half_of(to_float(reinterpret_cast<const T*>(sb0 + static_cast<size_t>(gy) * io.src_pitch)[gx0 - 1]));
            tc[1] = Cfg::half_of(to_float(reinterpret_cast<const T*>(sb1 + static_cast<size_t>(gy) * io.src_pitch)[gx0 - 1]));
        }
    }
    __syncthreads();
    const uint32_t plane_bytes = static_cast<uint32_t>(io.dst_pitch) * a.dst_h;
    const BufferRsrc d0 = make_rsrc(static_cast<char*>(io.dst) + f0 * io.dst_frame_stride, plane_bytes);  // wave-uniform
    const BufferRsrc d1 = make_rsrc(static_cast<char*>(io.dst) + f1 * io.dst_frame_stride, plane_bytes);
    if (edge_tile) {
        if constexpr (RG == 8) {
            quad2_edge_columns<T, Cfg, 6, 7, f32x2, 1, Word>(a, io, tile, tile_x, j0, wave, lane, d0, d1, f1_ok);
        } else {
            quad2_edge_columns<T, Cfg, 6, 7, float, 2>(a, io, reinterpret_cast<const float*>(tile), tile_x, j0, wave, lane, d0, d0, false);
            if (f1_ok) quad2_edge_columns<T, Cfg, 6, 7, float, 2>(a, io, reinterpret_cast<const float*>(tile) + 1, tile_x, j0, wave, lane, d1, d1, false);
        }
    }
    const int ia = i0 + 2 * lane;  // the lane's first period
    if (ia >= a.ni) return;        // no barrier below
    const bool b_ok = ia + 1 < a.ni;
    f32x2 w[kQuad2ShareClasses / 2];
#pragma unroll
    for (int k = 0; k < kQuad2ShareClasses / 2; ++k) w[k] = f32x2{a.share_w[2 * k], a.share_w[2 * k + 1]};
    const uint32_t xoff = static_cast<uint32_t>(a.ix0 + 2 * ia) * static_cast<uint32_t>(sizeof(T));
    for (int st = 0; st < Cfg::kStripsPerWave; ++st) {
        const int jb = Cfg::kStripRows * (wave * Cfg::kStripsPerWave + st);  // the strip's first period row in the tile
        if (j0 + jb >= a.nj) break;                                          // wave-uniform: bottom tiles
        const Word* wb = tile + jb * Cfg::kLdsPitch + 2 * lane;
        f32x2 acc[8 * Cfg::kStripRows];
        auto store = [&](auto PR) {
            constexpr int pr = decltype(PR)::value;
            if constexpr (pr >= 0) {
                const int j = j0 + jb + pr;
                if (j < a.nj) {  // wave-uniform: partial strips of bottom tiles
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const uint32_t so = static_cast<uint32_t>(a.iy0 + 2 * j + q) * static_cast<uint32_t>(io.dst_pitch);
                        const f32x2* r = acc + 4 * (2 * pr + q);
                        store_quad_buf<T>(d0, xoff, so, f32x2{r[0].x, r[1].x}, f32x2{r[2].x, r[3].x}, io.peak, b_ok);
                        if (f1_ok) store_quad_buf<T>(d1, xoff, so, f32x2{r[0].y, r[1].y}, f32x2{r[2].y, r[3].y}, io.peak, b_ok);
                    }
                }
            }
        };
        if constexpr (Cfg::kBf16) quad2_share_walk16<Cfg>(acc, wb, w, std::make_integer_sequence<int, Cfg::kStripRows + 5>{}, store);
        else quad2_share_strip<Cfg>(acc, wb, w, std::make_integer_sequence<int, Cfg::kStripRows + 5>{}, store);
    }
}

// INNER: bit 2 * ly + q set = taps 0 and 5 of kernel row ly are zero for both phases p of q and are not executed (the disc's chord
// in the box's edge rows).  Instantiated for no such rows and for the pattern of the 2x up-scale with tap 3 at blur 1 (q = 0: the
// last kernel row, q = 1: the first): the launcher takes the instantiation whose mask is a subset of the plan's.
constexpr uint32_t kQuad2InnerTap3 = PeriodicArgs::kQuadInnerTap3;
// NT: taps per kernel row -- 6, or 7 for the 6-row x 7-column support (chroma planes sited as MPEG-2 at 2x: the disc spans six
// source rows but, shifted by an eighth of a sample, seven columns; PeriodicArgs::quad_taps).
// The integer kInnerTap3 instances have the frame-pair form (quad2_share_body); the full-tile one's strips of 8 period rows hold 96
// accumulators and run at four waves per SIMD (128 VGPRs), every other instance at six (80).
template <typename T, uint32_t INNER, int NT>
constexpr bool quad2_share_instance() { return !is_float_sample_v<T> && INNER == kQuad2InnerTap3 && NT == 6; }
template <typename T, int RG, uint32_t INNER, int NT = 6>
__global__ __launch_bounds__(256, (quad2_share_instance<T, INNER, NT>() && RG == 8 ? 4 : 6)) void ewa_periodic_quad2_kernel(const PeriodicArgs a,
                                                                                                                       const PlaneIO io) {
    using Cfg = Quad2Cfg<RG>;
    constexpr int FS = Cfg::FS;
    static_assert(RG % 4 == 0, "the four waves of a workgroup take RG / 4 row groups each");
    // (two words in front of the tile: row 0's "column -1", see the edge columns below; the tile stays 8-byte aligned)
    // The frame-pair form (quad2_share_body) of the integer kInnerTap3 instances stages its tile into the same words.
    constexpr bool kShare = quad2_share_instance<T, INNER, NT>();
    using ShareCfg = Quad2ShareCfg<T, RG>;
    constexpr int kWords = 2 + Cfg::kLdsRows * Cfg::kLdsPitch;
    if constexpr (kShare && RG == 8) {  // (what follows is dead code here: neither its registers nor its tile are allocated)
        __shared__ __attribute__((aligned(16))) float share_words[ShareCfg::kLdsFloats];
        quad2_share_body<T, RG>(a, io, share_words);
        return;
    }
    __shared__ __attribute__((aligned(16))) float tile_words[kShare && ShareCfg::kLdsFloats > kWords ? ShareCfg::kLdsFloats : kWords];
    if constexpr (kShare) {
        if (quad2_share_runs<RG>(io)) {  // workgroup-uniform
            quad2_share_body<T, RG>(a, io, tile_words);
            return;
        }
    }
    float* const tile = tile_words + 2;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int tile_x, tile_y;
    swizzled_tile(tile_x, tile_y);
    const int i0 = tile_x * Cfg::kTileCols;
    const int j0 = tile_y * Cfg::kTileRows;
    const size_t frame = blockIdx.z;
    if (skips_frame(a, frame)) return;  // float planes: the other launch's frame
    // integer planes: this tile column also computes the plane's border columns of its rows (PeriodicArgs::EdgeColumns)
    const bool edge_tile = edge_tile_of<T>(a, tile_x);
    {   // stage the source tile as fp32, all loads in front of the LDS writes (see ewa_periodic_kernel)
        const int gx0 = a.min_sx + i0;
        const int gy0 = a.min_sy + j0;
        const char* sbase = static_cast<const char*>(io.src) + frame * io.src_frame_stride;
        constexpr int kRowsPerWave = (Cfg::kLdsRows + 3) / 4;
        constexpr int kColsPerLane = (Cfg::kLdsCols + 63) / 64;
        T staged[kRowsPerWave][kColsPerLane];
        NonFinite<T> nonfinite(a, frame);
#pragma unroll
        for (int i = 0; i < kRowsPerWave; ++i) {
            int gy = gy0 + wave + 4 * i;
            gy = gy < a.src_h ? gy : a.src_h - 1;
            const T* srow = reinterpret_cast<const T*>(sbase + static_cast<size_t>(gy) * io.src_pitch);
#pragma unroll
            for (int k = 0; k < kColsPerLane; ++k) {
                int gx = gx0 + lane + 64 * k;
                gx = gx < a.src_w ? gx : a.src_w - 1;
                staged[i][k] = srow[gx];
            }
        }
#pragma unroll
        for (int i = 0; i < kRowsPerWave; ++i) {
            const int r = wave + 4 * i;
#pragma unroll
            for (int k = 0; k < kColsPerLane; ++k) {
                const int c = lane + 64 * k;
                // (the pitch's two spare words stay unwritten here: the second is the next row's column -1)
                if (r < Cfg::kLdsRows && c < Cfg::kLdsCols) tile[r * Cfg::kLdsPitch + c] = nonfinite.take(staged[i][k]);
            }
        }
        if constexpr (!is_float_sample_v<T>) {
            if (edge_tile) stage_edge_column<T, Cfg>(a, io, tile, tile_x, sbase, gx0, gy0, wave, lane);
        }
    }
    __syncthreads();
    const BufferRsrc drsrc = make_rsrc(static_cast<char*>(io.dst) + frame * io.dst_frame_stride,
                                       static_cast<uint32_t>(io.dst_pitch) * a.dst_h);  // wave-uniform
    if constexpr (!is_float_sample_v<T>) {
        if (edge_tile) quad2_edge_columns<T, Cfg, 6, 7>(a, io, tile, tile_x, j0, wave, lane, drsrc, drsrc, false);
    }
    const int ia = i0 + 2 * lane;  // the lane's first period
    if (ia >= a.ni) return;        // no barrier below
    const bool b_ok = ia + 1 < a.ni;

    const JINC_CONSTANT f32x2* quad = (const JINC_CONSTANT f32x2*)(a.quad);
    // both phases of an axis share the window origin, which is also the tile's (host: quad != nullptr only then)
    const float* base = tile + 2 * lane;
    const uint32_t xoff = static_cast<uint32_t>(a.ix0 + 2 * ia) * static_cast<uint32_t>(sizeof(T));

    constexpr int kGroupsPerWave = RG / 4;
    const int g_first = wave * kGroupsPerWave;
    if (j0 + g_first * FS >= a.nj) return;  // wave-uniform: bottom tiles
    f32x2 win[24];
    {
        const float* wb = base + (g_first * FS) * Cfg::kLdsPitch;
        quad2_load_row<0>(win, wb + 0 * Cfg::kLdsPitch);
        quad2_load_row<1>(win, wb + 1 * Cfg::kLdsPitch);
        quad2_load_row<2>(win, wb + 2 * Cfg::kLdsPitch);
        quad2_load_row<3>(win, wb + 3 * Cfg::kLdsPitch);
        quad2_load_row<4>(win, wb + 4 * Cfg::kLdsPitch);
    }
    for (int g = g_first; g < g_first + kGroupsPerWave; ++g) {
        if (j0 + g * FS >= a.nj) break;  // wave-uniform
        const float* gbase = base + (g * FS) * Cfg::kLdsPitch;
#define JINC_QUAD2_ROW(U)                                                                                          \
    {                                                                                                              \
        quad2_load_row<(U + FS - 1) % FS>(win, gbase + (U + FS - 1) * Cfg::kLdsPitch);                              \
        f32x2 acc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};                                            \
        uint32_t zero;                                                                                              \
        asm volatile("s_mov_b32 %0, 0" : "=s"(zero)); /* opaque: keeps the coefficient loads inside the row loop */ \
        quad2_pixel6<U, INNER, NT>(acc, win, quad + zero);                                                          \
        const int j = j0 + g * FS + U;                                                                              \
        if (j < a.nj) {                                                                                             \
            const uint32_t so = static_cast<uint32_t>(a.iy0 + 2 * j) * io.dst_pitch;                                \
            store_quad_buf<T>(drsrc, xoff, so, acc[0], acc[1], io.peak, b_ok);                                      \
            store_quad_buf<T>(drsrc, xoff, so + static_cast<uint32_t>(io.dst_pitch), acc[2], acc[3], io.peak, b_ok); \
        }                                                                                                           \
    }
        JINC_QUAD2_ROW(0) JINC_QUAD2_ROW(1) JINC_QUAD2_ROW(2) JINC_QUAD2_ROW(3) JINC_QUAD2_ROW(4) JINC_QUAD2_ROW(5)
#undef JINC_QUAD2_ROW
    }
}

template <typename T, int RG>
int launch_periodic_quad2_t(const PeriodicArgs& pa, const PlaneIO& io, hipStream_t stream) {
    using Cfg = Quad2Cfg<RG>;
    dim3 grid((pa.ni + Cfg::kTileCols - 1) / Cfg::kTileCols, (pa.nj + Cfg::kTileRows - 1) / Cfg::kTileRows, io.nframes);
    if (pa.quad_taps == 7 && quad_span7_fits(pa.quad_span7, PeriodicArgs::kQuadSpan7Mpeg2)) {  // the chords of MPEG-2 sited chroma at 2x: 36 of 42 taps
        hipLaunchKernelGGL((ewa_periodic_quad2_kernel<T, RG, PeriodicArgs::kQuadSpan7Mpeg2, 7>), grid, dim3(256, 1, 1), 0, stream, pa, io);
        knobs::note_instance("ewa_periodic_quad2_kernel", "%s, %d, %uu, 7", knobs::type_name<T>(), RG, PeriodicArgs::kQuadSpan7Mpeg2);
    } else if (pa.quad_taps == 7 && quad_span7_fits(pa.quad_span7, PeriodicArgs::kQuadSpan7Mpeg2Swapped)) {
        hipLaunchKernelGGL((ewa_periodic_quad2_kernel<T, RG, PeriodicArgs::kQuadSpan7Mpeg2Swapped, 7>), grid, dim3(256, 1, 1), 0, stream, pa, io);
        knobs::note_instance("ewa_periodic_quad2_kernel", "%s, %d, %uu, 7", knobs::type_name<T>(), RG, PeriodicArgs::kQuadSpan7Mpeg2Swapped);
    } else if (pa.quad_taps == 7) {
        hipLaunchKernelGGL((ewa_periodic_quad2_kernel<T, RG, 0u, 7>), grid, dim3(256, 1, 1), 0, stream, pa, io);
        knobs::note_instance("ewa_periodic_quad2_kernel", "%s, %d, 0u, 7", knobs::type_name<T>(), RG);
    } else if ((pa.quad_inner & kQuad2InnerTap3) == kQuad2InnerTap3) {
        bool share = false;
        if constexpr (!is_float_sample_v<T>) share = true;
        if (share && pa.quad_share) {  // integer planes: the frame-pair form, on tiles of its own (quad2_share_body)
            using ShareCfg = Quad2ShareCfg<T, RG>;
            if (quad2_share_runs<RG>(io))
                grid = dim3((pa.ni + ShareCfg::kTileCols - 1) / ShareCfg::kTileCols, (pa.nj + ShareCfg::kTileRows - 1) / ShareCfg::kTileRows,
                            (io.nframes + 1) / 2);
        } else if (share) {  // ... whose instance needs the symmetry classes: a plan that does not follow them takes every tap
            hipLaunchKernelGGL((ewa_periodic_quad2_kernel<T, RG, 0u>), grid, dim3(256, 1, 1), 0, stream, pa, io);
            knobs::note_instance("ewa_periodic_quad2_kernel", "%s, %d, 0u, 6", knobs::type_name<T>(), RG);
            return static_cast<int>(hipGetLastError());
        }
        hipLaunchKernelGGL((ewa_periodic_quad2_kernel<T, RG, kQuad2InnerTap3>), grid, dim3(256, 1, 1), 0, stream, pa, io);
        knobs::note_instance("ewa_periodic_quad2_kernel", "%s, %d, %uu, 6", knobs::type_name<T>(), RG, kQuad2InnerTap3);
    } else {
        hipLaunchKernelGGL((ewa_periodic_quad2_kernel<T, RG, 0u>), grid, dim3(256, 1, 1), 0, stream, pa, io);
        knobs::note_instance("ewa_periodic_quad2_kernel", "%s, %d, 0u, 6", knobs::type_name<T>(), RG);
    }
    return static_cast<int>(hipGetLastError());
}

}  // namespace

int JINC_QUAD2_LAUNCH(const PeriodicArgs& pa, const PlaneIO& io, hipStream_t stream) {
    return for_sample_type(io, [&](auto t) { return launch_periodic_quad2_t<decltype(t), JINC_QUAD2_RG>(pa, io, stream); });
}

}  // namespace jinc
