// kernel_periodic_quad2x8.hip -- periodic interior kernel, quad form with two periods per lane on the trimmed 8-row support (2x
// up-scales with tap 4): ewa_periodic_quad2x8_kernel with Quad2x8Cfg, the 8-tap rows quad2_row8 / quad2_row8_t1 / _t2 under the chord
// pattern TR8 (quad2_pixel8), the 9-tap span rows quad2_row9_span (8 rows x 9 columns: chroma sited as MPEG-2; quad2_pixel9),
// quad2x8_load_row and launch_periodic_quad2x8_t behind launch_periodic_quad2x8.  The four-sample store, the edge columns, the
// coefficient fetches, the chord pattern and the packed-multiply macros are shared with the other quad units:
// kernel_periodic_quad_common.inc.  See kernel_periodic.hip for the family, device_common.hpp for the parity rules.
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
// Two periods per lane on the trimmed 8 x 8 support (ewa_periodic_quad2x8_kernel): ewa_periodic_quad2_kernel's mapping for tap 4
// ------------------------------------------------------------------------------------------------
// A lane owns two adjacent periods = 4 x 2 output samples from one 8-row x 9-column register window (rows kept ten wide: five
// register pairs, five aligned ds_read_b64 per row), four chains interleaved two by two, coefficient pairs shared by both
// periods.  100 registers: five waves per SIMD.
template <int RG>
struct Quad2x8Cfg {
    static constexpr int FS = 8;
    static constexpr int kTileCols = 128;
    static constexpr int kTileRows = FS * RG;
    static constexpr int kLdsCols = kTileCols + FS;   // lane 63 reads columns 126 .. 135
    static constexpr int kLdsPitch = 138;             // even
    static constexpr int kLdsRows = kTileRows + FS - 1;
};

// quad2_row8 (below) without the first and last t taps of the kernel row (t = 1: taps 1 .. 6, t = 2: taps 2 .. 5), for the rows the chord
// pattern TR8 shortens (kernel_periodic_quad_common.inc; the one-period forms: kernel_periodic_quad.hip quad_row8_t1 / _t2).
__device__ __forceinline__ void quad2_row8_t1(f32x2& acc_a, f32x2& acc_b, f32x2 w0, f32x2 w1, f32x2 w2, f32x2 w3, f32x2 c1, f32x2 c2, f32x2 c3, f32x2 c4, f32x2 c5, f32x2 c6) {
    f32x2 ta, tb;
    asm("v_pk_mul_f32 %2, %4, %8 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_mul_f32 %3, %5, %8 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3\n\t"
        "v_pk_mul_f32 %2, %5, %9 op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %3, %5, %9 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3\n\t"
        "v_pk_mul_f32 %2, %5, %10 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_mul_f32 %3, %6, %10 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3\n\t"
        "v_pk_mul_f32 %2, %6, %11 op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %3, %6, %11 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3\n\t"
        "v_pk_mul_f32 %2, %6, %12 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_mul_f32 %3, %7, %12 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3\n\t"
        "v_pk_mul_f32 %2, %7, %13 op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %3, %7, %13 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3"
        : "+v"(acc_a), "+v"(acc_b), "=&v"(ta), "=&v"(tb)
        : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "s"(c1), "s"(c2), "s"(c3), "s"(c4), "s"(c5), "s"(c6));
}
__device__ __forceinline__ void quad2_row8_t2(f32x2& acc_a, f32x2& acc_b, f32x2 w1, f32x2 w2, f32x2 w3, f32x2 c2, f32x2 c3, f32x2 c4, f32x2 c5) {
    f32x2 ta, tb;
    asm("v_pk_mul_f32 %2, %4, %7 op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %3, %4, %7 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3\n\t"
        "v_pk_mul_f32 %2, %4, %8 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_mul_f32 %3, %5, %8 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3\n\t"
        "v_pk_mul_f32 %2, %5, %9 op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %3, %5, %9 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3\n\t"
        "v_pk_mul_f32 %2, %5, %10 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_mul_f32 %3, %6, %10 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3"
        : "+v"(acc_a), "+v"(acc_b), "=&v"(ta), "=&v"(tb)
        : "v"(w1), "v"(w2), "v"(w3), "s"(c2), "s"(c3), "s"(c4), "s"(c5));
}

__device__ __forceinline__ void quad2_row8(f32x2& acc_a, f32x2& acc_b, f32x2 w0, f32x2 w1, f32x2 w2, f32x2 w3, f32x2 w4, f32x2 c0, f32x2 c1,
                                           f32x2 c2, f32x2 c3, f32x2 c4, f32x2 c5, f32x2 c6, f32x2 c7) {
    f32x2 ta, tb;
    asm(JINC_LO("%2", "%4", "%9") JINC_HI("%3", "%4", "%9") JINC_ADD2       // tap 0: A column 0, B column 1
        JINC_HI("%2", "%4", "%10") JINC_LO("%3", "%5", "%10") JINC_ADD2     // tap 1: A 1, B 2
        JINC_LO("%2", "%5", "%11") JINC_HI("%3", "%5", "%11") JINC_ADD2     // tap 2
        JINC_HI("%2", "%5", "%12") JINC_LO("%3", "%6", "%12") JINC_ADD2     // tap 3
        JINC_LO("%2", "%6", "%13") JINC_HI("%3", "%6", "%13") JINC_ADD2     // tap 4
        JINC_HI("%2", "%6", "%14") JINC_LO("%3", "%7", "%14") JINC_ADD2     // tap 5
        JINC_LO("%2", "%7", "%15") JINC_HI("%3", "%7", "%15") JINC_ADD2     // tap 6
        JINC_HI("%2", "%7", "%16") JINC_LO("%3", "%8", "%16")               // tap 7: A 7, B 8
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3"
        : "+v"(acc_a), "+v"(acc_b), "=&v"(ta), "=&v"(tb)
        : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "v"(w4), "s"(c0), "s"(c1), "s"(c2), "s"(c3), "s"(c4), "s"(c5), "s"(c6), "s"(c7));
}
#undef JINC_LO
#undef JINC_HI
#undef JINC_ADD2

template <int SLOT>
__device__ __forceinline__ void quad2x8_load_row(f32x2 (&w)[40], const float* p) {
    const f32x2* p2 = reinterpret_cast<const f32x2*>(p);
#pragma unroll
    for (int m = 0; m < 5; ++m) w[5 * SLOT + m] = p2[m];
}

template <int U, uint32_t TR8>
__device__ __forceinline__ void quad2_pixel8(f32x2 (&acc)[4], const f32x2 (&w)[40], const JINC_CONSTANT f32x2* quad) {
    f32x2 ca[16], cb[16];
    quad_fetch(ca, quad, 0);
#define JINC_QUAD2X8_STEP(LY, CUR, NEXT)                                                                                                  \
    if constexpr (LY < 7) quad_fetch(NEXT, quad, LY + 1);                                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                                                                     \
    quad_arrived(CUR);                                                                                                                     \
    {                                                                                                                                      \
        constexpr int S = 5 * ((U + LY) % 8);                                                                                              \
        if constexpr (quad8_trim_of(TR8, LY, 0) == 2)                                                                                      \
            quad2_row8_t2(acc[0], acc[1], w[S + 1], w[S + 2], w[S + 3], CUR[2], CUR[3], CUR[4], CUR[5]);                                   \
        else if constexpr (quad8_trim_of(TR8, LY, 0) == 1)                                                                                 \
            quad2_row8_t1(acc[0], acc[1], w[S], w[S + 1], w[S + 2], w[S + 3], CUR[1], CUR[2], CUR[3], CUR[4], CUR[5], CUR[6]);             \
        else                                                                                                                               \
            quad2_row8(acc[0], acc[1], w[S], w[S + 1], w[S + 2], w[S + 3], w[S + 4], CUR[0], CUR[1], CUR[2], CUR[3], CUR[4], CUR[5],       \
                       CUR[6], CUR[7]);                                                                                                    \
        if constexpr (quad8_trim_of(TR8, LY, 1) == 2)                                                                                      \
            quad2_row8_t2(acc[2], acc[3], w[S + 1], w[S + 2], w[S + 3], CUR[10], CUR[11], CUR[12], CUR[13]);                               \
        else if constexpr (quad8_trim_of(TR8, LY, 1) == 1)                                                                                 \
            quad2_row8_t1(acc[2], acc[3], w[S], w[S + 1], w[S + 2], w[S + 3], CUR[9], CUR[10], CUR[11], CUR[12], CUR[13], CUR[14]);        \
        else                                                                                                                               \
            quad2_row8(acc[2], acc[3], w[S], w[S + 1], w[S + 2], w[S + 3], w[S + 4], CUR[8], CUR[9], CUR[10], CUR[11], CUR[12], CUR[13],   \
                       CUR[14], CUR[15]);                                                                                                  \
    }                                                                                                                                      \
    __builtin_amdgcn_sched_barrier(0);
    JINC_QUAD2X8_STEP(0, ca, cb)
    JINC_QUAD2X8_STEP(1, cb, ca)
    JINC_QUAD2X8_STEP(2, ca, cb)
    JINC_QUAD2X8_STEP(3, cb, ca)
    JINC_QUAD2X8_STEP(4, ca, cb)
    JINC_QUAD2X8_STEP(5, cb, ca)
    JINC_QUAD2X8_STEP(6, ca, cb)
    JINC_QUAD2X8_STEP(7, cb, ca)
#undef JINC_QUAD2X8_STEP
}

// Nine taps per kernel row for both periods of a lane (the 8-row x 9-column support: chroma planes sited as MPEG-2 at 2x with tap 4):
// period A reads columns 0 .. 8, period B columns 1 .. 9 of the row's five register pairs; FORM = the span of the row's taps that
// is executed (0: all nine, 1: taps 1 .. 8, 2: 1 .. 7, 3: 2 .. 7, 4: 2 .. 6 -- the others carry zero coefficients for both phases p).
#define JINC_Q9_EVEN(W, C) /* tap t even: period A = the low half of pair t / 2, B its high half */                         \
    "v_pk_mul_f32 %2, " W ", " C " op_sel_hi:[0,1]\n\tv_pk_mul_f32 %3, " W ", " C " op_sel:[1,0] op_sel_hi:[1,1]\n\t" \
    "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3\n\t"
#define JINC_Q9_ODD(W, WN, C) /* tap t odd: A = the high half of pair t / 2, B the low half of the next pair */             \
    "v_pk_mul_f32 %2, " W ", " C " op_sel:[1,0] op_sel_hi:[1,1]\n\tv_pk_mul_f32 %3, " WN ", " C " op_sel_hi:[0,1]\n\t" \
    "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %3\n\t"
#define JINC_Q9_T0 JINC_Q9_EVEN("%4", "%9")
#define JINC_Q9_T1 JINC_Q9_ODD("%4", "%5", "%10")
#define JINC_Q9_T2 JINC_Q9_EVEN("%5", "%11")
#define JINC_Q9_T3 JINC_Q9_ODD("%5", "%6", "%12")
#define JINC_Q9_T4 JINC_Q9_EVEN("%6", "%13")
#define JINC_Q9_T5 JINC_Q9_ODD("%6", "%7", "%14")
#define JINC_Q9_T6 JINC_Q9_EVEN("%7", "%15")
#define JINC_Q9_T7 JINC_Q9_ODD("%7", "%8", "%16")
#define JINC_Q9_T8 JINC_Q9_EVEN("%8", "%17")
#define JINC_Q9_OPERANDS                                                                                                          \
    : "+v"(acc_a), "+v"(acc_b), "=&v"(ta), "=&v"(tb)                                                                               \
    : "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]), "v"(w[4]), "s"(c[0]), "s"(c[1]), "s"(c[2]), "s"(c[3]), "s"(c[4]), "s"(c[5]), "s"(c[6]), \
      "s"(c[7]), "s"(c[8])
template <int FORM>
__device__ __forceinline__ void quad2_row9_span(f32x2& acc_a, f32x2& acc_b, const f32x2 (&w)[5], const f32x2 (&c)[10]) {
    static_assert(FORM >= 0 && FORM <= 4, "span forms of the nine-tap row");
    f32x2 ta, tb;
    if constexpr (FORM == 0)
        asm(JINC_Q9_T0 JINC_Q9_T1 JINC_Q9_T2 JINC_Q9_T3 JINC_Q9_T4 JINC_Q9_T5 JINC_Q9_T6 JINC_Q9_T7 JINC_Q9_T8 "" JINC_Q9_OPERANDS);
    else if constexpr (FORM == 1)
        asm(JINC_Q9_T1 JINC_Q9_T2 JINC_Q9_T3 JINC_Q9_T4 JINC_Q9_T5 JINC_Q9_T6 JINC_Q9_T7 JINC_Q9_T8 "" JINC_Q9_OPERANDS);
    else if constexpr (FORM == 2)
        asm(JINC_Q9_T1 JINC_Q9_T2 JINC_Q9_T3 JINC_Q9_T4 JINC_Q9_T5 JINC_Q9_T6 JINC_Q9_T7 "" JINC_Q9_OPERANDS);
    else if constexpr (FORM == 3)
        asm(JINC_Q9_T2 JINC_Q9_T3 JINC_Q9_T4 JINC_Q9_T5 JINC_Q9_T6 JINC_Q9_T7 "" JINC_Q9_OPERANDS);
    else
        asm(JINC_Q9_T2 JINC_Q9_T3 JINC_Q9_T4 JINC_Q9_T5 JINC_Q9_T6 "" JINC_Q9_OPERANDS);
}
#undef JINC_Q9_EVEN
#undef JINC_Q9_ODD
#undef JINC_Q9_T0
#undef JINC_Q9_T1
#undef JINC_Q9_T2
#undef JINC_Q9_T3
#undef JINC_Q9_T4
#undef JINC_Q9_T5
#undef JINC_Q9_T6
#undef JINC_Q9_T7
#undef JINC_Q9_T8
#undef JINC_Q9_OPERANDS

// One output row pair of both periods on the 8 x 9 support.  The ten coefficient pairs of a (kernel row, q) are 20 SGPRs: the two
// row phases alternate through two sets (as quad_pixel9): the pairs of (ly, q = 1) are requested before the taps of (ly, q = 0) are
// issued, those of (ly + 1, q = 0) before the taps of (ly, q = 1).  Layout: quad[ly][q][10 pairs][p] (device_plan.cpp attach_quad, NX = 9).
template <int U, uint64_t SPAN9>
__device__ __forceinline__ void quad2_pixel9(f32x2 (&acc)[4], const f32x2 (&w)[40], const JINC_CONSTANT f32x2* quad) {
    f32x2 ca[10], cb[10];
    quad_fetch10(ca, quad, 0);
#define JINC_QUAD2X9_STEP(LY)                                                                                      \
    quad_fetch10(cb, quad, 2 * LY + 1);                                                                            \
    __builtin_amdgcn_sched_barrier(0);                                                                             \
    quad_arrived10(ca);                                                                                            \
    {                                                                                                              \
        constexpr int S = 5 * ((U + LY) % 8);                                                                      \
        const f32x2 row[5] = {w[S], w[S + 1], w[S + 2], w[S + 3], w[S + 4]};                                       \
        quad2_row9_span<static_cast<int>((SPAN9 >> (3 * (2 * LY))) & 7u)>(acc[0], acc[1], row, ca);                 \
        __builtin_amdgcn_sched_barrier(0);                                                                         \
        if constexpr (LY < 7) quad_fetch10(ca, quad, 2 * LY + 2);                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                         \
        quad_arrived10(cb);                                                                                        \
        quad2_row9_span<static_cast<int>((SPAN9 >> (3 * (2 * LY + 1))) & 7u)>(acc[2], acc[3], row, cb);             \
    }                                                                                                              \
    __builtin_amdgcn_sched_barrier(0);
    JINC_QUAD2X9_STEP(0) JINC_QUAD2X9_STEP(1) JINC_QUAD2X9_STEP(2) JINC_QUAD2X9_STEP(3) JINC_QUAD2X9_STEP(4) JINC_QUAD2X9_STEP(5)
    JINC_QUAD2X9_STEP(6) JINC_QUAD2X9_STEP(7)
#undef JINC_QUAD2X9_STEP
}

// NT: taps per kernel row -- 8, or 9 for the 8-row x 9-column support (then SPAN9 = the span form of every (kernel row, q), TR8 unused).
template <typename T, int RG, uint32_t TR8, int NT = 8, uint64_t SPAN9 = 0>
__global__ __launch_bounds__(256, 5) void ewa_periodic_quad2x8_kernel(const PeriodicArgs a, const PlaneIO io) {
    using Cfg = Quad2x8Cfg<RG>;
    constexpr int FS = Cfg::FS;
    static_assert(RG % 4 == 0, "the four waves of a workgroup take RG / 4 row groups each");
    // (two words in front of the tile: row 0's "column -1" of the edge columns, stage_edge_column; the tile stays 8-byte aligned)
    __shared__ __attribute__((aligned(16))) float tile_words[2 + Cfg::kLdsRows * Cfg::kLdsPitch];
    float* const tile = tile_words + 2;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int tile_x, tile_y;
    swizzled_tile(tile_x, tile_y);
    const int i0 = tile_x * Cfg::kTileCols;
    const int j0 = tile_y * Cfg::kTileRows;
    const size_t frame = blockIdx.z;
    if (skips_frame(a, frame)) return;  // float planes: the other launch's frame
    const bool edge_tile = edge_tile_of<T>(a, tile_x);  // integer planes: this tile column computes the plane's border columns of its rows
    {   // stage the source tile as fp32, in two halves of the rows (all loads of a half in front of its LDS writes): the whole
        // tile at once would hold more staged registers than the compute phase has
        const int gx0 = a.min_sx + i0;
        const int gy0 = a.min_sy + j0;
        const char* sbase = static_cast<const char*>(io.src) + frame * io.src_frame_stride;
        constexpr int kRowsPerWave = (Cfg::kLdsRows + 3) / 4;
        constexpr int kHalf = (kRowsPerWave + 1) / 2;
        constexpr int kColsPerLane = (Cfg::kLdsPitch + 63) / 64;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            T staged[kHalf][kColsPerLane];
            NonFinite<T> nonfinite(a, frame);
#pragma unroll
            for (int i = 0; i < kHalf; ++i) {
                int gy = gy0 + wave + 4 * (h * kHalf + i);
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
            for (int i = 0; i < kHalf; ++i) {
                const int r = wave + 4 * (h * kHalf + i);
#pragma unroll
                for (int k = 0; k < kColsPerLane; ++k) {
                    const int c = lane + 64 * k;
                    // (the pitch's two spare words stay unwritten here: the second is the next row's column -1)
                    if (r < Cfg::kLdsRows && c < Cfg::kLdsCols) tile[r * Cfg::kLdsPitch + c] = nonfinite.take(staged[i][k]);
                }
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
        if (edge_tile) quad2_edge_columns<T, Cfg, 8, 9>(a, io, tile, tile_x, j0, wave, lane, drsrc, drsrc, false);
    }
    const int ia = i0 + 2 * lane;
    if (ia >= a.ni) return;  // no barrier below
    const bool b_ok = ia + 1 < a.ni;

    const JINC_CONSTANT f32x2* quad = (const JINC_CONSTANT f32x2*)(a.quad);
    const float* base = tile + 2 * lane;
    const uint32_t xoff = static_cast<uint32_t>(a.ix0 + 2 * ia) * static_cast<uint32_t>(sizeof(T));

    constexpr int kGroupsPerWave = RG / 4;
    const int g_first = wave * kGroupsPerWave;
    if (j0 + g_first * FS >= a.nj) return;  // wave-uniform: bottom tiles
    f32x2 win[40];
    {
        const float* wb = base + (g_first * FS) * Cfg::kLdsPitch;
        quad2x8_load_row<0>(win, wb + 0 * Cfg::kLdsPitch);
        quad2x8_load_row<1>(win, wb + 1 * Cfg::kLdsPitch);
        quad2x8_load_row<2>(win, wb + 2 * Cfg::kLdsPitch);
        quad2x8_load_row<3>(win, wb + 3 * Cfg::kLdsPitch);
        quad2x8_load_row<4>(win, wb + 4 * Cfg::kLdsPitch);
        quad2x8_load_row<5>(win, wb + 5 * Cfg::kLdsPitch);
        quad2x8_load_row<6>(win, wb + 6 * Cfg::kLdsPitch);
    }
    for (int g = g_first; g < g_first + kGroupsPerWave; ++g) {
        if (j0 + g * FS >= a.nj) break;  // wave-uniform
        const float* gbase = base + (g * FS) * Cfg::kLdsPitch;
#define JINC_QUAD2X8_ROW(U)                                                                                        \
    {                                                                                                              \
        quad2x8_load_row<(U + FS - 1) % FS>(win, gbase + (U + FS - 1) * Cfg::kLdsPitch);                            \
        f32x2 acc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};                                            \
        uint32_t zero;                                                                                              \
        asm volatile("s_mov_b32 %0, 0" : "=s"(zero)); /* opaque: keeps the coefficient loads inside the row loop */ \
        if constexpr (NT == 9) quad2_pixel9<U, SPAN9>(acc, win, quad + zero);                                       \
        else quad2_pixel8<U, TR8>(acc, win, quad + zero);                                                           \
        const int j = j0 + g * FS + U;                                                                              \
        if (j < a.nj) {                                                                                             \
            const uint32_t so = static_cast<uint32_t>(a.iy0 + 2 * j) * io.dst_pitch;                                \
            store_quad_buf<T>(drsrc, xoff, so, acc[0], acc[1], io.peak, b_ok);                                      \
            store_quad_buf<T>(drsrc, xoff, so + static_cast<uint32_t>(io.dst_pitch), acc[2], acc[3], io.peak, b_ok); \
        }                                                                                                           \
    }
        JINC_QUAD2X8_ROW(0) JINC_QUAD2X8_ROW(1) JINC_QUAD2X8_ROW(2) JINC_QUAD2X8_ROW(3) JINC_QUAD2X8_ROW(4) JINC_QUAD2X8_ROW(5) JINC_QUAD2X8_ROW(6)
        JINC_QUAD2X8_ROW(7)
#undef JINC_QUAD2X8_ROW
    }
}

template <typename T, int RG>
int launch_periodic_quad2x8_t(const PeriodicArgs& pa, const PlaneIO& io, hipStream_t stream) {
    using Cfg = Quad2x8Cfg<RG>;
    dim3 grid((pa.ni + Cfg::kTileCols - 1) / Cfg::kTileCols, (pa.nj + Cfg::kTileRows - 1) / Cfg::kTileRows, io.nframes);
    if (pa.quad_taps == 9) {  // the 8-row x 9-column support (chroma at tap 4), by the chord pattern the plan's spans fit
        const uint64_t span = quad_span9_fits(pa.quad_span7, kQuadSpan9Mpeg2) ? kQuadSpan9Mpeg2 : quad_span9_fits(pa.quad_span7, kQuadSpan9Mpeg2Swapped) ? kQuadSpan9Mpeg2Swapped : 0;
        if (span == kQuadSpan9Mpeg2)
            hipLaunchKernelGGL((ewa_periodic_quad2x8_kernel<T, RG, 0u, 9, kQuadSpan9Mpeg2>), grid, dim3(256, 1, 1), 0, stream, pa, io);
        else if (span == kQuadSpan9Mpeg2Swapped)
            hipLaunchKernelGGL((ewa_periodic_quad2x8_kernel<T, RG, 0u, 9, kQuadSpan9Mpeg2Swapped>), grid, dim3(256, 1, 1), 0, stream, pa, io);
        else
            hipLaunchKernelGGL((ewa_periodic_quad2x8_kernel<T, RG, 0u, 9, 0>), grid, dim3(256, 1, 1), 0, stream, pa, io);
        knobs::note_instance("ewa_periodic_quad2x8_kernel", "%s, %d, 0u, 9, %lluul", knobs::type_name<T>(), RG, static_cast<unsigned long long>(span));
        return static_cast<int>(hipGetLastError());
    }
    const bool pattern = quad8_pattern_fits(pa.quad_trim8, kQuad8TrimTap4);
    if (pattern)
        hipLaunchKernelGGL((ewa_periodic_quad2x8_kernel<T, RG, kQuad8TrimTap4>), grid, dim3(256, 1, 1), 0, stream, pa, io);
    else
        hipLaunchKernelGGL((ewa_periodic_quad2x8_kernel<T, RG, 0u>), grid, dim3(256, 1, 1), 0, stream, pa, io);
    knobs::note_instance("ewa_periodic_quad2x8_kernel", "%s, %d, %uu, 8, 0ul", knobs::type_name<T>(), RG, pattern ? kQuad8TrimTap4 : 0u);  // (as rocprofv3 spells it)
    return static_cast<int>(hipGetLastError());
}

}  // namespace

int launch_periodic_quad2x8(const PeriodicArgs& pa, const PlaneIO& io, hipStream_t stream) {
    return for_sample_type(io, [&](auto t) { return launch_periodic_quad2x8_t<decltype(t), 4>(pa, io, stream); });
}

}  // namespace jinc
