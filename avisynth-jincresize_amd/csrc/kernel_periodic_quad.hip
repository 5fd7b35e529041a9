// kernel_periodic_quad.hip -- periodic interior kernels, quad form with one period per lane (2x up-scales whose two phases per axis
// share their window origin): one body, quad_body, on three supports
//   ewa_periodic_quad_kernel   7 x 7 (QuadForm7: quad_row7_even / _odd, quad_load_row7, quad_pixel7)
//   ewa_periodic_quad9_kernel  9 x 9 (QuadForm9: quad_row9_even / _odd, quad_load_row9, quad_pixel9)
//   ewa_periodic_quad8_kernel  8 x 8, trimmed by the chord pattern TR8 (QuadForm8: quad_row8, quad_row8_t1 / _t2, quad_load_row8, quad_pixel8)
// with the two-sample store store_pair_buf, for_each_index and the launchers behind launch_periodic_quad.  The coefficient fetches
// and the chord pattern are shared with the two-periods-per-lane forms: kernel_periodic_quad_common.inc.  The tile (PeriodicCfg) is
// the window kernel's: kernel_periodic_common.inc.  See kernel_periodic.hip for the family, device_common.hpp for the parity rules.
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
// Periodic interior kernel, quad form: 2x up-scales whose two phases per axis share their window origin
// ------------------------------------------------------------------------------------------------
// For a 2x up-scale the output pixels (2i, 2i+1) x (2j, 2j+1) of a period read the SAME fs x fs source window (plan:
// start_x[0] == start_x[1], start_y[0] == start_y[1]) with four different coefficient sets.  A lane owns one period
// column and keeps ONE register window for all four chains; the chains of the two horizontally adjacent pixels travel
// as the two halves of a register pair, so every tap of both is one v_pk_mul_f32 (sample broadcast to both halves by
// op_sel, coefficient pair = (phase 0, phase 1) from an aligned SGPR pair) and one v_pk_add_f32 -- two exact IEEE
// products / sums per instruction, each half the reference's sequential chain bit for bit, nothing fused or reassociated.
// Against ewa_periodic_kernel: half the VALU instructions per output sample on the faster packed pair (70 against 58
// Tops/s in the probe), a quarter of the LDS reads and stores, the same 8 waves per SIMD (one window per lane) -- but the
// 4 x fs x fs coefficients no longer fit the SGPR file: the pairs of one kernel row (2 x 16 dwords) are re-read from the
// scalar cache per kernel row and output row pair (always hits: 4 sets).
// Coefficient layout (host: attach_quad): quad[ly][q][8 pairs][p], the pair lx = (set(p=0,q), set(p=1,q))[ly][lx].
template <int FS>
struct QuadTaps;  // packed taps of one kernel row, window row held as pairs of a flat register array

// 7 taps starting at an EVEN flat index: pairs w0..w3 hold taps (0,1) (2,3) (4,5) (6,-)
__device__ __forceinline__ void quad_row7_even(f32x2& acc, f32x2 w0, f32x2 w1, f32x2 w2, f32x2 w3, f32x2 c0, f32x2 c1, f32x2 c2, f32x2 c3,
                                               f32x2 c4, f32x2 c5, f32x2 c6) {
    f32x2 t;
    asm("v_pk_mul_f32 %1, %2, %6 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %2, %7 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %3, %8 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %3, %9 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %4, %10 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %4, %11 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %5, %12 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1"
        : "+v"(acc), "=&v"(t)
        : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "s"(c0), "s"(c1), "s"(c2), "s"(c3), "s"(c4), "s"(c5), "s"(c6));
}
// 7 taps starting at an ODD flat index: pairs w0..w3 hold taps (-,0) (1,2) (3,4) (5,6)
__device__ __forceinline__ void quad_row7_odd(f32x2& acc, f32x2 w0, f32x2 w1, f32x2 w2, f32x2 w3, f32x2 c0, f32x2 c1, f32x2 c2, f32x2 c3,
                                              f32x2 c4, f32x2 c5, f32x2 c6) {
    f32x2 t;
    asm("v_pk_mul_f32 %1, %2, %6 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %3, %7 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %3, %8 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %4, %9 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %4, %10 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %5, %11 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %5, %12 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1"
        : "+v"(acc), "=&v"(t)
        : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "s"(c0), "s"(c1), "s"(c2), "s"(c3), "s"(c4), "s"(c5), "s"(c6));
}

// fs 9: nine taps starting at an EVEN flat index: pairs w0..w4 hold taps (0,1) (2,3) (4,5) (6,7) (8,-)
__device__ __forceinline__ void quad_row9_even(f32x2& acc, f32x2 w0, f32x2 w1, f32x2 w2, f32x2 w3, f32x2 w4, f32x2 c0, f32x2 c1, f32x2 c2,
                                               f32x2 c3, f32x2 c4, f32x2 c5, f32x2 c6, f32x2 c7, f32x2 c8) {
    f32x2 t;
    asm("v_pk_mul_f32 %1, %2, %7 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %2, %8 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %3, %9 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %3, %10 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %4, %11 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %4, %12 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %5, %13 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %5, %14 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %6, %15 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1"
        : "+v"(acc), "=&v"(t)
        : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "v"(w4), "s"(c0), "s"(c1), "s"(c2), "s"(c3), "s"(c4), "s"(c5), "s"(c6), "s"(c7), "s"(c8));
}
// ... at an ODD flat index: pairs w0..w4 hold taps (-,0) (1,2) (3,4) (5,6) (7,8)
__device__ __forceinline__ void quad_row9_odd(f32x2& acc, f32x2 w0, f32x2 w1, f32x2 w2, f32x2 w3, f32x2 w4, f32x2 c0, f32x2 c1, f32x2 c2,
                                              f32x2 c3, f32x2 c4, f32x2 c5, f32x2 c6, f32x2 c7, f32x2 c8) {
    f32x2 t;
    asm("v_pk_mul_f32 %1, %2, %7 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %3, %8 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %3, %9 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %4, %10 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %4, %11 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %5, %12 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %5, %13 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %6, %14 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %6, %15 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1"
        : "+v"(acc), "=&v"(t)
        : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "v"(w4), "s"(c0), "s"(c1), "s"(c2), "s"(c3), "s"(c4), "s"(c5), "s"(c6), "s"(c7), "s"(c8));
}
template <int SLOT>
__device__ __forceinline__ void quad_row9(f32x2& acc, const f32x2 (&w)[41], const f32x2 (&c)[10]) {
    constexpr int K0 = 9 * SLOT, P = K0 / 2;
    if constexpr (K0 % 2 == 0)
        quad_row9_even(acc, w[P], w[P + 1], w[P + 2], w[P + 3], w[P + 4], c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8]);
    else
        quad_row9_odd(acc, w[P], w[P + 1], w[P + 2], w[P + 3], w[P + 4], c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8]);
}
template <int SLOT>
__device__ __forceinline__ void quad_load_row9(f32x2 (&w)[41], const float* p) {
#pragma unroll
    for (int lx = 0; lx < 9; ++lx) {
        constexpr int K0 = 9 * SLOT;
        const float v = p[lx];
        if ((K0 + lx) % 2 == 0) w[(K0 + lx) / 2].x = v;
        else w[(K0 + lx) / 2].y = v;
    }
}
template <int U>
__device__ __forceinline__ void quad_pixel9(f32x2& acc0, f32x2& acc1, const f32x2 (&w)[41], const JINC_CONSTANT f32x2* quad) {
    f32x2 ca[10], cb[10];
    quad_fetch10(ca, quad, 0);
#define JINC_QUAD9_STEP(LY)                                                   \
    quad_fetch10(cb, quad, 2 * LY + 1);                                        \
    __builtin_amdgcn_sched_barrier(0);                                         \
    quad_arrived10(ca);                                                        \
    quad_row9<(U + LY) % 9>(acc0, w, ca);                                      \
    __builtin_amdgcn_sched_barrier(0);                                         \
    if constexpr (LY < 8) quad_fetch10(ca, quad, 2 * LY + 2);                  \
    __builtin_amdgcn_sched_barrier(0);                                         \
    quad_arrived10(cb);                                                        \
    quad_row9<(U + LY) % 9>(acc1, w, cb);                                      \
    __builtin_amdgcn_sched_barrier(0);
    JINC_QUAD9_STEP(0) JINC_QUAD9_STEP(1) JINC_QUAD9_STEP(2) JINC_QUAD9_STEP(3) JINC_QUAD9_STEP(4) JINC_QUAD9_STEP(5)
    JINC_QUAD9_STEP(6) JINC_QUAD9_STEP(7) JINC_QUAD9_STEP(8)
#undef JINC_QUAD9_STEP
}

// Window slot `slot` (7 samples at flat indices 7 * slot ..) times the seven coefficient pairs c[0..6] onto acc.
template <int SLOT>
__device__ __forceinline__ void quad_row7(f32x2& acc, const f32x2 (&w)[25], const f32x2 (&c)[8]) {
    constexpr int K0 = 7 * SLOT, P = K0 / 2;
    if constexpr (K0 % 2 == 0)
        quad_row7_even(acc, w[P], w[P + 1], w[P + 2], w[P + 3], c[0], c[1], c[2], c[3], c[4], c[5], c[6]);
    else
        quad_row7_odd(acc, w[P], w[P + 1], w[P + 2], w[P + 3], c[0], c[1], c[2], c[3], c[4], c[5], c[6]);
}

template <int SLOT>
__device__ __forceinline__ void quad_load_row7(f32x2 (&w)[25], const float* p) {
#pragma unroll
    for (int lx = 0; lx < 7; ++lx) {
        constexpr int K0 = 7 * SLOT;
        const float v = p[lx];
        if ((K0 + lx) % 2 == 0) w[(K0 + lx) / 2].x = v;
        else w[(K0 + lx) / 2].y = v;
    }
}

// One output row pair: window slots (U + ly) % 7 hold kernel rows ly = 0..6; acc0 = (q = 0: phases p = 0, 1), acc1 = (q = 1).
// The coefficient pairs of kernel row ly + 1 are requested before the taps of row ly are issued (two sets of 32 SGPRs
// taken alternately); `quad` must not be loop-invariant in the caller, or the compiler hoists all 224 loads out of the row
// loop and spills them (measured: 264 spilled SGPRs).
template <int U>
__device__ __forceinline__ void quad_pixel7(f32x2& acc0, f32x2& acc1, const f32x2 (&w)[25], const JINC_CONSTANT f32x2* quad) {
    f32x2 ca[16], cb[16];
    quad_fetch(ca, quad, 0);
#define JINC_QUAD_STEP(LY, CUR, NEXT)                                         \
    if constexpr (LY < 6) quad_fetch(NEXT, quad, LY + 1);                      \
    __builtin_amdgcn_sched_barrier(0);                                         \
    quad_arrived(CUR);                                                         \
    quad_row7<(U + LY) % 7>(acc0, w, reinterpret_cast<const f32x2(&)[8]>(CUR[0])); \
    quad_row7<(U + LY) % 7>(acc1, w, reinterpret_cast<const f32x2(&)[8]>(CUR[8])); \
    __builtin_amdgcn_sched_barrier(0);
    JINC_QUAD_STEP(0, ca, cb)
    JINC_QUAD_STEP(1, cb, ca)
    JINC_QUAD_STEP(2, ca, cb)
    JINC_QUAD_STEP(3, cb, ca)
    JINC_QUAD_STEP(4, ca, cb)
    JINC_QUAD_STEP(5, cb, ca)
    JINC_QUAD_STEP(6, ca, cb)
#undef JINC_QUAD_STEP
}

// ------------------------------------------------------------------------------------------------
// Periodic interior kernel, quad form on a trimmed 8 x 8 support (tap 4 at 2x: Jinc64Resize, C4)
// ------------------------------------------------------------------------------------------------
// The fs-7 quad form on eight taps per kernel row: every row starts on a register pair (no odd / even variants), the eight
// coefficient pairs of a kernel row and q are exactly one s_load_dwordx16.  Against the window kernel on the same support:
// half the VALU instructions, a quarter of the LDS reads, and -- what counts on float planes -- the two horizontally adjacent
// samples of a lane leave as ONE store, so a wave's row is one contiguous run instead of every other sample of two.
__device__ __forceinline__ void quad_row8(f32x2& acc, f32x2 w0, f32x2 w1, f32x2 w2, f32x2 w3, f32x2 c0, f32x2 c1, f32x2 c2, f32x2 c3, f32x2 c4,
                                          f32x2 c5, f32x2 c6, f32x2 c7) {
    f32x2 t;
    asm("v_pk_mul_f32 %1, %2, %6 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %2, %7 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %3, %8 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %3, %9 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %4, %10 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %4, %11 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %5, %12 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %5, %13 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1"
        : "+v"(acc), "=&v"(t)
        : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "s"(c0), "s"(c1), "s"(c2), "s"(c3), "s"(c4), "s"(c5), "s"(c6), "s"(c7));
}

// Kernel rows of the 8 x 8 support without their first and last t taps (t = 1: taps 1 .. 6, t = 2: taps 2 .. 5): rows in which those
// taps carry zero coefficients for both phases p of a q -- the disc's chords near the box's top and bottom (compile-time
// pattern TR8 of the quad kernels below; generated, like the full rows, as one asm statement each).
__device__ __forceinline__ void quad_row8_t1(f32x2& acc, f32x2 w0, f32x2 w1, f32x2 w2, f32x2 w3, f32x2 c1, f32x2 c2, f32x2 c3, f32x2 c4, f32x2 c5, f32x2 c6) {
    f32x2 t;
    asm("v_pk_mul_f32 %1, %2, %6 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %3, %7 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %3, %8 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %4, %9 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %4, %10 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %5, %11 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1"
        : "+v"(acc), "=&v"(t)
        : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "s"(c1), "s"(c2), "s"(c3), "s"(c4), "s"(c5), "s"(c6));
}
__device__ __forceinline__ void quad_row8_t2(f32x2& acc, f32x2 w1, f32x2 w2, f32x2 c2, f32x2 c3, f32x2 c4, f32x2 c5) {
    f32x2 t;
    asm("v_pk_mul_f32 %1, %2, %4 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %2, %5 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %3, %6 op_sel_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %3, %7 op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1"
        : "+v"(acc), "=&v"(t)
        : "v"(w1), "v"(w2), "s"(c2), "s"(c3), "s"(c4), "s"(c5));
}

template <int SLOT>
__device__ __forceinline__ void quad_load_row8(f32x2 (&w)[32], const float* p) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        w[4 * SLOT + m].x = p[2 * m];
        w[4 * SLOT + m].y = p[2 * m + 1];
    }
}

template <int U, uint32_t TR8>
__device__ __forceinline__ void quad_pixel8(f32x2& acc0, f32x2& acc1, const f32x2 (&w)[32], const JINC_CONSTANT f32x2* quad) {
    f32x2 ca[16], cb[16];
    quad_fetch(ca, quad, 0);
#define JINC_QUAD8_STEP(LY, CUR, NEXT)                                                                                              \
    if constexpr (LY < 7) quad_fetch(NEXT, quad, LY + 1);                                                                            \
    __builtin_amdgcn_sched_barrier(0);                                                                                               \
    quad_arrived(CUR);                                                                                                               \
    {                                                                                                                                \
        constexpr int S = 4 * ((U + LY) % 8);                                                                                        \
        if constexpr (quad8_trim_of(TR8, LY, 0) == 2)                                                                                \
            quad_row8_t2(acc0, w[S + 1], w[S + 2], CUR[2], CUR[3], CUR[4], CUR[5]);                                                  \
        else if constexpr (quad8_trim_of(TR8, LY, 0) == 1)                                                                           \
            quad_row8_t1(acc0, w[S], w[S + 1], w[S + 2], w[S + 3], CUR[1], CUR[2], CUR[3], CUR[4], CUR[5], CUR[6]);                  \
        else                                                                                                                         \
            quad_row8(acc0, w[S], w[S + 1], w[S + 2], w[S + 3], CUR[0], CUR[1], CUR[2], CUR[3], CUR[4], CUR[5], CUR[6], CUR[7]);     \
        if constexpr (quad8_trim_of(TR8, LY, 1) == 2)                                                                                \
            quad_row8_t2(acc1, w[S + 1], w[S + 2], CUR[10], CUR[11], CUR[12], CUR[13]);                                              \
        else if constexpr (quad8_trim_of(TR8, LY, 1) == 1)                                                                           \
            quad_row8_t1(acc1, w[S], w[S + 1], w[S + 2], w[S + 3], CUR[9], CUR[10], CUR[11], CUR[12], CUR[13], CUR[14]);             \
        else                                                                                                                         \
            quad_row8(acc1, w[S], w[S + 1], w[S + 2], w[S + 3], CUR[8], CUR[9], CUR[10], CUR[11], CUR[12], CUR[13], CUR[14], CUR[15]); \
    }                                                                                                                                \
    __builtin_amdgcn_sched_barrier(0);
    JINC_QUAD8_STEP(0, ca, cb)
    JINC_QUAD8_STEP(1, cb, ca)
    JINC_QUAD8_STEP(2, ca, cb)
    JINC_QUAD8_STEP(3, cb, ca)
    JINC_QUAD8_STEP(4, ca, cb)
    JINC_QUAD8_STEP(5, cb, ca)
    JINC_QUAD8_STEP(6, ca, cb)
    JINC_QUAD8_STEP(7, cb, ca)
#undef JINC_QUAD8_STEP
}

// Two horizontally adjacent samples of a lane through the buffer resource: one 2-sample store.
template <typename T>
__device__ __forceinline__ void store_pair_buf(BufferRsrc rsrc, uint32_t voffset, uint32_t soffset, f32x2 r, float peak) {
    if constexpr (std::is_same_v<T, float>) {
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, r), rsrc, voffset, soffset, 0);
    } else if constexpr (std::is_same_v<T, uint8_t>) {
        uint32_t w = __builtin_amdgcn_cvt_pk_u8_f32(r.x, 0u, 0u);
        w = __builtin_amdgcn_cvt_pk_u8_f32(r.y, 1u, w);
        __builtin_amdgcn_raw_buffer_store_b16(static_cast<uint16_t>(w), rsrc, voffset, soffset, 0);
    } else {
        __builtin_amdgcn_raw_buffer_store_b32(round_pair16<T>(r.x, r.y, peak), rsrc, voffset, soffset, 0);
    }
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>), in order: a loop whose index is a compile-time constant.
template <typename F, int... I>
__device__ __forceinline__ void for_each_index_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void for_each_index(F&& f) {
    for_each_index_impl(f, std::make_integer_sequence<int, N>{});
}

// The three one-period quad kernels are one body (quad_body).  Form: the filter size, the register pairs of the FS x FS window,
// the loader of window slot SLOT and the chains of one output row pair at window rotation U.
struct QuadForm7 {
    static constexpr int FS = 7, kWinPairs = 25;
    template <int SLOT>
    static __device__ __forceinline__ void load_row(f32x2 (&w)[kWinPairs], const float* p) { quad_load_row7<SLOT>(w, p); }
    template <int U>
    static __device__ __forceinline__ void pixel(f32x2& acc0, f32x2& acc1, const f32x2 (&w)[kWinPairs], const JINC_CONSTANT f32x2* quad) {
        quad_pixel7<U>(acc0, acc1, w, quad);
    }
};
struct QuadForm9 {
    static constexpr int FS = 9, kWinPairs = 41;
    template <int SLOT>
    static __device__ __forceinline__ void load_row(f32x2 (&w)[kWinPairs], const float* p) { quad_load_row9<SLOT>(w, p); }
    template <int U>
    static __device__ __forceinline__ void pixel(f32x2& acc0, f32x2& acc1, const f32x2 (&w)[kWinPairs], const JINC_CONSTANT f32x2* quad) {
        quad_pixel9<U>(acc0, acc1, w, quad);
    }
};
template <uint32_t TR8>
struct QuadForm8 {
    static constexpr int FS = 8, kWinPairs = 32;
    template <int SLOT>
    static __device__ __forceinline__ void load_row(f32x2 (&w)[kWinPairs], const float* p) { quad_load_row8<SLOT>(w, p); }
    template <int U>
    static __device__ __forceinline__ void pixel(f32x2& acc0, f32x2& acc1, const f32x2 (&w)[kWinPairs], const JINC_CONSTANT f32x2* quad) {
        quad_pixel8<U, TR8>(acc0, acc1, w, quad);
    }
};

template <typename T, int RG, typename Form>
__device__ __forceinline__ void quad_body(const PeriodicArgs& a, const PlaneIO& io, float* tile) {
    constexpr int FS = Form::FS;
    using Cfg = PeriodicCfg<FS, RG>;
    static_assert(RG % 4 == 0, "the four waves of a workgroup take RG / 4 row groups each");

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int tile_x, tile_y;
    swizzled_tile(tile_x, tile_y);
    const int i0 = tile_x * kTileCols;
    const int j0 = tile_y * Cfg::kTileRows;
    const size_t frame = blockIdx.z;
    if (skips_frame(a, frame)) return;  // float planes: the other launch's frame
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
                if (r < Cfg::kLdsRows && c < Cfg::kLdsCols) tile[r * Cfg::kLdsPitch + c] = nonfinite.take(staged[i][k]);
            }
        }
    }
    __syncthreads();
    if ((i0 + lane) >= a.ni) return;  // no barrier below

    const JINC_CONSTANT f32x2* quad = (const JINC_CONSTANT f32x2*)(a.quad);
    // both phases of an axis share the window origin (host: quad != nullptr only then)
    const float* base = tile + (a.start_y[0] - a.min_sy) * Cfg::kLdsPitch + (a.start_x[0] - a.min_sx) + lane;
    const BufferRsrc drsrc = make_rsrc(static_cast<char*>(io.dst) + frame * io.dst_frame_stride,
                                       static_cast<uint32_t>(io.dst_pitch) * a.dst_h);  // wave-uniform
    const uint32_t xoff = static_cast<uint32_t>(a.ix0 + 2 * (i0 + lane)) * static_cast<uint32_t>(sizeof(T));

    constexpr int kGroupsPerWave = RG / 4;
    const int g_first = wave * kGroupsPerWave;
    if (j0 + g_first * FS >= a.nj) return;  // wave-uniform: bottom tiles
    f32x2 win[Form::kWinPairs];
    const float* wb = base + (g_first * FS) * Cfg::kLdsPitch;
    for_each_index<FS - 1>([&](auto SLOT) __attribute__((always_inline)) {
        constexpr int S = decltype(SLOT)::value;
        Form::template load_row<S>(win, wb + S * Cfg::kLdsPitch);
    });
    for (int g = g_first; g < g_first + kGroupsPerWave; ++g) {
        if (j0 + g * FS >= a.nj) break;  // wave-uniform
        const float* gbase = base + (g * FS) * Cfg::kLdsPitch;
        for_each_index<FS>([&](auto ROW) __attribute__((always_inline)) {  // the group's FS output row pairs, unrolled: the window's rotation is a compile-time constant
            constexpr int U = decltype(ROW)::value;
            Form::template load_row<(U + FS - 1) % FS>(win, gbase + (U + FS - 1) * Cfg::kLdsPitch);
            f32x2 acc0 = {0.f, 0.f}, acc1 = {0.f, 0.f};
            uint32_t zero;
            asm volatile("s_mov_b32 %0, 0" : "=s"(zero));  // opaque: keeps the coefficient loads inside the row loop
            Form::template pixel<U>(acc0, acc1, win, quad + zero);
            const int j = j0 + g * FS + U;
            if (j < a.nj) {
                const uint32_t so = static_cast<uint32_t>(a.iy0 + 2 * j) * io.dst_pitch;
                store_pair_buf<T>(drsrc, xoff, so, acc0, io.peak);
                store_pair_buf<T>(drsrc, xoff, so + static_cast<uint32_t>(io.dst_pitch), acc1, io.peak);
            }
        });
    }
}

template <typename T, int RG>
__global__ __launch_bounds__(256, 6) void ewa_periodic_quad_kernel(const PeriodicArgs a, const PlaneIO io) {
    using Cfg = PeriodicCfg<7, RG>;
    __shared__ float tile[Cfg::kLdsRows * Cfg::kLdsPitch];
    quad_body<T, RG, QuadForm7>(a, io, tile);
}

// fs 9 (tap 4 at 2x: C4): the same kernel with a 9 x 9 window (41 register pairs: 5 waves per SIMD, as the window kernel of
// fs 9) and the coefficient pairs of the two phase rows taken alternately (quad_pixel9).
template <typename T, int RG>
__global__ __launch_bounds__(256, 5) void ewa_periodic_quad9_kernel(const PeriodicArgs a, const PlaneIO io) {
    using Cfg = PeriodicCfg<9, RG>;
    __shared__ float tile[Cfg::kLdsRows * Cfg::kLdsPitch];
    quad_body<T, RG, QuadForm9>(a, io, tile);
}

// The trimmed 8 x 8 support (above): TR8 = the compile-time pattern of its shortened kernel rows.
template <typename T, int RG, uint32_t TR8>
__global__ __launch_bounds__(256, 6) void ewa_periodic_quad8_kernel(const PeriodicArgs a, const PlaneIO io) {
    using Cfg = PeriodicCfg<8, RG>;
    __shared__ float tile[Cfg::kLdsRows * Cfg::kLdsPitch];
    quad_body<T, RG, QuadForm8<TR8>>(a, io, tile);
}

template <typename T, int RG>
int launch_periodic_quad_t(const PeriodicArgs& pa, const PlaneIO& io, hipStream_t stream) {
    using Cfg = PeriodicCfg<7, RG>;
    dim3 grid((pa.ni + kTileCols - 1) / kTileCols, (pa.nj + Cfg::kTileRows - 1) / Cfg::kTileRows, io.nframes);
    hipLaunchKernelGGL((ewa_periodic_quad_kernel<T, RG>), grid, dim3(256, 1, 1), 0, stream, pa, io);
    knobs::note_instance("ewa_periodic_quad_kernel", "%s, %d", knobs::type_name<T>(), RG);
    return static_cast<int>(hipGetLastError());
}

template <typename T, int RG>
int launch_periodic_quad9_t(const PeriodicArgs& pa, const PlaneIO& io, hipStream_t stream) {
    using Cfg = PeriodicCfg<9, RG>;
    dim3 grid((pa.ni + kTileCols - 1) / kTileCols, (pa.nj + Cfg::kTileRows - 1) / Cfg::kTileRows, io.nframes);
    hipLaunchKernelGGL((ewa_periodic_quad9_kernel<T, RG>), grid, dim3(256, 1, 1), 0, stream, pa, io);
    knobs::note_instance("ewa_periodic_quad9_kernel", "%s, %d", knobs::type_name<T>(), RG);
    return static_cast<int>(hipGetLastError());
}

template <typename T, int RG>
int launch_periodic_quad8_t(const PeriodicArgs& pa, const PlaneIO& io, hipStream_t stream) {
    using Cfg = PeriodicCfg<8, RG>;
    dim3 grid((pa.ni + kTileCols - 1) / kTileCols, (pa.nj + Cfg::kTileRows - 1) / Cfg::kTileRows, io.nframes);
    const bool pattern = quad8_pattern_fits(pa.quad_trim8, kQuad8TrimTap4);
    if (pattern)
        hipLaunchKernelGGL((ewa_periodic_quad8_kernel<T, RG, kQuad8TrimTap4>), grid, dim3(256, 1, 1), 0, stream, pa, io);
    else
        hipLaunchKernelGGL((ewa_periodic_quad8_kernel<T, RG, 0u>), grid, dim3(256, 1, 1), 0, stream, pa, io);
    knobs::note_instance("ewa_periodic_quad8_kernel", "%s, %d, %uu", knobs::type_name<T>(), RG, pattern ? kQuad8TrimTap4 : 0u);
    return static_cast<int>(hipGetLastError());
}

}  // namespace

int launch_periodic_quad(const PeriodicArgs& pa, const PlaneIO& io, hipStream_t stream, int fs, int rg) {
    return for_sample_type(io, [&](auto t) {
        using T = decltype(t);
        if (fs == 8 && rg == 8) return launch_periodic_quad8_t<T, 8>(pa, io, stream);
        if (fs == 8 && rg == 4) return launch_periodic_quad8_t<T, 4>(pa, io, stream);
        if (fs == 7 && rg == 8) return launch_periodic_quad_t<T, 8>(pa, io, stream);
        if (fs == 7 && rg == 4) return launch_periodic_quad_t<T, 4>(pa, io, stream);
        if (fs == 9 && rg == 4) return launch_periodic_quad9_t<T, 4>(pa, io, stream);
        return static_cast<int>(hipErrorInvalidValue);
    });
}

}  // namespace jinc
