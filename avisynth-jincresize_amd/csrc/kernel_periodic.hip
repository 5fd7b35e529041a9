// kernel_periodic.hip -- interior kernels of exactly phase-periodic plans (integer up-scales): the launcher of the whole family
// and the window kernels.  One translation unit per kernel family:
//   kernel_periodic.hip          (this file) launch_periodic / launch_periodic_fs: which variant and filter size reach which family;
//                                periodic_supported;
//                                ewa_periodic_kernel     fs 6 .. 9: one phase per wave, coefficients in SGPRs, source tile in LDS as
//                                                        fp32, fs x fs register window sliding down the tile (compile-time rotation)
//                                ewa_periodic_pk_kernel  the same with two columns per lane on v_pk_mul_f32 / v_pk_add_f32 (A/B variant)
//   kernel_periodic_quad.hip     2x up-scales, one period per lane: ewa_periodic_quad_kernel / _quad9_ / _quad8_ (7 x 7, 9 x 9, 8 x 8)
//   kernel_periodic_quad2.inc    2x, two periods per lane on the trimmed 6-row support: ewa_periodic_quad2_kernel, frame-pair form;
//                                compiled as kernel_periodic_quad2_rg8.hip and kernel_periodic_quad2_rg4.hip (tiles of 8 / 4 row groups)
//   kernel_periodic_quad2x8.hip  2x, two periods per lane on the trimmed 8-row support: ewa_periodic_quad2x8_kernel
//   kernel_periodic_rows.hip     any fs <= 17: ewa_periodic_rows_kernel, 4 x 4 chains per lane, ly-major loop, column-plane LDS layout
// Shared, included inside namespace jinc { namespace {: kernel_periodic_common.inc (every unit, and kernel_rowpair.hip),
// kernel_periodic_quad_common.inc (the three quad units).  Across units: kernel_periodic_launch.h.
// See device_common.hpp for the parity rules.
#include "device_common.hpp"
#include "kernel_periodic_launch.h"
#include "knobs.h"

#pragma clang fp contract(off)

namespace jinc {
namespace {

#include "kernel_periodic_common.inc"

// ------------------------------------------------------------------------------------------------
// Periodic interior kernel
// ------------------------------------------------------------------------------------------------
template <typename T, int FS, int RG>
__global__ __launch_bounds__(256) void ewa_periodic_kernel(const PeriodicArgs a, const PlaneIO io) {
    using Cfg = PeriodicCfg<FS, RG>;
    __shared__ float tile[Cfg::kLdsRows * Cfg::kLdsPitch];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int tile_x, tile_y;
    swizzled_tile(tile_x, tile_y);
    const int i0 = tile_x * kTileCols;
    const int j0 = tile_y * Cfg::kTileRows;
    const size_t frame = blockIdx.z;
    if (skips_frame(a, frame)) return;  // float planes: the other launch's frame

    // The coefficients of the wave's first phase do not depend on the tile: request them (scalar loads) BEFORE the
    // staging loads and the barrier, so that their latency overlaps the staging instead of following it.
    const int nphase = a.px * a.py;
    float cf[FS * FS];
    if (wave < nphase) {
        const JINC_CONSTANT float* cs0 =
            (const JINC_CONSTANT float*)(a.coeffs + static_cast<size_t>(a.set[wave]) * (FS * padded_row(FS)));
#pragma unroll
        for (int k = 0; k < FS * FS; ++k) cf[k] = cs0[(k / FS) * padded_row(FS) + (k % FS)];
    }

    // ---- stage the source tile as fp32 (each source sample converted once) ----
    {
        const int gx0 = a.min_sx + i0;
        const int gy0 = a.min_sy + j0;
        const char* sbase = static_cast<const char*>(io.src) + frame * io.src_frame_stride;
        // Fully unrolled with all loads in front of the LDS writes: one memory latency per tile instead of one per
        // row (a rolled loop is load -> wait -> write per iteration, 16 round trips during which the block's four
        // waves compute nothing).
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

    for (int ph = wave; ph < nphase; ph += 4) {
        const int q = ph / a.px;
        const int p = ph - q * a.px;

        // wave-uniform coefficients -> SGPRs (the first phase's are already on their way)
        if (ph != wave) {
            const JINC_CONSTANT float* cs =
                (const JINC_CONSTANT float*)(a.coeffs + static_cast<size_t>(a.set[ph]) * (FS * padded_row(FS)));
#pragma unroll
            for (int k = 0; k < FS * FS; ++k) cf[k] = cs[(k / FS) * padded_row(FS) + (k % FS)];
        }

        const float* base = tile + (a.start_y[q] - a.min_sy) * Cfg::kLdsPitch + (a.start_x[p] - a.min_sx) + lane;

        const unsigned x = a.ix0 + a.px * (i0 + lane) + p;  // per-lane output column
        if ((i0 + lane) >= a.ni) continue;                   // whole phase loop under one exec mask
        const BufferRsrc drsrc = make_rsrc(static_cast<char*>(io.dst) + frame * io.dst_frame_stride,
                                           static_cast<uint32_t>(io.dst_pitch) * a.dst_h);  // wave-uniform
        const uint32_t xoff = x * static_cast<uint32_t>(sizeof(T));

        float win[FS][FS];
#pragma unroll
        for (int r = 0; r < FS - 1; ++r)
#pragma unroll
            for (int lx = 0; lx < FS; ++lx) win[r][lx] = base[r * Cfg::kLdsPitch + lx];

        for (int g = 0; g < Cfg::kRowGroups; ++g) {
            if (j0 + g * FS >= a.nj) break;  // wave-uniform: the bottom tiles usually need fewer groups
            const float* gbase = base + (g * FS) * Cfg::kLdsPitch;
#pragma unroll
            for (int u = 0; u < FS; ++u) {
                // newest window row: tile row g*FS + u + FS-1 -> slot (u + FS-1) % FS
#pragma unroll
                for (int lx = 0; lx < FS; ++lx)
                    win[(u + FS - 1) % FS][lx] = gbase[(u + FS - 1) * Cfg::kLdsPitch + lx];

                float acc = 0.f;
#pragma unroll
                for (int ly = 0; ly < FS; ++ly)
#pragma unroll
                    for (int lx = 0; lx < FS; ++lx) acc = acc + win[(u + ly) % FS][lx] * cf[ly * FS + lx];

                const int j = j0 + g * FS + u;  // wave-uniform
                if (j < a.nj) {
                    const int y = a.iy0 + a.py * j + q;
                    store_sample_buf<T>(drsrc, xoff, static_cast<uint32_t>(y) * io.dst_pitch, acc, io.peak);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Periodic interior kernel, packed-math form (experimental A/B variant)
// ------------------------------------------------------------------------------------------------
// Same algorithm as ewa_periodic_kernel, but a lane owns TWO source-aligned columns 64 apart and keeps
// both register windows as 2-vectors, so every tap is one v_pk_mul_f32 + one v_pk_add_f32 (two
// independent IEEE products / sums per instruction; nothing is fused or reassociated: each half is
// exactly the scalar chain).  The coefficient stays in an SGPR and is broadcast to both halves by op_sel.

// acc-independent product of a 2-vector with ONE coefficient taken from the low (HI = false) or high half of
// an aligned SGPR pair, broadcast to both halves by op_sel -- written as asm because the compiler otherwise
// materialises every (c, c) splat as its own SGPR pair (98 SGPRs for fs = 7 -> spills).  Register-only VALU.
// One kernel row (7 taps) of the packed chain as a single asm statement: acc += w[lx] * c[lx], lx = 0..6, each tap
// v_pk_mul_f32 (coefficient = low or high half of an aligned SGPR pair, broadcast to both halves by op_sel)
// followed by v_pk_add_f32 -- un-fused, in order.  One statement per row keeps the compiler's per-statement
// boundary pad (one s_nop) at 1 per 14 instructions; register-only VALU, interlocked by hardware.
__device__ __forceinline__ void pk_row7(f32x2& acc, const f32x2 (&w)[7], f32x2 p01, f32x2 p23, f32x2 p45, f32x2 p6x) {
    f32x2 t;
    asm("v_pk_mul_f32 %1, %2, %9 op_sel_hi:[1,0]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %3, %9 op_sel:[0,1] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %4, %10 op_sel_hi:[1,0]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %5, %10 op_sel:[0,1] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %6, %11 op_sel_hi:[1,0]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %7, %11 op_sel:[0,1] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %0, %0, %1\n\t"
        "v_pk_mul_f32 %1, %8, %12 op_sel_hi:[1,0]\n\t"
        "v_pk_add_f32 %0, %0, %1"
        : "+v"(acc), "=&v"(t)
        : "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]), "v"(w[4]), "v"(w[5]), "v"(w[6]), "s"(p01), "s"(p23), "s"(p45), "s"(p6x));
}

template <int FS, int RG>
struct PeriodicPkCfg {
    static constexpr int kRowGroups = RG;
    static constexpr int kTileRows = FS * RG;
    static constexpr int kTileCols = 128;
    static constexpr int kSrcCols = kTileCols + FS;  // source columns staged per tile row
    // LDS row = pairs: pair k = (source column k, source column 64 + k), k = 0 .. 64+FS-1, so that a lane's two
    // windows (columns lane+lx and 64+lane+lx) arrive as one aligned ds_read_b64 -> one VGPR pair.
    static constexpr int kPairsPerRow = 64 + FS;
    static constexpr int kLdsPitch = 2 * kPairsPerRow + 2;  // floats; even (8-byte aligned rows)
    static constexpr int kLdsRows = kTileRows + FS;
};

template <typename T, int FS, int RG>
__global__ __launch_bounds__(256) void ewa_periodic_pk_kernel(const PeriodicArgs a, const PlaneIO io) {
    using Cfg = PeriodicPkCfg<FS, RG>;
    __shared__ __attribute__((aligned(16))) float tile[Cfg::kLdsRows * Cfg::kLdsPitch];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int tile_x, tile_y;
    swizzled_tile(tile_x, tile_y);
    const int i0 = tile_x * Cfg::kTileCols;
    const int j0 = tile_y * Cfg::kTileRows;
    const size_t frame = blockIdx.z;
    if (skips_frame(a, frame)) return;  // float planes: the other launch's frame
    {
        const int gx0 = a.min_sx + i0;
        const int gy0 = a.min_sy + j0;
        const char* sbase = static_cast<const char*>(io.src) + frame * io.src_frame_stride;
        // all loads in front of the LDS writes (see ewa_periodic_kernel)
        constexpr int kRowsPerWave = (Cfg::kLdsRows + 3) / 4;
        constexpr int kColsPerLane = (Cfg::kSrcCols + 63) / 64;
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
            float* trow = tile + r * Cfg::kLdsPitch;
#pragma unroll
            for (int k = 0; k < kColsPerLane; ++k) {
                const int c = lane + 64 * k;
                if (r < Cfg::kLdsRows && c < Cfg::kSrcCols) {
                    const float v = nonfinite.take(staged[i][k]);
                    if (c < Cfg::kPairsPerRow) trow[2 * c] = v;        // first element of pair c
                    if (c >= 64) trow[2 * (c - 64) + 1] = v;           // second element of pair c - 64
                }
            }
        }
    }
    __syncthreads();

    const int nphase = a.px * a.py;
    for (int ph = wave; ph < nphase; ph += 4) {
        const int q = ph / a.px;
        const int p = ph - q * a.px;
        const JINC_CONSTANT float* cs =
            (const JINC_CONSTANT float*)(a.coeffs + static_cast<size_t>(a.set[ph]) * (FS * padded_row(FS)));
        // coefficient rows as aligned 64-bit SGPR pairs (rows are padded to a multiple of 4 floats)
        constexpr int kPairs = padded_row(FS) / 2;
        const JINC_CONSTANT f32x2* cs2 = (const JINC_CONSTANT f32x2*)cs;
        f32x2 cp[FS * kPairs];
#pragma unroll
        for (int k = 0; k < FS * kPairs; ++k) cp[k] = cs2[k];

        const f32x2* base = reinterpret_cast<const f32x2*>(tile + (a.start_y[q] - a.min_sy) * Cfg::kLdsPitch) +
                            (a.start_x[p] - a.min_sx) + lane;
        constexpr int kPitch2 = Cfg::kLdsPitch / 2;  // row pitch in pairs
        const int ia = i0 + lane;
        if (ia >= a.ni) continue;
        const bool b_ok = ia + 64 < a.ni;
        const BufferRsrc drsrc = make_rsrc(static_cast<char*>(io.dst) + frame * io.dst_frame_stride,
                                           static_cast<uint32_t>(io.dst_pitch) * a.dst_h);
        const uint32_t xoff_a = (a.ix0 + a.px * ia + p) * static_cast<uint32_t>(sizeof(T));
        const uint32_t xoff_b = xoff_a + 64u * a.px * static_cast<uint32_t>(sizeof(T));

        f32x2 win[FS][FS];
#pragma unroll
        for (int r = 0; r < FS - 1; ++r)
#pragma unroll
            for (int lx = 0; lx < FS; ++lx) win[r][lx] = base[r * kPitch2 + lx];

        for (int g = 0; g < Cfg::kRowGroups; ++g) {
            if (j0 + g * FS >= a.nj) break;
            const f32x2* gbase = base + (g * FS) * kPitch2;
#pragma unroll
            for (int u = 0; u < FS; ++u) {
#pragma unroll
                for (int lx = 0; lx < FS; ++lx) win[(u + FS - 1) % FS][lx] = gbase[(u + FS - 1) * kPitch2 + lx];
                f32x2 acc = {0.f, 0.f};
                static_assert(FS == 7, "packed variant is written for fs = 7");
#pragma unroll
                for (int ly = 0; ly < FS; ++ly)
                    pk_row7(acc, win[(u + ly) % FS], cp[ly * kPairs], cp[ly * kPairs + 1], cp[ly * kPairs + 2], cp[ly * kPairs + 3]);
                const int j = j0 + g * FS + u;
                if (j < a.nj) {
                    const uint32_t soff = static_cast<uint32_t>(a.iy0 + a.py * j + q) * io.dst_pitch;
                    store_sample_buf<T>(drsrc, xoff_a, soff, acc.x, io.peak);
                    if (b_ok) store_sample_buf<T>(drsrc, xoff_b, soff, acc.y, io.peak);
                }
            }
        }
    }
}

template <typename T, int FS, int RG = PeriodicCfg<FS>::kRowGroups>
int launch_periodic_t(const PeriodicArgs& pa, const PlaneIO& io, hipStream_t stream) {
    using Cfg = PeriodicCfg<FS, RG>;
    dim3 grid((pa.ni + kTileCols - 1) / kTileCols, (pa.nj + Cfg::kTileRows - 1) / Cfg::kTileRows, io.nframes);
    hipLaunchKernelGGL((ewa_periodic_kernel<T, FS, RG>), grid, dim3(256, 1, 1), 0, stream, pa, io);
    knobs::note_instance("ewa_periodic_kernel", "%s, %d, %d", knobs::type_name<T>(), FS, RG);
    return static_cast<int>(hipGetLastError());
}

template <typename T, int FS, int RG>
int launch_periodic_pk_t(const PeriodicArgs& pa, const PlaneIO& io, hipStream_t stream) {
    using Cfg = PeriodicPkCfg<FS, RG>;
    dim3 grid((pa.ni + Cfg::kTileCols - 1) / Cfg::kTileCols, (pa.nj + Cfg::kTileRows - 1) / Cfg::kTileRows, io.nframes);
    hipLaunchKernelGGL((ewa_periodic_pk_kernel<T, FS, RG>), grid, dim3(256, 1, 1), 0, stream, pa, io);
    knobs::note_instance("ewa_periodic_pk_kernel", "%s, %d, %d", knobs::type_name<T>(), FS, RG);
    return static_cast<int>(hipGetLastError());
}

// The window kernel and its packed variant for the sample type of the launch.
template <int FS, int RG = PeriodicCfg<FS>::kRowGroups>
int launch_window(const PeriodicArgs& pa, const PlaneIO& io, hipStream_t stream) {
    return for_sample_type(io, [&](auto t) { return launch_periodic_t<decltype(t), FS, RG>(pa, io, stream); });
}
template <int RG>
int launch_pk(const PeriodicArgs& pa, const PlaneIO& io, hipStream_t stream) {
    return for_sample_type(io, [&](auto t) { return launch_periodic_pk_t<decltype(t), 7, RG>(pa, io, stream); });
}

// Which variant and filter size reach which family: here and nowhere else.  The families behind launch_periodic_quad2_rg8 / _rg4 /
// _quad2x8 / _quad / _rows are units of their own (kernel_periodic_launch.h).
int launch_periodic_fs(const PeriodicArgs& pa, int fs, const PlaneIO& io, hipStream_t stream, int variant) {
    if ((variant == 5 || variant == 6) && fs == 6 && pa.quad)  // trimmed support, two periods per lane: 5 = tiles of 8 row groups, 6 = of 4
        return variant == 5 ? launch_periodic_quad2_rg8(pa, io, stream) : launch_periodic_quad2_rg4(pa, io, stream);
    if (variant == 7 && fs == 8 && pa.quad) return launch_periodic_quad2x8(pa, io, stream);  // two periods per lane
    // Border columns handed over with the interior launch (PeriodicArgs::edge) are computed by the two launchers above and by
    // nobody else: a caller that dropped its own column launches on the strength of them and then lands anywhere below -- a knob
    // changed between its decision and this one, a rule edited on one side only -- must hear about it, not ship frames with
    // unwritten columns.
    if (pa.edge.coeffs) return static_cast<int>(hipErrorInvalidValue);
    if ((variant == 5 || variant == 6) && fs == 8 && pa.quad)  // trimmed 8 x 8 support: 5 = tiles of 8 row groups, 6 = of 4
        return launch_periodic_quad(pa, io, stream, 8, variant == 5 ? 8 : 4);
    if ((variant == 5 || variant == 6) && fs == 7 && pa.quad)  // quad form: 5 = tiles of 8 row groups, 6 = of 4 (small calls)
        return launch_periodic_quad(pa, io, stream, 7, variant == 5 ? 8 : 4);
    if ((variant == 5 || variant == 6) && fs == 9 && pa.quad)
        return launch_periodic_quad(pa, io, stream, 9, 4);  // (8 row groups per tile: the staging's registers spill, no gain over the window kernel)
    if (variant == 3 && fs == 7) return launch_pk<4>(pa, io, stream);
    if (variant == 4 && fs == 7) return launch_pk<8>(pa, io, stream);
    if (variant == 2 && fs == 7) return launch_window<7, 4>(pa, io, stream);
    if (variant == 2 && fs == 9) return launch_window<9, 6>(pa, io, stream);
    if (variant == 2 && fs == 6) return launch_window<6, 4>(pa, io, stream);
    if (variant == 2 && fs == 8) return launch_window<8, 5>(pa, io, stream);
    if (variant == 1 && (fs == 7 || fs == 9 || fs == 6 || fs == 8)) return launch_periodic_rows(pa, io, stream, fs);
    switch (fs) {  // (even sizes: trimmed supports of integer planes, device_plan.cpp trim_periodic)
        case 3:
        case 4:
        case 5: return launch_periodic_rows(pa, io, stream, fs);
        case 6: return launch_window<6>(pa, io, stream);
        case 7: return launch_window<7>(pa, io, stream);
        case 8: return launch_window<8>(pa, io, stream);
        case 9: return launch_window<9>(pa, io, stream);
        case 10:
        case 11:
        case 12:
        case 13:
        case 14:
        case 15:
        case 16:
        case 17: return launch_periodic_rows(pa, io, stream, fs);
        default: return static_cast<int>(hipErrorInvalidValue);
    }
}

}  // namespace

bool periodic_supported(int fs, int px, int py, int sx, int sy) {
    if (sx != 1 || sy != 1) return false;
    if (px < 1 || py < 1 || px > 8 || py > 8) return false;
    return fs >= 3 && fs <= 17 && (fs & 1);  // taps 1..8 at >= 1x scale
}

int launch_periodic(const PeriodicArgs& args, int fs, const PlaneIO& io, void* stream, int variant) {
    if (args.ni <= 0 || args.nj <= 0 || io.nframes <= 0) return 0;
    // 2x up-scales with 12 .. 17 taps per kernel row: the rows kernel's packed phase-pair form (kernel_rowpair.hip) wherever the
    // plan carries its coefficient pairs; variant 1 (kernel mode 3) and the knob ROWS_PAIR = 0 keep ewa_periodic_rows_kernel
    // Short kernel rows (6 .. 9 taps: taps 3 and 4) stay with the window and quad forms, which measure ahead there (C2 847 : 816
    // Gpix/s, C4 152 : 139; profiles/round5/rowpair_small_ab.log); the knob ROWPAIR_SMALL = 1 puts them on the pair form wherever
    // the plan carries the pairs and no A/B variant of the other kernels is asked for.
    if (args.rowpair && knobs::flag(JINC_KNOB_ROWS_PAIR, true)) {
        const int taps = args.quad_taps ? args.quad_taps : fs;  // (6 rows x 7 columns: fs = 6 rows, 7 taps per row)
        const bool auto_variant = variant == 0 || variant == 2 || variant == 5 || variant == 6 || variant == 7;
        if (args.rowpair_n == taps && !args.edge.coeffs &&  // (edge columns: the caller counts on a two-periods quad form)
            ((fs >= 10 && variant == 0) || (fs < 10 && auto_variant && knobs::geti(JINC_KNOB_ROWPAIR_SMALL, 0) == 1)))
            return launch_rowpair(args, io, stream);
    }
    return launch_periodic_fs(args, fs, io, static_cast<hipStream_t>(stream), variant);
}

}  // namespace jinc
