// kernel_periodic_rows.hip -- periodic interior kernel, row-streamed form: ewa_periodic_rows_kernel for any filter size 3 .. 17
// (RowsCfg, rows_kernel_row, rows_item) and launch_rows_k / launch_rows_t behind launch_periodic_rows.  See kernel_periodic.hip for
// the family, kernel_rowpair.hip for the packed phase-pair form of the same kernel, device_common.hpp for the parity rules.
#include "device_common.hpp"
#include "kernel_periodic_launch.h"
#include "knobs.h"

#pragma clang fp contract(off)

namespace jinc {
namespace {

#include "kernel_periodic_common.inc"

// ------------------------------------------------------------------------------------------------
// Periodic interior kernel, row-streamed form (any filter size, used for fs > 9)
// ------------------------------------------------------------------------------------------------
// Same phase-uniform idea as ewa_periodic_kernel (one phase per wave => coefficients in SGPRs), but
// sized for footprints whose fs x fs window does not fit the register file (fs = 17: 289 values):
//   * a lane owns K = 4 consecutive source-aligned columns and R = 4 consecutive period-rows
//     (16 independent accumulation chains), so one LDS row segment of fs+K-1 samples feeds K*fs taps;
//   * the loop runs ly-major: the fs coefficients of kernel row ly sit in SGPRs and are reused by
//     all 16 pixels; each pixel still sees its taps in (ly, lx) raster order, so every chain is the
//     reference's sequential chain;
//   * the LDS tile is stored as K column-planes (column c -> plane c % K, index c / K) so that the
//     64 lanes of a wave, which are K columns apart, read consecutive LDS words (no bank conflicts).
template <int FS, int KC = 4>
struct RowsCfg {
    static constexpr int K = KC;       // columns per lane (4, or 3 when that wastes fewer overhanging columns)
    static constexpr int R = 4;        // rows per chunk (accumulators per lane = R * K)
    static constexpr int kChunks = 4;  // chunks per tile
    static constexpr int kTileRows = R * kChunks;
    static constexpr int kTileCols = 64 * K;
    static constexpr int kCols = kTileCols + FS;  // + (FS-1) halo + 1 phase spread
    static constexpr int kPlaneMin = 64 + (FS + K - 1) / K + 1;
    static constexpr int kPlane = ((kPlaneMin - 8 + 31) / 32) * 32 + 8;  // == 8 (mod 32): the K planes start on distinct banks
    static constexpr int kRows = kTileRows + FS;  // + (FS-1) halo + 1 phase spread
    // LDS layout [plane][row][index]: every ds_read of a lane stays within 255 dwords of one of K
    // per-plane base registers (ds_read2_b32 immediate range), so the inner loop has no address VALU.
    static constexpr int kPlaneStride = kRows * kPlane;  // kRows is odd -> plane bases fall on distinct banks
    static constexpr int kWaves = 8;
    static constexpr int kThreads = 64 * kWaves;
};

// One kernel row of a rows item on the taps lx = TR .. FS-1-TR: the taps in front of and behind that span carry the
// coefficient 0.0f in this kernel row of this phase (the EWA disc's chord; host: trim_periodic, row_trim) and are left out,
// which is exact for the integer planes the trimmed support is built for.  TR = 0: every tap.
template <int FS, int KC, int OFF, int TR>
__device__ __forceinline__ void rows_kernel_row(float (&acc)[4][KC], const float* __restrict__ tile, const unsigned (&plane_off)[KC],
                                                const JINC_CONSTANT float* crow) {
    using Cfg = RowsCfg<FS, KC>;
    constexpr int K = Cfg::K, R = Cfg::R, N = FS - 2 * TR;
    static_assert(R == 4, "four chain rows per lane");
    float c[N];
#pragma unroll
    for (int lx = 0; lx < N; ++lx) c[lx] = crow[TR + lx];
#pragma unroll
    for (int jj = 0; jj < R; ++jj) {
        float seg[N + K - 1];
#pragma unroll
        for (int u = 0; u < N + K - 1; ++u)
            seg[u] = tile[plane_off[(u + TR + OFF) % K] + (jj * Cfg::kPlane + (u + TR + OFF) / K)];
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int lx = 0; lx < N; ++lx) acc[jj][k] = acc[jj][k] + seg[k + lx] * c[lx];
    }
}

template <typename T, int FS, int KC, int OFF>
__device__ __forceinline__ void rows_item(const float* __restrict__ tile, unsigned base_off, const JINC_CONSTANT float* cs,
                                          const JINC_CONSTANT int32_t* row_trim, int nrows, BufferRsrc drsrc,
                                          int dst_pitch, float peak, int y0, int ystep, int rows_valid, unsigned x0,
                                          unsigned xstep, int cols_valid) {
    using Cfg = RowsCfg<FS, KC>;
    constexpr int K = Cfg::K, R = Cfg::R;
    float acc[R][K];
#pragma unroll
    for (int jj = 0; jj < R; ++jj)
#pragma unroll
        for (int k = 0; k < K; ++k) acc[jj][k] = 0.f;

    // One LDS word offset per plane, kept in its own VGPR (the empty asm stops the compiler from
    // re-deriving plane bases as "base + large constant" with a VALU add in front of every read).
    unsigned plane_off[K];
#pragma unroll
    for (int m = 0; m < K; ++m) {
        plane_off[m] = base_off + m * Cfg::kPlaneStride;
        asm volatile("" : "+v"(plane_off[m]));
    }

    for (int ly = 0; ly < nrows; ++ly) {  // (FS, or fewer on a support that is wider than tall: PeriodicArgs::rows_ny)
        const JINC_CONSTANT float* crow = cs + ly * padded_row(FS);
        // taps this kernel row leaves out on either side (wave-uniform: the phase's, from the plan); spans are offered in
        // steps of one tap up to five, a row whose zero flanks are wider takes the widest
        const int tr = row_trim ? row_trim[ly] : 0;
        if constexpr (FS >= 12) {
            switch (tr) {
                case 0: rows_kernel_row<FS, KC, OFF, 0>(acc, tile, plane_off, crow); break;
                case 1: rows_kernel_row<FS, KC, OFF, 1>(acc, tile, plane_off, crow); break;
                case 2: rows_kernel_row<FS, KC, OFF, 2>(acc, tile, plane_off, crow); break;
                case 3: rows_kernel_row<FS, KC, OFF, 3>(acc, tile, plane_off, crow); break;
                case 4: rows_kernel_row<FS, KC, OFF, 4>(acc, tile, plane_off, crow); break;
                default: rows_kernel_row<FS, KC, OFF, 5>(acc, tile, plane_off, crow); break;
            }
        } else if constexpr (FS >= 6) {
            switch (tr) {
                case 0: rows_kernel_row<FS, KC, OFF, 0>(acc, tile, plane_off, crow); break;
                case 1: rows_kernel_row<FS, KC, OFF, 1>(acc, tile, plane_off, crow); break;
                default: rows_kernel_row<FS, KC, OFF, 2>(acc, tile, plane_off, crow); break;
            }
        } else {
            rows_kernel_row<FS, KC, OFF, 0>(acc, tile, plane_off, crow);
        }
#pragma unroll
        for (int m = 0; m < K; ++m) plane_off[m] += Cfg::kPlane;  // next kernel row
    }
#pragma unroll
    for (int jj = 0; jj < R; ++jj) {
        if (jj < rows_valid) {  // wave-uniform
            const uint32_t soff = static_cast<uint32_t>(y0 + jj * ystep) * dst_pitch;
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (k < cols_valid)
                    store_sample_buf<T>(drsrc, (x0 + k * xstep) * static_cast<uint32_t>(sizeof(T)), soff, acc[jj][k], peak);
        }
    }
}

template <typename T, int FS, int KC>
__global__ __launch_bounds__(512, 8) void ewa_periodic_rows_kernel(const PeriodicArgs a, const PlaneIO io) {
    using Cfg = RowsCfg<FS, KC>;
    constexpr int K = Cfg::K, R = Cfg::R;
    __shared__ float tile[K * Cfg::kPlaneStride];

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
        // all loads in front of the LDS writes: one memory latency per tile instead of one per row (see ewa_periodic_kernel)
        constexpr int kRowsPerWave = (Cfg::kRows + Cfg::kWaves - 1) / Cfg::kWaves;
        constexpr int kColsPerLane = (Cfg::kCols + 63) / 64;
        T staged[kRowsPerWave][kColsPerLane];
        NonFinite<T> nonfinite(a, frame);
#pragma unroll
        for (int i = 0; i < kRowsPerWave; ++i) {
            int gy = gy0 + wave + Cfg::kWaves * i;
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
            const int r = wave + Cfg::kWaves * i;
#pragma unroll
            for (int k = 0; k < kColsPerLane; ++k) {
                const int c = lane + 64 * k;
                if (r < Cfg::kRows && c < Cfg::kCols)
                    tile[(c % K) * Cfg::kPlaneStride + r * Cfg::kPlane + c / K] = nonfinite.take(staged[i][k]);
            }
        }
    }
    __syncthreads();

    const BufferRsrc dframe = make_rsrc(static_cast<char*>(io.dst) + frame * io.dst_frame_stride,
                                        static_cast<uint32_t>(io.dst_pitch) * a.dst_h);
    const int nphase = a.px * a.py;
    const int nitems = nphase * Cfg::kChunks;
    const int cols_valid = a.ni - (i0 + K * lane);  // per lane: how many of its K columns exist
    if (cols_valid <= 0) return;
    for (int item = wave; item < nitems; item += Cfg::kWaves) {
        const int ch = item / nphase;
        const int ph = item - ch * nphase;
        const int q = ph / a.px;
        const int p = ph - q * a.px;
        const int j = j0 + ch * R;  // first period-row of the chunk
        const int rows_valid = a.nj - j;
        if (rows_valid <= 0) continue;
        const int nrows = a.rows_ny ? a.rows_ny : FS;
        const JINC_CONSTANT float* cs =
            (const JINC_CONSTANT float*)(a.coeffs + static_cast<size_t>(a.set[ph]) * (static_cast<size_t>(nrows) * padded_row(FS)));
        const unsigned base = ((a.start_y[q] - a.min_sy) + ch * R) * Cfg::kPlane + lane;
        const int y0 = a.iy0 + a.py * j + q;
        const unsigned x0 = a.ix0 + a.px * (i0 + K * lane) + p;
        const JINC_CONSTANT int32_t* row_trim = a.row_trim ? (const JINC_CONSTANT int32_t*)(a.row_trim) + ph * 32 : nullptr;
        if (a.start_x[p] - a.min_sx)
            rows_item<T, FS, KC, 1>(tile, base, cs, row_trim, nrows, dframe, io.dst_pitch, io.peak, y0, a.py, rows_valid, x0, a.px, cols_valid);
        else
            rows_item<T, FS, KC, 0>(tile, base, cs, row_trim, nrows, dframe, io.dst_pitch, io.peak, y0, a.py, rows_valid, x0, a.px, cols_valid);
    }
}

template <typename T, int FS, int KC>
int launch_rows_k(const PeriodicArgs& pa, const PlaneIO& io, hipStream_t stream) {
    using Cfg = RowsCfg<FS, KC>;
    dim3 grid((pa.ni + Cfg::kTileCols - 1) / Cfg::kTileCols, (pa.nj + Cfg::kTileRows - 1) / Cfg::kTileRows, io.nframes);
    hipLaunchKernelGGL((ewa_periodic_rows_kernel<T, FS, KC>), grid, dim3(Cfg::kThreads, 1, 1), 0, stream, pa, io);
    knobs::note_instance("ewa_periodic_rows_kernel", "%s, %d, %d", knobs::type_name<T>(), FS, KC);
    return static_cast<int>(hipGetLastError());
}

// Tile width 256 (K = 4) or 192 (K = 3) columns: whichever leaves fewer overhanging (idle) lanes in the last tile
// column; ties go to K = 4 (fewer LDS reads per tap).
template <typename T, int FS>
int launch_rows_t(const PeriodicArgs& pa, const PlaneIO& io, hipStream_t stream) {
    const long long cover4 = (pa.ni + 255) / 256 * 256LL, cover3 = (pa.ni + 191) / 192 * 192LL;
    if (cover3 * 100 < cover4 * 97) return launch_rows_k<T, FS, 3>(pa, io, stream);
    return launch_rows_k<T, FS, 4>(pa, io, stream);
}

}  // namespace

int launch_periodic_rows(const PeriodicArgs& pa, const PlaneIO& io, hipStream_t stream, int fs) {
    return for_sample_type(io, [&](auto t) {
        using T = decltype(t);
        switch (fs) {
            case 3: return launch_rows_t<T, 3>(pa, io, stream);
            case 4: return launch_rows_t<T, 4>(pa, io, stream);
            case 5: return launch_rows_t<T, 5>(pa, io, stream);
            case 6: return launch_rows_t<T, 6>(pa, io, stream);
            case 7: return launch_rows_t<T, 7>(pa, io, stream);
            case 8: return launch_rows_t<T, 8>(pa, io, stream);
            case 9: return launch_rows_t<T, 9>(pa, io, stream);
            case 10: return launch_rows_t<T, 10>(pa, io, stream);
            case 11: return launch_rows_t<T, 11>(pa, io, stream);
            case 12: return launch_rows_t<T, 12>(pa, io, stream);
            case 13: return launch_rows_t<T, 13>(pa, io, stream);
            case 14: return launch_rows_t<T, 14>(pa, io, stream);
            case 15: return launch_rows_t<T, 15>(pa, io, stream);
            case 16: return launch_rows_t<T, 16>(pa, io, stream);
            case 17: return launch_rows_t<T, 17>(pa, io, stream);
            default: return static_cast<int>(hipErrorInvalidValue);
        }
    });
}

}  // namespace jinc
