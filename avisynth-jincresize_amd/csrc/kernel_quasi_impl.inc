// kernel_quasi_impl.inc -- body of the quasi-periodic kernel for ONE filter size (JINC_QUASI_FS), included by
// kernel_quasi[_exact|_lane]_fs{7,9}.hip so that sizes and variants compile in parallel.  JINC_QUASI_EXACT selects
// the variant: 1 = exactly periodic plans (one set per phase in SGPRs, no per-row lookup); 0 = drifting plans with a
// waterfall over the distinct sets of the wave (coefficients in SGPRs); 2 = drifting plans with PER-LANE coefficient
// registers (no waterfall).
#include "device_common.hpp"

#pragma clang fp contract(off)

namespace jinc {
namespace {

// ------------------------------------------------------------------------------------------------
// Quasi-periodic interior kernel (ratios whose phases drift: 1.5x, 3x, ...)
// ------------------------------------------------------------------------------------------------
// The reference accumulates output positions in float, so for ratios such as 3/2 or 3 the quantised
// phase of a column/row is only NEARLY periodic: along 1920 columns a residue class changes its
// coefficient class about ten times.  The window ORIGINS, however, stay exactly affine per residue.
// This kernel keeps everything of ewa_periodic_kernel that depends on the origins only -- source tile
// staged once as fp32 in LDS, lanes = consecutive periods, fs x fs register window sliding down the
// tile with compile-time rotation (SY new source rows per output row) -- and looks the coefficient set
// up per (row, lane): row class from an LDS copy (wave-uniform), lane class loaded once per phase, set id
// from an LDS copy of the class-pair table.  Variant 0: the set of the previous row stays in SGPRs and a waterfall
// over the distinct sets of the wave runs one pass per set.  That looked cheap on paper (a residue class changes its
// coefficient class ~10 times along 1920 columns) but those ten change points fall into ten different 64-lane groups:
// on 1.5x, 57 % of all wave-rows hold two sets and 20 % three (2.4x the ideal VALU instruction count by PMC).
// Variant 2 therefore gives every lane ITS OWN 49 / 81 coefficient registers, loaded with 16-byte per-lane loads
// (lanes of one set share the address) when the lane's set changes -- which happens only when the wave-uniform row
// class changes (about ten times along the height) or a new phase starts -- so every row is one pass of
// v_mul_f32 / v_add_f32 on two VGPR operands, whatever the mix of sets in the wave.
template <typename T, int FS, int SX, int SY, int VARIANT>
__global__ __launch_bounds__(256) void ewa_quasi_kernel(const QuasiArgs a, const PlaneIO io) {
    constexpr bool EXACT = VARIANT == 1;
    constexpr bool LANE_COEF = VARIANT == 2;
    extern __shared__ __attribute__((aligned(16))) float q_smem[];
    float* tile = q_smem;
    int* l_iset = reinterpret_cast<int*>(tile + a.lds_rows * quasi_pitch_words(FS, SX));
    int* l_rc = l_iset + a.n_row_classes * a.n_col_classes;

    const int nthreads = blockDim.x;
    const int nwaves = nthreads >> 6;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile_rows = a.rg * FS;  // output rows (per row phase) of a tile
    int tile_x, tile_y;
    swizzled_tile(tile_x, tile_y);
    const int i0 = tile_x * 64;
    const int j0 = tile_y * tile_rows;
    // blockIdx.z = (frame, share of the tile's phases): small calls split a tile's phases over several workgroups, each
    // staging the tile again -- one frame of a plan with 72 phases is otherwise 72 workgroups of 18 phases per wave
    const int split = a.phase_split;
    const size_t frame = blockIdx.z / split;
    const int share = blockIdx.z % split;
    constexpr int pitch = quasi_pitch_words(FS, SX);   // compile-time: all LDS offsets below are immediates
    constexpr int kPlane = quasi_plane_words(FS, SX);

    {
        const int gx0 = a.min_sx + SX * i0;
        const int gy0 = a.min_sy + SY * j0;
        const char* sbase = static_cast<const char*>(io.src) + frame * io.src_frame_stride;
        // Four rows per wave and pass, all loads in front of the LDS writes: a rolled load -> wait -> write loop costs
        // one memory round trip per row during which the block computes nothing.
        constexpr int kColsPerLane = (quasi_tile_cols(FS, SX) + 63) / 64;
        for (int r0 = wave; r0 < a.lds_rows; r0 += 4 * nwaves) {
            T staged[4][kColsPerLane];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int gy = gy0 + r0 + i * nwaves;
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
            for (int i = 0; i < 4; ++i) {
                const int r = r0 + i * nwaves;
#pragma unroll
                for (int k = 0; k < kColsPerLane; ++k) {
                    const int c = lane + 64 * k;
                    // SX column planes per row (column c -> plane c % SX, index c / SX): the lanes of a wave are SX
                    // source columns apart, so within a plane they read consecutive LDS words (no bank conflicts)
                    if (r < a.lds_rows && c < a.lds_cols) tile[r * pitch + (c % SX) * kPlane + c / SX] = to_float(staged[i][k]);
                }
            }
        }
        if constexpr (!EXACT) {
            const int ntab = a.n_row_classes * a.n_col_classes;
            for (int k = threadIdx.x; k < ntab; k += nthreads) l_iset[k] = a.interior_set[k];
            // classes of the tile's output rows, in output order: entry py*jj + q <-> row iy0 + py*(j0+jj) + q
            const int nrows = a.py * tile_rows;
            for (int k = threadIdx.x; k < nrows; k += nthreads) {
                const int jj = k / a.py;
                l_rc[k] = (j0 + jj) < a.nj ? a.row_class[a.iy0 + a.py * j0 + k] : 0;
            }
        }
    }
    __syncthreads();

    const BufferRsrc drsrc = make_rsrc(static_cast<char*>(io.dst) + frame * io.dst_frame_stride,
                                       static_cast<uint32_t>(io.dst_pitch) * a.dst_h);
    const int nphase = a.px * a.py;
    for (int ph = wave + nwaves * share; ph < nphase; ph += nwaves * split) {
        const int q = ph / a.px;
        const int p = ph - q * a.px;
        const int ia = i0 + lane;
        const bool valid = ia < a.ni;
        const unsigned long long valid_mask = __ballot(valid);
        if (valid_mask == 0) continue;
        const unsigned x = a.ix0 + a.px * (valid ? ia : i0) + p;
        int cc = 0;
        if constexpr (!EXACT) cc = a.col_class[x];  // one global load per phase and lane
        const uint32_t xoff = x * static_cast<uint32_t>(sizeof(T));
        // one base pointer per plane: source column off + lx (lx = SX*k + m) lives at bptr[m][k]
        const int off = a.start_x[p] - a.min_sx;
        const float* bptr[SX];
#pragma unroll
        for (int m = 0; m < SX; ++m)
            bptr[m] = tile + (a.start_y[q] - a.min_sy) * pitch + ((off + m) % SX) * kPlane + (off + m) / SX + lane;

        float win[FS][FS];
#pragma unroll
        for (int r = 0; r < FS - SY; ++r)
#pragma unroll
            for (int lx = 0; lx < FS; ++lx) win[r][lx] = bptr[lx % SX][r * pitch + lx / SX];

        float cf[FS * FS];
        int cur_set = -1;   // variant 0: set sitting in the SGPRs
        int cur_rc = -1;    // variant 2: row class the lanes' coefficient registers were loaded for
        if constexpr (EXACT) {
            // exactly periodic plan: one set per phase, resolved on the host
            const int set_ph = a.phase_set[ph];
            const JINC_CONSTANT float* cs =
                (const JINC_CONSTANT float*)(a.coeffs + static_cast<size_t>(set_ph) * (FS * padded_row(FS)));
#pragma unroll
            for (int k = 0; k < FS * FS; ++k) cf[k] = cs[(k / FS) * padded_row(FS) + (k % FS)];
        } else {
#pragma unroll
            for (int k = 0; k < FS * FS; ++k) cf[k] = 0.f;
        }

        for (int g = 0; g < a.rg; ++g) {
            if (j0 + g * FS >= a.nj) break;  // wave-uniform
            const int grow = (SY * g * FS) * pitch;
#pragma unroll
            for (int t = 0; t < FS; ++t) {
                // window of output row t covers relative source rows SY*t .. SY*t+FS-1; the SY newest arrive now
#pragma unroll
                for (int k = 0; k < SY; ++k) {
                    const int rel = SY * t + FS - SY + k;
#pragma unroll
                    for (int lx = 0; lx < FS; ++lx) win[rel % FS][lx] = bptr[lx % SX][grow + rel * pitch + lx / SX];
                }
                const int jj = g * FS + t;
                if constexpr (EXACT) {
                    if (j0 + jj < a.nj && valid) {
                        float acc = 0.f;
#pragma unroll
                        for (int ly = 0; ly < FS; ++ly)
#pragma unroll
                            for (int lx = 0; lx < FS; ++lx) acc = acc + win[(SY * t + ly) % FS][lx] * cf[ly * FS + lx];
                        const int y = a.iy0 + a.py * (j0 + jj) + q;
                        store_sample_buf<T>(drsrc, xoff, static_cast<uint32_t>(y) * io.dst_pitch, acc, io.peak);
                    }
                } else if (j0 + jj < a.nj) {  // wave-uniform
                    const int rc = __builtin_amdgcn_readfirstlane(l_rc[a.py * jj + q]);
                    if constexpr (LANE_COEF) {
                        if (rc != cur_rc) {  // wave-uniform: first row of the phase, then only where the row class drifts
                            const int set = l_iset[rc * a.n_col_classes + cc];
                            const float4* c4 = reinterpret_cast<const float4*>(a.coeffs + static_cast<size_t>(set) * (FS * padded_row(FS)));
#pragma unroll
                            for (int ly = 0; ly < FS; ++ly)
#pragma unroll
                                for (int v = 0; v < padded_row(FS) / 4; ++v) {
                                    const float4 c = c4[ly * (padded_row(FS) / 4) + v];
                                    if (4 * v + 0 < FS) cf[ly * FS + 4 * v + 0] = c.x;
                                    if (4 * v + 1 < FS) cf[ly * FS + 4 * v + 1] = c.y;
                                    if (4 * v + 2 < FS) cf[ly * FS + 4 * v + 2] = c.z;
                                    if (4 * v + 3 < FS) cf[ly * FS + 4 * v + 3] = c.w;
                                }
                            cur_rc = rc;
                        }
                        if (valid) {
                            float acc = 0.f;
#pragma unroll
                            for (int ly = 0; ly < FS; ++ly)
#pragma unroll
                                for (int lx = 0; lx < FS; ++lx) acc = acc + win[(SY * t + ly) % FS][lx] * cf[ly * FS + lx];
                            const int y = a.iy0 + a.py * (j0 + jj) + q;
                            store_sample_buf<T>(drsrc, xoff, static_cast<uint32_t>(y) * io.dst_pitch, acc, io.peak);
                        }
                        continue;
                    }
                    const int set = l_iset[rc * a.n_col_classes + cc];
                    float acc = 0.f;
                    unsigned long long todo = valid_mask;
                    while (todo) {
                        // lanes that use the set already sitting in SGPRs go first: a wave that straddles a
                        // change point then reloads one set per row instead of two
                        const unsigned long long cached = __ballot(set == cur_set) & todo;
                        const int leader = __ffsll(static_cast<long long>(cached ? cached : todo)) - 1;
                        const int u = __builtin_amdgcn_readlane(set, leader);
                        if (u != cur_set) {  // wave-uniform: only at the class change points of the drift
                            const JINC_CONSTANT float* cs =
                                (const JINC_CONSTANT float*)(a.coeffs + static_cast<size_t>(u) * (FS * padded_row(FS)));
#pragma unroll
                            for (int k = 0; k < FS * FS; ++k) cf[k] = cs[(k / FS) * padded_row(FS) + (k % FS)];
                            cur_set = u;
                        }
                        const bool mine = valid && set == u;
                        if (mine) {
#pragma unroll
                            for (int ly = 0; ly < FS; ++ly)
#pragma unroll
                                for (int lx = 0; lx < FS; ++lx)
                                    acc = acc + win[(SY * t + ly) % FS][lx] * cf[ly * FS + lx];
                        }
                        todo &= ~__ballot(mine);
                    }
                    if (valid) {
                        const int y = a.iy0 + a.py * (j0 + jj) + q;
                        store_sample_buf<T>(drsrc, xoff, static_cast<uint32_t>(y) * io.dst_pitch, acc, io.peak);
                    }
                }
            }
        }
    }
}


template <typename T, int FS, int SX, int SY>
int launch_quasi_t(const QuasiArgs& qa, const PlaneIO& io, hipStream_t stream) {
    const size_t lds = sizeof(float) * static_cast<size_t>(qa.lds_rows) * qa.lds_pitch +
                       sizeof(int) * (static_cast<size_t>(qa.n_col_classes) * qa.n_row_classes + qa.py * qa.rg * FS);
    const int tile_rows = qa.rg * FS;
    dim3 grid((qa.ni + 63) / 64, (qa.nj + tile_rows - 1) / tile_rows, io.nframes * (qa.phase_split > 0 ? qa.phase_split : 1));
    hipLaunchKernelGGL((ewa_quasi_kernel<T, FS, SX, SY, JINC_QUASI_EXACT>), grid, dim3(64 * qa.nwaves, 1, 1), lds, stream, qa, io);
    return static_cast<int>(hipGetLastError());
}
template <typename T, int FS, int SX>
int launch_quasi_sy(const QuasiArgs& qa, const PlaneIO& io, hipStream_t stream) {
    switch (qa.sy) {
        case 1: return launch_quasi_t<T, FS, SX, 1>(qa, io, stream);
        case 2: return launch_quasi_t<T, FS, SX, 2>(qa, io, stream);
        case 3: return launch_quasi_t<T, FS, SX, 3>(qa, io, stream);
        default: return launch_quasi_t<T, FS, SX, 4>(qa, io, stream);
    }
}
template <typename T, int FS>
int launch_quasi_sx(const QuasiArgs& qa, const PlaneIO& io, hipStream_t stream) {
    switch (qa.sx) {
        case 1: return launch_quasi_sy<T, FS, 1>(qa, io, stream);
        case 2: return launch_quasi_sy<T, FS, 2>(qa, io, stream);
        case 3: return launch_quasi_sy<T, FS, 3>(qa, io, stream);
        default: return launch_quasi_sy<T, FS, 4>(qa, io, stream);
    }
}
}  // namespace

#define JINC_CAT2(a, b) a##b
#define JINC_CAT(a, b) JINC_CAT2(a, b)
#if JINC_QUASI_EXACT == 1
#define JINC_QUASI_ENTRY JINC_CAT(launch_quasi_exact_fs, JINC_QUASI_FS)
#elif JINC_QUASI_EXACT == 2
#define JINC_QUASI_ENTRY JINC_CAT(launch_quasi_lane_fs, JINC_QUASI_FS)
#else
#define JINC_QUASI_ENTRY JINC_CAT(launch_quasi_fs, JINC_QUASI_FS)
#endif
int JINC_QUASI_ENTRY(const QuasiArgs& args, const PlaneIO& io, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (io.sample_bytes) {
        case 1: return launch_quasi_sx<uint8_t, JINC_QUASI_FS>(args, io, s);
        case 2:
            if (io.sample_kind == kSampleHalf) return launch_quasi_sx<half_t, JINC_QUASI_FS>(args, io, s);
            if (io.sample_kind == kSampleBFloat16) return launch_quasi_sx<bf16_t, JINC_QUASI_FS>(args, io, s);
            return launch_quasi_sx<uint16_t, JINC_QUASI_FS>(args, io, s);
        default: return launch_quasi_sx<float, JINC_QUASI_FS>(args, io, s);
    }
}

}  // namespace jinc
