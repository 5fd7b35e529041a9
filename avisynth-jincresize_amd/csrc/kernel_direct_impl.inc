// kernel_direct_impl.inc -- ewa_direct_kernel (included by kernel_direct.hip and the kernel_direct_walk_*.hip units):
// exactly phase-periodic plans of ANY filter size and source step 1..4, without an LDS tile.  Two roles (MODE):
//   kDirectInterior  the interior of plans the register/LDS kernels of kernel_periodic*.hip do not cover: integer and
//                    rational down-scales (1/2: fs 13 step 2, 1/3: fs 20 step 3, 2/3: fs 10 step 3 period 2, ...)
//                    and up-scales with taps 9..16 (fs 19..33);
//   kDirectRowStrip  the top/bottom border rows of EVERY exactly periodic plan (interior column range): a border row
//                    is an interior row with its own window origin and its own coefficient set per column phase.
// The left/right border columns are kernel_colstrip.hip's (lanes have to run along y there -- without LDS staging that
// is one cache line per lane and fetch, measured 3x slower); the four corners stay with the gather kernel.
// See device_common.hpp for the parity rules.
//
// Why no LDS tile: a down-scale by s reads s*s source samples per output sample, so an fp32 LDS tile for the
// 16 chains x 64 lanes of one wave costs 36 KB at s = 3 before the (fs-1)-wide halo -- two waves per CU.  Instead
// every lane reads the row segment its K adjacent output columns share straight from memory in the SOURCE format
// (u8: 1 byte per sample) with 16-byte buffer loads and converts it in registers; L1/L2 supply the reuse between
// lanes and waves.  In the interior's row-walk forms (DirectShape 2 / 3, the default) a lane fetches and converts every
// source row segment of its item once and all chain rows that meet the row accumulate from it (see "Row walk" below);
// the round-1 form (shape 0: one fetch per chain row and kernel row) remains for filter sizes the walk's step scheme
// does not cover and for the strips.
// Buffer loads are bounds-checked by the hardware against the plane's size and only naturally aligned dwords are
// fetched, so the whole-segment fetches (up to a block of taps past the window, whole segments of partially valid
// lanes, one step past an item's last source row) can never leave the aligned dwords that hold the plane.
#include <cstdlib>

#include "device_common.hpp"

#pragma clang fp contract(off)

namespace jinc {
namespace {

enum : int { kDirectInterior = 0, kDirectRowStrip = 1, kDirectRuns = 2 };

// Chains per lane.  K adjacent output columns of one phase share a row segment; R output rows of one phase share
// the coefficients (a strip row owns a coefficient set: R = 1).
// B: taps per step of the lx loop -- a step's segment (B + SX*(K-1) samples) is what a lane holds in registers.
// D: steps whose segments are fetched together before any of them is computed.  The interior has enough waves in
// flight to hide the fetch latency by switching; the strip launches do not.
// SHAPE (interior only):
//   0  4 columns x 4 rows per lane, every chain row fetches its own segments (the round-1 form; any fs)
//   2  4 columns x 4 rows, row walk: the item's SOURCE rows are walked once, each segment is fetched and converted once
//      and every chain row that meets the source row at one of its kernel rows accumulates from it (direct_row_walk)
//   3  8 columns x 4 rows, row walk
// The wide shape fetches and converts NT + 7*SX samples per 8 columns instead of NT + 3*SX per 4 (fs 13, step 2: 3.4
// instead of 4.75 samples per chain and kernel row) and holds 32 accumulators; kernel_direct.hip takes it for 8-bit
// batches that fill the device.
template <typename T, int MODE, int SHAPE = 0>
struct DirectShape {
    static constexpr bool kWalk = SHAPE >= 2;
    static constexpr int K = SHAPE == 3 ? 8 : 4;
    static constexpr int R = MODE != kDirectRowStrip ? 4 : 1;
    static constexpr int B = MODE != kDirectRowStrip ? 16 : 8;
    static constexpr int D = MODE != kDirectRowStrip ? 1 : 4;
};
// Waves per SIMD the register allocation has to leave room for.  The 4-column walk over float planes at source steps 1 / 2 needs
// 81 registers when left alone -- one allocation step above the 80 that six waves may have; held to 80 its single-step loops
// (WalkFixed) still keep everything in registers (the multi-step form with 16-tap steps spills 4 dwords).  Float 4K -> 1080p
// +3.5 % on top of the folded offsets (same A/B); longer segments (steps 3 / 4) would spill by the hundred: no bound there.
#ifndef JINC_DIRECT_WALK_WAVES
#define JINC_DIRECT_WALK_WAVES 6  // (-DJINC_DIRECT_WALK_WAVES=1: no bound, for A/B builds)
#endif
template <typename T, int SX, int MODE, int SHAPE>
constexpr int direct_min_waves() {
    return (MODE != kDirectRowStrip && SHAPE == 2 && SX <= 2 && sizeof(T) == 4) ? JINC_DIRECT_WALK_WAVES : 1;
}

// Row segment of a lane in the source format: RW naturally aligned dwords from byte offset voffset (+ soffset), both
// multiples of 4, fetched as 16/8/4-byte pieces.  The lane's first sample sits SH = 0..3 bytes into the first dword;
// SH is the same for every lane of a wave (the lane stride SX*4 samples is a multiple of 4 bytes) and a template
// parameter of everything below, so the samples are picked out of the aligned dwords by the conversion itself
// (v_cvt_f32_ubyteN / SDWA word select) -- no funnel shifts.  Nothing outside the aligned dwords that hold the
// plane's samples is ever touched: the buffer resource bounds the rest.
// The wave-uniform row offset travels in the instruction's soffset.  LLVM documents soffset of raw.buffer.load as
// "excluded from bounds checking"; on gfx950 the hardware does include it -- a fetch is out of range when
// voffset + imm + soffset reaches num_records, also for soffset alone beyond num_records (measured:
// profiles/probes/soffset_probe.hip, profiles/round2/soffset_probe.log).  Because everything here rests on that, the same
// probe runs on the device when a filter is created (buffer_range_check_covers_soffset) and the direct kernel is not
// used where it fails; tests/test_gpu_parity.py::test_buffer_range_check_premise pins it too.  (Moving the row offset
// into a per-row descriptor instead costs 20 % of this issue-bound kernel's speed: D12 60 -> 48 % of the VALU peak.)
template <int RW, bool FOLD = false>
__device__ __forceinline__ void load_raw(BufferRsrc rsrc, uint32_t voffset, uint32_t soffset, uint32_t (&raw)[RW]) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    // FOLD: the constant parts of the piece addresses go into the instructions' immediate offsets.  Left alone, the compiler forms
    // voffset + 16, + 32, ... once in front of the row loop and keeps each in a register of its own (5 for a float segment).
    // Same-box A/B (profiles/round3/direct_registers_ab.txt): float 4K -> 1080p +3.5 %, 8-bit +0.8 %, 16-bit -4 % -- so not there.
    if constexpr (FOLD) asm volatile("" : "+v"(voffset));
    int w = 0;
#pragma unroll
    for (; w + 4 <= RW; w += 4) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voffset + 4 * w, soffset, 0);
        raw[w] = v.x, raw[w + 1] = v.y, raw[w + 2] = v.z, raw[w + 3] = v.w;
    }
    if constexpr (RW % 4 >= 2) {
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, voffset + 4 * w, soffset, 0);
        raw[w] = v.x, raw[w + 1] = v.y;
        w += 2;
    }
    if constexpr (RW % 2 == 1) raw[w] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, voffset + 4 * w, soffset, 0);
}

// dwords that hold NS samples starting SH bytes into the first one
template <typename T>
__host__ __device__ constexpr int segment_words(int ns, int sh) {
    return (ns * static_cast<int>(sizeof(T)) + sh + 3) / 4;
}

template <typename T, int NS, int RW, int SH>
__device__ __forceinline__ void convert_segment(const uint32_t (&raw)[RW], float (&seg)[NS]) {
    static_assert(NS * static_cast<int>(sizeof(T)) + SH <= 4 * RW, "segment larger than its raw words");
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        constexpr int SB = static_cast<int>(sizeof(T));
        const int b = i * SB + SH;  // byte position of sample i in the raw words (compile-time after unrolling)
        if constexpr (sizeof(T) == 1)
            seg[i] = static_cast<float>((raw[b / 4] >> (8 * (b % 4))) & 0xffu);  // v_cvt_f32_ubyteN
        else if constexpr (std::is_same_v<T, half_t>)
            seg[i] = (b % 4) ? half_hi(raw[b / 4]) : half_lo(raw[b / 4]);
        else if constexpr (std::is_same_v<T, bf16_t>)
            seg[i] = (b % 4) ? bf16_hi(raw[b / 4]) : bf16_lo(raw[b / 4]);  // a mask or a shift, no conversion
        else if constexpr (sizeof(T) == 2)
            seg[i] = static_cast<float>((raw[b / 4] >> (8 * (b % 4))) & 0xffffu);  // SDWA word select
        else
            seg[i] = __builtin_bit_cast(float, raw[b / 4]);
    }
}

// NT taps (lx = lx0 .. lx0+NT-1) of kernel row ly for all R x K chains of the lane, from segments already in
// registers.  Every chain still meets its taps in (ly, lx) raster order: steps run in lx order inside ly order.
template <typename T, int SX, int NT, int R, int K, int RW, int NC, int SH>
__device__ __forceinline__ void mac_rows(float (&acc)[R][K], const uint32_t (&raw)[R][RW], const float (&cf)[NC]) {
    constexpr int NS = NT + SX * (K - 1);
#pragma unroll
    for (int jj = 0; jj < R; ++jj) {
        // The tail variants (NT = 1 .. B-1) share their conversions and products with the full step; left alone, the
        // compiler hoists all of them above the variant ladder (hundreds of live VGPRs).  Passing the raw words
        // through an empty asm makes them private to this variant.
        uint32_t rw[RW];
#pragma unroll
        for (int w = 0; w < RW; ++w) {
            rw[w] = raw[jj][w];
            asm volatile("" : "+v"(rw[w]));
        }
        float seg[NS];
        convert_segment<T, NS, RW, SH>(rw, seg);
        // tap-major over the K chains of the row: neighbouring instructions belong to different chains, so a
        // wave does not wait for its own previous add (each chain still sees its taps in lx order)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int k = 0; k < K; ++k) acc[jj][k] = acc[jj][k] + seg[SX * k + t] * cf[t];
    }
}

// remaining >= B: a full step; otherwise the tail of the kernel row with a compile-time tap count
template <typename T, int SX, int NT, int R, int K, int RW, int NC, int SH>
struct MacSelect {
    static __device__ __forceinline__ void run(int remaining, float (&acc)[R][K], const uint32_t (&raw)[R][RW],
                                               const float (&cf)[NC]) {
        if (remaining >= NT)
            mac_rows<T, SX, NT, R, K, RW, NC, SH>(acc, raw, cf);
        else
            MacSelect<T, SX, NT - 1, R, K, RW, NC, SH>::run(remaining, acc, raw, cf);
    }
};
template <typename T, int SX, int R, int K, int RW, int NC, int SH>
struct MacSelect<T, SX, 0, R, K, RW, NC, SH> {
    static __device__ __forceinline__ void run(int, float (&)[R][K], const uint32_t (&)[R][RW], const float (&)[NC]) {}
};

// Interior form (one step at a time): every variant fetches exactly the dwords ITS tap count needs -- the tail of a
// kernel row, or a kernel row shorter than a full step (fs 13 with 16-tap steps), would otherwise fetch a full
// step's segment: one buffer_load more per row than necessary.
template <typename T, int SX, int NT, int R, int K, int NC, int SH>
struct FetchMacSelect {
    static __device__ __forceinline__ void run(int remaining, float (&acc)[R][K], BufferRsrc rsrc, const uint32_t (&voff)[R],
                                               uint32_t srow, uint32_t srow_step, const float (&cf)[NC]) {
        if (remaining >= NT) {
            constexpr int RWN = segment_words<T>(NT + SX * (K - 1), SH);
            uint32_t raw[R][RWN];
#pragma unroll
            for (int jj = 0; jj < R; ++jj) load_raw<RWN>(rsrc, voff[jj], srow + static_cast<uint32_t>(jj) * srow_step, raw[jj]);
            mac_rows<T, SX, NT, R, K, RWN, NC, SH>(acc, raw, cf);
        } else {
            FetchMacSelect<T, SX, NT - 1, R, K, NC, SH>::run(remaining, acc, rsrc, voff, srow, srow_step, cf);
        }
    }
};
template <typename T, int SX, int R, int K, int NC, int SH>
struct FetchMacSelect<T, SX, 0, R, K, NC, SH> {
    static __device__ __forceinline__ void run(int, float (&)[R][K], BufferRsrc, const uint32_t (&)[R], uint32_t, uint32_t,
                                               const float (&)[NC]) {}
};

// Row walk (interior): chain row jj (period-row j + jj) meets source row r of the item at its kernel row
// ly = r - sy*jj.  Walking r upwards gives every chain its kernel rows in order, and inside a source row the steps run
// in lx order, so each chain still sees its taps in (ly, lx) raster order -- but a segment is fetched and converted
// once per source row instead of once per (chain row, kernel row): (sy*(R-1) + fs) / (R*fs) of the fetches (fs 13,
// step 2, R 4: 19 instead of 52), and the segment of the NEXT step is in flight while the current one is accumulated
// (two register sets, taken alternately).
//
// A kernel row is cut into nsx = ceil(fs / 16) steps of equal length nta = ceil(fs / nsx); the last step of a row has
// `last` = fs - (nsx-1)*nta taps, nta-2 <= last <= nta for nsx <= 3.  nta is a compile-time constant of the walk
// (9..16), the last step picks one of three tap counts.  Plans outside that (fs < 9, fs > 48) use shape 0.
// Smallest compile-time tap count of a step (and smallest filter size) of the row walk.  With 7 the walk also covers fs 7 / 8,
// but gains nothing there (4/3x, fs 7: 344 against 340 Gpix/s in the round-1 form, the quasi-periodic kernel 411; C2 423
// against 433): per source row too little work stands against the scalar bookkeeping.
constexpr int kWalkMinTaps = 7;          // of the walk's step ladders (the runs form takes fs 7 / 8 plans when forced: kernel mode 14)
constexpr int kWalkMinTapsPeriodic = 9;  // the interior of exactly periodic plans takes the walk from here on (see above)
struct WalkSteps {
    int nsx, nta, last;
};
__host__ __device__ inline WalkSteps walk_steps(int fs) {
    WalkSteps w;
    w.nsx = (fs + 15) / 16;
    w.nta = (fs + w.nsx - 1) / w.nsx;
    w.last = fs - (w.nsx - 1) * w.nta;
    return w;
}
__host__ __device__ inline bool walk_supported(int fs) {
    const WalkSteps w = walk_steps(fs);
    return fs >= kWalkMinTaps && w.nsx <= 3 && w.nta >= kWalkMinTaps && w.nta <= 16 && w.last >= w.nta - 2 && w.last >= 1;
}

// NT taps (lx0 .. lx0+NT-1) of source row r for the chain rows that meet it.  crow = the coefficient set's row r at
// lx0; chain row jj needs row r - sy*jj = crow - jj*jstride floats.  The rows of ALL R chain rows are loaded up front,
// also of those that do not meet r (kernel row outside 0..fs-1: up to kDirectCoeffSlackRows rows before or after the set
// -- the neighbouring sets, or the slack upload_table leaves around the coefficient array; never used), and pinned in
// front of the first branch, so the wave waits once per step for its scalar loads and no clamp sits in front of them.
template <typename T, int SX, int NT, int R, int K, int RWN, int SH>
__device__ __forceinline__ void walk_accumulate(float (&acc)[R][K], const uint32_t (&raw)[RWN], const JINC_CONSTANT float* crow,
                                                int jstride, int r, int sy, int fs, int rows) {
    static_assert((R - 1) * 4 <= kDirectCoeffSlackRows, "coefficient rows fetched outside a set");
    constexpr int NS = NT + SX * (K - 1);
    float cf[R][NT];
    bool on[R];
#pragma unroll
    for (int jj = 0; jj < R; ++jj) {
        const int ly = r - sy * jj;
        on[jj] = jj < rows && ly >= 0 && ly < fs;
        const JINC_CONSTANT float* c = crow - static_cast<ptrdiff_t>(jj) * jstride;
#pragma unroll
        for (int t = 0; t < NT; ++t) cf[jj][t] = c[t];
    }
    // pinned after ALL of them are issued: an empty asm counts as a use, i.e. it waits for the loads in front of it
#pragma unroll
    for (int jj = 0; jj < R; ++jj)
#pragma unroll
        for (int t = 0; t < NT; ++t) asm volatile("" : "+s"(cf[jj][t]));
    float seg[NS];  // the shorter tap counts of a row's last step convert a subset of the same samples: nothing to keep apart
    convert_segment<T, NS, RWN, SH>(raw, seg);
#pragma unroll
    for (int jj = 0; jj < R; ++jj) {
        if (on[jj]) {  // wave-uniform
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int k = 0; k < K; ++k) acc[jj][k] = acc[jj][k] + seg[SX * k + t] * cf[jj][t];
        }
    }
}

// Position of a step in the item: source row r, step i of the row.
struct WalkPos {
    int r = 0, i = 0;
    __device__ __forceinline__ void advance(int nsx) {
        if (++i == nsx) i = 0, ++r;
    }
};

template <typename T, int SX, int NTA, int R, int K, int SH>
struct WalkEqual {
    static constexpr int RWN = segment_words<T>(NTA + SX * (K - 1), SH);
    static constexpr uint32_t SB = static_cast<uint32_t>(sizeof(T));

    static __device__ __forceinline__ void fetch(uint32_t (&raw)[RWN], WalkPos& at, int nsx, BufferRsrc rsrc, uint32_t voff,
                                                 uint32_t soff0, uint32_t pitch) {
        // a step past the item's last one is fetched but not used; past the plane the range check answers 0
        load_raw<RWN, sizeof(T) != 2>(rsrc, voff, soff0 + static_cast<uint32_t>(at.r) * pitch + static_cast<uint32_t>(at.i * NTA) * SB, raw);
        at.advance(nsx);
    }
    static __device__ __forceinline__ void accumulate(float (&acc)[R][K], const uint32_t (&raw)[RWN], WalkPos& at, int nsx, int last,
                                                      const JINC_CONSTANT float* cs, int coeff_row, int sy, int fs, int rows) {
        const JINC_CONSTANT float* crow = cs + static_cast<ptrdiff_t>(at.r) * coeff_row + at.i * NTA;
        const int jstride = sy * coeff_row;
        if (at.i + 1 < nsx || last == NTA)
            walk_accumulate<T, SX, NTA, R, K, RWN, SH>(acc, raw, crow, jstride, at.r, sy, fs, rows);
        else if (last == NTA - 1)
            walk_accumulate<T, SX, NTA - 1, R, K, RWN, SH>(acc, raw, crow, jstride, at.r, sy, fs, rows);
        else
            walk_accumulate<T, SX, NTA - 2, R, K, RWN, SH>(acc, raw, crow, jstride, at.r, sy, fs, rows);
        at.advance(nsx);
    }
    static __device__ __forceinline__ void run(const WalkSteps w, float (&acc)[R][K], BufferRsrc rsrc, uint32_t voff, uint32_t soff0,
                                               uint32_t pitch, const JINC_CONSTANT float* cs, int coeff_row, int fs, int sy, int rows) {
        if (w.nta == NTA) {
            const int nsteps = (sy * (rows - 1) + fs) * w.nsx;
            uint32_t raw_a[RWN], raw_b[RWN];
            WalkPos f, c;  // next step to fetch / to accumulate
            fetch(raw_a, f, w.nsx, rsrc, voff, soff0, pitch);
#pragma unroll 1
            for (int s = 0; s < nsteps; s += 2) {
                fetch(raw_b, f, w.nsx, rsrc, voff, soff0, pitch);
                accumulate(acc, raw_a, c, w.nsx, w.last, cs, coeff_row, sy, fs, rows);
                fetch(raw_a, f, w.nsx, rsrc, voff, soff0, pitch);
                if (s + 1 < nsteps) accumulate(acc, raw_b, c, w.nsx, w.last, cs, coeff_row, sy, fs, rows);
            }
        } else if constexpr (NTA > kWalkMinTaps) {
            WalkEqual<T, SX, NTA - 1, R, K, SH>::run(w, acc, rsrc, voff, soff0, pitch, cs, coeff_row, fs, sy, rows);
        }
    }
};

// Kernel rows of a single step (fs <= 16) at source steps 2 and 3 -- the common down-scales -- get the leaner loop: the tap count
// is the only compile-time parameter, no step bookkeeping (measured against the general form above: 1/2 down-scale
// 8-bit +10 %, 16-bit +8 %, float +12 %, 2/3 +14 %).
template <typename T, int SX, int NT, int R, int K, int SH>
struct WalkFixed {
    static __device__ __forceinline__ void run(float (&acc)[R][K], BufferRsrc rsrc, uint32_t voff, uint32_t soff0, uint32_t pitch,
                                               const JINC_CONSTANT float* cs, int coeff_row, int fs, int sy, int rows) {
        if (fs == NT) {
            constexpr int RWN = segment_words<T>(NT + SX * (K - 1), SH);
            const int nr = sy * (rows - 1) + NT;
            uint32_t raw_a[RWN], raw_b[RWN];
            uint32_t srow = soff0;
            const int jstride = sy * coeff_row;
            const JINC_CONSTANT float* crow = cs;  // coefficient row r
            load_raw<RWN, sizeof(T) != 2>(rsrc, voff, srow, raw_a);
#pragma unroll 1
            for (int r = 0; r < nr; r += 2) {
                // a row past the item's last one is fetched but not used; past the plane the range check answers 0
                load_raw<RWN, sizeof(T) != 2>(rsrc, voff, srow + pitch, raw_b);
                walk_accumulate<T, SX, NT, R, K, RWN, SH>(acc, raw_a, crow, jstride, r, sy, NT, rows);
                srow += 2 * pitch;
                load_raw<RWN, sizeof(T) != 2>(rsrc, voff, srow, raw_a);
                if (r + 1 < nr) walk_accumulate<T, SX, NT, R, K, RWN, SH>(acc, raw_b, crow + coeff_row, jstride, r + 1, sy, NT, rows);
                crow += 2 * coeff_row;
            }
        } else if constexpr (NT > kWalkMinTaps) {
            WalkFixed<T, SX, NT - 1, R, K, SH>::run(acc, rsrc, voff, soff0, pitch, cs, coeff_row, fs, sy, rows);
        }
    }
};

// Which walk a launch may use (host and device agree through these):
//   single-step rows at source steps >= 2: WalkFixed, 4 or 8 columns per lane;
//   everything else walk_supported() covers: WalkEqual, 4 columns per lane only.
// (source step 4 has single-step rows at tap 1 only -- fs 10 -- and stays with the general form)
__host__ __device__ inline bool walk_fixed_applies(int fs, int sx) { return (sx == 2 || sx == 3) && fs >= kWalkMinTaps && fs <= 16; }
__host__ __device__ inline bool walk_wide_supported(int fs, int sx) { return walk_fixed_applies(fs, sx); }

template <typename T, int SX, int SHAPE, int SH, int R, int K>
__device__ __forceinline__ void direct_row_walk(float (&acc)[R][K], BufferRsrc srsrc, uint32_t voff, uint32_t soff0, uint32_t pitch,
                                                const JINC_CONSTANT float* cs, int coeff_row, int fs, int sy, int rows) {
    if constexpr (SX == 2 || SX == 3) {
        if (fs <= 16) {
            WalkFixed<T, SX, 16, R, K, SH>::run(acc, srsrc, voff, soff0, pitch, cs, coeff_row, fs, sy, rows);
            return;
        }
    }
    if constexpr (K == 4) WalkEqual<T, SX, 16, R, K, SH>::run(walk_steps(fs), acc, srsrc, voff, soff0, pitch, cs, coeff_row, fs, sy, rows);
}

// The whole tap loop of an item for one value of SH: steps in (ly, lx) raster order, step s covers kernel row
// s / nsx, taps (s % nsx) * B ...
template <typename T, int SX, int MODE, int SHAPE, int SH, int R, int K>
__device__ __forceinline__ void direct_steps(float (&acc)[R][K], BufferRsrc srsrc, const uint32_t (&voff)[R], uint32_t soff0,
                                             uint32_t srow_step, uint32_t pitch, const JINC_CONSTANT float* cs, int coeff_row,
                                             int fs) {
    using Shape = DirectShape<T, MODE, SHAPE>;
    static_assert(R == Shape::R && K == Shape::K, "chain shape of the mode");
    constexpr int B = Shape::B, D = Shape::D;
    constexpr int RW = segment_words<T>(B + SX * (K - 1), SH);  // dwords of a full step's segment
    constexpr uint32_t SB = static_cast<uint32_t>(sizeof(T));
    const int nsx = (fs + B - 1) / B;
    const int nsteps = fs * nsx;
    int ly = 0, lxi = 0;  // coordinates of the next step to fetch
#pragma unroll 1
    for (int s0 = 0; s0 < nsteps; s0 += D) {
        if constexpr (D == 1) {
            const int lx = lxi * B;
            const uint32_t srow = soff0 + static_cast<uint32_t>(ly) * pitch + static_cast<uint32_t>(lx) * SB;
            const JINC_CONSTANT float* c = cs + static_cast<size_t>(ly) * coeff_row + lx;
            float cf1[B];
#pragma unroll
            for (int t = 0; t < B; ++t) cf1[t] = c[t];  // wave-uniform -> SGPRs (the allocation has slack past the last row)
            FetchMacSelect<T, SX, B, R, K, B, SH>::run(fs - lx, acc, srsrc, voff, srow, srow_step, cf1);
            if (++lxi == nsx) lxi = 0, ++ly;
        } else {
            uint32_t raw[D][R][RW];
            float cf[D][B];
            int rem[D];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                if (s0 + d < nsteps) {  // wave-uniform
                    const int lx = lxi * B;
                    const uint32_t srow = soff0 + static_cast<uint32_t>(ly) * pitch + static_cast<uint32_t>(lx) * SB;
#pragma unroll
                    for (int jj = 0; jj < R; ++jj) load_raw<RW>(srsrc, voff[jj], srow + static_cast<uint32_t>(jj) * srow_step, raw[d][jj]);
                    const JINC_CONSTANT float* c = cs + static_cast<size_t>(ly) * coeff_row + lx;
#pragma unroll
                    for (int t = 0; t < B; ++t) cf[d][t] = c[t];  // wave-uniform -> SGPRs
                    rem[d] = fs - lx;
                    if (++lxi == nsx) lxi = 0, ++ly;
                }
            }
#pragma unroll
            for (int d = 0; d < D; ++d)
                if (s0 + d < nsteps) MacSelect<T, SX, B, R, K, RW, B, SH>::run(rem[d], acc, raw[d], cf[d]);
        }
    }
}

template <typename T, int SX, int MODE, int SHAPE, int SH, int R, int K>
__device__ __forceinline__ void direct_taps(float (&acc)[R][K], BufferRsrc srsrc, const uint32_t (&voff)[R], uint32_t soff0,
                                            uint32_t srow_step, uint32_t pitch, const JINC_CONSTANT float* cs, int coeff_row, int fs,
                                            int sy, int rows) {
    if constexpr (DirectShape<T, MODE, SHAPE>::kWalk)
        direct_row_walk<T, SX, SHAPE, SH>(acc, srsrc, voff[0], soff0, pitch, cs, coeff_row, fs, sy, rows);
    else
        direct_steps<T, SX, MODE, SHAPE, SH>(acc, srsrc, voff, soff0, srow_step, pitch, cs, coeff_row, fs);
}

__device__ __forceinline__ int plan_int(const int32_t* base, size_t index) {  // wave-uniform table lookup -> s_load
    return ((const JINC_CONSTANT int32_t*)base)[index];
}

// One wave = one item.
//   interior : phase (p, q) x 256 period-columns (4 per lane) x 4 period-rows (shape 0), or 64 (column group, row chunk)
//              pairs of a phase in raster order (row-walk shapes: packed lanes);
//   row strip: output row y x column phase p x 256 period-columns (4 per lane, 1 row);
// The four waves of a workgroup take consecutive items (phases of one row chunk / strip line first), so they share
// source rows in the L1.  A kernel row is walked in steps of B taps plus one shorter tail step.
template <typename T, int SX, int MODE, int SHAPE>
__global__ __launch_bounds__(256, (direct_min_waves<T, SX, MODE, SHAPE>())) void ewa_direct_kernel(const DirectArgs a, const PlaneIO io) {
    using Shape = DirectShape<T, MODE, SHAPE>;
    constexpr int K = Shape::K, R = Shape::R;
    constexpr uint32_t SB = static_cast<uint32_t>(sizeof(T));
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int tile_a, tile_b;
    swizzled_tile(tile_a, tile_b);  // tile_a: along the lane axis; tile_b: groups of 4 items
    const int item = ((MODE != kDirectRowStrip && Shape::kWalk) ? tile_a : tile_b) * 4 + wave;  // walk: 1-D grid of blocks
    const size_t frame = blockIdx.z;
    const uint32_t pitch = static_cast<uint32_t>(io.src_pitch);
    const int fs = a.fs;

    // ---- which chains does this lane own? ----
    int set;                 // wave-uniform coefficient set
    uint32_t voff[R];        // per-lane byte offset of the segments of its R rows (without ly / lx)
    uint32_t soff0;          // wave-uniform byte offset of kernel row 0, tap 0
    uint32_t srow_step;      // wave-uniform byte distance between the lane's R rows (interior only)
    bool row_ok[R];          // chain rows that exist
    int cols_valid = K;      // chain columns that exist
    int rows = R;            // chain rows the walk computes (wave-uniform).  The packed-lane forms leave it at R: their lanes may sit in
                             // different row chunks, row_ok[] is per lane there, and rows that do not exist are computed from fetches the
                             // range check answers and never stored.  A run-time count (largest over the wave's lanes) measured SLOWER: the
                             // compile-time R folds the `jj < rows` tests away (1.5x tap 8 at 128 frames 88.9 -> 78.3 Gpix/s, 4K -> 1080p
                             // 177.6 -> 175.6; profiles/experiments/direct_walk_wave_rows.diff, round3/direct_wave_rows_ab.txt)
    uint32_t dst_voff[R];    // per-lane byte offset of the first output sample of each row
    uint32_t dst_soff[R];    // wave-uniform part
    uint32_t dst_xstep = 0;  // bytes between the K output columns
    bool lane_ok;            // the lane owns at least one chain (checked after the wave-uniform set-up below: a
                             // divergent exit in front of it would push every uniform value into VGPRs)
    if constexpr (MODE == kDirectRuns) {
        // Runs form: the item belongs to one rectangle of a drifting plan (DirectRun, kernels.h) -- one coefficient set, windows
        // affine in the period index: the interior's packed-lane walk with the rectangle's numbers in place of the plane's.
        static_assert(Shape::kWalk, "the runs form is a row walk");
        if (item >= a.n_items) return;  // wave-uniform
        const int run_index = plan_int(a.item_run, static_cast<size_t>(item));
        const JINC_CONSTANT DirectRun& run = ((const JINC_CONSTANT DirectRun*)a.runs)[run_index];
        const int run_ni = run.ni, run_nj = run.nj;
        const uint32_t groups = static_cast<uint32_t>(run_ni + K - 1) / K;
        const uint32_t chunks = static_cast<uint32_t>(run_nj + R - 1) / R;
        const uint32_t mine = static_cast<uint32_t>(item - run.first_wave) * 64u + static_cast<uint32_t>(lane);
        lane_ok = mine < groups * chunks;
        const uint32_t ch = lane_ok ? mine / groups : 0u;
        const int i_lane = static_cast<int>(lane_ok ? mine - ch * groups : 0u) * K;
        const int j = static_cast<int>(ch) * R;
        cols_valid = run_ni - i_lane;
        set = run.set;
        soff0 = 0;
        srow_step = 0;
#pragma unroll
        for (int jj = 0; jj < R; ++jj) {
            voff[jj] = static_cast<uint32_t>(run.sx0 + SX * i_lane) * SB + static_cast<uint32_t>(run.sy0 + a.sy * j) * pitch;
            row_ok[jj] = j + jj < run_nj;  // per lane
            dst_voff[jj] = static_cast<uint32_t>(run.x0 + a.px * i_lane) * SB +
                           static_cast<uint32_t>(run.y0 + a.py * (j + jj)) * static_cast<uint32_t>(io.dst_pitch);
            dst_soff[jj] = 0;
        }
        dst_xstep = static_cast<uint32_t>(a.px) * SB;
    } else if constexpr (MODE == kDirectInterior && Shape::kWalk) {
        // Packed lanes: the (column group, row chunk) pairs of one phase are numbered row chunk by row chunk and dealt to
        // lanes 64 at a time, so only the last wave of a phase has idle lanes whatever the plane's width (a wave may
        // straddle two row chunks: the walk is the same for every lane, only the addresses differ).  tile_a = 0.
        const int nphase = a.px * a.py;
        const int range = item / nphase;
        const int ph = item - range * nphase;
        const int q = ph / a.px;
        const int p = ph - q * a.px;
        const uint32_t groups = static_cast<uint32_t>(a.ni + K - 1) / K;
        const uint32_t chunks = static_cast<uint32_t>(a.nj + R - 1) / R;
        const uint32_t first = static_cast<uint32_t>(range) * 64u;
        if (first >= groups * chunks) return;  // wave-uniform
        const uint32_t mine = first + static_cast<uint32_t>(lane);
        lane_ok = mine < groups * chunks;
        const uint32_t ch = lane_ok ? mine / groups : 0u;
        const int i_lane = static_cast<int>(lane_ok ? mine - ch * groups : 0u) * K;
        const int j = static_cast<int>(ch) * R;
        cols_valid = a.ni - i_lane;
        set = a.set[ph];
        soff0 = 0;
        srow_step = 0;
#pragma unroll
        for (int jj = 0; jj < R; ++jj) {
            voff[jj] = static_cast<uint32_t>(a.start_x[p] + SX * i_lane) * SB + static_cast<uint32_t>(a.start_y[q] + a.sy * j) * pitch;
            row_ok[jj] = j + jj < a.nj;  // per lane
            dst_voff[jj] = static_cast<uint32_t>(a.ix0 + a.px * i_lane + p) * SB +
                           static_cast<uint32_t>(a.iy0 + a.py * (j + jj) + q) * static_cast<uint32_t>(io.dst_pitch);
            dst_soff[jj] = 0;
        }
        dst_xstep = static_cast<uint32_t>(a.px) * SB;
    } else if constexpr (MODE == kDirectInterior) {
        const int nphase = a.px * a.py;
        const int ch = item / nphase;
        const int ph = item - ch * nphase;
        const int q = ph / a.px;
        const int p = ph - q * a.px;
        const int j = ch * R;  // first period-row of the chunk
        if (j >= a.nj) return;  // wave-uniform
        rows = a.nj - j < R ? a.nj - j : R;
        const int i_lane = tile_a * (64 * K) + K * lane;
        cols_valid = a.ni - i_lane;
        lane_ok = cols_valid > 0;
        set = a.set[ph];
        soff0 = static_cast<uint32_t>(a.start_y[q] + a.sy * j) * pitch;
        srow_step = static_cast<uint32_t>(a.sy) * pitch;
#pragma unroll
        for (int jj = 0; jj < R; ++jj) {
            voff[jj] = static_cast<uint32_t>(a.start_x[p] + SX * i_lane) * SB;
            row_ok[jj] = j + jj < a.nj;
            dst_voff[jj] = static_cast<uint32_t>(a.ix0 + a.px * i_lane + p) * SB;
            dst_soff[jj] = static_cast<uint32_t>(a.iy0 + a.py * (j + jj) + q) * static_cast<uint32_t>(io.dst_pitch);
        }
        dst_xstep = static_cast<uint32_t>(a.px) * SB;
    } else if constexpr (MODE == kDirectRowStrip) {
        const int line = item / a.px;
        const int p = item - line * a.px;
        if (line >= a.line_n[0] + a.line_n[1]) return;
        const int y = line < a.line_n[0] ? a.line0[0] + line : a.line0[1] + (line - a.line_n[0]);
        const int i_lane = tile_a * (64 * K) + K * lane;
        cols_valid = a.ni - i_lane;
        lane_ok = cols_valid > 0;
        const int xr = a.ix0 + p;  // representative column of the phase
        const int rc = plan_int(a.plan.row_class, y);
        set = rc < 0 ? plan_int(a.plan.brow_set, static_cast<size_t>(~rc) * a.plan.dst_w + xr)
                     : plan_int(a.plan.interior_set, static_cast<size_t>(rc) * a.plan.n_col_classes + plan_int(a.plan.col_class, xr));
        soff0 = static_cast<uint32_t>(plan_int(a.plan.row_start, y)) * pitch;
        srow_step = 0;
        voff[0] = static_cast<uint32_t>(a.start_x[p] + SX * i_lane) * SB;
        row_ok[0] = true;
        dst_voff[0] = static_cast<uint32_t>(a.ix0 + a.px * i_lane + p) * SB;
        dst_soff[0] = static_cast<uint32_t>(y) * static_cast<uint32_t>(io.dst_pitch);
        dst_xstep = static_cast<uint32_t>(a.px) * SB;
    }

    // Split every segment address into an aligned part and the byte shift SH of its first sample.  The host guarantees
    // that the pitch and the frame stride are multiples of 4; the plane's own misalignment (base & 3) joins the lane
    // offset.  The lane stride (SX * 4 samples) is a multiple of 4 bytes, so SH is the same for all lanes: one
    // wave-uniform switch selects the instantiation of the tap loop that has SH as a compile-time constant.
    const uintptr_t plane = reinterpret_cast<uintptr_t>(io.src) + frame * io.src_frame_stride;
    const uint32_t mis = static_cast<uint32_t>(plane & 3u) + (soff0 & 3u);
    soff0 &= ~3u;
    const uint32_t sh = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>((voff[0] + mis) & 3u)));
#pragma unroll
    for (int jj = 0; jj < R; ++jj) voff[jj] = (voff[jj] + mis) & ~3u;
    const BufferRsrc srsrc = make_rsrc(reinterpret_cast<char*>(plane & ~static_cast<uintptr_t>(3)), a.src_bytes);
    if (!lane_ok) return;
    const JINC_CONSTANT float* cs =
        (const JINC_CONSTANT float*)(a.coeffs + static_cast<size_t>(set) * (static_cast<size_t>(fs) * a.coeff_row));

    float acc[R][K];
#pragma unroll
    for (int jj = 0; jj < R; ++jj)
#pragma unroll
        for (int k = 0; k < K; ++k) acc[jj][k] = 0.f;

    if constexpr (sizeof(T) == 4) {
        direct_taps<T, SX, MODE, SHAPE, 0>(acc, srsrc, voff, soff0, srow_step, pitch, cs, a.coeff_row, fs, a.sy, rows);
    } else if constexpr (sizeof(T) == 2) {
        if (sh == 0)
            direct_taps<T, SX, MODE, SHAPE, 0>(acc, srsrc, voff, soff0, srow_step, pitch, cs, a.coeff_row, fs, a.sy, rows);
        else
            direct_taps<T, SX, MODE, SHAPE, 2>(acc, srsrc, voff, soff0, srow_step, pitch, cs, a.coeff_row, fs, a.sy, rows);
    } else {
        switch (sh) {
            case 0: direct_taps<T, SX, MODE, SHAPE, 0>(acc, srsrc, voff, soff0, srow_step, pitch, cs, a.coeff_row, fs, a.sy, rows); break;
            case 1: direct_taps<T, SX, MODE, SHAPE, 1>(acc, srsrc, voff, soff0, srow_step, pitch, cs, a.coeff_row, fs, a.sy, rows); break;
            case 2: direct_taps<T, SX, MODE, SHAPE, 2>(acc, srsrc, voff, soff0, srow_step, pitch, cs, a.coeff_row, fs, a.sy, rows); break;
            default: direct_taps<T, SX, MODE, SHAPE, 3>(acc, srsrc, voff, soff0, srow_step, pitch, cs, a.coeff_row, fs, a.sy, rows); break;
        }
    }

    const BufferRsrc drsrc = make_rsrc(static_cast<char*>(io.dst) + frame * io.dst_frame_stride,
                                       static_cast<uint32_t>(io.dst_pitch) * a.dst_h);
#pragma unroll
    for (int jj = 0; jj < R; ++jj) {
        if (row_ok[jj]) {  // (per lane in the packed-lane forms, wave-uniform otherwise)
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (k < cols_valid) store_sample_buf<T>(drsrc, dst_voff[jj] + k * dst_xstep, dst_soff[jj], acc[jj][k], io.peak);
        }
    }
}

template <typename T, int SX, int MODE, int SHAPE>
int launch_direct_shape(const DirectArgs& da, const PlaneIO& io, hipStream_t stream) {
    constexpr int K = DirectShape<T, MODE, SHAPE>::K, R = DirectShape<T, MODE, SHAPE>::R;
    int tiles = (da.ni + 64 * K - 1) / (64 * K);
    long long items = MODE == kDirectInterior ? static_cast<long long>((da.nj + R - 1) / R) * da.px * da.py
                                              : static_cast<long long>(da.line_n[0] + da.line_n[1]) * da.px;
    if constexpr (MODE == kDirectRuns) {
        tiles = 1;
        items = da.n_items;
    } else if constexpr (DirectShape<T, MODE, SHAPE>::kWalk) {  // packed lanes (see the kernel)
        const long long lanes = static_cast<long long>((da.ni + K - 1) / K) * ((da.nj + R - 1) / R);
        tiles = 1;
        items = (lanes + 63) / 64 * da.px * da.py;
    }
    if (tiles <= 0 || items <= 0) return 0;
    if ((items + 3) / 4 > 0x7fffffffLL) return static_cast<int>(hipErrorInvalidValue);
    // the linear block id is formed from (x, y) by swizzled_tile: blocks along y only would exceed the 65535 limit
    const long long blocks = (items + 3) / 4;
    dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(blocks), io.nframes);
    if constexpr (DirectShape<T, MODE, SHAPE>::kWalk) grid = dim3(static_cast<unsigned>(blocks), 1, io.nframes);
    hipLaunchKernelGGL((ewa_direct_kernel<T, SX, MODE, SHAPE>), grid, dim3(256, 1, 1), 0, stream, da, io);
    return static_cast<int>(hipGetLastError());
}

}  // namespace
}  // namespace jinc
