// kernels.h -- launch interface between the host filter (filter.cpp) and the gfx950 kernels
// (kernels.hip).  Plain structs of device pointers and sizes; no HIP types except the stream.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace jinc {

// Device-resident compact plan of one table (see plan.h for the meaning of each array).
struct DevicePlan {
    const int32_t* col_start = nullptr;
    const int32_t* row_start = nullptr;
    const int32_t* col_class = nullptr;
    const int32_t* row_class = nullptr;
    const int32_t* interior_set = nullptr;
    const int32_t* bcol_set = nullptr;
    const int32_t* brow_set = nullptr;
    const float* coeffs = nullptr;
    int src_w = 0, src_h = 0, dst_w = 0, dst_h = 0;
    int fs = 0;
    int n_col_classes = 0;
    // Dominant phase period of the output columns / rows (1..8): the lane stride of the gather kernel.
    int gather_period_x = 1, gather_period_y = 1;
};

constexpr int kSampleHalf = 1;
constexpr int kSampleBFloat16 = 2;

// One plane of a batch of frames, device pointers, pitches/strides in bytes.
struct PlaneIO {
    const void* src = nullptr;
    void* dst = nullptr;
    int src_pitch = 0, dst_pitch = 0;
    size_t src_frame_stride = 0, dst_frame_stride = 0;
    int nframes = 1;
    int sample_bytes = 1;  // 1: uint8, 2: uint16, binary16 or bfloat16 (sample_kind), 4: float
    int sample_kind = 0;   // kSampleHalf: IEEE binary16, kSampleBFloat16: bfloat16 samples (sample_bytes 2); else integer (1, 2 bytes) or fp32 (4 bytes)
    float peak = 255.f;    // clamp ceiling of integer planes (ref JincResize.cpp:582, :793)
};

// Up to four output rectangles handled by one gather launch (whole plane, or the border frame
// around the periodic interior).
struct RectList {
    int n = 0;
    int x0[4] = {0, 0, 0, 0}, y0[4] = {0, 0, 0, 0}, w[4] = {0, 0, 0, 0}, h[4] = {0, 0, 0, 0};
    // true for the border frame of a plan that is not exactly periodic: there nearly every pixel owns a
    // private coefficient set, so the kernel skips the uniform passes and loads coefficients per lane
    bool private_sets = false;
    // lane stride 1 instead of the plan's dominant period: for rectangles in which even pixels of one phase never
    // share a set (corners, border frame of drifting plans) the period stride only thins out the lanes
    bool unit_stride = false;
    // Optional lane-major copy of the coefficients of these rectangles' pixels (private_sets only): item i of
    // rectangle r (numbering: gather_item_index) owns fs * padded_row(fs) * 64 floats laid out
    // [kernel row][group of 4 taps][lane][4], so the 64 lanes of an item fetch their private coefficients with
    // contiguous 16-byte loads (1 KiB per wave and fetch) instead of touching 64 cache lines.
    const float* lane_coeffs = nullptr;
    long long lane_item_base[4] = {0, 0, 0, 0};
};

// How the gather kernel walks a rectangle: lane axis (0: lanes along x, 1: along y) and lane stride P; shared by
// launch_gather and by the host code that builds RectList::lane_coeffs.
inline void gather_rect_layout(const DevicePlan& plan, int w, int h, bool unit_stride, int& axis, int& P) {
    // Narrow rectangles (border columns, up to ~fs wide) put the lanes along y: a wave is then not mostly
    // idle, and its lanes share the border column's coefficient sets (along x every lane would own one).
    axis = (w < 64 && h > w) ? 1 : 0;
    // The lane stride exists to give the lanes of an item one coefficient set; where every pixel owns its set it only
    // thins out the lanes of narrow rectangles (a 33-pixel corner: 17 of 64 lanes at stride 2).
    P = unit_stride ? 1 : (axis == 0 ? plan.gather_period_x : plan.gather_period_y);
}
// Items of a rectangle are numbered (line * P + residue) * blocks_along + block, with line = row (axis 0) or column
// (axis 1) inside the rectangle and blocks_along = ceil(extent along the lane axis / (64 * P)).
inline long long gather_item_count(int w, int h, int axis, int P) {
    const int along = axis == 0 ? w : h, across = axis == 0 ? h : w;
    return static_cast<long long>(across) * P * ((along + 64 * P - 1) / (64 * P));
}

// Phase-periodic interior (see plan.h): output pixel (ix0 + px*i + p, iy0 + py*j + q) reads the
// source window at (start_x[p] + i, start_y[q] + j) with coefficient set set[q*px + p].
constexpr uint32_t span7_form(int ly, int q, uint32_t form) { return form << (2 * (2 * ly + q)); }  // (PeriodicArgs::kQuadSpan7Mpeg2)

// Symmetry classes of the 2x up-scale with tap 3 on the trimmed 6 x 6 support (ewa_periodic_quad2_kernel<integer, RG,
// kQuadInnerTap3, 6> on frame pairs; host check: device_plan.cpp quad2_share_classes).  Phase 0 of an axis sits 2.25 taps
// behind the window origin, phase 1 2.75, so tap t of phase ph is (2 m + 1) / 4 source steps from the output's centre with
// m = quad2_share_m(ph, t) in 0 .. 5.  An EWA weight depends on the distance alone: a tap's coefficient is a function of the
// unordered pair (m_x, m_y).  The 21 pairs are 18 inside the disc of radius 3.24 and 3 outside ((2 a + 1)^2 + (2 b + 1)^2 > 162:
// (3, 5), (4, 5), (5, 5)), whose coefficients are 0.  quad2_share_class numbers the 18 in (min, max) order, -1 for the others.
constexpr int kQuad2ShareClasses = 18;
constexpr int quad2_share_m(int ph, int t) {
    const int d = 4 * t - 9 - 2 * ph;
    return ((d < 0 ? -d : d) - 1) / 2;
}
constexpr bool quad2_share_inside(int a, int b) { return (2 * a + 1) * (2 * a + 1) + (2 * b + 1) * (2 * b + 1) <= 162; }
constexpr int quad2_share_class(int mx, int my) {
    const int a = mx < my ? mx : my, b = mx < my ? my : mx;
    if (!quad2_share_inside(a, b)) return -1;
    int k = 0;
    for (int lo = 0; lo < 6; ++lo)
        for (int hi = lo; hi < 6; ++hi) {
            if (!quad2_share_inside(lo, hi)) continue;
            if (lo == a && hi == b) return k;
            ++k;
        }
    return -1;
}
static_assert(quad2_share_class(4, 4) == kQuad2ShareClasses - 1 && quad2_share_class(5, 2) == 14 && quad2_share_class(3, 5) < 0 &&
                  quad2_share_m(0, 2) == 0 && quad2_share_m(1, 3) == 0 && quad2_share_m(0, 5) == 5 && quad2_share_m(1, 0) == 5,
              "class numbering");
// The frame-pair form walks strips 2 periods across and H period rows down (kernel_periodic_quad2.inc quad2_share_body).  A set of the strip's
// outputs: bit 4 * oy + ox, oy = 2 * period row + q, ox = 2 * period column + p.
struct Quad2ShareOuts {
    static constexpr int kMaxStripRows = 16;
    uint64_t w[kMaxStripRows / 8] = {};
    constexpr bool any() const {
        for (uint64_t v : w)
            if (v != 0) return true;
        return false;
    }
    constexpr bool has(int o) const { return ((w[o >> 6] >> (o & 63)) & 1u) != 0; }
    constexpr void set(int o) { w[o >> 6] |= uint64_t{1} << (o & 63); }
};
// The strip's outputs that take sample (r, c) of its 7-column x (H + 5)-row window with a coefficient of class k.
template <int H>
constexpr Quad2ShareOuts quad2_share_outs(int r, int c, int k) {
    static_assert(H <= Quad2ShareOuts::kMaxStripRows, "a strip's outputs index the words of one Quad2ShareOuts");
    Quad2ShareOuts m;
    for (int oy = 0; oy < 2 * H; ++oy)
        for (int ox = 0; ox < 4; ++ox) {
            const int ly = r - (oy >> 1), lx = c - (ox >> 1);
            if (ly < 0 || ly > 5 || lx < 0 || lx > 5) continue;
            if (quad2_share_class(quad2_share_m(ox & 1, lx), quad2_share_m(oy & 1, ly)) == k) m.set(4 * oy + ox);
        }
    return m;
}
// Products per strip and frame pair: the (sample, class) pairs some output of the strip takes, one v_pk_mul_f32 each.
template <int H>
constexpr int quad2_share_products() {
    int n = 0;
    for (int r = 0; r < H + 5; ++r)
        for (int c = 0; c < 7; ++c)
            for (int k = 0; k < kQuad2ShareClasses; ++k) n += quad2_share_outs<H>(r, c, k).any() ? 1 : 0;
    return n;
}
struct PeriodicArgs {
    const float* coeffs = nullptr;
    int px = 1, py = 1;
    int ix0 = 0, iy0 = 0;
    int ni = 0, nj = 0;          // number of whole periods covered in x / y
    int start_x[8] = {0}, start_y[8] = {0};
    int min_sx = 0, min_sy = 0;  // min over phases of start_x / start_y
    int set[64] = {0};
    int src_w = 0, src_h = 0;
    int dst_h = 0;  // rows of the destination plane (bounds of the store descriptor)
    // 2x up-scales whose phases share their window origin (ewa_periodic_quad_kernel): coefficient pairs
    // quad[ly][q][8 pairs][p] = (set(p=0,q), set(p=1,q))[ly][lx], or nullptr when the plan has no such form
    const float* quad = nullptr;
    // ewa_periodic_quad2_kernel: bit 2 * ly + q set = taps 0 and 5 of kernel row ly carry zero coefficients for both phases p of q
    uint32_t quad_inner = 0;
    int quad_taps = 0;  // ewa_periodic_quad2_kernel: taps per kernel row when they differ from the row count (7: the 6 x 7 support), else 0
    // the 6 x 7 support: zero coefficients in front of / behind the span of kernel row ly at row phase q for BOTH phases p, two bits each
    // (capped at 3) at 4 * (2 * ly + q) and 4 * (2 * ly + q) + 2
    uint64_t quad_span7 = 0;
    // ... and the span FORM of every (ly, q) the kernel is instantiated for (kernel_periodic_quad2.inc quad2_row7_span: 0 = all seven taps, 1 =
    // taps 1 .. 6, 2 = taps 1 .. 5, 3 = taps 2 .. 5), two bits at 2 * (2 * ly + q): chroma planes sited as MPEG-2 at 2x with tap 3 --
    // q = 0: forms 3 1 0 0 0 2 for ly = 0 .. 5, q = 1: 2 0 0 0 1 3.  36 of 42 taps.
    static constexpr uint32_t kQuadSpan7Mpeg2 = span7_form(0, 0, 3) | span7_form(1, 0, 1) | span7_form(5, 0, 2) | span7_form(0, 1, 2) |
                                                span7_form(4, 1, 1) | span7_form(5, 1, 3);
    // (the spans of the 8-row x 9-column support -- chroma at tap 4 -- use the same field: 16 (ly, q) entries of four bits)
    // (which output row is q = 0 follows from the parity of the interior's first row: the same pattern with the row phases exchanged)
    static constexpr uint32_t kQuadSpan7Mpeg2Swapped = span7_form(0, 1, 3) | span7_form(1, 1, 1) | span7_form(5, 1, 2) | span7_form(0, 0, 2) |
                                                       span7_form(4, 0, 1) | span7_form(5, 0, 3);
    static constexpr uint32_t kQuadInnerTap3 = (1u << (2 * 5 + 0)) | (1u << (2 * 0 + 1));  // the mask the kernel is instantiated for
    // integer planes on the 6 x 6 support whose four phase sets follow the symmetry classes above bit for bit (quad_share = 1):
    // share_w[class] is every tap of that class, the taps outside the disc are 0.0f.  The kInnerTap3 instance then computes frame
    // pairs, one product per (source sample, class) for all of the lane's outputs that need it (quad2_share_runs).
    int quad_share = 0;
    alignas(8) float share_w[kQuad2ShareClasses] = {};
    // quad forms on the 8 x 8 support: taps kernel row ly of q leaves out per side (0 .. 3), two bits at 2 * (2 * ly + q)
    uint32_t quad_trim8 = 0;
    static const uint32_t kQuad8TrimTap4;  // the pattern the kernels are instantiated for (below)
    // trimmed support only (ewa_periodic_rows_kernel): row_trim[phase * 32 + ly] = taps kernel row ly of the phase leaves out on
    // EITHER side (min of its leading and trailing zero coefficients, at most 5), or nullptr
    const int32_t* row_trim = nullptr;
    int rows_ny = 0;  // ewa_periodic_rows_kernel on a support with fewer kernel rows than taps per row: the row count (0: fs rows)
    // ewa_periodic_rowpair_kernel (2x up-scales with 12 .. 17 taps per kernel row whose two phases p share their window origin):
    // coefficient pairs rowpair[(q * rowpair_ny + ly) * rowpair_stride + 2 * lx + p] = set(p, q)[ly][lx], and per q the taps each
    // kernel row leaves out on either side for BOTH p, three bits per kernel row (bits 3 * ly ...), and in bits 54 .. 58 / 59 .. 63 the
    // first kernel row executed / the one behind the last (0: all rowpair_ny) -- the rows outside are zero for both p; nullptr: no such form
    // Border rows as launches of the same kernel (device_plan.cpp plan_rowpair_rows): the border rows of one end of the plane are the
    // py <= kRowPairMaxPhases "row phases" of a launch with nj = 1, every one with its own coefficient pairs and all with the window
    // origin start_y[0] (py > 8: start_y[q] is not read).  rowpair_strip_phases > 0 marks such a launch: its grid's y counts groups of
    // that many phases (a workgroup = one group x one tile column: 17 rows in one workgroup were three rounds of its eight waves on
    // a chip the launch does not fill -- C3: 46 us per launch), not tile rows.
    static constexpr int kRowPairMaxPhases = 24;
    int rowpair_strip_phases = 0;
    const float* rowpair = nullptr;
    int rowpair_n = 0, rowpair_ny = 0, rowpair_stride = 0;
    uint64_t rowpair_trim[kRowPairMaxPhases] = {};
    // float planes on the trimmed support: frame_flags[frame] (kernel_scan.hip: 1 = the frame's plane holds a non-finite
    // sample) decides which of two launches computes a frame -- a launch returns at once for frames whose flag differs from
    // run_when.  nullptr: every frame.
    const uint32_t* frame_flags = nullptr;
    uint32_t run_when = 0;
    // run_when == kRunAllAndFlag: the launch computes EVERY frame and sets frame_flags[frame] = 1 where it stages a non-finite
    // sample (the trimmed launch of a float plane is its own finite-sample scan; kernel_periodic_common.inc NonFinite)
    static constexpr uint32_t kRunAllAndFlag = 2;
    // ewa_periodic_quad2_kernel / ewa_periodic_quad2x8_kernel on integer planes: the plane's border COLUMNS beside the interior rows, computed by the first / last
    // tile column out of the tile it has staged anyway (device_plan.cpp plan_edge_columns; as kernels of their own the columns were
    // bound by the scattered 64-byte lines of their source windows and stores, not by arithmetic).  Side s (0 left, 1 right): n[s]
    // output columns from x0[s] on, all with the source window whose first column is LDS column lds_col[s] (-1: the column in front
    // of the tile, staged into the pitch's spare word) of tile column tile_x[s]; coefficient rows
    // coeffs[((s * kMaxPerSide + k) * 2 + q) * (NR * NCP) + ly * NCP + lx] = kernel rows r0 .. r0 + NR - 1 (the interior's trimmed rows: 6,
    // or 8 for ewa_periodic_quad2x8_kernel) of column k's set at row phase q, NCP = the filter size rounded up to a multiple of 4.
    // coeffs == nullptr: the border kernels compute the columns.
    struct EdgeColumns {
        static constexpr int kMaxPerSide = 16;
        const float* coeffs = nullptr;
        int n[2] = {0, 0}, x0[2] = {0, 0}, lds_col[2] = {0, 0}, tile_x[2] = {0, 0};
    } edge;
};

// Quad forms on the 8 x 8 support: per (kernel row ly, q) the taps left out per side, two bits at 2 * (2 * ly + q).  The pattern
// the kernels are instantiated for is the 2x up-scale with tap 4 (blur 1 and 0.98): q = 0 rows 0 / 6 / 7 leave out 1 / 1 / 2 taps
// per side, q = 1 rows 0 / 1 / 7 leave out 2 / 1 / 1 -- 56 instead of 64 taps per sample.
constexpr uint32_t quad8_bits(int ly, int q, int t) { return static_cast<uint32_t>(t) << (2 * (2 * ly + q)); }
constexpr uint32_t kQuad8TrimTap4Value = quad8_bits(0, 0, 1) | quad8_bits(6, 0, 1) | quad8_bits(7, 0, 2) | quad8_bits(0, 1, 2) |
                                         quad8_bits(1, 1, 1) | quad8_bits(7, 1, 1);
inline constexpr uint32_t PeriodicArgs::kQuad8TrimTap4 = kQuad8TrimTap4Value;
// Does the plan leave out at least what the span forms of `pattern` leave out?  (form -> taps left out in front / behind)
// The 8-row x 9-column support (chroma planes sited as MPEG-2 at 2x with tap 4; ewa_periodic_quad2x8_kernel with nine taps per kernel
// row): span FORM of every (ly, q), three bits at 3 * (2 * ly + q) -- 0 = all nine taps, 1 = taps 1 .. 8, 2 = 1 .. 7, 3 = 2 .. 7, 4 =
// 2 .. 6 (kernel_periodic_quad2x8.hip quad2_row9_span).  Blur 1: q = 0 forms 4 2 1 0 0 0 2 3 for ly = 0 .. 7, q = 1: 3 2 0 0 0 1 2 4 -- 60 of 72.
constexpr uint64_t span9_form(int ly, int q, uint64_t form) { return form << (3 * (2 * ly + q)); }
constexpr uint64_t kQuadSpan9Mpeg2 = span9_form(0, 0, 4) | span9_form(1, 0, 2) | span9_form(2, 0, 1) | span9_form(6, 0, 2) | span9_form(7, 0, 3) |
                                     span9_form(0, 1, 3) | span9_form(1, 1, 2) | span9_form(5, 1, 1) | span9_form(6, 1, 2) | span9_form(7, 1, 4);
constexpr uint64_t kQuadSpan9Mpeg2Swapped = span9_form(0, 1, 4) | span9_form(1, 1, 2) | span9_form(2, 1, 1) | span9_form(6, 1, 2) | span9_form(7, 1, 3) |
                                            span9_form(0, 0, 3) | span9_form(1, 0, 2) | span9_form(5, 0, 1) | span9_form(6, 0, 2) | span9_form(7, 0, 4);
inline bool quad_span9_fits(uint64_t plan, uint64_t pattern) {  // plan: lead / trail per (ly, q) as in PeriodicArgs::quad_span7
    constexpr int lead[5] = {0, 1, 1, 2, 2}, trail[5] = {0, 0, 1, 1, 2};
    for (int k = 0; k < 16; ++k) {
        const int form = static_cast<int>((pattern >> (3 * k)) & 7u);
        if (form > 4) return false;
        if (static_cast<int>((plan >> (4 * k)) & 3u) < lead[form] || static_cast<int>((plan >> (4 * k + 2)) & 3u) < trail[form]) return false;
    }
    return true;
}
// Do the four phase sets of a 6 x 6 support follow the symmetry classes of quad2_share_class bit for bit?  sets[q * 2 + p] = the
// dense 6 x 6 set of phase (p, q).  Every tap of a class must hold the same bits (share_w[class] receives them), every tap outside
// the disc exactly 0.0f: then one product per (sample, class) feeds every chain that takes that tap, bit-identical to a product per
// chain.  Host only.
inline bool quad2_share_classes(const float* const sets[4], float* share_w) {
    bool seen[kQuad2ShareClasses] = {};
    for (int q = 0; q < 2; ++q)
        for (int p = 0; p < 2; ++p)
            for (int ly = 0; ly < 6; ++ly)
                for (int lx = 0; lx < 6; ++lx) {
                    const float c = sets[q * 2 + p][ly * 6 + lx];
                    const int k = quad2_share_class(quad2_share_m(p, lx), quad2_share_m(q, ly));
                    if (k < 0) {
                        if (c != 0.f) return false;
                        continue;
                    }
                    if (!seen[k]) {
                        seen[k] = true;
                        share_w[k] = c;
                    } else if (std::memcmp(&share_w[k], &c, sizeof(float)) != 0) {
                        return false;
                    }
                }
    return true;
}
inline int quad_span9_taps(uint64_t pattern) {  // taps the pattern executes over the 16 (ly, q) rows: twice the taps per sample
    constexpr int n[5] = {9, 8, 7, 6, 5};
    int t = 0;
    for (int k = 0; k < 16; ++k) t += n[(pattern >> (3 * k)) & 7u];
    return t;
}
inline bool quad_span7_fits(uint64_t plan, uint32_t pattern) {
    constexpr int lead[4] = {0, 1, 1, 2}, trail[4] = {0, 0, 1, 1};
    for (int k = 0; k < 12; ++k) {
        const int form = static_cast<int>((pattern >> (2 * k)) & 3u);
        if (static_cast<int>((plan >> (4 * k)) & 3u) < lead[form] || static_cast<int>((plan >> (4 * k + 2)) & 3u) < trail[form]) return false;
    }
    return true;
}
inline int quad_span7_taps(uint32_t pattern) {  // taps per sample the pattern executes, both q averaged x 2 (12 (ly, q) rows)
    constexpr int n[4] = {7, 6, 5, 4};
    int t = 0;
    for (int k = 0; k < 12; ++k) t += n[(pattern >> (2 * k)) & 3u];
    return t;
}
inline bool quad8_pattern_fits(uint32_t plan, uint32_t pattern) {  // the plan leaves out at least what the pattern leaves out
    for (int k = 0; k < 16; ++k)
        if (((plan >> (2 * k)) & 3u) < ((pattern >> (2 * k)) & 3u)) return false;
    return true;
}

// Quasi-periodic interior: the window origins are affine per residue (output pixel (ix0 + px*i + p,
// iy0 + py*j + q) reads the source window at (start_x[p] + sx*i, start_y[q] + sy*j)) but the coefficient
// set is looked up per row and per lane, because the phase classes of drifting ratios change along the axes.
struct QuasiArgs {
    const float* coeffs = nullptr;
    const int32_t* col_class = nullptr;
    const int32_t* row_class = nullptr;
    const int32_t* interior_set = nullptr;
    int n_col_classes = 0, n_row_classes = 0;
    int px = 1, py = 1, sx = 1, sy = 1;
    int ix0 = 0, iy0 = 0, ni = 0, nj = 0;
    int start_x[16] = {0}, start_y[16] = {0};
    int min_sx = 0, min_sy = 0;
    int lds_cols = 0, lds_rows = 0, lds_pitch = 0;  // fp32 source tile staged per workgroup
    int lds_plane = 0;                              // words per column plane (sx planes per tile row)
    int rg = 1;                                     // row groups (of fs output rows) per tile
    int nwaves = 4;                                 // waves per workgroup (divides px*py evenly where possible)
    int exact = 0;                                  // plan is exactly periodic: one set per phase, no per-row lookup
    int phase_split = 1;                            // workgroups per (tile, frame): each takes every phase_split-th share of the phases
    int phase_set[256] = {0};                       // exact plans: set id of phase q*px + p
    int src_w = 0, src_h = 0, dst_h = 0;
};

// LDS row layout of the quasi-periodic kernel, a compile-time function of (filter size, source step) so that every
// LDS offset of its inner loop is an immediate: sx column planes of quasi_plane_words() words each.
constexpr int quasi_tile_cols(int fs, int sx) { return sx * 64 + fs + sx; }  // 64 lanes + window + phase spread <= sx
constexpr int quasi_plane_words(int fs, int sx) {
    const int w = (quasi_tile_cols(fs, sx) + sx - 1) / sx + 1;
    return (sx == 2 || sx == 4) ? ((w + 15) / 32) * 32 + (sx == 2 ? 16 : 8) : w;  // even steps: planes on distinct banks
}
constexpr int quasi_pitch_words(int fs, int sx) { return sx * quasi_plane_words(fs, sx); }

bool quasi_supported(int fs, int px, int py, int sx, int sy, int n_col_classes, int n_row_classes);
// Fills the tile geometry fields (lds_*, rg, nwaves) of `args`; returns false if no configuration fits.
bool quasi_configure(QuasiArgs& args, int fs, int spread_x, int spread_y);
int launch_quasi(const QuasiArgs& args, int fs, const PlaneIO& io, void* stream);

// Exactly periodic plans of any filter size and source step 1..4 (kernel_direct.hip; no LDS, row segments are read
// from memory in the source format with bounds-checked buffer loads).
//   interior  : output pixel (ix0 + px*i + p, iy0 + py*j + q), i < ni, j < nj, reads the source window at
//               (start_x[p] + sx*i, start_y[q] + sy*j) with coefficient set set[q*px + p];
//   row strips: the output rows line0[k] .. line0[k]+line_n[k]-1 (k = 0, 1: above / below the interior) over the
//               interior's column range; window row and coefficient set come from the plan tables per row and phase.
// The row walk of kernel_direct_impl.inc loads coefficient rows up to this many rows before / after a set without using
// them ((R-1) * sy = 3 * 4); upload_table keeps that much addressable memory around the coefficient array.
constexpr int kDirectCoeffSlackRows = 12;
// One rectangle of the runs form (plans whose window origins are affine per residue while the phase classes change now and
// then along an axis -- 1.5x, 3x, ...: PlanePlan::quasi): the pixels of column phase p and row phase q whose period-columns lie
// in one run of constant column class and whose period-rows lie in one run of constant row class.  They share ONE coefficient
// set, and their windows advance by (sx, sy) source samples per period -- inside the rectangle the plan is exactly periodic.
struct DirectRun {
    int32_t set = 0;
    int32_t x0 = 0, y0 = 0;    // output pixel of the first period (then every px-th column, py-th row)
    int32_t sx0 = 0, sy0 = 0;  // its window origin
    int32_t ni = 0, nj = 0;    // periods
    int32_t first_wave = 0;    // items before this rectangle's first (an item = 64 lanes x 4 x 4 periods)
};

struct DirectArgs {
    const float* coeffs = nullptr;
    int fs = 0, coeff_row = 0;   // filter size; floats per coefficient row on the device (padded_row(fs))
    int px = 1, py = 1, sx = 1, sy = 1;
    int ix0 = 0, iy0 = 0, ni = 0, nj = 0;
    int start_x[16] = {0}, start_y[16] = {0};
    int set[256] = {0};          // interior only
    int line0[2] = {0, 0}, line_n[2] = {0, 0};  // strips only
    DevicePlan plan;             // strips only: row/column tables
    uint32_t src_bytes = 0;      // readable bytes from the aligned-down base of one source plane (filter.cpp direct_src_bytes)
    int dst_h = 0;
    // runs form only: the rectangles, the rectangle of every item, items per frame
    const DirectRun* runs = nullptr;
    const int32_t* item_run = nullptr;
    int n_items = 0;
};
bool direct_supported(int fs, int px, int py, int sx, int sy);
// Probe of the hardware premise of kernel_direct.hip (the buffer range check covers the scalar offset): `buf` holds
// 2 * nbytes bytes with dword i = i, `out` 128 dwords.  See load_raw in kernel_direct.hip.
int launch_soffset_probe(const uint32_t* buf, uint32_t nbytes, uint32_t* out, void* stream);
int launch_direct(const DirectArgs& args, const PlaneIO& io, void* stream);
// Interior form launch_direct picks (kernel_direct_impl.inc DirectShape: 0 per-chain fetches, 2 row walk, 3 row walk with 8
// columns per lane); set_direct_shape forces one process-wide where it applies (tests, A/B runs; -1 = automatic),
// last_direct_shape reports the most recent launch's.
void set_direct_shape(int shape);
int last_direct_shape();
// row-walk interior forms (DirectShape 2 / 3), one translation unit per sample type and source step
// (kernel_direct_walk_*_sx*.hip)
#define JINC_DECLARE_DIRECT_WALK(tag)                                                            \
    int launch_direct_walk_##tag##_sx1(const DirectArgs&, const PlaneIO&, void* stream, int shape); \
    int launch_direct_walk_##tag##_sx2(const DirectArgs&, const PlaneIO&, void* stream, int shape); \
    int launch_direct_walk_##tag##_sx3(const DirectArgs&, const PlaneIO&, void* stream, int shape); \
    int launch_direct_walk_##tag##_sx4(const DirectArgs&, const PlaneIO&, void* stream, int shape);
JINC_DECLARE_DIRECT_WALK(u8)
JINC_DECLARE_DIRECT_WALK(u16)
JINC_DECLARE_DIRECT_WALK(f16)
JINC_DECLARE_DIRECT_WALK(bf16)
JINC_DECLARE_DIRECT_WALK(f32)
#undef JINC_DECLARE_DIRECT_WALK
int launch_direct_row_strips(const DirectArgs& args, const PlaneIO& io, void* stream);
// Runs form (DirectRun): ewa_direct_kernel's row walk over the rectangles of a drifting plan, one launch per plane.
bool direct_runs_supported(int fs, int px, int py, int sx, int sy);
int launch_direct_runs(const DirectArgs& args, const PlaneIO& io, void* stream);
#define JINC_DECLARE_DIRECT_RUNS(tag)                                                 \
    int launch_direct_runs_##tag##_sx1(const DirectArgs&, const PlaneIO&, void* stream); \
    int launch_direct_runs_##tag##_sx2(const DirectArgs&, const PlaneIO&, void* stream); \
    int launch_direct_runs_##tag##_sx3(const DirectArgs&, const PlaneIO&, void* stream); \
    int launch_direct_runs_##tag##_sx4(const DirectArgs&, const PlaneIO&, void* stream);
JINC_DECLARE_DIRECT_RUNS(u8)
JINC_DECLARE_DIRECT_RUNS(u16)
JINC_DECLARE_DIRECT_RUNS(f16)
JINC_DECLARE_DIRECT_RUNS(bf16)
JINC_DECLARE_DIRECT_RUNS(f32)
#undef JINC_DECLARE_DIRECT_RUNS

// Left / right border columns of an exactly periodic plan over the interior's row range (kernel_colstrip.hip):
// item = (output column x, row phase q), lanes = 64 consecutive period-rows, source footprint staged in LDS.
struct ColStripArgs {
    const float* coeffs = nullptr;
    int fs = 0, coeff_row = 0;
    int py = 1, sy = 1, iy0 = 0, nj = 0;
    int start_y[16] = {0};
    int min_sy = 0, spread_y = 0;          // min over phases of start_y, max - min
    int x0[2] = {0, 0}, nx[2] = {0, 0};    // output column runs: left, right
    int src_c0[2] = {0, 0}, src_w[2] = {0, 0};  // source columns their windows cover
    int groups[2] = {0, 0}, group_cols = 1;     // blocks per run, columns per block (colstrip_configure)
    int col_shift = 0;                          // staging: 1 << col_shift lanes per source row
    DevicePlan plan;
};
bool colstrip_configure(ColStripArgs& args);
int launch_colstrip(const ColStripArgs& args, const PlaneIO& io, void* stream);

// Frame-lane kernel (kernel_framelane.hip): batches of frames, any plan.  The 64 lanes of a wave are the same output
// pixel of 64 different frames, so coefficients are wave-uniform (SGPRs) whatever the plan's structure.
constexpr int kFrameLaneMaxTile = 32;  // output tile edge limit
// LDS bytes of a workgroup's tables in front of its tile: window origins of the tile's columns and rows, and the coefficient
// set of every pixel (row pitch kFrameLaneMaxTile) for the tile's (1 << ty_shift) rows.
constexpr int kFrameLaneTableBytes(int ty_shift) { return (2 * kFrameLaneMaxTile + kFrameLaneMaxTile * (1 << ty_shift)) * 4; }
constexpr int kFrameLanePosBytes(size_t sample_bytes) { return static_cast<int>(64 * sample_bytes + 4); }  // LDS bytes per source position
// Frame-pair form (kernel_framelane_pair.hip): 128 frames per workgroup, a lane owns two adjacent frames; 8-byte pad for
// float planes keeps a lane's pair 8-byte aligned at every position.
constexpr int kFrameLanePairFrames = 128;
constexpr int kFrameLanePairPosBytes(size_t sample_bytes) { return static_cast<int>(128 * sample_bytes + (sample_bytes == 4 ? 8 : 4)); }
struct FrameLaneArgs {
    DevicePlan plan;
    PlaneIO io;
    RectList rects;           // rectangles of the output plane to compute (x0/y0/w/h only)
    int block_begin[5] = {0, 0, 0, 0, 0};  // first tile of each rectangle; [4] = number of tiles
    int tiles_x[4] = {1, 1, 1, 1};
    int tx_shift = 5, ty_shift = 5;        // tile = (1 << tx_shift) x (1 << ty_shift) output pixels, tx >= 4, ty >= 4
    int threads = 512;
    int lds_bytes = 0;
    int vec_store_ok = 0;     // bit 0: destination base, pitch and frame stride are multiples of 4 samples; bit 1: of 16 bytes
    int variant = 0;          // 0: automatic (sliding-window form for filter sizes 5, 7, 8, 9), 1: row-segment form always
    int pair = 0;             // 1: configured for the frame-pair form (128 frames per workgroup)
    int subgroups = 0;        // ewa_framelane_sub_kernel: sub-groups per wave (2 / 4 / 8 = 32 / 16 / 8 frames per workgroup); set per launch
};
// Chooses the tile size for the rectangles `rects` of plane plan `p` (host arrays) so that every tile's source
// footprint fits the LDS budget and is at most 64 columns wide; false if no tile size fits (huge filter footprints).
struct PlanePlan;
bool framelane_configure(const PlanePlan& p, const RectList& rects, int sample_bytes, int nframes_hint, FrameLaneArgs& out);
int launch_framelane(const FrameLaneArgs& args, void* stream);
// Groups of fewer than 64 frames (kernel_framelane_sub.hip): a wave is args.subgroups sub-groups of 64 / subgroups lanes, each on
// its own output row of the tile; filter sizes 5, 7, 8, 9 (the sliding-window form's) on a tile configuration of framelane_configure.
bool framelane_sub_supported(int fs, int subgroups, int ty_shift);
int launch_framelane_sub(const FrameLaneArgs& args, void* stream);
// Frame-pair form: filter sizes 5 and 7 only (two windows per lane in 128 registers); false otherwise or if no tile fits.
bool framelane_pair_configure(const PlanePlan& p, const RectList& rects, int sample_bytes, int nframes_hint, FrameLaneArgs& out);
int launch_framelane_pair(const FrameLaneArgs& args, void* stream);

// Generic gather kernel: one lane per output pixel, any plan.  Returns a hipError_t value as int.
int launch_gather(const DevicePlan& plan, const PlaneIO& io, const RectList& rects, void* stream);

// True when a specialised periodic kernel exists for this filter size / period / sample type.
bool periodic_supported(int fs, int px, int py, int sx, int sy);
// variant: 0 = default choice per filter size, 1 = always the row-streamed kernel (A/B measurements)
int launch_periodic(const PeriodicArgs& args, int fs, const PlaneIO& io, void* stream, int variant = 0);
// kernel_strip.hip: border rows (axis 0: lanes along x) or border columns (axis 1: lanes along y) of an exactly periodic plan,
// one register window per lane for the strip's whole thickness.  A group = the lines (output rows | columns) of one strip: they
// share the source lines [origin, origin + fs) across the strip; along the strip output coordinate i0 + P * i + p reads the
// window at start[p] + i (source step 1) and line `l` of group g uses coefficient set sets[(set_base[g] + l) * P + p].
struct StripArgs {
    const float* coeffs = nullptr;
    const int32_t* sets = nullptr;  // device
    int fs = 0, axis = 0;
    int P = 1, S = 1;
    int i0 = 0, ni = 0;
    int start[16] = {0};
    int min_start = 0, spread = 0;
    int ngroups = 0;
    int line0[4] = {0, 0, 0, 0}, nlines[4] = {0, 0, 0, 0}, origin[4] = {0, 0, 0, 0}, set_base[4] = {0, 0, 0, 0};
    int src_w = 0, src_h = 0, dst_h = 0;
};
// Border columns on packed column pairs (kernel_colpair.hip): side s (0 left, 1 right) = n[s] output columns from x0[s] on, all with the
// source window columns origin[s] .. origin[s] + fs - 1; output row iy0 + py * j + q reads the source rows start_y[q] + j ...
// coeffs[(((s * kMaxGroups + g) * py + q) * fs + ly) * 4 fs + 4 lx + k] = set(x0[s] + 4 g + k, q)[ly][lx] (0 beyond the side's last column).
struct ColPairArgs {
    static constexpr int kMaxGroups = 6;  // groups of four columns per side
    const float* coeffs = nullptr;
    int fs = 0, py = 1, iy0 = 0, nj = 0;
    int start_y[4] = {0, 0, 0, 0};
    int min_sy = 0, spread = 0;
    int n[2] = {0, 0}, x0[2] = {0, 0}, origin[2] = {0, 0};
    int src_w = 0, src_h = 0, dst_h = 0;
};
bool colpair_supported(int fs, int py, int sy, int spread);
int launch_colpair(const ColPairArgs& args, const PlaneIO& io, void* stream);

bool strip_supported(int fs, int period, int step, int spread);
int launch_strip(const StripArgs& args, const PlaneIO& io, void* stream);
// kernel_rowpair.hip: the row-streamed kernel in packed phase-pair form (PeriodicArgs::rowpair; 12 .. 17 taps per kernel row)
bool rowpair_supported(int taps_per_row);
bool rowpair_strip_supported(int taps_per_row);  // ... as strips of border rows (PeriodicArgs::rowpair_strip_phases)
int launch_rowpair(const PeriodicArgs& args, const PlaneIO& io, void* stream);
// kernel_scan.hip: flags[frame] = 1 where the frame's float source plane (w x h samples) holds an infinity or a NaN
int launch_finite_scan(const PlaneIO& io, int w, int h, uint32_t* flags, void* stream);
// ... the same over the samples of the plane OUTSIDE the rectangle [rx0, rx1) x [ry0, ry1) only (what a trimmed launch that flags
// the samples it stages itself does not see: PeriodicArgs::kRunAllAndFlag)
int launch_finite_scan_outside(const PlaneIO& io, int w, int h, int rx0, int ry0, int rx1, int ry1, uint32_t* flags, void* stream);

// Compatibility modes: the summation order of the reference's SIMD paths (kernel_simdorder.hip).  order 1 = SSE4.1,
// 2 = AVX2, 3 = AVX-512; min_val = lower clamp of float source samples of this plane.
int launch_simd_order(const DevicePlan& plan, const PlaneIO& io, int order, float min_val, void* stream);

// Frame transport by the shader (kernel_blit.hip): entry = one plane of one frame, `rows` rows of `row_bytes` bytes from
// src (pitch src_pitch) to dst (pitch dst_pitch); either side may be host memory mapped into the device's address space.
// unit = 16 / 4 / 1: widest access both pointers and pitches allow (blit_unit).  The table lives in memory the device can
// read (the pipeline keeps it in pinned host memory); one launch moves entries [first, first + count).
struct BlitEntry {
    const void* src = nullptr;
    void* dst = nullptr;
    uint32_t src_pitch = 0, dst_pitch = 0, row_bytes = 0, rows = 0, unit = 1, pad = 0;
};
int blit_unit(const void* src, const void* dst, uint32_t src_pitch, uint32_t dst_pitch);
// max_rows / max_row_bytes: the largest plane among the entries (work is cut into slices of ~64 KB of rows); workgroups:
// how many run at once (the link bounds the kernel, the rest of the chip stays free for the resampling kernels).
int launch_blit_rows(const BlitEntry* table_device, int first, int count, uint32_t max_rows, uint32_t max_row_bytes, int workgroups,
                     void* stream);

// Interleaved samples <-> dense planes (kernel_interleave.hip; jinc_filter_process_device_strided).  A channel group = the planes
// whose samples share the pixels of one interleaved buffer: `step` samples per pixel, channel c of pixel x of row y of frame n at
// packed + n * packed_frame_stride + y * packed_pitch + (x * step + c) * sample_bytes, and in the dense plane of channel c
// (plane[c]; nullptr: that channel was not given and is neither read nor written) at plane[c] + n * plane_frame_stride +
// y * plane_pitch + x * sample_bytes.  Channel 0 is always given (the group's lowest base).  The dense planes are the filter's own:
// bases, pitch and frame stride multiples of 256 bytes.
// unit: widest access the packed side allows (16 / 4: base, pitch and frame stride are multiples of it; 0: sample-sized accesses
// only); vec_pixels: the leading pixels of every row that move by such accesses, a multiple of the 16 / sample_bytes pixels a lane
// owns -- the merge of an incomplete group has none (only the given channels' samples may be stored to), the split of one stops in
// front of the row's last pixel, whose missing channels may lie behind the end of the caller's buffer.
// shift[c] (jinc_filter_process_device_shifted, 16-bit samples): the packed side keeps channel c's sample in the high bits of its
// word -- the dense plane holds packed >> shift, the packed side gets (dense << shift) & 0xffff.  A group with a shift may have
// step 1: one dense plane of the caller's, shifted into / out of its dense stand-in.
struct InterleaveGroup {
    char* packed = nullptr;
    char* plane[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t packed_frame_stride = 0, plane_frame_stride = 0;
    uint32_t packed_pitch = 0, plane_pitch = 0, width = 0, rows = 0, vec_pixels = 0, unit = 0;
    uint8_t shift[4] = {0, 0, 0, 0};
};
// The groups of ONE launch travel as kernel arguments: a table in memory would have to stay untouched until the launch has run,
// and the call returns before that.
struct InterleaveArgs {
    InterleaveGroup g[4];
    int ngroups = 0;
};
// One launch over every group and frame of `a`: sample_bytes 1, 2 or 4; step 2, 3 or 4 (the same for all groups of a launch).
// With a non-zero shift in any group the launch takes the shifted forms: sample_bytes 2 only, step 1 .. 4.
// shifted (may be nullptr) receives that decision: true when the launch took a shifted form (jinc_debug_last_groups).
int launch_split_samples(const InterleaveArgs& a, int sample_bytes, int step, int nframes, void* stream, bool* shifted = nullptr);
int launch_merge_samples(const InterleaveArgs& a, int sample_bytes, int step, int nframes, void* stream, bool* shifted = nullptr);

// 10:10:10:2 words <-> three dense 16-bit planes (kernel_interleave.hip; jinc_filter_process_device_packed10).  One little-endian
// 32-bit word per pixel: pixel x of row y of frame n at packed + n * packed_frame_stride + y * packed_pitch + 4 * x, its value of
// plane c in bits offset[c] .. offset[c] + 9; the dense plane of c holds that value in a 16-bit sample at plane[c] +
// n * plane_frame_stride + y * plane_pitch + 2 * x.  The three planes have one size; they are the filter's own (bases, pitch and
// frame stride multiples of 256 bytes).  packed base, pitch and frame stride are multiples of 4 (dispatch.cpp refuses others).
// unit: 16 where they are multiples of 16 as well (16-byte accesses on the word side), else 4 (dwords); vec_pixels: the leading
// pixels of a row that move 8 per lane, a multiple of 8; the rest of the row moves word by word.
// fill (pack only): the bits of every stored word outside the three fields -- the caller's dst_fill with the fields cleared.
struct FieldArgs {
    char* packed = nullptr;
    char* plane[3] = {nullptr, nullptr, nullptr};
    size_t packed_frame_stride = 0, plane_frame_stride = 0;
    uint32_t packed_pitch = 0, plane_pitch = 0, width = 0, rows = 0, vec_pixels = 0, unit = 4;
    uint32_t offset[3] = {0, 0, 0};
    uint32_t fill = 0;
};
// One launch over every row and frame of `a`.
int launch_unpack_fields(const FieldArgs& a, int nframes, void* stream);
int launch_pack_fields(const FieldArgs& a, int nframes, void* stream);

// v210 blocks <-> the three dense 16-bit planes of a 10-bit 4:2:2 frame (kernel_interleave.hip, v210_rows.h;
// jinc_filter_process_device_v210).  Block b of row y of frame n lies at blocks + n * block_frame_stride + y * block_pitch + 16 * b
// and holds luma samples 6b .. 6b+5 and chroma samples 3b .. 3b+2 of both chroma planes (the field table: v210_rows.h).  plane[0]
// is the luma plane, `width` samples wide, sample x at plane[0] + n * luma_frame_stride + y * luma_pitch + 2 * x; plane[1] = Cb
// and plane[2] = Cr are width / 2 wide and share chroma_pitch and chroma_frame_stride.  The planes are the filter's own (bases,
// pitches and frame strides multiples of 256 bytes).  Base, pitch and frame stride of the blocks are multiples of 4 (dispatch.cpp
// refuses others); unit: 16 where they are multiples of 16 as well (one 16-byte access per block), else 4 (four dwords).
// whole_blocks: width / 6, the blocks of a row whose six pixels all lie inside it; a row has one more, partial, block when
// width is no multiple of 6.
struct V210Args {
    char* blocks = nullptr;
    char* plane[3] = {nullptr, nullptr, nullptr};
    size_t block_frame_stride = 0, luma_frame_stride = 0, chroma_frame_stride = 0;
    uint32_t block_pitch = 0, luma_pitch = 0, chroma_pitch = 0, width = 0, rows = 0, whole_blocks = 0, unit = 4;
};
// One launch over every row and frame of `a`.
int launch_unpack_v210(const V210Args& a, int nframes, void* stream);
int launch_pack_v210(const V210Args& a, int nframes, void* stream);

// Integer samples -> the dense planes of an fp32 / binary16 filter (kernel_widen.hip, widen_rows.h;
// jinc_filter_process_device_widened).  A channel group as in InterleaveGroup, read only: `step` source samples of src_bytes (1: a
// byte; 2: a little-endian 16-bit word) per pixel at packed, channel c of pixel x of row y of frame n at packed +
// n * packed_frame_stride + y * packed_pitch + (x * step + c) * src_bytes.  The dense plane of channel c (plane[c]; nullptr: not
// given, neither read nor written) holds float / binary16 ((raw >> shift[c]) & mask) at plane[c] + n * plane_frame_stride +
// y * plane_pitch + x * out_bytes.  A group may have step 1: every source plane of such a call takes a stand-in.  The dense planes
// are the filter's own: bases, pitch and frame stride multiples of 256 bytes.
// unit / vec_pixels as in InterleaveGroup, with 16 / src_bytes pixels per lane: a group with a channel missing stops its vectors in
// front of the row's last pixel.
struct WidenGroup {
    const char* packed = nullptr;
    char* plane[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t packed_frame_stride = 0, plane_frame_stride = 0;
    uint32_t packed_pitch = 0, plane_pitch = 0, width = 0, rows = 0, vec_pixels = 0, unit = 0;
    uint8_t shift[4] = {0, 0, 0, 0};
    float scale[4] = {1.f, 1.f, 1.f, 1.f}, offset[4] = {0.f, 0.f, 0.f, 0.f};  // read by the scaled forms only
};
struct WidenArgs {
    WidenGroup g[4];
    int ngroups = 0;
    uint32_t mask = 0xffu;  // (1 << src_bits) - 1
};
// One launch over every group and frame of `a`: src_bytes 1 or 2 (a byte takes no shift: mask 0xff, shifts 0); step 1 .. 4 (the
// same for all groups of a launch); out_bytes 4 (fp32) or 2 (out_kind 0 / kSampleHalf: binary16, every value must be <= 2047 to be
// exact; out_kind kSampleBFloat16: bfloat16, src_bytes 1 only -- nine bits are not exact).
// scaled (jinc_filter_process_device_widened_scaled): plane c holds fl32(fl32(float(value) * scale[c]) + offset[c]) -- two fp32
// roundings, never an FMA -- narrowed round-to-nearest-even into 16-bit planes; the conversion is a defined rounding, so neither the
// 2047 rule nor the bytes-only rule of bfloat16 applies.
int launch_widen_samples(const WidenArgs& a, int src_bytes, int step, int out_bytes, int out_kind, int nframes, void* stream, bool scaled = false);
// 10:10:10:2 words / v210 blocks -> the three dense planes of an fp32 / binary16 filter (kernel_widen.hip, widen_fields_rows.h,
// widen_v210_rows.h; jinc_filter_process_device_widened_packed10 / _v210).  The records are FieldArgs and V210Args as they are, read
// with samples of out_bytes (4: fp32, 2: binary16) on the plane side: plane c holds float / binary16 of the 10-bit field value at
// plane[c] + n * frame stride + y * pitch + x * out_bytes (pitches and frame strides stay in bytes).  The word / block side is read
// only; `fill` is not read.  One launch over every row and frame of `a`.
// The scaled forms (jinc_filter_process_device_widened_packed10_scaled / _widened_v210_scaled): the records carry one pair per plane
// (library order; v210: Y, Cb, Cr) behind FieldArgs / V210Args, as NarrowFieldArgs / NarrowV210Args below do, and plane c holds
// fl32(fl32(float(field) * value_scale[c]) + value_offset[c]) -- two fp32 roundings, never an FMA -- narrowed round-to-nearest-even
// into 16-bit planes: a defined rounding, so bfloat16 planes are filled too.  The pairs are kernel arguments, the same in every lane.
struct WidenFieldArgs : FieldArgs {
    float value_scale[3] = {1.f, 1.f, 1.f}, value_offset[3] = {0.f, 0.f, 0.f};  // read by the scaled forms only
};
struct WidenV210Args : V210Args {
    float value_scale[3] = {1.f, 1.f, 1.f}, value_offset[3] = {0.f, 0.f, 0.f};  // read by the scaled forms only
};
// out_kind 0 (fp32), kSampleHalf or kSampleBFloat16; bfloat16 with scaled only (ten bits are not exact in it): every other shape
// is hipErrorInvalidValue, never a silent skip.
int launch_widen_fields(const WidenFieldArgs& a, int out_kind, int nframes, void* stream, bool scaled = false);
int launch_widen_v210(const WidenV210Args& a, int out_kind, int nframes, void* stream, bool scaled = false);

// The dense planes of an fp32 / binary16 / bfloat16 filter -> INTEGER samples (kernel_narrow.hip, narrow_rows.h;
// jinc_filter_process_device_narrowed): the mirror of WidenGroup.  A channel group as in InterleaveGroup, written only: `step`
// destination samples of dst_bytes (1: a byte; 2: a little-endian 16-bit word) per pixel at packed, channel c of pixel x of row y of
// frame n at packed + n * packed_frame_stride + y * packed_pitch + (x * step + c) * dst_bytes.  The dense plane of channel c
// (plane[c]; nullptr: not given, its samples are not stored to) holds the filter's results, in_bytes (4: fp32; 2: binary16 or
// bfloat16) a sample, at plane[c] + n * plane_frame_stride + y * plane_pitch + x * in_bytes; the stored sample is
// lrintf(clamp(result, 0, peak)) << shift[c].  A group may have step 1: every destination plane of such a call takes a stand-in.  The
// dense planes are the filter's own: bases, pitch and frame stride multiples of 256 bytes.
// unit as in InterleaveGroup, of the packed side; vec_pixels: the leading pixels of every row stored by such accesses, a multiple of
// the 16 / dst_bytes pixels a lane owns -- none in a group with a channel missing (only the given channels' samples may be stored to).
struct NarrowGroup {
    char* packed = nullptr;
    const char* plane[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t packed_frame_stride = 0, plane_frame_stride = 0;
    uint32_t packed_pitch = 0, plane_pitch = 0, width = 0, rows = 0, vec_pixels = 0, unit = 0;
    uint8_t shift[4] = {0, 0, 0, 0};
    float scale[4] = {1.f, 1.f, 1.f, 1.f}, offset[4] = {0.f, 0.f, 0.f, 0.f};  // read by the scaled forms only
};
struct NarrowArgs {
    NarrowGroup g[4];
    int ngroups = 0;
    float peak = 255.f;  // (1 << dst_bits) - 1
};
// One launch over every group and frame of `a`: in_kind 0 (fp32), kSampleHalf or kSampleBFloat16; step 1 .. 4 (the same for all
// groups of a launch); dst_bytes 1 (peak 255, shifts 0) or 2 (peak 511 .. 65535, peak << shift below 65536).
// scaled (jinc_filter_process_device_narrowed_scaled): the stored sample is
// lrintf(clamp(fl32(fl32(result * scale[c]) + offset[c]), 0, peak)) << shift[c] -- two fp32 roundings, never an FMA.
int launch_narrow_samples(const NarrowArgs& a, int in_kind, int step, int dst_bytes, int nframes, void* stream, bool scaled = false);
// The three dense planes of an fp32 / binary16 / bfloat16 filter -> 10:10:10:2 words / v210 blocks (kernel_narrow.hip,
// narrow_fields_rows.h, narrow_v210_rows.h; jinc_filter_process_device_narrowed_packed10 / _v210).  The records are FieldArgs and
// V210Args with the scaled calls' pair per plane behind them; the plane side is READ only, with samples of in_bytes (4: fp32; 2:
// binary16 or bfloat16) at plane[c] + n * frame stride + y * pitch + x * in_bytes (pitches and frame strides stay in bytes), and the
// word / block side is written only: field c of a word or block holds lrintf(clamp(result, 0, 1023)) -- or, in the scaled forms,
// lrintf(clamp(fl32(fl32(result * value_scale[c]) + value_offset[c]), 0, 1023)): two fp32 roundings, never an FMA.  Words are stored
// whole with `fill` in the bits outside the fields; blocks are stored whole with zeros in bits 30 - 31 and in the fields of a partial
// last block beyond `width`.
struct NarrowFieldArgs : FieldArgs {
    float value_scale[3] = {1.f, 1.f, 1.f}, value_offset[3] = {0.f, 0.f, 0.f};  // read by the scaled forms only
};
struct NarrowV210Args : V210Args {
    float value_scale[3] = {1.f, 1.f, 1.f}, value_offset[3] = {0.f, 0.f, 0.f};  // read by the scaled forms only
};
// One launch over every row and frame of `a`: in_kind 0 (fp32), kSampleHalf or kSampleBFloat16.
int launch_narrow_fields(const NarrowFieldArgs& a, int in_kind, int nframes, void* stream, bool scaled = false);
int launch_narrow_v210(const NarrowV210Args& a, int in_kind, int nframes, void* stream, bool scaled = false);

// The 3x3 output matrix of a float filter (kernel_matrix.hip, matrix_rows.h; jinc_filter_set_output_matrix): planes 0 .. 2 of an
// fp32 / binary16 / bfloat16 filter's results, three planes of ONE size, updated in place.  Sample x of row y of frame n of plane c
// lies at plane[c] + n * frame_stride[c] + y * pitch[c] + x * sample bytes (4: fp32; 2: binary16 or bfloat16); with r0, r1, r2 the
// three samples of a pixel widened exactly to fp32, plane i gets
//   fl32(fl32(fl32(fl32(m[3i] * r0) + fl32(m[3i+1] * r1)) + fl32(m[3i+2] * r2)) + offset[i])
// -- three multiplies and three adds, each rounded to fp32, in this order, never an FMA -- rounded to nearest even into the sample
// type by the conversions the kernels' own stores use.  The planes are the result stand-ins (256-byte aligned) or the caller's own
// destination planes: unit is 16 where every base, pitch and frame stride is a multiple of 16 bytes, 4 where of 4 only, else 0;
// vec_pixels: the leading pixels of every row moved by 16-byte (unit 16) or dword (unit 4) accesses, a multiple of the 16 / sample
// bytes pixels a lane owns, 0 with unit 0.  Nothing beyond `width` samples of a row is read or written.
struct MatrixArgs {
    char* plane[3] = {nullptr, nullptr, nullptr};
    size_t frame_stride[3] = {0, 0, 0};
    uint32_t pitch[3] = {0, 0, 0};
    uint32_t width = 0, rows = 0, vec_pixels = 0, unit = 0;
    float m[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, offset[3] = {0.f, 0.f, 0.f};
};
// One launch over every row and frame of `a`: kind 0 (fp32), kSampleHalf or kSampleBFloat16; anything else, a null plane or a
// unit / vec_pixels pair that is none of the above is hipErrorInvalidValue, never a silent skip.
int launch_output_matrix(const MatrixArgs& a, int kind, int nframes, void* stream);

// Measurement hook (kernel_probe.hip): `samplers` single-lane workgroups stamp the shader clock counter and the 100 MHz
// real-time counter until *stop_flag (device memory) becomes non-zero or max_seconds pass; out[2 k] = shader ticks,
// out[2 k + 1] = real-time ticks of sampler k.
int launch_clock_sampler(const int* stop_flag, unsigned long long* out, int samplers, double max_seconds, void* stream);

// Measurement hook: `blocks` x 256 lanes run iters x 8 (v_mul_f32 with an SGPR coefficient, v_add_f32 onto one chain);
// out holds blocks x 256 floats.
int launch_valu_pair_probe(float* out, int blocks, int iters, void* stream);

// Test hook: applies the kernels' float -> sample conversion (clamp, round-half-even, store) to n sums.
int launch_debug_convert(const float* in, void* out, int n, int sample_bytes, float peak, void* stream);
// ... the binary16 stores of half planes (both the plain and the buffer-store paths, and the packed pair)
int launch_debug_convert_half(const float* in, uint16_t* out, int n, void* stream);
// ... and the bfloat16 stores (the single conversion and the packed pair's)
int launch_debug_convert_bfloat16(const float* in, uint16_t* out, int n, void* stream);

}  // namespace jinc
