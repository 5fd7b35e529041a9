// Stand-alone driver of the SCALED form of csrc/widen_rows.h (tests/test_scaled_host.py), built once plain and once under
// AddressSanitizer + UndefinedBehaviorSanitizer: widen_row<SB, N, OB, KIND, true> runs on the CPU lane by lane, exactly as the
// kernel calls it, for every form SB x N x (fp32, binary16, bfloat16), widths 1 .. 70, the three access classes (16-byte, dword,
// sample sized), groups with every channel given or with channels missing, and a scale / offset pair of its own for every channel:
// the limited-range luma and chroma pairs of the depth, the full-range pair and an odd negative one.  Bytes hold 8 bits; words hold
// 10 bits at shift 6 and all 16 bits at shift 0, into every type -- the scaled conversion is a rounding, not a claim of exactness.
// And, with one sample per pixel, ALL 65536 16-bit values in one row at the full-range pair, the limited-range luma pair, a pair
// that overflows binary16 and a negative scale, into the three types: subnormals, ties and infinities of the 16-bit roundings.
// Every buffer is allocated to EXACTLY the bytes the contract allows to be touched, as in widen_rows_main.cpp; row padding holds a
// canary that is checked, and the source must come back unchanged.
// The expectations are NOT computed here: every case is written to the file named on the command line -- a header of 16 uint32
// (SB, N, OB, KIND, bits, width, rows, unit, given-channel mask, shift[4], 3 x 0), scale[4] and offset[4] as fp32, the source samples
// row by row without padding, then the dense plane of every given channel row by row without padding -- and the test compares with
// numpy.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "widen_rows.h"

namespace {

uint32_t g_state = 0x2545F491u;
uint32_t rnd() {  // xorshift32
    g_state ^= g_state << 13, g_state ^= g_state >> 17, g_state ^= g_state << 5;
    return g_state;
}

constexpr unsigned char kCanary = 0xA5;

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

template <int SB, int N, int OB, int KIND>
void run_rows(const jinc::WidenGroup& g, uint32_t mask) {
    for (uint32_t row = 0; row < g.rows; ++row)
        for (uint32_t lane = 0; lane < 64; ++lane) jinc::widen::widen_row<SB, N, OB, KIND, true>(g, mask, 0, row, lane);
}

template <int SB, int OB, int KIND>
void run_by_step(int n, const jinc::WidenGroup& g, uint32_t mask) {
    switch (n) {
        case 1: return run_rows<SB, 1, OB, KIND>(g, mask);
        case 2: return run_rows<SB, 2, OB, KIND>(g, mask);
        case 3: return run_rows<SB, 3, OB, KIND>(g, mask);
        case 4: return run_rows<SB, 4, OB, KIND>(g, mask);
    }
    abort();
}

template <int SB>
void run_by_kind(int n, int ob, int kind, const jinc::WidenGroup& g, uint32_t mask) {
    if (ob == 4) run_by_step<SB, 4, 0>(n, g, mask);
    else if (kind == jinc::kSampleBFloat16) run_by_step<SB, 2, jinc::kSampleBFloat16>(n, g, mask);
    else run_by_step<SB, 2, jinc::kSampleHalf>(n, g, mask);
}

void run(int sb, int n, int ob, int kind, const jinc::WidenGroup& g, uint32_t mask) {
    if (sb == 1) run_by_kind<1>(n, ob, kind, g, mask);
    else run_by_kind<2>(n, ob, kind, g, mask);
}

struct Pair {
    float scale, offset;
};

// The pairs of a depth: limited-range luma, limited-range chroma, full range, and one no range table holds.
void pairs_of(int bits, Pair out[4]) {
    const double k = static_cast<double>(1 << (bits - 8)), peak = static_cast<double>((1 << bits) - 1);
    out[0] = {static_cast<float>(1.0 / (219.0 * k)), static_cast<float>(-16.0 * k / (219.0 * k))};
    out[1] = {static_cast<float>(1.0 / (224.0 * k)), static_cast<float>(-128.0 * k / (224.0 * k))};
    out[2] = {static_cast<float>(1.0 / peak), 0.f};
    out[3] = {-0.37f, 3.25f};
}

// given: bit c = channel c has a plane (bit 0 always).  values: the samples of channel 0's only row (rows 1, n 1), or nullptr for
// pseudo-random sources.  Returns the number of wrong bytes outside the samples.
long one_case(FILE* out, int sb, int n, int ob, int kind, int bits, int shift, int width, int rows, uint32_t unit, uint32_t given,
              const Pair pairs[4], const std::vector<uint16_t>* values) {
    long wrong = 0;
    int last_given = 0;
    for (int c = 0; c < n; ++c)
        if (given >> c & 1) last_given = c;
    // source: base offset and pitch of the access class; the allocation ends behind the last given sample
    const size_t row_bytes = static_cast<size_t>(width) * n * sb;
    const size_t lead = unit == 16 ? 0 : unit == 4 ? 4 : sb;
    const size_t pitch = unit == 16 ? align_up(row_bytes, 16) : unit == 4 ? align_up(row_bytes, 16) + 4 : align_up(row_bytes, 4) + (sb == 1 ? 1 : 2);
    const size_t last_row = (static_cast<size_t>(width - 1) * n + last_given + 1) * sb;
    const size_t src_bytes = lead + pitch * (rows - 1) + last_row;
    void* p = nullptr;
    if (posix_memalign(&p, 16, src_bytes)) abort();
    unsigned char* src = static_cast<unsigned char*>(p);
    for (size_t k = 0; k < src_bytes; ++k) src[k] = static_cast<unsigned char>(rnd());  // (every bit below and above the sample included)
    if (values)
        for (int x = 0; x < width; ++x) {
            const uint16_t v = static_cast<uint16_t>((*values)[x] << shift);
            memcpy(src + lead + static_cast<size_t>(x) * sb, &v, sb);
        }
    const std::vector<unsigned char> src_before(src, src + src_bytes);

    jinc::WidenGroup g;
    g.packed = reinterpret_cast<const char*>(src) + lead;
    g.packed_pitch = static_cast<uint32_t>(pitch);
    g.width = static_cast<uint32_t>(width), g.rows = static_cast<uint32_t>(rows);
    g.unit = unit;
    const uint32_t lane_pixels = 16u / sb, vec_from = given == (1u << n) - 1u ? width : width - 1;
    g.vec_pixels = unit ? vec_from / lane_pixels * lane_pixels : 0u;
    const size_t dense_row = static_cast<size_t>(width) * ob, dense_pitch = align_up(dense_row, 16);
    const size_t dense_bytes = dense_pitch * (rows - 1) + dense_row;
    g.plane_pitch = static_cast<uint32_t>(dense_pitch);
    uint32_t shifts[4] = {0, 0, 0, 0};
    float scales[4] = {1.f, 1.f, 1.f, 1.f}, offsets[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < n; ++c) {
        shifts[c] = (c & 1) ? shift / 2 : shift;  // (channels of one pixel with shifts of their own)
        g.shift[c] = static_cast<uint8_t>(shifts[c]);
        g.scale[c] = scales[c] = pairs[c].scale, g.offset[c] = offsets[c] = pairs[c].offset;
        if (!(given >> c & 1)) continue;
        if (posix_memalign(&p, 16, dense_bytes)) abort();
        g.plane[c] = static_cast<char*>(p);
        memset(g.plane[c], kCanary, dense_bytes);
    }
    const uint32_t mask = (1u << bits) - 1u;
    run(sb, n, ob, kind, g, mask);

    if (memcmp(src_before.data(), src, src_bytes)) ++wrong;  // (the source is read only)
    const uint32_t header[16] = {static_cast<uint32_t>(sb), static_cast<uint32_t>(n), static_cast<uint32_t>(ob), static_cast<uint32_t>(kind),
                                 static_cast<uint32_t>(bits), static_cast<uint32_t>(width), static_cast<uint32_t>(rows), unit, given,
                                 shifts[0], shifts[1], shifts[2], shifts[3], 0, 0, 0};
    fwrite(header, 4, 16, out);
    fwrite(scales, 4, 4, out);
    fwrite(offsets, 4, 4, out);
    const std::vector<unsigned char> zeros(row_bytes, 0);
    for (int row = 0; row < rows; ++row) {
        const size_t have = row + 1 < rows ? row_bytes : last_row;
        fwrite(src + lead + pitch * row, 1, have, out);
        fwrite(zeros.data(), 1, row_bytes - have, out);  // (samples behind the last given one are not part of the buffer)
    }
    for (int c = 0; c < n; ++c) {
        if (!g.plane[c]) continue;
        for (int row = 0; row < rows; ++row) {
            fwrite(g.plane[c] + dense_pitch * row, 1, dense_row, out);
            for (size_t k = dense_row; row + 1 < rows && k < dense_pitch; ++k)
                if (static_cast<unsigned char>(g.plane[c][dense_pitch * row + k]) != kCanary) {
                    if (!wrong) printf("SB %d N %d OB %d width %d unit %u: byte %zu behind row %d of plane %d was written\n", sb, n, ob, width, unit, k - dense_row, row, c);
                    ++wrong;
                }
        }
        free(g.plane[c]);
    }
    free(src);
    return wrong;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s OUTPUT\n", argv[0]);
        return 2;
    }
    FILE* out = fopen(argv[1], "wb");
    if (!out) return 2;
    long cases = 0, wrong = 0;
    const int forms[3][2] = {{4, 0}, {2, jinc::kSampleHalf}, {2, jinc::kSampleBFloat16}};  // (OB, KIND)
    // 1. geometry: every form, widths 1 .. 70, the access classes, channels missing
    for (int sb : {1, 2})
        for (int n = 1; n <= 4; ++n)
            for (const auto& form : forms) {
                const std::vector<int> depths = sb == 1 ? std::vector<int>{8} : std::vector<int>{10, 16};
                for (int bits : depths) {
                    const int shift = 8 * sb - bits;
                    Pair pairs[4];
                    pairs_of(bits, pairs);
                    for (int width = 1; width <= 70; ++width)
                        for (uint32_t unit : {16u, 4u, 0u}) {
                            std::vector<uint32_t> givens = {(1u << n) - 1u};
                            if (n >= 2) givens.push_back(1u);                    // the lowest channel alone
                            if (n >= 3) givens.push_back(1u | (1u << (n - 1)));  // ... and with the highest
                            for (uint32_t given : givens) {
                                wrong += one_case(out, sb, n, form[0], form[1], bits, shift, width, 2, unit, given, pairs, nullptr);
                                ++cases;
                            }
                        }
                }
            }
    // 2. values: every 16-bit value (and every 10-bit value at shift 6), one sample per pixel, whole lanes and a tail
    std::vector<uint16_t> all16(65536 + 5), all10(1024 + 5);
    for (size_t k = 0; k < all16.size(); ++k) all16[k] = static_cast<uint16_t>(k);
    for (size_t k = 0; k < all10.size(); ++k) all10[k] = static_cast<uint16_t>(k & 1023u);
    for (const auto& form : forms) {
        Pair p16[4], p10[4];
        pairs_of(16, p16), pairs_of(10, p10);
        const Pair chosen16[4] = {p16[2], p16[0], {2.f, -7.f}, {-1.f / 65535.f, 1.f}};  // full, limited luma, beyond 65504, downwards
        for (const Pair& pr : chosen16) {
            const Pair one[4] = {pr, pr, pr, pr};
            for (uint32_t unit : {16u, 0u}) {
                wrong += one_case(out, 2, 1, form[0], form[1], 16, 0, static_cast<int>(all16.size()), 1, unit, 1u, one, &all16);
                ++cases;
            }
        }
        for (int c = 0; c < 2; ++c) {
            const Pair one[4] = {p10[c], p10[c], p10[c], p10[c]};
            wrong += one_case(out, 2, 1, form[0], form[1], 10, 6, static_cast<int>(all10.size()), 1, 16u, 1u, one, &all10);
            ++cases;
        }
    }
    if (fclose(out)) return 2;
    printf("widen scaled rows: %ld cases, %ld wrong\n", cases, wrong);
    return wrong ? 1 : 0;
}
