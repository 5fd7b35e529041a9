// Stand-alone driver of the SCALED form of csrc/narrow_rows.h (tests/test_scaled_host.py), built once plain and once under
// AddressSanitizer + UndefinedBehaviorSanitizer: narrow_row<KIND, N, DB, true> runs on the CPU lane by lane, exactly as the kernel
// calls it, for every form KIND x N x DB, shift 0 and the largest shift of the depth, widths 1 .. 70, the three access classes
// (16-byte, dword, sample sized), groups with every channel given or with channels missing, and a scale / offset pair of its own
// for every channel: the limited-range luma and chroma pairs of the depth (219 k / 16 k, 224 k / 128 k), the full-range pair and an
// odd negative one.  The planes hold values from 0.15 below 0 to 0.15 above 1, so both clamps are hit, and now and then an
// infinity, a NaN or a zero of either sign.  And, with one sample per pixel, long rows: pseudo-random fp32 values and specials, and
// ALL 65536 patterns of the two 16-bit types, at the limited-range luma pair and the full-range pair of every depth.
// Every buffer is allocated to EXACTLY the bytes the contract allows to be touched, as in narrow_rows_main.cpp; every destination
// byte that is no given sample holds a canary, and the planes must come back unchanged.
// The expectations are NOT computed here: every case is written to the file named on the command line -- a header of 16 uint32
// (kind, N, DB, bits, width, rows, unit, given-channel mask, shift[4], lead, pitch, destination bytes, 0), scale[4] and offset[4] as
// fp32, the dense plane of every given channel row by row without padding, then the whole destination buffer -- and the test
// compares with numpy.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "narrow_rows.h"

namespace {

uint32_t g_state = 0x2545F491u;
uint32_t rnd() {  // xorshift32
    g_state ^= g_state << 13, g_state ^= g_state >> 17, g_state ^= g_state << 5;
    return g_state;
}

constexpr unsigned char kCanary = 0xA5;

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

template <int KIND, int N, int DB>
void run_rows(const jinc::NarrowGroup& g, float peak) {
    for (uint32_t row = 0; row < g.rows; ++row)
        for (uint32_t lane = 0; lane < 64; ++lane) jinc::narrow::narrow_row<KIND, N, DB, true>(g, peak, 0, row, lane);
}

template <int KIND, int DB>
void run_by_step(int n, const jinc::NarrowGroup& g, float peak) {
    switch (n) {
        case 1: return run_rows<KIND, 1, DB>(g, peak);
        case 2: return run_rows<KIND, 2, DB>(g, peak);
        case 3: return run_rows<KIND, 3, DB>(g, peak);
        case 4: return run_rows<KIND, 4, DB>(g, peak);
    }
    abort();
}

template <int KIND>
void run_by_size(int n, int db, const jinc::NarrowGroup& g, float peak) {
    if (db == 1) run_by_step<KIND, 1>(n, g, peak);
    else run_by_step<KIND, 2>(n, g, peak);
}

void run(int kind, int n, int db, const jinc::NarrowGroup& g, float peak) {
    if (kind == 0) run_by_size<0>(n, db, g, peak);
    else if (kind == jinc::kSampleHalf) run_by_size<jinc::kSampleHalf>(n, db, g, peak);
    else run_by_size<jinc::kSampleBFloat16>(n, db, g, peak);
}

struct Pair {
    float scale, offset;
};

// The pairs of a depth: limited-range luma, limited-range chroma, full range, and one no range table holds.
void pairs_of(int bits, Pair out[4]) {
    const float k = static_cast<float>(1 << (bits - 8)), peak = static_cast<float>((1 << bits) - 1);
    out[0] = {219.f * k, 16.f * k};
    out[1] = {224.f * k, 128.f * k};
    out[2] = {peak, 0.f};
    out[3] = {-0.37f * peak, 0.8125f * peak};
}

uint32_t bits_of(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return b;
}

// A pseudo-random sample of `kind` around 0 .. 1: multiples of 2^-13 from 0.15 below 0 to 0.15 above 1 in fp32, patterns whose
// exponents span 2^-10 .. 2 in the 16-bit types, and now and then an infinity, a NaN or a zero of either sign.
uint32_t random_sample(int kind) {
    const uint32_t r = rnd();
    if (r % 29u == 0u) {
        static const uint32_t special32[6] = {0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00001u, 0x80000000u, 0u};
        const uint32_t s = special32[(r >> 8) % 6u];
        return kind == 0 ? s : kind == jinc::kSampleHalf ? ((s >> 16) & 0x8000u) | ((s & 0x7f800000u) ? 0x7c00u : 0u) | ((s & 0x7fffffu) ? 0x200u : 0u)
                                                         : s >> 16;
    }
    if (kind == 0) return bits_of(static_cast<float>(static_cast<int>((r >> 4) % 10650u) - 1229) * (1.f / 8192.f));
    const uint32_t sign = (r >> 5) % 7u == 0u ? 1u : 0u;
    if (kind == jinc::kSampleHalf) return (sign << 15) | ((5u + (r >> 8) % 11u) << 10) | ((r >> 16) & 1023u);
    return (sign << 15) | ((117u + (r >> 8) % 11u) << 7) | ((r >> 16) & 127u);
}

// given: bit c = channel c has a plane (bit 0 always).  values: the samples of channel 0's only row (rows 1, n 1), or nullptr for
// pseudo-random planes.  Returns the number of planes that were written.
long one_case(FILE* out, int kind, int n, int db, int bits, int shift, int width, int rows, uint32_t unit, uint32_t given,
              const Pair pairs[4], const std::vector<uint32_t>* values) {
    long wrong = 0;
    const size_t ib = kind == 0 ? 4 : 2;
    int last_given = 0;
    for (int c = 0; c < n; ++c)
        if (given >> c & 1) last_given = c;
    // destination: base offset and pitch of the access class; the allocation ends behind the last given sample
    const size_t row_bytes = static_cast<size_t>(width) * n * db;
    const size_t lead = unit == 16 ? 0 : unit == 4 ? 4 : db;
    const size_t pitch = unit == 16 ? align_up(row_bytes, 16) : unit == 4 ? align_up(row_bytes, 16) + 4 : align_up(row_bytes, 4) + (db == 1 ? 1 : 2);
    const size_t last_row = (static_cast<size_t>(width - 1) * n + last_given + 1) * db;
    const size_t dst_bytes = lead + pitch * (rows - 1) + last_row;
    void* p = nullptr;
    if (posix_memalign(&p, 16, dst_bytes)) abort();
    unsigned char* dst = static_cast<unsigned char*>(p);
    memset(dst, kCanary, dst_bytes);

    jinc::NarrowGroup g;
    g.packed = reinterpret_cast<char*>(dst) + lead;
    g.packed_pitch = static_cast<uint32_t>(pitch);
    g.width = static_cast<uint32_t>(width), g.rows = static_cast<uint32_t>(rows);
    g.unit = unit;
    const uint32_t lane_pixels = 16u / db;
    g.vec_pixels = (unit && given == (1u << n) - 1u) ? width / lane_pixels * lane_pixels : 0u;
    const size_t dense_row = static_cast<size_t>(width) * ib, dense_pitch = align_up(dense_row, 16);
    const size_t dense_bytes = dense_pitch * (rows - 1) + dense_row;
    g.plane_pitch = static_cast<uint32_t>(dense_pitch);
    uint32_t shifts[4] = {0, 0, 0, 0};
    float scales[4] = {1.f, 1.f, 1.f, 1.f}, offsets[4] = {0.f, 0.f, 0.f, 0.f};
    std::vector<unsigned char> before[4];
    for (int c = 0; c < n; ++c) {
        shifts[c] = (c & 1) ? shift / 2 : shift;  // (channels of one pixel with shifts of their own)
        g.shift[c] = static_cast<uint8_t>(shifts[c]);
        g.scale[c] = scales[c] = pairs[c].scale, g.offset[c] = offsets[c] = pairs[c].offset;
        if (!(given >> c & 1)) continue;
        if (posix_memalign(&p, 16, dense_bytes)) abort();
        unsigned char* plane = static_cast<unsigned char*>(p);
        memset(plane, kCanary, dense_bytes);
        for (int row = 0; row < rows; ++row)
            for (int x = 0; x < width; ++x) {
                const uint32_t s = values ? (*values)[x] : random_sample(kind);
                memcpy(plane + dense_pitch * row + x * ib, &s, ib);  // (little-endian: the low bytes of a 16-bit pattern)
            }
        before[c].assign(plane, plane + dense_bytes);
        g.plane[c] = reinterpret_cast<const char*>(plane);
    }
    run(kind, n, db, g, static_cast<float>((1u << bits) - 1u));

    const uint32_t header[16] = {static_cast<uint32_t>(kind), static_cast<uint32_t>(n), static_cast<uint32_t>(db), static_cast<uint32_t>(bits),
                                 static_cast<uint32_t>(width), static_cast<uint32_t>(rows), unit, given, shifts[0], shifts[1], shifts[2], shifts[3],
                                 static_cast<uint32_t>(lead), static_cast<uint32_t>(pitch), static_cast<uint32_t>(dst_bytes), 0};
    fwrite(header, 4, 16, out);
    fwrite(scales, 4, 4, out);
    fwrite(offsets, 4, 4, out);
    for (int c = 0; c < n; ++c) {
        if (!g.plane[c]) continue;
        if (memcmp(before[c].data(), g.plane[c], dense_bytes)) ++wrong;  // (the planes are read only)
        for (int row = 0; row < rows; ++row) fwrite(g.plane[c] + dense_pitch * row, 1, dense_row, out);
        free(const_cast<char*>(g.plane[c]));
    }
    fwrite(dst, 1, dst_bytes, out);
    free(dst);
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
    const int kinds[3] = {0, jinc::kSampleHalf, jinc::kSampleBFloat16};
    // 1. geometry: every form, widths 1 .. 70, the access classes, channels missing
    for (int kind : kinds)
        for (int n = 1; n <= 4; ++n)
            for (int db : {1, 2}) {
                const int bits = db == 1 ? 8 : 10;
                Pair pairs[4];
                pairs_of(bits, pairs);
                for (int shift : {0, 8 * db - bits}) {
                    for (int width = 1; width <= 70; ++width)
                        for (uint32_t unit : {16u, 4u, 0u}) {
                            std::vector<uint32_t> givens = {(1u << n) - 1u};
                            if (n >= 2) givens.push_back(1u);                    // the lowest channel alone
                            if (n >= 3) givens.push_back(1u | (1u << (n - 1)));  // ... and with the highest
                            for (uint32_t given : givens) {
                                wrong += one_case(out, kind, n, db, bits, shift, width, 2, unit, given, pairs, nullptr);
                                ++cases;
                            }
                        }
                    if (db == 1) break;  // (a byte has one shift: 0)
                }
            }
    // 2. values: one sample per pixel, whole lanes and a tail, every depth at its largest shift
    std::vector<uint32_t> f32;
    for (int k = 0; k < 40000; ++k) f32.push_back(random_sample(0));
    for (float v : {0.f, 1.f, 0.5f, -0.0730593607f, 1.0867579909f, 1e-45f, -1e-45f, 3e38f, -3e38f, 1e9f})
        f32.push_back(bits_of(v)), f32.push_back(bits_of(-v));
    for (uint32_t b : {0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, 0xffffffffu, 0x80000000u, 0u}) f32.push_back(b);
    f32.resize(f32.size() + 5, bits_of(0.5f));  // (... and a tail that is no whole lane)
    std::vector<uint32_t> all16(65536 + 5);
    for (uint32_t k = 0; k < all16.size(); ++k) all16[k] = k & 0xffffu;
    for (int bits : {8, 10, 12, 16}) {
        const int db = bits > 8 ? 2 : 1, shift = 8 * db - bits;
        Pair pairs[4];
        pairs_of(bits, pairs);
        for (int which : {0, 2}) {
            const Pair one[4] = {pairs[which], pairs[which], pairs[which], pairs[which]};
            for (uint32_t unit : {16u, 0u}) {
                wrong += one_case(out, 0, 1, db, bits, shift, static_cast<int>(f32.size()), 1, unit, 1u, one, &f32);
                wrong += one_case(out, jinc::kSampleHalf, 1, db, bits, shift, static_cast<int>(all16.size()), 1, unit, 1u, one, &all16);
                wrong += one_case(out, jinc::kSampleBFloat16, 1, db, bits, shift, static_cast<int>(all16.size()), 1, unit, 1u, one, &all16);
                cases += 3;
            }
        }
    }
    if (fclose(out)) return 2;
    printf("narrow scaled rows: %ld cases, %ld wrong\n", cases, wrong);
    return wrong ? 1 : 0;
}
