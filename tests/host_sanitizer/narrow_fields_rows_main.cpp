// Stand-alone driver of csrc/narrow_fields_rows.h (tests/test_narrowed_words_host.py), built once plain and once under
// AddressSanitizer + UndefinedBehaviorSanitizer: the row function of narrow_fields_kernel runs on the CPU lane by lane, exactly as the
// kernel calls it, for the three kinds, scaled and not, widths 1 .. 70 and 1031 (two whole trips of 64 lanes x 8 pixels and a
// tail), both access units, 1 .. 3 rows and two layouts (Y410 with a fill that has bits inside and outside the fields, and the legal
// odd word [22, 0, 11]); and over long rows of chosen values: every tie k + 0.5 for k = 0 .. 1025, bounds, NaNs, infinities, zeros
// of either sign and negatives in fp32, and ALL 65536 patterns of the two 16-bit types.  Every buffer is allocated to EXACTLY the
// bytes the contract allows to be touched: a dense plane ends behind the last sample of its last row, the destination behind the
// last word of its last row, so one byte beyond either is a sanitizer report; every destination byte that is no word holds a canary,
// and the planes must come back unchanged.
// The expectations are NOT computed here: every case is written to the file named on the command line -- a header of 24 uint32
// (kind, scaled, width, rows, unit, offsets[3], fill as given to the row function, lead, pitch, destination bytes, scale[3] and
// offset[3] as float bits, 6 x 0), the three dense planes row by row without padding, then the whole destination buffer -- and the
// test compares with numpy.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "narrow_fields_rows.h"

namespace {

uint32_t g_state = 0x2545F491u;
uint32_t rnd() {  // xorshift32
    g_state ^= g_state << 13, g_state ^= g_state >> 17, g_state ^= g_state << 5;
    return g_state;
}

constexpr unsigned char kCanary = 0xA5;

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

uint32_t bits_of(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return b;
}

// A pseudo-random sample of `kind` around 0 .. 1023: quarters (ties among them) from below 0 to above the peak in fp32, patterns
// whose exponents span that range in the 16-bit types, and now and then an infinity, a NaN or a zero of either sign.
uint32_t random_sample(int kind) {
    const uint32_t r = rnd();
    if (r % 29u == 0u) {
        static const uint32_t special32[6] = {0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00001u, 0x80000000u, 0u};
        const uint32_t s = special32[(r >> 8) % 6u];
        return kind == 0 ? s : kind == jinc::kSampleHalf ? ((s >> 16) & 0x8000u) | ((s & 0x7f800000u) ? 0x7c00u : 0u) | ((s & 0x7fffffu) ? 0x200u : 0u)
                                                         : s >> 16;
    }
    if (kind == 0) return bits_of(static_cast<float>(static_cast<int>((r >> 4) % 4960u) - 400) * 0.25f);
    const uint32_t sign = (r >> 5) % 7u == 0u ? 1u : 0u;
    if (kind == jinc::kSampleHalf) return (sign << 15) | ((9u + (r >> 8) % 19u) << 10) | ((r >> 16) & 1023u);  // exponents -6 .. 12
    return (sign << 15) | ((121u + (r >> 8) % 19u) << 7) | ((r >> 16) & 127u);
}

template <int KIND, bool Scaled>
void run_rows(const jinc::NarrowFieldArgs& a) {
    for (uint32_t row = 0; row < a.rows; ++row)
        for (uint32_t lane = 0; lane < 64; ++lane) jinc::narrow::narrow_fields_row<KIND, Scaled>(a, 0, row, lane);
}
template <int KIND>
void run_kind(const jinc::NarrowFieldArgs& a, bool scaled) {
    if (scaled) run_rows<KIND, true>(a);
    else run_rows<KIND, false>(a);
}

// values: the samples of every plane's only row (plane c starts at values[c * 7 mod size]), or nullptr for pseudo-random planes.
// Returns the number of planes that were written.
long one_case(FILE* out, int kind, bool scaled, int width, int rows, uint32_t unit, const int offsets[3], uint32_t fill,
              const std::vector<uint32_t>* values) {
    long wrong = 0;
    const size_t ib = kind == 0 ? 4 : 2;
    const size_t row_bytes = static_cast<size_t>(width) * 4;
    const size_t lead = unit == 16 ? 0 : 4, pitch = unit == 16 ? align_up(row_bytes, 16) : align_up(row_bytes, 16) + 4;
    const size_t dst_bytes = lead + pitch * (rows - 1) + row_bytes;
    void* p = nullptr;
    if (posix_memalign(&p, 16, dst_bytes)) abort();
    unsigned char* dst = static_cast<unsigned char*>(p);
    memset(dst, kCanary, dst_bytes);

    jinc::NarrowFieldArgs a;
    a.packed = reinterpret_cast<char*>(dst) + lead;
    a.packed_pitch = static_cast<uint32_t>(pitch);
    a.width = static_cast<uint32_t>(width), a.rows = static_cast<uint32_t>(rows), a.unit = unit;
    a.vec_pixels = a.width / 8u * 8u;
    uint32_t mask = 0;
    for (int c = 0; c < 3; ++c) a.offset[c] = static_cast<uint32_t>(offsets[c]), mask |= 1023u << offsets[c];
    a.fill = fill & ~mask;
    const float scales[3] = {0.5f, -1.f, 1.0009775f}, adds[3] = {100.25f, 1000.f, -0.5f};
    for (int c = 0; c < 3; ++c) a.value_scale[c] = scaled ? scales[c] : 1.f, a.value_offset[c] = scaled ? adds[c] : 0.f;
    const size_t dense_row = static_cast<size_t>(width) * ib, dense_pitch = align_up(dense_row, 16);
    const size_t dense_bytes = dense_pitch * (rows - 1) + dense_row;
    a.plane_pitch = static_cast<uint32_t>(dense_pitch);
    std::vector<unsigned char> before[3];
    for (int c = 0; c < 3; ++c) {
        if (posix_memalign(&p, 16, dense_bytes)) abort();
        unsigned char* plane = static_cast<unsigned char*>(p);
        memset(plane, kCanary, dense_bytes);
        for (int row = 0; row < rows; ++row)
            for (int x = 0; x < width; ++x) {
                const uint32_t s = values ? (*values)[(static_cast<size_t>(x) + 7u * c) % values->size()] : random_sample(kind);
                memcpy(plane + dense_pitch * row + x * ib, &s, ib);  // (little-endian: the low bytes of a 16-bit pattern)
            }
        before[c].assign(plane, plane + dense_bytes);
        a.plane[c] = reinterpret_cast<char*>(plane);
    }
    if (kind == 0) run_kind<0>(a, scaled);
    else if (kind == jinc::kSampleHalf) run_kind<jinc::kSampleHalf>(a, scaled);
    else run_kind<jinc::kSampleBFloat16>(a, scaled);

    const uint32_t header[24] = {static_cast<uint32_t>(kind), scaled ? 1u : 0u, a.width, a.rows, unit, a.offset[0], a.offset[1], a.offset[2], a.fill,
                                 static_cast<uint32_t>(lead), static_cast<uint32_t>(pitch), static_cast<uint32_t>(dst_bytes),
                                 bits_of(a.value_scale[0]), bits_of(a.value_scale[1]), bits_of(a.value_scale[2]),
                                 bits_of(a.value_offset[0]), bits_of(a.value_offset[1]), bits_of(a.value_offset[2]), 0, 0, 0, 0, 0, 0};
    fwrite(header, 4, 24, out);
    for (int c = 0; c < 3; ++c) {
        if (memcmp(before[c].data(), a.plane[c], dense_bytes)) ++wrong;  // (the planes are read only)
        for (int row = 0; row < rows; ++row) fwrite(a.plane[c] + dense_pitch * row, 1, dense_row, out);
        free(a.plane[c]);
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
    const int y410[3] = {10, 0, 20}, odd[3] = {22, 0, 11};
    // 1. geometry
    for (int kind : kinds)
        for (bool scaled : {false, true})
            for (uint32_t unit : {16u, 4u})
                for (int rows = 1; rows <= 3; ++rows)
                    for (int i = 1; i <= 71; ++i) {
                        const int width = i <= 70 ? i : 1031;
                        wrong += one_case(out, kind, scaled, width, rows, unit, y410, 0xC5A5A5A5u, nullptr);
                        wrong += one_case(out, kind, scaled, width, rows, unit, odd, 0xFFFFFFFFu, nullptr);
                        cases += 2;
                    }
    // 2. values: whole lanes and a tail
    std::vector<uint32_t> f32;
    for (int k = -3; k <= 1025; ++k) f32.push_back(bits_of(static_cast<float>(k) + 0.5f));  // every tie
    for (int k = -2; k <= 1026; k += (k == 3 ? 1017 : 1)) f32.push_back(bits_of(static_cast<float>(k)));  // both bounds
    for (float v : {0.49999997f, 0.50000006f, 1e-45f, -1e-45f, 3e38f, -3e38f, 1e9f, 16777216.f, 8388608.5f})
        f32.push_back(bits_of(v)), f32.push_back(bits_of(1023.f - v)), f32.push_back(bits_of(1023.f + v));
    for (uint32_t b : {0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, 0xffffffffu, 0x80000000u, 0u}) f32.push_back(b);
    f32.resize(f32.size() / 8 * 8 + 13, bits_of(0.5f));  // (... and a tail that is no whole lane)
    std::vector<uint32_t> all16(65536 + 5);
    for (uint32_t k = 0; k < all16.size(); ++k) all16[k] = k & 0xffffu;
    for (bool scaled : {false, true})
        for (uint32_t unit : {16u, 4u}) {
            wrong += one_case(out, 0, scaled, static_cast<int>(f32.size()), 1, unit, y410, 0xC0000000u, &f32);
            wrong += one_case(out, jinc::kSampleHalf, scaled, static_cast<int>(all16.size()), 1, unit, y410, 0xC0000000u, &all16);
            wrong += one_case(out, jinc::kSampleBFloat16, scaled, static_cast<int>(all16.size()), 1, unit, odd, 0u, &all16);
            cases += 3;
        }
    if (fclose(out)) return 2;
    printf("narrow fields rows: %ld cases, %ld wrong\n", cases, wrong);
    return wrong ? 1 : 0;
}
