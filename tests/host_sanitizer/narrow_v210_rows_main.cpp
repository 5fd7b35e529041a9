// Stand-alone driver of csrc/narrow_v210_rows.h (tests/test_narrowed_words_host.py), built once plain and once under
// AddressSanitizer + UndefinedBehaviorSanitizer: the row functions of narrow_v210_kernel run on the CPU lane by lane and trip by
// trip, exactly as the kernel calls them, with the cross-lane move modelled by indexing the partner's state, for the three kinds,
// scaled and not, every even width 2 .. 800, both access units and 1 .. 3 rows; and over long rows of chosen values: every tie
// k + 0.5 for k = 0 .. 1025, bounds, NaNs, infinities, zeros of either sign and negatives in fp32, and ALL 65536 patterns of the two
// 16-bit types.  Every buffer is allocated to EXACTLY the bytes the contract allows to be touched -- the blocks of `rows` rows of
// 16 * ceil(width / 6) bytes, a luma plane of width samples per row, chroma planes of width / 2 samples per row (rows start at a
// multiple of 8 bytes for fp32 and of 4 bytes for the 16-bit types, as the pair loads need) -- so one byte beyond any of them is a
// sanitizer report; every destination byte that is no block holds a canary, and the planes must come back unchanged.
// The expectations are NOT computed here: every case is written to the file named on the command line -- a header of 16 uint32
// (kind, scaled, width, rows, unit, lead, pitch, destination bytes, scale[3] and offset[3] as float bits, 2 x 0), the luma, Cb and
// Cr planes row by row without padding, then the whole destination buffer -- and the test compares with numpy.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "narrow_v210_rows.h"

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

// As in narrow_fields_rows_main.cpp.
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

// The kernel's walk over one row: a wave of 64 lanes, one block per lane and trip.
template <int KIND, bool Scaled>
void run_row(const jinc::NarrowV210Args& a, uint32_t row) {
    namespace v = jinc::v210;
    const uint32_t paired = v::paired_blocks(a), blocks = v::row_blocks(a);
    const v::RowOf r = v::row_of(a, 0, row);
    for (uint32_t trip = 0; trip < paired; trip += 64) {
        v::LaneState s[64];
        uint32_t y[64][3];
        for (uint32_t lane = 0; lane < 64; ++lane)
            if (trip + lane < paired) v::narrow_pair_begin<KIND, Scaled>(a, r, trip + lane, y[lane], s[lane]);
        for (uint32_t lane = 0; lane < 64; ++lane)
            if (trip + lane < paired) v::pack_pair_end(a, r, trip + lane, y[lane], s[lane], s[lane ^ 1].send);
    }
    for (uint32_t lane = 0; lane < 64; ++lane)
        for (uint32_t b = paired + lane; b < blocks; b += 64) v::narrow_tail<KIND, Scaled>(a, r, b);
}
template <int KIND>
void run_kind(const jinc::NarrowV210Args& a, bool scaled) {
    for (uint32_t row = 0; row < a.rows; ++row) {
        if (scaled) run_row<KIND, true>(a, row);
        else run_row<KIND, false>(a, row);
    }
}

// values: the samples of every plane's only row (luma from values[0] on, Cb from values[7], Cr from the middle: the two chroma rows
// together cover what the luma row covers), or nullptr for pseudo-random planes.
// Returns the number of planes that were written.
long one_case(FILE* out, int kind, bool scaled, int width, int rows, uint32_t unit, const std::vector<uint32_t>* values) {
    long wrong = 0;
    const size_t ib = kind == 0 ? 4 : 2;
    const size_t row_bytes = 16 * ((static_cast<size_t>(width) + 5) / 6);
    const size_t lead = unit == 16 ? 0 : 4, pitch = row_bytes + lead;
    const size_t dst_bytes = lead + pitch * (rows - 1) + row_bytes;
    void* p = nullptr;
    if (posix_memalign(&p, 16, dst_bytes)) abort();
    unsigned char* dst = static_cast<unsigned char*>(p);
    memset(dst, kCanary, dst_bytes);

    jinc::NarrowV210Args a;
    a.blocks = reinterpret_cast<char*>(dst) + lead;
    a.block_pitch = static_cast<uint32_t>(pitch);
    a.width = static_cast<uint32_t>(width), a.rows = static_cast<uint32_t>(rows), a.whole_blocks = static_cast<uint32_t>(width / 6), a.unit = unit;
    const float scales[3] = {0.5f, -1.f, 1.0009775f}, adds[3] = {100.25f, 1000.f, -0.5f};
    for (int c = 0; c < 3; ++c) a.value_scale[c] = scaled ? scales[c] : 1.f, a.value_offset[c] = scaled ? adds[c] : 0.f;
    const size_t pair_align = ib == 4 ? 8 : 4;
    const size_t samples[3] = {static_cast<size_t>(width), static_cast<size_t>(width / 2), static_cast<size_t>(width / 2)};
    size_t plane_pitch[3], plane_bytes[3];
    std::vector<unsigned char> before[3];
    for (int c = 0; c < 3; ++c) {
        plane_pitch[c] = align_up(samples[c] * ib, pair_align);
        plane_bytes[c] = plane_pitch[c] * (rows - 1) + samples[c] * ib;
        if (posix_memalign(&p, 16, plane_bytes[c] ? plane_bytes[c] : 1)) abort();
        unsigned char* plane = static_cast<unsigned char*>(p);
        memset(plane, kCanary, plane_bytes[c]);
        for (int row = 0; row < rows; ++row)
            for (size_t x = 0; x < samples[c]; ++x) {
                const uint32_t s = values ? (*values)[(x + (c == 2 ? values->size() / 2 : 7u * c)) % values->size()] : random_sample(kind);
                memcpy(plane + plane_pitch[c] * row + x * ib, &s, ib);  // (little-endian: the low bytes of a 16-bit pattern)
            }
        before[c].assign(plane, plane + plane_bytes[c]);
        a.plane[c] = reinterpret_cast<char*>(plane);
    }
    a.luma_pitch = static_cast<uint32_t>(plane_pitch[0]), a.chroma_pitch = static_cast<uint32_t>(plane_pitch[1]);
    if (kind == 0) run_kind<0>(a, scaled);
    else if (kind == jinc::kSampleHalf) run_kind<jinc::kSampleHalf>(a, scaled);
    else run_kind<jinc::kSampleBFloat16>(a, scaled);

    const uint32_t header[16] = {static_cast<uint32_t>(kind), scaled ? 1u : 0u, a.width, a.rows, unit, static_cast<uint32_t>(lead),
                                 static_cast<uint32_t>(pitch), static_cast<uint32_t>(dst_bytes),
                                 bits_of(a.value_scale[0]), bits_of(a.value_scale[1]), bits_of(a.value_scale[2]),
                                 bits_of(a.value_offset[0]), bits_of(a.value_offset[1]), bits_of(a.value_offset[2]), 0, 0};
    fwrite(header, 4, 16, out);
    for (int c = 0; c < 3; ++c) {
        if (memcmp(before[c].data(), a.plane[c], plane_bytes[c])) ++wrong;  // (the planes are read only)
        for (int row = 0; row < rows; ++row) fwrite(a.plane[c] + plane_pitch[c] * row, 1, samples[c] * ib, out);
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
    // 1. geometry
    for (int width = 2; width <= 800; width += 2)
        for (int kind : kinds)
            for (bool scaled : {false, true})
                for (uint32_t unit : {16u, 4u})
                    for (int rows = 1; rows <= 3; ++rows) {
                        wrong += one_case(out, kind, scaled, width, rows, unit, nullptr);
                        ++cases;
                    }
    // 2. values: pairs of blocks, an odd whole block and a partial one
    std::vector<uint32_t> f32;
    for (int k = -3; k <= 1025; ++k) f32.push_back(bits_of(static_cast<float>(k) + 0.5f));  // every tie
    for (int k = -2; k <= 1026; k += (k == 3 ? 1017 : 1)) f32.push_back(bits_of(static_cast<float>(k)));  // both bounds
    for (float v : {0.49999997f, 0.50000006f, 1e-45f, -1e-45f, 3e38f, -3e38f, 1e9f, 16777216.f, 8388608.5f})
        f32.push_back(bits_of(v)), f32.push_back(bits_of(1023.f - v)), f32.push_back(bits_of(1023.f + v));
    for (uint32_t b : {0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, 0xffffffffu, 0x80000000u, 0u}) f32.push_back(b);
    f32.resize(f32.size() / 12 * 12 + 12 + 6 + 4, bits_of(0.5f));  // (... an odd whole block and a partial one of four pixels)
    std::vector<uint32_t> all16(65536 + 10);                       // 10 924 whole blocks and a partial one of two pixels
    for (uint32_t k = 0; k < all16.size(); ++k) all16[k] = k & 0xffffu;
    for (bool scaled : {false, true})
        for (uint32_t unit : {16u, 4u}) {
            wrong += one_case(out, 0, scaled, static_cast<int>(f32.size()), 1, unit, &f32);
            wrong += one_case(out, jinc::kSampleHalf, scaled, static_cast<int>(all16.size()), 1, unit, &all16);
            wrong += one_case(out, jinc::kSampleBFloat16, scaled, static_cast<int>(all16.size()), 1, unit, &all16);
            cases += 3;
        }
    if (fclose(out)) return 2;
    printf("narrow v210 rows: %ld cases, %ld wrong\n", cases, wrong);
    return wrong ? 1 : 0;
}
