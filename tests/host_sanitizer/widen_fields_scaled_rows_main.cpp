// Stand-alone driver of the SCALED forms of csrc/widen_fields_rows.h (tests/test_widened_words_scaled_host.py), built once plain
// and once under AddressSanitizer + UndefinedBehaviorSanitizer: the row function of widen_fields_kernel<OB, KIND, true> runs on the
// CPU lane by lane, exactly as the kernel calls it, for the three plane types (fp32, binary16, bfloat16), both access classes of
// the word side (16-byte, dword), widths 1 .. 70 and 1030 (a second trip of the wave), 1 .. 3 rows and three sets of three
// DIFFERENT pairs, each with a negative scale; one set overflows binary16 and reaches its subnormals.  Every buffer is allocated to
// EXACTLY the bytes the contract allows to be touched: the words end behind the last word of the last row, a dense plane behind the
// last sample of its last row, so one byte beyond either is a sanitizer report; the planes' row padding holds a canary, and the
// words -- pseudo-random in every bit -- must come back unchanged.
// The expectations are NOT computed here: every case is written to the file named on the command line -- a header of 16 uint32
// (kind, width, rows, unit, offset[3], the bits of scale[3], the bits of offset[3], the planes' pitch in bytes, 2 x 0), the words row
// by row without padding, then the three dense planes row by row WITH their padding (the last row without) -- and the test
// compares samples and padding with numpy.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "widen_fields_rows.h"

namespace {

uint32_t g_state = 0x9E3779B9u;
uint32_t rnd() {  // xorshift32
    g_state ^= g_state << 13, g_state ^= g_state >> 17, g_state ^= g_state << 5;
    return g_state;
}

constexpr unsigned char kCanary = 0xA5;
const uint32_t kOffsets[3][3] = {{10, 0, 20}, {12, 22, 2}, {22, 0, 11}};
// (scale, offset) per plane: limited-range 10-bit luma and chroma and a negative scale; a negative power of two, full-range chroma
// and a third; past binary16's largest value, into its subnormals, and a negative scale with a tie-prone offset.
const float kPairs[3][3][2] = {{{1.0f / 876.0f, -64.0f / 876.0f}, {1.0f / 896.0f, -512.0f / 896.0f}, {-1.0f / 1023.0f, 1.0f}},
                               {{-0.00390625f, 3.5f}, {1.0f / 1023.0f, -512.0f / 1023.0f}, {1.0f / 3.0f, 0.1f}},
                               {{70.0f, -5.0f}, {1e-7f, 0.0f}, {-64.5f, 0.25f}}};

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
uint32_t bits_of(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return b;
}

template <int OB, int KIND>
void run_rows(const jinc::WidenFieldArgs& a) {
    for (uint32_t row = 0; row < a.rows; ++row)
        for (uint32_t lane = 0; lane < 64; ++lane) jinc::widen::widen_fields_row<OB, KIND, true>(a, 0, row, lane);
}

// kind: 0 fp32, jinc::kSampleHalf, jinc::kSampleBFloat16.  Returns 1 when the words were written.
long one_case(FILE* out, int kind, int width, int rows, uint32_t unit, const uint32_t offsets[3], const float pairs[3][2]) {
    long wrong = 0;
    const int ob = kind == 0 ? 4 : 2;
    const size_t row_bytes = static_cast<size_t>(width) * 4;
    const size_t lead = unit == 16 ? 0 : 4;
    const size_t pitch = align_up(row_bytes, 16) + (unit == 16 ? 0 : 4);
    const size_t src_bytes = lead + pitch * (rows - 1) + row_bytes;
    void* p = nullptr;
    if (posix_memalign(&p, 16, src_bytes)) abort();
    unsigned char* src = static_cast<unsigned char*>(p);
    for (size_t k = 0; k < src_bytes; ++k) src[k] = static_cast<unsigned char>(rnd());  // (every bit outside the fields included)
    const std::vector<unsigned char> src_before(src, src + src_bytes);

    jinc::WidenFieldArgs a;
    a.packed = reinterpret_cast<char*>(src) + lead;
    a.packed_pitch = static_cast<uint32_t>(pitch);
    a.width = static_cast<uint32_t>(width), a.rows = static_cast<uint32_t>(rows);
    a.unit = unit;
    a.vec_pixels = a.width / 8 * 8;
    a.fill = 0xFFFFFFFFu;  // (not read)
    const size_t dense_row = static_cast<size_t>(width) * ob, dense_pitch = align_up(dense_row, 16);
    const size_t dense_bytes = dense_pitch * (rows - 1) + dense_row;
    a.plane_pitch = static_cast<uint32_t>(dense_pitch);
    for (int c = 0; c < 3; ++c) {
        a.offset[c] = offsets[c];
        a.value_scale[c] = pairs[c][0], a.value_offset[c] = pairs[c][1];
        if (posix_memalign(&p, 16, dense_bytes)) abort();
        a.plane[c] = static_cast<char*>(p);
        memset(a.plane[c], kCanary, dense_bytes);
    }
    if (kind == 0) run_rows<4, 0>(a);
    else if (kind == jinc::kSampleHalf) run_rows<2, jinc::kSampleHalf>(a);
    else run_rows<2, jinc::kSampleBFloat16>(a);

    if (memcmp(src_before.data(), src, src_bytes)) ++wrong;  // (the words are read only)
    const uint32_t header[16] = {static_cast<uint32_t>(kind), static_cast<uint32_t>(width), static_cast<uint32_t>(rows), unit, offsets[0], offsets[1],
                                 offsets[2], bits_of(pairs[0][0]), bits_of(pairs[1][0]), bits_of(pairs[2][0]), bits_of(pairs[0][1]),
                                 bits_of(pairs[1][1]), bits_of(pairs[2][1]), static_cast<uint32_t>(dense_pitch), 0, 0};
    fwrite(header, 4, 16, out);
    for (int row = 0; row < rows; ++row) fwrite(src + lead + pitch * row, 1, row_bytes, out);
    for (int c = 0; c < 3; ++c) {
        fwrite(a.plane[c], 1, dense_bytes, out);
        free(a.plane[c]);
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
    for (int kind : {0, jinc::kSampleHalf, jinc::kSampleBFloat16})
        for (uint32_t unit : {16u, 4u})
            for (int width = 1; width <= 71; ++width) {
                const int w = width == 71 ? 1030 : width;
                wrong += one_case(out, kind, w, 1 + w % 3, unit, kOffsets[cases % 3], kPairs[(cases / 3) % 3]);
                ++cases;
            }
    if (fclose(out)) return 2;
    printf("widen fields scaled rows: %ld cases, %ld wrong\n", cases, wrong);
    return wrong ? 1 : 0;
}
