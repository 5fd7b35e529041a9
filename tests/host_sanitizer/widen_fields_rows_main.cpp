// Stand-alone driver of csrc/widen_fields_rows.h (tests/test_widened_words_host.py), built once plain and once under
// AddressSanitizer + UndefinedBehaviorSanitizer: the row function of widen_fields_kernel runs on the CPU lane by lane, exactly as
// the kernel calls it, for both plane types, both access classes of the word side (16-byte, dword), three words (Y410,
// BGRX1010102 and a word with spare bits at 10 and 21) and the widths below.  Every buffer is allocated to EXACTLY the bytes the
// contract allows to be touched: the words end behind the last word of the last row, a dense plane behind the last sample of its
// last row, so one byte beyond either is a sanitizer report; the planes' row padding holds a canary that is checked, and the words
// -- pseudo-random in every bit, the bits outside the fields included -- must come back unchanged.
// The expectations are NOT computed here: every case is written to the file named on the command line -- a header of 16 uint32
// (OB, width, rows, unit, offset[3], 9 x 0), the words row by row without padding, then the three dense planes row by row without
// padding -- and the test compares with numpy.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "widen_fields_rows.h"

namespace {

uint32_t g_state = 0x2545F491u;
uint32_t rnd() {  // xorshift32
    g_state ^= g_state << 13, g_state ^= g_state >> 17, g_state ^= g_state << 5;
    return g_state;
}

constexpr unsigned char kCanary = 0xA5;
const int kWidths[] = {1, 7, 8, 9, 63, 64, 65, 513, 1031};
const uint32_t kOffsets[3][3] = {{10, 0, 20}, {12, 22, 2}, {22, 0, 11}};

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

template <int OB>
void run_rows(const jinc::FieldArgs& a) {
    for (uint32_t row = 0; row < a.rows; ++row)
        for (uint32_t lane = 0; lane < 64; ++lane) jinc::widen::widen_fields_row<OB>(a, 0, row, lane);
}

// Returns the number of wrong bytes outside the samples.
long one_case(FILE* out, int ob, int width, int rows, uint32_t unit, const uint32_t offsets[3]) {
    long wrong = 0;
    const size_t row_bytes = static_cast<size_t>(width) * 4;
    const size_t lead = unit == 16 ? 0 : 4;
    const size_t pitch = align_up(row_bytes, 16) + (unit == 16 ? 0 : 4);
    const size_t src_bytes = lead + pitch * (rows - 1) + row_bytes;
    void* p = nullptr;
    if (posix_memalign(&p, 16, src_bytes)) abort();
    unsigned char* src = static_cast<unsigned char*>(p);
    for (size_t k = 0; k < src_bytes; ++k) src[k] = static_cast<unsigned char>(rnd());  // (every bit outside the fields included)
    const std::vector<unsigned char> src_before(src, src + src_bytes);

    jinc::FieldArgs a;
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
        if (posix_memalign(&p, 16, dense_bytes)) abort();
        a.plane[c] = static_cast<char*>(p);
        memset(a.plane[c], kCanary, dense_bytes);
    }
    if (ob == 4) run_rows<4>(a);
    else run_rows<2>(a);

    if (memcmp(src_before.data(), src, src_bytes)) ++wrong;  // (the words are read only)
    const uint32_t header[16] = {static_cast<uint32_t>(ob), static_cast<uint32_t>(width), static_cast<uint32_t>(rows), unit, offsets[0], offsets[1],
                                 offsets[2], 0, 0, 0, 0, 0, 0, 0, 0, 0};
    fwrite(header, 4, 16, out);
    for (int row = 0; row < rows; ++row) fwrite(src + lead + pitch * row, 1, row_bytes, out);
    for (int c = 0; c < 3; ++c) {
        for (int row = 0; row < rows; ++row) {
            fwrite(a.plane[c] + dense_pitch * row, 1, dense_row, out);
            for (size_t k = dense_row; row + 1 < rows && k < dense_pitch; ++k)
                if (static_cast<unsigned char>(a.plane[c][dense_pitch * row + k]) != kCanary) {
                    if (!wrong) printf("OB %d width %d unit %u: byte %zu behind row %d of plane %d was written\n", ob, width, unit, k - dense_row, row, c);
                    ++wrong;
                }
        }
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
    for (int ob : {4, 2})
        for (uint32_t unit : {16u, 4u})
            for (const auto& offsets : kOffsets)
                for (int width : kWidths) {
                    wrong += one_case(out, ob, width, 3, unit, offsets);
                    ++cases;
                }
    if (fclose(out)) return 2;
    printf("widen fields rows: %ld cases, %ld wrong\n", cases, wrong);
    return wrong ? 1 : 0;
}
