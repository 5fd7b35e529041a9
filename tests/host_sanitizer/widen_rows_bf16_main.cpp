// Stand-alone driver of the bfloat16 form of csrc/widen_rows.h (tests/test_bfloat16_widened.py), built once plain and once under
// AddressSanitizer + UndefinedBehaviorSanitizer: widen_row<1, N, 2, kSampleBFloat16> -- bytes into bfloat16 planes, the one source
// size that is exact in that type -- runs on the CPU lane by lane, exactly as widen_samples_kernel calls it, for N = 1 .. 4, the
// widths below, the three access classes (16-byte, dword, sample sized) and groups with every channel given or with channels
// missing.  As in widen_rows_main.cpp every buffer is allocated to EXACTLY the bytes the contract allows to be touched: the source
// ends behind the last GIVEN sample of its last row, a dense plane behind the last sample of its last row, so one byte beyond either
// is a sanitizer report; row padding holds a canary that is checked, and the source must come back unchanged.
// The expectations are NOT computed here: every case is written to the file named on the command line -- a header of 16 uint32
// (SB, N, OB, bits, width, rows, unit, given-channel mask, 8 x 0), the source bytes row by row without padding, then the dense plane
// of every given channel row by row without padding -- and the test compares with numpy.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "widen_rows.h"

namespace {

uint32_t g_state = 0x9E3779B9u;
uint32_t rnd() {  // xorshift32
    g_state ^= g_state << 13, g_state ^= g_state >> 17, g_state ^= g_state << 5;
    return g_state;
}

constexpr unsigned char kCanary = 0xA5;
const int kWidths[] = {1, 7, 15, 16, 17, 63, 64, 65, 1031};

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

template <int N>
void run_rows(const jinc::WidenGroup& g) {
    for (uint32_t row = 0; row < g.rows; ++row)
        for (uint32_t lane = 0; lane < 64; ++lane) jinc::widen::widen_row<1, N, 2, jinc::kSampleBFloat16>(g, 0xffu, 0, row, lane);
}

void run(int n, const jinc::WidenGroup& g) {
    switch (n) {
        case 1: return run_rows<1>(g);
        case 2: return run_rows<2>(g);
        case 3: return run_rows<3>(g);
        case 4: return run_rows<4>(g);
    }
    abort();
}

// given: bit c = channel c has a plane (bit 0 always).  Returns the number of wrong bytes outside the samples.
long one_case(FILE* out, int n, int width, int rows, uint32_t unit, uint32_t given) {
    long wrong = 0;
    int last_given = 0;
    for (int c = 0; c < n; ++c)
        if (given >> c & 1) last_given = c;
    const size_t row_bytes = static_cast<size_t>(width) * n;
    const size_t lead = unit == 16 ? 0 : unit == 4 ? 4 : 1;
    const size_t pitch = unit == 16 ? align_up(row_bytes, 16) : unit == 4 ? align_up(row_bytes, 16) + 4 : align_up(row_bytes, 4) + 1;
    const size_t last_row = static_cast<size_t>(width - 1) * n + last_given + 1;
    const size_t src_bytes = lead + pitch * (rows - 1) + last_row;
    void* p = nullptr;
    if (posix_memalign(&p, 16, src_bytes)) abort();
    unsigned char* src = static_cast<unsigned char*>(p);
    for (size_t k = 0; k < src_bytes; ++k) src[k] = static_cast<unsigned char>(rnd());
    const std::vector<unsigned char> src_before(src, src + src_bytes);

    jinc::WidenGroup g;
    g.packed = reinterpret_cast<const char*>(src) + lead;
    g.packed_pitch = static_cast<uint32_t>(pitch);
    g.width = static_cast<uint32_t>(width), g.rows = static_cast<uint32_t>(rows);
    g.unit = unit;
    const uint32_t vec_from = given == (1u << n) - 1u ? width : width - 1;
    g.vec_pixels = unit ? vec_from / 16u * 16u : 0u;
    const size_t dense_row = static_cast<size_t>(width) * 2, dense_pitch = align_up(dense_row, 16);
    const size_t dense_bytes = dense_pitch * (rows - 1) + dense_row;
    g.plane_pitch = static_cast<uint32_t>(dense_pitch);
    for (int c = 0; c < n; ++c) {
        g.shift[c] = 0;  // (a byte is its value)
        if (!(given >> c & 1)) continue;
        if (posix_memalign(&p, 16, dense_bytes)) abort();
        g.plane[c] = static_cast<char*>(p);
        memset(g.plane[c], kCanary, dense_bytes);
    }
    run(n, g);

    if (memcmp(src_before.data(), src, src_bytes)) ++wrong;  // (the source is read only)
    const uint32_t header[16] = {1u, static_cast<uint32_t>(n), 2u, 8u, static_cast<uint32_t>(width), static_cast<uint32_t>(rows), unit, given,
                                 0, 0, 0, 0, 0, 0, 0, 0};
    fwrite(header, 4, 16, out);
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
                    if (!wrong) printf("N %d width %d unit %u: byte %zu behind row %d of plane %d was written\n", n, width, unit, k - dense_row, row, c);
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
    for (int n = 1; n <= 4; ++n)
        for (int width : kWidths)
            for (uint32_t unit : {16u, 4u, 0u}) {
                std::vector<uint32_t> givens = {(1u << n) - 1u};
                if (n >= 2) givens.push_back(1u);                    // the lowest channel alone
                if (n >= 3) givens.push_back(1u | (1u << (n - 1)));  // ... and with the highest
                for (uint32_t given : givens) {
                    wrong += one_case(out, n, width, 2, unit, given);
                    ++cases;
                }
            }
    if (fclose(out)) return 2;
    printf("widen rows bfloat16: %ld cases, %ld wrong\n", cases, wrong);
    return wrong ? 1 : 0;
}
