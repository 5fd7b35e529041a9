// Stand-alone driver of csrc/widen_rows.h (tests/test_widened_host.py), built once plain and once under AddressSanitizer +
// UndefinedBehaviorSanitizer: the row function of widen_samples_kernel runs on the CPU lane by lane, exactly as the kernel calls it,
// for every form SB x N x OB, shifts 0 / 4 / 6 on 16-bit words, the widths below, the three access classes (16-byte, dword, sample
// sized) and groups with every channel given or with channels missing.  Every buffer is allocated to EXACTLY the bytes the contract
// allows to be touched: the source ends behind the last GIVEN sample of its last row, a dense plane behind the last sample of its
// last row, so one byte beyond either is a sanitizer report; row padding and the bytes in front of an offset base hold a canary
// that is checked, and the source must come back unchanged.
// The expectations are NOT computed here: every case is written to the file named on the command line -- a header of 16 uint32
// (SB, N, OB, bits, width, rows, unit, given-channel mask, shift[4], 4 x 0), the source samples row by row without padding, then
// the dense plane of every given channel row by row without padding -- and the test compares with numpy.
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
const int kWidths[] = {1, 7, 8, 9, 63, 64, 65, 1031};

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

template <int SB, int N, int OB>
void run_rows(const jinc::WidenGroup& g, uint32_t mask) {
    for (uint32_t row = 0; row < g.rows; ++row)
        for (uint32_t lane = 0; lane < 64; ++lane) jinc::widen::widen_row<SB, N, OB>(g, mask, 0, row, lane);
}

template <int SB, int OB>
void run_by_step(int n, const jinc::WidenGroup& g, uint32_t mask) {
    switch (n) {
        case 1: return run_rows<SB, 1, OB>(g, mask);
        case 2: return run_rows<SB, 2, OB>(g, mask);
        case 3: return run_rows<SB, 3, OB>(g, mask);
        case 4: return run_rows<SB, 4, OB>(g, mask);
    }
    abort();
}

void run(int sb, int n, int ob, const jinc::WidenGroup& g, uint32_t mask) {
    if (sb == 1 && ob == 4) run_by_step<1, 4>(n, g, mask);
    else if (sb == 1 && ob == 2) run_by_step<1, 2>(n, g, mask);
    else if (sb == 2 && ob == 4) run_by_step<2, 4>(n, g, mask);
    else run_by_step<2, 2>(n, g, mask);
}

// given: bit c = channel c has a plane (bit 0 always).  Returns the number of wrong bytes outside the samples.
long one_case(FILE* out, int sb, int n, int ob, int bits, int shift, int width, int rows, uint32_t unit, uint32_t given) {
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
    for (int c = 0; c < n; ++c) {
        shifts[c] = (c & 1) ? shift / 2 : shift;  // (channels of one pixel with shifts of their own)
        g.shift[c] = static_cast<uint8_t>(shifts[c]);
        if (!(given >> c & 1)) continue;
        if (posix_memalign(&p, 16, dense_bytes)) abort();
        g.plane[c] = static_cast<char*>(p);
        memset(g.plane[c], kCanary, dense_bytes);
    }
    const uint32_t mask = (1u << bits) - 1u;
    run(sb, n, ob, g, mask);

    if (memcmp(src_before.data(), src, src_bytes)) ++wrong;  // (the source is read only)
    const uint32_t header[16] = {static_cast<uint32_t>(sb), static_cast<uint32_t>(n), static_cast<uint32_t>(ob), static_cast<uint32_t>(bits),
                                 static_cast<uint32_t>(width), static_cast<uint32_t>(rows), unit, given, shifts[0], shifts[1], shifts[2], shifts[3],
                                 0, 0, 0, 0};
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
    for (int sb : {1, 2})
        for (int n = 1; n <= 4; ++n)
            for (int ob : {4, 2})
                for (int shift : {0, 4, 6}) {
                    if (sb == 1 && shift) continue;  // (a byte is its value)
                    // 8 bits in a byte; 10 bits in a word at every shift, and with fp32 planes all 16 bits at shift 0
                    std::vector<int> widths_of_bits = {sb == 1 ? 8 : 10};
                    if (sb == 2 && ob == 4 && shift == 0) widths_of_bits.push_back(16);
                    for (int bits : widths_of_bits)
                        for (int width : kWidths)
                            for (uint32_t unit : {16u, 4u, 0u}) {
                                std::vector<uint32_t> givens = {(1u << n) - 1u};
                                if (n >= 2) givens.push_back(1u);                              // the lowest channel alone
                                if (n >= 3) givens.push_back(1u | (1u << (n - 1)));            // ... and with the highest
                                for (uint32_t given : givens) {
                                    wrong += one_case(out, sb, n, ob, bits, shift, width, 2, unit, given);
                                    ++cases;
                                }
                            }
                }
    if (fclose(out)) return 2;
    printf("widen rows: %ld cases, %ld wrong\n", cases, wrong);
    return wrong ? 1 : 0;
}
