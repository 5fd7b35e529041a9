// Stand-alone driver of csrc/widen_v210_rows.h (tests/test_widened_words_host.py), built once plain and once under
// AddressSanitizer + UndefinedBehaviorSanitizer: the row functions of widen_v210_kernel run on the CPU lane by lane and trip by
// trip, exactly as the kernel calls them, with the cross-lane move modelled by indexing the partner's state.  Every buffer is
// allocated to EXACTLY the bytes the contract allows to be touched -- the blocks of `rows` rows of 16 * ceil(width / 6) bytes, a
// luma plane of width samples per row, chroma planes of width / 2 samples per row -- so one byte beyond any of them is a sanitizer
// report.  (The pair stores need rows that start at a multiple of 8 bytes (fp32) or 4 bytes (binary16); a chroma row of width / 2
// samples is not always that long, so such rows are followed by a canary that is checked, except the last row, which ends the
// allocation.)  The blocks are pseudo-random in every bit -- bits 30 - 31 and the fields of a partial last block beyond `width`
// included -- and must come back unchanged.
// The expectations are NOT computed here: every case is written to the file named on the command line -- a header of 16 uint32
// (OB, width, rows, unit, 12 x 0), the blocks row by row, then the luma, Cb and Cr planes row by row without padding -- and the
// test compares with numpy.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "widen_v210_rows.h"

namespace {

uint32_t g_state = 0x2545F491u;
uint32_t rnd() {  // xorshift32
    g_state ^= g_state << 13, g_state ^= g_state >> 17, g_state ^= g_state << 5;
    return g_state;
}

constexpr unsigned char kCanary = 0xA5;

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The kernel's walk over one row: a wave of 64 lanes, one block per lane and trip.
template <int OB>
void run_row(const jinc::V210Args& a, uint32_t row) {
    namespace v = jinc::v210;
    const uint32_t paired = v::paired_blocks(a), blocks = v::row_blocks(a);
    const v::RowOf r = v::row_of(a, 0, row);
    for (uint32_t trip = 0; trip < paired; trip += 64) {
        v::LaneState s[64];
        for (uint32_t lane = 0; lane < 64; ++lane)
            if (trip + lane < paired) v::widen_pair_begin<OB>(a, r, trip + lane, s[lane]);
        for (uint32_t lane = 0; lane < 64; ++lane)
            if (trip + lane < paired) v::widen_pair_end<OB>(a, r, trip + lane, s[lane], s[lane ^ 1].send);
    }
    for (uint32_t lane = 0; lane < 64; ++lane)
        for (uint32_t b = paired + lane; b < blocks; b += 64) v::widen_tail<OB>(a, r, b);
}

// Returns the number of wrong bytes outside the samples.
long one_case(FILE* out, int ob, int width, int rows, uint32_t unit) {
    long wrong = 0;
    const size_t row_bytes = 16 * ((static_cast<size_t>(width) + 5) / 6);
    const size_t lead = unit == 16 ? 0 : 4, block_pitch = row_bytes + lead;
    const size_t block_bytes = lead + block_pitch * (rows - 1) + row_bytes;
    const size_t pair_align = ob == 4 ? 8 : 4;
    const size_t row_of_plane[3] = {static_cast<size_t>(width) * ob, static_cast<size_t>(width / 2) * ob, static_cast<size_t>(width / 2) * ob};
    size_t pitch[3], bytes[3];
    void* p = nullptr;
    if (posix_memalign(&p, 16, block_bytes)) abort();
    unsigned char* blocks = static_cast<unsigned char*>(p);
    for (size_t k = 0; k < block_bytes; ++k) blocks[k] = static_cast<unsigned char>(rnd());
    const std::vector<unsigned char> blocks_before(blocks, blocks + block_bytes);

    jinc::V210Args a;
    a.blocks = reinterpret_cast<char*>(blocks) + lead;
    a.block_pitch = static_cast<uint32_t>(block_pitch);
    a.width = static_cast<uint32_t>(width), a.rows = static_cast<uint32_t>(rows), a.whole_blocks = static_cast<uint32_t>(width / 6), a.unit = unit;
    for (int c = 0; c < 3; ++c) {
        pitch[c] = align_up(row_of_plane[c], pair_align);
        bytes[c] = pitch[c] * (rows - 1) + row_of_plane[c];
        if (posix_memalign(&p, 16, bytes[c] ? bytes[c] : 1)) abort();
        a.plane[c] = static_cast<char*>(p);
        memset(a.plane[c], kCanary, bytes[c]);
    }
    a.luma_pitch = static_cast<uint32_t>(pitch[0]), a.chroma_pitch = static_cast<uint32_t>(pitch[1]);
    for (int row = 0; row < rows; ++row) {
        if (ob == 4) run_row<4>(a, static_cast<uint32_t>(row));
        else run_row<2>(a, static_cast<uint32_t>(row));
    }

    if (memcmp(blocks_before.data(), blocks, block_bytes)) ++wrong;  // (the blocks are read only)
    const uint32_t header[16] = {static_cast<uint32_t>(ob), static_cast<uint32_t>(width), static_cast<uint32_t>(rows), unit, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    fwrite(header, 4, 16, out);
    for (int row = 0; row < rows; ++row) fwrite(blocks + lead + block_pitch * row, 1, row_bytes, out);
    for (int c = 0; c < 3; ++c) {
        for (int row = 0; row < rows; ++row) {
            fwrite(a.plane[c] + pitch[c] * row, 1, row_of_plane[c], out);
            for (size_t k = row_of_plane[c]; row + 1 < rows && k < pitch[c]; ++k)
                if (static_cast<unsigned char>(a.plane[c][pitch[c] * row + k]) != kCanary) {
                    if (!wrong) printf("OB %d width %d rows %d unit %u: byte %zu behind row %d of plane %d was written\n", ob, width, rows, unit, k - row_of_plane[c], row, c);
                    ++wrong;
                }
        }
        free(a.plane[c]);
    }
    free(blocks);
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
    for (int width = 2; width <= 800; width += 2)
        for (int ob : {4, 2})
            for (uint32_t unit : {16u, 4u})
                for (int rows = 1; rows <= 3; ++rows) {
                    wrong += one_case(out, ob, width, rows, unit);
                    ++cases;
                }
    if (fclose(out)) return 2;
    printf("widen v210 rows: %ld cases, %ld wrong\n", cases, wrong);
    return wrong ? 1 : 0;
}
