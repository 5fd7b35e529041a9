// Stand-alone driver of the SCALED forms of csrc/widen_v210_rows.h (tests/test_widened_words_scaled_host.py), built once plain and
// once under AddressSanitizer + UndefinedBehaviorSanitizer: the row functions of widen_v210_kernel<OB, KIND, true> run on the CPU
// lane by lane and trip by trip, exactly as the kernel calls them, with the cross-lane move modelled by indexing the partner's
// state, for the three plane types (fp32, binary16, bfloat16), both access classes of the block side, every even width 2 .. 100 and
// 782 (a second trip of the paired loop), 1 .. 3 rows and three sets of three DIFFERENT pairs (Y, Cb, Cr), each with a negative
// scale -- a swap of plane 1's and plane 2's pair in the even / odd lane shows.  Every buffer is allocated to EXACTLY the bytes the
// contract allows to be touched -- the blocks of `rows` rows of 16 * ceil(width / 6) bytes, a luma plane of width samples per row,
// chroma planes of width / 2 samples per row -- so one byte beyond any of them is a sanitizer report.  (The pair stores need rows
// that start at a multiple of 8 bytes (fp32) or 4 bytes (16-bit types); rows that are not that long are followed by a canary.)  The
// blocks are pseudo-random in every bit and must come back unchanged.
// The expectations are NOT computed here: every case is written to the file named on the command line -- a header of 16 uint32
// (kind, width, rows, unit, the bits of scale[3], the bits of offset[3], the pitches of the luma and the chroma planes in bytes,
// 4 x 0), the blocks row by row, then the luma, Cb and Cr planes row by row WITH their padding (the last row without) -- and the test
// compares samples and padding with numpy.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "widen_v210_rows.h"

namespace {

uint32_t g_state = 0x9E3779B9u;
uint32_t rnd() {  // xorshift32
    g_state ^= g_state << 13, g_state ^= g_state >> 17, g_state ^= g_state << 5;
    return g_state;
}

constexpr unsigned char kCanary = 0xA5;
// (scale, offset) of Y, Cb, Cr: as in widen_fields_scaled_rows_main.cpp.
const float kPairs[3][3][2] = {{{1.0f / 876.0f, -64.0f / 876.0f}, {1.0f / 896.0f, -512.0f / 896.0f}, {-1.0f / 1023.0f, 1.0f}},
                               {{-0.00390625f, 3.5f}, {1.0f / 1023.0f, -512.0f / 1023.0f}, {1.0f / 3.0f, 0.1f}},
                               {{70.0f, -5.0f}, {1e-7f, 0.0f}, {-64.5f, 0.25f}}};

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
uint32_t bits_of(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return b;
}

// The kernel's walk over one row: a wave of 64 lanes, one block per lane and trip.
template <int OB, int KIND>
void run_row(const jinc::WidenV210Args& a, uint32_t row) {
    namespace v = jinc::v210;
    const uint32_t paired = v::paired_blocks(a), blocks = v::row_blocks(a);
    const v::RowOf r = v::row_of(a, 0, row);
    for (uint32_t trip = 0; trip < paired; trip += 64) {
        v::LaneState s[64];
        for (uint32_t lane = 0; lane < 64; ++lane)
            if (trip + lane < paired) v::widen_pair_begin<OB, KIND, true>(a, r, trip + lane, s[lane]);
        for (uint32_t lane = 0; lane < 64; ++lane)
            if (trip + lane < paired) v::widen_pair_end<OB, KIND, true>(a, r, trip + lane, s[lane], s[lane ^ 1].send);
    }
    for (uint32_t lane = 0; lane < 64; ++lane)
        for (uint32_t b = paired + lane; b < blocks; b += 64) v::widen_tail<OB, KIND, true>(a, r, b);
}

// kind: 0 fp32, jinc::kSampleHalf, jinc::kSampleBFloat16.  Returns 1 when the blocks were written.
long one_case(FILE* out, int kind, int width, int rows, uint32_t unit, const float pairs[3][2]) {
    long wrong = 0;
    const int ob = kind == 0 ? 4 : 2;
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

    jinc::WidenV210Args a;
    a.blocks = reinterpret_cast<char*>(blocks) + lead;
    a.block_pitch = static_cast<uint32_t>(block_pitch);
    a.width = static_cast<uint32_t>(width), a.rows = static_cast<uint32_t>(rows), a.whole_blocks = static_cast<uint32_t>(width / 6), a.unit = unit;
    for (int c = 0; c < 3; ++c) {
        pitch[c] = align_up(row_of_plane[c], pair_align);
        bytes[c] = pitch[c] * (rows - 1) + row_of_plane[c];
        if (posix_memalign(&p, 16, bytes[c] ? bytes[c] : 1)) abort();
        a.plane[c] = static_cast<char*>(p);
        memset(a.plane[c], kCanary, bytes[c]);
        a.value_scale[c] = pairs[c][0], a.value_offset[c] = pairs[c][1];
    }
    a.luma_pitch = static_cast<uint32_t>(pitch[0]), a.chroma_pitch = static_cast<uint32_t>(pitch[1]);
    for (int row = 0; row < rows; ++row) {
        if (kind == 0) run_row<4, 0>(a, static_cast<uint32_t>(row));
        else if (kind == jinc::kSampleHalf) run_row<2, jinc::kSampleHalf>(a, static_cast<uint32_t>(row));
        else run_row<2, jinc::kSampleBFloat16>(a, static_cast<uint32_t>(row));
    }

    if (memcmp(blocks_before.data(), blocks, block_bytes)) ++wrong;  // (the blocks are read only)
    const uint32_t header[16] = {static_cast<uint32_t>(kind), static_cast<uint32_t>(width), static_cast<uint32_t>(rows), unit, bits_of(pairs[0][0]),
                                 bits_of(pairs[1][0]), bits_of(pairs[2][0]), bits_of(pairs[0][1]), bits_of(pairs[1][1]), bits_of(pairs[2][1]),
                                 static_cast<uint32_t>(pitch[0]), static_cast<uint32_t>(pitch[1]), 0, 0, 0, 0};
    fwrite(header, 4, 16, out);
    for (int row = 0; row < rows; ++row) fwrite(blocks + lead + block_pitch * row, 1, row_bytes, out);
    for (int c = 0; c < 3; ++c) {
        fwrite(a.plane[c], 1, bytes[c], out);
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
    for (int kind : {0, jinc::kSampleHalf, jinc::kSampleBFloat16})
        for (uint32_t unit : {16u, 4u})
            for (int rows = 1; rows <= 3; ++rows)
                for (int width = 2; width <= 102; width += 2) {
                    wrong += one_case(out, kind, width == 102 ? 782 : width, rows, unit, kPairs[cases % 3]);
                    ++cases;
                }
    if (fclose(out)) return 2;
    printf("widen v210 scaled rows: %ld cases, %ld wrong\n", cases, wrong);
    return wrong ? 1 : 0;
}
