// Stand-alone driver of csrc/v210_rows.h under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_v210_rows_host.py): the
// row functions of the v210 kernels run on the CPU lane by lane and trip by trip, exactly as unpack_v210_kernel / pack_v210_kernel
// call them, with the cross-lane move modelled by indexing the partner's state.  Every buffer is allocated to EXACTLY the bytes the
// contract allows to be touched -- the blocks of `rows` rows at pitch = 16 * ceil(width / 6), a luma plane of 2 * width bytes per
// row, chroma planes of width bytes per row -- so one byte beyond any of them is a sanitizer report.  (A chroma row of width bytes
// is 2 mod 4 long when width is; the planes' pitch must be a multiple of 4, so such rows are followed by 2 bytes of a canary
// that is checked, except the last row, which ends the allocation.)
// The expectations come from a scalar decoder / encoder written here from the format's table, independent of the header's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "v210_rows.h"

namespace {

uint32_t g_state = 0x2545F491u;
uint32_t rnd() {  // xorshift32
    g_state ^= g_state << 13, g_state ^= g_state >> 17, g_state ^= g_state << 5;
    return g_state;
}

// (word, bit offset) of the block's fields, from the table of the format
const int kY[6][2] = {{0, 10}, {1, 0}, {1, 20}, {2, 10}, {3, 0}, {3, 20}};
const int kCb[3][2] = {{0, 0}, {1, 10}, {2, 20}};
const int kCr[3][2] = {{0, 20}, {2, 0}, {3, 10}};

uint32_t field(const uint32_t* row_words, int block, const int where[2]) { return (row_words[4 * block + where[0]] >> where[1]) & 1023u; }
void set_field(uint32_t* row_words, int block, const int where[2], uint32_t v) { row_words[4 * block + where[0]] |= (v & 1023u) << where[1]; }

struct Buffers {
    int width, rows;
    size_t row_bytes, luma_pitch, chroma_pitch, luma_bytes, chroma_bytes;
    char *blocks, *y, *u, *v;
    Buffers(int w, int r) : width(w), rows(r) {
        row_bytes = 16 * ((static_cast<size_t>(w) + 5) / 6);
        luma_pitch = 2 * static_cast<size_t>(w);
        chroma_pitch = (static_cast<size_t>(w) + 3) / 4 * 4;
        luma_bytes = luma_pitch * r;
        chroma_bytes = chroma_pitch * (r - 1) + w;
        void* p[4];
        const size_t bytes[4] = {row_bytes * r, luma_bytes, chroma_bytes, chroma_bytes};
        for (int i = 0; i < 4; ++i)
            if (posix_memalign(&p[i], 16, bytes[i])) abort();
        blocks = static_cast<char*>(p[0]), y = static_cast<char*>(p[1]), u = static_cast<char*>(p[2]), v = static_cast<char*>(p[3]);
    }
    ~Buffers() { free(blocks), free(y), free(u), free(v); }
    jinc::V210Args args(uint32_t unit) const {
        jinc::V210Args a;
        a.blocks = blocks, a.plane[0] = y, a.plane[1] = u, a.plane[2] = v;
        a.block_pitch = static_cast<uint32_t>(row_bytes), a.luma_pitch = static_cast<uint32_t>(luma_pitch), a.chroma_pitch = static_cast<uint32_t>(chroma_pitch);
        a.width = static_cast<uint32_t>(width), a.rows = static_cast<uint32_t>(rows), a.whole_blocks = static_cast<uint32_t>(width / 6), a.unit = unit;
        return a;
    }
    uint32_t* words(int row) const { return reinterpret_cast<uint32_t*>(blocks + row * row_bytes); }
    uint16_t* luma(int row) const { return reinterpret_cast<uint16_t*>(y + row * luma_pitch); }
    uint16_t* cb(int row) const { return reinterpret_cast<uint16_t*>(u + row * chroma_pitch); }
    uint16_t* cr(int row) const { return reinterpret_cast<uint16_t*>(v + row * chroma_pitch); }
};

// The kernels' walk over one row: a wave of 64 lanes, one block per lane and trip.
template <bool Pack>
void run_row(const jinc::V210Args& a, uint32_t row) {
    namespace v = jinc::v210;
    const uint32_t paired = v::paired_blocks(a), blocks = v::row_blocks(a);
    const v::RowOf r = v::row_of(a, 0, row);
    for (uint32_t trip = 0; trip < paired; trip += 64) {
        v::LaneState s[64];
        uint32_t y[64][3];
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t b = trip + lane;
            if (b >= paired) continue;
            if (Pack) v::pack_pair_begin(a, r, b, y[lane], s[lane]);
            else v::unpack_pair_begin(a, r, b, s[lane]);
        }
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t b = trip + lane;
            if (b >= paired) continue;
            if (Pack) v::pack_pair_end(a, r, b, y[lane], s[lane], s[lane ^ 1].send);
            else v::unpack_pair_end(a, r, b, s[lane], s[lane ^ 1].send);
        }
    }
    for (uint32_t lane = 0; lane < 64; ++lane)
        for (uint32_t b = paired + lane; b < blocks; b += 64) {
            if (Pack) v::pack_tail(a, r, b);
            else v::unpack_tail(a, r, b);
        }
}

constexpr unsigned char kCanary = 0xA5;

long check_chroma_pads(const Buffers& B, const char* what) {
    long wrong = 0;
    for (int row = 0; row + 1 < B.rows; ++row)
        for (size_t k = B.width; k < B.chroma_pitch; ++k)
            for (const char* p : {B.u, B.v})
                if (static_cast<unsigned char>(p[row * B.chroma_pitch + k]) != kCanary) {
                    if (!wrong) printf("%s: width %d rows %d: byte %zu behind chroma row %d was written\n", what, B.width, B.rows, k - B.width, row);
                    ++wrong;
                }
    return wrong;
}

long one_case(int width, int rows, uint32_t unit) {
    long wrong = 0;
    Buffers B(width, rows);
    const jinc::V210Args a = B.args(unit);
    const int blocks = static_cast<int>(B.row_bytes / 16);

    // ---- unpack: pseudo-random words (bits 30 - 31 and the unused fields of a partial block included) against the scalar decoder
    for (size_t k = 0; k < B.row_bytes * rows / 4; ++k) reinterpret_cast<uint32_t*>(B.blocks)[k] = rnd();
    memset(B.y, kCanary, B.luma_bytes), memset(B.u, kCanary, B.chroma_bytes), memset(B.v, kCanary, B.chroma_bytes);
    std::vector<char> blocks_before(B.blocks, B.blocks + B.row_bytes * rows);
    for (int row = 0; row < rows; ++row) run_row<false>(a, static_cast<uint32_t>(row));
    for (int row = 0; row < rows; ++row) {
        for (int x = 0; x < width; ++x)
            if (B.luma(row)[x] != field(B.words(row), x / 6, kY[x % 6])) ++wrong;
        for (int x = 0; x < width / 2; ++x) {
            if (B.cb(row)[x] != field(B.words(row), x / 3, kCb[x % 3])) ++wrong;
            if (B.cr(row)[x] != field(B.words(row), x / 3, kCr[x % 3])) ++wrong;
        }
    }
    wrong += check_chroma_pads(B, "unpack");
    if (memcmp(blocks_before.data(), B.blocks, blocks_before.size())) ++wrong;  // (the source is read only)
    if (wrong) printf("unpack: width %d rows %d unit %u: %ld wrong\n", width, rows, unit, wrong);

    // ---- pack: those planes into blocks that start as pseudo-random bytes, against the scalar encoder (zeros wherever no sample goes)
    long wrong_pack = 0;
    std::vector<uint32_t> want(B.row_bytes * rows / 4, 0u);
    for (int row = 0; row < rows; ++row) {
        uint32_t* w = want.data() + row * (B.row_bytes / 4);
        for (int x = 0; x < width; ++x) set_field(w, x / 6, kY[x % 6], B.luma(row)[x]);
        for (int x = 0; x < width / 2; ++x) set_field(w, x / 3, kCb[x % 3], B.cb(row)[x]), set_field(w, x / 3, kCr[x % 3], B.cr(row)[x]);
    }
    for (size_t k = 0; k < B.row_bytes * rows / 4; ++k) reinterpret_cast<uint32_t*>(B.blocks)[k] = rnd();
    for (int row = 0; row < rows; ++row) run_row<true>(a, static_cast<uint32_t>(row));
    for (int row = 0; row < rows; ++row)
        for (int k = 0; k < 4 * blocks; ++k) {
            const uint32_t got = B.words(row)[k], exp = want[row * (B.row_bytes / 4) + k];
            if (got != exp || (got >> 30)) {
                if (!wrong_pack) printf("pack: width %d rows %d unit %u: row %d word %d is %08x, expected %08x\n", width, rows, unit, row, k, got, exp);
                ++wrong_pack;
            }
        }
    wrong_pack += check_chroma_pads(B, "pack");
    return wrong + wrong_pack;
}

}  // namespace

int main() {
    long cases = 0, wrong = 0;
    for (int width = 2; width <= 800; width += 2)
        for (int rows = 1; rows <= 3; ++rows)
            for (uint32_t unit : {16u, 4u}) {
                wrong += one_case(width, rows, unit);
                cases += 2;  // both directions
            }
    printf("v210 rows: %ld cases, %ld wrong\n", cases, wrong);
    return wrong ? 1 : 0;
}
