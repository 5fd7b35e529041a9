// Stand-alone driver of csrc/matrix_rows.h (tests/test_colour_matrix_host.py), built once plain and once under AddressSanitizer +
// UndefinedBehaviorSanitizer: the row function of output_matrix_kernel runs on the CPU lane by lane, exactly as the kernel calls it,
// for the three sample kinds, widths 1, 3, 4, 7, 8, 9, 255, 256, 257, 260 and 517 (tail only, one vector step, the 64-lane trip
// boundary of both sample sizes, a second trip), the three access classes (16-byte, dword, sample sized), two frames of three rows.
// Every plane is allocated to EXACTLY the bytes the contract allows to be touched -- it ends behind the last sample of the last row
// of the last frame, so one byte beyond is a sanitizer report -- and every byte that is no sample (the lead in front of the base,
// the padding of every row) holds a canary.  Finite samples only.
// The expectations are NOT computed here: every case is written to the file named on the command line -- a header of 32 words
// (uint32 kind, width, rows, frames, unit, lead, bytes[3], pitch[3], frame stride[3], 0; float m[9], offset[3]; 4 x 0), the three
// planes' whole buffers as they were, then the three as the row function left them -- and the test compares with numpy.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "matrix_rows.h"

namespace {

uint32_t g_state = 0x2545F491u;
uint32_t rnd() {  // xorshift32
    g_state ^= g_state << 13, g_state ^= g_state >> 17, g_state ^= g_state << 5;
    return g_state;
}

constexpr unsigned char kCanary = 0xA5;

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// A finite sample of `kind`: mostly values in -1.5 .. 1.5 (what normalised Y'CbCr and a little overshoot hold), now and then one
// 2^-18 times that (results in the subnormals of binary16), a larger one, or a zero of either sign.
uint32_t random_sample(int kind) {
    const uint32_t r = rnd();
    float v = (static_cast<float>(r >> 8) * (1.f / 16777216.f) - 0.5f) * 3.f;
    if (r % 13u == 0u) v *= 3.814697265625e-6f;
    if (r % 17u == 0u) v *= 1000.f;
    if (r % 31u == 0u) v = (r & 32u) ? -0.f : 0.f;
    if (kind == 0) return jinc::widen::float_bits(v);
    return kind == jinc::kSampleHalf ? jinc::widen::host_half_rne(v) : jinc::widen::host_bf16_rne(v);
}

template <int KIND>
void run_rows(const jinc::MatrixArgs& a, uint32_t frames) {
    for (uint32_t frame = 0; frame < frames; ++frame)
        for (uint32_t row = 0; row < a.rows; ++row)
            for (uint32_t lane = 0; lane < 64; ++lane) jinc::matrix::matrix_row<KIND>(a, frame, row, lane);
}

void one_case(FILE* out, int kind, int width, uint32_t unit) {
    const uint32_t rows = 3, frames = 2;
    const size_t sb = kind == 0 ? 4 : 2, row_bytes = static_cast<size_t>(width) * sb;
    // base offset, pitch and frame stride of the access class (every plane with a pitch of its own)
    const size_t lead = unit == 16 ? 16 : unit == 4 ? 4 : sb;
    jinc::MatrixArgs a;
    unsigned char* buf[3];
    size_t bytes[3];
    for (int c = 0; c < 3; ++c) {
        const size_t pitch = unit == 16 ? align_up(row_bytes, 16) + 16 * c : unit == 4 ? align_up(row_bytes, 16) + 4 + 8 * c : align_up(row_bytes, 4) + sb + 4 * c;
        const size_t fs = pitch * rows + (unit == 16 ? 32 : unit == 4 ? 20 : 3 * sb);
        bytes[c] = lead + fs * (frames - 1) + pitch * (rows - 1) + row_bytes;
        void* p = nullptr;
        if (posix_memalign(&p, 16, bytes[c])) abort();
        buf[c] = static_cast<unsigned char*>(p);
        memset(buf[c], kCanary, bytes[c]);
        for (uint32_t f = 0; f < frames; ++f)
            for (uint32_t y = 0; y < rows; ++y)
                for (int x = 0; x < width; ++x) {
                    const uint32_t s = random_sample(kind);
                    memcpy(buf[c] + lead + fs * f + pitch * y + x * sb, &s, sb);  // (little-endian: the low bytes of a 16-bit pattern)
                }
        a.plane[c] = reinterpret_cast<char*>(buf[c]) + lead;
        a.pitch[c] = static_cast<uint32_t>(pitch), a.frame_stride[c] = fs;
    }
    a.width = static_cast<uint32_t>(width), a.rows = rows, a.unit = unit;
    const uint32_t lane_pixels = static_cast<uint32_t>(16 / sb);
    a.vec_pixels = unit ? a.width / lane_pixels * lane_pixels : 0u;
    static const float m[9] = {1.f, 0.0009765625f, 1.5748f, 1.f, -0.18732427f, -0.46812427f, 1.f, 1.8556f, -0.001953125f};
    static const float offset[3] = {0.0625f, -0.03125f, 0.015625f};
    memcpy(a.m, m, sizeof m), memcpy(a.offset, offset, sizeof offset);

    uint32_t header[32] = {static_cast<uint32_t>(kind), a.width, rows, frames, unit, static_cast<uint32_t>(lead)};
    for (int c = 0; c < 3; ++c)
        header[6 + c] = static_cast<uint32_t>(bytes[c]), header[9 + c] = a.pitch[c], header[12 + c] = static_cast<uint32_t>(a.frame_stride[c]);
    memcpy(header + 16, m, sizeof m), memcpy(header + 25, offset, sizeof offset);
    fwrite(header, 4, 32, out);
    for (int c = 0; c < 3; ++c) fwrite(buf[c], 1, bytes[c], out);
    if (kind == 0) run_rows<0>(a, frames);
    else if (kind == jinc::kSampleHalf) run_rows<jinc::kSampleHalf>(a, frames);
    else run_rows<jinc::kSampleBFloat16>(a, frames);
    for (int c = 0; c < 3; ++c) {
        fwrite(buf[c], 1, bytes[c], out);
        free(buf[c]);
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s OUTPUT\n", argv[0]);
        return 2;
    }
    FILE* out = fopen(argv[1], "wb");
    if (!out) return 2;
    long cases = 0;
    for (int kind : {0, jinc::kSampleHalf, jinc::kSampleBFloat16})
        for (int width : {1, 3, 4, 7, 8, 9, 255, 256, 257, 260, 517})
            for (uint32_t unit : {16u, 4u, 0u}) {
                one_case(out, kind, width, unit);
                ++cases;
            }
    if (fclose(out)) return 2;
    printf("matrix rows: %ld cases\n", cases);
    return 0;
}
