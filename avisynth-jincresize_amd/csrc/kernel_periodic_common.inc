// kernel_periodic_common.inc -- pieces shared by the kernels of the periodic family (kernel_periodic*.hip, kernel_rowpair.hip);
// included INSIDE namespace jinc { namespace { of the including translation unit.
typedef float f32x2 __attribute__((ext_vector_type(2)));

// Float planes on the trimmed support (PeriodicArgs::frame_flags, run_when; csrc/dispatch.cpp): a launch with run_when 0 / 1
// returns at once for frames whose flag differs; a launch with run_when == kRunAllAndFlag computes every frame and SETS the flag
// of a frame in whose staged samples it meets an infinity or a NaN -- the kernel reads every source sample of its tiles anyway, so
// the finite-sample scan costs a compare per staged sample instead of a pass over the source.  (The full-window launch behind it,
// run_when 1, then computes those frames again.)
constexpr uint32_t kRunAllAndFlag = PeriodicArgs::kRunAllAndFlag;
__device__ __forceinline__ bool skips_frame(const PeriodicArgs& a, size_t frame) {
    return a.frame_flags && a.run_when != kRunAllAndFlag && ((const JINC_CONSTANT uint32_t*)a.frame_flags)[frame] != a.run_when;
}
// Per thread and tile: did an exponent of all ones (an infinity or a NaN) pass through the staging registers?  Declared beside
// the staging registers; its destructor, at the end of the staging block, sets the frame's flag.  Integer planes: nothing.
template <typename T>
struct NonFinite {
    const PeriodicArgs& a;
    const size_t frame;
    uint32_t acc = 0;
    __device__ __forceinline__ NonFinite(const PeriodicArgs& a_, size_t frame_) : a(a_), frame(frame_) {}
    __device__ __forceinline__ float take(T v) {
        // (exponent 0xff: the biased field plus one carries into the sign bit)
        if constexpr (is_float_sample_v<T>) acc |= nonfinite_bit(v);
        return to_float(v);
    }
    __device__ __forceinline__ ~NonFinite() {
        if constexpr (is_float_sample_v<T>) {
            if (a.run_when == kRunAllAndFlag && (acc & 0x80000000u)) const_cast<uint32_t*>(a.frame_flags)[frame] = 1u;  // (every writer writes 1)
        }
    }
};

constexpr int kTileCols = 64;  // source-aligned columns per tile = lanes of a wave

// Tile of the window kernel (ewa_periodic_kernel) and of the one-period quad forms (kernel_periodic_quad.hip).
// RG: row groups of FS rows per tile.  A/B on MI355X: fs 7 (C2) 8 groups = 4 groups (was +2.3 % before the staging loads
// were issued together), 16 groups 10 % slower; fs 9 (C4, 88 VGPRs = 5 waves/SIMD) 9 groups +3.9 % over 6 -- 27 KB of
// LDS per block still allows the 5 blocks per CU the registers allow.
template <int FS, int RG = (FS <= 7 ? 8 : 9)>
struct PeriodicCfg {
    static constexpr int kRowGroups = RG;
    static constexpr int kTileRows = FS * kRowGroups;     // period-rows per tile (multiple of FS)
    static constexpr int kLdsCols = kTileCols + FS;       // 64 + (FS-1) halo + 1 phase spread
    static constexpr int kLdsPitch = kLdsCols + 1;        // odd pitch not needed for row reads; keeps staging writes spread
    static constexpr int kLdsRows = kTileRows + FS;       // TJ + (FS-1) halo + 1 phase spread
};

// The sample type of a launch: f(T{}) with T = uint8_t, uint16_t, half_t, bf16_t or float as io describes the planes.  Every
// launcher of the family that crosses a unit boundary (kernel_periodic_launch.h) picks its instantiations through this.
template <typename F>
int for_sample_type(const PlaneIO& io, F&& f) {
    switch (io.sample_bytes) {
        case 1: return f(uint8_t{});
        case 2:
            if (io.sample_kind == kSampleHalf) return f(half_t{});
            if (io.sample_kind == kSampleBFloat16) return f(bf16_t{});
            return f(uint16_t{});
        default: return f(float{});
    }
}
