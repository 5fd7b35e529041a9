// widen_fields_rows.h -- one lane's share of one row of the pass that widens 10:10:10:2 words (kernel_widen.hip widen_fields_kernel;
// kernels.h FieldArgs), as a plain inline function for host and device: a stand-alone host program runs exactly this code lane by
// lane against exactly sized buffers (tests/host_sanitizer/widen_fields_rows_main.cpp).
//
// One little-endian 32-bit word per pixel becomes one fp32 (OB = 4) or binary16 (OB = 2) sample in each of three dense planes:
// plane c holds float((word >> offset[c]) & 1023).  The conversion is exact: ten bits are an fp32 and a binary16 value alike.
//
// A lane owns 8 pixels per step, as in unpack_fields_kernel: two 16-byte loads on the word side (consecutive lanes, consecutive
// addresses; eight dwords where base, pitch or frame stride is a multiple of 4 only) and, per plane, OB / 2 adjacent 16-byte
// vectors of converted samples -- a wave's trip stores one contiguous piece of 64 x 8 x OB bytes (2 KiB fp32, 1 KiB binary16) to
// each plane.  The offsets are the same in every lane.  The rest of the row goes word by word under the width guard.  Nothing
// beyond `width` words is read and nothing beyond `width` samples is stored; the words are never written (`fill` is not read).
//
// The scaled forms (trailing template parameters KIND and Scaled; jinc_filter_process_device_widened_packed10_scaled; kernels.h
// WidenFieldArgs): plane c holds s = fl32(fl32(float(field) * value_scale[c]) + value_offset[c]) -- widen_rows.h's scaled_value, two
// fp32 roundings, never an FMA -- and 16-bit planes hold s narrowed round-to-nearest-even by widen_rows.h's pair_bits / rounded_bits,
// the ONE definition of that rounding; bfloat16 planes (KIND = kSampleBFloat16) exist in this form only.  The pair of a plane is the
// same in every lane, as its offset; the unscaled forms read neither.  Loads, stores and guards are the unscaled forms'.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernels.h"
#include "widen_rows.h"

namespace jinc {
namespace widen {

// The field at `offset` of a word as the bits of its converted value: v_cvt_f32_u32 behind shift and mask, v_cvt_f16_f32 on top.
template <int OB>
JINC_WIDEN_HD uint32_t field_bits(uint32_t word, uint32_t offset) {
    const float v = static_cast<float>((word >> offset) & 1023u);
    if constexpr (OB == 4) return float_bits(v);
    else return half_bits(v);
}
// ... and as the fp32 sample the plane holds: the value itself, or widen_rows.h's scaled_value of it (one multiply, one add).
template <bool Scaled>
JINC_WIDEN_HD float field_sample(uint32_t word, uint32_t offset, float scale, float value_offset) {
    const float v = static_cast<float>((word >> offset) & 1023u);
    if constexpr (Scaled) return scaled_value(v, scale, value_offset);
    else return v;
}

// Lane `lane` of the wave that owns row `row` of frame `frame`.  Args: FieldArgs, or WidenFieldArgs for the scaled forms.
template <int OB, int KIND = 0, bool Scaled = false, class Args>
JINC_WIDEN_HD void widen_fields_row(const Args& a, uint32_t frame, uint32_t row, uint32_t lane) {
    static_assert(OB == 4 || OB == 2, "no such form");
    static_assert(KIND == 0 || (KIND == kSampleHalf && OB == 2) || (KIND == kSampleBFloat16 && OB == 2 && Scaled), "no such form");
    const char* __restrict__ packed = a.packed + frame * a.packed_frame_stride + static_cast<size_t>(row) * a.packed_pitch;
    const size_t dense = frame * a.plane_frame_stride + static_cast<size_t>(row) * a.plane_pitch;
    for (uint32_t x = lane * 8; x < a.vec_pixels; x += 64 * 8) {
        uint32_t w[8];
        load_pixels<2>(packed + static_cast<size_t>(x) * 4, a.unit, w);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t sh = a.offset[c];
            float sc = 1.f, of = 0.f;
            if constexpr (Scaled) sc = a.value_scale[c], of = a.value_offset[c];
            char* out = a.plane[c] + dense + static_cast<size_t>(x) * OB;
            uint32_t o[4];
            if constexpr (OB == 4) {
#pragma unroll
                for (int v = 0; v < 2; ++v) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[k] = float_bits(field_sample<Scaled>(w[4 * v + k], sh, sc, of));
                    store16(out + 16 * v, o);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = pair_bits<KIND, Scaled>(field_sample<Scaled>(w[2 * k], sh, sc, of), field_sample<Scaled>(w[2 * k + 1], sh, sc, of));
                store16(out, o);
            }
        }
    }
    for (uint32_t x = a.vec_pixels + lane; x < a.width; x += 64) {
        const uint32_t w = reinterpret_cast<const uint32_t*>(packed)[x];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float sc = 1.f, of = 0.f;
            if constexpr (Scaled) sc = a.value_scale[c], of = a.value_offset[c];
            const float s = field_sample<Scaled>(w, a.offset[c], sc, of);
            if constexpr (OB == 4) reinterpret_cast<uint32_t*>(a.plane[c] + dense)[x] = float_bits(s);
            else if constexpr (Scaled) reinterpret_cast<uint16_t*>(a.plane[c] + dense)[x] = static_cast<uint16_t>(rounded_bits<KIND>(s));
            else reinterpret_cast<uint16_t*>(a.plane[c] + dense)[x] = static_cast<uint16_t>(half_bits(s));
        }
    }
}

}  // namespace widen
}  // namespace jinc
