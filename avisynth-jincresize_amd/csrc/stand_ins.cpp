// stand_ins.cpp -- device frames that do not lie as the filter's dense planes (jinc_filter_process_device_strided and every call
// behind it in include/jincresize_hip.h).  The resampling kernels keep their dense planes: a plane that lies otherwise takes a dense
// STAND-IN of the filter's sample type in a scratch allocation of the filter's, a pass in front of enqueue fills the source stand-ins,
// a pass behind it empties the result stand-ins, and planes that are dense where they lie go to the kernels as they are.
// A call is two SideSpecs (filter_internal.h), one per side, and each side is handled on its own:
//   plan_side   which planes of the side take a stand-in, in which channel groups, and the checks of the side's form
//   pass_side   the launches that fill (source) or empty (destination) the stand-ins of one slice
// run_on_stand_ins is what every such call shares: the scratch, the slicing under the knob strided_scratch_bytes, the order split ->
// enqueue -> merge on the caller's stream and the event ring between successive calls.  Any source form pairs with any destination
// form; the ABI exposes the pairings it documents (filter.cpp).
//
// The forms, source / destination pass (kernel_interleave.hip, kernel_widen.hip, kernel_narrow.hip):
//   Planes               split_samples / merge_samples: planes with a sample step (NV12 / P016, packed RGB(A)) and / or a sample shift
//                        (P010 / P012 / Y210: the sample in the high bits of its word).  Planes of one pixel form a channel group and
//                        move in one launch per step value; a plane of step 1 with a shift is a group of its own; a plane of step 1
//                        and shift 0 takes no stand-in.  The arithmetic kernels see low-aligned values, as ever.
//   Planes, converts     widen_samples / narrow_samples: INTEGER samples of `bits` bits (8: bytes, 9 .. 16: 16-bit words) into / out
//                        of an fp32 / binary16 / bfloat16 filter.  EVERY plane takes a stand-in, dense ones included (for
//                        groups_of_side every plane counts as having a shift, in the integer samples' bytes).  Widening stores
//                        float((raw >> shift) & mask), exact, or with a scale / offset fl32(fl32(float(value) * scale) + offset);
//                        narrowing stores lrintf(clamp(r, 0, peak)) << shift, with a scale / offset r = fl32(fl32(r * scale) + offset).
//                        From the stand-ins on the call is enqueue on float planes: same plan, same kernels, same finite scan.
//   Words10              unpack_fields / pack_fields: ONE buffer of 10:10:10:2 words (Y410, R10G10B10A2 and kin), one group of the
//                        side's three planes, one launch per slice.  `fields`: the three bit offsets in plane order; `fill`: the bits
//                        of every stored word outside them.
//   Words10, converts    widen_fields / narrow_fields: the same words into / out of a float filter, float(field) (ten bits: exact in
//                        fp32 and binary16) and lrintf(clamp(r, 0, 1023)), behind the scaled calls' multiply and add.
//   V210                 unpack_v210 / pack_v210: ONE buffer of v210 blocks (10-bit 4:2:2, six pixels in 16 bytes; v210_rows.h), one
//                        group of the luma stand-in and the two chroma stand-ins of half its width, one launch per slice.
//   V210, converts       widen_v210 / narrow_v210: as the words.
// The report (jinc_debug_last_strided) counts a source pass's launches as split launches and a destination pass's as merge launches.
#include "filter_internal.h"
#include "knobs.h"
#include "v210_rows.h"

namespace jinc {
namespace host {

namespace {
thread_local StridedReport t_last_strided;
thread_local GroupsReport t_last_groups;  // cleared wherever t_last_strided is: what a call that runs no pass leaves
thread_local int t_matrix_launches = 0;   // likewise: the output matrix launches of the call (jinc_debug_last_matrix_launches)

// GroupRecord::direction
enum : int { kWiden = 0, kNarrow = 1, kSplit = 2, kMerge = 3, kUnpackFields = 4, kPackFields = 5, kWidenFields = 6, kUnpackV210 = 7, kPackV210 = 8, kWidenV210 = 9, kNarrowFields = 10, kNarrowV210 = 11 };

// One entry of jinc_debug_last_groups: a pass of a slice by the numbers its launch gets.  Only the call's first slice is kept: the
// later ones differ in their frames alone.  The source pass of a slice runs in front of its destination pass and each fills its
// arguments group by group, so the entries stand source side first, each side in the order of its groups' first planes.
void record_pass(const jinc_filter& f, int direction, int step, int members, size_t sample_bytes, bool scaled, uint32_t unit,
                 uint32_t vec_pixels, uint32_t width, uint32_t rows, int first_frame) {
    if (first_frame != 0 || t_last_groups.count >= GroupsReport::kCapacity) return;
    GroupRecord& r = t_last_groups.g[t_last_groups.count++];
    r.direction = direction, r.step = step, r.members = members, r.sample_bytes = static_cast<int>(sample_bytes);
    r.sample_type = f.half ? JINC_SAMPLE_FLOAT16 : f.bf16 ? JINC_SAMPLE_BFLOAT16 : JINC_SAMPLE_DEFAULT;
    r.scaled = scaled ? 1 : 0;
    r.unit = unit, r.vec_pixels = vec_pixels, r.width = width, r.rows = rows;
    r.shifted = 0;
}
// The split / merge entries from `from` on whose groups travelled in the launch of `step`: what launch_by_shape decided for it.
void record_shifted(int from, int direction, int step, bool shifted, int first_frame) {
    if (first_frame != 0) return;
    for (int i = from; i < t_last_groups.count; ++i)
        if (t_last_groups.g[i].direction == direction && t_last_groups.g[i].step == step) t_last_groups.g[i].shifted = shifted ? 1 : 0;
}
// The field and block passes: the three planes of the filter as one group (step and members 3), samples of the filter's size.
void record_fields(const jinc_filter& f, int direction, const jinc::FieldArgs& a, int first_frame, bool scaled) {
    record_pass(f, direction, 3, 3, static_cast<size_t>(f.vi_in.component_size), scaled, a.unit, a.vec_pixels, a.width, a.rows, first_frame);
}
void record_v210(const jinc_filter& f, int direction, const jinc::V210Args& a, int first_frame, bool scaled) {  // (vec_pixels: the pixels of the blocks that move in pairs)
    record_pass(f, direction, 3, 3, static_cast<size_t>(f.vi_in.component_size), scaled, a.unit, 6u * jinc::v210::paired_blocks(a), a.width, a.rows, first_frame);
}

// Dense planes behind a call: 1 GiB unless the knob says otherwise.  Derived, not measured, per frame of a 1080p -> 4K call with rows
// padded to 256 bytes (a call of 128 frames is what the full-group batch kernels want; below kSliceFrames a slice is not rounded):
//   NV12 / P016 chroma, both sides      2 x (1024 x 540 + 2048 x 1080) = 5.5 MB: 128 frames in one slice.
//   16-bit, every plane shifted         the luma as well, 2 x (2048 x 540 + 4096 x 1080) + 3840 x 1080 + 7680 x 2160 = 31.8 MB: 33
//                                       frames, a call of 128 runs as 33 + 33 + 33 + 29 and no slice fills a whole group of the batch
//                                       kernels.  Callers that send long shifted calls raise the knob (4.1 GB for 128 frames).
//   words, both sides                   3 x (3840 x 1080 + 7680 x 2160) = 62 208 000 bytes: 17 frames, 7 x 17 + 9.
//   v210, both sides                    the source's chroma rows of 1920 bytes are padded to 2048: (3840 + 2 x 2048) x 1080 +
//                                       (7680 + 2 x 3840) x 2160 = 41 748 480 bytes: 25 frames, 5 x 25 + 3.
//   NV12 / P010 widened into fp32       7680 x 1080 + 2 x 3840 x 540 = 12 441 600 bytes: 86 frames, 86 + 42; into binary16 half of
//                                       that, 172 frames, rounded down to 128: one slice.
//   fp32 narrowed into NV12             15 360 x 2160 + 2 x 7680 x 1080 = 49 766 400 bytes: 21 frames, 6 x 21 + 2.
//   fp32 narrowed into words / v210     3 x 15 360 x 2160 = 99 532 800 bytes: 10 frames; (15 360 + 2 x 7680) x 2160 = 66 355 200: 16.
constexpr size_t kStridedScratchDefaultBytes = size_t(1) << 30;
constexpr int kSliceFrames = 128;  // slices are multiples of this where the cap allows (kFrameLanePairFrames: whole groups of the batch kernels)

struct Side {
    int group_of[4], channel_of[4], ngroups = 0;
    int w[4], h[4];
    size_t dense_pitch[4] = {0, 0, 0, 0}, dense_fs[4] = {0, 0, 0, 0};  // of the planes with a stand-in (0: the plane is dense where it lies)
    size_t offset[4] = {0, 0, 0, 0};                                    // of a stand-in's frames in the scratch, per frame of a slice
};

int step_of(const int* step, int i) { return step ? step[i] : 1; }
int shift_of(const int* shift, int i) { return shift ? shift[i] : 0; }
size_t stride_of(const SideSpec& spec, int i, int nframes) { return nframes > 1 ? spec.frame_stride[i] : 0; }
// Bytes of a sample where the caller keeps it: the integer samples' of a converting side, else the filter's.
size_t outside_bytes(const jinc_filter& f, const SideSpec& spec) {
    return spec.converts ? (spec.bits > 8 ? 2 : 1) : static_cast<size_t>(f.vi_in.component_size);
}

void check_strided_planes(const jinc_filter& f, const SideSpec& spec, const Side& s, int nframes) {
    const size_t sb = static_cast<size_t>(f.vi_in.component_size);
    for (int i = 0; i < f.planecount; ++i) {
        if (s.group_of[i] < 0) continue;  // (planes that go to the kernels where they lie: validate_planes)
        if (!spec.base[i]) throw ArgError("JincResize: null plane pointer.");
        if (spec.pitch[i] <= 0 || spec.pitch[i] % sb) throw ArgError("JincResize: plane pitch is not a multiple of the sample size.");
        if (reinterpret_cast<uintptr_t>(spec.base[i]) % sb) throw ArgError("JincResize: plane pointer is not aligned to the sample size.");
        if (stride_of(spec, i, nframes) % sb) throw ArgError("JincResize: frame stride is not a multiple of the sample size.");
        if (static_cast<size_t>(spec.pitch[i]) < (static_cast<size_t>(s.w[i] - 1) * step_of(spec.step, i) + 1) * sb)
            throw ArgError("JincResize: plane pitch is smaller than the row size at this sample step.");
    }
}

// (base alignment and the row's size of a converting side's planes: filter.cpp, in front of the device check)
void check_converting_planes(const jinc_filter& f, const SideSpec& spec, bool is_destination, int nframes) {
    const size_t bytes = outside_bytes(f, spec);
    const std::string side = is_destination ? "destination" : "source";
    for (int i = 0; i < f.planecount; ++i) {
        if (!spec.base[i]) throw ArgError("JincResize: null plane pointer.");
        if (spec.pitch[i] <= 0 || spec.pitch[i] % bytes) throw ArgError(("JincResize: " + side + " pitch is not a multiple of the " + side + " sample size.").c_str());
        if (stride_of(spec, i, nframes) % bytes) throw ArgError(("JincResize: " + side + " frame stride is not a multiple of the " + side + " sample size.").c_str());
    }
}

// (a word holds one sample of each plane, so the three stand-ins have one size: filter.cpp has refused a side whose chroma is
// sub-sampled with a message of the call's own; field_args reads the first plane's size for all three)
void check_packed10_side(const SideSpec& spec, const Side& s, int nframes) {
    const int pitch = spec.pitch[0];
    if (!spec.base[0]) throw ArgError("JincResize: null plane pointer.");
    if (s.w[1] != s.w[0] || s.w[2] != s.w[0] || s.h[1] != s.h[0] || s.h[2] != s.h[0])
        throw ArgError("JincResize: packed 10-bit words need three planes of one size on their side of the filter.");
    if (reinterpret_cast<uintptr_t>(spec.base[0]) % 4) throw ArgError("JincResize: packed 10-bit words are not aligned to 4 bytes.");
    if (pitch <= 0 || pitch % 4) throw ArgError("JincResize: pitch of packed 10-bit words is not a multiple of 4.");
    if (stride_of(spec, 0, nframes) % 4) throw ArgError("JincResize: frame stride of packed 10-bit words is not a multiple of 4.");
    if (static_cast<size_t>(pitch) < 4 * static_cast<size_t>(s.w[0])) throw ArgError("JincResize: pitch of packed 10-bit words is smaller than 4 * width.");
}

void check_v210_side(const SideSpec& spec, const Side& s, int nframes) {
    const int pitch = spec.pitch[0];
    if (!spec.base[0]) throw ArgError("JincResize: null plane pointer.");
    if (s.w[0] != 2 * s.w[1] || s.w[1] != s.w[2] || s.h[0] != s.h[1] || s.h[1] != s.h[2])
        throw ArgError("JincResize: v210 blocks need an even width and chroma planes of half that width.");
    if (reinterpret_cast<uintptr_t>(spec.base[0]) % 4) throw ArgError("JincResize: v210 blocks are not aligned to 4 bytes.");
    if (pitch <= 0 || pitch % 4) throw ArgError("JincResize: pitch of v210 blocks is not a multiple of 4.");
    if (stride_of(spec, 0, nframes) % 4) throw ArgError("JincResize: frame stride of v210 blocks is not a multiple of 4.");
    if (static_cast<size_t>(pitch) < v210_row_bytes(s.w[0]))
        throw ArgError("JincResize: pitch of v210 blocks is smaller than the row's blocks (16 * ceil(width / 6) bytes).");
}

// strided_groups, and with `shift` also every plane of step 1 with a non-zero shift as a group of its own
int groups_of_side(const void* const base[4], const int pitch[4], const int* step, const int* shift, const size_t* frame_stride,
                   const int width[4], const int height[4], int component_size, int nplanes, int group_of[4], int channel_of[4]) {
    int ngroups = 0, first[4] = {0, 0, 0, 0};
    uintptr_t lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
    const uintptr_t sb = static_cast<uintptr_t>(component_size);
    auto fs_of = [&](int i) { return frame_stride ? frame_stride[i] : size_t(0); };
    for (int i = 0; i < nplanes; ++i) {
        group_of[i] = channel_of[i] = -1;
        const int n = step_of(step, i);
        if (n <= 1 && shift_of(shift, i) == 0) continue;
        const uintptr_t b = reinterpret_cast<uintptr_t>(base[i]);
        for (int g = 0; g < ngroups && group_of[i] < 0 && n > 1; ++g) {
            const int j = first[g];
            if (step_of(step, j) != n || pitch[j] != pitch[i] || fs_of(j) != fs_of(i) || width[j] != width[i] || height[j] != height[i]) continue;
            const uintptr_t nlo = std::min(lo[g], b), nhi = std::max(hi[g], b);
            if (nhi - nlo >= static_cast<uintptr_t>(n) * sb || (b - nlo) % sb || (lo[g] - nlo) % sb) continue;  // not one pixel
            bool distinct = true;
            for (int k = 0; k < i; ++k) distinct &= !(group_of[k] == g && base[k] == base[i]);
            if (!distinct) continue;
            group_of[i] = g, lo[g] = nlo, hi[g] = nhi;
        }
        if (group_of[i] < 0) group_of[i] = ngroups, first[ngroups] = i, lo[ngroups] = hi[ngroups] = b, ++ngroups;
    }
    for (int i = 0; i < nplanes; ++i)
        if (group_of[i] >= 0) channel_of[i] = static_cast<int>((reinterpret_cast<uintptr_t>(base[i]) - lo[group_of[i]]) / sb);
    return ngroups;
}

// Which planes of one side take a stand-in, and the side's checks.
void plan_side(const jinc_filter& f, const SideSpec& spec, bool is_destination, int nframes, Side& s) {
    for (int i = 0; i < f.planecount; ++i) f.plane_dims(is_destination ? f.vi_out : f.vi_in, i, s.w[i], s.h[i]);
    if (spec.form == SideSpec::Planes) {
        // A converting side: every plane is a member of a group (every plane counts as having a shift); planes of one pixel share a
        // group by the strided call's rule, in the integer samples' bytes.
        static const int kEveryPlane[4] = {1, 1, 1, 1};
        size_t fs[4];
        for (int i = 0; i < 4; ++i) fs[i] = stride_of(spec, i, nframes);
        s.ngroups = groups_of_side(spec.base, spec.pitch, spec.step, spec.converts ? kEveryPlane : spec.shift, fs, s.w, s.h,
                                   static_cast<int>(outside_bytes(f, spec)), f.planecount, s.group_of, s.channel_of);
        if (spec.converts)
            check_converting_planes(f, spec, is_destination, nframes);
        else
            check_strided_planes(f, spec, s, nframes);
        return;
    }
    for (int i = 0; i < f.planecount; ++i) s.group_of[i] = s.channel_of[i] = 0;  // one group of the three planes
    s.ngroups = 1;
    if (spec.form == SideSpec::Words10)
        check_packed10_side(spec, s, nframes);
    else
        check_v210_side(spec, s, nframes);
}

// The groups of a Planes side as launch arguments, one Args per step (a call's groups normally share one).  Args is InterleaveArgs,
// WidenArgs or NarrowArgs; per_channel(group, channel, plane) sets what only some of them have (scale / offset).  `storing`: the
// pass writes the caller's samples (merge, narrow), else it reads them (split, widen).
template <class Args, class PerChannel>
void fill_groups(const jinc_filter& f, const SideSpec& spec, const Side& s, int direction, bool storing, char* scratch, int first_frame,
                 int slice_frames, int nframes, Args by_step[5], PerChannel per_channel) {
    const size_t bytes = outside_bytes(f, spec);
    for (int g = 0; g < s.ngroups; ++g) {
        typename std::decay<decltype(by_step->g[0])>::type e;
        int members = 0, first = -1;
        uintptr_t lo = 0;
        for (int i = 0; i < f.planecount; ++i) {
            if (s.group_of[i] != g) continue;
            if (first < 0) first = i;
            const uintptr_t b = reinterpret_cast<uintptr_t>(spec.base[i]);
            lo = members ? std::min(lo, b) : b;
            ++members;
            e.plane[s.channel_of[i]] = scratch + s.offset[i] * static_cast<size_t>(slice_frames);
            e.shift[s.channel_of[i]] = static_cast<uint8_t>(shift_of(spec.shift, i));
            per_channel(e, s.channel_of[i], i);  // (plane i's pair travels with its channel of the group)
        }
        const int n = step_of(spec.step, first);
        const size_t frame_stride = stride_of(spec, first, nframes);
        e.packed = reinterpret_cast<char*>(lo) + static_cast<size_t>(first_frame) * frame_stride;
        e.packed_frame_stride = frame_stride;
        e.plane_frame_stride = s.dense_fs[first];
        e.packed_pitch = static_cast<uint32_t>(spec.pitch[first]);
        e.plane_pitch = static_cast<uint32_t>(s.dense_pitch[first]);
        e.width = static_cast<uint32_t>(s.w[first]);
        e.rows = static_cast<uint32_t>(s.h[first]);
        const uintptr_t a = lo | static_cast<uintptr_t>(spec.pitch[first]) | static_cast<uintptr_t>(frame_stride);
        e.unit = a % 16 == 0 ? 16u : a % 4 == 0 ? 4u : 0u;
        const uint32_t lane_pixels = static_cast<uint32_t>(16 / bytes);
        // A group with a channel missing: a storing pass stores sample by sample (only the given channels' samples may be stored to), a
        // reading pass leaves the row's last pixel to the tail (its missing samples may lie behind the caller's buffer).
        const uint32_t vec_from = members == n ? e.width : storing ? 0u : e.width - 1;
        e.vec_pixels = e.unit ? vec_from / lane_pixels * lane_pixels : 0u;
        record_pass(f, direction, n, members, bytes, spec.scale || spec.offset, e.unit, e.vec_pixels, e.width, e.rows, first_frame);
        by_step[n].g[by_step[n].ngroups++] = e;
    }
}

// One buffer of words as a launch argument.  fields: the three bit offsets (checked: filter.cpp).
jinc::FieldArgs field_args(const SideSpec& spec, const Side& s, char* scratch, int first_frame, int slice_frames, int nframes) {
    jinc::FieldArgs a;
    const size_t frame_stride = stride_of(spec, 0, nframes);
    a.packed = const_cast<char*>(static_cast<const char*>(spec.base[0])) + static_cast<size_t>(first_frame) * frame_stride;
    a.packed_frame_stride = frame_stride;
    a.packed_pitch = static_cast<uint32_t>(spec.pitch[0]);
    a.plane_pitch = static_cast<uint32_t>(s.dense_pitch[0]);
    a.plane_frame_stride = s.dense_fs[0];
    a.width = static_cast<uint32_t>(s.w[0]);
    a.rows = static_cast<uint32_t>(s.h[0]);
    const uintptr_t al = reinterpret_cast<uintptr_t>(spec.base[0]) | static_cast<uintptr_t>(spec.pitch[0]) | static_cast<uintptr_t>(frame_stride);
    a.unit = al % 16 == 0 ? 16u : 4u;
    a.vec_pixels = a.width / 8 * 8;
    uint32_t mask = 0;
    for (int c = 0; c < 3; ++c) {
        a.plane[c] = scratch + s.offset[c] * static_cast<size_t>(slice_frames);
        a.offset[c] = static_cast<uint32_t>(spec.fields[c]);
        mask |= 1023u << spec.fields[c];
    }
    a.fill = spec.fill & ~mask;
    return a;
}

// One buffer of blocks as a launch argument: plane 0 is the luma stand-in, planes 1 and 2 the chroma stand-ins (one size).
jinc::V210Args v210_args(const SideSpec& spec, const Side& s, char* scratch, int first_frame, int slice_frames, int nframes) {
    jinc::V210Args a;
    const size_t frame_stride = stride_of(spec, 0, nframes);
    a.blocks = const_cast<char*>(static_cast<const char*>(spec.base[0])) + static_cast<size_t>(first_frame) * frame_stride;
    a.block_frame_stride = frame_stride;
    a.block_pitch = static_cast<uint32_t>(spec.pitch[0]);
    a.luma_pitch = static_cast<uint32_t>(s.dense_pitch[0]);
    a.chroma_pitch = static_cast<uint32_t>(s.dense_pitch[1]);
    a.luma_frame_stride = s.dense_fs[0];
    a.chroma_frame_stride = s.dense_fs[1];
    a.width = static_cast<uint32_t>(s.w[0]);
    a.rows = static_cast<uint32_t>(s.h[0]);
    a.whole_blocks = a.width / 6;
    const uintptr_t al = reinterpret_cast<uintptr_t>(spec.base[0]) | static_cast<uintptr_t>(spec.pitch[0]) | static_cast<uintptr_t>(frame_stride);
    a.unit = al % 16 == 0 ? 16u : 4u;
    for (int c = 0; c < 3; ++c) a.plane[c] = scratch + s.offset[c] * static_cast<size_t>(slice_frames);
    return a;
}

// The scaled calls' pair per plane of a converting one-buffer side (Scaled: Widen / Narrow FieldArgs / V210Args).
template <class Scaled, class Plain>
Scaled with_pairs(const SideSpec& spec, const Plain& plain) {
    Scaled a;
    static_cast<Plain&>(a) = plain;
    for (int c = 0; c < 3; ++c) a.value_scale[c] = spec.scale ? spec.scale[c] : 1.f, a.value_offset[c] = spec.offset ? spec.offset[c] : 0.f;
    return a;
}

void launched(int rc, const char* what) { hip_check(static_cast<hipError_t>(rc), what); }

// The pass of one side over frames [k0, k0 + n) of the call, whose stand-ins hold `slice` frames: the source side's fills them, the
// destination side's empties them.  Returns the number of launches.
int pass_side(const jinc_filter& f, const SideSpec& spec, const Side& s, bool is_destination, char* scratch, int k0, int slice, int n,
              int nframes, hipStream_t stream) {
    if (s.ngroups == 0) return 0;
    const int sb = f.vi_in.component_size, kind = f.sample_kind();
    const bool scaled = spec.scale || spec.offset;
    if (spec.form == SideSpec::Words10) {
        const jinc::FieldArgs a = field_args(spec, s, scratch, k0, slice, nframes);
        record_fields(f, spec.converts ? (is_destination ? kNarrowFields : kWidenFields) : (is_destination ? kPackFields : kUnpackFields), a, k0, scaled);
        if (!spec.converts)
            is_destination ? launched(jinc::launch_pack_fields(a, n, stream), "pack launch") : launched(jinc::launch_unpack_fields(a, n, stream), "unpack launch");
        else if (is_destination)
            launched(jinc::launch_narrow_fields(with_pairs<jinc::NarrowFieldArgs>(spec, a), kind, n, stream, scaled), "narrow fields launch");
        else
            launched(jinc::launch_widen_fields(with_pairs<jinc::WidenFieldArgs>(spec, a), kind, n, stream, scaled), "widen fields launch");
        return 1;
    }
    if (spec.form == SideSpec::V210) {
        const jinc::V210Args a = v210_args(spec, s, scratch, k0, slice, nframes);
        record_v210(f, spec.converts ? (is_destination ? kNarrowV210 : kWidenV210) : (is_destination ? kPackV210 : kUnpackV210), a, k0, scaled);
        if (!spec.converts)
            is_destination ? launched(jinc::launch_pack_v210(a, n, stream), "v210 pack launch") : launched(jinc::launch_unpack_v210(a, n, stream), "v210 unpack launch");
        else if (is_destination)
            launched(jinc::launch_narrow_v210(with_pairs<jinc::NarrowV210Args>(spec, a), kind, n, stream, scaled), "narrow v210 launch");
        else
            launched(jinc::launch_widen_v210(with_pairs<jinc::WidenV210Args>(spec, a), kind, n, stream, scaled), "widen v210 launch");
        return 1;
    }
    // Planes: one launch per step value present (step 1: planes that only have a shift, or any plane of a converting side).
    int launches = 0;
    auto pairs = [&](auto& e, int channel, int plane) {
        e.scale[channel] = spec.scale ? spec.scale[plane] : 1.f;
        e.offset[channel] = spec.offset ? spec.offset[plane] : 0.f;
    };
    if (!spec.converts) {
        InterleaveArgs by_step[5];
        const int recorded = t_last_groups.count, direction = is_destination ? kMerge : kSplit;
        fill_groups(f, spec, s, direction, is_destination, scratch, k0, slice, nframes, by_step, [](InterleaveGroup&, int, int) {});
        for (int step = 1; step <= 4; ++step) {
            if (!by_step[step].ngroups) continue;
            bool shifted = false;
            if (is_destination)
                launched(jinc::launch_merge_samples(by_step[step], sb, step, n, stream, &shifted), "merge launch");
            else
                launched(jinc::launch_split_samples(by_step[step], sb, step, n, stream, &shifted), "split launch");
            record_shifted(recorded, direction, step, shifted, k0);
            ++launches;
        }
    } else if (is_destination) {
        NarrowArgs by_step[5];
        fill_groups(f, spec, s, kNarrow, true, scratch, k0, slice, nframes, by_step, pairs);
        for (int step = 1; step <= 4; ++step) {
            if (!by_step[step].ngroups) continue;
            by_step[step].peak = static_cast<float>((1u << spec.bits) - 1u);
            launched(jinc::launch_narrow_samples(by_step[step], kind, step, static_cast<int>(outside_bytes(f, spec)), n, stream, scaled), "narrow launch");
            ++launches;
        }
    } else {
        WidenArgs by_step[5];
        fill_groups(f, spec, s, kWiden, false, scratch, k0, slice, nframes, by_step, pairs);
        for (int step = 1; step <= 4; ++step) {
            if (!by_step[step].ngroups) continue;
            by_step[step].mask = (1u << spec.bits) - 1u;
            launched(jinc::launch_widen_samples(by_step[step], static_cast<int>(outside_bytes(f, spec)), step, sb, kind, n, stream, scaled), "widen launch");
            ++launches;
        }
    }
    return launches;
}

// The part every call with stand-ins shares: `in` / `out` say which planes of a side take a dense stand-in (group_of >= 0; of those
// planes base, pitch and frame stride are not read here).
void run_on_stand_ins(jinc_filter& f, const SideSpec& src, const SideSpec& dst, Side& in, Side& out, int nframes, hipStream_t stream) {
    const size_t sb = static_cast<size_t>(f.vi_in.component_size);

    // Dense planes of the strided ones: pitch and frame stride multiples of 256 bytes, like the look-ahead pipeline's group buffers.
    size_t per_frame = 0;
    for (Side* s : {&in, &out})
        for (int i = 0; i < f.planecount; ++i) {
            if (s->group_of[i] < 0) continue;
            s->dense_pitch[i] = align_up(static_cast<size_t>(s->w[i]) * sb, 256);
            s->dense_fs[i] = s->dense_pitch[i] * static_cast<size_t>(s->h[i]);
            s->offset[i] = per_frame;
            per_frame += s->dense_fs[i];
        }
    const double cap_knob = knobs::get(JINC_KNOB_STRIDED_SCRATCH_BYTES, static_cast<double>(kStridedScratchDefaultBytes));
    const size_t cap = cap_knob < 1.0 ? size_t(1) : static_cast<size_t>(cap_knob);
    int slice = static_cast<int>(std::min<size_t>(static_cast<size_t>(nframes), std::max<size_t>(cap / per_frame, 1)));
    if (slice < nframes && slice >= kSliceFrames) slice = slice / kSliceFrames * kSliceFrames;

    // The planes as the kernels will get them: dense ones where they lie, strided ones as their dense stand-ins.
    const void* s_run[4] = {nullptr, nullptr, nullptr, nullptr};
    void* d_run[4] = {nullptr, nullptr, nullptr, nullptr};
    int sp_run[4] = {0, 0, 0, 0}, dp_run[4] = {0, 0, 0, 0};
    size_t sfs_run[4] = {0, 0, 0, 0}, dfs_run[4] = {0, 0, 0, 0};
    for (int i = 0; i < f.planecount; ++i) {
        const bool si = in.group_of[i] >= 0, di = out.group_of[i] >= 0;
        s_run[i] = si ? static_cast<const void*>(nullptr) : src.base[i];
        d_run[i] = di ? static_cast<void*>(nullptr) : const_cast<void*>(dst.base[i]);
        sp_run[i] = si ? static_cast<int>(in.dense_pitch[i]) : src.pitch[i];
        dp_run[i] = di ? static_cast<int>(out.dense_pitch[i]) : dst.pitch[i];
        sfs_run[i] = si ? in.dense_fs[i] : stride_of(src, i, nframes);
        dfs_run[i] = di ? out.dense_fs[i] : stride_of(dst, i, nframes);
    }
    const size_t need = per_frame * static_cast<size_t>(slice);
    if (need > f.strided_scratch_bytes) {
        if (f.strided_scratch) {
            hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize(strided scratch)");  // launches of earlier calls may still use the old planes
            (void)hipFree(f.strided_scratch);
        }
        f.strided_scratch = nullptr, f.strided_scratch_bytes = 0, f.strided_pending = false;
        hip_check(hipMalloc(&f.strided_scratch, need), "hipMalloc(strided scratch)");
        f.strided_scratch_bytes = need;
    }
    char* scratch = static_cast<char*>(f.strided_scratch);
    for (int i = 0; i < f.planecount; ++i) {
        if (in.group_of[i] >= 0) s_run[i] = scratch + in.offset[i] * static_cast<size_t>(slice);
        if (out.group_of[i] >= 0) d_run[i] = scratch + out.offset[i] * static_cast<size_t>(slice);
    }
    validate_planes(f, s_run, sp_run, sfs_run, d_run, dp_run, dfs_run, nframes);  // (before anything is queued)

    // The dense planes are shared by successive calls: a call on ANOTHER stream than the previous strided call's waits for that
    // call's last merge (same stream: stream order does it).  A ring of events, one per call in turn, like the fork / join events:
    // no event is recorded again while a stream may still be waiting on it.
    const unsigned turn = f.strided_turn % jinc_filter::kForkEvents;
    if (f.strided_pending && stream != f.strided_last_stream)
        hip_check(hipStreamWaitEvent(stream, f.ev_strided[(f.strided_turn + jinc_filter::kForkEvents - 1) % jinc_filter::kForkEvents], 0), "hipStreamWaitEvent(strided)");
    if (!f.ev_strided[turn]) hip_check(hipEventCreateWithFlags(&f.ev_strided[turn], hipEventDisableTiming), "hipEventCreate(strided)");

    StridedReport report{0, 0, 0, static_cast<long long>(f.strided_scratch_bytes)};
    for (int k0 = 0; k0 < nframes; k0 += slice) {
        const int n = std::min(slice, nframes - k0);
        const void* s_now[4];
        void* d_now[4];
        for (int i = 0; i < 4; ++i) {
            s_now[i] = (i < f.planecount && in.group_of[i] < 0) ? static_cast<const char*>(src.base[i]) + static_cast<size_t>(k0) * sfs_run[i] : s_run[i];
            d_now[i] = (i < f.planecount && out.group_of[i] < 0) ? const_cast<char*>(static_cast<const char*>(dst.base[i])) + static_cast<size_t>(k0) * dfs_run[i] : d_run[i];
        }
        // Order on the caller's stream: split -> enqueue -> merge.  enqueue's side-stream kernels start behind ev_fork, which it records
        // on `stream` AFTER the split queued here, and `stream` goes on only behind ev_join, recorded on the side stream after its last
        // kernel: the merge queued below follows both streams' kernels.
        report.split_launches += pass_side(f, src, in, false, scratch, k0, slice, n, nframes, stream);
        enqueue(f, s_now, sp_run, sfs_run, d_now, dp_run, dfs_run, n, stream);
        apply_output_matrix(f, d_now, dp_run, dfs_run, n, stream);  // (nothing without a matrix; behind ev_join, in front of the merge)
        report.merge_launches += pass_side(f, dst, out, true, scratch, k0, slice, n, nframes, stream);
        ++report.slices;
    }
    hip_check(hipEventRecord(f.ev_strided[turn], stream), "hipEventRecord(strided)");
    ++f.strided_turn;
    f.strided_pending = true;
    f.strided_last_stream = stream;
    t_last_strided = report;
}

}  // namespace

size_t v210_row_bytes(int width) { return width < 1 ? 0 : 16 * ((static_cast<size_t>(width) + 5) / 6); }

int strided_groups(const void* const base[4], const int pitch[4], const int* step, const size_t* frame_stride, const int width[4],
                   const int height[4], int component_size, int nplanes, int group_of[4], int channel_of[4]) {
    return groups_of_side(base, pitch, step, nullptr, frame_stride, width, height, component_size, nplanes, group_of, channel_of);
}

const StridedReport& last_strided_report() { return t_last_strided; }
const GroupsReport& last_groups_report() { return t_last_groups; }

// The pass of jinc_filter_set_output_matrix over planes 0 .. 2 as the resampling kernels have left them (the setter has seen to it
// that they have one size): in place, one launch, on the caller's stream -- enqueue has joined its side stream back by now.
void apply_output_matrix(const jinc_filter& f, void* const planes[4], const int pitch[4], const size_t frame_stride[4], int nframes,
                         hipStream_t stream) {
    if (!f.has_matrix) return;
    jinc::MatrixArgs a;
    int w = 0, h = 0;
    f.plane_dims(f.vi_out, 0, w, h);
    uintptr_t al = 0;
    for (int c = 0; c < 3; ++c) {
        a.plane[c] = static_cast<char*>(planes[c]);
        a.pitch[c] = static_cast<uint32_t>(pitch[c]);
        a.frame_stride[c] = (nframes > 1 && frame_stride) ? frame_stride[c] : 0;
        al |= reinterpret_cast<uintptr_t>(planes[c]) | static_cast<uintptr_t>(pitch[c]) | static_cast<uintptr_t>(a.frame_stride[c]);
    }
    a.width = static_cast<uint32_t>(w), a.rows = static_cast<uint32_t>(h);
    a.unit = al % 16 == 0 ? 16u : al % 4 == 0 ? 4u : 0u;  // (as fill_groups has it, over all three planes)
    const uint32_t lane_pixels = 16u / static_cast<uint32_t>(f.vi_in.component_size);
    a.vec_pixels = a.unit ? a.width / lane_pixels * lane_pixels : 0u;
    for (int k = 0; k < 9; ++k) a.m[k] = f.matrix[k];
    for (int k = 0; k < 3; ++k) a.offset[k] = f.matrix_offset[k];
    launched(jinc::launch_output_matrix(a, f.sample_kind(), nframes, stream), "output matrix launch");
    ++t_matrix_launches;
}
void reset_matrix_launches() { t_matrix_launches = 0; }
int last_matrix_launches() { return t_matrix_launches; }

void enqueue_sides(jinc_filter& f, const SideSpec& src, const SideSpec& dst, int nframes, hipStream_t stream) {
    t_last_strided = {0, 0, 0, static_cast<long long>(f.strided_scratch_bytes)};  // (also what a refused call leaves: it launched nothing)
    t_last_groups.count = 0;
    t_matrix_launches = 0;
    // The source side is planned and checked first, then the destination side.  (Before the two sides were described apart, the
    // widened calls for words and blocks checked their destination planes first: their source checks repeat what filter.cpp has
    // refused with texts of its own, all but the odd width of a v210 source, which a call with a faulty destination as well now
    // hears of first.)
    Side in, out;
    plan_side(f, src, false, nframes, in);
    plan_side(f, dst, true, nframes, out);
    if (in.ngroups == 0 && out.ngroups == 0) {  // dense planes on both sides (Planes, not converting): the call IS jinc_filter_process_device
        enqueue(f, src.base, src.pitch, src.frame_stride, const_cast<void* const*>(dst.base), dst.pitch, dst.frame_stride, nframes, stream);
        apply_output_matrix(f, const_cast<void* const*>(dst.base), dst.pitch, dst.frame_stride, nframes, stream);
        return;
    }
    run_on_stand_ins(f, src, dst, in, out, nframes, stream);
}

}  // namespace host
}  // namespace jinc
