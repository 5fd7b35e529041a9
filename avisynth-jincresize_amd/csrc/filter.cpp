// filter.cpp -- host side of libjincresize_hip.so: the C ABI declared in include/jincresize_hip.h.
//
// Mirrors the reference plugin's filter life cycle for the accelerated path
// ("ref:" = /root/reference/src/JincResize.cpp):
//   jinc_filter_create      <- Create_JincResize      (ref :654-984)  same defaults, same checks in
//                                                      the same order, same error strings
//   jinc_filter_get_frame   <- process_frame call in JincResize_GetFrame (ref :615)
//   jinc_filter_free        <- free_JincResize         (ref :632-647)
//   jinc_alias_args         <- resizer()/resizer_jincresize<taps> (ref :1007-1040)
// There is no CPU fallback: without a HIP device every frame call fails loudly.
#include <cctype>

#include "filter_internal.h"
#include "knobs.h"

using namespace jinc::host;

namespace {
thread_local std::string g_last_error;
// What jinc_filter_get_frame and jinc_filter_submit (and so a jinc_batch, which submits) tell a filter with an output matrix.
const char* const kMatrixOnHostFrames =
    "JincResize: this filter has an output matrix (jinc_filter_set_output_matrix), which only the jinc_filter_process_device* calls apply; "
    "host frames are not supported with one.";
}  // namespace

namespace jinc {
namespace host {
int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}
}  // namespace host
}  // namespace jinc

namespace {

template <typename Fn>
int guarded(Fn&& fn) {
    try {
        fn();
        g_last_error.clear();
        return JINC_OK;
    } catch (const ArgError& e) {
        return fail(JINC_ERR_INVALID_ARG, e.what());
    } catch (const HipError& e) {
        return fail(JINC_ERR_HIP, e.what());
    } catch (const std::bad_alloc&) {
        return fail(JINC_ERR_NOMEM, "JincResize: out of memory.");
    } catch (const std::exception& e) {
        return fail(JINC_ERR_UNSUPPORTED, e.what());
    }
}

const jinc::PlanePlan* table_or_null(const jinc_filter* f, int table) {
    if (!f || table < 0 || table >= static_cast<int>(f->plans.size())) return nullptr;
    return &f->plans[table];
}

// What the widened and the narrowed calls for words and blocks refuse alike, behind the checks of the filter (and the offsets): the
// steps of the OTHER side's planes, then base, pitch and frame stride of the one buffer.  `call` / `other`: "widened" / "destination",
// "narrowed" / "source"; `what`: "packed 10-bit words" / "v210 blocks"; row_bytes: what a row occupies.  Returns a message, empty
// when there is nothing to refuse.
std::string refuse_words(const jinc_filter* f, const char* call, const char* other, const char* what, const void* buffer, int pitch,
                         size_t frame_stride, size_t row_bytes, const char* row_text, const int* other_sample_step, int nframes) {
    const std::string of_call = std::string(" of ") + call + " " + what;
    for (int i = 0; other_sample_step && i < f->planecount; ++i)
        if (other_sample_step[i] < 1 || other_sample_step[i] > 4)
            return std::string("JincResize: ") + other + " sample step of a " + call + " call for " + what + " must be in 1..4 (got " +
                   std::to_string(other_sample_step[i]) + ").";
    if (reinterpret_cast<uintptr_t>(buffer) % 4) return std::string("JincResize: ") + call + " " + what + " are not aligned to 4 bytes.";
    if (pitch % 4) return "JincResize: pitch " + std::to_string(pitch) + of_call + " is not a multiple of 4.";
    if (nframes > 1 && frame_stride % 4) return "JincResize: frame stride " + std::to_string(frame_stride) + of_call + " is not a multiple of 4.";
    if (pitch <= 0 || static_cast<size_t>(pitch) < row_bytes)
        return "JincResize: pitch " + std::to_string(pitch) + of_call + " is smaller than the row's " + std::to_string(row_bytes) + " bytes (" + row_text + ").";
    return std::string();
}

// The three bit offsets of a 10:10:10:2 word (NULL: nothing to refuse here): each in 0..22, no two fields overlapping.  `word`:
// "packed" / "widened packed" / "narrowed packed"; with_values: the message ends in the offending offsets.
std::string refuse_fields(const char* word, const int* o, bool with_values) {
    for (int i = 0; o && i < 3; ++i)
        if (o[i] < 0 || o[i] > 22)
            return std::string("JincResize: a field offset of a ") + word + " 10:10:10:2 word must be in 0..22" +
                   (with_values ? " (got " + std::to_string(o[i]) + ")" : std::string()) + ".";
    for (int i = 0; o && i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (o[i] - o[j] < 10 && o[j] - o[i] < 10)
                return std::string("JincResize: two fields of a ") + word + " 10:10:10:2 word overlap" +
                       (with_values ? " (offsets " + std::to_string(o[i]) + " and " + std::to_string(o[j]) + ")" : std::string()) + ".";
    return std::string();
}

// The shape rules of the stand-in calls are per side: a side of packed 10:10:10:2 words needs that side of the filter without
// sub-sampling, a side of v210 blocks needs it 4:2:2.  Filters whose two sides share their sub-sampling (jinc_filter_create /
// _create_ex) are refused by the calls' own texts; these are what a filter of jinc_filter_create_out with ANOTHER output
// sub-sampling is told: `what` names the words or blocks, `side` is "source" or "destination".
std::string refuse_side(const jinc_filter* f, const char* what, const char* side, const char* needs) {
    const bool source = side[0] == 's';
    const jinc_video_info& vi = source ? f->vi_in : f->vi_out;
    return std::string("JincResize: ") + what + " on the " + side + " side need a filter whose " + (source ? "input" : "output") + " is " + needs +
           "; this filter's " + (source ? "input" : "output") + " has sub_w " + std::to_string(vi.sub_w) + " and sub_h " + std::to_string(vi.sub_h) + ".";
}

// What the two scaled calls refuse of their own: a scale or offset of a used plane that is NaN or infinite, a scale that is zero.
// `side` is "source" (widened) or "destination" (narrowed).  Empty: nothing to refuse.
std::string refuse_scale_offset(const char* side, const float* scale, const float* offset, int planes) {
    for (int i = 0; i < planes; ++i) {
        const std::string of_plane = std::string(side) + " plane " + std::to_string(i);
        if (scale && std::isnan(scale[i])) return "JincResize: the scale of " + of_plane + " is NaN.";
        if (scale && std::isinf(scale[i])) return "JincResize: the scale of " + of_plane + " is infinite.";
        if (scale && scale[i] == 0.f) return "JincResize: the scale of " + of_plane + " is zero.";
        if (offset && std::isnan(offset[i])) return "JincResize: the offset of " + of_plane + " is NaN.";
        if (offset && std::isinf(offset[i])) return "JincResize: the offset of " + of_plane + " is infinite.";
    }
    return std::string();
}

// One side of a stand-in call from the caller's arrays (any of them NULL: an empty side; the call is refused before it is read) ...
SideSpec side_of_arrays(const jinc_filter* f, SideSpec::Form form, const void* const base[4], const int pitch[4], const size_t* frame_stride,
                        const int* step = nullptr, const int* shift = nullptr) {
    SideSpec s;
    s.form = form, s.step = step, s.shift = shift;
    for (int i = 0; base && pitch && i < f->planecount; ++i)
        s.base[i] = base[i], s.pitch[i] = pitch[i], s.frame_stride[i] = frame_stride ? frame_stride[i] : 0;
    return s;
}
// ... and from ONE buffer of words or blocks.
SideSpec side_of_buffer(SideSpec::Form form, const void* buffer, int pitch, size_t frame_stride) {
    SideSpec s;
    s.form = form, s.base[0] = buffer, s.pitch[0] = pitch, s.frame_stride[0] = frame_stride;
    return s;
}
SideSpec converting(SideSpec s, int bits, const float* scale, const float* offset) {
    s.converts = true, s.bits = bits, s.scale = scale, s.offset = offset;
    return s;
}

// What every stand-in call ends with, behind its own refusals: null argument, no device, nframes and frame strides, in this order,
// then the call.  arrays_given: no array the call reads is NULL; strides_given: nor the frame strides of a side that has an array of them.
int run_sides(jinc_filter* f, bool arrays_given, bool strides_given, const SideSpec& src, const SideSpec& dst, int nframes, void* hip_stream) {
    if (!arrays_given) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (f->device < 0) return fail(JINC_ERR_NO_DEVICE, "JincResize: filter was created without a HIP device (device < 0).");
    if (nframes < 1 || nframes > 65535) return fail(JINC_ERR_INVALID_ARG, "JincResize: nframes must be in 1..65535.");
    if (nframes > 1 && !strides_given) return fail(JINC_ERR_INVALID_ARG, "JincResize: frame strides are required for nframes > 1.");
    return guarded([&] {
        hip_check(hipSetDevice(f->device), "hipSetDevice");
        enqueue_sides(*f, src, dst, nframes, static_cast<hipStream_t>(hip_stream));  // (NULL stream: the HIP null stream)
    });
}
}  // namespace

extern "C" {

int jinc_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return 0;
    return count;
}

int jinc_pick_device(void) {
    static std::atomic<unsigned> counter{0};
    const int n = jinc_device_count();
    if (n <= 0) return -1;
    return static_cast<int>(counter.fetch_add(1) % static_cast<unsigned>(n));
}

const char* jinc_last_error(void) { return g_last_error.c_str(); }

int jinc_filter_create(const jinc_video_info* vi, const jinc_args* args, int device, jinc_filter** out, char* err,
                       size_t err_len) {
    return jinc_filter_create_ex(vi, args, JINC_SAMPLE_DEFAULT, device, out, err, err_len);
}

int jinc_filter_create_ex(const jinc_video_info* vi, const jinc_args* args, int sample_type, int device, jinc_filter** out, char* err,
                          size_t err_len) {
    return jinc_filter_create_out(vi, args, sample_type, -1, -1, device, out, err, err_len);
}

int jinc_filter_create_out(const jinc_video_info* vi, const jinc_args* args, int sample_type, int out_sub_w, int out_sub_h, int device,
                           jinc_filter** out, char* err, size_t err_len) {
    if (out) *out = nullptr;
    if (err && err_len) err[0] = '\0';
    if (!vi || !args || !out) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    std::unique_ptr<jinc_filter> f(new (std::nothrow) jinc_filter());
    if (!f) return fail(JINC_ERR_NOMEM, "JincResize: out of memory.");
    int rc = guarded([&] {
        if (sample_type != JINC_SAMPLE_DEFAULT && sample_type != JINC_SAMPLE_FLOAT16 && sample_type != JINC_SAMPLE_BFLOAT16)
            throw ArgError("JincResize: sample type must be JINC_SAMPLE_DEFAULT, JINC_SAMPLE_FLOAT16 or JINC_SAMPLE_BFLOAT16.");
        if (sample_type == JINC_SAMPLE_FLOAT16 && (vi->bits_per_component != 16 || vi->component_size != 2))
            throw ArgError("JincResize: half-precision float clips must have 16 bits per component and 2-byte samples.");
        if (sample_type == JINC_SAMPLE_BFLOAT16 && (vi->bits_per_component != 16 || vi->component_size != 2))
            throw ArgError("JincResize: bfloat16 clips must have 16 bits per component and 2-byte samples.");
        f->half = sample_type == JINC_SAMPLE_FLOAT16;
        f->bf16 = sample_type == JINC_SAMPLE_BFLOAT16;
        configure(*f, *vi, *args, out_sub_w, out_sub_h);
        if (device >= 0) init_device(*f, device);
    });
    if (rc == JINC_ERR_HIP && device >= 0 && jinc_device_count() == 0) rc = JINC_ERR_NO_DEVICE;
    if (rc != JINC_OK) {
        if (err && err_len) {
            std::strncpy(err, g_last_error.c_str(), err_len - 1);
            err[err_len - 1] = '\0';
        }
        return rc;
    }
    *out = f.release();
    return JINC_OK;
}

void jinc_filter_free(jinc_filter* f) { delete f; }

int jinc_filter_output_info(const jinc_filter* f, jinc_video_info* out_vi) {
    if (!f || !out_vi) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    *out_vi = f->vi_out;
    return JINC_OK;
}

int jinc_filter_chroma_location(const jinc_filter* f) {
    if (!f) return -1;
    return f->chroma_location_mode == JINC_CHROMA_LOCATION_BY_SITING ? f->chroma_location_by_siting : f->chroma_location;
}

int jinc_filter_set_chroma_location_mode(jinc_filter* f, int mode) {
    if (!f || (mode != JINC_CHROMA_LOCATION_AS_REFERENCE && mode != JINC_CHROMA_LOCATION_BY_SITING))
        return fail(JINC_ERR_INVALID_ARG, "JincResize: chroma location mode must be 0 or 1.");
    f->chroma_location_mode = mode;
    return JINC_OK;
}

int jinc_filter_get_frame(jinc_filter* f, const void* const src[4], const int src_pitch[4], void* const dst[4],
                          const int dst_pitch[4]) {
    if (!f || !src || !dst || !src_pitch || !dst_pitch) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (f->has_matrix) return fail(JINC_ERR_UNSUPPORTED, kMatrixOnHostFrames);
    if (f->device < 0) return fail(JINC_ERR_NO_DEVICE, "JincResize: filter was created without a HIP device (device < 0).");
    return guarded([&] {
        hip_check(hipSetDevice(f->device), "hipSetDevice");
        drain_pipeline(*f);  // a synchronous frame must not overtake frames still in the pipeline
        wait_frame(*f, submit_frame(*f, src, src_pitch, dst, dst_pitch));
    });
}

int jinc_filter_set_pipeline_group(jinc_filter* f, int depth, int group, int register_host_buffers) {
    if (!f || depth < 1 || depth > kMaxPipelineDepth) return fail(JINC_ERR_INVALID_ARG, "JincResize: pipeline depth must be 1..256.");
    if (group < 0 || group > depth) return fail(JINC_ERR_INVALID_ARG, "JincResize: frames per launch must be 0 (automatic) .. depth.");
    if (f->device < 0) return fail(JINC_ERR_NO_DEVICE, "JincResize: filter was created without a HIP device (device < 0).");
    return guarded([&] {
        hip_check(hipSetDevice(f->device), "hipSetDevice");
        configure_pipeline(*f, depth, group, register_host_buffers);  // 0 staged, 3 the runtime's own mapping, anything else cached registrations
    });
}

int jinc_filter_set_pipeline(jinc_filter* f, int depth, int register_host_buffers) {
    return jinc_filter_set_pipeline_group(f, depth, 0, register_host_buffers);
}

int jinc_filter_pipeline_group(const jinc_filter* f) { return f ? f->group_frames : 0; }

int jinc_filter_submit(jinc_filter* f, const void* const src[4], const int src_pitch[4], void* const dst[4],
                       const int dst_pitch[4], long long* ticket) {
    if (!f || !src || !dst || !src_pitch || !dst_pitch || !ticket) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (f->has_matrix) return fail(JINC_ERR_UNSUPPORTED, kMatrixOnHostFrames);
    if (f->device < 0) return fail(JINC_ERR_NO_DEVICE, "JincResize: filter was created without a HIP device (device < 0).");
    return guarded([&] {
        hip_check(hipSetDevice(f->device), "hipSetDevice");
        *ticket = submit_frame(*f, src, src_pitch, dst, dst_pitch);
    });
}

int jinc_filter_adopt_host_range(jinc_filter* f, void* base, size_t bytes) {
    if (!f || !base || !bytes) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (f->device < 0) return fail(JINC_ERR_NO_DEVICE, "JincResize: filter was created without a HIP device (device < 0).");
    return guarded([&] {
        hip_check(hipSetDevice(f->device), "hipSetDevice");
        adopt_host_range(*f, base, bytes);
    });
}

int jinc_filter_release_host_range(jinc_filter* f, void* base, size_t bytes) {
    if (!f || !base || !bytes) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (f->device < 0) return fail(JINC_ERR_NO_DEVICE, "JincResize: filter was created without a HIP device (device < 0).");
    return guarded([&] {
        hip_check(hipSetDevice(f->device), "hipSetDevice");
        release_host_range(*f, base, bytes);
    });
}

long long jinc_debug_staged_frames(void) { return staged_frames(); }

int jinc_debug_usable_cpus(void) { return copy_lanes_cpus(); }

int jinc_debug_copy_rows(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t row_bytes, int rows, int may_use_helpers) {
    if (!dst || !src || rows < 0 || dst_pitch < row_bytes || src_pitch < row_bytes) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad copy.");
    copy_plane_rows(static_cast<char*>(dst), dst_pitch, static_cast<const char*>(src), src_pitch, row_bytes, rows, may_use_helpers != 0);
    return JINC_OK;
}

int jinc_debug_transport_counts(long long* by_shader, long long* by_dma, long long* pinned_ranges, int reset) {
    transport_counts(by_shader, by_dma, pinned_ranges, reset != 0);
    return JINC_OK;
}

int jinc_filter_flush(jinc_filter* f) {
    if (!f) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (f->device < 0) return fail(JINC_ERR_NO_DEVICE, "JincResize: filter was created without a HIP device (device < 0).");
    return guarded([&] {
        hip_check(hipSetDevice(f->device), "hipSetDevice");
        if (f->open_group >= 0) launch_open_group(*f);
    });
}

int jinc_filter_wait(jinc_filter* f, long long ticket) {
    if (!f) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (f->device < 0) return fail(JINC_ERR_NO_DEVICE, "JincResize: filter was created without a HIP device (device < 0).");
    return guarded([&] {
        hip_check(hipSetDevice(f->device), "hipSetDevice");
        wait_frame(*f, ticket);
    });
}

int jinc_filter_process_device(jinc_filter* f, const void* const src[4], const int src_pitch[4],
                               const size_t src_frame_stride[4], void* const dst[4], const int dst_pitch[4],
                               const size_t dst_frame_stride[4], int nframes, void* hip_stream) {
    if (!f || !src || !dst || !src_pitch || !dst_pitch) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (f->device < 0) return fail(JINC_ERR_NO_DEVICE, "JincResize: filter was created without a HIP device (device < 0).");
    if (nframes < 1 || nframes > 65535) return fail(JINC_ERR_INVALID_ARG, "JincResize: nframes must be in 1..65535.");
    if (nframes > 1 && (!src_frame_stride || !dst_frame_stride))
        return fail(JINC_ERR_INVALID_ARG, "JincResize: frame strides are required for nframes > 1.");
    return guarded([&] {
        hip_check(hipSetDevice(f->device), "hipSetDevice");
        hipStream_t s = static_cast<hipStream_t>(hip_stream);  // NULL = the HIP null stream, ordered with the caller's default-stream work
        reset_matrix_launches();
        enqueue(*f, src, src_pitch, src_frame_stride, dst, dst_pitch, dst_frame_stride, nframes, s);
        apply_output_matrix(*f, dst, dst_pitch, dst_frame_stride, nframes, s);  // (jinc_filter_set_output_matrix; nothing without one)
    });
}

int jinc_filter_process_device_strided(jinc_filter* f, const void* const src[4], const int src_pitch[4], const int src_sample_step[4],
                                       const size_t src_frame_stride[4], void* const dst[4], const int dst_pitch[4],
                                       const int dst_sample_step[4], const size_t dst_frame_stride[4], int nframes, void* hip_stream) {
    return jinc_filter_process_device_shifted(f, src, src_pitch, src_sample_step, nullptr, src_frame_stride, dst, dst_pitch, dst_sample_step,
                                              nullptr, dst_frame_stride, nframes, hip_stream);
}

int jinc_filter_process_device_shifted(jinc_filter* f, const void* const src[4], const int src_pitch[4], const int src_sample_step[4],
                                       const int src_sample_shift[4], const size_t src_frame_stride[4], void* const dst[4],
                                       const int dst_pitch[4], const int dst_sample_step[4], const int dst_sample_shift[4],
                                       const size_t dst_frame_stride[4], int nframes, void* hip_stream) {
    // null checks, the step range and the shift range first (they need no device), then the checks of jinc_filter_process_device in its order
    if (!f || !src || !dst || !src_pitch || !dst_pitch) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    for (const int* step : {src_sample_step, dst_sample_step})
        for (int i = 0; step && i < f->planecount; ++i)
            if (step[i] < 1 || step[i] > 4) return fail(JINC_ERR_INVALID_ARG, "JincResize: sample step must be in 1..4.");
    // A shift is the padding below a sample in its word: integer samples narrower than their container (10 / 12 / 14 bits in 16).
    const bool integer = !f->float_samples();  // (binary16 and bfloat16 fill their 16 bits)
    const int spare = integer ? 8 * f->vi_in.component_size - f->vi_in.bits_per_component : 0;
    for (const int* shift : {src_sample_shift, dst_sample_shift})
        for (int i = 0; shift && i < f->planecount; ++i) {
            if (shift[i] < 0) return fail(JINC_ERR_INVALID_ARG, "JincResize: sample shift must not be negative.");
            if (shift[i] > 0 && spare <= 0)
                return fail(JINC_ERR_INVALID_ARG, "JincResize: a sample shift needs integer samples narrower than their container (10, 12 or 14 bits in 16).");
            if (shift[i] > spare)
                return fail(JINC_ERR_INVALID_ARG, "JincResize: sample shift is larger than the padding of the sample's container (" +
                                                      std::to_string(spare) + " bits).");
        }
    return run_sides(f, true, src_frame_stride && dst_frame_stride,
                     side_of_arrays(f, SideSpec::Planes, src, src_pitch, src_frame_stride, src_sample_step, src_sample_shift),
                     side_of_arrays(f, SideSpec::Planes, dst, dst_pitch, dst_frame_stride, dst_sample_step, dst_sample_shift), nframes, hip_stream);
}

int jinc_filter_process_device_packed10(jinc_filter* f, const void* const src[4], const int src_pitch[4], const int src_field_offset[3],
                                        const size_t src_frame_stride[4], void* const dst[4], const int dst_pitch[4],
                                        const int dst_field_offset[3], unsigned dst_fill, const size_t dst_frame_stride[4], int nframes,
                                        void* hip_stream) {
    // the filter and the offsets first (they need no device), then the checks of jinc_filter_process_device_shifted in its order
    if (!f) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (src_field_offset || dst_field_offset) {
        const bool sides_ok = (!src_field_offset || jinc_filter::side_is_444(f->vi_in)) && (!dst_field_offset || jinc_filter::side_is_444(f->vi_out));
        if (f->planecount != 3 || (!f->converts_chroma() && !sides_ok) || f->float_samples() || f->vi_in.component_size != 2 || f->vi_in.bits_per_component != 10)
            return fail(JINC_ERR_INVALID_ARG, "JincResize: packed 10:10:10:2 words need a filter with three 10-bit components in 16-bit samples and no "
                                              "sub-sampling (YUV444P10, RGBP10).");
        if (src_field_offset && !jinc_filter::side_is_444(f->vi_in))
            return fail(JINC_ERR_INVALID_ARG, refuse_side(f, "packed 10:10:10:2 words", "source", "not sub-sampled (4:4:4)"));
        if (dst_field_offset && !jinc_filter::side_is_444(f->vi_out))
            return fail(JINC_ERR_INVALID_ARG, refuse_side(f, "packed 10:10:10:2 words", "destination", "not sub-sampled (4:4:4)"));
        for (const int* o : {src_field_offset, dst_field_offset}) {
            const std::string refusal = refuse_fields("packed", o, false);
            if (!refusal.empty()) return fail(JINC_ERR_INVALID_ARG, refusal);
        }
    }
    SideSpec in = side_of_arrays(f, src_field_offset ? SideSpec::Words10 : SideSpec::Planes, src, src_pitch, src_frame_stride);
    SideSpec out = side_of_arrays(f, dst_field_offset ? SideSpec::Words10 : SideSpec::Planes, dst, dst_pitch, dst_frame_stride);
    in.fields = src_field_offset, out.fields = dst_field_offset, out.fill = dst_fill;
    return run_sides(f, src && dst && src_pitch && dst_pitch, src_frame_stride && dst_frame_stride, in, out, nframes, hip_stream);
}

int jinc_filter_process_device_v210(jinc_filter* f, const void* const src[4], const int src_pitch[4], int src_is_v210,
                                    const size_t src_frame_stride[4], void* const dst[4], const int dst_pitch[4], int dst_is_v210,
                                    const size_t dst_frame_stride[4], int nframes, void* hip_stream) {
    // the filter first (it needs no device), then the checks of jinc_filter_process_device_shifted in its order
    if (!f) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (src_is_v210 || dst_is_v210) {
        const bool sides_ok = (!src_is_v210 || jinc_filter::side_is_422(f->vi_in)) && (!dst_is_v210 || jinc_filter::side_is_422(f->vi_out));
        if (f->planecount != 3 || (!f->converts_chroma() && !sides_ok) || f->float_samples() || f->vi_in.component_size != 2 ||
            f->vi_in.bits_per_component != 10)
            return fail(JINC_ERR_INVALID_ARG, "JincResize: v210 blocks need a filter with three 10-bit components in 16-bit samples and 4:2:2 "
                                              "sub-sampling (YUV422P10).");
        if (src_is_v210 && !jinc_filter::side_is_422(f->vi_in))
            return fail(JINC_ERR_INVALID_ARG, refuse_side(f, "v210 blocks", "source", "4:2:2 (sub_w 1, sub_h 0)"));
        if (dst_is_v210 && !jinc_filter::side_is_422(f->vi_out))
            return fail(JINC_ERR_INVALID_ARG, refuse_side(f, "v210 blocks", "destination", "4:2:2 (sub_w 1, sub_h 0)"));
    }
    return run_sides(f, src && dst && src_pitch && dst_pitch, src_frame_stride && dst_frame_stride,
                     side_of_arrays(f, src_is_v210 ? SideSpec::V210 : SideSpec::Planes, src, src_pitch, src_frame_stride),
                     side_of_arrays(f, dst_is_v210 ? SideSpec::V210 : SideSpec::Planes, dst, dst_pitch, dst_frame_stride), nframes, hip_stream);
}

namespace {
// jinc_filter_process_device_shifted_packed10 / _v210_packed10: the filter and the offsets first (they need no device).
// `says`: a message, empty when there is nothing to refuse.
void refuse_into_packed10(const jinc_filter* f, bool src_is_v210, const int* dst_field_offset, std::string& says) {
    if (f->planecount != 3 || f->float_samples() || f->vi_in.component_size != 2 || f->vi_in.bits_per_component != 10)
        { says = "JincResize: a packed 10:10:10:2 destination needs a filter with three 10-bit components in 16-bit samples."; return; }
    if (src_is_v210 && !jinc_filter::side_is_422(f->vi_in)) { says = refuse_side(f, "v210 blocks", "source", "4:2:2 (sub_w 1, sub_h 0)"); return; }
    if (!jinc_filter::side_is_444(f->vi_out)) { says = refuse_side(f, "packed 10:10:10:2 words", "destination", "not sub-sampled (4:4:4)"); return; }
    says = refuse_fields("packed", dst_field_offset, false);
}
}  // namespace

int jinc_filter_process_device_shifted_packed10(jinc_filter* f, const void* const src[4], const int src_pitch[4], const int src_sample_step[4],
                                                const int src_sample_shift[4], const size_t src_frame_stride[4], void* dst, int dst_pitch,
                                                const int dst_field_offset[3], unsigned dst_fill, size_t dst_frame_stride, int nframes,
                                                void* hip_stream) {
    if (!f) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    std::string refusal;
    refuse_into_packed10(f, false, dst_field_offset, refusal);
    if (!refusal.empty()) return fail(JINC_ERR_INVALID_ARG, refusal);
    for (int i = 0; src_sample_step && i < 3; ++i)
        if (src_sample_step[i] < 1 || src_sample_step[i] > 4) return fail(JINC_ERR_INVALID_ARG, "JincResize: sample step must be in 1..4.");
    for (int i = 0; src_sample_shift && i < 3; ++i) {
        if (src_sample_shift[i] < 0) return fail(JINC_ERR_INVALID_ARG, "JincResize: sample shift must not be negative.");
        if (src_sample_shift[i] > 6)
            return fail(JINC_ERR_INVALID_ARG, "JincResize: sample shift is larger than the padding of the sample's container (6 bits).");
    }
    SideSpec out = side_of_buffer(SideSpec::Words10, dst, dst_pitch, dst_frame_stride);
    out.fields = dst_field_offset, out.fill = dst_fill;
    return run_sides(f, src && src_pitch && dst && dst_field_offset, src_frame_stride != nullptr,
                     side_of_arrays(f, SideSpec::Planes, src, src_pitch, src_frame_stride, src_sample_step, src_sample_shift), out, nframes, hip_stream);
}

int jinc_filter_process_device_v210_packed10(jinc_filter* f, const void* src, int src_pitch, size_t src_frame_stride, void* dst, int dst_pitch,
                                             const int dst_field_offset[3], unsigned dst_fill, size_t dst_frame_stride, int nframes,
                                             void* hip_stream) {
    if (!f) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    std::string refusal;
    refuse_into_packed10(f, true, dst_field_offset, refusal);
    if (!refusal.empty()) return fail(JINC_ERR_INVALID_ARG, refusal);
    SideSpec out = side_of_buffer(SideSpec::Words10, dst, dst_pitch, dst_frame_stride);
    out.fields = dst_field_offset, out.fill = dst_fill;
    return run_sides(f, src && dst && dst_field_offset, true, side_of_buffer(SideSpec::V210, src, src_pitch, src_frame_stride), out, nframes, hip_stream);
}

size_t jinc_v210_row_bytes(int width) { return v210_row_bytes(width); }

namespace {
// jinc_filter_process_device_widened and, with a scale or an offset array given, jinc_filter_process_device_widened_scaled.
int process_device_widened(jinc_filter* f, const void* const src[4], const int src_pitch[4], const int src_sample_step[4],
                           const int src_sample_shift[4], int src_bits, const float* src_scale, const float* src_offset,
                           const size_t src_frame_stride[4], void* const dst[4], const int dst_pitch[4], const int dst_sample_step[4],
                           const size_t dst_frame_stride[4], int nframes, void* hip_stream) {
    // the filter, src_bits, the steps, the shifts and the source's bases and pitches first (they need no device), then the checks
    // of jinc_filter_process_device_shifted in its order
    const bool scaled = src_scale || src_offset;  // (a defined rounding, no claim of exactness: every depth into every float type)
    if (!f) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (!f->float_samples())
        return fail(JINC_ERR_INVALID_ARG, "JincResize: widened integer sources need an fp32 or binary16 filter, or a bfloat16 filter for 8-bit sources; this filter has " +
                                              std::to_string(f->vi_in.bits_per_component) + "-bit integer samples (use jinc_filter_process_device_shifted).");
    if (src_bits < 8 || src_bits > 16)
        return fail(JINC_ERR_INVALID_ARG, "JincResize: src_bits must be in 8..16 (got " + std::to_string(src_bits) + ").");
    if (!scaled && f->half && src_bits > 11)
        return fail(JINC_ERR_INVALID_ARG, "JincResize: " + std::to_string(src_bits) + "-bit samples are not exact in binary16 (at most 11 bits): "
                                              "widen them into an fp32 filter.");
    if (!scaled && f->bf16 && src_bits > 8)
        return fail(JINC_ERR_INVALID_ARG, "JincResize: " + std::to_string(src_bits) + "-bit samples are not exact in bfloat16 (at most 8 bits): "
                                              "widen them into an fp32 filter.");
    for (const int* step : {src_sample_step, dst_sample_step})
        for (int i = 0; step && i < f->planecount; ++i)
            if (step[i] < 1 || step[i] > 4)
                return fail(JINC_ERR_INVALID_ARG, std::string("JincResize: ") + (step == src_sample_step ? "source" : "destination") +
                                                      " sample step must be in 1..4 (got " + std::to_string(step[i]) + ").");
    const int src_bytes = src_bits > 8 ? 2 : 1, spare = 8 * src_bytes - src_bits;
    for (int i = 0; src_sample_shift && i < f->planecount; ++i) {
        if (src_sample_shift[i] < 0) return fail(JINC_ERR_INVALID_ARG, "JincResize: sample shift must not be negative.");
        if (src_sample_shift[i] > spare)
            return fail(JINC_ERR_INVALID_ARG, "JincResize: sample shift " + std::to_string(src_sample_shift[i]) + " is larger than the padding of a " +
                                                  std::to_string(src_bits) + "-bit sample in its container (" + std::to_string(spare) + " bits).");
    }
    for (int i = 0; src && src_pitch && i < f->planecount; ++i) {
        int w = 0, h = 0;
        f->plane_dims(f->vi_in, i, w, h);
        if (reinterpret_cast<uintptr_t>(src[i]) % static_cast<uintptr_t>(src_bytes))
            return fail(JINC_ERR_INVALID_ARG, "JincResize: source plane pointer is not aligned to the source sample size.");
        const size_t step = static_cast<size_t>(src_sample_step ? src_sample_step[i] : 1);
        const size_t need = (static_cast<size_t>(w - 1) * step + 1) * static_cast<size_t>(src_bytes);
        if (src_pitch[i] < 0 || static_cast<size_t>(src_pitch[i]) < need)
            return fail(JINC_ERR_INVALID_ARG, "JincResize: source pitch " + std::to_string(src_pitch[i]) + " is smaller than the row of " +
                                                  std::to_string(need) + " bytes at this sample step and size.");
    }
    const std::string refusal = refuse_scale_offset("source", src_scale, src_offset, f->planecount);
    if (!refusal.empty()) return fail(JINC_ERR_INVALID_ARG, refusal);
    return run_sides(f, src && dst && src_pitch && dst_pitch, src_frame_stride && dst_frame_stride,
                     converting(side_of_arrays(f, SideSpec::Planes, src, src_pitch, src_frame_stride, src_sample_step, src_sample_shift), src_bits, src_scale, src_offset),
                     side_of_arrays(f, SideSpec::Planes, dst, dst_pitch, dst_frame_stride, dst_sample_step), nframes, hip_stream);
}
}  // namespace

int jinc_filter_process_device_widened(jinc_filter* f, const void* const src[4], const int src_pitch[4], const int src_sample_step[4],
                                       const int src_sample_shift[4], int src_bits, const size_t src_frame_stride[4], void* const dst[4],
                                       const int dst_pitch[4], const int dst_sample_step[4], const size_t dst_frame_stride[4], int nframes,
                                       void* hip_stream) {
    return process_device_widened(f, src, src_pitch, src_sample_step, src_sample_shift, src_bits, nullptr, nullptr, src_frame_stride, dst,
                                  dst_pitch, dst_sample_step, dst_frame_stride, nframes, hip_stream);
}

int jinc_filter_process_device_widened_scaled(jinc_filter* f, const void* const src[4], const int src_pitch[4],
                                              const int src_sample_step[4], const int src_sample_shift[4], int src_bits,
                                              const float src_scale[4], const float src_offset[4], const size_t src_frame_stride[4],
                                              void* const dst[4], const int dst_pitch[4], const int dst_sample_step[4],
                                              const size_t dst_frame_stride[4], int nframes, void* hip_stream) {
    return process_device_widened(f, src, src_pitch, src_sample_step, src_sample_shift, src_bits, src_scale, src_offset, src_frame_stride,
                                  dst, dst_pitch, dst_sample_step, dst_frame_stride, nframes, hip_stream);
}

namespace {
// jinc_filter_process_device_narrowed and, with a scale or an offset array given, jinc_filter_process_device_narrowed_scaled.
int process_device_narrowed(jinc_filter* f, const void* const src[4], const int src_pitch[4], const int src_sample_step[4],
                            const size_t src_frame_stride[4], void* const dst[4], const int dst_pitch[4], const int dst_sample_step[4],
                            const int dst_sample_shift[4], int dst_bits, const float* dst_scale, const float* dst_offset,
                            const size_t dst_frame_stride[4], int nframes, void* hip_stream) {
    // the filter, dst_bits, the steps, the shifts and the destination's bases and pitches first (they need no device), then the
    // checks of jinc_filter_process_device_shifted in its order
    if (!f) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (!f->float_samples())
        return fail(JINC_ERR_INVALID_ARG, "JincResize: narrowed integer destinations need an fp32, binary16 or bfloat16 filter; this filter has " +
                                              std::to_string(f->vi_in.bits_per_component) + "-bit integer samples (use jinc_filter_process_device_shifted).");
    if (dst_bits < 8 || dst_bits > 16)
        return fail(JINC_ERR_INVALID_ARG, "JincResize: dst_bits must be in 8..16 (got " + std::to_string(dst_bits) + ").");
    for (const int* step : {src_sample_step, dst_sample_step})
        for (int i = 0; step && i < f->planecount; ++i)
            if (step[i] < 1 || step[i] > 4)
                return fail(JINC_ERR_INVALID_ARG, std::string("JincResize: ") + (step == src_sample_step ? "source" : "destination") +
                                                      " sample step of a narrowed call must be in 1..4 (got " + std::to_string(step[i]) + ").");
    const int dst_bytes = dst_bits > 8 ? 2 : 1, spare = 8 * dst_bytes - dst_bits;
    for (int i = 0; dst_sample_shift && i < f->planecount; ++i) {
        if (dst_sample_shift[i] < 0) return fail(JINC_ERR_INVALID_ARG, "JincResize: destination sample shift must not be negative.");
        if (dst_sample_shift[i] > spare)
            return fail(JINC_ERR_INVALID_ARG, "JincResize: destination sample shift " + std::to_string(dst_sample_shift[i]) + " is larger than the padding of a " +
                                                  std::to_string(dst_bits) + "-bit sample in its container (" + std::to_string(spare) + " bits).");
    }
    for (int i = 0; dst && dst_pitch && i < f->planecount; ++i) {
        int w = 0, h = 0;
        f->plane_dims(f->vi_out, i, w, h);
        if (reinterpret_cast<uintptr_t>(dst[i]) % static_cast<uintptr_t>(dst_bytes))
            return fail(JINC_ERR_INVALID_ARG, "JincResize: destination plane pointer is not aligned to the destination sample size.");
        const size_t step = static_cast<size_t>(dst_sample_step ? dst_sample_step[i] : 1);
        const size_t need = (static_cast<size_t>(w - 1) * step + 1) * static_cast<size_t>(dst_bytes);
        if (dst_pitch[i] < 0 || static_cast<size_t>(dst_pitch[i]) < need)
            return fail(JINC_ERR_INVALID_ARG, "JincResize: destination pitch " + std::to_string(dst_pitch[i]) + " is smaller than the row of " +
                                                  std::to_string(need) + " bytes at this sample step and size.");
    }
    const std::string refusal = refuse_scale_offset("destination", dst_scale, dst_offset, f->planecount);
    if (!refusal.empty()) return fail(JINC_ERR_INVALID_ARG, refusal);
    return run_sides(f, src && dst && src_pitch && dst_pitch, src_frame_stride && dst_frame_stride,
                     side_of_arrays(f, SideSpec::Planes, src, src_pitch, src_frame_stride, src_sample_step),
                     converting(side_of_arrays(f, SideSpec::Planes, dst, dst_pitch, dst_frame_stride, dst_sample_step, dst_sample_shift), dst_bits, dst_scale, dst_offset),
                     nframes, hip_stream);
}
}  // namespace

int jinc_filter_process_device_narrowed(jinc_filter* f, const void* const src[4], const int src_pitch[4], const int src_sample_step[4],
                                        const size_t src_frame_stride[4], void* const dst[4], const int dst_pitch[4],
                                        const int dst_sample_step[4], const int dst_sample_shift[4], int dst_bits,
                                        const size_t dst_frame_stride[4], int nframes, void* hip_stream) {
    return process_device_narrowed(f, src, src_pitch, src_sample_step, src_frame_stride, dst, dst_pitch, dst_sample_step, dst_sample_shift,
                                   dst_bits, nullptr, nullptr, dst_frame_stride, nframes, hip_stream);
}

int jinc_filter_process_device_narrowed_scaled(jinc_filter* f, const void* const src[4], const int src_pitch[4],
                                               const int src_sample_step[4], const size_t src_frame_stride[4], void* const dst[4],
                                               const int dst_pitch[4], const int dst_sample_step[4], const int dst_sample_shift[4],
                                               int dst_bits, const float dst_scale[4], const float dst_offset[4],
                                               const size_t dst_frame_stride[4], int nframes, void* hip_stream) {
    return process_device_narrowed(f, src, src_pitch, src_sample_step, src_frame_stride, dst, dst_pitch, dst_sample_step, dst_sample_shift,
                                   dst_bits, dst_scale, dst_offset, dst_frame_stride, nframes, hip_stream);
}

int jinc_code_range(int bits, int range, int plane_kind, float* to_float_scale, float* to_float_offset, float* to_code_scale,
                    float* to_code_offset) {
    if (bits < 8 || bits > 16) return fail(JINC_ERR_INVALID_ARG, "JincResize: bits of a code range must be in 8..16 (got " + std::to_string(bits) + ").");
    if (range != JINC_RANGE_FULL && range != JINC_RANGE_LIMITED)
        return fail(JINC_ERR_INVALID_ARG, "JincResize: the range of a code range must be JINC_RANGE_FULL or JINC_RANGE_LIMITED.");
    if (plane_kind != JINC_PLANE_LUMA_OR_RGB && plane_kind != JINC_PLANE_CHROMA)
        return fail(JINC_ERR_INVALID_ARG, "JincResize: the plane kind of a code range must be JINC_PLANE_LUMA_OR_RGB or JINC_PLANE_CHROMA.");
    const bool chroma = plane_kind == JINC_PLANE_CHROMA;
    const int k = 1 << (bits - 8);
    const int den = range == JINC_RANGE_LIMITED ? (chroma ? 224 : 219) * k : (1 << bits) - 1;
    const int zero = range == JINC_RANGE_LIMITED ? (chroma ? 128 : 16) * k : (chroma ? 1 << (bits - 1) : 0);
    if (to_float_scale) *to_float_scale = static_cast<float>(1.0 / den);  // (computed in double, rounded once)
    if (to_float_offset) *to_float_offset = static_cast<float>(-static_cast<double>(zero) / den);
    if (to_code_scale) *to_code_scale = static_cast<float>(den);  // (exact: below 2^24)
    if (to_code_offset) *to_code_offset = static_cast<float>(zero);
    return JINC_OK;
}

namespace {
// jinc_filter_process_device_widened_packed10 and, with a scale or an offset array given, jinc_filter_process_device_widened_packed10_scaled.
int process_device_widened_packed10(jinc_filter* f, const void* src, int src_pitch, const int src_field_offset[3], const float* src_scale,
                                    const float* src_offset, size_t src_frame_stride, void* const dst[4], const int dst_pitch[4],
                                    const int dst_sample_step[4], const size_t dst_frame_stride[4], int nframes, void* hip_stream) {
    // the filter, the offsets, the destination steps, the source's base, pitch and frame stride and the pairs first (they need no
    // device), then the checks of jinc_filter_process_device_shifted in its order
    const bool scaled = src_scale || src_offset;  // (a defined rounding, no claim of exactness: bfloat16 filters too)
    if (!f) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (!f->float_samples())
        return fail(JINC_ERR_INVALID_ARG, "JincResize: widened packed 10:10:10:2 words need an fp32 or binary16 filter; this filter has " +
                                              std::to_string(f->vi_in.bits_per_component) + "-bit integer samples (use jinc_filter_process_device_packed10).");
    if (!scaled && f->bf16)
        return fail(JINC_ERR_INVALID_ARG, "JincResize: widened packed 10:10:10:2 words do not go into a bfloat16 filter: 10-bit fields are not exact in "
                                          "bfloat16 (at most 8 bits); widen them into an fp32 or binary16 filter.");
    if (f->planecount == 3 && f->converts_chroma() && !jinc_filter::side_is_444(f->vi_in))
        return fail(JINC_ERR_INVALID_ARG, refuse_side(f, "widened packed 10:10:10:2 words", "source", "not sub-sampled (4:4:4)"));
    if (f->planecount != 3 || !jinc_filter::side_is_444(f->vi_in))
        return fail(JINC_ERR_INVALID_ARG, "JincResize: widened packed 10:10:10:2 words need a float filter with three components and no sub-sampling "
                                          "(YUV444PS, YUV444PH, RGBPS, RGBPH); this filter has " + std::to_string(f->planecount) + " component(s), sub_w " +
                                              std::to_string(f->vi_in.sub_w) + " and sub_h " + std::to_string(f->vi_in.sub_h) + ".");
    std::string refusal = refuse_fields("widened packed", src_field_offset, true);
    int w = 0, h = 0;
    f->plane_dims(f->vi_in, 0, w, h);
    if (refusal.empty())
        refusal = refuse_words(f, "widened", "destination", "packed 10-bit words", src, src_pitch, src_frame_stride, 4 * static_cast<size_t>(w),
                               "4 * width", dst_sample_step, nframes);
    if (refusal.empty()) refusal = refuse_scale_offset("packed 10-bit source", src_scale, src_offset, 3);
    if (!refusal.empty()) return fail(JINC_ERR_INVALID_ARG, refusal);
    SideSpec in = converting(side_of_buffer(SideSpec::Words10, src, src_pitch, src_frame_stride), 10, src_scale, src_offset);
    in.fields = src_field_offset;
    return run_sides(f, src && src_field_offset && dst && dst_pitch, dst_frame_stride != nullptr, in,
                     side_of_arrays(f, SideSpec::Planes, dst, dst_pitch, dst_frame_stride, dst_sample_step), nframes, hip_stream);
}
}  // namespace

int jinc_filter_process_device_widened_packed10(jinc_filter* f, const void* src, int src_pitch, const int src_field_offset[3],
                                                size_t src_frame_stride, void* const dst[4], const int dst_pitch[4],
                                                const int dst_sample_step[4], const size_t dst_frame_stride[4], int nframes,
                                                void* hip_stream) {
    return process_device_widened_packed10(f, src, src_pitch, src_field_offset, nullptr, nullptr, src_frame_stride, dst, dst_pitch,
                                           dst_sample_step, dst_frame_stride, nframes, hip_stream);
}

int jinc_filter_process_device_widened_packed10_scaled(jinc_filter* f, const void* src, int src_pitch, const int src_field_offset[3],
                                                       const float src_scale[3], const float src_offset[3], size_t src_frame_stride,
                                                       void* const dst[4], const int dst_pitch[4], const int dst_sample_step[4],
                                                       const size_t dst_frame_stride[4], int nframes, void* hip_stream) {
    return process_device_widened_packed10(f, src, src_pitch, src_field_offset, src_scale, src_offset, src_frame_stride, dst, dst_pitch,
                                           dst_sample_step, dst_frame_stride, nframes, hip_stream);
}

namespace {
// jinc_filter_process_device_widened_v210 and, with a scale or an offset array given, jinc_filter_process_device_widened_v210_scaled.
int process_device_widened_v210(jinc_filter* f, const void* src, int src_pitch, const float* src_scale, const float* src_offset,
                                size_t src_frame_stride, void* const dst[4], const int dst_pitch[4], const int dst_sample_step[4],
                                const size_t dst_frame_stride[4], int nframes, void* hip_stream) {
    // the filter, the destination steps, the source's base, pitch and frame stride and the pairs first (they need no device), then
    // the checks of jinc_filter_process_device_shifted in its order
    const bool scaled = src_scale || src_offset;  // (a defined rounding, no claim of exactness: bfloat16 filters too)
    if (!f) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (!f->float_samples())
        return fail(JINC_ERR_INVALID_ARG, "JincResize: widened v210 blocks need an fp32 or binary16 filter; this filter has " +
                                              std::to_string(f->vi_in.bits_per_component) + "-bit integer samples (use jinc_filter_process_device_v210).");
    if (!scaled && f->bf16)
        return fail(JINC_ERR_INVALID_ARG, "JincResize: widened v210 blocks do not go into a bfloat16 filter: 10-bit samples are not exact in bfloat16 "
                                          "(at most 8 bits); widen them into an fp32 or binary16 filter.");
    if (f->planecount == 3 && f->converts_chroma() && !jinc_filter::side_is_422(f->vi_in))
        return fail(JINC_ERR_INVALID_ARG, refuse_side(f, "widened v210 blocks", "source", "4:2:2 (sub_w 1, sub_h 0)"));
    if (f->planecount != 3 || !jinc_filter::side_is_422(f->vi_in))
        return fail(JINC_ERR_INVALID_ARG, "JincResize: widened v210 blocks need a float filter with three components and 4:2:2 sub-sampling "
                                          "(YUV422PS, YUV422PH: sub_w 1, sub_h 0); this filter has " + std::to_string(f->planecount) + " component(s), sub_w " +
                                              std::to_string(f->vi_in.sub_w) + " and sub_h " + std::to_string(f->vi_in.sub_h) + ".");
    int w = 0, h = 0;
    f->plane_dims(f->vi_in, 0, w, h);
    std::string refusal = refuse_words(f, "widened", "destination", "v210 blocks", src, src_pitch, src_frame_stride, v210_row_bytes(w),
                                       "16 * ceil(width / 6)", dst_sample_step, nframes);
    if (refusal.empty()) refusal = refuse_scale_offset("v210 source", src_scale, src_offset, 3);
    if (!refusal.empty()) return fail(JINC_ERR_INVALID_ARG, refusal);
    return run_sides(f, src && dst && dst_pitch, dst_frame_stride != nullptr,
                     converting(side_of_buffer(SideSpec::V210, src, src_pitch, src_frame_stride), 10, src_scale, src_offset),
                     side_of_arrays(f, SideSpec::Planes, dst, dst_pitch, dst_frame_stride, dst_sample_step), nframes, hip_stream);
}
}  // namespace

int jinc_filter_process_device_widened_v210(jinc_filter* f, const void* src, int src_pitch, size_t src_frame_stride, void* const dst[4],
                                            const int dst_pitch[4], const int dst_sample_step[4], const size_t dst_frame_stride[4],
                                            int nframes, void* hip_stream) {
    return process_device_widened_v210(f, src, src_pitch, nullptr, nullptr, src_frame_stride, dst, dst_pitch, dst_sample_step, dst_frame_stride,
                                       nframes, hip_stream);
}

int jinc_filter_process_device_widened_v210_scaled(jinc_filter* f, const void* src, int src_pitch, const float src_scale[3],
                                                   const float src_offset[3], size_t src_frame_stride, void* const dst[4],
                                                   const int dst_pitch[4], const int dst_sample_step[4], const size_t dst_frame_stride[4],
                                                   int nframes, void* hip_stream) {
    return process_device_widened_v210(f, src, src_pitch, src_scale, src_offset, src_frame_stride, dst, dst_pitch, dst_sample_step,
                                       dst_frame_stride, nframes, hip_stream);
}

int jinc_filter_process_device_narrowed_packed10(jinc_filter* f, const void* const src[4], const int src_pitch[4],
                                                 const int src_sample_step[4], const size_t src_frame_stride[4], void* dst, int dst_pitch,
                                                 const int dst_field_offset[3], unsigned dst_fill, const float dst_scale[3],
                                                 const float dst_offset[3], size_t dst_frame_stride, int nframes, void* hip_stream) {
    // the filter, the offsets, the source steps, the destination's base, pitch and frame stride and the scales first (they need no
    // device), then the checks of jinc_filter_process_device_shifted in its order
    if (!f) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (!f->float_samples())
        return fail(JINC_ERR_INVALID_ARG, "JincResize: narrowed packed 10:10:10:2 words need an fp32, binary16 or bfloat16 filter; this filter has " +
                                              std::to_string(f->vi_in.bits_per_component) + "-bit integer samples (use jinc_filter_process_device_packed10).");
    if (f->planecount == 3 && f->converts_chroma() && !jinc_filter::side_is_444(f->vi_out))
        return fail(JINC_ERR_INVALID_ARG, refuse_side(f, "narrowed packed 10:10:10:2 words", "destination", "not sub-sampled (4:4:4)"));
    if (f->planecount != 3 || !jinc_filter::side_is_444(f->vi_out))
        return fail(JINC_ERR_INVALID_ARG, "JincResize: narrowed packed 10:10:10:2 words need a float filter with three components and no sub-sampling "
                                          "(YUV444PS, YUV444PH, RGBPS, RGBPH and their bfloat16 twins); this filter has " + std::to_string(f->planecount) +
                                              " component(s), sub_w " + std::to_string(f->vi_in.sub_w) + " and sub_h " + std::to_string(f->vi_in.sub_h) + ".");
    std::string refusal = refuse_fields("narrowed packed", dst_field_offset, true);
    int w = 0, h = 0;
    f->plane_dims(f->vi_out, 0, w, h);
    if (refusal.empty())
        refusal = refuse_words(f, "narrowed", "source", "packed 10-bit words", dst, dst_pitch, dst_frame_stride, 4 * static_cast<size_t>(w), "4 * width",
                               src_sample_step, nframes);
    if (refusal.empty()) refusal = refuse_scale_offset("packed 10-bit destination", dst_scale, dst_offset, 3);
    if (!refusal.empty()) return fail(JINC_ERR_INVALID_ARG, refusal);
    SideSpec out = converting(side_of_buffer(SideSpec::Words10, dst, dst_pitch, dst_frame_stride), 10, dst_scale, dst_offset);
    out.fields = dst_field_offset, out.fill = dst_fill;
    return run_sides(f, src && src_pitch && dst && dst_field_offset, src_frame_stride != nullptr,
                     side_of_arrays(f, SideSpec::Planes, src, src_pitch, src_frame_stride, src_sample_step), out, nframes, hip_stream);
}

int jinc_filter_process_device_narrowed_v210(jinc_filter* f, const void* const src[4], const int src_pitch[4], const int src_sample_step[4],
                                             const size_t src_frame_stride[4], void* dst, int dst_pitch, const float dst_scale[3],
                                             const float dst_offset[3], size_t dst_frame_stride, int nframes, void* hip_stream) {
    // the filter, the source steps, the destination's base, pitch and frame stride and the scales first (they need no device), then
    // the checks of jinc_filter_process_device_shifted in its order
    if (!f) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (!f->float_samples())
        return fail(JINC_ERR_INVALID_ARG, "JincResize: narrowed v210 blocks need an fp32, binary16 or bfloat16 filter; this filter has " +
                                              std::to_string(f->vi_in.bits_per_component) + "-bit integer samples (use jinc_filter_process_device_v210).");
    if (f->planecount == 3 && f->converts_chroma() && !jinc_filter::side_is_422(f->vi_out))
        return fail(JINC_ERR_INVALID_ARG, refuse_side(f, "narrowed v210 blocks", "destination", "4:2:2 (sub_w 1, sub_h 0)"));
    if (f->planecount != 3 || !jinc_filter::side_is_422(f->vi_out))
        return fail(JINC_ERR_INVALID_ARG, "JincResize: narrowed v210 blocks need a float filter with three components and 4:2:2 sub-sampling "
                                          "(YUV422PS, YUV422PH and their bfloat16 twin: sub_w 1, sub_h 0); this filter has " + std::to_string(f->planecount) +
                                              " component(s), sub_w " + std::to_string(f->vi_in.sub_w) + " and sub_h " + std::to_string(f->vi_in.sub_h) + ".");
    int w = 0, h = 0;
    f->plane_dims(f->vi_out, 0, w, h);
    std::string refusal = refuse_words(f, "narrowed", "source", "v210 blocks", dst, dst_pitch, dst_frame_stride, v210_row_bytes(w),
                                       "16 * ceil(width / 6)", src_sample_step, nframes);
    if (refusal.empty()) refusal = refuse_scale_offset("v210 destination", dst_scale, dst_offset, 3);
    if (!refusal.empty()) return fail(JINC_ERR_INVALID_ARG, refusal);
    return run_sides(f, src && src_pitch && dst, src_frame_stride != nullptr,
                     side_of_arrays(f, SideSpec::Planes, src, src_pitch, src_frame_stride, src_sample_step),
                     converting(side_of_buffer(SideSpec::V210, dst, dst_pitch, dst_frame_stride), 10, dst_scale, dst_offset), nframes, hip_stream);
}

int jinc_packed10_layout(const char* name, int field_offset[3], unsigned* opaque_fill) {
    // offsets of the library's planes (Y, U, V or G, B, R) in the word
    static const struct {
        const char* name;
        int offset[3];
    } kLayouts[] = {
        {"Y410", {10, 0, 20}},         // U 0, Y 10, V 20, A 30
        {"R10G10B10A2", {10, 20, 0}},  // DXGI: R 0, G 10, B 20, A 30
        {"ABGR2101010", {10, 20, 0}},  // DRM names list the components from the high bits down
        {"XBGR2101010", {10, 20, 0}},
        {"ARGB2101010", {10, 0, 20}},
        {"XRGB2101010", {10, 0, 20}},
        {"RGBA1010102", {12, 2, 22}},
        {"RGBX1010102", {12, 2, 22}},
        {"BGRA1010102", {12, 22, 2}},
        {"BGRX1010102", {12, 22, 2}},
    };
    if (!name || !field_offset) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    for (const auto& l : kLayouts) {
        size_t k = 0;
        while (name[k] && l.name[k] && std::toupper(static_cast<unsigned char>(name[k])) == l.name[k]) ++k;
        if (name[k] || l.name[k]) continue;
        unsigned fields = 0;
        for (int i = 0; i < 3; ++i) field_offset[i] = l.offset[i], fields |= 1023u << l.offset[i];
        if (opaque_fill) *opaque_fill = ~fields;
        return JINC_OK;
    }
    return fail(JINC_ERR_INVALID_ARG, std::string("JincResize: unknown packed 10:10:10:2 layout \"") + name + "\".");
}

int jinc_debug_strided_groups(const void* const base[4], const int pitch[4], const int step[4], const size_t frame_stride[4],
                              const int width[4], const int height[4], int component_size, int nplanes, int group_of[4], int channel_of[4]) {
    if (!base || !pitch || !width || !height || !group_of || !channel_of || nplanes < 0 || nplanes > 4 ||
        (component_size != 1 && component_size != 2 && component_size != 4))
        return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    return strided_groups(base, pitch, step, frame_stride, width, height, component_size, nplanes, group_of, channel_of);
}

int jinc_debug_last_strided(int* split_launches, int* merge_launches, int* slices, long long* scratch_bytes) {
    const StridedReport& r = last_strided_report();
    if (split_launches) *split_launches = r.split_launches;
    if (merge_launches) *merge_launches = r.merge_launches;
    if (slices) *slices = r.slices;
    if (scratch_bytes) *scratch_bytes = r.scratch_bytes;
    return JINC_OK;
}

int jinc_debug_plane_extent_check(jinc_filter* f, const int src_pitch[4], const int dst_pitch[4]) {
    if (!f || !src_pitch || !dst_pitch) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    for (int i = 0; i < f->planecount; ++i) {
        const jinc::TableGeometry& g = f->plans[static_cast<size_t>(f->table_of_plane(i))].g;
        if (const char* says = plane_size_refusal(src_pitch[i], g.src_w, g.src_h, dst_pitch[i], g.dst_h, f->vi_in.component_size))
            return fail(JINC_ERR_INVALID_ARG, says);
    }
    return JINC_OK;
}

int jinc_debug_last_groups(jinc_group_info* groups, int capacity) {
    const GroupsReport& r = last_groups_report();
    for (int i = 0; groups && i < r.count && i < capacity; ++i) {
        const GroupRecord& g = r.g[i];
        groups[i].direction = g.direction, groups[i].n = g.step, groups[i].members = g.members, groups[i].sample_bytes = g.sample_bytes;
        groups[i].sample_type = g.sample_type, groups[i].scaled = g.scaled;
        groups[i].unit = static_cast<int>(g.unit), groups[i].vec_pixels = static_cast<int>(g.vec_pixels);
        groups[i].width = static_cast<int>(g.width), groups[i].rows = static_cast<int>(g.rows);
        groups[i].shifted = g.shifted;
    }
    return r.count;
}

int jinc_filter_sync(jinc_filter* f) {
    if (!f) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (f->device < 0) return fail(JINC_ERR_NO_DEVICE, "JincResize: filter was created without a HIP device (device < 0).");
    return guarded([&] {
        hip_check(hipSetDevice(f->device), "hipSetDevice");
        drain_pipeline(*f);
        hip_check(hipStreamSynchronize(f->stream), "stream sync");
    });
}

int jinc_alias_args(int taps, const jinc_args* in, jinc_args* out) {
    if (!in || !out) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (taps != 3 && taps != 4 && taps != 6 && taps != 8)
        return fail(JINC_ERR_INVALID_ARG, "JincResize: alias tap count must be 3, 4, 6 or 8.");
    jinc_args a{};
    a.target_width = in->target_width;
    a.target_height = in->target_height;
    const unsigned forwarded = JINC_ARG_SRC_LEFT | JINC_ARG_SRC_TOP | JINC_ARG_SRC_WIDTH | JINC_ARG_SRC_HEIGHT |
                               JINC_ARG_QUANT_X | JINC_ARG_QUANT_Y | JINC_ARG_CPLACE | JINC_ARG_THREADS;
    a.defined = (in->defined & forwarded) | JINC_ARG_TAP;
    a.src_left = in->src_left;
    a.src_top = in->src_top;
    a.src_width = in->src_width;
    a.src_height = in->src_height;
    a.quant_x = in->quant_x;
    a.quant_y = in->quant_y;
    a.cplace = in->cplace;
    a.threads = in->threads;
    a.tap = taps;
    a.frame0_chroma_location = in->frame0_chroma_location;
    a.cpu_has_sse41 = in->cpu_has_sse41;
    a.cpu_has_avx2 = in->cpu_has_avx2;
    a.cpu_has_avx512f = in->cpu_has_avx512f;
    *out = a;
    return JINC_OK;
}

int jinc_filter_num_tables(const jinc_filter* f) { return f ? static_cast<int>(f->plans.size()) : 0; }

int jinc_filter_plan_info(const jinc_filter* f, int table, jinc_plan_info* out) {
    const jinc::PlanePlan* p = table_or_null(f, table);
    if (!p || !out) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad table index.");
    jinc_plan_info i{};
    i.src_width = p->g.src_w;
    i.src_height = p->g.src_h;
    i.dst_width = p->g.dst_w;
    i.dst_height = p->g.dst_h;
    i.filter_size = p->fs;
    i.num_sets = p->num_sets;
    i.periodic = p->periodic ? 1 : 0;
    i.period_x = p->px;
    i.period_y = p->py;
    i.step_x = p->sx;
    i.step_y = p->sy;
    i.interior_x0 = p->ix0;
    i.interior_x1 = p->ix1;
    i.interior_y0 = p->iy0;
    i.interior_y1 = p->iy1;
    i.plan_bytes = static_cast<int64_t>(4) * (p->col_start.size() + p->row_start.size() + p->col_class.size() +
                                              p->row_class.size() + p->interior_set.size() + p->bcol_set.size() +
                                              p->brow_set.size() + p->coeffs.size());
    i.quasi = p->quasi ? 1 : 0;
    i.quasi_period_x = p->qpx;
    i.quasi_period_y = p->qpy;
    i.quasi_step_x = p->qsx;
    i.quasi_step_y = p->qsy;
    *out = i;
    return JINC_OK;
}

int jinc_filter_plan_pixel(const jinc_filter* f, int table, int x, int y, int* start_x, int* start_y, float* coeffs) {
    const jinc::PlanePlan* p = table_or_null(f, table);
    if (!p || x < 0 || y < 0 || x >= p->g.dst_w || y >= p->g.dst_h)
        return fail(JINC_ERR_INVALID_ARG, "JincResize: bad table index or pixel.");
    if (start_x) *start_x = p->col_start[x];
    if (start_y) *start_y = p->row_start[y];
    if (coeffs) std::memcpy(coeffs, p->set_ptr(p->set_of(x, y)), sizeof(float) * p->fs * p->fs);
    return JINC_OK;
}

int jinc_filter_plan_dump(const jinc_filter* f, int table, int* start_x, int* start_y, int* set_id) {
    const jinc::PlanePlan* p = table_or_null(f, table);
    if (!p) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad table index.");
    if (start_x) std::memcpy(start_x, p->col_start.data(), sizeof(int) * p->g.dst_w);
    if (start_y) std::memcpy(start_y, p->row_start.data(), sizeof(int) * p->g.dst_h);
    if (set_id)
        for (int y = 0; y < p->g.dst_h; ++y)
            for (int x = 0; x < p->g.dst_w; ++x) set_id[static_cast<size_t>(y) * p->g.dst_w + x] = p->set_of(x, y);
    return JINC_OK;
}

int jinc_filter_plan_runs(const jinc_filter* f, int table, int* n_runs, int* n_items, int32_t* runs, int capacity) {
    const jinc::PlanePlan* p = table_or_null(f, table);
    if (!p || !n_runs || !n_items) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad table index or null argument.");
    std::vector<jinc::PlanRun> list;
    std::vector<int32_t> item_run;
    if (!jinc::build_plan_runs(*p, list, item_run)) list.clear(), item_run.clear();
    *n_runs = static_cast<int>(list.size());
    *n_items = static_cast<int>(item_run.size());
    if (runs && capacity > 0)
        std::memcpy(runs, list.data(), sizeof(jinc::PlanRun) * std::min<size_t>(list.size(), static_cast<size_t>(capacity)));
    return JINC_OK;
}

int jinc_filter_plan_set(const jinc_filter* f, int table, int set, float* coeffs) {
    const jinc::PlanePlan* p = table_or_null(f, table);
    if (!p || !coeffs || set < 0 || set >= p->num_sets) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad table or set index.");
    std::memcpy(coeffs, p->set_ptr(set), sizeof(float) * p->fs * p->fs);
    return JINC_OK;
}

int jinc_filter_lut(const jinc_filter* f, double* lut1024) {
    if (!f || !lut1024) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    std::memcpy(lut1024, f->lut.v.data(), sizeof(double) * jinc::kLutSamples);
    return JINC_OK;
}

int jinc_filter_set_profiling(jinc_filter* f, int enable) {
    if (!f) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    f->profiling = enable != 0;
    return JINC_OK;
}

int jinc_filter_kernel_times(jinc_filter* f, double* periodic_ms, int* periodic_launches, double* gather_ms,
                             int* gather_launches) {
    if (!f) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (f->device < 0) return fail(JINC_ERR_NO_DEVICE, "JincResize: filter was created without a HIP device (device < 0).");
    return guarded([&] {
        hip_check(hipSetDevice(f->device), "hipSetDevice");
        auto collect = [](std::vector<EventPair>& v, double* ms_out, int* n_out) {
            double total = 0.0;
            for (auto& e : v) {
                hip_check(hipEventSynchronize(e.stop), "hipEventSynchronize");
                float ms = 0.f;
                hip_check(hipEventElapsedTime(&ms, e.start, e.stop), "hipEventElapsedTime");
                total += ms;
                (void)hipEventDestroy(e.start);
                (void)hipEventDestroy(e.stop);
            }
            if (ms_out) *ms_out = total;
            if (n_out) *n_out = static_cast<int>(v.size());
            v.clear();
        };
        collect(f->ev_periodic, periodic_ms, periodic_launches);
        collect(f->ev_gather, gather_ms, gather_launches);
    });
}

int jinc_debug_convert_half(const float* sums, uint16_t* out, int n, int device) {
    if (!sums || !out || n < 0) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    return guarded([&] {
        hip_check(hipSetDevice(device), "hipSetDevice");
        float* d_in = nullptr;
        uint16_t* d_out = nullptr;
        hip_check(hipMalloc(&d_in, sizeof(float) * (n + 1)), "hipMalloc");
        hip_check(hipMalloc(&d_out, sizeof(uint16_t) * (n + 1)), "hipMalloc");
        bounce_upload(d_in, sums, sizeof(float) * n, "upload of the sums");
        hip_check(static_cast<hipError_t>(jinc::launch_debug_convert_half(d_in, d_out, n, nullptr)), "convert launch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        bounce_download(out, d_out, sizeof(uint16_t) * n, "download of the samples");
        (void)hipFree(d_in);
        (void)hipFree(d_out);
    });
}

int jinc_debug_convert_bfloat16(const float* sums, uint16_t* out, int n, int device) {
    if (!sums || !out || n < 0) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    return guarded([&] {
        hip_check(hipSetDevice(device), "hipSetDevice");
        float* d_in = nullptr;
        uint16_t* d_out = nullptr;
        hip_check(hipMalloc(&d_in, sizeof(float) * (n + 1)), "hipMalloc");
        hip_check(hipMalloc(&d_out, sizeof(uint16_t) * (n + 1)), "hipMalloc");
        bounce_upload(d_in, sums, sizeof(float) * n, "upload of the sums");
        hip_check(static_cast<hipError_t>(jinc::launch_debug_convert_bfloat16(d_in, d_out, n, nullptr)), "convert launch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        bounce_download(out, d_out, sizeof(uint16_t) * n, "download of the samples");
        (void)hipFree(d_in);
        (void)hipFree(d_out);
    });
}

int jinc_debug_convert(const float* sums, void* out, int n, int sample_bytes, float peak, int device) {
    if (!sums || !out || n < 0 || (sample_bytes != 1 && sample_bytes != 2 && sample_bytes != 4))
        return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    return guarded([&] {
        hip_check(hipSetDevice(device), "hipSetDevice");
        float* d_in = nullptr;
        void* d_out = nullptr;
        hip_check(hipMalloc(&d_in, sizeof(float) * (n + 1)), "hipMalloc");
        hip_check(hipMalloc(&d_out, static_cast<size_t>(sample_bytes) * (n + 1)), "hipMalloc");
        bounce_upload(d_in, sums, sizeof(float) * n, "upload of the sums");
        hip_check(static_cast<hipError_t>(jinc::launch_debug_convert(d_in, d_out, n, sample_bytes, peak, nullptr)), "convert launch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        bounce_download(out, d_out, static_cast<size_t>(sample_bytes) * n, "download of the samples");
        (void)hipFree(d_in);
        (void)hipFree(d_out);
    });
}

int jinc_debug_narrow(const void* in, int in_kind, void* out, int n, int dst_bits, int shift, int device) {
    const bool kind_ok = in_kind == JINC_SAMPLE_DEFAULT || in_kind == JINC_SAMPLE_FLOAT16 || in_kind == JINC_SAMPLE_BFLOAT16;
    if (!in || !out || n < 0 || !kind_ok || dst_bits < 8 || dst_bits > 16) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    const size_t in_bytes = in_kind == JINC_SAMPLE_DEFAULT ? 4 : 2, dst_bytes = dst_bits > 8 ? 2 : 1;
    if (shift < 0 || shift > static_cast<int>(8 * dst_bytes) - dst_bits) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    if (n == 0) return JINC_OK;
    return guarded([&] {
        hip_check(hipSetDevice(device), "hipSetDevice");
        char *d_in = nullptr, *d_out = nullptr;
        hip_check(hipMalloc(&d_in, in_bytes * (n + 1)), "hipMalloc");
        hip_check(hipMalloc(&d_out, dst_bytes * (n + 1)), "hipMalloc");
        bounce_upload(d_in, in, in_bytes * n, "upload of the values");
        jinc::NarrowArgs a;  // one group of one dense row: whole lanes by 16-byte accesses, the rest sample by sample
        a.ngroups = 1;
        a.peak = static_cast<float>((1u << dst_bits) - 1u);
        jinc::NarrowGroup& g = a.g[0];
        g.packed = d_out, g.plane[0] = d_in;
        g.packed_pitch = static_cast<uint32_t>(dst_bytes * n), g.plane_pitch = static_cast<uint32_t>(in_bytes * n);
        g.width = static_cast<uint32_t>(n), g.rows = 1, g.unit = 16;
        g.vec_pixels = g.width / static_cast<uint32_t>(16 / dst_bytes) * static_cast<uint32_t>(16 / dst_bytes);
        g.shift[0] = static_cast<uint8_t>(shift);
        const int kind = in_kind == JINC_SAMPLE_FLOAT16 ? jinc::kSampleHalf : in_kind == JINC_SAMPLE_BFLOAT16 ? jinc::kSampleBFloat16 : 0;
        hip_check(static_cast<hipError_t>(jinc::launch_narrow_samples(a, kind, 1, static_cast<int>(dst_bytes), 1, nullptr)), "narrow launch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        bounce_download(out, d_out, dst_bytes * n, "download of the samples");
        (void)hipFree(d_in);
        (void)hipFree(d_out);
    });
}

int jinc_debug_narrow_scaled(const void* in, int in_kind, void* out, int n, int dst_bits, int shift, float scale, float offset, int device) {
    const bool kind_ok = in_kind == JINC_SAMPLE_DEFAULT || in_kind == JINC_SAMPLE_FLOAT16 || in_kind == JINC_SAMPLE_BFLOAT16;
    if (!in || !out || n < 0 || !kind_ok || dst_bits < 8 || dst_bits > 16) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    const size_t in_bytes = in_kind == JINC_SAMPLE_DEFAULT ? 4 : 2, dst_bytes = dst_bits > 8 ? 2 : 1;
    if (shift < 0 || shift > static_cast<int>(8 * dst_bytes) - dst_bits) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    if (!std::isfinite(scale) || !std::isfinite(offset) || scale == 0.f) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    if (n == 0) return JINC_OK;
    return guarded([&] {
        hip_check(hipSetDevice(device), "hipSetDevice");
        char *d_in = nullptr, *d_out = nullptr;
        hip_check(hipMalloc(&d_in, in_bytes * (n + 1)), "hipMalloc");
        hip_check(hipMalloc(&d_out, dst_bytes * (n + 1)), "hipMalloc");
        bounce_upload(d_in, in, in_bytes * n, "upload of the values");
        jinc::NarrowArgs a;  // one group of one dense row: whole lanes by 16-byte accesses, the rest sample by sample
        a.ngroups = 1;
        a.peak = static_cast<float>((1u << dst_bits) - 1u);
        jinc::NarrowGroup& g = a.g[0];
        g.packed = d_out, g.plane[0] = d_in;
        g.packed_pitch = static_cast<uint32_t>(dst_bytes * n), g.plane_pitch = static_cast<uint32_t>(in_bytes * n);
        g.width = static_cast<uint32_t>(n), g.rows = 1, g.unit = 16;
        g.vec_pixels = g.width / static_cast<uint32_t>(16 / dst_bytes) * static_cast<uint32_t>(16 / dst_bytes);
        g.shift[0] = static_cast<uint8_t>(shift);
        g.scale[0] = scale, g.offset[0] = offset;
        const int kind = in_kind == JINC_SAMPLE_FLOAT16 ? jinc::kSampleHalf : in_kind == JINC_SAMPLE_BFLOAT16 ? jinc::kSampleBFloat16 : 0;
        hip_check(static_cast<hipError_t>(jinc::launch_narrow_samples(a, kind, 1, static_cast<int>(dst_bytes), 1, nullptr, true)), "narrow launch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        bounce_download(out, d_out, dst_bytes * n, "download of the samples");
        (void)hipFree(d_in);
        (void)hipFree(d_out);
    });
}

namespace {
// What the two hooks below share: the kind, the pair per plane (finite, scale not zero) and the upload of ONE dense row per plane,
// samples[c] of them in plane c, into buffers of the device's own (256-byte aligned, as the stand-ins are).
int kernel_kind(int in_kind) { return in_kind == JINC_SAMPLE_FLOAT16 ? jinc::kSampleHalf : in_kind == JINC_SAMPLE_BFLOAT16 ? jinc::kSampleBFloat16 : 0; }
bool hook_pairs_ok(const float* scale, const float* offset) {
    for (int c = 0; c < 3; ++c) {
        if (scale && (!std::isfinite(scale[c]) || scale[c] == 0.f)) return false;
        if (offset && !std::isfinite(offset[c])) return false;
    }
    return true;
}
}  // namespace

int jinc_debug_narrow_fields(const void* const in[3], int in_kind, uint32_t* out_words, int n, const int field_offset[3], unsigned fill,
                             const float* scale, const float* offset, int device) {
    const bool kind_ok = in_kind == JINC_SAMPLE_DEFAULT || in_kind == JINC_SAMPLE_FLOAT16 || in_kind == JINC_SAMPLE_BFLOAT16;
    if (!in || !in[0] || !in[1] || !in[2] || !out_words || n < 0 || !kind_ok || !field_offset || !hook_pairs_ok(scale, offset))
        return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    for (int i = 0; i < 3; ++i) {
        if (field_offset[i] < 0 || field_offset[i] > 22) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
        for (int j = i + 1; j < 3; ++j)
            if (field_offset[i] - field_offset[j] < 10 && field_offset[j] - field_offset[i] < 10) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    }
    if (n == 0) return JINC_OK;
    const size_t in_bytes = in_kind == JINC_SAMPLE_DEFAULT ? 4 : 2;
    return guarded([&] {
        hip_check(hipSetDevice(device), "hipSetDevice");
        char *d_in[3] = {nullptr, nullptr, nullptr}, *d_out = nullptr;
        jinc::NarrowFieldArgs a;  // one dense row: whole lanes of 8 pixels by 16-byte accesses, the rest word by word
        uint32_t mask = 0;
        for (int c = 0; c < 3; ++c) {
            hip_check(hipMalloc(&d_in[c], in_bytes * (n + 1)), "hipMalloc");
            bounce_upload(d_in[c], in[c], in_bytes * n, "upload of the values");
            a.plane[c] = d_in[c];
            a.offset[c] = static_cast<uint32_t>(field_offset[c]);
            mask |= 1023u << field_offset[c];
            a.value_scale[c] = scale ? scale[c] : 1.f, a.value_offset[c] = offset ? offset[c] : 0.f;
        }
        hip_check(hipMalloc(&d_out, 4 * static_cast<size_t>(n + 1)), "hipMalloc");
        a.packed = d_out;
        a.packed_pitch = static_cast<uint32_t>(4 * n), a.plane_pitch = static_cast<uint32_t>(in_bytes * n);
        a.width = static_cast<uint32_t>(n), a.rows = 1, a.unit = 16, a.vec_pixels = a.width / 8u * 8u;
        a.fill = fill & ~mask;
        hip_check(static_cast<hipError_t>(jinc::launch_narrow_fields(a, kernel_kind(in_kind), 1, nullptr, scale || offset)), "narrow fields launch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        bounce_download(out_words, d_out, 4 * static_cast<size_t>(n), "download of the words");
        for (int c = 0; c < 3; ++c) (void)hipFree(d_in[c]);
        (void)hipFree(d_out);
    });
}

int jinc_debug_narrow_v210(const void* const in[3], int in_kind, void* out_blocks, int width, const float* scale, const float* offset,
                           int device) {
    const bool kind_ok = in_kind == JINC_SAMPLE_DEFAULT || in_kind == JINC_SAMPLE_FLOAT16 || in_kind == JINC_SAMPLE_BFLOAT16;
    if (!in || !in[0] || !in[1] || !in[2] || !out_blocks || width < 0 || (width & 1) || !kind_ok || !hook_pairs_ok(scale, offset))
        return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    if (width == 0) return JINC_OK;
    const size_t in_bytes = in_kind == JINC_SAMPLE_DEFAULT ? 4 : 2, row_bytes = v210_row_bytes(width);
    return guarded([&] {
        hip_check(hipSetDevice(device), "hipSetDevice");
        char *d_in[3] = {nullptr, nullptr, nullptr}, *d_out = nullptr;
        jinc::NarrowV210Args a;  // one dense row: the blocks in pairs, the odd whole block and the partial one sample by sample
        for (int c = 0; c < 3; ++c) {
            const size_t samples = static_cast<size_t>(c == 0 ? width : width / 2);
            hip_check(hipMalloc(&d_in[c], in_bytes * (samples + 1)), "hipMalloc");
            bounce_upload(d_in[c], in[c], in_bytes * samples, "upload of the values");
            a.plane[c] = d_in[c];
            a.value_scale[c] = scale ? scale[c] : 1.f, a.value_offset[c] = offset ? offset[c] : 0.f;
        }
        hip_check(hipMalloc(&d_out, row_bytes), "hipMalloc");
        a.blocks = d_out;
        a.block_pitch = static_cast<uint32_t>(row_bytes);
        a.luma_pitch = static_cast<uint32_t>(in_bytes * width), a.chroma_pitch = static_cast<uint32_t>(in_bytes * (width / 2));
        a.width = static_cast<uint32_t>(width), a.rows = 1, a.whole_blocks = a.width / 6, a.unit = 16;
        hip_check(static_cast<hipError_t>(jinc::launch_narrow_v210(a, kernel_kind(in_kind), 1, nullptr, scale || offset)), "narrow v210 launch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        bounce_download(out_blocks, d_out, row_bytes, "download of the blocks");
        for (int c = 0; c < 3; ++c) (void)hipFree(d_in[c]);
        (void)hipFree(d_out);
    });
}

int jinc_debug_widen_scaled(const void* in, int src_bits, int shift, float scale, float offset, int out_kind, void* out, int n, int device) {
    const bool kind_ok = out_kind == JINC_SAMPLE_DEFAULT || out_kind == JINC_SAMPLE_FLOAT16 || out_kind == JINC_SAMPLE_BFLOAT16;
    if (!in || !out || n < 0 || !kind_ok || src_bits < 8 || src_bits > 16) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    const size_t src_bytes = src_bits > 8 ? 2 : 1, out_bytes = out_kind == JINC_SAMPLE_DEFAULT ? 4 : 2;
    if (shift < 0 || shift > static_cast<int>(8 * src_bytes) - src_bits) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    if (!std::isfinite(scale) || !std::isfinite(offset) || scale == 0.f) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    if (n == 0) return JINC_OK;
    return guarded([&] {
        hip_check(hipSetDevice(device), "hipSetDevice");
        char *d_in = nullptr, *d_out = nullptr;
        hip_check(hipMalloc(&d_in, src_bytes * (n + 1)), "hipMalloc");
        hip_check(hipMalloc(&d_out, out_bytes * (n + 1)), "hipMalloc");
        bounce_upload(d_in, in, src_bytes * n, "upload of the samples");
        jinc::WidenArgs a;  // one group of one dense row: whole lanes by 16-byte accesses, the rest sample by sample
        a.ngroups = 1;
        a.mask = (1u << src_bits) - 1u;
        jinc::WidenGroup& g = a.g[0];
        g.packed = d_in, g.plane[0] = d_out;
        g.packed_pitch = static_cast<uint32_t>(src_bytes * n), g.plane_pitch = static_cast<uint32_t>(out_bytes * n);
        g.width = static_cast<uint32_t>(n), g.rows = 1, g.unit = 16;
        g.vec_pixels = g.width / static_cast<uint32_t>(16 / src_bytes) * static_cast<uint32_t>(16 / src_bytes);
        g.shift[0] = static_cast<uint8_t>(shift);
        g.scale[0] = scale, g.offset[0] = offset;
        const int kind = out_kind == JINC_SAMPLE_FLOAT16 ? jinc::kSampleHalf : out_kind == JINC_SAMPLE_BFLOAT16 ? jinc::kSampleBFloat16 : 0;
        hip_check(static_cast<hipError_t>(jinc::launch_widen_samples(a, static_cast<int>(src_bytes), 1, static_cast<int>(out_bytes), kind, 1, nullptr, true)), "widen launch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        bounce_download(out, d_out, out_bytes * n, "download of the samples");
        (void)hipFree(d_in);
        (void)hipFree(d_out);
    });
}

int jinc_debug_widen_fields(const uint32_t* words, int n, const int field_offset[3], const float* scale, const float* offset, int out_kind,
                            void* const out[3], int device) {
    const bool kind_ok = out_kind == JINC_SAMPLE_DEFAULT || out_kind == JINC_SAMPLE_FLOAT16 || out_kind == JINC_SAMPLE_BFLOAT16;
    if (!words || !out || !out[0] || !out[1] || !out[2] || n < 0 || !kind_ok || !field_offset || !hook_pairs_ok(scale, offset))
        return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    if (out_kind == JINC_SAMPLE_BFLOAT16 && !scale && !offset) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");  // (the unscaled form has no bfloat16 planes)
    for (int i = 0; i < 3; ++i) {
        if (field_offset[i] < 0 || field_offset[i] > 22) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
        for (int j = i + 1; j < 3; ++j)
            if (field_offset[i] - field_offset[j] < 10 && field_offset[j] - field_offset[i] < 10) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    }
    if (n == 0) return JINC_OK;
    const size_t out_bytes = out_kind == JINC_SAMPLE_DEFAULT ? 4 : 2;
    return guarded([&] {
        hip_check(hipSetDevice(device), "hipSetDevice");
        char *d_out[3] = {nullptr, nullptr, nullptr}, *d_in = nullptr;
        jinc::WidenFieldArgs a;  // one dense row: whole lanes of 8 pixels by 16-byte accesses, the rest word by word
        hip_check(hipMalloc(&d_in, 4 * static_cast<size_t>(n + 1)), "hipMalloc");
        bounce_upload(d_in, words, 4 * static_cast<size_t>(n), "upload of the words");
        for (int c = 0; c < 3; ++c) {
            hip_check(hipMalloc(&d_out[c], out_bytes * (n + 1)), "hipMalloc");
            a.plane[c] = d_out[c];
            a.offset[c] = static_cast<uint32_t>(field_offset[c]);
            a.value_scale[c] = scale ? scale[c] : 1.f, a.value_offset[c] = offset ? offset[c] : 0.f;
        }
        a.packed = d_in;
        a.packed_pitch = static_cast<uint32_t>(4 * n), a.plane_pitch = static_cast<uint32_t>(out_bytes * n);
        a.width = static_cast<uint32_t>(n), a.rows = 1, a.unit = 16, a.vec_pixels = a.width / 8u * 8u;
        hip_check(static_cast<hipError_t>(jinc::launch_widen_fields(a, kernel_kind(out_kind), 1, nullptr, scale || offset)), "widen fields launch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        for (int c = 0; c < 3; ++c) {
            bounce_download(out[c], d_out[c], out_bytes * n, "download of the samples");
            (void)hipFree(d_out[c]);
        }
        (void)hipFree(d_in);
    });
}

int jinc_debug_widen_v210(const void* blocks, int width, const float* scale, const float* offset, int out_kind, void* const out[3], int device) {
    const bool kind_ok = out_kind == JINC_SAMPLE_DEFAULT || out_kind == JINC_SAMPLE_FLOAT16 || out_kind == JINC_SAMPLE_BFLOAT16;
    if (!blocks || !out || !out[0] || !out[1] || !out[2] || width < 0 || (width & 1) || !kind_ok || !hook_pairs_ok(scale, offset))
        return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    if (out_kind == JINC_SAMPLE_BFLOAT16 && !scale && !offset) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");  // (the unscaled form has no bfloat16 planes)
    if (width == 0) return JINC_OK;
    const size_t out_bytes = out_kind == JINC_SAMPLE_DEFAULT ? 4 : 2, row_bytes = v210_row_bytes(width);
    return guarded([&] {
        hip_check(hipSetDevice(device), "hipSetDevice");
        char *d_out[3] = {nullptr, nullptr, nullptr}, *d_in = nullptr;
        jinc::WidenV210Args a;  // one dense row: the blocks in pairs, the odd whole block and the partial one sample by sample
        hip_check(hipMalloc(&d_in, row_bytes), "hipMalloc");
        bounce_upload(d_in, blocks, row_bytes, "upload of the blocks");
        for (int c = 0; c < 3; ++c) {
            const size_t samples = static_cast<size_t>(c == 0 ? width : width / 2);
            hip_check(hipMalloc(&d_out[c], out_bytes * (samples + 1)), "hipMalloc");
            a.plane[c] = d_out[c];
            a.value_scale[c] = scale ? scale[c] : 1.f, a.value_offset[c] = offset ? offset[c] : 0.f;
        }
        a.blocks = d_in;
        a.block_pitch = static_cast<uint32_t>(row_bytes);
        a.luma_pitch = static_cast<uint32_t>(out_bytes * width), a.chroma_pitch = static_cast<uint32_t>(out_bytes * (width / 2));
        a.width = static_cast<uint32_t>(width), a.rows = 1, a.whole_blocks = a.width / 6, a.unit = 16;
        hip_check(static_cast<hipError_t>(jinc::launch_widen_v210(a, kernel_kind(out_kind), 1, nullptr, scale || offset)), "widen v210 launch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        for (int c = 0; c < 3; ++c) {
            const size_t samples = static_cast<size_t>(c == 0 ? width : width / 2);
            bounce_download(out[c], d_out[c], out_bytes * samples, "download of the samples");
            (void)hipFree(d_out[c]);
        }
        (void)hipFree(d_in);
    });
}

const char* jinc_filter_interior_kernel(const jinc_filter* f, int table) {
    if (!f || f->device < 0 || table < 0 || table >= static_cast<int>(f->tables.size())) return "";
    const DeviceTable& t = f->tables[table];
    const int m = f->kernel_mode;
    const bool quasi = t.use_quasi && (m == 7 || m == 8 || m == 10 || (m != 1 && !t.use_periodic));
    const bool periodic = t.use_periodic && m != 1 && m != 7 && m != 8 && m != 10;
    if (t.use_direct && m != 1 && (m == 9 || (!periodic && !quasi))) return "ewa_direct_kernel";
    if (t.use_runs && f->direct_premise && (m == 14 || (m == 0 && t.plan.fs >= 9))) return "ewa_direct_runs_kernel";
    if (quasi) return "ewa_quasi_kernel";
    if (periodic) {
        const int fs = (t.trim_fs > 0 && t.trim_nx == t.trim_fs && !f->full_window && m != 5 && m != 6) ? t.trim_fs : t.plan.fs;
        if (m == 5 || m == 6) return t.plan.fs == 7 ? "ewa_periodic_pk_kernel" : "ewa_periodic_kernel";
        if (m == 3 || fs < 6 || fs > 9) return "ewa_periodic_rows_kernel";
        return "ewa_periodic_kernel";
    }
    return "ewa_gather_kernel";
}

namespace {
// Does the periodic family run `t` on its trimmed support under the filter's kernel mode?  (csrc/dispatch.cpp Choice::trimmed
// without what depends on the call: float planes take it from Rules::kFloatTrimMinTaps taps per plane and call on.)
bool runs_trimmed(const jinc_filter* f, const DeviceTable& t) {
    return t.trim_fs > 0 && !f->full_window && f->kernel_mode != 5 && f->kernel_mode != 6;
}
}  // namespace

int jinc_filter_periodic_support(const jinc_filter* f, int table) {
    if (!f || f->device < 0 || table < 0 || table >= static_cast<int>(f->tables.size())) return 0;
    const DeviceTable& t = f->tables[table];
    if (!t.use_periodic) return 0;
    return runs_trimmed(f, t) ? t.trim_fs : t.plan.fs;
}

double jinc_filter_periodic_taps(const jinc_filter* f, int table, int rows_kernel) {
    if (!f || f->device < 0 || table < 0 || table >= static_cast<int>(f->tables.size())) return 0;
    const DeviceTable& t = f->tables[table];
    if (rows_kernel == 2) {  // the direct kernel's interior
        if (!t.use_direct) return 0;
        const int n = (t.direct_trim_fs > 0 && !f->full_window) ? t.direct_trim_fs : t.plan.fs;
        return static_cast<double>(n) * n;
    }
    if (!t.use_periodic) return 0;
    const bool trimmed = runs_trimmed(f, t);
    if (rows_kernel == 4) {  // ewa_periodic_rowpair_kernel: the spans both phases p of a (q, kernel row) share
        const jinc::PeriodicArgs& pa = (trimmed && t.trim_nx == t.trim_fs) ? t.periodic_trim : t.periodic;
        double taps = 0;
        for (int q = 0; q < pa.py; ++q) {
            const int first = static_cast<int>(pa.rowpair_trim[q] >> 54) & 31, last = static_cast<int>(pa.rowpair_trim[q] >> 59) & 31;  // kernel rows executed
            for (int ly = first; ly < (last ? last : pa.rowpair_ny); ++ly) taps += pa.rowpair_n - 2 * static_cast<int>((pa.rowpair_trim[q] >> (3 * ly)) & 7u);
        }
        return pa.rowpair ? taps / pa.py : 0.0;
    }
    if (rows_kernel == 3 && t.trim_fs == 8 && t.trim_nx == 9 && trimmed)  // 8 rows x 9 columns; with the MPEG-2 chords 60 of the 72
        return (jinc::quad_span9_fits(t.periodic_trim.quad_span7, jinc::kQuadSpan9Mpeg2) || jinc::quad_span9_fits(t.periodic_trim.quad_span7, jinc::kQuadSpan9Mpeg2Swapped))
                   ? jinc::quad_span9_taps(jinc::kQuadSpan9Mpeg2) / 2.0
                   : 72.0;
    if (rows_kernel == 3 && t.trim_fs == 6 && t.trim_nx == 7 && trimmed)  // 6 rows x 7 columns; with the MPEG-2 chords 36 of the 42
        return (jinc::quad_span7_fits(t.periodic_trim.quad_span7, jinc::PeriodicArgs::kQuadSpan7Mpeg2) ||
                jinc::quad_span7_fits(t.periodic_trim.quad_span7, jinc::PeriodicArgs::kQuadSpan7Mpeg2Swapped))
                   ? jinc::quad_span7_taps(jinc::PeriodicArgs::kQuadSpan7Mpeg2) / 2.0
                   : 42.0;
    if (rows_kernel == 3 && t.trim_fs == 6 && trimmed &&  // ewa_periodic_quad2_kernel: chord rows on four taps (half the samples each)
        (t.periodic_trim.quad_inner & jinc::PeriodicArgs::kQuadInnerTap3) == jinc::PeriodicArgs::kQuadInnerTap3)
        return 34.0;
    if (rows_kernel == 3 && t.trim_fs == 8 && trimmed && t.periodic_trim.quad &&  // quad forms on the 8 x 8 support with the tap-4 pattern
        jinc::quad8_pattern_fits(t.periodic_trim.quad_trim8, jinc::kQuad8TrimTap4Value))
        return 56.0;
    if (trimmed && t.trim_nx == t.trim_fs) return rows_kernel == 1 ? t.trim_rows_taps : static_cast<double>(t.trim_fs) * t.trim_fs;
    return static_cast<double>(t.plan.fs) * t.plan.fs;
}

int jinc_filter_set_simd_order(jinc_filter* f, int order) {
    if (!f || order < 0 || order > 3) return fail(JINC_ERR_INVALID_ARG, "JincResize: SIMD order must be 0..3.");
    if (f->half && order != 0)
        return fail(JINC_ERR_UNSUPPORTED, "JincResize: SIMD-order modes do not exist for half-precision float clips (the reference has no half path).");
    if (f->bf16 && order != 0)
        return fail(JINC_ERR_UNSUPPORTED, "JincResize: SIMD-order modes do not exist for bfloat16 clips (the reference has no bfloat16 path).");
    f->simd_order = order;
    return JINC_OK;
}

int jinc_filter_set_output_matrix(jinc_filter* f, const float m[9], const float offset[3]) {
    if (!f) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (!m) {  // (clearing needs no check: what a filter without a matrix does is what it always did)
        f->has_matrix = false;
        g_last_error.clear();
        return JINC_OK;
    }
    if (!f->float_samples())
        return fail(JINC_ERR_UNSUPPORTED, "JincResize: an output matrix needs a float, half or bfloat16 filter (this one has integer samples of " +
                                              std::to_string(f->vi_in.bits_per_component) + " bits).");
    if (f->planecount < 3)
        return fail(JINC_ERR_UNSUPPORTED, "JincResize: an output matrix needs three planes (this filter has " + std::to_string(f->planecount) + ").");
    int w[3], h[3];
    for (int i = 0; i < 3; ++i) f->plane_dims(f->vi_out, i, w[i], h[i]);
    if (w[1] != w[0] || w[2] != w[0] || h[1] != h[0] || h[2] != h[0])
        return fail(JINC_ERR_UNSUPPORTED, "JincResize: an output matrix needs output planes 0..2 of one size (4:4:4; jinc_filter_create_out(..., 0, 0) "
                                          "gives that from 4:2:0 and 4:2:2 input); this filter's output has sub_w " + std::to_string(f->vi_out.sub_w) + " and sub_h " +
                                              std::to_string(f->vi_out.sub_h) + ".");
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(m[k])) return fail(JINC_ERR_INVALID_ARG, "JincResize: entry " + std::to_string(k) + " of the output matrix is not finite.");
    for (int k = 0; offset && k < 3; ++k)
        if (!std::isfinite(offset[k])) return fail(JINC_ERR_INVALID_ARG, "JincResize: entry " + std::to_string(k) + " of the output matrix's offset is not finite.");
    for (int k = 0; k < 9; ++k) f->matrix[k] = m[k];
    for (int k = 0; k < 3; ++k) f->matrix_offset[k] = offset ? offset[k] : 0.f;
    f->has_matrix = true;
    g_last_error.clear();
    return JINC_OK;
}

int jinc_colour_matrix(int standard, int direction, float m[9]) {
    if (!m) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    if (standard != JINC_MATRIX_BT601 && standard != JINC_MATRIX_BT709 && standard != JINC_MATRIX_BT2020_NCL)
        return fail(JINC_ERR_INVALID_ARG, "JincResize: the standard of a colour matrix must be JINC_MATRIX_BT601, JINC_MATRIX_BT709 or JINC_MATRIX_BT2020_NCL.");
    if (direction != JINC_YCBCR_TO_RGB && direction != JINC_RGB_TO_YCBCR)
        return fail(JINC_ERR_INVALID_ARG, "JincResize: the direction of a colour matrix must be JINC_YCBCR_TO_RGB or JINC_RGB_TO_YCBCR.");
    const double kr = standard == JINC_MATRIX_BT601 ? 0.299 : standard == JINC_MATRIX_BT709 ? 0.2126 : 0.2627;
    const double kb = standard == JINC_MATRIX_BT601 ? 0.114 : standard == JINC_MATRIX_BT709 ? 0.0722 : 0.0593;
    const double kg = 1.0 - kr - kb;
    // (every entry in double, in the order the header writes it, rounded once)
    const double to_rgb[9] = {1.0, 0.0, 2.0 * (1.0 - kr),
                              1.0, -2.0 * kb * (1.0 - kb) / kg, -2.0 * kr * (1.0 - kr) / kg,
                              1.0, 2.0 * (1.0 - kb), 0.0};
    const double to_ycbcr[9] = {kr, kg, kb,
                                -kr / (2.0 * (1.0 - kb)), -kg / (2.0 * (1.0 - kb)), 0.5,
                                0.5, -kg / (2.0 * (1.0 - kr)), -kb / (2.0 * (1.0 - kr))};
    for (int k = 0; k < 9; ++k) m[k] = static_cast<float>(direction == JINC_YCBCR_TO_RGB ? to_rgb[k] : to_ycbcr[k]);
    return JINC_OK;
}

int jinc_debug_last_matrix_launches(void) { return last_matrix_launches(); }

int jinc_debug_matrix_rows(void* const rows[3], int in_kind, int n, const float m[9], const float offset[3], int device) {
    const bool kind_ok = in_kind == JINC_SAMPLE_DEFAULT || in_kind == JINC_SAMPLE_FLOAT16 || in_kind == JINC_SAMPLE_BFLOAT16;
    if (!rows || !rows[0] || !rows[1] || !rows[2] || !m || n < 0 || !kind_ok) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(m[k])) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    for (int k = 0; offset && k < 3; ++k)
        if (!std::isfinite(offset[k])) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    if (n == 0) return JINC_OK;
    const size_t bytes = (in_kind == JINC_SAMPLE_DEFAULT ? 4 : 2) * static_cast<size_t>(n);
    return guarded([&] {
        hip_check(hipSetDevice(device), "hipSetDevice");
        char* d[3] = {nullptr, nullptr, nullptr};
        jinc::MatrixArgs a;  // three dense rows: whole lanes by 16-byte accesses, the rest sample by sample
        for (int c = 0; c < 3; ++c) {
            hip_check(hipMalloc(&d[c], bytes + 16), "hipMalloc");
            bounce_upload(d[c], rows[c], bytes, "upload of the values");
            a.plane[c] = d[c], a.pitch[c] = static_cast<uint32_t>(align_up(bytes, 16));  // (one row: the pitch only has to suit the unit)
        }
        const uint32_t lane_pixels = in_kind == JINC_SAMPLE_DEFAULT ? 4u : 8u;
        a.width = static_cast<uint32_t>(n), a.rows = 1, a.unit = 16, a.vec_pixels = a.width / lane_pixels * lane_pixels;
        for (int k = 0; k < 9; ++k) a.m[k] = m[k];
        for (int k = 0; k < 3; ++k) a.offset[k] = offset ? offset[k] : 0.f;
        const int kind = in_kind == JINC_SAMPLE_FLOAT16 ? jinc::kSampleHalf : in_kind == JINC_SAMPLE_BFLOAT16 ? jinc::kSampleBFloat16 : 0;
        hip_check(static_cast<hipError_t>(jinc::launch_output_matrix(a, kind, 1, nullptr)), "output matrix launch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        for (int c = 0; c < 3; ++c) {
            bounce_download(rows[c], d[c], bytes, "download of the samples");
            (void)hipFree(d[c]);
        }
    });
}

int jinc_debug_buffer_range_check(int device) {
    const int r = buffer_range_check_covers_soffset(device);
    if (r < 0) return fail(JINC_ERR_HIP, "JincResize: the buffer range-check probe could not run.");
    return r;
}

int jinc_debug_set_direct_shape(int shape) {
    if (shape != -1 && shape != 0 && shape != 2 && shape != 3) return fail(JINC_ERR_INVALID_ARG, "JincResize: direct shape must be -1, 0, 2 or 3.");
    jinc::set_direct_shape(shape);
    return JINC_OK;
}

int jinc_debug_last_direct_shape(void) { return jinc::last_direct_shape(); }

const char* jinc_filter_last_kernel(const jinc_filter* f, int table) {
    if (!f || f->device < 0 || table < 0 || table >= static_cast<int>(f->tables.size())) return "";
    return f->tables[table].last_kernel;
}

const char* jinc_filter_last_instance(const jinc_filter* f, int table) {
    if (!f || f->device < 0 || table < 0 || table >= static_cast<int>(f->tables.size())) return "";
    return f->tables[table].last_instance.c_str();
}

int jinc_filter_last_finite_flags(const jinc_filter* f, int plane, uint32_t* flags, int capacity) {
    if (!f || f->device < 0 || plane < 0 || plane >= f->planecount) return 0;
    const jinc_filter::LastFlags& r = f->last_flags[plane];
    if (r.frames <= 0 || !f->finite_flags) return 0;
    const int rc = guarded([&] {
        hip_check(hipSetDevice(f->device), "hipSetDevice");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize(finite flags)");  // the call's launches may lie on any stream
        const int n = std::min(capacity, r.frames);
        if (flags && n > 0) hip_check(hipMemcpy(flags, f->finite_flags + r.first, sizeof(uint32_t) * n, hipMemcpyDeviceToHost), "hipMemcpy(finite flags)");
    });
    return rc != JINC_OK ? rc : r.frames;
}

int jinc_debug_set_knob(int knob, double value) {
    if (knob < 0 || knob >= JINC_KNOB_COUNT) return fail(JINC_ERR_INVALID_ARG, "JincResize: no such knob.");
    if (knob == JINC_KNOB_DIRECT_SHAPE) return jinc_debug_set_direct_shape(static_cast<int>(value));
    jinc::knobs::set(knob, value);
    return JINC_OK;
}

int jinc_debug_clear_knob(int knob) {
    if (knob >= JINC_KNOB_COUNT) return fail(JINC_ERR_INVALID_ARG, "JincResize: no such knob.");
    jinc::knobs::clear(knob);
    if (knob < 0 || knob == JINC_KNOB_DIRECT_SHAPE) jinc::set_direct_shape(-1);
    return JINC_OK;
}

int jinc_debug_get_knob(int knob, double* value) {
    if (knob < 0 || knob >= JINC_KNOB_COUNT) return fail(JINC_ERR_INVALID_ARG, "JincResize: no such knob.");
    if (!jinc::knobs::is_set(knob)) return 0;
    if (value) *value = jinc::knobs::get(knob, 0.0);
    return 1;
}

const char* jinc_debug_knob_name(int knob) { return jinc::knobs::name(knob); }
int jinc_debug_chord_pattern(int taps_per_row, uint64_t spans) {
    if (taps_per_row == 7)
        return jinc::quad_span7_fits(spans, jinc::PeriodicArgs::kQuadSpan7Mpeg2) ? 1 : jinc::quad_span7_fits(spans, jinc::PeriodicArgs::kQuadSpan7Mpeg2Swapped) ? 2 : 0;
    if (taps_per_row == 9) return jinc::quad_span9_fits(spans, jinc::kQuadSpan9Mpeg2) ? 1 : jinc::quad_span9_fits(spans, jinc::kQuadSpan9Mpeg2Swapped) ? 2 : 0;
    return -1;
}

int jinc_debug_quad2_share(const float* sets, float* share_w) {
    if (!sets || !share_w) return 0;
    const float* const phase_sets[4] = {sets, sets + 36, sets + 72, sets + 108};
    return jinc::quad2_share_classes(phase_sets, share_w) ? 1 : 0;
}
int jinc_debug_quad2_share_products(int strip_rows) {
    switch (strip_rows) {
        case 2: return jinc::quad2_share_products<2>();
        case 8: return jinc::quad2_share_products<8>();
        case 16: return jinc::quad2_share_products<16>();
        default: return -1;
    }
}

// Shader-clock sampler beside the kernels being timed (kernel_probe.hip).
struct jinc_clock_sampler {
    int device = 0;
    hipStream_t stream = nullptr, control = nullptr;
    int* stop = nullptr;                 // DEVICE memory, raised by a memset on the control stream (a flag in pinned host
                                         // memory is not seen by a running kernel here: the samplers ran to their time limit)
    unsigned long long* out = nullptr;   // pinned host memory, 2 x kSamplers
    static constexpr int kSamplers = 8;
};

int jinc_debug_clock_sampler_start(int device, double max_seconds, jinc_clock_sampler** out) {
    if (!out || max_seconds <= 0.0 || max_seconds > 120.0) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    *out = nullptr;
    std::unique_ptr<jinc_clock_sampler> s(new jinc_clock_sampler());
    s->device = device;
    const int rc = guarded([&] {
        hip_check(hipSetDevice(device), "hipSetDevice");
        // default priority: a dispatch that stays active on a HIGH-priority stream throttles the wave launch of every other
        // queue for as long as it lives (measured: eight sleeping sampler waves at the highest priority cost the direct
        // kernels 10-15 %: 1080p -> 720p 256 -> 223 Gpix/s; profiles/round3/clock_sampler_priority.log)
        hip_check(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking), "hipStreamCreate");
        hip_check(hipStreamCreateWithFlags(&s->control, hipStreamNonBlocking), "hipStreamCreate");
        hip_check(hipMalloc(reinterpret_cast<void**>(&s->stop), 256), "hipMalloc");
        hip_check(hipMemsetAsync(s->stop, 0, 256, s->control), "hipMemsetAsync");
        hip_check(hipStreamSynchronize(s->control), "stream sync");
        hip_check(hipHostMalloc(reinterpret_cast<void**>(&s->out), sizeof(unsigned long long) * 2 * jinc_clock_sampler::kSamplers, hipHostMallocDefault),
                  "hipHostMalloc");
        std::memset(s->out, 0, sizeof(unsigned long long) * 2 * jinc_clock_sampler::kSamplers);
        hip_check(static_cast<hipError_t>(jinc::launch_clock_sampler(s->stop, s->out, jinc_clock_sampler::kSamplers, max_seconds, s->stream)),
                  "clock sampler launch");
    });
    if (rc != JINC_OK) {
        if (s->stream) (void)hipStreamSynchronize(s->stream);
        if (s->stop) (void)hipFree(s->stop);
        if (s->out) (void)hipHostFree(s->out);
        if (s->stream) (void)hipStreamDestroy(s->stream);
        if (s->control) (void)hipStreamDestroy(s->control);
        return rc;
    }
    *out = s.release();
    return JINC_OK;
}

int jinc_debug_clock_sampler_stop(jinc_clock_sampler* s, double* ghz_min, double* ghz_median, double* ghz_max) {
    if (!s) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    const int rc = guarded([&] {
        hip_check(hipSetDevice(s->device), "hipSetDevice");
        hip_check(hipMemsetAsync(s->stop, 1, 4, s->control), "hipMemsetAsync(stop flag)");  // any non-zero value stops the samplers
        hip_check(hipStreamSynchronize(s->control), "stream sync");
        hip_check(hipStreamSynchronize(s->stream), "stream sync");
        std::vector<double> ghz;
        for (int k = 0; k < jinc_clock_sampler::kSamplers; ++k)
            if (s->out[2 * k + 1] > 0) ghz.push_back(static_cast<double>(s->out[2 * k]) / static_cast<double>(s->out[2 * k + 1]) * 0.1);
        std::sort(ghz.begin(), ghz.end());
        if (ghz.empty()) throw HipError("JincResize: the clock samplers did not run.");
        if (ghz_min) *ghz_min = ghz.front();
        if (ghz_max) *ghz_max = ghz.back();
        if (ghz_median) *ghz_median = 0.5 * (ghz[(ghz.size() - 1) / 2] + ghz[ghz.size() / 2]);
    });
    (void)hipFree(s->stop);
    (void)hipHostFree(s->out);
    (void)hipStreamDestroy(s->stream);
    (void)hipStreamDestroy(s->control);
    delete s;
    return rc;
}

int jinc_debug_valu_pair_probe(int device, int waves_per_simd, double* tops, double* shader_clock_ghz) {
    if (waves_per_simd < 1 || waves_per_simd > 8 || !tops) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad argument.");
    return guarded([&] {
        hip_check(hipSetDevice(device), "hipSetDevice");
        hipDeviceProp_t prop;
        hip_check(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties");
        const int blocks = prop.multiProcessorCount * waves_per_simd;  // 256 threads = one wave per SIMD of a CU
        const int iters = 100000;                                     // ~15 ms at 8 waves per SIMD
        float* out = nullptr;
        hip_check(hipMalloc(&out, sizeof(float) * 256 * blocks), "hipMalloc");
        hipEvent_t e0 = nullptr, e1 = nullptr;
        hip_check(hipEventCreate(&e0), "hipEventCreate");
        hip_check(hipEventCreate(&e1), "hipEventCreate");
        jinc_clock_sampler* cs = nullptr;
        double best = 1e30, ghz = 0.0;
        for (int rep = 0; rep < 4; ++rep) {  // the first launch ramps the clock; the last one is sampled
            if (rep == 3 && shader_clock_ghz) (void)jinc_debug_clock_sampler_start(device, 5.0, &cs);
            hip_check(hipEventRecord(e0, nullptr), "hipEventRecord");
            hip_check(static_cast<hipError_t>(jinc::launch_valu_pair_probe(out, blocks, iters, nullptr)), "probe launch");
            hip_check(hipEventRecord(e1, nullptr), "hipEventRecord");
            hip_check(hipEventSynchronize(e1), "hipEventSynchronize");
            float ms = 0.f;
            hip_check(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
            if (rep > 0) best = std::min(best, static_cast<double>(ms));
        }
        if (cs) (void)jinc_debug_clock_sampler_stop(cs, nullptr, &ghz, nullptr);
        *tops = 16.0 * iters * 256.0 * blocks / (best * 1e-3) / 1e12;
        if (shader_clock_ghz) *shader_clock_ghz = ghz;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        (void)hipFree(out);
    });
}

const char* jinc_debug_last_call(int* nframes) {
    if (nframes) *nframes = last_call_frames_in_process();
    return last_interior_kernel_in_process();
}

int jinc_filter_last_border(const jinc_filter* f, int table) {
    if (!f || f->device < 0 || table < 0 || table >= static_cast<int>(f->tables.size())) return 0;
    return f->tables[table].last_border;
}

const char* jinc_debug_last_instance(void) { return last_interior_instance_in_process(); }

int jinc_filter_direct_premise(const jinc_filter* f) { return (f && f->device >= 0) ? (f->direct_premise ? 1 : 0) : -1; }

int jinc_filter_set_border_strips(jinc_filter* f, int enable) {
    if (!f) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    f->border_strips = enable < 0 ? -1 : enable > 4 ? 1 : enable;  // -1: by call size; 2: rows as strips, columns on the gather kernel; 3: ewa_strip_kernel; 4: 3 + columns inside the interior kernel
    g_last_error.clear();
    return JINC_OK;
}

int jinc_filter_set_kernel_mode(jinc_filter* f, int mode) {
    if (!f || mode < 0 || mode > 16) return fail(JINC_ERR_INVALID_ARG, "JincResize: bad kernel mode.");
    f->full_window = mode == 15;  // 15 = the automatic choice, but on the reference's full window (no trimmed support)
    f->kernel_mode = mode == 15 ? 0 : mode;
    return JINC_OK;
}

int jinc_filter_set_border_overlap(jinc_filter* f, int enable) {
    if (!f) return fail(JINC_ERR_INVALID_ARG, "JincResize: null argument.");
    f->overlap_border = enable < 0 ? -1 : (enable != 0);
    return JINC_OK;
}

}  // extern "C"
