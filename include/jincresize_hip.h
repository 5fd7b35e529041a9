/*
 * jincresize_hip.h -- C ABI of libjincresize_hip.so, the MI355X (gfx950) replacement for the
 * per-frame hot path of Asd-g/AviSynth-JincResize v2.1.4.
 *
 * "ref:" citations are /root/reference/src/JincResize.cpp unless another file is named.
 *
 * What this boundary replaces in the reference plugin:
 *   - Create_JincResize's argument handling + table construction          (ref :654-984)
 *   - (d->*d->process_frame)(src, dst, vi) inside JincResize_GetFrame      (ref :615), i.e. the
 *     resize_plane_{c,sse41,avx2,avx512}<T,thr,subsampled> kernels        (ref :536-601 and
 *     resize_plane_sse41.cpp / _avx2.cpp / _avx512.cpp) and their row dispatch (ref :589-599)
 *   - free_JincResize                                                     (ref :632-647)
 * The AviSynth registration glue (avisynth_c_plugin_init, the Jinc36/64/144/256 aliases,
 * _ChromaLocation frame property) stays on the plugin side and calls these entry points; the
 * binding is shown in INTEGRATION.md.
 *
 * Results are those of the reference's opt=0 C++ path (resize_plane_c): bit-exact for 8..16-bit
 * integer planes and for float planes (strict sequential un-fused fp32 accumulation).
 *
 * Plain pointers and sizes only; no C++ or framework types cross this boundary.  Every function
 * returning int returns 0 on success and a negative jinc_status on failure; the message is
 * available from jinc_last_error() (thread-local) and, for jinc_filter_create, also copied to
 * the caller's buffer because AviSynth reports Create-time errors as strings (ref :682-687).
 */
#ifndef JINCRESIZE_HIP_H
#define JINCRESIZE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define JINC_API __attribute__((visibility("default")))
#else
#define JINC_API
#endif

typedef enum jinc_status {
    JINC_OK = 0,
    JINC_ERR_INVALID_ARG = -1, /* argument rejected with one of the reference's "JincResize: ..." messages */
    JINC_ERR_NO_DEVICE = -2,   /* no usable HIP device / HIP runtime error */
    JINC_ERR_HIP = -3,
    JINC_ERR_NOMEM = -4,
    JINC_ERR_UNSUPPORTED = -5  /* geometry the reference itself handles with undefined behaviour */
} jinc_status;

/* The AVS_VideoInfo facts Create_JincResize / resize_plane_c read from the input clip:
 * avs_is_planar (ref :700), width/height (ref :783-784), avs_bits_per_component (ref :793),
 * avs_num_components (ref :798), avs_is_444 / avs_is_rgb (ref :826), avs_is_420 (ref :744),
 * avs_get_plane_{width,height}_subsampling(vi, AVS_PLANAR_U) (ref :833-834),
 * avs_component_size (ref :903). */
typedef struct jinc_video_info {
    int width;
    int height;
    int bits_per_component; /* 8, 10, 12, 14, 16 or 32 (float) */
    int component_size;     /* bytes per sample: 1, 2 or 4 */
    int num_components;     /* 1 (Y), 3 or 4 (with alpha) */
    int is_planar;          /* non-zero for planar formats */
    int is_rgb;             /* planar RGB(A): plane order G,B,R,A (ref :540) */
    int sub_w;              /* log2 horizontal chroma subsampling (0 for Y/444/RGB) */
    int sub_h;              /* log2 vertical chroma subsampling */
} jinc_video_info;

/* Bits of jinc_args.defined: which optional script arguments were given (avs_defined). */
enum {
    JINC_ARG_SRC_LEFT = 1 << 0,
    JINC_ARG_SRC_TOP = 1 << 1,
    JINC_ARG_SRC_WIDTH = 1 << 2,
    JINC_ARG_SRC_HEIGHT = 1 << 3,
    JINC_ARG_QUANT_X = 1 << 4,
    JINC_ARG_QUANT_Y = 1 << 5,
    JINC_ARG_TAP = 1 << 6,
    JINC_ARG_BLUR = 1 << 7,
    JINC_ARG_CPLACE = 1 << 8,
    JINC_ARG_THREADS = 1 << 9,
    JINC_ARG_OPT = 1 << 10,
    JINC_ARG_INITIAL_CAPACITY = 1 << 11,
    JINC_ARG_INITIAL_FACTOR = 1 << 12
};

/* The script arguments of JincResize(), in registration order (ref :1044-1060), as the plugin
 * reads them in Create_JincResize (ref :703-789).  Arguments whose bit is clear in `defined`
 * take the reference's defaults. */
typedef struct jinc_args {
    int target_width;       /* "i" (required) */
    int target_height;      /* "i" (required) */
    double src_left;        /* [src_left]f   default 0 */
    double src_top;         /* [src_top]f    default 0 */
    double src_width;       /* [src_width]f  default clip width;  <= 0: relative (ref :763-765) */
    double src_height;      /* [src_height]f default clip height; <= 0: relative (ref :768-770) */
    int quant_x;            /* [quant_x]i    default 256, 1..256 */
    int quant_y;            /* [quant_y]i    default 256, 1..256 */
    int tap;                /* [tap]i        default 3, 1..16 */
    double blur;            /* [blur]f       default (and 0) -> 1.0 (ref :772-774) */
    const char *cplace;     /* [cplace]s     "MPEG2" | "MPEG1" | "topleft", case-insensitive */
    int threads;            /* [threads]i    0 or 1 (ref :758-760, :901): 1 keeps the copies of pageable planes on the calling thread, 0 lets large planes use the library's helper threads */
    int opt;                /* [opt]i        -1..3; validated as in the reference, advisory on the GPU path */
    int initial_capacity;   /* [initial_capacity]i > 0; validated, otherwise unused (scratch sizing only) */
    double initial_factor;  /* [initial_factor]f >= 1.0; validated, otherwise unused */
    unsigned defined;       /* JINC_ARG_* bits */
    /* Host facts the reference queries from the script environment: */
    int frame0_chroma_location; /* _ChromaLocation of frame 0 if that property is an int, else -1 = "no such property"
                                   (only consulted when cplace is not given; ref :727-742).  0 / 1 / 2 select the
                                   siting; ANY other integer the property holds -- negative ones too: pass them as 3 --
                                   is the reference's "invalid _ChromaLocation" (switch default, :737) */
    int cpu_has_sse41;      /* avs_get_cpu_flags() & AVS_CPUF_SSE4_1 (ref :755) */
    int cpu_has_avx2;       /* ... & AVS_CPUF_AVX2    (ref :753) */
    int cpu_has_avx512f;    /* ... & AVS_CPUF_AVX512F (ref :751) */
} jinc_args;

/* Opaque filter instance = the reference's `JincResize` object (JincResize.h:39-57) plus its
 * device-resident plan.  One instance is not re-entrant (AviSynth MT_MULTI_INSTANCE, ref :649-652):
 * create one per host thread; instances share nothing mutable. */
typedef struct jinc_filter jinc_filter;

/* Number of usable HIP devices (0 when there is none); replaces nothing, used to shard frames. */
JINC_API int jinc_device_count(void);

/* Round-robin device index for hosts that create one filter instance per worker thread (AviSynth Prefetch(N),
 * MT_MULTI_INSTANCE, ref :649-652): successive calls return 0, 1, ..., jinc_device_count()-1, 0, ... so that the
 * instances -- and with them the frames, which are independent units -- spread over the GPUs of the node with no
 * data exchanged between devices.  Returns -1 when there is no device. */
JINC_API int jinc_pick_device(void);

/* Message of the last failure on the calling thread ("" if none). */
JINC_API const char *jinc_last_error(void);

/* Create_JincResize (ref :654-984): validates the arguments with the reference's rules and error
 * strings, derives crop/chroma geometry (ref :762-866), builds the LUT and the coefficient plan(s)
 * and uploads them to HIP device `device`.  On failure *out is NULL and the message (e.g.
 * "JincResize: tap must be between 1..16.") is copied to err (if err_len > 0). */
JINC_API int jinc_filter_create(const jinc_video_info *vi, const jinc_args *args, int device,
                                jinc_filter **out, char *err, size_t err_len);

/* Sample types beyond the reference.  JINC_SAMPLE_DEFAULT: the type bits_per_component says (8 .. 16: unsigned integers,
 * 32: fp32), exactly what jinc_filter_create does.  JINC_SAMPLE_FLOAT16: IEEE binary16 planes (VapourSynth GRAYH, YUV4xxPH,
 * RGBH), which need bits_per_component == 16 and component_size == 2.  A half plane is defined by the fp32 path: every
 * sample widens exactly to fp32 (subnormals, infinities and NaNs included), the result is what the library computes for
 * that fp32 plane (same plan, same un-fused (ly, lx) chain, the trimmed support only on frames whose samples are all
 * finite), and it narrows to binary16 with round-to-nearest-even: |r| >= 65520 becomes an infinity, subnormal results
 * and the sign of zero are kept, nothing is clamped.  The reference has no half formats; its SIMD-order modes
 * (jinc_filter_set_simd_order 1 .. 3) do not exist for half filters.
 * JINC_SAMPLE_BFLOAT16: bfloat16 planes, the 16-bit type networks on this hardware read; they too need bits_per_component
 * == 16 and component_size == 2.  A bfloat16 sample is the upper 16 bits of an IEEE fp32 value, and a bfloat16 filter
 *   1. widens: fp32 bits = sample bits << 16, exact for every pattern, subnormals, infinities and NaNs included;
 *   2. computes exactly what the library computes for that fp32 plane (same plan, same un-fused (ly, lx) chain, the trimmed
 *      support only on frames whose samples are all finite, nothing clamped);
 *   3. narrows the fp32 result with round-to-nearest-even: results at or beyond 0x7f7f8000 in magnitude become +-inf,
 *      subnormal results and the sign of zero are kept, and a NaN result is stored as a NaN (never as an infinity).
 * The kernel choice is fp32's, as for half.  No SIMD-order modes either: a non-zero order is JINC_ERR_UNSUPPORTED. */
#define JINC_SAMPLE_DEFAULT 0
#define JINC_SAMPLE_FLOAT16 1
#define JINC_SAMPLE_BFLOAT16 3 /* (2 is not a sample type: it stays refused, as before bfloat16 existed) */

/* jinc_filter_create with a sample type: jinc_filter_create(...) is jinc_filter_create_ex(..., JINC_SAMPLE_DEFAULT, ...).
 * A sample type other than the three above (2 included), or JINC_SAMPLE_FLOAT16 / JINC_SAMPLE_BFLOAT16 with bits_per_component != 16 or
 * component_size != 2, is JINC_ERR_INVALID_ARG with a "JincResize: ..." message.  device = -1 builds a host-only plan, as for
 * create. */
JINC_API int jinc_filter_create_ex(const jinc_video_info *vi, const jinc_args *args, int sample_type, int device,
                                   jinc_filter **out, char *err, size_t err_len);

/* jinc_filter_create_ex with the OUTPUT's chroma sub-sampling (beyond the reference, whose output always has the input's): a
 * decoder's 4:2:0 / 4:2:2 frames leave with chroma on the luma grid (networks, Y410 / RGB10A2 swap chains, every YCbCr -> RGB step
 * want that), 4:4:4 planes leave as 4:2:0 / 4:2:2.  out_sub_w / out_sub_h are log2 factors like jinc_video_info.sub_w / sub_h:
 *   -1, -1            the input's: the call IS jinc_filter_create_ex -- same plans, same bits, same messages;
 *   the input's own   the same filter (the target must then be a multiple of the factors, see below);
 *   (0,0) (1,0) (1,1) 4:4:4, 4:2:2, 4:2:0 output from a 4:4:4, 4:2:2 or 4:2:0 YUV(A) clip of any sample type: all nine pairs.
 * jinc_filter_output_info reports the output's values; every surface (get_frame, submit / wait, process_device and its variants,
 * jinc_batch_process) takes source planes of the input's extents and writes destination planes of the output's.
 * Definition.  Plane 0 (and alpha) is what a Y-only filter with the same arguments computes.  Planes 1 and 2 are, bit for bit, what
 * a Y-only filter computes for a clip of the input's chroma size (width >> sub_w, height >> sub_h), target (target_width >>
 * out_sub_w, target_height >> out_sub_h), the same quant_x / quant_y / tap / blur, and per axis, with d_i = 1 << sub (input),
 * d_o = 1 << out_sub, r = clip size / target size (as doubles) and crop / crop_size the resolved src_left / src_width (src_top /
 * src_height):
 *   src_left (src_top)     = (k + crop) / d_i,  k = 0.5 * ((d_i - 1) - r * (d_o - 1)) on a co-sited axis, else crop / d_i
 *   src_width (src_height) = crop_size / d_i
 * An axis is co-sited horizontally for cplace mpeg2 and topleft, vertically for topleft; for d_i = d_o = 2 this is the
 * reference's (0.5 * (1 - r) + crop) / 2.  cplace / _ChromaLocation describe the siting of whichever side is sub-sampled (of both
 * when both are); "topleft" is taken when the input OR the output is 4:2:0.  jinc_filter_chroma_location follows the output: 2
 * (or the by-siting value) for a sub-sampled output, -1 for a 4:4:4 one.
 * JINC_ERR_INVALID_ARG, behind the reference's own checks and before any device work, each with a message of its own: out_sub
 * other than -1 / -1 on an RGB or Y-only clip; a value outside -1, 0, 1 or only one of the two -1; (0,1) (4:4:0 output); a 4:1:1
 * or 4:4:0 clip with an output that differs from it; target_width / target_height that is no multiple of 1 << out_sub_w /
 * 1 << out_sub_h.
 * The stand-in calls' shape rules hold per side: packed 10:10:10:2 words need that SIDE of the filter 4:4:4, v210 blocks need it
 * 4:2:2, and the planes of a channel group share their extent on their side -- so NV12 / P010 go to planar 4:4:4 float planes
 * through _widened[_scaled], P010 and v210 to Y410 through _shifted_packed10 / _v210_packed10 (below), 4:4:4 float planes to NV12 /
 * P010 / v210 through _narrowed[_scaled] / _narrowed_v210. */
JINC_API int jinc_filter_create_out(const jinc_video_info *vi, const jinc_args *args, int sample_type, int out_sub_w, int out_sub_h,
                                    int device, jinc_filter **out, char *err, size_t err_len);

/* A decoder's P010 (or any planes of jinc_filter_process_device_shifted's source side: a sample step 1..4 and a shift 0..6 per plane,
 * either array may be NULL) into ONE buffer of 10:10:10:2 words (the destination side of jinc_filter_process_device_packed10: three
 * bit offsets in plane order, 0..22 and not overlapping, dst_fill outside the fields; base, pitch and frame stride multiples of 4,
 * pitch >= 4 * width) -- for an integer filter with three 10-bit components in 16-bit samples whose OUTPUT is 4:4:4
 * (jinc_filter_create_out(..., 0, 0, ...) on YUV420P10 / YUV422P10, or YUV444P10 / RGBP10 themselves).  The same two passes as
 * those calls -- the split of the source side, the pack of the destination side -- around the unchanged resampling launches, so
 * the words hold, bit for bit, what jinc_filter_process_device writes into dense planes of the same values.  Frame strides of the
 * source are required for nframes > 1. */
JINC_API int jinc_filter_process_device_shifted_packed10(jinc_filter *f, const void *const src[4], const int src_pitch[4],
                                                         const int src_sample_step[4], const int src_sample_shift[4],
                                                         const size_t src_frame_stride[4], void *dst, int dst_pitch,
                                                         const int dst_field_offset[3], unsigned dst_fill, size_t dst_frame_stride,
                                                         int nframes, void *hip_stream);
/* ... and v210 blocks (the source side of jinc_filter_process_device_v210: ONE buffer, rows of jinc_v210_row_bytes(width) bytes)
 * into such words: the filter's INPUT is 4:2:2, its output 4:4:4 (jinc_filter_create_out(..., 0, 0, ...) on YUV422P10). */
JINC_API int jinc_filter_process_device_v210_packed10(jinc_filter *f, const void *src, int src_pitch, size_t src_frame_stride, void *dst,
                                                      int dst_pitch, const int dst_field_offset[3], unsigned dst_fill,
                                                      size_t dst_frame_stride, int nframes, void *hip_stream);

/* free_JincResize (ref :632-647). NULL is allowed. */
JINC_API void jinc_filter_free(jinc_filter *f);

/* The output clip's AVS_VideoInfo: the input's with width/height replaced (ref :791-792) -- and sub_w / sub_h, for a filter of
 * jinc_filter_create_out. */
JINC_API int jinc_filter_output_info(const jinc_filter *f, jinc_video_info *out_vi);

/* Value JincResize_GetFrame writes to the _ChromaLocation frame property (ref :617-625): **2 for every 4:2:0 / 4:2:2 /
 * 4:1:1 output, whatever the siting**; -1 when the property is not written (4:4:4, Y, RGB).  The reference's source
 * reads as "0 mpeg2, 1 mpeg1, 2 topleft", but it compares the member `d->cplace`, which nothing assigns (`new
 * JincResize()` :676; the siting string is the LOCAL `cplace` declared at :715), so the binary always takes the `else`
 * at :623-624.  A drop-in writes what the binary writes.  (Pixels are not affected: the local string drives the chroma
 * geometry, :838-841.) */
JINC_API int jinc_filter_chroma_location(const jinc_filter *f);

/* Private switch, in the manner of jinc_filter_set_simd_order: JINC_CHROMA_LOCATION_BY_SITING makes
 * jinc_filter_chroma_location return what the reference's source means to write -- 0 mpeg2, 1 mpeg1, 2 topleft, by the
 * cplace argument or frame 0's property -- for hosts that want the property to describe the chroma they get.  A
 * deliberate deviation from the reference binary; off by default. */
#define JINC_CHROMA_LOCATION_AS_REFERENCE 0
#define JINC_CHROMA_LOCATION_BY_SITING 1
JINC_API int jinc_filter_set_chroma_location_mode(jinc_filter *f, int mode);

/* The body of JincResize_GetFrame between avs_new_video_frame_p and avs_prop_set_int, i.e.
 * (d->*d->process_frame)(src, dst, vi) (ref :615), on HOST plane buffers as AviSynth hands them
 * over (avs_get_read_ptr_p / avs_get_write_ptr_p, pitches from avs_get_pitch_p in bytes).
 * Planes are indexed in the reference's processing order (ref :539-541): {Y,U,V,A} or {G,B,R,A}.
 * Synchronous: copies to the device, runs the kernels, copies back, returns when dst is complete. */
JINC_API int jinc_filter_get_frame(jinc_filter *f, const void *const src[4], const int src_pitch[4],
                                   void *const dst[4], const int dst_pitch[4]);

/* ---- Look-ahead pipeline around GetFrame (frame transport) -------------------------
 * A host that knows which frames come next (a plugin that prefetches fi->child frames n+1..n+k, a batch tool)
 * keeps up to `depth` (1..256) frames in flight per instance.  The surface stays per frame, as the reference's
 * GetFrame is (ref :603-630): jinc_filter_submit takes ONE frame (its H2D copy is queued at once) and returns a
 * ticket; jinc_filter_wait blocks until THAT frame's destination planes are complete.  In between the library
 * coalesces: `group` consecutively submitted frames share one strided device buffer and ONE set of kernel
 * launches (the batch kernels -- lanes = frames, wide tiles -- that single-frame calls cannot use), followed by one
 * D2H copy per frame.  A group leaves when it is full, when a wait asks for one of its frames, or on
 * jinc_filter_flush.  group = 0 picks depth / 2 (depth >= 8; else 1): one group computes while the client collects
 * the previous one.  src and dst must stay valid and untouched until the frame's wait returns.  Frames are
 * independent, so neither grouping nor completion order changes results.
 * register_host_buffers: how the library treats the caller's plane buffers --
 *   0 (a new instance's state)  pageable, and only the CPU ever touches them: source rows are copied into a pinned buffer of the
 *      library's own at submit (small frames in groups of four or more: when their group is launched), result rows out of one when the
 *      frame's event has fired (in jinc_filter_wait; frames nobody waits for arrive when their group buffer is reused, on
 *      jinc_filter_set_pipeline and on jinc_filter_free).  The DMA engines move whole planes between those buffers and the
 *      device; the device never maps the caller's pages.  Large planes are copied by up to six threads (a process-wide pool of
 *      helpers, idle otherwise) unless the script said threads = 1.  Costs pinned host memory of the size of the device staging
 *      (frames in flight x frame bytes, at most 4 GiB: larger groups are halved).  C2: 2 570 - 2 900 frames/s at one frame in
 *      flight, 5 280 - 6 000 at eight over four boxes (CPU work: it varies with the host; profiles/round6/host_modes*.log).
 *   3  pageable planes handed to the HIP runtime as they are (hipMemcpy2DAsync on the caller's pointers): the default of rounds
 *      1 - 5.  On this ROCm build the runtime maps the caller's pages into the device behind such a copy and keeps the mapping
 *      for a while; C2 3 879 / 4 283 frames/s.  Full test runs and one measuring script of round 6 ended in GPU memory access
 *      faults on heap addresses inside such copies; the cause was not established (profiles/round6/README.md).
 *   any other value  registered once with hipHostRegister (exactly the plane's bytes) and CACHED by address range, least recently
 *      used out: asynchronous copies, results written by the shader, no cost per frame once a buffer has been seen (C2 4 020 /
 *      5 631 / 6 125 frames/s at 1 / 8 / 128 frames in flight).  For hosts whose frame memory is a pool that STAYS MAPPED: the
 *      caller guarantees that such buffers stay allocated until jinc_filter_free or jinc_filter_set_pipeline(f, depth, 0).  The
 *      runtime consults its table of registered ranges for every host pointer it is handed, so a registration that outlives its
 *      pages makes a later buffer at those addresses travel through a dead mapping (a GPU memory access fault) or be refused
 *      (hipErrorInvalidValue when it starts inside the range and runs past its end) -- and the library cannot see a range that
 *      came back at the same addresses.  The frame memory should also OWN ITS PAGES (allocations of whole pages, as large frame
 *      buffers are): planes carved out of the malloc heap share their first and last page with whatever else lives there, and
 *      every GPU memory access fault the tests of this mode ran into in round 6 was on such a heap address; with the planes in
 *      mappings of their own they did not recur (profiles/round6/README.md).
 *   Planes inside a range the caller pinned itself (jinc_filter_adopt_host_range) travel through that mapping in every mode.
 *   Round 6 also built, measured and withdrew "registered at submit, unregistered when the frame's wait returns" (4 508 C2
 *   frames/s): registration at frame rate.
 * A failed launch is reported by the submit that triggered it and by every wait on a frame of that group.
 * jinc_filter_get_frame == submit + wait (after draining frames still in flight). */
JINC_API int jinc_filter_set_pipeline(jinc_filter *f, int depth, int register_host_buffers);
JINC_API int jinc_filter_set_pipeline_group(jinc_filter *f, int depth, int group, int register_host_buffers);
JINC_API int jinc_filter_submit(jinc_filter *f, const void *const src[4], const int src_pitch[4], void *const dst[4],
                                const int dst_pitch[4], long long *ticket);
JINC_API int jinc_filter_flush(jinc_filter *f); /* launch the frames submitted so far (no more are coming) */
/* For hosts that pin their frame memory themselves (a frame pool allocated with hipHostMalloc, or pinned once with
 * hipHostRegister(..., hipHostRegisterPortable)): tells the instance that [base, base + bytes) is pinned and stays so
 * until jinc_filter_free.  Planes inside such a range travel like planes the instance pinned itself (asynchronous
 * copies, results written by the shader), with no registration cost per frame and whatever register_host_buffers
 * says; the instance never unregisters them. */
JINC_API int jinc_filter_adopt_host_range(jinc_filter *f, void *base, size_t bytes);
/* The counterpart: the caller is about to unpin or free [base, base + bytes).  Waits for the instance's frames in flight
 * and forgets every adopted range that touches it (planes there are pageable again unless adopted anew). */
JINC_API int jinc_filter_release_host_range(jinc_filter *f, void *base, size_t bytes);
JINC_API int jinc_filter_wait(jinc_filter *f, long long ticket);

/* Same computation on DEVICE-resident planes, asynchronously on `hip_stream` (a hipStream_t; NULL is
 * the HIP null stream, i.e. ordered with the caller's default-stream work), for a batch of `nframes` independent frames (frames are the
 * sharding unit; no frame reads another).  Plane i of frame n starts at
 * src[i] + n*src_frame_stride[i] bytes (likewise dst).  Pitches/strides in bytes; sample alignment
 * required.  src and dst must not overlap.  Returns after enqueueing. */
JINC_API int jinc_filter_process_device(jinc_filter *f, const void *const src[4], const int src_pitch[4],
                                        const size_t src_frame_stride[4], void *const dst[4],
                                        const int dst_pitch[4], const size_t dst_frame_stride[4],
                                        int nframes, void *hip_stream);

/* jinc_filter_process_device on planes whose samples need not lie side by side: the semi-planar frames of video decoders
 * (NV12, P016; 10-bit samples in the LOW bits of their words -- a decoder's P010 goes through jinc_filter_process_device_shifted
 * below) and packed RGB(A).  Sample x of row y of frame n of plane i lies at
 *   base[i] + n * frame_stride[i] + y * pitch[i] + x * sample_step[i] * component_size;
 * steps are in samples, 1 .. 4 (1: dense), a NULL step array means all ones; planes keep the library's order (Y,U,V,A or
 * G,B,R,A).  NV12: U = uv, V = uv + 1 sample, both step 2.  BGRA: B = p, G = p + 1, R = p + 2, A = p + 3, all step 4.  Source
 * and destination layouts are independent.  With every step 1 the call IS jinc_filter_process_device.  Otherwise planes with
 * step 1 are used where they lie; the others are split into dense planes of the filter's own (device memory, allocated on
 * first use), resampled by the same kernels, and merged into the destination -- all ordered on `hip_stream`.
 * A step outside 1 .. 4, a strided plane whose pitch is below ((width - 1) * step + 1) * component_size, and a base that is
 * not aligned to the sample size are JINC_ERR_INVALID_ARG; nframes and frame strides as for jinc_filter_process_device.
 * The library stores to no byte of the destination that is not a sample of a plane it was given: the X of BGRX under a
 * three-component filter, row padding and the bytes between a lone strided plane's samples are not read and written back,
 * they are not written.  src and dst must not overlap; destination planes may (and normally do) share one buffer.
 * One strided call at a time uses the filter's dense planes: a later one on another stream waits for the earlier one. */
JINC_API int jinc_filter_process_device_strided(jinc_filter *f, const void *const src[4], const int src_pitch[4],
                                                const int src_sample_step[4], const size_t src_frame_stride[4],
                                                void *const dst[4], const int dst_pitch[4], const int dst_sample_step[4],
                                                const size_t dst_frame_stride[4], int nframes, void *hip_stream);

/* jinc_filter_process_device_strided on 16-bit words that hold their sample in the HIGH bits, as hardware decoders and encoders
 * write them: P010 (10 bits, shift 6), P012 (12 bits, shift 4), Y210 / Y212.  (The strided call reads and writes the sample in
 * the LOW bits of its word; what it takes as "P010" is semi-planar YUV420P10 with low-aligned samples.)  Everything is as there,
 * plus a shift in bits per plane and side; a NULL shift array means all zeros.
 *   The value of a source sample is raw >> shift: the low `shift` bits are discarded whatever they hold.  The call computes
 *   exactly what jinc_filter_process_device computes for dense planes of those values -- lrintf(clamp(r, 0, peak)) on the 10-bit
 *   value, not a rounding of the 16-bit word -- and stores result << shift as the whole sample: padding bits are written as zeros.
 * Source and destination shifts are independent (P010 in, planar low-aligned YUV420P10 out, or the reverse).
 *   P010:  Y = y, step 1; U = uv, V = uv + 1 sample, step 2; all shift 6.       P012: the same with shift 4.
 *   Y210:  Y = p, step 2; U = p + 1 sample, V = p + 3 samples, step 4; all shift 6 (filter: 4:2:2, 10 bits).
 * A shift must lie in 0 .. 8 * component_size - bits_per_component and only integer samples take a non-zero one: in practice
 * component_size 2 with 10, 12 or 14 bits.  A negative shift, a larger one, and any non-zero shift on an 8-bit, 16-bit, fp32 or
 * binary16 filter are JINC_ERR_INVALID_ARG, each with a message of its own, before anything is queued.
 * With every shift 0 the call IS jinc_filter_process_device_strided (the same launches); with every step 1 as well it is
 * jinc_filter_process_device.  A plane with a non-zero shift on a side takes a dense stand-in of the filter's own on that side
 * even at step 1, so the luma of a P010 frame lives in those dense planes too: one 1080p -> 4K frame needs about 31 MB of them
 * instead of 5.5 MB, and the 1 GiB default (knob strided_scratch_bytes, test header) cuts a long call into slices of 33 frames
 * where the unshifted call runs 128 at once.  The no-overwrite guarantee carries over: no byte of the destination is stored to
 * unless it belongs to a sample of a given plane; the padding bits inside a sample belong to it. */
JINC_API int jinc_filter_process_device_shifted(jinc_filter *f, const void *const src[4], const int src_pitch[4],
                                                const int src_sample_step[4], const int src_sample_shift[4],
                                                const size_t src_frame_stride[4], void *const dst[4], const int dst_pitch[4],
                                                const int dst_sample_step[4], const int dst_sample_shift[4],
                                                const size_t dst_frame_stride[4], int nframes, void *hip_stream);

/* jinc_filter_process_device on frames that keep three 10-bit samples in ONE 32-bit word per pixel (10:10:10:2): Y410 (4:4:4
 * 10-bit as decoders and VA-API / DXGI surfaces carry it), R10G10B10A2 / A2B10G10R10 and the DRM XRGB2101010, XBGR2101010,
 * RGBX1010102, BGRX1010102 orders (HDR10 swap chains and scan-out).  Neither a sample step nor a shift describes them: the
 * samples sit at bit offsets that are no byte offsets.
 *   A side whose field_offset array is NULL is dense planes, exactly as in jinc_filter_process_device; with both NULL the call
 *   IS that call (the same launches, on any filter).  A side with an array is ONE buffer of little-endian 32-bit words, one per
 *   pixel: only element [0] of its base, pitch and frame stride arrays is read.  Pixel x of row y of frame n is the word at
 *   base[0] + n * frame_stride[0] + y * pitch[0] + 4 * x, and its value of plane i (library order Y,U,V or G,B,R) is
 *   (word >> field_offset[i]) & 1023.  Source and destination are independent: Y410 in and planar YUV444P10 out, the reverse,
 *   or different words on the two sides.
 *   The call computes exactly what jinc_filter_process_device computes for dense low-aligned 10-bit planes of those values.
 *   Source bits outside the three fields are ignored whatever they hold (the 2-bit alpha is not resampled).  A destination word
 *   is stored whole, (r0 << o0) | (r1 << o1) | (r2 << o2) | (dst_fill & ~fields): the spare bits belong to the pixel, so
 *   dst_fill 0xC0000000 makes an opaque Y410 / A2.. word.  No byte outside the `width` words of each row of each frame is
 *   stored to: row padding and the gaps between frames stay as they are.  The destination is never read.
 * Accepted only on a filter with three components, no sub-sampling, component_size 2 and bits_per_component 10 (YUV444P10,
 * RGBP10).  Any other filter (four components, fp32 and binary16 included), an offset outside 0 .. 22, and two fields that
 * overlap are JINC_ERR_INVALID_ARG, each with a message of its own, before the device check and before anything is queued;
 * then null arguments, nframes and frame strides as for jinc_filter_process_device_shifted.  A packed base, pitch or frame
 * stride that is no multiple of 4 and a pitch below 4 * width are JINC_ERR_INVALID_ARG with nothing written.  Base, pitch and
 * frame stride that are multiples of 16 get 16-byte accesses, others dwords.
 * A packed side takes dense stand-ins of the filter's own for its three planes (the scratch of the strided call, same knob
 * strided_scratch_bytes, same ordering between calls): 3 x 2 bytes per pixel of that side, rows padded to 256 bytes.  1080p ->
 * 4K with both sides packed is 3 x 2 x (1920 x 1080 + 3840 x 2160) = 62 208 000 bytes per frame, so the 1 GiB default runs a
 * long call in slices of 17 frames (128 frames: 7 x 17 + 9); with only the source packed 86 frames fit, with only the
 * destination 21.  Callers that send long calls raise the knob. */
JINC_API int jinc_filter_process_device_packed10(jinc_filter *f, const void *const src[4], const int src_pitch[4],
                                                 const int src_field_offset[3], const size_t src_frame_stride[4],
                                                 void *const dst[4], const int dst_pitch[4], const int dst_field_offset[3],
                                                 unsigned dst_fill, const size_t dst_frame_stride[4], int nframes,
                                                 void *hip_stream);

/* jinc_filter_process_device on v210 frames: 10-bit 4:2:2 in 128-bit groups of six pixels, as SDI capture and playout cards
 * (AJA, Blackmagic, Bluefish) DMA it and as ProRes / DNxHR tool chains exchange it.  Neither a sample step, a shift nor one word
 * per pixel describes it: six pixels share four words in a pattern that repeats only every 128 bits.
 *   A row is a run of 16-byte blocks of four little-endian 32-bit words.  Block b holds luma samples 6b .. 6b+5 and samples
 *   3b .. 3b+2 of each chroma plane, three 10-bit fields per word at bits 0, 10 and 20 (bits 30 - 31 are unused):
 *       word 0: Cb[3b]   Y[6b]     Cr[3b]            word 2: Cr[3b+1] Y[6b+3]   Cb[3b+2]
 *       word 1: Y[6b+1]  Cb[3b+1]  Y[6b+2]           word 3: Y[6b+4]  Cr[3b+2]  Y[6b+5]
 *   A row of `width` luma samples occupies jinc_v210_row_bytes(width) = 16 * ceil(width / 6) bytes; the last block is partial
 *   (2 luma + 1 Cb + 1 Cr, or 4 luma + 2 Cb + 2 Cr) when width is no multiple of 6.  Writers conventionally pad rows to 128
 *   bytes (48 pixels): that padding is part of the pitch, not of the row's blocks.
 *   A side whose flag is 0 is dense planes, exactly as in jinc_filter_process_device; with both flags 0 the call IS that call
 *   (the same launches, on any filter).  A side whose flag is set is ONE buffer of blocks: only element [0] of its base, pitch
 *   and frame stride arrays is read; block b of row y of frame n lies at base[0] + n * frame_stride[0] + y * pitch[0] + 16 * b.
 *   Source and destination are independent: v210 in and planar YUV422P10 out, the reverse, or v210 on both sides.
 *   The call computes exactly what jinc_filter_process_device computes for dense low-aligned 10-bit planes Y, U = Cb, V = Cr of
 *   the field values.  Source bits 30 - 31, the fields of a partial last block beyond `width` and everything behind the row's
 *   blocks are ignored whatever they hold.  Each destination row gets exactly its jinc_v210_row_bytes(width) bytes stored,
 *   every block whole: bits 30 - 31 of every word and the unused fields of a partial last block are zeros.  No byte outside
 *   those blocks is stored to -- row padding (the 128-byte convention included) and the gaps between frames stay as they are.
 *   The destination is never read.
 * Accepted only on a filter with three components, sub_w 1 and sub_h 0, component_size 2 and bits_per_component 10, not
 * binary16 (YUV422P10).  Any other filter with a flag set is JINC_ERR_INVALID_ARG, before the null checks of the plane arrays
 * and before the device check; then null arguments, nframes and frame strides as for jinc_filter_process_device_shifted.  A
 * v210 base, pitch or frame stride that is no multiple of 4 and a pitch below jinc_v210_row_bytes(width) are
 * JINC_ERR_INVALID_ARG, each with a message of its own and with nothing written.  Base, pitch and frame stride that are all
 * multiples of 16 get 16-byte accesses on the block side, others dwords.
 * A v210 side takes dense stand-ins of the filter's own for its three planes (the scratch of the strided call, same knob
 * strided_scratch_bytes, same ordering between calls, so these calls may alternate with strided, shifted and packed10 ones on
 * one filter): 4 bytes per pixel of that side, rows padded to 256 bytes.  1080p -> 4K with both sides v210: the source's chroma
 * rows of 960 x 2 = 1920 bytes are padded to 2048, the other rows (3840, 7680, 3840 bytes) are multiples of 256 already, so a
 * frame needs (3840 + 2 x 2048) x 1080 + (7680 + 2 x 3840) x 2160 = 8 570 880 + 33 177 600 = 41 748 480 bytes and the 1 GiB
 * default runs a long call in slices of 25 frames (128 frames: 5 x 25 + 3); with only the source v210 125 frames fit (128 frames:
 * 125 + 3), with only the destination 32. */
JINC_API int jinc_filter_process_device_v210(jinc_filter *f, const void *const src[4], const int src_pitch[4], int src_is_v210,
                                             const size_t src_frame_stride[4], void *const dst[4], const int dst_pitch[4],
                                             int dst_is_v210, const size_t dst_frame_stride[4], int nframes, void *hip_stream);

/* Bytes of the blocks of one v210 row of `width` luma samples: 16 * ceil(width / 6); 0 for width < 1.  Needs no device. */
JINC_API size_t jinc_v210_row_bytes(int width);

/* INTEGER device frames into an fp32 or binary16 filter: a decoder's NV12 / P010 surface resampled straight into the float or half
 * planes a network reads, with nothing rounded to a code value on the way.
 *   `f` is an fp32 filter (bits_per_component 32) or a binary16 filter (JINC_SAMPLE_FLOAT16); its geometry, number of components
 *   and sub-sampling describe the frame exactly as for jinc_filter_process_device_strided.
 *   The SOURCE is integer samples, addressed exactly as in jinc_filter_process_device_shifted (base, pitch, step 1 .. 4 in samples,
 *   shift, frame stride; NULL step and shift arrays mean all ones and all zeros), but the sample size comes from src_bits, not from
 *   the filter: src_bits 8 is 1-byte samples, src_bits 9 .. 16 little-endian 2-byte words.  Sample x of row y of frame n of plane i
 *   lies at base[i] + n * frame_stride[i] + y * pitch[i] + x * step[i] * bytes, a shift lies in 0 .. 8 * bytes - src_bits, and the
 *   value of a source sample is (raw >> shift) & ((1 << src_bits) - 1): whatever lies below and above the sample is ignored.  The
 *   source is never written.
 *   The DESTINATION is float / half planes of the filter's own type: exactly the dst side of jinc_filter_process_device_strided on
 *   that filter, steps included (interleaved RGB float output through the same merge), with the same no-overwrite guarantee.
 *     NV12 into YUV420PS:           Y = y, step 1; U = uv, V = uv + 1 sample, step 2; src_bits 8.
 *     P010 into YUV420PH or PS:     the same with src_bits 10 and all shifts 6.
 *     BGRA8 into RGBPS:             G = p + 1, B = p, R = p + 2, all step 4; src_bits 8.
 *     planar YUV420P10:             steps 1, shifts 0, src_bits 10.
 *   The result is exactly what jinc_filter_process_device computes on that filter for dense planes holding those values converted
 *   to the filter's sample type (the conversion is exact): the same plan, the same un-fused chain, the trimmed support (integer
 *   values are always finite), nothing clamped, and for half filters the same round-to-nearest-even narrowing of the fp32 sum.
 *   Since the integer filters convert every source sample to float before the multiply, the fp32 result is their sum in front of
 *   clamp and lrintf.
 *   A binary16 filter needs src_bits <= 11, so that every value is exact in binary16 (8-bit and 10-bit sources: NV12, P010, Y210);
 *   wider samples go into an fp32 filter.  A bfloat16 filter (JINC_SAMPLE_BFLOAT16) needs src_bits == 8 for the same reason: its
 *   eight significant bits hold every integer up to 256 and no 9-bit sample (NV12, BGRA8 and planar 8-bit frames; NV12 into
 *   YUV420PBF is the first line above with a bfloat16 filter).
 * JINC_ERR_INVALID_ARG, each with a message of its own, before the device check and before anything is queued: an integer filter;
 * src_bits outside 8 .. 16; src_bits above 11 on a binary16 filter; src_bits above 8 on a bfloat16 filter; a step outside 1 .. 4 (either side); a shift outside its range;
 * a source base not aligned to the source sample size; a source pitch below ((width - 1) * step + 1) * bytes of that plane.  Then
 * null arguments, nframes and frame strides as for jinc_filter_process_device_shifted.
 * EVERY source plane takes a dense float / half stand-in of the filter's own (the scratch of the strided call: same knob
 * strided_scratch_bytes, same slicing of long calls, same ordering between calls, so these calls may alternate with strided ones
 * on one filter), rows padded to 256 bytes; a destination plane takes one only where its step is not 1.  1080p -> 4K NV12 into
 * planar fp32: 1920 x 4 = 7680 and 960 x 4 = 3840 bytes per row are multiples of 256 already, so a frame needs 7680 x 1080 +
 * 2 x 3840 x 540 = 12 441 600 bytes and the 1 GiB default holds floor(1 073 741 824 / 12 441 600) = 86 frames (a call of 128 runs
 * as 86 + 42); P010 into planar binary16 needs half of that, 6 220 800 bytes, 172 frames: a call of 128 in one slice.
 * Y410 / RGB10A2 words and v210 blocks have calls of their own: jinc_filter_process_device_widened_packed10 / _v210 below. */
JINC_API int jinc_filter_process_device_widened(jinc_filter *f, const void *const src[4], const int src_pitch[4],
                                                const int src_sample_step[4], const int src_sample_shift[4], int src_bits,
                                                const size_t src_frame_stride[4], void *const dst[4], const int dst_pitch[4],
                                                const int dst_sample_step[4], const size_t dst_frame_stride[4], int nframes,
                                                void *hip_stream);

/* The results of an fp32, binary16 or bfloat16 filter into INTEGER device frames: what a network leaves in float / half / bfloat16
 * planes, in code-value units, resampled in float and written straight into an encoder's or a display's NV12 / P010 / Y210 / BGRA
 * surface.  The way back out of jinc_filter_process_device_widened.
 *   `f` is an fp32 filter (bits_per_component 32), a binary16 filter (JINC_SAMPLE_FLOAT16) or a bfloat16 filter
 *   (JINC_SAMPLE_BFLOAT16); its geometry, number of components and sub-sampling describe the frame exactly as for
 *   jinc_filter_process_device_strided.
 *   The SOURCE is exactly the src side of jinc_filter_process_device_strided on that filter: planes of the filter's own type, steps
 *   1 .. 4 (NULL: all ones).  The source is never written.
 *   The DESTINATION is integer samples, addressed exactly as the dst side of jinc_filter_process_device_shifted (base, pitch, step
 *   1 .. 4 in samples, shift, frame stride; NULL step and shift arrays mean all ones and all zeros), but the sample size comes from
 *   dst_bits, not from the filter: dst_bits 8 is 1-byte samples, dst_bits 9 .. 16 little-endian 2-byte words.  Sample x of row y of
 *   frame n of plane i lies at base[i] + n * frame_stride[i] + y * pitch[i] + x * step[i] * bytes, a shift lies in
 *   0 .. 8 * bytes - dst_bits, and the stored sample is value << shift as the whole byte / word: padding bits are zeros.
 *     NV12 from YUV420PS / PH:      Y = y, step 1; U = uv, V = uv + 1 sample, step 2; dst_bits 8.
 *     P010 / P012:                  the same with dst_bits 10 / 12 and all shifts 6 / 4.
 *     Y210 from YUV422PS:           Y = p, step 2; U = p + 1, V = p + 3 samples, step 4, one buffer; dst_bits 10, shifts 6.
 *     BGRA8 from RGBPS:             G = p + 1, B = p, R = p + 2, all step 4; dst_bits 8 (the X bytes are not stored to).
 *     planar YUV420P10:             steps 1, shifts 0, dst_bits 10.
 *   DEFINITION.  Let r be what jinc_filter_process_device stores on that filter for the same source planes, widened exactly to
 *   fp32, and peak = (1 << dst_bits) - 1.  Then value = lrintf(clamp(r, 0, peak)), round half to even; a NaN becomes 0, -inf and -0
 *   become 0, +inf becomes peak: the step the integer filters end in.  For binary16 and bfloat16 filters r is the ALREADY NARROWED
 *   16-bit result, so such a call rounds twice -- once to the filter's type, once to the code value; an fp32 filter rounds once.
 *   CONSEQUENCE.  The integer filters convert every source sample to float before the multiply, so on an fp32 filter whose source
 *   planes hold integers in 0 .. peak, with dst_bits equal to an integer format's depth, the result equals that integer filter's
 *   jinc_filter_process_device output, bit for bit.
 *   No scale or offset lies between the float range and the code values here (jinc_filter_process_device_narrowed_scaled below
 *   has one), nothing is dithered, no colour is converted.
 * As in the shifted call: no destination byte is stored to unless it belongs to a sample of a given plane (the X of BGRX under a
 * three-component filter, row padding and gaps between frames keep their values), the destination is never read, and destination
 * planes may share a buffer.
 * JINC_ERR_INVALID_ARG, each with a message of its own, before the device check and before anything is queued: an integer filter;
 * dst_bits outside 8 .. 16; a step outside 1 .. 4 (either side); a negative shift; a shift above its range; a destination base not
 * aligned to the destination sample size; a destination pitch below ((width - 1) * step + 1) * bytes of that plane.  Then null
 * arguments, nframes and frame strides as for jinc_filter_process_device_shifted; a destination pitch or frame stride that is no
 * multiple of the destination sample size is refused behind the device check.  Destination base, pitch and frame stride that are
 * all multiples of 16 get 16-byte stores, all multiples of 4 dwords, others sample-sized stores.
 * EVERY destination plane takes a dense stand-in of the filter's own type (the scratch of the strided call: same knob
 * strided_scratch_bytes, same slicing of long calls, same ordering between calls, so these calls may alternate with strided,
 * shifted, packed and widened ones on one filter), rows padded to 256 bytes; a source plane takes one only where its step is not 1.
 * 1080p -> 4K from planar fp32 into NV12: 3840 x 4 = 15 360 and 1920 x 4 = 7680 bytes per row are multiples of 256 already, so a
 * frame needs 15 360 x 2160 + 2 x 7680 x 1080 = 49 766 400 bytes and the 1 GiB default holds floor(1 073 741 824 / 49 766 400) = 21
 * frames (a call of 128 runs as 6 x 21 + 2); from binary16 or bfloat16 half of that, 24 883 200 bytes, 43 frames (43 + 43 + 42).
 * 10:10:10:2 words and v210 blocks are destinations of jinc_filter_process_device_narrowed_packed10 / _narrowed_v210 below. */
JINC_API int jinc_filter_process_device_narrowed(jinc_filter *f, const void *const src[4], const int src_pitch[4],
                                                 const int src_sample_step[4], const size_t src_frame_stride[4], void *const dst[4],
                                                 const int dst_pitch[4], const int dst_sample_step[4], const int dst_sample_shift[4],
                                                 int dst_bits, const size_t dst_frame_stride[4], int nframes, void *hip_stream);

/* The widened and the narrowed call with a SCALE and an OFFSET between code values and the float range: networks read 0 .. 1, or
 * (v - 16) / 219 for limited-range luma and (v - 128) / 224 for chroma, not code values, and the arithmetic runs where the samples
 * are in registers already instead of in a pass of the caller's over the float planes.
 *   The argument lists are those of jinc_filter_process_device_widened / _narrowed plus two arrays of four floats in the
 *   library's plane order (Y,U,V or G,B,R, then A).  A NULL scale array means all 1.0; a NULL offset array means all 0.0.
 *   WIDENED.  Let v = (raw >> shift[i]) & ((1 << src_bits) - 1).  The sample of plane i is
 *       s = fl32(fl32(float(v) * src_scale[i]) + src_offset[i]).
 *   That is two fp32 roundings and never an FMA.  An fp32 filter holds s.  A binary16 filter holds s narrowed
 *   round-to-nearest-even: overflow to +-inf, subnormals kept.  A bfloat16 filter holds s narrowed round-to-nearest-even, by the
 *   rule its results are stored with (+-inf from 0x7f7f8000 on, subnormals kept).  The call's result is exactly what
 *   jinc_filter_process_device computes on that filter for dense planes holding those samples.
 *   NARROWED.  Let r be what jinc_filter_process_device stores for the same source planes, widened exactly to fp32.  The stored
 *   sample is
 *       lrintf(clamp(fl32(fl32(r * dst_scale[i]) + dst_offset[i]), 0, peak)) << shift[i].
 *   Everything else is as in the narrowed call: NaN -> 0, +inf -> peak, padding bits zero, the destination is never read, no byte
 *   outside a given sample is stored to.
 *   BOTH ARRAYS NULL.  The call IS the existing call.  It makes the same launches, the same refusals and the same
 *   jinc_debug_last_strided report.  The src_bits <= 11 and src_bits = 8 rules for half and bfloat16 filters still apply.
 *   EITHER ARRAY NON-NULL.  The scaled form runs.  src_bits 8 .. 16 is accepted for all three float types, because the conversion
 *   is a defined rounding and not a claim of exactness: P010 into bfloat16 planes and P016 into half planes, normalised.
 *     NV12 into YUV420PH, limited range in 0 .. 1:  jinc_code_range(8, JINC_RANGE_LIMITED, JINC_PLANE_LUMA_OR_RGB, ...) gives
 *     src_scale[0] / src_offset[0], JINC_PLANE_CHROMA those of planes 1 and 2; the to_code pair is the way back for the narrowed call.
 * JINC_ERR_INVALID_ARG, each with a message of its own that names the side and the plane, before the device check and before
 * anything is queued: a scale or offset of a used plane (index below the filter's number of components) that is NaN or infinite; a
 * scale that is zero.  All refusals of the underlying call stay as they are, with the same texts, and come first.
 * Stand-ins, slicing under strided_scratch_bytes, the order on the caller's stream and the jinc_debug_last_strided counts are exactly
 * those of the unscaled calls: the scaled form adds no pass and no launch, only one multiply and one add per sample in the widening /
 * narrowing kernel. */
JINC_API int jinc_filter_process_device_widened_scaled(jinc_filter *f, const void *const src[4], const int src_pitch[4],
                                                       const int src_sample_step[4], const int src_sample_shift[4], int src_bits,
                                                       const float src_scale[4], const float src_offset[4],
                                                       const size_t src_frame_stride[4], void *const dst[4], const int dst_pitch[4],
                                                       const int dst_sample_step[4], const size_t dst_frame_stride[4], int nframes,
                                                       void *hip_stream);
JINC_API int jinc_filter_process_device_narrowed_scaled(jinc_filter *f, const void *const src[4], const int src_pitch[4],
                                                        const int src_sample_step[4], const size_t src_frame_stride[4],
                                                        void *const dst[4], const int dst_pitch[4], const int dst_sample_step[4],
                                                        const int dst_sample_shift[4], int dst_bits, const float dst_scale[4],
                                                        const float dst_offset[4], const size_t dst_frame_stride[4], int nframes,
                                                        void *hip_stream);

/* Scale and offset between the code values of a `bits`-bit plane (8 .. 16) and the float range 0 .. 1 (luma, RGB) or -0.5 .. 0.5
 * (chroma), for the two calls above.  Needs no device.  With k = 2^(bits - 8):
 *       range, plane kind            den            zero
 *       limited, luma or RGB         219 k          16 k
 *       limited, chroma              224 k          128 k
 *       full, luma or RGB            2^bits - 1     0
 *       full, chroma                 2^bits - 1     2^(bits - 1)
 *   to_float_scale = (float)(1.0 / den) and to_float_offset = (float)(-(double)zero / den): both are computed in double and
 *   rounded once.  to_code_scale = (float)den and to_code_offset = (float)zero: both are exact.  Any pointer may be NULL.
 * bits outside 8 .. 16, another range or another plane kind is JINC_ERR_INVALID_ARG. */
#define JINC_RANGE_FULL 0
#define JINC_RANGE_LIMITED 1
#define JINC_PLANE_LUMA_OR_RGB 0
#define JINC_PLANE_CHROMA 1
JINC_API int jinc_code_range(int bits, int range, int plane_kind, float *to_float_scale, float *to_float_offset, float *to_code_scale,
                             float *to_code_offset);

/* 10:10:10:2 WORDS into an fp32 or binary16 filter: the HDR 4:4:4 surface of decoders and swap chains (Y410, R10G10B10A2, the DRM
 * 2101010 / 1010102 orders) resampled straight into the float or half planes a network reads, with nothing rounded to a code value
 * and nothing clamped on the way.
 *   `f` is an fp32 or binary16 filter with three components and no sub-sampling (YUV444PS, YUV444PH, RGBPS, RGBPH).
 *   The SOURCE is ONE buffer of little-endian 32-bit words, one per pixel, addressed exactly as the packed side of
 *   jinc_filter_process_device_packed10: pixel x of row y of frame n is the word at src + n * src_frame_stride + y * src_pitch +
 *   4 * x and its value of plane i (library order Y,U,V or G,B,R; jinc_packed10_layout gives the offsets in that order) is
 *   (word >> src_field_offset[i]) & 1023.  Source bits outside the three fields and everything behind a row's `width` words are
 *   ignored whatever they hold (the 2-bit alpha is not resampled).  The source is never written.  src_frame_stride is read only
 *   for nframes > 1.
 *   The DESTINATION is exactly the dst side of jinc_filter_process_device_widened, which is the strided call's: the filter's own
 *   float / half planes with steps 1 .. 4 (NULL: all ones; interleaved float RGB through the same merge), with the same
 *   no-overwrite guarantee.
 *   The result is exactly what jinc_filter_process_device computes on that filter for dense planes holding the field values
 *   converted to the filter's sample type.  Ten bits are exact in fp32 and in binary16 alike, so half filters need no extra rule.
 *   The same plan, the same un-fused chain, the same finite scan (which finds nothing), and for half filters the same
 *   round-to-nearest-even narrowing of the fp32 sum.  Ten bits are NOT exact in bfloat16: a bfloat16 filter is refused.
 * JINC_ERR_INVALID_ARG, each with a message of its own, before the null checks of the plane arrays, before the device check and
 * before anything is queued: an integer filter; a bfloat16 filter; a float filter of another shape (four components, sub-sampled
 * chroma, a single plane); an offset outside 0 .. 22; two fields that overlap; a destination step outside 1 .. 4; a source base, a source pitch or
 * (with nframes > 1) a source frame stride that is no multiple of 4; a source pitch below 4 * width.  Then null arguments, nframes
 * and frame strides as for jinc_filter_process_device_shifted.  Base, pitch and frame stride that are all multiples of 16 get
 * 16-byte loads, others dwords.
 * The three source planes take dense stand-ins of the filter's own type (the scratch of the strided call: same knob
 * strided_scratch_bytes, same slicing of long calls, same ordering between calls, so these calls may alternate with strided and
 * widened ones on one filter), rows padded to 256 bytes; a destination plane takes one only where its step is not 1.  1080p Y410
 * into planar fp32: rows of 1920 x 4 = 7680 bytes are multiples of 256 already, so a frame needs 3 x 7680 x 1080 = 24 883 200
 * bytes and the 1 GiB default holds floor(1 073 741 824 / 24 883 200) = 43 frames (a call of 128 runs as 43 + 43 + 42); into planar
 * binary16 3 x 3840 x 1080 = 12 441 600 bytes, 86 frames (86 + 42). */
JINC_API int jinc_filter_process_device_widened_packed10(jinc_filter *f, const void *src, int src_pitch,
                                                         const int src_field_offset[3], size_t src_frame_stride,
                                                         void *const dst[4], const int dst_pitch[4],
                                                         const int dst_sample_step[4], const size_t dst_frame_stride[4],
                                                         int nframes, void *hip_stream);

/* v210 BLOCKS into an fp32 or binary16 filter: the SDI / ProRes 4:2:2 surface resampled straight into float or half planes.
 *   `f` is an fp32 or binary16 filter with three components, sub_w 1 and sub_h 0 (YUV422PS, YUV422PH).
 *   The SOURCE is ONE buffer of blocks, addressed exactly as the v210 side of jinc_filter_process_device_v210 (the field table is
 *   there): block b of row y of frame n lies at src + n * src_frame_stride + y * src_pitch + 16 * b, and a row of `width` luma
 *   samples is jinc_v210_row_bytes(width) bytes.  Bits 30 - 31 of every word, the fields of a partial last block beyond `width`
 *   and everything behind the row's blocks (the conventional 128-byte padding included) are ignored whatever they hold.  The
 *   source is never written.  src_frame_stride is read only for nframes > 1.
 *   DESTINATION and result are as for jinc_filter_process_device_widened_packed10, with planes Y, U = Cb, V = Cr.
 * JINC_ERR_INVALID_ARG, each with a message of its own, before the null checks of the plane arrays, before the device check and
 * before anything is queued: an integer filter; a bfloat16 filter (ten bits are not exact in bfloat16); a float filter of another
 * shape (four components, no or another sub-sampling, a single plane); a destination step outside 1 .. 4; a source base, a source pitch or (with nframes > 1) a source frame stride
 * that is no multiple of 4; a source pitch below jinc_v210_row_bytes(width).  Then null arguments, nframes and frame strides as
 * for jinc_filter_process_device_shifted.  Base, pitch and frame stride that are all multiples of 16 get one 16-byte load per
 * block, others four dwords.
 * Stand-ins as above.  1080p v210 into planar fp32: rows of 7680 and 3840 bytes, (7680 + 2 x 3840) x 1080 = 16 588 800 bytes a
 * frame, floor(1 073 741 824 / 16 588 800) = 64 frames under the 1 GiB default (a call of 128 runs as 64 + 64); into planar
 * binary16 the chroma rows of 960 x 2 = 1920 bytes are padded to 2048: (3840 + 2 x 2048) x 1080 = 8 570 880 bytes, 125 frames
 * (125 + 3). */
JINC_API int jinc_filter_process_device_widened_v210(jinc_filter *f, const void *src, int src_pitch, size_t src_frame_stride,
                                                     void *const dst[4], const int dst_pitch[4], const int dst_sample_step[4],
                                                     const size_t dst_frame_stride[4], int nframes, void *hip_stream);

/* The two calls above with a SCALE and an OFFSET per plane between the 10-bit code values and the float range, as
 * jinc_filter_process_device_widened_scaled has them: a Y410 swap-chain frame or a v210 capture frame straight into float, half or
 * bfloat16 planes in the range a network reads, with no pass of the caller's over three float planes per frame.
 *   The argument lists are those of jinc_filter_process_device_widened_packed10 / _widened_v210 plus two arrays of THREE floats in
 *   the library's plane order (Y,U,V / G,B,R; v210: Y, Cb, Cr).  A NULL scale array means all 1.0; a NULL offset array all 0.0.
 *   DEFINITION.  Let v = (word >> src_field_offset[i]) & 1023 (words) or the 10-bit field of the block (v210).  The sample of
 *   plane i is
 *       s = fl32(fl32(float(v) * src_scale[i]) + src_offset[i]).
 *   That is two fp32 roundings and never an FMA.  An fp32 filter holds s.  A binary16 filter holds s rounded to nearest even
 *   (overflow to +-inf, subnormals kept).  A bfloat16 filter holds s rounded to nearest even by the rule its results are stored
 *   with.  The call's result is exactly what jinc_filter_process_device computes on that filter for dense planes holding those
 *   samples.
 *   BOTH ARRAYS NULL.  The call IS the unscaled call: the same launches, the same jinc_debug_last_strided report, the same
 *   refusals with the same texts -- bfloat16 filters included.
 *   EITHER ARRAY NON-NULL.  fp32, binary16 AND bfloat16 filters of the right shape are accepted (words: three components, no
 *   sub-sampling; blocks: 4:2:2), because the conversion is a defined rounding and not a claim of exactness.
 *     Y410 limited range into YUV444PH in 0 .. 1: jinc_code_range(10, JINC_RANGE_LIMITED, JINC_PLANE_LUMA_OR_RGB, ...) gives
 *     src_scale[0] / src_offset[0], JINC_PLANE_CHROMA those of planes 1 and 2; the to_code pairs are dst_scale / dst_offset of
 *     jinc_filter_process_device_narrowed_packed10 / _narrowed_v210, the way back.
 * JINC_ERR_INVALID_ARG: every refusal of the unscaled call stays, with its text, and comes first.  Then, before the null checks of
 * the plane arrays, before the device check and before anything is queued: a scale that is NaN, infinite or zero and an offset that
 * is NaN or infinite (the message names the plane).
 * Stand-ins, slicing under strided_scratch_bytes, the order on the caller's stream and the jinc_debug_last_strided counts are those
 * of the unscaled calls: the scaled form adds no pass and no launch, only one multiply and one add per sample in the widening
 * kernel.  A bfloat16 filter's stand-ins have the binary16 sizes.
 * Not covered: host-plane surfaces and the plugin shells, the 2-bit alpha, four-component filters, colour conversion. */
JINC_API int jinc_filter_process_device_widened_packed10_scaled(jinc_filter *f, const void *src, int src_pitch,
                                                                const int src_field_offset[3], const float src_scale[3],
                                                                const float src_offset[3], size_t src_frame_stride,
                                                                void *const dst[4], const int dst_pitch[4],
                                                                const int dst_sample_step[4], const size_t dst_frame_stride[4],
                                                                int nframes, void *hip_stream);
JINC_API int jinc_filter_process_device_widened_v210_scaled(jinc_filter *f, const void *src, int src_pitch, const float src_scale[3],
                                                            const float src_offset[3], size_t src_frame_stride, void *const dst[4],
                                                            const int dst_pitch[4], const int dst_sample_step[4],
                                                            const size_t dst_frame_stride[4], int nframes, void *hip_stream);

/* The results of an fp32, binary16 or bfloat16 filter into 10:10:10:2 WORDS or v210 BLOCKS: the way back out of the float planes
 * for the two 10-bit surfaces that no step and no shift describes -- a swap chain's or encoder's Y410 / R10G10B10A2 frame, a
 * playout card's v210 frame -- with the optional scale and offset of the scaled calls built in, so that no clamp / round / pack
 * pass of the caller's and no rounding to 10 bits in front of an integer filter is needed.
 *   `f` is an fp32, binary16 (JINC_SAMPLE_FLOAT16) or bfloat16 (JINC_SAMPLE_BFLOAT16) filter with three components.  Words take a
 *   filter with no sub-sampling (YUV444PS / PH, RGBPS / PH and their bfloat16 twins); blocks take one with sub_w 1 and sub_h 0
 *   (YUV422PS / PH / bfloat16).  bfloat16 is accepted here, unlike in the widened word calls: the conversion to a code value is a
 *   defined rounding, not a claim of exactness, exactly as in jinc_filter_process_device_narrowed.
 *   The SOURCE is exactly the src side of jinc_filter_process_device_narrowed, which is the strided call's: planes of the filter's
 *   own type with steps 1 .. 4 (NULL: all ones).  The source is never written.
 *   The DESTINATION is ONE buffer, given as scalars and addressed exactly as the packed side of
 *   jinc_filter_process_device_packed10 (pixel x of row y of frame n is the word at dst + n * dst_frame_stride + y * dst_pitch +
 *   4 * x) or the v210 side of jinc_filter_process_device_v210 (a row is jinc_v210_row_bytes(out_width) bytes of 16-byte blocks;
 *   the field table is above).  dst_frame_stride is read only for nframes > 1.
 *   DEFINITION.  Let r_i be what jinc_filter_process_device stores on that filter for plane i (library order Y,U,V / G,B,R),
 *   widened exactly to fp32 -- for binary16 / bfloat16 the already narrowed result, so such a call rounds twice, as the narrowed
 *   call does.  t_i = r_i when both arrays are NULL, otherwise t_i = fl32(fl32(r_i * dst_scale[i]) + dst_offset[i]) (a NULL scale
 *   array means 1.0, a NULL offset array 0.0): two fp32 roundings and never an FMA.  v_i = lrintf(clamp(t_i, 0, 1023)), round half
 *   to even; a NaN, -inf and -0 become 0, +inf becomes 1023.
 *   WORDS: the stored word is (v0 << o0) | (v1 << o1) | (v2 << o2) | (dst_fill & ~fields), o_i = dst_field_offset[i]
 *   (jinc_packed10_layout gives offsets and the opaque fill).  The word is stored whole; nothing outside the `width` words of a row
 *   is stored to.
 *   BLOCKS: every block of the row is built in registers and stored whole, bits 30 - 31 zero, the fields of a partial last block
 *   beyond `width` zero.  Nothing outside the row's blocks is stored to: the conventional 128-byte padding keeps its bytes.
 *   The destination is never read.
 *   CONSEQUENCES.  (a) On an fp32 filter whose planes hold integers in 0 .. 1023, with no scale and no offset, the buffer equals what
 *   jinc_filter_process_device_packed10 on YUV444P10 / RGBP10, or jinc_filter_process_device_v210 on YUV422P10, stores for the same
 *   values with the same offsets and fill, bit for bit.  (b) For every filter type the field values equal what
 *   jinc_filter_process_device_narrowed (or _narrowed_scaled when arrays are given) stores with dst_bits 10, steps 1 and shifts 0
 *   into planar words.
 * JINC_ERR_INVALID_ARG, each with a message of its own, before the null checks of the plane arrays, before the device check and
 * before anything is queued: an integer filter; a float filter of another shape (four components, a single plane, the wrong
 * sub-sampling); an offset outside 0 .. 22; two fields that overlap; a source step outside 1 .. 4; a destination base, a destination
 * pitch or (with nframes > 1) a destination frame stride that is no multiple of 4; a destination pitch below 4 * width (words) or
 * jinc_v210_row_bytes(width) (blocks); a scale that is NaN, infinite or zero and an offset that is NaN or infinite (the message
 * names the plane).  Then null arguments, nframes and frame strides as for jinc_filter_process_device_shifted.  Base, pitch and
 * frame stride that are all multiples of 16 get 16-byte stores, others dwords.
 * The three destination planes take dense stand-ins of the filter's own type (the scratch of the strided call: same knob
 * strided_scratch_bytes, same slicing of long calls, same ordering between calls, so these calls may alternate with strided,
 * shifted, packed10, v210, widened and narrowed ones on one filter), rows padded to 256 bytes; a source plane takes one only where
 * its step is not 1.  jinc_debug_last_strided counts the pass as one merge launch per slice.  1080p -> 4K from a planar source
 * (4K rows of 15 360, 7680 and 3840 bytes are multiples of 256 already; every count is below the 128-frame rounding of long
 * slices, so none is rounded):
 *     Y410 from fp32              3 x 15 360 x 2160 = 99 532 800 bytes        floor(1 073 741 824 / 99 532 800) = 10 frames (128 = 12 x 10 + 8)
 *     Y410 from a 16-bit type     3 x 7680 x 2160 = 49 766 400 bytes          21 frames (6 x 21 + 2)
 *     v210 from fp32              (15 360 + 2 x 7680) x 2160 = 66 355 200     16 frames (8 x 16)
 *     v210 from a 16-bit type     (7680 + 2 x 3840) x 2160 = 33 177 600       32 frames (4 x 32)
 * Not covered: host-plane surfaces and the plugin shells, the 2-bit alpha as a resampled plane (it comes from dst_fill),
 * four-component filters, colour conversion and dithering. */
JINC_API int jinc_filter_process_device_narrowed_packed10(jinc_filter *f, const void *const src[4], const int src_pitch[4],
                                                          const int src_sample_step[4], const size_t src_frame_stride[4], void *dst,
                                                          int dst_pitch, const int dst_field_offset[3], unsigned dst_fill,
                                                          const float dst_scale[3], const float dst_offset[3],
                                                          size_t dst_frame_stride, int nframes, void *hip_stream);
JINC_API int jinc_filter_process_device_narrowed_v210(jinc_filter *f, const void *const src[4], const int src_pitch[4],
                                                      const int src_sample_step[4], const size_t src_frame_stride[4], void *dst,
                                                      int dst_pitch, const float dst_scale[3], const float dst_offset[3],
                                                      size_t dst_frame_stride, int nframes, void *hip_stream);

/* The field offsets of a named 10:10:10:2 word in the library's plane order, and the fill that sets every spare bit (an opaque
 * pixel); opaque_fill may be NULL.  Needs no device.  Names match without regard to case; an unknown one is
 * JINC_ERR_INVALID_ARG.
 *   Y410                                                  {10,  0, 20}   U 0, Y 10, V 20, A 30
 *   R10G10B10A2 (DXGI) = DRM ABGR2101010 / XBGR2101010    {10, 20,  0}   R 0, G 10, B 20       (planes G, B, R)
 *   XRGB2101010 / ARGB2101010                             {10,  0, 20}   B 0, G 10, R 20
 *   RGBX1010102 / RGBA1010102                             {12,  2, 22}   B 2, G 12, R 22
 *   BGRX1010102 / BGRA1010102                             {12, 22,  2}   R 2, G 12, B 22 */
JINC_API int jinc_packed10_layout(const char *name, int field_offset[3], unsigned *opaque_fill);

/* Block until everything enqueued on the filter's own stream (jinc_filter_get_frame) has finished.
 * Work given to jinc_filter_process_device is synchronised by the caller through its stream. */
JINC_API int jinc_filter_sync(jinc_filter *f);

/* ---- Frames of a clip sharded over the HIP devices of the node (BASELINE.json configs[4]) --------
 * Frames are independent units (JincResize_GetFrame touches frame n only, ref :603-630) and the plan is read-only, so
 * the shard needs no exchange between devices: frame n is computed on device jinc_shard_device(n, G) = n mod G, every
 * device holds a replica of the plan (one filter instance) and keeps `streams_per_device` (1..256) frames in flight
 * through the look-ahead pipeline above (frames coalesced into groups of streams_per_device / 2 per launch), driven by
 * one host thread per device.  No collective.
 * ndevices <= 0: all visible devices.  register_host_buffers: 0 pageable, copied through the instances' own pinned buffers; 3 pageable,
 * handed to the runtime; any other value: the planes of a jinc_batch_process call are
 * pinned by one registrar thread per device running ahead of the submissions (exact byte ranges, planes that follow each
 * other merged) and stay pinned until jinc_batch_free: the caller keeps them allocated until then (a caller that re-uses its
 * planes call after call pays once).  The worker and the registrar of device d run on the CPUs of d's NUMA node (sysfs numa_node of the
 * device's PCI function); jinc_batch_set_affinity(b, 0) leaves the threads where the scheduler puts them.
 * jinc_batch_device_cpus: the CPUs found for the batch's device_index-th device (returns their number, 0 if unknown).
 * jinc_batch_process: src_planes / dst_planes hold 4 pointers per frame ([frame][plane], planes in the reference's
 * processing order, unused planes NULL), HOST buffers with the given pitches (bytes); returns when every frame is
 * complete.  Errors: first failure's status, message from jinc_batch_last_error(). */
typedef struct jinc_batch jinc_batch;
JINC_API int jinc_shard_device(int frame, int ndevices);
JINC_API int jinc_batch_create(const jinc_video_info *vi, const jinc_args *args, int ndevices, int streams_per_device,
                               int register_host_buffers, jinc_batch **out, char *err, size_t err_len);
/* jinc_batch_create with a sample type (JINC_SAMPLE_DEFAULT / JINC_SAMPLE_FLOAT16 / JINC_SAMPLE_BFLOAT16, as jinc_filter_create_ex). */
JINC_API int jinc_batch_create_ex(const jinc_video_info *vi, const jinc_args *args, int sample_type, int ndevices,
                                  int streams_per_device, int register_host_buffers, jinc_batch **out, char *err, size_t err_len);
/* jinc_batch_create_ex with the output's chroma sub-sampling (-1, -1: the input's), as jinc_filter_create_out. */
JINC_API int jinc_batch_create_out(const jinc_video_info *vi, const jinc_args *args, int sample_type, int out_sub_w, int out_sub_h,
                                   int ndevices, int streams_per_device, int register_host_buffers, jinc_batch **out, char *err,
                                   size_t err_len);
JINC_API int jinc_batch_devices(const jinc_batch *b);
JINC_API int jinc_batch_set_affinity(jinc_batch *b, int on);
JINC_API int jinc_batch_device_cpus(const jinc_batch *b, int device_index, int *cpus, int max_cpus);
JINC_API int jinc_batch_device_of_frame(const jinc_batch *b, int frame);
JINC_API int jinc_batch_process(jinc_batch *b, int nframes, const void *const *src_planes, const int src_pitch[4],
                                void *const *dst_planes, const int dst_pitch[4]);
JINC_API void jinc_batch_free(jinc_batch *b);
JINC_API const char *jinc_batch_last_error(void);

/* ---- Jinc36Resize / Jinc64Resize / Jinc144Resize / Jinc256Resize (ref :986-1040, :1061-1108) ----
 * Builds the argument set the alias forwards through avs_invoke("JincResize", ...): the three
 * positional arguments plus, when defined, src_left/top/width/height, quant_x/y, cplace, threads
 * (ref :1007-1029), plus tap = taps (3, 4, 6 or 8; ref :1037).  Everything else stays undefined. */
JINC_API int jinc_alias_args(int taps, const jinc_args *alias_in, jinc_args *out);

/* Compatibility modes for users who diff against the reference's SIMD output: 1 / 2 / 3 reproduce
 * the summation order of its opt = 1 (SSE4.1: 4 lane-partial sums, multiply + add), opt = 2 (AVX2: 8 partial sums, FMA)
 * and opt = 3 (AVX-512: 16 partial sums, FMA) paths bit for bit -- horizontal-sum tree, cvtps_epi32 + packus saturation
 * (to 65535 / 255, not to the clip's peak) and the lower clamp of float sources included (ref resize_plane_sse41.cpp:41-90,
 * resize_plane_avx2.cpp:45-98, resize_plane_avx512.cpp:45-103).  0 (default) = the opt = 0 result, the parity target.
 * A private switch: the public `opt` argument does not select it.  Slow path (no LDS staging). */
JINC_API int jinc_filter_set_simd_order(jinc_filter *f, int order);

/* ---- A 3x3 colour matrix on a float filter's result planes ----
 * Decoders give Y'CbCr, networks and displays take R'G'B': with a matrix set, every jinc_filter_process_device* call -- the planar
 * call, _strided, _shifted, _packed10, _v210, _shifted_packed10, _v210_packed10 and every _widened* and _narrowed* call -- hands
 * its destination side o = M r + offset where it handed r.  For each output pixel with planar results r0, r1, r2 (what the call
 * would have left in planes 0 .. 2, widened exactly to fp32)
 *     o_i = fl32( fl32( fl32( fl32(m[3i] * r0) + fl32(m[3i+1] * r1) ) + fl32(m[3i+2] * r2) ) + offset[i] )      i = 0, 1, 2
 * -- three multiplies and three adds, each rounded to fp32, in this order, never a fused multiply-add.  `m` is row-major.  An fp32
 * filter stores o_i; a binary16 or bfloat16 filter rounds once more here: o_i goes to nearest even into the filter's sample type (the
 * conversion its kernels store results with) -- on top of the rounding the resampling kernels ended in -- and a destination pass
 * that narrows (the _narrowed* calls) reads that rounded sample.  Non-finite inputs follow IEEE arithmetic; NaN payloads are not
 * specified.
 *   Output i goes to plane i: the caller orders the rows of `m` to suit its plane order (and its columns to suit the planes the
 * filter resamples).  jinc_colour_matrix gives rows in R, G, B order, which is the order of a packed RGB destination whose channels
 * the call's pointers and steps place; AviSynth's planar RGB is G, B, R, so a caller that writes RGBPS planes passes rows 1, 2, 0 of
 * it.  A fourth plane (alpha) is not touched.  Everything behind the matrix is unchanged: a destination pass (merge, narrow with its
 * scale / offset, pack into words or blocks) sees o where it saw r.  It is a pass of its own -- one kernel launch per slice of a
 * call, in place on the dense result planes -- and the resampling kernels, jinc_filter_set_simd_order and the kernel modes are
 * independent of it: the matrix reads whatever the chosen kernel wrote.
 *   m == NULL clears the matrix (offset is not read); offset == NULL means zeros.  Needs no device.  Refused where the filter
 * decides it: an integer filter, a filter with fewer than three planes and a filter whose output planes 0 .. 2 are not of one size
 * (the output must be 4:4:4: RGB, YUV444, or a 4:2:0 / 4:2:2 input through jinc_filter_create_out(..., 0, 0)) are JINC_ERR_UNSUPPORTED; a
 * NaN or an infinity in m or offset is JINC_ERR_INVALID_ARG.
 *   With a matrix set the host-frame entries -- jinc_filter_get_frame, jinc_filter_submit, and so a jinc_batch built on them --
 * return JINC_ERR_UNSUPPORTED and launch nothing: the matrix belongs to the device calls. */
JINC_API int jinc_filter_set_output_matrix(jinc_filter *f, const float m[9], const float offset[3]);

/* The usual matrices between normalised Y' in 0 .. 1, Cb / Cr in -0.5 .. 0.5 (exactly what jinc_code_range produces) and R'G'B' in
 * 0 .. 1, row-major in m.  Needs no device.  With Kr / Kb = 0.299 / 0.114 (JINC_MATRIX_BT601), 0.2126 / 0.0722 (JINC_MATRIX_BT709),
 * 0.2627 / 0.0593 (JINC_MATRIX_BT2020_NCL) and Kg = 1.0 - Kr - Kb:
 *   JINC_YCBCR_TO_RGB (rows R, G, B; columns Y', Cb, Cr)        JINC_RGB_TO_YCBCR (rows Y', Cb, Cr; columns R, G, B)
 *       1    0                          2.0 * (1.0 - Kr)             Kr                         Kg                         Kb
 *       1    -2.0 * Kb * (1.0 - Kb) / Kg   -2.0 * Kr * (1.0 - Kr) / Kg    -Kr / (2.0 * (1.0 - Kb))   -Kg / (2.0 * (1.0 - Kb))   0.5
 *       1    2.0 * (1.0 - Kb)           0                            0.5                        -Kg / (2.0 * (1.0 - Kr))   -Kb / (2.0 * (1.0 - Kr))
 * Every entry is computed in double, in the order written, and rounded to float once.  Any other standard or direction, or a NULL m,
 * is JINC_ERR_INVALID_ARG. */
#define JINC_MATRIX_BT601 0
#define JINC_MATRIX_BT709 1
#define JINC_MATRIX_BT2020_NCL 2
#define JINC_YCBCR_TO_RGB 0
#define JINC_RGB_TO_YCBCR 1
JINC_API int jinc_colour_matrix(int standard, int direction, float m[9]);

/* Plan introspection, kernel-selection knobs for A/B measurements, test hooks and kernel timing live in
 * jincresize_hip_test.h: they are exported by the same library but are not part of the drop-in boundary. */

#ifdef __cplusplus
}
#endif
#endif /* JINCRESIZE_HIP_H */
