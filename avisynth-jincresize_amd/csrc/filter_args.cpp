// filter_args.cpp -- Create_JincResize's argument handling and geometry derivation for the accelerated path
// ("ref:" = /root/reference/src/JincResize.cpp :700-866): same defaults, same checks in the same order, same error strings.
#include "filter_internal.h"
#include <cctype>

namespace jinc {
namespace host {

namespace {
bool is_yuv_subsampled(const jinc_video_info& vi, int sw, int sh) {
    return !vi.is_rgb && vi.num_components >= 3 && vi.sub_w == sw && vi.sub_h == sh;
}

std::string lower(std::string s) {
    for (auto& c : s) c = static_cast<char>(std::tolower(static_cast<unsigned char>(c)));
    return s;
}

}  // namespace

// ---- Create_JincResize argument handling (ref :700-789), then geometry (ref :791-866) ------------
// out_sub_w / out_sub_h (jinc_filter_create_out): the OUTPUT's chroma sub-sampling, -1 / -1 = the input's (the reference's filter).
void configure(jinc_filter& f, const jinc_video_info& vi, const jinc_args& a, int out_sub_w, int out_sub_h) {
    auto has = [&](unsigned bit) { return (a.defined & bit) != 0; };

    if (!vi.is_planar) throw ArgError("JincResize: clip must be in planar format.");

    const int tap = has(JINC_ARG_TAP) ? a.tap : 3;
    if (tap < 1 || tap > 16) throw ArgError("JincResize: tap must be between 1..16.");

    const int quant_x = has(JINC_ARG_QUANT_X) ? a.quant_x : 256;
    if (quant_x < 1 || quant_x > 256) throw ArgError("JincResize: quant_x must be between 1..256.");
    const int quant_y = has(JINC_ARG_QUANT_Y) ? a.quant_y : 256;
    if (quant_y < 1 || quant_y > 256) throw ArgError("JincResize: quant_y must be between 1..256.");

    std::string cplace = (has(JINC_ARG_CPLACE) && a.cplace) ? a.cplace : "";
    if (!cplace.empty()) {
        cplace = lower(cplace);
        if (cplace != "mpeg2" && cplace != "mpeg1" && cplace != "topleft")
            throw ArgError("JincResize: cplace must be MPEG2, MPEG1 or topleft.");
    } else {
        if (a.frame0_chroma_location != -1) {  // the property exists and is an integer (ref :730)
            switch (a.frame0_chroma_location) {
                case 0: cplace = "mpeg2"; break;
                case 1: cplace = "mpeg1"; break;
                case 2: cplace = "topleft"; break;
                default: throw ArgError("JincResize: invalid _ChromaLocation");
            }
        } else {
            cplace = "mpeg2";
        }
    }
    const bool is_420 = is_yuv_subsampled(vi, 1, 1);
    // (the siting describes whichever side is sub-sampled: a 4:2:0 OUTPUT of a YUV clip takes topleft as a 4:2:0 input does)
    const bool out_is_420 = !vi.is_rgb && vi.num_components >= 3 && out_sub_w == 1 && out_sub_h == 1;
    if (cplace == "topleft" && !is_420 && !out_is_420)
        throw ArgError("JincResize: topleft must be used only for 4:2:0 chroma subsampling.");

    const int opt = has(JINC_ARG_OPT) ? a.opt : -1;
    if (opt > 3) throw ArgError("JincResize: opt higher than 3 is not allowed.");
    if (opt == 3 && !a.cpu_has_avx512f) throw ArgError("JincResize: opt=3 requires AVX-512F.");
    if (opt == 2 && !a.cpu_has_avx2) throw ArgError("JincResize: opt=2 requires AVX2.");
    if (opt == 1 && !a.cpu_has_sse41) throw ArgError("JincResize: opt=1 requires SSE4.1.");

    const int threads = has(JINC_ARG_THREADS) ? a.threads : 0;
    if (threads < 0 || threads > 1) throw ArgError("JincResize: threads must be either 0 or 1.");
    f.copy_helpers = threads != 1;  // the reference: 1 = this thread only, 0 = every core (ref :901); here: the copies of pageable planes

    double crop_left = has(JINC_ARG_SRC_LEFT) ? a.src_left : 0.0;
    double crop_width = has(JINC_ARG_SRC_WIDTH) ? a.src_width : static_cast<double>(vi.width);
    if (crop_width <= 0.0) crop_width = vi.width - crop_left + crop_width;
    double crop_top = has(JINC_ARG_SRC_TOP) ? a.src_top : 0.0;
    double crop_height = has(JINC_ARG_SRC_HEIGHT) ? a.src_height : static_cast<double>(vi.height);
    if (crop_height <= 0.0) crop_height = vi.height - crop_top + crop_height;

    double blur = has(JINC_ARG_BLUR) ? a.blur : 0.0;
    if (!blur) blur = 1.0;

    const int target_width = a.target_width;
    const int target_height = a.target_height;

    const double initial_factor = has(JINC_ARG_INITIAL_FACTOR) ? a.initial_factor : 1.50;
    if (initial_factor < 1.0) throw ArgError("JincResize: initial_factor must be eqaul to or greater than 1.0.");

    const int src_width = vi.width;
    const int src_height = vi.height;
    const int initial_capacity = has(JINC_ARG_INITIAL_CAPACITY)
                                     ? a.initial_capacity
                                     : std::max(target_width * target_height, src_width * src_height);
    if (initial_capacity <= 0) throw ArgError("JincResize: initial_capacity must be greater than 0.");

    // ---- the output's chroma sub-sampling (beyond the reference): behind its checks, in front of any work ----
    const bool has_chroma = !vi.is_rgb && vi.num_components >= 3;
    const bool out_given = out_sub_w != -1 || out_sub_h != -1;
    const bool out_is_input = out_sub_w == vi.sub_w && out_sub_h == vi.sub_h;
    if (out_given) {
        if (!has_chroma) throw ArgError("JincResize: an output chroma sub-sampling needs a YUV clip with chroma planes (not RGB, not Y).");
        if (!out_is_input) {
            if (out_sub_w < -1 || out_sub_w > 1 || out_sub_h < -1 || out_sub_h > 1)
                throw ArgError("JincResize: out_sub_w and out_sub_h must be -1, 0 or 1.");
            if (out_sub_w == -1 || out_sub_h == -1) throw ArgError("JincResize: out_sub_w and out_sub_h must both be -1 or both be given.");
            if (out_sub_w == 0 && out_sub_h == 1) throw ArgError("JincResize: 4:4:0 output (out_sub_w 0, out_sub_h 1) is not supported.");
            if (!(vi.sub_w == 0 && vi.sub_h == 0) && !(vi.sub_w == 1 && vi.sub_h == 0) && !(vi.sub_w == 1 && vi.sub_h == 1))
                throw ArgError("JincResize: 4:1:1 and 4:4:0 clips keep their chroma sub-sampling (give -1 or the clip's own values).");
        }
        if (target_width % (1 << out_sub_w))
            throw ArgError("JincResize: target_width must be a multiple of the output's horizontal chroma sub-sampling factor.");
        if (target_height % (1 << out_sub_h))
            throw ArgError("JincResize: target_height must be a multiple of the output's vertical chroma sub-sampling factor.");
    }
    const int in_sub_w = vi.sub_w, in_sub_h = vi.sub_h;
    if (!out_given) out_sub_w = in_sub_w, out_sub_h = in_sub_h;

    // ---- ref :791-866 ----
    f.vi_in = vi;
    f.vi_out = vi;
    f.vi_out.width = target_width;
    f.vi_out.height = target_height;
    f.vi_out.sub_w = out_sub_w;
    f.vi_out.sub_h = out_sub_h;
    f.cplace = cplace;
    f.peak = (vi.bits_per_component <= 16 && !f.half && !f.bf16) ? static_cast<float>((1 << vi.bits_per_component) - 1) : 0.f;  // (half, bfloat16: no clamp)
    f.planecount = vi.num_components;
    const double radius = jinc::jinc_radius(tap);
    jinc::build_lut(f.lut, radius, blur);

    jinc::TableGeometry g;
    g.quant_x = quant_x;
    g.quant_y = quant_y;
    g.src_w = src_width;
    g.src_h = src_height;
    g.dst_w = target_width;
    g.dst_h = target_height;
    g.radius = radius;
    g.crop_left = crop_left;
    g.crop_top = crop_top;
    g.crop_w = crop_width;
    g.crop_h = crop_height;

    // A chroma plan of its own wherever either side's chroma grid is not the luma grid (plane_dims shifts by each side's own values).
    const bool is_444 = !vi.is_rgb && in_sub_w == 0 && in_sub_h == 0 && out_sub_w == 0 && out_sub_h == 0;
    f.subsampled = f.planecount > 1 && !(is_444 || vi.is_rgb);
    f.plans.push_back(jinc::build_plane_plan(f.lut, g));
    if (f.subsampled) {
        const double div_w = 1 << in_sub_w;
        const double div_h = 1 << in_sub_h;
        // Offset of a co-sited axis in luma samples: a co-sited grid of factor d maps its
        // coordinate c to luma d c - (d - 1) / 2, so output grid (d_o) o luma map (r u + crop) o input grid (d_i) leaves
        // 0.5 ((d_i - 1) - r (d_o - 1)).  Equal factors keep the reference's line as it stands, 0.5 (1 - r) -- which is the same
        // value for d = 2 and the reference's own for 4:1:1 (d = 4, ref :838-841).
        auto co_sited = [](double d_i, double d_o, double r) {
            return d_i == d_o ? 0.5 * (1.0 - r) : 0.5 * ((d_i - 1.0) - r * (d_o - 1.0));
        };
        const double crop_left_uv =
            (cplace == "mpeg2" || cplace == "topleft")
                ? (co_sited(div_w, 1 << out_sub_w, static_cast<double>(src_width) / target_width) + crop_left) / div_w
                : crop_left / div_w;
        const double crop_top_uv =
            (cplace == "topleft") ? (co_sited(div_h, 1 << out_sub_h, static_cast<double>(src_height) / target_height) + crop_top) / div_h
                                  : crop_top / div_h;
        jinc::TableGeometry gc = g;
        gc.src_w = src_width >> in_sub_w;
        gc.src_h = src_height >> in_sub_h;
        gc.dst_w = target_width >> out_sub_w;
        gc.dst_h = target_height >> out_sub_h;
        gc.crop_left = crop_left_uv;
        gc.crop_top = crop_top_uv;
        gc.crop_w = crop_width / div_w;
        gc.crop_h = crop_height / div_h;
        f.plans.push_back(jinc::build_plane_plan(f.lut, gc));
    }

    // ref :617-625.  The reference compares `d->cplace`, a member that nothing ever assigns (`new JincResize()` :676
    // leaves it empty; the string the arguments and frame 0 decide is the LOCAL `cplace` of :715, which drives the
    // chroma geometry above and nothing else), so its GetFrame always takes the `else` of :623-624 and writes 2.
    // chroma_location is what the reference binary writes; chroma_location_by_siting is what its source means to
    // write, kept behind jinc_filter_set_chroma_location_mode.
    // (the property describes the frames this filter WRITES: it follows vi_out)
    if (is_yuv_subsampled(f.vi_out, 1, 1) || is_yuv_subsampled(f.vi_out, 1, 0) || is_yuv_subsampled(f.vi_out, 2, 0)) {
        f.chroma_location = 2;
        f.chroma_location_by_siting = cplace == "mpeg2" ? 0 : (cplace == "mpeg1" ? 1 : 2);
    } else {
        f.chroma_location = -1;
        f.chroma_location_by_siting = -1;
    }
}

}  // namespace host
}  // namespace jinc
