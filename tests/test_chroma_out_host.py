"""jinc_filter_create_out without a device: the output's chroma sub-sampling as an argument (4:2:0 in, 4:4:4 out and the like).
What is held here is the DEFINITION of include/jincresize_hip.h: plane 0 is a Y-only filter with the same arguments, planes 1 and 2
are a Y-only filter of the input's chroma size whose target and crop follow, per axis, from
    d_i = 1 << in_sub,  d_o = 1 << out_sub,  r = clip size / target size,
    src_left = (k + crop) / d_i with k = 0.5 * ((d_i - 1) - r * (d_o - 1)) on a co-sited axis, else crop / d_i,
    src_width = crop_size / d_i.
The twin's arguments are recomputed HERE in Python doubles and the plans are compared through the plan hooks of test_plan_host.py,
byte for byte.  -1 / -1 and the input's own values must be jinc_filter_create_ex."""
import numpy as np
import pytest

from conftest import oracle_kwargs

INVALID_ARG = -1
SUBS = {"444": (0, 0), "422": (1, 0), "420": (1, 1)}
GEOM = (64, 48, 128, 96)   # interior, border rows, border columns and corners on every plane of every pair
CROP = dict(src_left=1.3, src_top=0.7, src_width=60.5, src_height=45.25)   # fractional origin, a width smaller than the clip


def twin_kwargs(sw, sh, tw, th, in_sub, out_sub, kw):
    """(format-independent) clip size, target and script arguments of the Y-only twin of the chroma planes."""
    cplace = kw.get("cplace", "mpeg2").lower()
    crop = [kw.get("src_left", 0.0), kw.get("src_top", 0.0)]
    size = [kw.get("src_width", float(sw)), kw.get("src_height", float(sh))]
    src, tgt = (sw, sh), (tw, th)
    co = (cplace in ("mpeg2", "topleft"), cplace == "topleft")
    uv, uv_size = [], []
    for a in range(2):
        if size[a] <= 0.0:
            size[a] = src[a] - crop[a] + size[a]
        d_i, d_o, r = float(1 << in_sub[a]), float(1 << out_sub[a]), float(src[a]) / tgt[a]
        k = 0.5 * ((d_i - 1.0) - r * (d_o - 1.0)) if co[a] else 0.0
        uv.append((k + crop[a]) / d_i)
        uv_size.append(size[a] / d_i)
    assert uv_size[0] > 0 and uv_size[1] > 0
    out = {k: v for k, v in kw.items() if k in ("tap", "blur", "quant_x", "quant_y")}
    out.update(src_left=uv[0], src_top=uv[1], src_width=uv_size[0], src_height=uv_size[1])
    return (sw >> in_sub[0], sh >> in_sub[1], tw >> out_sub[0], th >> out_sub[1]), out


def luma_kwargs(kw):
    return {k: v for k, v in kw.items() if k != "cplace"}


def plan_of(f, table):
    info = f.plan_info(table)
    fields = tuple(getattr(info, n) for n, _ in info._fields_)
    sx, sy, ids = f.plan_dump(table)
    return fields, sx.tobytes(), sy.tobytes(), ids.tobytes(), f.plan_sets(table).tobytes()


def assert_same_plans(a, b, what):
    assert a.num_tables == b.num_tables, what
    assert a.lut().tobytes() == b.lut().tobytes(), what
    for t in range(a.num_tables):
        assert plan_of(a, t) == plan_of(b, t), f"{what}: table {t}"


def chroma_table(f):
    return 1 if f.num_tables == 2 else 0


# ---- the surface ------------------------------------------------------------------------------------------------------------------

def test_the_entries_are_exported_declared_and_mirrored(pkg):
    import inspect
    header = " ".join(open(pkg.HEADER_PATH).read().split())
    for name in ("jinc_filter_process_device_shifted_packed10", "jinc_filter_process_device_v210_packed10"):
        assert hasattr(pkg.Filter, name[len("jinc_filter_"):]), name
    for name in ("jinc_filter_create_out", "jinc_batch_create_out", "jinc_filter_process_device_shifted_packed10",
                 "jinc_filter_process_device_v210_packed10"):
        assert name in pkg.EXPORTS and hasattr(pkg.lib(), name), name
        assert name + "(" in header, name
    assert "int jinc_filter_create_out(const jinc_video_info *vi, const jinc_args *args, int sample_type, int out_sub_w, int out_sub_h, " \
           "int device, jinc_filter **out, char *err, size_t err_len);" in header
    assert "int jinc_batch_create_out(const jinc_video_info *vi, const jinc_args *args, int sample_type, int out_sub_w, int out_sub_h, " \
           "int ndevices, int streams_per_device, int register_host_buffers, jinc_batch **out, char *err, size_t err_len);" in header
    assert "out_sub" in inspect.signature(pkg.Filter.__init__).parameters
    assert "out_sub" in inspect.signature(pkg.Batch.__init__).parameters


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

REFUSALS = [
    ("rgb", "RGBP8", (0, 0), GEOM, {}, "JincResize: an output chroma sub-sampling needs a YUV clip with chroma planes (not RGB, not Y)."),
    ("y_only", "Y8", (1, 1), GEOM, {}, "JincResize: an output chroma sub-sampling needs a YUV clip with chroma planes (not RGB, not Y)."),
    ("y_only_444", "Y16", (0, 0), GEOM, {}, "JincResize: an output chroma sub-sampling needs a YUV clip with chroma planes (not RGB, not Y)."),
    ("value_2", "YUV420P8", (2, 0), GEOM, {}, "JincResize: out_sub_w and out_sub_h must be -1, 0 or 1."),
    ("value_minus_2", "YUV420P8", (0, -2), GEOM, {}, "JincResize: out_sub_w and out_sub_h must be -1, 0 or 1."),
    ("one_minus_1_w", "YUV420P8", (-1, 0), GEOM, {}, "JincResize: out_sub_w and out_sub_h must both be -1 or both be given."),
    ("one_minus_1_h", "YUV444PS", (1, -1), GEOM, {}, "JincResize: out_sub_w and out_sub_h must both be -1 or both be given."),
    ("out_440", "YUV420P8", (0, 1), GEOM, {}, "JincResize: 4:4:0 output (out_sub_w 0, out_sub_h 1) is not supported."),
    ("out_440_from_444", "YUV444P16", (0, 1), GEOM, {}, "JincResize: 4:4:0 output (out_sub_w 0, out_sub_h 1) is not supported."),
    ("in_411", "YUV411P8", (0, 0), GEOM, {}, "JincResize: 4:1:1 and 4:4:0 clips keep their chroma sub-sampling (give -1 or the clip's own values)."),
    ("in_411_to_420", "YUV411P8", (1, 1), GEOM, {}, "JincResize: 4:1:1 and 4:4:0 clips keep their chroma sub-sampling (give -1 or the clip's own values)."),
    ("in_440", ("YUV440P8", 8, 0, 1), (0, 0), GEOM, {}, "JincResize: 4:1:1 and 4:4:0 clips keep their chroma sub-sampling (give -1 or the clip's own values)."),
    ("odd_width", "YUV444P8", (1, 1), (64, 48, 127, 96), {}, "JincResize: target_width must be a multiple of the output's horizontal chroma sub-sampling factor."),
    ("odd_width_422", "YUV420P8", (1, 0), (64, 48, 127, 96), {}, "JincResize: target_width must be a multiple of the output's horizontal chroma sub-sampling factor."),
    ("odd_height", "YUV444P8", (1, 1), (64, 48, 128, 95), {}, "JincResize: target_height must be a multiple of the output's vertical chroma sub-sampling factor."),
    ("odd_height_same", "YUV420P8", (1, 1), (64, 48, 128, 95), {}, "JincResize: target_height must be a multiple of the output's vertical chroma sub-sampling factor."),
    # topleft keeps the reference's refusal and text where neither side is 4:2:0
    ("topleft_422_to_444", "YUV422P8", (0, 0), GEOM, dict(cplace="topleft"), "JincResize: topleft must be used only for 4:2:0 chroma subsampling."),
    ("topleft_444_to_422", "YUV444P8", (1, 0), GEOM, dict(cplace="topleft"), "JincResize: topleft must be used only for 4:2:0 chroma subsampling."),
    ("topleft_rgb", "RGBP8", (1, 1), GEOM, dict(cplace="topleft"), "JincResize: topleft must be used only for 4:2:0 chroma subsampling."),
    # the reference's own checks come first, with their texts
    ("tap_first", "YUV420P8", (7, 7), GEOM, dict(tap=17), "JincResize: tap must be between 1..16."),
    ("capacity_first", "RGBP8", (0, 0), GEOM, dict(initial_capacity=0), "JincResize: initial_capacity must be greater than 0."),
]


def fmt_of(pkg, spec):
    if isinstance(spec, str):
        return pkg.FORMATS[spec]
    name, bits, sw, sh = spec
    return pkg.Format(name, bits, 3, sw, sh)


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals_and_their_messages(pkg, case):
    _, spec, out_sub, (sw, sh, tw, th), kw, says = case
    with pytest.raises(pkg.JincError) as e:
        pkg.Filter(fmt_of(pkg, spec), sw, sh, tw, th, device=-1, out_sub=out_sub, **kw)
    assert e.value.code == INVALID_ARG and str(e.value) == says


def test_a_clip_of_411_or_440_takes_its_own_values(pkg):
    """"Giving the input's own values yields the same filter" holds for the two shapes that convert to nothing else as well."""
    for spec in ("YUV411P8", ("YUV440P8", 8, 0, 1)):
        fmt = fmt_of(pkg, spec)
        a = pkg.Filter(fmt, *GEOM, device=-1)
        b = pkg.Filter(fmt, *GEOM, device=-1, out_sub=(fmt.sub_w, fmt.sub_h))
        assert_same_plans(a, b, fmt.name)
        assert b.out_fmt == fmt and a.chroma_location == b.chroma_location


def test_the_calls_into_packed_words_check_the_filter_per_side(pkg):
    """P010 / v210 in, Y410 out: the filter is judged before anything else, so a host-only instance shows the texts."""
    p, i, z, y410 = [64, 64, 64], [256, 256, 256], [0, 0, 0], [10, 0, 20]

    def refused(call, says):
        with pytest.raises(pkg.JincError) as e:
            call()
        assert e.value.code == INVALID_ARG and str(e.value) == says

    f = pkg.Filter(pkg.FORMATS["YUV420P10"], *GEOM, device=-1)   # output 4:2:0
    refused(lambda: f.process_device_shifted_packed10(p, i, [1, 2, 2], [6, 6, 6], z, 64, 512, y410, 0, 0, 1),
            "JincResize: packed 10:10:10:2 words on the destination side need a filter whose output is not sub-sampled (4:4:4); "
            "this filter's output has sub_w 1 and sub_h 1.")
    f = pkg.Filter(pkg.FORMATS["YUV420P10"], *GEOM, device=-1, out_sub=(0, 0))
    refused(lambda: f.process_device_v210_packed10(64, 512, 0, 64, 512, y410, 0, 0, 1),
            "JincResize: v210 blocks on the source side need a filter whose input is 4:2:2 (sub_w 1, sub_h 0); "
            "this filter's input has sub_w 1 and sub_h 1.")
    refused(lambda: f.process_device_shifted_packed10(p, i, [1, 2, 5], None, z, 64, 512, y410, 0, 0, 1), "JincResize: sample step must be in 1..4.")
    refused(lambda: f.process_device_shifted_packed10(p, i, None, [7, 0, 0], z, 64, 512, y410, 0, 0, 1),
            "JincResize: sample shift is larger than the padding of the sample's container (6 bits).")
    refused(lambda: f.process_device_shifted_packed10(p, i, None, None, z, 64, 512, [0, 5, 20], 0, 0, 1),
            "JincResize: two fields of a packed 10:10:10:2 word overlap.")
    with pytest.raises(pkg.JincError) as e:   # everything in order: what is left is the missing device
        f.process_device_shifted_packed10(p, i, [1, 2, 2], [6, 6, 6], z, 64, 512, y410, 0, 0, 1)
    assert e.value.code == -2
    f = pkg.Filter(pkg.FORMATS["YUV420P8"], *GEOM, device=-1, out_sub=(0, 0))
    refused(lambda: f.process_device_shifted_packed10(p, i, None, None, z, 64, 512, y410, 0, 0, 1),
            "JincResize: a packed 10:10:10:2 destination needs a filter with three 10-bit components in 16-bit samples.")


# ---- -1 / -1 and the input's own values: jinc_filter_create_ex ---------------------------------------------------------------------

@pytest.mark.parametrize("cplace", ["mpeg2", "mpeg1", "topleft"])
@pytest.mark.parametrize("name", ["YUV420P8", "YUV422P8", "YUV420PS", "YUVA420P16"])
@pytest.mark.parametrize("kw", [{}, CROP], ids=["whole", "crop"])
def test_minus_one_and_the_inputs_own_values_are_create_ex(pkg, name, cplace, kw):
    fmt = pkg.FORMATS[name]
    if cplace == "topleft" and (fmt.sub_w, fmt.sub_h) != (1, 1):
        for out_sub in ((-1, -1), (fmt.sub_w, fmt.sub_h)):
            with pytest.raises(pkg.JincError) as e:
                pkg.Filter(fmt, *GEOM, device=-1, out_sub=out_sub, cplace=cplace, **kw)
            assert str(e.value) == "JincResize: topleft must be used only for 4:2:0 chroma subsampling."
        return
    ex = pkg.Filter(fmt, *GEOM, device=-1, cplace=cplace, **kw)
    for out_sub in ((-1, -1), (fmt.sub_w, fmt.sub_h)):
        out = pkg.Filter(fmt, *GEOM, device=-1, out_sub=out_sub, cplace=cplace, **kw)
        assert_same_plans(ex, out, f"{name} {cplace} out_sub {out_sub}")
        assert out.chroma_location == ex.chroma_location == 2
        assert out.out_dims() == ex.out_dims() and out.out_fmt == fmt
        out.close()
    ex.close()


# ---- the nine pairs: the chroma plan is the Y-only twin's ---------------------------------------------------------------------------

PAIRS = [(i, o) for i in SUBS for o in SUBS]
GEOMETRIES = [
    ("2x", GEOM, {}),
    ("2x_tap4", GEOM, dict(tap=4)),
    ("crop", GEOM, dict(CROP, blur=0.95, quant_x=64, quant_y=37)),
    ("relative_crop", (64, 48, 128, 96), dict(src_left=2.0, src_top=-1.5, src_width=-3.0, src_height=-2.25)),
    ("1x", (64, 48, 64, 48), {}),
    ("1.37x", (160, 96, 220, 132), {}),
    ("down", (128, 96, 64, 48), {}),
]


# (topleft where it is allowed: a 4:2:0 side; its refusal elsewhere is in REFUSALS)
PLAN_CASES = [(p, g, c) for p in PAIRS for g in GEOMETRIES for c in ("mpeg2", "mpeg1", "topleft") if c != "topleft" or "420" in p]


@pytest.mark.parametrize("case", PLAN_CASES, ids=[f"{p[0]}to{p[1]}_{g[0]}_{c}" for p, g, c in PLAN_CASES])
def test_every_plane_has_the_plan_of_its_y_only_twin(pkg, case):
    (i, o), (_, (sw, sh, tw, th), kw), cplace = case
    kw = dict(kw, cplace=cplace)
    f = pkg.Filter(pkg.FORMATS[f"YUV{i}P8"], sw, sh, tw, th, device=-1, out_sub=SUBS[o], **kw)
    what = f"{i} -> {o} {sw}x{sh}->{tw}x{th} {kw}"
    assert f.num_tables == (1 if i == o == "444" else 2), what
    luma = pkg.Filter(pkg.FORMATS["Y8"], sw, sh, tw, th, device=-1, **luma_kwargs(kw))
    assert plan_of(f, 0) == plan_of(luma, 0), what + ": luma"
    (csw, csh, ctw, cth), ckw = twin_kwargs(sw, sh, tw, th, SUBS[i], SUBS[o], kw)
    twin = pkg.Filter(pkg.FORMATS["Y8"], csw, csh, ctw, cth, device=-1, **ckw)
    assert plan_of(f, chroma_table(f)) == plan_of(twin, 0), what + f": chroma against Y8 {csw}x{csh}->{ctw}x{cth} {ckw}"
    assert f.lut().tobytes() == twin.lut().tobytes()
    for g in (f, luma, twin):
        g.close()


def test_the_reference_geometry_is_the_formula_at_equal_factors(pkg, O):
    """4:2:0 -> 4:2:0 and 4:2:2 -> 4:2:2 through the formula's twin equal the ORACLE's chroma table of the reference derivation.
    (A check of this file's twin_kwargs against the reference's geometry, not of the product: it needs no new code to pass.)"""
    for name, sub in (("YUV420P8", (1, 1)), ("YUV422P8", (1, 0))):
        for cplace in ("mpeg2", "mpeg1") + (("topleft",) if sub == (1, 1) else ()):
            kw = dict(CROP, cplace=cplace)
            (csw, csh, ctw, cth), ckw = twin_kwargs(*GEOM, sub, sub, kw)
            of = O.OracleFilter(O.FORMATS[name], *GEOM, **oracle_kwargs(kw))
            ot = O.OracleFilter(O.FORMATS["Y8"], csw, csh, ctw, cth, **oracle_kwargs(ckw))
            assert np.array_equal(of.tables[1].meta(), ot.tables[0].meta()), (name, cplace)
            assert of.tables[1].factor().tobytes() == ot.tables[0].factor().tobytes(), (name, cplace)


# ---- output_info and chroma_location ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", PAIRS, ids=[f"{i}to{o}" for i, o in PAIRS])
def test_output_info_and_chroma_location_follow_the_output(pkg, pair):
    import ctypes as C
    i, o = pair
    for name in (f"YUV{i}P10", f"YUVA{i}PS", f"YUV{i}PH", f"YUV{i}PBF"):
        fmt = pkg.FORMATS[name]
        for cplace, by_siting in (("mpeg2", 0), ("mpeg1", 1)) + ((("topleft", 2),) if "420" in pair else ()):
            f = pkg.Filter(fmt, *GEOM, device=-1, out_sub=SUBS[o], cplace=cplace)
            vi = pkg.VideoInfo()
            assert pkg.lib().jinc_filter_output_info(f._h, C.byref(vi)) == 0
            assert (vi.width, vi.height, vi.sub_w, vi.sub_h) == (128, 96) + SUBS[o]
            assert (vi.bits_per_component, vi.component_size, vi.num_components, vi.is_rgb) == (fmt.bits, fmt.sample_bytes, fmt.planes, 0)
            chroma = (128 >> SUBS[o][0], 96 >> SUBS[o][1])
            assert f.out_dims() == [(128, 96), chroma, chroma] + ([(128, 96)] if fmt.planes == 4 else [])
            assert (f.out_fmt.sub_w, f.out_fmt.sub_h) == SUBS[o] and f.out_fmt.dtype == fmt.dtype and f.out_fmt.sample_type == fmt.sample_type
            assert f.chroma_location == (-1 if o == "444" else 2)
            f.set_chroma_location_mode(1)
            assert f.chroma_location == (-1 if o == "444" else by_siting)
            f.close()


def test_frame0_chroma_location_selects_the_siting_of_the_output(pkg):
    """No cplace: _ChromaLocation of frame 0 decides, for a 4:4:4 clip that leaves as 4:2:0 as for a 4:2:0 clip."""
    a = pkg.Filter(pkg.FORMATS["YUV444P8"], *GEOM, device=-1, out_sub=(1, 1), frame0_chroma_location=2)
    b = pkg.Filter(pkg.FORMATS["YUV444P8"], *GEOM, device=-1, out_sub=(1, 1), cplace="topleft")
    assert_same_plans(a, b, "frame 0 property")
    a.set_chroma_location_mode(1)
    assert a.chroma_location == 2


# ---- a frame through the host plan -------------------------------------------------------------------------------------------------

def apply_plan(f, table, src, peak):
    """The reference's (ly, lx) chain on the product's HOST plan, in numpy float32 (un-fused), for integer planes."""
    sx, sy, ids = f.plan_dump(table)
    sets = f.plan_sets(table)
    fs = sets.shape[1]
    coef = sets[ids]
    acc = np.zeros(ids.shape, np.float32)
    for ly in range(fs):
        for lx in range(fs):
            acc = acc + src[sy[:, None] + ly, sx[None, :] + lx].astype(np.float32) * coef[:, :, ly, lx]
    return np.rint(np.clip(acc, np.float32(0), np.float32(peak))).astype(src.dtype)


@pytest.mark.parametrize("cplace", ["mpeg2", "mpeg1", "topleft"])
def test_a_420_frame_through_the_host_plan_equals_the_three_single_plane_oracles(pkg, O, cplace):
    sw, sh, tw, th = GEOM
    kw = dict(cplace=cplace)
    f = pkg.Filter(pkg.FORMATS["YUV420P8"], sw, sh, tw, th, device=-1, out_sub=(0, 0), **kw)
    src = O.lcg_frame(O.FORMATS["YUV420P8"], sw, sh, seed=77)
    (csw, csh, ctw, cth), ckw = twin_kwargs(sw, sh, tw, th, (1, 1), (0, 0), kw)
    assert (csw, csh, ctw, cth) == (32, 24, 128, 96)
    want = [O.OracleFilter(O.FORMATS["Y8"], sw, sh, tw, th).get_frame([src[0]])[0]]
    chroma = O.OracleFilter(O.FORMATS["Y8"], csw, csh, ctw, cth, **oracle_kwargs(ckw))
    want += [chroma.get_frame([src[1]])[0], chroma.get_frame([src[2]])[0]]
    for i in range(3):
        got = apply_plan(f, 0 if i == 0 else 1, src[i], 255)
        assert got.shape == (th, tw)
        assert np.array_equal(got, want[i][:th, :tw]), f"plane {i} {cplace}"
    assert len({w[:th, :tw].tobytes() for w in want}) == 3
    f.close()
