"""jinc_filter_process_device_narrowed on the device: the results of fp32, binary16 and bfloat16 filters into INTEGER frames (NV12,
P010, Y210, BGRA8, planar 16-bit).  The expected result of every case comes from a run of jinc_filter_process_device on the same
filter and the same planes, read back, widened exactly to float32 and narrowed by numpy under the definition
    value = rint(clip(r, 0, peak)) << shift        (round half to even; a NaN becomes 0)
-- never from the narrowed call's own output -- and is compared bit for bit.  Every destination lies inside a larger buffer of
pseudo-random bytes whose other bytes must keep their value (test_strided.py's Side, whose helpers and layouts this file uses), the
source must come back unchanged and jinc_debug_last_strided must report the launches the call is documented to make.
The common shape is 262 x 38 -> 524 x 76 at tap 3, 2 frames (test_widened.py argues for it): a luma row of 524 is whole lanes'
pixels and a tail for bytes and for words, the 4:2:0 chroma row of 131 pixels is odd, and 76 / 38 rows are several row blocks."""
import numpy as np
import pytest

from test_narrowed_host import definition
from test_shifted import Y210, SharedRowSide
from test_strided import Side, packed, planar, run_planar, semi_planar
from test_widened import assert_bits_equal, assert_source_unchanged, raw_of
from test_widened import call as widened_call

pytestmark = pytest.mark.gpu

GEOM = (262, 38, 524, 76)
KW = dict(tap=3)
N = 2


def side_for(layout):
    return SharedRowSide if layout == Y210 else Side


def to_type(fmt, v):
    """float32 values as samples of the filter's type (bfloat16: the upper halves of the fp32 patterns, as uint16)."""
    v = np.ascontiguousarray(v, np.float32)
    if fmt.bfloat16:
        return (v.view(np.uint32) >> 16).astype(np.uint16)
    return v.astype(fmt.dtype)


def widened(fmt, p):
    """A plane of the filter's type widened exactly to float32."""
    if fmt.bfloat16:
        return (np.ascontiguousarray(p).astype(np.uint32) << 16).view(np.float32)
    return np.asarray(p).astype(np.float32)


def sources(fmt, sw, sh, n, peak, seed):
    """n frames in code-value units, from 0.15 peak below 0 to 0.15 peak above the peak: results on both sides of both bounds."""
    rng = np.random.default_rng(seed)
    return [[to_type(fmt, rng.uniform(-0.15 * peak, 1.15 * peak, (h, w))) for (w, h) in fmt.plane_dims(sw, sh)] for _ in range(n)]


def expected(fmt, planar_frames, bits, shifts, dtype):
    peak = (1 << bits) - 1
    return [[(definition(widened(fmt, p), peak) << s).astype(dtype) for p, s in zip(planes, shifts)] for planes in planar_frames]


def narrowed_call(f, src, dst, shifts, bits, n, stream, steps=True):
    f.process_device_narrowed(src.ptrs(), src.pitches(), src.steps() if steps else None, src.strides(), dst.ptrs(), dst.pitches(),
                              dst.steps() if steps else None, shifts, bits, dst.strides(), n, stream=stream.cuda_stream)


def make_sides(torch, f, frames, src_layout, dst_layout, bits, n, dst_align=16, seeds=(11, 12)):
    src = Side(torch, f.fmt.plane_dims(f.src_w, f.src_h), f.fmt.dtype, src_layout, n, seed=seeds[0]).fill(frames).upload()
    dst = side_for(dst_layout)(torch, f.out_dims(), np.uint8 if bits == 8 else np.uint16, dst_layout, n, dst_align, seed=seeds[1]).upload()
    return src, dst


def assert_equal(got, want, dims, what):
    for k in range(len(want)):
        for i, (w, h) in enumerate(dims):
            a, b = got[k][i][:h, :w], want[k][i][:h, :w]
            assert a.dtype == b.dtype, (a.dtype, b.dtype)
            bad = np.argwhere(a != b)
            assert len(bad) == 0, f"{what}: frame {k} plane {i} differs at {len(bad)} samples; first (x={bad[0][1]}, y={bad[0][0]}): " \
                                  f"got {a[bad[0][0], bad[0][1]]}, want {b[bad[0][0], bad[0][1]]}"


_PLANAR = {}


def planar_reference(torch, f, key, frames, n):
    """jinc_filter_process_device on dense planes of the same frames: once per case, never changed."""
    if key not in _PLANAR:
        _PLANAR[key] = run_planar(torch, f, frames, n)
    return _PLANAR[key]


def check_call(torch, pkg, name, bits, shifts, dst_layout, expect_report, n=N, geom=GEOM, src_layout=None, frames=None, seed=5,
               null_steps=False, dst_align=16, key=None):
    """One narrowed call against the planar call on the same filter and planes, narrowed by numpy; returns (got, planar result)."""
    sw, sh, tw, th = geom
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    planes = f.fmt.planes
    if frames is None:
        frames = sources(f.fmt, sw, sh, n, (1 << bits) - 1, seed)
        key = key or (name, geom, bits, n, seed)
    what = f"{name} {sw}x{sh}->{tw}x{th} {n} frame(s) -> {bits}-bit {dst_layout} shifts {shifts} align {dst_align}"
    src, dst = make_sides(torch, f, frames, src_layout or planar(planes), dst_layout, bits, n, dst_align)
    s = torch.cuda.current_stream()
    narrowed_call(f, src, dst, shifts, bits, n, s, steps=not null_steps)
    s.synchronize()
    report = f.last_strided()
    print(f"{what}: last_strided {report}, last_call {pkg.last_call()}")
    got = dst.frames_and_guards(what)
    assert_source_unchanged(src, what)
    assert report[:3] == expect_report, report
    want_planar = planar_reference(torch, f, key, frames, n) if key else run_planar(torch, f, frames, n)
    want = expected(f.fmt, want_planar, bits, shifts or [0] * planes, got[0][0].dtype)
    assert_equal(got, want, f.out_dims(), what + " against the planar call narrowed by numpy")
    for k in range(n):   # padding bits are zeros: the stored sample is value << shift as the whole word
        for p, sft in zip(got[k], shifts or [0] * planes):
            assert int(np.count_nonzero(p & p.dtype.type((1 << sft) - 1))) == 0, f"{what}: non-zero bits below the sample"
            assert int(p.max()) <= ((1 << bits) - 1) << sft
    f.close()
    return got, want_planar


BGRA = packed("BGRA", 4, 3)

# (id, filter, dst_bits, shifts, destination layout, source layout or None = planar, (split, narrow, slices))
CASES = [
    ("nv12_f32", "YUV420PS", 8, None, semi_planar(), None, (0, 2, 1)),
    ("nv12_f16", "YUV420PH", 8, None, semi_planar(), None, (0, 2, 1)),
    ("nv12_bf16", "YUV420PBF", 8, None, semi_planar(), None, (0, 2, 1)),
    ("p010_f32", "YUV420PS", 10, [6] * 3, semi_planar(), None, (0, 2, 1)),
    ("p010_f16", "YUV420PH", 10, [6] * 3, semi_planar(), None, (0, 2, 1)),
    ("y210_f32", "YUV422PS", 10, [6] * 3, Y210, None, (0, 2, 1)),
    ("bgra8_f32", "RGBPS", 8, None, BGRA, None, (0, 1, 1)),                       # three components: every X byte is a guard byte
    ("rgb_f32_to_bgra8", "RGBPS", 8, None, BGRA, packed("RGB", 3, 3), (1, 1, 1)),  # interleaved float RGB in: split and narrow both counted
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_equals_the_planar_call_narrowed_by_numpy(gpu_pkg, case):
    torch = pytest.importorskip("torch")
    _, name, bits, shifts, dst_layout, src_layout, report = case
    got, want_planar = check_call(torch, gpu_pkg, name, bits, shifts, dst_layout, report, src_layout=src_layout)
    fmt, peak = gpu_pkg.FORMATS[name], (1 << bits) - 1
    below = sum(int((widened(fmt, p) < 0).sum()) for planes in want_planar for p in planes)
    above = sum(int((widened(fmt, p) > peak).sum()) for planes in want_planar for p in planes)
    print(f"{below} results below 0, {above} above the peak")
    assert below > 0 and above > 0   # (the clamp has work on both sides)


def test_planar_16_bit_with_null_steps_and_shifts(gpu_pkg):
    """YUV444PS -> planar 16-bit words, step and shift arrays NULL on both sides: one launch for the three planes."""
    torch = pytest.importorskip("torch")
    check_call(torch, gpu_pkg, "YUV444PS", 16, None, planar(3), (0, 1, 1), null_steps=True)


# ---- the integer twin -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits,int_name", [(8, "YUV420P8"), (10, "YUV420P10"), (16, "YUV420P16")])
def test_fp32_planes_holding_integers_equal_the_integer_filter(gpu_pkg, bits, int_name):
    """The integer filters convert every source sample to float before the multiply and end in lrintf(clamp(sum, 0, peak)): an fp32
    filter on planes holding the same integers, narrowed to the same depth, IS that filter -- bit for bit, no tolerance."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = GEOM
    fmt_i = gpu_pkg.FORMATS[int_name]
    rng = np.random.default_rng(300 + bits)
    ints = [[rng.integers(0, 1 << bits, (h, w)).astype(fmt_i.dtype) for (w, h) in fmt_i.plane_dims(sw, sh)] for _ in range(N)]
    floats = [[p.astype(np.float32) for p in planes] for planes in ints]
    got, _ = check_call(torch, gpu_pkg, "YUV420PS", bits, None, planar(3), (0, 1, 1), frames=floats)
    f = gpu_pkg.Filter(fmt_i, sw, sh, tw, th, device=0, **KW)
    want = run_planar(torch, f, ints, N)
    assert_equal(got, want, f.out_dims(), f"fp32 narrowed to {bits} bits against {int_name}")
    f.close()


# ---- specials -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,bits,shifts", [("YUV420PS", 8, None), ("YUV420PS", 10, [6] * 3), ("YUV420PH", 8, None), ("YUV420PBF", 8, None)],
                         ids=["f32_nv12", "f32_p010", "f16_nv12", "bf16_nv12"])
def test_values_outside_the_range_and_non_finite_samples(gpu_pkg, name, bits, shifts):
    """Frame 0 finite with results below 0 and above the peak; frame 1 with a +inf, a -inf and a NaN sample in every source plane, so
    the planar result holds infinities of both signs and NaNs (inf - inf under the negative lobes): a NaN becomes 0, -inf 0, +inf peak."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = GEOM
    fmt, peak = gpu_pkg.FORMATS[name], (1 << bits) - 1
    frames = [[widened(fmt, p).copy() for p in planes] for planes in sources(fmt, sw, sh, N, peak, seed=17)]
    for p in frames[1]:
        h, w = p.shape
        p[h // 4, w // 4], p[h // 2, w // 2], p[3 * h // 4, 3 * w // 4] = np.inf, -np.inf, np.nan
    frames = [[to_type(fmt, p) for p in planes] for planes in frames]
    got, want_planar = check_call(torch, gpu_pkg, name, bits, shifts, semi_planar(), (0, 2, 1), frames=frames)
    r0 = np.concatenate([widened(fmt, p).ravel() for p in want_planar[0]])
    r1 = np.concatenate([widened(fmt, p).ravel() for p in want_planar[1]])
    counts = dict(below=int((r0 < 0).sum()), above=int((r0 > peak).sum()), nan=int(np.isnan(r1).sum()), pinf=int(np.isposinf(r1).sum()),
                  ninf=int(np.isneginf(r1).sum()))
    print(counts)
    assert np.isfinite(r0).all() and counts["below"] > 0 and counts["above"] > 0
    assert counts["nan"] > 0 and counts["pinf"] > 0 and counts["ninf"] > 0
    for i, p in enumerate(want_planar[1]):   # spelled out once more, beside the definition: where the planar result is NaN, the sample is 0
        w, h = f_dims = gpu_pkg.FORMATS[name].plane_dims(tw, th)[i]
        r, g = widened(fmt, p)[:h, :w], got[1][i][:h, :w] >> (shifts[i] if shifts else 0)
        assert (g[np.isnan(r)] == 0).all() and (g[np.isneginf(r)] == 0).all() and (g[np.isposinf(r)] == peak).all(), f_dims


# ---- alignment classes ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("align", [16, 4, 1])
@pytest.mark.parametrize("name,bits,shifts", [("YUV420PS", 8, None), ("YUV420PS", 10, [6] * 3), ("YUV420PH", 8, None), ("YUV420PBF", 10, [6] * 3)],
                         ids=["f32_nv12", "f32_p010", "f16_nv12", "bf16_p010"])
def test_alignment_classes(gpu_pkg, name, bits, shifts, align):
    """Destination base, pitch and frame stride multiples of 16 (16-byte stores), of 4 only (dwords), of the sample size only
    (sample by sample), for the N = 1 form (luma) and the N = 2 form (chroma) of one call."""
    torch = pytest.importorskip("torch")
    check_call(torch, gpu_pkg, name, bits, shifts, semi_planar(), (0, 2, 1), dst_align=align)


@pytest.mark.parametrize("align", [16, 4, 1])
def test_packed_rgba_alignment_classes(gpu_pkg, align):
    """RGBAPS -> BGRA8 with all four channels: the N = 4 form on whole pixels in every access class."""
    torch = pytest.importorskip("torch")
    check_call(torch, gpu_pkg, "RGBAPS", 8, None, packed("BGRA", 4, 4), (0, 1, 1), dst_align=align)


def test_rows_longer_than_one_trip_of_the_wave(gpu_pkg):
    """Y32 1035 x 8 -> 2070 x 16 bytes: two whole trips of 64 lanes x 16 pixels, a third of two lanes, and a tail of 6."""
    torch = pytest.importorskip("torch")
    check_call(torch, gpu_pkg, "Y32", 8, None, planar(1), (0, 1, 1), n=1, geom=(1035, 8, 2070, 16))


# ---- slices -----------------------------------------------------------------------------------------------------------------------------------

def test_a_call_beyond_the_scratch_cap_runs_in_slices(gpu_pkg):
    """strided_scratch_bytes = two frames' stand-ins -- fp32 rows of 524 x 4 = 2096 and 262 x 4 = 1048 bytes padded to 2304 and 1280,
    76 and 2 x 38 of them: 272 384 bytes a frame -- so 3 frames run as 2 + 1, each slice with a luma and a chroma launch; the result
    equals the unsliced call's, and slice count and scratch bytes equal the formula."""
    torch = pytest.importorskip("torch")
    per_frame = 2304 * 76 + 2 * 1280 * 38
    assert per_frame == sum((w * 4 + 255) // 256 * 256 * h for (w, h) in gpu_pkg.FORMATS["YUV420PS"].plane_dims(524, 76))
    frames = sources(gpu_pkg.FORMATS["YUV420PS"], 262, 38, 3, 255, seed=23)
    try:
        gpu_pkg.set_knob("strided_scratch_bytes", 2 * per_frame)
        sliced, _ = check_call(torch, gpu_pkg, "YUV420PS", 8, None, semi_planar(), (0, 4, 2), n=3, frames=frames, key=("slices", 3))
        assert gpu_pkg.last_strided() == (0, 4, 2, 2 * per_frame), gpu_pkg.last_strided()
    finally:
        gpu_pkg.clear_knob("strided_scratch_bytes")
    whole, _ = check_call(torch, gpu_pkg, "YUV420PS", 8, None, semi_planar(), (0, 2, 1), n=3, frames=frames, key=("slices", 3))
    assert gpu_pkg.last_strided() == (0, 2, 1, 3 * per_frame), gpu_pkg.last_strided()
    assert_equal(sliced, whole, gpu_pkg.FORMATS["YUV420PS"].plane_dims(524, 76), "sliced against unsliced")


# ---- alternation --------------------------------------------------------------------------------------------------------------------------------

def test_narrowed_widened_strided_and_narrowed_alternate_on_one_filter(gpu_pkg):
    """narrowed (-> NV12), widened (NV12 ->), strided (float NV12-style planes) and narrowed (-> P010) on ONE filter and two streams
    without a synchronise in between: the four share the scratch, whose stand-ins have another size in every call.  Every result
    equals that of the same call run alone."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = GEOM
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YUV420PS"], sw, sh, tw, th, device=0, **KW)
    fmt = f.fmt
    a_frames, d_frames = sources(fmt, sw, sh, N, 255, seed=31), sources(fmt, sw, sh, N, 1023, seed=34)
    rng = np.random.default_rng(32)
    b_vals = [[rng.integers(0, 256, (h, w), dtype=np.uint16) for (w, h) in fmt.plane_dims(sw, sh)] for _ in range(N)]
    c_frames = sources(fmt, sw, sh, N, 255, seed=33)

    def sides():
        a = make_sides(torch, f, a_frames, planar(3), semi_planar(), 8, N, seeds=(41, 51))
        b_src = Side(torch, fmt.plane_dims(sw, sh), np.uint8, semi_planar(), N, seed=42).fill(raw_of(b_vals, 8, [0] * 3)).upload()
        b_dst = Side(torch, f.out_dims(), np.float32, planar(3), N, seed=52).upload()
        c_src = Side(torch, fmt.plane_dims(sw, sh), np.float32, semi_planar(), N, seed=43).fill(c_frames).upload()
        c_dst = Side(torch, f.out_dims(), np.float32, semi_planar(), N, seed=53).upload()
        d = make_sides(torch, f, d_frames, planar(3), semi_planar(), 10, N, seeds=(44, 54))
        return a, (b_src, b_dst), (c_src, c_dst), d

    def calls(S, streams, between):
        a, b, c, d = S
        reports = []
        narrowed_call(f, a[0], a[1], None, 8, N, streams[0])
        reports.append(f.last_strided()[:3]), between()
        widened_call(f, b[0], b[1], None, 8, N, streams[1])
        reports.append(f.last_strided()[:3]), between()
        f.process_device_strided(c[0].ptrs(), c[0].pitches(), c[0].steps(), c[0].strides(), c[1].ptrs(), c[1].pitches(), c[1].steps(),
                                 c[1].strides(), N, stream=streams[0].cuda_stream)
        reports.append(f.last_strided()[:3]), between()
        narrowed_call(f, d[0], d[1], [6] * 3, 10, N, streams[1])
        reports.append(f.last_strided()[:3]), between()
        return reports

    together, alone = sides(), sides()
    torch.cuda.synchronize()   # (the uploads are done before the side streams start)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    reports = calls(together, streams, lambda: None)
    torch.cuda.synchronize()
    assert reports == [(0, 2, 1), (2, 0, 1), (1, 1, 1), (0, 2, 1)], reports
    s = torch.cuda.current_stream()
    assert calls(alone, [s, s], torch.cuda.synchronize) == reports
    for k, what in enumerate(("first narrowed call", "widened call", "strided call", "second narrowed call")):
        got, want = together[k][1].frames_and_guards(what), alone[k][1].frames_and_guards(what + " alone")
        if got[0][0].dtype == np.float32:
            assert_bits_equal(got, want, f.out_dims(), what)
        else:
            assert_equal(got, want, f.out_dims(), what)
    # ... and the narrowed ones alone are what the definition says
    for S, frames, bits, shifts in ((alone[0], a_frames, 8, [0] * 3), (alone[3], d_frames, 10, [6] * 3)):
        want = expected(fmt, run_planar(torch, f, frames, N), bits, shifts, np.uint8 if bits == 8 else np.uint16)
        assert_equal(S[1].frames_and_guards("alone"), want, f.out_dims(), f"{bits}-bit narrowed call alone")
    f.close()


# ---- the hook: ties and specials through the kernel itself ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("bits", [8, 10, 12, 16])
def test_hook_over_ties_bounds_and_specials(gpu_pkg, kind, bits):
    """narrow_samples_kernel on one dense row of the values of test_gpu_parity.py::test_integer_conversion_ties (every tie k + 0.5,
    both clamp bounds, values just around ties, huge values, infinities, NaN and negative zero), converted to the input kind first
    (binary16: round to nearest; bfloat16: the upper half of the fp32 pattern), at shift 0 and at the depth's largest shift, and rolled
    so that every value meets another position in a lane's vector and the row's tail."""
    peak = float((1 << bits) - 1)
    ties = np.arange(-3, int(peak) + 3, dtype=np.float64) + 0.5
    if len(ties) > 6000:
        ties = np.concatenate([ties[:3000], ties[-3000:]])
    with np.errstate(over="ignore"):
        vals = np.concatenate([
            ties, np.nextafter(ties.astype(np.float32), np.float32(np.inf)),
            np.nextafter(ties.astype(np.float32), np.float32(-np.inf)),
            np.array([0.0, -0.0, 0.49999997, 0.50000006, peak, peak - 0.5, peak + 0.4999, peak + 0.5, peak + 1e6, 3e9, 1e30,
                      -1e-30, -0.4, -0.5, -0.51, -1e9, np.inf, -np.inf, 1e-45, -1e-45, np.nan, -np.nan]),
            np.random.default_rng(0).uniform(-5, peak + 5, 5000),
        ]).astype(np.float32)
        if kind == "f16":
            given = vals.astype(np.float16)
            r = given.astype(np.float32)
        elif kind == "bf16":
            given = (vals.view(np.uint32) >> 16).astype(np.uint16)
            r = (given.astype(np.uint32) << 16).view(np.float32)
        else:
            given = r = vals
    assert np.isnan(r).any() and np.isposinf(r).any() and np.isneginf(r).any() and (np.signbit(r) & (r == 0)).any()
    spare = (8 if bits == 8 else 16) - bits
    for shift in sorted({0, spare}):
        want = (definition(r, int(peak)) << shift).astype(np.uint8 if bits == 8 else np.uint16)
        for roll in (0, 3):
            got = gpu_pkg.debug_narrow(np.roll(given, roll), bits, shift, bfloat16=kind == "bf16")
            w = np.roll(want, roll)
            assert got.dtype == w.dtype and np.array_equal(got, w), (kind, bits, shift, roll, np.roll(r, roll)[got != w][:8], got[got != w][:8], w[got != w][:8])
