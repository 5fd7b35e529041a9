"""jinc_filter_process_device_widened on the device: INTEGER frames (NV12, P010, Y210, BGRA8, planar 16-bit) into fp32 and binary16
filters.  The result must be, bit for bit (compared as integers), what jinc_filter_process_device computes on the same filter for
dense float / half planes holding the source's values -- built on the host with numpy from the same raw source -- and, for the
cases that say so, the CPU oracle's fp32 result for those planes and the INTEGER filter's result once clamped and rounded.  The
source must come back unchanged and every destination lies inside a larger buffer of pseudo-random bytes whose other bytes must
keep their value (test_strided.py's Side, whose helpers and layouts this file uses).
The common shape is 262 x 38 -> 524 x 76 at tap 3: a luma row is 16 whole lanes' pixels and a tail, the 4:2:0 chroma row of 131
pixels is odd -- some lanes on vectors, a tail, an odd sample count -- and 38 / 19 rows are several row blocks."""
import numpy as np
import pytest

from conftest import oracle_kwargs
from test_shifted import Y210, SharedRowSide
from test_strided import INVALID_ARG, Side, packed, planar, run_planar, semi_planar
from test_widened_host import IDS, REFUSALS

pytestmark = pytest.mark.gpu

GEOM = (262, 38, 524, 76)
KW = dict(tap=3)


def side_for(layout):
    return SharedRowSide if layout == Y210 else Side


def values(pkg, name, sw, sh, bits, n, seed=7):
    """n frames of pseudo-random `bits`-bit values in the filter's plane sizes (uint16 arrays)."""
    rng = np.random.default_rng(seed * 1000 + bits)
    return [[rng.integers(0, 1 << bits, (h, w), dtype=np.uint16) for (w, h) in pkg.FORMATS[name].plane_dims(sw, sh)] for _ in range(n)]


def raw_of(vals, bits, shifts, dirty_seed=None):
    """The values as the source keeps them: value << shift in uint8 / uint16; dirty_seed: pseudo-random bits below AND above the sample."""
    dtype = np.uint8 if bits == 8 else np.uint16
    word = 8 * np.dtype(dtype).itemsize
    rng = np.random.default_rng(dirty_seed)
    out = []
    for planes in vals:
        row = []
        for p, s in zip(planes, shifts):
            r = (p.astype(np.uint32) << s)
            if dirty_seed is not None:
                junk = rng.integers(0, 1 << word, p.shape, dtype=np.uint32)
                r |= junk & ~np.uint32(((1 << bits) - 1) << s) & np.uint32((1 << word) - 1)
            row.append(r.astype(dtype))
        out.append(row)
    return out


def bits_of(a):
    return np.ascontiguousarray(a).view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def assert_bits_equal(got, want, dims, what):
    for k in range(len(want)):
        for i, (w, h) in enumerate(dims):
            a, b = bits_of(got[k][i][:h, :w]), bits_of(want[k][i][:h, :w])
            assert a.dtype == b.dtype
            bad = np.argwhere(a != b)
            assert len(bad) == 0, f"{what}: frame {k} plane {i} differs at {len(bad)} samples; first (x={bad[0][1]}, y={bad[0][0]}): " \
                                  f"got {got[k][i][bad[0][0], bad[0][1]]!r}, want {want[k][i][bad[0][0], bad[0][1]]!r}"


_PLANAR = {}


def planar_reference(torch, f, key, vals, n):
    """jinc_filter_process_device on dense planes of the values converted to the filter's type with numpy: once per case."""
    if key not in _PLANAR:
        dense = [[p.astype(f.fmt.dtype) for p in planes] for planes in vals]
        _PLANAR[key] = run_planar(torch, f, dense, n)
    return _PLANAR[key]


def make_sides(torch, f, raw, src_layout, dst_layout, n, src_align=16, seeds=(11, 12), **side_kw):
    src = side_for(src_layout)(torch, f.fmt.plane_dims(f.src_w, f.src_h), raw[0][0].dtype, src_layout, n, src_align, seed=seeds[0], **side_kw)
    src.fill(raw).upload()
    dst = Side(torch, f.out_dims(), f.fmt.dtype, dst_layout, n, seed=seeds[1]).upload()
    return src, dst


def call(f, src, dst, shifts, bits, n, stream, steps=True):
    f.process_device_widened(src.ptrs(), src.pitches(), src.steps() if steps else None, shifts, bits, src.strides(),
                             dst.ptrs(), dst.pitches(), dst.steps(), dst.strides(), n, stream=stream.cuda_stream)


def assert_source_unchanged(src, what):
    image = src.download()
    for b, B in src.bufs.items():
        assert np.array_equal(image[b], B["host"]), f"{what}: the source buffer {b} was written"


def check_call(torch, pkg, name, geom, n, bits, shifts, src_layout, dst_layout=None, expect_report=None, dirty_seed=None, kw=KW, **side_kw):
    """One widened call against the planar call on the same filter; returns (filter's output frames, values)."""
    sw, sh, tw, th = geom
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=0, **kw)
    planes = f.fmt.planes
    vals = values(pkg, name, sw, sh, bits, n)
    raw = raw_of(vals, bits, shifts or [0] * planes, dirty_seed)
    what = f"{bits}-bit {src_layout} -> {name} {sw}x{sh}->{tw}x{th} {n} frame(s) shifts {shifts}"
    src, dst = make_sides(torch, f, raw, src_layout, dst_layout or planar(planes), n, **side_kw)
    s = torch.cuda.current_stream()
    call(f, src, dst, shifts, bits, n, s)
    s.synchronize()
    report = f.last_strided()
    print(f"{what}: last_strided {report}, last_call {pkg.last_call()}")
    got = dst.frames_and_guards(what)
    assert_source_unchanged(src, what)
    if expect_report is not None:
        assert report[:3] == expect_report, report
    want = planar_reference(torch, f, (name, geom, bits, n, tuple(sorted(kw.items()))), vals, n)
    assert_bits_equal(got, want, f.out_dims(), what + " against the planar call")
    f.close()
    return got, vals


BGRA = packed("BGRA", 4, 3)

# (id, filter, src_bits, shifts, source layout, destination layout or None = planar, (widen, merge, slices))
CASES = [
    ("nv12_f32", "YUV420PS", 8, None, semi_planar(), None, (2, 0, 1)),
    ("p010_f32", "YUV420PS", 10, [6] * 3, semi_planar(), None, (2, 0, 1)),
    ("p010_f16", "YUV420PH", 10, [6] * 3, semi_planar(), None, (2, 0, 1)),
    ("y210_f16", "YUV422PH", 10, [6] * 3, Y210, None, (2, 0, 1)),
    ("bgra8_f32_rgb", "RGBPS", 8, None, BGRA, packed("RGB", 3, 3), (1, 1, 1)),   # interleaved float RGB out through the merge
    ("yuv444p16_f32", "YUV444PS", 16, None, planar(3), None, (1, 0, 1)),
]


# ---- 1. against the float call --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_equals_the_float_call_on_widened_planes(gpu_pkg, case, n):
    torch = pytest.importorskip("torch")
    _, name, bits, shifts, src_layout, dst_layout, report = case
    check_call(torch, gpu_pkg, name, GEOM, n, bits, shifts, src_layout, dst_layout, expect_report=report)


# ---- 2. against the oracle, 3. against the integer filter ---------------------------------------------------------------------------------

def integer_result(torch, pkg, name, raw, shifts, n=1):
    """The integer filter's planar, low-aligned result for the same source and the same source arguments."""
    sw, sh, tw, th = GEOM
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    src = Side(torch, f.fmt.plane_dims(sw, sh), f.fmt.dtype, semi_planar(), n, seed=11).fill(raw).upload()
    dst = Side(torch, f.out_dims(), f.fmt.dtype, planar(3), n, seed=12).upload()
    s = torch.cuda.current_stream()
    if shifts is None:
        f.process_device_strided(src.ptrs(), src.pitches(), src.steps(), src.strides(), dst.ptrs(), dst.pitches(), dst.steps(), dst.strides(), n, stream=s.cuda_stream)
    else:
        f.process_device_shifted(src.ptrs(), src.pitches(), src.steps(), shifts, src.strides(), dst.ptrs(), dst.pitches(), dst.steps(), None, dst.strides(), n, stream=s.cuda_stream)
    s.synchronize()
    got = dst.frames_and_guards(name)
    f.close()
    return got


@pytest.mark.parametrize("bits,shifts,int_name", [(8, None, "YUV420P8"), (10, [6] * 3, "YUV420P10")], ids=["nv12", "p010"])
def test_fp32_equals_the_oracle_and_rounds_to_the_integer_filter(gpu_pkg, O, bits, shifts, int_name):
    """fp32 result == the oracle's fp32 result for the widened planes, bit for bit; and rint(clip(fp32, 0, peak)) == what the integer
    filter stores for the same source through process_device_strided / _shifted, bit for bit: the integer filters convert every
    sample to float before the multiply, so the float result IS their sum in front of clamp and lrintf."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = GEOM
    got, vals = check_call(torch, gpu_pkg, "YUV420PS", GEOM, 1, bits, shifts, semi_planar(), expect_report=(2, 0, 1))
    dims = gpu_pkg.FORMATS["YUV420PS"].plane_dims(tw, th)
    want = O.OracleFilter(O.FORMATS["YUV420PS"], sw, sh, tw, th, **oracle_kwargs(KW)).get_frame([p.astype(np.float32) for p in vals[0]], threads=8)
    assert_bits_equal(got, [want], dims, f"{bits}-bit into YUV420PS against the oracle")
    peak = (1 << bits) - 1
    ints = integer_result(torch, gpu_pkg, int_name, raw_of(vals, bits, shifts or [0] * 3), shifts)
    for i, (w, h) in enumerate(dims):
        r = got[0][i][:h, :w]
        rounded = np.rint(np.clip(r, 0, peak)).astype(ints[0][i].dtype)
        differ = int((rounded != ints[0][i][:h, :w]).sum())
        print(f"{int_name} plane {i}: fp32 range {float(r.min()):.3f} .. {float(r.max()):.3f}, {int((r < 0).sum())} below 0, {int((r > peak).sum())} above the peak, {differ} differ")
        assert differ == 0, f"plane {i}: {differ} samples of the rounded fp32 result differ from {int_name}"


def test_half_equals_the_oracle_narrowed(gpu_pkg, O):
    """P010 into YUV420PH: the oracle's fp32 result for the widened planes, narrowed by numpy.float16 (round to nearest even), bit for
    bit.  No fp32 result reaches 65520, where binary16 overflows: 10-bit sources cannot get there."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = GEOM
    got, vals = check_call(torch, gpu_pkg, "YUV420PH", GEOM, 1, 10, [6] * 3, semi_planar(), expect_report=(2, 0, 1))
    want = O.OracleFilter(O.FORMATS["YUV420PS"], sw, sh, tw, th, **oracle_kwargs(KW)).get_frame([p.astype(np.float32) for p in vals[0]], threads=8)
    dims = gpu_pkg.FORMATS["YUV420PH"].plane_dims(tw, th)
    largest = max(float(np.abs(p[:h, :w]).max()) for p, (w, h) in zip(want, dims))
    print("largest fp32 magnitude", largest)
    assert largest < 65520.0
    assert_bits_equal(got, [[p.astype(np.float16) for p in want]], dims, "P010 into YUV420PH against the oracle narrowed")


# ---- 4. masking ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["YUV420PS", "YUV420PH"])
@pytest.mark.parametrize("shift", [6, 0], ids=["high_aligned_dirty_low_bits", "low_aligned_dirty_high_bits"])
def test_bits_outside_the_sample_are_ignored(gpu_pkg, name, shift):
    """Pseudo-random bits in every position of the word that is not the sample's: the result is the clean source's (the planar call
    on the values)."""
    torch = pytest.importorskip("torch")
    check_call(torch, gpu_pkg, name, GEOM, 1, 10, [shift] * 3, semi_planar(), expect_report=(2, 0, 1), dirty_seed=99)


# ---- 5. alignment classes -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("align", [16, 4, 1])
@pytest.mark.parametrize("bits,shifts,name", [(8, None, "YUV420PS"), (10, [6] * 3, "YUV420PS"), (10, [6] * 3, "YUV420PH")], ids=["nv12_f32", "p010_f32", "p010_f16"])
def test_alignment_classes(gpu_pkg, bits, shifts, name, align):
    """Source base, pitch and frame stride multiples of 16 (16-byte loads), of 4 only (dwords), of the sample size only (sample by
    sample), for the N = 1 form (luma) and the N = 2 form (chroma) of one call."""
    torch = pytest.importorskip("torch")
    check_call(torch, gpu_pkg, name, GEOM, 3, bits, shifts, semi_planar(), expect_report=(2, 0, 1), src_align=align)


@pytest.mark.parametrize("align", [16, 4, 1])
@pytest.mark.parametrize("bits", [8, 10])
def test_incomplete_group_v_without_u(gpu_pkg, bits, align):
    """Y and U dense, V at the second sample of a two-sample pixel whose first sample is not given: the pass reads whole pixels up to
    the last but one and the last V alone, and the U stand-in comes from the dense plane."""
    torch = pytest.importorskip("torch")
    sb = 1 if bits == 8 else 2
    lone_v = [(0, 0, 1), (1, 0, 1), (2, 1, 2)]
    lead = {16: {2: 64 - sb}, 4: {2: 68 - sb}}.get(align)   # V itself on a 16- / 4-byte boundary, so that the pass takes its class's accesses
    check_call(torch, gpu_pkg, "YUV420PS", GEOM, 2, bits, None if bits == 8 else [6] * 3, lone_v, expect_report=(2, 0, 1), src_align=align, lead=lead)


# ---- 6. a second trip along the row ----------------------------------------------------------------------------------------------------------

def test_rows_longer_than_one_trip_of_the_wave(gpu_pkg):
    """2070 bytes a row: two whole trips of 64 lanes x 16 pixels, a third of two lanes, and a tail of 6."""
    torch = pytest.importorskip("torch")
    check_call(torch, gpu_pkg, "Y32", (2070, 16, 4140, 32), 1, 8, None, planar(1), expect_report=(1, 0, 1))


# ---- 7. another geometry ---------------------------------------------------------------------------------------------------------------------

def test_non_2x_geometry(gpu_pkg):
    """262 x 38 -> 359 x 52 (1.37 x): the stand-ins feed whatever kernels the rules choose, not only the periodic family."""
    torch = pytest.importorskip("torch")
    check_call(torch, gpu_pkg, "YUV420PS", (262, 38, 359, 52), 2, 8, None, semi_planar(), expect_report=(2, 0, 1))


# ---- 8. slices ---------------------------------------------------------------------------------------------------------------------------------

def test_a_call_beyond_the_scratch_cap_runs_in_slices(gpu_pkg):
    """strided_scratch_bytes = two frames' stand-ins (fp32 rows of 1048 and 524 bytes padded to 1280 and 768): 5 frames run as
    2 + 2 + 1, each slice with a luma and a chroma launch, and every frame equals its single-frame result."""
    torch = pytest.importorskip("torch")
    per_frame = 1280 * 38 + 2 * 768 * 19
    try:
        gpu_pkg.set_knob("strided_scratch_bytes", 2 * per_frame)
        got, vals = check_call(torch, gpu_pkg, "YUV420PS", GEOM, 5, 8, None, semi_planar(), expect_report=(6, 0, 3))
    finally:
        gpu_pkg.clear_knob("strided_scratch_bytes")
    sw, sh, tw, th = GEOM
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YUV420PS"], sw, sh, tw, th, device=0, **KW)
    s = torch.cuda.current_stream()
    for k in range(5):
        src, dst = make_sides(torch, f, raw_of(vals[k:k + 1], 8, [0] * 3), semi_planar(), planar(3), 1)
        call(f, src, dst, None, 8, 1, s)
        s.synchronize()
        assert f.last_strided()[:3] == (2, 0, 1)
        assert_bits_equal([got[k]], dst.frames_and_guards(f"frame {k} alone"), f.out_dims(), f"frame {k} of the sliced call against its single-frame call")
    f.close()


# ---- 9. streams, and strided calls in between ---------------------------------------------------------------------------------------------------

def test_two_widened_calls_back_to_back_on_two_streams(gpu_pkg):
    """One filter, two calls on different frames queued without a synchronise in between on two streams: they share the stand-ins, so
    the second call's widening waits for the first call's kernels."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = GEOM
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YUV420PS"], sw, sh, tw, th, device=0, **KW)
    vals = values(gpu_pkg, "YUV420PS", sw, sh, 10, 6, seed=8)
    sides = [make_sides(torch, f, raw_of(vals[3 * c:3 * c + 3], 10, [6] * 3), semi_planar(), planar(3), 3, seeds=(21 + c, 31 + c)) for c in range(2)]
    torch.cuda.synchronize()   # (the uploads are done before the side streams start)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for c, (src, dst) in enumerate(sides):
        call(f, src, dst, [6] * 3, 10, 3, streams[c])
    torch.cuda.synchronize()
    want = run_planar(torch, f, [[p.astype(np.float32) for p in planes] for planes in vals], 6)
    for c, (src, dst) in enumerate(sides):
        assert_bits_equal(dst.frames_and_guards(f"call {c}"), want[3 * c:3 * c + 3], f.out_dims(), f"call {c} of two streams")
    f.close()


def test_widened_and_strided_calls_alternate_on_one_filter(gpu_pkg):
    """widened, strided (float NV12-style planes), widened on one stream of one float filter without a synchronise in between: the
    three share the scratch, whose stand-ins have another size in the strided call."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = GEOM
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YUV420PS"], sw, sh, tw, th, device=0, **KW)
    vals = values(gpu_pkg, "YUV420PS", sw, sh, 8, 6, seed=9)
    floats = [[p.astype(np.float32) for p in planes] for planes in vals]
    want = run_planar(torch, f, floats, 6)
    a = make_sides(torch, f, raw_of(vals[0:2], 8, [0] * 3), semi_planar(), planar(3), 2, seeds=(41, 51))
    b_src = Side(torch, f.fmt.plane_dims(sw, sh), np.float32, semi_planar(), 2, seed=42).fill(floats[2:4]).upload()
    b_dst = Side(torch, f.out_dims(), np.float32, semi_planar(), 2, seed=52).upload()
    c = make_sides(torch, f, raw_of(vals[4:6], 8, [0] * 3), semi_planar(), planar(3), 2, seeds=(43, 53))
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    call(f, a[0], a[1], None, 8, 2, s)
    f.process_device_strided(b_src.ptrs(), b_src.pitches(), b_src.steps(), b_src.strides(), b_dst.ptrs(), b_dst.pitches(), b_dst.steps(), b_dst.strides(), 2, stream=s.cuda_stream)
    assert f.last_strided()[:3] == (1, 1, 1)
    call(f, c[0], c[1], None, 8, 2, s)
    assert f.last_strided()[:3] == (2, 0, 1)
    s.synchronize()
    for k0, dst, what in ((0, a[1], "first widened call"), (2, b_dst, "strided call in between"), (4, c[1], "second widened call")):
        assert_bits_equal(dst.frames_and_guards(what), want[k0:k0 + 2], f.out_dims(), what)
    f.close()


# ---- 10. finite flags ---------------------------------------------------------------------------------------------------------------------------

def test_every_frame_is_reported_finite(gpu_pkg):
    """The widened call keeps the float filter's finite scan (it runs enqueue as any float call does) and the scan finds nothing.
    BGRA8 150 x 70 -> RGBPS 300 x 140, the shape at which test_strided.py sees every plane of a float RGB filter take the flagged
    path once the trimmed support is in use at tap 3 (float_trim_min_taps = 0; the 131 x 19 chroma planes of the common shape do not
    take it, with this call or with the planar one): every plane reports flag 0 for every frame."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = 150, 70, 300, 140
    n = 3
    with gpu_pkg.knobs(float_trim_min_taps=0):
        f = gpu_pkg.Filter(gpu_pkg.FORMATS["RGBPS"], sw, sh, tw, th, device=0, **KW)
        assert 0 < f.periodic_support(0) < f.plan_info(0).filter_size
        vals = values(gpu_pkg, "RGBPS", sw, sh, 8, n)
        src, dst = make_sides(torch, f, raw_of(vals, 8, [0] * 3), BGRA, planar(3), n)
        s = torch.cuda.current_stream()
        call(f, src, dst, None, 8, n, s)
        s.synchronize()
        assert f.last_strided()[:3] == (1, 0, 1)
        for i in range(3):
            flags = f.last_finite_flags(i)
            print(f"plane {i} flags {None if flags is None else flags.tolist()}")
            assert flags is not None, f"plane {i} did not take the flagged path"
            assert flags.tolist() == [0] * n, (i, flags.tolist())
        want = run_planar(torch, f, [[p.astype(np.float32) for p in planes] for planes in vals], n)
        assert_bits_equal(dst.frames_and_guards("trimmed support"), want, f.out_dims(), "on the trimmed support")
        f.close()


# ---- 11. refusals ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,kw,says", REFUSALS, ids=IDS)
def test_refusals_write_nothing_and_launch_nothing(gpu_pkg, name, kw, says):
    """The refusals of test_widened_host.py on a filter WITH a device and real buffers: the same error, the destination's bytes as
    they were, and jinc_debug_last_call still names the call made before."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = 40, 24, 80, 48
    marker = gpu_pkg.Filter(gpu_pkg.FORMATS["Y8"], 64, 48, 96, 72, device=0, tap=3)   # a call nothing below could be mistaken for
    run_planar(torch, marker, [[np.zeros((48, 64), np.uint8)]] * 2, 2)
    marker.close()
    before = gpu_pkg.last_call()
    assert before[1] == 2
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[name], sw, sh, tw, th, device=0, tap=3)
    bits = kw.get("src_bits", 8)
    sb = 1 if bits <= 8 else 2
    src = Side(torch, f.fmt.plane_dims(sw, sh), np.uint16, semi_planar(), 1, seed=61).upload()   # (room for either sample size)
    dst = Side(torch, f.out_dims(), f.fmt.dtype, planar(3), 1, seed=62).upload()
    base = src.ptrs()
    usual = (4096, 8192, 8192 + sb)
    ptrs = [base[0], base[1], base[1] + sb]
    ptrs = [p + (given - u) for p, given, u in zip(ptrs, kw.get("ptrs", usual), usual)]
    steps = kw.get("steps", (1, 2, 2))
    with pytest.raises(gpu_pkg.JincError) as e:
        f.process_device_widened(ptrs, list(kw.get("pitches", (80, 80, 80))), None if steps is None else list(steps), kw.get("shifts"), bits,
                                 src.strides(), dst.ptrs(), dst.pitches(), kw.get("dst_steps"), dst.strides(), 1, stream=torch.cuda.current_stream().cuda_stream)
    assert e.value.code == INVALID_ARG and says in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert gpu_pkg.last_call() == before, (before, gpu_pkg.last_call())
    image = dst.download()
    for b, B in dst.bufs.items():
        assert np.array_equal(image[b], B["host"]), "a refused call wrote to the destination"
    f.close()
