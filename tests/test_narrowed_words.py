"""jinc_filter_process_device_narrowed_packed10 / _narrowed_v210 on the device: the results of fp32, binary16 and bfloat16 filters
into Y410 / RGB10A2 words and v210 blocks.  Every comparison is bit for bit, against results the library computes by OTHER calls:
(a) jinc_filter_process_device_packed10 / _v210 on the 10-bit integer filter for integer planes, and (b)
jinc_filter_process_device_narrowed / _narrowed_scaled into planar 10-bit words, packed by numpy.  Every destination lies inside a
larger buffer of pseudo-random bytes whose bytes outside the rows' words / blocks must keep their value (test_packed10.py's
PackedSide, test_v210.py's V210Side), the source must come back unchanged, the spare bits of every word are the fill's and bits
30 - 31 and the absent fields of a partial block are zeros.  The shapes are those files' and test_widened_words.py's (what a lane, a
trip and a tail are is written there)."""
import numpy as np
import pytest

from test_narrowed import assert_equal, sources
from test_narrowed_words_host import KIND_BF16, KIND_HALF, as_float32, codes, v210_blocks
from test_packed10 import BGRX1010102, ODD, OPAQUE, R10G10B10A2, Y410, PackedSide
from test_packed10 import call as call_packed10
from test_packed10 import make_sides as make_packed10_sides
from test_strided import Side, packed, planar, run
from test_v210 import V210Side
from test_v210 import call as call_v210
from test_v210 import make_sides as make_v210_sides
from test_widened import assert_bits_equal, assert_source_unchanged, raw_of, values
from test_widened import call as call_widened
from test_widened import make_sides as make_widened_sides

pytestmark = pytest.mark.gpu

KW = dict(tap=3)
WORDS_WIDE, WORDS_SHORT, WORDS_NARROW = (261, 21, 522, 42), (20, 12, 36, 20), (7, 7, 7, 8)
V210_WIDE, V210_SHORT, V210_MID, V210_NARROW = (386, 9, 772, 18), (20, 12, 36, 20), (22, 8, 44, 16), (14, 7, 16, 8)
RGB = packed("RGB", 3, 3)
FILL = 0x5A5A5A5A   # bits inside and outside every layout's fields


def make_dst(torch, f, kind, n, offsets=Y410, align=16, seed=12, **kw):
    if kind == "packed10":
        return PackedSide(torch, f.out_dims(), offsets, n, align, seed=seed, **kw).upload()
    return V210Side(torch, f.out_dims(), n, align, seed=seed, **kw).upload()


def make_src(torch, f, frames, n, layout=None, seed=11):
    return Side(torch, f.fmt.plane_dims(f.src_w, f.src_h), f.fmt.dtype, layout or planar(3), n, seed=seed).fill(frames).upload()


def call(f, kind, src, dst, n, stream, offsets=Y410, fill=FILL, scales=None, adds=None):
    if kind == "packed10":
        f.process_device_narrowed_packed10(src.ptrs(), src.pitches(), src.steps(), src.strides(), dst.ptrs()[0], dst.pitches()[0], offsets, fill,
                                           scales, adds, dst.strides()[0], n, stream=stream.cuda_stream)
    else:
        f.process_device_narrowed_v210(src.ptrs(), src.pitches(), src.steps(), src.strides(), dst.ptrs()[0], dst.pitches()[0], scales, adds,
                                       dst.strides()[0], n, stream=stream.cuda_stream)


def results(dst, kind, fill, what):
    """The field values of every frame; the guard bytes, the spare bits (words) and the bits that carry no sample (blocks) are checked."""
    return dst.frames_and_guards(fill, what) if kind == "packed10" else dst.frames_and_guards(what)


def planar_codes(torch, f, frames, n, scales=None, adds=None, layout=None):
    """What jinc_filter_process_device_narrowed (_scaled when an array is given) stores with dst_bits 10, steps 1, shifts 0."""
    src = make_src(torch, f, frames, n, layout, seed=21)
    dst = Side(torch, f.out_dims(), np.uint16, planar(3), n, seed=22).upload()
    s = torch.cuda.current_stream()
    if scales is None and adds is None:
        f.process_device_narrowed(src.ptrs(), src.pitches(), src.steps(), src.strides(), dst.ptrs(), dst.pitches(), dst.steps(), None, 10,
                                  dst.strides(), n, stream=s.cuda_stream)
    else:
        f.process_device_narrowed_scaled(src.ptrs(), src.pitches(), src.steps(), src.strides(), dst.ptrs(), dst.pitches(), dst.steps(), None, 10,
                                         scales, adds, dst.strides(), n, stream=s.cuda_stream)
    s.synchronize()
    return dst.frames_and_guards("planar 10-bit words")


def check_against_planar(torch, pkg, kind, name, geom, n, offsets=Y410, fill=FILL, scales=None, adds=None, frames=None, layout=None,
                         expect_report=(0, 1, 1), seed=5, **dst_kw):
    """One call against the planar narrowed call on the same filter and planes; returns (field values, report, the filter's groups)."""
    sw, sh, tw, th = geom
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    if frames is None:
        frames = sources(f.fmt, sw, sh, n, 1023, seed)
    what = f"{name} {sw}x{sh}->{tw}x{th} {n} frame(s) -> {kind} {offsets if kind == 'packed10' else ''} scales {scales} offsets {adds} {dst_kw}"
    src, dst = make_src(torch, f, frames, n, layout), make_dst(torch, f, kind, n, offsets, **dst_kw)
    s = torch.cuda.current_stream()
    call(f, kind, src, dst, n, s, offsets, fill, scales, adds)
    s.synchronize()
    report, groups = f.last_strided(), pkg.last_groups()
    print(f"{what}: last_strided {report}, groups {groups}")
    got = results(dst, kind, fill, what)
    assert_source_unchanged(src, what)
    if expect_report is not None:
        assert report[:3] == expect_report, report
    want = planar_codes(torch, f, frames, n, scales, adds, layout)
    assert_equal(got, want, f.out_dims(), what + " against the planar narrowed call")
    f.close()
    return got, report, groups


# ---- 1. consequence (a): the integer filters' words and blocks -----------------------------------------------------------------------------

def check_against_integer_filter(torch, pkg, kind, name, int_name, geom, n, offsets=Y410, fill=OPAQUE, layout=None, expect_report=(0, 1, 1)):
    """An fp32 filter on integer planes 0 .. 1023, no scale and no offset: the whole destination buffer -- words or blocks, and
    every guard byte around them -- equals the one process_device_packed10 / process_device_v210 leaves on the 10-bit filter."""
    sw, sh, tw, th = geom
    vals = values(pkg, int_name, sw, sh, 10, n)
    s = torch.cuda.current_stream()
    fi = pkg.Filter(pkg.FORMATS[int_name], sw, sh, tw, th, device=0, **KW)
    if kind == "packed10":
        isrc, idst = make_packed10_sides(torch, fi, vals, None, offsets, n)
        call_packed10(fi, isrc, idst, None, offsets, fill, n, s)
    else:
        isrc, idst = make_v210_sides(torch, fi, vals, False, True, n)
        call_v210(fi, isrc, idst, False, True, n, s)
    s.synchronize()
    want_image = idst.download()
    want = results(idst, kind, fill, int_name)
    fi.close()
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    frames = [[p.astype(np.float32) for p in planes] for planes in vals]
    src, dst = make_src(torch, f, frames, n, layout), make_dst(torch, f, kind, n, offsets)   # (the same pseudo-random buffer: seed 12)
    assert np.array_equal(dst.host, idst.host)
    call(f, kind, src, dst, n, s, offsets, fill)
    s.synchronize()
    what = f"{name} against {int_name} {sw}x{sh}->{tw}x{th} {n} frame(s) {kind} {offsets}"
    report = f.last_strided()
    print(f"{what}: last_strided {report}")
    got = results(dst, kind, fill, what)
    assert_source_unchanged(src, what)
    assert report[:3] == expect_report, report
    assert_equal(got, want, f.out_dims(), what)
    assert np.array_equal(dst.download(), want_image), f"{what}: the buffers differ"
    f.close()


WORDS_CASES = [("y410", "YUV444PS", "YUV444P10", Y410, None, (0, 1, 1)), ("r10g10b10a2", "RGBPS", "RGBP10", R10G10B10A2, None, (0, 1, 1)),
               ("bgrx1010102_from_rgb", "RGBPS", "RGBP10", BGRX1010102, RGB, (1, 1, 1))]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("geom", [WORDS_WIDE, WORDS_SHORT, WORDS_NARROW], ids=["261x21", "20x12", "7x7"])
@pytest.mark.parametrize("case", WORDS_CASES, ids=[c[0] for c in WORDS_CASES])
def test_words_equal_the_integer_filters_words(gpu_pkg, case, geom, n):
    torch = pytest.importorskip("torch")
    _, name, int_name, offsets, layout, report = case
    check_against_integer_filter(torch, gpu_pkg, "packed10", name, int_name, geom, n, offsets, layout=layout, expect_report=report)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("geom", [V210_WIDE, V210_SHORT, V210_MID, V210_NARROW], ids=["386x9", "20x12", "22x8", "14x7"])
def test_blocks_equal_the_integer_filters_blocks(gpu_pkg, geom, n):
    torch = pytest.importorskip("torch")
    check_against_integer_filter(torch, gpu_pkg, "v210", "YUV422PS", "YUV422P10", geom, n)


# ---- 2. consequence (b): the planar narrowed calls' values ----------------------------------------------------------------------------------

def to_code_pairs(pkg, rng):
    luma, chroma = pkg.code_range(10, rng, pkg.PLANE_LUMA_OR_RGB), pkg.code_range(10, rng, pkg.PLANE_CHROMA)
    return [float(luma[2]), float(chroma[2]), float(chroma[2])], [float(luma[3]), float(chroma[3]), float(chroma[3])]


def unit_range_sources(fmt, sw, sh, n, seed):
    """Planes uniform in -0.1 .. 1.1: scaled to code values they fall on both sides of both bounds."""
    from test_narrowed import to_type
    rng = np.random.default_rng(seed)
    return [[to_type(fmt, rng.uniform(-0.1, 1.1, (h, w))) for (w, h) in fmt.plane_dims(sw, sh)] for _ in range(n)]


PAIRS = ["none", "full", "limited", "negative"]


@pytest.mark.parametrize("pairs", PAIRS)
@pytest.mark.parametrize("kind,family,geom", [("packed10", "YUV444P", WORDS_WIDE), ("v210", "YUV422P", V210_WIDE)], ids=["words", "v210"])
@pytest.mark.parametrize("suffix", ["S", "H", "BF"], ids=["f32", "f16", "bf16"])
def test_fields_equal_the_planar_narrowed_call(gpu_pkg, suffix, kind, family, geom, pairs):
    torch = pytest.importorskip("torch")
    name = family + suffix
    fmt, (sw, sh) = gpu_pkg.FORMATS[name], geom[:2]
    if pairs == "none":
        scales, adds, frames = None, None, sources(fmt, sw, sh, 2, 1023, 5)
    else:
        frames = unit_range_sources(fmt, sw, sh, 2, 6)
        if pairs == "negative":
            scales, adds = [-1023.0, 1023.0, 1023.0], [1023.0, 0.0, 0.0]
        else:
            scales, adds = to_code_pairs(gpu_pkg, gpu_pkg.RANGE_FULL if pairs == "full" else gpu_pkg.RANGE_LIMITED)
            assert scales[0] != scales[1] or adds[0] != adds[1]   # luma and chroma pairs differ per plane
    got, _, groups = check_against_planar(torch, gpu_pkg, kind, name, geom, 2, scales=scales, adds=adds, frames=frames)
    assert groups[-1]["scaled"] == (0 if pairs == "none" else 1) and groups[-1]["sample_type"] == fmt.sample_type
    if pairs != "limited":   # (limited range leaves the planes a few codes beyond the bounds only: no claim there)
        spread = {int(p.min()) for p in got[0]} | {int(p.max()) for p in got[0]}
        assert 0 in spread and 1023 in spread, spread   # both bounds are reached


def test_only_one_array_given(gpu_pkg):
    """A NULL scale array means 1.0, a NULL offset array 0.0: each alone runs the scaled form."""
    torch = pytest.importorskip("torch")
    check_against_planar(torch, gpu_pkg, "packed10", "YUV444PS", WORDS_SHORT, 1, scales=[0.5, 2.0, -1.0])
    check_against_planar(torch, gpu_pkg, "v210", "YUV422PH", V210_SHORT, 1, adds=[-100.25, 64.0, 0.5])


# ---- 3. second trips along the row ----------------------------------------------------------------------------------------------------------

def test_word_rows_longer_than_one_trip_of_the_wave(gpu_pkg):
    """1030 words a row: two whole trips of 64 lanes x 8 pixels and a tail of 6."""
    torch = pytest.importorskip("torch")
    _, _, groups = check_against_planar(torch, gpu_pkg, "packed10", "YUV444PS", (515, 8, 1030, 16), 1)
    (narrow,) = groups
    assert (narrow["direction"], narrow["n"], narrow["members"], narrow["unit"], narrow["vec_pixels"], narrow["width"], narrow["rows"]) == (10, 3, 3, 16, 1024, 1030, 16), narrow


def test_v210_rows_longer_than_one_trip_of_the_wave(gpu_pkg):
    """782 pixels a row: 130 whole blocks and a 2-pixel partial one, so lanes 0 and 1 make a second trip of the paired loop of
    narrow_v210_kernel, DPP exchange included."""
    torch = pytest.importorskip("torch")
    _, _, groups = check_against_planar(torch, gpu_pkg, "v210", "YUV422PS", (390, 7, 782, 14), 2)
    (narrow,) = groups
    assert (narrow["direction"], narrow["n"], narrow["members"], narrow["unit"], narrow["vec_pixels"], narrow["width"], narrow["rows"]) == (11, 3, 3, 16, 780, 782, 14), narrow


# ---- 4. access classes ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,name,geom", [("packed10", "YUV444PS", WORDS_WIDE), ("packed10", "YUV444PBF", WORDS_SHORT), ("v210", "YUV422PS", V210_WIDE),
                                            ("v210", "YUV422PH", V210_SHORT)], ids=["words_f32", "words_bf16", "v210_f32", "v210_f16"])
def test_alignment_classes(gpu_pkg, kind, name, geom):
    """Destination base, pitch and frame stride multiples of 16 (16-byte stores) and of 4 only (lead 68, pitch and frame stride 4 mod
    16: dwords): the same bits, and the record shows the unit."""
    torch = pytest.importorskip("torch")
    got = {}
    for align in (16, 4):
        got[align], _, groups = check_against_planar(torch, gpu_pkg, kind, name, geom, 3, offsets=ODD, align=align)
        (narrow,) = groups
        vec = geom[2] // 8 * 8 if kind == "packed10" else 6 * (geom[2] // 6 // 2 * 2)
        assert (narrow["direction"], narrow["unit"], narrow["vec_pixels"], narrow["width"], narrow["rows"]) == (10 if kind == "packed10" else 11, align, vec, geom[2], geom[3]), narrow
        assert narrow["sample_bytes"] == gpu_pkg.FORMATS[name].sample_bytes
    assert_equal(got[4], got[16], gpu_pkg.FORMATS[name].plane_dims(geom[2], geom[3]), "multiples of 4 only against multiples of 16")


def test_the_conventional_128_byte_v210_pitch_keeps_its_padding(gpu_pkg):
    torch = pytest.importorskip("torch")
    from test_v210 import conventional_pitch, row_bytes
    tw, th = V210_WIDE[2:]
    pitch = conventional_pitch(tw)
    assert pitch > row_bytes(tw) and pitch % 128 == 0 and gpu_pkg.v210_row_bytes(tw) == row_bytes(tw)
    check_against_planar(torch, gpu_pkg, "v210", "YUV422PS", V210_WIDE, 3, pitch=pitch, fs=pitch * th)
    check_against_planar(torch, gpu_pkg, "v210", "YUV422PH", V210_SHORT, 2, pitch=row_bytes(V210_SHORT[2]), fs=row_bytes(V210_SHORT[2]) * V210_SHORT[3])


# ---- 5. the hooks: ties, non-finite values, all patterns --------------------------------------------------------------------------------------

def tie_table():
    ties = np.arange(-3, 1026, dtype=np.float32) + np.float32(0.5)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, -0.25, -1e30, 1e30, 1023.0, 1023.49, 1023.5, 1024.0, 0.49999997, 0.50000006], np.float32)
    return np.concatenate([ties, special, np.full(5, 0.5, np.float32)])   # (... and a tail that is no whole lane)


def hook_planes(kind):
    """(the three rows for the fields hook, their kernel kind, bfloat16 flag)"""
    if kind == "f32":
        t = tie_table()
        return [t, np.roll(t, 7), t[::-1].copy()], 0, False
    patterns = np.arange(65536 + 5, dtype=np.uint32).astype(np.uint16)
    rows = [patterns, np.roll(patterns, 7), patterns[::-1].copy()]
    if kind == "f16":
        return [r.view(np.float16) for r in rows], KIND_HALF, False
    return rows, KIND_BF16, True


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_hooks_equal_numpy_on_ties_non_finite_values_and_all_patterns(gpu_pkg, kind, scaled):
    rows, kernel_kind, bf16 = hook_planes(kind)
    scales, adds = ([0.5, -1.0, 1.0009775], [100.25, 1000.0, -0.5]) if scaled else (None, None)
    raw = [np.ascontiguousarray(r).view(np.uint8) for r in rows]
    v = [codes(as_float32(raw[c], kernel_kind), scaled, scales[c] if scaled else 1, adds[c] if scaled else 0) for c in range(3)]
    # words
    got = gpu_pkg.debug_narrow_fields(rows, ODD, 0xFFFFFFFF, scales, adds, bfloat16=bf16)
    mask = sum(1023 << o for o in ODD)
    want = np.full(v[0].size, 0xFFFFFFFF & ~mask, np.uint32)
    for c, o in enumerate(ODD):
        want |= v[c] << np.uint32(o)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} words differ, first at {int(bad[0])}: got {int(got[bad[0]]):#x}, want {int(want[bad[0]]):#x}"
    # blocks: the first row as luma, halves of the two others as chroma
    width = rows[0].size // 2 * 2
    planes = [rows[0][:width], rows[1][:width // 2], rows[2][:width // 2]]
    got = gpu_pkg.debug_narrow_v210(planes, scales, adds, bfloat16=bf16)
    want = v210_blocks([v[0][:width].reshape(1, -1), v[1][:width // 2].reshape(1, -1), v[2][:width // 2].reshape(1, -1)]).reshape(-1)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} block words differ, first at {int(bad[0])}: got {int(got[bad[0]]):#x}, want {int(want[bad[0]]):#x}"


# ---- 6. slices, streams and other calls in between ---------------------------------------------------------------------------------------------

# Result stand-ins per frame, fp32 rows padded to 256 bytes.  Words: 3 planes of 522 x 4 = 2088 -> 2304 bytes x 42 rows.  v210: luma
# 772 x 4 = 3088 -> 3328 bytes, each chroma plane 386 x 4 = 1544 -> 1792 bytes, x 18 rows: the small-shape counterpart of the
# header's 3 x 15 360 x 2160 and (15 360 + 2 x 7680) x 2160.
SLICES = [("packed10", "YUV444PS", WORDS_WIDE, 3 * 2304 * 42), ("v210", "YUV422PS", V210_WIDE, 18 * (3328 + 2 * 1792))]


@pytest.mark.parametrize("kind,name,geom,per_frame", SLICES, ids=["words", "v210"])
def test_a_call_beyond_the_scratch_cap_runs_in_slices(gpu_pkg, kind, name, geom, per_frame):
    """strided_scratch_bytes = two frames' stand-ins: 5 frames run as 2 + 2 + 1 with one narrowing launch each, the scratch the call
    reports is exactly the two frames' derived size, and the result equals the one-slice run."""
    torch = pytest.importorskip("torch")
    one, report, _ = check_against_planar(torch, gpu_pkg, kind, name, geom, 5, seed=9)
    assert report[:3] == (0, 1, 1) and report[3] >= 5 * per_frame
    with gpu_pkg.knobs(strided_scratch_bytes=2 * per_frame):
        sw, sh, tw, th = geom
        f = gpu_pkg.Filter(gpu_pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
        frames = sources(f.fmt, sw, sh, 5, 1023, 9)
        src, dst = make_src(torch, f, frames, 5), make_dst(torch, f, kind, 5)
        s = torch.cuda.current_stream()
        call(f, kind, src, dst, 5, s)
        s.synchronize()
        report = f.last_strided()
        assert report == (0, 3, 3, 2 * per_frame), (report, per_frame)
        assert_equal(results(dst, kind, FILL, "sliced"), one, f.out_dims(), "the sliced call against the one-slice call")
        f.close()


def test_strided_new_and_widened_calls_alternate_on_two_streams(gpu_pkg):
    """A strided call (interleaved float RGB in and out), the new call, an 8-bit widened call and the new call again on ONE RGBPS
    filter, alternating between two streams without a synchronise in between: they share the stand-ins and leave each other's
    results alone."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = WORDS_WIDE
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["RGBPS"], sw, sh, tw, th, device=0, **KW)
    fa, fb, fc = (sources(f.fmt, sw, sh, 2, 1023, seed) for seed in (31, 32, 33))
    vals = values(gpu_pkg, "RGBPS", sw, sh, 8, 2, seed=9)
    # what each call must give, each from a run of its own
    want_strided = run(torch, f, fa, RGB, RGB, 2)
    want_b, want_c = planar_codes(torch, f, fb, 2), planar_codes(torch, f, fc, 2)
    wsrc, wdst = make_widened_sides(torch, f, raw_of(vals, 8, [0] * 3), planar(3), planar(3), 2, seeds=(42, 52))
    s0 = torch.cuda.current_stream()
    call_widened(f, wsrc, wdst, None, 8, 2, s0)
    s0.synchronize()
    want_widened = wdst.frames_and_guards("widened alone")
    # the four calls
    a_src = Side(torch, f.fmt.plane_dims(sw, sh), np.float32, RGB, 2, seed=61).fill(fa).upload()
    a_dst = Side(torch, f.out_dims(), np.float32, RGB, 2, seed=62).upload()
    b_src, b_dst = make_src(torch, f, fb, 2, seed=63), make_dst(torch, f, "packed10", 2, R10G10B10A2, seed=64)
    wsrc2, wdst2 = make_widened_sides(torch, f, raw_of(vals, 8, [0] * 3), planar(3), planar(3), 2, seeds=(65, 66))
    c_src, c_dst = make_src(torch, f, fc, 2, RGB, seed=67), make_dst(torch, f, "packed10", 2, BGRX1010102, align=4, seed=68)
    torch.cuda.synchronize()   # (the uploads are done before the side streams start)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    f.process_device_strided(a_src.ptrs(), a_src.pitches(), a_src.steps(), a_src.strides(), a_dst.ptrs(), a_dst.pitches(), a_dst.steps(), a_dst.strides(), 2,
                             stream=streams[0].cuda_stream)
    assert f.last_strided()[:3] == (1, 1, 1)
    call(f, "packed10", b_src, b_dst, 2, streams[1], R10G10B10A2)
    assert f.last_strided()[:3] == (0, 1, 1)
    call_widened(f, wsrc2, wdst2, None, 8, 2, streams[0])
    assert f.last_strided()[:3] == (1, 0, 1)
    call(f, "packed10", c_src, c_dst, 2, streams[1], BGRX1010102)
    assert f.last_strided()[:3] == (1, 1, 1)
    torch.cuda.synchronize()
    assert_bits_equal(a_dst.frames_and_guards("strided"), want_strided, f.out_dims(), "the strided call")
    assert_equal(results(b_dst, "packed10", FILL, "first new call"), want_b, f.out_dims(), "the first new call")
    assert_bits_equal(wdst2.frames_and_guards("widened"), want_widened, f.out_dims(), "the widened call in between")
    assert_equal(results(c_dst, "packed10", FILL, "second new call"), want_c, f.out_dims(), "the second new call")
    f.close()
