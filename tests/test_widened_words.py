"""jinc_filter_process_device_widened_packed10 / _v210 on the device: Y410 / RGB10A2 words and v210 blocks into fp32 and binary16
filters.  The result must be, bit for bit (compared as integers), what jinc_filter_process_device computes on the same filter for
dense float / half planes holding the field values -- built on the host with numpy -- and, for the cases that say so, the CPU
oracle's fp32 result for those planes and the INTEGER filter's result for the same source once clamped and rounded.  Every source
carries pseudo-random bits wherever no sample lies (outside the fields, in bits 30 - 31, in the fields of a partial block beyond
`width`, in the row padding) and must come back unchanged; every destination lies inside a larger buffer of pseudo-random bytes
whose other bytes must keep their value.  The sides are test_packed10.py's PackedSide, test_v210.py's V210Side and
test_strided.py's Side; the shapes are those files' (what a lane, a trip and a tail are is written there)."""
import numpy as np
import pytest

from conftest import oracle_kwargs
from test_packed10 import BGRX1010102, ODD, R10G10B10A2, Y410, PackedSide
from test_packed10 import call as call_packed10
from test_packed10 import make_sides as make_packed10_sides
from test_strided import INVALID_ARG, Side, packed, planar, run_planar, semi_planar
from test_v210 import V210Side, conventional_pitch, row_bytes
from test_v210 import call as call_v210
from test_v210 import make_sides as make_v210_sides
from test_widened import assert_bits_equal, planar_reference, raw_of, values
from test_widened import call as call_widened
from test_widened import make_sides as make_widened_sides

pytestmark = pytest.mark.gpu

KW = dict(tap=3)
WORDS_WIDE, WORDS_SHORT, WORDS_NARROW = (261, 21, 522, 42), (20, 12, 36, 20), (7, 7, 7, 8)
V210_WIDE, V210_SHORT, V210_MID, V210_NARROW = (386, 9, 772, 18), (20, 12, 36, 20), (22, 8, 44, 16), (14, 7, 16, 8)
RGB = packed("RGB", 3, 3)


def make_source(torch, f, kind, vals, n, offsets=Y410, align=16, seed=11, clean=False, **src_kw):
    dims = f.fmt.plane_dims(f.src_w, f.src_h)
    src = PackedSide(torch, dims, offsets, n, align, seed=seed, **src_kw) if kind == "packed10" else V210Side(torch, dims, n, align, seed=seed, **src_kw)
    if clean:
        src.host[...] = 0
    return src.fill(vals).upload()


def call(f, kind, src, dst, n, stream, offsets=Y410):
    if kind == "packed10":
        f.process_device_widened_packed10(src.ptrs()[0], src.pitches()[0], offsets, src.strides()[0], dst.ptrs(), dst.pitches(), dst.steps(), dst.strides(), n,
                                          stream=stream.cuda_stream)
    else:
        f.process_device_widened_v210(src.ptrs()[0], src.pitches()[0], src.strides()[0], dst.ptrs(), dst.pitches(), dst.steps(), dst.strides(), n,
                                      stream=stream.cuda_stream)


def check_call(torch, pkg, kind, name, geom, n, offsets=Y410, dst_layout=None, expect_report=(1, 0, 1), kw=KW, seed=7, **src_kw):
    """One call against the planar call on the same filter; returns (the call's output frames, the values, the report)."""
    sw, sh, tw, th = geom
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=0, **kw)
    vals = values(pkg, name, sw, sh, 10, n, seed=seed)
    what = f"{kind} {offsets if kind == 'packed10' else ''} -> {name} {sw}x{sh}->{tw}x{th} {n} frame(s) {src_kw}"
    src = make_source(torch, f, kind, vals, n, offsets, **src_kw)
    dst = Side(torch, f.out_dims(), f.fmt.dtype, dst_layout or planar(3), n, seed=12).upload()
    s = torch.cuda.current_stream()
    call(f, kind, src, dst, n, s, offsets)
    s.synchronize()
    report = f.last_strided()
    print(f"{what}: last_strided {report}, last_call {pkg.last_call()}")
    got = dst.frames_and_guards(what)
    assert np.array_equal(src.download(), src.host), f"{what}: the source was written"
    if expect_report is not None:
        assert report[:3] == expect_report, report
    want = planar_reference(torch, f, ("words", name, geom, n, seed, tuple(sorted(kw.items()))), vals, n)
    assert_bits_equal(got, want, f.out_dims(), what + " against the planar call")
    f.close()
    return got, vals, report


# ---- 1. against the float call --------------------------------------------------------------------------------------------------------

WORDS_CASES = [("y410_f32", "YUV444PS", Y410, None, (1, 0, 1)), ("y410_f16", "YUV444PH", Y410, None, (1, 0, 1)),
               ("r10g10b10a2_f32", "RGBPS", R10G10B10A2, None, (1, 0, 1)), ("bgrx1010102_f32_rgb", "RGBPS", BGRX1010102, RGB, (1, 1, 1))]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("geom", [WORDS_WIDE, WORDS_SHORT, WORDS_NARROW], ids=["261x21", "20x12", "7x7"])
@pytest.mark.parametrize("case", WORDS_CASES, ids=[c[0] for c in WORDS_CASES])
def test_words_equal_the_float_call_on_widened_planes(gpu_pkg, case, geom, n):
    torch = pytest.importorskip("torch")
    _, name, offsets, dst_layout, report = case
    check_call(torch, gpu_pkg, "packed10", name, geom, n, offsets, dst_layout, expect_report=report)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("geom", [V210_WIDE, V210_SHORT, V210_MID, V210_NARROW], ids=["386x9", "20x12", "22x8", "14x7"])
@pytest.mark.parametrize("name", ["YUV422PS", "YUV422PH"])
def test_v210_equals_the_float_call_on_widened_planes(gpu_pkg, name, geom, n):
    torch = pytest.importorskip("torch")
    check_call(torch, gpu_pkg, "v210", name, geom, n)


# ---- 2. a second trip along the row ----------------------------------------------------------------------------------------------------------

def test_word_rows_longer_than_one_trip_of_the_wave(gpu_pkg):
    """1030 words a row: two whole trips of 64 lanes x 8 pixels and a tail of 6."""
    torch = pytest.importorskip("torch")
    check_call(torch, gpu_pkg, "packed10", "YUV444PS", (1030, 8, 2060, 16), 1)


def test_v210_rows_longer_than_one_trip_of_the_wave(gpu_pkg):
    """782 pixels a row: 130 whole blocks and a 2-pixel partial one, so lanes 0 and 1 make a second trip of the paired loop of
    widen_v210_kernel, DPP exchange included."""
    torch = pytest.importorskip("torch")
    check_call(torch, gpu_pkg, "v210", "YUV422PS", (782, 7, 1564, 14), 2)
    (widen,) = gpu_pkg.last_groups()
    assert (widen["direction"], widen["unit"], widen["vec_pixels"], widen["width"]) == (9, 16, 780, 782) and widen["vec_pixels"] > 6 * 128


# ---- 3. against the oracle and the integer filter ------------------------------------------------------------------------------------------

KINDS = [("packed10", "YUV444P", WORDS_WIDE), ("v210", "YUV422P", V210_WIDE)]
_ORACLE = {}


def oracle_fp32(O, kind, family, geom, vals):
    if kind not in _ORACLE:
        sw, sh, tw, th = geom
        _ORACLE[kind] = O.OracleFilter(O.FORMATS[family + "S"], sw, sh, tw, th, **oracle_kwargs(KW)).get_frame([p.astype(np.float32) for p in vals[0]], threads=8)
    return _ORACLE[kind]


@pytest.mark.parametrize("kind,family,geom", KINDS, ids=[k[0] for k in KINDS])
def test_fp32_equals_the_oracle_and_rounds_to_the_integer_filter(gpu_pkg, O, kind, family, geom):
    """fp32 result == the oracle's fp32 result for the widened planes, bit for bit; and rint(clip(fp32, 0, 1023)) == what
    process_device_packed10 / process_device_v210 store into planar YUV444P10 / YUV422P10 for the same source, with 0 samples
    differing: the integer filters convert every sample to float before the multiply, so the float result IS their sum in front of
    clamp and lrintf."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = geom
    got, vals, _ = check_call(torch, gpu_pkg, kind, family + "S", geom, 1)
    dims = gpu_pkg.FORMATS[family + "S"].plane_dims(tw, th)
    assert_bits_equal(got, [oracle_fp32(O, kind, family, geom, vals)], dims, f"{kind} into {family}S against the oracle")
    fi = gpu_pkg.Filter(gpu_pkg.FORMATS[family + "10"], sw, sh, tw, th, device=0, **KW)
    s = torch.cuda.current_stream()
    if kind == "packed10":
        src, dst = make_packed10_sides(torch, fi, vals, Y410, None, 1)
        call_packed10(fi, src, dst, Y410, None, 0, 1, s)
    else:
        src, dst = make_v210_sides(torch, fi, vals, True, False, 1)
        call_v210(fi, src, dst, True, False, 1, s)
    s.synchronize()
    ints = dst.frames_and_guards(f"{family}10")
    fi.close()
    for i, (w, h) in enumerate(dims):
        r = got[0][i][:h, :w]
        rounded = np.rint(np.clip(r, 0, 1023)).astype(np.uint16)
        differ = int((rounded != ints[0][i][:h, :w]).sum())
        print(f"{family}10 plane {i}: fp32 range {float(r.min()):.3f} .. {float(r.max()):.3f}, {int((r < 0).sum())} below 0, {int((r > 1023).sum())} above the peak, {differ} differ")
        assert differ == 0, f"plane {i}: {differ} samples of the rounded fp32 result differ from {family}10"


@pytest.mark.parametrize("kind,family,geom", KINDS, ids=[k[0] for k in KINDS])
def test_half_equals_the_oracle_narrowed(gpu_pkg, O, kind, family, geom):
    """The oracle's fp32 result for the widened planes, narrowed by numpy.float16 (round to nearest even), bit for bit.  No fp32
    result reaches 65520, where binary16 overflows: 10-bit sources cannot get there."""
    torch = pytest.importorskip("torch")
    got, vals, _ = check_call(torch, gpu_pkg, kind, family + "H", geom, 1)
    want = oracle_fp32(O, kind, family, geom, vals)
    dims = gpu_pkg.FORMATS[family + "H"].plane_dims(geom[2], geom[3])
    largest = max(float(np.abs(p[:h, :w]).max()) for p, (w, h) in zip(want, dims))
    print("largest fp32 magnitude", largest)
    assert largest < 65520.0
    assert_bits_equal(got, [[p.astype(np.float16) for p in want]], dims, f"{kind} into {family}H against the oracle narrowed")


# ---- 4. bits that carry no sample --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,name,geom,offsets", [("packed10", "YUV444PS", WORDS_WIDE, ODD), ("packed10", "RGBPH", WORDS_SHORT, BGRX1010102),
                                                    ("v210", "YUV422PS", V210_WIDE, None), ("v210", "YUV422PH", V210_MID, None)],
                         ids=["words_spare_10_21_f32", "words_bgrx_f16", "v210_386_f32", "v210_22_f16"])
def test_bits_that_carry_no_sample_are_ignored(gpu_pkg, kind, name, geom, offsets):
    """The same values once in a buffer of zeros and once in a buffer of pseudo-random bytes -- spare bits of the words; bits
    30 - 31, the fields of the partial last block beyond `width` (386 and 22 leave some) and the row padding of v210: the two
    results are equal, and both are the planar call's on the values."""
    torch = pytest.importorskip("torch")
    clean, _, _ = check_call(torch, gpu_pkg, kind, name, geom, 2, offsets, clean=True)
    dirty, _, _ = check_call(torch, gpu_pkg, kind, name, geom, 2, offsets)
    sw, sh, tw, th = geom
    assert_bits_equal(dirty, clean, gpu_pkg.FORMATS[name].plane_dims(tw, th), "dirty source against the clean one")


# ---- 5. alignment classes, pitches, refusals -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("align", [16, 4])
@pytest.mark.parametrize("kind,name,geom", [("packed10", "YUV444PS", WORDS_WIDE), ("packed10", "YUV444PH", WORDS_SHORT), ("v210", "YUV422PS", V210_WIDE),
                                            ("v210", "YUV422PH", V210_SHORT)], ids=["words_f32", "words_f16", "v210_f32", "v210_f16"])
def test_alignment_classes(gpu_pkg, kind, name, geom, align):
    """Source base, pitch and frame stride multiples of 16 (16-byte loads) and of 4 only (lead 68, pitch and frame stride 4 mod 16:
    dwords)."""
    torch = pytest.importorskip("torch")
    check_call(torch, gpu_pkg, kind, name, geom, 3, align=align)
    # the record (jinc_debug_last_groups): widen_fields is direction 6 (8 pixels a lane and step), widen_v210 9 (vec_pixels: 6 pixels x
    # the blocks that move in pairs); the destination's planes are dense and leave no entry
    (widen,) = gpu_pkg.last_groups()
    vec = geom[0] // 8 * 8 if kind == "packed10" else 6 * (geom[0] // 6 // 2 * 2)
    assert (widen["direction"], widen["unit"], widen["vec_pixels"], widen["width"], widen["rows"]) == (6 if kind == "packed10" else 9, align, vec, geom[0], geom[1]), widen
    assert widen["sample_bytes"] == gpu_pkg.FORMATS[name].sample_bytes and widen["sample_type"] == gpu_pkg.FORMATS[name].sample_type


@pytest.mark.parametrize("kind,name,geom", [("packed10", "YUV444PS", WORDS_SHORT), ("v210", "YUV422PS", V210_WIDE), ("v210", "YUV422PH", V210_SHORT)],
                         ids=["words", "v210_386", "v210_20"])
def test_the_smallest_pitch_is_accepted(gpu_pkg, kind, name, geom):
    """pitch = 4 * width / v210_row_bytes(width): rows follow each other without padding, the frames too."""
    torch = pytest.importorskip("torch")
    sw, sh = geom[:2]
    pitch = 4 * sw if kind == "packed10" else row_bytes(sw)
    if kind == "v210":
        assert gpu_pkg.v210_row_bytes(sw) == pitch
    check_call(torch, gpu_pkg, kind, name, geom, 3, pitch=pitch, fs=pitch * sh)


@pytest.mark.parametrize("geom", [V210_WIDE, V210_SHORT], ids=["386x9", "20x12"])
def test_the_conventional_128_byte_v210_pitch(gpu_pkg, geom):
    """Rows padded to 128 bytes (48 pixels) as capture cards write them, frames back to back; the padding holds pseudo-random bytes."""
    torch = pytest.importorskip("torch")
    sw, sh = geom[:2]
    pitch = conventional_pitch(sw)
    assert pitch > row_bytes(sw) and pitch % 128 == 0
    check_call(torch, gpu_pkg, "v210", "YUV422PS", geom, 3, pitch=pitch, fs=pitch * sh)


@pytest.mark.parametrize("kind,name,geom", [("packed10", "YUV444PS", WORDS_SHORT), ("v210", "YUV422PS", V210_SHORT)], ids=["words", "v210"])
def test_misaligned_or_short_rows_are_refused_and_nothing_is_written(gpu_pkg, kind, name, geom):
    """Base, pitch, frame stride at 2 mod 4 and a pitch 4 bytes short of the row: INVALID_ARG with a message of its own, the
    destination byte for byte as it was, and jinc_debug_last_call still names the call made before."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = geom
    n = 3
    marker = gpu_pkg.Filter(gpu_pkg.FORMATS["Y8"], 64, 48, 96, 72, device=0, tap=3)   # a call nothing below could be mistaken for
    run_planar(torch, marker, [[np.zeros((48, 64), np.uint8)]] * 2, 2)
    marker.close()
    before = gpu_pkg.last_call()
    assert before[1] == 2
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    src = make_source(torch, f, kind, values(gpu_pkg, name, sw, sh, 10, n), n)
    dst = Side(torch, f.out_dims(), f.fmt.dtype, planar(3), n, seed=62).upload()
    s = torch.cuda.current_stream()
    ptr, pitch, fs = src.ptrs()[0], src.pitches()[0], src.strides()[0]
    row = 4 * sw if kind == "packed10" else row_bytes(sw)
    messages = set()
    for p, pi, st in ((ptr + 2, pitch, fs), (ptr, pitch + 2, fs), (ptr, pitch, fs + 2), (ptr, row - 4, fs)):
        with pytest.raises(gpu_pkg.JincError) as e:
            if kind == "packed10":
                f.process_device_widened_packed10(p, pi, Y410, st, dst.ptrs(), dst.pitches(), dst.steps(), dst.strides(), n, stream=s.cuda_stream)
            else:
                f.process_device_widened_v210(p, pi, st, dst.ptrs(), dst.pitches(), dst.steps(), dst.strides(), n, stream=s.cuda_stream)
        assert e.value.code == INVALID_ARG and str(e.value).startswith("JincResize:"), str(e.value)
        messages.add(str(e.value))
    print(sorted(messages))
    assert len(messages) == 4   # alignment of the base, of the pitch, of the frame stride; the short pitch
    torch.cuda.synchronize()
    assert gpu_pkg.last_call() == before, (before, gpu_pkg.last_call())
    image = dst.download()
    for b, B in dst.bufs.items():
        assert np.array_equal(image[b], B["host"]), "a refused call wrote to the destination"
    f.close()


# ---- 6. slices ---------------------------------------------------------------------------------------------------------------------------------

# Stand-ins per frame, fp32 rows padded to 256 bytes.  Words: 3 planes of 261 x 4 = 1044 -> 1280 bytes x 21 rows.  v210: luma
# 386 x 4 = 1544 -> 1792 bytes, each chroma plane 193 x 4 = 772 -> 1024 bytes, x 9 rows.
SLICES = [("packed10", "YUV444PS", WORDS_WIDE, 3 * 1280 * 21), ("v210", "YUV422PS", V210_WIDE, 9 * (1792 + 2 * 1024))]


@pytest.mark.parametrize("kind,name,geom,per_frame", SLICES, ids=["words", "v210"])
def test_a_call_beyond_the_scratch_cap_runs_in_slices(gpu_pkg, kind, name, geom, per_frame):
    """strided_scratch_bytes = two frames' stand-ins: 5 frames run as 2 + 2 + 1 with one widening launch each, the scratch the call
    reports is exactly the two frames' derived size, and every frame equals its single-frame call."""
    torch = pytest.importorskip("torch")
    with gpu_pkg.knobs(strided_scratch_bytes=2 * per_frame):
        got, vals, report = check_call(torch, gpu_pkg, kind, name, geom, 5, expect_report=(3, 0, 3))
    assert report[3] == 2 * per_frame, (report, per_frame)
    sw, sh, tw, th = geom
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    s = torch.cuda.current_stream()
    for k in range(5):
        src = make_source(torch, f, kind, vals[k:k + 1], 1)
        dst = Side(torch, f.out_dims(), f.fmt.dtype, planar(3), 1, seed=12).upload()
        call(f, kind, src, dst, 1, s)
        s.synchronize()
        assert f.last_strided()[:3] == (1, 0, 1)
        assert_bits_equal([got[k]], dst.frames_and_guards(f"frame {k} alone"), f.out_dims(), f"frame {k} of the sliced call against its single-frame call")
    f.close()


# ---- 7. streams, and other calls in between ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,name,geom", [("packed10", "YUV444PS", WORDS_WIDE), ("v210", "YUV422PS", V210_WIDE)], ids=["words", "v210"])
def test_two_calls_back_to_back_on_two_streams(gpu_pkg, kind, name, geom):
    """One filter, two calls on different frames queued without a synchronise in between on two streams: they share the stand-ins, so
    the second call's widening waits for the first call's kernels."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = geom
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    vals = values(gpu_pkg, name, sw, sh, 10, 6, seed=8)
    sides = [(make_source(torch, f, kind, vals[3 * c:3 * c + 3], 3, seed=21 + c), Side(torch, f.out_dims(), f.fmt.dtype, planar(3), 3, seed=31 + c).upload())
             for c in range(2)]
    torch.cuda.synchronize()   # (the uploads are done before the side streams start)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for c, (src, dst) in enumerate(sides):
        call(f, kind, src, dst, 3, streams[c])
    torch.cuda.synchronize()
    want = run_planar(torch, f, [[p.astype(np.float32) for p in planes] for planes in vals], 6)
    for c, (src, dst) in enumerate(sides):
        assert_bits_equal(dst.frames_and_guards(f"call {c}"), want[3 * c:3 * c + 3], f.out_dims(), f"call {c} of two streams")
    f.close()


def test_words_and_widened_calls_alternate_on_one_filter(gpu_pkg):
    """Y410 words, an 8-bit NV12-style source through jinc_filter_process_device_widened (Y dense, U and V interleaved at step 2),
    Y410 words again, on one stream of one YUV444PS filter without a synchronise in between: the three share the scratch."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = WORDS_WIDE
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YUV444PS"], sw, sh, tw, th, device=0, **KW)
    vals = values(gpu_pkg, "YUV444PS", sw, sh, 10, 2, seed=9) + values(gpu_pkg, "YUV444PS", sw, sh, 8, 2, seed=9) + values(gpu_pkg, "YUV444PS", sw, sh, 10, 2, seed=10)
    want = run_planar(torch, f, [[p.astype(np.float32) for p in planes] for planes in vals], 6)
    a = (make_source(torch, f, "packed10", vals[0:2], 2, seed=41), Side(torch, f.out_dims(), np.float32, planar(3), 2, seed=51).upload())
    b = make_widened_sides(torch, f, raw_of(vals[2:4], 8, [0] * 3), semi_planar(), planar(3), 2, seeds=(42, 52))
    c = (make_source(torch, f, "packed10", vals[4:6], 2, seed=43), Side(torch, f.out_dims(), np.float32, planar(3), 2, seed=53).upload())
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    call(f, "packed10", a[0], a[1], 2, s)
    assert f.last_strided()[:3] == (1, 0, 1)
    call_widened(f, b[0], b[1], None, 8, 2, s)
    assert f.last_strided()[:3] == (2, 0, 1)
    call(f, "packed10", c[0], c[1], 2, s)
    assert f.last_strided()[:3] == (1, 0, 1)
    s.synchronize()
    for k0, dst, what in ((0, a[1], "first words call"), (2, b[1], "widened call in between"), (4, c[1], "second words call")):
        assert_bits_equal(dst.frames_and_guards(what), want[k0:k0 + 2], f.out_dims(), what)
    f.close()


# ---- 8. finite flags ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,name,offsets", [("packed10", "RGBPS", R10G10B10A2), ("v210", "YUV422PS", None)], ids=["words", "v210"])
def test_every_frame_is_reported_finite(gpu_pkg, kind, name, offsets):
    """The calls keep the float filter's finite scan (they run enqueue as any float call does) and the scan finds nothing.
    150 x 70 -> 300 x 140 with float_trim_min_taps = 0, the shape at which test_widened.py sees every plane of a float RGB filter take
    the flagged path: wherever the flagged path runs, every frame's flag is 0 -- on every plane of the RGB filter, and at least on
    the luma plane of the 4:2:2 one."""
    torch = pytest.importorskip("torch")
    geom = (150, 70, 300, 140)
    n = 3
    with gpu_pkg.knobs(float_trim_min_taps=0):
        f = gpu_pkg.Filter(gpu_pkg.FORMATS[name], *geom, device=0, **KW)
        assert 0 < f.periodic_support(0) < f.plan_info(0).filter_size
        vals = values(gpu_pkg, name, geom[0], geom[1], 10, n)
        src = make_source(torch, f, kind, vals, n, offsets)
        dst = Side(torch, f.out_dims(), f.fmt.dtype, planar(3), n, seed=12).upload()
        s = torch.cuda.current_stream()
        call(f, kind, src, dst, n, s, offsets)
        s.synchronize()
        assert f.last_strided()[:3] == (1, 0, 1)
        flagged = []
        for i in range(3):
            flags = f.last_finite_flags(i)
            print(f"plane {i} flags {None if flags is None else flags.tolist()}")
            if flags is not None:
                flagged.append(i)
                assert flags.tolist() == [0] * n, (i, flags.tolist())
        assert flagged == [0, 1, 2] if kind == "packed10" else 0 in flagged, flagged
        want = run_planar(torch, f, [[p.astype(np.float32) for p in planes] for planes in vals], n)
        assert_bits_equal(dst.frames_and_guards("trimmed support"), want, f.out_dims(), "on the trimmed support")
        f.close()


# ---- 9. other plans ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,name,geom", [("packed10", "RGBPS", (150, 100, 206, 137)), ("v210", "YUV422PH", (300, 200, 150, 100))],
                         ids=["words_150x100_to_206x137", "v210_300x200_to_150x100"])
def test_other_plans_behind_the_pass(gpu_pkg, kind, name, geom):
    """Whatever arithmetic kernels the rules choose run on the stand-ins: not only the 2x tap-3 family."""
    torch = pytest.importorskip("torch")
    check_call(torch, gpu_pkg, kind, name, geom, 2, R10G10B10A2)
