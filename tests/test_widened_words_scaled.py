"""jinc_filter_process_device_widened_packed10_scaled / _widened_v210_scaled on the device: Y410 / RGB10A2 words and v210 blocks into
fp32, binary16 and bfloat16 filters with a scale and an offset per plane.  The result must be, bit for bit, what
jinc_filter_process_device computes on the same filter for dense planes holding s = fl32(fl32(float(v) * scale) + offset), narrowed
per type -- built on the host with numpy (test_scaled_host.widened_definition).  Every call takes three DIFFERENT pairs, one of them
with a negative scale: jinc_code_range gives Cb and Cr the same pair, with which a swap of planes 1 and 2 in the even / odd lane of
the v210 pass would not show.  Sources, destinations and their guards are test_widened_words.py's; the hooks
(jinc_debug_widen_fields / _widen_v210) put every code value through the real kernels at every field position."""
import numpy as np
import pytest

from test_packed10 import BGRX1010102, R10G10B10A2, Y410
from test_scaled import dense_planes, fused_fp32, kind_of
from test_scaled_host import BF16, HALF, widened_definition
from test_strided import Side, packed, planar, run_planar, semi_planar
from test_widened import assert_bits_equal, values
from test_widened_words import V210_MID, V210_NARROW, V210_WIDE, WORDS_NARROW, WORDS_SHORT, WORDS_WIDE, make_source
from test_widened_words import call as call_unscaled
from test_widened_words_host import V210_FIELDS

pytestmark = pytest.mark.gpu

KW = dict(tap=3)
RGB = packed("RGB", 3, 3)
# Three different pairs per call (Y / G, U / B / Cb, V / R / Cr): limited-range 10-bit luma, a NEGATIVE scale, limited-range chroma.
SCALES = [1.0 / 876.0, -1.0 / 1023.0, 1.0 / 896.0]
OFFSETS = [-64.0 / 876.0, 1.0, -512.0 / 896.0]


def call(f, kind, src, dst, n, stream, scales, offsets, field_offsets=Y410):
    if kind == "packed10":
        f.process_device_widened_packed10_scaled(src.ptrs()[0], src.pitches()[0], field_offsets, scales, offsets, src.strides()[0], dst.ptrs(),
                                                 dst.pitches(), dst.steps(), dst.strides(), n, stream=stream.cuda_stream)
    else:
        f.process_device_widened_v210_scaled(src.ptrs()[0], src.pitches()[0], scales, offsets, src.strides()[0], dst.ptrs(), dst.pitches(),
                                             dst.steps(), dst.strides(), n, stream=stream.cuda_stream)


_PLANAR = {}


def planar_reference(torch, f, key, vals, scales, offsets, n):
    """jinc_filter_process_device on numpy's planes of the definition: once per case."""
    if key not in _PLANAR:
        _PLANAR[key] = run_planar(torch, f, dense_planes(f.fmt, vals, scales, offsets), n)
    return _PLANAR[key]


def check_call(torch, pkg, kind, name, geom, n, field_offsets=Y410, dst_layout=None, expect_report=(1, 0, 1), scales=SCALES, offsets=OFFSETS,
               seed=7, **src_kw):
    """One scaled call against the planar call on the same filter; returns (the call's output frames, the values)."""
    sw, sh, tw, th = geom
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    vals = values(pkg, name, sw, sh, 10, n, seed=seed)
    what = f"{kind} {field_offsets if kind == 'packed10' else ''} -> {name} {sw}x{sh}->{tw}x{th} {n} frame(s) scaled {src_kw}"
    src = make_source(torch, f, kind, vals, n, field_offsets, **src_kw)   # (pseudo-random bits wherever no sample lies)
    dst = Side(torch, f.out_dims(), f.fmt.dtype, dst_layout or planar(3), n, seed=12).upload()
    s = torch.cuda.current_stream()
    call(f, kind, src, dst, n, s, scales, offsets, field_offsets)
    s.synchronize()
    report = f.last_strided()
    groups = pkg.last_groups()
    print(f"{what}: last_strided {report}, last_groups {groups}")
    got = dst.frames_and_guards(what)   # (the guards around the destination are checked there)
    assert np.array_equal(src.download(), src.host), f"{what}: the source was written"
    assert report[:3] == expect_report, report
    widen = groups[0]
    assert (widen["direction"], widen["scaled"], widen["sample_type"]) == (6 if kind == "packed10" else 9, 1, f.fmt.sample_type), widen
    assert (widen["width"], widen["rows"], widen["sample_bytes"]) == (sw, sh, f.fmt.sample_bytes), widen
    sc = scales or [1.0] * 3
    of = offsets or [0.0] * 3
    key = (kind, name, geom, n, seed, tuple(sc), tuple(of))
    assert_bits_equal(got, planar_reference(torch, f, key, vals, sc, of, n), f.out_dims(), what + " against the planar call on numpy's planes")
    f.close()
    return got, vals


# ---- 1. against the planar call ---------------------------------------------------------------------------------------------------------

WORDS_CASES = [("y410_f32", "YUV444PS", Y410, None, (1, 0, 1)), ("y410_f16", "YUV444PH", Y410, None, (1, 0, 1)),
               ("y410_bf16", "YUV444PBF", Y410, None, (1, 0, 1)), ("r10g10b10a2_f32", "RGBPS", R10G10B10A2, None, (1, 0, 1)),
               ("r10g10b10a2_bf16", "RGBPBF", R10G10B10A2, None, (1, 0, 1)), ("bgrx1010102_f32_rgb", "RGBPS", BGRX1010102, RGB, (1, 1, 1))]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("geom", [WORDS_WIDE, WORDS_SHORT, WORDS_NARROW], ids=["261x21", "20x12", "7x7"])
@pytest.mark.parametrize("case", WORDS_CASES, ids=[c[0] for c in WORDS_CASES])
def test_words_equal_the_planar_call_on_scaled_planes(gpu_pkg, case, geom, n):
    torch = pytest.importorskip("torch")
    _, name, field_offsets, dst_layout, report = case
    check_call(torch, gpu_pkg, "packed10", name, geom, n, field_offsets, dst_layout, expect_report=report)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("geom", [V210_WIDE, V210_MID, V210_NARROW], ids=["386x9", "22x8", "14x7"])
@pytest.mark.parametrize("name", ["YUV422PS", "YUV422PH", "YUV422PBF"])
def test_v210_equals_the_planar_call_on_scaled_planes(gpu_pkg, name, geom, n):
    torch = pytest.importorskip("torch")
    check_call(torch, gpu_pkg, "v210", name, geom, n)


@pytest.mark.parametrize("kind,name,geom", [("packed10", "YUV444PS", WORDS_WIDE), ("packed10", "YUV444PBF", WORDS_SHORT), ("v210", "YUV422PS", V210_WIDE),
                                            ("v210", "YUV422PH", V210_MID)], ids=["words_f32", "words_bf16", "v210_f32", "v210_f16"])
def test_dword_only_source_alignment(gpu_pkg, kind, name, geom):
    """Source base, pitch and frame stride multiples of 4 only: dwords on the word / block side (16: the cases above)."""
    torch = pytest.importorskip("torch")
    check_call(torch, gpu_pkg, kind, name, geom, 3, align=4)
    widen = gpu_pkg.last_groups()[0]
    vec = geom[0] // 8 * 8 if kind == "packed10" else 6 * (geom[0] // 6 // 2 * 2)
    assert (widen["unit"], widen["vec_pixels"]) == (4, vec), widen


def test_scale_alone_and_offset_alone(gpu_pkg):
    """A NULL scale array means 1.0, a NULL offset array 0.0."""
    torch = pytest.importorskip("torch")
    check_call(torch, gpu_pkg, "packed10", "YUV444PH", WORDS_SHORT, 1, scales=SCALES, offsets=None)
    check_call(torch, gpu_pkg, "v210", "YUV422PS", V210_MID, 1, scales=None, offsets=OFFSETS)


# ---- 2. a second trip of the wave --------------------------------------------------------------------------------------------------------

def test_word_rows_longer_than_one_trip_of_the_wave(gpu_pkg):
    """1030 words a row: two whole trips of 64 lanes x 8 pixels and a tail of 6."""
    torch = pytest.importorskip("torch")
    check_call(torch, gpu_pkg, "packed10", "YUV444PS", (1030, 8, 2060, 16), 1)
    widen = gpu_pkg.last_groups()[0]
    assert (widen["unit"], widen["vec_pixels"], widen["width"]) == (16, 1024, 1030), widen


def test_v210_rows_longer_than_one_trip_of_the_wave(gpu_pkg):
    """782 pixels a row: 130 whole blocks and a 2-pixel partial one, so lanes 0 and 1 make a second trip of the paired loop, DPP
    exchange included."""
    torch = pytest.importorskip("torch")
    check_call(torch, gpu_pkg, "v210", "YUV422PS", (782, 7, 1564, 14), 2)
    widen = gpu_pkg.last_groups()[0]
    assert (widen["direction"], widen["unit"], widen["vec_pixels"], widen["width"]) == (9, 16, 780, 782) and widen["vec_pixels"] > 6 * 128


# ---- 3. every code value through the hooks ---------------------------------------------------------------------------------------------------

OUT_KINDS = [("f32", 0), ("f16", HALF), ("bf16", BF16)]


def code_pairs(pkg):
    """(name, (scale, offset)): limited-range luma, limited-range chroma and full-range chroma of jinc_code_range(10, ...)."""
    return [("limited_luma", pkg.code_range(10, pkg.RANGE_LIMITED, pkg.PLANE_LUMA_OR_RGB)[:2]),
            ("limited_chroma", pkg.code_range(10, pkg.RANGE_LIMITED, pkg.PLANE_CHROMA)[:2]),
            ("full_chroma", pkg.code_range(10, pkg.RANGE_FULL, pkg.PLANE_CHROMA)[:2])]


def out_kind_of(pkg, kind):
    return {0: pkg.SAMPLE_DEFAULT, HALF: pkg.SAMPLE_FLOAT16, BF16: pkg.SAMPLE_BFLOAT16}[kind]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint16)


def words_with_codes(field_offsets, plane):
    """1024 + 5 words (whole lanes of 8 and a tail): field `plane` counts through every code, the other bits are pseudo-random."""
    rng = np.random.default_rng(100 + plane)
    codes = np.arange(1029, dtype=np.uint32) % 1024
    junk = rng.integers(0, 1 << 32, codes.size, dtype=np.uint64).astype(np.uint32)
    o = np.uint32(field_offsets[plane])
    return (junk & ~(np.uint32(1023) << o)) | (codes << o)


def blocks_with_codes(field):
    """A row of 2 x 1024 + 2 blocks -- pairs, the odd whole block and, with width = 6 x 2049 + 4, a partial one: field `field` of
    every block counts through the codes, every other bit is pseudo-random.  Returns (words, width)."""
    nblocks = 2050
    rng = np.random.default_rng(200 + field)
    words = rng.integers(0, 1 << 32, (nblocks, 4), dtype=np.uint64).astype(np.uint32)
    _, _, word, offset = V210_FIELDS[field]
    codes = (np.arange(nblocks, dtype=np.uint32) // 2) % 1024
    words[:, word] = (words[:, word] & ~(np.uint32(1023) << np.uint32(offset))) | (codes << np.uint32(offset))
    return words, 6 * (nblocks - 1) + 4


def v210_values(words, width):
    nblocks = words.shape[0]
    widths = (width, width // 2, width // 2)
    vals = [np.zeros(w, np.uint32) for w in widths]
    for plane, j, word, offset in V210_FIELDS:
        x = (6 if plane == 0 else 3) * np.arange(nblocks) + j
        valid = x < widths[plane]
        vals[plane][x[valid]] = (words[valid, word] >> np.uint32(offset)) & np.uint32(1023)
    return vals


@pytest.mark.parametrize("out,kind", OUT_KINDS, ids=[k[0] for k in OUT_KINDS])
def test_every_code_at_every_field_position_of_a_word(gpu_pkg, out, kind):
    """All 1024 codes at each of the three field positions, with each of the three pairs in each plane, against numpy bit for bit.
    In fp32 a fused multiply-add differs from the definition on hundreds of the 1024 codes for each of these pairs, so the fp32
    case catches contraction."""
    named = code_pairs(gpu_pkg)
    for rot in range(3):   # every pair visits every plane
        pairs = [named[(c + rot) % 3][1] for c in range(3)]
        scales, offsets = [p[0] for p in pairs], [p[1] for p in pairs]
        for field_offsets in (Y410, BGRX1010102):
            for plane in range(3):
                words = words_with_codes(field_offsets, plane)
                got = gpu_pkg.debug_widen_fields(words, field_offsets, scales, offsets, out_kind_of(gpu_pkg, kind))
                for c in range(3):
                    v = (words >> np.uint32(field_offsets[c])) & np.uint32(1023)
                    want = widened_definition(v, scales[c], offsets[c], kind)
                    assert np.array_equal(bits(got[c]), want), (out, rot, field_offsets, plane, c, int((bits(got[c]) != want).sum()))
                assert set(((words >> np.uint32(field_offsets[plane])) & np.uint32(1023)).tolist()) == set(range(1024))
    if kind == 0:
        codes = np.arange(1024, dtype=np.uint32)
        for name, (s, o) in named:
            differ = int((widened_definition(codes, s, o, 0) != fused_fp32(codes, s, o).view(np.uint32)).sum())
            print(f"{name}: a fused multiply-add differs on {differ} of 1024 codes")
            assert differ >= 400, (name, differ)


@pytest.mark.parametrize("out,kind", OUT_KINDS, ids=[k[0] for k in OUT_KINDS])
def test_every_code_at_every_field_of_a_block(gpu_pkg, out, kind):
    """All 1024 codes at each of the twelve fields of a block -- in even and odd blocks, pairs and tails -- with every pair in every
    plane, against numpy bit for bit."""
    named = code_pairs(gpu_pkg)
    for field in range(12):
        rot = field % 3
        pairs = [named[(c + rot) % 3][1] for c in range(3)]
        scales, offsets = [p[0] for p in pairs], [p[1] for p in pairs]
        words, width = blocks_with_codes(field)
        got = gpu_pkg.debug_widen_v210(words.ravel(), width, scales, offsets, out_kind_of(gpu_pkg, kind))
        vals = v210_values(words, width)
        for c in range(3):
            want = widened_definition(vals[c], scales[c], offsets[c], kind)
            assert np.array_equal(bits(got[c]), want), (out, field, c, int((bits(got[c]) != want).sum()))


def test_the_hooks_with_null_arrays_run_the_unscaled_form(gpu_pkg):
    words = words_with_codes(Y410, 0)
    blocks, width = blocks_with_codes(1)
    for kind, dtype in ((0, np.float32), (HALF, np.float16)):
        got = gpu_pkg.debug_widen_fields(words, Y410, None, None, out_kind_of(gpu_pkg, kind))
        for c in range(3):
            assert np.array_equal(got[c], ((words >> np.uint32(Y410[c])) & np.uint32(1023)).astype(dtype))
        got = gpu_pkg.debug_widen_v210(blocks.ravel(), width, None, None, out_kind_of(gpu_pkg, kind))
        for c, v in enumerate(v210_values(blocks, width)):
            assert np.array_equal(got[c], v.astype(dtype))


# ---- 4. the identity pair ------------------------------------------------------------------------------------------------------------------

def unscaled_result(torch, pkg, kind, name, geom, n, field_offsets=Y410, seed=7):
    sw, sh, tw, th = geom
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    vals = values(pkg, name, sw, sh, 10, n, seed=seed)
    src = make_source(torch, f, kind, vals, n, field_offsets)
    dst = Side(torch, f.out_dims(), f.fmt.dtype, planar(3), n, seed=12).upload()
    s = torch.cuda.current_stream()
    call_unscaled(f, kind, src, dst, n, s, field_offsets)
    s.synchronize()
    out = dst.frames_and_guards("unscaled call"), f.last_strided(), pkg.last_groups(), f.out_dims()
    f.close()
    return out


@pytest.mark.parametrize("kind,name,geom", [("packed10", "YUV444PS", WORDS_SHORT), ("packed10", "YUV444PH", WORDS_SHORT), ("v210", "YUV422PS", V210_MID),
                                            ("v210", "YUV422PH", V210_MID)], ids=["words_f32", "words_f16", "v210_f32", "v210_f16"])
def test_identity_arrays_give_the_unscaled_output(gpu_pkg, kind, name, geom):
    """Scale 1.0 and offset 0.0 given as arrays: the scaled form runs (scaled 1 in the record) and stores the unscaled call's bits."""
    torch = pytest.importorskip("torch")
    got, _ = check_call(torch, gpu_pkg, kind, name, geom, 2, scales=[1.0] * 3, offsets=[0.0] * 3)
    want, _, _, dims = unscaled_result(torch, gpu_pkg, kind, name, geom, 2)
    assert_bits_equal(got, want, dims, "identity arrays against the unscaled call")


# ---- 5. the way back, fp32 ----------------------------------------------------------------------------------------------------------------------

def test_every_code_comes_back_through_widen_and_narrow_in_fp32(gpu_pkg):
    """Widen with the to_float pair, narrow with the to_code pair: every one of the 1024 codes is returned, for full and limited range,
    luma and chroma -- through the real kernels on both ways.  (Not claimed for the 16-bit types.)"""
    pkg = gpu_pkg
    ranges = [pkg.code_range(10, r, k) for r in (pkg.RANGE_FULL, pkg.RANGE_LIMITED) for k in (pkg.PLANE_LUMA_OR_RGB, pkg.PLANE_CHROMA)]
    codes = np.arange(1029, dtype=np.uint32) % 1024
    for trio in ([0, 1, 2], [3, 2, 1], [1, 3, 0]):   # every range in some plane, different pairs within a call
        to_float = ([ranges[i][0] for i in trio], [ranges[i][1] for i in trio])
        to_code = ([ranges[i][2] for i in trio], [ranges[i][3] for i in trio])
        words = (codes << np.uint32(Y410[0])) | (((codes * 7 + 3) % 1024) << np.uint32(Y410[1])) | (((1023 - codes) % 1024) << np.uint32(Y410[2]))
        planes = pkg.debug_widen_fields(words, Y410, *to_float)
        back = pkg.debug_narrow_fields(planes, Y410, 0, *to_code)
        misses = int((back != words).sum())
        print(f"words, ranges {trio}: {misses} misses")
        assert misses == 0
        nblocks = 344   # 2064 luma samples: every code twice in luma, once in each chroma plane
        width = 6 * nblocks
        luma, chroma = np.arange(width, dtype=np.uint32) % 1024, np.arange(width // 2, dtype=np.uint32) % 1024
        blocks = pkg.debug_narrow_v210([luma.astype(np.float32), chroma.astype(np.float32), (1023 - chroma).astype(np.float32)])
        planes = pkg.debug_widen_v210(blocks, width, *to_float)
        back = pkg.debug_narrow_v210(planes, *to_code)
        misses = int((back != blocks).sum())
        print(f"blocks, ranges {trio}: {misses} misses")
        assert misses == 0


# ---- 6. both arrays NULL ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,name,geom", [("packed10", "YUV444PS", WORDS_WIDE), ("packed10", "RGBPH", WORDS_SHORT), ("v210", "YUV422PS", V210_WIDE),
                                            ("v210", "YUV422PH", V210_MID)], ids=["words_f32", "words_f16", "v210_f32", "v210_f16"])
def test_null_arrays_are_the_unscaled_call(gpu_pkg, kind, name, geom):
    """The same output and the same reports as process_device_widened_packed10 / _v210 -- scaled 0 in the record."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = geom
    n = 2
    want, want_report, want_groups, dims = unscaled_result(torch, gpu_pkg, kind, name, geom, n, R10G10B10A2)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    src = make_source(torch, f, kind, values(gpu_pkg, name, sw, sh, 10, n), n, R10G10B10A2)
    dst = Side(torch, f.out_dims(), f.fmt.dtype, planar(3), n, seed=12).upload()
    s = torch.cuda.current_stream()
    call(f, kind, src, dst, n, s, None, None, R10G10B10A2)
    s.synchronize()
    assert f.last_strided() == want_report and gpu_pkg.last_groups() == want_groups, (f.last_strided(), gpu_pkg.last_groups())
    assert want_groups[0]["scaled"] == 0
    assert_bits_equal(dst.frames_and_guards("NULL arrays"), want, dims, "NULL arrays against the unscaled call")
    f.close()


@pytest.mark.parametrize("kind,name,geom", [("packed10", "YUV444PBF", WORDS_SHORT), ("v210", "YUV422PBF", V210_MID)], ids=["words", "v210"])
def test_refused_calls_leave_the_records_and_the_destination(gpu_pkg, kind, name, geom):
    """bfloat16 with NULL arrays (the unscaled call's refusal) and a bad pair: INVALID_ARG, both debug records as the call before left
    them, no destination byte written."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = geom
    check_call(torch, gpu_pkg, kind, name, geom, 1)
    before = (gpu_pkg.last_strided(), gpu_pkg.last_groups())
    assert before[0][:3] == (1, 0, 1) and len(before[1]) == 1
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    src = make_source(torch, f, kind, values(gpu_pkg, name, sw, sh, 10, 1), 1)
    dst = Side(torch, f.out_dims(), f.fmt.dtype, planar(3), 1, seed=62).upload()
    s = torch.cuda.current_stream()
    for scales, offsets, says in ((None, None, "bfloat16"), ([1.0, float("nan"), 1.0], None, "plane 1 is NaN"), (None, [0.0, 0.0, float("inf")], "plane 2 is infinite")):
        with pytest.raises(gpu_pkg.JincError) as e:
            call(f, kind, src, dst, 1, s, scales, offsets)
        assert e.value.code == -1 and says in str(e.value), str(e.value)
        assert (gpu_pkg.last_strided(), gpu_pkg.last_groups()) == before
    torch.cuda.synchronize()
    image = dst.download()
    for b, B in dst.bufs.items():
        assert np.array_equal(image[b], B["host"]), "a refused call wrote to the destination"
    f.close()


# ---- 7. alternation on one filter ---------------------------------------------------------------------------------------------------------------

def test_scaled_words_strided_and_unscaled_words_calls_alternate_on_one_filter(gpu_pkg):
    """A scaled words call, a strided call (float planes, U and V interleaved) and an unscaled words call in turn on one stream of one
    YUV444PS filter without a synchronise in between: the three share the scratch; each equals its stand-alone result."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = WORDS_WIDE
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YUV444PS"], sw, sh, tw, th, device=0, **KW)
    vals = values(gpu_pkg, "YUV444PS", sw, sh, 10, 6, seed=9)
    floats = [[p.astype(np.float32) for p in planes] for planes in vals]
    want_scaled = run_planar(torch, f, dense_planes(f.fmt, vals[0:2], SCALES, OFFSETS), 2)
    want_plain = run_planar(torch, f, floats[2:6], 4)
    a = (make_source(torch, f, "packed10", vals[0:2], 2, seed=41), Side(torch, f.out_dims(), np.float32, planar(3), 2, seed=51).upload())
    b_src = Side(torch, f.fmt.plane_dims(sw, sh), np.float32, semi_planar(), 2, seed=42).fill(floats[2:4]).upload()
    b_dst = Side(torch, f.out_dims(), np.float32, semi_planar(), 2, seed=52).upload()
    c = (make_source(torch, f, "packed10", vals[4:6], 2, seed=43), Side(torch, f.out_dims(), np.float32, planar(3), 2, seed=53).upload())
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    call(f, "packed10", a[0], a[1], 2, s, SCALES, OFFSETS)
    assert f.last_strided()[:3] == (1, 0, 1) and gpu_pkg.last_groups()[0]["scaled"] == 1
    f.process_device_strided(b_src.ptrs(), b_src.pitches(), b_src.steps(), b_src.strides(), b_dst.ptrs(), b_dst.pitches(), b_dst.steps(), b_dst.strides(), 2,
                             stream=s.cuda_stream)
    assert f.last_strided()[:3] == (1, 1, 1)
    call_unscaled(f, "packed10", c[0], c[1], 2, s)
    assert f.last_strided()[:3] == (1, 0, 1) and gpu_pkg.last_groups()[0]["scaled"] == 0
    s.synchronize()
    assert_bits_equal(a[1].frames_and_guards("scaled words call"), want_scaled, f.out_dims(), "scaled words call")
    assert_bits_equal(b_dst.frames_and_guards("strided call in between"), want_plain[0:2], f.out_dims(), "strided call in between")
    assert_bits_equal(c[1].frames_and_guards("unscaled words call"), want_plain[2:4], f.out_dims(), "unscaled words call")
    f.close()
