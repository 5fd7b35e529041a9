"""jinc_filter_process_device_widened_scaled / _narrowed_scaled on the device: a scale and an offset between code values and the float
range, applied in the widening and the narrowing pass.  Expected values never come from the call under test:
  widened   numpy builds the dense planes from the raw samples under the definition, s = fl32(fl32(float(v) * scale) + offset),
            narrowed round-to-nearest-even for binary16 and bfloat16 planes; jinc_filter_process_device on those planes is the
            expected result, compared bit for bit;
  narrowed  the planar call's result, scaled, offset and narrowed by numpy, rint(clip(fl32(fl32(r * scale) + offset), 0, peak)) << shift,
            compared bit for bit.
Every destination lies inside a larger buffer of pseudo-random bytes whose other bytes must keep their value, the source must come
back unchanged, and jinc_debug_last_strided must report what the unscaled call reports.  The shape is the sibling files' 262 x 38 ->
524 x 76 at tap 3, 2 frames (test_widened.py argues for it).
An FMA in place of multiply-then-add must show: the limited-range cases assert that a fused computation (emulated in float64,
rounded once) differs from the definition at 10 % of their own source samples or more, and a separate test sends values whose STORED
integer differs between the two computations through the narrowing pass."""
import numpy as np
import pytest

import test_narrowed as TN
import test_widened as TW
from test_scaled_host import BF16, HALF, bf16_rne, narrowed_definition, widened_definition
from test_shifted import Y210
from test_strided import Side, packed, planar, run_planar, semi_planar
from test_widened import assert_bits_equal, assert_source_unchanged, raw_of, values

pytestmark = pytest.mark.gpu

GEOM = (262, 38, 524, 76)
KW = dict(tap=3)
N = 2
BGRA = packed("BGRA", 4, 3)   # three components: the X / A byte of every pixel is no sample of the call


def kind_of(fmt):
    return BF16 if fmt.bfloat16 else HALF if fmt.half else 0


def pairs(pkg, bits, rng, planes, rgb=False, to_code=False):
    """(scales, offsets) of jinc_code_range for the planes of a YUV (luma, chroma, chroma) or RGB filter."""
    kinds = [pkg.PLANE_LUMA_OR_RGB if rgb or i == 0 or i == 3 else pkg.PLANE_CHROMA for i in range(planes)]
    got = [pkg.code_range(bits, rng, k) for k in kinds]
    return ([g[2] for g in got], [g[3] for g in got]) if to_code else ([g[0] for g in got], [g[1] for g in got])


def fused_fp32(v, scale, offset):
    """What an FMA gives: the exact product and sum (float64 holds both: 16 + 24 bits, then an addend of 24 bits), rounded ONCE."""
    return (v.astype(np.float64) * np.float64(np.float32(scale)) + np.float64(np.float32(offset))).astype(np.float32)


# ---- widened --------------------------------------------------------------------------------------------------------------------------------

def dense_planes(fmt, vals, scales, offsets):
    """The planes the definition says the filter reads, in the filter's dtype (bfloat16: uint16 bit patterns)."""
    kind = kind_of(fmt)
    return [[widened_definition(p.astype(np.uint32), s, o, kind).view(fmt.dtype) for p, s, o in zip(planes, scales, offsets)] for planes in vals]


def check_widened(torch, pkg, name, bits, shifts, scales, offsets, src_layout, dst_layout=None, report=None, fused_must_show=False,
                  unscaled_exists=True, **side_kw):
    sw, sh, tw, th = GEOM
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    planes = f.fmt.planes
    vals = values(pkg, name, sw, sh, bits, N)
    raw = raw_of(vals, bits, shifts or [0] * planes, dirty_seed=77 if bits not in (8, 16) else None)
    what = f"{bits}-bit {src_layout} -> {name} scaled {[float(s) for s in scales or []]} {[float(o) for o in offsets or []]}"
    src, dst = TW.make_sides(torch, f, raw, src_layout, dst_layout or planar(planes), N, **side_kw)
    s = torch.cuda.current_stream()
    f.process_device_widened_scaled(src.ptrs(), src.pitches(), src.steps(), shifts, bits, scales, offsets, src.strides(), dst.ptrs(),
                                    dst.pitches(), dst.steps(), dst.strides(), N, stream=s.cuda_stream)
    s.synchronize()
    got_report = f.last_strided()
    print(f"{what}: last_strided {got_report}, last_call {pkg.last_call()}")
    got = dst.frames_and_guards(what)
    assert_source_unchanged(src, what)
    assert got_report[:3] == report, got_report
    if unscaled_exists:   # the same launches, slices and scratch as the unscaled call on the same sides
        _, dst2 = TW.make_sides(torch, f, raw, src_layout, dst_layout or planar(planes), N, seeds=(11, 15), **side_kw)
        TW.call(f, src, dst2, shifts, bits, N, s)
        s.synchronize()
        assert f.last_strided() == got_report, (f.last_strided(), got_report)
    sc = scales or [1.0] * planes
    of = offsets or [0.0] * planes
    want = run_planar(torch, f, dense_planes(f.fmt, vals, sc, of), N)
    assert_bits_equal(got, want, f.out_dims(), what + " against the planar call on numpy's planes")
    if fused_must_show:
        for i in range(planes):
            v = np.concatenate([fr[i].ravel() for fr in vals]).astype(np.uint32)
            unfused = widened_definition(v, sc[i], of[i], 0)
            fused = fused_fp32(v, sc[i], of[i]).view(np.uint32)
            share = float((unfused != fused).mean())
            kind, note = kind_of(f.fmt), ""
            if kind:   # (most of the fp32 differences vanish in the 16-bit rounding: the fp32 cases are where every one is stored)
                fused16 = bf16_rne(fused.view(np.float32)) if kind == BF16 else fused.view(np.float32).astype(np.float16).view(np.uint16)
                note = f", the stored 16-bit samples at {100 * float((widened_definition(v, sc[i], of[i], kind) != fused16).mean()):.2f} %"
            print(f"plane {i}: fused and un-fused fp32 samples differ at {100 * share:.1f} % of {v.size} source samples{note}")
            assert share >= 0.10, (i, share)
    f.close()
    return got


def test_nv12_into_fp32_full_range(gpu_pkg):
    torch = pytest.importorskip("torch")
    sc, of = pairs(gpu_pkg, 8, gpu_pkg.RANGE_FULL, 3)
    check_widened(torch, gpu_pkg, "YUV420PS", 8, None, sc, of, semi_planar(), report=(2, 0, 1))


def test_p010_into_fp32_limited_range_is_not_fused(gpu_pkg):
    """fp32 planes hold the two roundings as they are: 39 % (luma) and 51 % (chroma) of all 10-bit values give other bits fused."""
    torch = pytest.importorskip("torch")
    sc, of = pairs(gpu_pkg, 10, gpu_pkg.RANGE_LIMITED, 3)
    check_widened(torch, gpu_pkg, "YUV420PS", 10, [6] * 3, sc, of, semi_planar(), report=(2, 0, 1), fused_must_show=True)


def test_nv12_into_fp32_limited_range_is_not_fused(gpu_pkg):
    torch = pytest.importorskip("torch")
    sc, of = pairs(gpu_pkg, 8, gpu_pkg.RANGE_LIMITED, 3)
    check_widened(torch, gpu_pkg, "YUV420PS", 8, None, sc, of, semi_planar(), report=(2, 0, 1), fused_must_show=True)


def test_p010_into_half_limited_range(gpu_pkg):
    """Luma and chroma with scale / offset pairs of their own."""
    torch = pytest.importorskip("torch")
    sc, of = pairs(gpu_pkg, 10, gpu_pkg.RANGE_LIMITED, 3)
    assert sc[0] != sc[1] and of[0] != of[1]
    check_widened(torch, gpu_pkg, "YUV420PH", 10, [6] * 3, sc, of, semi_planar(), report=(2, 0, 1), fused_must_show=True)


def test_p016_into_half_full_range(gpu_pkg):
    """16-bit words into binary16 planes -- refused unscaled.  v / 65535 below 2^-14 are binary16 subnormals, most others round."""
    torch = pytest.importorskip("torch")
    sc, of = pairs(gpu_pkg, 16, gpu_pkg.RANGE_FULL, 3)
    check_widened(torch, gpu_pkg, "YUV420PH", 16, None, sc, [0.0] * 3, semi_planar(), report=(2, 0, 1), unscaled_exists=False)
    v = np.unique(np.concatenate([p.ravel() for fr in values(gpu_pkg, "YUV420PH", 262, 38, 16, N) for p in fr])).astype(np.uint32)
    s = widened_definition(v, sc[0], 0.0, 0).view(np.float32)
    h = s.astype(np.float16)
    sub, rounded = int(((h != 0) & (h < np.float16(6.104e-5))).sum()), int((h.astype(np.float32) != s).sum())
    print(f"{sub} of {v.size} distinct source values are binary16 subnormals, {rounded} are rounded")
    assert sub > 0 and rounded > v.size // 2


def test_p010_into_bfloat16_limited_range(gpu_pkg):
    """10-bit words into bfloat16 planes -- refused unscaled."""
    torch = pytest.importorskip("torch")
    sc, of = pairs(gpu_pkg, 10, gpu_pkg.RANGE_LIMITED, 3)
    check_widened(torch, gpu_pkg, "YUV420PBF", 10, [6] * 3, sc, of, semi_planar(), report=(2, 0, 1), fused_must_show=True, unscaled_exists=False)


def test_bgra8_into_interleaved_float_rgb(gpu_pkg):
    torch = pytest.importorskip("torch")
    sc, of = pairs(gpu_pkg, 8, gpu_pkg.RANGE_FULL, 3, rgb=True)
    check_widened(torch, gpu_pkg, "RGBPS", 8, None, sc, of, BGRA, packed("RGB", 3, 3), report=(1, 1, 1))


def test_bgrx8_under_a_three_component_filter(gpu_pkg):
    """A channel missing: the pass reads whole pixels up to the last but one and the last pixel sample by sample; every plane with a
    pair of its own, so a pair that travelled with the wrong channel shows."""
    torch = pytest.importorskip("torch")
    check_widened(torch, gpu_pkg, "RGBPS", 8, None, [1 / 255.0, -1 / 219.0, 2.0], [0.0, 1.0, -16 / 219.0], BGRA, report=(1, 0, 1))


@pytest.mark.parametrize("name,bits,shifts", [("YUV420PS", 8, None), ("YUV420PH", 16, None), ("YUV420PBF", 10, [6] * 3)], ids=["nv12_f32", "p016_f16", "p010_bf16"])
def test_source_base_off_4_byte_alignment(gpu_pkg, name, bits, shifts):
    """Base, pitch and frame stride multiples of the sample size only: every sample moves through the sample-by-sample loop."""
    torch = pytest.importorskip("torch")
    sc, of = pairs(gpu_pkg, bits, gpu_pkg.RANGE_LIMITED, 3)
    check_widened(torch, gpu_pkg, name, bits, shifts, sc, of, semi_planar(), report=(2, 0, 1), unscaled_exists=name == "YUV420PS", src_align=1)


def test_scale_alone_and_offset_alone(gpu_pkg):
    """A NULL offset array means all 0.0, a NULL scale array all 1.0: the scaled form runs with either."""
    torch = pytest.importorskip("torch")
    check_widened(torch, gpu_pkg, "YUV420PS", 8, None, [1 / 219.0, 1 / 224.0, 1 / 224.0], None, semi_planar(), report=(2, 0, 1))
    check_widened(torch, gpu_pkg, "YUV420PS", 8, None, None, [-16.0, -128.0, -128.0], semi_planar(), report=(2, 0, 1))


# ---- narrowed -------------------------------------------------------------------------------------------------------------------------------

def normalised_sources(fmt, sw, sh, n, peak, scales, offsets, seed):
    """n frames whose code values span 0.15 peak below 0 to 0.15 peak above the peak, taken back into the float range."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        planes = []
        for i, (w, h) in enumerate(fmt.plane_dims(sw, sh)):
            code = rng.uniform(-0.15 * peak, 1.15 * peak, (h, w))
            v = ((code - float(offsets[i])) / float(scales[i])).astype(np.float32)
            planes.append(bf16_rne(v) if fmt.bfloat16 else v.astype(fmt.dtype))
        out.append(planes)
    return out


def check_narrowed(torch, pkg, name, bits, shifts, scales, offsets, dst_layout, report, seed=5):
    sw, sh, tw, th = GEOM
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    planes, peak = f.fmt.planes, (1 << bits) - 1
    frames = normalised_sources(f.fmt, sw, sh, N, peak, scales, offsets, seed)
    what = f"{name} -> {bits}-bit {dst_layout} shifts {shifts} scaled {[float(s) for s in scales]} {[float(o) for o in offsets]}"
    src, dst = TN.make_sides(torch, f, frames, planar(planes), dst_layout, bits, N)
    s = torch.cuda.current_stream()
    f.process_device_narrowed_scaled(src.ptrs(), src.pitches(), src.steps(), src.strides(), dst.ptrs(), dst.pitches(), dst.steps(), shifts, bits,
                                     scales, offsets, dst.strides(), N, stream=s.cuda_stream)
    s.synchronize()
    got_report = f.last_strided()
    print(f"{what}: last_strided {got_report}, last_call {pkg.last_call()}")
    got = dst.frames_and_guards(what)
    assert_source_unchanged(src, what)
    assert got_report[:3] == report, got_report
    _, dst2 = TN.make_sides(torch, f, frames, planar(planes), dst_layout, bits, N, seeds=(11, 16))
    TN.narrowed_call(f, src, dst2, shifts, bits, N, s)   # the same launches, slices and scratch as the unscaled call on the same sides
    s.synchronize()
    assert f.last_strided() == got_report, (f.last_strided(), got_report)
    r = run_planar(torch, f, frames, N)
    sft = shifts or [0] * planes
    want = [[(narrowed_definition(TN.widened(f.fmt, p), scales[i], offsets[i], peak) << sft[i]).astype(got[0][0].dtype) for i, p in enumerate(fr)] for fr in r]
    TN.assert_equal(got, want, f.out_dims(), what + " against the planar call scaled and narrowed by numpy")
    below = above = total = 0
    for fr in r:
        for i, p in enumerate(fr):
            w, h = f.out_dims()[i]
            with np.errstate(over="ignore"):
                t = (TN.widened(f.fmt, p)[:h, :w] * np.float32(scales[i]) + np.float32(offsets[i])).astype(np.float32)
            below, above, total = below + int((t < 0).sum()), above + int((t > peak).sum()), total + t.size
    print(f"{below} of {total} scaled results below 0, {above} above the peak")
    assert below > 0 and above > 0   # (both clamps have work)
    for k in range(N):   # padding bits are zeros
        for p, sh_ in zip(got[k], sft):
            assert int(np.count_nonzero(p & p.dtype.type((1 << sh_) - 1))) == 0 and int(p.max()) <= peak << sh_
    f.close()


# (id, filter, dst_bits, shifts, range, rgb, destination layout, (split, narrow, slices))
NARROWED = [
    ("f32_full_to_nv12", "YUV420PS", 8, None, "FULL", False, semi_planar(), (0, 2, 1)),
    ("f16_limited_to_p010", "YUV420PH", 10, [6] * 3, "LIMITED", False, semi_planar(), (0, 2, 1)),
    ("bf16_to_nv12", "YUV420PBF", 8, None, "LIMITED", False, semi_planar(), (0, 2, 1)),
    ("rgb_f32_to_bgra8", "RGBPS", 8, None, "FULL", True, BGRA, (0, 1, 1)),
    ("f32_422_to_y210", "YUV422PS", 10, [6] * 3, "LIMITED", False, Y210, (0, 2, 1)),
]


@pytest.mark.parametrize("case", NARROWED, ids=[c[0] for c in NARROWED])
def test_narrowed_equals_the_planar_call_scaled_and_narrowed_by_numpy(gpu_pkg, case):
    torch = pytest.importorskip("torch")
    _, name, bits, shifts, rng, rgb, layout, report = case
    sc, of = pairs(gpu_pkg, bits, getattr(gpu_pkg, "RANGE_" + rng), 3, rgb=rgb, to_code=True)
    check_narrowed(torch, gpu_pkg, name, bits, shifts, sc, of, layout, report)


def test_narrowed_scale_alone_offset_alone_and_a_negative_scale(gpu_pkg):
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = GEOM
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YUV420PS"], sw, sh, tw, th, device=0, **KW)
    frames = TN.sources(f.fmt, sw, sh, N, 1.0, seed=9)   # -0.15 .. 1.15
    r = run_planar(torch, f, frames, N)
    s = torch.cuda.current_stream()
    for scales, offsets in (([255.0] * 3, None), (None, [100.25, 60.5, 7.75]), ([-255.0, 219.0, -224.0], [255.0, 16.0, 240.0])):
        src, dst = TN.make_sides(torch, f, frames, planar(3), semi_planar(), 8, N)
        f.process_device_narrowed_scaled(src.ptrs(), src.pitches(), src.steps(), src.strides(), dst.ptrs(), dst.pitches(), dst.steps(), None, 8,
                                         scales, offsets, dst.strides(), N, stream=s.cuda_stream)
        s.synchronize()
        assert f.last_strided()[:3] == (0, 2, 1)
        got = dst.frames_and_guards(f"{scales} {offsets}")
        sc, of = scales or [1.0] * 3, offsets or [0.0] * 3
        want = [[narrowed_definition(p, sc[i], of[i], 255).astype(np.uint8) for i, p in enumerate(fr)] for fr in r]
        TN.assert_equal(got, want, f.out_dims(), f"scales {scales} offsets {offsets}")
    f.close()


# ---- fusing must show in the narrowing pass too --------------------------------------------------------------------------------------------------

_FUSED = {}


def values_whose_stored_integer_differs():
    """Values at which rint(clip(fma(r, scale, offset))) is not rint(clip(fl32(fl32(r * scale) + offset))), at the limited-range luma
    pairs of 8 bits (219, 16) and 10 bits (876, 64): {bits: (found at random, found beside ties)}.  At random: 2 x 10^7 seeded r in
    -0.08 .. 1.09, in chunks -- the two computations rarely differ after rounding, at (219, 16) four times more rarely still (the
    product's ulp is a quarter).  Beside ties: the 16 fp32 values on either side of every (k + 0.5 - offset) / scale."""
    if not _FUSED:
        def differing(r, bits, scale, offset):
            peak = (1 << bits) - 1
            fused = np.rint(np.clip(fused_fp32(r, scale, offset), 0, peak)).astype(np.uint32)
            return r[narrowed_definition(r, scale, offset, peak) != fused]
        pair_of = {8: (219.0, 16.0), 10: (876.0, 64.0)}
        rng = np.random.default_rng(20240)
        at_random = {8: [], 10: []}
        for _ in range(10):
            r = rng.uniform(-0.08, 1.09, 2_000_000).astype(np.float32)
            for bits, (scale, offset) in pair_of.items():
                at_random[bits].append(differing(r, bits, scale, offset))
        for bits, (scale, offset) in pair_of.items():
            up = down = ((np.arange((1 << bits) - 1) + 0.5 - offset) / scale).astype(np.float32)
            beside = [up]
            for _ in range(16):
                up, down = np.nextafter(up, np.float32(2)), np.nextafter(down, np.float32(-2))
                beside += [up, down]
            _FUSED[bits] = (np.concatenate(at_random[bits]), differing(np.concatenate(beside), bits, scale, offset))
    return _FUSED


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("bits", [8, 10])
def test_narrowing_pass_does_not_fuse(gpu_pkg, kind, bits):
    """The values the search found, padded with ordinary values to whole lanes and a tail, through narrow_samples_kernel's scaled form
    alone.  In fp32 every found value gives another stored integer when fused, so a fused kernel cannot pass; binary16 and bfloat16
    inputs have at most 11 significant bits, their products with 219 or 876 are exact in fp32 and nothing can differ -- those kinds
    check the same values, rounded to their type, against the definition."""
    at_random, beside_ties = values_whose_stored_integer_differs()[bits]
    print(f"{at_random.size} of 2e7 random values and {beside_ties.size} values beside ties whose stored {bits}-bit integer differs fused against un-fused")
    if bits == 10:
        assert at_random.size >= 32, at_random.size   # (876, 64): the random search alone must find them
    found = np.concatenate([at_random, beside_ties])
    assert found.size >= 32, found.size
    scale, offset = (219.0, 16.0) if bits == 8 else (876.0, 64.0)
    peak, shift = (1 << bits) - 1, 0 if bits == 8 else 6
    lane = 16 if bits == 8 else 8
    pad = np.random.default_rng(3).uniform(-0.1, 1.1, (found.size + 2047) // 2048 * 2048 + 3 * lane + 5 - found.size).astype(np.float32)
    vals = np.concatenate([found, pad])   # two trips of the wave and more, whole lanes, and a tail
    assert vals.size % lane and vals.size > 64 * lane
    if kind == "f16":
        given = vals.astype(np.float16)
        r = given.astype(np.float32)
    elif kind == "bf16":
        given = bf16_rne(vals)
        r = (given.astype(np.uint32) << 16).view(np.float32)
    else:
        given = r = vals
    want = (narrowed_definition(r, scale, offset, peak) << shift).astype(np.uint8 if bits == 8 else np.uint16)
    if kind == "f32":
        fused = (np.rint(np.clip(fused_fp32(r, scale, offset), 0, peak)).astype(np.uint32) << shift).astype(want.dtype)
        assert int((fused != want).sum()) >= found.size   # (what a fused kernel would store differs at every found value)
    for roll in (0, 3):   # every value in another position of a lane's vector, some in the tail
        got = gpu_pkg.debug_narrow_scaled(np.roll(given, roll), bits, shift, scale, offset, bfloat16=kind == "bf16")
        w = np.roll(want, roll)
        assert got.dtype == w.dtype and np.array_equal(got, w), (kind, bits, roll, int((got != w).sum()), np.roll(r, roll)[got != w][:8], got[got != w][:8], w[got != w][:8])


# ---- exhaustive conversion --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("out", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("pair", ["full", "limited_luma"])
def test_every_16_bit_value_through_the_widening_pass(gpu_pkg, out, pair):
    """All 65 536 values (and five more, so that the row has a tail) at (1 / 65535, 0) and at the limited-range 16-bit luma pair, bit
    for bit against numpy: binary16 subnormals below 2^-14, ties, and the negative values below code 4096."""
    pkg = gpu_pkg
    scale, offset = pkg.code_range(16, pkg.RANGE_FULL if pair == "full" else pkg.RANGE_LIMITED, pkg.PLANE_LUMA_OR_RGB)[:2]
    if pair == "full":
        assert scale == np.float32(1.0 / 65535) and offset == 0
    raw = (np.arange(65536 + 5) & 0xffff).astype(np.uint16)
    kind = {"f32": 0, "f16": HALF, "bf16": BF16}[out]
    want = widened_definition(raw.astype(np.uint32), scale, offset, kind)
    for roll in (0, 3):
        got = pkg.debug_widen_scaled(np.roll(raw, roll), 16, 0, scale, offset, {"f32": pkg.SAMPLE_DEFAULT, "f16": pkg.SAMPLE_FLOAT16, "bf16": pkg.SAMPLE_BFLOAT16}[out])
        got = np.ascontiguousarray(got).view(want.dtype)
        w = np.roll(want, roll)
        bad = np.flatnonzero(got != w)
        assert bad.size == 0, (out, pair, roll, bad.size, np.roll(raw, roll)[bad[:8]], got[bad[:8]], w[bad[:8]])
    if out == "f16":
        h = want.view(np.float16)
        assert ((h != 0) & (np.abs(h) < np.float16(6.104e-5))).any()   # subnormals were among them


@pytest.mark.parametrize("out", ["f32", "f16", "bf16"])
def test_10_bit_values_at_shift_6_and_bytes_through_the_widening_pass(gpu_pkg, out):
    pkg = gpu_pkg
    kind = {"f32": 0, "f16": HALF, "bf16": BF16}[out]
    out_kind = {"f32": pkg.SAMPLE_DEFAULT, "f16": pkg.SAMPLE_FLOAT16, "bf16": pkg.SAMPLE_BFLOAT16}[out]
    rng = np.random.default_rng(4)
    for bits, shift, plane in ((10, 6, pkg.PLANE_CHROMA), (10, 0, pkg.PLANE_LUMA_OR_RGB), (8, 0, pkg.PLANE_LUMA_OR_RGB), (8, 0, pkg.PLANE_CHROMA)):
        scale, offset = pkg.code_range(bits, pkg.RANGE_LIMITED, plane)[:2]
        v = np.concatenate([np.arange(1 << bits), rng.integers(0, 1 << bits, 1029)]).astype(np.uint32)
        junk = rng.integers(0, 1 << 16, v.size).astype(np.uint32) & ~np.uint32(((1 << bits) - 1) << shift) & np.uint32(0xffff if bits > 8 else 0)
        raw = ((v << shift) | junk).astype(np.uint8 if bits == 8 else np.uint16)
        want = widened_definition(v, scale, offset, kind)
        got = np.ascontiguousarray(pkg.debug_widen_scaled(raw, bits, shift, scale, offset, out_kind)).view(want.dtype)
        assert np.array_equal(got, want), (out, bits, shift, int((got != want).sum()))


# ---- identity ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,bits,shifts", [("YUV420PS", 8, None), ("YUV420PS", 10, [6] * 3), ("YUV420PH", 10, [6] * 3)], ids=["nv12_f32", "p010_f32", "p010_f16"])
def test_identity_arrays_and_null_arrays_give_the_unscaled_widened_call(gpu_pkg, name, bits, shifts):
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = GEOM
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    raw = raw_of(values(gpu_pkg, name, sw, sh, bits, N), bits, shifts or [0] * 3)
    s = torch.cuda.current_stream()
    results, reports, calls = [], [], []
    for arrays in ("unscaled", ([1.0] * 3, [0.0] * 3), (None, None)):
        src, dst = TW.make_sides(torch, f, raw, semi_planar(), planar(3), N)
        if arrays == "unscaled":
            TW.call(f, src, dst, shifts, bits, N, s)
        else:
            f.process_device_widened_scaled(src.ptrs(), src.pitches(), src.steps(), shifts, bits, arrays[0], arrays[1], src.strides(), dst.ptrs(),
                                            dst.pitches(), dst.steps(), dst.strides(), N, stream=s.cuda_stream)
        s.synchronize()
        results.append(dst.frames_and_guards(str(arrays)))
        reports.append(f.last_strided())
        calls.append(gpu_pkg.last_call())
    assert reports[0] == reports[1] == reports[2] and reports[0][:3] == (2, 0, 1), reports
    assert calls[0] == calls[2], calls   # both arrays NULL: the same launches
    for k in (1, 2):
        assert_bits_equal(results[k], results[0], f.out_dims(), f"{name} {bits}-bit: arrays {k} against the unscaled call")
    f.close()


@pytest.mark.parametrize("name,bits,shifts", [("YUV420PS", 8, None), ("YUV420PS", 10, [6] * 3), ("YUV420PBF", 10, [6] * 3)], ids=["nv12_f32", "p010_f32", "p010_bf16"])
def test_identity_arrays_and_null_arrays_give_the_unscaled_narrowed_call(gpu_pkg, name, bits, shifts):
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = GEOM
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    frames = TN.sources(f.fmt, sw, sh, N, (1 << bits) - 1, seed=6)
    s = torch.cuda.current_stream()
    results, reports, calls = [], [], []
    for arrays in ("unscaled", ([1.0] * 3, [0.0] * 3), (None, None)):
        src, dst = TN.make_sides(torch, f, frames, planar(3), semi_planar(), bits, N)
        if arrays == "unscaled":
            TN.narrowed_call(f, src, dst, shifts, bits, N, s)
        else:
            f.process_device_narrowed_scaled(src.ptrs(), src.pitches(), src.steps(), src.strides(), dst.ptrs(), dst.pitches(), dst.steps(), shifts,
                                             bits, arrays[0], arrays[1], dst.strides(), N, stream=s.cuda_stream)
        s.synchronize()
        results.append(dst.frames_and_guards(str(arrays)))
        reports.append(f.last_strided())
        calls.append(gpu_pkg.last_call())
    assert reports[0] == reports[1] == reports[2] and reports[0][:3] == (0, 2, 1), reports
    assert calls[0] == calls[2], calls   # both arrays NULL: the same launches
    for k in (1, 2):
        TN.assert_equal(results[k], results[0], f.out_dims(), f"{name} {bits}-bit: arrays {k} against the unscaled call")
    f.close()


def test_wide_samples_with_null_arrays_are_refused_on_the_device_too(gpu_pkg):
    """P016 into a half filter and P010 into a bfloat16 filter with both arrays NULL: refused as the unscaled call refuses them, with
    nothing written; with a scale given they run (the cases above)."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = GEOM
    for name, bits, shifts in (("YUV420PH", 16, None), ("YUV420PBF", 10, [6] * 3)):
        f = gpu_pkg.Filter(gpu_pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
        raw = raw_of(values(gpu_pkg, name, sw, sh, bits, 1), bits, shifts or [0] * 3)
        src, dst = TW.make_sides(torch, f, raw, semi_planar(), planar(3), 1)
        with pytest.raises(gpu_pkg.JincError) as e:
            f.process_device_widened_scaled(src.ptrs(), src.pitches(), src.steps(), shifts, bits, None, None, src.strides(), dst.ptrs(), dst.pitches(),
                                            dst.steps(), dst.strides(), 1, stream=torch.cuda.current_stream().cuda_stream)
        assert e.value.code == -1 and "not exact in" in str(e.value), str(e.value)
        torch.cuda.synchronize()
        image = dst.download()
        for b, B in dst.bufs.items():
            assert np.array_equal(image[b], B["host"]), "a refused call wrote to the destination"
        f.close()
