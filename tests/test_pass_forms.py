"""Every form of widen_samples_kernel and narrow_samples_kernel that the public calls can reach, on the device: N = 1 .. 4 samples per
pixel x bytes / 16-bit words x fp32 / binary16 / bfloat16 planes x unscaled / scaled, each through the 16-byte accesses, the dwords
and the sample-by-sample loop.  The host tests run the row functions lane by lane (csrc/widen_rows.h, csrc/narrow_rows.h); on the
device the same functions become other code -- round_sample_u8, round_pair_u16, v_cvt_f32_ubyte*, scale / offset / shift held per
channel in scalar registers -- and only a run there checks it.  The layouts are the ones with EVERY channel given (NV12 / P010 style
for N = 1 and 2, BGR24 / RGB48 for N = 3, BGRA32 / RGBA64 for N = 4), so that the vector loops run, with a channel order that is not the
plane order, a shift and a (scale, offset) pair of its own per plane, and one negative scale.

Expected values never come from the pass under test, and the tolerance is zero:
  widened   numpy builds the dense planes from the raw samples by the definition; jinc_filter_process_device on those planes is the
            expected result, compared bit for bit;
  narrowed  the planar call's result goes through numpy, rint(clip(fl32(fl32(r * scale) + offset), 0, peak)) << shift, compared byte
            for byte.
Every destination lies in a larger buffer of seeded bytes whose other bytes must keep their value, the source must come back
unchanged, jinc_debug_last_strided must report the documented launches (and for a scaled call what the unscaled call on the same
sides reports), and jinc_debug_last_groups must say which loop ran: unit and vec_pixels of every group.  The last test of the file
holds the set of forms seen with vec_pixels > 0 against the full reachable set.

Reachable: 48 narrowing forms and 44 of the 48 widening forms.  The four that no public call reaches are the UNSCALED widening of
16-bit words into bfloat16 planes at N = 1, 2, 3 and 4 -- widen_row<2, N, 2, kSampleBFloat16, false>: nine bits and more are not exact
in bfloat16, the unscaled call refuses them (test_words_into_bfloat16_unscaled_are_refused) and the kernel has no such instantiation.
Unscaled binary16 filters take words of up to 11 bits only, so their word forms run at the 10-bit setting alone.

Geometry: tap 3, 2 frames, integer rows of 524 samples (chroma 262).  A byte lane owns 16 pixels: 32 lanes and a tail of 12 (chroma
6); a word lane owns 8: 65 lanes, so lane 0 makes a second trip, and a tail of 4; 38 or 76 rows leave the last row block of 4 waves
partly empty.  Narrowing is the siblings' 262 x 38 -> 524 x 76, widening 524 x 38 -> 262 x 20."""
import numpy as np
import pytest

import test_narrowed as TN
import test_widened as TW
from test_narrowed import widened
from test_narrowed_host import definition
from test_scaled import dense_planes
from test_scaled_host import bf16_rne, narrowed_definition
from test_shifted import Y210
from test_strided import INVALID_ARG, packed, planar, run_planar, semi_planar
from test_widened import assert_bits_equal, assert_source_unchanged, raw_of, values

pytestmark = pytest.mark.gpu

KW = dict(tap=3)
N = 2
NARROW_GEOM = (262, 38, 524, 76)
WIDEN_GEOM = (524, 38, 262, 20)
WIDEN, NARROW = 0, 1   # jinc_group_info.direction
KINDS = ("f32", "f16", "bf16")
TAG = {"f32": "S", "f16": "H", "bf16": "BF"}

# layout -> (filter family, the integer side)
LAYOUTS = {
    "nv": ("YUV420P", semi_planar()),            # luma N = 1 and chroma N = 2 in one call
    "rgb": ("RGBP", packed("BGR", 3, 3)),        # planes G, B, R at channels 1, 0, 2
    "rgba": ("RGBAP", packed("BGRA", 4, 4)),     # planes G, B, R, A at channels 1, 0, 2, 3
}
# (bits, shifts by plane): bytes; words at the top of round_pair_u16's range; 10-bit words with another shift in every plane
SETTINGS = [(8, None), (16, None), (10, [6, 4, 2, 0])]
ALIGNS = (16, 4, 1)   # test_strided.Side: base, pitch and frame stride multiples of 16, of 4 only, of the sample size only

SEEN = set()   # (direction, kind, n, sample bytes, scaled, unit) of every complete group that ran with vec_pixels > 0


def filter_name(layout, kind):
    return LAYOUTS[layout][0] + TAG[kind]


def kind_name(fmt):
    return "bf16" if fmt.bfloat16 else "f16" if fmt.half else "f32"


def to_float_pairs(pkg, bits, planes):
    """(scales, offsets) from code values to the float range, one pair per plane, no two equal: the limited-range luma pair of
    jinc_code_range, a NEGATIVE limited-range chroma scale (1 at code 16 k, 0 at code 240 k), the full-range chroma pair and an inverted
    full range."""
    k, peak = 1 << (bits - 8), (1 << bits) - 1
    luma, chroma = pkg.code_range(bits, pkg.RANGE_LIMITED, pkg.PLANE_LUMA_OR_RGB), pkg.code_range(bits, pkg.RANGE_FULL, pkg.PLANE_CHROMA)
    sc = [luma[0], np.float32(-1.0 / (224 * k)), chroma[0], np.float32(-1.0 / peak)]
    of = [luma[1], np.float32(240.0 / 224), chroma[1], np.float32(1.0)]
    assert len(set(zip(map(float, sc), map(float, of)))) == 4 and len(set(map(float, sc))) == 4 and len(set(map(float, of))) == 4
    return sc[:planes], of[:planes]


def to_code_pairs(pkg, bits, planes):
    """The same four the other way: from the float range to code values."""
    k, peak = 1 << (bits - 8), (1 << bits) - 1
    luma, chroma = pkg.code_range(bits, pkg.RANGE_LIMITED, pkg.PLANE_LUMA_OR_RGB), pkg.code_range(bits, pkg.RANGE_FULL, pkg.PLANE_CHROMA)
    sc = [luma[2], np.float32(-224.0 * k), chroma[2], np.float32(-float(peak))]
    of = [luma[3], np.float32(240.0 * k), chroma[3], np.float32(peak)]
    assert len(set(map(float, sc))) == 4 and len(set(map(float, of))) == 4 and float(sc[0]) == 219 * k and float(of[0]) == 16 * k
    return sc[:planes], of[:planes]


# ---- the record -----------------------------------------------------------------------------------------------------------------------

def group_shapes(layout, dims):
    """(n, members, width, rows) of the channel groups of an integer side, in the order of each group's first plane."""
    shapes, index = [], {}
    for i, (b, chan, step) in enumerate(layout):
        key = (b, step)
        if key not in index:
            index[key] = len(shapes)
            shapes.append([step, 0, dims[i][0], dims[i][1]])
        shapes[index[key]][1] += 1
    return [tuple(s) for s in shapes]


def check_groups(groups, direction, fmt, layout, dims, sb, scaled, units, what):
    """jinc_debug_last_groups against what the layout and the access class say.  Complete groups move width // P * P pixels by
    vectors (P = 16 / sample bytes pixels a lane); a group with a channel missing none when narrowed, (width - 1) // P * P when
    widened; unit 0 means no vectors at all."""
    shapes = group_shapes(layout, dims)
    assert len(groups) == len(shapes) == len(units), (what, groups, shapes)
    P = 16 // sb
    for g, (n, members, w, h), unit in zip(groups, shapes, units):
        assert (g["direction"], g["n"], g["members"], g["sample_bytes"], g["sample_type"], g["scaled"], g["width"], g["rows"]) == \
               (direction, n, members, sb, fmt.sample_type, int(scaled), w, h), (what, g)
        assert g["unit"] == unit, (what, g)
        if members == n:
            vec = w // P * P if unit else 0
        else:
            vec = 0 if direction == NARROW or not unit else (w - 1) // P * P
        assert g["vec_pixels"] == vec, (what, g, vec)
        if unit and members == n:
            assert vec > 0, (what, g)
            SEEN.add((direction, kind_name(fmt), n, sb, bool(scaled), unit))


def units_of(align, ngroups):
    return [align if align in (16, 4) else 0] * ngroups


# ---- widened ------------------------------------------------------------------------------------------------------------------------------

def widened_call(f, src, dst, shifts, bits, pairs, n, stream):
    if pairs is None:
        TW.call(f, src, dst, shifts, bits, n, stream)
    else:
        f.process_device_widened_scaled(src.ptrs(), src.pitches(), src.steps(), shifts, bits, pairs[0], pairs[1], src.strides(), dst.ptrs(),
                                        dst.pitches(), dst.steps(), dst.strides(), n, stream=stream.cuda_stream)


def run_widened(torch, pkg, f, raw, bits, shifts, layout, align, pairs, want, report, units, what, n=N, seeds=(11, 12), src=None, **side_kw):
    """One widened call (pairs None: unscaled) held against `want`; returns (source side, last_strided)."""
    made, dst = TW.make_sides(torch, f, raw, layout, planar(f.fmt.planes), n, src_align=align, seeds=seeds, **side_kw)
    src = src or made
    s = torch.cuda.current_stream()
    widened_call(f, src, dst, shifts, bits, pairs, n, s)
    s.synchronize()
    got_report, groups = f.last_strided(), f.last_groups()
    got = dst.frames_and_guards(what)
    assert_source_unchanged(src, what)
    assert got_report[:3] == report, (what, got_report)
    check_groups(groups, WIDEN, f.fmt, layout, f.fmt.plane_dims(f.src_w, f.src_h), 1 if bits == 8 else 2, pairs is not None, units, what)
    assert_bits_equal(got, want, f.out_dims(), what + " against the planar call on numpy's planes")
    return src, got_report


def widened_settings(kind):
    """(bits, shifts, an unscaled call exists) for a filter kind: binary16 takes at most 11 bits unscaled, bfloat16 bytes only."""
    for bits, shifts in SETTINGS:
        yield bits, shifts, not (kind == "f16" and bits > 11 or kind == "bf16" and bits > 8)


def check_widened_forms(torch, pkg, kind, layout_name, geom=WIDEN_GEOM, n=N, settings=None, aligns=ALIGNS):
    name, layout = filter_name(layout_name, kind), LAYOUTS[layout_name][1]
    sw, sh, tw, th = geom
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    planes = f.fmt.planes
    report = (len(group_shapes(layout, f.fmt.plane_dims(sw, sh))), 0, 1)   # one widening launch per step value, no merge: planar planes out
    for bits, shifts, unscaled_exists in settings or widened_settings(kind):
        shifts = shifts and shifts[:planes]
        vals = values(pkg, name, sw, sh, bits, n)
        raw = raw_of(vals, bits, shifts or [0] * planes, dirty_seed=77 if bits == 10 else None)
        pairs = to_float_pairs(pkg, bits, planes)
        # the planar references, once per distinct input: the planes the definition says the filter reads, built by numpy
        want_scaled = run_planar(torch, f, dense_planes(f.fmt, vals, *pairs), n)
        want_plain = run_planar(torch, f, dense_planes(f.fmt, vals, [1.0] * planes, [0.0] * planes), n) if unscaled_exists else None
        for align in aligns:
            what = f"{bits}-bit {layout_name} shifts {shifts} align {align} -> {name}"
            units = units_of(align, report[0])
            src, scaled_report = run_widened(torch, pkg, f, raw, bits, shifts, layout, align, pairs, want_scaled, report, units, what + " scaled", n=n)
            if unscaled_exists:   # on the same source side: the same launches, slices and scratch bytes
                _, plain_report = run_widened(torch, pkg, f, raw, bits, shifts, layout, align, None, want_plain, report, units, what, n=n, seeds=(11, 15), src=src)
                assert plain_report == scaled_report, (what, plain_report, scaled_report)
    f.close()


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("kind", KINDS)
def test_widened_forms(gpu_pkg, kind, layout):
    torch = pytest.importorskip("torch")
    check_widened_forms(torch, gpu_pkg, kind, layout)


# ---- narrowed -----------------------------------------------------------------------------------------------------------------------------

def sources_for(fmt, sw, sh, n, peak, pairs, seed):
    """n frames whose code values span 0.15 peak below 0 to 0.15 peak above the peak, taken back through the pairs into the filter's
    range (test_scaled.normalised_sources; no pairs: test_narrowed.sources) -- both clamps have work.  Frame 1 carries one +inf, one
    -inf and one NaN in every plane, a quarter of the plane apart.  binary16 holds nothing above 65504: its unscaled 16-bit sources
    stop at 60000."""
    rng = np.random.default_rng(seed)
    top = 1.15 * peak if pairs is not None or not fmt.half else min(1.15 * peak, 60000.0)
    out = []
    for k in range(n):
        frame = []
        for i, (w, h) in enumerate(fmt.plane_dims(sw, sh)):
            code = rng.uniform(-0.15 * peak, top, (h, w))
            v = (code if pairs is None else (code - float(pairs[1][i])) / float(pairs[0][i])).astype(np.float32)
            if k == 1:
                assert w // 4 >= 16
                v[h // 4, w // 4], v[h // 2, w // 2], v[3 * h // 4, 3 * w // 4] = np.inf, -np.inf, np.nan
            frame.append(bf16_rne(v) if fmt.bfloat16 else v.astype(fmt.dtype))
        out.append(frame)
    return out


def narrowed_expectation(fmt, planar_frames, dims, bits, shifts, pairs, dtype, what, ties_must_show):
    """The planar call's result through numpy's definition, and what the case must contain: results on both sides of both bounds in
    every plane, exact k + 0.5 ties, and in frame 1 a NaN and both infinities in front of the conversion."""
    peak = (1 << bits) - 1
    want = []
    for k, planes in enumerate(planar_frames):
        frame = []
        for i, p in enumerate(planes):
            w, h = dims[i]
            r = widened(fmt, p)
            if pairs is None:
                t, value = r, definition(r, peak)
            else:
                with np.errstate(over="ignore", invalid="ignore"):
                    t = ((r * np.float32(pairs[0][i])).astype(np.float32) + np.float32(pairs[1][i])).astype(np.float32)
                value = narrowed_definition(r, pairs[0][i], pairs[1][i], peak)
            frame.append((value << shifts[i]).astype(dtype))
            t, value = t[:h, :w], value[:h, :w]
            finite = t[np.isfinite(t)]
            below, above = int((finite < 0).sum()), int((finite > peak).sum())
            inside = finite[(finite > 0) & (finite < peak)]
            ties = int((inside - np.floor(inside) == 0.5).sum())
            print(f"{what} frame {k} plane {i}: {below} below 0, {above} above the peak, {ties} ties, {int(np.isnan(t).sum())} NaN, "
                  f"{int(np.isposinf(t).sum())} +inf, {int(np.isneginf(t).sum())} -inf")
            assert below > 0, (what, k, i)
            if not (fmt.half and pairs is None and bits == 16):   # (no finite binary16 value lies above 65535)
                assert above > 0, (what, k, i)
            if ties_must_show:
                assert ties > 0, (what, k, i)
            if k == 1:   # spelled out beside the definition: a NaN and -inf become 0, +inf the peak
                assert np.isnan(t).any() and np.isposinf(t).any() and np.isneginf(t).any(), (what, i)
                assert (value[np.isnan(t)] == 0).all() and (value[np.isneginf(t)] == 0).all() and (value[np.isposinf(t)] == peak).all(), (what, i)
        want.append(frame)
    return want


def narrowed_call(f, src, dst, shifts, bits, pairs, n, stream):
    if pairs is None:
        TN.narrowed_call(f, src, dst, shifts, bits, n, stream)
    else:
        f.process_device_narrowed_scaled(src.ptrs(), src.pitches(), src.steps(), src.strides(), dst.ptrs(), dst.pitches(), dst.steps(), shifts, bits,
                                         pairs[0], pairs[1], dst.strides(), n, stream=stream.cuda_stream)


def run_narrowed(torch, pkg, f, frames, bits, shifts, layout, align, pairs, want, report, units, what, n=N, seeds=(11, 12), src=None, compare=True):
    """One narrowed call (pairs None: unscaled) held against `want`; returns (source side, last_strided)."""
    made, dst = TN.make_sides(torch, f, frames, planar(f.fmt.planes), layout, bits, n, dst_align=align, seeds=seeds)
    src = src or made
    s = torch.cuda.current_stream()
    narrowed_call(f, src, dst, shifts, bits, pairs, n, s)
    s.synchronize()
    got_report, groups = f.last_strided(), f.last_groups()
    got = dst.frames_and_guards(what)
    assert_source_unchanged(src, what)
    assert got_report[:3] == report, (what, got_report)
    check_groups(groups, NARROW, f.fmt, layout, f.out_dims(), 1 if bits == 8 else 2, pairs is not None, units, what)
    if compare:
        TN.assert_equal(got, want, f.out_dims(), what + " against the planar call narrowed by numpy")
        for k in range(n):   # padding bits are zeros: the stored sample is value << shift as the whole word
            for p, sft in zip(got[k], shifts or [0] * f.fmt.planes):
                assert int(np.count_nonzero(p & p.dtype.type((1 << sft) - 1))) == 0 and int(p.max()) <= ((1 << bits) - 1) << sft, what
    return src, got_report


def check_narrowed_forms(torch, pkg, kind, layout_name, geom=NARROW_GEOM, n=N, settings=SETTINGS, aligns=ALIGNS):
    name, layout = filter_name(layout_name, kind), LAYOUTS[layout_name][1]
    sw, sh, tw, th = geom
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    planes, dims = f.fmt.planes, f.out_dims()
    report = (0, len(group_shapes(layout, dims)), 1)   # planar planes in: no split; one narrowing launch per step value
    for bits, shifts in settings:
        shifts = shifts and shifts[:planes]
        dtype = np.uint8 if bits == 8 else np.uint16
        peak = (1 << bits) - 1
        for pairs in (None, to_code_pairs(pkg, bits, planes)):
            tag = f"{name} -> {bits}-bit {layout_name} shifts {shifts}" + (" scaled" if pairs else "")
            frames = sources_for(f.fmt, sw, sh, n, peak, pairs, seed=5 + bits)
            # binary16 and bfloat16 results (11 and 8 significant bits) hit k + 0.5 exactly wherever their spacing is 0.5 or finer:
            # unscaled, below 1024 and below 128 -- a good part of the range of bytes and of 10-bit words
            ties_must_show = kind != "f32" and pairs is None and bits in (8, 10)
            want = narrowed_expectation(f.fmt, run_planar(torch, f, frames, n), dims, bits, shifts or [0] * planes, pairs, dtype, tag, ties_must_show)
            for align in aligns:
                what = f"{tag} align {align}"
                units = units_of(align, report[1])
                src, got_report = run_narrowed(torch, pkg, f, frames, bits, shifts, layout, align, pairs, want, report, units, what, n=n)
                if pairs is not None:   # the unscaled call on the same sides: the same launches, slices and scratch bytes
                    _, plain_report = run_narrowed(torch, pkg, f, frames, bits, shifts, layout, align, None, None, report, units, what + " (unscaled, for its report)",
                                                   n=n, seeds=(11, 16), src=src, compare=False)
                    assert plain_report == got_report, (what, plain_report, got_report)
    f.close()


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("kind", KINDS)
def test_narrowed_forms(gpu_pkg, kind, layout):
    torch = pytest.importorskip("torch")
    check_narrowed_forms(torch, gpu_pkg, kind, layout)


# ---- a second trip of the wave at N = 3 ------------------------------------------------------------------------------------------------------

def test_rgb24_rows_longer_than_one_trip_of_the_wave(gpu_pkg):
    """The N = 3 twin of the siblings' 2070-byte rows: 2070 pixels of BGR24 are two whole trips of 64 lanes x 16 pixels, a third of two
    lanes (129 lanes' worth: 2064 pixels) and a tail of 6 pixels, narrowed from RGBPS (1035 x 8 -> 2070 x 16) and widened into it
    (2070 x 16 -> 4140 x 32); one frame."""
    torch = pytest.importorskip("torch")
    bytes_only = SETTINGS[:1]
    check_narrowed_forms(torch, gpu_pkg, "f32", "rgb", geom=(1035, 8, 2070, 16), n=1, settings=bytes_only, aligns=(16,))
    assert gpu_pkg.last_groups()[0]["vec_pixels"] == 2064 and gpu_pkg.last_groups()[0]["width"] == 2070
    check_widened_forms(torch, gpu_pkg, "f32", "rgb", geom=(2070, 16, 4140, 32), n=1, settings=[(8, None, True)], aligns=(16,))
    assert gpu_pkg.last_groups()[0]["vec_pixels"] == 2064 and gpu_pkg.last_groups()[0]["width"] == 2070


# ---- incomplete groups: what the record shows -------------------------------------------------------------------------------------------------

BGRX = packed("BGRA", 4, 3)   # three components at step 4: the X byte of every pixel is no sample of the call
# (id, filter, bits, shifts, integer side, narrowed units, widened (lead, units))
INCOMPLETE = [
    ("bgrx8", "RGBPS", 8, None, BGRX, [16], [(None, [16])]),
    # Y at step 2 from the buffer's base, U and V at step 4 from one sample behind it: whichever of the two groups starts on a 16-byte
    # boundary has the vectors, the other one starts 2 bytes off a dword and moves sample by sample
    ("y210", "YUV422PS", 10, [6, 6, 6], Y210, [16, 0], [(None, [16, 0]), ({0: 62}, [0, 16])]),
]


@pytest.mark.parametrize("case", INCOMPLETE, ids=[c[0] for c in INCOMPLETE])
def test_narrowed_incomplete_groups_store_sample_by_sample(gpu_pkg, case):
    """A group with a channel missing stores only the given channels' samples: vec_pixels is 0 whatever the alignment, and the X
    bytes of BGRX (guard bytes of the destination) and every other plane's samples keep their values."""
    torch = pytest.importorskip("torch")
    _, name, bits, shifts, layout, units, _ = case
    sw, sh, tw, th = NARROW_GEOM
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    dims = f.out_dims()
    report = (0, len(units), 1)
    assert all(members < n for n, members, _, _ in group_shapes(layout, dims))
    for pairs in (None, to_code_pairs(gpu_pkg, bits, 3)):
        what = f"{name} -> {bits}-bit {case[0]}" + (" scaled" if pairs else "")
        frames = sources_for(f.fmt, sw, sh, N, (1 << bits) - 1, pairs, seed=7)
        want = narrowed_expectation(f.fmt, run_planar(torch, f, frames, N), dims, bits, shifts or [0] * 3, pairs, np.uint8 if bits == 8 else np.uint16, what, False)
        run_narrowed(torch, gpu_pkg, f, frames, bits, shifts, layout, 16, pairs, want, report, units, what)
        assert [g["vec_pixels"] for g in f.last_groups()] == [0] * len(units)
    f.close()


@pytest.mark.parametrize("case", INCOMPLETE, ids=[c[0] for c in INCOMPLETE])
def test_widened_incomplete_groups_stop_in_front_of_the_last_pixel(gpu_pkg, case):
    """A group with a channel missing reads whole pixels up to the last but one -- vec_pixels == (width - 1) // P * P -- and the last
    pixel's given samples one by one."""
    torch = pytest.importorskip("torch")
    _, name, bits, shifts, layout, _, classes = case
    sw, sh, tw, th = WIDEN_GEOM
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    P = 16 if bits == 8 else 8
    shapes = group_shapes(layout, f.fmt.plane_dims(sw, sh))
    assert all(members < n for n, members, _, _ in shapes)
    vals = values(gpu_pkg, name, sw, sh, bits, N)
    raw = raw_of(vals, bits, shifts or [0] * 3, dirty_seed=77 if bits == 10 else None)
    pairs = to_float_pairs(gpu_pkg, bits, 3)
    want_scaled = run_planar(torch, f, dense_planes(f.fmt, vals, *pairs), N)
    want_plain = run_planar(torch, f, dense_planes(f.fmt, vals, [1.0] * 3, [0.0] * 3), N)
    for lead, units in classes:
        kw = dict(lead=lead) if lead else {}
        what = f"{bits}-bit {case[0]} lead {lead} -> {name}"
        src, scaled_report = run_widened(torch, gpu_pkg, f, raw, bits, shifts, layout, 16, pairs, want_scaled, (len(units), 0, 1), units, what + " scaled", **kw)
        assert [g["vec_pixels"] for g in f.last_groups()] == [(w - 1) // P * P if u else 0 for (_, _, w, _), u in zip(shapes, units)]
        _, plain_report = run_widened(torch, gpu_pkg, f, raw, bits, shifts, layout, 16, None, want_plain, (len(units), 0, 1), units, what, seeds=(11, 15), src=src, **kw)
        assert plain_report == scaled_report
    f.close()


# ---- the four forms nothing reaches -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_words_into_bfloat16_unscaled_are_refused(gpu_pkg, layout):
    """10-bit and 16-bit words into a bfloat16 filter without a scale: refused on the arguments alone at N = 1 and 2 (nv), 3 and 4,
    nothing is written, and both records stay what the call before left."""
    torch = pytest.importorskip("torch")
    name, int_layout = filter_name(layout, "bf16"), LAYOUTS[layout][1]
    sw, sh, tw, th = WIDEN_GEOM
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    planes = f.fmt.planes
    for bits, shifts in SETTINGS[1:]:
        shifts = shifts and shifts[:planes]
        raw = raw_of(values(gpu_pkg, name, sw, sh, bits, 1), bits, shifts or [0] * planes)
        src, dst = TW.make_sides(torch, f, raw, int_layout, planar(planes), 1)
        before = (f.last_strided(), f.last_groups())
        with pytest.raises(gpu_pkg.JincError) as e:
            TW.call(f, src, dst, shifts, bits, 1, torch.cuda.current_stream())
        assert e.value.code == INVALID_ARG and "not exact in bfloat16" in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert (f.last_strided(), f.last_groups()) == before
        image = dst.download()
        for b, B in dst.bufs.items():
            assert np.array_equal(image[b], B["host"]), "a refused call wrote to the destination"
        assert_source_unchanged(src, f"{bits}-bit {layout} refused")
    f.close()


# ---- the form set -------------------------------------------------------------------------------------------------------------------------------

def reachable_forms():
    forms = set()
    for kind in KINDS:
        for n in (1, 2, 3, 4):
            for sb in (1, 2):
                for scaled in (False, True):
                    forms.add((NARROW, kind, n, sb, scaled))
                    if not (kind == "bf16" and sb == 2 and not scaled):
                        forms.add((WIDEN, kind, n, sb, scaled))
    return forms


def test_zz_every_reachable_form_ran_on_vectors():
    """Must run after the tests above (it does in file order): every reachable form was seen as a complete group with vec_pixels > 0,
    once through 16-byte accesses and once through dwords.  A later edit that drops a case, or a dispatch change that sends groups
    sample by sample, fails here."""
    forms = reachable_forms()
    narrow, widen = [x for x in forms if x[0] == NARROW], [x for x in forms if x[0] == WIDEN]
    assert len(narrow) == 48 and len(widen) == 44
    want = {form + (unit,) for form in forms for unit in (16, 4)}
    seen_forms = {x[:5] for x in SEEN}
    print(f"{len([x for x in seen_forms if x[0] == NARROW])} narrow and {len([x for x in seen_forms if x[0] == WIDEN])} widen forms seen with vec_pixels > 0, "
          f"{len(SEEN)} with their access class")
    assert SEEN, "no form test ran in this session: run the whole file"
    missing = sorted(want - SEEN)
    assert not missing, f"{len(missing)} forms never ran on vectors (direction, kind, n, sample bytes, scaled, unit): {missing}"
    assert SEEN == want, sorted(SEEN - want)
