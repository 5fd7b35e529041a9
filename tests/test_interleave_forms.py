"""Every form of split_samples_kernel<B, N, Shifted> and merge_samples_kernel<B, N, Shifted> that launch_by_shape holds, on the device:
B = 1, 2, 4 bytes a sample x N = 2, 3, 4 samples a pixel unshifted and B = 2 x N = 1, 2, 3, 4 shifted -- 13 forms in each direction --
each through the 16-byte accesses, the dwords and the sample-by-sample loop.  The layouts are the ones with EVERY channel given
(NV12 / P010 style for N = 1 and 2, BGR for N = 3, BGRA for N = 4: the channel order is never the plane order), so that the vector
loops run; both sides of a call have the layout and the access class under test, so one call runs the split and the merge.

Expected values never pass through the passes under test, and the tolerance is zero: numpy builds the dense planes the definition
says the filter reads -- the samples themselves, raw >> shift for a shifted source -- jinc_filter_process_device on those planes is
the expected result, and the destination must hold it bit for bit, for a shifted destination as the whole word result << shift
(padding bits zero).  Integer sources carry pseudo-random bits below and above the sample, every plane of a side has a shift of its
own and the two sides have different shift lists: a pass that used channel 0's shift or mask for every channel fails.  (The merge's
`& mask[c]` is not observable from a public call: results are clamped to the sample's bits and a shift never exceeds the padding,
so result << shift stays inside its half of the dword; dropping it passes this file.)  fp32 and
binary16 frames carry NaN and both infinities, bfloat16 frames arbitrary 16-bit patterns: the passes move bytes and look at no value.
Every destination lies in a larger buffer of seeded bytes whose other bytes must keep their value, the source must come back
unchanged, jinc_debug_last_strided must report one launch per direction and step value, and jinc_debug_last_groups must say which
loop ran: (direction, n, members, sample_bytes, shifted, unit, vec_pixels, width, rows) of every group, computed here from the
layout and the alignment alone.  The last test holds the set of forms seen against the full set.

Reachable: all 26 forms with vec_pixels > 0 at unit 16 and at unit 4 (52), and 20 of the 26 at unit 0.  The six that no public call
reaches are the B = 4 forms (N = 2, 3, 4, both directions) at unit 0: unit is 0 only where the group's base, pitch or frame stride
is no multiple of 4, and for 4-byte samples check_strided_planes refuses each of those ("not aligned to the sample size", "not a
multiple of the sample size"): test_fp32_samples_off_a_dword_are_refused.  For B = 4 the sample-size class IS the dword class, and
Side(align=1) gives it (lead 68, pitch 4 mod 8): it is run and recorded as unit 4.

Geometry: tap 3, 2 frames, 263 x 19 -> 526 x 38 (4:2:0 chroma 131 x 9 -> 263 x 19): no row count is a multiple of 4, so the last
block of four waves is partly empty on both sides.  A lane owns P = 16 / B pixels and a wave's trip is 64 P = 1024 / 512 / 256
pixels for B = 1 / 2 / 4.  Rows, as vector pixels + sample tail:
            B = 1        B = 2        B = 4
  131       128 + 3      128 + 3      128 + 3
  263       256 + 7      256 + 7      260 + 3   (B = 4: 65 lanes, lane 0 makes a second trip)
  526       512 + 14     520 + 6      524 + 2   (B = 2: 65 lanes, a second trip; B = 4: 131 lanes, three trips)
so at B = 4 both directions make a second trip in the common geometry, and at B = 2 the merge does.  The long cases add the rest:
  B = 2 split, unshifted and shifted: 526 x 7 -> 1052 x 14, source 520 + 6 (65 lanes), destination 1048 + 4 (131 lanes);
  B = 1 both directions: 1046 x 7 -> 2092 x 14, source 1040 + 6 (65 lanes), destination 2080 + 12 (130 lanes, three trips).
The closing test asserts a vec_pixels above one trip for every (direction, B, shifted)."""
import numpy as np
import pytest

from test_pass_forms import group_shapes
from test_strided import INVALID_ARG, Side, packed, planar, run_planar, semi_planar
from test_widened import assert_bits_equal, assert_source_unchanged, raw_of, values

pytestmark = pytest.mark.gpu

KW = dict(tap=3)
N = 2
GEOM = (263, 19, 526, 38)
SPLIT, MERGE = 2, 3   # jinc_group_info.direction
ALIGNS = (16, 4, 1)   # test_strided.Side: base, pitch and frame stride multiples of 16, of 4 only, of the sample size only
ONE_TRIP = {1: 1024, 2: 512, 4: 256}

LAYOUTS = {2: semi_planar(), 3: packed("BGR", 3, 3), 4: packed("BGRA", 4, 4)}   # by the largest step: planes G, B, R(, A) at channels 1, 0, 2(, 3)

# (filter, largest step, source shifts, destination shifts)
UNSHIFTED = [(name, step, None, None) for name, step in (
    ("YUV420P8", 2), ("RGBP8", 3), ("RGBAP8", 4),
    ("YUV420P16", 2), ("RGBP16", 3), ("RGBAP16", 4), ("RGBPH", 3), ("RGBPBF", 3), ("RGBAPH", 4),
    ("YUV420PS", 2), ("RGBPS", 3), ("RGBAPS", 4))]
SHIFTED = [
    ("YUV420P10", 2, [6, 4, 2], [4, 2, 6]),          # P010: luma N = 1, chroma N = 2
    ("YUV420P12", 2, [4, 2, 3], [1, 4, 2]),          # P012
    ("YUV420P14", 2, [2, 1, 0], [1, 0, 2]),          # shift 2 is all the padding a 14-bit sample has; V (U) beside it shifts by 0
    ("RGBP10", 3, [6, 4, 2], [2, 6, 4]),
    ("RGBAP10", 4, [6, 4, 2, 0], [1, 6, 3, 5]),
]
CASES = UNSHIFTED + SHIFTED

SEEN = set()       # (direction, B, N, shifted, unit) of every complete group
SEEN_VEC = set()   # ... of those that ran with vec_pixels > 0
LONGEST = {}       # (direction, B, shifted) -> the largest vec_pixels seen


def case_id(case):
    return f"{case[0]}_step{case[1]}" + ("_shifted" if case[2] else "")


# ---- frames ---------------------------------------------------------------------------------------------------------------------------

def float_frames(fmt, sw, sh, n, seed):
    """fp32 / binary16: normal values with one NaN, one +inf and one -inf in every plane of frame 1, each plane at places of its own;
    bfloat16: finite patterns of moderate exponents with eight arbitrary 16-bit patterns in every plane of frame 1."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        frame = []
        for i, (w, h) in enumerate(fmt.plane_dims(sw, sh)):
            if fmt.bfloat16:
                v = (rng.integers(0, 2, (h, w), dtype=np.uint16) << 15) | (rng.integers(120, 132, (h, w), dtype=np.uint16) << 7) | rng.integers(0, 128, (h, w), dtype=np.uint16)
                if k == 1:
                    ys, xs = rng.integers(0, h, 8), rng.integers(0, w, 8)
                    v[ys, xs] = rng.integers(0, 1 << 16, 8, dtype=np.uint16)
                    v[(h // 2 + i) % h, (w // 3 + 5 * i) % w] = 0x7fc1 + i   # a NaN with a payload
                    v[(h // 3 + i) % h, (w // 2 + 7 * i) % w] = 0xff80       # -inf
            else:
                v = (rng.standard_normal((h, w)) * 0.5).astype(fmt.dtype)
                if k == 1:
                    v[(h // 2 + i) % h, (w // 3 + 5 * i) % w] = np.nan
                    v[(h // 3 + i) % h, (w // 2 + 7 * i) % w] = np.inf
                    v[(h // 4 + i) % h, (2 * w // 3 + 3 * i) % w] = -np.inf
            frame.append(v)
        out.append(frame)
    return out


def source_frames(pkg, name, sw, sh, n, src_shifts):
    """(the frames as the source keeps them, the dense planes the definition says the filter reads)."""
    fmt = pkg.FORMATS[name]
    if fmt.half or fmt.bfloat16 or fmt.bits == 32:
        frames = float_frames(fmt, sw, sh, n, seed=len(name) * 100 + fmt.planes)
        return frames, frames
    vals = values(pkg, name, sw, sh, fmt.bits, n)
    if src_shifts is None:
        raw = [[p.astype(fmt.dtype) for p in planes] for planes in vals]
        return raw, raw
    raw = raw_of(vals, fmt.bits, src_shifts, dirty_seed=77)
    dense = [[p >> np.uint16(s) for p, s in zip(planes, src_shifts)] for planes in raw]
    assert any(int((p & np.uint16((1 << s) - 1)).max()) > 0 for planes in raw for p, s in zip(planes, src_shifts) if s), "the padding bits are not dirty"
    return raw, dense


# ---- the record ---------------------------------------------------------------------------------------------------------------------------

def side_groups(side, shifts):
    """What one side of a strided / shifted call leaves in the record, from the layout, the shifts and the buffers' numbers alone:
    [(n, members, shifted, unit, width, rows, pixels a lane)] in the order of each group's first plane.  A plane at step 1 without a
    shift has no stand-in and no group.  shifted is the launch's: any shift among the groups of that step.  unit: the widest of 16 / 4
    that divides the group's lowest base, its pitch and its frame stride."""
    shifts = shifts or [0] * len(side.layout)
    groups, index = [], {}
    for i, (b, chan, step) in enumerate(side.layout):
        if step == 1 and shifts[i] == 0:
            continue
        key = (b, step)
        if key not in index:
            index[key] = len(groups)
            groups.append(dict(n=step, members=0, lo=None, buf=b, dims=side.dims[i], shift=False))
        g = groups[index[key]]
        g["members"] += 1
        g["lo"] = chan if g["lo"] is None else min(g["lo"], chan)
        g["shift"] |= shifts[i] != 0
    shifted_launch = {}
    for g in groups:
        shifted_launch[g["n"]] = shifted_launch.get(g["n"], False) or g["shift"]
    out = []
    P = 16 // side.sb
    for g in groups:
        B = side.bufs[g["buf"]]
        a = (B["dev"].data_ptr() + B["lead"] + g["lo"] * side.sb) | B["pitch"] | (B["fs"] if side.n > 1 else 0)
        unit = 16 if a % 16 == 0 else 4 if a % 4 == 0 else 0
        out.append((g["n"], g["members"], int(shifted_launch[g["n"]]), unit, g["dims"][0], g["dims"][1], P))
    return out


def check_record(groups, src, dst, src_shifts, dst_shifts, sb, what):
    """jinc_debug_last_groups against side_groups: the source's split groups, then the destination's merge groups.  Complete groups
    move width // P * P pixels by vectors, the merge of an incomplete one none, the split of one (width - 1) // P * P."""
    want = [(SPLIT,) + g for g in side_groups(src, src_shifts)] + [(MERGE,) + g for g in side_groups(dst, dst_shifts)]
    assert len(groups) == len(want), (what, groups, want)
    for g, (direction, n, members, shifted, unit, w, h, P) in zip(groups, want):
        vec_from = w if members == n else 0 if direction == MERGE else w - 1
        vec = vec_from // P * P if unit else 0
        got = (g["direction"], g["n"], g["members"], g["sample_bytes"], g["shifted"], g["unit"], g["vec_pixels"], g["width"], g["rows"])
        assert got == (direction, n, members, sb, shifted, unit, vec, w, h), (what, g)
        assert g["scaled"] == 0, (what, g)
        if members == n:
            SEEN.add((direction, sb, n, bool(shifted), unit))
            if unit:
                assert vec > 0, (what, g)
                SEEN_VEC.add((direction, sb, n, bool(shifted), unit))
                key = (direction, sb, bool(shifted))
                LONGEST[key] = max(LONGEST.get(key, 0), vec)
    return want


def launches(want, direction):
    return len({n for (d, n, *_) in want if d == direction})


# ---- one call -----------------------------------------------------------------------------------------------------------------------------

def widen_bytes(frames):
    """(assert_bits_equal compares 2- and 4-byte samples: bytes go up to 16-bit words, value for value)"""
    return [[p.astype(np.uint16) if p.dtype == np.uint8 else p for p in planes] for planes in frames]


def run_call(torch, f, raw, want, src_layout, dst_layout, src_shifts, dst_shifts, src_align, dst_align, what, **side_kw):
    """One strided (no shifts) or shifted call held against `want`, the planar call's planes; returns the record it was held against."""
    fmt = f.fmt
    src = Side(torch, fmt.plane_dims(f.src_w, f.src_h), fmt.dtype, src_layout, N, src_align, seed=11, **{k[4:]: v for k, v in side_kw.items() if k.startswith("src_")}).fill(raw).upload()
    dst = Side(torch, f.out_dims(), fmt.dtype, dst_layout, N, dst_align, seed=12, **{k[4:]: v for k, v in side_kw.items() if k.startswith("dst_")}).upload()
    s = torch.cuda.current_stream()
    if src_shifts is None and dst_shifts is None:
        f.process_device_strided(src.ptrs(), src.pitches(), src.steps(), src.strides(), dst.ptrs(), dst.pitches(), dst.steps(), dst.strides(), N, stream=s.cuda_stream)
    else:
        f.process_device_shifted(src.ptrs(), src.pitches(), src.steps(), src_shifts, src.strides(), dst.ptrs(), dst.pitches(), dst.steps(), dst_shifts, dst.strides(), N,
                                 stream=s.cuda_stream)
    s.synchronize()
    report, groups = f.last_strided(), f.last_groups()
    got = dst.frames_and_guards(what)
    assert_source_unchanged(src, what)
    record = check_record(groups, src, dst, src_shifts, dst_shifts, fmt.sample_bytes, what)
    assert report[:3] == (launches(record, SPLIT), launches(record, MERGE), 1), (what, report)
    if dst_shifts is not None:   # the whole word: result << shift, padding bits zero
        want = [[p << np.uint16(sft) for p, sft in zip(planes, dst_shifts)] for planes in want]
        for planes in got:
            for p, sft in zip(planes, dst_shifts):
                assert int(np.count_nonzero(p & np.uint16((1 << sft) - 1))) == 0, f"{what}: non-zero padding bits in the destination"
    assert_bits_equal(widen_bytes(got), widen_bytes(want), f.out_dims(), what + " against the planar call on numpy's planes")
    return record


def check_forms(torch, pkg, case, geom=GEOM, aligns=ALIGNS):
    name, step, src_shifts, dst_shifts = case
    sw, sh, tw, th = geom
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    layout = LAYOUTS[step][:f.fmt.planes]
    assert len(layout) == f.fmt.planes and all(members == n for n, members, _, _ in group_shapes(layout, f.out_dims()))
    raw, dense = source_frames(pkg, name, sw, sh, N, src_shifts)
    want = run_planar(torch, f, dense, N)   # the planar reference, once per case
    for align in aligns:
        what = f"{name} {sw}x{sh}->{tw}x{th} step {step} shifts {src_shifts} -> {dst_shifts} align {align}"
        record = run_call(torch, f, raw, want, layout, layout, src_shifts, dst_shifts, align, align, what)
        class_unit = align if align in (16, 4) else 4 if f.fmt.sample_bytes == 4 else 0
        assert [g[4] for g in record] == [class_unit] * len(record), (what, record)
        assert all(g[3] == int(src_shifts is not None) for g in record), (what, record)
        assert len(record) == 2 * ((2 if src_shifts else 1) if step == 2 else 1), (what, record)
    f.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_split_and_merge_forms(gpu_pkg, case):
    torch = pytest.importorskip("torch")
    check_forms(torch, gpu_pkg, case)


# ---- a second trip of the wave ---------------------------------------------------------------------------------------------------------------

LONG = [
    (("RGBP8", 3, None, None), (1046, 7, 2092, 14)),
    (("RGBP16", 3, None, None), (526, 7, 1052, 14)),
    (("RGBP10", 3, [6, 4, 2], [2, 6, 4]), (526, 7, 1052, 14)),
]


@pytest.mark.parametrize("case,geom", LONG, ids=[case_id(c) for c, _ in LONG])
def test_rows_longer_than_one_trip_of_the_wave(gpu_pkg, case, geom):
    """The docstring's long cases, at alignment 16: the split's x += 64 * P runs at B = 1 and B = 2 as well."""
    torch = pytest.importorskip("torch")
    check_forms(torch, gpu_pkg, case, geom=geom, aligns=(16,))
    sb = gpu_pkg.FORMATS[case[0]].sample_bytes
    split, merge = gpu_pkg.last_groups()
    P = 16 // sb
    assert (split["direction"], split["vec_pixels"]) == (SPLIT, geom[0] // P * P) and split["vec_pixels"] > ONE_TRIP[sb]
    assert (merge["direction"], merge["vec_pixels"]) == (MERGE, geom[2] // P * P) and merge["vec_pixels"] > ONE_TRIP[sb]


# ---- incomplete groups: what the record shows --------------------------------------------------------------------------------------------

# (id, filter, order at step 4 with three planes given, the unit at alignment 16)
INCOMPLETE = [
    ("bgrx8", "RGBP8", "BGRA", 16),
    ("bgrx16", "RGBP16", "BGRA", 16),
    # X R G B: the lowest GIVEN channel is R, one sample behind the 16-byte boundary the buffer starts on -- the group's base is
    # base + 1, + 2 or + 4 bytes, so bytes and words move sample by sample and fp32 samples by dwords
    ("xrgb8", "RGBP8", "ARGB", 0),
    ("xrgb16", "RGBP16", "ARGB", 0),
    ("xrgb32", "RGBPS", "ARGB", 4),
]


@pytest.mark.parametrize("case", INCOMPLETE, ids=[c[0] for c in INCOMPLETE])
def test_incomplete_groups_carry_the_record(gpu_pkg, case):
    """Three of four channels: the merge stores sample by sample whatever the alignment (vec_pixels 0; the X samples are guard bytes),
    the split reads whole pixels up to the last but one ((width - 1) // P * P) where the group's base allows vectors at all."""
    torch = pytest.importorskip("torch")
    _, name, order, unit = case
    sw, sh, tw, th = GEOM
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    layout = packed(order, 4, 3)
    raw, dense = source_frames(gpu_pkg, name, sw, sh, N, None)
    want = run_planar(torch, f, dense, N)
    record = run_call(torch, f, raw, want, layout, layout, None, None, 16, 16, f"{name} {order} without its fourth channel")
    P = 16 // f.fmt.sample_bytes
    split, merge = gpu_pkg.last_groups()
    assert (split["direction"], split["n"], split["members"], split["unit"], split["vec_pixels"]) == (SPLIT, 4, 3, unit, (sw - 1) // P * P if unit else 0)
    assert (merge["direction"], merge["n"], merge["members"], merge["unit"], merge["vec_pixels"]) == (MERGE, 4, 3, unit, 0)
    assert [g[4] for g in record] == [unit, unit]
    f.close()


# ---- the six forms nothing reaches -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,step", [("YUV420PS", 2), ("RGBPS", 3), ("RGBAPS", 4)])
def test_fp32_samples_off_a_dword_are_refused(gpu_pkg, name, step):
    """unit 0 needs a base, a pitch or a frame stride that is no multiple of 4; with 4-byte samples each of them is refused on either
    side, nothing is written, and the record is empty (the call reached the device check and launched nothing)."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = GEOM
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    fmt = f.fmt
    layout = LAYOUTS[step][:fmt.planes]
    src = Side(torch, fmt.plane_dims(sw, sh), fmt.dtype, layout, N, seed=41).upload()
    dst = Side(torch, f.out_dims(), fmt.dtype, layout, N, seed=42).upload()
    s = torch.cuda.current_stream()
    strided = [i for i, (b, chan, st) in enumerate(layout) if st > 1]
    good = dict(sp=src.ptrs(), spitch=src.pitches(), sfs=src.strides(), dp=dst.ptrs(), dpitch=dst.pitches(), dfs=dst.strides())
    for key, text in (("sp", "aligned to the sample size"), ("dp", "aligned to the sample size"), ("spitch", "pitch is not a multiple of the sample size"),
                      ("dpitch", "pitch is not a multiple of the sample size"), ("sfs", "frame stride is not a multiple of the sample size"),
                      ("dfs", "frame stride is not a multiple of the sample size")):
        a = dict(good)
        a[key] = [v + 2 if i in strided else v for i, v in enumerate(good[key])]
        with pytest.raises(gpu_pkg.JincError) as e:
            f.process_device_strided(a["sp"], a["spitch"], src.steps(), a["sfs"], a["dp"], a["dpitch"], dst.steps(), a["dfs"], N, stream=s.cuda_stream)
        assert e.value.code == INVALID_ARG and text in str(e.value), (key, str(e.value))
        assert f.last_groups() == [], key
    s.synchronize()
    image = dst.download()
    for b, B in dst.bufs.items():
        assert np.array_equal(image[b], B["host"]), "a refused call wrote to the destination"
    f.close()


# ---- the form set ---------------------------------------------------------------------------------------------------------------------------------

def all_forms():
    forms = set()
    for direction in (SPLIT, MERGE):
        for n in (2, 3, 4):
            for sb in (1, 2, 4):
                forms.add((direction, sb, n, False))
        for n in (1, 2, 3, 4):
            forms.add((direction, 2, n, True))
    return forms


def test_zz_every_form_ran_in_every_access_class():
    """Must run after the tests above (it does in file order): every form of launch_by_shape was seen as a complete group with
    vec_pixels > 0 through 16-byte accesses and through dwords, every form but the B = 4 ones sample by sample, and every
    (direction, B, shiftedness) with a row longer than one trip of the wave.  A later edit that drops a case, a Side whose numbers fall
    into another class, or a dispatch change that sends groups sample by sample, fails here."""
    forms = all_forms()
    assert len(forms) == 26
    want_vec = {form + (unit,) for form in forms for unit in (16, 4)}
    want_zero = {form + (0,) for form in forms if form[1] != 4}
    assert len(want_vec) == 52 and len(want_zero) == 20
    assert SEEN, "no form test ran in this session: run the whole file"
    seen_zero = {x for x in SEEN if x[4] == 0}
    print(f"{len(SEEN_VEC)} form / unit pairs seen with vec_pixels > 0, {len(seen_zero)} at unit 0 (6 of the 26 are unreachable: B = 4), longest rows {sorted(LONGEST.items())}")
    missing = sorted(want_vec - SEEN_VEC)
    assert not missing, f"{len(missing)} forms never ran on vectors (direction, B, N, shifted, unit): {missing}"
    assert SEEN_VEC == want_vec, sorted(SEEN_VEC - want_vec)
    assert seen_zero == want_zero, (sorted(want_zero - seen_zero), sorted(seen_zero - want_zero))
    for direction in (SPLIT, MERGE):
        for sb, shifted in ((1, False), (2, False), (2, True), (4, False)):
            assert LONGEST.get((direction, sb, shifted), 0) > ONE_TRIP[sb], (direction, sb, shifted, LONGEST)
