"""Half-precision (binary16) planes on EVERY kernel form, against their definition (tests/test_half_planes.py):
oracle_fp32(src.astype(float32)).astype(float16), bit for bit, NaN positions compared.  tests/test_half_planes.py reaches the
automatic choice, the gather kernel and the full window only; here every form that has a half_t instantiation of its own is forced
the way its own test file forces it for integer / fp32 planes, on the YH / YUV...PH / RGBPH twin of cases that file already holds.

Every case makes two comparisons: the half filter's result against the definition, and against the fp32 filter of the same geometry
(Y32 for YH, ...PS for ...PH), forced the same way, fed the widened samples, its result narrowed with numpy.  The first failing alone
says "the form differs from the oracle for fp32 planes too at this shape"; a failure of the second says "the half instantiation does
not compute what the fp32 one computes".

Reaching a form is asserted, never assumed: half planes take the decisions of fp32 planes of the same geometry (dispatch.cpp, rule_sb),
so the half filter must have run the form exactly when the fp32 twin did -- with the twin's instance, `float` replaced by `_Float16`,
and the twin's border kernels.  A case skips only where the twin does not reach the form either.  The periodic family and the
row-pair kernel name their sample type in last_instance; the other launchers (quasi-periodic, direct, runs, frame-lane family, strip,
column-pair, colstrip) record their plain name, which is compared as it is: there the bits of the `wide` sample set are what tells a
half_t instance from a uint16_t one.

Sample sets: `unit` (the LCG frame in [0, 1]), `wide` (test_half_planes.wide_frame: the whole finite range, a quarter at 65504, a
quarter subnormal) and, for the border forms, `noise` (both signs, +-inf and two NaN patterns inside the first / last fs source
rows and columns of the last frame).  The first test needs no GPU: it holds the case lists to what they claim."""
import re

import numpy as np
import pytest

from conftest import oracle_kwargs, to_device, to_host
from test_direct_runs import RUN_CASES, RUNS
from test_float_trim_paths import _padded_runner, _put
from test_framelane_pair import _run_batch
from test_gpu_parity import DIRECT_CASES, WALK_CASES, _random_case, _random_case_v2, _random_case_v3
from test_half_planes import assert_half_equal, definition, fp32_name, unit_frame, wide_frame

gpu = pytest.mark.gpu
H, F = "_Float16", "float"


def half_name(name):
    """The half format that stands for a format of the integer / fp32 case lists: Y* -> YH, RGBP* -> RGBPH, YUV420P* -> YUV420PH ..."""
    m = re.fullmatch(r"(Y|RGBP|RGBAP|YUVA?4\d\dP)(\d+|S)", name)
    assert m, name
    return "YH" if m.group(1) == "Y" else m.group(1) + "H"


def _half_case(c):
    return (half_name(c[0]),) + tuple(c[1:6])


def _cid(c):
    extra = "_".join(f"{k}{v}" for k, v in c[5].items() if k in ("tap", "cplace", "src_left"))
    return f"{c[0]}_{c[1]}x{c[2]}to{c[3]}x{c[4]}" + (f"_{extra}" if extra else "")


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
# Every list: (format, src_w, src_h, dst_w, dst_h, arguments, what the plan must be).  "What the plan must be" is checked on the host by
# test_half_form_cases_are_what_they_claim: ("periodic", (px, py, sx, sy) or None, fs), ("quasi", (qpx, qpy, qsx, qsy) or None, fs),
# ("quasi+periodic", ...) for 4/3x, ("none", None, fs).  Group 6's plans are not exactly periodic; two of its five geometries (5/6 and 15/8)
# have affine window origins all the same, which the batch rules leave to the frame-lane family below 128 frames.

# 1. the periodic family at integer ratios (tests/test_gpu_parity.py::test_kernel_variants_match_oracle, test_rowpair.py)
G1_TAP3 = [
    ("YH", 333, 211, 666, 422, {}, ("periodic", (2, 2, 1, 1), 7)),       # odd width: rows end in the low half of a dword, ragged tiles
    ("YH", 200, 150, 400, 300, {}, ("periodic", (2, 2, 1, 1), 7)),
    ("YUV420PH", 258, 130, 516, 260, {}, ("periodic", (2, 2, 1, 1), 7)),  # chroma 129 wide
    ("YH", 100, 80, 400, 320, {}, ("periodic", (4, 4, 1, 1), 7)),        # 4x
]
G1_MODES = {2: "window", 3: "rows", 4: "window_rg4", 5: "packed_rg4", 6: "packed_rg8", 13: "quad", 15: "full_window", 9: "direct"}
G1_TAP4 = [
    ("YH", 200, 120, 400, 240, dict(tap=4), ("periodic", (2, 2, 1, 1), 9)),
    ("RGBPH", 131, 77, 262, 154, dict(tap=4), ("periodic", (2, 2, 1, 1), 9)),
]
G1_TAP2 = ("YH", 150, 100, 300, 200, dict(tap=2), ("periodic", (2, 2, 1, 1), 5))
G1_ROWPAIR = [
    ("YH", 160, 120, 320, 240, dict(tap=6), ("periodic", (2, 2, 1, 1), 13)),
    ("YH", 160, 120, 320, 240, dict(tap=8), ("periodic", (2, 2, 1, 1), 17)),
]


def _periodic_pattern(mode, fs, knobs):
    """The instance a forced kernel mode must give on an fp32 plane ({T}: the sample type), from dispatch.cpp's launch_plane."""
    if mode == 2:
        return r"ewa_periodic_kernel<{T}, \d+, \d+>"
    if mode == 3:
        return r"ewa_periodic_rows_kernel<{T}, \d+, \d+>"
    if mode == 4:   # half-height tiles: four row groups
        return r"ewa_periodic_kernel<{T}, \d+, 4>"
    if mode in (5, 6):
        return r"ewa_periodic_pk_kernel<{T}, 7, \d+>"
    if mode == 13:
        if fs == 9:
            return r"ewa_periodic_quad2x8_kernel<{T}, .*>" if knobs.get("quad2x8") else r"ewa_periodic_quad8_kernel<{T}, .*>"
        return r"ewa_periodic_quad\w*_kernel<{T}, .*>"
    if mode == 15:   # the automatic choice on the reference's full window: the window kernel, or on small calls of fs 9 its quad form
        return rf"ewa_periodic_kernel<{{T}}, {fs}, \d+>|ewa_periodic_quad9_kernel<{{T}}, \d+>" if fs == 9 else rf"ewa_periodic_kernel<{{T}}, {fs}, \d+>"
    assert mode == 9
    return "ewa_direct_kernel"


# 2. the quasi-periodic kernel (test_gpu_parity.py QUASI_CASES)
G2 = [
    ("YH", 320, 180, 480, 270, {}, ("quasi", (3, 3, 2, 2), 7)),
    ("YH", 211, 97, 633, 291, {}, ("quasi", (3, 3, 1, 1), 7)),               # 3x, odd width
    ("YH", 150, 120, 225, 180, dict(tap=4), ("quasi", (3, 3, 2, 2), 9)),
    ("YH", 240, 160, 640, 360, {}, ("quasi", (8, 9, 3, 4), 7)),              # 8/3 x 9/4
    ("YH", 360, 270, 480, 360, {}, ("quasi+periodic", (4, 4, 3, 3), 7)),     # 4/3x: exactly periodic at source step 3
    ("YUV420PH", 256, 144, 384, 216, {}, ("quasi", (3, 3, 2, 2), 7)),
]
G2_MODES = {7: "quasi", 8: "quasi_waterfall", 10: "quasi_lane_coefficients", 0: "auto", 1: "gather"}

def _unique(cases):
    """Two integer cases of one geometry are one half case."""
    out = []
    for c in cases:
        if c not in out:
            out.append(c)
    return out


# 3. the direct kernel: test_gpu_parity.py DIRECT_CASES (those the issue names) and every row of WALK_CASES, as half planes
_DIRECT_PICK = [(384, 216, 192, 108), (384, 216, 128, 72), (384, 216, 256, 144), (400, 300, 200, 100), (300, 200, 100, 50), (1100, 100, 550, 50),
                (300, 200, 600, 400), (200, 120, 400, 240), (160, 100, 640, 400), (128, 128, 128, 128), (256, 144, 128, 72)]
G3_DIRECT = _unique([_half_case(c) + (("periodic", c[6], None),) for c in DIRECT_CASES if tuple(c[1:5]) in _DIRECT_PICK])
# two more rows so that every source step has a single-step row (fs 9 .. 16) and a two-step row (fs 17 .. 32) on the row walk
G3_WALK = _unique([_half_case(c) + (("periodic", None, None),) for c in WALK_CASES]) + [
    ("YH", 150, 110, 300, 220, dict(tap=6), ("periodic", (2, 2, 1, 1), 13)),   # source step 1, single-step row
    ("YH", 404, 220, 101, 55, dict(tap=2), ("periodic", (1, 1, 4, 4), 18)),    # source step 4, two-step row
]

# 4. the runs form (test_direct_runs.py RUN_CASES without the full-size one)
# ... and without 322 x 182 with blur and quantisation, whose plan is exactly periodic on this build (no runs for any sample type)
G4 = _unique([_half_case(c) + (("runs", None, None),) for c in RUN_CASES if c[1] <= 640 and "blur" not in c[5]])

# 5. border forms
G5_STRIP = [   # test_strip_kernel.py: filter sizes 5 / 7 / 9 at source step 1
    ("YH", 192, 108, 384, 216, dict(tap=3), ("periodic", (2, 2, 1, 1), 7)),
    ("YH", 333, 211, 666, 422, dict(tap=3), ("periodic", (2, 2, 1, 1), 7)),
    ("YH", 150, 100, 300, 200, dict(tap=4), ("periodic", (2, 2, 1, 1), 9)),
    ("YH", 150, 100, 300, 200, dict(tap=2), ("periodic", (2, 2, 1, 1), 5)),
    ("YH", 131, 77, 262, 154, dict(tap=4, blur=0.98), ("periodic", (2, 2, 1, 1), 9)),
    # (column groups of 6 + 6 and 8 + 8 output columns: with the odd widths of the unshifted cases every residue mod 4.  3x -- test_strip_kernel.py's
    # 97 x 61 -- has a periodic interior but private border sets on this build: no strip border for any sample type)
    ("YH", 192, 108, 384, 216, dict(tap=3, src_left=0.5, src_top=0.5), ("periodic", (2, 2, 1, 1), 7)),
    ("YH", 192, 108, 384, 216, dict(tap=4, src_left=0.5), ("periodic", (2, 2, 1, 1), 9)),
    ("YH", 96, 64, 384, 256, dict(tap=3), ("periodic", (4, 4, 1, 1), 7)),
    ("YUV420PH", 256, 144, 512, 288, dict(tap=3), ("periodic", (2, 2, 1, 1), 7)),
]   # (test_strip_kernel.py's cropped case is not exactly periodic on this build: it has no strip border for any sample type)
G5_COLPAIR = [   # test_colpair.py's Y32 / RGBPS cases
    ("YH", 160, 100, 320, 200, dict(tap=6), ("periodic", (2, 2, 1, 1), 13)),
    ("RGBPH", 131, 77, 262, 154, dict(tap=5), ("periodic", (2, 2, 1, 1), 11)),
    ("YH", 150, 100, 300, 200, dict(tap=4, blur=0.98), ("periodic", (2, 2, 1, 1), 9)),
]
G5_ROWPAIR_ROWS = [   # test_rowpair_rows.py: taps 5 .. 8
    ("RGBPH", 131, 77, 262, 154, dict(tap=5), ("periodic", (2, 2, 1, 1), 11)),
    ("YH", 160, 100, 320, 200, dict(tap=6), ("periodic", (2, 2, 1, 1), 13)),
    ("YH", 263, 151, 526, 302, dict(tap=7), ("periodic", (2, 2, 1, 1), 15)),
    ("YH", 333, 111, 666, 222, dict(tap=8), ("periodic", (2, 2, 1, 1), 17)),
]
G5_COLSTRIP = [("YH", 192, 108, 384, 216, dict(tap=3), ("periodic", (2, 2, 1, 1), 7)),
               ("Y32", 192, 108, 384, 216, dict(tap=3), ("periodic", (2, 2, 1, 1), 7)),
               ("Y8", 192, 108, 384, 216, dict(tap=3), ("periodic", (2, 2, 1, 1), 7))]
G5_EDGE = [("YH", 192, 108, 384, 216, dict(tap=3), ("periodic", (2, 2, 1, 1), 7)),
           ("YH", 192, 108, 384, 216, dict(tap=4), ("periodic", (2, 2, 1, 1), 9))]

# 6. batch forms (test_framelane_sub.py's geometries)
G6 = [
    ("YH", 160, 90, 219, 123, {}, ("none", None, 7)),
    ("YH", 192, 108, 160, 90, {}, ("quasi", (5, 5, 6, 6), 8)),               # (affine origins, 25 phases: not exactly periodic)
    ("YH", 128, 72, 240, 135, dict(tap=4), ("quasi", (15, 15, 8, 8), 9)),
    ("YUV420PH", 160, 96, 222, 130, dict(cplace="topleft"), ("none", None, 7)),
    ("YH", 37, 29, 51, 40, {}, ("none", None, 7)),
]
G6_SUB_N = [2, 3, 7, 9, 16, 17, 31, 33, 50, 63]
G6_AUTO_N = [48, 49, 64, 70, 128, 192]

ALL_GROUPS = {1: G1_TAP3 + G1_TAP4 + [G1_TAP2] + G1_ROWPAIR, 2: G2, 3: G3_DIRECT + G3_WALK, 4: G4,
              5: G5_STRIP + G5_COLPAIR + G5_ROWPAIR_ROWS + G5_COLSTRIP + G5_EDGE, 6: G6}


# ---- the CPU half ---------------------------------------------------------------------------------------------------------------------

def _column_groups(f):
    """Border columns of table 0 as ewa_strip_kernel groups them (device_plan.cpp: consecutive columns with one window origin)."""
    info = f.plan_info(0)
    sx, _, _ = f.plan_dump(0)
    out = []
    for a, b in ((0, info.interior_x0), (info.interior_x1, info.dst_width)):
        x = a
        while x < b:
            m = x
            while m < b and sx[m] == sx[x]:
                m += 1
            out.append(m - x)
            x = m
    return out


def test_half_form_cases_are_what_they_claim(pkg, O):
    """Host-only plans of every case of groups 1 .. 6: the oracle accepts the geometry and the plan has the structure the group's
    kernels need; the walk cases give every source step a single-step and a two-step row; the strip cases' column groups have
    every residue mod 4 (packed 4-sample store and the sample-by-sample tail); and per group the definition's result for the `wide`
    set of one case holds +-inf and subnormals, i.e. the narrowing edges are in the expected values."""
    walk = {}
    residues = set()
    for group, cases in ALL_GROUPS.items():
        for c in cases:
            name, sw, sh, tw, th, kw, (kind, period, fs) = c
            oname = name if name in ("Y32", "Y8") else fp32_name(name)
            of = O.OracleFilter(O.FORMATS[oname], sw, sh, tw, th, **oracle_kwargs(kw))
            f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1, **kw)
            info = f.plan_info(0)
            what = f"group {group} {_cid(c)}"
            assert info.filter_size == of.tables[0].filter_size, what
            if fs is not None:
                assert info.filter_size == fs, (what, info.filter_size)
            q = (info.quasi_period_x, info.quasi_period_y, info.quasi_step_x, info.quasi_step_y)
            p = (info.period_x, info.period_y, info.step_x, info.step_y)
            if kind == "periodic":
                assert info.periodic == 1, what
                assert period is None or p == period, (what, p)
            elif kind == "quasi":
                assert (info.quasi, info.periodic) == (1, 0), what
                assert period is None or q == period, (what, q)
            elif kind == "quasi+periodic":
                assert (info.quasi, info.periodic) == (1, 1) and q == period and p == period, (what, q, p)
            elif kind == "runs":
                assert (info.quasi, info.periodic) == (1, 0), what
                runs, items = f.plan_runs(0)
                assert len(runs) > 0 and items > 0 and info.filter_size >= 9, what
            else:
                assert kind == "none" and (info.quasi, info.periodic) == (0, 0), (what, info.quasi, info.periodic)
            if c in G3_WALK:
                walk.setdefault(info.step_x, set()).add(info.filter_size)
            if c in G5_STRIP:
                residues |= {n % 4 for n in _column_groups(f)}
            f.close()
    for sx in (1, 2, 3, 4):   # kernel_direct_impl.inc walk_steps: one step up to 16 taps, two up to 32
        assert any(9 <= fs <= 16 for fs in walk[sx]) and any(17 <= fs <= 32 for fs in walk[sx]), (sx, sorted(walk[sx]))
    assert residues == {0, 1, 2, 3}, residues
    for group, c in ((1, G1_TAP3[1]), (2, G2[0]), (3, G3_DIRECT[0]), (4, G4[0]), (5, G5_STRIP[0]), (6, G6[0])):
        src = wide_frame(pkg, c[0], c[1], c[2], 4242)
        bits = definition(O, c[0], c[1], c[2], c[3], c[4], c[5], src)[0][:c[4], :c[3]].view(np.uint16) & 0x7fff
        assert (bits == 0x7c00).any() and ((bits > 0) & (bits < 0x0400)).any(), f"group {group} {_cid(c)}: no overflow / no subnormal result"


def test_run_batch_round_trips_half_planes():
    """tests/test_framelane_pair._run_batch carries 2-byte samples as torch.int16 / the frames' own dtype and views the result with
    the frames' dtype: for float16 that must be a bit view, never a value conversion."""
    torch = pytest.importorskip("torch")
    bits = np.arange(0, 1 << 16, dtype=np.uint16).reshape(256, 256)   # every binary16 pattern, NaN payloads included
    a = bits.view(np.float16)
    t = torch.from_numpy(np.ascontiguousarray(a))
    assert t.dtype == torch.float16
    back = torch.stack([t, t])[1].numpy()
    assert np.array_equal(back.view(np.uint16), bits)
    as_int16 = torch.zeros((256, 256), dtype=torch.int16)
    as_int16.copy_(t.view(torch.int16))
    assert np.array_equal(as_int16.numpy().view(np.float16).view(np.uint16), bits)


@gpu
def test_device_copies_round_trip_half_planes(gpu_pkg):
    """... and the copies _run_batch makes (conftest.to_device / to_host, through pinned memory) keep every pattern too."""
    torch = pytest.importorskip("torch")
    bits = np.arange(0, 1 << 16, dtype=np.uint16).reshape(256, 256)
    t = to_device(torch.stack([torch.from_numpy(bits.view(np.float16))]))
    assert np.array_equal(to_host(t[0]).numpy().view(np.uint16), bits)
    assert np.array_equal(to_host(t.view(torch.int16)[0]).numpy().view(np.float16).view(np.uint16), bits)


# ---- shared machinery of the GPU half --------------------------------------------------------------------------------------------------

_FRAMES = {}   # (case, samples[, n]) -> (frames, the definition's planes per frame): the oracle runs once per geometry, not per mode
_SEEN = {}     # group -> {instance or kernel name of the half filter: cases}
_WALKS = set()  # (source step, filter size, DirectShape, base) of the half direct-kernel calls
_STRIP_RESIDUES = set()  # column group sizes mod 4 of the cases that ran ewa_strip_kernel


def _key(case):
    return (case[0], case[1], case[2], case[3], case[4], tuple(sorted(case[5].items())))


def _noise_frame(pkg, hname, sw, sh, rng, non_finite):
    out = []
    for (pw, ph) in pkg.FORMATS[hname].plane_dims(sw, sh):
        p = pkg.alloc_plane(pw, ph, np.float16)
        p[...] = (rng.standard_normal(p.shape) * 0.8).astype(np.float16)
        out.append(p)
    if non_finite:   # bit patterns of test_float_trim_paths._put: +inf, 0x7c01, -inf, quiet NaN
        _put(out[0], sh // 3, 1, 0)
        _put(out[0], sh // 2, sw - 2, 3)
        _put(out[0], 1, sw // 3, 1)
        _put(out[0], sh - 2, sw // 2, 2)
    return out


def _frames(pkg, O, case, samples, n=1):
    hname, sw, sh, tw, th, kw = case[:6]
    if samples == "noise":
        key = (_key(case), samples, n)
        if key not in _FRAMES:
            rng = np.random.default_rng(6)
            srcs = [_noise_frame(pkg, hname, sw, sh, rng, k == n - 1) for k in range(n)]
            wants = [definition(O, hname, sw, sh, tw, th, kw, s) for s in srcs]
            assert np.isnan(wants[-1][0]).any() and np.isinf(wants[-1][0]).any()
            _FRAMES[key] = (srcs, wants)
        return _FRAMES[key]
    srcs, wants = _FRAMES.setdefault((_key(case), samples), ([], []))
    while len(srcs) < n:
        k = len(srcs)
        src = unit_frame(O, hname, sw, sh, 4242 + k) if samples == "unit" else wide_frame(pkg, hname, sw, sh, 4242 + k)
        srcs.append(src)
        wants.append(definition(O, hname, sw, sh, tw, th, kw, src))
    return srcs[:n], wants[:n]


def _widen(srcs):
    return [[np.ascontiguousarray(p.astype(np.float32)) for p in s] for s in srcs]


def _narrow(planes):
    with np.errstate(over="ignore"):
        return [np.ascontiguousarray(p).astype(np.float16) for p in planes]


def _call(pkg, torch, f, srcs, mode=0, strips=None, knobs=None):
    if strips is not None:
        f.set_border_strips(strips)
    with pkg.knobs(**(knobs or {})):
        if len(srcs) == 1:
            f.set_kernel_mode(mode)
            return [f.get_frame(srcs[0])]
        return _run_batch(torch, pkg, f, f.fmt, srcs, len(srcs), mode)


def _state(f):
    return [(f.last_instance(t), f.last_kernel(t), f.last_border(t)) for t in range(f.num_tables)]


def _as_half(state):
    return [(i.replace("<" + F, "<" + H), k, b) for (i, k, b) in state]


def _note(group, state, what):
    for inst, _, border in state:
        _SEEN.setdefault(group, {}).setdefault(f"{inst} [border {border}]", []).append(what)
    print(f"half form, group {group}: {what}: " + "; ".join(f"{i} [border {b}]" for i, _, b in state))


def _compare(got_h, wants, got_f, dims, what):
    """Both comparisons of one call; the message says which of them failed."""
    errors = []
    for k in range(len(got_h)):
        for name, want in (("the definition", wants[k]), ("the fp32 twin, narrowed", _narrow(got_f[k]))):
            try:
                assert_half_equal(got_h[k], want, dims, what=f"{what} frame {k} vs {name}")
            except AssertionError as e:
                errors.append(str(e))
    if errors:
        sides = {("definition" in e, "twin" in e) for e in errors}
        verdict = "the half instantiation differs from fp32" if any(t for _, t in sides) else "the fp32 form gives the same bits: the form itself differs from the oracle"
        raise AssertionError(f"{verdict}\n" + "\n".join(errors[:6]))


def _twins(pkg, case):
    hname, sw, sh, tw, th, kw = case[:6]
    return (pkg.Filter(pkg.FORMATS[hname], sw, sh, tw, th, device=0, **kw),
            pkg.Filter(pkg.FORMATS[fp32_name(hname)], sw, sh, tw, th, device=0, **kw))


def _fold_shape(state):
    """ewa_framelane_win1k_kernel is ewa_framelane_win_kernel's 1024-thread shape (one body: kernel_framelane_win_body.inc).  Which of
    the two runs follows from the LDS tile framelane_configure finds, and a tile of binary16 samples is half the bytes of an fp32 one:
    that choice is the one thing a half filter does not share with its fp32 twin, by design.  Both shapes must occur (last test)."""
    return [(i.replace("win1k", "win"), k.replace("win1k", "win"), b) for (i, k, b) in state]


def _check_form(pkg, O, group, case, samples, reached, what, n=1, run=None, fold=lambda state: state, **force):
    """One case: the half filter and its fp32 twin under the same forcing; `reached(state, T)` says whether the form under test ran
    with sample type T.  Returns the half filter's results."""
    torch = pytest.importorskip("torch")
    srcs, wants = _frames(pkg, O, case, samples, n)
    run = run or (lambda f, s: _call(pkg, torch, f, s, **force))
    fh, ff = _twins(pkg, case)
    try:
        got_f = run(ff, _widen(srcs))
        state_f = _state(ff)
        got_h = run(fh, srcs)
        state_h = _state(fh)
        if not reached(state_f, F):
            assert not reached(state_h, H), f"{what}: the fp32 twin did not reach the form ({state_f}) but the half filter did ({state_h})"
            pytest.skip(f"the fp32 twin does not reach the form either: {state_f}")
        assert reached(state_h, H), f"{what}: the fp32 twin reached the form ({state_f}), the half filter ran {state_h}"
        assert fold(state_h) == fold(_as_half(state_f)), f"{what}: half {state_h}, fp32 twin {state_f}"
        _note(group, state_h, what)
        _compare(got_h, wants, got_f, fh.out_dims(), what)
        return got_h
    finally:
        fh.close()
        ff.close()


def _instance(pattern):
    return lambda state, T: re.fullmatch(pattern.replace("{T}", T), state[0][0]) is not None


def _kernel(name):
    return lambda state, T: state[0][1] == name and state[0][0] == name


def _border(bits, none_of=0):
    return lambda state, T: state[0][2] & bits == bits and state[0][2] & none_of == 0


SAMPLES = ["unit", "wide"]
BORDER_SAMPLES = ["unit", "wide", "noise"]


# ---- 1. periodic variants ---------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("mode", sorted(G1_MODES), ids=[G1_MODES[m] for m in sorted(G1_MODES)])
@pytest.mark.parametrize("case", G1_TAP3, ids=_cid)
def test_periodic_variants_tap3(gpu_pkg, O, case, mode, samples):
    _check_form(gpu_pkg, O, 1, case, samples, _instance(_periodic_pattern(mode, 7, {})), f"{_cid(case)} mode {mode} {samples}", mode=mode)


@gpu
@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("two", [0, 1], ids=["quad2x8_0", "quad2x8_1"])
@pytest.mark.parametrize("mode", [2, 13, 15], ids=["window", "quad", "full_window"])
@pytest.mark.parametrize("case", G1_TAP4, ids=_cid)
def test_periodic_variants_tap4(gpu_pkg, O, case, mode, two, samples):
    knobs = dict(quad2x8=two)
    _check_form(gpu_pkg, O, 1, case, samples, _instance(_periodic_pattern(mode, 9, knobs)), f"{_cid(case)} mode {mode} quad2x8={two} {samples}",
                mode=mode, knobs=knobs)


@gpu
@pytest.mark.parametrize("samples", SAMPLES)
def test_periodic_rows_kernel_tap2(gpu_pkg, O, samples):
    _check_form(gpu_pkg, O, 1, G1_TAP2, samples, _instance(_periodic_pattern(3, 5, {})), f"{_cid(G1_TAP2)} mode 3 {samples}", mode=3)


@gpu
@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("lw", [0, 64, 32, 16], ids=["auto", "256x16", "128x32", "64x64"])
@pytest.mark.parametrize("case", G1_ROWPAIR, ids=_cid)
def test_rowpair_form(gpu_pkg, O, case, lw, samples):
    pattern = r"ewa_periodic_rowpair_kernel<{T}, \d+, " + (str(lw) if lw else r"\d+") + r", \d+>"
    _check_form(gpu_pkg, O, 1, case, samples, _instance(pattern), f"{_cid(case)} rows_pair={lw} {samples}", mode=0,
                knobs={"rows_pair": lw} if lw else {})


# ---- 2. the quasi-periodic kernel -------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("mode", sorted(G2_MODES), ids=[G2_MODES[m] for m in sorted(G2_MODES)])
@pytest.mark.parametrize("case", G2, ids=_cid)
def test_quasi_periodic_kernel(gpu_pkg, O, case, mode, samples):
    """Modes 7 / 8 / 10 must run ewa_quasi_kernel; 0 and 1 are there for agreement (whatever the twin runs: the gather kernel)."""
    reached = _kernel("ewa_quasi_kernel") if mode in (7, 8, 10) else (lambda state, T: True)
    _check_form(gpu_pkg, O, 2, case, samples, reached, f"{_cid(case)} mode {mode} {samples}", mode=mode)


@gpu
@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("split", [1, 2])
def test_quasi_periodic_kernel_with_split_phases(gpu_pkg, O, split, samples):
    """A tile's phases split over workgroups (what small calls do under the automatic choice), by the knob."""
    _check_form(gpu_pkg, O, 2, G2[0], samples, _kernel("ewa_quasi_kernel"), f"{_cid(G2[0])} quasi_split={split} {samples}", mode=7,
                knobs=dict(quasi_split=split))


# ---- 3. the direct kernel ---------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("mode", [9, 0], ids=["direct", "auto"])
@pytest.mark.parametrize("case", G3_DIRECT, ids=_cid)
def test_direct_kernel(gpu_pkg, O, case, mode, samples):
    reached = _kernel("ewa_direct_kernel") if mode == 9 else (lambda state, T: True)
    _check_form(gpu_pkg, O, 3, case, samples, reached, f"{_cid(case)} mode {mode} {samples}", mode=mode)


# (three planes go through get_frame, base 0 only; the one-plane cases take both bases)
WALK_RUNS = [(c, b) for c in G3_WALK for b in (0, 2) if b == 0 or c[0] == "YH"]


@gpu
@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("case,base", WALK_RUNS, ids=[f"{_cid(c)}-base{b}" for c, b in WALK_RUNS])
def test_direct_kernel_row_walk(gpu_pkg, O, case, base, samples):
    """Kernel mode 9 on every row of WALK_CASES.  The instance name does not carry the byte shift SH of a lane's first sample: it is
    (2 * start_x[phase] + plane base) & 3 (kernel_direct_impl.inc), the same for all lanes of a phase, and a plan with one column
    phase has one shift only.  So every one-plane case runs twice from device memory: with the plane's base on a dword and 2 bytes
    behind one, which swaps half_lo and half_hi for every phase -- both shifts occur for every source step and filter size.  The
    buffer around the plane holds 0xFF bytes (NaN): a sample fetched from outside the plane shows."""
    torch = pytest.importorskip("torch")
    hname, sw, sh = case[0], case[1], case[2]
    planes = gpu_pkg.FORMATS[hname].planes
    shapes = []

    def run(f, srcs):
        sb = np.dtype(f.fmt.dtype).itemsize
        if planes > 1:
            out = _call(gpu_pkg, torch, f, srcs, mode=9)
        else:   # rows and frames a multiple of 4 bytes apart (the direct kernel's premise), the base `base` bytes behind a dword
            out = _padded_runner(sw, sh, 64 + (base if sb == 2 else 0), (-sw * sb) % 4 + 4, 8)(torch, gpu_pkg, f, f.fmt, srcs, 1, 9)
        shapes.append(gpu_pkg.last_direct_shape())
        return out

    _check_form(gpu_pkg, O, 3, case, samples, _kernel("ewa_direct_kernel"), f"{_cid(case)} base {base} {samples}", run=run)
    assert shapes[0] == shapes[1], f"DirectShape: fp32 twin {shapes[0]}, half {shapes[1]}"
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[hname], *case[1:5], device=-1, **case[5])
    info = f.plan_info(0)
    f.close()
    _WALKS.add((info.step_x, info.filter_size, shapes[1], base))
    print(f"half form, group 3: {_cid(case)}: source step {info.step_x}, fs {info.filter_size}, DirectShape {shapes[1]}, base {base}")


# ---- 4. the runs form -------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("case", G4, ids=_cid)
def test_runs_form(gpu_pkg, O, case, samples):
    _check_form(gpu_pkg, O, 4, case, samples, _kernel(RUNS), f"{_cid(case)} mode 14 {samples}", mode=14)


@gpu
@pytest.mark.parametrize("samples", SAMPLES)
def test_runs_form_falls_back_to_gather_on_a_pitch_that_is_no_multiple_of_4_bytes(gpu_pkg, O, samples):
    """test_direct_runs.py's pitch case for 2-byte float samples: 202 samples a row, five frames; rows 404 bytes apart run the runs form,
    rows 406 bytes apart (a multiple of the sample size only) cannot be fetched as aligned dwords: the gather kernel, same bits."""
    torch = pytest.importorskip("torch")
    case = ("YH", 202, 120, 303, 180, dict(tap=6))
    n = 5
    srcs, wants = _frames(gpu_pkg, O, case, samples, n)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YH"], *case[1:5], device=0, **case[5])
    assert f.plan_info().quasi == 1 and f.plan_info().periodic == 0
    outs = {}
    for extra, kernel in ((0, RUNS), (2, "ewa_gather_kernel"), (4, RUNS)):
        outs[extra] = _padded_runner(202, 120, 0, extra, 0)(torch, gpu_pkg, f, f.fmt, srcs, n, 14)
        assert f.last_kernel(0) == kernel, (extra, f.last_kernel(0))
        for k in range(n):
            assert_half_equal(outs[extra][k], wants[k], f.out_dims(), what=f"pitch {404 + extra} frame {k} ({kernel})")
    f.close()


# ---- 5. border forms --------------------------------------------------------------------------------------------------------------------

def _border_case(pkg, O, case, samples, n, reached, what, strips, knobs=None, mode=0, others=()):
    """The form's border (`strips`, `knobs`) through _check_form; then the same half frames under every (strips, knobs) of `others` --
    the gather kernel's border (0) among them -- must give the same bits."""
    torch = pytest.importorskip("torch")
    got = _check_form(pkg, O, 5, case, samples, reached, what, n=n, mode=mode, strips=strips, knobs=knobs)
    srcs, _ = _frames(pkg, O, case, samples, n)
    f = pkg.Filter(pkg.FORMATS[case[0]], *case[1:5], device=0, **case[5])
    try:
        for o_strips, o_knobs, must_not in others:
            other = _call(pkg, torch, f, srcs, mode=mode, strips=o_strips, knobs=o_knobs)
            assert all(f.last_border(t) & must_not == 0 for t in range(f.num_tables)), (o_strips, o_knobs, [f.last_border(t) for t in range(f.num_tables)])
            if o_strips == 0:
                assert f.last_border(0) == 1, f.last_border(0)
            for k in range(n):
                assert_half_equal(got[k], other[k], f.out_dims(), what=f"{what} frame {k} vs border form {o_strips} {o_knobs}")
    finally:
        f.close()


@gpu
@pytest.mark.parametrize("samples", BORDER_SAMPLES)
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("case", G5_STRIP, ids=_cid)
def test_strip_kernel_rows_and_columns(gpu_pkg, O, case, n, samples):
    """ewa_strip_kernel over rows and columns (border strips 3; last_border bits 16 and 32).  The columns hold the packed 4-sample half
    store: the cases' column groups have every residue mod 4 (the CPU test), so both the 8-byte store and the tail run."""
    _border_case(gpu_pkg, O, case, samples, n, _border(48), f"{_cid(case)} strips 3 n={n} {samples}", 3, others=[(1, None, 0), (0, None, 0)])
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[case[0]], *case[1:5], device=-1, **case[5])
    _STRIP_RESIDUES.update(g % 4 for g in _column_groups(f))   # (of a case that did run ewa_strip_kernel: a skip does not come here)
    f.close()


@gpu
@pytest.mark.parametrize("samples", BORDER_SAMPLES)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("case", G5_COLPAIR, ids=_cid)
def test_column_pairs(gpu_pkg, O, case, n, samples):
    _border_case(gpu_pkg, O, case, samples, n, _border(256, none_of=64 | 32 | 8 | 4 | 1), f"{_cid(case)} colpair n={n} {samples}", 4,
                 knobs=dict(colpair=1), others=[(4, dict(colpair=0), 256), (0, dict(colpair=1), 0)])


@gpu
@pytest.mark.parametrize("samples", BORDER_SAMPLES)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("case", G5_ROWPAIR_ROWS, ids=_cid)
def test_border_rows_on_the_pair_kernel(gpu_pkg, O, case, n, samples):
    _border_case(gpu_pkg, O, case, samples, n, _border(128, none_of=16 | 2), f"{_cid(case)} rowpair rows n={n} {samples}", 4,
                 others=[(4, dict(rowpair_rows=0), 128), (0, None, 0)])


# (integer planes have the LCG frame only)
COLSTRIP_RUNS = [(c, smp) for c in G5_COLSTRIP for smp in BORDER_SAMPLES if c[0] != "Y8" or smp == "unit"]


@gpu
@pytest.mark.parametrize("case,samples", COLSTRIP_RUNS, ids=[f"{_cid(c)}-{smp}" for c, smp in COLSTRIP_RUNS])
def test_colstrip_kernel(gpu_pkg, O, case, samples):
    """ewa_colstrip_kernel (last_border bit 4): the column form of border strips 1 on a single frame, where none of the newer forms is
    chosen.  For half planes with their fp32 twin; for Y32 and Y8 against the oracle, since no other test names the kernel."""
    name, sw, sh, tw, th, kw = case[:6]
    what = f"{_cid(case)} colstrip {samples}"
    if name == "YH":
        _border_case(gpu_pkg, O, case, samples, 1, _border(4 | 2, none_of=256 | 64 | 32 | 16 | 8), what, 1, others=[(0, None, 0)])
        return
    ofmt = O.FORMATS[name]
    if name == "Y8":
        src = O.lcg_frame(ofmt, sw, sh, seed=4242)
    else:
        src = _widen(_frames(gpu_pkg, O, ("YH",) + tuple(case[1:6]), samples, 1)[0])[0]
    want = O.OracleFilter(ofmt, sw, sh, tw, th, **oracle_kwargs(kw)).get_frame(src, threads=4)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[name], sw, sh, tw, th, device=0, **kw)
    try:
        f.set_border_strips(1)
        got = f.get_frame(src)
        assert f.last_border(0) & 4 and f.last_border(0) & (256 | 64 | 32 | 8) == 0, f.last_border(0)
        f.set_border_strips(0)
        gathered = f.get_frame(src)
        assert f.last_border(0) == 1
        for i, (w, h) in enumerate(f.out_dims()):
            a, b, g = got[i][:h, :w], want[i][:h, :w], gathered[i][:h, :w]
            na = np.isnan(a) if a.dtype == np.float32 else np.zeros(a.shape, bool)
            nb = np.isnan(b) if b.dtype == np.float32 else np.zeros(b.shape, bool)
            assert np.array_equal(na, nb), f"{what}: NaN footprint differs"
            assert np.array_equal(np.ascontiguousarray(a[~na]).view(np.uint8), np.ascontiguousarray(b[~nb]).view(np.uint8)), f"{what}: colstrip vs oracle"
            assert np.array_equal(np.ascontiguousarray(a[~na]).view(np.uint8), np.ascontiguousarray(g[~na]).view(np.uint8)), f"{what}: colstrip vs gather border"
    finally:
        f.close()


@gpu
@pytest.mark.parametrize("samples", BORDER_SAMPLES)
@pytest.mark.parametrize("case", G5_EDGE, ids=_cid)
def test_edge_columns_stay_integer_only(gpu_pkg, O, case, samples):
    """test_edge_columns.py's forcing (border strips 4, quad form, two periods per lane) on a half plane: the interior kernel's edge
    tiles are not configured for float planes (last_border bit 64 stays 0) and the result is still the definition's."""
    _border_case(gpu_pkg, O, case, samples, 1, lambda state, T: state[0][2] & 64 == 0, f"{_cid(case)} edge forcing {samples}", 4,
                 knobs=dict(quad2x8=1), mode=13, others=[(0, dict(quad2x8=1), 64)])


# ---- 6. batch forms ---------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("n", G6_SUB_N)
@pytest.mark.parametrize("case", G6, ids=_cid)
def test_framelane_sub_groups(gpu_pkg, O, case, n, samples):
    _check_form(gpu_pkg, O, 6, case, samples, _kernel("ewa_framelane_sub_kernel"), f"{_cid(case)} mode 16 n={n} {samples}", n=n, mode=16)


@gpu
@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("n", G6_AUTO_N)
@pytest.mark.parametrize("case", G6, ids=_cid)
def test_batches_under_the_automatic_choice(gpu_pkg, O, case, n, samples):
    """Whatever the fp32 twin runs for the batch (win / win1k, the generic frame-lane kernel, the pair form from 128 frames on), the
    half filter runs it too (_check_form compares the kernels of every table; _fold_shape: the window kernel's two launch shapes count
    as one kernel) -- and it must be one of the frame-lane family."""
    _check_form(gpu_pkg, O, 6, case, samples, lambda state, T: state[0][1].startswith("ewa_framelane"), f"{_cid(case)} auto n={n} {samples}", n=n, mode=0,
                fold=_fold_shape)


@gpu
def test_framelane_sub_unaligned_destination(gpu_pkg, O):
    """test_framelane_sub.py::test_unaligned_destination for half planes: destination pitches and offsets that are multiples of the
    sample size but not of 4 or 8 bytes cannot take the packed 4-sample stores; bytes between the rows stay untouched."""
    torch = pytest.importorskip("torch")
    case = ("YH", 100, 60, 137, 83, {})
    n = 13
    srcs, wants = _frames(gpu_pkg, O, case, "wide", n)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YH"], *case[1:5], device=0)
    f.set_kernel_mode(16)
    tw, th = 137, 83
    src_t = to_device(torch.stack([torch.from_numpy(np.ascontiguousarray(s[0])) for s in srcs]))
    for pitch, offset in ((278, 0), (278, 2), (276, 6), (274, 2), (280, 0)):
        assert pitch % 2 == 0 and offset % 2 == 0 and pitch >= 2 * tw
        buf = torch.full((n * th * pitch + 16,), 0xAB, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream()
        f.process_device([src_t.data_ptr()], [src_t.stride(1) * 2], [src_t.stride(0) * 2], [buf.data_ptr() + offset], [pitch], [th * pitch], n,
                         stream=stream.cuda_stream)
        stream.synchronize()
        assert f.last_kernel(0) == "ewa_framelane_sub_kernel"
        out = to_host(buf).numpy()
        body = out[offset:offset + n * th * pitch].reshape(n, th, pitch)
        for k in range(n):
            got = np.ascontiguousarray(body[k, :, :2 * tw]).view(np.float16)
            assert_half_equal([got], wants[k], [(tw, th)], what=f"pitch {pitch} offset {offset} frame {k}")
        assert (body[:, :, 2 * tw:] == 0xAB).all(), "padding between rows was written"
        assert (out[:offset] == 0xAB).all() and (out[offset + n * th * pitch:] == 0xAB).all()
    f.close()


# ---- 7. seeded sweep --------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("seed", range(16))
@pytest.mark.parametrize("gen", [1, 2, 3], ids=["small", "structured", "extreme"])
def test_randomised_arguments_on_half_planes(gpu_pkg, O, seed, gen):
    """The three generators of test_gpu_parity.py with their formats mapped to half (Y32 -> YH, RGBPS -> RGBPH, YUV420PS -> YUV420PH;
    integer draws to the half format of the same layout), 16 seeds each, unit samples: the automatic choice, then everything
    test_randomised_arguments forces -- border strips 1 / 3 / 4, the quad forms under border strips 4, modes 2 / 3 / 13 / 15 on periodic
    plans, modes 7 / 8 / 10 / 14 on quasi plans -- each against the definition and the fp32 twin under the same forcing."""
    rng = np.random.default_rng(1000 * gen + seed)
    fmt, sw, sh, tw, th, kw = {1: _random_case, 2: _random_case_v2, 3: _random_case_v3}[gen](rng)
    hname = half_name(fmt)
    try:
        O.OracleFilter(O.FORMATS[fp32_name(hname)], sw, sh, tw, th, **oracle_kwargs(kw))
    except Exception:
        pytest.skip("oracle rejects this geometry")
    try:
        fh, ff = _twins(gpu_pkg, (hname, sw, sh, tw, th, kw))
    except gpu_pkg.JincError as e:
        assert "smaller than the filter footprint" in str(e)
        return
    what = f"gen {gen} seed {seed}: {hname} {sw}x{sh}->{tw}x{th} {kw}"
    src = unit_frame(O, hname, sw, sh, seed)
    want = definition(O, hname, sw, sh, tw, th, kw, src)
    wide = _widen([src])[0]
    dims = fh.out_dims()

    def both(label, **knobs):
        with gpu_pkg.knobs(**knobs):
            got_f = ff.get_frame(wide)
            got_h = fh.get_frame(src)
        assert _state(fh) == _as_half(_state(ff)), f"{what} {label}: half {_state(fh)}, fp32 twin {_state(ff)}"
        _note(7, _state(fh), f"{what} {label}")
        _compare([got_h], [want], [got_f], dims, f"{what} {label}")

    def force(mode=None, strips=None):
        for f in (fh, ff):
            if mode is not None:
                f.set_kernel_mode(mode)
            if strips is not None:
                f.set_border_strips(strips)

    try:
        both("auto")
        if any(fh.plan_info(t).periodic for t in range(fh.num_tables)):
            for strips in (1, 3, 4):
                force(strips=strips)
                both(f"border strips {strips}")
            force(mode=13, strips=4)
            both("border strips 4, quad forms", quad2x8=1)
            force(mode=0, strips=-1)
            for mode in (2, 3, 13, 15):
                force(mode=mode)
                both(f"kernel mode {mode}")
            force(mode=0)
        if any(fh.plan_info(t).quasi for t in range(fh.num_tables)):
            for mode in (7, 8, 10, 14):
                force(mode=mode)
                both(f"kernel mode {mode}")
    finally:
        fh.close()
        ff.close()


# ---- what ran ---------------------------------------------------------------------------------------------------------------------------

@gpu
def test_zz_every_group_ran_on_half_instances():
    """Prints, per group, the instances the half filters ran (for the record), and holds the groups to their forms: every group saw
    its kernels, the periodic family's instances name _Float16, and every source step's walk unit of the direct kernel ran a
    single-step row (fs 9 .. 16) and a two-step row (fs 17 .. 32) from both bases; ewa_strip_kernel's column groups had every size mod 4."""
    for group in sorted(_SEEN):
        print(f"group {group}:")
        for inst in sorted(_SEEN[group]):
            print(f"  {len(_SEEN[group][inst]):4d} x {inst}")
    if set(_SEEN) != {1, 2, 3, 4, 5, 6, 7}:
        pytest.skip("only part of the module ran in this session")
    names = {g: " ".join(_SEEN[g]) for g in _SEEN}
    for g in _SEEN:
        for inst in _SEEN[g]:
            assert "<" not in inst or "<" + H in inst, inst
    for kernel in ("ewa_periodic_kernel<", "ewa_periodic_rows_kernel<", "ewa_periodic_pk_kernel<", "ewa_periodic_quad2_kernel<", "ewa_periodic_quad8_kernel<",
                   "ewa_periodic_quad2x8_kernel<", "ewa_periodic_rowpair_kernel<", "ewa_direct_kernel"):
        assert kernel in names[1], kernel
    assert "ewa_quasi_kernel" in names[2] and "ewa_direct_kernel" in names[3] and RUNS in names[4]
    for kernel in ("ewa_framelane_sub_kernel", "ewa_framelane_win_kernel", "ewa_framelane_win1k_kernel", "ewa_framelane_pair_kernel"):
        assert kernel in names[6], kernel
    assert _STRIP_RESIDUES == {0, 1, 2, 3}, _STRIP_RESIDUES   # the packed 4-sample store and every length of the tail
    for sx in (1, 2, 3, 4):
        for base in (0, 2):
            ran = {fs for (s, fs, shape, b) in _WALKS if s == sx and b == base and shape >= 2}
            assert any(9 <= fs <= 16 for fs in ran) and any(17 <= fs <= 32 for fs in ran), (sx, base, sorted(_WALKS))
