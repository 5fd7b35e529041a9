"""bfloat16 planes on EVERY kernel form, against their definition (tests/test_bfloat16_host.py): narrow(oracle_fp32(widen(src))), bit
for bit, NaN positions compared.  tests/test_bfloat16_planes.py reaches the automatic choice, the gather kernel and the full window
only; here every form that has a bf16_t instantiation of its own is forced the way tests/test_half_forms.py forces it for binary16
planes, on THAT file's case groups and mode tables (imported, not copied) with the formats mapped YH -> YBF, YUV420PH -> YUV420PBF ...

Every case makes two comparisons: the bfloat16 filter's result against the definition, and against the fp32 filter of the same
geometry, forced the same way, fed the widened samples, its result narrowed with the definition's narrow().  Reaching a form is
asserted, never assumed: bfloat16 planes take the decisions of fp32 planes of the same geometry (dispatch.cpp, rule_sb), so the
bfloat16 filter must have run the form exactly when the fp32 twin did -- with the twin's instance, `float` replaced by `__bf16`, and
the twin's border kernels.  A case skips only where the twin does not reach the form either (the half file has the same two skips).

Sample sets: `unit`, `wide` (test_bfloat16_host.wide_frame) and, for the border forms, `noise` (both signs, +-inf and two NaN
patterns inside the first / last source rows and columns of the last frame)."""
import re

import numpy as np
import pytest

from conftest import oracle_kwargs, to_device, to_host
from test_bfloat16_host import assert_bf16_equal, definition, fp32_name, is_nan, narrow, unit_frame, wide_frame, widen
from test_direct_runs import RUNS
from test_float_trim_paths import _padded_runner
from test_gpu_parity import _random_case, _random_case_v2, _random_case_v3
from test_half_forms import (BORDER_SAMPLES, G1_MODES, G1_ROWPAIR, G1_TAP2, G1_TAP3, G1_TAP4, G2, G2_MODES, G3_DIRECT, G4, G5_COLPAIR, G5_COLSTRIP,
                             G5_EDGE, G5_ROWPAIR_ROWS, G5_STRIP, G6, G6_AUTO_N, G6_SUB_N, SAMPLES, WALK_RUNS, _border, _call, _cid, _column_groups,
                             _fold_shape, _instance, _kernel, _key, _periodic_pattern, _state, half_name)

pytestmark = pytest.mark.gpu
B, F = "__bf16", "float"


def bf_name(hname):
    assert hname.endswith("H"), hname
    return hname[:-1] + "BF"


def bf(case):
    return (bf_name(case[0]),) + tuple(case[1:])


def bfs(cases):
    return [bf(c) for c in cases if c[0].endswith("H")]


_FRAMES = {}
_SEEN = {}
_WALKS = set()
_STRIP_RESIDUES = set()
INF, NINF, NAN, NAN1 = 0x7f80, 0xff80, 0x7fc0, 0x7f81


def _noise_frame(pkg, bname, sw, sh, rng, non_finite):
    out = []
    for (pw, ph) in pkg.FORMATS[bname].plane_dims(sw, sh):
        p = pkg.alloc_plane(pw, ph, np.uint16)
        p[...] = narrow((rng.standard_normal(p.shape) * 0.8).astype(np.float32))
        out.append(p)
    if non_finite:
        out[0][sh // 3, 1], out[0][sh // 2, sw - 2], out[0][1, sw // 3], out[0][sh - 2, sw // 2] = INF, NAN1, NINF, NAN
    return out


def _frames(pkg, O, case, samples, n=1):
    bname, sw, sh, tw, th, kw = case[:6]
    if samples == "noise":
        key = (_key(case), samples, n)
        if key not in _FRAMES:
            rng = np.random.default_rng(6)
            srcs = [_noise_frame(pkg, bname, sw, sh, rng, k == n - 1) for k in range(n)]
            wants = [definition(O, bname, sw, sh, tw, th, kw, s) for s in srcs]
            assert is_nan(wants[-1][0]).any() and ((wants[-1][0] & 0x7fff) == INF).any()
            _FRAMES[key] = (srcs, wants)
        return _FRAMES[key]
    srcs, wants = _FRAMES.setdefault((_key(case), samples), ([], []))
    while len(srcs) < n:
        k = len(srcs)
        src = unit_frame(O, bname, sw, sh, 4242 + k) if samples == "unit" else wide_frame(pkg, bname, sw, sh, 4242 + k)
        srcs.append(src)
        wants.append(definition(O, bname, sw, sh, tw, th, kw, src))
    return srcs[:n], wants[:n]


def _widen(srcs):
    return [[widen(p) for p in s] for s in srcs]


def _as_bf(state):
    return [(i.replace("<" + F, "<" + B), k, b) for (i, k, b) in state]


def _note(group, state, what):
    for inst, _, border in state:
        _SEEN.setdefault(group, {}).setdefault(f"{inst} [border {border}]", []).append(what)
    print(f"bfloat16 form, group {group}: {what}: " + "; ".join(f"{i} [border {b}]" for i, _, b in state))


def _compare(got_b, wants, got_f, dims, what):
    errors = []
    for k in range(len(got_b)):
        with np.errstate(over="ignore", invalid="ignore"):
            twin = [narrow(p) for p in got_f[k]]
        for name, want in (("the definition", wants[k]), ("the fp32 twin, narrowed", twin)):
            try:
                assert_bf16_equal(got_b[k], want, dims, what=f"{what} frame {k} vs {name}")
            except AssertionError as e:
                errors.append(str(e))
    if errors:
        verdict = "the bfloat16 instantiation differs from fp32" if any("twin" in e for e in errors) else "the fp32 form gives the same bits: the form itself differs from the oracle"
        raise AssertionError(f"{verdict}\n" + "\n".join(errors[:6]))


def _twins(pkg, case):
    bname, sw, sh, tw, th, kw = case[:6]
    return (pkg.Filter(pkg.FORMATS[bname], sw, sh, tw, th, device=0, **kw),
            pkg.Filter(pkg.FORMATS[fp32_name(bname)], sw, sh, tw, th, device=0, **kw))


def _check_form(pkg, O, group, case, samples, reached, what, n=1, run=None, fold=lambda state: state, **force):
    torch = pytest.importorskip("torch")
    srcs, wants = _frames(pkg, O, case, samples, n)
    run = run or (lambda f, s: _call(pkg, torch, f, s, **force))
    fb, ff = _twins(pkg, case)
    try:
        got_f = run(ff, _widen(srcs))
        state_f = _state(ff)
        got_b = run(fb, srcs)
        state_b = _state(fb)
        if not reached(state_f, F):
            assert not reached(state_b, B), f"{what}: the fp32 twin did not reach the form ({state_f}) but the bfloat16 filter did ({state_b})"
            pytest.skip(f"the fp32 twin does not reach the form either: {state_f}")
        assert reached(state_b, B), f"{what}: the fp32 twin reached the form ({state_f}), the bfloat16 filter ran {state_b}"
        assert fold(state_b) == fold(_as_bf(state_f)), f"{what}: bfloat16 {state_b}, fp32 twin {state_f}"
        _note(group, state_b, what)
        _compare(got_b, wants, got_f, fb.out_dims(), what)
        return got_b
    finally:
        fb.close()
        ff.close()


# ---- 1. periodic variants ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("mode", sorted(G1_MODES), ids=[G1_MODES[m] for m in sorted(G1_MODES)])
@pytest.mark.parametrize("case", bfs(G1_TAP3), ids=_cid)
def test_periodic_variants_tap3(gpu_pkg, O, case, mode, samples):
    _check_form(gpu_pkg, O, 1, case, samples, _instance(_periodic_pattern(mode, 7, {})), f"{_cid(case)} mode {mode} {samples}", mode=mode)


@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("two", [0, 1], ids=["quad2x8_0", "quad2x8_1"])
@pytest.mark.parametrize("mode", [2, 13, 15], ids=["window", "quad", "full_window"])
@pytest.mark.parametrize("case", bfs(G1_TAP4), ids=_cid)
def test_periodic_variants_tap4(gpu_pkg, O, case, mode, two, samples):
    knobs = dict(quad2x8=two)
    _check_form(gpu_pkg, O, 1, case, samples, _instance(_periodic_pattern(mode, 9, knobs)), f"{_cid(case)} mode {mode} quad2x8={two} {samples}",
                mode=mode, knobs=knobs)


@pytest.mark.parametrize("samples", SAMPLES)
def test_periodic_rows_kernel_tap2(gpu_pkg, O, samples):
    case = bf(G1_TAP2)
    _check_form(gpu_pkg, O, 1, case, samples, _instance(_periodic_pattern(3, 5, {})), f"{_cid(case)} mode 3 {samples}", mode=3)


@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("lw", [0, 64, 32, 16], ids=["auto", "256x16", "128x32", "64x64"])
@pytest.mark.parametrize("case", bfs(G1_ROWPAIR), ids=_cid)
def test_rowpair_form(gpu_pkg, O, case, lw, samples):
    pattern = r"ewa_periodic_rowpair_kernel<{T}, \d+, " + (str(lw) if lw else r"\d+") + r", \d+>"
    _check_form(gpu_pkg, O, 1, case, samples, _instance(pattern), f"{_cid(case)} rows_pair={lw} {samples}", mode=0,
                knobs={"rows_pair": lw} if lw else {})


# ---- 2. the quasi-periodic kernel -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("mode", sorted(G2_MODES), ids=[G2_MODES[m] for m in sorted(G2_MODES)])
@pytest.mark.parametrize("case", bfs(G2), ids=_cid)
def test_quasi_periodic_kernel(gpu_pkg, O, case, mode, samples):
    reached = _kernel("ewa_quasi_kernel") if mode in (7, 8, 10) else (lambda state, T: True)
    _check_form(gpu_pkg, O, 2, case, samples, reached, f"{_cid(case)} mode {mode} {samples}", mode=mode)


@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("split", [1, 2])
def test_quasi_periodic_kernel_with_split_phases(gpu_pkg, O, split, samples):
    case = bf(G2[0])
    _check_form(gpu_pkg, O, 2, case, samples, _kernel("ewa_quasi_kernel"), f"{_cid(case)} quasi_split={split} {samples}", mode=7,
                knobs=dict(quasi_split=split))


# ---- 3. the direct kernel ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("mode", [9, 0], ids=["direct", "auto"])
@pytest.mark.parametrize("case", bfs(G3_DIRECT), ids=_cid)
def test_direct_kernel(gpu_pkg, O, case, mode, samples):
    reached = _kernel("ewa_direct_kernel") if mode == 9 else (lambda state, T: True)
    _check_form(gpu_pkg, O, 3, case, samples, reached, f"{_cid(case)} mode {mode} {samples}", mode=mode)


BF_WALK_RUNS = [(bf(c), b) for c, b in WALK_RUNS]


@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("case,base", BF_WALK_RUNS, ids=[f"{_cid(c)}-base{b}" for c, b in BF_WALK_RUNS])
def test_direct_kernel_row_walk(gpu_pkg, O, case, base, samples):
    """Kernel mode 9 on every row of the half file's walk cases.  Every one-plane case runs twice from device memory: with the
    plane's base on a dword and 2 bytes behind one, which swaps bf16_lo and bf16_hi for every phase.  The buffer around the plane
    holds 0xFF bytes (a NaN in bfloat16 too): a sample fetched from outside the plane shows."""
    torch = pytest.importorskip("torch")
    bname, sw, sh = case[0], case[1], case[2]
    planes = gpu_pkg.FORMATS[bname].planes
    shapes = []

    def run(f, srcs):
        sb = np.dtype(f.fmt.dtype).itemsize
        if planes > 1:
            out = _call(gpu_pkg, torch, f, srcs, mode=9)
        else:
            out = _padded_runner(sw, sh, 64 + (base if sb == 2 else 0), (-sw * sb) % 4 + 4, 8)(torch, gpu_pkg, f, f.fmt, srcs, 1, 9)
        shapes.append(gpu_pkg.last_direct_shape())
        return out

    _check_form(gpu_pkg, O, 3, case, samples, _kernel("ewa_direct_kernel"), f"{_cid(case)} base {base} {samples}", run=run)
    assert shapes[0] == shapes[1], f"DirectShape: fp32 twin {shapes[0]}, bfloat16 {shapes[1]}"
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[bname], *case[1:5], device=-1, **case[5])
    info = f.plan_info(0)
    f.close()
    _WALKS.add((info.step_x, info.filter_size, shapes[1], base))


# ---- 4. the runs form -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("case", bfs(G4), ids=_cid)
def test_runs_form(gpu_pkg, O, case, samples):
    _check_form(gpu_pkg, O, 4, case, samples, _kernel(RUNS), f"{_cid(case)} mode 14 {samples}", mode=14)


@pytest.mark.parametrize("samples", SAMPLES)
def test_runs_form_falls_back_to_gather_on_a_pitch_that_is_no_multiple_of_4_bytes(gpu_pkg, O, samples):
    torch = pytest.importorskip("torch")
    case = ("YBF", 202, 120, 303, 180, dict(tap=6))
    n = 5
    srcs, wants = _frames(gpu_pkg, O, case, samples, n)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YBF"], *case[1:5], device=0, **case[5])
    assert f.plan_info().quasi == 1 and f.plan_info().periodic == 0
    for extra, kernel in ((0, RUNS), (2, "ewa_gather_kernel"), (4, RUNS)):
        out = _padded_runner(202, 120, 0, extra, 0)(torch, gpu_pkg, f, f.fmt, srcs, n, 14)
        assert f.last_kernel(0) == kernel, (extra, f.last_kernel(0))
        for k in range(n):
            assert_bf16_equal(out[k], wants[k], f.out_dims(), what=f"pitch {404 + extra} frame {k} ({kernel})")
    f.close()


# ---- 5. border forms --------------------------------------------------------------------------------------------------------------------

def _border_case(pkg, O, case, samples, n, reached, what, strips, knobs=None, mode=0, others=()):
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
                assert_bf16_equal(got[k], other[k], f.out_dims(), what=f"{what} frame {k} vs border form {o_strips} {o_knobs}")
    finally:
        f.close()


@pytest.mark.parametrize("samples", BORDER_SAMPLES)
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("case", bfs(G5_STRIP), ids=_cid)
def test_strip_kernel_rows_and_columns(gpu_pkg, O, case, n, samples):
    _border_case(gpu_pkg, O, case, samples, n, _border(48), f"{_cid(case)} strips 3 n={n} {samples}", 3, others=[(1, None, 0), (0, None, 0)])
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[case[0]], *case[1:5], device=-1, **case[5])
    _STRIP_RESIDUES.update(g % 4 for g in _column_groups(f))
    f.close()


@pytest.mark.parametrize("samples", BORDER_SAMPLES)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("case", bfs(G5_COLPAIR), ids=_cid)
def test_column_pairs(gpu_pkg, O, case, n, samples):
    _border_case(gpu_pkg, O, case, samples, n, _border(256, none_of=64 | 32 | 8 | 4 | 1), f"{_cid(case)} colpair n={n} {samples}", 4,
                 knobs=dict(colpair=1), others=[(4, dict(colpair=0), 256), (0, dict(colpair=1), 0)])


@pytest.mark.parametrize("samples", BORDER_SAMPLES)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("case", bfs(G5_ROWPAIR_ROWS), ids=_cid)
def test_border_rows_on_the_pair_kernel(gpu_pkg, O, case, n, samples):
    _border_case(gpu_pkg, O, case, samples, n, _border(128, none_of=16 | 2), f"{_cid(case)} rowpair rows n={n} {samples}", 4,
                 others=[(4, dict(rowpair_rows=0), 128), (0, None, 0)])


@pytest.mark.parametrize("samples", BORDER_SAMPLES)
@pytest.mark.parametrize("case", bfs(G5_COLSTRIP), ids=_cid)
def test_colstrip_kernel(gpu_pkg, O, case, samples):
    _border_case(gpu_pkg, O, case, samples, 1, _border(4 | 2, none_of=256 | 64 | 32 | 16 | 8), f"{_cid(case)} colstrip {samples}", 1, others=[(0, None, 0)])


@pytest.mark.parametrize("samples", BORDER_SAMPLES)
@pytest.mark.parametrize("case", bfs(G5_EDGE), ids=_cid)
def test_edge_columns_stay_integer_only(gpu_pkg, O, case, samples):
    _border_case(gpu_pkg, O, case, samples, 1, lambda state, T: state[0][2] & 64 == 0, f"{_cid(case)} edge forcing {samples}", 4,
                 knobs=dict(quad2x8=1), mode=13, others=[(0, dict(quad2x8=1), 64)])


# ---- 6. batch forms ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("n", G6_SUB_N)
@pytest.mark.parametrize("case", bfs(G6), ids=_cid)
def test_framelane_sub_groups(gpu_pkg, O, case, n, samples):
    _check_form(gpu_pkg, O, 6, case, samples, _kernel("ewa_framelane_sub_kernel"), f"{_cid(case)} mode 16 n={n} {samples}", n=n, mode=16)


@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("n", G6_AUTO_N)
@pytest.mark.parametrize("case", bfs(G6), ids=_cid)
def test_batches_under_the_automatic_choice(gpu_pkg, O, case, n, samples):
    _check_form(gpu_pkg, O, 6, case, samples, lambda state, T: state[0][1].startswith("ewa_framelane"), f"{_cid(case)} auto n={n} {samples}", n=n, mode=0,
                fold=_fold_shape)


def test_framelane_sub_unaligned_destination(gpu_pkg, O):
    """Destination pitches and offsets that are multiples of the sample size but not of 4 or 8 bytes cannot take the packed 4-sample
    stores; bytes between the rows stay untouched."""
    torch = pytest.importorskip("torch")
    case = ("YBF", 100, 60, 137, 83, {})
    n = 13
    srcs, wants = _frames(gpu_pkg, O, case, "wide", n)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YBF"], *case[1:5], device=0)
    f.set_kernel_mode(16)
    tw, th = 137, 83
    src_t = to_device(torch.stack([torch.from_numpy(np.ascontiguousarray(s[0]).view(np.int16)) for s in srcs]))
    for pitch, offset in ((278, 0), (278, 2), (276, 6), (274, 2), (280, 0)):
        buf = torch.full((n * th * pitch + 16,), 0xAB, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream()
        f.process_device([src_t.data_ptr()], [src_t.stride(1) * 2], [src_t.stride(0) * 2], [buf.data_ptr() + offset], [pitch], [th * pitch], n,
                         stream=stream.cuda_stream)
        stream.synchronize()
        assert f.last_kernel(0) == "ewa_framelane_sub_kernel"
        out = to_host(buf).numpy()
        body = out[offset:offset + n * th * pitch].reshape(n, th, pitch)
        for k in range(n):
            got = np.ascontiguousarray(body[k, :, :2 * tw]).view(np.uint16)
            assert_bf16_equal([got], wants[k], [(tw, th)], what=f"pitch {pitch} offset {offset} frame {k}")
        assert (body[:, :, 2 * tw:] == 0xAB).all(), "padding between rows was written"
        assert (out[:offset] == 0xAB).all() and (out[offset + n * th * pitch:] == 0xAB).all()
    f.close()


# ---- 7. seeded sweep --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("gen", [1, 2, 3], ids=["small", "structured", "extreme"])
def test_randomised_arguments_on_bfloat16_planes(gpu_pkg, O, seed, gen):
    """The three generators of test_gpu_parity.py with their formats mapped to bfloat16, 8 seeds each, unit samples: the automatic
    choice, then everything the half file's sweep forces, each against the definition and the fp32 twin under the same forcing."""
    rng = np.random.default_rng(1000 * gen + seed)
    fmt, sw, sh, tw, th, kw = {1: _random_case, 2: _random_case_v2, 3: _random_case_v3}[gen](rng)
    bname = bf_name(half_name(fmt))
    try:
        O.OracleFilter(O.FORMATS[fp32_name(bname)], sw, sh, tw, th, **oracle_kwargs(kw))
    except Exception:
        pytest.skip("oracle rejects this geometry")
    try:
        fb, ff = _twins(gpu_pkg, (bname, sw, sh, tw, th, kw))
    except gpu_pkg.JincError as e:
        assert "smaller than the filter footprint" in str(e)
        return
    what = f"gen {gen} seed {seed}: {bname} {sw}x{sh}->{tw}x{th} {kw}"
    src = unit_frame(O, bname, sw, sh, seed)
    want = definition(O, bname, sw, sh, tw, th, kw, src)
    wide = _widen([src])[0]
    dims = fb.out_dims()

    def both(label, **knobs):
        with gpu_pkg.knobs(**knobs):
            got_f = ff.get_frame(wide)
            got_b = fb.get_frame(src)
        assert _state(fb) == _as_bf(_state(ff)), f"{what} {label}: bfloat16 {_state(fb)}, fp32 twin {_state(ff)}"
        _note(7, _state(fb), f"{what} {label}")
        _compare([got_b], [want], [got_f], dims, f"{what} {label}")

    def force(mode=None, strips=None):
        for f in (fb, ff):
            if mode is not None:
                f.set_kernel_mode(mode)
            if strips is not None:
                f.set_border_strips(strips)

    try:
        both("auto")
        if any(fb.plan_info(t).periodic for t in range(fb.num_tables)):
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
        if any(fb.plan_info(t).quasi for t in range(fb.num_tables)):
            for mode in (7, 8, 10, 14):
                force(mode=mode)
                both(f"kernel mode {mode}")
    finally:
        fb.close()
        ff.close()


# ---- what ran ---------------------------------------------------------------------------------------------------------------------------

def test_zz_every_group_ran_on_bfloat16_instances():
    """Prints, per group, the instances the bfloat16 filters ran, and holds the groups to their forms: every group saw its kernels,
    every instance that names a sample type names __bf16, and every source step's walk unit of the direct kernel ran a single-step
    row (fs 9 .. 16) and a two-step row (fs 17 .. 32) from both bases; ewa_strip_kernel's column groups had every size mod 4."""
    for group in sorted(_SEEN):
        print(f"group {group}:")
        for inst in sorted(_SEEN[group]):
            print(f"  {len(_SEEN[group][inst]):4d} x {inst}")
    if set(_SEEN) != {1, 2, 3, 4, 5, 6, 7}:
        pytest.skip("only part of the module ran in this session")
    names = {g: " ".join(_SEEN[g]) for g in _SEEN}
    for g in _SEEN:
        for inst in _SEEN[g]:
            assert "<" not in inst or "<" + B in inst, inst
        assert g in (2, 3, 4, 6, 7) or "<" + B in names[g], (g, "no instance of this group names the bfloat16 type")
    for kernel in ("ewa_periodic_kernel<", "ewa_periodic_rows_kernel<", "ewa_periodic_pk_kernel<", "ewa_periodic_quad2_kernel<", "ewa_periodic_quad8_kernel<",
                   "ewa_periodic_quad2x8_kernel<", "ewa_periodic_rowpair_kernel<", "ewa_direct_kernel"):
        assert kernel + (B if kernel.endswith("<") else "") in names[1], kernel
    assert "ewa_quasi_kernel" in names[2] and "ewa_direct_kernel" in names[3] and RUNS in names[4]
    for kernel in ("ewa_framelane_sub_kernel", "ewa_framelane_win_kernel", "ewa_framelane_win1k_kernel", "ewa_framelane_pair_kernel"):
        assert kernel in names[6], kernel
    assert _STRIP_RESIDUES == {0, 1, 2, 3}, _STRIP_RESIDUES
    for sx in (1, 2, 3, 4):
        for base in (0, 2):
            ran = {fs for (s, fs, shape, b) in _WALKS if s == sx and b == base and shape >= 2}
            assert any(9 <= fs <= 16 for fs in ran) and any(17 <= fs <= 32 for fs in ran), (sx, base, sorted(_WALKS))
