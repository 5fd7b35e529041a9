"""The frame-pair form of the 2x tap-3 interior (ewa_periodic_quad2_kernel<integer, RG, 1026u, 6>, kernel_periodic_quad2.inc
quad2_share_body): one product per (source sample, symmetry class), added into every chain of the lane's 4 x 4 outputs that takes it.

CPU: the compile-time class map (csrc/kernels.h quad2_share_class) against the oracle's own coefficient sets -- the classes are
derived here from the output centres and tap positions, independently of the library -- and plans that are not such a 2x up-scale
are turned down.  GPU: C2's geometry on 8- and 16-bit planes at 1 .. 40 frames per call (both tile heights), the forced fallback
(knob quad_share = 0) and small planes whose edge tiles compute the border columns, all against the oracle."""
import numpy as np
import pytest

from conftest import assert_planes_equal, oracle_kwargs

C2 = ("Y8", 1920, 1080, 3840, 2160)


def _classes():
    """(lo, hi) -> class number: the pairs of distance classes inside the disc, in (lo, hi) order."""
    inside = [(a, b) for a in range(6) for b in range(a, 6) if (2 * a + 1) ** 2 + (2 * b + 1) ** 2 <= 162]
    return {ab: k for k, ab in enumerate(inside)}


def _oracle_phase_sets(pkg, O, fmt, sw, sh, tw, th, kw, table=0):
    """The interior's four phase sets (p, q) from the ORACLE's table, cut to the joint non-zero box, with every tap's distances
    (|dx|, |dy|) from its output's centre in source steps."""
    f = pkg.Filter(pkg.FORMATS[fmt], sw, sh, tw, th, device=-1, **kw)
    info = f.plan_info(table)
    f.close()
    assert info.periodic and info.period_x == 2 and info.period_y == 2
    of = O.OracleFilter(O.FORMATS[fmt], sw, sh, tw, th, **oracle_kwargs(kw))
    ot = of.tables[table]
    fs, meta = ot.filter_size, ot.meta()
    x0, y0 = info.interior_x0 + 2 * 40, info.interior_y0 + 2 * 30   # a period well inside
    sx_scale, sy_scale = ot.src_w / ot.dst_w, ot.src_h / ot.dst_h
    full, dist = {}, {}
    for q in range(2):
        for p in range(2):
            x, y = x0 + p, y0 + q
            full[p, q] = ot.coeff_set(x, y).copy()
            cx, cy = (x + 0.5) * sx_scale - 0.5, (y + 0.5) * sy_scale - 0.5
            sx, sy = int(meta[y, x, 0]), int(meta[y, x, 1])
            dist[p, q] = (np.abs(sx + np.arange(fs) - cx), np.abs(sy + np.arange(fs) - cy), sx, sy)
    assert len({(d[2], d[3]) for d in dist.values()}) == 1, "the phases of a period share their window origin"
    rows = [r for r in range(fs) if any(full[k][r].any() for k in full)]
    cols = [c for c in range(fs) if any(full[k][:, c].any() for k in full)]
    r0, c0 = rows[0], cols[0]
    nr, nc = rows[-1] - r0 + 1, cols[-1] - c0 + 1
    sets = {k: np.ascontiguousarray(v[r0:r0 + nr, c0:c0 + nc], dtype=np.float32) for k, v in full.items()}
    dists = {k: (d[0][c0:c0 + nc], d[1][r0:r0 + nr]) for k, d in dist.items()}
    return sets, dists, (nr, nc)


def _library_check(pkg, sets):
    dense = np.ascontiguousarray(np.stack([sets[p, q].ravel() for q in range(2) for p in range(2)]), dtype=np.float32)
    w = np.zeros(18, np.float32)
    ok = pkg.lib().jinc_debug_quad2_share(dense.ctypes.data, w.ctypes.data)
    return ok, w


@pytest.mark.parametrize("cfg", ["C2", "C2H"])
def test_class_map_matches_the_oracle_tables(pkg, O, cfg):
    fmt = "Y8" if cfg == "C2" else "YUV420P16"   # C2H: C2's geometry on 16-bit 4:2:0 -- its luma table is the 6 x 6 case
    sets, dists, shape = _oracle_phase_sets(pkg, O, fmt, 1920, 1080, 3840, 2160, dict(tap=3))
    assert shape == (6, 6), shape
    ok, w = _library_check(pkg, sets)
    assert ok == 1, "the library turned down C2's own phase sets"
    classes = _classes()
    assert len(classes) == 18
    by_class = {}
    nonzero = 0
    for (p, q), s in sets.items():
        dx, dy = dists[p, q]
        for ly in range(6):
            for lx in range(6):
                mx, my = (2 * dx[lx] - 0.5), (2 * dy[ly] - 0.5)
                assert abs(mx - round(mx)) < 1e-9 and abs(my - round(my)) < 1e-9, "taps sit (2 m + 1) / 4 steps from the centre"
                key = tuple(sorted((int(round(mx)), int(round(my)))))
                c = s[ly, lx]
                if key not in classes:
                    assert c == 0.0, (key, c)
                    continue
                nonzero += c != 0.0
                by_class.setdefault(classes[key], set()).add(np.float32(c).view(np.uint32).item())
    assert nonzero == 4 * 31, nonzero   # 31 non-zero taps per output
    assert sorted(by_class) == list(range(18))
    for k, bits in by_class.items():
        assert len(bits) == 1, f"class {k} holds {len(bits)} different coefficients"
        assert np.float32(w[k]).view(np.uint32).item() == next(iter(bits)), f"share_w[{k}]"


def test_plans_that_are_not_the_2x_classes_are_turned_down(pkg, O):
    sets, _, _ = _oracle_phase_sets(pkg, O, *C2, dict(tap=3))
    # the column phases exchanged: tap t of phase 0 is no longer 2.25 taps behind the origin
    assert _library_check(pkg, {(p, q): sets[1 - p, q] for p in range(2) for q in range(2)})[0] == 0
    # one tap of one class changed by an ulp
    bent = {k: v.copy() for k, v in sets.items()}
    bent[0, 0][2, 2] = np.nextafter(bent[0, 0][2, 2], np.float32(2))
    assert _library_check(pkg, bent)[0] == 0
    # a tap outside the disc that is not zero
    bent = {k: v.copy() for k, v in sets.items()}
    bent[1, 1][0, 0] = np.float32(1e-3)
    assert _library_check(pkg, bent)[0] == 0
    # a 3x up-scale: four of its phase sets cut to 6 x 6
    f = pkg.Filter(pkg.FORMATS["Y8"], 640, 360, 1920, 1080, device=-1, tap=3)
    info = f.plan_info(0)
    _, _, ids = f.plan_dump(0)
    all_sets = f.plan_sets(0)
    f.close()
    fs = info.filter_size
    x0, y0 = info.interior_x0, info.interior_y0
    three = {(p, q): np.ascontiguousarray(all_sets[ids[y0 + q, x0 + p]].reshape(fs, fs)[:6, :6], dtype=np.float32)
             for p in range(2) for q in range(2)}
    assert _library_check(pkg, three)[0] == 0


# ------------------------------------------------------------------------------------------------ GPU


def _frames(O, fmt, sw, sh, n, seed):
    return [O.lcg_frame(O.FORMATS[fmt], sw, sh, seed=seed + k) for k in range(n)]


def _check_batch(gpu_pkg, O, fmt, geom, kw, n, seed, *, create_knobs=None, run_knobs=None, mode=0, strips=None):
    torch = pytest.importorskip("torch")
    from test_framelane_pair import _run_batch
    sw, sh, tw, th = geom
    ofmt, gfmt = O.FORMATS[fmt], gpu_pkg.FORMATS[fmt]
    of = O.OracleFilter(ofmt, sw, sh, tw, th, **oracle_kwargs(kw))
    with gpu_pkg.knobs(**(create_knobs or {})):   # (quad_share is read when the plan is built)
        f = gpu_pkg.Filter(gfmt, sw, sh, tw, th, device=0, **kw)
    if strips is not None:
        f.set_border_strips(strips)
    srcs = _frames(O, fmt, sw, sh, n, seed)
    with gpu_pkg.knobs(**(run_knobs or {})):
        got = _run_batch(torch, gpu_pkg, f, gfmt, srcs, n, mode)
    inst = [f.last_instance(t) for t in range(f.num_tables)]
    borders = [f.last_border(t) for t in range(f.num_tables)]
    dims = f.out_dims()
    f.close()
    for k in range(n):
        key = (fmt, geom, tuple(sorted(kw.items())), seed + k)
        if key not in _WANT:   # (the C2 cases share their frames: the oracle computes each once)
            _WANT[key] = of.get_frame(srcs[k], threads=8)
        assert_planes_equal(got[k], _WANT[key], dims, what=f"{fmt} {geom} frame {k} of {n}")
    return inst, borders


_WANT = {}


@pytest.mark.gpu
@pytest.mark.parametrize("rg", [None, 8])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 40])
@pytest.mark.parametrize("fmt,tname", [("Y8", "unsigned char"), ("Y16", "unsigned short")])
def test_c2_geometry_matches_the_oracle(gpu_pkg, O, fmt, tname, n, rg):
    """Every frame of the call, so the first and the last pair (the odd count's half pair included); rg = 8 forces the full-tile
    instance, which has no per-frame body: single frames run there as a pair whose second half is not stored."""
    run_knobs = {"quad_rg": rg} if rg else {}
    # (one frame of C2 does not fill the chip with the quad form: kernel mode QUAD forces it there)
    mode = gpu_pkg.KernelMode.QUAD if n == 1 else 0
    inst, _ = _check_batch(gpu_pkg, O, fmt, C2[1:], dict(tap=3), n, 700, run_knobs=run_knobs, mode=mode)
    tiles = (rg,) if rg else (4, 8)   # (the automatic tile height is dispatch.cpp's call)
    assert inst[0] in [f"ewa_periodic_quad2_kernel<{tname}, {t}, 1026u, 6>" for t in tiles], inst[0]


@pytest.mark.gpu
@pytest.mark.parametrize("rg", [None, 8])
def test_forced_fallback_takes_every_tap_and_matches(gpu_pkg, O, rg):
    run_knobs = {"quad_rg": rg} if rg else {}
    inst, _ = _check_batch(gpu_pkg, O, "Y8", C2[1:], dict(tap=3), 3, 700, create_knobs={"quad_share": 0}, run_knobs=run_knobs)
    assert inst[0] in [f"ewa_periodic_quad2_kernel<unsigned char, {t}, 0u, 6>" for t in ((rg,) if rg else (4, 8))], inst[0]


EDGE_CASES = [
    ("Y8", (192, 108, 384, 216)),      # one tile column: both sides in the same workgroups
    ("Y8", (500, 70, 1000, 140)),      # four tile columns, the last one partial
    ("Y8", (263, 301, 526, 602)),      # odd sizes, a partial last tile row
    ("Y8", (135, 50, 270, 100)),       # the last tile column holds four periods
    ("Y16", (333, 211, 666, 422)),
    ("Y10", (150, 100, 300, 200)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 5])
@pytest.mark.parametrize("fmt,geom", EDGE_CASES, ids=lambda c: str(c))
def test_small_planes_with_edge_tiles(gpu_pkg, O, fmt, geom, n):
    inst, borders = _check_batch(gpu_pkg, O, fmt, geom, dict(tap=3), n, 300 + n, mode=gpu_pkg.KernelMode.QUAD, strips=4)
    assert inst[0].startswith("ewa_periodic_quad2_kernel<") and inst[0].endswith(", 1026u, 6>"), inst[0]
    assert borders[0] & 64, borders[0]   # the border columns came out of the edge tiles
