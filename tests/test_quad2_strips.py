"""The strip walk of the frame-pair 2x tap-3 interior (ewa_periodic_quad2_kernel<integer, RG, 1026u, 6>, kernel_periodic_quad2.inc
quad2_share_body): a lane walks a strip of H period rows (8 on full tiles of 32 period rows, 2 on half tiles of 16) and stores each
period row when its six source rows are done.  Bottom tiles end in partial strips, so the plane heights here leave every kind of last
strip: interior period rows nj with nj mod 32 in {1, 5, 7, 8, 9, 31} and nj < 8.  Widths give edge tiles on both sides (the border
columns come out of them).  Every frame of 2, 3 and 7 frames per call, 8- and 16-bit planes, both tile heights through quad_rg, against
the oracle."""
import functools

import pytest

from test_quad2_share import _check_batch

SW = 300   # three tile columns of 128 periods: edge tiles on both sides, the last one partial
RESIDUES = [1, 5, 7, 8, 9, 31]


@functools.lru_cache(maxsize=None)
def _period_rows(pkg, fmt, sh):
    """The interior's period rows (nj) of a 2x tap-3 plan of SW x sh, or None when the plan is not periodic with period 2."""
    f = pkg.Filter(pkg.FORMATS[fmt], SW, sh, 2 * SW, 2 * sh, device=-1, tap=3)
    info = f.plan_info(0)
    f.close()
    if not (info.periodic and info.period_x == 2 and info.period_y == 2):
        return None
    return (info.interior_y1 - info.interior_y0) // 2


def _height(pkg, fmt, want):
    """The smallest source height whose interior has nj period rows with want(nj)."""
    for sh in range(8, 400):
        nj = _period_rows(pkg, fmt, sh)
        if nj is not None and nj > 0 and want(nj):
            return sh, nj
    pytest.fail("no such height")


CASES = [(f"mod32_{r}", lambda nj, r=r: nj % 32 == r and nj > 32) for r in RESIDUES] + [("below_8", lambda nj: nj < 8)]


@pytest.mark.parametrize("fmt", ["Y8", "Y16"])
def test_heights_cover_every_partial_strip(pkg, fmt):
    """(CPU) The heights the GPU cases below use reach every residue, so a change of the plan's margins cannot quietly drop one."""
    for name, want in CASES:
        sh, nj = _height(pkg, fmt, want)
        assert want(nj), (name, sh, nj)


@pytest.mark.gpu
@pytest.mark.parametrize("rg", [4, 8])
@pytest.mark.parametrize("fmt,tname", [("Y8", "unsigned char"), ("Y16", "unsigned short")])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_partial_strips_match_the_oracle(gpu_pkg, O, case, fmt, tname, rg):
    sh, _ = _height(gpu_pkg, fmt, case[1])
    inst, borders = _check_batch(gpu_pkg, O, fmt, (SW, sh, 2 * SW, 2 * sh), dict(tap=3), 3, 900 + sh, run_knobs={"quad_rg": rg},
                                 mode=gpu_pkg.KernelMode.QUAD, strips=4)
    assert inst[0] == f"ewa_periodic_quad2_kernel<{tname}, {rg}, 1026u, 6>", inst[0]
    assert borders[0] & 64, borders[0]   # the border columns came out of the edge tiles


@pytest.mark.gpu
@pytest.mark.parametrize("rg", [4, 8])
@pytest.mark.parametrize("n", [2, 7])
@pytest.mark.parametrize("fmt,tname", [("Y8", "unsigned char"), ("Y16", "unsigned short")])
def test_frame_counts_match_the_oracle(gpu_pkg, O, fmt, tname, n, rg):
    """Even and odd counts: every pair full, and the last pair's high half repeating the low frame (stored once)."""
    sh, _ = _height(gpu_pkg, fmt, CASES[4][1])   # nj mod 32 = 9: a strip of one period row at the bottom of full tiles
    inst, borders = _check_batch(gpu_pkg, O, fmt, (SW, sh, 2 * SW, 2 * sh), dict(tap=3), n, 1300 + n, run_knobs={"quad_rg": rg},
                                 mode=gpu_pkg.KernelMode.QUAD, strips=4)
    assert inst[0] == f"ewa_periodic_quad2_kernel<{tname}, {rg}, 1026u, 6>", inst[0]
    assert borders[0] & 64, borders[0]
