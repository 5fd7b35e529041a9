"""What the trimmed frame-pair 2x tap-3 interior (ewa_periodic_quad2_kernel<integer, RG, 1026u, 6>, kernel_periodic_quad2.inc quad2_share_body)
puts at risk, against the oracle's bytes, 8- and 16-bit planes, both tile heights through quad_rg:
  * a chain opens with its first product instead of 0 + product, so it may carry -0 where it carried +0: frames of nothing but zeros,
    and zero runs wider than the 6 x 6 support next to full-scale samples;
  * the tile is staged from aligned dwords: source widths of every residue mod 4, a partial last tile column, heights that use the bottom
    clamp, and source planes that are views into a larger buffer full of a non-zero sentinel (a pitch wider than the row, bytes in front of
    the first and behind the last frame, pitches and frame strides that are no multiple of 4), so a staged column or row that was not
    clamped shows as a wrong output.  The buffer always extends past the planes: nothing here depends on a load faulting;
  * the edge tiles' border columns run on frame pairs: 2, 3 and 7 frames on planes so narrow that every tile is an edge tile."""
import numpy as np
import pytest

import test_framelane_pair
import test_quad2_share
from conftest import to_device, to_host
from test_quad2_share import _check_batch

TYPES = [("Y8", "unsigned char"), ("Y16", "unsigned short")]
QUAD2 = "ewa_periodic_quad2_kernel<{}, {}, 1026u, 6>"


def _zero_frames(O, fmt, sw, sh, n, seed):
    return [[np.zeros_like(p) for p in O.lcg_frame(O.FORMATS[fmt], sw, sh, seed=seed)] for _ in range(n)]


def _blocky_frames(O, fmt, sw, sh, n, seed):
    """Noise in which blocks of 12 x 12 samples are all zero or all full scale: zero runs wider than the support next to the peak."""
    ofmt = O.FORMATS[fmt]
    peak = (1 << ofmt.bits) - 1
    out = []
    for k in range(n):
        planes = O.lcg_frame(ofmt, sw, sh, seed=seed + k)
        rng = np.random.default_rng(seed + k)
        kind = rng.integers(0, 3, size=((sh + 11) // 12, (sw + 11) // 12))   # 0: zeros, 1: peak, 2: noise
        kind = np.kron(kind, np.ones((12, 12), dtype=kind.dtype))[:sh, :sw]
        p = planes[0]
        p[:sh, :sw][kind == 0] = 0
        p[:sh, :sw][kind == 1] = peak
        out.append(planes)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("rg", [4, 8])
@pytest.mark.parametrize("frames", [_zero_frames, _blocky_frames], ids=["zeros", "blocks"])
@pytest.mark.parametrize("fmt,tname", TYPES)
def test_chains_that_open_with_a_zero_product(gpu_pkg, O, monkeypatch, fmt, tname, frames, rg):
    monkeypatch.setattr(test_quad2_share, "_frames", frames)
    seed = 5100 if frames is _zero_frames else 5200   # (_check_batch keeps the oracle's frames by seed)
    inst, borders = _check_batch(gpu_pkg, O, fmt, (300, 70, 600, 140), dict(tap=3), 3, seed, run_knobs={"quad_rg": rg},
                                 mode=gpu_pkg.KernelMode.QUAD, strips=4)
    assert inst[0] == QUAD2.format(tname, rg), inst[0]
    assert borders[0] & 64, borders[0]


def _sentinel_runner(sw, sh, lead, row_extra, gap):
    """_run_batch for one-plane formats with the source frames laid into a device buffer of sentinel bytes: `lead` bytes in front of the
    first frame, rows `row_extra` bytes apart beyond their samples, frames `gap` bytes apart beyond their rows, and 4 KB behind."""
    def run(torch, gpu_pkg, f, gfmt, frames, n, mode, pad=64):
        np_dtype = frames[0][0].dtype
        sb = np.dtype(np_dtype).itemsize
        pitch = sw * sb + row_extra
        stride = sh * pitch + gap
        buf = np.full(lead + n * stride + 4096, 0xA5, dtype=np.uint8)
        for k in range(n):
            rows = np.ascontiguousarray(frames[k][0][:sh, :sw]).view(np.uint8).reshape(sh, sw * sb)
            for y in range(sh):
                o = lead + k * stride + y * pitch
                buf[o:o + sw * sb] = rows[y]
        src = to_device(torch.from_numpy(buf))
        tdtype = {1: torch.uint8, 2: torch.int16}[sb]
        (w, h), = f.out_dims()
        dst = torch.zeros((n, h, (w * sb + pad - 1) // pad * pad // sb), dtype=tdtype, device="cuda")
        f.set_kernel_mode(mode)
        stream = torch.cuda.current_stream()
        f.process_device([src.data_ptr() + lead], [pitch], [stride], [dst.data_ptr()], [dst.stride(1) * sb], [dst.stride(0) * sb], n,
                         stream=stream.cuda_stream)
        stream.synchronize()
        return [[to_host(dst[k]).numpy().view(np_dtype)] for k in range(n)]
    return run


# (bytes in front, bytes per row beyond the samples, bytes per frame beyond the rows) x sample size: dense planes, whose rows and frames
# follow each other at once (what a dword holds beside a row's end is the next row), and planes spread out at odd distances
LAYOUTS = {"dense": (0, 0, 0), "spread": (3, 7, 5)}


@pytest.mark.gpu
@pytest.mark.parametrize("rg", [4, 8])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("sw,sh", [(297, 70), (298, 41), (299, 70), (300, 41)])
@pytest.mark.parametrize("fmt,tname", TYPES)
def test_planes_inside_a_buffer_of_sentinels(gpu_pkg, O, monkeypatch, fmt, tname, sw, sh, layout, rg):
    """Three tile columns, the last one partial (its staged columns reach past the plane: replicated), bottom tiles whose staged rows
    do; the widths take every residue mod 4, and with them the dense pitch."""
    sb = 1 if fmt == "Y8" else 2
    lead, row_extra, gap = (v * sb for v in LAYOUTS[layout])   # (16-bit samples stay 2-byte aligned)
    monkeypatch.setattr(test_framelane_pair, "_run_batch", _sentinel_runner(sw, sh, lead, row_extra, gap))
    inst, _ = _check_batch(gpu_pkg, O, fmt, (sw, sh, 2 * sw, 2 * sh), dict(tap=3), 3, 5300 + sw, run_knobs={"quad_rg": rg},
                           mode=gpu_pkg.KernelMode.QUAD, strips=4)
    # (which kernel takes the border columns is the host's call on such planes -- dispatch.cpp direct_ok -- and not asserted here: the
    # interior's staged tile is the subject, and every output sample is compared)
    assert inst[0] == QUAD2.format(tname, rg), inst[0]


@pytest.mark.gpu
@pytest.mark.parametrize("rg", [4, 8])
@pytest.mark.parametrize("n", [2, 3, 7])
@pytest.mark.parametrize("sw", [100, 200], ids=["one_tile_column", "two_tile_columns"])
@pytest.mark.parametrize("fmt,tname", TYPES)
def test_every_tile_is_an_edge_tile(gpu_pkg, O, fmt, tname, sw, n, rg):
    """Both border sides out of one workgroup, or one side each: full pairs, and an odd count's last pair stored once."""
    inst, borders = _check_batch(gpu_pkg, O, fmt, (sw, 90, 2 * sw, 180), dict(tap=3), n, 5400 + n, run_knobs={"quad_rg": rg},
                                 mode=gpu_pkg.KernelMode.QUAD, strips=4)
    assert inst[0] == QUAD2.format(tname, rg), inst[0]
    assert borders[0] & 64, borders[0]
