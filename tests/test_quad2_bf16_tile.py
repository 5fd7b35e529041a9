"""The bf16 pair tile of the 8-bit full-tile frame-pair kernel (ewa_periodic_quad2_kernel<unsigned char, 8, 1026u, 6>,
kernel_periodic_quad2.inc Quad2ShareTile<16, 1, 1, true>): the staged tile holds one 32-bit word per frame pair, each half a sample's bfloat16,
and a lane walks a strip of 16 period rows (tiles of 128 x 64 periods), reading each half with a d16_hi LDS load into a register whose low
half stays zero.  16-bit planes keep the f32 pair tile and strips of 8.

GPU, every byte against the oracle, small planes at the places the new form can go wrong: tile seams and a partial bottom tile whose
last strip is partial, at 2, 3 and 66 frames; bottom tiles that leave exactly wave 3 idle, and one period row; frames of a pair at
different `& 3` leads; samples at both ends of the range.  The same shapes on Y16, which must stay on its own instance.
CPU: the products per strip from the library's compile-time map, and the same count of v_pk_mul_f32 in the walk's ISA listing with no
VALU instruction per window sample."""
import collections
import os
import re

import numpy as np
import pytest

from conftest import assert_planes_equal, oracle_kwargs, to_device, to_host
from test_quad2_share import _check_batch
from test_quad2_strips import _height, _period_rows

SW, SH = 300, 100   # three tile columns of 128 periods, the last one partial
INSTANCE = {"Y8": "ewa_periodic_quad2_kernel<unsigned char, 8, 1026u, 6>", "Y16": "ewa_periodic_quad2_kernel<unsigned short, 8, 1026u, 6>"}
STRIP = {"Y8": 16, "Y16": 8}
PRODUCTS = {8: 991, 16: 1719}   # 13.4 per output pair at 16 rows, 15.5 at 8; the steady state is 91 per source row


def _forced(gpu_pkg, O, fmt, geom, n, seed):
    inst, borders = _check_batch(gpu_pkg, O, fmt, geom, dict(tap=3), n, seed, run_knobs={"quad_rg": 8}, mode=gpu_pkg.KernelMode.QUAD,
                                 strips=4)
    assert inst[0] == INSTANCE[fmt], inst[0]
    assert borders[0] & 64, borders[0]   # the border columns came out of the edge tiles


@pytest.mark.parametrize("fmt", ["Y8", "Y16"])
def test_the_seam_plane_has_a_partial_bottom_tile_with_a_partial_last_strip(pkg, fmt):
    """(CPU) What the GPU cases below rely on: one full tile of 64 period rows and a partial one ending inside a strip of 16."""
    nj = _period_rows(pkg, fmt, SH)
    assert 64 < nj < 128 and (nj - 64) % 16 != 0, nj


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 66])
@pytest.mark.parametrize("fmt", ["Y8", "Y16"])
def test_tile_seams_and_frame_counts(gpu_pkg, O, fmt, n):
    """Even and odd counts (the last pair's high half repeats the low frame) and more than one frame group."""
    _forced(gpu_pkg, O, fmt, (SW, SH, 2 * SW, 2 * SH), n, 4100 + n)


BOTTOMS = [("wave_3_idle", lambda nj: nj % 64 == 48), ("one_period_row", lambda nj: nj % 64 == 1 and nj > 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", BOTTOMS, ids=[c[0] for c in BOTTOMS])
@pytest.mark.parametrize("fmt", ["Y8", "Y16"])
def test_bottom_tiles(gpu_pkg, O, fmt, case):
    sh, nj = _height(gpu_pkg, fmt, case[1])
    assert case[1](nj), (sh, nj)
    _forced(gpu_pkg, O, fmt, (SW, sh, 2 * SW, 2 * sh), 3, 4200 + sh)


def _run_planes(torch, gpu_pkg, fmt, planes, lead, pitch, gap):
    """One forced full-tile call over `planes` (n single-plane frames) laid out in one byte buffer: frame k's plane starts `lead` bytes
    in, frames `pitch * h + gap` bytes apart.  Returns the frames' outputs and the instance that ran."""
    n, (h, w) = len(planes), planes[0].shape
    sb = planes[0].dtype.itemsize
    fstride = pitch * h + gap
    host = np.zeros(lead + n * fstride + 64, np.uint8)
    for k, p in enumerate(planes):
        np.ndarray((h, w), p.dtype, host, lead + k * fstride, (pitch, sb))[...] = p
    src = to_device(torch.from_numpy(host))
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[fmt], w, h, 2 * w, 2 * h, device=0, tap=3)
    f.set_border_strips(4)
    (dw, dh), = f.out_dims()
    dpitch = (dw * sb + 63) // 64 * 64
    dst = torch.zeros((n, dh, dpitch), dtype=torch.uint8, device="cuda")
    f.set_kernel_mode(gpu_pkg.KernelMode.QUAD)
    stream = torch.cuda.current_stream()
    with gpu_pkg.knobs(quad_rg=8):
        f.process_device([src.data_ptr() + lead], [pitch], [fstride], [dst.data_ptr()], [dpitch], [dh * dpitch], n, stream=stream.cuda_stream)
    stream.synchronize()
    inst = f.last_instance(0)
    f.close()
    out = to_host(dst).numpy()
    return [[np.ascontiguousarray(out[k]).view(planes[0].dtype)] for k in range(n)], inst, (dw, dh)


def _against_oracle(O, fmt, planes, got, dims, what):
    h, w = planes[0].shape
    of = O.OracleFilter(O.FORMATS[fmt], w, h, 2 * w, 2 * h, **oracle_kwargs(dict(tap=3)))
    for k, p in enumerate(planes):
        assert_planes_equal(got[k], of.get_frame([p], threads=8), [dims], what=f"{what} frame {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,lead,pitch,gap", [("Y8", 65, 303, 1), ("Y8", 66, 301, 3), ("Y16", 66, 602, 2)],
                         ids=["Y8_odd_pitch_odd_stride", "Y8_lead_2_stride_3", "Y16_lead_2"])
def test_frames_of_a_pair_at_different_leads(gpu_pkg, O, fmt, lead, pitch, gap):
    """Odd pitches and frame strides (303 is the odd pitch of the strided calls' tests): the rows of a frame and the two frames of a pair
    start at different offsets into their dwords, so each takes its own shift into the tile."""
    torch = pytest.importorskip("torch")
    ofmt = O.FORMATS[fmt]
    planes = [np.ascontiguousarray(O.lcg_frame(ofmt, SW, SH, seed=4300 + k)[0][:SH, :SW]) for k in range(3)]   # (without the rows' padding)
    assert (pitch * SH + gap) % 4 != 0
    got, inst, dims = _run_planes(torch, gpu_pkg, fmt, planes, lead, pitch, gap)
    assert inst == INSTANCE[fmt], inst
    _against_oracle(O, fmt, planes, got, dims, f"{fmt} lead {lead} pitch {pitch}")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,peak", [("Y8", 255), ("Y16", 65535)])
def test_extreme_samples(gpu_pkg, O, fmt, peak):
    """All-0 (every chain a sum of zero products, some of them -0), all-peak and checkerboards of both: bf16 is exact at both ends."""
    torch = pytest.importorskip("torch")
    dt = np.uint8 if peak == 255 else np.uint16
    yy, xx = np.mgrid[0:SH, 0:SW]
    checker = (((yy + xx) & 1) * peak).astype(dt)
    planes = [np.zeros((SH, SW), dt), np.full((SH, SW), peak, dt), checker, (peak - checker).astype(dt), np.zeros((SH, SW), dt)]
    pitch = SW * np.dtype(dt).itemsize
    got, inst, dims = _run_planes(torch, gpu_pkg, fmt, planes, 64, pitch, 0)
    assert inst == INSTANCE[fmt], inst
    _against_oracle(O, fmt, planes, got, dims, f"{fmt} extreme samples")


# ------------------------------------------------------------------------------------------------ CPU


def test_products_per_strip(pkg):
    """The (sample, class) pairs some output of a strip takes, from the kernel's own compile-time map: 91 per source row in the steady
    state, 263 on top of H x 91 for the five rows at each end of a strip, whatever its height."""
    L = pkg.lib()
    assert {h: L.jinc_debug_quad2_share_products(h) for h in PRODUCTS} == PRODUCTS
    assert PRODUCTS[16] - 16 * 91 == PRODUCTS[8] - 8 * 91 == 263
    assert PRODUCTS[16] / 128 < 13.5 < 15.4 < PRODUCTS[8] / 64
    assert L.jinc_debug_quad2_share_products(7) == -1


def _kernel_ops(pkg, mangled_part):
    path = [p for p in pkg.ISA_PATHS if p.endswith("kernel_periodic_quad2_rg8-gfx950.s")][0]
    if not os.path.exists(path):
        pkg.build()
    lines = open(path).read().splitlines()
    starts = [i for i, ln in enumerate(lines) if re.match(r"_ZN4jinc\S*" + mangled_part + r"\S*:", ln)]
    assert len(starts) == 1, starts
    end = next(i for i in range(starts[0], len(lines)) if lines[i].startswith(".Lfunc_end"))
    return [ln.split()[0] for ln in lines[starts[0] + 1:end] if ln.startswith("\t") and not ln.strip().startswith((".", ";"))]


def test_the_walk_in_the_isa_listing(pkg):
    """The 8-bit full-tile kernel's strip walk, from its first d16_hi load to the end of the kernel (the staging and the edge columns
    lie in front of it): one v_pk_mul_f32 per product, 30 v_pk_add_f32 per output pair, two d16_hi loads per window sample, and no VALU
    instruction per window sample (147 of them) to shift, mask, merge or convert what was loaded -- the handful allowed here is address
    and predicate arithmetic in front of the walk, counted once per strip.  The output conversions are one v_cvt_pk_u8_f32 per sample."""
    ops = _kernel_ops(pkg, "ewa_periodic_quad2_kernelIhLi8ELj1026ELi6E")
    first = ops.index("ds_read_u16_d16_hi")
    walk = collections.Counter(ops[first:])
    samples = 7 * (16 + 5)
    assert walk["ds_read_u16_d16_hi"] == 2 * samples
    assert walk["v_pk_mul_f32"] == PRODUCTS[16]
    assert walk["v_pk_add_f32"] == 30 * 128
    assert walk["v_cvt_pk_u8_f32"] == 2 * 128
    per_sample = {op: n for op, n in walk.items() if re.match(r"v_(lshl|lshr|ashr|bfe|bfi|perm|and|or|cvt_f32|mov|alignbit|pack)", op)}
    assert sum(per_sample.values()) < 32, per_sample
    assert not [op for op in walk if op.startswith(("ds_read_b", "ds_read2", "ds_write", "scratch_", "v_pk_fma"))], walk
    # Between a d16_hi load and its hand-placed wait the compiler believes the register defined: nothing may copy, re-pair or spill a
    # window register there.  The walk's only moves zero the low halves, in front of the first wait; the walk's waits are the
    # hand-placed ones, one per window sample, and none the compiler added.
    first_wait = first + ops[first:].index("s_waitcnt")
    behind = collections.Counter(ops[first_wait:])
    moved = {op: n for op, n in behind.items() if op.startswith(("v_mov", "v_pk_mov", "v_accvgpr", "v_swap", "scratch_", "v_writelane"))}
    assert moved == {}, moved
    assert walk["s_waitcnt"] == samples
    # the 16-bit instance keeps the f32 pair tile and strips of 8: 128-bit reads, no d16 access at all, and over the whole kernel the
    # walk's 991 products and 30 x 64 adds beside the edge columns' 2 sides x 4 columns x 42 taps of each
    ops16 = collections.Counter(_kernel_ops(pkg, "ewa_periodic_quad2_kernelItLi8ELj1026ELi6E"))
    assert ops16["ds_read_u16_d16_hi"] == 0 and ops16["ds_write_b16_d16_hi"] == 0 and ops16["ds_read_b128"] >= 3 * (8 + 5)
    edge = 2 * 4 * 42
    assert ops16["v_pk_mul_f32"] == PRODUCTS[8] + edge and ops16["v_pk_add_f32"] == 30 * 64 + edge
    assert collections.Counter(ops)["v_pk_mul_f32"] == PRODUCTS[16] + edge and collections.Counter(ops)["v_pk_add_f32"] == 30 * 128 + edge


def test_the_16_bit_kernel_is_the_one_without_the_switch(pkg):
    """The tile's switch leaves the 16-bit instance alone, the staging included: its listing held 287 VALU instructions in front of the
    barrier and 4590 in all before the switch existed, and holds them still.  (The staging indexes a per-lane pointer with wave-uniform
    offsets; folding the lane's term into each store's index cost 75 VALU instructions per wave and 0.2 to 1 % of the 16-bit step.)"""
    ops16 = _kernel_ops(pkg, "ewa_periodic_quad2_kernelItLi8ELj1026ELi6E")
    staging = ops16[:ops16.index("s_barrier")]
    assert sum(op.startswith("v_") for op in staging) == 287
    assert sum(op.startswith("v_") for op in ops16) == 4590
