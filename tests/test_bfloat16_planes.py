"""bfloat16 planes on the GPU, against their definition (include/jincresize_hip.h, JINC_SAMPLE_BFLOAT16; the test-side form is
tests/test_bfloat16_host.py): widen every sample to fp32 (bits << 16), compute what the library computes for the fp32 plane,
narrow the result with round-to-nearest-even.  Expected value: narrow(oracle_fp32(widen(src))), bit for bit, NaN positions compared
but not NaN payloads.  The twin of tests/test_half_planes.py: the same CASES and BATCH_CASES with the formats mapped to bfloat16.

Sample sets: `unit` (the fp32 LCG frame narrowed to bfloat16) and `wide` (test_bfloat16_host.wide_frame: random finite samples of
both signs with biased exponents 0 .. 0xdf, the left quarter 0x7f7f, the bottom quarter subnormals only; the host file asserts on
the oracle alone that its expected planes hold +-inf, subnormals and at least 50 % finite results)."""
import re

import numpy as np
import pytest

from conftest import fresh_planes, to_device, to_host
from test_bfloat16_host import assert_bf16_equal, conversion_set, definition, fp32_name, is_nan, narrow, unit_frame, wide_conditions, wide_frame, widen
from test_half_planes import BATCH_CASES as HALF_BATCH_CASES, CASES as HALF_CASES, _id

pytestmark = pytest.mark.gpu


def bf_name(hname):
    assert hname.endswith("H")
    return hname[:-1] + "BF"


CASES = [(bf_name(c[0]),) + tuple(c[1:]) for c in HALF_CASES]
BATCH_CASES = [(bf_name(c[0]),) + tuple(c[1:]) for c in HALF_BATCH_CASES]

_WANT = {}   # (case id, samples) -> (source, expected planes): the oracle runs once per geometry and sample set, not per kernel mode


def _frame_and_definition(pkg, O, case, samples):
    key = (_id(case), samples)
    if key not in _WANT:
        bname, sw, sh, tw, th, kw = case
        src = unit_frame(O, bname, sw, sh, 4242) if samples == "unit" else wide_frame(pkg, bname, sw, sh, 4242)
        _WANT[key] = (src, definition(O, bname, sw, sh, tw, th, kw, src))
    return _WANT[key]


@pytest.mark.parametrize("samples", ["unit", "wide"])
@pytest.mark.parametrize("mode", [0, 1, 15], ids=["auto", "gather", "full_window"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_get_frame_matches_the_definition(gpu_pkg, O, case, mode, samples):
    bname, sw, sh, tw, th, kw = case
    src, want = _frame_and_definition(gpu_pkg, O, case, samples)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[bname], sw, sh, tw, th, device=0, **kw)
    f.set_kernel_mode(mode)
    got = f.get_frame(src)
    assert_bf16_equal(got, want, f.out_dims(), what=f"{_id(case)} mode {mode} {samples}")
    f.close()


def test_wide_samples_reach_overflow_and_subnormal_results(gpu_pkg, O):
    """The wide sample set does what it is there for: results of +-inf and subnormal results, both on the device as defined."""
    case = ("YBF", 320, 180, 640, 360, {})
    src, want = _frame_and_definition(gpu_pkg, O, case, "wide")
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YBF"], 320, 180, 640, 360, device=0)
    got = f.get_frame(src)
    f.close()
    assert_bf16_equal(got, want, [(640, 360)], what="wide")
    inf, sub, finite = wide_conditions(np.ascontiguousarray(got[0][:360, :640]))
    assert inf and sub and finite >= 0.5, (inf, sub, finite)


def _run_device(torch, f, frames, dims):
    """process_device on a batch of frames (device-resident planes, padded rows); returns the output planes per frame as uint16."""
    n = len(frames)
    sdims = f.fmt.plane_dims(f.src_w, f.src_h)   # (planes of one call may come with different row padding: unit and wide frames)
    src_t = [to_device(torch.stack([torch.from_numpy(np.ascontiguousarray(fr[i][:h, :w]).view(np.int16)) for fr in frames])) for i, (w, h) in enumerate(sdims)]
    dst_t = [torch.zeros((n, h, (w * 2 + 63) // 64 * 32), dtype=torch.int16, device="cuda") for (w, h) in dims]
    f.process_device([t.data_ptr() for t in src_t], [t.stride(1) * 2 for t in src_t], [t.stride(0) * 2 for t in src_t],
                     [t.data_ptr() for t in dst_t], [t.stride(1) * 2 for t in dst_t], [t.stride(0) * 2 for t in dst_t], n)
    torch.cuda.synchronize()
    outs = [to_host(t).numpy().view(np.uint16) for t in dst_t]
    return [[o[k] for o in outs] for k in range(n)]


@pytest.mark.parametrize("n", [1, 16, 128])
@pytest.mark.parametrize("case", BATCH_CASES, ids=_id)
def test_batches_take_the_fp32_kernels(gpu_pkg, O, case, n):
    """process_device batches of distinct frames through the frame-lane, pair and sub-group forms: every frame against the fp32
    filter's own result narrowed, the first and last against the definition, and the bfloat16 filter ran the kernel the fp32 filter
    of the same geometry runs for the same batch."""
    torch = pytest.importorskip("torch")
    bname, sw, sh, tw, th, kw = case
    fb = gpu_pkg.Filter(gpu_pkg.FORMATS[bname], sw, sh, tw, th, device=0, **kw)
    ff = gpu_pkg.Filter(gpu_pkg.FORMATS[fp32_name(bname)], sw, sh, tw, th, device=0, **kw)
    dims = fb.out_dims()
    frames = [unit_frame(O, bname, sw, sh, 900 + k) for k in range(n)]
    got = _run_device(torch, fb, frames, dims)
    kernels_b = [fb.last_kernel(t) for t in range(fb.num_tables)]
    src32 = [[widen(p) for p in fr] for fr in frames]
    src_t = [to_device(torch.stack([torch.from_numpy(np.ascontiguousarray(fr[i])) for fr in src32])) for i in range(len(src32[0]))]
    dst_t = [torch.zeros((n, h, (w * 4 + 63) // 64 * 16), dtype=torch.float32, device="cuda") for (w, h) in dims]
    ff.process_device([t.data_ptr() for t in src_t], [t.stride(1) * 4 for t in src_t], [t.stride(0) * 4 for t in src_t],
                      [t.data_ptr() for t in dst_t], [t.stride(1) * 4 for t in dst_t], [t.stride(0) * 4 for t in dst_t], n)
    torch.cuda.synchronize()
    out32 = [to_host(t).numpy() for t in dst_t]
    assert kernels_b == [ff.last_kernel(t) for t in range(ff.num_tables)]
    for k in range(n):
        want = [narrow(o[k]) for o in out32]
        assert_bf16_equal(got[k], want, dims, what=f"{_id(case)} n={n} frame {k} ({kernels_b[0]})")
    for k in sorted({0, n - 1}):
        assert_bf16_equal(got[k], definition(O, bname, sw, sh, tw, th, kw, frames[k]), dims, what=f"{_id(case)} n={n} frame {k} vs oracle")
    fb.close()
    ff.close()


@pytest.mark.parametrize("mode", [0, 15], ids=["auto", "full_window"])
def test_non_finite_frames_in_a_batch(gpu_pkg, O, mode):
    """Infinities and NaNs at interior, border and corner positions in some frames of a batch: those frames take the full support
    (their result matches the definition, NaNs included) and the finite frames keep the trimmed support's bits: the automatic choice
    runs the trimmed launch and flags exactly the frames that hold a non-finite sample; kernel mode 15 flags nothing.  The finite
    frames hold 0x7f7f and 0x7c00 (65536.0: binary16's infinity pattern, finite here) -- a scan with the wrong exponent mask flags
    them."""
    torch = pytest.importorskip("torch")
    bname, sw, sh, tw, th, kw = "YBF", 320, 180, 640, 360, {}
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[bname], sw, sh, tw, th, device=0, **kw)
    f.set_kernel_mode(mode)
    dims = f.out_dims()
    frames = [unit_frame(O, bname, sw, sh, 300 + k) for k in range(16)]
    INF, NINF, NAN, NAN1 = 0x7f80, 0xff80, 0x7fc0, 0x7f81
    spots = {3: [(90, 160, INF)], 6: [(0, 77, NAN)], 9: [(sh - 1, sw - 1, NINF), (0, 0, NAN1)], 12: [(1, 150, NAN), (100, 2, INF)]}
    for k, s in spots.items():
        for (y, x, v) in s:
            frames[k][0][y, x] = v
    for k in (1, 2):
        frames[k][0][60, 100], frames[k][0][0, 0], frames[k][0][sh - 1, 5] = 0x7c00, 0x7f7f, 0xfc00
    if mode == 0:   # (the automatic choice trims float planes from 1e9 taps per plane and call on: here by the knob)
        with gpu_pkg.knobs(float_trim_min_taps=0):
            got = _run_device(torch, f, frames, dims)
        assert re.fullmatch(r"ewa_periodic_quad2_kernel<__bf16, \d+, \d+u, 6>", f.last_instance(0)), f.last_instance(0)
        assert f.periodic_support(0) == 6 < f.plan_info(0).filter_size
        flags = f.last_finite_flags(0)
        assert flags is not None and flags.tolist() == [1 if k in spots else 0 for k in range(16)], flags
    else:
        got = _run_device(torch, f, frames, dims)
        assert re.fullmatch(r"ewa_periodic_kernel<__bf16, 7, \d+>", f.last_instance(0)), f.last_instance(0)
        assert f.periodic_support(0) == 7 and f.last_finite_flags(0) is None
    for k in range(16):
        want = definition(O, bname, sw, sh, tw, th, kw, frames[k])
        assert_bf16_equal(got[k], want, dims, what=f"frame {k}")
        if k in spots:
            assert is_nan(got[k][0][:th, :tw]).any()
    f.close()


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "shifted_by_one"])
def test_debug_convert_bfloat16_against_the_definition(gpu_pkg, shift):
    """The store conversion on all 65 536 upper halves x six lower halves; the hook runs the single store on elements 4k and 4k + 1
    and the pair store on 4k + 2 (low lane) and 4k + 3 (high lane), so the set shifted by one element gives every value the lanes
    it missed."""
    sums = conversion_set().view(np.float32)
    if shift:
        sums = np.concatenate([np.zeros(shift, np.float32), sums])
    got = gpu_pkg.debug_convert_bfloat16(sums)
    want = narrow(sums)
    assert got.dtype == np.uint16 and got.shape == want.shape
    nan = np.isnan(sums)
    assert np.array_equal(is_nan(got), nan), "NaN positions differ (a NaN must stay a NaN, never become an infinity)"
    bad = np.flatnonzero(got[~nan] != want[~nan])
    assert len(bad) == 0, (f"{len(bad)} conversions differ; first: {sums[~nan][bad[0]]!r} ({sums[~nan].view(np.uint32)[bad[0]]:#010x}) -> "
                           f"{got[~nan][bad[0]]:#06x}, want {want[~nan][bad[0]]:#06x}")


def test_host_paths_match_the_device_result(gpu_pkg, O, pooling_host):
    """get_frame, look-ahead submit / wait at depth 4 on pageable planes and with the library's pool, and one jinc_batch_process on
    one device: all bit-equal to process_device's result (the host surfaces are keyed on the sample size: nothing of theirs changed)."""
    torch = pytest.importorskip("torch")
    bname, sw, sh, tw, th, kw = "YUV420PBF", 320, 180, 640, 360, dict(cplace="mpeg2")
    fmt = gpu_pkg.FORMATS[bname]
    frames = [wide_frame(gpu_pkg, bname, sw, sh, 60 + k) if k % 2 else unit_frame(O, bname, sw, sh, 60 + k) for k in range(6)]
    f = gpu_pkg.Filter(fmt, sw, sh, tw, th, device=0, **kw)
    dims = f.out_dims()
    ref = _run_device(torch, f, frames, dims)
    for k in (0, 1):
        assert_bf16_equal(ref[k], definition(O, bname, sw, sh, tw, th, kw, frames[k]), dims, what=f"device frame {k}")
    assert_bf16_equal(f.get_frame(frames[1]), ref[1], dims, what="get_frame")
    for pin in (gpu_pkg.PIN_NONE, gpu_pkg.PIN_POOL):
        f.set_pipeline(4, pin)
        srcs = [fresh_planes(fmt.plane_dims(sw, sh), np.uint16) for _ in frames]
        for s, fr in zip(srcs, frames):
            for a, b in zip(s, fr):
                a[:, :b.shape[1]] = b[:, :a.shape[1]]
        dsts = [fresh_planes(dims, np.uint16) for _ in frames]
        tickets = [f.submit(s, d) for s, d in zip(srcs, dsts)]
        for k in (2, 0, 5, 1, 3, 4):
            f.wait(tickets[k])
            assert_bf16_equal(dsts[k], ref[k], dims, what=f"submit/wait pin {pin} frame {k}")
        f.set_pipeline(1, gpu_pkg.PIN_NONE)
        del srcs, dsts
    f.close()
    b = gpu_pkg.Batch(fmt, sw, sh, tw, th, ndevices=1, streams=2, **kw)
    outs = b.process(frames)
    b.close()
    for k in range(len(frames)):
        assert_bf16_equal(outs[k], ref[k], dims, what=f"batch frame {k}")


def test_strided_call_writes_interleaved_bfloat16_rgb(gpu_pkg, O):
    """Planar bfloat16 G, B, R in, ONE interleaved RGB buffer out (destination step 3, the planes' bases one sample apart): every
    channel bit-equal to the planar call; the bytes between the rows stay untouched."""
    torch = pytest.importorskip("torch")
    bname, sw, sh, tw, th, kw = "RGBPBF", 131, 77, 262, 154, dict(tap=4)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[bname], sw, sh, tw, th, device=0, **kw)
    dims = f.out_dims()
    frames = [wide_frame(gpu_pkg, bname, sw, sh, 11), unit_frame(O, bname, sw, sh, 12)]
    n = len(frames)
    ref = _run_device(torch, f, frames, dims)
    assert_bf16_equal(ref[1], definition(O, bname, sw, sh, tw, th, kw, frames[1]), dims, what="planar frame 1")
    src_t = [to_device(torch.stack([torch.from_numpy(np.ascontiguousarray(fr[i][:sh, :sw]).view(np.int16)) for fr in frames])) for i in range(3)]
    pitch = 3 * tw * 2 + 10                                   # (a multiple of the sample size, no multiple of 4)
    buf = torch.full((n * th * pitch + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    f.process_device_strided([t.data_ptr() for t in src_t], [t.stride(1) * 2 for t in src_t], None, [t.stride(0) * 2 for t in src_t],
                             [buf.data_ptr() + 2 * c for c in range(3)], [pitch] * 3, [3, 3, 3], [th * pitch] * 3, n)
    torch.cuda.synchronize()
    out = to_host(buf).numpy()
    body = out[:n * th * pitch].reshape(n, th, pitch)
    for k in range(n):
        rgb = np.ascontiguousarray(body[k, :, :3 * tw * 2]).view(np.uint16).reshape(th, tw, 3)
        got = [np.ascontiguousarray(rgb[:, :, c]) for c in range(3)]
        assert_bf16_equal(got, ref[k], dims, what=f"interleaved frame {k}")
    assert (body[:, :, 3 * tw * 2:] == 0xAB).all() and (out[n * th * pitch:] == 0xAB).all()
    with pytest.raises(gpu_pkg.JincError) as e:   # a shift is refused as for binary16
        f.process_device_shifted([t.data_ptr() for t in src_t], [t.stride(1) * 2 for t in src_t], None, [1, 0, 0], [t.stride(0) * 2 for t in src_t],
                                 [buf.data_ptr() + 2 * c for c in range(3)], [pitch] * 3, [3, 3, 3], None, [th * pitch] * 3, n)
    assert e.value.code == -1 and "sample shift" in str(e.value)
    f.close()
