"""Half-precision (IEEE binary16) float planes on the GPU, against their definition (include/jincresize_hip.h,
JINC_SAMPLE_FLOAT16): widen every sample to fp32, compute what the library computes for the fp32 plane, narrow the result to
binary16 with round-to-nearest-even.  Expected value: oracle_fp32(src.astype(float32)).astype(float16), bit for bit, NaN
positions compared but not NaN payloads."""
import re

import numpy as np
import pytest

from conftest import fresh_planes, oracle_kwargs, to_device, to_host
from test_half_planes_host import HalfCore, vs  # noqa: F401

pytestmark = pytest.mark.gpu


def fp32_name(hname):
    return "Y32" if hname == "YH" else hname[:-1] + "S"


CASES = [
    ("YH", 64, 48, 160, 120, {}),                                   # non-periodic
    ("YH", 640, 360, 1280, 720, {}),                                # 2x tap 3: quad forms + border frame
    ("YH", 320, 180, 640, 360, {}),                                 # 2x tap 3, one frame's worth of small tiles
    ("YH", 160, 120, 320, 240, dict(tap=8)),                        # 2x tap 8: row-pair form, fs 17
    ("YH", 200, 120, 400, 240, dict(tap=4)),                        # fs 9
    ("YH", 150, 100, 300, 200, dict(tap=2)),                        # fs 5 rows kernel
    ("YH", 131, 77, 262, 154, {}),                                  # ragged tiles
    ("YH", 97, 61, 291, 183, {}),                                   # 3x
    ("YH", 320, 180, 480, 270, {}),                                 # 1.5x: gather
    ("YH", 480, 270, 320, 180, {}),                                 # down-scale: direct kernel
    ("YH", 256, 256, 128, 128, {}),                                 # 2:1 down-scale, source step 2
    ("YH", 50, 40, 120, 96, dict(tap=4, blur=0.98, src_left=-2.5, src_top=1.25, src_width=55, src_height=41.5, quant_x=7, quant_y=13)),
    ("YH", 37, 23, 91, 50, dict(tap=3, blur=0.9, src_left=1.3, src_top=0.7, src_width=33.1, src_height=20.2)),
    ("YUV420PH", 128, 96, 256, 192, dict(cplace="mpeg2")),
    ("YUV420PH", 128, 96, 256, 192, dict(cplace="mpeg1")),
    ("YUV420PH", 128, 96, 256, 192, dict(cplace="topleft")),
    ("YUV420PH", 88, 108, 132, 162, dict(tap=2, quant_x=255, quant_y=67, cplace="mpeg2")),
    ("YUVA420PH", 128, 96, 256, 192, {}),                           # alpha
    ("YUV422PH", 128, 96, 300, 200, {}),
    ("RGBPH", 200, 100, 400, 200, dict(tap=4, blur=0.98)),          # C4 in miniature
]


def _id(c):
    extra = "_".join(f"{k}{v}" for k, v in c[5].items() if k in ("tap", "cplace"))
    return f"{c[0]}_{c[1]}x{c[2]}to{c[3]}x{c[4]}" + (f"_{extra}" if extra else "")


def unit_frame(O, hname, w, h, seed):
    """The LCG frame of the fp32 format (samples in [0, 1]) as binary16."""
    return [p.astype(np.float16) for p in O.lcg_frame(O.FORMATS[fp32_name(hname)], w, h, seed=seed)]


def wide_frame(pkg, hname, w, h, seed):
    """Samples over the whole finite binary16 range, subnormals and both signs included; the left quarter of a plane is 65504 (the
    overshoot beside that step overflows to infinity) and the bottom quarter holds subnormals only (subnormal results)."""
    rng = np.random.default_rng(seed)
    out = []
    for (pw, ph) in pkg.FORMATS[hname].plane_dims(w, h):
        p = pkg.alloc_plane(pw, ph, np.float16)
        bits = rng.integers(0, 0x7c00, size=p.shape, dtype=np.uint16) | (rng.integers(0, 2, size=p.shape, dtype=np.uint16) << 15)
        bits[:, :pw // 4] = 0x7bff
        bits[ph - ph // 4:, pw // 4:] = rng.integers(0, 0x0400, size=bits[ph - ph // 4:, pw // 4:].shape, dtype=np.uint16)
        p.view(np.uint16)[...] = bits
        out.append(p)
    return out


def definition(O, hname, sw, sh, tw, th, kw, src):
    of = O.OracleFilter(O.FORMATS[fp32_name(hname)], sw, sh, tw, th, **oracle_kwargs(kw))
    with np.errstate(over="ignore"):
        return [p.astype(np.float16) for p in of.get_frame([s.astype(np.float32) for s in src], threads=4)]


def assert_half_equal(got, want, dims, what=""):
    for i, (w, h) in enumerate(dims):
        a = np.ascontiguousarray(got[i][:h, :w])
        b = np.ascontiguousarray(want[i][:h, :w])
        assert a.dtype == np.float16 and b.dtype == np.float16
        na, nb = np.isnan(a), np.isnan(b)
        bad = np.argwhere((na != nb) | (~na & (a.view(np.uint16) != b.view(np.uint16))))
        if len(bad):
            y, x = bad[0]
            raise AssertionError(f"{what}: plane {i} differs at {len(bad)} samples; first (x={x}, y={y}): "
                                 f"got {a[y, x]!r} ({a.view(np.uint16)[y, x]:#06x}), want {b[y, x]!r} ({b.view(np.uint16)[y, x]:#06x})")


@pytest.mark.parametrize("samples", ["unit", "wide"])
@pytest.mark.parametrize("mode", [0, 1, 15], ids=["auto", "gather", "full_window"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_get_frame_matches_the_definition(gpu_pkg, O, case, mode, samples):
    hname, sw, sh, tw, th, kw = case
    src = unit_frame(O, hname, sw, sh, 4242) if samples == "unit" else wide_frame(gpu_pkg, hname, sw, sh, 4242)
    want = definition(O, hname, sw, sh, tw, th, kw, src)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[hname], sw, sh, tw, th, device=0, **kw)
    f.set_kernel_mode(mode)
    got = f.get_frame(src)
    assert_half_equal(got, want, f.out_dims(), what=f"{_id(case)} mode {mode} {samples}")
    f.close()


def test_wide_samples_reach_overflow_and_subnormal_results(gpu_pkg, O):
    """The wide sample set does what it is there for: results of +-inf and subnormal results, both on the device as defined."""
    hname, sw, sh, tw, th = "YH", 320, 180, 640, 360
    src = wide_frame(gpu_pkg, hname, sw, sh, 4242)
    want = definition(O, hname, sw, sh, tw, th, {}, src)[0][:th, :tw]
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[hname], sw, sh, tw, th, device=0)
    got = f.get_frame(src)
    f.close()
    assert_half_equal(got, [want], [(tw, th)], what="wide")
    bits = want.view(np.uint16) & 0x7fff
    assert (bits == 0x7c00).any() and ((bits > 0) & (bits < 0x0400)).any()


def _run_device(torch, f, frames, dims):
    """process_device on a batch of frames (device-resident planes, padded rows); returns the output planes per frame."""
    n = len(frames)
    src_t = [to_device(torch.stack([torch.from_numpy(np.ascontiguousarray(fr[i])) for fr in frames])) for i in range(len(frames[0]))]
    dst_t = [torch.zeros((n, h, (w * 2 + 63) // 64 * 32), dtype=torch.float16, device="cuda") for (w, h) in dims]
    f.process_device([t.data_ptr() for t in src_t], [t.stride(1) * 2 for t in src_t], [t.stride(0) * 2 for t in src_t],
                     [t.data_ptr() for t in dst_t], [t.stride(1) * 2 for t in dst_t], [t.stride(0) * 2 for t in dst_t], n)
    torch.cuda.synchronize()
    outs = [to_host(t).numpy() for t in dst_t]
    return [[o[k] for o in outs] for k in range(n)]


BATCH_CASES = [
    ("YH", 160, 90, 219, 123, {}),                  # 1.37x, fs 7: the frame-lane family (64 / 128 frames: the pair form)
    ("YH", 192, 108, 160, 90, {}),                  # 5/6 down-scale, fs 8
    ("YH", 320, 180, 640, 360, {}),                 # 2x: periodic family
    ("YUV420PH", 160, 96, 222, 130, dict(cplace="topleft")),
]


@pytest.mark.parametrize("n", [1, 16, 128])
@pytest.mark.parametrize("case", BATCH_CASES, ids=_id)
def test_batches_take_the_fp32_kernels(gpu_pkg, O, case, n):
    """process_device batches of distinct frames: every frame against the definition, and the half filter ran the kernel the fp32
    filter of the same geometry runs for the same batch (half planes are native on the batch forms, not left on gather)."""
    torch = pytest.importorskip("torch")
    hname, sw, sh, tw, th, kw = case
    fh = gpu_pkg.Filter(gpu_pkg.FORMATS[hname], sw, sh, tw, th, device=0, **kw)
    ff = gpu_pkg.Filter(gpu_pkg.FORMATS[fp32_name(hname)], sw, sh, tw, th, device=0, **kw)
    dims = fh.out_dims()
    frames = [unit_frame(O, hname, sw, sh, 900 + k) for k in range(n)]
    got = _run_device(torch, fh, frames, dims)
    kernels_h = [fh.last_kernel(t) for t in range(fh.num_tables)]
    src32 = [[p.astype(np.float32) for p in fr] for fr in frames]
    src_t = [to_device(torch.stack([torch.from_numpy(np.ascontiguousarray(fr[i])) for fr in src32])) for i in range(len(src32[0]))]
    dst_t = [torch.zeros((n, h, (w * 4 + 63) // 64 * 16), dtype=torch.float32, device="cuda") for (w, h) in dims]
    ff.process_device([t.data_ptr() for t in src_t], [t.stride(1) * 4 for t in src_t], [t.stride(0) * 4 for t in src_t],
                      [t.data_ptr() for t in dst_t], [t.stride(1) * 4 for t in dst_t], [t.stride(0) * 4 for t in dst_t], n)
    torch.cuda.synchronize()
    out32 = [to_host(t).numpy() for t in dst_t]
    assert kernels_h == [ff.last_kernel(t) for t in range(ff.num_tables)]
    for k in range(n):
        with np.errstate(over="ignore"):
            want = [o[k].astype(np.float16) for o in out32]   # the fp32 filter's own result (bit-equal to the oracle elsewhere)
        assert_half_equal(got[k], want, dims, what=f"{_id(case)} n={n} frame {k} ({kernels_h[0]})")
    for k in sorted({0, n - 1}):
        assert_half_equal(got[k], definition(O, hname, sw, sh, tw, th, kw, frames[k]), dims, what=f"{_id(case)} n={n} frame {k} vs oracle")
    fh.close()
    ff.close()


@pytest.mark.parametrize("mode", [0, 15], ids=["auto", "full_window"])
def test_non_finite_frames_in_a_batch(gpu_pkg, O, mode):
    """Infinities and NaNs at interior, border and corner positions in some frames of a batch: those frames take the full support
    (their result matches the definition, NaNs included) and the finite frames keep the trimmed support's bits: the automatic choice
    runs the trimmed launch and flags exactly the frames that hold a non-finite sample; kernel mode 15 flags nothing."""
    torch = pytest.importorskip("torch")
    hname, sw, sh, tw, th, kw = "YH", 320, 180, 640, 360, {}
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[hname], sw, sh, tw, th, device=0, **kw)
    f.set_kernel_mode(mode)
    dims = f.out_dims()
    frames = [unit_frame(O, hname, sw, sh, 300 + k) for k in range(16)]
    spots = {3: [(90, 160, np.inf)], 6: [(0, 77, np.nan)], 9: [(sh - 1, sw - 1, -np.inf), (0, 0, np.nan)], 12: [(1, 150, np.nan), (100, 2, np.inf)]}
    for k, s in spots.items():
        for (y, x, v) in s:
            frames[k][0][y, x] = v
    if mode == 0:   # (the automatic choice trims float planes from 1e9 taps per plane and call on: here by the knob)
        with gpu_pkg.knobs(float_trim_min_taps=0):
            got = _run_device(torch, f, frames, dims)
        # 3 x 8 tiles of 128 x 24 periods x 16 frames fill the chip: two periods per lane on the 6 x 6 support
        assert re.fullmatch(r"ewa_periodic_quad2_kernel<_Float16, \d+, \d+u, 6>", f.last_instance(0)), f.last_instance(0)
        assert f.periodic_support(0) == 6 < f.plan_info(0).filter_size
        flags = f.last_finite_flags(0)
        assert flags is not None and flags.tolist() == [1 if k in spots else 0 for k in range(16)], flags
    else:
        got = _run_device(torch, f, frames, dims)
        assert re.fullmatch(r"ewa_periodic_kernel<_Float16, 7, \d+>", f.last_instance(0)), f.last_instance(0)
        assert f.periodic_support(0) == 7 and f.last_finite_flags(0) is None
    for k in range(16):
        want = definition(O, hname, sw, sh, tw, th, kw, frames[k])
        assert_half_equal(got[k], want, dims, what=f"frame {k}")
        if k in spots:
            assert np.isnan(got[k][0][:th, :tw]).any()
    f.close()


def test_debug_convert_half_against_numpy(gpu_pkg):
    h = np.arange(0, 0x7c00, dtype=np.uint16).view(np.float16)           # every finite non-negative binary16 value
    lo, hi = h[:-1].astype(np.float32), h[1:].astype(np.float32)
    ties = (lo + (hi - lo) / np.float32(2)).astype(np.float32)            # exact midpoints (fp32 holds them): ties at every exponent
    specials = np.array([65504.0, np.nextafter(np.float32(65520.0), np.float32(0)), 65520.0, 65536.0, 1e30, np.inf, -np.inf, np.nan,
                         6.097555e-05, 6.1035156e-05, 0.0, -0.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0000001, 2.0 ** -26, 1e-40,
                         -65520.0, -65519.99, -2.0 ** -25], np.float32)
    rng = np.random.default_rng(5)
    rand = rng.integers(0, 2 ** 32, size=4096, dtype=np.uint64).astype(np.uint32).view(np.float32)
    for sums in (ties, -ties, ties + np.float32(2.0 ** -30) * ties, specials, rand):
        sums = np.ascontiguousarray(sums, dtype=np.float32)
        got = gpu_pkg.debug_convert_half(sums)
        with np.errstate(over="ignore", invalid="ignore"):
            want = sums.astype(np.float16)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        bad = np.flatnonzero(got.view(np.uint16)[~nan] != want.view(np.uint16)[~nan])
        assert len(bad) == 0, f"{len(bad)} conversions differ; first: {sums[~nan][bad[0]]!r} -> {got[~nan][bad[0]]!r}, want {want[~nan][bad[0]]!r}"


def test_host_paths_match_the_device_result(gpu_pkg, O, pooling_host, vs):  # noqa: F811
    """get_frame, look-ahead submit / wait with the library's pinned buffers (0) and cached registrations (2), one
    jinc_batch_process and the VapourSynth shell: all bit-equal to process_device's result."""
    torch = pytest.importorskip("torch")
    hname, sw, sh, tw, th, kw = "YUV420PH", 320, 180, 640, 360, dict(cplace="mpeg2")
    fmt = gpu_pkg.FORMATS[hname]
    frames = [wide_frame(gpu_pkg, hname, sw, sh, 60 + k) if k % 2 else unit_frame(O, hname, sw, sh, 60 + k) for k in range(6)]
    f = gpu_pkg.Filter(fmt, sw, sh, tw, th, device=0, **kw)
    dims = f.out_dims()
    ref = _run_device(torch, f, frames, dims)
    for k in (0, 1):
        assert_half_equal(ref[k], definition(O, hname, sw, sh, tw, th, kw, frames[k]), dims, what=f"device frame {k}")
    assert_half_equal(f.get_frame(frames[1]), ref[1], dims, what="get_frame")
    for pin in (gpu_pkg.PIN_NONE, gpu_pkg.PIN_POOL):
        f.set_pipeline(4, pin)
        srcs = [fresh_planes(fmt.plane_dims(sw, sh), np.float16) for _ in frames]
        for s, fr in zip(srcs, frames):
            for a, b in zip(s, fr):
                a[:, :b.shape[1]] = b[:, :a.shape[1]]
        dsts = [fresh_planes(dims, np.float16) for _ in frames]
        tickets = [f.submit(s, d) for s, d in zip(srcs, dsts)]
        for k in (2, 0, 5, 1, 3, 4):
            f.wait(tickets[k])
            assert_half_equal(dsts[k], ref[k], dims, what=f"submit/wait pin {pin} frame {k}")
        f.set_pipeline(1, gpu_pkg.PIN_NONE)
        del srcs, dsts
    f.close()
    b = gpu_pkg.Batch(fmt, sw, sh, tw, th, ndevices=1, streams=2, **kw)
    outs = b.process(frames)
    b.close()
    for k in range(len(frames)):
        assert_half_equal(outs[k], ref[k], dims, what=f"batch frame {k}")
    c = HalfCore(vs)
    src = c.source_half(fmt, sw, sh, frames[:2])
    node, err = c.invoke("JincResize", src, tw, th, **kw)
    assert err is None, err
    for n in (1, 0):
        fr, err = c.get_frame(node, n)
        assert err is None, err
        got = [c.read_plane(fr, i, np.float16) for i in range(fmt.planes)]
        assert_half_equal(got, ref[n], dims, what=f"VapourSynth frame {n}")
        vs.mockvs_frame_release(fr)
    vs.mockvs_node_release(node)
    vs.mockvs_node_release(src)
    assert c.live() == (0, 0)
    c.close()
