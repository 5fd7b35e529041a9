"""jinc_filter_create_out on the device: 4:2:0 / 4:2:2 frames that leave with chroma on the luma grid, 4:4:4 frames that leave
sub-sampled.  Every result is compared, bit for bit, with the CPU oracle's SINGLE-PLANE results under the definition of
include/jincresize_hip.h: plane 0 (and alpha) a Y-only filter with the same arguments, planes 1 and 2 the Y-only twin whose
arguments tests/test_chroma_out_host.py recomputes in Python doubles (twin_kwargs).  Half and bfloat16 planes are defined by the
fp32 path: widened exactly, the fp32 oracle, narrowed with round-to-nearest-even.
The common shape is luma 64 x 48 -> 128 x 96: interior, border rows, border columns and corners on every plane of every pair
(chroma 32 x 24 -> 128 x 96 at 4x, 64 x 48 -> 64 x 48 with a shift, 128 x 96 -> 64 x 48 at 0.5x for the 1x case)."""
import numpy as np
import pytest

from conftest import oracle_kwargs
from test_chroma_out_host import SUBS, luma_kwargs, twin_kwargs
from test_narrowed_words import planar_codes
from test_packed10 import OPAQUE, Y410, PackedSide
from test_strided import INVALID_ARG, Side, planar, run_planar, semi_planar
from test_v210 import V210Side

pytestmark = pytest.mark.gpu

GEOM = (64, 48, 128, 96)
SAME = (64, 48, 64, 48)
DRIFT = (160, 96, 220, 132)   # 1.37x: no phase structure, the frame-lane kernels' plans


# ---- samples and the definition --------------------------------------------------------------------------------------------------

def oracle_y(fmt):
    return "Y32" if (fmt.half or fmt.bfloat16 or fmt.bits == 32) else f"Y{fmt.bits}"


def widen(fmt, p):
    if fmt.half:
        return p.astype(np.float32)
    if fmt.bfloat16:
        return (p.astype(np.uint32) << 16).view(np.float32)
    return p


def narrow(fmt, r):
    if fmt.half:
        return r.astype(np.float16)
    if fmt.bfloat16:   # (finite results only: round to nearest even on the upper 16 bits)
        u = np.ascontiguousarray(r).view(np.uint32)
        return ((u + np.uint32(0x7fff) + ((u >> 16) & np.uint32(1))) >> 16).astype(np.uint16)
    return r


def source_frame(O, fmt, sw, sh, seed):
    ofmt = O.Format(fmt.name, 32 if (fmt.half or fmt.bfloat16) else fmt.bits, fmt.planes, fmt.sub_w, fmt.sub_h)
    planes = O.lcg_frame(ofmt, sw, sh, seed=seed)
    if fmt.half:
        return [p.astype(np.float16) for p in planes]
    if fmt.bfloat16:
        return [(p.view(np.uint32) >> 16).astype(np.uint16) for p in planes]
    return planes


_ORACLES = {}


def definition(O, fmt, geom, out_sub, kw, src):
    """The frame by the definition: every plane from a single-plane oracle filter."""
    sw, sh, tw, th = geom
    key = (oracle_y(fmt), geom, (fmt.sub_w, fmt.sub_h), tuple(out_sub), tuple(sorted(kw.items())))
    if key not in _ORACLES:
        yf = O.FORMATS[oracle_y(fmt)]
        (csw, csh, ctw, cth), ckw = twin_kwargs(sw, sh, tw, th, (fmt.sub_w, fmt.sub_h), out_sub, kw)
        _ORACLES[key] = (O.OracleFilter(yf, sw, sh, tw, th, **oracle_kwargs(luma_kwargs(kw))),
                         O.OracleFilter(yf, csw, csh, ctw, cth, **oracle_kwargs(ckw)))
    luma, chroma = _ORACLES[key]
    out = []
    for i, p in enumerate(src):
        of = chroma if i in (1, 2) else luma
        out.append(narrow(fmt, of.get_frame([np.ascontiguousarray(widen(fmt, p))], threads=4)[0]))
    return out


def assert_frame(got, want, dims, what):
    for i, (w, h) in enumerate(dims):
        a, b = np.ascontiguousarray(got[i][:h, :w]), np.ascontiguousarray(want[i][:h, :w])
        assert a.dtype == b.dtype and a.shape == b.shape == (h, w), (what, i, a.dtype, b.dtype, a.shape, b.shape)
        ua, ub = a.view(f"u{a.dtype.itemsize}"), b.view(f"u{b.dtype.itemsize}")
        bad = np.argwhere(ua != ub)
        assert len(bad) == 0, f"{what}: plane {i} differs at {len(bad)} of {w * h} samples; first (x={bad[0][1]}, y={bad[0][0]}): " \
                              f"got {a[bad[0][0], bad[0][1]]!r}, want {b[bad[0][0], bad[0][1]]!r}"


_FRAMES = {}


def frames_and_wants(O, pkg, name, geom, out_sub, kw, n):
    """n source frames and their definition, computed once per case and left unchanged."""
    fmt = pkg.FORMATS[name]
    key = (name, geom, tuple(out_sub), tuple(sorted(kw.items())))
    have = _FRAMES.setdefault(key, ([], []))
    while len(have[0]) < n:
        src = source_frame(O, fmt, geom[0], geom[1], 500 + len(have[0]))
        have[0].append(src)
        have[1].append(definition(O, fmt, geom, out_sub, kw, src))
    return have[0][:n], have[1][:n]


def make(pkg, name, geom, out, kw):
    return pkg.Filter(pkg.FORMATS[name], *geom, device=0, out_sub=SUBS[out], **kw)


# ---- get_frame: pairs, sample types, taps, sitings ----------------------------------------------------------------------------------

FRAME_CASES = [(f"YUV420P{t}", "444", GEOM, dict(tap=tap)) for t in ("8", "16", "S", "H", "BF") for tap in (3, 4)] + [
    ("YUV422P8", "444", GEOM, {}), ("YUV422PS", "444", GEOM, dict(cplace="mpeg1")),
    ("YUV444P8", "420", GEOM, {}), ("YUV444PS", "420", GEOM, dict(cplace="topleft")),      # chroma 1x with a quarter-sample shift
    ("YUV444P8", "420", SAME, {}), ("YUV444PH", "420", SAME, dict(cplace="mpeg1")),      # chroma 0.5x
    ("YUV420P8", "422", GEOM, {}), ("YUV420P10", "422", GEOM, dict(cplace="topleft")),
    ("YUV422P8", "420", GEOM, {}), ("YUV444P16", "422", GEOM, {}),
    ("YUV420P8", "444", GEOM, dict(cplace="mpeg1")), ("YUV420P8", "444", GEOM, dict(cplace="topleft")),
    ("YUVA420P8", "444", GEOM, {}),
    ("YUV420P8", "444", GEOM, dict(src_left=1.3, src_top=0.7, src_width=60.5, src_height=45.25, blur=0.95)),
    ("YUV420P8", "444", DRIFT, {}),
]


def _id(c):
    return f"{c[0]}_to{c[1]}_{c[2][0]}x{c[2][1]}to{c[2][2]}x{c[2][3]}" + "".join(f"_{k}{v}" for k, v in c[3].items() if k in ("tap", "cplace", "blur"))


@pytest.mark.parametrize("case", FRAME_CASES, ids=_id)
def test_get_frame_is_the_single_plane_oracles(gpu_pkg, O, case):
    name, out, geom, kw = case
    (src,), (want,) = frames_and_wants(O, gpu_pkg, name, geom, SUBS[out], kw, 1)
    f = make(gpu_pkg, name, geom, out, kw)
    chroma = (geom[2] >> SUBS[out][0], geom[3] >> SUBS[out][1])
    assert f.out_dims()[:3] == [(geom[2], geom[3]), chroma, chroma]
    got = f.get_frame(src)
    assert_frame(got, want, f.out_dims(), _id(case))
    f.close()


# ---- process_device: one frame and batches; the frame-lane forms --------------------------------------------------------------------

DEVICE_CASES = [("YUV420P8", "444", GEOM, {}, 1), ("YUV420P8", "444", GEOM, {}, 5), ("YUV420PS", "444", GEOM, dict(tap=4), 3),
                ("YUV444P8", "420", GEOM, {}, 3), ("YUV444PBF", "420", SAME, {}, 2), ("YUV422P16", "444", GEOM, {}, 2),
                ("YUV420P8", "444", DRIFT, {}, 16), ("YUV420P8", "444", DRIFT, {}, 64), ("YUV444PS", "420", DRIFT, {}, 16),
                ("YUV444PS", "420", DRIFT, {}, 64)]


@pytest.mark.parametrize("case", DEVICE_CASES, ids=lambda c: f"{_id(c[:4])}_n{c[4]}")
def test_process_device_is_the_single_plane_oracles(gpu_pkg, O, case):
    torch = pytest.importorskip("torch")
    name, out, geom, kw, n = case
    distinct = min(n, 16)   # (longer batches repeat their first 16 frames: the expectations are computed once)
    frames, wants = frames_and_wants(O, gpu_pkg, name, geom, SUBS[out], kw, distinct)
    f = make(gpu_pkg, name, geom, out, kw)
    got = run_planar(torch, f, [frames[k % distinct] for k in range(n)], n)
    print(f"{_id(case[:4])} n {n}: luma {f.last_kernel(0)}, chroma {f.last_kernel(1)}")
    for k in range(n):
        assert_frame(got[k], wants[k % distinct], f.out_dims(), f"{_id(case[:4])} frame {k} of {n}")
    # the up-scaling chroma plans (fs 7) reach the frame-lane kernels from 16 frames on; the down-scaling chroma of the 4:4:4 -> 4:2:0
    # case (220 -> 110 from 160: fs above 9) from 24 frames on (dispatch.cpp Rules), so its batch of 16 stays on the gather kernel
    if geom == DRIFT and out == "444":
        assert "framelane" in f.last_kernel(0) and "framelane" in f.last_kernel(1), (f.last_kernel(0), f.last_kernel(1))
    f.close()


def test_submit_at_depth_8_with_pageable_planes(gpu_pkg, O):
    name, out, geom, kw, n = "YUV420P8", "444", GEOM, {}, 12
    frames, wants = frames_and_wants(O, gpu_pkg, name, geom, SUBS[out], kw, n)
    f = make(gpu_pkg, name, geom, out, kw)
    f.set_pipeline(8)
    outs = [[gpu_pkg.alloc_plane(w, h, f.fmt.dtype) for (w, h) in f.out_dims()] for _ in range(n)]
    tickets = [f.submit(frames[k], outs[k]) for k in range(n)]
    for k in reversed(range(n)):
        f.wait(tickets[k])
    for k in range(n):
        assert_frame(outs[k], wants[k], f.out_dims(), f"submit frame {k}")
    f.close()


@pytest.mark.parametrize("name,out", [("YUV420P8", "444"), ("YUV444PS", "420")])
def test_batch_process_on_one_device(gpu_pkg, O, name, out):
    n = 6
    frames, wants = frames_and_wants(O, gpu_pkg, name, GEOM, SUBS[out], {}, n)
    b = gpu_pkg.Batch(gpu_pkg.FORMATS[name], *GEOM, ndevices=1, streams=4, out_sub=SUBS[out])
    chroma = (GEOM[2] >> SUBS[out][0], GEOM[3] >> SUBS[out][1])
    assert b.out_dims() == [(GEOM[2], GEOM[3]), chroma, chroma]
    got = b.process(frames)
    for k in range(n):
        assert_frame(got[k], wants[k], b.out_dims(), f"batch frame {k}")
    b.close()


# ---- each chroma plane takes the kernel of its Y-only twin ---------------------------------------------------------------------------

# (the last three sit where the limits on a call's size lie: the whole call's samples and taps are about three times a chroma plane's)
CHOICE_CASES = [("YUV420P8", "444", (320, 180, 480, 270), {}, None), ("YUV420P8", "444", (320, 180, 640, 360), {}, None),
                ("YUV444P8", "420", (320, 180, 640, 360), dict(tap=4), None),
                ("YUV420P8", "444", GEOM, {}, "periodic"), ("YUV420PS", "444", GEOM, dict(tap=4), "periodic"),
                ("YUV444P8", "420", GEOM, {}, None), ("YUV444P8", "420", SAME, {}, "direct"), ("YUV420P8", "444", DRIFT, {}, None)]


@pytest.mark.parametrize("n", [1, 16, 64])
@pytest.mark.parametrize("case", CHOICE_CASES, ids=lambda c: _id(c[:4]))
def test_a_chroma_plane_takes_the_kernel_of_its_twin(gpu_pkg, O, case, n):
    """The twin runs alone, the chroma planes beside a luma plane: same frame count per call, same plane, same pitches."""
    torch = pytest.importorskip("torch")
    name, out, geom, kw, family = case
    fmt = gpu_pkg.FORMATS[name]
    src = source_frame(O, fmt, geom[0], geom[1], 900)
    f = make(gpu_pkg, name, geom, out, kw)
    run_planar(torch, f, [src] * n, n)
    (csw, csh, ctw, cth), ckw = twin_kwargs(*geom, (fmt.sub_w, fmt.sub_h), SUBS[out], kw)
    twin = gpu_pkg.Filter(gpu_pkg.FORMATS[gpu_pkg_y(fmt)], csw, csh, ctw, cth, device=0, **ckw)
    run_planar(torch, twin, [[src[1]]] * n, n)
    mine, its = (f.last_kernel(1), f.last_border(1)), (twin.last_kernel(0), twin.last_border(0))
    print(f"{_id(case[:4])} n {n}: chroma {mine} (instance {f.last_instance(1)}), twin {its} (instance {twin.last_instance(0)})")
    if family:
        assert family in mine[0], mine
    assert mine == its, (mine, its)   # interior kernel and border form
    assert f.last_instance(1) == twin.last_instance(0), (f.last_instance(1), twin.last_instance(0))
    f.close()
    twin.close()


def gpu_pkg_y(fmt):
    return "YH" if fmt.half else "YBF" if fmt.bfloat16 else "Y32" if fmt.bits == 32 else f"Y{fmt.bits}"


# ---- the stand-in calls: each against the planar call on dense planes of the same values ------------------------------------------------

def test_nv12_into_planar_444_fp32_through_widened_scaled(gpu_pkg):
    torch = pytest.importorskip("torch")
    pkg, n = gpu_pkg, 2
    f = make(pkg, "YUV420PS", GEOM, "444", {})
    rng = np.random.default_rng(31)
    raw = [[rng.integers(0, 256, (h, w)).astype(np.uint8) for (w, h) in f.fmt.plane_dims(64, 48)] for _ in range(n)]
    scales, adds = [], []
    for kind in (0, 1, 1):
        s, a = pkg.code_range(8, 1, kind)[:2]   # limited range, luma / chroma
        scales.append(s)
        adds.append(a)
    src = Side(torch, f.fmt.plane_dims(64, 48), np.uint8, semi_planar(), n, seed=11).fill(raw).upload()
    dst = Side(torch, f.out_dims(), np.float32, planar(3), n, seed=12).upload()
    s = torch.cuda.current_stream()
    f.process_device_widened_scaled(src.ptrs(), src.pitches(), src.steps(), None, 8, scales, adds, src.strides(), dst.ptrs(), dst.pitches(),
                                    dst.steps(), dst.strides(), n, stream=s.cuda_stream)
    s.synchronize()
    assert f.last_strided()[:3] == (2, 0, 1)   # Y and the UV pair widened, nothing merged, one slice
    got = dst.frames_and_guards("NV12 -> planar 4:4:4 fp32")
    floats = [[(p.astype(np.float32) * np.float32(sc) + np.float32(ad)).astype(np.float32) for p, sc, ad in zip(planes, scales, adds)] for planes in raw]
    want = run_planar(torch, f, floats, n)
    for k in range(n):
        assert_frame(got[k], want[k], f.out_dims(), f"widened_scaled frame {k}")
        assert got[k][1].shape == (96, 128)
    f.close()


def test_planar_420_10_bit_into_y410_words(gpu_pkg, O):
    """The packed10 call with dense 4:2:0 source planes and a packed destination: the destination side is 4:4:4, the source side not."""
    torch = pytest.importorskip("torch")
    pkg, n = gpu_pkg, 2
    frames, wants = frames_and_wants(O, pkg, "YUV420P10", GEOM, (0, 0), {}, n)
    f = make(pkg, "YUV420P10", GEOM, "444", {})
    src = Side(torch, f.fmt.plane_dims(64, 48), np.uint16, planar(3), n, seed=11).fill(frames).upload()
    dst = PackedSide(torch, f.out_dims(), Y410, n, seed=12).upload()
    s = torch.cuda.current_stream()
    f.process_device_packed10(src.ptrs(), src.pitches(), None, src.strides(), dst.ptrs(), dst.pitches(), Y410, OPAQUE, dst.strides(), n, stream=s.cuda_stream)
    s.synchronize()
    assert f.last_strided()[:3] == (0, 1, 1)
    got = dst.frames_and_guards(OPAQUE, "4:2:0 planes -> Y410")
    want = run_planar(torch, f, frames, n)
    for k in range(n):
        assert_frame(got[k], want[k], f.out_dims(), f"Y410 frame {k} against the planar call")
        assert_frame(got[k], wants[k], f.out_dims(), f"Y410 frame {k} against the oracle")
    f.close()


def test_v210_blocks_into_planar_444(gpu_pkg, O):
    torch = pytest.importorskip("torch")
    pkg, n = gpu_pkg, 2
    frames, wants = frames_and_wants(O, pkg, "YUV422P10", GEOM, (0, 0), {}, n)
    f = make(pkg, "YUV422P10", GEOM, "444", {})
    src = V210Side(torch, f.fmt.plane_dims(64, 48), n, seed=11).fill(frames).upload()
    dst = Side(torch, f.out_dims(), np.uint16, planar(3), n, seed=12).upload()
    s = torch.cuda.current_stream()
    f.process_device_v210(src.ptrs(), src.pitches(), True, src.strides(), dst.ptrs(), dst.pitches(), False, dst.strides(), n, stream=s.cuda_stream)
    s.synchronize()
    assert f.last_strided()[:3] == (1, 0, 1)
    got = dst.frames_and_guards("v210 -> planar 4:4:4")
    want = run_planar(torch, f, frames, n)
    for k in range(n):
        assert_frame(got[k], want[k], f.out_dims(), f"v210 source frame {k} against the planar call")
        assert_frame(got[k], wants[k], f.out_dims(), f"v210 source frame {k} against the oracle")
    f.close()


def test_p010_into_y410_words_in_one_call(gpu_pkg, O):
    """NV12-shaped 10-bit planes with the sample in the HIGH bits of its word (P010) in, Y410 out, on a 4:2:0 -> 4:4:4 filter."""
    torch = pytest.importorskip("torch")
    pkg, n = gpu_pkg, 2
    frames, wants = frames_and_wants(O, pkg, "YUV420P10", GEOM, (0, 0), {}, n)
    f = make(pkg, "YUV420P10", GEOM, "444", {})
    raw = [[(p.astype(np.uint16) << 6) for p in planes] for planes in frames]
    src = Side(torch, f.fmt.plane_dims(64, 48), np.uint16, semi_planar(), n, seed=11).fill(raw).upload()
    dst = PackedSide(torch, f.out_dims(), Y410, n, seed=12).upload()
    s = torch.cuda.current_stream()
    f.process_device_shifted_packed10(src.ptrs(), src.pitches(), src.steps(), [6, 6, 6], src.strides(), dst.ptrs()[0], dst.pitches()[0], Y410, OPAQUE,
                                      dst.strides()[0], n, stream=s.cuda_stream)
    s.synchronize()
    assert f.last_strided()[:3] == (2, 1, 1)   # Y (shifted, step 1) and the UV pair (step 2) split, one pack, one slice
    got = dst.frames_and_guards(OPAQUE, "P010 -> Y410")
    want = run_planar(torch, f, frames, n)
    for k in range(n):
        assert_frame(got[k], want[k], f.out_dims(), f"P010 -> Y410 frame {k} against the planar call")
        assert_frame(got[k], wants[k], f.out_dims(), f"P010 -> Y410 frame {k} against the oracle")
    f.close()


def test_v210_blocks_into_y410_words_in_one_call(gpu_pkg, O):
    torch = pytest.importorskip("torch")
    pkg, n = gpu_pkg, 2
    frames, wants = frames_and_wants(O, pkg, "YUV422P10", GEOM, (0, 0), {}, n)
    f = make(pkg, "YUV422P10", GEOM, "444", {})
    src = V210Side(torch, f.fmt.plane_dims(64, 48), n, seed=11).fill(frames).upload()
    dst = PackedSide(torch, f.out_dims(), Y410, n, seed=12).upload()
    s = torch.cuda.current_stream()
    f.process_device_v210_packed10(src.ptrs()[0], src.pitches()[0], src.strides()[0], dst.ptrs()[0], dst.pitches()[0], Y410, OPAQUE, dst.strides()[0], n,
                                   stream=s.cuda_stream)
    s.synchronize()
    assert f.last_strided()[:3] == (1, 1, 1)
    got = dst.frames_and_guards(OPAQUE, "v210 -> Y410")
    want = run_planar(torch, f, frames, n)
    for k in range(n):
        assert_frame(got[k], want[k], f.out_dims(), f"v210 -> Y410 frame {k} against the planar call")
        assert_frame(got[k], wants[k], f.out_dims(), f"v210 -> Y410 frame {k} against the oracle")
    f.close()


def unit_sources(fmt, n, seed, peak):
    rng = np.random.default_rng(seed)
    return [[narrow(fmt, rng.uniform(-0.1 * peak, 1.1 * peak, (h, w)).astype(np.float32)) for (w, h) in fmt.plane_dims(64, 48)] for _ in range(n)]


def test_444_fp32_into_nv12_through_narrowed(gpu_pkg):
    torch = pytest.importorskip("torch")
    pkg, n = gpu_pkg, 2
    f = make(pkg, "YUV444PS", GEOM, "420", {})
    frames = unit_sources(f.fmt, n, 41, 255)
    src = Side(torch, f.fmt.plane_dims(64, 48), np.float32, planar(3), n, seed=11).fill(frames).upload()
    dst = Side(torch, f.out_dims(), np.uint8, semi_planar(), n, seed=12).upload()
    s = torch.cuda.current_stream()
    f.process_device_narrowed(src.ptrs(), src.pitches(), src.steps(), src.strides(), dst.ptrs(), dst.pitches(), dst.steps(), None, 8, dst.strides(), n,
                              stream=s.cuda_stream)
    s.synchronize()
    assert f.last_strided()[:3] == (0, 2, 1)   # Y at step 1, the UV pair at step 2
    got = dst.frames_and_guards("4:4:4 fp32 -> NV12")
    planar_result = run_planar(torch, f, frames, n)
    for k in range(n):
        want = [np.rint(np.clip(p, 0, 255)).astype(np.uint8) for p in planar_result[k]]
        assert_frame(got[k], want, f.out_dims(), f"narrowed frame {k}")
        assert got[k][1].shape == (48, 64)
    f.close()


def test_444_half_into_v210_through_narrowed_v210(gpu_pkg):
    torch = pytest.importorskip("torch")
    pkg, n = gpu_pkg, 2
    f = make(pkg, "YUV444PH", GEOM, "422", {})
    frames = unit_sources(f.fmt, n, 43, 1023)
    src = Side(torch, f.fmt.plane_dims(64, 48), np.float16, planar(3), n, seed=11).fill(frames).upload()
    dst = V210Side(torch, f.out_dims(), n, seed=12).upload()
    s = torch.cuda.current_stream()
    f.process_device_narrowed_v210(src.ptrs(), src.pitches(), src.steps(), src.strides(), dst.ptrs()[0], dst.pitches()[0], None, None, dst.strides()[0], n,
                                   stream=s.cuda_stream)
    s.synchronize()
    assert f.last_strided()[:3] == (0, 1, 1)
    got = dst.frames_and_guards("4:4:4 half -> v210")
    want = planar_codes(torch, f, frames, n)
    for k in range(n):
        assert_frame(got[k], want[k], f.out_dims(), f"narrowed_v210 frame {k}")
    f.close()


# ---- the shape rules are per side ------------------------------------------------------------------------------------------------------

def _refused(pkg, call, says):
    with pytest.raises(pkg.JincError) as e:
        call()
    assert e.value.code == INVALID_ARG and str(e.value) == says


def test_a_side_of_the_wrong_shape_is_refused_with_the_per_side_text(gpu_pkg):
    pkg = gpu_pkg
    p, i, z = [64, 64, 64], [256, 256, 256], [0, 0, 0]
    f = make(pkg, "YUV444P10", GEOM, "420", {})   # packed source: fine; packed destination: the output is 4:2:0
    _refused(pkg, lambda: f.process_device_packed10(p, i, None, z, p, i, Y410, OPAQUE, z, 1),
             "JincResize: packed 10:10:10:2 words on the destination side need a filter whose output is not sub-sampled (4:4:4); "
             "this filter's output has sub_w 1 and sub_h 1.")
    f.close()
    f = make(pkg, "YUV422P10", GEOM, "444", {})   # v210 source: fine; v210 destination: the output is 4:4:4
    _refused(pkg, lambda: f.process_device_v210(p, i, False, z, p, i, True, z, 1),
             "JincResize: v210 blocks on the destination side need a filter whose output is 4:2:2 (sub_w 1, sub_h 0); "
             "this filter's output has sub_w 0 and sub_h 0.")
    _refused(pkg, lambda: f.process_device_packed10(p, i, Y410, z, p, i, None, OPAQUE, z, 1),
             "JincResize: packed 10:10:10:2 words on the source side need a filter whose input is not sub-sampled (4:4:4); "
             "this filter's input has sub_w 1 and sub_h 0.")
    f.close()
    f = make(pkg, "YUV444PS", GEOM, "420", {})
    _refused(pkg, lambda: f.process_device_narrowed_packed10(p, i, None, z, 64, 512, Y410, OPAQUE, None, None, 0, 1),
             "JincResize: narrowed packed 10:10:10:2 words on the destination side need a filter whose output is not sub-sampled (4:4:4); "
             "this filter's output has sub_w 1 and sub_h 1.")
    _refused(pkg, lambda: f.process_device_narrowed_v210(p, i, None, z, 64, 512, None, None, 0, 1),
             "JincResize: narrowed v210 blocks on the destination side need a filter whose output is 4:2:2 (sub_w 1, sub_h 0); "
             "this filter's output has sub_w 1 and sub_h 1.")
    f.close()
    f = make(pkg, "YUV420PS", GEOM, "444", {})
    _refused(pkg, lambda: f.process_device_widened_packed10(64, 512, Y410, 0, p, i, None, z, 1),
             "JincResize: widened packed 10:10:10:2 words on the source side need a filter whose input is not sub-sampled (4:4:4); "
             "this filter's input has sub_w 1 and sub_h 1.")
    _refused(pkg, lambda: f.process_device_widened_v210(64, 512, 0, p, i, None, z, 1),
             "JincResize: widened v210 blocks on the source side need a filter whose input is 4:2:2 (sub_w 1, sub_h 0); "
             "this filter's input has sub_w 1 and sub_h 1.")
    f.close()
