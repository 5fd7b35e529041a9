"""ewa_simd_order_kernel (csrc/kernel_simdorder.hip, the summation orders of the reference's opt = 1 / 2 / 3) on every call form:
batches through jinc_filter_process_device, a pipeline group, the stand-in calls of the integer filters (NV12, P010, Y410, v210), a
float filter behind the widened and narrowed calls, the converting filters of jinc_filter_create_out and frames with non-finite
samples.  tests/test_simd_order.py and the opt rows of tests/golden/reference_sweep.json reach the kernel through Filter.get_frame
alone: one frame, tight host planes, finite samples.

Every comparison is bit for bit; float NaNs compare by position (x86 and the GPU give the default NaN different signs).  The
expectation is always the scalar restatement oracle/simd_order.c (OracleFilter.get_frame_simd / Table.resize_simd), frame by frame
and plane by plane -- never a second run of the product -- and every test asserts that each table's last kernel was
ewa_simd_order_kernel.  The lower clamp of float source samples is what most cases are about: min_val is -0.5 on planes 1 .. of a
YUV clip (alpha included, as the reference's `i && !is_rgb`), 0 on plane 0 and on every plane of an RGB clip."""
import numpy as np
import pytest

import test_narrowed
import test_packed10
import test_shifted
import test_v210
import test_widened
from conftest import oracle_kwargs, to_device, to_host
from test_chroma_out_host import SUBS, luma_kwargs, twin_kwargs
from test_narrowed_host import definition as narrowed_definition
from test_simd_order import _frame
from test_strided import Side, planar, run, run_planar, semi_planar

pytestmark = pytest.mark.gpu

SIMD_KERNEL = "ewa_simd_order_kernel"
ORDERS = dict(argvalues=[1, 2, 3], ids=["sse41_order", "avx2_order", "avx512_order"])
SENTINEL = 0xA5


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want, dims, what):
    """Bit-equal visible planes; on float planes the NaN footprints must coincide and every other sample be bit-equal."""
    for i, (w, h) in enumerate(dims):
        a, b = np.ascontiguousarray(got[i][:h, :w]), np.ascontiguousarray(want[i][:h, :w])
        assert a.dtype == b.dtype and a.shape == b.shape == (h, w), (what, i, a.dtype, b.dtype, a.shape, b.shape)
        ua, ub = bits_of(a), bits_of(b)
        if a.dtype == np.float32:
            na, nb = np.isnan(a), np.isnan(b)
            assert np.array_equal(na, nb), f"{what}: plane {i}: NaN at {int(na.sum())} samples, expected at {int(nb.sum())}; {int((na != nb).sum())} positions differ"
            ua, ub = np.where(na, 0, ua), np.where(nb, 0, ub)
        bad = np.argwhere(ua != ub)
        assert len(bad) == 0, f"{what}: plane {i} differs at {len(bad)} of {w * h} samples; first (x={bad[0][1]}, y={bad[0][0]}): " \
                              f"got {a[bad[0][0], bad[0][1]]!r}, want {b[bad[0][0], bad[0][1]]!r}"


def assert_simd_kernel(f):
    for t in range(f.num_tables):
        assert f.last_kernel(t) == SIMD_KERNEL, (t, f.last_kernel(t))


_ORACLES = {}


def oracle_filter(O, fmt, geom, kw):
    key = (fmt, geom, tuple(sorted(kw.items())))
    if key not in _ORACLES:
        _ORACLES[key] = O.OracleFilter(O.FORMATS[fmt], *geom, **oracle_kwargs(kw))
    return _ORACLES[key]


# ---- 1. batches through process_device -------------------------------------------------------------------------------------------------

BATCH_CASES = [
    ("Y8", (97, 61, 291, 183), {}),                               # fs 7, unrolled
    ("Y16", (150, 100, 300, 200), dict(tap=6)),                   # fs 13, unrolled
    ("Y8", (192, 108, 128, 72), {}),                              # fs 10, generic
    ("Y8", (120, 90, 240, 180), dict(tap=16)),                    # fs 33, generic, three 16-lane groups per kernel row
    ("Y16", (300, 200, 100, 50), dict(tap=4)),                    # generic, down-scale
    ("Y32", (64, 48, 40, 30), {}),                                # generic, float down-scale
    ("YUV420P8", (128, 96, 256, 192), dict(cplace="mpeg2")),      # two tables
    ("YUV444PS", (96, 64, 192, 128), dict(tap=4)),                # chroma clamp -0.5
    ("RGBPS", (96, 64, 150, 100), dict(tap=3, blur=0.98)),        # clamp 0 on all planes
    ("YUVA444PS", (64, 48, 128, 96), {}),                         # the alpha plane clamps at -0.5
    ("RGBAPS", (64, 48, 128, 96), {}),                            # the alpha plane clamps at 0
]
BATCH_FRAMES = 5
_BATCH = {}


def batch_frames_and_wants(O, case, order):
    """Five differently seeded frames of the case and their expectation under `order` (0: the opt = 0 oracle), computed once."""
    fmt, geom, kw = case
    key = (fmt, geom, tuple(sorted(kw.items())))
    if key not in _BATCH:
        _BATCH[key] = ([_frame(O, fmt, geom[0], geom[1], 1000 + 17 * k) for k in range(BATCH_FRAMES)], {})
    frames, wants = _BATCH[key]
    if order not in wants:
        of = oracle_filter(O, fmt, geom, kw)
        wants[order] = [of.get_frame_simd(order, s, threads=4) if order else of.get_frame(s, threads=4) for s in frames]
    return frames, wants[order]


class SentinelPlanes:
    """The planes of `n` frames on one side of a process_device call, each plane in a device buffer of its own that is filled with one
    sentinel byte: the pitch is no multiple of 64, the frame stride is larger than pitch x height and no multiple of the pitch."""

    def __init__(self, torch, dims, dtype, n):
        self.dims, self.dtype, self.n, self.torch = dims, np.dtype(dtype), n, torch
        self.planes = []
        for (w, h) in dims:
            row = w * self.dtype.itemsize
            pitch = (row + 15) // 16 * 16 + 16
            if pitch % 64 == 0:
                pitch += 16
            stride = pitch * h + 48
            assert pitch % 64 != 0 and stride > pitch * h and stride % pitch != 0 and pitch > 48
            self.planes.append(dict(w=w, h=h, row=row, lead=64, pitch=pitch, stride=stride, host=np.full(64 + n * stride + 256, SENTINEL, np.uint8), dev=None))

    def view(self, image, P, k):
        return np.ndarray((P["h"], P["w"]), self.dtype, image, P["lead"] + k * P["stride"], (P["pitch"], self.dtype.itemsize))

    def fill(self, frames):
        for i, P in enumerate(self.planes):
            for k in range(self.n):
                self.view(P["host"], P, k)[...] = frames[k][i][:P["h"], :P["w"]]
        return self

    def upload(self):
        for P in self.planes:
            P["dev"] = to_device(self.torch.from_numpy(P["host"]))
        return self

    def ptrs(self):
        return [P["dev"].data_ptr() + P["lead"] for P in self.planes]

    def pitches(self):
        return [P["pitch"] for P in self.planes]

    def strides(self):
        return [P["stride"] for P in self.planes]

    def frames_and_gaps(self, what):
        """The planes of every frame, after asserting that every byte between rows and frames still holds the sentinel."""
        got = [[None] * len(self.planes) for _ in range(self.n)]
        for i, P in enumerate(self.planes):
            image = to_host(P["dev"]).numpy()
            gap = np.ones(image.size, bool)
            for k in range(self.n):
                np.ndarray((P["h"], P["row"]), np.bool_, gap, P["lead"] + k * P["stride"], (P["pitch"], 1))[...] = False
                got[k][i] = np.ascontiguousarray(self.view(image, P, k))
            written = np.flatnonzero(gap & (image != SENTINEL))
            assert written.size == 0, f"{what}: plane {i}: {written.size} bytes between rows and frames were written, first at byte " \
                                      f"{int(written[0])} (lead {P['lead']}, pitch {P['pitch']}, frame stride {P['stride']}, row {P['row']} bytes)"
        return got


def run_batch(torch, f, frames, n, what):
    src = SentinelPlanes(torch, f.fmt.plane_dims(f.src_w, f.src_h), f.fmt.dtype, n).fill(frames).upload()
    dst = SentinelPlanes(torch, f.out_dims(), f.fmt.dtype, n).upload()
    s = torch.cuda.current_stream()
    f.process_device(src.ptrs(), src.pitches(), src.strides(), dst.ptrs(), dst.pitches(), dst.strides(), n, stream=s.cuda_stream)
    s.synchronize()
    return dst.frames_and_gaps(what)


@pytest.mark.parametrize("order", **ORDERS)
@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("case", BATCH_CASES, ids=lambda c: f"{c[0]}_{c[1][0]}x{c[1][1]}to{c[1][2]}x{c[1][3]}")
def test_batches_through_process_device(gpu_pkg, O, case, n, order):
    """Frames of a batch are the kernel's grid z: both frame strides, and the clamp of every plane kind, on every size path."""
    torch = pytest.importorskip("torch")
    fmt, geom, kw = case
    frames, wants = batch_frames_and_wants(O, case, order)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[fmt], *geom, device=0, **kw)
    f.set_simd_order(order)
    what = f"{fmt} {geom} order {order}, {n} frames"
    got = run_batch(torch, f, frames, n, what)
    assert_simd_kernel(f)
    for k in range(n):
        assert_same(got[k], wants[k], f.out_dims(), f"{what}, frame {k}")
    f.set_simd_order(0)   # back to the parity target on the same filter
    _, wants0 = batch_frames_and_wants(O, case, 0)
    got = run_batch(torch, f, frames, n, what + ", back at order 0")
    assert all(f.last_kernel(t) != SIMD_KERNEL for t in range(f.num_tables))
    for k in range(n):
        assert_same(got[k], wants0[k], f.out_dims(), f"{what}, frame {k} back at order 0")
    f.close()


# ---- 2. a pipeline group ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,geom,kw,order", [("YUV420P8", (128, 96, 256, 192), dict(cplace="mpeg2"), 2), ("Y32", (128, 96, 256, 192), {}, 1)],
                         ids=["YUV420P8_avx2_order", "Y32_sse41_order"])
def test_pipeline_groups_of_four(gpu_pkg, O, fmt, geom, kw, order):
    """Ten frames through submit / wait at depth 8 in groups of 4 (a group is one batch launch: frames in grid z); tickets waited for
    out of order; then order 0 and one synchronous frame on the filter that still has its pipeline."""
    of = oracle_filter(O, fmt, geom, kw)
    srcs = [_frame(O, fmt, geom[0], geom[1], 2000 + 13 * k) for k in range(10)]
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[fmt], *geom, device=0, **kw)
    f.set_simd_order(order)
    f.set_pipeline(depth=8, group=4)
    assert f.pipeline_group == 4
    dsts = [[gpu_pkg.alloc_plane(w, h, f.fmt.dtype) for (w, h) in f.out_dims()] for _ in range(10)]
    tickets = [f.submit(srcs[k], dsts[k]) for k in range(8)]
    for k in (5, 0, 7):
        f.wait(tickets[k])
        assert_simd_kernel(f)
    tickets += [f.submit(srcs[k], dsts[k]) for k in (8, 9)]
    for k in (9, 2, 6, 1, 8, 3, 4):
        f.wait(tickets[k])
    assert_simd_kernel(f)
    for k in range(10):
        assert_same(dsts[k], of.get_frame_simd(order, srcs[k], threads=4), f.out_dims(), f"{fmt} order {order}, frame {k} of the pipeline")
    f.set_simd_order(0)
    got = f.get_frame(srcs[3])
    assert all(f.last_kernel(t) != SIMD_KERNEL for t in range(f.num_tables))
    assert_same(got, of.get_frame(srcs[3], threads=4), f.out_dims(), f"{fmt}: the frame after switching back to order 0")
    f.close()


# ---- 3. stand-in calls on integer filters ----------------------------------------------------------------------------------------------
# The expectation is the restatement's frame of the dense (de-interleaved) source; the helpers of the stand-in tests de-interleave the
# destination (and check its guard bytes and spare bits), which compares the same samples as re-interleaving the expectation.  An
# integer store of the SIMD paths saturates to the TYPE's range, so a 10-bit plane may hold a result above 1023: a 10-bit field keeps
# its low 10 bits, as numpy's own re-interleaving (value << shift in 16 bits, value & 1023 in a field) does.

STAND_IN_FRAMES = 3
STAND_INS = {
    "nv12_strided": ("YUV420P8", (102, 38, 204, 76)),       # odd chroma width 51: vectors and a tail in the split / merge passes
    "p010_shifted": ("YUV420P10", (102, 38, 204, 76)),
    "y410_packed10": ("YUV444P10", (70, 21, 140, 42)),
    "v210": ("YUV422P10", (48, 20, 100, 40)),                 # 48 luma columns in: whole blocks; 100 out: a partial last block of 4
}
_STAND_IN = {}


def stand_in_frames_and_wants(O, name, order):
    fmt, geom = STAND_INS[name]
    if name not in _STAND_IN:
        _STAND_IN[name] = ([O.lcg_frame(O.FORMATS[fmt], geom[0], geom[1], seed=300 + 7 * k) for k in range(STAND_IN_FRAMES)], {})
    frames, wants = _STAND_IN[name]
    if order not in wants:
        of = oracle_filter(O, fmt, geom, dict(tap=3))
        wants[order] = [of.get_frame_simd(order, s, threads=4) for s in frames]
    return frames, wants[order]


def low_bits(frames, bits):
    return [[p & p.dtype.type((1 << bits) - 1) for p in planes] for planes in frames]


@pytest.mark.parametrize("order", **ORDERS)
@pytest.mark.parametrize("name", list(STAND_INS))
def test_stand_in_calls_on_integer_filters(gpu_pkg, O, name, order):
    torch = pytest.importorskip("torch")
    fmt, geom = STAND_INS[name]
    n = STAND_IN_FRAMES
    frames, wants = stand_in_frames_and_wants(O, name, order)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[fmt], *geom, device=0, tap=3)
    f.set_simd_order(order)
    what = f"{name} {fmt} {geom} order {order}"
    s = torch.cuda.current_stream()
    if name == "nv12_strided":
        got = run(torch, f, frames, semi_planar(), semi_planar(), n, what=what)
    elif name == "p010_shifted":
        src, dst = test_shifted.make_sides(torch, f, frames, semi_planar(), semi_planar(), [6] * 3, n)
        test_shifted.call(f, src, dst, [6] * 3, [6] * 3, n, s)
        s.synchronize()
        got = test_shifted.values_of(dst.frames_and_guards(what), [6] * 3, what)
    elif name == "y410_packed10":
        src, dst = test_packed10.make_sides(torch, f, frames, test_packed10.Y410, test_packed10.Y410, n)
        test_packed10.call(f, src, dst, test_packed10.Y410, test_packed10.Y410, test_packed10.OPAQUE, n, s)
        s.synchronize()
        got = test_packed10.results(dst, test_packed10.Y410, test_packed10.OPAQUE, what)
    else:
        src, dst = test_v210.make_sides(torch, f, frames, True, True, n)
        assert src.w % 6 == 0 and dst.w % 6 != 0
        test_v210.call(f, src, dst, True, True, n, s)
        s.synchronize()
        got = dst.frames_and_guards(what)
    assert_simd_kernel(f)
    assert f.last_strided()[:2] != (0, 0), f.last_strided()   # (the stand-in passes ran around the kernel)
    bits = f.fmt.bits
    above = sum(int((p[:h, :w] >= (1 << bits)).sum()) for planes in wants for p, (w, h) in zip(planes, f.out_dims()))
    print(f"{what}: {above} expected samples above the {bits}-bit peak")
    want = wants if bits == 8 else low_bits(wants, bits)
    for k in range(n):
        assert_same(got[k], want[k], f.out_dims(), f"{what}, frame {k}")
    f.close()


# ---- 4. a float filter behind the widened and narrowed calls ---------------------------------------------------------------------------

FLOAT_GEOM = (102, 38, 204, 76)


@pytest.mark.parametrize("order", **ORDERS)
@pytest.mark.parametrize("scaled", [False, True], ids=["code_values", "scaled_to_unit_range"])
def test_nv12_into_a_float_filter_through_the_widened_call(gpu_pkg, O, order, scaled):
    """NV12 -> YUV420PS.  The kernel clamps the WIDENED values, luma at 0 and chroma at -0.5.  Code values 0 .. 255 lie above both
    clamps; the scaled call puts luma on (v - 16) / 255 and chroma on (v - 128) / 255, so that luma values below 0 and chroma values
    below -0.5 (code value 0: -0.50196) exist and chroma values in -0.5 .. 0 must stay."""
    torch = pytest.importorskip("torch")
    n = 3
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YUV420PS"], *FLOAT_GEOM, device=0, tap=3)
    f.set_simd_order(order)
    vals = test_widened.values(gpu_pkg, "YUV420PS", FLOAT_GEOM[0], FLOAT_GEOM[1], 8, n, seed=9)
    raw = test_widened.raw_of(vals, 8, [0] * 3)
    src, dst = test_widened.make_sides(torch, f, raw, semi_planar(), planar(3), n)
    s = torch.cuda.current_stream()
    scale = float(np.float32(1.0 / 255.0))
    offsets = [float(np.float32(-16.0 / 255.0)), float(np.float32(-128.0 / 255.0)), float(np.float32(-128.0 / 255.0))]
    if scaled:
        f.process_device_widened_scaled(src.ptrs(), src.pitches(), src.steps(), None, 8, [scale] * 3, offsets, src.strides(),
                                        dst.ptrs(), dst.pitches(), dst.steps(), dst.strides(), n, stream=s.cuda_stream)
        model = [[p.astype(np.float32) * np.float32(scale) + np.float32(o) for p, o in zip(planes, offsets)] for planes in vals]
        assert min(float(p.min()) for planes in model for p in planes[1:]) < -0.5 and min(float(planes[0].min()) for planes in model) < 0
    else:
        test_widened.call(f, src, dst, None, 8, n, s)
        model = [[p.astype(np.float32) for p in planes] for planes in vals]
    s.synchronize()
    what = f"NV12 into YUV420PS {'scaled ' if scaled else ''}order {order}"
    got = dst.frames_and_guards(what)
    test_widened.assert_source_unchanged(src, what)
    assert_simd_kernel(f)
    of = oracle_filter(O, "YUV420PS", FLOAT_GEOM, dict(tap=3))
    for k in range(n):
        assert_same(got[k], of.get_frame_simd(order, model[k], threads=4), f.out_dims(), f"{what}, frame {k}")
    f.close()


@pytest.mark.parametrize("order", **ORDERS)
def test_a_float_filter_into_8_bit_planes_through_the_narrowed_call(gpu_pkg, O, order):
    """YUV444PS -> planar 8-bit.  The sources run from 0.15 peak below 0 to 0.15 peak above the peak (test_narrowed.sources), so the
    clamp of every plane has work; the stored sample is the numpy narrowing of the restatement's float result."""
    torch = pytest.importorskip("torch")
    n = 2
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YUV444PS"], *FLOAT_GEOM, device=0, tap=3)
    f.set_simd_order(order)
    frames = test_narrowed.sources(f.fmt, FLOAT_GEOM[0], FLOAT_GEOM[1], n, 255, seed=15)
    src, dst = test_narrowed.make_sides(torch, f, frames, planar(3), planar(3), 8, n)
    s = torch.cuda.current_stream()
    test_narrowed.narrowed_call(f, src, dst, None, 8, n, s)
    s.synchronize()
    what = f"YUV444PS into 8-bit planes order {order}"
    got = dst.frames_and_guards(what)
    test_widened.assert_source_unchanged(src, what)
    assert_simd_kernel(f)
    of = oracle_filter(O, "YUV444PS", FLOAT_GEOM, dict(tap=3))
    for k in range(n):
        want = [narrowed_definition(p, 255).astype(np.uint8) for p in of.get_frame_simd(order, frames[k], threads=4)]
        assert_same(got[k], want, f.out_dims(), f"{what}, frame {k}")
    f.close()


# ---- 5. converting filters -------------------------------------------------------------------------------------------------------------

CONVERT_GEOM = (64, 48, 128, 96)
_CONVERT = {}


def converted_frames_and_wants(O, fmt, out, order, n=4):
    """Plane 0: the Y-only twin's restatement (a Y clip: min_val 0).  Planes 1 and 2: the chroma twin's table (tests/test_chroma_out.py)
    under resize_simd with min_val -0.5 given explicitly -- the twin is a Y clip, whose get_frame_simd would clamp at 0."""
    sw, sh, tw, th = CONVERT_GEOM
    ofmt = O.FORMATS[fmt]
    key = (fmt, out)
    if key not in _CONVERT:
        y = O.FORMATS["Y32" if ofmt.bits == 32 else f"Y{ofmt.bits}"]
        (csw, csh, ctw, cth), ckw = twin_kwargs(sw, sh, tw, th, (ofmt.sub_w, ofmt.sub_h), SUBS[out], {})
        _CONVERT[key] = (O.OracleFilter(y, sw, sh, tw, th, **oracle_kwargs(luma_kwargs({}))),
                         O.OracleFilter(y, csw, csh, ctw, cth, **oracle_kwargs(ckw)),
                         [_frame(O, fmt, sw, sh, 3000 + 11 * k) for k in range(n)], {})
    luma, chroma, frames, wants = _CONVERT[key]
    if order not in wants:
        wants[order] = []
        for src in frames:
            planes = [luma.get_frame_simd(order, [src[0]], threads=4)[0]]
            for i in (1, 2):
                d = O.alloc_plane(chroma.target_w, chroma.target_h, ofmt.dtype)
                chroma.tables[0].resize_simd(order, src[i], d, -0.5, threads=4)
                planes.append(d)
            wants[order].append(planes)
    return frames, wants[order]


@pytest.mark.parametrize("order", **ORDERS)
@pytest.mark.parametrize("fmt,out", [("YUV420P8", "444"), ("YUV444PS", "420")], ids=["YUV420P8_to444", "YUV444PS_to420"])
def test_converting_filters(gpu_pkg, O, fmt, out, order):
    """jinc_filter_create_out at 2x luma: the chroma planes' clamp follows the SOURCE clip's plane kind (-0.5), whatever the
    sub-sampling on either side; one frame through get_frame and four through process_device."""
    torch = pytest.importorskip("torch")
    frames, wants = converted_frames_and_wants(O, fmt, out, order)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[fmt], *CONVERT_GEOM, device=0, out_sub=SUBS[out])
    assert f.num_tables == 2
    f.set_simd_order(order)
    what = f"{fmt} -> {out} order {order}"
    got = f.get_frame(frames[0])
    assert_simd_kernel(f)
    assert_same(got, wants[0], f.out_dims(), what + ", get_frame")
    got = run_planar(torch, f, frames, 4)
    assert_simd_kernel(f)
    for k in range(4):
        assert_same(got[k], wants[k], f.out_dims(), f"{what}, frame {k} of 4")
    f.close()


# ---- 6. non-finite float samples -------------------------------------------------------------------------------------------------------

DENORMALS = [1e-41, -3e-39, 1.1e-38]   # (those of tests/golden/make_reference_sweep.source_frame)
# filter sizes 7 and 9, both unrolled in the kernel; the generic loop and the unrolled rows share the clamp (the `tap` lambda)
NONFINITE_CASES = [("Y32", (96, 64, 192, 128), dict(tap=3)), ("YUV444PS", (90, 62, 135, 93), dict(tap=4))]
_NONFINITE = {}


def nonfinite_frames(O, fmt, geom, kw):
    """Four frames on the same finite samples (normal x 0.6, -0.0 sprinkled in) with specials at the four corners, the middle of each
    edge, the centre and about 1 % of the remaining samples:
      all       +inf, -inf, NaN and the three denormals in turn
      no_pinf   the same places, NaN, -inf and the denormals only
      clamped   no_pinf with every NaN and -inf replaced by the plane's min_val
      finite    all with every NaN and -inf replaced by min_val and every +inf by 1.0
    and, per plane, the mask of the output samples whose fs x fs window holds no +inf of `all`."""
    key = (fmt, geom)
    if key in _NONFINITE:
        return _NONFINITE[key]
    sw, sh = geom[0], geom[1]
    of = oracle_filter(O, fmt, geom, kw)
    base = _frame(O, fmt, sw, sh, 4000)
    rng = np.random.default_rng(4001)
    every = np.array([np.inf, -np.inf, np.nan] + DENORMALS, np.float32)
    mild = np.array([np.nan, -np.inf] + DENORMALS, np.float32)
    out = {k: [p.copy() for p in base] for k in ("all", "no_pinf", "clamped", "finite")}
    out["clean_of_pinf"] = []
    for i, (w, h) in enumerate(of.fmt.plane_dims(sw, sh)):
        min_val = np.float32(-0.5 if (i and not of.fmt.rgb) else 0.0)
        zeros = rng.random((h, w)) < 0.01
        for k in ("all", "no_pinf", "clamped", "finite"):
            out[k][i][:h, :w][zeros] = np.float32(-0.0)
        places = [(y, x) for y in (0, h // 2, h - 1) for x in (0, w // 2, w - 1)]
        taken = set(places)
        for j in rng.choice(w * h, (w * h) // 100, replace=False):
            if (int(j) // w, int(j) % w) not in taken:
                places.append((int(j) // w, int(j) % w))
        for k, (y, x) in enumerate(places):
            a, b = every[k % len(every)], mild[k % len(mild)]
            out["all"][i][y, x], out["no_pinf"][i][y, x] = a, b
            out["clamped"][i][y, x] = min_val if (np.isnan(b) or np.isneginf(b)) else b
            out["finite"][i][y, x] = np.float32(1.0) if np.isposinf(a) else (min_val if (np.isnan(a) or np.isneginf(a)) else a)
        t = of.table_for_plane(i)
        fs, meta = t.filter_size, t.meta()
        held = np.zeros((h + 1, w + 1), np.int64)
        held[1:, 1:] = np.cumsum(np.cumsum(np.isposinf(out["all"][i][:h, :w]), axis=0), axis=1)
        x0, y0 = meta[:, :, 0].astype(np.int64), meta[:, :, 1].astype(np.int64)
        assert x0.min() >= 0 and y0.min() >= 0 and (x0 + fs).max() <= w and (y0 + fs).max() <= h
        out["clean_of_pinf"].append((held[y0 + fs, x0 + fs] - held[y0, x0 + fs] - held[y0 + fs, x0] + held[y0, x0]) == 0)
    _NONFINITE[key] = out
    return out


def check_non_finite_properties(frames_out, dims, masks, what):
    """frames_out: name -> planes, computed by ONE implementation (the kernel or the restatement)."""
    for i, (w, h) in enumerate(dims):
        a, b = (bits_of(frames_out[k][i][:h, :w]) for k in ("no_pinf", "clamped"))
        assert not np.isnan(frames_out["no_pinf"][i][:h, :w]).any(), f"{what}: plane {i}: a frame without +inf gave NaN"
        assert np.array_equal(a, b), f"{what}: plane {i}: NaN / -inf samples do not act as min_val at {int((a != b).sum())} samples"
        m = masks[i]
        assert 0 < int(m.sum()) < m.size
        a, b = (bits_of(frames_out[k][i][:h, :w]) for k in ("all", "finite"))
        assert np.array_equal(a[m], b[m]), f"{what}: plane {i}: {int((a[m] != b[m]).sum())} samples with no +inf in their window differ from the finite frame's"


@pytest.mark.parametrize("order", **ORDERS)
@pytest.mark.parametrize("case", NONFINITE_CASES, ids=[c[0] for c in NONFINITE_CASES])
def test_non_finite_float_samples(gpu_pkg, O, case, order):
    """`v > min_val ? v : min_val` is the reference's max_ps(src, min_val): NaN and -inf become min_val.  +inf survives, meets the
    plan's exactly-zero coefficients and becomes NaN inside the sums.  +inf is held to the restatement only: in the reference a +inf to
    the right of the window meets the zero padding of the coefficient row, so its own sample depends on memory outside the window."""
    fmt, geom, kw = case
    of = oracle_filter(O, fmt, geom, kw)
    frames = nonfinite_frames(O, fmt, geom, kw)
    names = ("all", "no_pinf", "clamped", "finite")
    want = {k: of.get_frame_simd(order, frames[k], threads=4) for k in names}
    dims = of.out_dims()
    for i, (w, h) in enumerate(dims):   # the case tests what it is for
        v = want["all"][i][:h, :w]
        assert np.isnan(v).any() and np.isposinf(v).any() and np.isfinite(v).any(), f"plane {i}"
    check_non_finite_properties(want, dims, frames["clean_of_pinf"], f"restatement, {fmt} order {order}")
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[fmt], *geom, device=0, **kw)
    f.set_simd_order(order)
    got = {k: f.get_frame(frames[k]) for k in names}
    assert_simd_kernel(f)
    f.close()
    for k in names:
        assert_same(got[k], want[k], dims, f"{fmt} order {order}, frame '{k}'")
    check_non_finite_properties(got, dims, frames["clean_of_pinf"], f"kernel, {fmt} order {order}")
