"""Float planes (fp32 and binary16) on the trimmed support with non-finite frames: the path of csrc/dispatch.cpp that runs the
periodic kernels on the bounding box of the phase sets' non-zero coefficients, has the trimmed launch flag the frames in which it
stages an infinity or a NaN (NonFinite<T>, kernel_periodic_common.inc; finite_scan_outside_kernel for the rim no tile stages;
finite_scan_kernel under the knob float_scan) and computes the flagged frames again on the reference's full window.

Every GPU case asserts, in this order:
  (a) the interior ran on the trimmed support: last_instance names the expected kernel family with the sample type and the
      trimmed support (6 for tap 3, 8 for tap 4 -- ewa_periodic_quad8_kernel carries it in its name --, fs - 1 for taps 5 .. 8), and
      periodic_support < filter_size;
  (b) the flags of the call (Filter.last_finite_flags) equal, plane for plane and frame for frame, "this plane of this frame holds a
      non-finite sample" as the host computes it -- a missed flag is wrong pixels, a false one a silently slower call;
  (c) every frame equals its expected value: fp32 the oracle's bits (NaN positions compared, payloads not), binary16
      oracle_fp32(src.astype(float32)).astype(float16) as tests/test_half_planes.py defines it.

The file's last test needs no GPU: it proves from the plan's own tables that the interior spots used here are met by output
samples through a tap whose coefficient is exactly 0.0f, i.e. that a kernel which wrongly kept the trimmed result of such a frame
would miss NaNs the oracle has.  (That is why the GPU tests carry the gpu mark one by one instead of a module-wide pytestmark.)"""
import re

import numpy as np
import pytest

from conftest import oracle_kwargs, to_device, to_host
from test_framelane_pair import _run_batch
from test_half_planes import assert_half_equal, definition

gpu = pytest.mark.gpu

# sample type -> (one-plane format, numpy dtype, the type as the instance names spell it)
TYPES = {"f32": ("Y32", np.float32, "float"), "f16": ("YH", np.float16, "_Float16")}
SW, SH = 150, 70   # the geometry of test_gpu_parity.py::test_one_non_finite_sample_anywhere_in_a_float_plane, at 2x


def _fmt_names(typ, family="Y"):
    """(library format name, oracle format name) of a sample type: Y32 / YH, RGBPS / RGBPH, YUV420PS / YUV420PH."""
    if family == "Y":
        return TYPES[typ][0], "Y32"
    return family + ("S" if typ == "f32" else "H"), family + "S"


def _put(plane, y, x, k):
    """Writes one of +inf, -inf, a quiet NaN and the NaN with the smallest payload (binary16 0x7c01, fp32 0x7f800001: exponent all
    ones and one mantissa bit, where an exponent test and a `> infinity` test on the bits diverge from one that looks at the top
    mantissa bits only) to plane[y, x], as bits."""
    u = {2: np.uint16, 4: np.uint32}[plane.dtype.itemsize]
    patterns = {2: (0x7c00, 0xfc00, 0x7e00, 0x7c01), 4: (0x7f800000, 0xff800000, 0x7fc00000, 0x7f800001)}[plane.dtype.itemsize]
    plane.view(u)[y, x] = patterns[k % 4]


def _spots(sw, sh, fs):
    """Corners, the first and last rows and columns and their neighbours up to fs + 2 in, tile seams, the middle."""
    edge = list(range(0, fs + 2))
    xs = sorted(set(edge + [sw - 1 - e for e in edge] + [x for x in (63, 64, 65, 127, 128, 129) if x < sw] + [sw // 2]))
    ys = sorted(set(edge + [sh - 1 - e for e in edge] + [sh // 2]))
    return [(ys[i % len(ys)], x) for i, x in enumerate(xs)] + [(y, xs[(3 * i) % len(xs)]) for i, y in enumerate(ys)] + \
           [(0, 0), (0, sw - 1), (sh - 1, 0), (sh - 1, sw - 1)]


def _noise(rng, w, h, dtype):
    """Noise of both signs, and in every plane two finite samples next to the top of the format's range (binary16 +-60000 =
    0x7b53, fp32 +-2e38 = 0x7f167699; far enough apart that no window holds both): the largest exponents that are NOT all ones,
    which a flag test that is off by one bit takes for non-finite -- a false flag that only the flag assertion can see."""
    p = (rng.standard_normal((h, w)) * 0.7).astype(dtype)
    big = 60000.0 if np.dtype(dtype).itemsize == 2 else 2e38
    y, x = int(rng.integers(0, h // 2 - 1)), int(rng.integers(0, w // 2 - 1))
    p[y, x] = big
    p[h - 1 - y, w - 1 - x] = -big
    return p


def _want(O, typ, family, sw, sh, kw, src):
    """Expected planes of one frame."""
    lname, oname = _fmt_names(typ, family)
    if typ == "f16":
        return definition(O, lname, sw, sh, 2 * sw, 2 * sh, kw, src)
    return O.OracleFilter(O.FORMATS[oname], sw, sh, 2 * sw, 2 * sh, **oracle_kwargs(kw)).get_frame(src, threads=8)


_BATCHES = {}


def _spot_batch(O, typ, sw, sh, tap, nmin=0):
    """One frame per spot with one non-finite sample there (the four special values in turn), every fourth frame finite; at least
    `nmin` frames (further rounds over the spots).  Returns (frames, expected planes per frame); kept per geometry, since the
    expectation does not depend on the kernel that is asked for."""
    key = (typ, sw, sh, tap, nmin)
    if key not in _BATCHES:
        dtype = TYPES[typ][1]
        fs = O.OracleFilter(O.FORMATS["Y32"], sw, sh, 2 * sw, 2 * sh, tap=tap).tables[0].filter_size
        spots = _spots(sw, sh, fs)
        while len(spots) < nmin:
            spots = spots + spots
        rng = np.random.default_rng(23 + tap)
        srcs = []
        for k, (y, x) in enumerate(spots):
            p = _noise(rng, sw, sh, dtype)
            if k % 4 != 3:
                _put(p, y, x, k // 4 + k)
            srcs.append([p])
        wants = [_want(O, typ, "Y", sw, sh, dict(tap=tap), s) for s in srcs]
        assert any(np.isnan(w[0]).any() for w in wants[:3])
        _BATCHES[key] = (srcs, wants)
    return _BATCHES[key]


def _instance_pattern(typ, tap, n, f, table=0, rg=None):
    """The instance dispatch.cpp (Choice::trimmed, quad_chosen, the variant rules of launch_plane) and launch_periodic reach for a 2x
    float plane on the trimmed support under kernel mode 0 with `n` frames per call:
      tap 3 (6 x 6): two periods per lane (quad2) where the launch fills the chip with its 128 x 24 tiles -- quad2_fills: tiles x
        frames >= 256 -- on half-height tiles (4 row groups) below 12000 full-tile workgroups; otherwise the window kernel on its
        half-height tiles (4 row groups of 6 rows);
      tap 4 (8 x 8): the quad form, one period per lane (float planes never take two), half-height tiles below 6144 workgroups;
      taps 5 .. 8 (10 .. 16 taps per row): the row-pair form.
    The knob quad_rg = 8 / 4 forces the quad forms' tile height."""
    T = TYPES[typ][2]
    info = f.plan_info(table)
    ni = (info.interior_x1 - info.interior_x0) // info.period_x
    nj = (info.interior_y1 - info.interior_y0) // info.period_y
    if tap == 3:
        if ((ni + 127) // 128) * ((nj + 23) // 24) * n >= 256:
            return rf"ewa_periodic_quad2_kernel<{T}, {rg or 4}, \d+u, 6>"
        return rf"ewa_periodic_kernel<{T}, 6, 4>"
    if tap == 4:
        return rf"ewa_periodic_quad8_kernel<{T}, {rg or 4}, \d+u>"
    return rf"ewa_periodic_rowpair_kernel<{T}, {2 * tap}, \d+, \d+>"


def _check(f, typ, srcs, got, wants, patterns, what):
    """(a), (b), (c) of the module docstring for the call that has just run.  `patterns`: per table, the expected instance."""
    n = len(srcs)
    for t, pat in enumerate(patterns):
        assert re.fullmatch(pat, f.last_instance(t)), f"{what}: table {t} ran {f.last_instance(t)!r}, expected {pat}"
        assert 0 < f.periodic_support(t) < f.plan_info(t).filter_size, f"{what}: table {t} has no trimmed support"
    for i in range(f.fmt.planes):
        flags = f.last_finite_flags(i)
        assert flags is not None, f"{what}: plane {i} did not take the flagged path"
        expect = np.array([0 if np.isfinite(srcs[k][i].astype(np.float32)).all() else 1 for k in range(n)], np.uint32)
        print(f"{what}: plane {i} flags {flags.tolist()}")
        assert flags.shape == expect.shape and np.array_equal(flags, expect), \
            f"{what}: plane {i} flags differ in frames {np.flatnonzero(flags != expect).tolist()} (got {flags.tolist()}, expected {expect.tolist()})"
    dims = f.out_dims()
    for k in range(n):
        if typ == "f16":
            assert_half_equal(got[k], wants[k], dims, what=f"{what} frame {k}")
            continue
        for i, (w, h) in enumerate(dims):
            a, b = got[k][i][:h, :w], wants[k][i][:h, :w]
            na, nb = np.isnan(a), np.isnan(b)
            assert np.array_equal(na, nb), f"{what} frame {k} plane {i}: NaN footprint differs ({int(na.sum())} vs {int(nb.sum())})"
            assert np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)), f"{what} frame {k} plane {i}: bits differ"


def _filter(gpu_pkg, typ, sw, sh, tap, family="Y", **kw):
    return gpu_pkg.Filter(gpu_pkg.FORMATS[_fmt_names(typ, family)[0]], sw, sh, 2 * sw, 2 * sh, device=0, tap=tap, **kw)


def _knobs(gpu_pkg, rg=None, **more):
    kv = dict(float_trim_min_taps=0, **more)
    if rg:
        kv["quad_rg"] = rg
    return gpu_pkg.knobs(**kv)


# ---- 1. one non-finite sample anywhere, half planes, forced kernel modes -------------------------------------------------------------

@gpu
@pytest.mark.parametrize("sw", [150, 149], ids=["w150", "w149_last_sample_in_a_low_half"])
@pytest.mark.parametrize("tap", [3, 4, 8])
@pytest.mark.parametrize("mode", [2, 3, 13], ids=["window", "rows", "quad"])
def test_one_non_finite_sample_anywhere_in_a_half_plane(gpu_pkg, O, tap, mode, sw):
    """test_gpu_parity.py::test_one_non_finite_sample_anywhere_in_a_float_plane for binary16 planes: one frame per position of a
    single +inf / -inf / quiet NaN / 0x7c01, every fourth frame finite, under the forced modes (which trim at any call size).  The
    second width puts a row's last sample into the low half of a dword.  Instances: the window kernel (mode 2; taps per row above 9:
    the row-pair form), the rows kernel (mode 3), the quad forms of the 6 x 6 and 8 x 8 supports (mode 13; tap 8 has none: row-pair)."""
    torch = pytest.importorskip("torch")
    srcs, wants = _spot_batch(O, "f16", sw, SH, tap)
    f = _filter(gpu_pkg, "f16", sw, SH, tap)
    n = 2 * tap   # trimmed support
    pat = {2: rf"ewa_periodic_kernel<_Float16, {n}, \d+>" if tap < 5 else rf"ewa_periodic_rowpair_kernel<_Float16, {n}, \d+, \d+>",
           3: rf"ewa_periodic_rows_kernel<_Float16, {n}, \d+>",
           13: {3: r"ewa_periodic_quad2_kernel<_Float16, \d+, \d+u, 6>", 4: r"ewa_periodic_quad8_kernel<_Float16, \d+, \d+u>",
                8: rf"ewa_periodic_rowpair_kernel<_Float16, {n}, \d+, \d+>"}[tap]}[mode]
    got = _run_batch(torch, gpu_pkg, f, f.fmt, srcs, len(srcs), mode)
    _check(f, "f16", srcs, got, wants, [pat], f"YH {sw}x{SH} tap {tap} mode {mode}")
    f.close()


# ---- 2. the automatic choice on the trimmed support ----------------------------------------------------------------------------------

AUTO = [(3, None), (3, 4), (3, 8), (4, None), (4, 4), (4, 8), (5, None), (6, None), (7, None), (8, None)]


@gpu
@pytest.mark.parametrize("tap,rg", AUTO, ids=[f"tap{t}" + (f"_rg{r}" if r else "") for t, r in AUTO])
@pytest.mark.parametrize("typ", sorted(TYPES))
def test_automatic_choice_on_the_trimmed_support(gpu_pkg, O, typ, tap, rg):
    """Kernel mode 0 with float_trim_min_taps = 0 (the rule bench.py's float configurations reach by size): quad2 on 6 x 6 (tap 3 --
    the spot list is 48 frames there, which with two tile columns and three half-height tile rows makes quad2_fills true: 288 >= 256),
    quad8 on 8 x 8 (tap 4), both tile heights through quad_rg, the row-pair form for taps 5 .. 8."""
    torch = pytest.importorskip("torch")
    srcs, wants = _spot_batch(O, typ, SW, SH, tap)
    f = _filter(gpu_pkg, typ, SW, SH, tap)
    pat = _instance_pattern(typ, tap, len(srcs), f, rg=rg)
    assert ("quad2" in pat) == (tap == 3) and ("quad8" in pat) == (tap == 4) and ("rowpair" in pat) == (tap >= 5)
    with _knobs(gpu_pkg, rg):
        got = _run_batch(torch, gpu_pkg, f, f.fmt, srcs, len(srcs), 0)
    _check(f, typ, srcs, got, wants, [pat], f"{typ} tap {tap} rg {rg} auto")
    f.close()


@gpu
@pytest.mark.parametrize("typ", sorted(TYPES))
def test_automatic_choice_on_a_short_batch_takes_the_window_kernels_half_tiles(gpu_pkg, O, typ):
    """Twelve frames of the tap-3 spot list do not fill the chip with quad2's tiles: the 6 x 6 window kernel on half-height tiles."""
    torch = pytest.importorskip("torch")
    srcs, wants = _spot_batch(O, typ, SW, SH, 3)
    pick = [0, 1, 2, 3, 11, 19, 24, 25, 30, 44, 45, 47]
    srcs, wants = [srcs[k] for k in pick], [wants[k] for k in pick]
    f = _filter(gpu_pkg, typ, SW, SH, 3)
    pat = _instance_pattern(typ, 3, len(srcs), f)
    assert pat.startswith("ewa_periodic_kernel<")
    with _knobs(gpu_pkg):
        got = _run_batch(torch, gpu_pkg, f, f.fmt, srcs, len(srcs), 0)
    _check(f, typ, srcs, got, wants, [pat], f"{typ} tap 3 short batch")
    f.close()


@gpu
@pytest.mark.parametrize("family,tap,kw", [("RGBP", 4, {}), ("YUV420P", 3, dict(cplace="mpeg1"))], ids=["RGBP_tap4", "YUV420P_tap3"])
@pytest.mark.parametrize("typ", sorted(TYPES))
def test_automatic_choice_flags_plane_by_plane(gpu_pkg, O, typ, family, tap, kw):
    """Three planes per frame, the non-finite sample in ONE of them, the plane rotating from frame to frame (every fourth frame
    finite): each plane's flags are its own -- the plane index into the ring of flag sets is right, and a chroma plane's flag does not
    reach luma.  (4:2:0 with chroma sited as MPEG-1: luma and chroma both have the 6 x 6 support, which the window kernel takes at
    any call size; 16 frames do not fill the chip with quad2's tiles.)"""
    torch = pytest.importorskip("torch")
    dtype = TYPES[typ][1]
    sw, sh, n = 152, 72, 16
    lname, _ = _fmt_names(typ, family)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[lname], sw, sh, 2 * sw, 2 * sh, device=0, tap=tap, **kw)
    dims = f.fmt.plane_dims(sw, sh)
    fs = f.plan_info(0).filter_size
    rng = np.random.default_rng(31)
    srcs = []
    for k in range(n):
        src = [_noise(rng, w, h, dtype) for (w, h) in dims]
        if k % 4 != 3:
            i = k % 3
            w, h = dims[i]
            y, x = [(h // 2, w // 2), (0, w - 1), (h - 1, 1), (fs, 64 if w > 70 else 33), (2, fs + 1)][k % 5]
            _put(src[i], y, x, k)
        srcs.append(src)
    wants = [_want(O, typ, family, sw, sh, dict(tap=tap, **kw), s) for s in srcs]
    pats = [_instance_pattern(typ, tap, n, f, table=t) for t in range(f.num_tables)]
    with _knobs(gpu_pkg):
        got = _run_batch(torch, gpu_pkg, f, f.fmt, srcs, n, 0)
    _check(f, typ, srcs, got, wants, pats, f"{lname} tap {tap}")
    f.close()


# ---- 3. border forms ---------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("strips", [0, 3], ids=["gather_border", "strip_kernel"])
@pytest.mark.parametrize("tap", [3, 4])
@pytest.mark.parametrize("typ", sorted(TYPES))
def test_border_forms_under_the_trimmed_interior(gpu_pkg, O, typ, tap, strips):
    """The spots within a filter size of each edge give the oracle's NaN footprint whichever kernel computes the border frame, and
    raise the frame's flag although no interior tile may stage them (finite_scan_outside_kernel's rim)."""
    torch = pytest.importorskip("torch")
    srcs, wants = _spot_batch(O, typ, SW, SH, tap)
    f = _filter(gpu_pkg, typ, SW, SH, tap)
    f.set_border_strips(strips)
    pat = _instance_pattern(typ, tap, len(srcs), f)
    with _knobs(gpu_pkg):
        got = _run_batch(torch, gpu_pkg, f, f.fmt, srcs, len(srcs), 0)
    assert strips != 0 or f.last_border(0) == 1, f.last_border(0)   # (1: the gather kernel over the whole border frame)
    _check(f, typ, srcs, got, wants, [pat], f"{typ} tap {tap} border form {strips}")
    f.close()


# ---- 4. the scan pass in front -----------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("sw,sh", [(149, 70), (150, 70), (1030, 45)], ids=["w149", "w150", "w1030_grid_stride_wraps"])
@pytest.mark.parametrize("tap", [3, 4])
@pytest.mark.parametrize("typ", sorted(TYPES))
def test_scan_pass_in_front(gpu_pkg, O, typ, tap, sw, sh):
    """Knob float_scan = 1: finite_scan_kernel reads every source sample and the trimmed launch skips the flagged frames.  Heights
    that are no multiple of its 8 rows per block; at 1030 samples a block's threads come round a second time."""
    torch = pytest.importorskip("torch")
    srcs, wants = _spot_batch(O, typ, sw, sh, tap, nmin=48 if sw < 1000 else 0)
    f = _filter(gpu_pkg, typ, sw, sh, tap)
    pat = _instance_pattern(typ, tap, len(srcs), f)
    with _knobs(gpu_pkg, float_scan=1):
        got = _run_batch(torch, gpu_pkg, f, f.fmt, srcs, len(srcs), 0)
    _check(f, typ, srcs, got, wants, [pat], f"{typ} {sw}x{sh} tap {tap} scan pass")
    f.close()


# ---- 5. padding that holds NaN patterns ----------------------------------------------------------------------------------------------

def _padded_runner(sw, sh, lead, row_extra, gap, fill=0xFF):
    """_run_batch for one-plane formats (the idea of test_quad2_trim.py's _sentinel_runner, for float samples): the source frames lie
    in a device buffer of `fill` bytes -- 0xFF: a NaN in both sample widths -- `lead` bytes behind its start, rows `row_extra` bytes
    apart beyond their samples, frames `gap` bytes apart beyond their rows, and 4 KB behind the last."""
    def run(torch, gpu_pkg, f, gfmt, frames, n, mode, pad=64):
        np_dtype = frames[0][0].dtype
        sb = np.dtype(np_dtype).itemsize
        pitch = sw * sb + row_extra
        stride = sh * pitch + gap
        buf = np.full(lead + n * stride + 4096, fill, dtype=np.uint8)
        for k in range(n):
            rows = np.ascontiguousarray(frames[k][0][:sh, :sw]).view(np.uint8).reshape(sh, sw * sb)
            for y in range(sh):
                o = lead + k * stride + y * pitch
                buf[o:o + sw * sb] = rows[y]
        src = to_device(torch.from_numpy(buf))
        (w, h), = f.out_dims()
        dst = torch.zeros((n, h, (w * sb + pad - 1) // pad * pad), dtype=torch.uint8, device="cuda")
        f.set_kernel_mode(mode)
        stream = torch.cuda.current_stream()
        f.process_device([src.data_ptr() + lead], [pitch], [stride], [dst.data_ptr()], [dst.stride(1)], [dst.stride(0)], n,
                         stream=stream.cuda_stream)
        stream.synchronize()
        return [[to_host(dst[k]).numpy().view(np_dtype)] for k in range(n)]
    return run


@gpu
@pytest.mark.parametrize("sw,sh", [(148, 41), (149, 70), (150, 41), (151, 70)])
@pytest.mark.parametrize("tap", [3, 4, 8])
@pytest.mark.parametrize("typ", sorted(TYPES))
def test_padding_that_holds_nan_patterns_raises_no_flag(gpu_pkg, O, typ, tap, sw, sh):
    """Finite frames inside a buffer of 0xFF bytes: 3 samples in front of the first frame, rows 7 samples and frames 5 samples apart
    beyond their content (for binary16 a pitch and a frame stride that are no multiple of 4 bytes), 4 KB behind.  A staged sample
    that was not clamped to the plane -- the other half of a row's last dword, a column or a row past the edge -- would show as a
    raised flag (and, where a non-zero tap met it, as a NaN): every flag must be 0 and every frame the oracle's.  Widths of every
    residue mod 4, heights whose bottom tiles use the row clamp; 48 frames, so that tap 3 runs quad2."""
    torch = pytest.importorskip("torch")
    dtype = TYPES[typ][1]
    sb = np.dtype(dtype).itemsize
    n = 48 if tap == 3 else 6
    rng = np.random.default_rng(1000 * tap + sw)
    srcs = [[_noise(rng, sw, sh, dtype)] for _ in range(n)]
    wants = [_want(O, typ, "Y", sw, sh, dict(tap=tap), s) for s in srcs]
    f = _filter(gpu_pkg, typ, sw, sh, tap)
    pat = _instance_pattern(typ, tap, n, f)
    with _knobs(gpu_pkg):
        got = _padded_runner(sw, sh, 3 * sb, 7 * sb, 5 * sb)(torch, gpu_pkg, f, f.fmt, srcs, n, 0)
    _check(f, typ, srcs, got, wants, [pat], f"{typ} {sw}x{sh} tap {tap} in 0xFF padding")
    assert not f.last_finite_flags(0).any()
    f.close()


# ---- 6. the ring of flag sets and its reallocation -----------------------------------------------------------------------------------

# Frames per call: growth (3 -> 7 reallocates the sets), a smaller call in larger sets, and 18 calls in all -- more than the 16 flag
# sets of jinc_filter::kForkEvents, so that the ring comes round.  Which frames of a call hold a non-finite sample: none, all, some.
RING_CALLS = [3, 3, 7, 2] + [2] * 14
RING_BAD = [(0,), (), (0, 1, 2, 3, 4, 5, 6), (1,), (), (0, 1), (0,), (1,), (), (0, 1), (1,), (), (0,), (0, 1), (), (1,), (0,), ()]
assert len(RING_CALLS) == len(RING_BAD) == 18 and RING_BAD[1] == () and len(RING_BAD[2]) == RING_CALLS[2]


def _ring_frames(O, typ):
    dtype = TYPES[typ][1]
    rng = np.random.default_rng(77)
    calls = []
    for c, (n, bad) in enumerate(zip(RING_CALLS, RING_BAD)):
        srcs = []
        for k in range(n):
            p = _noise(rng, SW, SH, dtype)
            if k in bad:
                y, x = _spots(SW, SH, 7)[(5 * c + 11 * k) % 48]
                _put(p, y, x, c + k)
            srcs.append([p])
        calls.append((srcs, [_want(O, typ, "Y", SW, SH, dict(tap=3), s) for s in srcs]))
    return calls


@gpu
@pytest.mark.parametrize("typ", sorted(TYPES))
def test_ring_of_flag_sets_call_after_call(gpu_pkg, O, typ):
    """One filter, calls of 3, 3, 7, 2 and fourteen more of 2 frames, different frames non-finite in each (none, all, some): flags and
    outputs after every call -- a set that kept an earlier call's flags, or a set read at the stride of the old allocation, shows."""
    torch = pytest.importorskip("torch")
    calls = _ring_frames(O, typ)
    f = _filter(gpu_pkg, typ, SW, SH, 3)
    with _knobs(gpu_pkg):
        for c, (srcs, wants) in enumerate(calls):
            got = _run_batch(torch, gpu_pkg, f, f.fmt, srcs, len(srcs), 0)
            _check(f, typ, srcs, got, wants, [_instance_pattern(typ, 3, len(srcs), f)], f"{typ} call {c} ({len(srcs)} frames)")
    f.close()


@gpu
@pytest.mark.parametrize("typ", sorted(TYPES))
def test_ring_of_flag_sets_with_calls_queued_on_two_streams(gpu_pkg, O, typ):
    """The same calls queued back to back, in turn on two streams, one synchronise at the end: calls may overlap on the device, and
    none may clear or read a set another still uses.  Outputs only (the hook reads the last call's set)."""
    torch = pytest.importorskip("torch")
    dtype = TYPES[typ][1]
    sb = np.dtype(dtype).itemsize
    calls = _ring_frames(O, typ)
    f = _filter(gpu_pkg, typ, SW, SH, 3)
    (w, h), = f.out_dims()
    tdtype = torch.float32 if typ == "f32" else torch.float16
    src_t = [to_device(torch.stack([torch.from_numpy(np.ascontiguousarray(s[0])) for s in srcs])) for srcs, _ in calls]
    dst_t = [torch.zeros((len(srcs), h, (w * sb + 63) // 64 * 64 // sb), dtype=tdtype, device="cuda") for srcs, _ in calls]
    torch.cuda.synchronize()   # (the uploads and the zero fills are done before the side streams start)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    with _knobs(gpu_pkg):
        f.set_kernel_mode(0)
        for c, (srcs, _) in enumerate(calls):
            s, d = src_t[c], dst_t[c]
            f.process_device([s.data_ptr()], [s.stride(1) * sb], [s.stride(0) * sb], [d.data_ptr()], [d.stride(1) * sb], [d.stride(0) * sb],
                             len(srcs), stream=streams[c % 2].cuda_stream)
    torch.cuda.synchronize()
    for c, (srcs, wants) in enumerate(calls):
        out = to_host(dst_t[c]).numpy()
        for k in range(len(srcs)):
            if typ == "f16":
                assert_half_equal([out[k]], wants[k], [(w, h)], what=f"call {c} frame {k}")
            else:
                a, b = out[k][:h, :w], wants[k][0][:h, :w]
                na, nb = np.isnan(a), np.isnan(b)
                assert np.array_equal(na, nb), f"call {c} frame {k}: NaN footprint differs ({int(na.sum())} vs {int(nb.sum())})"
                assert np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)), f"call {c} frame {k}: bits differ"
    f.close()


# ---- 7. discrimination: the spots are met through zero coefficients (no GPU) --------------------------------------------------------

@pytest.mark.parametrize("tap", [3, 4, 5, 6, 7, 8])
def test_interior_spots_are_met_through_zero_coefficients(pkg, tap):
    """For the middle and the tile-seam spots of the geometry above, from the plan's own tables (a host-only instance: the window
    origin of every output sample and its coefficient set, what jinc_filter_plan_pixel returns sample by sample): the interior
    output samples whose window holds the spot under a coefficient of exactly 0.0f.  The oracle multiplies that tap and gives NaN
    there; a launch on the trimmed support leaves it out.  More than none for every tap: a kernel that kept the trimmed result of
    such a frame cannot pass (b) and (c) above."""
    f = pkg.Filter(pkg.FORMATS["Y32"], SW, SH, 2 * SW, 2 * SH, device=-1, tap=tap)
    info = f.plan_info(0)
    fs = info.filter_size
    assert info.periodic and fs == 2 * tap + 1
    start_x, start_y, ids = f.plan_dump(0)
    sets = f.plan_sets(0)
    interior = np.zeros(ids.shape, bool)
    interior[info.interior_y0:info.interior_y1, info.interior_x0:info.interior_x1] = True
    for (sy, sx) in [(SH // 2, SW // 2), (SH // 2, 63), (SH // 2, 64), (SH // 2, 65), (SH // 2, 127), (SH // 2, 128), (SH // 2, 129)]:
        dy = sy - start_y[:, None] + 0 * start_x[None, :]
        dx = sx - start_x[None, :] + 0 * start_y[:, None]
        inside = (dy >= 0) & (dy < fs) & (dx >= 0) & (dx < fs) & interior
        coeff = sets[ids, np.clip(dy, 0, fs - 1), np.clip(dx, 0, fs - 1)]
        zero_only = int((inside & (coeff == 0.0)).sum())
        assert inside.sum() >= fs * fs and zero_only > 0, f"tap {tap}, spot ({sx}, {sy}): {zero_only} of {int(inside.sum())} outputs"
    f.close()
