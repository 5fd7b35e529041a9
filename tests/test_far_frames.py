"""Every kernel form at offsets beyond 4 GiB: small frames whose frame strides, or whose own rows, put them more than 2^31 and more
than 2^32 bytes behind the plane pointer the library is given, compared bit for bit with oracle/ frame by frame.

The workload's own batches live there (1024 frames of 1920 x 1080 -> 3840 x 2160 have an 8.5 GB destination); the rest of the suite
keeps its frames a few MB apart, so a truncated `frame * stride`, a 32-bit `row * pitch` or a signed buffer offset passes it.

Layout (class Arenas, one per module).  Two device buffers of ~6 GiB, source and destination, from torch.empty: never filled, never
downloaded.  The base handed to the library is arena + 2^31 + MARGIN, and the arena ends at base + 2^32 + MARGIN + LARGEST.  A
signed 32-bit truncation of any offset lands in [base - 2^31, base + 2^31), an unsigned one in [base, base + 2^32), and a plane with
its guards (at most MARGIN bytes) behind such a wrong origin still ends inside the allocation.

    INVARIANT: a latent addressing bug shows as wrong bytes or a disturbed guard, never as a memory fault.

Arenas.place asserts it for every (stride, pitch, n, plane size) it is given.  Every destination plane lies between two guard
windows of GUARD bytes (at least two rows) of a sentinel byte, which also fills the pitch gap of every row; only planes and guards
are read back, and a guard byte that changed fails the case with frame, plane and offset.  Every frame of a batch has its own seed:
a load from a wrapped address reads another frame's samples (or memory nobody wrote) and cannot compare equal.

Frame strides: ceil((2^32 + MARGIN) / (n - 1)) rounded up to the sample size, once as a multiple of 4 bytes and once as no multiple
of 4 (what the direct kernel and the strip border refuse, so those plans run elsewhere; 4-byte samples have the first only).  With
n = 3 frame 1 lies beyond 2^31 and frame 2 beyond 2^32.  Each interior form runs with a far source and a dense destination, a dense
source and a far destination, and both far, so that a store bug and a load bug are told apart.

Each case forces its form as the form's own test file does (kernel mode, knobs, border strips) and asserts last_instance /
last_kernel / last_border: a case whose kernel is not the one it was written for fails, it does not skip.  The module skips as a
whole, and only, when the device has less free memory than the two arenas need.

Beside the one-plane batches: the chroma planes of ONE frame more than 2^31 / 2^32 bytes apart (dispatch.cpp's plane_pair), and the
stand-in calls (NV12, P010, Y410, v210, widened, narrowed) with their packed side moved into an arena at far strides, each against
the oracle and against the planar call, with last_strided and the direction of last_groups asserted.

Planes that span 4 GiB themselves: a destination plane just below 2^32 bytes whose last rows start beyond 2^31 is written correctly;
one of 2^32 bytes or more is refused, and so is a source plane of 2^32 bytes or more (tests/test_far_frames_host.py pins both
messages without a device)."""
import re

import numpy as np
import pytest

from conftest import oracle_kwargs
from test_bfloat16_host import definition as bf16_definition, is_nan as bf16_is_nan, unit_frame as bf16_unit_frame
from test_half_planes import definition as half_definition, unit_frame as half_unit_frame

pytestmark = pytest.mark.gpu

G31, G32 = 1 << 31, 1 << 32
MARGIN = 4 << 20       # >= the largest plane with its guards; also what a last frame's offset may exceed 2^32 by
LARGEST = 1 << 20      # >= the largest plane (384 x 216 float samples, rows padded: 345 600 bytes) with its guards
GUARD = 4096
ARENA_BYTES = G31 + MARGIN + G32 + MARGIN + LARGEST
SENTINEL = 0xA5
MAX_W, MAX_H = 384, 216

# format -> (oracle format, numpy dtype of the planes, the sample type as the instance names spell it)
TYPES = {"Y8": ("Y8", np.uint8, "unsigned char"), "Y16": ("Y16", np.uint16, "unsigned short"), "Y10": ("Y10", np.uint16, "unsigned short"),
         "Y32": ("Y32", np.float32, "float"), "YH": ("Y32", np.float16, "_Float16"), "YBF": ("Y32", np.uint16, "__bf16")}


def far_stride(n, sb, multiple_of_4):
    """ceil((2^32 + MARGIN) / (n - 1)) as a multiple of the sample size: of 4 bytes, or (1- and 2-byte samples) of no 4."""
    s = -(-(G32 + MARGIN) // max(n - 1, 1))
    s = -(-s // 4) * 4
    if not multiple_of_4:
        assert sb < 4
        s += sb
    assert s % sb == 0 and (s % 4 == 0) == multiple_of_4
    return s


class Arenas:
    """The two buffers, where a batch's frames lie in them, the copies in and out, the guards."""

    def __init__(self, torch):
        self.torch = torch
        self.src = torch.empty(ARENA_BYTES, dtype=torch.uint8, device="cuda")
        self.dst = torch.empty(ARENA_BYTES, dtype=torch.uint8, device="cuda")

    def release(self):
        self.src = self.dst = None
        self.torch.cuda.empty_cache()

    @staticmethod
    def base_offset():
        return G31 + MARGIN

    def base(self, arena):
        return arena.data_ptr() + self.base_offset()

    def place(self, n, pitch, rows, row_bytes, stride, first=0):
        """Offsets from the base of the n planes of one batch (frame k at first + k * stride), after the invariant of the module
        docstring has been asserted for them."""
        plane = pitch * (rows - 1) + row_bytes
        spanning = plane > LARGEST            # a plane that spans GiB itself (its frames lie in its pitch gap, close to the base)
        assert row_bytes <= pitch and (spanning or 2 * pitch <= GUARD), (pitch, rows, row_bytes)
        # what lies behind an origin the kernel got wrong: the whole plane, or (spanning planes: the wrong value is a row's offset) a row
        extent = row_bytes if spanning else plane
        assert n == 1 or stride >= extent + 2 * GUARD, f"frames overlap: stride {stride}, {extent} bytes with guards"
        offs = [first + k * stride for k in range(n)]
        lo, hi = -self.base_offset(), ARENA_BYTES - self.base_offset()     # the arena as offsets from the base
        for o in offs:
            assert 0 <= o - GUARD and o + plane + GUARD <= hi, f"frame at {o:#x} leaves the arena"
        assert not spanning or (plane < G32 and offs[-1] <= MARGIN)
        # a signed truncation of any offset is at least -2^31, an unsigned one below 2^32; a spanning plane's frame origin is exact
        # (below MARGIN) and its row offsets are what may be truncated:
        assert lo <= -G31 - GUARD, "a signed truncation leaves the arena"
        assert (offs[-1] if spanning else 0) + G32 + extent + GUARD <= hi, "an unsigned truncation leaves the arena"
        return offs

    def _view(self, arena, off, rows, row_bytes, pitch):
        return arena.as_strided((rows, row_bytes), (pitch, 1), self.base_offset() + off)

    def _pinned(self, a):
        t = self.torch.empty(a.shape, dtype=self.torch.uint8, pin_memory=True)
        t.numpy()[...] = a
        return t

    def upload(self, off, rows_u8, pitch, fill=0xFF):
        """One source plane (a 2-D uint8 array of its rows) at `off`; its guards and row gaps hold `fill` (a NaN in every float type)."""
        rows, row_bytes = rows_u8.shape
        plane = pitch * (rows - 1) + row_bytes
        if plane <= MARGIN:
            a0 = self.base_offset() + off - GUARD
            self.src[a0:a0 + plane + 2 * GUARD].fill_(fill)
        self._view(self.src, off, rows, row_bytes, pitch).copy_(self._pinned(rows_u8))

    def arm(self, off, rows, row_bytes, pitch):
        """Sentinel over a destination plane, its row gaps and both guards (planes that span GiB: the guards and each row's surroundings)."""
        plane = pitch * (rows - 1) + row_bytes
        a0 = self.base_offset() + off
        if plane <= MARGIN:
            self.dst[a0 - GUARD:a0 + plane + GUARD].fill_(SENTINEL)
            return
        for y in range(rows):
            self.dst[a0 + y * pitch - GUARD:a0 + y * pitch + row_bytes + GUARD].fill_(SENTINEL)

    def download(self, off, rows, row_bytes, pitch, what):
        """The rows of a destination plane (2-D uint8), after its guards and gaps were found untouched."""
        plane = pitch * (rows - 1) + row_bytes
        a0 = self.base_offset() + off
        if plane <= MARGIN:
            host = self.torch.empty(plane + 2 * GUARD, dtype=self.torch.uint8, pin_memory=True)
            host.copy_(self.dst[a0 - GUARD:a0 + plane + GUARD])
            raw = host.numpy()
            body = np.full(rows * pitch, SENTINEL, np.uint8)
            body[:plane] = raw[GUARD:GUARD + plane]
            body = body.reshape(rows, pitch)
            untouched = np.ones(raw.shape, bool)
            untouched[GUARD:GUARD + plane] = (np.arange(plane) % pitch) >= row_bytes
            bad = np.flatnonzero(untouched & (raw != SENTINEL))
            assert bad.size == 0, f"{what}: {bad.size} guard bytes changed, first at plane offset {int(bad[0]) - GUARD} (row {(int(bad[0]) - GUARD) // pitch})"
            return np.ascontiguousarray(body[:, :row_bytes])
        out = np.empty((rows, row_bytes), np.uint8)
        host = self.torch.empty(row_bytes + 2 * GUARD, dtype=self.torch.uint8, pin_memory=True)
        for y in range(rows):
            host.copy_(self.dst[a0 + y * pitch - GUARD:a0 + y * pitch + row_bytes + GUARD])
            raw = host.numpy()
            out[y] = raw[GUARD:GUARD + row_bytes]
            bad = np.flatnonzero(np.concatenate([raw[:GUARD], raw[GUARD + row_bytes:]]) != SENTINEL)
            assert bad.size == 0, f"{what}: row {y}: {bad.size} guard bytes changed, first {int(bad[0])}"
        return out


@pytest.fixture(scope="module")
def arenas(gpu_pkg):
    torch = pytest.importorskip("torch")
    free, _ = torch.cuda.mem_get_info()
    need = 2 * ARENA_BYTES + (1 << 30)
    if free < need:
        pytest.skip(f"the device has {free >> 20} MiB free, the two arenas need {need >> 20} MiB")
    a = Arenas(torch)
    yield a
    a.release()
    del a


# ---- frames and what they must become ------------------------------------------------------------------------------------------------------

_WANT = {}


def _frame_and_want(pkg, O, fmt, geo, kw, seed, order=0):
    """(source plane, expected plane) of one frame, both as the format's numpy dtype; the oracle runs once per (geometry, seed).
    order 1 .. 3: the expectation is the oracle's restatement of that summation order (integer and fp32 planes)."""
    key = (fmt, geo, tuple(sorted(kw.items())), seed, order)
    if key not in _WANT:
        sw, sh, tw, th = geo
        oname = TYPES[fmt][0]
        if fmt == "YH":
            src = half_unit_frame(O, fmt, sw, sh, seed)
            want = half_definition(O, fmt, sw, sh, tw, th, kw, src)
        elif fmt == "YBF":
            src = bf16_unit_frame(O, fmt, sw, sh, seed)
            want = bf16_definition(O, fmt, sw, sh, tw, th, kw, src)
        else:
            src = O.lcg_frame(O.FORMATS[oname], sw, sh, seed=seed)
            of = O.OracleFilter(O.FORMATS[oname], sw, sh, tw, th, **oracle_kwargs(kw))
            want = of.get_frame_simd(order, src, threads=4) if order else of.get_frame(src, threads=4)
        _WANT[key] = (np.ascontiguousarray(src[0][:sh, :sw]), np.ascontiguousarray(want[0][:th, :tw]))
    return _WANT[key]


def _same(fmt, got, want):
    """Positions where `got` differs from `want` by the format's definition (NaNs by position)."""
    if fmt == "Y32":
        na, nb = np.isnan(got), np.isnan(want)
        return (na != nb) | (~na & (got.view(np.uint32) != want.view(np.uint32)))
    if fmt == "YH":
        na, nb = np.isnan(got), np.isnan(want)
        return (na != nb) | (~na & (got.view(np.uint16) != want.view(np.uint16)))
    if fmt == "YBF":
        na, nb = bf16_is_nan(got), bf16_is_nan(want)
        return (na != nb) | (~na & (got != want))
    return got != want


def _pitch(width_bytes, extra):
    return (width_bytes + 63) // 64 * 64 + extra


LAYOUTS = ["far_src", "far_dst", "both_far"]


def run_far(pkg, O, arenas, fmt, geo, kw, n, layout, m4=True, mode=0, knobs=None, strips=None, simd_order=None, seed0=7000,
            src_extra=0, dst_extra=0, late=False):
    """One batch of n one-plane frames through process_device in `layout`; every frame compared with the oracle, every guard checked.
    Returns the filter (the caller asserts what ran and closes it)."""
    torch = arenas.torch
    sw, sh, tw, th = geo
    assert max(sw, tw) <= MAX_W and max(sh, th) <= MAX_H, "no frame larger than 384 x 216 on either side"
    dtype = TYPES[fmt][1]
    sb = np.dtype(dtype).itemsize
    spitch, dpitch = _pitch(sw * sb, src_extra), _pitch(tw * sb, dst_extra)
    sfoot = (spitch * sh + 2 * GUARD + 255) // 256 * 256
    dfoot = (dpitch * th + 2 * GUARD + 255) // 256 * 256
    far = far_stride(n, sb, m4 or sb == 4)
    first = GUARD + ((G32 + 8192) if n == 1 else 0)    # a single frame: the PLANE lies beyond 2^32
    if late:   # the batch's FIRST frame beyond 2^31 already (every wave's first frame base is far), the last beyond 2^32
        first = G31 + (64 << 10)
        far = -(-(G31 + MARGIN) // (n - 1) // 4) * 4 + (0 if m4 or sb == 4 else sb)
    sstride = far if layout in ("far_src", "both_far") else sfoot
    # (source and destination strides differ: the destination's far stride is one 256-byte step longer where both are far)
    dstride = (far + (256 if layout == "both_far" and n > 2 and not late else 0)) if layout in ("far_dst", "both_far") else dfoot
    soffs = arenas.place(n, spitch, sh, sw * sb, sstride, first if layout != "far_dst" else GUARD)
    doffs = arenas.place(n, dpitch, th, tw * sb, dstride, first if layout != "far_src" else GUARD)
    if n >= 3:
        for offs, is_far in ((soffs, layout != "far_dst"), (doffs, layout != "far_src")):
            assert not is_far or (offs[n // 2] >= G31 and offs[-1] >= G32), [hex(o) for o in offs]
    wants = []
    for k in range(n):
        src, want = _frame_and_want(pkg, O, fmt, geo, kw, seed0 + k, simd_order or 0)
        wants.append(want)
        arenas.upload(soffs[k], np.ascontiguousarray(src).view(np.uint8).reshape(sh, sw * sb), spitch)
        arenas.arm(doffs[k], th, tw * sb, dpitch)
    with pkg.knobs(**(knobs or {})):    # (around the filter's creation too: the knob trim is read when the device tables are built)
        f = pkg.Filter(pkg.FORMATS[fmt], sw, sh, tw, th, device=0, **kw)
    try:
        f.set_kernel_mode(mode)
        if strips is not None:
            f.set_border_strips(strips)
        if simd_order is not None:
            f.set_simd_order(simd_order)
        stream = torch.cuda.current_stream()
        with pkg.knobs(**(knobs or {})):
            f.process_device([arenas.base(arenas.src) + soffs[0]], [spitch], [sstride], [arenas.base(arenas.dst) + doffs[0]], [dpitch], [dstride], n,
                             stream=stream.cuda_stream)
            stream.synchronize()
        what = f"{fmt} {sw}x{sh}->{tw}x{th} {kw} n={n} {layout} stride%4={'0' if m4 or sb == 4 else 'x'} mode {mode}"
        print(f"far frames: {what}: {f.last_instance(0)} [border {f.last_border(0)}]")
        for k in range(n):
            raw = arenas.download(doffs[k], th, tw * sb, dpitch, f"{what} frame {k} (destination offset {doffs[k]:#x})")
            got = raw.view(dtype).reshape(th, tw)
            bad = np.argwhere(_same(fmt, got, wants[k]))
            assert len(bad) == 0, (f"{what}: frame {k} (source offset {soffs[k]:#x}, destination offset {doffs[k]:#x}) differs from the oracle at "
                                   f"{len(bad)} samples, first (x={bad[0][1]}, y={bad[0][0]}): got {got[tuple(bad[0])]!r}, want {wants[k][tuple(bad[0])]!r}")
    except BaseException:
        f.close()
        raise
    return f


def _expect(f, form, pattern=None, kernel=None, border=None, border_none_of=0, T=None):
    """The call ran what the case was written for; the filter is closed either way."""
    try:
        inst, name, bits = f.last_instance(0), f.last_kernel(0), f.last_border(0)
        if pattern is not None:
            assert re.fullmatch(pattern.replace("{T}", T or ""), inst), f"{form}: ran {inst!r}, expected {pattern.replace('{T}', T or '')}"
        if kernel is not None:
            assert name == kernel, f"{form}: ran {name!r}, expected {kernel}"
        if border is not None:
            assert bits & border == border and bits & border_none_of == 0, f"{form}: border kernels {bits}, expected {border} and none of {border_none_of}"
        print(f"far frames, {form}: {inst} [border {bits}]")
    finally:
        f.close()


def _T(fmt):
    return TYPES[fmt][2]


INT = ["Y8", "Y16"]
ALL = ["Y8", "Y16", "Y32", "YH", "YBF"]
# Geometries: the issue's list (64 x 48 -> 128 x 96, 150 x 70 -> 300 x 140, 192 x 108 -> 384 x 216, 160 x 96 -> 220 x 132) and shapes of the tests that
# already assert the form: DIRECT from test_gpu_parity.py's DIRECT_CASES / WALK_CASES, RUNS_CASES from test_direct_runs.py's RUN_CASES (and
# their chroma-free twins), QUASI from test_gpu_parity.py's QUASI_CASES / test_half_forms.py's G2, SIMD from test_simd_order_calls.py's
# BATCH_CASES, the generic frame-lane kernel's 150 x 100 -> 330 x 190 tap 6 (fs 13) from test_framelane.py's BATCH_CASES.
GEO_A, GEO_B, GEO_C, GEO_D = (64, 48, 128, 96), (150, 70, 300, 140), (192, 108, 384, 216), (160, 96, 220, 132)

# ---- the periodic family ---------------------------------------------------------------------------------------------------------------------
# (form, formats, geometry, arguments, kernel mode, knobs, instance pattern)
PERIODIC = [
    ("periodic_tap3", ALL, GEO_A, dict(tap=3), 2, {}, r"ewa_periodic_kernel<{T}, \d+, \d+>"),
    ("periodic_tap4", ALL, GEO_B, dict(tap=4), 2, {}, r"ewa_periodic_kernel<{T}, \d+, \d+>"),
    ("periodic_pk", INT, GEO_B, dict(tap=3), 6, {}, r"ewa_periodic_pk_kernel<{T}, 7, \d+>"),
    ("periodic_rows_tap3", INT, GEO_B, dict(tap=3), 3, {}, r"ewa_periodic_rows_kernel<{T}, \d+, \d+>"),
    ("periodic_rows_tap2", INT, GEO_A, dict(tap=2), 3, {}, r"ewa_periodic_rows_kernel<{T}, \d+, \d+>"),
    # (ewa_periodic_quad_kernel is the quad form of the reference's full 7 x 7 window: the knob trim = 0 keeps a plan on it)
    ("periodic_quad", ["Y8", "Y16", "Y32"], GEO_B, dict(tap=3), 13, dict(trim=0), r"ewa_periodic_quad_kernel<{T}, .*>"),
    ("periodic_quad8", ALL, GEO_B, dict(tap=4), 13, dict(quad2x8=0), r"ewa_periodic_quad8_kernel<{T}, .*>"),
    ("periodic_quad9", ["Y8", "Y16", "Y32"], GEO_B, dict(tap=4), 15, {}, r"ewa_periodic_quad9_kernel<{T}, \d+>"),
    ("periodic_quad2x8", INT, GEO_C, dict(tap=4), 13, dict(quad2x8=1), r"ewa_periodic_quad2x8_kernel<{T}, .*>"),
    ("periodic_quad2_u16", ["Y16"], GEO_B, dict(tap=3), 13, {}, r"ewa_periodic_quad2_kernel<{T}, \d+, \d+u, 6>"),
    ("periodic_quad2_f32", ["Y32"], GEO_B, dict(tap=3), 13, {}, r"ewa_periodic_quad2_kernel<{T}, \d+, \d+u, 6>"),
] + [(f"rowpair_tap{tap}", ALL if tap == 6 else INT, GEO_B, dict(tap=tap), 0, {}, r"ewa_periodic_rowpair_kernel<{T}, \d+, \d+, \d+>") for tap in (5, 6, 7, 8)]

PERIODIC_RUNS = [(c, fmt, layout) for c in PERIODIC for fmt in c[1] for layout in LAYOUTS]


@pytest.mark.parametrize("case,fmt,layout", PERIODIC_RUNS, ids=[f"{c[0]}-{fmt}-{lay}" for c, fmt, lay in PERIODIC_RUNS])
def test_periodic_family(gpu_pkg, O, arenas, case, fmt, layout):
    """n = 3: frame 1 beyond 2^31, frame 2 beyond 2^32.  The far-source runs take the stride that is no multiple of 4 bytes where the
    sample size allows one (these kernels need no alignment of a frame stride), the others the multiple of 4."""
    form, _, geo, kw, mode, knobs, pattern = case
    f = run_far(gpu_pkg, O, arenas, fmt, geo, kw, 3, layout, m4=(layout != "far_src"), mode=mode, knobs=knobs)
    _expect(f, form, pattern=pattern, T=_T(fmt))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", [3, 4, 5])
def test_quad2_frame_pairs_of_8_bit_planes(gpu_pkg, O, arenas, n, layout):
    """ewa_periodic_quad2_kernel<unsigned char, 8, ...>: two frames per workgroup on the bf16 pair tile.  n = 3: the pair (0, 1) lies on
    both sides of 2^31 and frame 2 has no partner; n = 4: the pair (2, 3) on both sides of 2^32; n = 5: pairs (0, 1), (2, 3) below, the
    single frame 4 beyond 2^32."""
    f = run_far(gpu_pkg, O, arenas, "Y8", GEO_B, dict(tap=3), n, layout, mode=13, knobs=dict(quad_rg=8))
    _expect(f, "periodic_quad2_u8_rg8", pattern=r"ewa_periodic_quad2_kernel<unsigned char, 8, \d+u, 6>")


# ---- direct, runs, quasi, gather ---------------------------------------------------------------------------------------------------------------

DIRECT = [("Y8", (384, 216, 192, 108), {}), ("Y16", (384, 216, 128, 72), {}), ("Y32", (384, 216, 256, 144), {}),
          ("YH", (384, 216, 192, 108), {}), ("YBF", (384, 216, 192, 108), {}),
          ("Y8", (303, 213, 202, 142), dict(tap=4)), ("Y16", (306, 216, 204, 144), dict(tap=5)), ("Y32", (300, 210, 200, 140), {})]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt,geo,kw", DIRECT, ids=[f"{c[0]}_{c[1][0]}x{c[1][1]}to{c[1][2]}x{c[1][3]}" for c in DIRECT])
def test_direct_kernel(gpu_pkg, O, arenas, fmt, geo, kw, layout):
    """Kernel mode 9, frame strides that are multiples of 4 bytes (the kernel's premise): DIRECT_CASES' and WALK_CASES' small shapes."""
    f = run_far(gpu_pkg, O, arenas, fmt, geo, kw, 3, layout, mode=9)
    _expect(f, "direct", kernel="ewa_direct_kernel")


@pytest.mark.parametrize("fmt", ["Y8", "Y16"])
def test_direct_kernel_declines_a_stride_that_is_no_multiple_of_4(gpu_pkg, O, arenas, fmt):
    """... and with the other far stride the plan runs elsewhere, with the same bits."""
    f = run_far(gpu_pkg, O, arenas, fmt, (384, 216, 192, 108), {}, 3, "both_far", m4=False, mode=9)
    assert f.last_kernel(0) != "ewa_direct_kernel", f.last_kernel(0)
    _expect(f, "direct_declined")


RUNS_CASES = [("Y32", (150, 120, 225, 180), dict(tap=4)), ("Y8", (256, 144, 384, 216), dict(tap=8)), ("Y16", (150, 120, 225, 180), dict(tap=5))]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt,geo,kw", RUNS_CASES, ids=[c[0] for c in RUNS_CASES])
def test_runs_form(gpu_pkg, O, arenas, fmt, geo, kw, layout):
    f = run_far(gpu_pkg, O, arenas, fmt, geo, kw, 3, layout, mode=14)
    _expect(f, "runs", kernel="ewa_direct_runs_kernel")


QUASI = [(fmt, geo, kw, mode) for fmt, geo, kw in (("Y8", (256, 144, 384, 216), {}), ("Y16", (150, 120, 225, 180), dict(tap=4)), ("Y32", (150, 120, 225, 180), dict(tap=4)))
         for mode in (7, 8, 10)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt,geo,kw,mode", QUASI, ids=[f"{c[0]}_mode{c[3]}" for c in QUASI])
def test_quasi_kernel(gpu_pkg, O, arenas, fmt, geo, kw, mode, layout):
    """The exact form, the waterfall and the per-lane coefficient form (kernel modes 7 / 8 / 10) on the affine-origin shapes."""
    f = run_far(gpu_pkg, O, arenas, fmt, geo, kw, 3, layout, m4=(layout != "far_src"), mode=mode)
    _expect(f, f"quasi_mode{mode}", kernel="ewa_quasi_kernel")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("fmt", ALL)
def test_gather_kernel(gpu_pkg, O, arenas, fmt, n, layout):
    """n = 1: ONE frame whose plane lies beyond 2^32 (kernel_gather.hip derives frame = slot % nf); n = 3 with the odd stride."""
    f = run_far(gpu_pkg, O, arenas, fmt, GEO_D, {}, n, layout, m4=False, mode=1)
    _expect(f, "gather", kernel="ewa_gather_kernel")


# ---- the frame-lane family ---------------------------------------------------------------------------------------------------------------------

FL = [("sub", fmt, GEO_D, {}, n, 16, "ewa_framelane_sub_kernel") for fmt in ALL for n in (3, 16, 33)] + \
     [("win", fmt, GEO_D, {}, 64, 0, "ewa_framelane_win_kernel") for fmt in ALL] + \
     [("pair", fmt, GEO_D, {}, 128, 0, "ewa_framelane_pair_kernel") for fmt in INT] + \
     [("pair_and_one", fmt, GEO_D, {}, 129, 0, "ewa_gather_kernel") for fmt in INT] + \
     [("generic", fmt, (150, 100, 330, 190), dict(tap=6), 24, 11, "ewa_framelane_kernel") for fmt in INT]
# "late": the batch begins beyond 2^31, so EVERY wave's first frame base is far (with the batch at the base a wave's first frame lies
# below 2^31 for all of these but 33 sub-group frames, and a truncated first base passes: profiles/far_frames/README.md)
FL_RUNS = [(c, layout, late) for c in FL for layout in LAYOUTS for late in (False, True) if not late or layout != "far_dst" or c[4] >= 24]


@pytest.mark.parametrize("case,layout,late", FL_RUNS, ids=[f"{c[0]}-{c[1]}-n{c[4]}-{lay}{'-late' if late else ''}" for c, lay, late in FL_RUNS])
def test_framelane_family(gpu_pkg, O, arenas, case, layout, late):
    """Lanes are frames: fl_stage forms a frame's rows from 32-bit offsets behind a 64-bit frame base.  n = 16 / 33 / 64 / 128 / 129 put
    the later lanes beyond 2^31 and 2^32 inside one wave.  The far-destination runs take the odd stride (sample-by-sample stores).
    129 frames are 128 on the frame-pair form and the last one, the frame beyond 2^32, as a call of its own, which these plans
    give to the gather kernel (tests/test_framelane.py): last_kernel names that last part."""
    form, fmt, geo, kw, n, mode, kernel = case
    f = run_far(gpu_pkg, O, arenas, fmt, geo, kw, n, layout, m4=(layout != "far_dst"), mode=mode, late=late)
    _expect(f, f"framelane_{form}", pattern=kernel)


# ---- the SIMD-order kernel ---------------------------------------------------------------------------------------------------------------------

SIMD = [("Y8", (97, 61, 291, 183), {}), ("Y16", (150, 100, 300, 200), dict(tap=6)), ("Y32", (64, 48, 40, 30), {})]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("order", [1, 2, 3, 0])
@pytest.mark.parametrize("fmt,geo,kw", SIMD, ids=[c[0] for c in SIMD])
def test_simd_order_kernel(gpu_pkg, O, arenas, fmt, geo, kw, order, layout):
    """Orders 1 .. 3 (SSE4.1 / AVX2 / AVX-512 summation) against the oracle's restatement of that order, on shapes of
    test_simd_order_calls.py; order 0 on the same shapes is the automatic choice against the opt = 0 oracle."""
    f = run_far(gpu_pkg, O, arenas, fmt, geo, kw, 3, layout, m4=(layout != "far_src"), simd_order=order)
    if order:
        _expect(f, "simd_order", kernel="ewa_simd_order_kernel")
    else:
        assert f.last_kernel(0) != "ewa_simd_order_kernel"
        _expect(f, "simd_order_0")


# ---- border forms ------------------------------------------------------------------------------------------------------------------------------
# (form, formats, geometry, arguments, n, kernel mode, border strips, knobs, last_border bits, none of)
BORDERS = [
    ("strip_rows_and_columns", ALL, GEO_C, dict(tap=3), 3, 0, 3, {}, 48, 0),
    ("strip_rows_and_columns_tap4", INT, GEO_B, dict(tap=4), 3, 0, 3, {}, 48, 0),
    ("colstrip", ["Y8", "Y16", "Y32"], GEO_C, dict(tap=3), 3, 0, 1, {}, 4, 256 | 64 | 32 | 8),
    ("colpair", ["Y8", "Y16", "Y32"], GEO_B, dict(tap=6), 3, 0, 4, dict(colpair=1), 256, 64 | 32 | 8 | 4 | 1),
    ("rowpair_rows", ["Y8", "Y16", "Y32"], GEO_B, dict(tap=6), 3, 0, 4, {}, 128, 16 | 2),
    ("edge_columns_quad2", INT, GEO_C, dict(tap=3), 3, 13, 4, {}, 64, 0),
    ("edge_columns_quad2x8", INT, GEO_C, dict(tap=4), 3, 13, 4, dict(quad2x8=1), 64, 0),
]
BORDER_RUNS = [(c, fmt, layout) for c in BORDERS for fmt in c[1] for layout in LAYOUTS]


@pytest.mark.parametrize("case,fmt,layout", BORDER_RUNS, ids=[f"{c[0]}-{fmt}-{lay}" for c, fmt, lay in BORDER_RUNS])
def test_border_forms(gpu_pkg, O, arenas, case, fmt, layout):
    """Strides that are multiples of 4 bytes: the strip border shares the direct kernel's premise."""
    form, _, geo, kw, n, mode, strips, knobs, bits, none_of = case
    f = run_far(gpu_pkg, O, arenas, fmt, geo, kw, n, layout, mode=mode, strips=strips, knobs=knobs)
    _expect(f, f"border_{form}", border=bits, border_none_of=none_of)


# ---- flagged frames: the finite scans -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scan", [0, 1], ids=["rim_scan", "float_scan"])
@pytest.mark.parametrize("where", ["last", "past_2_31"])
@pytest.mark.parametrize("tap", [3, 4])
@pytest.mark.parametrize("fmt", ["Y32", "YH"])
def test_flags_name_the_far_frame(gpu_pkg, O, arenas, fmt, tap, where, scan):
    """Float planes on the trimmed support, 5 frames with far source and destination strides; one +inf (tap 3) or NaN (tap 4) in the
    last frame only, or in the first frame past 2^31 only.  finite_scan_outside_kernel (the rim; the spot lies in the plane's first
    row) or, under the knob float_scan, finite_scan_kernel must flag exactly that frame: (a) trimmed instance, (b) flags, (c) bits."""
    torch = arenas.torch
    n, geo = 5, GEO_B
    sw, sh, tw, th = geo
    dtype = TYPES[fmt][1]
    sb = np.dtype(dtype).itemsize
    kw = dict(tap=tap)
    stride = far_stride(n, sb, True)
    spitch, dpitch = _pitch(sw * sb, 0), _pitch(tw * sb, 0)
    soffs = arenas.place(n, spitch, sh, sw * sb, stride, GUARD)
    doffs = arenas.place(n, dpitch, th, tw * sb, stride + 256, GUARD)
    hit = n - 1 if where == "last" else min(k for k in range(n) if soffs[k] >= G31)
    assert where == "last" or (soffs[hit] >= G31 and soffs[hit - 1] < G31 and hit != n - 1)
    oname = "Y32"
    of = O.OracleFilter(O.FORMATS[oname], sw, sh, tw, th, **oracle_kwargs(kw))
    wants = []
    for k in range(n):
        src = O.lcg_frame(O.FORMATS[oname], sw, sh, seed=7300 + k)[0][:sh, :sw].astype(dtype)
        if k == hit:
            src[0, sw // 2] = np.inf if tap == 3 else np.nan
        with np.errstate(over="ignore", invalid="ignore"):
            want = of.get_frame([np.ascontiguousarray(src.astype(np.float32))], threads=4)[0][:th, :tw].astype(dtype)
        wants.append(want)
        arenas.upload(soffs[k], np.ascontiguousarray(src).view(np.uint8).reshape(sh, sw * sb), spitch)
        arenas.arm(doffs[k], th, tw * sb, dpitch)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[fmt], sw, sh, tw, th, device=0, **kw)
    try:
        stream = torch.cuda.current_stream()
        with gpu_pkg.knobs(float_trim_min_taps=0, float_scan=scan):
            f.process_device([arenas.base(arenas.src) + soffs[0]], [spitch], [stride], [arenas.base(arenas.dst) + doffs[0]], [dpitch], [stride + 256], n,
                             stream=stream.cuda_stream)
            stream.synchronize()
        what = f"{fmt} tap {tap} {where} scan {scan}"
        T = TYPES[fmt][2]
        pat = rf"ewa_periodic_kernel<{T}, 6, \d+>|ewa_periodic_quad2_kernel<{T}, \d+, \d+u, 6>" if tap == 3 else rf"ewa_periodic_quad8_kernel<{T}, \d+, \d+u>"
        assert re.fullmatch(pat, f.last_instance(0)), f"{what}: ran {f.last_instance(0)!r}"
        assert 0 < f.periodic_support(0) < f.plan_info(0).filter_size
        flags = f.last_finite_flags(0)
        assert flags is not None, f"{what}: the call did not take the flagged path"
        assert flags.tolist() == [int(k == hit) for k in range(n)], f"{what}: flags {flags.tolist()}, the non-finite sample is in frame {hit}"
        for k in range(n):
            got = arenas.download(doffs[k], th, tw * sb, dpitch, f"{what} frame {k}").view(dtype).reshape(th, tw)
            bad = np.argwhere(_same(fmt, got, wants[k]))
            assert len(bad) == 0, f"{what}: frame {k} differs from the oracle at {len(bad)} samples, first {bad[0].tolist()}"
        assert np.isnan(wants[hit]).any()
    finally:
        f.close()


# ---- destination planes that span GiB themselves ---------------------------------------------------------------------------------------------------

SPAN_ROWS = 96
SPAN_PITCH = ((G32 - (1 << 20)) // SPAN_ROWS) // 64 * 64 + 4     # 96 rows end just below 2^32; a multiple of 64 plus one float


@pytest.mark.parametrize("form,fmt,geo,kw,n,mode", [
    ("periodic", "Y8", GEO_A, dict(tap=3), 1, 2), ("periodic", "Y32", GEO_A, dict(tap=3), 1, 2),
    ("gather", "Y16", (64, 48, 160, 120), {}, 1, 1),
    ("framelane_sub", "Y8", (64, 48, 160, 120), {}, 3, 16),
], ids=["periodic_u8", "periodic_f32", "gather_u16", "framelane_sub_u8"])
def test_destination_plane_just_below_4_gib(gpu_pkg, O, arenas, form, fmt, geo, kw, n, mode):
    """pitch * height just below 2^32 and the rows of the lower half beyond 2^31: the store offsets use all 32 bits and must not be
    taken for signed.  The frames of a batch lie inside the pitch gap, 1 MiB apart."""
    torch = arenas.torch
    sw, sh, tw, th = geo
    dtype = TYPES[fmt][1]
    sb = np.dtype(dtype).itemsize
    pitch = SPAN_PITCH if th == SPAN_ROWS else ((G32 - (1 << 20)) // th) // 64 * 64 + 4
    assert pitch * th < G32 and pitch * (th - 2) >= G31 and pitch * (th // 2 + 1) >= G31 and pitch % sb == 0 and pitch % 64 == 4
    spitch = _pitch(sw * sb, 0)
    sstride = (spitch * sh + 2 * GUARD + 255) // 256 * 256
    dstride = 1 << 20
    soffs = arenas.place(n, spitch, sh, sw * sb, sstride, GUARD)
    doffs = arenas.place(n, pitch, th, tw * sb, dstride, GUARD)
    wants = []
    for k in range(n):
        src, want = _frame_and_want(gpu_pkg, O, fmt, geo, kw, 7500 + k)
        wants.append(want)
        arenas.upload(soffs[k], np.ascontiguousarray(src).view(np.uint8).reshape(sh, sw * sb), spitch)
    for k in range(n):
        arenas.arm(doffs[k], th, tw * sb, pitch)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[fmt], sw, sh, tw, th, device=0, **kw)
    try:
        f.set_kernel_mode(mode)
        stream = torch.cuda.current_stream()
        f.process_device([arenas.base(arenas.src) + soffs[0]], [spitch], [sstride], [arenas.base(arenas.dst) + doffs[0]], [pitch], [dstride], n,
                         stream=stream.cuda_stream)
        stream.synchronize()
        name = {"periodic": "ewa_periodic_kernel", "gather": "ewa_gather_kernel", "framelane_sub": "ewa_framelane_sub_kernel"}[form]
        assert f.last_kernel(0) == name, f.last_kernel(0)
        for k in range(n):
            got = arenas.download(doffs[k], th, tw * sb, pitch, f"spanning destination {form} frame {k}").view(dtype).reshape(th, tw)
            bad = np.argwhere(_same(fmt, got, wants[k]))
            assert len(bad) == 0, f"spanning destination {form}: frame {k} differs at {len(bad)} samples, first (y, x) {bad[0].tolist()}"
    finally:
        f.close()


def test_planes_of_4_gib_are_refused_before_anything_is_queued(gpu_pkg, arenas):
    """A destination plane of 2^32 bytes or more, and a source plane of 2^32 bytes or more: refused with their messages, and the
    sentinel in front of the destination is untouched (nothing ran)."""
    sw, sh, tw, th = GEO_A
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["Y8"], sw, sh, tw, th, device=0)
    try:
        a0 = arenas.base_offset()
        arenas.dst[a0:a0 + 4096].fill_(SENTINEL)
        big_d = -(-G32 // th)
        with pytest.raises(gpu_pkg.JincError, match=r"destination plane larger than 4 GiB is not supported \(32-bit store offsets\)"):
            f.process_device([arenas.base(arenas.src)], [64], [0], [arenas.base(arenas.dst)], [big_d], [0], 1)
        big_s = -(-G32 // (sh - 1))
        with pytest.raises(gpu_pkg.JincError, match=r"source plane larger than 4 GiB is not supported \(32-bit fetch offsets\)"):
            f.process_device([arenas.base(arenas.src)], [big_s], [0], [arenas.base(arenas.dst)], [128], [0], 1)
        arenas.torch.cuda.synchronize()
        host = arenas.torch.empty(4096, dtype=arenas.torch.uint8, pin_memory=True)
        host.copy_(arenas.dst[a0:a0 + 4096])
        assert (host.numpy() == SENTINEL).all()
    finally:
        f.close()


# ---- planes of one frame as frames of one plane (plane_pair) ----------------------------------------------------------------------------------

PAIRS = [("YUV420P8", (128, 96, 256, 192), dict(cplace="mpeg1")), ("YUV444PS", (96, 64, 192, 128), {})]   # (test_gpu_parity.py's CASES)


@pytest.mark.parametrize("apart", ["past_2_31", "past_2_32", "v_before_u"])
@pytest.mark.parametrize("name,geo,kw", PAIRS, ids=[c[0] for c in PAIRS])
def test_chroma_planes_far_apart(gpu_pkg, O, arenas, name, geo, kw, apart):
    """ONE frame whose U and V planes, of equal pitch, lie more than 2^31 / more than 2^32 bytes apart on both sides (dispatch.cpp's
    plane_pair may launch them as frames 0 and 1 of one plane, the distance as the frame stride), and once V in front of U, which
    the pairing rule declines: the chroma planes are the oracle's whichever path the call takes."""
    torch = arenas.torch
    sw, sh, tw, th = geo
    fmt, ofmt = gpu_pkg.FORMATS[name], O.FORMATS[name]
    sb = np.dtype(fmt.dtype).itemsize
    gap = {"past_2_31": G31 + (64 << 10), "past_2_32": G32 + (64 << 10), "v_before_u": G32 + (64 << 10)}[apart]
    near = [GUARD, GUARD + (1 << 20), GUARD + (1 << 20) + gap]
    if apart == "v_before_u":
        near = [GUARD, GUARD + (1 << 20) + gap, GUARD + (1 << 20)]
    src = O.lcg_frame(ofmt, sw, sh, seed=7700)
    want = O.OracleFilter(ofmt, sw, sh, tw, th, **oracle_kwargs(kw)).get_frame(src, threads=4)
    sdims, ddims = fmt.plane_dims(sw, sh), fmt.plane_dims(tw, th)
    sp = [_pitch(w * sb, 0) for w, h in sdims]
    dp = [_pitch(w * sb, 0) for w, h in ddims]
    soffs = [arenas.place(1, sp[i], sdims[i][1], sdims[i][0] * sb, 0, near[i])[0] for i in range(3)]
    doffs = [arenas.place(1, dp[i], ddims[i][1], ddims[i][0] * sb, 0, near[i] + (256 if i == 2 else 0))[0] for i in range(3)]
    for i, (w, h) in enumerate(sdims):
        arenas.upload(soffs[i], np.ascontiguousarray(src[i][:h, :w]).view(np.uint8).reshape(h, w * sb), sp[i])
    for i, (w, h) in enumerate(ddims):
        arenas.arm(doffs[i], h, w * sb, dp[i])
    f = gpu_pkg.Filter(fmt, sw, sh, tw, th, device=0, **kw)
    try:
        stream = torch.cuda.current_stream()
        f.process_device([arenas.base(arenas.src) + o for o in soffs], sp, [0, 0, 0], [arenas.base(arenas.dst) + o for o in doffs], dp, [0, 0, 0], 1,
                         stream=stream.cuda_stream)
        stream.synchronize()
        print(f"far frames, plane pair {name} {apart}: {[f.last_instance(t) for t in range(f.num_tables)]}")
        key = "Y32" if sb == 4 else "Y8"
        for i, (w, h) in enumerate(ddims):
            got = arenas.download(doffs[i], h, w * sb, dp[i], f"{name} {apart} plane {i}").view(fmt.dtype).reshape(h, w)
            bad = np.argwhere(_same(key, got, np.ascontiguousarray(want[i][:h, :w])))
            assert len(bad) == 0, f"{name} {apart}: plane {i} (destination offset {doffs[i]:#x}) differs from the oracle at {len(bad)} samples, first {bad[0].tolist()}"
    finally:
        f.close()


# ---- the pass kernels: stand-in calls with a far packed side ---------------------------------------------------------------------------------------
# The sides are built by the stand-in tests' own helpers (dense, frames `fs` bytes apart), then one side is MOVED into an arena with
# far frame strides: its bytes frame by frame, its pointers, its strides and its download are replaced, everything else (the host
# image, the guard comparison of every byte outside the samples, the de-interleaving) is the helper's.

def _side_buffers(side):
    """The device buffers of a side as (get, set) accessors over lead / fs / host / dev: tests/test_strided.py's Side keeps a dict per
    buffer, the word and block sides of test_packed10.py / test_v210.py are one buffer themselves."""
    if hasattr(side, "bufs"):
        return [(B.__getitem__, B.__setitem__, b) for b, B in side.bufs.items()]
    return [(lambda k: getattr(side, k), lambda k, v: setattr(side, k, v), None)]


def move_far(arenas, side, which, n):
    from conftest import to_host
    arena = arenas.src if which == "src" else arenas.dst
    bo = arenas.base_offset()
    moved = {}
    for j, (get, _, b) in enumerate(_side_buffers(side)):
        lead, fs, dev = get("lead"), get("fs"), get("dev")
        far = far_stride(n, 1, True) // 16 * 16 + 16 + fs % 16         # (the alignment class of the helper's own frame stride)
        origin = GUARD + j * (192 << 10)
        assert j < 4 and lead + fs + 256 + 2 * GUARD <= (192 << 10) and far >= fs + 256 + 2 * GUARD and dev.numel() == lead + n * fs + 256
        offs = [origin + lead + k * far for k in range(n)]
        lo, hi = -bo, ARENA_BYTES - bo
        # the module's invariant for this buffer: every frame inside, and behind any truncated offset a whole frame with its guards
        assert lo <= -G31 - GUARD - lead and G32 + fs + 256 + GUARD <= hi and offs[-1] + fs + 256 + GUARD <= hi and offs[n // 2] >= G31 and offs[-1] >= G32
        arena[bo + origin - GUARD:bo + origin].fill_(SENTINEL)
        arena[bo + origin:bo + origin + lead].copy_(dev[:lead])
        for k in range(n):
            end = fs + (256 if k == n - 1 else 0)
            arena[bo + offs[k]:bo + offs[k] + end].copy_(dev[lead + k * fs:lead + k * fs + end])
            arena[bo + offs[k] + end:bo + offs[k] + end + GUARD].fill_(SENTINEL)
        moved[b] = dict(lead=lead, fs=fs, dev=dev, far=far, origin=origin, offs=offs, delta=arena.data_ptr() + bo + origin - dev.data_ptr())

    def gather(b):
        m = moved[b]
        back = m["dev"].clone()
        back[:m["lead"]].copy_(arena[bo + m["origin"]:bo + m["origin"] + m["lead"]])
        guards = [arena[bo + m["origin"] - GUARD:bo + m["origin"]]]
        for k in range(n):
            end = m["fs"] + (256 if k == n - 1 else 0)
            back[m["lead"] + k * m["fs"]:m["lead"] + k * m["fs"] + end].copy_(arena[bo + m["offs"][k]:bo + m["offs"][k] + end])
            guards.append(arena[bo + m["offs"][k] + end:bo + m["offs"][k] + end + GUARD])
        for g, t in enumerate(guards):
            bad = np.flatnonzero(to_host(t).numpy() != SENTINEL)
            assert bad.size == 0, f"far {which} side: guard window {g} of buffer {b}: {bad.size} bytes changed, first {int(bad[0])}"
        return to_host(back).numpy()

    ptrs, strides = side.ptrs(), side.strides()
    if hasattr(side, "bufs"):
        side.ptrs = lambda: [p + moved[b]["delta"] for p, (b, chan, step) in zip(ptrs, side.layout)]
        side.strides = lambda: [moved[b]["far"] for (b, chan, step) in side.layout]
        side.download = lambda: {b: gather(b) for b in moved}
    else:
        side.ptrs = lambda: [ptrs[0] + moved[None]["delta"]] + list(ptrs[1:])
        side.strides = lambda: [moved[None]["far"]] + list(strides[1:])
        side.download = lambda: gather(None)
    return side


STAND_IN_GEO = (102, 38, 204, 76)     # (test_simd_order_calls.py's STAND_INS / FLOAT_GEOM: odd chroma width, vectors and a tail in the passes)
SPLIT, MERGE, WIDENED, NARROWED, UNPACK_FIELDS, PACK_FIELDS, UNPACK_V210, PACK_V210 = 2, 3, 0, 1, 4, 5, 7, 8   # jinc_debug_last_groups: direction
STAND_INS = ["nv12_strided", "p010_shifted", "y410_packed10", "v210", "nv12_widened", "p010_widened", "rgb24_widened", "nv12_widened_scaled",
             "narrowed_nv12", "narrowed_rgba64", "narrowed_nv12_scaled"]
FAR_SIDES = [(name, side) for name in STAND_INS for side in ("src", "dst") if not (side == "dst" and "widened" in name) and not (side == "src" and "narrowed" in name)]


def _int_frames(O, name, geo, n, seed):
    return [O.lcg_frame(O.FORMATS[name], geo[0], geo[1], seed=seed + 7 * k) for k in range(n)]


def _cmp(key, got, want, dims, what):
    for k in range(len(want)):
        for i, (w, h) in enumerate(dims):
            a, b = np.ascontiguousarray(got[k][i][:h, :w]), np.ascontiguousarray(want[k][i][:h, :w])
            bad = np.argwhere(_same(key, a, b))
            assert len(bad) == 0, f"{what}: frame {k} plane {i} differs at {len(bad)} samples, first (y, x) {bad[0].tolist()}: got {a[tuple(bad[0])]!r}, want {b[tuple(bad[0])]!r}"


@pytest.mark.parametrize("name,far_side", FAR_SIDES, ids=[f"{n}-far_{s}" for n, s in FAR_SIDES])
def test_stand_in_calls_with_a_far_packed_side(gpu_pkg, O, arenas, name, far_side):
    """n = 3 frames whose packed (or, for the float side of a widened / narrowed call, planar) side lies in an arena with frame 1
    beyond 2^31 and frame 2 beyond 2^32; the library's scratch is where it is.  Each call against the oracle AND against the planar
    call on dense planes; last_strided and the direction of last_groups say that the pass meant is the pass that ran."""
    import test_narrowed
    import test_packed10
    import test_shifted
    import test_v210
    import test_widened
    from test_narrowed_host import definition as narrowed_definition
    from test_strided import Side, packed, planar, run_planar, semi_planar
    torch = arenas.torch
    pkg, n, s = gpu_pkg, 3, arenas.torch.cuda.current_stream()
    what = f"{name} far {far_side}"
    geo = STAND_IN_GEO
    far = lambda src, dst: move_far(arenas, src if far_side == "src" else dst, far_side, n)
    key, planar_of = "Y8", None
    if name == "nv12_strided":
        f = pkg.Filter(pkg.FORMATS["YUV420P8"], *geo, device=0, tap=3)
        frames = _int_frames(O, "YUV420P8", geo, n, 300)
        src = Side(torch, f.fmt.plane_dims(f.src_w, f.src_h), f.fmt.dtype, semi_planar(), n, 16, seed=11).fill(frames).upload()
        dst = Side(torch, f.out_dims(), f.fmt.dtype, semi_planar(), n, 16, seed=12).upload()
        far(src, dst)
        f.process_device_strided(src.ptrs(), src.pitches(), src.steps(), src.strides(), dst.ptrs(), dst.pitches(), dst.steps(), dst.strides(), n, stream=s.cuda_stream)
        s.synchronize()
        got, model, oname, direction = dst.frames_and_guards(what), frames, "YUV420P8", SPLIT if far_side == "src" else MERGE
    elif name == "p010_shifted":
        f = pkg.Filter(pkg.FORMATS["YUV420P10"], *geo, device=0, tap=3)
        frames = _int_frames(O, "YUV420P10", geo, n, 310)
        src, dst = test_shifted.make_sides(torch, f, frames, semi_planar(), semi_planar(), [6] * 3, n)
        far(src, dst)
        test_shifted.call(f, src, dst, [6] * 3, [6] * 3, n, s)
        s.synchronize()
        got, model, oname, direction = test_shifted.values_of(dst.frames_and_guards(what), [6] * 3, what), frames, "YUV420P10", SPLIT if far_side == "src" else MERGE
    elif name == "y410_packed10":
        geo = (70, 21, 140, 42)
        f = pkg.Filter(pkg.FORMATS["YUV444P10"], *geo, device=0, tap=3)
        frames = _int_frames(O, "YUV444P10", geo, n, 320)
        src, dst = test_packed10.make_sides(torch, f, frames, test_packed10.Y410, test_packed10.Y410, n)
        far(src, dst)
        test_packed10.call(f, src, dst, test_packed10.Y410, test_packed10.Y410, test_packed10.OPAQUE, n, s)
        s.synchronize()
        got, model, oname = test_packed10.results(dst, test_packed10.Y410, test_packed10.OPAQUE, what), frames, "YUV444P10"
        direction = UNPACK_FIELDS if far_side == "src" else PACK_FIELDS
    elif name == "v210":
        geo = (48, 20, 100, 40)
        f = pkg.Filter(pkg.FORMATS["YUV422P10"], *geo, device=0, tap=3)
        frames = _int_frames(O, "YUV422P10", geo, n, 330)
        src, dst = test_v210.make_sides(torch, f, frames, True, True, n)
        far(src, dst)
        test_v210.call(f, src, dst, True, True, n, s)
        s.synchronize()
        got, model, oname, direction = dst.frames_and_guards(what), frames, "YUV422P10", UNPACK_V210 if far_side == "src" else PACK_V210
    elif "widened" in name:
        fname, layout, bits, shifts = {"nv12": ("YUV420PS", semi_planar(), 8, None), "p010": ("YUV420PS", semi_planar(), 10, [6] * 3),
                                       "rgb24": ("RGBPS", packed("RGB", 3, 3), 8, None)}[name.split("_")[0]]
        f = pkg.Filter(pkg.FORMATS[fname], *geo, device=0, tap=3)
        vals = test_widened.values(pkg, fname, geo[0], geo[1], bits, n, seed=9)
        src, dst = test_widened.make_sides(torch, f, test_widened.raw_of(vals, bits, shifts or [0] * 3), layout, planar(3), n)
        far(src, dst)
        if name.endswith("scaled"):
            scale, offs = float(np.float32(1.0 / 255.0)), [float(np.float32(-16.0 / 255.0)), float(np.float32(-128.0 / 255.0)), float(np.float32(-128.0 / 255.0))]
            f.process_device_widened_scaled(src.ptrs(), src.pitches(), src.steps(), None, 8, [scale] * 3, offs, src.strides(),
                                            dst.ptrs(), dst.pitches(), dst.steps(), dst.strides(), n, stream=s.cuda_stream)
            model = [[p.astype(np.float32) * np.float32(scale) + np.float32(o) for p, o in zip(planes, offs)] for planes in vals]
        else:
            test_widened.call(f, src, dst, shifts, bits, n, s)
            model = [[p.astype(np.float32) for p in planes] for planes in vals]
        s.synchronize()
        got, oname, direction, key = dst.frames_and_guards(what), fname, WIDENED, "Y32"
        test_widened.assert_source_unchanged(src, what)
    else:
        fname, layout, bits = {"narrowed_nv12": ("YUV420PS", semi_planar(), 8), "narrowed_nv12_scaled": ("YUV420PS", semi_planar(), 8),
                               "narrowed_rgba64": ("RGBAPS", packed("RGBA", 4, 4), 16)}[name]
        peak = (1 << bits) - 1
        f = pkg.Filter(pkg.FORMATS[fname], *geo, device=0, tap=3)
        scaled = name.endswith("scaled")
        model = test_narrowed.sources(f.fmt, geo[0], geo[1], n, 1 if scaled else peak, seed=15)
        src, dst = test_narrowed.make_sides(torch, f, model, planar(f.fmt.planes), layout, bits, n)
        far(src, dst)
        if scaled:
            f.process_device_narrowed_scaled(src.ptrs(), src.pitches(), src.steps(), src.strides(), dst.ptrs(), dst.pitches(), dst.steps(), None, bits,
                                             [float(peak)] * 4, [0.0] * 4, dst.strides(), n, stream=s.cuda_stream)
        else:
            test_narrowed.narrowed_call(f, src, dst, None, bits, n, s)
        s.synchronize()
        got, oname, direction = dst.frames_and_guards(what), fname, NARROWED
        udt = np.uint8 if bits == 8 else np.uint16
        planar_of = lambda planes: [narrowed_definition(p * np.float32(peak) if scaled else p, peak).astype(udt) for p in planes]
    try:
        report, groups = f.last_strided(), f.last_groups()
        print(f"far frames, {what}: last_strided {report}, directions {[g['direction'] for g in groups]}")
        assert (report[0] if far_side == "src" else report[1]) > 0, report
        assert direction in [g["direction"] for g in groups], (direction, groups)
        of = O.OracleFilter(O.FORMATS[oname], *geo, tap=3)
        wants = [of.get_frame(m, threads=4) for m in model]
        dense = run_planar(torch, f, model, n)
        if planar_of is not None:
            wants, dense = [planar_of(w) for w in wants], [planar_of(d) for d in dense]
        if f.fmt.bits == 10:
            wants = [[p & np.uint16(1023) for p in planes] for planes in wants]
        dims = f.out_dims()
        _cmp(key, got, wants, dims, what + " against the oracle")
        _cmp(key, got, dense, dims, what + " against the planar call")
    finally:
        f.close()


# ---- stand-in calls that combine two passes, or take words / blocks on one side and planes on the other ------------------------------------------------

WIDEN_FIELDS, WIDEN_V210, NARROW_FIELDS, NARROW_V210 = 6, 9, 10, 11   # jinc_debug_last_groups: direction
COMBINED = [("widened_packed10", "src"), ("widened_packed10_scaled", "src"), ("widened_v210", "src"), ("widened_v210_scaled", "src"),
            ("narrowed_packed10", "dst"), ("narrowed_v210", "dst"), ("shifted_packed10", "src"), ("shifted_packed10", "dst"),
            ("v210_packed10", "src"), ("v210_packed10", "dst")]
WORDS_GEO, BLOCKS_GEO = (70, 21, 140, 42), (48, 20, 100, 40)   # (test_simd_order_calls.py's STAND_INS: whole and partial v210 blocks)


@pytest.mark.parametrize("name,far_side", COMBINED, ids=[f"{n}-far_{s}" for n, s in COMBINED])
def test_combined_stand_in_calls_with_a_far_side(gpu_pkg, O, arenas, name, far_side):
    """Y410 words / v210 blocks into float filters (one widening field / block pass), float results into words / blocks (one narrowing
    pass), and P010 planes / v210 blocks into Y410 words on a filter whose output is 4:4:4 (a split or block pass in, a field pass
    out): 3 frames, the word / block / semi-planar side at far strides, against the oracle and against the planar call."""
    import test_chroma_out
    import test_narrowed_words
    import test_widened
    import test_widened_words
    from test_narrowed import sources
    from test_narrowed_host import definition as narrowed_definition
    from test_packed10 import OPAQUE, Y410, PackedSide
    from test_strided import Side, planar, run_planar, semi_planar
    from test_v210 import V210Side
    torch = arenas.torch
    pkg, n, s = gpu_pkg, 3, arenas.torch.cuda.current_stream()
    what = f"{name} far {far_side}"
    key, post = "Y8", None
    if name.startswith("widened"):
        kind = "packed10" if "packed10" in name else "v210"
        fname, geo = ("YUV444PS", WORDS_GEO) if kind == "packed10" else ("YUV422PS", BLOCKS_GEO)
        f = pkg.Filter(pkg.FORMATS[fname], *geo, device=0, tap=3)
        vals = test_widened.values(pkg, fname, geo[0], geo[1], 10, n, seed=7)
        src = test_widened_words.make_source(torch, f, kind, vals, n, Y410)
        dst = Side(torch, f.out_dims(), f.fmt.dtype, planar(3), n, seed=12).upload()
        move_far(arenas, src, "src", n)
        if name.endswith("scaled"):
            scales = [float(np.float32(1.0 / 1023.0))] * 3
            adds = [float(np.float32(-64.0 / 1023.0)), float(np.float32(-512.0 / 1023.0)), float(np.float32(-512.0 / 1023.0))]
            if kind == "packed10":
                f.process_device_widened_packed10_scaled(src.ptrs()[0], src.pitches()[0], Y410, scales, adds, src.strides()[0], dst.ptrs(), dst.pitches(),
                                                         dst.steps(), dst.strides(), n, stream=s.cuda_stream)
            else:
                f.process_device_widened_v210_scaled(src.ptrs()[0], src.pitches()[0], scales, adds, src.strides()[0], dst.ptrs(), dst.pitches(),
                                                     dst.steps(), dst.strides(), n, stream=s.cuda_stream)
            model = [[p.astype(np.float32) * np.float32(sc) + np.float32(a) for p, sc, a in zip(planes, scales, adds)] for planes in vals]
        else:
            test_widened_words.call(f, kind, src, dst, n, s, Y410)
            model = [[p.astype(np.float32) for p in planes] for planes in vals]
        s.synchronize()
        got, key, direction = dst.frames_and_guards(what), "Y32", WIDEN_FIELDS if kind == "packed10" else WIDEN_V210
        assert np.array_equal(src.download(), src.host), f"{what}: the source was written"
        wants = [O.OracleFilter(O.FORMATS[fname], *geo, tap=3).get_frame(m, threads=4) for m in model]
    elif name.startswith("narrowed"):
        kind = "packed10" if "packed10" in name else "v210"
        fname, geo = ("YUV444PS", WORDS_GEO) if kind == "packed10" else ("YUV422PS", BLOCKS_GEO)
        f = pkg.Filter(pkg.FORMATS[fname], *geo, device=0, tap=3)
        model = sources(f.fmt, geo[0], geo[1], n, 1023, 5)
        src = test_narrowed_words.make_src(torch, f, model, n)
        dst = test_narrowed_words.make_dst(torch, f, kind, n, Y410)
        move_far(arenas, dst, "dst", n)
        test_narrowed_words.call(f, kind, src, dst, n, s, Y410, test_narrowed_words.FILL)
        s.synchronize()
        got, direction = test_narrowed_words.results(dst, kind, test_narrowed_words.FILL, what), NARROW_FIELDS if kind == "packed10" else NARROW_V210
        post = lambda planes: [narrowed_definition(p, 1023).astype(np.uint16) for p in planes]
        wants = [O.OracleFilter(O.FORMATS[fname], *geo, tap=3).get_frame(m, threads=4) for m in model]
    else:
        geo = test_chroma_out.GEOM
        fname = "YUV420P10" if name == "shifted_packed10" else "YUV422P10"
        model, wants = test_chroma_out.frames_and_wants(O, pkg, fname, geo, (0, 0), {}, n)
        f = test_chroma_out.make(pkg, fname, geo, "444", {})
        dst = PackedSide(torch, f.out_dims(), Y410, n, seed=12).upload()
        if name == "shifted_packed10":
            raw = [[(p.astype(np.uint16) << 6) for p in planes] for planes in model]
            src = Side(torch, f.fmt.plane_dims(geo[0], geo[1]), np.uint16, semi_planar(), n, seed=11).fill(raw).upload()
            move_far(arenas, src if far_side == "src" else dst, far_side, n)
            f.process_device_shifted_packed10(src.ptrs(), src.pitches(), src.steps(), [6, 6, 6], src.strides(), dst.ptrs()[0], dst.pitches()[0], Y410, OPAQUE,
                                              dst.strides()[0], n, stream=s.cuda_stream)
            direction = SPLIT if far_side == "src" else PACK_FIELDS
        else:
            src = V210Side(torch, f.fmt.plane_dims(geo[0], geo[1]), n, seed=11).fill(model).upload()
            move_far(arenas, src if far_side == "src" else dst, far_side, n)
            f.process_device_v210_packed10(src.ptrs()[0], src.pitches()[0], src.strides()[0], dst.ptrs()[0], dst.pitches()[0], Y410, OPAQUE, dst.strides()[0], n,
                                           stream=s.cuda_stream)
            direction = UNPACK_V210 if far_side == "src" else PACK_FIELDS
        s.synchronize()
        got = dst.frames_and_guards(OPAQUE, what)
    try:
        report, groups = f.last_strided(), f.last_groups()
        print(f"far frames, {what}: last_strided {report}, directions {[g['direction'] for g in groups]}")
        assert (report[0] if far_side == "src" else report[1]) > 0, report
        assert direction in [g["direction"] for g in groups], (direction, groups)
        dense = run_planar(torch, f, model, n)
        if post is not None:
            wants, dense = [post(w) for w in wants], [post(d) for d in dense]
        dims = f.out_dims()
        _cmp(key, got, wants, dims, what + " against the oracle")
        _cmp(key, got, dense, dims, what + " against the planar call")
    finally:
        f.close()
