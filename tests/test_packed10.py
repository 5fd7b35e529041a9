"""jinc_filter_process_device_packed10 on the device: frames that keep three 10-bit samples in ONE 32-bit word per pixel (Y410,
R10G10B10A2 and the DRM 2101010 / 1010102 orders).  Every case is bit-exact against the CPU oracle run on the field values AND
against jinc_filter_process_device on dense planes of those values; the source words carry pseudo-random bits outside the fields;
every destination word must hold the fill outside its fields; every destination lies inside a larger buffer of pseudo-random bytes
and no byte outside the rows' 4 * width bytes may change (lead, row padding, frame gaps, trail).  The helpers for dense planes, the
frames and the expectations are test_strided.py's.

Shapes: a lane of the pack / unpack kernels owns 8 pixels per step, a wave 512.  261 x 21 -> 522 x 42: the source row is one trip
with a 5-pixel tail, the destination row gives lane 0 a second trip and leaves a 2-pixel tail, 21 and 42 rows are no multiples of the
4 rows of a block.  20 x 12 -> 36 x 20: short rows, 4-pixel tails.  7 x 7 -> 7 x 8: rows shorter than a lane's 8 pixels, everything
goes through the tail (6 x 5 -> 7 x 6 is refused by the filter -- the source is smaller than the tap-3 footprint; 7 x 7 is the
smallest source it takes at tap 3)."""
import numpy as np
import pytest

from conftest import to_device, to_host
from test_shifted import raw_frames, values_of
from test_strided import INVALID_ARG, Side, assert_frames, frames_and_wants, planar, run_planar

pytestmark = pytest.mark.gpu

Y410 = [10, 0, 20]
R10G10B10A2 = [10, 20, 0]
BGRX1010102 = [12, 22, 2]
ODD = [22, 0, 11]          # a legal word no format uses: spare bits 10 and 21
OPAQUE = 0xC0000000

WIDE = (261, 21, 522, 42)
SHORT = (20, 12, 36, 20)
NARROW = (7, 7, 7, 8)


def fields_mask(offsets):
    return sum(1023 << o for o in offsets) & 0xFFFFFFFF


class PackedSide:
    """`n` frames of 32-bit words in one buffer of pseudo-random bytes: host image, device copy, pointers.  Elements [1] and [2] of
    pointers, pitches and strides are values the library would refuse if it read them."""

    def __init__(self, torch, dims, offsets, n, align=16, seed=1, lead=None, pitch=None, fs=None):
        (self.w, self.h), self.offsets, self.n = dims[0], list(offsets), n
        row = 4 * self.w
        if align == 16:
            ld, p, gap = 64, (row + 15) // 16 * 16 + 16, 32
        else:   # multiples of 4 only: lead 68, pitch and frame stride 4 mod 16
            ld, p = 68, (row + 15) // 16 * 16 + 4
            gap = (4 - p * self.h) % 16 + 16
        self.lead = ld if lead is None else lead
        self.pitch = p if pitch is None else pitch
        self.fs = self.pitch * self.h + gap if fs is None else fs
        if align == 16:
            assert self.lead % 16 == 0 and self.pitch % 16 == 0 and self.fs % 16 == 0
        elif lead is None and pitch is None and fs is None:
            assert self.lead % 16 == 4 and self.pitch % 16 == 4 and self.fs % 16 == 4
        rng = np.random.default_rng(seed)
        self.host = rng.integers(0, 256, self.lead + n * self.fs + 256, dtype=np.uint8)
        self.torch, self.dev = torch, None

    def words(self, image, k):
        return np.ndarray((self.h, self.w), "<u4", image, self.lead + k * self.fs, (self.pitch, 4))

    def fill(self, frames):
        """The field values of frames[k][i], pseudo-random bits everywhere else in the word."""
        keep = np.uint32(~fields_mask(self.offsets) & 0xFFFFFFFF)
        for k in range(self.n):
            w = self.words(self.host, k)
            word = w & keep   # (the buffer's own random bytes)
            for i, o in enumerate(self.offsets):
                word |= np.asarray(frames[k][i][:self.h, :self.w], np.uint32) << np.uint32(o)
            w[...] = word
        return self

    def upload(self):
        self.dev = to_device(self.torch.from_numpy(self.host))
        return self

    def ptrs(self):
        return [self.dev.data_ptr() + self.lead, 1, 3]

    def pitches(self):
        return [self.pitch, 3, -2]

    def strides(self):
        return [self.fs, 1, 2]

    def download(self):
        return to_host(self.dev).numpy()

    def frames_and_guards(self, fill, what=""):
        """The three planes of every frame, after asserting that every word holds `fill` outside its fields and that no byte outside
        the rows' words has changed."""
        image = self.download()
        untouched = np.ones(image.size, bool)
        for k in range(self.n):
            np.ndarray((self.h, 4 * self.w), np.bool_, untouched, self.lead + k * self.fs, (self.pitch, 1))[...] = False
        changed = np.flatnonzero(untouched & (image != self.host))
        assert changed.size == 0, f"{what}: {changed.size} guard bytes were written, first at byte {int(changed[0])} " \
                                  f"(lead {self.lead}, pitch {self.pitch}, frame stride {self.fs}, row {4 * self.w} bytes)"
        mask = fields_mask(self.offsets)
        got = []
        for k in range(self.n):
            w = self.words(image, k)
            spare = int(np.count_nonzero((w & np.uint32(~mask & 0xFFFFFFFF)) != np.uint32(fill & ~mask & 0xFFFFFFFF)))
            assert spare == 0, f"{what}: frame {k}: {spare} words whose bits outside the fields are not the fill's"
            got.append([((w >> np.uint32(o)) & np.uint32(1023)).astype(np.uint16) for o in self.offsets])
        return got


def make_side(torch, dims, dtype, offsets, n, align, seed, **kw):
    if offsets is None:
        return Side(torch, dims, dtype, planar(3), n, seed=seed)
    return PackedSide(torch, dims, offsets, n, align, seed=seed, **kw)


def make_sides(torch, f, frames, src_off, dst_off, n, src_align=16, dst_align=16, seeds=(11, 12), src_kw=None, dst_kw=None):
    fmt = f.fmt
    src = make_side(torch, fmt.plane_dims(f.src_w, f.src_h), fmt.dtype, src_off, n, src_align, seeds[0], **(src_kw or {})).fill(frames).upload()
    dst = make_side(torch, f.out_dims(), fmt.dtype, dst_off, n, dst_align, seeds[1], **(dst_kw or {})).upload()
    return src, dst


def call(f, src, dst, src_off, dst_off, fill, n, stream):
    f.process_device_packed10(src.ptrs(), src.pitches(), src_off, src.strides(), dst.ptrs(), dst.pitches(), dst_off, fill, dst.strides(), n,
                              stream=stream.cuda_stream)


def results(dst, dst_off, fill, what):
    return dst.frames_and_guards(what) if dst_off is None else dst.frames_and_guards(fill, what)


_PLANAR = {}


def planar_results(torch, f, key, frames, n):
    """jinc_filter_process_device on dense planes of the values: once per geometry, arguments and frame count."""
    if key not in _PLANAR:
        _PLANAR[key] = run_planar(torch, f, frames, n)
    return _PLANAR[key]


def check_call(torch, O, pkg, name, geom, n, src_off, dst_off, fill=OPAQUE, kw=None, expect_report=None, **side_kw):
    sw, sh, tw, th = geom
    kw = kw or dict(tap=3)
    frames, wants = frames_and_wants(O, pkg, name, sw, sh, tw, th, kw, n)
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=0, **kw)
    what = f"{name} {sw}x{sh}->{tw}x{th} {kw} {n} frame(s) offsets {src_off} -> {dst_off} fill {fill:#x}"
    src, dst = make_sides(torch, f, frames, src_off, dst_off, n, **side_kw)
    s = torch.cuda.current_stream()
    call(f, src, dst, src_off, dst_off, fill, n, s)
    s.synchronize()
    report = f.last_strided()
    print(f"{what}: last_strided {report}")
    got = results(dst, dst_off, fill, what)
    if expect_report is None:
        expect_report = (int(src_off is not None), int(dst_off is not None), 1)
    assert report[:3] == expect_report, report
    assert_frames(f.fmt, got, wants, f.out_dims(), what + " against the oracle")
    key = (name,) + tuple(geom) + tuple(sorted(kw.items())) + (n,)
    assert_frames(f.fmt, got, planar_results(torch, f, key, frames, n), f.out_dims(), what + " against the planar call")
    f.close()


# ---- 1. layouts ------------------------------------------------------------------------------------------------------------------------

LAYOUT_CASES = [("YUV444P10", Y410, Y410, OPAQUE), ("RGBP10", R10G10B10A2, BGRX1010102, 3), ("RGBP10", R10G10B10A2, BGRX1010102, 0),
                ("YUV444P10", ODD, ODD, 0xFFFFFFFF), ("RGBP10", ODD, Y410, 0x00200400)]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("geom", [WIDE, SHORT, NARROW], ids=["261x21", "20x12", "7x7"])
@pytest.mark.parametrize("name,src_off,dst_off,fill", LAYOUT_CASES, ids=["Y410", "R10G10B10A2_to_BGRX_fill3", "R10G10B10A2_to_BGRX_fill0", "odd_ones", "odd_to_Y410"])
def test_layouts(gpu_pkg, O, name, src_off, dst_off, fill, geom, n):
    """Y410 in and out, opaque; R10G10B10A2 in and BGRX1010102 out with both spare bits set and clear; a word no format uses, with a
    fill of all ones (the fields must be cleared from it) and one whose set bits lie INSIDE the destination's fields (ignored)."""
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, name, geom, n, src_off, dst_off, fill)


def test_the_named_layouts_drive_a_call(gpu_pkg, O):
    torch = pytest.importorskip("torch")
    src_off, _ = gpu_pkg.packed10_layout("xrgb2101010")
    dst_off, fill = gpu_pkg.packed10_layout("RGBA1010102")
    assert fill == 3
    check_call(torch, O, gpu_pkg, "RGBP10", SHORT, 2, src_off, dst_off, fill)


# ---- 2. alignment ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("geom", [WIDE, SHORT, NARROW], ids=["261x21", "20x12", "7x7"])
@pytest.mark.parametrize("src_align,dst_align", [(4, 4), (16, 4), (4, 16)], ids=["4_4", "16_4", "4_16"])
def test_multiples_of_4_only(gpu_pkg, O, src_align, dst_align, geom, n):
    """Lead 68, pitch and frame stride 4 mod 16: dword accesses on that side.  (Multiples of 16 on both sides: every other test.)"""
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, "YUV444P10", geom, n, Y410, Y410, src_align=src_align, dst_align=dst_align)
    # the record (jinc_debug_last_groups): unpack_fields is direction 4, pack_fields 5; a lane moves 8 pixels per step
    unpack, pack = gpu_pkg.last_groups()
    assert (unpack["direction"], unpack["unit"], unpack["vec_pixels"], unpack["width"], unpack["rows"]) == (4, src_align, geom[0] // 8 * 8, geom[0], geom[1]), unpack
    assert (pack["direction"], pack["unit"], pack["vec_pixels"], pack["width"], pack["rows"]) == (5, dst_align, geom[2] // 8 * 8, geom[2], geom[3]), pack


def test_rows_longer_than_one_trip_of_the_wave_on_both_sides(gpu_pkg, O):
    """526 x 7 -> 1052 x 14: a lane owns 8 pixels and a wave's trip is 512, so the source's 520 + 6 send lane 0 on a second trip of the
    vector loop in unpack_fields_kernel, and the destination's 1048 + 4 are two whole trips and three lanes of a third in
    pack_fields_kernel."""
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, "YUV444P10", (526, 7, 1052, 14), 2, Y410, Y410)
    unpack, pack = gpu_pkg.last_groups()
    assert (unpack["direction"], unpack["unit"], unpack["vec_pixels"], unpack["width"]) == (4, 16, 520, 526) and unpack["vec_pixels"] > 512
    assert (pack["direction"], pack["unit"], pack["vec_pixels"], pack["width"]) == (5, 16, 1048, 1052) and pack["vec_pixels"] > 512


def test_the_smallest_pitch_is_accepted(gpu_pkg, O):
    """pitch = 4 * width on both sides: rows follow each other without padding, the frames too."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = SHORT
    check_call(torch, O, gpu_pkg, "YUV444P10", SHORT, 3, Y410, Y410, src_kw=dict(pitch=4 * sw, fs=4 * sw * sh), dst_kw=dict(pitch=4 * tw, fs=4 * tw * th))


def test_misaligned_or_short_rows_are_refused_and_nothing_is_written(gpu_pkg, O):
    """Base, pitch, frame stride at 2 mod 4, and a pitch of 4 * width - 4, on either side: INVALID_ARG, no launch, the destination
    byte for byte as it was."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = SHORT
    n = 3
    frames, _ = frames_and_wants(O, gpu_pkg, "YUV444P10", sw, sh, tw, th, dict(tap=3), n)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YUV444P10"], sw, sh, tw, th, device=0, tap=3)
    src, dst = make_sides(torch, f, frames, Y410, Y410, n)
    s = torch.cuda.current_stream()
    call(f, src, dst, Y410, Y410, OPAQUE, n, s)   # a good call first: the report of a refused one must not be this one's
    s.synchronize()
    assert f.last_strided()[:3] == (1, 1, 1)
    dst = PackedSide(torch, f.out_dims(), Y410, n, seed=42).upload()
    good = dict(sp=src.ptrs(), spitch=src.pitches(), sfs=src.strides(), dp=dst.ptrs(), dpitch=dst.pitches(), dfs=dst.strides())
    bad = []
    for side, width in (("s", sw), ("d", tw)):
        bad.append({side + "p": [good[side + "p"][0] + 2, 1, 3]})
        bad.append({side + "pitch": [good[side + "pitch"][0] + 2, 3, -2]})
        bad.append({side + "fs": [good[side + "fs"][0] + 2, 1, 2]})
        bad.append({side + "pitch": [4 * width - 4, 3, -2]})
    messages = set()
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(gpu_pkg.JincError) as e:
            f.process_device_packed10(a["sp"], a["spitch"], Y410, a["sfs"], a["dp"], a["dpitch"], Y410, OPAQUE, a["dfs"], n, stream=s.cuda_stream)
        assert e.value.code == INVALID_ARG and str(e.value).startswith("JincResize:"), (change, str(e.value))
        assert f.last_strided()[:3] == (0, 0, 0), (change, f.last_strided())
        messages.add(str(e.value))
    print(sorted(messages))
    assert len(messages) == 4   # alignment of the base, of the pitch, of the frame stride; the short pitch
    s.synchronize()
    assert np.array_equal(dst.download(), dst.host), "a refused call wrote to the destination"
    f.close()


# ---- 3. one side only --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("geom", [WIDE, NARROW], ids=["261x21", "7x7"])
def test_y410_in_planar_out_and_the_reverse(gpu_pkg, O, geom, n):
    """The dense side is the caller's planes where they lie (guard bytes checked as in test_strided.py)."""
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, "YUV444P10", geom, n, Y410, None, expect_report=(1, 0, 1))
    check_call(torch, O, gpu_pkg, "YUV444P10", geom, n, None, Y410, expect_report=(0, 1, 1))


def test_with_both_sides_dense_the_call_is_the_planar_call(gpu_pkg, O):
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = SHORT
    n = 3
    frames, wants = frames_and_wants(O, gpu_pkg, "YUV444P10", sw, sh, tw, th, dict(tap=3), n)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YUV444P10"], sw, sh, tw, th, device=0, tap=3)
    run_planar(torch, f, frames, n)
    planar_call = gpu_pkg.last_call()
    src, dst = make_sides(torch, f, frames, None, None, n)
    s = torch.cuda.current_stream()
    call(f, src, dst, None, None, OPAQUE, n, s)
    s.synchronize()
    assert f.last_strided()[:3] == (0, 0, 0) and gpu_pkg.last_call() == planar_call and planar_call[1] == n
    assert_frames(f.fmt, dst.frames_and_guards("both sides dense"), wants, f.out_dims(), "both sides dense")
    f.close()


# ---- 4. slices ---------------------------------------------------------------------------------------------------------------------------

def test_a_call_beyond_the_scratch_cap_runs_in_slices(gpu_pkg, O):
    """Dense stand-ins per frame: 3 planes x (261 x 2 = 522 -> 768 bytes x 21 rows + 522 x 2 = 1044 -> 1280 bytes x 42 rows).  With
    the cap just below two frames' worth a call of 5 runs frame by frame; with room for two, as 2 + 2 + 1."""
    torch = pytest.importorskip("torch")
    per_frame = 3 * (768 * 21 + 1280 * 42)
    with gpu_pkg.knobs(strided_scratch_bytes=2 * per_frame - 256):
        check_call(torch, O, gpu_pkg, "YUV444P10", WIDE, 5, Y410, Y410, expect_report=(5, 5, 5))
    with gpu_pkg.knobs(strided_scratch_bytes=2 * per_frame):
        check_call(torch, O, gpu_pkg, "YUV444P10", WIDE, 5, Y410, Y410, expect_report=(3, 3, 3))


# ---- 5. two streams ----------------------------------------------------------------------------------------------------------------------

def test_two_calls_back_to_back_on_two_streams(gpu_pkg, O):
    """One filter, two calls on different frames queued without a synchronise in between on two streams: they share the dense
    stand-ins, so the second call's unpack waits for the first call's pack."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = WIDE
    frames, wants = frames_and_wants(O, gpu_pkg, "YUV444P10", sw, sh, tw, th, dict(tap=3), 6)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YUV444P10"], sw, sh, tw, th, device=0, tap=3)
    sides = [make_sides(torch, f, frames[3 * c:3 * c + 3], Y410, Y410, 3, seeds=(21 + c, 31 + c)) for c in range(2)]
    torch.cuda.synchronize()   # (the uploads are done before the side streams start)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for c, (src, dst) in enumerate(sides):
        call(f, src, dst, Y410, Y410, OPAQUE, 3, streams[c])
    torch.cuda.synchronize()
    for c, (src, dst) in enumerate(sides):
        assert_frames(f.fmt, dst.frames_and_guards(OPAQUE, f"call {c}"), wants[3 * c:3 * c + 3], f.out_dims(), f"call {c} of two streams")
    f.close()


# ---- 6. the scratch and the event ring serve the shifted call too ---------------------------------------------------------------------

def test_packed10_and_shifted_calls_alternate_on_one_filter(gpu_pkg, O):
    """YUV444P10: a Y410 call and a shifted call (planar layout, every plane shifted by 6 on both sides: three stand-ins per side
    as well) take turns on two streams without a synchronise in between, twice over."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = WIDE
    frames, wants = frames_and_wants(O, gpu_pkg, "YUV444P10", sw, sh, tw, th, dict(tap=3), 4)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YUV444P10"], sw, sh, tw, th, device=0, tap=3)
    fmt = f.fmt
    calls = []
    for c in range(4):
        mine = frames[c:c + 1] * 2 if c == 3 else frames[c:c + 2]   # two frames per call
        want = wants[c:c + 1] * 2 if c == 3 else wants[c:c + 2]
        if c % 2 == 0:
            src, dst = make_sides(torch, f, mine, Y410, Y410, 2, seeds=(51 + c, 61 + c))
        else:
            src = Side(torch, fmt.plane_dims(sw, sh), fmt.dtype, planar(3), 2, seed=51 + c).fill(raw_frames(mine, [6] * 3, 71 + c)).upload()
            dst = Side(torch, f.out_dims(), fmt.dtype, planar(3), 2, seed=61 + c).upload()
        calls.append((src, dst, want))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    reports = []
    for c, (src, dst, want) in enumerate(calls):
        if c % 2 == 0:
            call(f, src, dst, Y410, Y410, OPAQUE, 2, streams[c % 2])
        else:
            f.process_device_shifted(src.ptrs(), src.pitches(), None, [6] * 3, src.strides(), dst.ptrs(), dst.pitches(), None, [6] * 3, dst.strides(), 2,
                                     stream=streams[c % 2].cuda_stream)
        reports.append(f.last_strided()[:3])
    torch.cuda.synchronize()
    assert reports == [(1, 1, 1)] * 4, reports
    for c, (src, dst, want) in enumerate(calls):
        got = dst.frames_and_guards(OPAQUE, f"call {c}") if c % 2 == 0 else values_of(dst.frames_and_guards(f"call {c}"), [6] * 3, f"call {c}")
        assert_frames(fmt, got, want, f.out_dims(), f"call {c} ({'packed10' if c % 2 == 0 else 'shifted'})")
    f.close()


# ---- 7. other plans ------------------------------------------------------------------------------------------------------------------------

OTHER = [(WIDE, dict(tap=4)), ((150, 100, 206, 137), dict(tap=3)), ((300, 200, 150, 100), dict(tap=3))]


@pytest.mark.parametrize("geom,kw", OTHER, ids=["tap4_2x", "150x100_to_206x137", "300x200_to_150x100"])
def test_other_plans_behind_the_passes(gpu_pkg, O, geom, kw):
    """Whatever arithmetic kernels the rules choose run on the stand-ins: not only the 2x tap-3 family."""
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, "RGBP10", geom, 2, R10G10B10A2, R10G10B10A2, fill=OPAQUE, kw=kw)
