"""jinc_filter_process_device_v210 on the device: 10-bit 4:2:2 frames in 16-byte blocks of six pixels (four little-endian words,
three 10-bit fields each at bits 0, 10 and 20; the table is in include/jincresize_hip.h).  Every case is bit-exact against the CPU
oracle run on the field values AND against jinc_filter_process_device on dense planes of those values; the source blocks carry
pseudo-random bits in 30 - 31 and in the unused fields of partial blocks; every destination lies inside a larger buffer of
pseudo-random bytes, no byte outside the rows' v210_row_bytes(width) bytes may change (lead, row padding, frame gaps, trail) and
inside them bits 30 - 31 and the unused fields must be zeros.  The helpers for dense planes, the frames and the expectations are
test_strided.py's, those of the shifted call test_shifted.py's.

Shapes: a lane of the pack / unpack kernels owns one block (6 pixels) per trip, a wave 64 blocks = 384 pixels; whole blocks move in
pairs of lanes, what pairs leave over (the odd whole block, the partial last block) moves sample by sample.
  WIDE   386 x 9 -> 772 x 18: the source row is one whole trip (64 blocks) and a 2-pixel partial block on lane 0's second trip,
         with an odd chroma width of 193; the destination row is two whole trips (128 blocks) and a 4-pixel partial block; 9 and
         18 rows are no multiples of the 4 rows of a launch's row block.
  SHORT  20 x 12 -> 36 x 20: residues 2 and 0, block counts odd (3 whole: one pair, one odd whole block, then the partial one) and
         even (6: pairs only), rows far shorter than a trip.
  MID    22 x 8 -> 44 x 16: residues 4 and 2 (3 whole + 4 pixels; 7 whole + 2 pixels).
  NARROW 14 x 7 -> 16 x 8: the smallest source a tap-3 YUV422P10 filter accepts (its chroma plane is 7 x 7; 8 x 7 is refused),
         residues 2 and 4, two whole blocks each."""
import numpy as np
import pytest

from conftest import to_device, to_host
from test_shifted import raw_frames, values_of
from test_strided import INVALID_ARG, Side, assert_frames, frames_and_wants, planar, run_planar

pytestmark = pytest.mark.gpu

NAME = "YUV422P10"
WIDE = (386, 9, 772, 18)
SHORT = (20, 12, 36, 20)
MID = (22, 8, 44, 16)
NARROW = (14, 7, 16, 8)

# (plane, sample of the block, word, bit offset) of a block's twelve fields
FIELDS = [(1, 0, 0, 0), (0, 0, 0, 10), (2, 0, 0, 20),
          (0, 1, 1, 0), (1, 1, 1, 10), (0, 2, 1, 20),
          (2, 1, 2, 0), (0, 3, 2, 10), (1, 2, 2, 20),
          (0, 4, 3, 0), (2, 2, 3, 10), (0, 5, 3, 20)]


def row_bytes(width):
    return 16 * ((width + 5) // 6)


def conventional_pitch(width):
    return (row_bytes(width) + 127) // 128 * 128


class V210Side:
    """`n` frames of v210 blocks in one buffer of pseudo-random bytes: host image, device copy, pointers.  Elements [1] and [2] of
    pointers, pitches and strides are values the library would refuse if it read them."""

    def __init__(self, torch, dims, n, align=16, seed=1, lead=None, pitch=None, fs=None):
        (self.w, self.h), self.n = dims[0], n
        assert dims[1] == (self.w // 2, self.h) and dims[2] == dims[1] and self.w % 2 == 0
        self.row = row_bytes(self.w)
        self.nblocks = self.row // 16
        if align == 16:
            ld, p, gap = 64, self.row + 16, 32
        else:   # multiples of 4 only: lead 68, pitch and frame stride 4 mod 16
            ld, p = 68, self.row + 4
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
        return np.ndarray((self.h, self.nblocks, 4), "<u4", image, self.lead + k * self.fs, (self.pitch, 16, 4))

    def fields(self):
        """(plane, sample indices, blocks that hold one, word, bit offset) of the fields that carry a sample of the row."""
        for plane, j, word, offset in FIELDS:
            per, width = (6, self.w) if plane == 0 else (3, self.w // 2)
            x = per * np.arange(self.nblocks) + j
            valid = x < width
            yield plane, x[valid], np.flatnonzero(valid), word, offset

    def fill(self, frames):
        """The field values of frames[k][i]; every other bit of the blocks keeps the buffer's pseudo-random value."""
        for k in range(self.n):
            w = self.words(self.host, k)
            for plane, x, blocks, word, offset in self.fields():
                values = np.asarray(frames[k][plane], np.uint32)[:self.h, x]
                w[:, blocks, word] = (w[:, blocks, word] & np.uint32(~(1023 << offset) & 0xFFFFFFFF)) | (values << np.uint32(offset))
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

    def frames_and_guards(self, what=""):
        """The three planes of every frame, after asserting that no byte outside the rows' blocks has changed and that inside them
        every bit that carries no sample is zero."""
        image = self.download()
        untouched = np.ones(image.size, bool)
        for k in range(self.n):
            np.ndarray((self.h, self.row), np.bool_, untouched, self.lead + k * self.fs, (self.pitch, 1))[...] = False
        changed = np.flatnonzero(untouched & (image != self.host))
        assert changed.size == 0, f"{what}: {changed.size} guard bytes were written, first at byte {int(changed[0])} " \
                                  f"(lead {self.lead}, pitch {self.pitch}, frame stride {self.fs}, row {self.row} bytes)"
        used = np.zeros((self.nblocks, 4), np.uint32)
        for plane, x, blocks, word, offset in self.fields():
            used[blocks, word] |= np.uint32(1023 << offset)
        got = []
        for k in range(self.n):
            w = self.words(image, k)
            spare = int(np.count_nonzero(w & ~used[None, :, :]))
            assert spare == 0, f"{what}: frame {k}: {spare} words with bits set in 30 - 31 or in an unused field"
            planes = [np.zeros((self.h, self.w), np.uint16), np.zeros((self.h, self.w // 2), np.uint16), np.zeros((self.h, self.w // 2), np.uint16)]
            for plane, x, blocks, word, offset in self.fields():
                planes[plane][:, x] = (w[:, blocks, word] >> np.uint32(offset)) & np.uint32(1023)
            got.append(planes)
        return got


def make_side(torch, dims, dtype, is_v210, n, align, seed, **kw):
    if not is_v210:
        return Side(torch, dims, dtype, planar(3), n, seed=seed)
    return V210Side(torch, dims, n, align, seed=seed, **kw)


def make_sides(torch, f, frames, src_v210, dst_v210, n, src_align=16, dst_align=16, seeds=(11, 12), src_kw=None, dst_kw=None):
    fmt = f.fmt
    src = make_side(torch, fmt.plane_dims(f.src_w, f.src_h), fmt.dtype, src_v210, n, src_align, seeds[0], **(src_kw or {})).fill(frames).upload()
    dst = make_side(torch, f.out_dims(), fmt.dtype, dst_v210, n, dst_align, seeds[1], **(dst_kw or {})).upload()
    return src, dst


def call(f, src, dst, src_v210, dst_v210, n, stream):
    f.process_device_v210(src.ptrs(), src.pitches(), src_v210, src.strides(), dst.ptrs(), dst.pitches(), dst_v210, dst.strides(), n,
                          stream=stream.cuda_stream)


_PLANAR = {}


def planar_results(torch, f, key, frames, n):
    """jinc_filter_process_device on dense planes of the values: once per geometry, arguments and frame count."""
    if key not in _PLANAR:
        _PLANAR[key] = run_planar(torch, f, frames, n)
    return _PLANAR[key]


def check_call(torch, O, pkg, geom, n, src_v210=True, dst_v210=True, kw=None, expect_report=None, **side_kw):
    sw, sh, tw, th = geom
    kw = kw or dict(tap=3)
    frames, wants = frames_and_wants(O, pkg, NAME, sw, sh, tw, th, kw, n)
    f = pkg.Filter(pkg.FORMATS[NAME], sw, sh, tw, th, device=0, **kw)
    what = f"{NAME} {sw}x{sh}->{tw}x{th} {kw} {n} frame(s) v210 {int(src_v210)} -> {int(dst_v210)} {side_kw}"
    src, dst = make_sides(torch, f, frames, src_v210, dst_v210, n, **side_kw)
    s = torch.cuda.current_stream()
    call(f, src, dst, src_v210, dst_v210, n, s)
    s.synchronize()
    report = f.last_strided()
    print(f"{what}: last_strided {report}")
    got = dst.frames_and_guards(what)
    if expect_report is None:
        expect_report = (int(src_v210), int(dst_v210), 1)
    assert report[:3] == expect_report, report
    assert_frames(f.fmt, got, wants, f.out_dims(), what + " against the oracle")
    key = tuple(geom) + tuple(sorted(kw.items())) + (n,)
    assert_frames(f.fmt, got, planar_results(torch, f, key, frames, n), f.out_dims(), what + " against the planar call")
    f.close()


GEOMS = dict(argvalues=[WIDE, SHORT, MID, NARROW], ids=["386x9", "20x12", "22x8", "14x7"])


# ---- 1. v210 on both sides -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("geom", **GEOMS)
def test_v210_in_and_out(gpu_pkg, O, geom, n):
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, geom, n)


# ---- 2. one side only --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("geom", [WIDE, NARROW], ids=["386x9", "14x7"])
def test_v210_in_planar_out_and_the_reverse(gpu_pkg, O, geom, n):
    """The dense side is the caller's planes where they lie (guard bytes checked as in test_strided.py)."""
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, geom, n, True, False, expect_report=(1, 0, 1))
    check_call(torch, O, gpu_pkg, geom, n, False, True, expect_report=(0, 1, 1))


# ---- 3. both sides dense -----------------------------------------------------------------------------------------------------------------

def test_with_both_sides_dense_the_call_is_the_planar_call(gpu_pkg, O):
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = SHORT
    n = 3
    frames, wants = frames_and_wants(O, gpu_pkg, NAME, sw, sh, tw, th, dict(tap=3), n)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[NAME], sw, sh, tw, th, device=0, tap=3)
    run_planar(torch, f, frames, n)
    planar_call = gpu_pkg.last_call()
    src, dst = make_sides(torch, f, frames, False, False, n)
    s = torch.cuda.current_stream()
    call(f, src, dst, False, False, n, s)
    s.synchronize()
    assert f.last_strided()[:3] == (0, 0, 0) and gpu_pkg.last_call() == planar_call and planar_call[1] == n
    assert_frames(f.fmt, dst.frames_and_guards("both sides dense"), wants, f.out_dims(), "both sides dense")
    f.close()


# ---- 4. alignment ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("geom", [WIDE, SHORT], ids=["386x9", "20x12"])
@pytest.mark.parametrize("src_align,dst_align", [(4, 4), (16, 4), (4, 16)], ids=["4_4", "16_4", "4_16"])
def test_multiples_of_4_only(gpu_pkg, O, src_align, dst_align, geom, n):
    """Lead 68, pitch and frame stride 4 mod 16: dword accesses on that side.  (Multiples of 16 on both sides: every other test.)"""
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, geom, n, src_align=src_align, dst_align=dst_align)
    # the record (jinc_debug_last_groups): unpack_v210 is direction 7, pack_v210 8; vec_pixels: 6 pixels x the blocks that move in pairs
    unpack, pack = gpu_pkg.last_groups()
    assert (unpack["direction"], unpack["unit"], unpack["vec_pixels"], unpack["width"], unpack["rows"]) == (7, src_align, 6 * (geom[0] // 6 // 2 * 2), geom[0], geom[1]), unpack
    assert (pack["direction"], pack["unit"], pack["vec_pixels"], pack["width"], pack["rows"]) == (8, dst_align, 6 * (geom[2] // 6 // 2 * 2), geom[2], geom[3]), pack


def test_source_rows_longer_than_one_trip_of_the_wave(gpu_pkg, O):
    """782 x 7 -> 1564 x 14: 130 whole blocks and a 2-pixel partial one on the source, so lanes 0 and 1 make a second trip of the
    paired loop of unpack_v210_kernel, DPP exchange included; the destination's 260 whole blocks are four trips and four lanes."""
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, (782, 7, 1564, 14), 2)
    unpack, pack = gpu_pkg.last_groups()
    assert (unpack["direction"], unpack["unit"], unpack["vec_pixels"], unpack["width"]) == (7, 16, 780, 782) and unpack["vec_pixels"] > 6 * 128
    assert (pack["direction"], pack["unit"], pack["vec_pixels"], pack["width"]) == (8, 16, 1560, 1564)


# ---- 5. / 6. pitches ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", [WIDE, SHORT], ids=["386x9", "20x12"])
def test_the_smallest_pitch_is_accepted(gpu_pkg, O, geom):
    """pitch = v210_row_bytes(width) on both sides: rows follow each other without padding, the frames too."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = geom
    assert gpu_pkg.v210_row_bytes(sw) == row_bytes(sw) and gpu_pkg.v210_row_bytes(tw) == row_bytes(tw)
    check_call(torch, O, gpu_pkg, geom, 3, src_kw=dict(pitch=row_bytes(sw), fs=row_bytes(sw) * sh), dst_kw=dict(pitch=row_bytes(tw), fs=row_bytes(tw) * th))


@pytest.mark.parametrize("geom", [WIDE, SHORT], ids=["386x9", "20x12"])
def test_the_conventional_128_byte_pitch(gpu_pkg, O, geom):
    """Rows padded to 128 bytes (48 pixels) as capture cards write them, frames back to back: 1040 -> 1152 and 2064 -> 2176 bytes
    (WIDE), 64 -> 128 and 96 -> 128 (SHORT).  The padding is guard bytes: it must stay as it was."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = geom
    sp, dp = conventional_pitch(sw), conventional_pitch(tw)
    assert sp > row_bytes(sw) and dp > row_bytes(tw) and sp % 128 == 0 and dp % 128 == 0
    check_call(torch, O, gpu_pkg, geom, 3, src_kw=dict(pitch=sp, fs=sp * sh), dst_kw=dict(pitch=dp, fs=dp * th))


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------

def test_misaligned_or_short_rows_are_refused_and_nothing_is_written(gpu_pkg, O):
    """Base, pitch, frame stride at 2 mod 4, and a pitch of v210_row_bytes(width) - 4, on either side: INVALID_ARG, no launch, the
    destination byte for byte as it was."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = SHORT
    n = 3
    frames, _ = frames_and_wants(O, gpu_pkg, NAME, sw, sh, tw, th, dict(tap=3), n)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[NAME], sw, sh, tw, th, device=0, tap=3)
    src, dst = make_sides(torch, f, frames, True, True, n)
    s = torch.cuda.current_stream()
    call(f, src, dst, True, True, n, s)   # a good call first: the report of a refused one must not be this one's
    s.synchronize()
    assert f.last_strided()[:3] == (1, 1, 1)
    dst = V210Side(torch, f.out_dims(), n, seed=42).upload()
    good = dict(sp=src.ptrs(), spitch=src.pitches(), sfs=src.strides(), dp=dst.ptrs(), dpitch=dst.pitches(), dfs=dst.strides())
    bad = []
    for side, width in (("s", sw), ("d", tw)):
        bad.append({side + "p": [good[side + "p"][0] + 2, 1, 3]})
        bad.append({side + "pitch": [good[side + "pitch"][0] + 2, 3, -2]})
        bad.append({side + "fs": [good[side + "fs"][0] + 2, 1, 2]})
        bad.append({side + "pitch": [row_bytes(width) - 4, 3, -2]})
    messages = set()
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(gpu_pkg.JincError) as e:
            f.process_device_v210(a["sp"], a["spitch"], True, a["sfs"], a["dp"], a["dpitch"], True, a["dfs"], n, stream=s.cuda_stream)
        assert e.value.code == INVALID_ARG and str(e.value).startswith("JincResize:"), (change, str(e.value))
        assert f.last_strided()[:3] == (0, 0, 0), (change, f.last_strided())
        messages.add(str(e.value))
    print(sorted(messages))
    assert len(messages) == 4   # alignment of the base, of the pitch, of the frame stride; the short pitch
    s.synchronize()
    assert np.array_equal(dst.download(), dst.host), "a refused call wrote to the destination"
    f.close()


# ---- 8. slices ---------------------------------------------------------------------------------------------------------------------------

def test_a_call_beyond_the_scratch_cap_runs_in_slices(gpu_pkg, O):
    """Dense stand-ins per frame of WIDE, rows padded to 256 bytes.  Source: luma 386 x 2 = 772 -> 1024 bytes, each chroma plane
    193 x 2 = 386 -> 512 bytes, x 9 rows = 9 x (1024 + 2 x 512) = 18 432.  Destination: luma 772 x 2 = 1544 -> 1792 bytes, each
    chroma plane 386 x 2 = 772 -> 1024 bytes, x 18 rows = 18 x (1792 + 2 x 1024) = 69 120.  Together 87 552 bytes.  With the cap
    just below two frames' worth a call of 5 runs frame by frame; with room for two, as 2 + 2 + 1."""
    torch = pytest.importorskip("torch")
    per_frame = 9 * (1024 + 2 * 512) + 18 * (1792 + 2 * 1024)
    assert per_frame == 87552
    with gpu_pkg.knobs(strided_scratch_bytes=2 * per_frame - 256):
        check_call(torch, O, gpu_pkg, WIDE, 5, expect_report=(5, 5, 5))
    with gpu_pkg.knobs(strided_scratch_bytes=2 * per_frame):
        check_call(torch, O, gpu_pkg, WIDE, 5, expect_report=(3, 3, 3))


# ---- 9. two streams ----------------------------------------------------------------------------------------------------------------------

def test_two_calls_back_to_back_on_two_streams(gpu_pkg, O):
    """One filter, two calls on different frames queued without a synchronise in between on two streams: they share the dense
    stand-ins, so the second call's unpack waits for the first call's pack."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = WIDE
    frames, wants = frames_and_wants(O, gpu_pkg, NAME, sw, sh, tw, th, dict(tap=3), 6)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[NAME], sw, sh, tw, th, device=0, tap=3)
    sides = [make_sides(torch, f, frames[3 * c:3 * c + 3], True, True, 3, seeds=(21 + c, 31 + c)) for c in range(2)]
    torch.cuda.synchronize()   # (the uploads are done before the side streams start)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for c, (src, dst) in enumerate(sides):
        call(f, src, dst, True, True, 3, streams[c])
    torch.cuda.synchronize()
    for c, (src, dst) in enumerate(sides):
        assert_frames(f.fmt, dst.frames_and_guards(f"call {c}"), wants[3 * c:3 * c + 3], f.out_dims(), f"call {c} of two streams")
    f.close()


# ---- 10. the scratch and the event ring serve the shifted call too --------------------------------------------------------------------

def test_v210_and_shifted_calls_alternate_on_one_filter(gpu_pkg, O):
    """A v210 call and a shifted call (planar layout, every plane shifted by 6 on both sides: three stand-ins per side as well) take
    turns on two streams without a synchronise in between, twice over."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = WIDE
    frames, wants = frames_and_wants(O, gpu_pkg, NAME, sw, sh, tw, th, dict(tap=3), 4)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[NAME], sw, sh, tw, th, device=0, tap=3)
    fmt = f.fmt
    calls = []
    for c in range(4):
        mine = frames[c:c + 1] * 2 if c == 3 else frames[c:c + 2]   # two frames per call
        want = wants[c:c + 1] * 2 if c == 3 else wants[c:c + 2]
        if c % 2 == 0:
            src, dst = make_sides(torch, f, mine, True, True, 2, seeds=(51 + c, 61 + c))
        else:
            src = Side(torch, fmt.plane_dims(sw, sh), fmt.dtype, planar(3), 2, seed=51 + c).fill(raw_frames(mine, [6] * 3, 71 + c)).upload()
            dst = Side(torch, f.out_dims(), fmt.dtype, planar(3), 2, seed=61 + c).upload()
        calls.append((src, dst, want))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    reports = []
    for c, (src, dst, want) in enumerate(calls):
        if c % 2 == 0:
            call(f, src, dst, True, True, 2, streams[c % 2])
        else:
            f.process_device_shifted(src.ptrs(), src.pitches(), None, [6] * 3, src.strides(), dst.ptrs(), dst.pitches(), None, [6] * 3, dst.strides(), 2,
                                     stream=streams[c % 2].cuda_stream)
        reports.append(f.last_strided()[:3])
    torch.cuda.synchronize()
    assert reports == [(1, 1, 1)] * 4, reports
    for c, (src, dst, want) in enumerate(calls):
        got = dst.frames_and_guards(f"call {c}") if c % 2 == 0 else values_of(dst.frames_and_guards(f"call {c}"), [6] * 3, f"call {c}")
        assert_frames(fmt, got, want, f.out_dims(), f"call {c} ({'v210' if c % 2 == 0 else 'shifted'})")
    f.close()


# ---- 11. other plans ---------------------------------------------------------------------------------------------------------------------

OTHER = [(WIDE, dict(tap=4)), ((150, 100, 206, 137), dict(tap=3)), ((300, 200, 150, 100), dict(tap=3))]


@pytest.mark.parametrize("geom,kw", OTHER, ids=["tap4_2x", "150x100_to_206x137", "300x200_to_150x100"])
def test_other_plans_behind_the_passes(gpu_pkg, O, geom, kw):
    """Whatever arithmetic kernels the rules choose run on the stand-ins: not only the 2x tap-3 family."""
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, geom, 2, kw=kw)
