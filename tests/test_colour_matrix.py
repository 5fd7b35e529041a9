"""jinc_filter_set_output_matrix on the device: every case runs the same call on a twin filter WITHOUT a matrix, applies the numpy
float32 emulation of
    o_i = fl32(fl32(fl32(fl32(m[3i] r0) + fl32(m[3i+1] r1)) + fl32(m[3i+2] r2)) + offset[i])
(tests/test_colour_matrix_host.py: products and sums taken one at a time, 16-bit filters rounded to nearest even) to the twin's
downloaded result planes, then the destination side's own documented arithmetic where there is one (the narrowed calls), and compares
the matrixed call's destination with that BIT FOR BIT -- every byte of the destination buffers, so the row gaps, the space between
frames and a channel that is not given must keep their sentinel.  The un-matrixed calls are pinned to the oracle by the rest of the
suite, which holds the feature to the oracle without touching it.

Not covered: a jinc_batch with a matrix.  A batch owns its filters and the interface has no way to give them a matrix, so the case
cannot be built; a batch submits through jinc_filter_submit, whose refusal is checked here."""
import numpy as np
import pytest

from conftest import to_device, to_host
from test_colour_matrix_host import BF16, HALF, emulate, narrow, widen

pytestmark = pytest.mark.gpu

UNSUPPORTED = -5
SENTINEL = 0xA5
OFFSET = [0.0625, -0.03125, 0.015625]


def _torch():
    return pytest.importorskip("torch")


def kind_of(fmt):
    return HALF if fmt.half else BF16 if fmt.bfloat16 else 0


def raw_type(fmt):
    return np.uint32 if fmt.sample_bytes == 4 else np.uint16


def align(v, a):
    return (v + a - 1) // a * a


class Dev:
    """A device copy of a host byte image (torch's allocations are at least 256-byte aligned: `lead` decides the access class)."""

    def __init__(self, image):
        self.t = to_device(_torch().from_numpy(image))
        self.ptr = self.t.data_ptr()
        assert self.ptr % 256 == 0

    def host(self):
        return to_host(self.t).numpy()


def chan(image, lay, n, h, w, dt):
    """The (n, h, w) samples of one plane or channel inside a byte image; lay = (buffer, offset, frame stride, pitch, sample step)."""
    _, off, fs, pitch, step = lay
    return np.ndarray((n, h, w), dt, image, off, (fs, pitch, step * np.dtype(dt).itemsize))


def planar_side(sb, w, h, n, nplanes, lead=0, pitch_extra=0):
    """Sentinel images and layouts of `nplanes` planes of one size, a buffer each, ending behind the last sample (plus a short tail)."""
    pitch = align(w * sb, 16) + pitch_extra
    fs = pitch * h + 64 + pitch_extra
    images = [np.full(lead + (n - 1) * fs + (h - 1) * pitch + w * sb + 32, SENTINEL, np.uint8) for _ in range(nplanes)]
    return images, [(c, lead, fs, pitch, 1) for c in range(nplanes)]


def interleaved_side(sb, w, h, n, step, channels, lead=0):
    """ONE buffer of `step` samples per pixel; channels: the channel of each plane."""
    pitch = align(w * step * sb, 4) + 4 * sb
    fs = pitch * h + 16 * sb
    image = np.full(lead + (n - 1) * fs + h * pitch + 32, SENTINEL, np.uint8)
    return [image], [(0, lead + c * sb, fs, pitch, step) for c in channels]


def float_frames(fmt, w, h, n, nplanes, seed):
    """n frames of normalised Y' (0 .. 1), Cb / Cr (-0.5 .. 0.5) and alpha planes as the format's bit patterns: [(n, h, w)] * nplanes."""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(nplanes):
        v = rng.random((n, h, w), dtype=np.float32) - (np.float32(0.5) if c in (1, 2) else np.float32(0))
        out.append(narrow(v, kind_of(fmt)).reshape(n, h, w))
    return out


def upload_planes(fmt, planes):
    """Dense source planes on the device: (devs, ptrs, pitches, frame strides)."""
    n, h, w = planes[0].shape
    images, lays = planar_side(fmt.sample_bytes, w, h, n, len(planes))
    for c, p in enumerate(planes):
        chan(images[c], lays[c], n, h, w, raw_type(fmt))[...] = p
    devs = [Dev(im) for im in images]
    return devs, [d.ptr + l[1] for d, l in zip(devs, lays)], [l[3] for l in lays], [l[2] for l in lays]


def side_args(devs, lays):
    return [devs[l[0]].ptr + l[1] for l in lays], [l[3] for l in lays], [l[2] for l in lays], [l[4] for l in lays]


def matrixed(fmt, twin_images, lays, n, h, w, m, offset):
    """What the matrixed call must leave where the twin left `twin_images`: planes 0 .. 2 through the emulation, every other byte as it is."""
    kind, dt = kind_of(fmt), raw_type(fmt)
    want = [im.copy() for im in twin_images]
    r = [widen(np.ascontiguousarray(chan(twin_images[l[0]], l, n, h, w, dt)), kind) for l in lays[:3]]
    assert all(np.isfinite(x).all() for x in r)
    o = emulate(r[0], r[1], r[2], m, offset)
    for c, l in enumerate(lays[:3]):
        chan(want[l[0]], l, n, h, w, dt)[...] = narrow(o[c], kind).reshape(n, h, w)
    assert any((a != b).any() for a, b in zip(want, twin_images)), "the matrix changes nothing: the case is vacuous"
    return want, o


def same_bytes(got, want, what):
    for b, (g, w_) in enumerate(zip(got, want)):
        bad = np.flatnonzero(g != w_)
        assert bad.size == 0, f"{what}: buffer {b}: {bad.size} bytes differ, first at {int(bad[0])}: got {int(g[bad[0]])}, want {int(w_[bad[0]])}"


def twins(pkg, fmt, geo, m, offset, out_sub=None, **kw):
    sw, sh, tw, th = geo
    f0 = pkg.Filter(fmt, sw, sh, tw, th, device=0, out_sub=out_sub, **kw)
    f1 = pkg.Filter(fmt, sw, sh, tw, th, device=0, out_sub=out_sub, **kw)
    f1.set_output_matrix(m, offset)
    return f0, f1


def run_both(pkg, f0, f1, images, call):
    """call(filter, devs) on the twin and on the matrixed filter, each into fresh copies of `images`; returns (twin images, matrixed
    images, matrix launches of the matrixed call, its last_strided)."""
    torch = _torch()
    d0, d1 = [Dev(im) for im in images], [Dev(im) for im in images]
    call(f0, d0)
    assert pkg.last_matrix_launches() == 0
    call(f1, d1)
    launches, strided = pkg.last_matrix_launches(), pkg.last_strided()
    torch.cuda.synchronize()
    return [d.host() for d in d0], [d.host() for d in d1], launches, strided


@pytest.fixture(scope="module")
def bt709(gpu_pkg):
    return gpu_pkg.colour_matrix(gpu_pkg.MATRIX_BT709, gpu_pkg.YCBCR_TO_RGB)


# ---- the planar call ------------------------------------------------------------------------------------------------------------------------

PLANAR = [("YUV444PS", 0, 0), ("YUV444PS", 4, 4), ("YUV444PH", 2, 2), ("YUV444PBF", 2, 2)]
# 131 x 7 -> 262 x 14.  (The issue names 131 x 5 -> 262 x 10; a tap-3 filter refuses source planes of fewer than 7 rows -- "smaller than
# the filter footprint" -- so no call exists on that shape.  7 rows is the smallest the filter takes; width, ratio, tap, frames, matrix
# and the three destination layouts are the issue's.)
GEO_PLANAR = (131, 7, 262, 14)


@pytest.mark.parametrize("name,lead,pitch_extra", PLANAR, ids=["f32_unit16", "f32_unit4", "f16_unit0", "bf16_unit0"])
def test_planar_call(gpu_pkg, bt709, name, lead, pitch_extra):
    """3 frames, tap 3: destination pitch a multiple of 16; a multiple of 4 only with the base moved by 4 bytes; 16-bit samples with the
    base moved by 2 bytes (the sample-by-sample path)."""
    pkg, fmt, n = gpu_pkg, gpu_pkg.FORMATS[name], 3
    sw, sh, tw, th = GEO_PLANAR
    src = upload_planes(fmt, float_frames(fmt, sw, sh, n, 3, 11))
    images, lays = planar_side(fmt.sample_bytes, tw, th, n, 3, lead, pitch_extra)
    al = lead | lays[0][3] | lays[0][2]
    assert (al % 16 == 0) == (lead == 0) and (al % 4 == 0) == (lead != 2)
    f0, f1 = twins(pkg, fmt, GEO_PLANAR, bt709, OFFSET, tap=3)

    def call(f, devs):
        ptrs, pitches, strides, _ = side_args(devs, lays)
        f.process_device(src[1], src[2], src[3], ptrs, pitches, strides, n)
    twin, got, launches, _ = run_both(pkg, f0, f1, images, call)
    want, _ = matrixed(fmt, twin, lays, n, th, tw, bt709, OFFSET)
    same_bytes(got, want, f"planar {name} lead {lead}")
    assert launches == 1
    f0.close(), f1.close()


def test_a_fourth_plane_is_not_touched(gpu_pkg, bt709):
    pkg, fmt, n, geo = gpu_pkg, gpu_pkg.FORMATS["YUVA444PS"], 2, (40, 12, 80, 24)
    sw, sh, tw, th = geo
    src = upload_planes(fmt, float_frames(fmt, sw, sh, n, 4, 12))
    images, lays = planar_side(4, tw, th, n, 4)
    f0, f1 = twins(pkg, fmt, geo, bt709, OFFSET, tap=3)

    def call(f, devs):
        ptrs, pitches, strides, _ = side_args(devs, lays)
        f.process_device(src[1], src[2], src[3], ptrs, pitches, strides, n)
    twin, got, launches, _ = run_both(pkg, f0, f1, images, call)
    want, _ = matrixed(fmt, twin, lays, n, th, tw, bt709, OFFSET)
    same_bytes(got, want, "YUVA444PS")
    assert np.array_equal(got[3], twin[3]) and (chan(got[3], lays[3], n, th, tw, np.uint32) != 0xA5A5A5A5).any() and launches == 1
    f0.close(), f1.close()


# ---- NV12 in, R'G'B' out: the widened scaled call on a 4:2:0 -> 4:4:4 filter --------------------------------------------------------------

GEO_NV12 = (38, 16, 77, 33)


def nv12_source(n, seed):
    """n limited-range NV12 frames of 38 x 16: (devs, ptrs, pitches, steps, strides) of Y, U = uv, V = uv + 1."""
    rng = np.random.default_rng(seed)
    sw, sh = GEO_NV12[:2]
    yi, yl = planar_side(1, sw, sh, n, 1)
    ci, cl = interleaved_side(1, sw // 2, sh // 2, n, 2, [0, 1])
    chan(yi[0], yl[0], n, sh, sw, np.uint8)[...] = rng.integers(16, 236, (n, sh, sw), dtype=np.uint8)
    for l in cl:
        chan(ci[0], l, n, sh // 2, sw // 2, np.uint8)[...] = rng.integers(16, 241, (n, sh // 2, sw // 2), dtype=np.uint8)
    devs = [Dev(yi[0]), Dev(ci[0])]
    lays = [yl[0], (1,) + cl[0][1:], (1,) + cl[1][1:]]
    return (devs,) + tuple(side_args(devs, lays))[:2] + ([1, 2, 2], [l[2] for l in lays])


def limited_pairs(pkg, bits=8):
    luma, chroma = pkg.code_range(bits, 1, 0), pkg.code_range(bits, 1, 1)
    return [luma[0], chroma[0], chroma[0]], [luma[1], chroma[1], chroma[1]], [luma[2], chroma[2], chroma[2]], [luma[3], chroma[3], chroma[3]]


@pytest.mark.parametrize("name,step", [("YUV420PS", 3), ("YUV420PH", 1), ("YUV420PBF", 1)], ids=["f32_rgb_step3", "f16_planes", "bf16_planes"])
def test_nv12_widened_scaled_into_rgb(gpu_pkg, bt709, name, step):
    """38 x 16 NV12 -> 77 x 33 (odd width: a tail; chroma brought to the luma grid by jinc_filter_create_out(..., 0, 0)): the fp32 filter
    into interleaved R'G'B' floats at destination step 3, the 16-bit filters into dense planes."""
    pkg, fmt, n = gpu_pkg, gpu_pkg.FORMATS[name], 2
    tw, th = GEO_NV12[2:]
    _, sp, spitch, ssteps, sstrides = src = nv12_source(n, 21)
    scale, off, _, _ = limited_pairs(pkg)
    if step == 3:
        images, lays = interleaved_side(4, tw, th, n, 3, [0, 1, 2])
    else:
        images, lays = planar_side(2, tw, th, n, 3)
    f0, f1 = twins(pkg, fmt, GEO_NV12, bt709, OFFSET, out_sub=(0, 0), tap=3)

    def call(f, devs):
        ptrs, pitches, strides, steps = side_args(devs, lays)
        f.process_device_widened_scaled(sp, spitch, ssteps, None, 8, scale, off, sstrides, ptrs, pitches, steps, strides, n)
    twin, got, launches, strided = run_both(pkg, f0, f1, images, call)
    want, _ = matrixed(fmt, twin, lays, n, th, tw, bt709, OFFSET)
    same_bytes(got, want, f"NV12 into {name} step {step}")
    assert launches == strided[2] == 1
    assert src[0] and f0.close() is None and f1.close() is None


# ---- the narrowed calls ---------------------------------------------------------------------------------------------------------------------

GEO_NARROW = (40, 12, 77, 23)


def narrow_codes(o, scale, offset, peak):
    """rint(clip(fl32(fl32(o * scale) + offset), 0, peak)): the narrowed scaled calls' documented arithmetic (a NaN becomes 0)."""
    v = ((o * np.float32(scale)).astype(np.float32) + np.float32(offset)).astype(np.float32)
    return np.rint(np.clip(np.where(np.isnan(v), np.float32(0), v), 0, peak)).astype(np.uint32)


def planar_twin_results(pkg, fmt, geo, n, seed, m, offset):
    """The dense result planes of the un-matrixed planar call through the emulation: (source side, [o0, o1, o2] as float32 (n, h, w))."""
    sw, sh, tw, th = geo
    src = upload_planes(fmt, float_frames(fmt, sw, sh, n, 3, seed))
    images, lays = planar_side(fmt.sample_bytes, tw, th, n, 3)
    f0 = pkg.Filter(fmt, sw, sh, tw, th, device=0, tap=3)
    devs = [Dev(im) for im in images]
    ptrs, pitches, strides, _ = side_args(devs, lays)
    f0.process_device(src[1], src[2], src[3], ptrs, pitches, strides, n)
    _torch().cuda.synchronize()
    twin = [d.host() for d in devs]
    f0.close()
    want, o = matrixed(fmt, twin, lays, n, th, tw, m, offset)
    kind, dt = kind_of(fmt), raw_type(fmt)
    stored = [widen(np.ascontiguousarray(chan(want[l[0]], l, n, th, tw, dt)), kind) for l in lays]   # (what the narrowing pass reads)
    return src, stored


@pytest.mark.parametrize("name", ["YUV444PS", "YUV444PH"])
def test_narrowed_scaled_into_bgra8_and_planar_10_bit(gpu_pkg, bt709, name):
    """BGRA8 at destination step 4 with no alpha channel given (its bytes keep the sentinel), and planar 10-bit words with shift 6."""
    pkg, fmt, n, geo = gpu_pkg, gpu_pkg.FORMATS[name], 2, GEO_NARROW
    sw, sh, tw, th = geo
    src, o = planar_twin_results(pkg, fmt, geo, n, 31, bt709, OFFSET)
    f1 = pkg.Filter(fmt, sw, sh, tw, th, device=0, tap=3)
    f1.set_output_matrix(bt709, OFFSET)
    # BGRA8: planes R, G, B at channels 2, 1, 0 of a four-byte pixel; full range, to_code pair 255 / 0
    images, lays = interleaved_side(1, tw, th, n, 4, [2, 1, 0])
    devs = [Dev(im) for im in images]
    ptrs, pitches, strides, steps = side_args(devs, lays)
    f1.process_device_narrowed_scaled(src[1], src[2], None, src[3], ptrs, pitches, steps, None, 8, [255.0] * 3, [0.0] * 3, strides, n)
    assert pkg.last_matrix_launches() == pkg.last_strided()[2] == 1
    _torch().cuda.synchronize()
    want = [im.copy() for im in images]
    for c, l in enumerate(lays):
        chan(want[0], l, n, th, tw, np.uint8)[...] = narrow_codes(o[c], 255.0, 0.0, 255).astype(np.uint8)
    same_bytes([devs[0].host()], want, f"{name} into BGRA8")
    assert (chan(want[0], (0, 3) + lays[0][2:], n, th, tw, np.uint8) == SENTINEL).all()
    # planar 10-bit words, shift 6 (the P010 layout of a 4:4:4 surface), limited-range R'G'B' codes 64 + 876 v
    images, lays = planar_side(2, tw, th, n, 3)
    devs = [Dev(im) for im in images]
    ptrs, pitches, strides, _ = side_args(devs, lays)
    f1.process_device_narrowed_scaled(src[1], src[2], None, src[3], ptrs, pitches, None, [6, 6, 6], 10, [876.0] * 3, [64.0] * 3, strides, n)
    assert pkg.last_matrix_launches() == 1
    _torch().cuda.synchronize()
    want = [im.copy() for im in images]
    for c, l in enumerate(lays):
        chan(want[c], l, n, th, tw, np.uint16)[...] = (narrow_codes(o[c], 876.0, 64.0, 1023) << 6).astype(np.uint16)
    same_bytes([d.host() for d in devs], want, f"{name} into planar 10-bit")
    f1.close()


def test_narrowed_packed10(gpu_pkg, bt709):
    """fp32 planes into R10G10B10A2-style words: field i holds rint(clip(fl32(fl32(o_i * 1023) + 0), 0, 1023))."""
    pkg, fmt, n, geo = gpu_pkg, gpu_pkg.FORMATS["YUV444PS"], 2, GEO_NARROW
    sw, sh, tw, th = geo
    src, o = planar_twin_results(pkg, fmt, geo, n, 41, bt709, OFFSET)
    fields, fill = pkg.packed10_layout("Y410")
    images, lays = interleaved_side(4, tw, th, n, 1, [0])
    dev = Dev(images[0])
    f1 = pkg.Filter(fmt, sw, sh, tw, th, device=0, tap=3)
    f1.set_output_matrix(bt709, OFFSET)
    f1.process_device_narrowed_packed10(src[1], src[2], None, src[3], dev.ptr + lays[0][1], lays[0][3], fields, fill, [1023.0] * 3, None, lays[0][2], n)
    assert pkg.last_matrix_launches() == 1
    _torch().cuda.synchronize()
    mask = sum(1023 << f for f in fields)
    words = np.full((n, th, tw), fill & ~mask & 0xFFFFFFFF, np.uint32)
    for c in range(3):
        words |= narrow_codes(o[c], 1023.0, 0.0, 1023) << np.uint32(fields[c])
    want = images[0].copy()
    chan(want, lays[0], n, th, tw, np.uint32)[...] = words
    same_bytes([dev.host()], [want], "narrowed packed10")
    f1.close()


def test_y410_widened_packed10_scaled(gpu_pkg, bt709):
    """Limited-range Y410 words into an fp32 4:4:4 filter, R'G'B' planes out."""
    pkg, fmt, n, geo = gpu_pkg, gpu_pkg.FORMATS["YUV444PS"], 2, GEO_NARROW
    sw, sh, tw, th = geo
    rng = np.random.default_rng(51)
    fields, _ = pkg.packed10_layout("Y410")
    simg, slay = interleaved_side(4, sw, sh, n, 1, [0])
    words = np.zeros((n, sh, sw), np.uint32)
    for c in range(3):
        words |= rng.integers(64, 941, (n, sh, sw)).astype(np.uint32) << np.uint32(fields[c])
    chan(simg[0], slay[0], n, sh, sw, np.uint32)[...] = words
    sdev = Dev(simg[0])
    scale, off, _, _ = limited_pairs(pkg, 10)
    images, lays = planar_side(4, tw, th, n, 3)
    f0, f1 = twins(pkg, fmt, geo, bt709, OFFSET, tap=3)

    def call(f, devs):
        ptrs, pitches, strides, _ = side_args(devs, lays)
        f.process_device_widened_packed10_scaled(sdev.ptr + slay[0][1], slay[0][3], fields, scale, off, slay[0][2], ptrs, pitches, None, strides, n)
    twin, got, launches, strided = run_both(pkg, f0, f1, images, call)
    want, _ = matrixed(fmt, twin, lays, n, th, tw, bt709, OFFSET)
    same_bytes(got, want, "Y410 widened")
    assert launches == strided[2] == 1
    f0.close(), f1.close()


def test_integer_filters_are_refused_at_the_setter(gpu_pkg, bt709):
    """The v210 -> Y410 pairing runs on a 10-bit INTEGER filter: there is no matrix to set, with a device as without one."""
    sw, sh, tw, th = (48, 16, 96, 32)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YUV422P10"], sw, sh, tw, th, device=0, out_sub=(0, 0))
    with pytest.raises(gpu_pkg.JincError) as e:
        f.set_output_matrix(bt709, OFFSET)
    assert e.value.code == UNSUPPORTED and "integer samples" in str(e.value)
    f.close()


# ---- slices, the launch count, clearing -------------------------------------------------------------------------------------------------------

def test_slices_launch_counts_and_clearing(gpu_pkg, bt709):
    pkg, fmt, n = gpu_pkg, gpu_pkg.FORMATS["YUV420PS"], 5
    tw, th = GEO_NV12[2:]
    keep, sp, spitch, ssteps, sstrides = nv12_source(n, 61)
    scale, off, _, _ = limited_pairs(pkg)
    images, lays = interleaved_side(4, tw, th, n, 3, [0, 1, 2])
    f0, f1 = twins(pkg, fmt, GEO_NV12, bt709, OFFSET, out_sub=(0, 0), tap=3)

    def call(f, devs):
        ptrs, pitches, strides, steps = side_args(devs, lays)
        f.process_device_widened_scaled(sp, spitch, ssteps, None, 8, scale, off, sstrides, ptrs, pitches, steps, strides, n)
    twin, one_slice, launches, strided = run_both(pkg, f0, f1, images, call)
    assert launches == strided[2] == 1
    # stand-ins of a frame: 256-byte rows of 38 and twice 19 floats, three times 33 rows of 77 floats in 512 bytes: two frames a slice
    per_frame = 256 * 16 + 2 * 256 * 8 + 3 * 512 * 33
    with pkg.knobs(strided_scratch_bytes=2 * per_frame):
        _, sliced, launches, strided = run_both(pkg, f0, f1, images, call)
    assert strided[2] == 3 and launches == 3, (launches, strided)
    same_bytes(sliced, one_slice, "three slices against one")
    same_bytes(one_slice, matrixed(fmt, twin, lays, n, th, tw, bt709, OFFSET)[0], "one slice")
    # cleared: not a launch, not a report field, not a byte differs from a filter that never had a matrix
    f1.set_output_matrix(None)
    d0, d1 = [Dev(im) for im in images], [Dev(im) for im in images]
    call(f0, d0)
    never = (pkg.last_matrix_launches(), pkg.last_strided()[:3], pkg.last_groups())
    call(f1, d1)
    assert (pkg.last_matrix_launches(), pkg.last_strided()[:3], pkg.last_groups()) == never and never[0] == 0
    _torch().cuda.synchronize()
    same_bytes([d.host() for d in d1], [d.host() for d in d0], "cleared")
    assert keep
    f0.close(), f1.close()


def test_host_frame_entries_launch_nothing_with_a_matrix(gpu_pkg, bt709):
    pkg, fmt = gpu_pkg, gpu_pkg.FORMATS["YUV444PS"]
    sw, sh, tw, th = GEO_NARROW
    f = pkg.Filter(fmt, sw, sh, tw, th, device=0, tap=3)
    src = [np.ascontiguousarray(p[0]).view(np.float32) for p in float_frames(fmt, sw, sh, 1, 3, 71)]
    got = f.get_frame(src)                       # (a call of this process, so that last_call names one)
    before = pkg.last_call()
    f.set_output_matrix(bt709, OFFSET)
    outs = [pkg.alloc_plane(tw, th, np.float32) for _ in range(3)]
    for entry in (lambda: f.get_frame(src), lambda: f.submit(src, outs)):
        with pytest.raises(pkg.JincError) as e:
            entry()
        assert e.value.code == UNSUPPORTED and "output matrix" in str(e.value)
    assert pkg.last_call() == before and all((o == 0).all() for o in outs)
    f.set_output_matrix(None)
    again = f.get_frame(src)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, again))
    f.close()


def test_the_hook_runs_the_kernel_on_three_rows(gpu_pkg, bt709):
    """jinc_debug_matrix_rows: whole lanes and a tail, every kind, against the emulation."""
    rng = np.random.default_rng(81)
    for kind, n in ((0, 4 * 64 + 7), (HALF, 8 * 64 + 13), (BF16, 8 * 64 + 13)):
        v = [rng.random(n, dtype=np.float32) - np.float32(0.5 * (c > 0)) for c in range(3)]
        rows = [narrow(x, kind) for x in v]
        given = [r.view(np.float32) if kind == 0 else r.view(np.float16) if kind == HALF else r for r in rows]
        got = gpu_pkg.debug_matrix_rows(given, bt709, OFFSET, bfloat16=(kind == BF16))
        o = emulate(*[widen(r, kind) for r in rows], bt709, OFFSET)
        for c in range(3):
            assert np.array_equal(np.ascontiguousarray(got[c]).view(rows[c].dtype), narrow(o[c], kind)), (kind, c)


# ---- beyond 4 GiB -----------------------------------------------------------------------------------------------------------------------------
# An arena as tests/test_far_frames.py builds it (own copy of the helper).  The base handed to the library is arena + 2^31 + MARGIN and
# the arena ends at base + 2^32 + MARGIN + LARGEST: a signed 32-bit truncation of any offset lands in [base - 2^31, base + 2^31), an
# unsigned one in [base, base + 2^32), and a plane with its guards (at most MARGIN bytes from the base) behind such a wrong origin
# still ends inside the allocation.
#     INVARIANT: a latent addressing bug shows as wrong bytes or a disturbed guard, never as a memory fault.

G31, G32 = 1 << 31, 1 << 32
MARGIN = 4 << 20
LARGEST = 1 << 20
GUARD = 4096
ARENA_BYTES = G31 + MARGIN + G32 + MARGIN + LARGEST


def test_destination_frames_beyond_4_gib(gpu_pkg, bt709):
    """Planar call, 3 frames, the destination frame stride puts frame 1 beyond 2^31 and frame 2 beyond 2^32 (the source is dense)."""
    torch = _torch()
    free, _ = torch.cuda.mem_get_info()
    if free < ARENA_BYTES + (1 << 30):
        pytest.skip(f"the device has {free >> 20} MiB free, the arena needs {(ARENA_BYTES + (1 << 30)) >> 20} MiB")
    pkg, fmt, n, geo = gpu_pkg, gpu_pkg.FORMATS["YUV444PS"], 3, (64, 12, 128, 24)
    sw, sh, tw, th = geo
    src = upload_planes(fmt, float_frames(fmt, sw, sh, n, 3, 91))
    # the twin on dense planes
    images, lays = planar_side(4, tw, th, n, 3)
    f0, f1 = twins(pkg, fmt, geo, bt709, OFFSET, tap=3)
    devs = [Dev(im) for im in images]
    ptrs, pitches, strides, _ = side_args(devs, lays)
    f0.process_device(src[1], src[2], src[3], ptrs, pitches, strides, n)
    torch.cuda.synchronize()
    _, o = matrixed(fmt, [d.host() for d in devs], lays, n, th, tw, bt709, OFFSET)
    # the matrixed call into the arena
    pitch, row_bytes = 512 + 16, tw * 4
    plane = pitch * (th - 1) + row_bytes
    stride = align(-(-(G32 + MARGIN) // (n - 1)), 16)   # ceil((2^32 + MARGIN) / (n - 1)), as test_far_frames.py's far_stride
    first = [GUARD + c * (256 << 10) for c in range(3)]
    offs = [[first[c] + k * stride for k in range(n)] for c in range(3)]
    bo, hi = G31 + MARGIN, ARENA_BYTES - (G31 + MARGIN)
    for c in range(3):   # the invariant, for every plane of every frame
        assert plane + 2 * GUARD <= (256 << 10) and first[c] + plane + GUARD <= MARGIN and 2 * pitch <= GUARD
        assert all(0 <= x - GUARD and x + plane + GUARD <= hi for x in offs[c]) and offs[c][1] >= G31 and offs[c][2] >= G32
        assert -bo <= -G31 - GUARD and G32 + first[c] + plane + GUARD <= hi
    arena = torch.empty(ARENA_BYTES, dtype=torch.uint8, device="cuda")
    try:
        for c in range(3):
            for x in offs[c]:
                arena[bo + x - GUARD:bo + x + plane + GUARD].fill_(SENTINEL)
        base = arena.data_ptr() + bo
        f1.process_device(src[1], src[2], src[3], [base + first[c] for c in range(3)], [pitch] * 3, [stride] * 3, n)
        assert pkg.last_matrix_launches() == 1
        torch.cuda.synchronize()
        for c in range(3):
            for k, x in enumerate(offs[c]):
                raw = to_host(arena[bo + x - GUARD:bo + x + plane + GUARD]).numpy()
                want = np.full(raw.shape, SENTINEL, np.uint8)
                np.ndarray((th, tw), np.uint32, want, GUARD, (pitch, 4))[...] = o[c][k].view(np.uint32)
                bad = np.flatnonzero(raw != want)
                assert bad.size == 0, f"plane {c} frame {k} (destination offset {x:#x}): {bad.size} bytes differ, first at {int(bad[0]) - GUARD}"
    finally:
        del arena
        torch.cuda.empty_cache()
        f0.close(), f1.close()
