"""jinc_filter_process_device_shifted on the device: 16-bit words that keep their sample in the HIGH bits (P010 / P012 / Y210 as
hardware decoders write them).  The value of a source sample is raw >> shift, a result is stored as value << shift.  Every case is
bit-exact against the CPU oracle run on the shifted-down values AND against jinc_filter_process_device on dense planes of those
values; the destination's padding bits must be zero; no byte outside the given planes' samples may change (guard bytes, as in
test_strided.py, whose helpers and shapes this file uses); the sources carry pseudo-random padding bits, so a pass that forgets to
discard them fails."""
import numpy as np
import pytest

from test_strided import INVALID_ARG, SEMI, Side, assert_frames, frames_and_wants, planar, run_planar, semi_planar

pytestmark = pytest.mark.gpu

Y210 = [(0, 0, 2), (0, 1, 4), (0, 3, 4)]   # Y0 U Y1 V in one buffer: Y at step 2, U and V at step 4


class SharedRowSide(Side):
    """Side for planes of DIFFERENT widths and steps in one buffer whose rows have the same bytes (Y210: w samples at step 2, w / 2
    at step 4): the buffer is laid out from the first plane, the others find their samples in it."""

    def __init__(self, torch, dims, dtype, layout, n, *args, **kw):
        assert len({b for b, _, _ in layout}) == 1 and len({w * step for (w, h), (b, c, step) in zip(dims, layout)}) == 1
        Side.__init__(self, torch, dims[:1], dtype, layout[:1], n, *args, **kw)
        self.dims, self.layout = dims, layout


def side_for(layout):
    return SharedRowSide if layout == Y210 else Side


def raw_frames(frames, shifts, seed):
    """value << shift with pseudo-random padding bits below."""
    rng = np.random.default_rng(seed)
    return [[(np.asarray(p, np.uint16) << np.uint16(s)) | rng.integers(0, 1 << s, np.asarray(p).shape, dtype=np.uint16)
             for p, s in zip(planes, shifts)] for planes in frames]


def values_of(got, shifts, what):
    """The destination's planes shifted down, after asserting that their padding bits are zero."""
    out = []
    for k, planes in enumerate(got):
        row = []
        for i, (p, s) in enumerate(zip(planes, shifts)):
            dirty = int(np.count_nonzero(p & np.uint16((1 << s) - 1)))
            assert dirty == 0, f"{what}: frame {k} plane {i}: {dirty} samples with non-zero padding bits"
            row.append(p >> np.uint16(s))
        out.append(row)
    return out


def call(f, src, dst, src_shifts, dst_shifts, n, stream, steps=True):
    f.process_device_shifted(src.ptrs(), src.pitches(), src.steps() if steps else None, src_shifts, src.strides(),
                             dst.ptrs(), dst.pitches(), dst.steps() if steps else None, dst_shifts, dst.strides(), n, stream=stream.cuda_stream)


def make_sides(torch, f, frames, src_layout, dst_layout, src_shifts, n, src_align=16, dst_align=16, seeds=(11, 12), **side_kw):
    fmt = f.fmt
    src = side_for(src_layout)(torch, fmt.plane_dims(f.src_w, f.src_h), fmt.dtype, src_layout, n, src_align, seed=seeds[0],
                               **{k[4:]: v for k, v in side_kw.items() if k.startswith("src_")})
    src.fill(raw_frames(frames, src_shifts or [0] * fmt.planes, seeds[0] + 100)).upload()
    dst = side_for(dst_layout)(torch, f.out_dims(), fmt.dtype, dst_layout, n, dst_align, seed=seeds[1],
                               **{k[4:]: v for k, v in side_kw.items() if k.startswith("dst_")}).upload()
    return src, dst


_PLANAR = {}


def planar_results(torch, f, key, frames, n):
    """jinc_filter_process_device on dense planes of the values: once per geometry and frame count."""
    if key + (n,) not in _PLANAR:
        _PLANAR[key + (n,)] = run_planar(torch, f, frames, n)
    return _PLANAR[key + (n,)]


def check_call(torch, O, pkg, name, geom, n, src_layout, dst_layout, src_shifts, dst_shifts, expect_report=None, **run_kw):
    sw, sh, tw, th = geom
    kw = dict(tap=3)
    frames, wants = frames_and_wants(O, pkg, name, sw, sh, tw, th, kw, n)
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=0, **kw)
    what = f"{name} {sw}x{sh}->{tw}x{th} {n} frame(s) shifts {src_shifts} -> {dst_shifts}"
    src, dst = make_sides(torch, f, frames, src_layout, dst_layout, src_shifts, n, **run_kw)
    s = torch.cuda.current_stream()
    call(f, src, dst, src_shifts, dst_shifts, n, s)
    s.synchronize()
    report = f.last_strided()
    print(f"{what}: last_strided {report}")
    got = values_of(dst.frames_and_guards(what), dst_shifts or [0] * f.fmt.planes, what)
    if expect_report is not None:
        assert report[:3] == expect_report, report
    assert_frames(f.fmt, got, wants, f.out_dims(), what + " against the oracle")
    assert_frames(f.fmt, got, planar_results(torch, f, (name,) + tuple(geom), frames, n), f.out_dims(), what + " against the planar call")
    f.close()


# ---- 1. P010 / P012 as decoders write them -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name,shift", [("YUV420P10", 6), ("YUV420P12", 4)], ids=["P010", "P012"])
def test_real_p010_in_and_out(gpu_pkg, O, name, shift, n):
    """Luma step 1, chroma step 2, all shifted: the luma row of 150 samples and the chroma row of 75 x 2 are both 300 bytes, whole
    16-byte vectors and a tail.  One launch per direction and step: luma (N = 1) and chroma (N = 2)."""
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, name, SEMI, n, semi_planar(), semi_planar(), [shift] * 3, [shift] * 3, expect_report=(2, 2, 1))


# ---- 2. Y210 -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3])
def test_y210_packed_422(gpu_pkg, O, n):
    """Y0 U Y1 V in one buffer: Y at step 2 (a group of one of two channels), U and V at step 4 (two of four), all shifted by 6."""
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, "YUV422P10", SEMI, n, Y210, Y210, [6] * 3, [6] * 3, expect_report=(2, 2, 1))


# ---- 3. one dense plane: the N = 1 form alone ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3])
def test_single_shifted_plane(gpu_pkg, O, n):
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, "Y10", SEMI, n, planar(1), planar(1), [6], [6], expect_report=(1, 1, 1))


# ---- 4. one side only, and unshifted planes beside shifted ones ----------------------------------------------------------------------

def test_p010_in_planar_low_aligned_out_and_the_reverse(gpu_pkg, O):
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, "YUV420P10", SEMI, 3, semi_planar(), planar(3), [6] * 3, None, expect_report=(2, 0, 1))
    check_call(torch, O, gpu_pkg, "YUV420P10", SEMI, 3, planar(3), semi_planar(), [0] * 3, [6] * 3, expect_report=(0, 2, 1))


@pytest.mark.parametrize("shifts", [[6, 0, 0], [0, 6, 6], [6, 6, 0], [0, 0, 6]], ids=lambda s: "".join(map(str, s)))
def test_planes_with_a_step_and_no_shift_beside_shifted_ones(gpu_pkg, O, shifts):
    """Chroma at step 2 with shift 0 next to a shifted luma (the chroma launch is the unshifted one); luma where it lies next to
    shifted chroma; U and V of one pixel with different shifts share a launch."""
    torch = pytest.importorskip("torch")
    launches = 2 if shifts[0] else 1
    check_call(torch, O, gpu_pkg, "YUV420P10", SEMI, 2, semi_planar(), semi_planar(), shifts, shifts, expect_report=(launches, launches, 1))


# ---- 5. alignment classes ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("align", [4, 1])
def test_other_alignment_classes(gpu_pkg, O, align):
    """Bases and pitches that are multiples of 4 but not of 16 (dword accesses), and of the sample size only, for the N = 1 form
    (luma) and the N = 2 form (chroma) of one call."""
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, "YUV420P10", SEMI, 3, semi_planar(), semi_planar(), [6] * 3, [6] * 3, expect_report=(2, 2, 1),
               src_align=align, dst_align=align)


@pytest.mark.parametrize("align", [16, 4, 1])
def test_incomplete_group_v_without_u(gpu_pkg, O, align):
    """One plane at the V position of a UV buffer, U not given: the split reads only that channel into the filter, the merge stores
    sample by sample and the U words between are guard bytes."""
    torch = pytest.importorskip("torch")
    lone_v = [(0, 1, 2)]
    lead = {16: {0: 62}, 4: {0: 66}}.get(align)   # V itself on a 16- / 4-byte boundary, so that the split takes its class's accesses
    check_call(torch, O, gpu_pkg, "Y10", SEMI, 2, lone_v, lone_v, [6], [6], expect_report=(1, 1, 1), src_align=align, dst_align=align,
               src_lead=lead, dst_lead=lead)


# ---- 6. another geometry ---------------------------------------------------------------------------------------------------------------

def test_non_2x_geometry(gpu_pkg, O):
    """150 x 100 -> 205 x 137: whatever arithmetic kernels the rules choose run behind the stand-ins."""
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, "YUV420P10", (150, 100, 205, 137), 2, semi_planar(), semi_planar(), [6] * 3, [6] * 3, expect_report=(2, 2, 1))


# ---- 7. slices -------------------------------------------------------------------------------------------------------------------------

def test_a_shifted_call_beyond_the_scratch_cap_runs_in_slices(gpu_pkg, O):
    """strided_scratch_bytes = three frames' dense planes, luma included (rows padded to 256 bytes): 7 frames run as 3 + 3 + 1, each
    slice with a luma and a chroma launch in each direction."""
    torch = pytest.importorskip("torch")
    per_frame = (512 * 100 + 2 * 256 * 50) + (768 * 200 + 2 * 512 * 100)
    with gpu_pkg.knobs(strided_scratch_bytes=3 * per_frame):
        check_call(torch, O, gpu_pkg, "YUV420P10", SEMI, 7, semi_planar(), semi_planar(), [6] * 3, [6] * 3, expect_report=(6, 6, 3))


# ---- 8. two streams --------------------------------------------------------------------------------------------------------------------

def test_two_shifted_calls_back_to_back_on_two_streams(gpu_pkg, O):
    """One filter, two calls on different frames queued without a synchronise in between on two streams: they share the dense planes,
    luma included, so the second call's split waits for the first call's merge."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = SEMI
    frames, wants = frames_and_wants(O, gpu_pkg, "YUV420P10", sw, sh, tw, th, dict(tap=3), 6)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YUV420P10"], sw, sh, tw, th, device=0, tap=3)
    sides = [make_sides(torch, f, frames[3 * c:3 * c + 3], semi_planar(), semi_planar(), [6] * 3, 3, seeds=(21 + c, 31 + c)) for c in range(2)]
    torch.cuda.synchronize()   # (the uploads are done before the side streams start)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for c, (src, dst) in enumerate(sides):
        call(f, src, dst, [6] * 3, [6] * 3, 3, streams[c])
    torch.cuda.synchronize()
    for c, (src, dst) in enumerate(sides):
        got = values_of(dst.frames_and_guards(f"call {c}"), [6] * 3, f"call {c}")
        assert_frames(f.fmt, got, wants[3 * c:3 * c + 3], f.out_dims(), f"call {c} of two streams")
    f.close()


# ---- 9. equivalence --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("zeros", [None, [0, 0, 0]], ids=["NULL", "zeros"])
def test_with_every_shift_zero_the_call_is_the_strided_call(gpu_pkg, O, zeros):
    """The same samples and the same report as process_device_strided on the same planes; with every step 1 as well, the planar
    call's last_call."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = SEMI
    n = 3
    frames, wants = frames_and_wants(O, gpu_pkg, "YUV420P10", sw, sh, tw, th, dict(tap=3), n)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YUV420P10"], sw, sh, tw, th, device=0, tap=3)
    s = torch.cuda.current_stream()
    src, dst = make_sides(torch, f, frames, semi_planar(), semi_planar(), None, n)
    f.process_device_strided(src.ptrs(), src.pitches(), src.steps(), src.strides(), dst.ptrs(), dst.pitches(), dst.steps(), dst.strides(), n, stream=s.cuda_stream)
    s.synchronize()
    strided_report, strided_call = f.last_strided(), gpu_pkg.last_call()
    strided = dst.frames_and_guards("strided call")
    src, dst = make_sides(torch, f, frames, semi_planar(), semi_planar(), None, n)
    call(f, src, dst, zeros, zeros, n, s)
    s.synchronize()
    assert f.last_strided() == strided_report and strided_report[:3] == (1, 1, 1) and gpu_pkg.last_call() == strided_call
    got = dst.frames_and_guards("shifted call, shifts 0")
    assert_frames(f.fmt, got, strided, f.out_dims(), "shifts 0 against the strided call")
    assert_frames(f.fmt, got, wants, f.out_dims(), "shifts 0 against the oracle")
    # every step 1 too: jinc_filter_process_device
    run_planar(torch, f, frames, n)
    planar_call = gpu_pkg.last_call()
    for steps in (True, False):
        src, dst = make_sides(torch, f, frames, planar(3), planar(3), None, n)
        call(f, src, dst, zeros, zeros, n, s, steps=steps)
        s.synchronize()
        assert f.last_strided()[:3] == (0, 0, 0) and gpu_pkg.last_call() == planar_call and planar_call[1] == n
        assert_frames(f.fmt, dst.frames_and_guards("all steps 1, shifts 0"), wants, f.out_dims(), "all steps 1, shifts 0")
    f.close()


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------------

REFUSED = [("YUV420P8", 6), ("YUV420P16", 6), ("YUV420PS", 6), ("YUV420PH", 6), ("YUV420P10", 7), ("YUV420P10", -1)]


@pytest.mark.parametrize("name,shift", REFUSED, ids=[f"{n}_shift{s}" for n, s in REFUSED])
def test_refused_shifts_write_nothing(gpu_pkg, name, shift):
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = SEMI
    f = gpu_pkg.Filter(gpu_pkg.FORMATS[name], sw, sh, tw, th, device=0, tap=3)
    fmt = f.fmt
    src = Side(torch, fmt.plane_dims(sw, sh), fmt.dtype, semi_planar(), 1, seed=41).upload()
    dst = Side(torch, f.out_dims(), fmt.dtype, semi_planar(), 1, seed=42).upload()
    s = torch.cuda.current_stream()
    messages = []
    for src_shifts, dst_shifts in (([shift] * 3, [shift] * 3), ([shift, 0, 0], None), (None, [0, 0, shift])):
        with pytest.raises(gpu_pkg.JincError) as e:
            call(f, src, dst, src_shifts, dst_shifts, 1, s)
        assert e.value.code == INVALID_ARG and str(e.value).startswith("JincResize:") and "shift" in str(e.value), str(e.value)
        messages.append(str(e.value))
    print(name, shift, messages[0])
    s.synchronize()
    image = dst.download()
    for b, B in dst.bufs.items():
        assert np.array_equal(image[b], B["host"]), "a refused call wrote to the destination"
    f.close()
