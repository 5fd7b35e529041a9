"""jinc_filter_process_device_strided on the device: semi-planar (NV12 / P010 / P016 style) and packed RGB(A) frames in, the same or
another layout out.  Every frame is checked against the CPU oracle AND against jinc_filter_process_device on the same samples;
every destination lies inside a larger buffer of pseudo-random bytes, and every byte that is not a sample of a plane given to the
call must keep its value (bytes in front of the base, row padding, the gap between frames, bytes behind the last row, channels that
were not given).  Shapes are the smallest at which the split / merge passes can go wrong: rows with a vector tail, bases and pitches
of every alignment class (16, 4, less), more than one row block, several frames."""
import numpy as np
import pytest

from conftest import assert_planes_equal, oracle_kwargs, to_device, to_host
from test_half_planes import assert_half_equal, definition, unit_frame

pytestmark = pytest.mark.gpu

INVALID_ARG = -1


# ---- layouts -------------------------------------------------------------------------------------------------------------------------
# A layout names, per plane (library order Y,U,V,A / G,B,R,A): (buffer, channel inside the pixel, samples per pixel).

def planar(nplanes):
    return [(i, 0, 1) for i in range(nplanes)]


def semi_planar(nplanes=3):
    """Y dense, U and V interleaved in one buffer (NV12, P010, P016; NV16 for 4:2:2)."""
    return [(0, 0, 1), (1, 0, 2), (1, 1, 2)][:nplanes]


def packed(order, step, nplanes):
    """order: the pixel's channels as letters, e.g. "BGRA"; planes G, B, R(, A) find their letter."""
    return [(0, order.index(c), step) for c in "GBRA"[:nplanes]]


class Side:
    """The planes of `n` frames on one side of a call: host image, device copy, pointers."""

    def __init__(self, torch, dims, dtype, layout, n, align=16, seed=1, lead=None, pitches=None):
        self.dims, self.dtype, self.layout, self.n = dims, np.dtype(dtype), layout, n
        sb = self.sb = self.dtype.itemsize
        rng = np.random.default_rng(seed)
        self.bufs = {}
        for i, (b, chan, step) in enumerate(layout):
            if b in self.bufs:
                assert self.bufs[b]["dims"] == dims[i] and self.bufs[b]["step"] == step
                continue
            w, h = dims[i]
            row = w * step * sb
            if align == 16:
                ld, pitch, gap = 64, (row + 15) // 16 * 16 + 16, 32
            elif align == 4:
                ld, pitch, gap = 68, (row + 15) // 16 * 16 + 4, 4
            else:   # no better than the sample size
                ld, pitch, gap = 64 + 2 * max(sb // 2, 1), (row + 3) // 4 * 4 + (1 if sb == 1 else 2 if sb == 2 else 4), sb
            if lead is not None and b in lead:
                ld = lead[b]
            if pitches is not None and b in pitches:
                pitch = pitches[b]
            fs = pitch * h + gap
            host = rng.integers(0, 256, ld + n * fs + 256, dtype=np.uint8)
            self.bufs[b] = dict(dims=dims[i], step=step, lead=ld, pitch=pitch, fs=fs, host=host, dev=None)
        self.torch = torch

    def view(self, image, i, k):
        b, chan, step = self.layout[i]
        B = self.bufs[b]
        w, h = self.dims[i]
        return np.ndarray((h, w), self.dtype, image[b], B["lead"] + k * B["fs"] + chan * self.sb, (B["pitch"], step * self.sb))

    def fill(self, frames):
        image = {b: B["host"] for b, B in self.bufs.items()}
        for k in range(self.n):
            for i, (w, h) in enumerate(self.dims):
                self.view(image, i, k)[...] = frames[k][i][:h, :w]
        return self

    def upload(self):
        for B in self.bufs.values():
            B["dev"] = to_device(self.torch.from_numpy(B["host"]))
        return self

    def ptrs(self):
        return [self.bufs[b]["dev"].data_ptr() + self.bufs[b]["lead"] + chan * self.sb for (b, chan, step) in self.layout]

    def pitches(self):
        return [self.bufs[b]["pitch"] for (b, chan, step) in self.layout]

    def steps(self):
        return [step for (b, chan, step) in self.layout]

    def strides(self):
        return [self.bufs[b]["fs"] for (b, chan, step) in self.layout]

    def download(self):
        return {b: to_host(B["dev"]).numpy() for b, B in self.bufs.items()}

    def frames_and_guards(self, what=""):
        """The planes of every frame, after asserting that no byte outside the given planes' samples has changed."""
        image = self.download()
        got = [[np.ascontiguousarray(self.view(image, i, k)) for i in range(len(self.dims))] for k in range(self.n)]
        for b, B in self.bufs.items():
            untouched = np.ones(B["host"].size, bool)
            mask_image = {b: untouched}
            for i, (bb, chan, step) in enumerate(self.layout):
                if bb != b:
                    continue
                for k in range(self.n):
                    for byte in range(self.sb):   # the sample's bytes
                        w, h = self.dims[i]
                        np.ndarray((h, w), np.bool_, mask_image[b], B["lead"] + k * B["fs"] + chan * self.sb + byte, (B["pitch"], step * self.sb))[...] = False
            changed = np.flatnonzero(untouched & (image[b] != B["host"]))
            assert changed.size == 0, f"{what}: {changed.size} guard bytes of buffer {b} were written, first at byte {int(changed[0])} " \
                                      f"(lead {B['lead']}, pitch {B['pitch']}, frame stride {B['fs']})"
        return got


def run(torch, f, frames, src_layout, dst_layout, n, src_align=16, dst_align=16, stream=None, null_steps=False, what="", **side_kw):
    """frames[:n] through process_device_strided; returns the destination's planes per frame (guard bytes checked)."""
    fmt = f.fmt
    src = Side(torch, fmt.plane_dims(f.src_w, f.src_h), fmt.dtype, src_layout, n, src_align, seed=11, **{k[4:]: v for k, v in side_kw.items() if k.startswith("src_")}).fill(frames).upload()
    dst = Side(torch, f.out_dims(), fmt.dtype, dst_layout, n, dst_align, seed=12, **{k[4:]: v for k, v in side_kw.items() if k.startswith("dst_")}).upload()
    s = stream if stream is not None else torch.cuda.current_stream()
    f.process_device_strided(src.ptrs(), src.pitches(), None if null_steps else src.steps(), src.strides(),
                             dst.ptrs(), dst.pitches(), None if null_steps else dst.steps(), dst.strides(), n, stream=s.cuda_stream)
    s.synchronize()
    return dst.frames_and_guards(what)


def run_planar(torch, f, frames, n):
    """The same frames through jinc_filter_process_device (dense planes)."""
    fmt = f.fmt
    src = Side(torch, fmt.plane_dims(f.src_w, f.src_h), fmt.dtype, planar(fmt.planes), n, seed=13).fill(frames).upload()
    dst = Side(torch, f.out_dims(), fmt.dtype, planar(fmt.planes), n, seed=14).upload()
    s = torch.cuda.current_stream()
    f.process_device(src.ptrs(), src.pitches(), src.strides(), dst.ptrs(), dst.pitches(), dst.strides(), n, stream=s.cuda_stream)
    s.synchronize()
    return dst.frames_and_guards("planar call")


# ---- frames and expectations, computed once per geometry -------------------------------------------------------------------------------

_CACHE = {}


def frames_and_wants(O, pkg, name, sw, sh, tw, th, kw, n):
    key = (name, sw, sh, tw, th, tuple(sorted(kw.items())))
    have = _CACHE.setdefault(key, ([], []))
    fmt = pkg.FORMATS[name]
    while len(have[0]) < n:
        k = len(have[0])
        if fmt.half:
            src = unit_frame(O, name, sw, sh, 100 + k)
            want = definition(O, name, sw, sh, tw, th, kw, src)
        else:
            src = O.lcg_frame(O.FORMATS[name], sw, sh, 100 + k)
            want = O.OracleFilter(O.FORMATS[name], sw, sh, tw, th, **oracle_kwargs(kw)).get_frame(src, threads=8)
        have[0].append(src)
        have[1].append(want)
    return have[0][:n], have[1][:n]


def assert_frames(fmt, got, want, dims, what):
    for k in range(len(want)):
        if fmt.half:
            assert_half_equal(got[k], want[k], dims, what=f"{what} frame {k}")
        else:
            assert_planes_equal(got[k], want[k], dims, what=f"{what} frame {k}")


def check_call(torch, O, pkg, name, geom, kw, n, src_layout, dst_layout, expect_report=None, **run_kw):
    sw, sh, tw, th = geom
    frames, wants = frames_and_wants(O, pkg, name, sw, sh, tw, th, kw, n)
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=0, **kw)
    what = f"{name} {sw}x{sh}->{tw}x{th} {n} frame(s)"
    got = run(torch, f, frames, src_layout, dst_layout, n, what=what, **run_kw)
    report = f.last_strided()
    print(f"{what}: last_strided {report}")
    if expect_report is not None:
        assert report[:3] == expect_report, report
    assert_frames(f.fmt, got, wants, f.out_dims(), what + " against the oracle")
    assert_frames(f.fmt, got, run_planar(torch, f, frames, n), f.out_dims(), what + " against the planar call")
    f.close()


# ---- 1. semi-planar ----------------------------------------------------------------------------------------------------------------

SEMI = (150, 100, 300, 200)


@pytest.mark.parametrize("n", [1, 3, 7])
@pytest.mark.parametrize("name", ["YUV420P8", "YUV420P10", "YUV420P16", "YUV422P8"])
def test_semi_planar_in_and_out(gpu_pkg, O, name, n):
    """NV12 / P010 / P016 / NV16: the chroma row of 75 pixels x 2 channels is 150 bytes (8-bit) or 300 (16-bit) -- whole 16-byte
    vectors and a tail; 50 .. 200 rows are several row blocks; one group of two planes on each side, so one split and one merge."""
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, name, SEMI, dict(tap=3), n, semi_planar(), semi_planar(), expect_report=(1, 1, 1))


@pytest.mark.parametrize("n", [1, 3])
def test_semi_planar_unaligned_takes_the_sample_sized_accesses(gpu_pkg, O, n):
    """The UV base 2 bytes behind a 16-byte boundary and odd pitches (153 in, 303 out): no 4-byte access is possible."""
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, "YUV420P8", SEMI, dict(tap=3), n, semi_planar(), semi_planar(), expect_report=(1, 1, 1),
               src_lead={1: 66}, src_pitches={1: 153}, dst_lead={1: 66}, dst_pitches={1: 303})


@pytest.mark.parametrize("align", [4, 1])
@pytest.mark.parametrize("name", ["YUV420P8", "YUV420P16"])
def test_semi_planar_other_alignment_classes(gpu_pkg, O, name, align):
    """Base and pitch multiples of 4 but not of 16 (dword accesses); multiples of the sample size only."""
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, name, SEMI, dict(tap=3), 3, semi_planar(), semi_planar(), expect_report=(1, 1, 1), src_align=align, dst_align=align)


# ---- 2. packed ----------------------------------------------------------------------------------------------------------------------

PACKED = [("RGBP8", 3), ("RGBP8", 4), ("RGBAP8", 4), ("RGBP16", 3), ("RGBP16", 4), ("RGBAPS", 4), ("RGBPH", 4)]


@pytest.mark.parametrize("tw", [61, 62, 63, 64])
@pytest.mark.parametrize("other_order", [False, True], ids=["BGR", "other"])
@pytest.mark.parametrize("name,step", PACKED, ids=[f"{n}_step{s}" for n, s in PACKED])
def test_packed_in_and_out(gpu_pkg, O, name, step, other_order, tw):
    """40 x 24 -> 61 .. 64 x 37 (a plan without periods; the destination row's bytes have every residue).  BGR(A) and one other
    channel order: RGB at step 3, ARGB at step 4 -- with three components that leaves channel 0 (X) out, the group's lowest base is
    then R.  Three components at step 4 are an incomplete group: its X bytes are guard bytes."""
    torch = pytest.importorskip("torch")
    planes = gpu_pkg.FORMATS[name].planes
    order = {3: ("BGR", "RGB"), 4: ("BGRA", "ARGB")}[step][int(other_order)]
    layout = packed(order, step, planes)
    check_call(torch, O, gpu_pkg, name, (40, 24, tw, 37), dict(tap=3), 2, layout, layout, expect_report=(1, 1, 1))


@pytest.mark.parametrize("align", [4, 1])
@pytest.mark.parametrize("name,step", [("RGBP8", 3), ("RGBP16", 3), ("RGBAP8", 4), ("RGBP16", 4)])
def test_packed_other_alignment_classes(gpu_pkg, O, name, step, align):
    torch = pytest.importorskip("torch")
    layout = packed("BGRA"[:step] if step == 4 else "BGR", step, gpu_pkg.FORMATS[name].planes)
    check_call(torch, O, gpu_pkg, name, (40, 24, 63, 37), dict(tap=3), 2, layout, layout, expect_report=(1, 1, 1), src_align=align, dst_align=align)


# ---- 3. mixed ------------------------------------------------------------------------------------------------------------------------

def test_nv12_in_planar_out(gpu_pkg, O):
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, "YUV420P8", SEMI, dict(tap=3), 3, semi_planar(), planar(3), expect_report=(1, 0, 1))


def test_planar_in_nv12_out(gpu_pkg, O):
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, "YUV420P8", SEMI, dict(tap=3), 3, planar(3), semi_planar(), expect_report=(0, 1, 1))


def test_rgb24_in_bgra_out(gpu_pkg, O):
    """Step 3 in, step 4 out (X untouched); and a lone strided plane: G of a four-channel pixel in, R of a three-channel one out."""
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, "RGBP8", (40, 24, 63, 37), dict(tap=3), 2, packed("RGB", 3, 3), packed("BGRA", 4, 3), expect_report=(1, 1, 1))
    check_call(torch, O, gpu_pkg, "Y8", (40, 24, 63, 37), dict(tap=3), 2, [(0, 1, 4)], [(0, 2, 3)], expect_report=(1, 1, 1))


# ---- 5. one pass ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 5])
def test_one_launch_per_direction_whatever_the_frame_count(gpu_pkg, O, n):
    """NV12 (one group of two planes per side) and BGRA (one group of four): exactly one split and one merge launch per slice.  With
    every step 1 -- given as ones or as NULL arrays -- the call is jinc_filter_process_device: no launch, the same last_call."""
    torch = pytest.importorskip("torch")
    check_call(torch, O, gpu_pkg, "YUV420P8", SEMI, dict(tap=3), n, semi_planar(), semi_planar(), expect_report=(1, 1, 1))
    check_call(torch, O, gpu_pkg, "RGBAP8", (40, 24, 63, 37), dict(tap=3), n, packed("BGRA", 4, 4), packed("BGRA", 4, 4), expect_report=(1, 1, 1))
    sw, sh, tw, th = SEMI
    frames, wants = frames_and_wants(O, gpu_pkg, "YUV420P8", sw, sh, tw, th, dict(tap=3), n)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YUV420P8"], sw, sh, tw, th, device=0, tap=3)
    run_planar(torch, f, frames, n)
    planar_call = gpu_pkg.last_call()
    for null_steps in (False, True):
        got = run(torch, f, frames, planar(3), planar(3), n, null_steps=null_steps)
        assert f.last_strided()[:3] == (0, 0, 0) and gpu_pkg.last_call() == planar_call and planar_call[1] == n
        assert_frames(f.fmt, got, wants, f.out_dims(), f"all steps 1 (NULL arrays: {null_steps})")
    f.close()


# ---- 6. slices -----------------------------------------------------------------------------------------------------------------------

def test_a_call_beyond_the_scratch_cap_runs_in_slices(gpu_pkg, O):
    """strided_scratch_bytes = three frames' dense planes: 7 frames run as 3 + 3 + 1."""
    torch = pytest.importorskip("torch")
    per_frame = 2 * (256 * 50) + 2 * (256 * 100)   # chroma rows of 75 / 150 bytes padded to 256, source + result, U + V
    with gpu_pkg.knobs(strided_scratch_bytes=3 * per_frame):
        check_call(torch, O, gpu_pkg, "YUV420P8", SEMI, dict(tap=3), 7, semi_planar(), semi_planar(), expect_report=(3, 3, 3))


# ---- 7. two streams ------------------------------------------------------------------------------------------------------------------

def test_two_calls_back_to_back_on_two_streams(gpu_pkg, O):
    """One filter, two strided calls on different frames, queued without a synchronise in between on two streams: the second call's
    split must wait for the first call's merge (they share the dense planes)."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = SEMI
    frames, wants = frames_and_wants(O, gpu_pkg, "YUV420P8", sw, sh, tw, th, dict(tap=3), 6)
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YUV420P8"], sw, sh, tw, th, device=0, tap=3)
    fmt = f.fmt
    sides = []
    for c in range(2):
        src = Side(torch, fmt.plane_dims(sw, sh), fmt.dtype, semi_planar(), 3, seed=21 + c).fill(frames[3 * c:3 * c + 3]).upload()
        dst = Side(torch, f.out_dims(), fmt.dtype, semi_planar(), 3, seed=31 + c).upload()
        sides.append((src, dst))
    torch.cuda.synchronize()   # (the uploads are done before the side streams start)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for c, (src, dst) in enumerate(sides):
        f.process_device_strided(src.ptrs(), src.pitches(), src.steps(), src.strides(), dst.ptrs(), dst.pitches(), dst.steps(), dst.strides(), 3,
                                 stream=streams[c].cuda_stream)
    torch.cuda.synchronize()
    for c, (src, dst) in enumerate(sides):
        assert_frames(fmt, dst.frames_and_guards(f"call {c}"), wants[3 * c:3 * c + 3], f.out_dims(), f"call {c} of two streams")
    f.close()


# ---- 8. non-finite float samples ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tap", [3, 4])
def test_non_finite_samples_in_one_channel_of_packed_float(gpu_pkg, O, tap):
    """RGBA float at step 4, 2x, on the trimmed support (float_trim_min_taps = 0): one NaN and one infinity in the B channel of frame
    1 of 3.  The finite scan and the flagged second launch see the dense planes: exactly plane B (index 1) of frame 1 is flagged, and
    every sample equals the planar call's and the oracle's as a bit pattern."""
    torch = pytest.importorskip("torch")
    sw, sh = 150, 70
    rng = np.random.default_rng(5 + tap)
    frames = [[(rng.standard_normal((sh, sw)) * 0.5).astype(np.float32) for _ in range(4)] for _ in range(3)]
    frames[1][1][sh // 2, sw // 2] = np.float32(np.nan)
    frames[1][1][7, sw - 3] = np.float32(np.inf)
    wants = [O.OracleFilter(O.FORMATS["RGBAPS"], sw, sh, 2 * sw, 2 * sh, tap=tap).get_frame(s, threads=8) for s in frames]
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["RGBAPS"], sw, sh, 2 * sw, 2 * sh, device=0, tap=tap)
    layout = packed("BGRA", 4, 4)
    with gpu_pkg.knobs(float_trim_min_taps=0):
        got = run(torch, f, frames, layout, layout, 3, what=f"RGBAPS tap {tap}")
        assert f.last_strided()[:3] == (1, 1, 1)
        assert 0 < f.periodic_support(0) < f.plan_info(0).filter_size
        for i in range(4):
            flags = f.last_finite_flags(i)
            assert flags is not None, f"plane {i} did not take the flagged path"
            print(f"tap {tap} plane {i} flags {flags.tolist()}")
            assert flags.tolist() == ([0, 1, 0] if i == 1 else [0, 0, 0]), (i, flags.tolist())
        ref = run_planar(torch, f, frames, 3)
    dims = f.out_dims()
    for k in range(3):
        for i, (w, h) in enumerate(dims):
            a, p, b = (x[:h, :w].view(np.uint32) for x in (got[k][i], ref[k][i], wants[k][i]))
            nan_a, nan_b = np.isnan(a.view(np.float32)), np.isnan(b.view(np.float32))
            print(f"tap {tap} frame {k} plane {i}: {int((a != p).sum())} samples differ from the planar call, {int((a != b).sum())} from the oracle "
                  f"({int((nan_a != nan_b).sum())} in the NaN footprint, {int((a != b)[~nan_a & ~nan_b].sum())} finite)")
            assert np.array_equal(a, p), f"frame {k} plane {i}: differs from the planar call"
            assert np.array_equal(a, b), f"frame {k} plane {i}: differs from the oracle"
    assert np.isnan(wants[1][1]).any() and not np.isnan(wants[1][0]).any()
    f.close()


# ---- 9. validation that needs the device -------------------------------------------------------------------------------------------------

def test_pitch_and_alignment_are_refused_and_nothing_is_written(gpu_pkg, O):
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = 40, 24, 63, 37
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["RGBP16"], sw, sh, tw, th, device=0, tap=3)
    fmt = f.fmt
    frames, _ = frames_and_wants(O, gpu_pkg, "RGBP16", sw, sh, tw, th, dict(tap=3), 1)
    layout = packed("BGR", 3, 3)
    src = Side(torch, fmt.plane_dims(sw, sh), fmt.dtype, layout, 1, seed=41).fill(frames).upload()
    dst = Side(torch, f.out_dims(), fmt.dtype, layout, 1, seed=42).upload()
    s = torch.cuda.current_stream()
    need_src, need_dst = ((sw - 1) * 3 + 1) * 2, ((tw - 1) * 3 + 1) * 2

    def call(sp=None, dp=None, sptr=None, dptr=None, n=1):
        f.process_device_strided(sptr or src.ptrs(), sp or src.pitches(), src.steps(), src.strides(), dptr or dst.ptrs(), dp or dst.pitches(),
                                 dst.steps(), dst.strides(), n, stream=s.cuda_stream)

    bad = [dict(sp=[need_src - 2] * 3), dict(dp=[need_dst - 2] * 3), dict(sp=[need_src + 1] * 3),
           dict(sptr=[p + 1 for p in src.ptrs()]), dict(dptr=[p + 1 for p in dst.ptrs()]), dict(n=0), dict(n=65536)]
    for kw in bad:
        with pytest.raises(gpu_pkg.JincError) as e:
            call(**kw)
        assert e.value.code == INVALID_ARG and str(e.value).startswith("JincResize:"), kw
    call(sp=[need_src] * 3, dp=None)   # the smallest pitch that holds the row is accepted (reads stay inside the buffer's rows)
    s.synchronize()
    dst2 = Side(torch, f.out_dims(), fmt.dtype, layout, 1, seed=42).upload()
    for kw in bad:
        with pytest.raises(gpu_pkg.JincError):
            f.process_device_strided(kw.get("sptr") or src.ptrs(), kw.get("sp") or src.pitches(), src.steps(), src.strides(),
                                     kw.get("dptr") or dst2.ptrs(), kw.get("dp") or dst2.pitches(), dst2.steps(), dst2.strides(), kw.get("n", 1),
                                     stream=s.cuda_stream)
    s.synchronize()
    image = dst2.download()
    for b, B in dst2.bufs.items():
        assert np.array_equal(image[b], B["host"]), "a refused call wrote to the destination"
    f.close()
