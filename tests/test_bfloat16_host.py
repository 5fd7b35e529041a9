"""bfloat16 planes (JINC_SAMPLE_BFLOAT16) on the host side, no GPU needed -- and the test-side DEFINITION the GPU files share.

A bfloat16 sample is the upper 16 bits of an IEEE fp32 value.  numpy has no such dtype: planes are np.uint16 holding the bit
patterns, and the definition lives on bit patterns:

    widen(u16)  = (u16.astype(u32) << 16).view(f32)                      exact for every pattern
    narrow(f32) = (u + 0x7fff + ((u >> 16) & 1)) >> 16                   round to nearest even, for every non-NaN input
                  "any NaN"                                              for NaN inputs

Expected planes are narrow(oracle_fp32(widen(src))); NaN positions are compared, NaN payloads are not.  The first test pins the
two functions to torch's float32 <-> bfloat16 conversions, which are not the code under test.

The `wide` sample set: random finite bfloat16 samples of both signs, the left quarter of a plane 0x7f7f (the largest finite value:
the overshoot beside that step overflows to +-inf), the bottom quarter subnormals only.  Random exponents over the WHOLE range break
"at least half of all results finite" (a window of fs^2 taps holds a sample near 2^127 almost surely, and the fp32 partial sums
overflow), so the random part draws its biased exponent from 0 .. WIDE_EXP_MAX = 0xdf (magnitudes below 2^97) and sits in the
right three quarters of the upper three quarters of a plane only; see test_wide_samples_meet_their_conditions_on_the_oracle."""
import ctypes as C

import numpy as np
import pytest

from conftest import oracle_kwargs

JINC_ERR_INVALID_ARG, JINC_ERR_NO_DEVICE, JINC_ERR_UNSUPPORTED = -1, -2, -5

BF_NAMES = ("YBF", "YUV420PBF", "YUV422PBF", "YUV444PBF", "YUV411PBF", "YUVA420PBF", "YUVA422PBF", "YUVA444PBF", "YUVA411PBF",
            "RGBPBF", "RGBAPBF")
WIDE_EXP_MAX = 0xdf


# ---- the definition -------------------------------------------------------------------------------------------------------------------

def widen(u16):
    return (np.ascontiguousarray(u16).astype(np.uint32) << 16).view(np.float32)


def narrow(f32):
    """bfloat16 bits of fp32 values, round to nearest even; NaN inputs give 0x7fc0 (callers compare NaN positions only)."""
    u = np.ascontiguousarray(f32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    out = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    out[np.isnan(f32)] = 0x7fc0
    return out


def is_nan(u16):
    return (np.asarray(u16) & 0x7fff) > 0x7f80


def fp32_name(bname):
    return "Y32" if bname == "YBF" else bname[:-2] + "S"


def unit_frame(O, bname, w, h, seed):
    """The LCG frame of the fp32 format (samples in [0, 1]) narrowed to bfloat16."""
    return [narrow(p) for p in O.lcg_frame(O.FORMATS[fp32_name(bname)], w, h, seed=seed)]


def wide_frame(pkg, bname, w, h, seed):
    rng = np.random.default_rng(seed)
    out = []
    for (pw, ph) in pkg.FORMATS[bname].plane_dims(w, h):
        p = pkg.alloc_plane(pw, ph, np.uint16)
        exp = rng.integers(0, WIDE_EXP_MAX + 1, size=p.shape, dtype=np.uint16)
        bits = (exp << 7) | rng.integers(0, 0x80, size=p.shape, dtype=np.uint16) | (rng.integers(0, 2, size=p.shape, dtype=np.uint16) << 15)
        bits[:, :pw // 4] = 0x7f7f
        bits[ph - ph // 4:, pw // 4:] = rng.integers(0, 0x0080, size=bits[ph - ph // 4:, pw // 4:].shape, dtype=np.uint16)
        p[...] = bits
        out.append(p)
    return out


def definition(O, bname, sw, sh, tw, th, kw, src):
    of = O.OracleFilter(O.FORMATS[fp32_name(bname)], sw, sh, tw, th, **oracle_kwargs(kw))
    with np.errstate(over="ignore", invalid="ignore"):
        return [narrow(p) for p in of.get_frame([widen(s) for s in src], threads=4)]


def assert_bf16_equal(got, want, dims, what=""):
    for i, (w, h) in enumerate(dims):
        a = np.ascontiguousarray(got[i][:h, :w])
        b = np.ascontiguousarray(want[i][:h, :w])
        assert a.dtype == np.uint16 and b.dtype == np.uint16
        na, nb = is_nan(a), is_nan(b)
        bad = np.argwhere((na != nb) | (~na & (a != b)))
        if len(bad):
            y, x = bad[0]
            raise AssertionError(f"{what}: plane {i} differs at {len(bad)} samples; first (x={x}, y={y}): "
                                 f"got {a[y, x]:#06x} ({widen(a[y:y + 1, x:x + 1])[0, 0]!r}), want {b[y, x]:#06x} ({widen(b[y:y + 1, x:x + 1])[0, 0]!r})")


def conversion_set():
    """All 65 536 upper halves x the lower halves that decide a rounding: 393 216 fp32 values, as bits."""
    hi = np.arange(0, 1 << 16, dtype=np.uint32) << 16
    return np.concatenate([hi | np.uint32(lo) for lo in (0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff)])


# ---- the definition against torch -----------------------------------------------------------------------------------------------------

def test_the_definition_is_torch_bfloat16():
    torch = pytest.importorskip("torch")
    u = conversion_set()
    f = u.view(np.float32)
    want = torch.from_numpy(f.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = narrow(f)
    nan = np.isnan(f)
    assert np.array_equal(is_nan(got), nan) and np.array_equal(is_nan(want), nan)
    assert np.array_equal(got[~nan], want[~nan])
    assert not (is_nan(got) & ((got & 0x7fff) == 0x7f80)).any()           # a NaN never becomes an infinity
    assert narrow(np.array([3.3895314e38], np.float32))[0] == 0x7f7f     # 0x7f7f7fff stays finite
    assert narrow(np.array([0x7f7f8000], np.uint32).view(np.float32))[0] == 0x7f80   # the tie above the largest finite value: +inf
    assert narrow(np.array([-0.0], np.float32))[0] == 0x8000 and narrow(np.array([1e-40], np.float32))[0] == 0x0001
    every = np.arange(0, 1 << 16, dtype=np.uint16)
    back = torch.from_numpy(every.view(np.int16).copy()).view(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(widen(every).view(np.uint32), back.view(np.uint32))


# ---- create-time checks ---------------------------------------------------------------------------------------------------------------

def _create_ex(pkg, vi, sample_type, w=64, h=48):
    vi_s = pkg.VideoInfo(*vi)
    a = pkg.Args()
    a.target_width, a.target_height = 2 * w, 2 * h
    a.frame0_chroma_location = -1
    out, err = C.c_void_p(), C.create_string_buffer(256)
    rc = pkg.lib().jinc_filter_create_ex(C.byref(vi_s), C.byref(a), sample_type, -1, C.byref(out), err, len(err))
    if out:
        pkg.lib().jinc_filter_free(out)
    return rc, err.value.decode()


def test_sample_type_value():
    import re
    from __graft_entry__ import load_package
    pkg = load_package()
    assert pkg.SAMPLE_BFLOAT16 == 3   # (2 stays an unknown sample type, refused as before: tests/test_half_planes_host.py)
    with open(pkg.HEADER_PATH) as fh:
        assert re.search(r"#define\s+JINC_SAMPLE_BFLOAT16\s+3\b", fh.read())


@pytest.mark.parametrize("bits,size", [(8, 1), (10, 2), (32, 4), (16, 1), (16, 4), (32, 2)])
def test_create_ex_refuses_bfloat16_with_the_wrong_sample_size(pkg, bits, size):
    rc, msg = _create_ex(pkg, (64, 48, bits, size, 1, 1, 0, 0, 0), pkg.SAMPLE_BFLOAT16)
    assert rc == JINC_ERR_INVALID_ARG
    assert msg.startswith("JincResize: bfloat16 ") and "16 bits" in msg
    rc, half_msg = _create_ex(pkg, (64, 48, bits, size, 1, 1, 0, 0, 0), pkg.SAMPLE_FLOAT16)
    assert rc == JINC_ERR_INVALID_ARG and half_msg != msg                 # a message of its own


@pytest.mark.parametrize("sample_type", [2, 4, -1, 16])
def test_create_ex_names_all_three_sample_types(pkg, sample_type):
    rc, msg = _create_ex(pkg, (64, 48, 16, 2, 1, 1, 0, 0, 0), sample_type)
    assert rc == JINC_ERR_INVALID_ARG and msg.startswith("JincResize: sample type must be ")
    for name in ("JINC_SAMPLE_DEFAULT", "JINC_SAMPLE_FLOAT16", "JINC_SAMPLE_BFLOAT16"):
        assert name in msg


@pytest.mark.parametrize("vi", [(64, 48, 16, 2, 1, 1, 0, 0, 0), (64, 48, 16, 2, 3, 1, 0, 1, 1), (64, 48, 16, 2, 4, 1, 1, 0, 0)],
                         ids=["Y", "420", "RGBA"])
def test_create_ex_accepts_bfloat16_clips_without_a_device(pkg, vi):
    assert _create_ex(pkg, vi, pkg.SAMPLE_BFLOAT16) == (0, "")


def test_batch_create_ex_takes_the_sample_type(pkg):
    """jinc_batch_create_ex hands the type to jinc_filter_create_ex: its refusal comes back through the batch call."""
    vi = pkg.VideoInfo(64, 48, 10, 2, 1, 1, 0, 0, 0)
    a = pkg.Args()
    a.target_width, a.target_height, a.frame0_chroma_location = 128, 96, -1
    out, err = C.c_void_p(), C.create_string_buffer(256)
    rc = pkg.lib().jinc_batch_create_ex(C.byref(vi), C.byref(a), pkg.SAMPLE_BFLOAT16, 1, 1, 0, C.byref(out), err, len(err))
    assert rc != 0 and not out
    if rc == JINC_ERR_INVALID_ARG:   # (a machine without a device may answer that first)
        assert err.value.decode().startswith("JincResize: bfloat16 ")


# ---- the Python mirror ----------------------------------------------------------------------------------------------------------------

def test_bfloat16_formats_in_the_python_mirror(pkg):
    for name in BF_NAMES:
        f = pkg.FORMATS[name]
        h = pkg.FORMATS[name[:-2] + "H"]
        assert f.bfloat16 and not f.half and f.bits == 16 and f.sample_bytes == 2 and f.dtype == np.uint16
        assert f.sample_type == pkg.SAMPLE_BFLOAT16 == 3
        assert (f.planes, f.sub_w, f.sub_h, f.rgb) == (h.planes, h.sub_w, h.sub_h, h.rgb)
        for (w, hh) in ((64, 48), (130, 98)):
            assert f.plane_dims(w, hh) == h.plane_dims(w, hh)
        vi = f.video_info(64, 48)
        assert (vi.bits_per_component, vi.component_size, vi.num_components) == (16, 2, f.planes)
    assert pkg.FORMATS["YUV420PBF"].plane_dims(130, 98) == [(130, 98), (65, 49), (65, 49)]
    assert pkg.FORMATS["RGBAPBF"].plane_dims(64, 48) == [(64, 48)] * 4
    assert not pkg.FORMATS["YH"].bfloat16 and not pkg.FORMATS["Y16"].bfloat16 and pkg.FORMATS["Y16"].sample_type == pkg.SAMPLE_DEFAULT
    assert "jinc_debug_convert_bfloat16" in pkg.EXPORTS and callable(pkg.debug_convert_bfloat16)
    assert "bfloat16" in pkg.Filter.process_device_widened.__doc__


@pytest.mark.parametrize("case", [("YBF", 64, 48, 160, 120, {}), ("YBF", 640, 360, 1280, 720, {}), ("YBF", 480, 270, 320, 180, {}),
                                  ("YUV420PBF", 128, 96, 256, 192, dict(cplace="mpeg2")), ("RGBPBF", 200, 100, 400, 200, dict(tap=4, blur=0.98))],
                         ids=lambda c: f"{c[0]}_{c[1]}x{c[2]}to{c[3]}x{c[4]}")
def test_bfloat16_plan_is_the_fp32_plan(pkg, case):
    bname, sw, sh, tw, th, kw = case
    fb = pkg.Filter(pkg.FORMATS[bname], sw, sh, tw, th, device=-1, **kw)
    ff = pkg.Filter(pkg.FORMATS[fp32_name(bname)], sw, sh, tw, th, device=-1, **kw)
    assert fb.num_tables == ff.num_tables and fb.out_dims() == ff.out_dims()
    for t in range(ff.num_tables):
        a, b = fb.plan_info(t), ff.plan_info(t)
        assert [getattr(a, n) for n, _ in a._fields_] == [getattr(b, n) for n, _ in b._fields_]
        assert np.array_equal(fb.plan_sets(t).view(np.uint32), ff.plan_sets(t).view(np.uint32))
    fb.close()
    ff.close()


def test_simd_order_modes_do_not_exist_for_bfloat16(pkg):
    f = pkg.Filter(pkg.FORMATS["YBF"], 64, 48, 128, 96, device=-1)
    h = pkg.Filter(pkg.FORMATS["YH"], 64, 48, 128, 96, device=-1)
    for order in (1, 2, 3):
        assert pkg.lib().jinc_filter_set_simd_order(f._h, order) == JINC_ERR_UNSUPPORTED
        msg = pkg.lib().jinc_last_error().decode()
        assert msg.startswith("JincResize: ") and "bfloat16" in msg
        assert pkg.lib().jinc_filter_set_simd_order(h._h, order) == JINC_ERR_UNSUPPORTED
        assert pkg.lib().jinc_last_error().decode() != msg                # a message of its own
    assert pkg.lib().jinc_filter_set_simd_order(f._h, 0) == 0
    f.close()
    h.close()


# ---- the device calls' refusals that need no device ------------------------------------------------------------------------------------

def test_widened_call_takes_8_bit_sources_only(pkg):
    f = pkg.Filter(pkg.FORMATS["YUV420PBF"], 64, 48, 128, 96, device=-1)
    ptrs, pitches = [4096, 8192, 8194], [64, 64, 64]
    for bits in (9, 10, 11, 16):
        with pytest.raises(pkg.JincError) as e:
            f.process_device_widened(ptrs, [128, 128, 128], [1, 2, 2], None, bits, None, ptrs, [256, 128, 128], None, None, 1)
        assert e.value.code == JINC_ERR_INVALID_ARG
        assert "not exact in bfloat16" in str(e.value) and f"{bits}-bit" in str(e.value)
    with pytest.raises(pkg.JincError) as e:   # 8 bits: accepted up to the device check
        f.process_device_widened(ptrs, pitches, [1, 2, 2], None, 8, None, ptrs, [256, 128, 128], None, None, 1)
    assert e.value.code == JINC_ERR_NO_DEVICE
    f.close()
    h = pkg.Filter(pkg.FORMATS["YUV420PH"], 64, 48, 128, 96, device=-1)
    with pytest.raises(pkg.JincError) as e:   # (binary16 keeps its own rule: 10 bits pass the check)
        h.process_device_widened(ptrs, [128, 128, 128], [1, 2, 2], None, 10, None, ptrs, [256, 128, 128], None, None, 1)
    assert e.value.code == JINC_ERR_NO_DEVICE
    h.close()


def test_words_and_blocks_calls_refuse_a_bfloat16_filter(pkg):
    f = pkg.Filter(pkg.FORMATS["RGBPBF"], 64, 48, 128, 96, device=-1)
    with pytest.raises(pkg.JincError) as e:
        f.process_device_widened_packed10(4096, 256, [10, 0, 20], 0, [4096] * 3, [256] * 3, None, None, 1)
    assert e.value.code == JINC_ERR_INVALID_ARG
    words = str(e.value)
    assert "10:10:10:2" in words and "bfloat16" in words
    f.close()
    f = pkg.Filter(pkg.FORMATS["YUV422PBF"], 96, 48, 192, 96, device=-1)
    with pytest.raises(pkg.JincError) as e:
        f.process_device_widened_v210(4096, 256, 0, [4096] * 3, [384, 192, 192], None, None, 1)
    assert e.value.code == JINC_ERR_INVALID_ARG
    blocks = str(e.value)
    assert "v210" in blocks and "bfloat16" in blocks and blocks != words
    # ... and the integer calls of the same sources keep refusing it (bits_per_component is 16)
    with pytest.raises(pkg.JincError) as e:
        f.process_device_v210([4096] * 3, [256] * 3, 1, None, [4096] * 3, [384, 192, 192], 0, None, 1)
    assert e.value.code == JINC_ERR_INVALID_ARG and "v210" in str(e.value)
    f.close()
    f = pkg.Filter(pkg.FORMATS["YUV444PBF"], 64, 48, 128, 96, device=-1)
    with pytest.raises(pkg.JincError) as e:
        f.process_device_packed10([4096] * 3, [256] * 3, [10, 0, 20], None, [4096] * 3, [256] * 3, None, 0, None, 1)
    assert e.value.code == JINC_ERR_INVALID_ARG and "10:10:10:2" in str(e.value)
    f.close()


def test_shifted_call_refuses_a_shift_on_bfloat16(pkg):
    f = pkg.Filter(pkg.FORMATS["YBF"], 64, 48, 128, 96, device=-1)
    for side in ("src", "dst"):
        shifts = dict(src=([2], None), dst=(None, [1]))[side]
        with pytest.raises(pkg.JincError) as e:
            f.process_device_shifted([4096], [128], None, shifts[0], None, [8192], [256], None, shifts[1], None, 1)
        assert e.value.code == JINC_ERR_INVALID_ARG and "sample shift" in str(e.value)
    with pytest.raises(pkg.JincError) as e:   # shift 0: on to the device check
        f.process_device_shifted([4096], [128], None, [0], None, [8192], [256], None, [0], None, 1)
    assert e.value.code == JINC_ERR_NO_DEVICE
    f.close()


# ---- the wide sample set --------------------------------------------------------------------------------------------------------------

def wide_conditions(want):
    """(some +-inf, some subnormal, share of finite results) of an expected plane."""
    mag = want & 0x7fff
    return bool((mag == 0x7f80).any()), bool(((mag > 0) & (mag < 0x0080)).any()), float((mag < 0x7f80).mean())


@pytest.mark.parametrize("case", [("YBF", 320, 180, 640, 360, {}), ("YBF", 64, 48, 160, 120, {}), ("YBF", 480, 270, 320, 180, {}),
                                  ("YBF", 160, 120, 320, 240, dict(tap=8)), ("RGBPBF", 200, 100, 400, 200, dict(tap=4, blur=0.98))],
                         ids=lambda c: f"{c[0]}_{c[1]}x{c[2]}to{c[3]}x{c[4]}")
def test_wide_samples_meet_their_conditions_on_the_oracle(pkg, O, case):
    """On the oracle alone, so that no GPU test can pass on a plane of NaNs: the expected planes of the wide set hold at least one
    +-inf, at least one subnormal result, and at least half of all results are finite."""
    bname, sw, sh, tw, th, kw = case
    src = wide_frame(pkg, bname, sw, sh, 4242)
    for s in src:
        mag = s & 0x7fff
        assert (mag < 0x7f80).all() and (s >> 15).any() and not (s >> 15).all()
    want = definition(O, bname, sw, sh, tw, th, kw, src)[0][:th, :tw]
    inf, sub, finite = wide_conditions(want)
    print(f"wide set {case[:5]}: inf {inf}, subnormal {sub}, finite share {finite:.3f}")
    assert inf and sub and finite >= 0.5, (inf, sub, finite)
