"""Half-precision (IEEE binary16) float planes on the host side, no GPU needed: jinc_filter_create_ex's checks, the plan of a
half filter against the fp32 filter of the same geometry, SIMD-order modes refused, and half clips through the VapourSynth
shell (tests/mock_vs/) -- a node of the input's format and the target size instead of an error."""
import ctypes as C

import numpy as np
import pytest

from test_plugin_vs_mock_host import Core, vs  # noqa: F401  (the session fixture that builds the shell + mock host)

JINC_ERR_INVALID_ARG, JINC_ERR_UNSUPPORTED = -1, -5

SHAPES = [
    ("YH", "Y32", 64, 48, 160, 120, {}),
    ("YH", "Y32", 640, 360, 1280, 720, {}),
    ("YH", "Y32", 97, 61, 291, 183, {}),
    ("YH", "Y32", 320, 180, 480, 270, dict(tap=8)),
    ("YH", "Y32", 480, 270, 320, 180, {}),
    ("YUV420PH", "YUV420PS", 128, 96, 256, 192, dict(cplace="mpeg2")),
    ("YUV420PH", "YUV420PS", 128, 96, 256, 192, dict(cplace="mpeg1")),
    ("YUV420PH", "YUV420PS", 128, 96, 256, 192, dict(cplace="topleft")),
    ("YUV422PH", "YUV422PS", 128, 96, 300, 200, {}),
    ("YUV411PH", "YUV411PS", 128, 96, 256, 192, dict(tap=4)),
    ("RGBPH", "RGBPS", 200, 100, 400, 200, dict(tap=4, blur=0.98)),
    ("YUVA420PH", "YUVA420PS", 50, 40, 120, 96, dict(tap=4, src_left=-2.5, src_top=1.25, src_width=55, src_height=41.5,
                                                     quant_x=7, quant_y=13)),
]


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


def test_half_formats_in_the_python_mirror(pkg):
    for name in ("YH", "YUV420PH", "YUV422PH", "YUV444PH", "YUV411PH", "YUVA420PH", "YUVA422PH", "YUVA444PH", "YUVA411PH",
                 "RGBPH", "RGBAPH"):
        f = pkg.FORMATS[name]
        assert f.half and f.bits == 16 and f.sample_bytes == 2 and f.dtype == np.float16 and f.sample_type == pkg.SAMPLE_FLOAT16
    assert pkg.FORMATS["Y32"].dtype == np.float32 and not pkg.FORMATS["Y32"].half and pkg.FORMATS["Y16"].dtype == np.uint16


@pytest.mark.parametrize("bits,size", [(8, 1), (10, 2), (32, 4), (16, 1), (16, 4), (32, 2)])
def test_create_ex_refuses_half_with_the_wrong_sample_size(pkg, bits, size):
    rc, msg = _create_ex(pkg, (64, 48, bits, size, 1, 1, 0, 0, 0), pkg.SAMPLE_FLOAT16)
    assert rc == JINC_ERR_INVALID_ARG
    assert msg.startswith("JincResize: ") and "16 bits" in msg


def test_create_ex_refuses_unknown_sample_types(pkg):
    rc, msg = _create_ex(pkg, (64, 48, 16, 2, 1, 1, 0, 0, 0), 2)
    assert rc == JINC_ERR_INVALID_ARG and msg.startswith("JincResize: ")


@pytest.mark.parametrize("vi", [(64, 48, 16, 2, 1, 1, 0, 0, 0), (64, 48, 16, 2, 3, 1, 0, 1, 1), (64, 48, 16, 2, 4, 1, 1, 0, 0)],
                         ids=["Y", "420", "RGBA"])
def test_create_ex_accepts_half_clips_without_a_device(pkg, vi):
    assert _create_ex(pkg, vi, pkg.SAMPLE_FLOAT16) == (0, "")
    assert _create_ex(pkg, vi, pkg.SAMPLE_DEFAULT) == (0, "")   # the same clip as 16-bit integers: create's behaviour


def test_create_ex_default_is_create(pkg):
    """The reference's own checks come first either way (here: tap out of range)."""
    for st in (pkg.SAMPLE_DEFAULT, pkg.SAMPLE_FLOAT16):
        vi = pkg.VideoInfo(64, 48, 16, 2, 1, 1, 0, 0, 0)
        a = pkg.Args()
        a.target_width, a.target_height, a.tap, a.defined = 128, 96, 17, pkg.ARG_BITS["tap"]
        a.frame0_chroma_location = -1
        out, err = C.c_void_p(), C.create_string_buffer(256)
        assert pkg.lib().jinc_filter_create_ex(C.byref(vi), C.byref(a), st, -1, C.byref(out), err, len(err)) == JINC_ERR_INVALID_ARG
        assert err.value.decode() == "JincResize: tap must be between 1..16." and not out


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: f"{c[0]}_{c[2]}x{c[3]}to{c[4]}x{c[5]}_" + "_".join(f"{k}{v}" for k, v in c[6].items()
                                                                                                        if k in ("tap", "cplace")))
def test_half_plan_is_the_fp32_plan(pkg, case):
    hname, fname, sw, sh, tw, th, kw = case
    fh = pkg.Filter(pkg.FORMATS[hname], sw, sh, tw, th, device=-1, **kw)
    ff = pkg.Filter(pkg.FORMATS[fname], sw, sh, tw, th, device=-1, **kw)
    assert fh.num_tables == ff.num_tables and fh.out_dims() == ff.out_dims()
    for t in range(ff.num_tables):
        a, b = fh.plan_info(t), ff.plan_info(t)
        assert [getattr(a, n) for n, _ in a._fields_] == [getattr(b, n) for n, _ in b._fields_]
        for x, y in zip(fh.plan_dump(t), ff.plan_dump(t)):
            assert np.array_equal(x, y)
        assert np.array_equal(fh.plan_sets(t).view(np.uint32), ff.plan_sets(t).view(np.uint32))
    fh.close()
    ff.close()


def test_simd_order_modes_do_not_exist_for_half(pkg):
    f = pkg.Filter(pkg.FORMATS["YH"], 64, 48, 128, 96, device=-1)
    for order in (1, 2, 3):
        rc = pkg.lib().jinc_filter_set_simd_order(f._h, order)
        assert rc == JINC_ERR_UNSUPPORTED
        assert pkg.lib().jinc_last_error().decode().startswith("JincResize: ")
    assert pkg.lib().jinc_filter_set_simd_order(f._h, 0) == 0
    f.close()


class HalfCore(Core):
    def source_half(self, fmt, w, h, frames):
        """A stFloat / 16-bit source (GRAYH, YUV4xxPH, RGBH) with the given float16 planes."""
        family = 2 if fmt.rgb else (1 if fmt.planes == 1 else 3)
        node = self.L.mockvs_source_new(self.h, w, h, family, 1, 16, 2, fmt.sub_w, fmt.sub_h, fmt.planes, len(frames), -1)
        for n, planes in enumerate(frames):
            fr = self.L.mockvs_source_frame(node, n)
            for i, p in enumerate(planes):
                _, row, hh, _ = self._dims(fr, i)
                self._plane(fr, i)[:, :] = np.ascontiguousarray(p[:hh]).view(np.uint8).reshape(hh, -1)[:, :row]
        return node


def half_frame(pkg, fmt, w, h, seed=7):
    rng = np.random.default_rng(seed)
    return [pkg.alloc_plane(pw, ph, np.float16) + rng.random((ph, 1), dtype=np.float32).astype(np.float16)
            for (pw, ph) in fmt.plane_dims(w, h)]


@pytest.mark.parametrize("name", ["YH", "YUV420PH", "RGBPH"])
@pytest.mark.parametrize("function", ["JincResize", "Jinc64Resize"])
def test_vapoursynth_shell_takes_half_clips(vs, pkg, name, function):  # noqa: F811
    c = HalfCore(vs)
    fmt = pkg.FORMATS[name]
    src = c.source_half(fmt, 64, 48, [half_frame(pkg, fmt, 64, 48)])
    node, err = c.invoke(function, src, 160, 120)
    assert err is None, err
    w, h, n, mode = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    vs.mockvs_node_info(node, C.byref(w), C.byref(h), C.byref(n), C.byref(mode))
    assert (w.value, h.value, n.value) == (160, 120, 1)
    vs.mockvs_node_release(node)
    vs.mockvs_node_release(src)
    assert c.live() == (0, 0)
    c.close()


def test_vapoursynth_shell_skips_the_simd_order_hook_for_half(vs, pkg, monkeypatch):  # noqa: F811
    monkeypatch.setenv("JINCRESIZE_SIMD_ORDER", "2")
    c = HalfCore(vs)
    fmt = pkg.FORMATS["YH"]
    src = c.source_half(fmt, 64, 48, [half_frame(pkg, fmt, 64, 48)])
    node, err = c.invoke("JincResize", src, 128, 96)
    assert err is None, err
    vs.mockvs_node_release(node)
    vs.mockvs_node_release(src)
    c.close()
