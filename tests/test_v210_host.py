"""Host side of jinc_filter_process_device_v210 and jinc_v210_row_bytes: the exports, the mirror, the header, the row size, and the
filter check -- it needs no device and comes before the null checks of the plane arrays and before the device check, so a filter
without a device shows it."""
import ctypes as C

import pytest

INVALID_ARG, NO_DEVICE = -1, -2


def test_the_entries_are_exported_declared_and_mirrored(pkg):
    header = open(pkg.HEADER_PATH).read()
    for name in ("jinc_filter_process_device_v210", "jinc_v210_row_bytes"):
        assert name in pkg.EXPORTS and hasattr(pkg.lib(), name)
        assert name + "(" in header
    assert "int src_is_v210" in header and "int dst_is_v210" in header
    assert hasattr(pkg.Filter, "process_device_v210") and hasattr(pkg, "v210_row_bytes")


@pytest.mark.parametrize("width,want", [(0, 0), (1, 16), (2, 16), (6, 16), (7, 32), (46, 128), (48, 128), (50, 144), (1920, 5120)])
def test_row_bytes(pkg, width, want):
    assert pkg.v210_row_bytes(width) == want
    assert pkg.v210_row_bytes(-width) == 0


def _call(f, src_is_v210, dst_is_v210):
    n = f.fmt.planes
    f.process_device_v210([256, 512, 768, 1024][:n], [4096] * n, src_is_v210, [0] * n,
                          [4096, 8192, 12288, 16384][:n], [8192] * n, dst_is_v210, [0] * n, 1)


def test_yuv422p10_reaches_the_device_check(pkg):
    f = pkg.Filter(pkg.FORMATS["YUV422P10"], 40, 24, 80, 48, device=-1)
    for src, dst in ((1, 1), (1, 0), (0, 1), (0, 0)):
        with pytest.raises(pkg.JincError) as e:
            _call(f, src, dst)
        assert e.value.code == NO_DEVICE, (src, dst, str(e.value))
    f.close()


REFUSED_FILTERS = ["YUV420P10", "YUV444P10", "YUV422P8", "YUV422P12", "YUV422P16", "YUVA422P10", "YUV422PH", "RGBP10", "Y10"]


@pytest.mark.parametrize("fmt", REFUSED_FILTERS)
def test_other_filters_are_refused_before_the_device_check(pkg, fmt):
    f = pkg.Filter(pkg.FORMATS[fmt], 40, 24, 80, 48, device=-1)
    messages = set()
    for src, dst in ((1, 0), (0, 1), (1, 1)):
        with pytest.raises(pkg.JincError) as e:
            _call(f, src, dst)
        assert e.value.code == INVALID_ARG and str(e.value).startswith("JincResize:"), (src, dst, str(e.value))
        messages.add(str(e.value))
        # ... even with null plane arrays: the filter is looked at first
        rc = pkg.lib().jinc_filter_process_device_v210(f._h, None, None, src, None, None, None, dst, None, 1, C.c_void_p(0))
        assert rc == INVALID_ARG
        messages.add(pkg.lib().jinc_last_error().decode())
    assert len(messages) == 1 and "YUV422P10" in messages.pop()
    with pytest.raises(pkg.JincError) as e:   # both sides dense: the call is jinc_filter_process_device, on any filter
        _call(f, 0, 0)
    assert e.value.code == NO_DEVICE, str(e.value)
    f.close()


def test_one_message_for_every_refused_filter(pkg):
    messages = set()
    for fmt in REFUSED_FILTERS:
        f = pkg.Filter(pkg.FORMATS[fmt], 40, 24, 80, 48, device=-1)
        with pytest.raises(pkg.JincError) as e:
            _call(f, 1, 1)
        messages.add(str(e.value))
        f.close()
    assert len(messages) == 1, messages


def test_null_plane_arrays_on_the_accepted_filter_are_a_null_argument(pkg):
    f = pkg.Filter(pkg.FORMATS["YUV422P10"], 40, 24, 80, 48, device=-1)
    rc = pkg.lib().jinc_filter_process_device_v210(f._h, None, None, 1, None, None, None, 1, None, 1, C.c_void_p(0))
    assert rc == INVALID_ARG and "null argument" in pkg.lib().jinc_last_error().decode()
    f.close()
