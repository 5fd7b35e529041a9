"""Host side of jinc_filter_process_device_packed10 and jinc_packed10_layout: the exports, the mirror, the header, the named layouts,
and the filter and offset checks -- they need no device and come before the device check, so a filter without one shows them."""
import pytest

INVALID_ARG, NO_DEVICE = -1, -2

# name -> offsets of the library's planes (Y, U, V or G, B, R) in the word
LAYOUTS = {
    "Y410": [10, 0, 20],
    "R10G10B10A2": [10, 20, 0], "ABGR2101010": [10, 20, 0], "XBGR2101010": [10, 20, 0],
    "XRGB2101010": [10, 0, 20], "ARGB2101010": [10, 0, 20],
    "RGBX1010102": [12, 2, 22], "RGBA1010102": [12, 2, 22],
    "BGRX1010102": [12, 22, 2], "BGRA1010102": [12, 22, 2],
}


def test_the_entries_are_exported_declared_and_mirrored(pkg):
    header = open(pkg.HEADER_PATH).read()
    for name in ("jinc_filter_process_device_packed10", "jinc_packed10_layout"):
        assert name in pkg.EXPORTS and hasattr(pkg.lib(), name)
        assert name + "(" in header
    assert "src_field_offset[3]" in header and "dst_field_offset[3]" in header and "unsigned dst_fill" in header
    assert hasattr(pkg.Filter, "process_device_packed10") and hasattr(pkg, "packed10_layout")


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_named_layouts(pkg, name):
    for spelled in (name, name.lower(), name.capitalize()):
        offsets, fill = pkg.packed10_layout(spelled)
        assert offsets == LAYOUTS[name], (spelled, offsets)
        fields = sum(1023 << o for o in offsets)
        assert fill == (~fields) & 0xFFFFFFFF and bin(fill).count("1") == 2, (spelled, hex(fill))


def test_an_unknown_layout_is_refused(pkg):
    for name in ("Y416", "", "Y410 ", "R10G10B10", "v210"):
        with pytest.raises(pkg.JincError) as e:
            pkg.packed10_layout(name)
        assert e.value.code == INVALID_ARG and str(e.value).startswith("JincResize:"), name


def _call(f, src_offsets, dst_offsets, fill=0xC0000000):
    n = f.fmt.planes
    f.process_device_packed10([256, 512, 768, 1024][:n], [4096] * n, src_offsets, [0] * n,
                              [4096, 8192, 12288, 16384][:n], [8192] * n, dst_offsets, fill, [0] * n, 1)


@pytest.mark.parametrize("fmt", ["YUV444P10", "RGBP10"])
def test_accepted_filters_reach_the_device_check(pkg, fmt):
    f = pkg.Filter(pkg.FORMATS[fmt], 40, 24, 80, 48, device=-1)
    for src, dst in (([10, 0, 20], [10, 0, 20]), ([10, 0, 20], None), (None, [12, 22, 2]), (None, None)):
        with pytest.raises(pkg.JincError) as e:
            _call(f, src, dst)
        assert e.value.code == NO_DEVICE, (src, dst, str(e.value))
    f.close()


REFUSED_FILTERS = ["YUV420P10", "YUV444P8", "YUV444P12", "YUV444P16", "YUVA444P10", "RGBPS", "RGBPH", "Y10"]


@pytest.mark.parametrize("fmt", REFUSED_FILTERS)
def test_other_filters_are_refused_before_the_device_check(pkg, fmt):
    f = pkg.Filter(pkg.FORMATS[fmt], 40, 24, 80, 48, device=-1)
    messages = set()
    for src, dst in (([10, 0, 20], None), (None, [10, 0, 20]), ([10, 0, 20], [10, 0, 20])):
        with pytest.raises(pkg.JincError) as e:
            _call(f, src, dst)
        assert e.value.code == INVALID_ARG and str(e.value).startswith("JincResize:"), (src, dst, str(e.value))
        messages.add(str(e.value))
    assert len(messages) == 1
    f.close()


@pytest.mark.parametrize("fmt", ["YUV444P10", "RGBP10"])
def test_offsets_are_checked_before_the_device(pkg, fmt):
    f = pkg.Filter(pkg.FORMATS[fmt], 40, 24, 80, 48, device=-1)

    def refused(offsets):
        out = set()
        for src, dst in ((offsets, None), (None, offsets), ([0, 10, 20], offsets), (offsets, [0, 10, 20])):
            with pytest.raises(pkg.JincError) as e:
                _call(f, src, dst)
            assert e.value.code == INVALID_ARG and str(e.value).startswith("JincResize:"), (offsets, src, dst, str(e.value))
            out.add(str(e.value))
        assert len(out) == 1, out
        return out.pop()

    range_messages = {refused(o) for bad in (-1, 23, 32) for o in ([bad, 10, 20], [0, bad, 20], [0, 10, bad])}
    overlap_messages = {refused(o) for o in ([0, 5, 20], [10, 10, 20], [0, 20, 11], [22, 13, 0])}
    print(range_messages, overlap_messages)
    assert len(range_messages) == 1 and len(overlap_messages) == 1 and range_messages != overlap_messages
    assert "overlap" in overlap_messages.pop() and "0..22" in range_messages.pop()
    for good in ([0, 10, 20], [2, 12, 22], [22, 0, 11]):
        for src, dst in ((good, None), (None, good), (good, good)):
            with pytest.raises(pkg.JincError) as e:
                _call(f, src, dst)
            assert e.value.code == NO_DEVICE, (good, str(e.value))
    f.close()
