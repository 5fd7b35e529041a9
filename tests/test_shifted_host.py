"""Host side of jinc_filter_process_device_shifted: the export, the mirror, the header, and the shift checks -- they need no device
and come before the device check, so a filter without one shows them."""
import pytest

INVALID_ARG, NO_DEVICE = -1, -2


def test_the_shifted_entry_is_exported_declared_and_mirrored(pkg):
    name = "jinc_filter_process_device_shifted"
    assert name in pkg.EXPORTS and hasattr(pkg.lib(), name)
    assert hasattr(pkg.Filter, "process_device_shifted")
    header = open(pkg.HEADER_PATH).read()
    assert name + "(" in header and "src_sample_shift[4]" in header and "dst_sample_shift[4]" in header


def _call(f, src_shifts, dst_shifts, steps=None):
    n = f.fmt.planes
    f.process_device_shifted([256, 512, 768, 1024][:n], [4096] * n, steps, src_shifts, [0] * n,
                             [4096, 8192, 12288, 16384][:n], [8192] * n, steps, dst_shifts, [0] * n, 1)


# (format, the largest shift it takes): 8 * component_size - bits for integer samples, none for float and binary16 ones
CASES = [("YUV420P8", 0), ("YUV420P10", 6), ("YUV420P12", 4), ("YUV420P14", 2), ("YUV420P16", 0), ("Y10", 6), ("YUV420PS", 0), ("YUV420PH", 0)]


@pytest.mark.parametrize("fmt,largest", CASES, ids=[c[0] for c in CASES])
def test_shifts_are_checked_against_the_format_before_the_device(pkg, fmt, largest):
    f = pkg.Filter(pkg.FORMATS[fmt], 40, 24, 80, 48, device=-1)
    n = f.fmt.planes
    messages = set()
    for side in (0, 1):
        for plane in range(n):
            for bad, word in ((-1, "negative"), (largest + 1, "shift"), (15, "shift"), (16, "shift"), (1 << 20, "shift")):
                shifts = [0] * n
                shifts[plane] = bad
                with pytest.raises(pkg.JincError) as e:
                    _call(f, shifts if side == 0 else None, None if side == 0 else shifts)
                assert e.value.code == INVALID_ARG and str(e.value).startswith("JincResize:") and word in str(e.value), (side, plane, bad, str(e.value))
                messages.add(str(e.value))
    print(sorted(messages))
    # a negative shift, a shift beyond the padding, and a shift on samples that fill their word (or are no integers) each say so
    assert len(messages) == 2
    assert any("negative" in m for m in messages)
    assert any(("larger" in m) == (largest > 0) and "negative" not in m for m in messages)
    # accepted shifts get as far as the device check; so do NULL arrays and zeros (the strided call itself)
    for shifts in (None, [0] * n, [largest] * n, [largest] + [0] * (n - 1)):
        for steps in (None, [1] + [2] * (n - 1) if n > 1 else [2]):
            with pytest.raises(pkg.JincError) as e:
                _call(f, shifts, shifts, steps)
            assert e.value.code == NO_DEVICE, (shifts, steps)
    f.close()


def test_the_step_check_of_the_strided_call_still_holds(pkg):
    f = pkg.Filter(pkg.FORMATS["YUV420P10"], 40, 24, 80, 48, device=-1)
    for bad in (0, 5, -1):
        with pytest.raises(pkg.JincError) as e:
            _call(f, [6, 6, 6], [6, 6, 6], [1, bad, 2])
        assert e.value.code == INVALID_ARG and "step" in str(e.value)
    f.close()
