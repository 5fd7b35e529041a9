"""Host side of jinc_filter_process_device_strided: the export, the checks that need no device (null arguments, the step range) and
the grouping of strided planes into channel groups (csrc/dispatch.cpp strided_groups), property-tested over random layouts.  No device
needed."""
import ctypes as C
import itertools
import threading

import numpy as np
import pytest

INVALID_ARG, NO_DEVICE = -1, -2


def test_the_strided_entry_is_exported_and_mirrored(pkg):
    header = open(pkg.HEADER_PATH).read()
    assert "jinc_filter_process_device_strided(" in header
    for name in ("jinc_filter_process_device_strided", "jinc_debug_strided_groups", "jinc_debug_last_strided", "jinc_debug_last_groups"):
        assert name in pkg.EXPORTS and hasattr(pkg.lib(), name), name
    test_header = open(pkg.TEST_HEADER_PATH).read()
    for name in ("jinc_debug_strided_groups", "jinc_debug_last_strided", "jinc_debug_last_groups"):
        assert name + "(" in test_header and name + "(" not in header, name
    assert hasattr(pkg.Filter, "process_device_strided") and hasattr(pkg.Filter, "last_strided") and hasattr(pkg.Filter, "strided_groups")
    assert hasattr(pkg.Filter, "last_groups") and callable(pkg.last_groups)
    assert "strided_scratch_bytes" in pkg.knob_ids()
    assert pkg.last_strided()[:3] == (0, 0, 0)


def test_the_groups_record_mirrors_the_header_and_is_empty_without_a_call(pkg):
    """jinc_group_info field for field (the mirror reads the struct by position), a NULL array and a capacity of 0 are taken, and a
    call refused for want of a device leaves the record empty, as it leaves the launch counts at zero."""
    test_header = open(pkg.TEST_HEADER_PATH).read()
    flat = " ".join(test_header.split())
    fields = [n for n, _ in pkg.GroupInfo._fields_]
    assert "typedef struct jinc_group_info { int " + ", ".join(fields) + "; } jinc_group_info;" in flat
    assert C.sizeof(pkg.GroupInfo) == 4 * len(fields) == 44 and fields[-1] == "shifted"
    # (both records are the calling thread's: a thread of its own has made no call, whatever the tests before this one left)
    failures = []

    def in_a_fresh_thread():
        try:
            L = pkg.lib()
            assert L.jinc_debug_last_groups(None, 0) == 0 and L.jinc_debug_last_groups(None, 8) == 0
            one = (pkg.GroupInfo * 1)()
            assert L.jinc_debug_last_groups(one, 1) == 0 and L.jinc_debug_last_groups(one, 0) == 0
            assert pkg.last_groups() == []
            for fmt, call in (("YUV420PS", "widened"), ("YUV420PS", "narrowed")):
                f = pkg.Filter(pkg.FORMATS[fmt], 40, 24, 80, 48, device=-1)
                with pytest.raises(pkg.JincError) as e:
                    if call == "widened":
                        f.process_device_widened([4096, 8192, 8193], [64] * 3, [1, 2, 2], None, 8, [0] * 3, [1 << 20, 2 << 20, 3 << 20], [512] * 3, None, [0] * 3, 1)
                    else:
                        f.process_device_narrowed([4096, 8192, 12288], [512] * 3, None, [0] * 3, [1 << 20, 2 << 20, (2 << 20) + 1], [80] * 3, [1, 2, 2], None, 8, [0] * 3, 1)
                assert e.value.code == NO_DEVICE
                assert pkg.last_groups() == [] and pkg.last_strided()[:3] == (0, 0, 0)
                f.close()
        except BaseException as e:   # noqa: B036 (handed to the test's thread below)
            failures.append(e)

    t = threading.Thread(target=in_a_fresh_thread)
    t.start()
    t.join()
    if failures:
        raise failures[0]


def _call(pkg, f, src_steps, dst_steps, src=(256, 512, 768, 1024), dst=(4096, 8192, 12288, 16384)):
    n = f.fmt.planes
    f.process_device_strided(list(src)[:n], [4096] * n, src_steps, [0] * n, list(dst)[:n], [8192] * n, dst_steps, [0] * n, 1)


@pytest.mark.parametrize("fmt", ["YUV420P8", "RGBAP16", "RGBPS", "RGBPH"])
def test_null_and_step_checks_come_before_the_device_check(pkg, fmt):
    f = pkg.Filter(pkg.FORMATS[fmt], 40, 24, 61, 37, device=-1)
    n = f.fmt.planes
    ones = [1] * n
    for bad in (0, 5, -1):
        for side in (0, 1):
            for plane in range(n):
                steps = list(ones)
                steps[plane] = bad
                with pytest.raises(pkg.JincError) as e:
                    _call(pkg, f, steps if side == 0 else ones, ones if side == 0 else steps)
                assert e.value.code == INVALID_ARG and str(e.value).startswith("JincResize:") and "step" in str(e.value), (bad, side, plane)
    L = pkg.lib()
    P4, I4 = C.c_void_p * 4, C.c_int * 4
    good = dict(src=P4(256, 512, 768, 1024), sp=I4(64, 64, 64, 64), dst=P4(4096, 8192, 12288, 16384), dp=I4(64, 64, 64, 64))
    for missing in ("src", "sp", "dst", "dp"):
        a = dict(good)
        a[missing] = None
        rc = L.jinc_filter_process_device_strided(f._h, a["src"], a["sp"], None, None, a["dst"], a["dp"], None, None, 1, None)
        assert rc == INVALID_ARG and L.jinc_last_error().decode().startswith("JincResize:"), missing
    assert L.jinc_filter_process_device_strided(None, good["src"], good["sp"], None, None, good["dst"], good["dp"], None, None, 1, None) == INVALID_ARG
    for steps in (None, ones, [2] * n, [4] * n, [1] + [2] * (n - 1), [3] * n):
        for dsteps in (None, steps):
            with pytest.raises(pkg.JincError) as e:
                _call(pkg, f, steps, dsteps)
            assert e.value.code == NO_DEVICE, (steps, dsteps)
    f.close()


# ---- grouping ------------------------------------------------------------------------------------------------------------------------

def _model(bases, pitches, steps, strides, widths, heights, sb):
    """The grouping as include/jincresize_hip_test.h words it, written down independently: planes in order; a strided plane joins the
    first group whose planes have its step, pitch, frame stride and dimensions and with which it still fits one N-sample pixel
    (lowest to highest base less than N samples, whole samples apart, no base twice); else it opens a group.  A plane's channel is
    its distance from the group's lowest base in samples."""
    groups, group_of = [], []
    for i, b in enumerate(bases):
        if steps[i] <= 1:
            group_of.append(-1)
            continue
        for g, members in enumerate(groups):
            j = members[0]
            if (steps[j], pitches[j], strides[j], widths[j], heights[j]) != (steps[i], pitches[i], strides[i], widths[i], heights[i]):
                continue
            all_b = [bases[k] for k in members] + [b]
            if max(all_b) - min(all_b) < steps[i] * sb and all((x - min(all_b)) % sb == 0 for x in all_b) and b not in all_b[:-1]:
                members.append(i)
                group_of.append(g)
                break
        else:
            groups.append([i])
            group_of.append(len(groups) - 1)
    channel_of = [-1 if g < 0 else (bases[i] - min(bases[k] for k in groups[g])) // sb for i, g in enumerate(group_of)]
    return len(groups), group_of, channel_of


def _check(pkg, bases, pitches, steps, strides, widths, heights, sb, expect_groups=None, expect_group_of=None, expect_channels=None):
    got = pkg.strided_groups(bases, pitches, steps, strides, widths, heights, sb)
    want = _model(bases, pitches, steps, strides, widths, heights, sb)
    assert got == want, (got, want, bases, pitches, steps, strides)
    if expect_groups is not None:
        assert got[0] == expect_groups, (got, bases)
    if expect_group_of is not None:
        assert got[1] == expect_group_of, (got, bases)
    if expect_channels is not None:
        assert got[2] == expect_channels, (got, bases)
    # properties: groups are numbered in order of their first plane; channels inside a group are distinct and below the step
    n, group_of, channel_of = got
    firsts = [group_of.index(g) for g in range(n)]
    assert firsts == sorted(firsts)
    for g in range(n):
        ch = [channel_of[i] for i in range(len(bases)) if group_of[i] == g]
        st = {steps[i] for i in range(len(bases)) if group_of[i] == g}
        assert len(st) == 1 and len(set(ch)) == len(ch) and min(ch) == 0 and max(ch) < st.pop()
    return got


def test_channel_groups_over_random_layouts(pkg):
    rng = np.random.default_rng(20261017)
    for trial in range(300):
        sb = int(rng.choice([1, 2, 4]))
        w, h = int(rng.integers(1, 500)), int(rng.integers(1, 300))
        cw, ch = (w + 1) // 2, (h + 1) // 2
        y = int(rng.integers(1, 1 << 40)) * sb
        uv = int(rng.integers(1, 1 << 40)) * sb
        pitch = int(rng.integers(cw * 2, cw * 2 + 64)) * sb
        fs = int(rng.integers(0, 1 << 24)) * sb
        ypitch = w * sb + 8 * sb
        # NV12 / P010 / P016, and NV21 (V first)
        for u, v, chans in ((uv, uv + sb, [-1, 0, 1]), (uv + sb, uv, [-1, 1, 0])):
            _check(pkg, [y, u, v], [ypitch, pitch, pitch], [1, 2, 2], [fs, fs, fs], [w, cw, cw], [h, ch, ch], sb, 1, [-1, 0, 0], chans)
        # the six channel orders of RGB24 (planes G, B, R): one group of three at step 3
        p = int(rng.integers(1, 1 << 40)) * sb
        for order in itertools.permutations(range(3)):
            bases = [p + c * sb for c in order]
            _check(pkg, bases, [pitch] * 3, [3] * 3, [fs] * 3, [w] * 3, [h] * 3, sb, 1, [0, 0, 0], list(order))
        # BGRA with A (G, B, R, A = p + 1, p, p + 2, p + 3) and BGRX without
        _check(pkg, [p + sb, p, p + 2 * sb, p + 3 * sb], [pitch] * 4, [4] * 4, [fs] * 4, [w] * 4, [h] * 4, sb, 1, [0] * 4, [1, 0, 2, 3])
        _check(pkg, [p + sb, p, p + 2 * sb], [pitch] * 3, [4] * 3, [fs] * 3, [w] * 3, [h] * 3, sb, 1, [0] * 3, [1, 0, 2])
        # two unrelated strided planes (far apart) and a dense one
        q = p + int(rng.integers(64, 1 << 20)) * sb
        _check(pkg, [y, p, q], [ypitch, pitch, pitch], [1, 2, 2], [fs] * 3, [w, cw, cw], [h, ch, ch], sb, 2, [-1, 0, 1], [-1, 0, 0])
        # equal steps but another pitch / another frame stride / other dimensions: not grouped
        _check(pkg, [y, uv, uv + sb], [ypitch, pitch, pitch + sb], [1, 2, 2], [fs] * 3, [w, cw, cw], [h, ch, ch], sb, 2, [-1, 0, 1], [-1, 0, 0])
        _check(pkg, [y, uv, uv + sb], [ypitch, pitch, pitch], [1, 2, 2], [fs, fs, fs + sb], [w, cw, cw], [h, ch, ch], sb, 2, [-1, 0, 1], [-1, 0, 0])
        _check(pkg, [y, uv, uv + sb], [ypitch, pitch, pitch], [1, 2, 2], [fs] * 3, [w, cw, cw + 1], [h, ch, ch], sb, 2, [-1, 0, 1], [-1, 0, 0])
        # different steps: not grouped
        _check(pkg, [y, uv, uv + sb], [ypitch, pitch, pitch], [1, 2, 4], [fs] * 3, [w, cw, cw], [h, ch, ch], sb, 2, [-1, 0, 1], [-1, 0, 0])
        # bases one pixel apart (and further): not grouped; the same base twice: not grouped
        for step in (2, 3, 4):
            for d in (step, step + 1, -step, 7 * step):
                _check(pkg, [p, p + d * sb], [pitch] * 2, [step] * 2, [fs] * 2, [w] * 2, [h] * 2, sb, 2, [0, 1], [0, 0])
            _check(pkg, [p, p], [pitch] * 2, [step] * 2, [fs] * 2, [w] * 2, [h] * 2, sb, 2, [0, 1], [0, 0])
            _check(pkg, [p, p + (step - 1) * sb], [pitch] * 2, [step] * 2, [fs] * 2, [w] * 2, [h] * 2, sb, 1, [0, 0], [0, step - 1])
        if sb > 1:   # a fraction of a sample apart: not one pixel's channels
            _check(pkg, [p, p + 1], [pitch] * 2, [4] * 2, [fs] * 2, [w] * 2, [h] * 2, sb, 2, [0, 1], [0, 0])
        # anything: random steps and bases near each other
        n = int(rng.integers(1, 5))
        steps = [int(rng.integers(1, 5)) for _ in range(n)]
        bases = [p + int(rng.integers(-5, 6)) * sb for _ in range(n)]
        pitches = [pitch + int(rng.integers(0, 2)) * sb for _ in range(n)]
        _check(pkg, bases, pitches, steps, [fs] * n, [w] * n, [h] * n, sb)
    # NULL step / frame-stride arrays: all dense, no groups
    assert pkg.strided_groups([64, 128], [32, 32], None, None, [8, 8], [8, 8], 1) == (0, [-1, -1], [-1, -1])
    assert pkg.strided_groups([64, 65], [32, 32], [2, 2], None, [8, 8], [8, 8], 1) == (1, [0, 0], [0, 1])
