"""Host side of jinc_filter_process_device_widened_packed10 / _v210 (Y410 / RGB10A2 words and v210 blocks into fp32 / binary16
filters): the exports, the mirror and the header; every refusal that needs no device, each with a message of its own, on filters
created with device = -1; and the row functions of widen_fields_kernel and widen_v210_kernel (csrc/widen_fields_rows.h,
csrc/widen_v210_rows.h) in stand-alone host programs (tests/host_sanitizer/widen_fields_rows_main.cpp, widen_v210_rows_main.cpp:
their own main; nothing is loaded into Python), built once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer,
whose output is compared with numpy's field.astype(float32 | float16) bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

INVALID_ARG, NO_DEVICE = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "avisynth-jincresize_amd")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
GEOM = (40, 24, 80, 48)
Y410, BGRX1010102, ODD = [10, 0, 20], [12, 22, 2], [22, 0, 11]   # ODD: a legal word no format uses, spare bits 10 and 21
ROW_V210 = 16 * ((40 + 5) // 6)   # 112 bytes


def test_the_entries_are_exported_declared_and_mirrored(pkg):
    header = open(pkg.HEADER_PATH).read()
    for name, method in (("jinc_filter_process_device_widened_packed10", "process_device_widened_packed10"),
                         ("jinc_filter_process_device_widened_v210", "process_device_widened_v210")):
        assert name in pkg.EXPORTS and hasattr(pkg.lib(), name)
        assert name + "(" in header
        assert hasattr(pkg.Filter, method)
    assert "are not taken as widened sources" not in header
    assert pkg.packed10_layout("Y410")[0] == Y410 and pkg.packed10_layout("BGRX1010102")[0] == BGRX1010102


# ---- the argument surface --------------------------------------------------------------------------------------------------------------

def _call(f, kind, offsets=Y410, ptr=4096, pitch=None, stride=0, dst_steps=None, nframes=1):
    """A 40 x 24 source unless told otherwise; the pointers are never dereferenced."""
    n = f.fmt.planes
    dst = ([1 << 20, 2 << 20, 3 << 20, 4 << 20][:n], [512] * n, dst_steps, [1 << 18] * n, nframes)
    if kind == "packed10":
        f.process_device_widened_packed10(ptr, 160 if pitch is None else pitch, offsets, stride, *dst)
    else:
        f.process_device_widened_v210(ptr, 128 if pitch is None else pitch, stride, *dst)


# (call, filter, call arguments, what the message must say)
REFUSALS = [
    ("packed10", "YUV444P10", dict(), "fp32 or binary16 filter"),
    ("packed10", "RGBP8", dict(), "fp32 or binary16 filter"),
    ("packed10", "RGBAPS", dict(), "three components"),
    ("packed10", "YUV420PS", dict(), "three components"),
    ("packed10", "YUV422PH", dict(), "three components"),
    ("packed10", "Y32", dict(), "three components"),
    ("packed10", "YUV444PS", dict(offsets=[-1, 10, 20]), "0..22"),
    ("packed10", "YUV444PS", dict(offsets=[10, 0, 23]), "0..22"),
    ("packed10", "YUV444PH", dict(offsets=[10, 0, 19]), "overlap"),
    ("packed10", "RGBPS", dict(offsets=[5, 5, 20]), "overlap"),
    ("packed10", "YUV444PS", dict(dst_steps=[1, 5, 1]), "step"),
    ("packed10", "RGBPS", dict(dst_steps=[0, 3, 3]), "step"),
    ("packed10", "YUV444PS", dict(ptr=4098), "aligned"),
    ("packed10", "YUV444PS", dict(pitch=162), "pitch 162 "),
    ("packed10", "YUV444PS", dict(stride=160 * 24 + 2, nframes=2), "frame stride"),
    ("packed10", "YUV444PS", dict(pitch=156), "pitch 156 "),
    ("v210", "YUV422P10", dict(), "fp32 or binary16 filter"),
    ("v210", "YUV422P8", dict(), "fp32 or binary16 filter"),
    ("v210", "YUVA422PS", dict(), "three components"),
    ("v210", "YUV444PS", dict(), "three components"),
    ("v210", "YUV420PH", dict(), "three components"),
    ("v210", "Y32", dict(), "three components"),
    ("v210", "YUV422PS", dict(dst_steps=[1, 1, 5]), "step"),
    ("v210", "YUV422PH", dict(dst_steps=[0, 1, 1]), "step"),
    ("v210", "YUV422PS", dict(ptr=4097), "aligned"),
    ("v210", "YUV422PS", dict(pitch=114), "pitch 114 "),
    ("v210", "YUV422PS", dict(stride=128 * 24 + 2, nframes=2), "frame stride"),
    ("v210", "YUV422PS", dict(pitch=ROW_V210 - 4), f"pitch {ROW_V210 - 4} "),
]
IDS = [f"{kind}_{name}_{'_'.join(f'{k}_{v}' for k, v in kw.items()) or 'filter'}".replace(" ", "").replace("[", "").replace("]", "").replace(",", "_")
       for kind, name, kw, _ in REFUSALS]


@pytest.mark.parametrize("kind,name,kw,says", REFUSALS, ids=IDS)
def test_refusals_come_before_the_device_check(pkg, kind, name, kw, says):
    sw, sh, tw, th = GEOM
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1)
    with pytest.raises(pkg.JincError) as e:
        _call(f, kind, **kw)
    assert e.value.code == INVALID_ARG and str(e.value).startswith("JincResize:") and says in str(e.value), str(e.value)
    f.close()


def test_every_refusal_has_a_message_of_its_own(pkg):
    sw, sh, tw, th = GEOM
    messages = []
    for kind, name, kw, _ in REFUSALS:
        f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1)
        with pytest.raises(pkg.JincError):
            _call(f, kind, **kw)
        messages.append(pkg.lib().jinc_last_error().decode())
        f.close()
    assert len(set(messages)) == len(REFUSALS), sorted(messages)


ACCEPTED = [
    ("packed10", "YUV444PS", dict()),
    ("packed10", "YUV444PH", dict()),
    ("packed10", "RGBPS", dict(offsets=BGRX1010102, dst_steps=[3, 3, 3])),
    ("packed10", "RGBPH", dict(offsets=ODD)),
    ("packed10", "YUV444PS", dict(pitch=164, ptr=4100, stride=164 * 24 + 4, nframes=2)),   # multiples of 4 only
    ("packed10", "YUV444PS", dict(stride=2)),                                             # one frame: the frame stride is not read
    ("v210", "YUV422PS", dict()),
    ("v210", "YUV422PH", dict()),
    ("v210", "YUV422PS", dict(pitch=ROW_V210)),                                           # the smallest pitch
    ("v210", "YUV422PS", dict(pitch=ROW_V210 + 4, ptr=4100, stride=(ROW_V210 + 4) * 24 + 4, nframes=2)),
    ("v210", "YUV422PH", dict(stride=2, dst_steps=[1, 2, 2])),
]


@pytest.mark.parametrize("kind,name,kw", ACCEPTED, ids=[f"{k}_{n}_{i}" for i, (k, n, _) in enumerate(ACCEPTED)])
def test_accepted_arguments_reach_the_device_check(pkg, kind, name, kw):
    sw, sh, tw, th = GEOM
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1)
    with pytest.raises(pkg.JincError) as e:
        _call(f, kind, **kw)
    assert e.value.code == NO_DEVICE, str(e.value)
    f.close()


def test_null_arguments_come_after_the_refusals(pkg):
    sw, sh, tw, th = GEOM
    L = pkg.lib()
    last = lambda: L.jinc_last_error().decode()
    off, bad_off = (C.c_int * 3)(*Y410), (C.c_int * 3)(10, 0, 23)
    f = pkg.Filter(pkg.FORMATS["YUV444PS"], sw, sh, tw, th, device=-1)
    call = L.jinc_filter_process_device_widened_packed10
    assert call(f._h, C.c_void_p(4096), 160, off, 0, None, None, None, None, 1, C.c_void_p(0)) == INVALID_ARG and "null argument" in last()
    assert call(f._h, None, 160, off, 0, None, None, None, None, 1, C.c_void_p(0)) == INVALID_ARG and "null argument" in last()
    assert call(f._h, C.c_void_p(4096), 160, None, 0, None, None, None, None, 1, C.c_void_p(0)) == INVALID_ARG and "null argument" in last()
    assert call(f._h, C.c_void_p(4096), 160, bad_off, 0, None, None, None, None, 1, C.c_void_p(0)) == INVALID_ARG and "0..22" in last()
    assert call(f._h, C.c_void_p(4096), 156, off, 0, None, None, None, None, 1, C.c_void_p(0)) == INVALID_ARG and "pitch 156 " in last()
    f.close()
    f = pkg.Filter(pkg.FORMATS["YUV422PS"], sw, sh, tw, th, device=-1)
    call = L.jinc_filter_process_device_widened_v210
    assert call(f._h, C.c_void_p(4096), 128, 0, None, None, None, None, 1, C.c_void_p(0)) == INVALID_ARG and "null argument" in last()
    assert call(f._h, None, 128, 0, None, None, None, None, 1, C.c_void_p(0)) == INVALID_ARG and "null argument" in last()
    assert call(f._h, C.c_void_p(4098), 128, 0, None, None, None, None, 1, C.c_void_p(0)) == INVALID_ARG and "aligned" in last()
    f.close()


# ---- the row functions -------------------------------------------------------------------------------------------------------------------

def _build_and_run(tmp_path, program, tag, extra):
    for header in ("widen_fields_rows.h", "widen_v210_rows.h"):
        assert os.path.exists(os.path.join(PKG, "csrc", header)), f"csrc/{header} is missing"
    exe, out_file = str(tmp_path / f"{program}_{tag}"), str(tmp_path / f"{program}_{tag}.bin")
    subprocess.run([CXX, "-g", "-std=c++17", "-ffp-contract=off", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", *extra,
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "host_sanitizer", program + "_main.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, out_file], capture_output=True, text=True, env=env, timeout=900)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out and "LeakSanitizer" not in out, out[-4000:]
    return out, np.fromfile(out_file, np.uint8)


def _converted(values, ob):
    return values.astype(np.float32).view(np.uint32) if ob == 4 else values.astype(np.float16).view(np.uint16)


FIELD_WIDTHS = {1, 7, 8, 9, 63, 64, 65, 513, 1031}


def _check_fields_against_numpy(out, blob):
    pos, cases, seen, dirty = 0, 0, set(), 0
    while pos < blob.size:
        ob, width, rows, unit, o0, o1, o2, *_ = blob[pos:pos + 64].view(np.uint32).tolist()
        pos += 64
        words = blob[pos:pos + rows * width * 4].view("<u4").reshape(rows, width)
        pos += rows * width * 4
        mask = sum(1023 << o for o in (o0, o1, o2))
        dirty += int(np.count_nonzero(words & np.uint32(~mask & 0xFFFFFFFF)))
        for c, o in enumerate((o0, o1, o2)):
            got = blob[pos:pos + rows * width * ob].view(np.uint32 if ob == 4 else np.uint16).reshape(rows, width)
            pos += rows * width * ob
            want = _converted((words >> np.uint32(o)) & np.uint32(1023), ob)
            assert np.array_equal(got, want), f"OB {ob} width {width} unit {unit} offsets {(o0, o1, o2)}: plane {c} differs at {int((got != want).sum())} samples"
        seen.add((ob, unit, (o0, o1, o2), width))
        cases += 1
    assert pos == blob.size
    assert f"widen fields rows: {cases} cases, 0 wrong" in out, out[-2000:]
    assert dirty > 0, "the source bits outside the fields are not dirty"
    for ob in (4, 2):
        for unit in (16, 4):
            for offsets in (Y410, BGRX1010102, ODD):
                assert {w for (a, u, o, w) in seen if (a, u, o) == (ob, unit, tuple(offsets))} == FIELD_WIDTHS, (ob, unit, offsets)
    return cases


# (plane, sample of the block, word, bit offset) of a v210 block's twelve fields, from the table in include/jincresize_hip.h
V210_FIELDS = [(1, 0, 0, 0), (0, 0, 0, 10), (2, 0, 0, 20),
               (0, 1, 1, 0), (1, 1, 1, 10), (0, 2, 1, 20),
               (2, 1, 2, 0), (0, 3, 2, 10), (1, 2, 2, 20),
               (0, 4, 3, 0), (2, 2, 3, 10), (0, 5, 3, 20)]


def _check_v210_against_numpy(out, blob):
    pos, cases, seen = 0, 0, set()
    while pos < blob.size:
        ob, width, rows, unit, *_ = blob[pos:pos + 64].view(np.uint32).tolist()
        pos += 64
        nblocks = (width + 5) // 6
        words = blob[pos:pos + rows * nblocks * 16].view("<u4").reshape(rows, nblocks, 4)
        pos += rows * nblocks * 16
        widths = (width, width // 2, width // 2)
        want = [np.zeros((rows, w), np.uint32) for w in widths]
        for plane, j, word, offset in V210_FIELDS:
            x = (6 if plane == 0 else 3) * np.arange(nblocks) + j
            valid = x < widths[plane]
            want[plane][:, x[valid]] = (words[:, valid, word] >> np.uint32(offset)) & np.uint32(1023)
        for plane, w in enumerate(widths):
            got = blob[pos:pos + rows * w * ob].view(np.uint32 if ob == 4 else np.uint16).reshape(rows, w)
            pos += rows * w * ob
            assert np.array_equal(got, _converted(want[plane], ob)), f"OB {ob} width {width} rows {rows} unit {unit}: plane {plane} differs"
        seen.add((ob, unit, rows, width))
        cases += 1
    assert pos == blob.size
    assert f"widen v210 rows: {cases} cases, 0 wrong" in out, out[-2000:]
    assert seen == {(ob, unit, rows, width) for ob in (4, 2) for unit in (16, 4) for rows in (1, 2, 3) for width in range(2, 801, 2)}
    return cases


PROGRAMS = [("widen_fields_rows", _check_fields_against_numpy), ("widen_v210_rows", _check_v210_against_numpy)]


@pytest.mark.parametrize("program,check", PROGRAMS, ids=[p for p, _ in PROGRAMS])
def test_row_functions_equal_numpy(tmp_path, program, check):
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not found")
    out, blob = _build_and_run(tmp_path, program, "plain", ["-O2"])
    print(check(out, blob), "cases")


@pytest.mark.parametrize("program,check", PROGRAMS, ids=[p for p, _ in PROGRAMS])
def test_row_functions_are_clean_under_asan_ubsan(tmp_path, program, check):
    """The same programs as stand-alone executables with -fsanitize=address,undefined: nothing preloaded, nothing loaded into Python.
    Their buffers end where the contract says the accesses end."""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not found")
    out, blob = _build_and_run(tmp_path, program, "san", ["-O1", "-fsanitize=address,undefined"])
    print(check(out, blob), "cases")
