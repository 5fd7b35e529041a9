"""Host side of jinc_filter_process_device_widened_packed10_scaled / _widened_v210_scaled (Y410 / RGB10A2 words and v210 blocks into
fp32 / binary16 / bfloat16 filters with a scale and an offset per plane): the exports, the mirror and the headers; every refusal
that needs no device on filters created with device = -1 -- the unscaled calls' refusals with their texts, first; then the pairs,
with messages that name the plane; bfloat16 filters refused with the unscaled text when both arrays are NULL and accepted when one
is given -- and the SCALED row functions of widen_fields_kernel and widen_v210_kernel (csrc/widen_fields_rows.h,
csrc/widen_v210_rows.h) in stand-alone host programs (tests/host_sanitizer/widen_fields_scaled_rows_main.cpp,
widen_v210_scaled_rows_main.cpp: their own main; nothing is loaded into Python), built once plain and once under AddressSanitizer +
UndefinedBehaviorSanitizer, whose output numpy checks bit for bit against s = fl32(fl32(float(v) * scale) + offset), narrowed per
type, together with the bytes behind every row."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_scaled_host import BF16, HALF, INF, NAN, widened_definition
from test_widened_words_host import REFUSALS as OLD_REFUSALS
from test_widened_words_host import ROW_V210, V210_FIELDS, Y410
from test_widened_words_host import _call as old_call

INVALID_ARG, NO_DEVICE = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "avisynth-jincresize_amd")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
GEOM = (40, 24, 80, 48)
SIDE = {"packed10": "packed 10-bit source", "v210": "v210 source"}


def test_the_entries_are_exported_declared_and_mirrored(pkg):
    header, test_header = open(pkg.HEADER_PATH).read(), open(pkg.TEST_HEADER_PATH).read()
    for name in ("jinc_filter_process_device_widened_packed10_scaled", "jinc_filter_process_device_widened_v210_scaled"):
        assert name in pkg.EXPORTS and hasattr(pkg.lib(), name), name
        assert name + "(" in header, name
        assert hasattr(pkg.Filter, name[len("jinc_filter_"):]), name
    for name in ("jinc_debug_widen_fields", "jinc_debug_widen_v210"):
        assert name in pkg.EXPORTS and hasattr(pkg.lib(), name), name
        assert name + "(" in test_header and name + "(" not in header, name
        assert callable(getattr(pkg, name[len("jinc_"):])), name


# ---- the argument surface --------------------------------------------------------------------------------------------------------------

def _call(f, kind, scales=None, offsets_add=None, offsets=Y410, ptr=4096, pitch=None, stride=0, dst_steps=None, nframes=1):
    """test_widened_words_host._call with the two arrays: a 40 x 24 source; the pointers are never dereferenced."""
    n = f.fmt.planes
    dst = ([1 << 20, 2 << 20, 3 << 20, 4 << 20][:n], [512] * n, dst_steps, [1 << 18] * n, nframes)
    if kind == "packed10":
        f.process_device_widened_packed10_scaled(ptr, 160 if pitch is None else pitch, offsets, scales, offsets_add, stride, *dst)
    else:
        f.process_device_widened_v210_scaled(ptr, 128 if pitch is None else pitch, scales, offsets_add, stride, *dst)


FILTERS = {"packed10": ("YUV444PS", "YUV444PH", "YUV444PBF", "RGBPBF"), "v210": ("YUV422PS", "YUV422PH", "YUV422PBF")}

# (id, scales, offsets, the plane at fault, which, how)
NEW_REFUSALS = [
    ("scale_nan", [1.0, NAN, 1.0], None, 1, "scale", "NaN"),
    ("scale_inf", [INF, 1.0, 1.0], None, 0, "scale", "infinite"),
    ("scale_minus_inf", [1.0, 1.0, -INF], [0.0] * 3, 2, "scale", "infinite"),
    ("scale_zero", [1.0, 1.0, 0.0], None, 2, "scale", "zero"),
    ("scale_minus_zero", [-0.0, 1.0, 1.0], [0.5] * 3, 0, "scale", "zero"),
    ("offset_nan", None, [0.0, 0.0, NAN], 2, "offset", "NaN"),
    ("offset_inf", [2.0] * 3, [0.0, INF, 0.0], 1, "offset", "infinite"),
    ("offset_minus_inf", None, [-INF, 0.0, 0.0], 0, "offset", "infinite"),
]


@pytest.mark.parametrize("case", NEW_REFUSALS, ids=[c[0] for c in NEW_REFUSALS])
@pytest.mark.parametrize("kind", ["packed10", "v210"])
def test_bad_pairs_are_refused_before_the_device_check_and_name_the_plane(pkg, kind, case):
    _, scales, offsets, plane, which, how = case
    sw, sh, tw, th = GEOM
    for name in FILTERS[kind]:
        f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1)
        before = (pkg.last_strided(), pkg.last_groups())
        with pytest.raises(pkg.JincError) as e:
            _call(f, kind, scales, offsets)
        text = str(e.value)
        assert e.value.code == INVALID_ARG and text.startswith("JincResize:"), text
        assert f"the {which} of {SIDE[kind]} plane {plane} is {how}" in text, text
        assert (pkg.last_strided(), pkg.last_groups()) == before   # (refused on its arguments: both records as they were)
        f.close()


def test_every_new_refusal_has_a_message_of_its_own(pkg):
    sw, sh, tw, th = GEOM
    messages = []
    for kind in ("packed10", "v210"):
        f = pkg.Filter(pkg.FORMATS[FILTERS[kind][0]], sw, sh, tw, th, device=-1)
        for _, scales, offsets, *_ in NEW_REFUSALS:
            with pytest.raises(pkg.JincError):
                _call(f, kind, scales, offsets)
            messages.append(pkg.lib().jinc_last_error().decode())
        f.close()
    # (what is wrong, with which value, of which plane, on which surface: no two cases share all four)
    assert len(set(messages)) == 2 * len(NEW_REFUSALS), sorted(messages)


def test_a_bad_pair_comes_before_the_null_checks_and_behind_the_unscaled_refusals(pkg):
    sw, sh, tw, th = GEOM
    L = pkg.lib()
    last = lambda: L.jinc_last_error().decode()
    F3 = C.c_float * 3
    off = (C.c_int * 3)(*Y410)
    f = pkg.Filter(pkg.FORMATS["YUV444PBF"], sw, sh, tw, th, device=-1)
    call = L.jinc_filter_process_device_widened_packed10_scaled
    # plane arrays NULL and a bad scale: the scale is named; a good pair: the null check
    assert call(f._h, C.c_void_p(4096), 160, off, F3(1, 0, 1), None, 0, None, None, None, None, 1, C.c_void_p(0)) == INVALID_ARG and "plane 1 is zero" in last()
    assert call(f._h, C.c_void_p(4096), 160, off, F3(1, 2, 3), None, 0, None, None, None, None, 1, C.c_void_p(0)) == INVALID_ARG and "null argument" in last()
    assert call(f._h, C.c_void_p(4096), 160, None, F3(1, 2, 3), None, 0, None, None, None, None, 1, C.c_void_p(0)) == INVALID_ARG and "null argument" in last()
    # a refusal of the unscaled call beside a bad pair: the unscaled call's comes first
    assert call(f._h, C.c_void_p(4096), 156, off, F3(NAN, 0, 1), None, 0, None, None, None, None, 1, C.c_void_p(0)) == INVALID_ARG and "pitch 156 " in last()
    f.close()
    f = pkg.Filter(pkg.FORMATS["YUV422PBF"], sw, sh, tw, th, device=-1)
    call = L.jinc_filter_process_device_widened_v210_scaled
    assert call(f._h, C.c_void_p(4096), 128, None, F3(0, INF, 0), 0, None, None, None, None, 1, C.c_void_p(0)) == INVALID_ARG and "offset of v210 source plane 1 is infinite" in last()
    assert call(f._h, C.c_void_p(4096), 128, None, F3(0, 1, 0), 0, None, None, None, None, 1, C.c_void_p(0)) == INVALID_ARG and "null argument" in last()
    assert call(f._h, C.c_void_p(4098), 128, F3(0, 1, 1), None, 0, None, None, None, None, 1, C.c_void_p(0)) == INVALID_ARG and "aligned" in last()
    f.close()


ARRAYS = {"both_null": dict(), "scale_given": dict(scales=[0.5, 0.25, -2.0]), "offset_given": dict(offsets_add=[0.25, -0.5, 1.0]),
          "bad_scale_given": dict(scales=[NAN, 0.0, INF])}


@pytest.mark.parametrize("arrays", sorted(ARRAYS))
def test_every_refusal_of_the_unscaled_calls_keeps_its_text(pkg, arrays):
    """The refusals of test_widened_words_host.py through the scaled entries: the same code and the same text as the unscaled entry
    gives, whether the arrays are NULL or given -- they come first, in front of a bad scale too."""
    sw, sh, tw, th = GEOM
    for kind, name, kw, says in OLD_REFUSALS:
        f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1)
        with pytest.raises(pkg.JincError):
            old_call(f, kind, **kw)
        old = pkg.lib().jinc_last_error().decode()
        with pytest.raises(pkg.JincError) as e:
            _call(f, kind, **ARRAYS[arrays], **kw)
        assert e.value.code == INVALID_ARG and pkg.lib().jinc_last_error().decode() == old and says in old, (kind, name, kw, str(e.value), old)
        f.close()


@pytest.mark.parametrize("kind,name", [("packed10", "YUV444PBF"), ("packed10", "RGBPBF"), ("v210", "YUV422PBF")])
def test_bfloat16_is_refused_with_null_arrays_and_accepted_with_one_given(pkg, kind, name):
    sw, sh, tw, th = GEOM
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1)
    with pytest.raises(pkg.JincError) as e:
        old_call(f, kind)
    old = str(e.value)
    assert e.value.code == INVALID_ARG and "bfloat16" in old and "not exact" in old, old
    with pytest.raises(pkg.JincError) as e:
        _call(f, kind)   # both arrays NULL: the call IS the unscaled call
    assert e.value.code == INVALID_ARG and str(e.value) == old, str(e.value)
    for arrays in (dict(scales=[0.5, 0.25, -2.0]), dict(offsets_add=[0.0, -0.5, 1.0]), dict(scales=[1.0] * 3, offsets_add=[0.0] * 3)):
        with pytest.raises(pkg.JincError) as e:
            _call(f, kind, **arrays)   # past every argument check: the device check is what stops it
        assert e.value.code == NO_DEVICE, str(e.value)
    f.close()


ACCEPTED = [
    ("packed10", "YUV444PS", dict(scales=[1 / 876, 1 / 896, -1 / 896])),
    ("packed10", "YUV444PH", dict(offsets_add=[0.0, -0.5, 0.5])),
    ("packed10", "RGBPBF", dict(scales=[1 / 1023] * 3, offsets=[12, 22, 2], dst_steps=[3, 3, 3])),
    ("packed10", "YUV444PS", dict(scales=[2.0] * 3, pitch=164, ptr=4100, stride=164 * 24 + 4, nframes=2)),
    ("v210", "YUV422PS", dict(scales=[1 / 876, 1 / 896, -1 / 896], offsets_add=[-16 / 219, -0.5, 0.5])),
    ("v210", "YUV422PH", dict(offsets_add=[1.0, 2.0, 3.0], pitch=ROW_V210)),
    ("v210", "YUV422PBF", dict(scales=[1e-3, -1e3, 7.0], stride=2, dst_steps=[1, 2, 2])),
    ("packed10", "YUV444PS", dict()),   # both NULL: the unscaled call, accepted as there
    ("v210", "YUV422PH", dict()),
]


@pytest.mark.parametrize("kind,name,kw", ACCEPTED, ids=[f"{k}_{n}_{i}" for i, (k, n, _) in enumerate(ACCEPTED)])
def test_accepted_arguments_reach_the_device_check(pkg, kind, name, kw):
    sw, sh, tw, th = GEOM
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1)
    before = (pkg.last_strided(), pkg.last_groups())
    with pytest.raises(pkg.JincError) as e:
        _call(f, kind, **kw)
    assert e.value.code == NO_DEVICE, str(e.value)
    assert (pkg.last_strided(), pkg.last_groups()) == before
    f.close()


def test_the_hooks_refuse_bad_arguments_without_a_device(pkg):
    words, blocks = np.zeros(8, np.uint32), np.zeros(8, np.uint32)
    for bad in (dict(scale=[1.0, 0.0, 1.0]), dict(offset=[0.0, NAN, 0.0]), dict(scale=[INF, 1.0, 1.0]), dict(out_kind=pkg.SAMPLE_BFLOAT16)):
        with pytest.raises(pkg.JincError) as e:
            pkg.debug_widen_fields(words, Y410, **bad)
        assert e.value.code == INVALID_ARG
        with pytest.raises(pkg.JincError) as e:
            pkg.debug_widen_v210(blocks, 12, **bad)
        assert e.value.code == INVALID_ARG
    with pytest.raises(pkg.JincError):
        pkg.debug_widen_fields(words, [10, 0, 19], scale=[1.0] * 3)
    assert [p.size for p in pkg.debug_widen_fields(np.zeros(0, np.uint32), Y410, scale=[1.0] * 3)] == [0, 0, 0]


# ---- the row functions -------------------------------------------------------------------------------------------------------------------

def _build_and_run(tmp_path, program, tag, extra):
    exe, out_file = str(tmp_path / f"{program}_{tag}"), str(tmp_path / f"{program}_{tag}.bin")
    subprocess.run([CXX, "-g", "-std=c++17", "-ffp-contract=off", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", *extra,
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "host_sanitizer", program + "_main.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, out_file], capture_output=True, text=True, env=env, timeout=900)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out and "LeakSanitizer" not in out, out[-4000:]
    return out, np.fromfile(out_file, np.uint8)


def _plane(blob, pos, rows, width, pitch, ob, what):
    """A plane written row by row with its padding (the last row without): (samples, new position); the padding must hold the canary."""
    size = pitch * (rows - 1) + width * ob
    raw = blob[pos:pos + size]
    padded = np.full(pitch * rows, 0xA5, np.uint8)
    padded[:size] = raw
    padded = padded.reshape(rows, pitch)
    assert (padded[:, width * ob:] == 0xA5).all(), f"{what}: bytes behind the row's {width} samples were stored to"
    return np.ascontiguousarray(padded[:, :width * ob]).view(np.uint32 if ob == 4 else np.uint16), pos + size


def _floats(bits):
    return np.array(bits, np.uint32).view(np.float32)


def _check_fields_against_numpy(out, blob):
    pos, cases, seen, pair_sets, specials = 0, 0, set(), set(), dict(inf=0, subnormal=0)
    while pos < blob.size:
        head = blob[pos:pos + 64].view(np.uint32).tolist()
        kind, width, rows, unit, o0, o1, o2 = head[:7]
        scales, offsets, pitch = _floats(head[7:10]), _floats(head[10:13]), head[13]
        pos += 64
        ob = 4 if kind == 0 else 2
        words = blob[pos:pos + rows * width * 4].view("<u4").reshape(rows, width)
        pos += rows * width * 4
        assert len({float(s) for s in scales}) == 3 and len({float(o) for o in offsets}) == 3 and (scales < 0).any()
        for c, o in enumerate((o0, o1, o2)):
            what = f"kind {kind} width {width} rows {rows} unit {unit} offsets {(o0, o1, o2)} plane {c}"
            got, pos = _plane(blob, pos, rows, width, pitch, ob, what)
            want = widened_definition((words >> np.uint32(o)) & np.uint32(1023), scales[c], offsets[c], kind)
            assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} samples differ"
            if kind == HALF:
                specials["inf"] += int(((want & 0x7fff) == 0x7c00).sum())
                specials["subnormal"] += int((((want & 0x7c00) == 0) & ((want & 0x3ff) != 0)).sum())
        seen.add((kind, unit, width, rows))
        pair_sets.add((kind, float(scales[0])))
        cases += 1
    assert pos == blob.size
    assert f"widen fields scaled rows: {cases} cases, 0 wrong" in out, out[-2000:]
    widths = set(range(1, 71)) | {1030}
    assert {(k, u, w) for (k, u, w, _) in seen} == {(k, u, w) for k in (0, HALF, BF16) for u in (16, 4) for w in widths}
    assert {r for (_, _, _, r) in seen} == {1, 2, 3}
    assert all(len({s for (k, s) in pair_sets if k == kind}) == 3 for kind in (0, HALF, BF16)), pair_sets
    assert specials["inf"] > 0 and specials["subnormal"] > 0, specials   # (binary16: overflow to inf, subnormals kept)
    return cases


def _check_v210_against_numpy(out, blob):
    pos, cases, seen = 0, 0, set()
    while pos < blob.size:
        head = blob[pos:pos + 64].view(np.uint32).tolist()
        kind, width, rows, unit = head[:4]
        scales, offsets, pitches = _floats(head[4:7]), _floats(head[7:10]), (head[10], head[11], head[11])
        pos += 64
        ob = 4 if kind == 0 else 2
        nblocks = (width + 5) // 6
        words = blob[pos:pos + rows * nblocks * 16].view("<u4").reshape(rows, nblocks, 4)
        pos += rows * nblocks * 16
        assert len({float(s) for s in scales}) == 3 and len({float(o) for o in offsets}) == 3 and (scales < 0).any()
        widths = (width, width // 2, width // 2)
        values = [np.zeros((rows, w), np.uint32) for w in widths]
        for plane, j, word, offset in V210_FIELDS:
            x = (6 if plane == 0 else 3) * np.arange(nblocks) + j
            valid = x < widths[plane]
            values[plane][:, x[valid]] = (words[:, valid, word] >> np.uint32(offset)) & np.uint32(1023)
        for plane, w in enumerate(widths):
            what = f"kind {kind} width {width} rows {rows} unit {unit} plane {plane}"
            got, pos = _plane(blob, pos, rows, w, pitches[plane], ob, what)
            want = widened_definition(values[plane], scales[plane], offsets[plane], kind)
            assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} samples differ"
        seen.add((kind, unit, rows, width))
        cases += 1
    assert pos == blob.size
    assert f"widen v210 scaled rows: {cases} cases, 0 wrong" in out, out[-2000:]
    assert seen == {(k, u, r, w) for k in (0, HALF, BF16) for u in (16, 4) for r in (1, 2, 3) for w in list(range(2, 101, 2)) + [782]}
    return cases


PROGRAMS = [("widen_fields_scaled_rows", _check_fields_against_numpy), ("widen_v210_scaled_rows", _check_v210_against_numpy)]


@pytest.mark.parametrize("program,check", PROGRAMS, ids=[p for p, _ in PROGRAMS])
def test_scaled_row_functions_equal_the_definition(tmp_path, program, check):
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not found")
    out, blob = _build_and_run(tmp_path, program, "plain", ["-O2"])
    print(check(out, blob), "cases")


@pytest.mark.parametrize("program,check", PROGRAMS, ids=[p for p, _ in PROGRAMS])
def test_scaled_row_functions_are_clean_under_asan_ubsan(tmp_path, program, check):
    """The same programs as stand-alone executables with -fsanitize=address,undefined: nothing preloaded, nothing loaded into Python.
    Their buffers end where the contract says the accesses end."""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not found")
    out, blob = _build_and_run(tmp_path, program, "san", ["-O1", "-fsanitize=address,undefined"])
    print(check(out, blob), "cases")
