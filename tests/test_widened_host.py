"""Host side of jinc_filter_process_device_widened (integer device frames into fp32 / binary16 filters): the export, the mirror and
the header; every refusal that needs no device, each with a message of its own, on filters created with device = -1; and the row
function of widen_samples_kernel (csrc/widen_rows.h) in a stand-alone host program (tests/host_sanitizer/widen_rows_main.cpp, its
own main; nothing is loaded into Python), built once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer, whose
output is compared with numpy's ((raw >> shift) & mask).astype(float32 | float16) bit for bit."""
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


def test_the_entry_is_exported_declared_and_mirrored(pkg):
    header = open(pkg.HEADER_PATH).read()
    name = "jinc_filter_process_device_widened"
    assert name in pkg.EXPORTS and hasattr(pkg.lib(), name)
    assert name + "(" in header and "int src_bits" in header
    assert hasattr(pkg.Filter, "process_device_widened")


# ---- the argument surface --------------------------------------------------------------------------------------------------------------

def _call(f, src_bits=8, steps=(1, 2, 2), shifts=None, dst_steps=None, ptrs=(4096, 8192, 8193), pitches=(64, 64, 64)):
    """An NV12-shaped source (40 x 24 luma, 20 x 12 chroma at step 2) unless told otherwise; the pointers are never dereferenced."""
    n = f.fmt.planes
    f.process_device_widened(list(ptrs)[:n], list(pitches)[:n], None if steps is None else list(steps)[:n], shifts, src_bits, [0] * n,
                             [1 << 20, 2 << 20, 3 << 20][:n], [512] * n, dst_steps, [0] * n, 1)


P010 = dict(src_bits=10, shifts=[6, 6, 6], ptrs=(4096, 8192, 8194), pitches=(80, 80, 80))

# (filter, call arguments, what the message must say)
REFUSALS = [
    ("YUV420P8", dict(), "fp32 or binary16 filter"),
    ("YUV420P10", dict(P010), "fp32 or binary16 filter"),
    ("YUV420PH", dict(P010, src_bits=12, shifts=[4, 4, 4]), "binary16"),
    ("YUV420PH", dict(P010, src_bits=16, shifts=None), "binary16"),
    ("YUV420PS", dict(src_bits=7), "src_bits"),
    ("YUV420PS", dict(src_bits=17), "src_bits"),
    ("YUV420PS", dict(P010, shifts=[6, -1, 6]), "negative"),
    ("YUV420PS", dict(shifts=[0, 0, 1]), "shift 1 "),
    ("YUV420PS", dict(P010, shifts=[7, 6, 6]), "shift 7 "),
    ("YUV420PS", dict(steps=(1, 0, 2)), "step"),
    ("YUV420PS", dict(steps=(1, 2, 5)), "step"),
    ("YUV420PS", dict(dst_steps=[1, 5, 1]), "step"),
    ("YUV420PS", dict(P010, ptrs=(4096, 8192, 8195)), "aligned"),
    ("YUV420PS", dict(pitches=(64, 38, 64)), "pitch 38 "),     # 20 chroma samples at step 2: ((20 - 1) * 2 + 1) * 1 = 39 bytes
    ("YUV420PS", dict(P010, pitches=(78, 80, 80)), "pitch 78 "),   # 40 luma words: 80 bytes
]
IDS = ["u8_filter", "u10_filter", "half_12_bits", "half_16_bits", "bits_7", "bits_17", "shift_negative", "shift_1_of_8_bits", "shift_7_of_10_bits",
       "step_0", "step_5", "dst_step_5", "odd_base_of_words", "short_chroma_pitch", "short_luma_pitch"]


@pytest.mark.parametrize("name,kw,says", REFUSALS, ids=IDS)
def test_refusals_come_before_the_device_check(pkg, name, kw, says):
    sw, sh, tw, th = GEOM
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1)
    with pytest.raises(pkg.JincError) as e:
        _call(f, **kw)
    assert e.value.code == INVALID_ARG and str(e.value).startswith("JincResize:") and says in str(e.value), str(e.value)
    f.close()


def test_every_refusal_has_a_message_of_its_own(pkg):
    sw, sh, tw, th = GEOM
    messages = []
    for name, kw, _ in REFUSALS:
        f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1)
        with pytest.raises(pkg.JincError):
            _call(f, **kw)
        messages.append(pkg.lib().jinc_last_error().decode())
        f.close()
    assert len(set(messages)) == len(REFUSALS), sorted(messages)


@pytest.mark.parametrize("name,kw", [("YUV420PS", dict()), ("YUV420PS", dict(P010)), ("YUV420PH", dict(P010)), ("YUV420PH", dict()),
                                     ("YUV420PS", dict(P010, src_bits=16, shifts=None)), ("YUV420PS", dict(steps=None, pitches=(40, 20, 20))),
                                     ("YUV420PS", dict(pitches=(40, 39, 39)))],
                         ids=["nv12_f32", "p010_f32", "p010_f16", "nv12_f16", "p016_f32", "planar_null_steps", "smallest_pitches"])
def test_accepted_arguments_reach_the_device_check(pkg, name, kw):
    sw, sh, tw, th = GEOM
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1)
    with pytest.raises(pkg.JincError) as e:
        _call(f, **kw)
    assert e.value.code == NO_DEVICE, str(e.value)
    f.close()


def test_null_plane_arrays_come_after_the_refusals(pkg):
    sw, sh, tw, th = GEOM
    f = pkg.Filter(pkg.FORMATS["YUV420PS"], sw, sh, tw, th, device=-1)
    L = pkg.lib()
    assert L.jinc_filter_process_device_widened(f._h, None, None, None, None, 8, None, None, None, None, None, 1, C.c_void_p(0)) == INVALID_ARG
    assert "null argument" in L.jinc_last_error().decode()
    assert L.jinc_filter_process_device_widened(f._h, None, None, None, None, 17, None, None, None, None, None, 1, C.c_void_p(0)) == INVALID_ARG
    assert "src_bits" in L.jinc_last_error().decode()
    f.close()


# ---- the row function --------------------------------------------------------------------------------------------------------------------

WIDTHS = {1, 7, 8, 9, 63, 64, 65, 1031}


def _build_and_run(tmp_path, tag, extra):
    header = os.path.join(PKG, "csrc", "widen_rows.h")
    assert os.path.exists(header), "csrc/widen_rows.h is missing"
    exe, out_file = str(tmp_path / f"widen_rows_{tag}"), str(tmp_path / f"widen_rows_{tag}.bin")
    subprocess.run([CXX, "-g", "-std=c++17", "-ffp-contract=off", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", *extra,
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "host_sanitizer", "widen_rows_main.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, out_file], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out and "LeakSanitizer" not in out, out[-4000:]
    return out, np.fromfile(out_file, np.uint8)


def _check_against_numpy(out, blob):
    pos, cases, seen = 0, 0, set()
    while pos < blob.size:
        sb, n, ob, bits, width, rows, unit, given, *rest = blob[pos:pos + 64].view(np.uint32).tolist()
        shifts = rest[:4]
        pos += 64
        raw = blob[pos:pos + rows * width * n * sb].view(np.uint8 if sb == 1 else np.uint16).reshape(rows, width, n).astype(np.uint32)
        pos += rows * width * n * sb
        what = f"SB {sb} N {n} OB {ob} bits {bits} shifts {shifts[:n]} width {width} unit {unit} given {given:#x}"
        for c in range(n):
            if not given >> c & 1:
                continue
            got = blob[pos:pos + rows * width * ob].view(np.uint32 if ob == 4 else np.uint16).reshape(rows, width)
            pos += rows * width * ob
            value = (raw[:, :, c] >> shifts[c]) & ((1 << bits) - 1)
            want = value.astype(np.float32).view(np.uint32) if ob == 4 else value.astype(np.float16).view(np.uint16)
            assert np.array_equal(got, want), f"{what}: plane {c} differs at {int((got != want).sum())} samples"
            if ob == 2:
                assert int(value.max()) <= 2047
        seen.add((sb, n, ob, shifts[0], width, unit))
        cases += 1
    assert pos == blob.size
    assert f"widen rows: {cases} cases, 0 wrong" in out, out[-2000:]
    for sb in (1, 2):
        for n in (1, 2, 3, 4):
            for ob in (4, 2):
                for shift in ((0,) if sb == 1 else (0, 4, 6)):
                    for unit in (16, 4, 0):
                        assert {w for (a, b, c, s, w, u) in seen if (a, b, c, s, u) == (sb, n, ob, shift, unit)} == WIDTHS, (sb, n, ob, shift, unit)
    return cases


def test_row_function_equals_numpy(tmp_path):
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not found")
    out, blob = _build_and_run(tmp_path, "plain", ["-O2"])
    print(_check_against_numpy(out, blob), "cases")


def test_row_function_is_clean_under_asan_ubsan(tmp_path):
    """The same program as a stand-alone executable with -fsanitize=address,undefined: nothing preloaded, nothing loaded into Python.
    Its buffers end where the contract says the accesses end."""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not found")
    out, blob = _build_and_run(tmp_path, "san", ["-O1", "-fsanitize=address,undefined"])
    print(_check_against_numpy(out, blob), "cases")
