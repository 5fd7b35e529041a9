"""Host side of jinc_filter_process_device_narrowed (the results of fp32 / binary16 / bfloat16 filters into integer device frames):
the export, the mirror and the header; every refusal that needs no device, each with a message of its own, on filters created with
device = -1; and the row function of narrow_samples_kernel (csrc/narrow_rows.h) in a stand-alone host program
(tests/host_sanitizer/narrow_rows_main.cpp, its own main; nothing is loaded into Python), built once plain and once under
AddressSanitizer + UndefinedBehaviorSanitizer, whose output and untouched guard bytes are compared with numpy's
np.rint(np.clip(r, 0, peak)) << shift (NaN -> 0) bit for bit."""
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
    name = "jinc_filter_process_device_narrowed"
    assert name in pkg.EXPORTS and hasattr(pkg.lib(), name)
    assert name + "(" in header and "int dst_bits" in header
    assert hasattr(pkg.Filter, "process_device_narrowed")
    assert "jinc_debug_narrow" in pkg.EXPORTS and hasattr(pkg.lib(), "jinc_debug_narrow") and callable(pkg.debug_narrow)
    assert "jinc_debug_narrow(" in open(pkg.TEST_HEADER_PATH).read()
    # what the header must state: the double rounding of the 16-bit filters and the integer filters' bit-exact twin
    flat = " ".join(header.split())
    assert "rounds twice" in flat and "bit for bit" in flat


# ---- the argument surface --------------------------------------------------------------------------------------------------------------

def _call(f, dst_bits=8, steps=None, dst_steps=(1, 2, 2), shifts=None, ptrs=(1 << 20, 2 << 20, (2 << 20) + 1), pitches=(80, 80, 80)):
    """An NV12-shaped destination (80 x 48 luma, 40 x 24 chroma at step 2) unless told otherwise; the pointers are never dereferenced."""
    n = f.fmt.planes
    f.process_device_narrowed([4096, 8192, 12288][:n], [512] * n, steps, [0] * n, list(ptrs)[:n], list(pitches)[:n],
                              None if dst_steps is None else list(dst_steps)[:n], shifts, dst_bits, [0] * n, 1)


P010 = dict(dst_bits=10, shifts=[6, 6, 6], ptrs=(1 << 20, 2 << 20, (2 << 20) + 2), pitches=(160, 160, 160))

# (filter, call arguments, what the message must say)
REFUSALS = [
    ("YUV420P8", dict(), "integer samples"),
    ("YUV420P10", dict(P010), "integer samples"),
    ("YUV420PS", dict(dst_bits=7), "dst_bits"),
    ("YUV420PS", dict(dst_bits=17), "dst_bits"),
    ("YUV420PH", dict(dst_bits=0), "dst_bits"),
    ("YUV420PS", dict(steps=[1, 0, 1]), "source sample step"),
    ("YUV420PS", dict(steps=[1, 1, 5]), "source sample step"),
    ("YUV420PS", dict(dst_steps=(1, 2, 5)), "destination sample step"),
    ("YUV420PS", dict(dst_steps=(0, 2, 2)), "destination sample step"),
    ("YUV420PS", dict(P010, shifts=[6, -1, 6]), "negative"),
    ("YUV420PS", dict(shifts=[0, 0, 1]), "shift 1 "),
    ("YUV420PS", dict(P010, shifts=[7, 6, 6]), "shift 7 "),
    ("YUV420PBF", dict(P010, dst_bits=12, shifts=[4, 5, 4]), "shift 5 "),
    ("YUV420PS", dict(P010, ptrs=(1 << 20, 2 << 20, (2 << 20) + 3)), "aligned"),
    ("YUV420PS", dict(pitches=(80, 78, 80)), "pitch 78 "),        # 40 chroma samples at step 2: ((40 - 1) * 2 + 1) * 1 = 79 bytes
    ("YUV420PS", dict(P010, pitches=(158, 160, 160)), "pitch 158 "),  # 80 luma words: 160 bytes
]
IDS = ["u8_filter", "u10_filter", "bits_7", "bits_17", "bits_0_half", "src_step_0", "src_step_5", "dst_step_5", "dst_step_0", "shift_negative",
       "shift_1_of_8_bits", "shift_7_of_10_bits", "shift_5_of_12_bits_bf16", "odd_base_of_words", "short_chroma_pitch", "short_luma_pitch"]


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
    # ... and the seven KINDS of refusal differ beyond the numbers they quote
    kinds = {"".join(ch for ch in m if not ch.isdigit()) for m in messages}
    assert len(kinds) >= 8, sorted(kinds)   # (seven kinds; the step names its side)


@pytest.mark.parametrize("name,kw", [("YUV420PS", dict()), ("YUV420PS", dict(P010)), ("YUV420PH", dict(P010)), ("YUV420PBF", dict()),
                                     ("YUV420PS", dict(P010, dst_bits=16, shifts=None)), ("YUV420PH", dict(P010, dst_bits=12, shifts=[4, 4, 4])),
                                     ("YUV420PS", dict(dst_steps=None, pitches=(80, 40, 40))), ("YUV420PS", dict(pitches=(80, 79, 79))),
                                     ("YUV420PS", dict(steps=[1, 2, 2]))],
                         ids=["nv12_f32", "p010_f32", "p010_f16", "nv12_bf16", "p016_f32", "p012_f16", "planar_null_steps", "smallest_pitches",
                              "interleaved_source"])
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
    assert L.jinc_filter_process_device_narrowed(f._h, None, None, None, None, None, None, None, None, 8, None, 1, C.c_void_p(0)) == INVALID_ARG
    assert "null argument" in L.jinc_last_error().decode()
    assert L.jinc_filter_process_device_narrowed(f._h, None, None, None, None, None, None, None, None, 17, None, 1, C.c_void_p(0)) == INVALID_ARG
    assert "dst_bits" in L.jinc_last_error().decode()
    assert L.jinc_filter_process_device_narrowed(None, None, None, None, None, None, None, None, None, 8, None, 1, C.c_void_p(0)) == INVALID_ARG
    f.close()


def test_the_hook_refuses_what_it_has_no_kernel_for(pkg):
    v = np.zeros(4, np.float32)
    for bits, shift in ((7, 0), (17, 0), (8, 1), (10, 7), (10, -1)):
        with pytest.raises(pkg.JincError) as e:
            pkg.debug_narrow(v, bits, shift, device=0)
        assert e.value.code == INVALID_ARG
    with pytest.raises(TypeError):
        pkg.debug_narrow(v, 8, 0, bfloat16=True)


# ---- the row function --------------------------------------------------------------------------------------------------------------------

HALF, BF16 = 1, 2   # kernels.h kSampleHalf, kSampleBFloat16
WIDTHS = set(range(1, 71))


def _build_and_run(tmp_path, tag, extra):
    header = os.path.join(PKG, "csrc", "narrow_rows.h")
    assert os.path.exists(header), "csrc/narrow_rows.h is missing"
    exe, out_file = str(tmp_path / f"narrow_rows_{tag}"), str(tmp_path / f"narrow_rows_{tag}.bin")
    subprocess.run([CXX, "-g", "-std=c++17", "-ffp-contract=off", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", *extra,
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "host_sanitizer", "narrow_rows_main.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, out_file], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out and "LeakSanitizer" not in out, out[-4000:]
    return out, np.fromfile(out_file, np.uint8)


def _widen(raw, kind):
    """The plane's samples widened exactly to float32."""
    if kind == 0:
        return raw.view(np.float32)
    if kind == HALF:
        return raw.view(np.float16).astype(np.float32)
    return (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32)


def definition(r, peak):
    """value = lrintf(clamp(r, 0, peak)), round half to even; a NaN becomes 0."""
    with np.errstate(invalid="ignore"):
        return np.rint(np.clip(np.where(np.isnan(r), np.float32(0), r), 0, peak)).astype(np.uint32)


def _check_against_numpy(out, blob):
    pos, cases, seen, values = 0, 0, set(), {}
    while pos < blob.size:
        kind, n, db, bits, width, rows, unit, given, s0, s1, s2, s3, lead, pitch, dst_bytes, _ = blob[pos:pos + 64].view(np.uint32).tolist()
        shifts = [s0, s1, s2, s3]
        pos += 64
        ib = 4 if kind == 0 else 2
        peak = (1 << bits) - 1
        what = f"kind {kind} N {n} DB {db} bits {bits} shifts {shifts[:n]} width {width} unit {unit} given {given:#x}"
        want = np.full(dst_bytes, 0xA5, np.uint8)   # the canary: every byte that is no given sample keeps it
        for c in range(n):
            if not given >> c & 1:
                continue
            raw = blob[pos:pos + rows * width * ib].copy()
            pos += rows * width * ib
            r = _widen(raw, kind).reshape(rows, width)
            v = (definition(r, peak) << shifts[c]).astype(np.uint8 if db == 1 else np.uint16)
            for byte in range(db):
                np.ndarray((rows, width), np.uint8, want, lead + c * db + byte, (pitch, n * db))[...] = (v >> (8 * byte)).astype(np.uint8)
            if rows == 1:   # the value cases: what they covered
                key = (kind, bits)
                values.setdefault(key, set()).update(np.unique(raw.view(np.uint32 if ib == 4 else np.uint16)).tolist())
        got = blob[pos:pos + dst_bytes]
        pos += dst_bytes
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{what}: {bad.size} destination bytes differ, first at byte {int(bad[0])} (lead {lead}, pitch {pitch}): " \
                              f"got {int(got[bad[0]])}, want {int(want[bad[0]])}"
        if rows > 1:
            seen.add((kind, n, db, shifts[0], width, unit, given == (1 << n) - 1))
        else:
            seen.add((kind, n, db, shifts[0], "values", unit, bits))
        cases += 1
    assert pos == blob.size
    assert f"narrow rows: {cases} cases, 0 wrong" in out, out[-2000:]
    for kind in (0, HALF, BF16):
        for n in (1, 2, 3, 4):
            for db in (1, 2):
                for shift in ((0,) if db == 1 else (0, 6)):
                    for unit in (16, 4, 0):
                        for complete in ((True,) if n == 1 else (True, False)):
                            have = {w for (k, a, b, s, w, u, full) in seen if (k, a, b, s, u, full) == (kind, n, db, shift, unit, complete)}
                            assert have == WIDTHS, (kind, n, db, shift, unit, complete)
        for bits in (8, 9, 10, 12, 14, 16):
            for shift in {0, (8 if bits == 8 else 16) - bits}:
                for unit in (16, 4, 0):
                    assert (kind, 1, 1 if bits == 8 else 2, shift, "values", unit, bits) in seen, (kind, bits, shift, unit)
    # the values: every tie k + 0.5 up to peak + 2, both bounds, both infinities, a NaN and -0 in fp32; every pattern in 16 bits
    for bits in (8, 9, 10, 12, 14, 16):
        peak = (1 << bits) - 1
        have = values[(0, bits)]
        ties = (np.arange(-1, peak + 3, dtype=np.float32) + np.float32(0.5)).view(np.uint32).tolist()
        assert set(ties) <= have, bits
        special = np.array([0.0, peak, peak + 1, -1.0, np.inf, -np.inf, np.nan, -0.0], np.float32).view(np.uint32).tolist()
        assert set(special) <= have, bits
        assert len(values[(HALF, bits)]) == 65536 and len(values[(BF16, bits)]) == 65536
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
