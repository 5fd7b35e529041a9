"""Host side of jinc_filter_set_output_matrix and jinc_colour_matrix (a 3 x 3 colour matrix on a float filter's result planes): the
exports, the mirror and the header; every refusal of the setter, each with a message of its own, on filters created with device = -1;
jinc_colour_matrix against the header's formulas in numpy float64; and the row function of output_matrix_kernel (csrc/matrix_rows.h)
in a stand-alone host program (tests/host_sanitizer/matrix_rows_main.cpp, its own main; nothing is loaded into Python), built once
plain and once under AddressSanitizer + UndefinedBehaviorSanitizer, whose output and untouched guard bytes are compared bit for bit
with a numpy float32 emulation of
    o_i = fl32(fl32(fl32(fl32(m[3i] r0) + fl32(m[3i+1] r1)) + fl32(m[3i+2] r2)) + offset[i])."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

INVALID_ARG, NO_DEVICE, UNSUPPORTED = -1, -2, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "avisynth-jincresize_amd")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
GEOM = (40, 24, 80, 48)
IDENTITY = [1, 0, 0, 0, 1, 0, 0, 0, 1]


def test_the_entries_are_exported_declared_and_mirrored(pkg):
    header = open(pkg.HEADER_PATH).read()
    for name in ("jinc_filter_set_output_matrix", "jinc_colour_matrix"):
        assert name in pkg.EXPORTS and hasattr(pkg.lib(), name)
        assert name + "(" in header
    assert hasattr(pkg.Filter, "set_output_matrix") and callable(pkg.colour_matrix)
    test_header = open(pkg.TEST_HEADER_PATH).read()
    for name in ("jinc_debug_last_matrix_launches", "jinc_debug_matrix_rows"):
        assert name in pkg.EXPORTS and hasattr(pkg.lib(), name) and name + "(" in test_header
    assert callable(pkg.last_matrix_launches) and callable(pkg.debug_matrix_rows)
    # what the header must state: the arithmetic, the extra rounding of the 16-bit filters, the plane order, the formulas
    flat = " ".join(header.split())
    assert "never a fused multiply-add" in flat and "rounds once more here" in flat
    assert "G, B, R" in flat and "A fourth plane (alpha) is not touched" in flat
    assert "Kg = 1.0 - Kr - Kb" in flat and "2.0 * (1.0 - Kr)" in flat and "-Kg / (2.0 * (1.0 - Kb))" in flat
    assert "JINC_MATRIX_BT2020_NCL" in header and "JINC_RGB_TO_YCBCR" in header


# ---- the setter ---------------------------------------------------------------------------------------------------------------------------

NAN, INF = float("nan"), float("inf")
# (format, out_sub, matrix, offset, code, what the message must say)
REFUSALS = [
    ("YUV444P8", None, IDENTITY, None, UNSUPPORTED, "integer samples"),
    ("YUV444P16", None, IDENTITY, None, UNSUPPORTED, "integer samples"),
    ("Y32", None, IDENTITY, None, UNSUPPORTED, "three planes"),
    ("YH", None, IDENTITY, None, UNSUPPORTED, "three planes"),
    ("YUV420PS", None, IDENTITY, None, UNSUPPORTED, "one size"),
    ("YUV422PH", None, IDENTITY, None, UNSUPPORTED, "one size"),
    ("YUV444PS", (1, 1), IDENTITY, None, UNSUPPORTED, "one size"),
    ("YUV444PS", None, [1, 0, 0, 0, NAN, 0, 0, 0, 1], None, INVALID_ARG, "entry 4 of the output matrix is not finite"),
    ("RGBPBF", None, [1, 0, 0, 0, 1, 0, 0, 0, -INF], None, INVALID_ARG, "entry 8 of the output matrix is not finite"),
    ("YUV444PH", None, IDENTITY, [0, INF, 0], INVALID_ARG, "entry 1 of the output matrix's offset is not finite"),
]
IDS = ["u8_filter", "u16_filter", "one_plane_f32", "one_plane_f16", "420_out", "422_out_half", "444_in_420_out", "nan_in_m", "inf_in_m_bf16",
       "inf_in_offset"]


@pytest.mark.parametrize("name,out_sub,m,offset,code,says", REFUSALS, ids=IDS)
def test_the_setter_refuses_on_filters_without_a_device(pkg, name, out_sub, m, offset, code, says):
    sw, sh, tw, th = GEOM
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1, out_sub=out_sub)
    with pytest.raises(pkg.JincError) as e:
        f.set_output_matrix(m, offset)
    assert e.value.code == code and str(e.value).startswith("JincResize:") and says in str(e.value), str(e.value)
    f.close()


def test_every_refusal_has_a_message_of_its_own(pkg):
    sw, sh, tw, th = GEOM
    kinds = set()
    for name, out_sub, m, offset, _, _ in REFUSALS:
        f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1, out_sub=out_sub)
        with pytest.raises(pkg.JincError):
            f.set_output_matrix(m, offset)
        kinds.add("".join(ch for ch in pkg.lib().jinc_last_error().decode() if not ch.isdigit()))
        f.close()
    assert len(kinds) == 5, sorted(kinds)   # integer filter, planes, sizes, entry of the matrix, entry of the offset


@pytest.mark.parametrize("name,out_sub", [("YUV444PS", None), ("YUV444PH", None), ("YUV444PBF", None), ("RGBPS", None), ("RGBAPS", None),
                                          ("YUVA444PH", None), ("YUV420PS", (0, 0)), ("YUV422PBF", (0, 0))])
def test_the_setter_accepts_444_outputs_of_float_filters(pkg, name, out_sub):
    sw, sh, tw, th = GEOM
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1, out_sub=out_sub)
    f.set_output_matrix(pkg.colour_matrix(pkg.MATRIX_BT709, pkg.YCBCR_TO_RGB), [0.0, 0.5, -0.5])
    f.set_output_matrix(IDENTITY)           # (NULL offset: zeros)
    f.set_output_matrix(None)
    f.close()


def _host_entries(pkg, f):
    """Return codes of jinc_filter_get_frame and jinc_filter_submit on a filter without a device (pointers are never read)."""
    L = pkg.lib()
    p, i, t = (C.c_void_p * 4)(4096, 8192, 12288, 0), (C.c_int * 4)(512, 512, 512, 0), C.c_longlong()
    return L.jinc_filter_get_frame(f._h, p, i, p, i), L.jinc_filter_submit(f._h, p, i, p, i, C.byref(t))


def test_host_frame_entries_refuse_a_filter_with_a_matrix_and_set_then_clear_refuses_nothing(pkg):
    sw, sh, tw, th = GEOM
    f = pkg.Filter(pkg.FORMATS["YUV444PS"], sw, sh, tw, th, device=-1)
    assert _host_entries(pkg, f) == (NO_DEVICE, NO_DEVICE)
    f.set_output_matrix(IDENTITY, [0, 0, 0])
    assert _host_entries(pkg, f) == (UNSUPPORTED, UNSUPPORTED)
    assert "output matrix" in pkg.lib().jinc_last_error().decode()
    # ... while a device call gets as far as it always did
    with pytest.raises(pkg.JincError) as e:
        f.process_device([4096, 8192, 12288], [512] * 3, [0] * 3, [1 << 20, 2 << 20, 3 << 20], [512] * 3, [0] * 3, 1)
    assert e.value.code == NO_DEVICE
    f.set_output_matrix(None)
    assert _host_entries(pkg, f) == (NO_DEVICE, NO_DEVICE)
    f.set_simd_order(1)   # (the other setters are independent of it, before and after)
    f.set_output_matrix(IDENTITY)
    f.set_simd_order(0)
    f.close()


def test_null_filter_is_refused(pkg):
    L = pkg.lib()
    assert L.jinc_filter_set_output_matrix(None, (C.c_float * 9)(*IDENTITY), None) == INVALID_ARG
    assert L.jinc_colour_matrix(0, 0, None) == INVALID_ARG


# ---- jinc_colour_matrix -------------------------------------------------------------------------------------------------------------------

KR_KB = {0: (0.299, 0.114), 1: (0.2126, 0.0722), 2: (0.2627, 0.0593)}


def formulas(standard, direction):
    """The header's formulas in float64, in the order written."""
    kr, kb = KR_KB[standard]
    kg = 1.0 - kr - kb
    if direction == 0:
        return np.array([[1.0, 0.0, 2.0 * (1.0 - kr)],
                         [1.0, -2.0 * kb * (1.0 - kb) / kg, -2.0 * kr * (1.0 - kr) / kg],
                         [1.0, 2.0 * (1.0 - kb), 0.0]], np.float64)
    return np.array([[kr, kg, kb],
                     [-kr / (2.0 * (1.0 - kb)), -kg / (2.0 * (1.0 - kb)), 0.5],
                     [0.5, -kg / (2.0 * (1.0 - kr)), -kb / (2.0 * (1.0 - kr))]], np.float64)


@pytest.mark.parametrize("standard", [0, 1, 2], ids=["bt601", "bt709", "bt2020ncl"])
@pytest.mark.parametrize("direction", [0, 1], ids=["to_rgb", "to_ycbcr"])
def test_colour_matrix_equals_the_formulas_rounded_once(pkg, standard, direction):
    assert (pkg.MATRIX_BT601, pkg.MATRIX_BT709, pkg.MATRIX_BT2020_NCL, pkg.YCBCR_TO_RGB, pkg.RGB_TO_YCBCR) == (0, 1, 2, 0, 1)
    got = pkg.colour_matrix(standard, direction)
    want = formulas(standard, direction).astype(np.float32)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)


@pytest.mark.parametrize("standard", [0, 1, 2], ids=["bt601", "bt709", "bt2020ncl"])
def test_the_two_directions_multiply_to_the_identity(pkg, standard):
    """Derived: an entry of the product sums three products of two entries rounded to float32 (2^-24 relative each): nine roundings of
    2^-24 per entry bound it by 2^-22 (no entry or partial sum exceeds 2 by much; the bound leaves a factor of two for that)."""
    a = pkg.colour_matrix(standard, pkg.YCBCR_TO_RGB).astype(np.float64)
    b = pkg.colour_matrix(standard, pkg.RGB_TO_YCBCR).astype(np.float64)
    for p in (a @ b, b @ a):
        err = np.abs(p - np.eye(3)).max()
        print(standard, err)
        assert err <= 2.0 ** -22, p


@pytest.mark.parametrize("standard,direction", [(-1, 0), (3, 0), (0, -1), (0, 2)])
def test_colour_matrix_refuses_what_it_does_not_know(pkg, standard, direction):
    with pytest.raises(pkg.JincError) as e:
        pkg.colour_matrix(standard, direction)
    assert e.value.code == INVALID_ARG and ("standard" if standard not in (0, 1, 2) else "direction") in str(e.value)


# ---- the row function --------------------------------------------------------------------------------------------------------------------

HALF, BF16 = 1, 2   # kernels.h kSampleHalf, kSampleBFloat16
WIDTHS = {1, 3, 4, 7, 8, 9, 255, 256, 257, 260, 517}


def widen(raw, kind):
    """Samples (uint32 / uint16 bit patterns) widened exactly to float32."""
    if kind == 0:
        return raw.view(np.float32)
    if kind == HALF:
        return raw.view(np.float16).astype(np.float32)
    return (raw.astype(np.uint32) << 16).view(np.float32)


def bf16_round(v):
    """float32 -> bfloat16 bit patterns, round to nearest even (finite values): the upper half plus the carry of the lower half."""
    bits = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return ((bits + np.uint32(0x7fff) + ((bits >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def narrow(v, kind):
    """float32 -> the sample type's bit patterns, round to nearest even."""
    if kind == 0:
        return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    if kind == HALF:
        with np.errstate(over="ignore"):
            return v.astype(np.float16).view(np.uint16)
    return bf16_round(v)


def emulate(r0, r1, r2, m, offset):
    """The definition on float32 arrays: np.float32 products and sums taken one at a time."""
    m = np.asarray(m, np.float32).reshape(3, 3)
    offset = np.asarray(offset, np.float32)
    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(3):
            p0 = (m[i, 0] * r0).astype(np.float32)
            p1 = (m[i, 1] * r1).astype(np.float32)
            p2 = (m[i, 2] * r2).astype(np.float32)
            two = (p0 + p1).astype(np.float32)
            three = (two + p2).astype(np.float32)
            out.append((three + offset[i]).astype(np.float32))
    return out


def _build_and_run(tmp_path, tag, extra):
    header = os.path.join(PKG, "csrc", "matrix_rows.h")
    assert os.path.exists(header), "csrc/matrix_rows.h is missing"
    exe, out_file = str(tmp_path / f"matrix_rows_{tag}"), str(tmp_path / f"matrix_rows_{tag}.bin")
    subprocess.run([CXX, "-g", "-std=c++17", "-ffp-contract=off", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", *extra,
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "host_sanitizer", "matrix_rows_main.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, out_file], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out and "LeakSanitizer" not in out, out[-4000:]
    return out, np.fromfile(out_file, np.uint8)


def _check_against_numpy(out, blob):
    pos, seen = 0, set()
    while pos < blob.size:
        head = blob[pos:pos + 128]
        kind, width, rows, frames, unit, lead, b0, b1, b2, p0, p1, p2, f0, f1, f2, _ = head[:64].view(np.uint32).tolist()
        m, offset = head[64:100].view(np.float32), head[100:112].view(np.float32)
        pos += 128
        sb = 4 if kind == 0 else 2
        dtype = np.uint32 if kind == 0 else np.uint16
        what = f"kind {kind} width {width} unit {unit}"
        assert (rows, frames) == (3, 2), what
        nbytes, pitch, fs = (b0, b1, b2), (p0, p1, p2), (f0, f1, f2)
        before, after = [], []
        for bufs in (before, after):
            for c in range(3):
                bufs.append(blob[pos:pos + nbytes[c]].copy())
                pos += nbytes[c]

        def samples(buf, c):   # a (frames, rows, width) view of plane c's samples inside its buffer
            return np.ndarray((frames, rows, width), dtype, buf, lead, (fs[c], pitch[c], sb))

        for c in range(3):   # the buffer ends with the last sample, and the access class is what the case says
            assert nbytes[c] == lead + fs[c] * (frames - 1) + pitch[c] * (rows - 1) + width * sb, what
            al = lead | pitch[c] | fs[c]
            assert al % (unit or sb) == 0 and (unit == 16 or al % 16) and (unit != 0 or sb == 4 or al % 4), what
        assert np.isfinite(np.concatenate([widen(samples(before[c], c).copy(), kind).ravel() for c in range(3)])).all(), what
        r = [widen(samples(before[c], c).copy(), kind) for c in range(3)]
        o = emulate(r[0], r[1], r[2], m, offset)
        for c in range(3):
            want = before[c].copy()   # (guards included: every byte that is no sample keeps its canary)
            samples(want, c)[...] = narrow(o[c], kind).reshape(frames, rows, width)
            bad = np.flatnonzero(after[c] != want)
            assert bad.size == 0, f"{what}: plane {c}: {bad.size} bytes differ, first at byte {int(bad[0])} (lead {lead}, pitch {pitch[c]}, " \
                                  f"frame stride {fs[c]}): got {int(after[c][bad[0]])}, want {int(want[bad[0]])}"
            guard = np.ones(nbytes[c], bool)
            np.ndarray((frames, rows, width * sb), bool, guard, lead, (fs[c], pitch[c], 1))[...] = False
            assert (after[c][guard] == 0xA5).all(), what
        seen.add((kind, width, unit))
    assert pos == blob.size
    assert f"matrix rows: {len(seen)} cases" in out, out[-2000:]
    assert seen == {(k, w, u) for k in (0, HALF, BF16) for w in WIDTHS for u in (16, 4, 0)}
    return len(seen)


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
