"""Host side of jinc_filter_process_device_widened_scaled / _narrowed_scaled (a scale and an offset between code values and the float
range) and of jinc_code_range: the exports, the mirror and the header's definitions; the new refusals -- a NaN, infinite or zero
scale, a NaN or infinite offset -- each with a message of its own that names the side and the plane, before the device check, on
filters created with device = -1; every refusal of the underlying calls, still with its old text; what the scaled form newly accepts
(16-bit words into half planes, 10-bit words into bfloat16 planes); and the SCALED row functions of csrc/widen_rows.h and
csrc/narrow_rows.h in stand-alone host programs (tests/host_sanitizer/widen_scaled_rows_main.cpp, narrow_scaled_rows_main.cpp, each
with its own main; nothing is loaded into Python), built once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer,
whose output is compared with numpy bit for bit: float32 multiply, then float32 add, then astype(float16) or a round-to-nearest-even
bfloat16 (widened), or rint(clip(., 0, peak)) << shift (narrowed)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_narrowed_host import REFUSALS as NARROWED_REFUSALS
from test_narrowed_host import definition
from test_widened_host import REFUSALS as WIDENED_REFUSALS

INVALID_ARG, NO_DEVICE = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "avisynth-jincresize_amd")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
GEOM = (40, 24, 80, 48)
HALF, BF16 = 1, 2   # kernels.h kSampleHalf, kSampleBFloat16
NAN, INF = float("nan"), float("inf")


def bf16_rne(v):
    """float32 values as bfloat16 bit patterns (uint16), rounded to nearest even; infinities stay, no NaN is given."""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def widened_definition(value, scale, offset, kind):
    """s = fl32(fl32(float(value) * scale) + offset) as the bits the plane holds: uint32 for fp32, uint16 for binary16 (numpy's
    astype rounds to nearest even, overflows to inf and keeps subnormals) and for bfloat16."""
    with np.errstate(over="ignore"):
        s = value.astype(np.float32) * np.float32(scale)
        s = (s + np.float32(offset)).astype(np.float32)
        if kind == 0:
            return s.view(np.uint32)
        return bf16_rne(s) if kind == BF16 else s.astype(np.float16).view(np.uint16)


def narrowed_definition(r, scale, offset, peak):
    """rint(clip(fl32(fl32(r * scale) + offset), 0, peak)); a NaN becomes 0."""
    with np.errstate(over="ignore", invalid="ignore"):
        t = r.astype(np.float32) * np.float32(scale)
        t = (t + np.float32(offset)).astype(np.float32)
    return definition(t, peak)


# ---- the surface --------------------------------------------------------------------------------------------------------------------------

def test_the_entries_are_exported_declared_and_mirrored(pkg):
    header, test_header = open(pkg.HEADER_PATH).read(), open(pkg.TEST_HEADER_PATH).read()
    for name in ("jinc_filter_process_device_widened_scaled", "jinc_filter_process_device_narrowed_scaled", "jinc_code_range"):
        assert name in pkg.EXPORTS and hasattr(pkg.lib(), name), name
        assert name + "(" in header, name
    for name in ("jinc_debug_widen_scaled", "jinc_debug_narrow_scaled"):
        assert name in pkg.EXPORTS and hasattr(pkg.lib(), name), name
        assert name + "(" in test_header and name + "(" not in header, name
    for name in ("process_device_widened_scaled", "process_device_narrowed_scaled"):
        assert hasattr(pkg.Filter, name), name
    assert callable(pkg.code_range) and callable(pkg.debug_widen_scaled) and callable(pkg.debug_narrow_scaled)
    flat = " ".join(" ".join(line.strip().removeprefix("*") for line in header.splitlines()).split())   # (without the comments' margin)
    # the definitions, as the header must state them
    assert "s = fl32(fl32(float(v) * src_scale[i]) + src_offset[i])" in flat
    assert "lrintf(clamp(fl32(fl32(r * dst_scale[i]) + dst_offset[i]), 0, peak)) << shift[i]" in flat
    assert "two fp32 roundings and never an FMA" in flat
    assert "The call IS the existing call" in flat
    assert "const float src_scale[4], const float src_offset[4]" in flat and "const float dst_scale[4]" in flat
    for word in ("JINC_RANGE_FULL", "JINC_RANGE_LIMITED", "JINC_PLANE_LUMA_OR_RGB", "JINC_PLANE_CHROMA"):
        assert "#define " + word in header, word


# ---- the argument surface ---------------------------------------------------------------------------------------------------------------------

def _widened(f, src_bits=8, steps=(1, 2, 2), shifts=None, dst_steps=None, ptrs=(4096, 8192, 8193), pitches=(64, 64, 64), scales=None, offsets=None):
    """test_widened_host._call with the two arrays: an NV12-shaped source; the pointers are never dereferenced."""
    n = f.fmt.planes
    f.process_device_widened_scaled(list(ptrs)[:n], list(pitches)[:n], None if steps is None else list(steps)[:n], shifts, src_bits, scales, offsets,
                                    [0] * n, [1 << 20, 2 << 20, 3 << 20][:n], [512] * n, dst_steps, [0] * n, 1)


def _narrowed(f, dst_bits=8, steps=None, dst_steps=(1, 2, 2), shifts=None, ptrs=(1 << 20, 2 << 20, (2 << 20) + 1), pitches=(80, 80, 80),
              scales=None, offsets=None):
    """test_narrowed_host._call with the two arrays: an NV12-shaped destination; the pointers are never dereferenced."""
    n = f.fmt.planes
    f.process_device_narrowed_scaled([4096, 8192, 12288][:n], [512] * n, steps, [0] * n, list(ptrs)[:n], list(pitches)[:n],
                                     None if dst_steps is None else list(dst_steps)[:n], shifts, dst_bits, scales, offsets, [0] * n, 1)


CALLS = {"widened": (_widened, "source"), "narrowed": (_narrowed, "destination")}

# (id, scales, offsets, the plane at fault, what the message must say)
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


@pytest.mark.parametrize("call", sorted(CALLS))
@pytest.mark.parametrize("case", NEW_REFUSALS, ids=[c[0] for c in NEW_REFUSALS])
def test_new_refusals_come_before_the_device_check_and_name_side_and_plane(pkg, call, case):
    _, scales, offsets, plane, which, how = case
    fn, side = CALLS[call]
    sw, sh, tw, th = GEOM
    for name in ("YUV420PS", "YUV420PH", "YUV420PBF"):
        f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1)
        with pytest.raises(pkg.JincError) as e:
            fn(f, scales=scales, offsets=offsets)
        text = str(e.value)
        assert e.value.code == INVALID_ARG and text.startswith("JincResize:"), text
        assert which in text and how in text and f"{side} plane {plane}" in text, text
        f.close()


def test_every_new_refusal_has_a_message_of_its_own(pkg):
    sw, sh, tw, th = GEOM
    f = pkg.Filter(pkg.FORMATS["YUV420PS"], sw, sh, tw, th, device=-1)
    messages = []
    for call in sorted(CALLS):
        for _, scales, offsets, *_ in NEW_REFUSALS:
            with pytest.raises(pkg.JincError):
                CALLS[call][0](f, scales=scales, offsets=offsets)
            messages.append(pkg.lib().jinc_last_error().decode())
    f.close()
    # -inf and -0 read as +inf and 0 of the same plane kind: 6 kinds x planes as given, never one text for two sides
    assert len(set(messages)) == len(messages), sorted(messages)
    kinds = {"".join(ch for ch in m if not ch.isdigit()) for m in messages}
    assert len(kinds) == 10, sorted(kinds)   # (NaN / infinite / zero scale, NaN / infinite offset) x (source, destination)


def test_a_bad_value_of_an_unused_plane_is_not_read(pkg):
    """Y32 has one plane: elements 1 .. 3 of the arrays belong to no plane of the filter."""
    f = pkg.Filter(pkg.FORMATS["Y32"], 40, 24, 80, 48, device=-1)
    L = pkg.lib()
    P4, I4, F4 = C.c_void_p * 4, C.c_int * 4, C.c_float * 4
    rc = L.jinc_filter_process_device_widened_scaled(f._h, P4(4096), I4(64), None, None, 8, F4(0.5, NAN, 0.0, INF), F4(0.0, NAN, INF, -INF), None,
                                                     P4(1 << 20), I4(512), None, None, 1, C.c_void_p(0))
    assert rc == NO_DEVICE, L.jinc_last_error().decode()
    rc = L.jinc_filter_process_device_narrowed_scaled(f._h, P4(4096), I4(512), None, None, P4(1 << 20), I4(80), None, None, 8, F4(0.5, NAN, 0.0, INF),
                                                      F4(0.0, NAN, INF, -INF), None, 1, C.c_void_p(0))
    assert rc == NO_DEVICE, L.jinc_last_error().decode()
    f.close()


def _old_message(pkg, fn_old, name, kw):
    sw, sh, tw, th = GEOM
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1)
    with pytest.raises(pkg.JincError):
        fn_old(f, **kw)
    text = pkg.lib().jinc_last_error().decode()
    f.close()
    return text


@pytest.mark.parametrize("arrays", ["both_null", "scale_given", "offset_given", "bad_scale_given"])
def test_every_refusal_of_the_underlying_calls_keeps_its_text(pkg, arrays):
    """The refusals of test_widened_host.py and test_narrowed_host.py through the scaled entries: the same code and the same text as
    the unscaled entry gives, whether the arrays are NULL or given -- they come first, in front of a bad scale too.  With an array
    given, the two exactness rules of half and bfloat16 filters are no refusals any more: those calls reach the device check."""
    import test_narrowed_host
    import test_widened_host
    extra = {"both_null": dict(), "scale_given": dict(scales=[0.5] * 3), "offset_given": dict(offsets=[0.25] * 3),
             "bad_scale_given": dict(scales=[NAN, 0.0, INF])}[arrays]
    sw, sh, tw, th = GEOM
    for fn_new, fn_old, refusals in ((_widened, test_widened_host._call, WIDENED_REFUSALS), (_narrowed, test_narrowed_host._call, NARROWED_REFUSALS)):
        for name, kw, says in refusals:
            old = _old_message(pkg, fn_old, name, kw)
            assert says in old
            f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1)
            with pytest.raises(pkg.JincError) as e:
                fn_new(f, **kw, **extra)
            exactness_rule = fn_new is _widened and "not exact in" in old
            if exactness_rule and arrays in ("scale_given", "offset_given"):
                assert e.value.code == NO_DEVICE, str(e.value)
            elif exactness_rule and arrays == "bad_scale_given":
                assert e.value.code == INVALID_ARG and "scale of source plane 0 is NaN" in str(e.value), str(e.value)
            else:
                assert e.value.code == INVALID_ARG and pkg.lib().jinc_last_error().decode() == old, (str(e.value), old)
            f.close()


P010 = dict(src_bits=10, shifts=[6, 6, 6], ptrs=(4096, 8192, 8194), pitches=(80, 80, 80))
P016 = dict(P010, src_bits=16, shifts=None)
NEWLY_ACCEPTED = [("YUV420PH", P016, "p016_f16"), ("YUV420PBF", P010, "p010_bf16")]


@pytest.mark.parametrize("name,kw,_id", NEWLY_ACCEPTED, ids=[c[2] for c in NEWLY_ACCEPTED])
@pytest.mark.parametrize("arrays", [dict(scales=[1 / 65535.0] * 3), dict(scales=[1.0] * 3, offsets=[0.0] * 3), dict(offsets=[-0.5] * 3)],
                         ids=["scale", "identity_arrays", "offset_only"])
def test_wide_samples_reach_the_device_check_with_an_array_given(pkg, name, kw, _id, arrays):
    sw, sh, tw, th = GEOM
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1)
    with pytest.raises(pkg.JincError) as e:
        _widened(f, **kw, **arrays)
    assert e.value.code == NO_DEVICE, str(e.value)
    f.close()


@pytest.mark.parametrize("name,kw,_id", NEWLY_ACCEPTED, ids=[c[2] for c in NEWLY_ACCEPTED])
def test_wide_samples_are_refused_as_today_with_both_arrays_null(pkg, name, kw, _id):
    import test_widened_host
    sw, sh, tw, th = GEOM
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1)
    with pytest.raises(pkg.JincError) as e:
        _widened(f, **kw)
    assert e.value.code == INVALID_ARG and "not exact in" in str(e.value), str(e.value)
    new = pkg.lib().jinc_last_error().decode()
    with pytest.raises(pkg.JincError):
        test_widened_host._call(f, **kw)
    assert pkg.lib().jinc_last_error().decode() == new
    f.close()


@pytest.mark.parametrize("call,name,kw", [("widened", "YUV420PS", dict()), ("widened", "YUV420PS", dict(P010)), ("widened", "YUV420PH", dict()),
                                          ("widened", "YUV420PBF", dict()), ("narrowed", "YUV420PS", dict()), ("narrowed", "YUV420PH", dict()),
                                          ("narrowed", "YUV420PBF", dict(dst_bits=10, shifts=[6] * 3, ptrs=(1 << 20, 2 << 20, (2 << 20) + 2), pitches=(160,) * 3))],
                         ids=["w_nv12_f32", "w_p010_f32", "w_nv12_f16", "w_nv12_bf16", "n_nv12_f32", "n_nv12_f16", "n_p010_bf16"])
def test_accepted_arguments_reach_the_device_check(pkg, call, name, kw):
    sw, sh, tw, th = GEOM
    for arrays in (dict(), dict(scales=[-2.5, 1e-30, 3e38], offsets=[1e30, -0.0, 0.0]), dict(scales=[1 / 219.0, 1 / 224.0, 1 / 224.0])):
        f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1)
        with pytest.raises(pkg.JincError) as e:
            CALLS[call][0](f, **kw, **arrays)
        assert e.value.code == NO_DEVICE, str(e.value)
        f.close()


def test_the_hooks_refuse_what_they_have_no_kernel_for(pkg):
    v, raw = np.zeros(4, np.float32), np.zeros(4, np.uint16)
    for bits, shift, scale, offset in ((7, 0, 1.0, 0.0), (17, 0, 1.0, 0.0), (8, 1, 1.0, 0.0), (10, 7, 1.0, 0.0), (10, -1, 1.0, 0.0),
                                       (10, 6, 0.0, 0.0), (10, 6, NAN, 0.0), (10, 6, INF, 0.0), (10, 6, 1.0, NAN), (10, 6, 1.0, -INF)):
        with pytest.raises(pkg.JincError) as e:
            pkg.debug_narrow_scaled(v, bits, shift, scale, offset, device=0)
        assert e.value.code == INVALID_ARG
        with pytest.raises(pkg.JincError) as e:
            pkg.debug_widen_scaled(raw, bits, shift, scale, offset, device=0)
        assert e.value.code == INVALID_ARG
    with pytest.raises(pkg.JincError) as e:
        pkg.debug_widen_scaled(raw, 10, 6, 1.0, 0.0, out_kind=2, device=0)   # (2 is no sample type)
    assert e.value.code == INVALID_ARG
    with pytest.raises(TypeError):
        pkg.debug_narrow_scaled(v, 8, 0, 1.0, 0.0, bfloat16=True)


# ---- jinc_code_range ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 10, 12, 16])
def test_code_range_is_the_table_rounded_once(pkg, bits):
    k = 1 << (bits - 8)
    table = {(pkg.RANGE_LIMITED, pkg.PLANE_LUMA_OR_RGB): (219 * k, 16 * k), (pkg.RANGE_LIMITED, pkg.PLANE_CHROMA): (224 * k, 128 * k),
             (pkg.RANGE_FULL, pkg.PLANE_LUMA_OR_RGB): ((1 << bits) - 1, 0), (pkg.RANGE_FULL, pkg.PLANE_CHROMA): ((1 << bits) - 1, 1 << (bits - 1))}
    for (rng, kind), (den, zero) in table.items():
        got = pkg.code_range(bits, rng, kind)
        want = (np.float32(1.0 / den), np.float32(-float(zero) / den), np.float32(den), np.float32(zero))
        assert [np.float32(g).view(np.uint32) for g in got] == [w.view(np.uint32) for w in want], (bits, rng, kind, got, want)
        assert float(got[2]) == den and float(got[3]) == zero   # (exact)
        # there and back: the code value itself for every value of the depth
        v = np.arange(1 << bits, dtype=np.float32)
        there = ((v * got[0]).astype(np.float32) + got[1]).astype(np.float32)
        back = np.rint(((there * got[2]).astype(np.float32) + got[3]).astype(np.float32))
        assert np.array_equal(back, v), (bits, rng, kind)


def test_code_range_takes_null_pointers_and_refuses_bad_arguments(pkg):
    L = pkg.lib()
    assert L.jinc_code_range(10, 1, 0, None, None, None, None) == 0
    s = C.c_float()
    assert L.jinc_code_range(10, 1, 0, None, None, C.byref(s), None) == 0 and s.value == 876.0
    assert L.jinc_code_range(10, 1, 1, None, C.byref(s), None, None) == 0 and np.float32(s.value) == np.float32(-512.0 / 896.0)
    messages = set()
    for bits, rng, kind in ((7, 0, 0), (17, 0, 0), (0, 1, 1), (8, 2, 0), (8, -1, 0), (8, 0, 2), (8, 0, -1)):
        s = C.c_float(123.0)
        assert L.jinc_code_range(bits, rng, kind, C.byref(s), None, None, None) == INVALID_ARG, (bits, rng, kind)
        assert s.value == 123.0
        messages.add("".join(ch for ch in L.jinc_last_error().decode() if not ch.isdigit() and ch != "-"))
        with pytest.raises(pkg.JincError):
            pkg.code_range(bits, rng, kind)
    assert len(messages) == 3, messages   # bits, range, plane kind


# ---- the row functions ------------------------------------------------------------------------------------------------------------------------------

WIDTHS = set(range(1, 71))


def _build_and_run(tmp_path, program, tag, extra):
    header = os.path.join(PKG, "csrc", f"{program}_rows.h")
    assert os.path.exists(header), f"csrc/{program}_rows.h is missing"
    exe, out_file = str(tmp_path / f"{program}_scaled_rows_{tag}"), str(tmp_path / f"{program}_scaled_rows_{tag}.bin")
    subprocess.run([CXX, "-g", "-std=c++17", "-ffp-contract=off", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", *extra,
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "host_sanitizer", f"{program}_scaled_rows_main.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, out_file], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out and "LeakSanitizer" not in out, out[-4000:]
    return out, np.fromfile(out_file, np.uint8)


def _check_widen_against_numpy(out, blob):
    pos, cases, seen, exhaustive = 0, 0, set(), {}
    while pos < blob.size:
        sb, n, ob, kind, bits, width, rows, unit, given, *rest = blob[pos:pos + 64].view(np.uint32).tolist()
        shifts = rest[:4]
        scales, offsets = blob[pos + 64:pos + 80].view(np.float32), blob[pos + 80:pos + 96].view(np.float32)
        pos += 96
        raw = blob[pos:pos + rows * width * n * sb].view(np.uint8 if sb == 1 else np.uint16).reshape(rows, width, n).astype(np.uint32)
        pos += rows * width * n * sb
        what = f"SB {sb} N {n} OB {ob} KIND {kind} bits {bits} shifts {shifts[:n]} width {width} unit {unit} given {given:#x}"
        assert (ob, kind) in ((4, 0), (2, HALF), (2, BF16)), what
        for c in range(n):
            if not given >> c & 1:
                continue
            got = blob[pos:pos + rows * width * ob].view(np.uint32 if ob == 4 else np.uint16).reshape(rows, width)
            pos += rows * width * ob
            value = (raw[:, :, c] >> shifts[c]) & ((1 << bits) - 1)
            want = widened_definition(value, scales[c], offsets[c], kind)
            bad = np.argwhere(got != want)
            assert len(bad) == 0, f"{what}: plane {c} (scale {scales[c]!r}, offset {offsets[c]!r}) differs at {len(bad)} samples; first x={bad[0][1]}: " \
                                  f"value {value[bad[0][0], bad[0][1]]}, got {got[bad[0][0], bad[0][1]]:#x}, want {want[bad[0][0], bad[0][1]]:#x}"
            if rows == 1 and np.unique(value).size == 1 << bits:
                exhaustive.setdefault((kind, bits), set()).add((float(scales[c]), float(offsets[c])))
                if kind == HALF and bits == 16:
                    h = want.view(np.float16)
                    exhaustive.setdefault("half", set()).update({"sub"} if ((h != 0) & (np.abs(h) < 6.1e-5)).any() else set())
                    exhaustive["half"].update({"inf"} if np.isinf(h).any() else set())
        if rows > 1:
            seen.add((sb, n, kind, bits, width, unit, given == (1 << n) - 1))
        cases += 1
    assert pos == blob.size
    assert f"widen scaled rows: {cases} cases, 0 wrong" in out, out[-2000:]
    for sb, depths in ((1, (8,)), (2, (10, 16))):
        for n in (1, 2, 3, 4):
            for kind in (0, HALF, BF16):
                for bits in depths:
                    for unit in (16, 4, 0):
                        for complete in ((True,) if n == 1 else (True, False)):
                            have = {w for (a, b, k, d, w, u, full) in seen if (a, b, k, d, u, full) == (sb, n, kind, bits, unit, complete)}
                            assert have == WIDTHS, (sb, n, kind, bits, unit, complete)
    for kind in (0, HALF, BF16):   # every 16-bit value at four pairs, every 10-bit value at the two limited-range pairs
        assert len(exhaustive[(kind, 16)]) == 4 and len(exhaustive[(kind, 10)]) == 2, exhaustive
    assert exhaustive["half"] == {"sub", "inf"}   # binary16 subnormals and the overflow to inf were among them
    return cases


def _check_narrow_against_numpy(out, blob):
    pos, cases, seen, clamped = 0, 0, set(), [0, 0, 0]
    while pos < blob.size:
        kind, n, db, bits, width, rows, unit, given, s0, s1, s2, s3, lead, pitch, dst_bytes, _ = blob[pos:pos + 64].view(np.uint32).tolist()
        shifts = [s0, s1, s2, s3]
        scales, offsets = blob[pos + 64:pos + 80].view(np.float32), blob[pos + 80:pos + 96].view(np.float32)
        pos += 96
        ib = 4 if kind == 0 else 2
        peak = (1 << bits) - 1
        what = f"kind {kind} N {n} DB {db} bits {bits} shifts {shifts[:n]} width {width} unit {unit} given {given:#x}"
        want = np.full(dst_bytes, 0xA5, np.uint8)   # the canary: every byte that is no given sample keeps it
        for c in range(n):
            if not given >> c & 1:
                continue
            raw = blob[pos:pos + rows * width * ib].copy()
            pos += rows * width * ib
            if kind == 0:
                r = raw.view(np.float32)
            elif kind == HALF:
                r = raw.view(np.float16).astype(np.float32)
            else:
                r = (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32)
            value = narrowed_definition(r.reshape(rows, width), scales[c], offsets[c], peak)
            clamped[0] += int((value == 0).sum())
            clamped[1] += int((value == peak).sum())
            clamped[2] += value.size
            v = (value << shifts[c]).astype(np.uint8 if db == 1 else np.uint16)
            for byte in range(db):
                np.ndarray((rows, width), np.uint8, want, lead + c * db + byte, (pitch, n * db))[...] = (v >> (8 * byte)).astype(np.uint8)
        got = blob[pos:pos + dst_bytes]
        pos += dst_bytes
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{what}: {bad.size} destination bytes differ, first at byte {int(bad[0])} (lead {lead}, pitch {pitch}): " \
                              f"got {int(got[bad[0]])}, want {int(want[bad[0]])}"
        if rows > 1:
            seen.add((kind, n, db, shifts[0], width, unit, given == (1 << n) - 1))
        else:
            seen.add((kind, 1, db, shifts[0], "values", unit, bits))
        cases += 1
    assert pos == blob.size
    assert f"narrow scaled rows: {cases} cases, 0 wrong" in out, out[-2000:]
    print(f"{clamped[0]} samples at 0, {clamped[1]} at the peak, of {clamped[2]}")
    assert clamped[0] > 1000 and clamped[1] > 1000   # (both clamps had work)
    for kind in (0, HALF, BF16):
        for n in (1, 2, 3, 4):
            for db in (1, 2):
                for shift in ((0,) if db == 1 else (0, 6)):
                    for unit in (16, 4, 0):
                        for complete in ((True,) if n == 1 else (True, False)):
                            have = {w for (k, a, b, s, w, u, full) in seen if (k, a, b, s, u, full) == (kind, n, db, shift, unit, complete)}
                            assert have == WIDTHS, (kind, n, db, shift, unit, complete)
        for bits in (8, 10, 12, 16):
            for unit in (16, 0):
                assert (kind, 1, 1 if bits == 8 else 2, (8 if bits == 8 else 16) - bits, "values", unit, bits) in seen, (kind, bits, unit)
    return cases


CHECKS = {"widen": _check_widen_against_numpy, "narrow": _check_narrow_against_numpy}


@pytest.mark.parametrize("program", ["widen", "narrow"])
def test_scaled_row_function_equals_numpy(tmp_path, program):
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not found")
    out, blob = _build_and_run(tmp_path, program, "plain", ["-O2"])
    print(CHECKS[program](out, blob), "cases")


@pytest.mark.parametrize("program", ["widen", "narrow"])
def test_scaled_row_function_is_clean_under_asan_ubsan(tmp_path, program):
    """The same programs as stand-alone executables with -fsanitize=address,undefined: nothing preloaded, nothing loaded into Python.
    Their buffers end where the contract says the accesses end."""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not found")
    out, blob = _build_and_run(tmp_path, program, "san", ["-O1", "-fsanitize=address,undefined"])
    print(CHECKS[program](out, blob), "cases")


def test_the_unscaled_row_programs_still_compile_untouched(tmp_path):
    """widen_row and narrow_row took a trailing template parameter: the programs written for four and three parameters build as they are."""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not found")
    for program in ("widen_rows_main.cpp", "widen_rows_bf16_main.cpp", "narrow_rows_main.cpp"):
        subprocess.run([CXX, "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(PKG, "csrc"),
                        os.path.join(ROOT, "tests", "host_sanitizer", program)], check=True)
