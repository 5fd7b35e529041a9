"""Host side of jinc_filter_process_device_narrowed_packed10 / _narrowed_v210 (the results of fp32 / binary16 / bfloat16 filters into
Y410 / RGB10A2 words and v210 blocks): the exports, the mirrors and the headers; every refusal that needs no device, each with a
message of its own, on filters created with device = -1; and the row functions of narrow_fields_kernel and narrow_v210_kernel
(csrc/narrow_fields_rows.h, csrc/narrow_v210_rows.h) in stand-alone host programs (tests/host_sanitizer/narrow_fields_rows_main.cpp,
narrow_v210_rows_main.cpp: their own main; nothing is loaded into Python), built once plain and once under AddressSanitizer +
UndefinedBehaviorSanitizer, whose every destination byte is compared with numpy's rint(clip(fl32(fl32(r * scale) + offset), 0, 1023))
packed into words / blocks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

INVALID_ARG, NO_DEVICE = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "avisynth-jincresize_amd")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
GEOM = (40, 24, 80, 48)                                  # the destination is 80 x 48
Y410, R10G10B10A2, BGRX1010102, ODD = [10, 0, 20], [10, 20, 0], [12, 22, 2], [22, 0, 11]   # ODD: a legal word no format uses
ROW_V210 = 16 * ((80 + 5) // 6)   # 224 bytes
NAN, INF = float("nan"), float("inf")
KIND_HALF, KIND_BF16 = 1, 2                              # csrc/kernels.h kSampleHalf, kSampleBFloat16


def test_the_entries_are_exported_declared_and_mirrored(pkg):
    header = open(pkg.HEADER_PATH).read()
    test_header = open(os.path.join(os.path.dirname(pkg.HEADER_PATH), "jincresize_hip_test.h")).read()
    for name, method in (("jinc_filter_process_device_narrowed_packed10", "process_device_narrowed_packed10"),
                         ("jinc_filter_process_device_narrowed_v210", "process_device_narrowed_v210")):
        assert name in pkg.EXPORTS and hasattr(pkg.lib(), name)
        assert name + "(" in header
        assert hasattr(pkg.Filter, method)
    for name, mirror in (("jinc_debug_narrow_fields", "debug_narrow_fields"), ("jinc_debug_narrow_v210", "debug_narrow_v210")):
        assert name in pkg.EXPORTS and hasattr(pkg.lib(), name) and hasattr(pkg, mirror)
        assert name + "(" in test_header and name not in header    # the hooks are declared in the test header only
    assert "are no destinations of this call" not in header
    assert "10 narrow_fields, 11 narrow_v210" in test_header


# ---- the argument surface --------------------------------------------------------------------------------------------------------------

def _call(f, kind, offsets=Y410, ptr=4096, pitch=None, stride=0, src_steps=None, nframes=1, fill=0, scales=None, adds=None, src_ptrs=None):
    """An 80 x 48 destination unless told otherwise; the pointers are never dereferenced."""
    n = f.fmt.planes
    src = (src_ptrs or [1 << 20, 2 << 20, 3 << 20, 4 << 20][:n], [512] * n, src_steps, [1 << 18] * n)
    if kind == "packed10":
        f.process_device_narrowed_packed10(*src, ptr, 320 if pitch is None else pitch, offsets, fill, scales, adds, stride, nframes)
    else:
        f.process_device_narrowed_v210(*src, ptr, 256 if pitch is None else pitch, scales, adds, stride, nframes)


# (call, filter, call arguments, what the message must say)
REFUSALS = [
    ("packed10", "YUV444P10", dict(), "fp32, binary16 or bfloat16 filter"),
    ("packed10", "RGBP8", dict(), "fp32, binary16 or bfloat16 filter"),
    ("packed10", "RGBAPS", dict(), "three components"),
    ("packed10", "YUV420PS", dict(), "three components"),
    ("packed10", "YUV422PH", dict(), "three components"),
    ("packed10", "Y32", dict(), "three components"),
    ("packed10", "YUV444PS", dict(offsets=[-1, 10, 20]), "0..22"),
    ("packed10", "YUV444PS", dict(offsets=[10, 0, 23]), "0..22"),
    ("packed10", "YUV444PH", dict(offsets=[10, 0, 19]), "overlap"),
    ("packed10", "RGBPS", dict(offsets=[5, 5, 20]), "overlap"),
    ("packed10", "YUV444PS", dict(src_steps=[1, 5, 1]), "step"),
    ("packed10", "RGBPS", dict(src_steps=[0, 3, 3]), "step"),
    ("packed10", "YUV444PS", dict(ptr=4098), "aligned"),
    ("packed10", "YUV444PS", dict(pitch=322), "pitch 322 "),
    ("packed10", "YUV444PS", dict(stride=320 * 48 + 2, nframes=2), "frame stride"),
    ("packed10", "YUV444PS", dict(pitch=316), "pitch 316 "),
    ("packed10", "YUV444PS", dict(scales=[NAN, 1, 1]), "scale of packed 10-bit destination plane 0 is NaN"),
    ("packed10", "YUV444PH", dict(scales=[1, INF, 1]), "scale of packed 10-bit destination plane 1 is infinite"),
    ("packed10", "YUV444PS", dict(scales=[1, 1, 0.0]), "scale of packed 10-bit destination plane 2 is zero"),
    ("packed10", "RGBPS", dict(adds=[0, NAN, 0]), "offset of packed 10-bit destination plane 1 is NaN"),
    ("packed10", "YUV444PS", dict(adds=[0, 0, -INF]), "offset of packed 10-bit destination plane 2 is infinite"),
    ("v210", "YUV422P10", dict(), "fp32, binary16 or bfloat16 filter"),
    ("v210", "YUV422P8", dict(), "fp32, binary16 or bfloat16 filter"),
    ("v210", "YUVA422PS", dict(), "three components"),
    ("v210", "YUV444PS", dict(), "three components"),
    ("v210", "YUV420PH", dict(), "three components"),
    ("v210", "Y32", dict(), "three components"),
    ("v210", "YUV422PS", dict(src_steps=[1, 1, 5]), "step"),
    ("v210", "YUV422PH", dict(src_steps=[0, 1, 1]), "step"),
    ("v210", "YUV422PS", dict(ptr=4097), "aligned"),
    ("v210", "YUV422PS", dict(pitch=226), "pitch 226 "),
    ("v210", "YUV422PS", dict(stride=256 * 48 + 2, nframes=2), "frame stride"),
    ("v210", "YUV422PS", dict(pitch=ROW_V210 - 4), f"pitch {ROW_V210 - 4} "),
    ("v210", "YUV422PS", dict(scales=[NAN, 1, 1]), "scale of v210 destination plane 0 is NaN"),
    ("v210", "YUV422PH", dict(scales=[1, -INF, 1]), "scale of v210 destination plane 1 is infinite"),
    ("v210", "YUV422PS", dict(scales=[1, 1, -0.0]), "scale of v210 destination plane 2 is zero"),
    ("v210", "YUV422PS", dict(adds=[NAN, 0, 0]), "offset of v210 destination plane 0 is NaN"),
    ("v210", "YUV422PS", dict(adds=[0, INF, 0]), "offset of v210 destination plane 1 is infinite"),
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


# interleaved float RGB as source: G = p + 4, B = p + 8, R = p, step 3
RGB_SRC = dict(src_ptrs=[(1 << 20) + 4, (1 << 20) + 8, 1 << 20], src_steps=[3, 3, 3])
ACCEPTED = [
    ("packed10", "YUV444PS", dict()),
    ("packed10", "YUV444PH", dict(scales=[876.0, 896.0, 896.0], adds=[64.0, 512.0, 512.0])),
    ("packed10", "YUV444PBF", dict(fill=0xC0000000)),
    ("packed10", "RGBPS", dict(offsets=R10G10B10A2, fill=0xFFFFFFFF)),
    ("packed10", "RGBPS", dict(offsets=BGRX1010102, **RGB_SRC)),
    ("packed10", "RGBPH", dict(offsets=ODD, scales=[-1.0, 1.0, 1.0])),
    ("packed10", "YUV444PS", dict(pitch=324, ptr=4100, stride=324 * 48 + 4, nframes=2)),   # multiples of 4 only
    ("packed10", "YUV444PS", dict(stride=2)),                                             # one frame: the frame stride is not read
    ("v210", "YUV422PS", dict()),
    ("v210", "YUV422PH", dict(adds=[64.0, 512.0, 512.0])),
    ("v210", "YUV422PBF", dict(scales=[876.0, 896.0, 896.0])),
    ("v210", "YUV422PS", dict(pitch=ROW_V210)),                                           # the smallest pitch
    ("v210", "YUV422PS", dict(pitch=ROW_V210 + 4, ptr=4100, stride=(ROW_V210 + 4) * 48 + 4, nframes=2)),
    ("v210", "YUV422PH", dict(stride=2, src_steps=[1, 2, 2])),
]
# ... and five named layouts (offsets and opaque fill from packed10_layout) on a bfloat16 filter
ACCEPTED += [("packed10", "RGBPBF", dict(offsets=name)) for name in ("Y410", "R10G10B10A2", "ARGB2101010", "RGBA1010102", "BGRX1010102")]


@pytest.mark.parametrize("kind,name,kw", ACCEPTED, ids=[f"{k}_{n}_{i}" for i, (k, n, _) in enumerate(ACCEPTED)])
def test_accepted_arguments_reach_the_device_check(pkg, kind, name, kw):
    sw, sh, tw, th = GEOM
    kw = dict(kw)
    if isinstance(kw.get("offsets"), str):
        kw["offsets"], kw["fill"] = pkg.packed10_layout(kw["offsets"])
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=-1)
    with pytest.raises(pkg.JincError) as e:
        _call(f, kind, **kw)
    assert e.value.code == NO_DEVICE, str(e.value)
    f.close()


def test_null_arguments_come_after_the_refusals(pkg):
    sw, sh, tw, th = GEOM
    L = pkg.lib()
    last = lambda: L.jinc_last_error().decode()
    P4, I4 = C.c_void_p * 4, C.c_int * 4
    src, pitches = P4(1 << 20, 2 << 20, 3 << 20, 0), I4(512, 512, 512, 0)
    off, bad_off, nan = (C.c_int * 3)(*Y410), (C.c_int * 3)(10, 0, 23), (C.c_float * 3)(NAN, 1, 1)
    f = pkg.Filter(pkg.FORMATS["YUV444PS"], sw, sh, tw, th, device=-1)
    call = L.jinc_filter_process_device_narrowed_packed10
    dst = C.c_void_p(4096)
    assert call(f._h, None, pitches, None, None, dst, 320, off, 0, None, None, 0, 1, C.c_void_p(0)) == INVALID_ARG and "null argument" in last()
    assert call(f._h, src, None, None, None, dst, 320, off, 0, None, None, 0, 1, C.c_void_p(0)) == INVALID_ARG and "null argument" in last()
    assert call(f._h, src, pitches, None, None, None, 320, off, 0, None, None, 0, 1, C.c_void_p(0)) == INVALID_ARG and "null argument" in last()
    assert call(f._h, src, pitches, None, None, dst, 320, None, 0, None, None, 0, 1, C.c_void_p(0)) == INVALID_ARG and "null argument" in last()
    assert call(f._h, None, None, None, None, dst, 320, bad_off, 0, None, None, 0, 1, C.c_void_p(0)) == INVALID_ARG and "0..22" in last()
    assert call(f._h, None, None, None, None, dst, 316, off, 0, None, None, 0, 1, C.c_void_p(0)) == INVALID_ARG and "pitch 316 " in last()
    assert call(f._h, None, None, None, None, dst, 320, off, 0, nan, None, 0, 1, C.c_void_p(0)) == INVALID_ARG and "is NaN" in last()
    assert call(f._h, src, pitches, None, None, dst, 320, off, 0, None, None, 0, 1, C.c_void_p(0)) == NO_DEVICE
    f.close()
    f = pkg.Filter(pkg.FORMATS["YUV422PS"], sw, sh, tw, th, device=-1)
    call = L.jinc_filter_process_device_narrowed_v210
    assert call(f._h, None, pitches, None, None, dst, 256, None, None, 0, 1, C.c_void_p(0)) == INVALID_ARG and "null argument" in last()
    assert call(f._h, src, pitches, None, None, None, 256, None, None, 0, 1, C.c_void_p(0)) == INVALID_ARG and "null argument" in last()
    assert call(f._h, None, None, None, None, C.c_void_p(4098), 256, None, None, 0, 1, C.c_void_p(0)) == INVALID_ARG and "aligned" in last()
    assert call(f._h, src, pitches, None, None, dst, 256, None, None, 0, 1, C.c_void_p(0)) == NO_DEVICE
    f.close()


# ---- the row functions -------------------------------------------------------------------------------------------------------------------

def _build_and_run(tmp_path, program, tag, extra):
    for header in ("narrow_fields_rows.h", "narrow_v210_rows.h"):
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


def as_float32(raw, kind):
    """The samples of a plane as the fp32 values the pass converts (exact widening)."""
    if kind == 0:
        return raw.view(np.float32)
    if kind == KIND_HALF:
        return raw.view(np.float16).astype(np.float32)
    return (raw.view(np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def codes(values, scaled, scale, offset):
    """rint(clip(fl32(fl32(r * scale) + offset), 0, 1023)), round half to even; NaN, -inf and -0 -> 0, +inf -> 1023."""
    with np.errstate(all="ignore"):
        t = values
        if scaled:
            t = (t * np.float32(scale)).astype(np.float32)
            t = (t + np.float32(offset)).astype(np.float32)
        clamped = np.where(t > 0, np.minimum(t, np.float32(1023)), np.float32(0))   # (a NaN compares false: 0)
        return np.rint(clamped).astype(np.uint32)


FIELD_WIDTHS = set(range(1, 71)) | {1031}
CANARY = 0xA5


def _check_fields_against_numpy(out, blob):
    pos, cases, seen, long_rows = 0, 0, set(), set()
    while pos < blob.size:
        head = blob[pos:pos + 96].view(np.uint32)
        kind, scaled, width, rows, unit, o0, o1, o2, fill, lead, pitch, dst_bytes = head[:12].tolist()
        scale, offset = head[12:15].view(np.float32), head[15:18].view(np.float32)
        pos += 96
        ib = 4 if kind == 0 else 2
        want = np.full((rows, width), fill, np.uint32)
        for c, o in enumerate((o0, o1, o2)):
            raw = blob[pos:pos + rows * width * ib]
            pos += rows * width * ib
            want |= codes(as_float32(raw, kind).reshape(rows, width), scaled, scale[c], offset[c]) << np.uint32(o)
        dst = blob[pos:pos + dst_bytes]
        pos += dst_bytes
        image = np.full(dst_bytes, CANARY, np.uint8)   # every destination byte: the words, and the canary everywhere else
        for row in range(rows):
            image[lead + row * pitch: lead + row * pitch + 4 * width] = want[row].astype("<u4").view(np.uint8)
        what = f"kind {kind} scaled {scaled} width {width} rows {rows} unit {unit} offsets {(o0, o1, o2)} fill {fill:#x}"
        assert np.array_equal(dst, image), f"{what}: {int((dst != image).sum())} destination bytes differ"
        assert (lead, pitch % 16) == ((0, 0) if unit == 16 else (4, 4)), what
        if width in FIELD_WIDTHS:
            seen.add((kind, scaled, unit, rows, (o0, o1, o2), width))
        if width > 1031:
            long_rows.add((kind, scaled, unit))
        cases += 1
    assert pos == blob.size
    assert f"narrow fields rows: {cases} cases, 0 wrong" in out, out[-2000:]
    for kind in (0, KIND_HALF, KIND_BF16):
        for scaled in (0, 1):
            for unit in (16, 4):
                assert (kind, scaled, unit) in long_rows, (kind, scaled, unit)   # the ties / all 65536 patterns
                for rows in (1, 2, 3):
                    for offsets in (Y410, ODD):
                        assert {w for (k, s, u, r, o, w) in seen if (k, s, u, r, o) == (kind, scaled, unit, rows, tuple(offsets))} >= FIELD_WIDTHS, (kind, scaled, unit, rows, offsets)
    return cases


# (plane, sample of the block, word, bit offset) of a v210 block's twelve fields, from the table in include/jincresize_hip.h
V210_FIELDS = [(1, 0, 0, 0), (0, 0, 0, 10), (2, 0, 0, 20),
               (0, 1, 1, 0), (1, 1, 1, 10), (0, 2, 1, 20),
               (2, 1, 2, 0), (0, 3, 2, 10), (1, 2, 2, 20),
               (0, 4, 3, 0), (2, 2, 3, 10), (0, 5, 3, 20)]


def v210_blocks(planes):
    """The blocks of rows of codes: planes = (luma (rows, width), cb (rows, width / 2), cr); returns (rows, blocks, 4) uint32 with
    zeros in bits 30 - 31 and in the fields of a partial last block beyond the width."""
    rows, width = planes[0].shape
    nblocks = (width + 5) // 6
    words = np.zeros((rows, nblocks, 4), np.uint32)
    for plane, j, word, offset in V210_FIELDS:
        x = (6 if plane == 0 else 3) * np.arange(nblocks) + j
        valid = x < planes[plane].shape[1]
        words[:, valid, word] |= planes[plane][:, x[valid]].astype(np.uint32) << np.uint32(offset)
    return words


def _check_v210_against_numpy(out, blob):
    pos, cases, seen, long_rows = 0, 0, set(), set()
    while pos < blob.size:
        head = blob[pos:pos + 64].view(np.uint32)
        kind, scaled, width, rows, unit, lead, pitch, dst_bytes = head[:8].tolist()
        scale, offset = head[8:11].view(np.float32), head[11:14].view(np.float32)
        pos += 64
        ib = 4 if kind == 0 else 2
        planes = []
        for c, w in enumerate((width, width // 2, width // 2)):
            raw = blob[pos:pos + rows * w * ib]
            pos += rows * w * ib
            planes.append(codes(as_float32(raw, kind).reshape(rows, w), scaled, scale[c], offset[c]))
        want = v210_blocks(planes)
        row_bytes = 16 * ((width + 5) // 6)
        dst = blob[pos:pos + dst_bytes]
        pos += dst_bytes
        image = np.full(dst_bytes, CANARY, np.uint8)
        for row in range(rows):
            image[lead + row * pitch: lead + row * pitch + row_bytes] = want[row].astype("<u4").reshape(-1).view(np.uint8)
        what = f"kind {kind} scaled {scaled} width {width} rows {rows} unit {unit}"
        assert np.array_equal(dst, image), f"{what}: {int((dst != image).sum())} destination bytes differ"
        if width <= 800:
            seen.add((kind, scaled, unit, rows, width))
        else:
            long_rows.add((kind, scaled, unit))
        cases += 1
    assert pos == blob.size
    assert f"narrow v210 rows: {cases} cases, 0 wrong" in out, out[-2000:]
    kinds = (0, KIND_HALF, KIND_BF16)
    assert seen == {(k, s, u, r, w) for k in kinds for s in (0, 1) for u in (16, 4) for r in (1, 2, 3) for w in range(2, 801, 2)}
    assert long_rows == {(k, s, u) for k in kinds for s in (0, 1) for u in (16, 4)}
    return cases


PROGRAMS = [("narrow_fields_rows", _check_fields_against_numpy), ("narrow_v210_rows", _check_v210_against_numpy)]


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
