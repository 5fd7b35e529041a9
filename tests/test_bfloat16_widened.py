"""8-bit device surfaces into bfloat16 filters through jinc_filter_process_device_widened -- NV12 into YUV420PBF, BGRA8 into RGBPBF,
planar YUV444P8 into YUV444PBF: the decoder-to-network case the type exists for.  The result must be, bit for bit, what
jinc_filter_process_device computes on the same filter for dense bfloat16 planes holding the source's values (every integer up to 256
is exact in bfloat16: the planes are built on the host with the definition's narrow(), tests/test_bfloat16_host.py), the source must
come back unchanged, the destination's guard bytes must keep their value (test_strided.py's Side), and last_strided reports the
launch counts the binary16 filter of the same call reports.

Shapes, the smallest of tests/test_widened.py: 262 x 38 -> 524 x 76 (a luma row of 16 whole lanes' pixels and a tail of 6, an odd 4:2:0
chroma row of 131 pixels, several row blocks) and 273 x 22 -> 546 x 44 (17 whole lanes' pixels and a tail of ONE pixel, an odd width);
source alignment 16, 4 and 1 -- the last with a pitch that is no multiple of 4.

The row function's bfloat16 form (csrc/widen_rows.h, widen_row<1, N, 2, kSampleBFloat16>) also runs in a stand-alone host program
with its own main (tests/host_sanitizer/widen_rows_bf16_main.cpp), lane by lane on exactly sized buffers, plain and under
-fsanitize=address,undefined; numpy checks its output.  Nothing is preloaded and nothing is loaded into Python.  Those two tests need
no GPU."""
import os
import subprocess

import numpy as np
import pytest

from test_bfloat16_host import assert_bf16_equal, definition, narrow, widen
from test_strided import packed, planar, run_planar, semi_planar
from test_widened import assert_source_unchanged, call, make_sides, raw_of, values
from test_widened_host import CXX, PKG, ROOT

gpu = pytest.mark.gpu

GEOM = (262, 38, 524, 76)
GEOM_TAIL1 = (273, 22, 546, 44)
KW = dict(tap=3)
BGRA = packed("BGRA", 4, 3)

# (id, bfloat16 filter, its binary16 twin, geometry, source layout, destination layout or None = planar, (widen, merge, slices))
CASES = [
    ("nv12", "YUV420PBF", "YUV420PH", GEOM, semi_planar(), None, (2, 0, 1)),
    ("bgra8", "RGBPBF", "RGBPH", GEOM_TAIL1, BGRA, None, (1, 0, 1)),
    ("bgra8_rgb", "RGBPBF", "RGBPH", GEOM_TAIL1, BGRA, packed("RGB", 3, 3), (1, 1, 1)),   # interleaved bfloat16 RGB out through the merge
    ("yuv444p8", "YUV444PBF", "YUV444PH", GEOM_TAIL1, planar(3), None, (1, 0, 1)),
]


def _widened(torch, pkg, name, geom, raw, src_layout, dst_layout, n, align, what):
    sw, sh, tw, th = geom
    f = pkg.Filter(pkg.FORMATS[name], sw, sh, tw, th, device=0, **KW)
    src, dst = make_sides(torch, f, raw, src_layout, dst_layout or planar(f.fmt.planes), n, src_align=align)
    s = torch.cuda.current_stream()
    call(f, src, dst, None, 8, n, s)
    s.synchronize()
    report = f.last_strided()
    got = dst.frames_and_guards(what)
    assert_source_unchanged(src, what)
    return f, got, report


@gpu
@pytest.mark.parametrize("align", [16, 4, 1])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_equals_the_planar_call_on_bfloat16_planes(gpu_pkg, case, n, align):
    torch = pytest.importorskip("torch")
    _, name, half_name, geom, src_layout, dst_layout, expect = case
    sw, sh, tw, th = geom
    vals = values(gpu_pkg, name, sw, sh, 8, n)
    for planes in vals:   # the ends of the range in every plane
        for p in planes:
            p[0, 0], p[-1, -1] = 255, 0
    raw = raw_of(vals, 8, [0] * 3)
    what = f"8-bit {case[0]} -> {name} {sw}x{sh}->{tw}x{th} {n} frame(s) align {align}"
    f, got, report = _widened(torch, gpu_pkg, name, geom, raw, src_layout, dst_layout, n, align, what)
    print(f"{what}: last_strided {report}")
    dense = [[narrow(p.astype(np.float32)) for p in planes] for planes in vals]
    for planes, ints in zip(dense, vals):
        for p, v in zip(planes, ints):
            assert np.array_equal(widen(p), v.astype(np.float32))   # (exact: no 8-bit value is rounded)
    want = run_planar(torch, f, dense, n)
    for k in range(n):
        assert_bf16_equal(got[k], want[k], f.out_dims(), what=f"{what} frame {k} against the planar call")
    f.close()
    assert report[:3] == expect, report
    fh, _, report_h = _widened(torch, gpu_pkg, half_name, geom, raw, src_layout, dst_layout, n, align, what + " (binary16 twin)")
    fh.close()
    assert report[:3] == report_h[:3], (report, report_h)


@gpu
def test_nv12_into_bfloat16_equals_the_definition(gpu_pkg, O):
    """... and the planar call is the definition's: NV12 into YUV420PBF against narrow(oracle_fp32(values))."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = GEOM
    vals = values(gpu_pkg, "YUV420PBF", sw, sh, 8, 1, seed=8)
    f, got, report = _widened(torch, gpu_pkg, "YUV420PBF", GEOM, raw_of(vals, 8, [0] * 3), semi_planar(), None, 1, 16, "nv12 vs the oracle")
    dims = f.out_dims()
    f.close()
    want = definition(O, "YUV420PBF", sw, sh, tw, th, KW, [narrow(p.astype(np.float32)) for p in vals[0]])
    assert_bf16_equal(got[0], want, dims, what="NV12 into YUV420PBF against the definition")


@gpu
def test_wider_sources_and_word_sources_are_refused_on_a_device_filter(gpu_pkg):
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = GEOM
    f = gpu_pkg.Filter(gpu_pkg.FORMATS["YUV420PBF"], sw, sh, tw, th, device=0, **KW)
    vals = values(gpu_pkg, "YUV420PBF", sw, sh, 10, 1)
    src, dst = make_sides(torch, f, raw_of(vals, 10, [6] * 3), semi_planar(), planar(3), 1)
    with pytest.raises(gpu_pkg.JincError) as e:
        call(f, src, dst, [6] * 3, 10, 1, torch.cuda.current_stream())
    assert e.value.code == -1 and "not exact in bfloat16" in str(e.value)
    dst.frames_and_guards("refused call")   # nothing was written
    f.close()


# ---- the row function in a stand-alone program -------------------------------------------------------------------------------------------

WIDTHS = {1, 7, 15, 16, 17, 63, 64, 65, 1031}


def _build_and_run(tmp_path, tag, extra):
    exe, out_file = str(tmp_path / f"widen_rows_bf16_{tag}"), str(tmp_path / f"widen_rows_bf16_{tag}.bin")
    subprocess.run([CXX, "-g", "-std=c++17", "-ffp-contract=off", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", *extra,
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "host_sanitizer", "widen_rows_bf16_main.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, out_file], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out and "LeakSanitizer" not in out, out[-4000:]
    return out, np.fromfile(out_file, np.uint8)


def _check_against_numpy(out, blob):
    pos, cases, seen = 0, 0, set()
    while pos < blob.size:
        sb, n, ob, bits, width, rows, unit, given, *_ = blob[pos:pos + 64].view(np.uint32).tolist()
        assert (sb, ob, bits) == (1, 2, 8)
        pos += 64
        raw = blob[pos:pos + rows * width * n].reshape(rows, width, n)
        pos += rows * width * n
        what = f"N {n} width {width} unit {unit} given {given:#x}"
        for c in range(n):
            if not given >> c & 1:
                continue
            got = blob[pos:pos + rows * width * 2].view(np.uint16).reshape(rows, width)
            pos += rows * width * 2
            want = narrow(raw[:, :, c].astype(np.float32))
            assert np.array_equal(widen(want), raw[:, :, c].astype(np.float32))
            assert np.array_equal(got, want), f"{what}: plane {c} differs at {int((got != want).sum())} samples"
        seen.add((n, width, unit))
        cases += 1
    assert pos == blob.size
    assert f"widen rows bfloat16: {cases} cases, 0 wrong" in out, out[-2000:]
    for n in (1, 2, 3, 4):
        for unit in (16, 4, 0):
            assert {w for (a, w, u) in seen if (a, u) == (n, unit)} == WIDTHS, (n, unit)
    return cases


def test_bfloat16_row_function_equals_numpy(tmp_path):
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not found")
    out, blob = _build_and_run(tmp_path, "plain", ["-O2"])
    print(_check_against_numpy(out, blob), "cases")


def test_bfloat16_row_function_is_clean_under_asan_ubsan(tmp_path):
    """The same program as a stand-alone executable with -fsanitize=address,undefined: nothing preloaded, nothing loaded into Python.
    Its buffers end where the contract says the accesses end."""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not found")
    out, blob = _build_and_run(tmp_path, "san", ["-O1", "-fsanitize=address,undefined"])
    print(_check_against_numpy(out, blob), "cases")
