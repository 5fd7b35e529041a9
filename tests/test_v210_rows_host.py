"""The row functions of the v210 kernels (csrc/v210_rows.h) on the CPU under AddressSanitizer + UndefinedBehaviorSanitizer: a
stand-alone program (tests/host_sanitizer/v210_rows_main.cpp, its own main; nothing is loaded into Python) runs exactly the code
the kernels run, lane by lane and trip by trip, for every even width from 2 to 800 (more than two wave-trips of 384 pixels), both
directions, both access units and 1 .. 3 rows, on buffers allocated to exactly the bytes the contract allows to be touched, and
compares with a scalar decoder / encoder of its own."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "avisynth-jincresize_amd")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
CASES = 400 * 3 * 2 * 2   # widths x rows x access units x directions


def test_v210_row_functions_are_clean_under_asan_ubsan(tmp_path):
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not found")
    header = os.path.join(PKG, "csrc", "v210_rows.h")
    assert os.path.exists(header), "csrc/v210_rows.h is missing"
    exe = str(tmp_path / "v210_rows")
    subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "host_sanitizer", "v210_rows_main.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert f"v210 rows: {CASES} cases, 0 wrong" in out, out[-4000:]
