"""oracle/build_ref.py -- TEST INFRASTRUCTURE ONLY: compiles the reference implementation's four translation units together
with this project's mock AviSynth host (tests/mock_avs/mock_host.cpp) into oracle/_ref/libref_mock_avs.so, so that the
reference can be run through its real entry points (avisynth_c_plugin_init -> Create_JincResize -> GetFrame) by
tests/golden/make_reference_sweep.py and tests/test_reference_sweep_host.py.

The reference's location is the recipe's variable REFERENCE_DIR (environment JINC_REFERENCE_DIR).  Where that directory
does not exist the recipe keeps whatever oracle/_ref/ holds and succeeds: the recorded fixture
tests/golden/reference_sweep.json is then what the tests hold oracle and kernels to.  Nothing of the reference and nothing
under oracle/_ref/ is ever committed (.gitignore).

Flags are the reference's own per file (its CMakeLists.txt:57-61): -O2 everywhere, no ISA flag on JincResize.cpp, the
SSE4.1 / AVX2 / AVX-512 sets on the three SIMD files only.  -O2 on GCC is kept so that sin / cos of one argument merge into
sincos, which DESIGN.md section 2 describes as part of what the opt=0 result is.  std::execution::par runs on the serial
backend where TBB is absent (threads=1 then computes what threads=0 does).

Caveat: the reference is compiled against this project's declaration of the API (oracle/ref_compat/avisynth_c.h wrapping
plugin/compat/avisynth_c.h), not the SDK's.  Mock host and reference share that one header, so layouts agree by construction;
the binary pins arithmetic and argument handling, not binary compatibility with a real AviSynth+.
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REFERENCE_DIR = os.environ.get("JINC_REFERENCE_DIR", "/root/reference")
OUT_DIR = os.path.join(HERE, "_ref")
LIB = os.path.join(OUT_DIR, "libref_mock_avs.so")
COMPAT = os.path.join(HERE, "ref_compat")
MOCK_HOST = os.path.join(ROOT, "tests", "mock_avs", "mock_host.cpp")

COMMON = ["-O2", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-w"]
UNITS = (  # (file, the reference's COMPILE_OPTIONS for it)
    ("JincResize.cpp", []),
    ("resize_plane_sse41.cpp", ["-mfpmath=sse", "-msse4.1"]),
    ("resize_plane_avx2.cpp", ["-mavx2", "-mfma"]),
    ("resize_plane_avx512.cpp", ["-mavx512f", "-mavx512bw", "-mavx512dq", "-mavx512vl", "-mfma"]),
)


def build(reference_dir: str = REFERENCE_DIR, cxx: str = os.environ.get("CXX", "g++")) -> str | None:
    """Returns the library's path, or None where there is neither a reference to compile nor an earlier build."""
    src_dir = os.path.join(reference_dir, "src")
    if not os.path.isdir(src_dir):
        return LIB if os.path.exists(LIB) else None
    sources = [os.path.join(src_dir, name) for name, _ in UNITS]
    deps = sources + [os.path.join(src_dir, "JincResize.h"), MOCK_HOST, os.path.join(COMPAT, "avisynth_c.h"),
                      os.path.join(COMPAT, "avs", "minmax.h"), os.path.join(ROOT, "plugin", "compat", "avisynth_c.h"), __file__]
    if os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in deps):
        return LIB
    os.makedirs(OUT_DIR, exist_ok=True)
    objects = []
    jobs = []
    for (name, flags), src in zip(UNITS + (("mock_host.cpp", []),), sources + [MOCK_HOST]):
        obj = os.path.join(OUT_DIR, os.path.splitext(name)[0] + ".o")
        objects.append(obj)
        cmd = [cxx, *COMMON, *flags, "-I" + COMPAT, "-I" + src_dir, "-c", src, "-o", obj]
        jobs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for cmd, p in jobs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("oracle/_ref: " + " ".join(cmd) + " failed:\n" + out[-4000:])
    # -Bsymbolic + hidden visibility: this host's avs_* / mock_* never bind to those of another mock host in the process
    cmd = [cxx, "-shared", "-Wl,-Bsymbolic", "-o", LIB, *objects]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("oracle/_ref: linking failed:\n" + r.stderr[-4000:])
    nm = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    loose = [line.split()[-1] for line in nm.splitlines() if line.split()[-1].startswith(("avs_", "mock_", "avisynth_"))]
    if loose:
        raise RuntimeError(f"oracle/_ref: {os.path.basename(LIB)} leaves host symbols undefined: {loose}")
    return LIB


if __name__ == "__main__":
    path = build()
    print(path if path else "oracle/_ref: no reference directory and no earlier build; nothing to do")
    sys.exit(0)
