"""Generator (and shared case list) of tests/golden/reference_sweep.json -- TEST INFRASTRUCTURE ONLY.

Runs the reference implementation, as oracle/build_ref.py compiled it together with the mock AviSynth host into
oracle/_ref/libref_mock_avs.so, through its real entry points (avisynth_c_plugin_init -> Create_JincResize -> GetFrame)
over a fixed, seeded list of cases and records per case: format, sizes, script function and arguments (every float
argument as the float32 value a script hands over, decimal and bit pattern), the frame seed, opt, the host's CPU flags,
the output dimensions, one crc32 per output plane and the _ChromaLocation property of the output frame.

Only the mock_* interface of the binary is used; the reference's sources are never read.  The fixture holds parameters,
crcs and property values only.

    python tests/golden/make_reference_sweep.py            # rewrites the fixture
    python tests/golden/make_reference_sweep.py --check    # compares, exit status 1 on a difference

crc32s are taken over the visible part of each plane (rows cut to row_size).  On float planes every NaN is replaced by
the one pattern 0x7FC00000 first: x86 and the GPU disagree on NaN sign and payload, and the suite's rule is "same NaN
footprint, same bits elsewhere".
"""
from __future__ import annotations

import ctypes as C
import json
import os
import struct
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "reference_sweep.json")
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libref_mock_avs.so")

CPUF_SSE41, CPUF_AVX2, CPUF_AVX512F = 0x400, 0x2000, 0x10000
FLOAT_ARGS = ("src_left", "src_top", "src_width", "src_height", "blur", "initial_factor")
ALIAS_TAPS = {"Jinc36Resize": 3, "Jinc64Resize": 4, "Jinc144Resize": 6, "Jinc256Resize": 8}
QUIET_NAN = 0x7FC00000


def oracle():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    return entry.load_oracle()


# ------------------------------------------------------------------------------------------------------------------
# the mock host's C interface (tests/mock_avs/mock_host.cpp), for any library that links that host
# ------------------------------------------------------------------------------------------------------------------
def bind(L):
    vp, ci = C.c_void_p, C.c_int
    for name, res, args in (
        ("mock_env_new", vp, [ci, ci, ci]), ("mock_env_free", None, [vp]), ("mock_load_plugin", C.c_char_p, [vp]),
        ("mock_function_count", ci, [vp]), ("mock_function_name", C.c_char_p, [vp, ci]),
        ("mock_live_frames", C.c_long, [vp]), ("mock_live_clips", C.c_long, [vp]),
        ("mock_source_new", vp, [vp] + [ci] * 12), ("mock_source_frame", vp, [vp, ci]),
        ("mock_frame_plane", vp, [vp, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]),
        ("mock_invoke", vp, [vp, C.c_char_p, vp, ci, ci, ci, C.POINTER(C.c_char_p), C.c_char_p, C.POINTER(ci),
                             C.POINTER(C.c_double), C.POINTER(C.c_char_p)]),
        ("mock_value_error", C.c_char_p, [vp]), ("mock_value_clip", vp, [vp]), ("mock_value_free", None, [vp]),
        ("mock_clip_info", None, [vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]), ("mock_clip_get_frame", vp, [vp, ci]),
        ("mock_clip_error", C.c_char_p, [vp]), ("mock_clip_release", None, [vp]), ("mock_source_release", None, [vp]),
        ("mock_frame_prop_int", ci, [vp, C.c_char_p, C.POINTER(C.c_longlong)]), ("mock_frame_release", None, [vp]),
    ):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


_ref = None


def reference_library():
    """The reference under the mock host, loaded RTLD_LOCAL; None where oracle/_ref/ holds no build of it."""
    global _ref
    if _ref is None and os.path.exists(REF_LIB):
        _ref = bind(C.CDLL(REF_LIB, mode=os.RTLD_LOCAL | os.RTLD_NOW))
    return _ref


class Env:
    """One script environment of a mock host library with its plugin loaded."""

    def __init__(self, L, cpu_flags, version=10, bugfix=0):
        self.L = L
        self.env = L.mock_env_new(version, bugfix, cpu_flags)
        self.description = L.mock_load_plugin(self.env).decode()

    def source(self, fmt, w, h, planes, planar=1, chroma_location=-1):
        clip = self.L.mock_source_new(self.env, w, h, fmt.bits, fmt.sample_bytes, fmt.planes, planar, int(fmt.rgb), fmt.sub_w, fmt.sub_h,
                                      1, chroma_location, 64)
        fr = self.L.mock_source_frame(clip, 0)
        for i, p in enumerate(planes or []):
            view, row = self._plane(fr, i)
            raw = np.ascontiguousarray(p[:view.shape[0]]).view(np.uint8).reshape(view.shape[0], -1)
            view[:, :row] = raw[:, :row]
        return clip

    def _plane(self, frame, index):
        pitch, row, hh = C.c_int(), C.c_int(), C.c_int()
        ptr = self.L.mock_frame_plane(frame, index, C.byref(pitch), C.byref(row), C.byref(hh))
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_ubyte)), shape=(hh.value, pitch.value)), row.value

    def read_plane(self, frame, index, dtype):
        view, row = self._plane(frame, index)
        return np.ascontiguousarray(view[:, :row]).view(dtype).copy()

    def invoke(self, name, clip, tw, th, named):
        """Floats travel as doubles to mock_invoke, which hands them over as 32-bit values (AVS_Value.d.floating_pt)."""
        keys = list(named)
        n = len(keys)
        names = (C.c_char_p * max(1, n))(*[k.encode() for k in keys])
        kinds = bytearray()
        ivals, fvals, svals = (C.c_int * max(1, n))(), (C.c_double * max(1, n))(), (C.c_char_p * max(1, n))()
        for i, k in enumerate(keys):
            v = named[k]
            if isinstance(v, str):
                kinds += b"s"
                svals[i] = v.encode()
            elif isinstance(v, float):
                kinds += b"f"
                fvals[i] = v
            else:
                kinds += b"i"
                ivals[i] = int(v)
        val = self.L.mock_invoke(self.env, name.encode(), clip, tw, th, n, names, bytes(kinds), ivals, fvals, svals)
        err = self.L.mock_value_error(val)
        out = (None, err.decode()) if err is not None else (self.L.mock_value_clip(val), None)
        self.L.mock_value_free(val)
        return out

    def prop(self, frame, key):
        v = C.c_longlong()
        return v.value if self.L.mock_frame_prop_int(frame, key.encode(), C.byref(v)) else None

    def close(self):
        self.L.mock_env_free(self.env)


# ------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------
def f32(v):
    return float(np.float32(v))


def f32_bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def _case(name, fmt, src, dst, args=None, *, seed, opt=0, function="JincResize", nonfinite=None, nonfinite_kinds=None, gpu_only=False,
          family=None):
    a = {k: (f32(v) if isinstance(v, float) else v) for k, v in (args or {}).items()}
    c = {"name": name, "format": fmt, "src": list(src), "dst": list(dst), "function": function, "args": a,
         "args_f32_bits": {k: f"{f32_bits(v):08x}" for k, v in a.items() if isinstance(v, float)},
         "seed": seed, "opt": opt,
         # opt = 0 rows run on a host that reports no SIMD: the alias functions have no `opt` and would take a SIMD path
         "cpu_flags": (CPUF_SSE41 | CPUF_AVX2 | CPUF_AVX512F) if opt else 0}
    if nonfinite is not None:
        c["nonfinite_seed"] = nonfinite
    if nonfinite_kinds is not None:
        c["nonfinite_kinds"] = list(nonfinite_kinds)   # which of SPECIALS the frame carries (absent: all of them)
    if gpu_only:
        c["gpu_only"] = True      # recorded once at full size; the host tests neither regenerate nor recompute it
    if family:
        c["family"] = family
    return c


# VERDICT r6, "Next round" item 1: the reference's answers to scripted (32-bit) float arguments, from an independent run
VERDICT_SCRIPT_FLOATS = {
    "sf_C4_RGBPS_3840x2160_tap4_blur098": "acd6b554",
    "sf_Y32_50x40_crop_quant": "6e53684c",
    "sf_YUV420P16_200x120_topleft_relcrop": "96653485",
    "sf_YUV420P8_128x96_mpeg1_blur11": "3ea0c72a",
    "sf_Y16_150x100_tap6": "0f6ff0c6",
    "sf_RGBPS_96x64_tap4_blur098": "6d776df9",
    "sf_YUV422P10_128x96_tap8": "cc9198d0",
}

# tests/test_gpu_parity.py SMALL_CASES with an output of at most 400 x 260 (tests/test_reference_sweep_host.py checks the copy)
SMALL_CASES = [
    ("Y8", 64, 48, 160, 120, {}),
    ("Y8", 200, 120, 400, 240, dict(tap=4)),
    ("Y8", 131, 77, 262, 154, {}),
    ("Y8", 97, 61, 291, 183, {}),
    ("Y8", 96, 64, 384, 256, {}),
    ("Y8", 1920 // 4, 1080 // 4, 1280 // 4, 720 // 4, {}),
    ("Y8", 64, 48, 40, 30, {}),
    ("Y8", 640, 480, 64, 48, {}),
    ("Y16", 300, 200, 100, 50, dict(tap=4)),
    ("Y32", 256, 256, 128, 128, {}),
    ("Y8", 37, 23, 91, 50, dict(tap=3, blur=0.9, src_left=1.3, src_top=0.7, src_width=33.1, src_height=20.2)),
    ("Y8", 50, 40, 120, 96, dict(tap=4, blur=0.98, src_left=-2.5, src_top=1.25, src_width=55, src_height=41.5,
                                 quant_x=7, quant_y=13)),
    ("Y8", 40, 30, 80, 60, dict(tap=2, src_left=0.125, src_top=0, src_width=20, src_height=15, quant_x=1, quant_y=1)),
    ("Y8", 100, 80, 300, 240, dict(tap=1)),
    ("Y8", 90, 70, 180, 140, dict(tap=5)),
    ("Y8", 160, 120, 320, 240, dict(tap=8)),
    ("Y8", 120, 90, 240, 180, dict(tap=16)),
    ("Y8", 150, 100, 300, 200, dict(tap=2)),
    ("Y16", 150, 100, 300, 200, dict(tap=6)),
    ("Y32", 150, 100, 300, 200, dict(tap=7)),
    ("Y10", 128, 96, 256, 192, {}),
    ("Y12", 128, 96, 256, 192, dict(tap=4)),
    ("Y14", 128, 96, 200, 150, {}),
    ("Y16", 128, 96, 256, 192, {}),
    ("Y32", 128, 96, 256, 192, {}),
    ("YUV420P8", 128, 96, 256, 192, dict(cplace="mpeg2")),
    ("YUV420P8", 128, 96, 256, 192, dict(cplace="mpeg1")),
    ("YUV420P8", 128, 96, 256, 192, dict(cplace="topleft")),
    ("YUV420P16", 160, 96, 320, 192, dict(tap=8, cplace="mpeg2")),
    ("YUV422P10", 128, 96, 300, 200, {}),
    ("YUV411P8", 128, 96, 256, 192, {}),
    ("YUV444P16", 96, 64, 192, 128, {}),
    ("YUVA420P8", 128, 96, 256, 192, {}),
    ("YUV420PS", 128, 96, 256, 192, {}),
    ("RGBP8", 96, 64, 192, 128, {}),
    ("RGBAP16", 96, 64, 200, 100, {}),
    ("RGBPS", 200, 100, 400, 200, dict(tap=4, blur=0.98)),
    ("YUV420P8", 88, 108, 132, 162, dict(tap=2, quant_x=255, quant_y=67, cplace="mpeg2")),
]

# the kernel families the dispatch can pick, each at its smallest shape that still has interior, border rows, border columns
# and a ragged last tile; "family" is the label tests/test_reference_sweep.py's coverage assertion goes by
FAMILY_CASES = [
    ("2x_tap3_u8", "Y8", (131, 77), (262, 154), dict(tap=3)),
    ("2x_tap4_u16", "Y16", (150, 100), (300, 200), dict(tap=4)),
    ("2x_tap6_rowpair", "Y8", (163, 101), (326, 202), dict(tap=6)),
    ("2x_tap8_rowpair_420p16", "YUV420P16", (160, 96), (320, 192), dict(tap=8)),
    ("3x", "Y8", (97, 61), (291, 183), dict(tap=3)),
    ("4x", "Y16", (96, 64), (384, 256), dict(tap=3)),
    ("1.37x_tap8", "Y8", (200, 120), (274, 164), dict(tap=8)),
    ("1.5x_tap8", "Y8", (200, 140), (300, 210), dict(tap=8)),
    ("half_direct", "Y8", (384, 216), (192, 108), dict(tap=3)),
    ("five_sixths_direct", "Y16", (300, 180), (250, 150), dict(tap=3)),
    ("tap12", "Y8", (120, 90), (240, 180), dict(tap=12)),
    ("drift_tap4_runs", "Y32", (150, 120), (225, 180), dict(tap=4)),
    ("2x_tap4_float_quad", "Y32", (150, 100), (300, 200), dict(tap=4)),
]

SWEEP_FORMATS = ["Y8", "Y10", "Y12", "Y14", "Y16", "Y32", "YUV420P8", "YUV420P10", "YUV420P16", "YUV420PS", "YUV422P8", "YUV422P12",
                 "YUV422P16", "YUV411P8", "YUV444P8", "YUV444P14", "YUV444PS", "RGBP8", "RGBP10", "RGBP16", "RGBPS", "RGBAP8", "RGBAPS",
                 "YUVA420P8", "YUVA422P10", "YUVA444P16"]


def _sweep_cases():
    """The seeded sweep: every format family and depth, taps 1..16, ratios 0.37..4, negative and relative crops, quant 1..256,
    blur 0.8..1.3, the three sitings, the four alias functions."""
    rng = np.random.default_rng(20240607)
    O = oracle()
    out = []
    taps = list(rng.permutation(16) + 1) + [3, 4, 8, 2, 6, 5, 12, 16, 1, 7]
    aliases = ["Jinc36Resize", "Jinc64Resize", "Jinc144Resize", "Jinc256Resize"]
    for i, fmt_name in enumerate(SWEEP_FORMATS):
        fmt = O.FORMATS[fmt_name]
        gx, gy = 1 << fmt.sub_w, 1 << fmt.sub_h
        function = aliases[i % 4] if i % 5 == 2 else "JincResize"
        tap = int(taps[i])
        rx, ry = (float(np.exp(rng.uniform(np.log(0.37), np.log(4.0)))) for _ in range(2))
        if tap > 8 or function == "Jinc256Resize":
            rx, ry = max(rx, 0.8), max(ry, 0.8)    # (keeps the reference's table build in the tens of milliseconds)
        mx, my = max(gx, 2), max(gy, 2)
        sw, sh = int(rng.integers(40, 121)) // mx * mx, int(rng.integers(32, 91)) // my * my
        u = rng.uniform(0.0, 1.0, 4)
        kind = i % 4
        radius = O.jinc_zero(ALIAS_TAPS.get(function, tap))
        while True:
            tw = min(400, max(16, int(round(sw * rx)))) // mx * mx
            th = min(260, max(16, int(round(sh * ry)))) // my * my
            args = {}
            if kind == 1:      # negative origin, window larger than the clip
                args.update(src_left=-(0.2 + 2.8 * u[0]), src_top=-(0.2 + 2.8 * u[1]), src_width=sw + 0.5 + 3.5 * u[2], src_height=sh + 0.5 + 3.5 * u[3])
            elif kind == 2:    # relative crop: width / height <= 0 count from the far edge
                args.update(src_left=0.1 + 3.9 * u[0], src_top=0.1 + 3.9 * u[1], src_width=-5.0 * u[2], src_height=-5.0 * u[3])
            elif kind == 3:    # fractional sub-window
                args.update(src_left=5.0 * u[0], src_top=5.0 * u[1], src_width=sw - 5.0 - 4.0 * u[2], src_height=sh - 5.0 - 4.0 * u[3])
            args = {k: float(v) for k, v in args.items()}
            # the reference reads outside a plane that is smaller than the filter footprint (and this project refuses such a
            # call): every plane, chroma included, keeps two samples more than the footprint
            cw = args.get("src_width", float(sw))
            ch = args.get("src_height", float(sh))
            cw = cw if cw > 0 else sw - args.get("src_left", 0.0) + cw
            ch = ch if ch > 0 else sh - args.get("src_top", 0.0) + ch
            fs = max(int(np.ceil(2.0 * radius / min(tw / cw, 1.0))), int(np.ceil(2.0 * radius / min(th / ch, 1.0))))
            if (sw >> fmt.sub_w) >= fs + 2 and (sh >> fmt.sub_h) >= fs + 2:
                break
            if (sw >> fmt.sub_w) < fs + 2:
                sw += mx
            if (sh >> fmt.sub_h) < fs + 2:
                sh += my
        if i % 3:
            args.update(quant_x=int(rng.integers(1, 257)), quant_y=int(rng.integers(1, 257)))
        if function == "JincResize":
            args["tap"] = tap
            if i % 2:
                args["blur"] = float(rng.uniform(0.8, 1.3))
        if fmt.sub_w or fmt.sub_h:
            sitings = ["mpeg2", "MPEG1", "TopLeft"] if (fmt.sub_w, fmt.sub_h) == (1, 1) else ["mpeg2", "mpeg1"]
            args["cplace"] = sitings[int(rng.integers(0, len(sitings)))]
        shown = ALIAS_TAPS.get(function, tap)
        out.append(_case(f"sweep{i:02d}_{fmt_name}_{sw}x{sh}to{tw}x{th}_tap{shown}", fmt_name, (sw, sh), (tw, th), args,
                         seed=1000 + i, function=function))
    return out


def cases():
    out = [
        _case("sf_C4_RGBPS_3840x2160_tap4_blur098", "RGBPS", (3840, 2160), (7680, 4320), dict(tap=4, blur=0.98), seed=12345, gpu_only=True),
        _case("sf_Y32_50x40_crop_quant", "Y32", (50, 40), (120, 96), dict(tap=4, blur=0.98, src_left=-2.5, src_top=1.25, src_width=55.0,
                                                                         src_height=41.5, quant_x=7, quant_y=13), seed=777),
        _case("sf_YUV420P16_200x120_topleft_relcrop", "YUV420P16", (200, 120), (300, 170),
              dict(tap=5, cplace="topleft", src_left=3.3, src_top=-1.7, src_width=-4.5, src_height=-2.0), seed=777),
        _case("sf_YUV420P8_128x96_mpeg1_blur11", "YUV420P8", (128, 96), (256, 192), dict(tap=3, blur=1.1, cplace="mpeg1", src_left=0.7, src_top=0.3),
              seed=777),
        _case("sf_Y16_150x100_tap6", "Y16", (150, 100), (300, 200), dict(tap=6, blur=0.95, src_left=0.1), seed=777),
        _case("sf_RGBPS_96x64_tap4_blur098", "RGBPS", (96, 64), (192, 128), dict(tap=4, blur=0.98), seed=777),
        _case("sf_YUV422P10_128x96_tap8", "YUV422P10", (128, 96), (300, 200), dict(tap=8, blur=1.05, src_width=-0.3, src_height=-0.7), seed=777),
    ]
    for k, (fmt, sw, sh, tw, th, kw) in enumerate(SMALL_CASES):
        extra = "_".join(f"{a}{v}" for a, v in kw.items() if a in ("tap", "cplace"))
        out.append(_case(f"small{k:02d}_{fmt}_{sw}x{sh}to{tw}x{th}" + (f"_{extra}" if extra else ""), fmt, (sw, sh), (tw, th), kw, seed=4242))
    out += _sweep_cases()
    for label, fmt, src, dst, kw in FAMILY_CASES:
        out.append(_case("family_" + label, fmt, src, dst, kw, seed=2024, family=label))
    out.append(_case("nonfinite_Y32_2x_tap3", "Y32", (96, 64), (192, 128), dict(tap=3), seed=31, nonfinite=5))
    out.append(_case("nonfinite_RGBPS_2x_tap4", "RGBPS", (90, 62), (180, 124), dict(tap=4), seed=32, nonfinite=6))
    for opt in (1, 2, 3):
        out.append(_case(f"simd_opt{opt}_Y8_C1_640x360", "Y8", (640, 360), (1280, 720), {}, seed=12345, opt=opt))
        out.append(_case(f"simd_opt{opt}_Y16_150x100_tap4", "Y16", (150, 100), (300, 200), dict(tap=4), seed=4242, opt=opt))
        out.append(_case(f"simd_opt{opt}_Y32_131x77", "Y32", (131, 77), (262, 154), {}, seed=4242, opt=opt))
        out.append(_case(f"simd_opt{opt}_YUV420PS_128x96_tap5", "YUV420PS", (128, 96), (200, 150), dict(tap=5, cplace="mpeg1"), seed=4242, opt=opt))
    # NaN, -inf and denormals under the SIMD orders.  No +inf: the reference's vector loads read up to 15 samples to the right of
    # the window and multiply them by the zero padding of the coefficient row, so a +inf there (0 x inf) makes the reference's own
    # sample depend on memory outside the window; max_ps turns NaN and -inf into min_val before the multiply, wherever they lie.
    for opt in (1, 2, 3):
        out.append(_case(f"simd_opt{opt}_Y32_96x64_tap3_nan_neginf", "Y32", (96, 64), (192, 128), dict(tap=3), seed=41, opt=opt,
                         nonfinite=7, nonfinite_kinds=NO_POS_INF))
        out.append(_case(f"simd_opt{opt}_YUV444PS_90x62_tap4_nan_neginf", "YUV444PS", (90, 62), (135, 93), dict(tap=4), seed=42, opt=opt,
                         nonfinite=8, nonfinite_kinds=NO_POS_INF))
    assert len({c["name"] for c in out}) == len(out)
    return out


# ------------------------------------------------------------------------------------------------------------------
# running a case
# ------------------------------------------------------------------------------------------------------------------
SPECIALS = {"+inf": [np.inf], "-inf": [-np.inf], "nan": [np.nan], "denormal": [1e-41, -3e-39, 1.1e-38]}
NO_POS_INF = ("-inf", "nan", "denormal")


def source_frame(O, case):
    """The seeded LCG frame of the case; `nonfinite_seed` scatters +inf, -inf, NaN and denormals over every plane -- or, where the
    case names them in `nonfinite_kinds`, only those kinds of SPECIALS."""
    fmt = O.FORMATS[case["format"]]
    sw, sh = case["src"]
    planes = O.lcg_frame(fmt, sw, sh, seed=case["seed"])
    if "nonfinite_seed" in case:
        rng = np.random.default_rng(case["nonfinite_seed"])
        specials = np.array([v for kind in case.get("nonfinite_kinds", SPECIALS) for v in SPECIALS[kind]], np.float32)
        for p, (pw, ph) in zip(planes, fmt.plane_dims(sw, sh)):
            for k in range(24):
                p[int(rng.integers(0, ph)), int(rng.integers(0, pw))] = specials[k % len(specials)]
            p[ph // 2:ph // 2 + 12, pw // 3:pw // 3 + 14] = np.float32(1e-41)   # a denormal block larger than the window
    return planes


def script_args(case):
    """The named arguments of the script call (opt is passed to JincResize itself only; the aliases do not take it)."""
    named = dict(case["args"])
    if case["function"] == "JincResize":
        named["opt"] = case["opt"]
    return named


def oracle_args(case):
    """OracleFilter / C ABI keyword arguments of the case: the float32 values as doubles, the alias's tap spelled out."""
    kw = {k: (v.lower() if k == "cplace" else v) for k, v in case["args"].items()}
    if case["function"] in ALIAS_TAPS:
        kw["tap"] = ALIAS_TAPS[case["function"]]
    return kw


def _visible_bytes(plane, w, h):
    a = np.ascontiguousarray(plane[:h, :w])
    if a.dtype == np.float32:
        a = a.view(np.uint32).copy()
        a[np.isnan(a.view(np.float32))] = QUIET_NAN
    return a.tobytes()


def plane_crc(plane, w, h):
    return f"{zlib.crc32(_visible_bytes(plane, w, h)) & 0xFFFFFFFF:08x}"


def frame_crc(planes, dims):
    """One crc32 chained over the planes in order (how tests/golden/kat.json and the verdicts quote a frame)."""
    c = 0
    for p, (w, h) in zip(planes, dims):
        c = zlib.crc32(_visible_bytes(p, w, h), c)
    return f"{c & 0xFFFFFFFF:08x}"


def plane_crcs(planes, dims):
    return [plane_crc(p, w, h) for p, (w, h) in zip(planes, dims)]


def run_host(L, O, case, src_planes=None):
    """The case through a mock host library `L`: (planes, (width, height), _ChromaLocation or None)."""
    fmt = O.FORMATS[case["format"]]
    sw, sh = case["src"]
    tw, th = case["dst"]
    env = Env(L, case["cpu_flags"])
    src = env.source(fmt, sw, sh, src_planes if src_planes is not None else source_frame(O, case))
    try:
        clip, err = env.invoke(case["function"], src, tw, th, script_args(case))
        if err is not None:
            raise RuntimeError(f"{case['name']}: {err}")
        w, h, n = C.c_int(), C.c_int(), C.c_int()
        L.mock_clip_info(clip, C.byref(w), C.byref(h), C.byref(n))
        fr = L.mock_clip_get_frame(clip, 0)
        if not fr:
            raise RuntimeError(f"{case['name']}: GetFrame failed: {L.mock_clip_error(clip)}")
        planes = [env.read_plane(fr, i, fmt.dtype) for i in range(fmt.planes)]
        loc = env.prop(fr, "_ChromaLocation")
        L.mock_frame_release(fr)
        L.mock_clip_release(clip)
    finally:
        L.mock_source_release(src)
        env.close()
    return planes, (w.value, h.value), loc


def record(L, O, case):
    planes, (w, h), loc = run_host(L, O, case)
    out = dict(case)
    out["out_dims"] = [w, h]
    dims = O.FORMATS[case["format"]].plane_dims(w, h)
    out["crc32"] = plane_crcs(planes, dims)
    out["crc32_frame"] = frame_crc(planes, dims)
    out["chroma_location"] = loc
    return out


def generate(include_gpu_only=True, previous=None):
    """The fixture's case list; rows marked gpu_only are taken from `previous` instead of being run when include_gpu_only is false."""
    L, O = reference_library(), oracle()
    if L is None:
        raise RuntimeError("oracle/_ref/libref_mock_avs.so is absent: run oracle/build_ref.py where the reference is available")
    kept = {c["name"]: c for c in (previous or [])}
    return [record(L, O, c) if (include_gpu_only or not c.get("gpu_only")) else kept[c["name"]] for c in cases()]


def load():
    with open(FIXTURE, encoding="utf-8") as fp:
        return json.load(fp)


def dump(rows):
    doc = {"source": "the reference implementation compiled by oracle/build_ref.py against plugin/compat/avisynth_c.h, run under "
                     "tests/mock_avs/mock_host.cpp through avisynth_c_plugin_init / Create_JincResize / GetFrame; frames: the seeded LCG "
                     "frame of oracle.lcg_frame; crc32 per visible plane, NaN -> 7fc00000 on float planes",
           "cases": rows}
    return json.dumps(doc, indent=1) + "\n"


if __name__ == "__main__":
    if "--check" in sys.argv:
        old = load()["cases"]
        new = generate(include_gpu_only=False, previous=old)
        bad = [a["name"] for a, b in zip(new, old) if a != b] + ([] if len(new) == len(old) else ["<case count>"])
        print("fixture is current" if not bad else f"fixture differs: {bad}")
        sys.exit(1 if bad else 0)
    rows = generate()
    for r in rows:   # the recipe against an independent run of the reference
        want = VERDICT_SCRIPT_FLOATS.get(r["name"])
        assert want is None or r["crc32_frame"] == want, (r["name"], r["crc32_frame"], want)
    with open(FIXTURE, "w", encoding="utf-8") as fp:
        fp.write(dump(rows))
    print(f"{FIXTURE}: {len(rows)} cases")
