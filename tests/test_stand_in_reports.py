"""What the stand-in calls report about themselves, pinned call by call: results alone cannot show a group that dropped from the
16-byte path to the sample-by-sample path, a launch too many or another slicing -- the pixels stay right.

One case per process_device_* method of Filter from _strided to _v210_packed10, scaled forms included.  Each case runs on a fresh
Filter (the scratch never shrinks, so scratch_bytes depends on what ran before), once with one frame and once with three frames under
a strided_scratch_bytes that holds two frames' dense planes, so the call runs as two slices.  last_strided() and last_groups() of
both runs are compared with tests/golden/stand_in_reports.json field for field; the one-frame result and frame 0 of the three-frame
result are compared with each other bit for bit.

Shapes: 38 x 8 -> 76 x 16, 2x tap 3 (4:2:0: 38 x 16 -> 76 x 32, which keeps the chroma planes above the filter's footprint).
38 = 6 whole v210 blocks and a 2-pixel tail = 4 whole 8-pixel vectors of words and a 6-pixel tail; the 4:2:2 chroma is 19 wide
(odd, with a vector tail).  Words run on 4:4:4 filters, v210 on 4:2:2, planes on NV12-style 4:2:0
(UV at step 2) with the luma plane shifted by 6 where the call takes shifts.  Every base and pitch is a multiple of 16, so `unit`
is 16 and the recorded paths are the vector paths.

The fixture is recorded by running this file as a script (`python tests/test_stand_in_reports.py --record [PATH]`) on the commit
BEFORE a change to the layer, never with the code under test."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import to_device, to_host

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stand_in_reports.json")
D420 = ([(38, 16), (19, 8), (19, 8)], [(76, 32), (38, 16), (38, 16)])   # (chroma of 19 x 4 lies under the filter's footprint)
D422 = ([(38, 8), (19, 8), (19, 8)], [(76, 16), (38, 16), (38, 16)])
D444 = ([(38, 8)] * 3, [(76, 16)] * 3)
NV, DENSE, PIXEL4 = [1, 2, 2], [1, 1, 1], [4, 4, 4]
Y410, FILL = [10, 0, 20], 0xC0000000
Y6 = [6, 0, 0]   # the luma plane keeps its sample in the high bits (P010's way), the chroma planes do not


def up16(n):
    return (n + 15) // 16 * 16


class PlaneSide:
    """Three planes by their steps: DENSE a buffer each, NV the luma alone and U / V one sample apart, PIXEL4 three of a pixel's four."""

    def __init__(self, dims, sb, steps):
        self.dims, self.sb, self.steps = dims, sb, steps
        if steps == DENSE:
            self.where = [(0, 0), (1, 0), (2, 0)]
            self.bufs = [(up16(w * sb), h) for (w, h) in dims]
        elif steps == NV:
            self.where = [(0, 0), (1, 0), (1, sb)]
            self.bufs = [(up16(dims[0][0] * sb), dims[0][1]), (up16(dims[1][0] * 2 * sb), dims[1][1])]
        else:
            self.where = [(0, 0), (0, sb), (0, 2 * sb)]
            self.bufs = [(up16(dims[0][0] * 4 * sb), dims[0][1])]

    def args(self, tensors):
        ptrs = [tensors[b].data_ptr() + off for (b, off) in self.where]
        return ptrs, [self.bufs[b][0] for (b, _) in self.where], [self.bufs[b][0] * self.bufs[b][1] for (b, _) in self.where]


class OneBuffer:
    """A side that is one buffer of 10:10:10:2 words (4 bytes a pixel) or of v210 blocks (rows padded to 128 bytes, as writers do)."""

    def __init__(self, dims, v210, row_bytes):
        self.bufs = [((row_bytes + 127) // 128 * 128 if v210 else up16(4 * dims[0][0]), dims[0][1])]

    def args(self, tensors):
        return tensors[0].data_ptr(), self.bufs[0][0], self.bufs[0][0] * self.bufs[0][1]


def samples(rng, kind, nbytes, bits=0, shift=0):
    """nbytes of source samples: 'u8', 'u16' (`bits` bits at `shift`), 'f32' / 'f16' / 'bf16' in [0, 1), 'u32' (words, blocks)."""
    if kind == "u8":
        return rng.integers(0, 256, nbytes, dtype=np.uint8)
    if kind == "u16":
        return (rng.integers(0, 1 << bits, nbytes // 2, dtype=np.uint16) << shift).astype(np.uint16).view(np.uint8)
    if kind == "u32":
        return rng.integers(0, 1 << 32, nbytes // 4, dtype=np.uint32).view(np.uint8)
    f = rng.random(nbytes // (4 if kind == "f32" else 2), dtype=np.float32)
    if kind == "f32":
        return f.view(np.uint8)
    return (f.astype(np.float16) if kind == "f16" else (f.view(np.uint32) >> 16).astype(np.uint16)).view(np.uint8)


# name -> the filter (format, out_sub, geometry from the two sides' plane dims), the two sides' buffers, the samples of each source
# buffer, the dims of the planes that take a dense stand-in (source side's first) and the method's call.  In a call `s` / `d` are the
# source / destination side's (pointers, pitches, frame strides), or (pointer, pitch, frame stride) of a side that is one buffer.
def cases(pkg):
    scale, offset = [1.0 / 1023] * 3, [0.0, -0.5, -0.5]
    back, add = [1023.0] * 3, [0.0, 512.0, 512.0]
    rb = pkg.v210_row_bytes
    every, chroma = [0, 1, 2], [1, 2]
    c = {}

    def case(name, fmt, out_sub, dims, src, dst, fill, stand_ins, call):
        c[name] = dict(fmt=fmt, out_sub=out_sub, geom=dims[0][0] + dims[1][0], src=src, dst=dst, fill=fill, call=call,
                       stand_ins=[dims[0][i] for i in stand_ins[0]] + [dims[1][i] for i in stand_ins[1]])

    def planes(dims, side, sb, steps):
        return PlaneSide(dims[side], sb, steps)

    def words(dims, side):
        return OneBuffer(dims[side], False, 0)

    def blocks(dims, side):
        return OneBuffer(dims[side], True, rb(dims[side][0][0]))

    case("strided", "YUV420P8", None, D420, planes(D420, 0, 1, NV), planes(D420, 1, 1, NV), [("u8",)] * 2, (chroma, chroma),
         lambda f, s, d, n: f.process_device_strided(s[0], s[1], NV, s[2], d[0], d[1], NV, d[2], n))
    case("shifted", "YUV420P10", None, D420, planes(D420, 0, 2, NV), planes(D420, 1, 2, NV), [("u16", 10, 6), ("u16", 10, 0)], (every, every),
         lambda f, s, d, n: f.process_device_shifted(s[0], s[1], NV, Y6, s[2], d[0], d[1], NV, Y6, d[2], n))
    case("packed10", "YUV444P10", None, D444, words(D444, 0), words(D444, 1), [("u32",)], (every, every),
         lambda f, s, d, n: f.process_device_packed10([s[0]], [s[1]], Y410, [s[2]], [d[0]], [d[1]], Y410, FILL, [d[2]], n))
    case("v210", "YUV422P10", None, D422, blocks(D422, 0), blocks(D422, 1), [("u32",)], (every, every),
         lambda f, s, d, n: f.process_device_v210([s[0]], [s[1]], True, [s[2]], [d[0]], [d[1]], True, [d[2]], n))
    case("widened", "YUV420PS", None, D420, planes(D420, 0, 2, NV), planes(D420, 1, 4, NV), [("u16", 10, 6), ("u16", 10, 0)], (every, chroma),
         lambda f, s, d, n: f.process_device_widened(s[0], s[1], NV, Y6, 10, s[2], d[0], d[1], NV, d[2], n))
    case("widened_packed10", "YUV444PS", None, D444, words(D444, 0), planes(D444, 1, 4, DENSE), [("u32",)], (every, []),
         lambda f, s, d, n: f.process_device_widened_packed10(s[0], s[1], Y410, s[2], d[0], d[1], None, d[2], n))
    case("widened_v210", "YUV422PS", None, D422, blocks(D422, 0), planes(D422, 1, 4, DENSE), [("u32",)], (every, []),
         lambda f, s, d, n: f.process_device_widened_v210(s[0], s[1], s[2], d[0], d[1], None, d[2], n))
    case("widened_packed10_scaled", "YUV444PH", None, D444, words(D444, 0), planes(D444, 1, 2, PIXEL4), [("u32",)], (every, every),
         lambda f, s, d, n: f.process_device_widened_packed10_scaled(s[0], s[1], Y410, scale, offset, s[2], d[0], d[1], PIXEL4, d[2], n))
    case("widened_v210_scaled", "YUV422PBF", None, D422, blocks(D422, 0), planes(D422, 1, 2, NV), [("u32",)], (every, chroma),
         lambda f, s, d, n: f.process_device_widened_v210_scaled(s[0], s[1], scale, offset, s[2], d[0], d[1], NV, d[2], n))
    case("narrowed", "YUV420PS", None, D420, planes(D420, 0, 4, NV), planes(D420, 1, 2, NV), [("f32",)] * 2, (chroma, every),
         lambda f, s, d, n: f.process_device_narrowed(s[0], s[1], NV, s[2], d[0], d[1], NV, Y6, 10, d[2], n))
    case("widened_scaled", "YUV420PH", None, D420, planes(D420, 0, 2, NV), planes(D420, 1, 2, DENSE), [("u16", 10, 6), ("u16", 10, 0)], (every, []),
         lambda f, s, d, n: f.process_device_widened_scaled(s[0], s[1], NV, Y6, 10, scale, offset, s[2], d[0], d[1], None, d[2], n))
    case("narrowed_scaled", "YUV420PBF", None, D420, planes(D420, 0, 2, DENSE), planes(D420, 1, 1, NV), [("bf16",)] * 3, ([], every),
         lambda f, s, d, n: f.process_device_narrowed_scaled(s[0], s[1], None, s[2], d[0], d[1], NV, None, 8, [255.0] * 3, [0.0, 128.0, 128.0], d[2], n))
    case("narrowed_packed10", "YUV444PS", None, D444, planes(D444, 0, 4, PIXEL4), words(D444, 1), [("f32",)], (every, every),
         lambda f, s, d, n: f.process_device_narrowed_packed10(s[0], s[1], PIXEL4, s[2], d[0], d[1], Y410, FILL, None, None, d[2], n))
    case("narrowed_v210", "YUV422PH", None, D422, planes(D422, 0, 2, NV), blocks(D422, 1), [("f16",)] * 2, (chroma, every),
         lambda f, s, d, n: f.process_device_narrowed_v210(s[0], s[1], NV, s[2], d[0], d[1], back, add, d[2], n))
    to444 = (D420[0], [D420[1][0]] * 3)
    case("shifted_packed10", "YUV420P10", (0, 0), to444, planes(to444, 0, 2, NV), words(to444, 1), [("u16", 10, 6), ("u16", 10, 0)], (every, every),
         lambda f, s, d, n: f.process_device_shifted_packed10(s[0], s[1], NV, Y6, s[2], d[0], d[1], Y410, FILL, d[2], n))
    to444 = (D422[0], [D422[1][0]] * 3)
    case("v210_packed10", "YUV422P10", (0, 0), to444, blocks(to444, 0), words(to444, 1), [("u32",)], (every, every),
         lambda f, s, d, n: f.process_device_v210_packed10(s[0], s[1], s[2], d[0], d[1], Y410, FILL, d[2], n))
    return c


CASE_NAMES = ["strided", "shifted", "packed10", "v210", "widened", "widened_packed10", "widened_v210", "widened_packed10_scaled",
              "widened_v210_scaled", "narrowed", "widened_scaled", "narrowed_scaled", "narrowed_packed10", "narrowed_v210",
              "shifted_packed10", "v210_packed10"]


def run_case(pkg, torch, name):
    """{"n1": report, "n3": report} of the case; asserts that frame 0 of the sliced call is the one-frame call's result."""
    case = cases(pkg)[name]
    fmt = pkg.FORMATS[case["fmt"]]
    # two frames' dense planes, the way the layer sizes them: rows of the FILTER's samples padded to 256 bytes
    per_frame = sum((w * fmt.sample_bytes + 255) // 256 * 256 * h for (w, h) in case["stand_ins"])
    rng = np.random.default_rng(38)
    frames = [np.stack([samples(rng, fill[0], pitch * rows, *fill[1:]) for _ in range(3)])
              for (pitch, rows), fill in zip(case["src"].bufs, case["fill"])]
    f = pkg.Filter(fmt, *case["geom"], device=0, tap=3, out_sub=case["out_sub"])
    out, results = {}, {}
    try:
        for n in (1, 3):
            src = [to_device(torch.from_numpy(np.ascontiguousarray(b[:n]).reshape(-1))) for b in frames]
            dst = [torch.zeros(n * pitch * rows, dtype=torch.uint8, device="cuda") for (pitch, rows) in case["dst"].bufs]
            if n == 3:
                pkg.set_knob("strided_scratch_bytes", 2 * per_frame)
            case["call"](f, case["src"].args(src), case["dst"].args(dst), n)
            torch.cuda.synchronize()
            split, merge, slices, scratch = f.last_strided()
            out[f"n{n}"] = {"strided": [split, merge, slices, scratch], "groups": f.last_groups()}
            results[n] = [to_host(t).numpy() for t in dst]
            # (one frame in one slice; three frames under a cap of two as 2 + 1, the scratch grown to the two frames of a slice)
            assert slices == min(n, 2) and scratch == min(n, 2) * per_frame, (name, n, out[f"n{n}"]["strided"], per_frame)
    finally:
        pkg.clear_knob("strided_scratch_bytes")
        f.close()
    for one, three in zip(results[1], results[3]):
        assert np.array_equal(one, three[:one.size]), f"{name}: frame 0 of the sliced call differs from the one-frame call"
    return out


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE, encoding="utf-8") as fp:
        return json.load(fp)


def test_the_fixture_names_every_call(recorded):
    assert sorted(recorded) == sorted(CASE_NAMES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_reports_are_the_recorded_ones(gpu_pkg, recorded, name):
    torch = pytest.importorskip("torch")
    got = run_case(gpu_pkg, torch, name)
    print(name, json.dumps(got))
    for run in ("n1", "n3"):
        want = recorded[name][run]
        assert got[run]["strided"] == want["strided"], (name, run, got[run]["strided"], want["strided"])
        assert len(got[run]["groups"]) == len(want["groups"]), (name, run, got[run]["groups"], want["groups"])
        for k, (g, w) in enumerate(zip(got[run]["groups"], want["groups"])):
            assert g == w, (name, run, k, g, w)


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_stand_in_reports.py --record [PATH]")
    import torch
    import __graft_entry__ as entry
    package = entry.load_package()
    package.lib()
    record = {name: run_case(package, torch, name) for name in CASE_NAMES}
    path = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    with open(path, "w", encoding="utf-8") as fp:
        json.dump(record, fp, indent=1, sort_keys=True)
        fp.write("\n")
    print(f"recorded {len(record)} calls of {package.LIB_PATH} into {path}")
