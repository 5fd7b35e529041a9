"""jinc_filter_process_device_widened_packed10 / _v210 next to the integer unpack passes on the same source, 1920x1080 -> 3840x2160,
tap 3, 128 frames per call (MI355X, one process, one box).

python profiles/strided/measure_widened_words.py [--profile] [--out DIR] [--frames N] [--reps R]

Calls, every destination planar, interleaved twice, events on the stream, median of R repetitions after a warm-up, the shader-clock
sampler running; strided_scratch_bytes is raised to 4 GiB so that every call is one slice:
  f32_444_planar  jinc_filter_process_device on YUV444PS       f32_y410  Y410 words widened into YUV444PS    (widen_fields_kernel<4>)
  f16_444_planar  ... on YUV444PH                              f16_y410  Y410 words widened into YUV444PH    (widen_fields_kernel<2>)
  u10_444_planar  ... on YUV444P10                             u10_y410  Y410 through ..._packed10, planar out (unpack_fields_kernel)
  f32_422_planar  ... on YUV422PS                              f32_v210  v210 blocks widened into YUV422PS   (widen_v210_kernel<4>)
  f16_422_planar  ... on YUV422PH                              f16_v210  v210 blocks widened into YUV422PH   (widen_v210_kernel<2>)
  u10_422_planar  ... on YUV422P10                             u10_v210  v210 through ..._v210, planar out    (unpack_v210_kernel)
A pass's time is its call's minus the planar call's on the same filter; the u10 rows are the passes of the parent commit, the
yardstick: the same source bytes, 16-bit stores.  A device-to-device copy of each pass's traffic stands beside it (a copy of
(read + written) / 2 bytes moves as many bytes as the pass).  No threshold: these are memory passes beside a VALU-bound filter.
--profile: two repetitions of the six non-planar calls only, for a `rocprofv3 --kernel-trace --stats` run of its own, whose
per-kernel averages are the passes' own times.
Writes widened_words_vs_unpack.json into --out (default: the current directory)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as entry  # noqa: E402
import torch  # noqa: E402

pkg = entry.load_package()
SW, SH, TW, TH = 1920, 1080, 3840, 2160


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return dict(ms_median=times[len(times) // 2], ms_min=times[0], ms_max=times[-1])


def planes(dims, dtype, n, hi):
    """Dense planes of n frames: (tensors, ptrs, pitches, strides)."""
    sb = torch.empty(0, dtype=dtype).element_size()
    if dtype in (torch.float32, torch.float16):
        t = [(torch.rand((n, h, w), device="cuda") * hi).to(dtype) for (w, h) in dims]
    else:
        t = [torch.randint(0, hi, (n, h, w), dtype=dtype, device="cuda") for (w, h) in dims]
    return t, [x.data_ptr() for x in t], [sb * w for (w, h) in dims], [sb * w * h for (w, h) in dims]


def copy_ms(nbytes, reps):
    a = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    r = timed(lambda: b.copy_(a), reps)
    del a, b
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=".")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if pkg.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    n = a.frames
    pkg.set_knob("strided_scratch_bytes", float(4 << 30))
    y410, _ = pkg.packed10_layout("Y410")
    row = pkg.v210_row_bytes(SW)
    # one buffer of pseudo-random words per source kind: every bit pattern is a legal source
    words = torch.randint(-2 ** 31, 2 ** 31 - 1, (n, SH, SW), dtype=torch.int32, device="cuda")
    blocks = torch.randint(-2 ** 31, 2 ** 31 - 1, (n, SH, row // 4), dtype=torch.int32, device="cuda")
    calls, keep, filters = {}, [words, blocks], {}
    for tag, fname, dtype, hi in (("f32_444", "YUV444PS", torch.float32, 1023.0), ("f16_444", "YUV444PH", torch.float16, 1023.0),
                                  ("u10_444", "YUV444P10", torch.int16, 1024), ("f32_422", "YUV422PS", torch.float32, 1023.0),
                                  ("f16_422", "YUV422PH", torch.float16, 1023.0), ("u10_422", "YUV422P10", torch.int16, 1024)):
        fmt = pkg.FORMATS[fname]
        f = filters[tag] = pkg.Filter(fmt, SW, SH, TW, TH, device=0, tap=3)
        st, sp, spitch, sfs = planes(fmt.plane_dims(SW, SH), dtype, n, hi)
        dt, dp, dpitch, dfs = planes(f.out_dims(), dtype, n, 1 if dtype == torch.int16 else 1.0)
        keep += [st, dt]
        calls[tag + "_planar"] = (lambda f=f, sp=sp, spitch=spitch, sfs=sfs, dp=dp, dpitch=dpitch, dfs=dfs: f.process_device(sp, spitch, sfs, dp, dpitch, dfs, n))
        kind, y = tag.split("_")
        if y == "444":
            src = (words.data_ptr(), 4 * SW, 4 * SW * SH)
            if kind == "u10":
                calls["u10_y410"] = (lambda f=f, s=src, dp=dp, dpitch=dpitch, dfs=dfs:
                                     f.process_device_packed10([s[0]] * 3, [s[1]] * 3, y410, [s[2]] * 3, dp, dpitch, None, 0, dfs, n))
            else:
                calls[kind + "_y410"] = (lambda f=f, s=src, dp=dp, dpitch=dpitch, dfs=dfs:
                                         f.process_device_widened_packed10(s[0], s[1], y410, s[2], dp, dpitch, None, dfs, n))
        else:
            src = (blocks.data_ptr(), row, row * SH)
            if kind == "u10":
                calls["u10_v210"] = (lambda f=f, s=src, dp=dp, dpitch=dpitch, dfs=dfs:
                                     f.process_device_v210([s[0]] * 3, [s[1]] * 3, True, [s[2]] * 3, dp, dpitch, False, dfs, n))
            else:
                calls[kind + "_v210"] = (lambda f=f, s=src, dp=dp, dpitch=dpitch, dfs=dfs:
                                         f.process_device_widened_v210(s[0], s[1], s[2], dp, dpitch, None, dfs, n))
    torch.cuda.synchronize()
    passes_of = {"f32_y410": "f32_444_planar", "f16_y410": "f16_444_planar", "u10_y410": "u10_444_planar",
                 "f32_v210": "f32_422_planar", "f16_v210": "f16_422_planar", "u10_v210": "u10_422_planar"}
    if a.profile:
        for name in passes_of:
            timed(calls[name], 2)
            print(name, "profiled; last_strided", pkg.last_strided(), flush=True)
        return
    px = n * SW * SH
    traffic = {   # bytes read, bytes written
        "f32_y410": (4 * px, 12 * px), "f16_y410": (4 * px, 6 * px), "u10_y410": (4 * px, 6 * px),
        "f32_v210": (n * row * SH, 8 * px), "f16_v210": (n * row * SH, 4 * px), "u10_v210": (n * row * SH, 4 * px),
    }
    with pkg.ClockSampler(0, 120.0) as clk:
        runs, reports = {k: [] for k in calls}, {}
        for _ in range(2):
            for name, fn in calls.items():
                runs[name].append(timed(fn, a.reps))
                if not name.endswith("_planar"):   # (the planar call leaves the report of the call before it)
                    reports[name] = pkg.last_strided()
        copies = {name: dict(read=r, written=w, copy=copy_ms((r + w) // 2, a.reps)) for name, (r, w) in traffic.items()}
    best = {k: min(v, key=lambda x: x["ms_median"])["ms_median"] for k, v in runs.items()}
    out = dict(frames=n, best_ms=best, runs=runs, last_strided=reports, passes=copies, shader_ghz_min_med_max=clk.ghz,
               pass_ms_by_difference={name: best[name] - best[planar] for name, planar in passes_of.items()})
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "widened_words_vs_unpack.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    for f in filters.values():
        f.close()


if __name__ == "__main__":
    main()
