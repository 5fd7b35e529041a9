"""jinc_filter_process_device_narrowed_packed10 / _v210 next to jinc_filter_process_device_narrowed into planar 10-bit planes of the
same filter, 1920x1080 -> 3840x2160, tap 3, 8 frames per call (MI355X, one process, one box).

python profiles/strided/measure_narrowed_words.py [--profile] [--out DIR] [--frames N] [--reps R]

Calls, every source planar, interleaved twice, events on the stream, median of R repetitions after a warm-up, the shader-clock
sampler running; strided_scratch_bytes is raised to 4 GiB so that every call is one slice:
  f32_444_planar  jinc_filter_process_device on YUV444PS     f32_444_narrow10  ..._narrowed, dst_bits 10, planar   f32_y410  ..._narrowed_packed10
  f16_444_planar  ... on YUV444PH                            f16_444_narrow10                                       f16_y410
  bf16_444_planar ... on YUV444PBF                           bf16_444_narrow10                                      bf16_y410
  f32_422_planar  ... on YUV422PS                            f32_422_narrow10                                       f32_v210  ..._narrowed_v210
  f16_422_planar  ... on YUV422PH                            f16_422_narrow10                                       f16_v210
  bf16_422_planar ... on YUV422PBF                           bf16_422_narrow10                                      bf16_v210
and f32_y410_scaled / f32_v210_scaled with the limited-range pairs of jinc_code_range.  A pass's time is its call's minus the planar
call's on the same filter; the narrow10 rows are the closest thing the parent commit can do -- the same number of passes, the same
bytes read, 2 bytes a sample written where a word holds three samples in 4 and a block six pixels in 16.  No threshold: these are
memory passes beside a VALU-bound filter.
--profile: two repetitions of the non-planar calls only, for a `rocprofv3 --kernel-trace --stats` run of its own, whose per-kernel
averages are the passes' own times.
Writes narrowed_words_vs_planar.json into --out (default: the current directory)."""
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
    """Dense planes of n frames: (tensors, ptrs, pitches, strides); values 0 .. hi (code-value units for the float types)."""
    sb = torch.empty(0, dtype=dtype).element_size()
    if dtype == torch.int16:
        t = [torch.zeros((n, h, w), dtype=dtype, device="cuda") for (w, h) in dims]
    else:
        t = [(torch.rand((n, h, w), device="cuda") * hi).to(dtype) for (w, h) in dims]
    return t, [x.data_ptr() for x in t], [sb * w for (w, h) in dims], [sb * w * h for (w, h) in dims]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=".")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if pkg.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    n = a.frames
    pkg.set_knob("strided_scratch_bytes", float(4 << 30))
    y410, opaque = pkg.packed10_layout("Y410")
    row = pkg.v210_row_bytes(TW)
    words = torch.zeros((n, TH, TW), dtype=torch.int32, device="cuda")
    blocks = torch.zeros((n, TH, row // 4), dtype=torch.int32, device="cuda")
    luma, chroma = pkg.code_range(10, pkg.RANGE_LIMITED, pkg.PLANE_LUMA_OR_RGB), pkg.code_range(10, pkg.RANGE_LIMITED, pkg.PLANE_CHROMA)
    scales, adds = [float(luma[2])] + [float(chroma[2])] * 2, [float(luma[3])] + [float(chroma[3])] * 2
    calls, keep, filters, passes_of = {}, [words, blocks], {}, {}
    for tag, fname, dtype in (("f32_444", "YUV444PS", torch.float32), ("f16_444", "YUV444PH", torch.float16), ("bf16_444", "YUV444PBF", torch.bfloat16),
                              ("f32_422", "YUV422PS", torch.float32), ("f16_422", "YUV422PH", torch.float16), ("bf16_422", "YUV422PBF", torch.bfloat16)):
        fmt = pkg.FORMATS[fname]
        f = filters[tag] = pkg.Filter(fmt, SW, SH, TW, TH, device=0, tap=3)
        st, sp, spitch, sfs = planes(fmt.plane_dims(SW, SH), dtype, n, 1023.0)
        dt, dp, dpitch, dfs = planes(f.out_dims(), dtype, n, 1.0)
        it, ip, ipitch, ifs = planes(f.out_dims(), torch.int16, n, 0)
        keep += [st, dt, it]
        src = (sp, spitch, None, sfs)
        calls[tag + "_planar"] = (lambda f=f, s=src, dp=dp, dpitch=dpitch, dfs=dfs: f.process_device(s[0], s[1], s[3], dp, dpitch, dfs, n))
        calls[tag + "_narrow10"] = (lambda f=f, s=src, ip=ip, ipitch=ipitch, ifs=ifs: f.process_device_narrowed(*s, ip, ipitch, None, None, 10, ifs, n))
        passes_of[tag + "_narrow10"] = tag + "_planar"
        kind, y = tag.split("_")
        if y == "444":
            dst = (words.data_ptr(), 4 * TW, 4 * TW * TH)
            calls[kind + "_y410"] = (lambda f=f, s=src, d=dst: f.process_device_narrowed_packed10(*s, d[0], d[1], y410, opaque, None, None, d[2], n))
            passes_of[kind + "_y410"] = tag + "_planar"
            if kind == "f32":
                calls["f32_y410_scaled"] = (lambda f=f, s=src, d=dst: f.process_device_narrowed_packed10(*s, d[0], d[1], y410, opaque, scales, adds, d[2], n))
                passes_of["f32_y410_scaled"] = tag + "_planar"
        else:
            dst = (blocks.data_ptr(), row, row * TH)
            calls[kind + "_v210"] = (lambda f=f, s=src, d=dst: f.process_device_narrowed_v210(*s, d[0], d[1], None, None, d[2], n))
            passes_of[kind + "_v210"] = tag + "_planar"
            if kind == "f32":
                calls["f32_v210_scaled"] = (lambda f=f, s=src, d=dst: f.process_device_narrowed_v210(*s, d[0], d[1], scales, adds, d[2], n))
                passes_of["f32_v210_scaled"] = tag + "_planar"
    torch.cuda.synchronize()
    if a.profile:
        for name in passes_of:
            timed(calls[name], 2)
            print(name, "profiled; last_strided", pkg.last_strided(), flush=True)
        return
    with pkg.ClockSampler(0, 120.0) as clk:
        runs, reports = {k: [] for k in calls}, {}
        for _ in range(2):
            for name, fn in calls.items():
                runs[name].append(timed(fn, a.reps))
                if not name.endswith("_planar"):   # (the planar call leaves the report of the call before it)
                    reports[name] = pkg.last_strided()
    best = {k: min(v, key=lambda x: x["ms_median"])["ms_median"] for k, v in runs.items()}
    out = dict(frames=n, best_ms=best, runs=runs, last_strided=reports, shader_ghz_min_med_max=clk.ghz,
               pass_ms_per_frame_by_difference={name: (best[name] - best[planar]) / n for name, planar in passes_of.items()})
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "narrowed_words_vs_planar.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    for f in filters.values():
        f.close()


if __name__ == "__main__":
    main()
