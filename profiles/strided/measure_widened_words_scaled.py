"""jinc_filter_process_device_widened_packed10_scaled / _widened_v210_scaled next to the unscaled calls on the same source and the
same filter, 1920x1080 -> 3840x2160, tap 3 (MI355X, one process, one box).  The unscaled kernels' instruction sequences are those of
the commit before the scaled forms, so the unscaled rows ARE that commit's passes.

python profiles/strided/measure_widened_words_scaled.py [--profile] [--out DIR] [--frames N] [--reps R]

Calls, every destination planar, events on the stream, median of R repetitions after a warm-up, unscaled and scaled alternating and
the whole list run twice (the better round kept), the shader-clock sampler running; strided_scratch_bytes is raised to 4 GiB so that
every call is one slice:
  f32_y410 / f32_y410_scaled    Y410 words into YUV444PS     widen_fields_kernel<4, 0, false> / <4, 0, true>
  f16_y410 / f16_y410_scaled    ... into YUV444PH            <2, 0, false> / <2, 1, true>
  bf16_y410_scaled              ... into YUV444PBF           <2, 2, true>   (the unscaled call refuses bfloat16)
  f32_v210 / f32_v210_scaled    v210 blocks into YUV422PS    widen_v210_kernel<4, 0, false> / <4, 0, true>
  f16_v210 / f16_v210_scaled    ... into YUV422PH            <2, 0, false> / <2, 1, true>
  bf16_v210_scaled              ... into YUV422PBF           <2, 2, true>
The pairs are the limited-range 10-bit luma pair, a negative scale and the limited-range chroma pair.  A call's time holds the
resampling kernels too; the difference scaled - unscaled is the cost of the multiply and add.  --profile: two repetitions of every
call only, for a `rocprofv3 --kernel-trace --stats` run of its own, whose per-kernel averages are the passes' own times.
Writes widened_words_scaled_vs_unscaled.json into --out (default: the current directory).  No threshold: the number is recorded."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as entry  # noqa: E402
import torch  # noqa: E402

pkg = entry.load_package()
SW, SH, TW, TH = 1920, 1080, 3840, 2160
SCALES, OFFSETS = [1.0 / 876.0, -1.0 / 1023.0, 1.0 / 896.0], [-64.0 / 876.0, 1.0, -512.0 / 896.0]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=".")
    ap.add_argument("--frames", type=int, default=16)
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
    calls, keep, filters = {}, [words, blocks], []
    for tag, fname, sb in (("f32_y410", "YUV444PS", 4), ("f16_y410", "YUV444PH", 2), ("bf16_y410", "YUV444PBF", 2),
                           ("f32_v210", "YUV422PS", 4), ("f16_v210", "YUV422PH", 2), ("bf16_v210", "YUV422PBF", 2)):
        f = pkg.Filter(pkg.FORMATS[fname], SW, SH, TW, TH, device=0, tap=3)
        filters.append(f)
        dt = [torch.empty((n, h, w * sb), dtype=torch.uint8, device="cuda") for (w, h) in f.out_dims()]
        keep.append(dt)
        dp, dpitch, dfs = [x.data_ptr() for x in dt], [sb * w for (w, h) in f.out_dims()], [sb * w * h for (w, h) in f.out_dims()]
        if tag.endswith("y410"):
            s = (words.data_ptr(), 4 * SW, 4 * SW * SH)
            if not tag.startswith("bf16"):
                calls[tag] = (lambda f=f, s=s, dp=dp, dpitch=dpitch, dfs=dfs: f.process_device_widened_packed10(s[0], s[1], y410, s[2], dp, dpitch, None, dfs, n))
            calls[tag + "_scaled"] = (lambda f=f, s=s, dp=dp, dpitch=dpitch, dfs=dfs:
                                      f.process_device_widened_packed10_scaled(s[0], s[1], y410, SCALES, OFFSETS, s[2], dp, dpitch, None, dfs, n))
        else:
            s = (blocks.data_ptr(), row, row * SH)
            if not tag.startswith("bf16"):
                calls[tag] = (lambda f=f, s=s, dp=dp, dpitch=dpitch, dfs=dfs: f.process_device_widened_v210(s[0], s[1], s[2], dp, dpitch, None, dfs, n))
            calls[tag + "_scaled"] = (lambda f=f, s=s, dp=dp, dpitch=dpitch, dfs=dfs:
                                      f.process_device_widened_v210_scaled(s[0], s[1], SCALES, OFFSETS, s[2], dp, dpitch, None, dfs, n))
    torch.cuda.synchronize()
    if a.profile:
        for name, fn in calls.items():
            timed(fn, 2)
            print(name, "profiled; last_strided", pkg.last_strided(), flush=True)
        return
    px = n * SW * SH
    traffic = {"f32_y410": (4 * px, 12 * px), "f16_y410": (4 * px, 6 * px), "bf16_y410": (4 * px, 6 * px),   # bytes read, bytes written
               "f32_v210": (n * row * SH, 8 * px), "f16_v210": (n * row * SH, 4 * px), "bf16_v210": (n * row * SH, 4 * px)}
    with pkg.ClockSampler(0, 120.0) as clk:
        runs, reports = {k: [] for k in calls}, {}
        for _ in range(2):
            for name, fn in calls.items():
                runs[name].append(timed(fn, a.reps))
                reports[name] = (pkg.last_strided(), pkg.last_groups()[0])
    best = {k: min(v, key=lambda x: x["ms_median"])["ms_median"] for k, v in runs.items()}
    out = dict(frames=n, best_ms=best, runs=runs, reports=reports, pass_bytes_read_written=traffic, shader_ghz_min_med_max=clk.ghz,
               scaled_minus_unscaled_ms_per_frame={k: (best[k + "_scaled"] - best[k]) / n for k in best if k + "_scaled" in best})
    print(json.dumps({k: v for k, v in out.items() if k not in ("runs", "reports")}), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "widened_words_scaled_vs_unscaled.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    for f in filters:
        f.close()


if __name__ == "__main__":
    main()
