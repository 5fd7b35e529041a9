"""The widened and the narrowed call with and without a scale and an offset, 1080p -> 4K 4:2:0 at tap 3 (MI355X, one process, one box):
do the two extra VALU operations per sample hide behind the pass's memory traffic?

python profiles/strided/measure_scaled.py [--out DIR] [--frames N] [--reps R] [--rounds K] [--package DIR] [--tag NAME]

One fp32 4:2:0 filter 1920x1080 -> 3840x2160 at tap 3, device-resident frames, events on the stream, the median of R repetitions
after a warm-up, the calls interleaved K times, the shader-clock sampler running; strided_scratch_bytes is raised to 4 GiB so that
every call is one slice:
  widened          NV12 1920x1080 widened into the filter's fp32 planes (code values), planar fp32 3840x2160 out
  widened_scaled   ... the same with the limited-range pairs of jinc_code_range: (Y - 16) / 219, (C - 128) / 224
  narrowed         planar fp32 1920x1080 in code values in, the result narrowed into NV12 3840x2160
  narrowed_scaled  ... planar fp32 in 0 .. 1 / -0.5 .. 0.5 in, the result taken back with 219 r + 16, 224 r + 128 and narrowed
The scaled calls make the launches of the unscaled ones (last_strided is recorded for each): what differs is one v_mul_f32 and one
v_add_f32 per sample inside widen_samples_kernel / narrow_samples_kernel.
--package DIR: measure the package in DIR (a build of another commit: its __init__.py and lib/) instead of this tree's; a package
without the scaled calls measures the two unscaled ones only.  Writes scaled_vs_unscaled[_TAG].json into --out."""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
W, H = 1920, 1080
CW, CH = W // 2, H // 2


def load(package_dir):
    if package_dir is None:
        sys.path.insert(0, ROOT)
        import __graft_entry__ as entry
        return entry.load_package()
    spec = importlib.util.spec_from_file_location("measured_package", os.path.join(package_dir, "__init__.py"), submodule_search_locations=[package_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["measured_package"] = mod
    spec.loader.exec_module(mod)
    return mod


def timed(torch, fn, reps):
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
    return dict(ms_median=times[len(times) // 2], ms_min=times[0], ms_max=times[-1], ms=times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--package", default=None)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    pkg = load(a.package)
    import torch
    if pkg.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    n = a.frames
    pkg.set_knob("strided_scratch_bytes", float(4 << 30))
    fmt = pkg.FORMATS["YUV420PS"]
    f = pkg.Filter(fmt, W, H, 2 * W, 2 * H, device=0, tap=3)
    has_scaled = hasattr(pkg.Filter, "process_device_widened_scaled")

    def float_planes(dims, lo, hi):
        t = [torch.rand((n, h, w), device="cuda") * (hi - lo) + lo for (w, h) in dims]
        return t, [x.data_ptr() for x in t], [4 * w for (w, h) in dims], [4 * w * h for (w, h) in dims]

    def nv12(w, h):
        y = torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device="cuda")
        uv = torch.randint(0, 256, (n, h // 2, w), dtype=torch.uint8, device="cuda")
        return [y, uv], [y.data_ptr(), uv.data_ptr(), uv.data_ptr() + 1], [w, w, w], [1, 2, 2], [w * h, w * (h // 2), w * (h // 2)]

    src_dims, dst_dims = fmt.plane_dims(W, H), f.out_dims()
    keep = []
    it, ip, ipitch, istep, ifs = nv12(W, H)                       # widened: NV12 1080p in
    ot, op, opitch, ofs = float_planes(dst_dims, 0.0, 1.0)        # ... planar fp32 4K out
    ct, cp, cpitch, cfs = float_planes(src_dims, 0.0, 255.0)      # narrowed: code values in
    ut, up_, upitch, ufs = float_planes(src_dims, 0.0, 1.0)       # narrowed_scaled: the float range in (chroma 0 .. 1 as well: same traffic)
    dt, dp, dpitch, dstep, dfs = nv12(2 * W, 2 * H)               # ... NV12 4K out
    keep += [it, ot, ct, ut, dt]
    calls = {"widened": lambda: f.process_device_widened(ip, ipitch, istep, None, 8, ifs, op, opitch, None, ofs, n),
             "narrowed": lambda: f.process_device_narrowed(cp, cpitch, None, cfs, dp, dpitch, dstep, None, 8, dfs, n)}
    if has_scaled:
        to_f = [pkg.code_range(8, pkg.RANGE_LIMITED, k) for k in (pkg.PLANE_LUMA_OR_RGB, pkg.PLANE_CHROMA, pkg.PLANE_CHROMA)]
        fs, fo, cs, co = ([float(t[k]) for t in to_f] for k in range(4))
        calls["widened_scaled"] = lambda: f.process_device_widened_scaled(ip, ipitch, istep, None, 8, fs, fo, ifs, op, opitch, None, ofs, n)
        calls["narrowed_scaled"] = lambda: f.process_device_narrowed_scaled(up_, upitch, None, ufs, dp, dpitch, dstep, None, 8, cs, co, dfs, n)
    order = [c for c in ("widened", "widened_scaled", "narrowed", "narrowed_scaled") if c in calls]
    torch.cuda.synchronize()
    with pkg.ClockSampler(0, 120.0) as clk:
        rounds, reports = [], {}
        for _ in range(a.rounds):
            r = {}
            for name in order:
                r[name] = timed(torch, calls[name], a.reps)
                reports[name] = pkg.last_strided()
            rounds.append(r)
    result = {}
    for name in order:
        medians = sorted(r[name]["ms_median"] for r in rounds)
        every = sorted(t for r in rounds for t in r[name]["ms"])
        result[name] = dict(call_ms_median_of_rounds=medians[len(medians) // 2], call_ms_median_per_round=medians, call_ms_min=every[0], call_ms_max=every[-1])
    out = dict(frames=n, reps=a.reps, rounds_run=a.rounds, package=a.package or "this tree", calls=result, last_strided=reports,
               shader_ghz_min_med_max=clk.ghz, rounds=rounds)
    print(json.dumps({k: v for k, v in out.items() if k != "rounds"}), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, f"scaled_vs_unscaled{'_' + a.tag if a.tag else ''}.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    f.close()


if __name__ == "__main__":
    main()
