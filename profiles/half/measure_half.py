"""Device-resident process_device: half planes against fp32 planes of the same shape (same box, same process).

python profiles/half/measure_half.py [shape [reps]]   -- all shapes: also writes half_vs_fp32.json into the current directory."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as entry  # noqa: E402
import torch  # noqa: E402

pkg = entry.load_package()
SHAPES = {
    "Y_1080p_to_4K_tap3_1024": ("YH", "Y32", 1920, 1080, 3840, 2160, dict(tap=3), 1024),
    "RGBP_4K_to_8K_tap4_16": ("RGBPH", "RGBPS", 3840, 2160, 7680, 4320, dict(tap=4), 16),
}


def run(fname, sw, sh, tw, th, kw, n, reps):
    fmt = pkg.FORMATS[fname]
    f = pkg.Filter(fmt, sw, sh, tw, th, device=0, **kw)
    tdt = torch.float16 if fmt.half else torch.float32
    sb = 2 if fmt.half else 4
    src = [torch.rand((n, h, w), device="cuda", dtype=torch.float32).to(tdt) for (w, h) in fmt.plane_dims(sw, sh)]
    dst = [torch.empty((n, h, w), device="cuda", dtype=tdt) for (w, h) in f.out_dims()]
    args = ([t.data_ptr() for t in src], [t.stride(1) * sb for t in src], [t.stride(0) * sb for t in src],
            [t.data_ptr() for t in dst], [t.stride(1) * sb for t in dst], [t.stride(0) * sb for t in dst], n)
    f.process_device(*args)   # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f.process_device(*args)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    kernel = f.last_instance(0)
    f.close()
    del src, dst
    torch.cuda.empty_cache()
    times.sort()
    med = times[len(times) // 2]
    return dict(format=fname, ms_median=med, ms_min=times[0], ms_max=times[-1], gpix_s=n * tw * th * fmt.planes / med / 1e6, kernel=kernel)


def main():
    only = sys.argv[1] if len(sys.argv) > 1 else None
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    out = {}
    for name, (hname, fname, sw, sh, tw, th, kw, n) in SHAPES.items():
        if only and name != only:
            continue
        with pkg.ClockSampler(0, 120.0) as clk:
            r = {}
            for rnd in range(2):   # interleaved: half, fp32, half, fp32
                for fmtn in (hname, fname):
                    res = run(fmtn, sw, sh, tw, th, kw, n, reps)
                    r.setdefault(fmtn, []).append(res)
        best = {k: min(v, key=lambda x: x["ms_median"]) for k, v in r.items()}
        out[name] = dict(runs=r, half_over_fp32_speed=best[fname]["ms_median"] / best[hname]["ms_median"], shader_ghz_min_med_max=clk.ghz)
        print(name, json.dumps({k: (best[k]["ms_median"], best[k]["kernel"]) for k in best}), "half/fp32 speed %.3f" % out[name]["half_over_fp32_speed"],
              "clock GHz", clk.ghz, flush=True)
    if not only:
        with open("half_vs_fp32.json", "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
