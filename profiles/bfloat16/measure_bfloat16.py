"""Device-resident process_device: bfloat16 planes against binary16 and fp32 planes of the same shape (same box, same process).

python profiles/bfloat16/measure_bfloat16.py [shape [reps]]   -- all shapes: also writes bfloat16_vs_half_vs_fp32.json into the
current directory.  The twin of profiles/half/measure_half.py with a third sample type."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as entry  # noqa: E402
import torch  # noqa: E402

pkg = entry.load_package()
SHAPES = {
    "Y_1080p_to_4K_tap3_1024": (("YBF", "YH", "Y32"), 1920, 1080, 3840, 2160, dict(tap=3), 1024),
    "RGBP_4K_to_8K_tap4_16": (("RGBPBF", "RGBPH", "RGBPS"), 3840, 2160, 7680, 4320, dict(tap=4), 16),
}


def run(fname, sw, sh, tw, th, kw, n, reps):
    fmt = pkg.FORMATS[fname]
    f = pkg.Filter(fmt, sw, sh, tw, th, device=0, **kw)
    tdt = torch.bfloat16 if fmt.bfloat16 else (torch.float16 if fmt.half else torch.float32)
    sb = fmt.sample_bytes
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
    for name, (formats, sw, sh, tw, th, kw, n) in SHAPES.items():
        if only and name != only:
            continue
        with pkg.ClockSampler(0, 120.0) as clk:
            r = {}
            for rnd in range(2):   # interleaved: bfloat16, half, fp32, bfloat16, half, fp32
                for fmtn in formats:
                    r.setdefault(fmtn, []).append(run(fmtn, sw, sh, tw, th, kw, n, reps))
        best = {k: min(v, key=lambda x: x["ms_median"]) for k, v in r.items()}
        bname, hname, fname = formats
        out[name] = dict(runs=r, bfloat16_over_fp32_speed=best[fname]["ms_median"] / best[bname]["ms_median"],
                         half_over_fp32_speed=best[fname]["ms_median"] / best[hname]["ms_median"],
                         bfloat16_over_half_speed=best[hname]["ms_median"] / best[bname]["ms_median"], shader_ghz_min_med_max=clk.ghz)
        print(name, json.dumps({k: (best[k]["ms_median"], best[k]["kernel"]) for k in best}),
              "bf16/fp32 speed %.3f, half/fp32 speed %.3f, bf16/half speed %.3f" % (out[name]["bfloat16_over_fp32_speed"], out[name]["half_over_fp32_speed"],
                                                                                   out[name]["bfloat16_over_half_speed"]),
              "clock GHz", clk.ghz, flush=True)
    if not only:
        with open("bfloat16_vs_half_vs_fp32.json", "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
