"""jinc_filter_process_device_widened next to the existing split, 1920x1080 -> 3840x2160, tap 3, 128 frames per call (MI355X, one
process, one box).

python profiles/strided/measure_widened.py [--profile] [--out DIR] [--frames N] [--reps R]

Calls, every destination planar, interleaved twice, events on the stream, median of R repetitions after a warm-up, the shader-clock
sampler running; strided_scratch_bytes is raised to 2 GiB so that every call is one slice:
  f32_planar   jinc_filter_process_device on YUV420PS                    f32_nv12   NV12 widened into YUV420PS
  f16_planar   jinc_filter_process_device on YUV420PH                    f16_p010   P010 (shift 6) widened into YUV420PH
  u10_planar   jinc_filter_process_device on YUV420P10                   u10_p010   P010 through jinc_filter_process_device_shifted
  u8_planar    jinc_filter_process_device on YUV420P8                    u8_nv12    NV12 through jinc_filter_process_device_strided
and a device-to-device copy of each pass's traffic (a copy of (read + written) / 2 bytes moves as many bytes as the pass).
--profile: two repetitions of the four non-planar calls only, for a `rocprofv3 --kernel-trace --stats` run of its own, whose
per-kernel averages are the passes' own times: widen_samples_kernel<1, 1, 4> / <1, 2, 4> (NV12 luma / chroma into fp32),
<2, 1, 2> / <2, 2, 2> (P010 into binary16), split_samples_kernel<2, 1, true> / <2, 2, true> (P010 luma / chroma, the same source
bytes as the binary16 widening) and split_samples_kernel<1, 2, false> (NV12 chroma).
Writes widened_vs_split.json into --out (default: the current directory)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as entry  # noqa: E402
import torch  # noqa: E402

pkg = entry.load_package()
SW, SH, TW, TH = 1920, 1080, 3840, 2160
CW, CH = SW // 2, SH // 2


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


def semi_planar(dtype, n, hi, up):
    """Y dense, U and V interleaved: (tensors, ptrs, pitches, steps, strides)."""
    sb = torch.empty(0, dtype=dtype).element_size()
    y = torch.randint(0, hi, (n, SH, SW), dtype=dtype, device="cuda") << up
    uv = torch.randint(0, hi, (n, CH, 2 * CW), dtype=dtype, device="cuda") << up
    return [y, uv], [y.data_ptr(), uv.data_ptr(), uv.data_ptr() + sb], [sb * SW, sb * 2 * CW, sb * 2 * CW], [1, 2, 2], [sb * SW * SH, sb * 2 * CW * CH, sb * 2 * CW * CH]


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
    pkg.set_knob("strided_scratch_bytes", float(2 << 30))
    calls, keep, filters = {}, [], {}
    for tag, fname, dtype, hi in (("f32", "YUV420PS", torch.float32, 255.0), ("f16", "YUV420PH", torch.float16, 1023.0),
                                  ("u10", "YUV420P10", torch.int16, 1024), ("u8", "YUV420P8", torch.uint8, 256)):
        fmt = pkg.FORMATS[fname]
        f = filters[tag] = pkg.Filter(fmt, SW, SH, TW, TH, device=0, tap=3)
        st, sp, spitch, sfs = planes(fmt.plane_dims(SW, SH), dtype, n, hi)
        dt, dp, dpitch, dfs = planes(f.out_dims(), dtype, n, 1 if dtype in (torch.int16, torch.uint8) else 1.0)
        keep += [st, dt]
        calls[tag + "_planar"] = (lambda f=f, sp=sp, spitch=spitch, sfs=sfs, dp=dp, dpitch=dpitch, dfs=dfs: f.process_device(sp, spitch, sfs, dp, dpitch, dfs, n))
        if tag == "f32":
            kt, p, pitch, step, fs = semi_planar(torch.uint8, n, 256, 0)
            calls["f32_nv12"] = (lambda f=f, p=p, pitch=pitch, step=step, fs=fs, dp=dp, dpitch=dpitch, dfs=dfs:
                                 f.process_device_widened(p, pitch, step, None, 8, fs, dp, dpitch, None, dfs, n))
        elif tag == "f16":
            kt, p, pitch, step, fs = semi_planar(torch.int16, n, 1024, 6)
            calls["f16_p010"] = (lambda f=f, p=p, pitch=pitch, step=step, fs=fs, dp=dp, dpitch=dpitch, dfs=dfs:
                                 f.process_device_widened(p, pitch, step, [6] * 3, 10, fs, dp, dpitch, None, dfs, n))
        elif tag == "u10":
            kt, p, pitch, step, fs = semi_planar(torch.int16, n, 1024, 6)
            calls["u10_p010"] = (lambda f=f, p=p, pitch=pitch, step=step, fs=fs, dp=dp, dpitch=dpitch, dfs=dfs:
                                 f.process_device_shifted(p, pitch, step, [6] * 3, fs, dp, dpitch, None, None, dfs, n))
        else:
            kt, p, pitch, step, fs = semi_planar(torch.uint8, n, 256, 0)
            calls["u8_nv12"] = (lambda f=f, p=p, pitch=pitch, step=step, fs=fs, dp=dp, dpitch=dpitch, dfs=dfs:
                                f.process_device_strided(p, pitch, step, fs, dp, dpitch, None, dfs, n))
        keep.append(kt)
    torch.cuda.synchronize()
    if a.profile:
        for name in ("f32_nv12", "f16_p010", "u10_p010", "u8_nv12"):
            timed(calls[name], 2)
            print(name, "profiled; last_strided", pkg.last_strided(), flush=True)
        return
    pixels = n * (SW * SH + 2 * CW * CH)   # source samples of a call
    passes = {   # bytes read, bytes written
        "f32_nv12": (pixels, 4 * pixels), "f16_p010": (2 * pixels, 2 * pixels), "u10_p010": (2 * pixels, 2 * pixels),
        "u8_nv12": (n * 2 * CW * CH, n * 2 * CW * CH),
    }
    with pkg.ClockSampler(0, 120.0) as clk:
        runs, reports = {k: [] for k in calls}, {}
        for _ in range(2):
            for name, fn in calls.items():
                runs[name].append(timed(fn, a.reps))
                if not name.endswith("_planar"):   # (the planar call leaves the report of the call before it)
                    reports[name] = pkg.last_strided()
        copies = {name: dict(read=r, written=w, copy=copy_ms((r + w) // 2, a.reps)) for name, (r, w) in passes.items()}
    best = {k: min(v, key=lambda x: x["ms_median"])["ms_median"] for k, v in runs.items()}
    out = dict(frames=n, best_ms=best, runs=runs, last_strided=reports, passes=copies, shader_ghz_min_med_max=clk.ghz,
               kernels={k: f.last_instance(0) for k, f in filters.items()},
               pass_ms_by_difference={"f32_nv12": best["f32_nv12"] - best["f32_planar"], "f16_p010": best["f16_p010"] - best["f16_planar"],
                                      "u10_p010": best["u10_p010"] - best["u10_planar"], "u8_nv12": best["u8_nv12"] - best["u8_planar"]})
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "widened_vs_split.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    for f in filters.values():
        f.close()


if __name__ == "__main__":
    main()
