"""The narrowing pass of jinc_filter_process_device_narrowed at 3840x2160 next to widen_samples_kernel on the mirrored traffic
(MI355X, one process, one box).

python profiles/strided/measure_narrowed.py [--profile] [--out DIR] [--frames N] [--reps R] [--rounds K]

Two fp32 4:2:0 filters at tap 3, device-resident frames, events on the stream, median of R repetitions after a warm-up, the six
calls interleaved K times, the shader-clock sampler running; strided_scratch_bytes is raised to 4 GiB so that every call is one slice:
  up_planar    jinc_filter_process_device 1920x1080 -> 3840x2160          dn_planar   jinc_filter_process_device 3840x2160 -> 1920x1080
  up_nv12      ... its planar fp32 result narrowed into NV12 (8 bits)      dn_nv12     NV12 3840x2160 widened into that filter
  up_p010      ... narrowed into P010 (10 bits, shift 6)                   dn_p010     P010 3840x2160 (shift 6) widened into it
A pass's time by events is its call's minus the planar call's on the same filter, per round; the narrowing pass reads 4 bytes and
writes 1 (NV12) or 2 (P010) per 4K sample, the widening pass reads 1 or 2 and writes 4: the same bytes, mirrored.
--profile: three repetitions of the four non-planar calls only, for a `rocprofv3 --kernel-trace --stats` run of its own, whose
per-kernel averages are the passes' own times: narrow_samples_kernel<0, 1, 1> / <0, 2, 1> (luma / chroma into NV12), <0, 1, 2> /
<0, 2, 2> (into P010) and widen_samples_kernel<1, 1, 4> / <1, 2, 4> / <2, 1, 4> / <2, 2, 4>.
Writes narrowed_vs_widened.json into --out (default: the current directory)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as entry  # noqa: E402
import torch  # noqa: E402

pkg = entry.load_package()
W, H = 3840, 2160
CW, CH = W // 2, H // 2


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


def float_planes(dims, n, hi):
    """Dense fp32 planes of n frames in code-value units: (tensors, ptrs, pitches, strides)."""
    t = [torch.rand((n, h, w), device="cuda") * hi for (w, h) in dims]
    return t, [x.data_ptr() for x in t], [4 * w for (w, h) in dims], [4 * w * h for (w, h) in dims]


def semi_planar(dtype, n, hi, up):
    """A 4K frame's Y dense, U and V interleaved: (tensors, ptrs, pitches, steps, strides)."""
    sb = torch.empty(0, dtype=dtype).element_size()
    y = torch.randint(0, hi, (n, H, W), dtype=dtype, device="cuda") << up
    uv = torch.randint(0, hi, (n, CH, 2 * CW), dtype=dtype, device="cuda") << up
    return [y, uv], [y.data_ptr(), uv.data_ptr(), uv.data_ptr() + sb], [sb * W, sb * 2 * CW, sb * 2 * CW], [1, 2, 2], [sb * W * H, sb * 2 * CW * CH, sb * 2 * CW * CH]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=".")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if pkg.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    n = a.frames
    pkg.set_knob("strided_scratch_bytes", float(4 << 30))
    fmt = pkg.FORMATS["YUV420PS"]
    up = pkg.Filter(fmt, W // 2, H // 2, W, H, device=0, tap=3)
    dn = pkg.Filter(fmt, W, H, W // 2, H // 2, device=0, tap=3)
    keep, calls = [], {}
    for bits, tag, dtype, shifts in ((8, "nv12", torch.uint8, None), (10, "p010", torch.int16, [6] * 3)):
        hi = float((1 << bits) - 1)
        st, sp, spitch, sfs = float_planes(fmt.plane_dims(W // 2, H // 2), n, hi)
        dt, dp, dpitch, dfs = float_planes(up.out_dims(), n, 1.0)
        kt, p, pitch, step, fs = semi_planar(dtype, n, 1 << bits, shifts[0] if shifts else 0)
        keep += [st, dt, kt]
        if bits == 8:
            calls["up_planar"] = lambda sp=sp, spitch=spitch, sfs=sfs, dp=dp, dpitch=dpitch, dfs=dfs: up.process_device(sp, spitch, sfs, dp, dpitch, dfs, n)
        calls["up_" + tag] = (lambda sp=sp, spitch=spitch, sfs=sfs, p=p, pitch=pitch, step=step, fs=fs, shifts=shifts, bits=bits:
                              up.process_device_narrowed(sp, spitch, None, sfs, p, pitch, step, shifts, bits, fs, n))
        # the mirror: the same 4K semi-planar buffers as the SOURCE of the down-scaling filter, fp32 planes of 1080p out
        ot, op, opitch, ofs = float_planes(dn.out_dims(), n, 1.0)
        keep.append(ot)
        if bits == 8:
            it, ip, ipitch, ifs = float_planes(fmt.plane_dims(W, H), n, hi)
            keep.append(it)
            calls["dn_planar"] = lambda ip=ip, ipitch=ipitch, ifs=ifs, op=op, opitch=opitch, ofs=ofs: dn.process_device(ip, ipitch, ifs, op, opitch, ofs, n)
        calls["dn_" + tag] = (lambda p=p, pitch=pitch, step=step, fs=fs, shifts=shifts, bits=bits, op=op, opitch=opitch, ofs=ofs:
                              dn.process_device_widened(p, pitch, step, shifts, bits, fs, op, opitch, None, ofs, n))
    torch.cuda.synchronize()
    passes = ("up_nv12", "up_p010", "dn_nv12", "dn_p010")
    if a.profile:
        for name in passes:
            timed(calls[name], 2)
            print(name, "profiled; last_strided", pkg.last_strided(), flush=True)
        return
    samples = n * (W * H + 2 * CW * CH)   # 4K samples of a call
    moved = {"up_nv12": (4 * samples, samples), "up_p010": (4 * samples, 2 * samples),   # bytes read, bytes written
             "dn_nv12": (samples, 4 * samples), "dn_p010": (2 * samples, 4 * samples)}
    with pkg.ClockSampler(0, 120.0) as clk:
        rounds, reports = [], {}
        for _ in range(a.rounds):
            r = {}
            for name, fn in calls.items():
                r[name] = timed(fn, a.reps)
                if not name.endswith("_planar"):   # (the planar call leaves the report of the call before it)
                    reports[name] = pkg.last_strided()
            rounds.append(r)
    result = {}
    for name in passes:
        planar = name[:3] + "planar"
        diffs = sorted(r[name]["ms_median"] - r[planar]["ms_median"] for r in rounds)
        rd, wr = moved[name]
        result[name] = dict(pass_ms_per_round=diffs, pass_ms_median=diffs[len(diffs) // 2], bytes_read=rd, bytes_written=wr,
                            gb_per_s_median=(rd + wr) / (diffs[len(diffs) // 2] * 1e-3) / 1e9,
                            gb_per_s_range=[(rd + wr) / (d * 1e-3) / 1e9 for d in (diffs[-1], diffs[0])],
                            call_ms=[r[name]["ms_median"] for r in rounds], planar_ms=[r[planar]["ms_median"] for r in rounds])
    out = dict(frames=n, reps=a.reps, passes=result, last_strided=reports, shader_ghz_min_med_max=clk.ghz, rounds=rounds)
    print(json.dumps({k: v for k, v in out.items() if k != "rounds"}), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "narrowed_vs_widened.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    up.close()
    dn.close()


if __name__ == "__main__":
    main()
