"""jinc_filter_process_device_strided against jinc_filter_process_device on the same samples (MI355X, one process, one box).

python profiles/strided/measure.py [--profile] [--out DIR]

Workloads: NV12 (YUV420P8, U and V interleaved) 1920x1080 -> 3840x2160, tap 3, 128 frames per call; BGRA (RGBAP8 at step 4)
1920x1080 -> 3840x2160, tap 3, 16 frames per call.  Per workload, interleaved twice: the planar call and the strided call, events
on the stream, 20 repetitions after a warm-up; and a device-to-device copy of each pass's byte count (a split reads the interleaved
bytes of the strided source planes and writes as many dense bytes: a copy of that many bytes moves the same traffic; likewise the
merge on the destination side), timed the same way in the same process.  --profile: two repetitions of the strided call only, for a
`rocprofv3 --kernel-trace --stats` run of its own (run.sh), whose per-kernel times are the split / merge kernels' own.
P010 (YUV420P10, samples in the high bits of 16-bit words, luma and chroma shifted by 6) 1920x1080 -> 3840x2160, tap 3, 32 frames per
call (one slice under the default cap): three calls instead of two -- jinc_filter_process_device_shifted, the unshifted strided call
on the same shapes (low-aligned samples) and the planar call -- and copies of the luma and the chroma passes' byte counts.
--only NAME[,NAME]: a subset of the workloads.
Writes strided_vs_planar.json into --out (default: the current directory)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as entry  # noqa: E402
import torch  # noqa: E402

pkg = entry.load_package()
WORKLOADS = {
    "NV12_1080p_to_4K_tap3_128": ("YUV420P8", "nv12", 128),
    "BGRA_1080p_to_4K_tap3_16": ("RGBAP8", "bgra", 16),
    "P010_1080p_to_4K_tap3_32": ("YUV420P10", "p010", 32),
}
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


def side(dims, layout, n):
    """Device buffers (uint8) for n frames; returns (tensors, ptrs, pitches, steps, strides, bytes of the strided planes)."""
    if layout in ("p010", "p010_low"):   # 16-bit words; p010: the 10-bit sample in the high bits, p010_low: in the low bits
        (w, h), (cw, ch) = dims[0], dims[1]
        up = 6 if layout == "p010" else 0   # (int16 holds the 16 bits; the sign is of no interest here)
        y = torch.randint(0, 1024, (n, h, w), dtype=torch.int16, device="cuda") << up
        uv = torch.randint(0, 1024, (n, ch, 2 * cw), dtype=torch.int16, device="cuda") << up
        return ([y, uv], [y.data_ptr(), uv.data_ptr(), uv.data_ptr() + 2], [2 * w, 4 * cw, 4 * cw], [1, 2, 2], [2 * w * h, 4 * cw * ch, 4 * cw * ch],
                (n * h * 2 * w, n * ch * 4 * cw))
    if layout == "planar16":
        t = [torch.randint(0, 1024, (n, h, w), dtype=torch.int16, device="cuda") for (w, h) in dims]
        return t, [x.data_ptr() for x in t], [2 * w for (w, h) in dims], [1] * len(dims), [2 * w * h for (w, h) in dims], 0
    if layout == "nv12":
        (w, h), (cw, ch) = dims[0], dims[1]
        y = torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device="cuda")
        uv = torch.randint(0, 256, (n, ch, 2 * cw), dtype=torch.uint8, device="cuda")
        return [y, uv], [y.data_ptr(), uv.data_ptr(), uv.data_ptr() + 1], [w, 2 * cw, 2 * cw], [1, 2, 2], [w * h, 2 * cw * ch, 2 * cw * ch], n * ch * 2 * cw
    if layout == "bgra":
        w, h = dims[0]
        p = torch.randint(0, 256, (n, h, 4 * w), dtype=torch.uint8, device="cuda")
        return [p], [p.data_ptr() + 1, p.data_ptr(), p.data_ptr() + 2, p.data_ptr() + 3], [4 * w] * 4, [4] * 4, [4 * w * h] * 4, n * h * 4 * w
    t = [torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device="cuda") for (w, h) in dims]
    return t, [x.data_ptr() for x in t], [w for (w, h) in dims], [1] * len(dims), [w * h for (w, h) in dims], 0


def copy_ms(nbytes, reps):
    a = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    r = timed(lambda: b.copy_(a), reps)
    del a, b
    return r


def p010(name, fname, n, a):
    """The shifted call, the unshifted strided call on the same shapes and the planar call, interleaved twice."""
    fmt = pkg.FORMATS[fname]
    f = pkg.Filter(fmt, SW, SH, TW, TH, device=0, tap=3)
    s_keep, sp, spitch, sstep, sfs, s_bytes = side(fmt.plane_dims(SW, SH), "p010", n)
    d_keep, dp, dpitch, dstep, dfs, d_bytes = side(f.out_dims(), "p010", n)
    ls_keep, lsp, lspitch, lsstep, lsfs, _ = side(fmt.plane_dims(SW, SH), "p010_low", n)
    ps_keep, psp, pspitch, _, psfs, _ = side(fmt.plane_dims(SW, SH), "planar16", n)
    pd_keep, pdp, pdpitch, _, pdfs, _ = side(f.out_dims(), "planar16", n)
    six = [6, 6, 6]

    def shifted():
        f.process_device_shifted(sp, spitch, sstep, six, sfs, dp, dpitch, dstep, six, dfs, n)

    def strided():   # (writes the shifted call's destination: the timing does not care)
        f.process_device_strided(lsp, lspitch, lsstep, lsfs, dp, dpitch, dstep, dfs, n)

    def planar():
        f.process_device(psp, pspitch, psfs, pdp, pdpitch, pdfs, n)

    if a.profile:
        timed(shifted, 2)
        print(name, "profiled; last_strided", f.last_strided(), flush=True)
        timed(strided, 2)
        f.close()
        return None
    with pkg.ClockSampler(0, 120.0) as clk:
        runs = {"planar": [], "strided": [], "shifted": []}
        reports = {}
        for _ in range(2):
            runs["planar"].append(timed(planar, a.reps))
            runs["strided"].append(timed(strided, a.reps))
            reports["strided"] = f.last_strided()
            runs["shifted"].append(timed(shifted, a.reps))
            reports["shifted"] = f.last_strided()
        kernel = f.last_instance(0)
        copies = {"luma_split_bytes": s_bytes[0], "chroma_split_bytes": s_bytes[1], "luma_merge_bytes": d_bytes[0], "chroma_merge_bytes": d_bytes[1]}
        for k in list(copies):
            copies["copy_of_" + k] = copy_ms(copies[k], a.reps)
    best = {k: min(v, key=lambda x: x["ms_median"])["ms_median"] for k, v in runs.items()}
    r = dict(format=fname, layout="p010", frames=n, runs=runs, copies=copies, last_strided=reports, kernel=kernel,
             shifted_over_planar_time=best["shifted"] / best["planar"], shifted_over_strided_time=best["shifted"] / best["strided"],
             strided_over_planar_time=best["strided"] / best["planar"], best_ms=best, shader_ghz_min_med_max=clk.ghz)
    print(name, json.dumps({k: v for k, v in r.items() if k not in ("runs",)}), flush=True)
    f.close()
    del s_keep, d_keep, ls_keep, ps_keep, pd_keep
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=".")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    if pkg.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    out = {}
    for name, (fname, layout, n) in WORKLOADS.items():
        if a.only and name not in a.only.split(","):
            continue
        if layout == "p010":
            out[name] = p010(name, fname, n, a)
            continue
        fmt = pkg.FORMATS[fname]
        f = pkg.Filter(fmt, SW, SH, TW, TH, device=0, tap=3)
        s_keep, sp, spitch, sstep, sfs, s_bytes = side(fmt.plane_dims(SW, SH), layout, n)
        d_keep, dp, dpitch, dstep, dfs, d_bytes = side(f.out_dims(), layout, n)
        ps_keep, psp, pspitch, _, psfs, _ = side(fmt.plane_dims(SW, SH), "planar", n)
        pd_keep, pdp, pdpitch, _, pdfs, _ = side(f.out_dims(), "planar", n)

        def strided():
            f.process_device_strided(sp, spitch, sstep, sfs, dp, dpitch, dstep, dfs, n)

        def planar():
            f.process_device(psp, pspitch, psfs, pdp, pdpitch, pdfs, n)

        if a.profile:
            timed(strided, 2)
            print(name, "profiled; last_strided", f.last_strided(), flush=True)
            f.close()
            continue
        with pkg.ClockSampler(0, 120.0) as clk:
            runs = {"planar": [], "strided": []}
            for _ in range(2):
                runs["planar"].append(timed(planar, a.reps))
                runs["strided"].append(timed(strided, a.reps))
            report = f.last_strided()
            kernel = f.last_instance(0)
            copies = {"split_bytes": s_bytes, "merge_bytes": d_bytes, "copy_of_split_bytes": copy_ms(s_bytes, a.reps), "copy_of_merge_bytes": copy_ms(d_bytes, a.reps)}
        best = {k: min(v, key=lambda x: x["ms_median"])["ms_median"] for k, v in runs.items()}
        out[name] = dict(format=fname, layout=layout, frames=n, runs=runs, copies=copies, last_strided=report, kernel=kernel,
                         strided_over_planar_time=best["strided"] / best["planar"], extra_ms=best["strided"] - best["planar"],
                         shader_ghz_min_med_max=clk.ghz)
        print(name, json.dumps({k: v for k, v in out[name].items() if k not in ("runs",)}), flush=True)
        f.close()
        del s_keep, d_keep, ps_keep, pd_keep
        torch.cuda.empty_cache()
    if not a.profile:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "strided_vs_planar.json"), "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
