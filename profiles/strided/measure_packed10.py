"""jinc_filter_process_device_packed10 against the planar call and the nearest existing pass pair (MI355X, one process, one box).

python profiles/strided/measure_packed10.py [--out DIR] [--reps N] [--frames 16,128]

RGBP10 1920x1080 -> 3840x2160, tap 3, device-resident frames, events on the stream, median of --reps repetitions after a warm-up,
the four calls interleaved twice with the shader-clock sampler running:
  a  jinc_filter_process_device on dense planes
  b  packed10, R10G10B10A2 words in and out
  c  packed10, words in, dense planes out
  d  jinc_filter_process_device_strided on RGBP16 with G, B, R at step 4 on both sides (64-bit pixels)
and, for the larger frame count, b again with strided_scratch_bytes raised so that the call is one slice.  A pass moves what it
reads plus what it writes (unpack: 4 + 6 bytes per source pixel, pack: 6 + 4 per result pixel); a device-to-device copy of half
that many bytes moves the same traffic and is timed the same way.  Writes packed10_vs_planar.json into --out."""
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


def planes(w, h, n):
    t = [torch.randint(0, 1024, (n, h, w), dtype=torch.int16, device="cuda") for _ in range(3)]
    return t, [x.data_ptr() for x in t], [2 * w] * 3, [2 * w * h] * 3


def words(w, h, n):
    t = torch.randint(0, 2 ** 31 - 1, (n, h, w), dtype=torch.int32, device="cuda")   # (bit 31 is a spare bit of this layout)
    return t, [t.data_ptr(), 0, 0], [4 * w, 0, 0], [4 * w * h, 0, 0]


def pixels64(w, h, n):
    """G, B, R of a 4 x 16-bit pixel (B G R X): planes in the library's order at step 4."""
    t = torch.randint(0, 1024, (n, h, 4 * w), dtype=torch.int16, device="cuda")
    p = t.data_ptr()
    return t, [p + 2, p, p + 4], [8 * w] * 3, [4] * 3, [8 * w * h] * 3


def copy_ms(nbytes, reps):
    a = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    r = timed(lambda: b.copy_(a), reps)
    del a, b
    return r


def bus_id():
    props = torch.cuda.get_device_properties(0)
    if hasattr(props, "pci_bus_id"):
        return "%04x:%02x:%02x.0" % (getattr(props, "pci_domain_id", 0), props.pci_bus_id, getattr(props, "pci_device_id", 0))
    return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", default="16,128")
    a = ap.parse_args()
    if pkg.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    offsets, fill = pkg.packed10_layout("R10G10B10A2")
    out = dict(device=torch.cuda.get_device_name(0), pci_bus_id=bus_id(), workloads={})
    counts = [int(x) for x in a.frames.split(",")]
    for n in counts:
        f10 = pkg.Filter(pkg.FORMATS["RGBP10"], SW, SH, TW, TH, device=0, tap=3)
        f16 = pkg.Filter(pkg.FORMATS["RGBP16"], SW, SH, TW, TH, device=0, tap=3)
        ps, psp, pspitch, psfs = planes(SW, SH, n)
        pd, pdp, pdpitch, pdfs = planes(TW, TH, n)
        ws, wsp, wspitch, wsfs = words(SW, SH, n)
        wd, wdp, wdpitch, wdfs = words(TW, TH, n)
        xs, xsp, xspitch, xsstep, xsfs = pixels64(SW, SH, n)
        xd, xdp, xdpitch, xdstep, xdfs = pixels64(TW, TH, n)
        calls = {
            "a_planar": lambda: f10.process_device(psp, pspitch, psfs, pdp, pdpitch, pdfs, n),
            "b_packed_in_packed_out": lambda: f10.process_device_packed10(wsp, wspitch, offsets, wsfs, wdp, wdpitch, offsets, fill, wdfs, n),
            "c_packed_in_planar_out": lambda: f10.process_device_packed10(wsp, wspitch, offsets, wsfs, pdp, pdpitch, None, 0, pdfs, n),
            "d_strided_rgbp16_step4": lambda: f16.process_device_strided(xsp, xspitch, xsstep, xsfs, xdp, xdpitch, xdstep, xdfs, n),
        }
        with pkg.ClockSampler(0, 300.0) as clk:
            runs = {k: [] for k in calls}
            reports = {}
            for _ in range(2):
                for k, fn in calls.items():
                    runs[k].append(timed(fn, a.reps))
                    reports[k] = list(f16.last_strided() if k.startswith("d_") else f10.last_strided())
            kernels = {"rgbp10": f10.last_instance(0), "rgbp16": f16.last_instance(0)}
            if n == max(counts) and reports["b_packed_in_packed_out"][2] > 1:
                with pkg.knobs(strided_scratch_bytes=float(n * 3 * 2 * (SW * SH + TW * TH))):
                    runs["b_one_slice"] = [timed(calls["b_packed_in_packed_out"], a.reps) for _ in range(2)]
                    reports["b_one_slice"] = list(f10.last_strided())
            unpack_bytes, pack_bytes = n * SW * SH * 10, n * TW * TH * 10
            copies = dict(unpack_bytes=unpack_bytes, pack_bytes=pack_bytes, copy_of_unpack_traffic=copy_ms(unpack_bytes // 2, a.reps),
                          copy_of_pack_traffic=copy_ms(pack_bytes // 2, a.reps))
        best = {k: min(v, key=lambda x: x["ms_median"])["ms_median"] for k, v in runs.items()}
        unpack_ms, pack_ms = best["c_packed_in_planar_out"] - best["a_planar"], best["b_packed_in_packed_out"] - best["c_packed_in_planar_out"]
        r = dict(frames=n, best_ms=best, runs=runs, last_strided=reports, kernels=kernels, copies=copies,
                 unpack_ms_c_minus_a=unpack_ms, pack_ms_b_minus_c=pack_ms,
                 unpack_gb_per_s=unpack_bytes / unpack_ms / 1e6 if unpack_ms > 0 else None, pack_gb_per_s=pack_bytes / pack_ms / 1e6 if pack_ms > 0 else None,
                 b_minus_a_ms=best["b_packed_in_packed_out"] - best["a_planar"], d_minus_a_ms=best["d_strided_rgbp16_step4"] - best["a_planar"],
                 d_pass_bytes=n * (SW * SH * (8 + 6) + TW * TH * (6 + 6)), b_pass_bytes=unpack_bytes + pack_bytes, shader_ghz_min_med_max=clk.ghz)
        out["workloads"]["RGBP10_1080p_to_4K_tap3_%d" % n] = r
        print(n, json.dumps({k: v for k, v in r.items() if k != "runs"}), flush=True)
        f10.close()
        f16.close()
        del ps, pd, ws, wd, xs, xd, calls
        torch.cuda.empty_cache()
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "packed10_vs_planar.json"), "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
