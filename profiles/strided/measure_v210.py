"""jinc_filter_process_device_v210 against the planar call, with the packed10 passes from the same run (MI355X, one process, one box).

python profiles/strided/measure_v210.py [--out DIR] [--reps N] [--frames 16]

YUV422P10 1920x1080 -> 3840x2160, tap 3, device-resident frames, events on the stream, median of --reps repetitions after a warm-up,
the calls interleaved twice with the shader-clock sampler running:
  a  jinc_filter_process_device on dense planes
  b  v210 blocks in and out
  c  v210 blocks in, dense planes out
  d  dense planes in, v210 blocks out
and, for the comparison of the passes' rates in the same run, RGBP10 on the same sizes:
  p  jinc_filter_process_device on dense planes
  q  packed10, R10G10B10A2 words in, dense planes out
  r  packed10, dense planes in, words out
A pass moves what it reads plus what it writes.  v210: 16 bytes of blocks per 6 pixels and 4 bytes of samples per pixel (2 luma +
2 x 1 chroma), 6 2/3 bytes per pixel in either direction; packed10: 4 + 6 bytes per pixel.  unpack = c - a (q - p), pack = d - a
(r - p).  v210 rows are 5120 and 10240 bytes, multiples of the conventional 128 already.  Writes v210_vs_planar.json into --out."""
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


def planes(w, h, n, chroma_w):
    t = [torch.randint(0, 1024, (n, h, pw), dtype=torch.int16, device="cuda") for pw in (w, chroma_w, chroma_w)]
    return t, [x.data_ptr() for x in t], [2 * w, 2 * chroma_w, 2 * chroma_w], [2 * w * h, 2 * chroma_w * h, 2 * chroma_w * h]


def blocks(w, h, n):
    row = pkg.v210_row_bytes(w)
    t = torch.randint(0, 2 ** 31 - 1, (n, h, row // 4), dtype=torch.int32, device="cuda")   # (bit 30 set in half of the words: ignored)
    return t, [t.data_ptr(), 0, 0], [row, 0, 0], [row * h, 0, 0]


def words(w, h, n):
    t = torch.randint(0, 2 ** 31 - 1, (n, h, w), dtype=torch.int32, device="cuda")
    return t, [t.data_ptr(), 0, 0], [4 * w, 0, 0], [4 * w * h, 0, 0]


def bus_id():
    props = torch.cuda.get_device_properties(0)
    if hasattr(props, "pci_bus_id"):
        return "%04x:%02x:%02x.0" % (getattr(props, "pci_domain_id", 0), props.pci_bus_id, getattr(props, "pci_device_id", 0))
    return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", default="16")
    a = ap.parse_args()
    if pkg.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    offsets, fill = pkg.packed10_layout("R10G10B10A2")
    out = dict(device=torch.cuda.get_device_name(0), pci_bus_id=bus_id(), workloads={})
    for n in [int(x) for x in a.frames.split(",")]:
        f422 = pkg.Filter(pkg.FORMATS["YUV422P10"], SW, SH, TW, TH, device=0, tap=3)
        frgb = pkg.Filter(pkg.FORMATS["RGBP10"], SW, SH, TW, TH, device=0, tap=3)
        ys, ysp, yspitch, ysfs = planes(SW, SH, n, SW // 2)
        yd, ydp, ydpitch, ydfs = planes(TW, TH, n, TW // 2)
        bs, bsp, bspitch, bsfs = blocks(SW, SH, n)
        bd, bdp, bdpitch, bdfs = blocks(TW, TH, n)
        ps, psp, pspitch, psfs = planes(SW, SH, n, SW)
        pd, pdp, pdpitch, pdfs = planes(TW, TH, n, TW)
        ws, wsp, wspitch, wsfs = words(SW, SH, n)
        wd, wdp, wdpitch, wdfs = words(TW, TH, n)
        calls = {
            "a_planar": lambda: f422.process_device(ysp, yspitch, ysfs, ydp, ydpitch, ydfs, n),
            "b_v210_in_v210_out": lambda: f422.process_device_v210(bsp, bspitch, True, bsfs, bdp, bdpitch, True, bdfs, n),
            "c_v210_in_planar_out": lambda: f422.process_device_v210(bsp, bspitch, True, bsfs, ydp, ydpitch, False, ydfs, n),
            "d_planar_in_v210_out": lambda: f422.process_device_v210(ysp, yspitch, False, ysfs, bdp, bdpitch, True, bdfs, n),
            "p_rgb_planar": lambda: frgb.process_device(psp, pspitch, psfs, pdp, pdpitch, pdfs, n),
            "q_rgb_packed10_in_planar_out": lambda: frgb.process_device_packed10(wsp, wspitch, offsets, wsfs, pdp, pdpitch, None, 0, pdfs, n),
            "r_rgb_planar_in_packed10_out": lambda: frgb.process_device_packed10(psp, pspitch, None, psfs, wdp, wdpitch, offsets, fill, wdfs, n),
        }
        with pkg.ClockSampler(0, 300.0) as clk:
            runs = {k: [] for k in calls}
            reports = {}
            for _ in range(2):
                for k, fn in calls.items():
                    runs[k].append(timed(fn, a.reps))
                    reports[k] = list((frgb if "_rgb_" in k else f422).last_strided())
        best = {k: min(v, key=lambda x: x["ms_median"])["ms_median"] for k, v in runs.items()}
        src_px, dst_px = n * SW * SH, n * TW * TH
        passes = {
            "v210_unpack": (src_px * 20 // 3, best["c_v210_in_planar_out"] - best["a_planar"]),
            "v210_pack": (dst_px * 20 // 3, best["d_planar_in_v210_out"] - best["a_planar"]),
            "packed10_unpack": (src_px * 10, best["q_rgb_packed10_in_planar_out"] - best["p_rgb_planar"]),
            "packed10_pack": (dst_px * 10, best["r_rgb_planar_in_packed10_out"] - best["p_rgb_planar"]),
        }
        r = dict(frames=n, best_ms=best, runs=runs, last_strided=reports, shader_ghz_min_med_max=clk.ghz,
                 passes={k: dict(bytes=b, ms=ms, gb_per_s=b / ms / 1e6 if ms > 0 else None) for k, (b, ms) in passes.items()})
        out["workloads"]["YUV422P10_1080p_to_4K_tap3_%d" % n] = r
        print(n, json.dumps({k: v for k, v in r.items() if k != "runs"}), flush=True)
        f422.close()
        frgb.close()
        del ys, yd, bs, bd, ps, pd, ws, wd, calls
        torch.cuda.empty_cache()
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "v210_vs_planar.json"), "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
