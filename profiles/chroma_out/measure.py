"""NV12-shaped 1080p 4:2:0 8-bit -> 4:4:4 4K, tap 3, through process_device: the combined call against the sum of its three Y-only twins."""
import json, sys, os
sys.path.insert(0, os.getcwd())
import torch
import __graft_entry__ as entry
pkg = entry.load_package(); pkg.lib()
SW, SH, TW, TH = 1920, 1080, 3840, 2160
out = {}
def planes(dims, n):
    return [torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device="cuda") for (w, h) in dims]
def args(ts):
    return [t.data_ptr() for t in ts], [t.stride(1) for t in ts], [t.stride(0) for t in ts]
def timed(fn, reps=10):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(reps):
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best
for n in (16, 128):
    f = pkg.Filter(pkg.FORMATS["YUV420P8"], SW, SH, TW, TH, device=0, out_sub=(0, 0))
    src = planes(f.fmt.plane_dims(SW, SH), n); dst = planes(f.out_dims(), n)
    s = torch.cuda.current_stream().cuda_stream
    sp, spi, sst = args(src); dp, dpi, dst_st = args(dst)
    t_all = timed(lambda: f.process_device(sp, spi, sst, dp, dpi, dst_st, n, stream=s))
    names = [f.last_kernel(0), f.last_kernel(1)]
    # the chroma planes' Y-only twin: 4:2:0 in, 4:4:4 out, mpeg2 -- co-sited horizontally, centred vertically
    csw, csh, ctw, cth = SW // 2, SH // 2, TW, TH
    ckw = dict(src_left=(0.5 * ((2.0 - 1.0) - (SW / TW) * (1.0 - 1.0)) + 0.0) / 2.0, src_top=0.0, src_width=SW / 2.0, src_height=SH / 2.0)
    fy = pkg.Filter(pkg.FORMATS["Y8"], SW, SH, TW, TH, device=0)
    fc = pkg.Filter(pkg.FORMATS["Y8"], csw, csh, ctw, cth, device=0, **ckw)
    t_y = timed(lambda: fy.process_device(sp[:1], spi[:1], sst[:1], dp[:1], dpi[:1], dst_st[:1], n, stream=s))
    t_u = timed(lambda: fc.process_device(sp[1:2], spi[1:2], sst[1:2], dp[1:2], dpi[1:2], dst_st[1:2], n, stream=s))
    t_v = timed(lambda: fc.process_device(sp[2:3], spi[2:3], sst[2:3], dp[2:3], dpi[2:3], dst_st[2:3], n, stream=s))
    out[n] = dict(combined_ms=t_all, twins_ms=[t_y, t_u, t_v], twins_sum_ms=t_y + t_u + t_v, kernels=names,
                  twin_kernels=[fy.last_kernel(0), fc.last_kernel(0)], instances=[f.last_instance(0), f.last_instance(1)])
    print(n, out[n], flush=True)
    del src, dst
    for x in (f, fy, fc): x.close()
    torch.cuda.empty_cache()
json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else "chroma_out_measure.json", "w"), indent=1)
