"""Windowed SSIM (hvq_picture_ssim, Context.picture_ssim) on the GPU: the workload of tools/metrics_bench.py -- 128 dense 640x480 4:2:0
streams, 8 resident pictures each, 1024 pairs (k, k - 1) (k - 1 taken inside the stream's 8 pictures).

Two measurements (steps of tools/benchlib.py):
  trace   the kernel trace of a child that launches, in a fixed order, hvq_ssim_kernel without maps, with maps, and
          -- in the same process, on the same pairs -- hvq_metrics_kernel, the yardstick: it reads exactly the same bytes.  One warm-up
          launch and `reps` launches each.  Kernel times are read from the trace: median with min-max; bytes = 2 x pic_bytes per pair
          (plus the maps written); the two ratios to the metrics kernel.
  route   the call against the route a user takes without it: export(..., "yuv444p") of both pictures -> float32 -> the same windows by
          avg_pool2d(8, stride 4) on a, b, a^2 + b^2 and a b -> the formula -> the mean per plane.  Both event-timed on one stream in
          alternating rounds; the two must agree on the luma mean (the chroma planes of the export are replicated to full size, so
          only luma is compared, and the route's float32 variances only agree to about 1e-4).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.benchlib import PEAK, add_common_arguments, drive, launch_stats, read_planned, resources, timed  # noqa: E402
from tools.metrics_bench import H, PIC_BYTES, W, pairs, setup      # noqa: E402


def child_trace(args):
    """the launches the trace is taken of, in the order trace_summary reads them by"""
    from hvqm4_amd.metrics import ssim_windows
    torch, ctx, sids = setup(args)
    a_s, a_o, refs = pairs(sids, args.per, False)
    n = len(a_s)
    windows = sum(r * c for r, c in ssim_windows(W, H, 2, 2))
    plan = []
    out = torch.empty((n, 3, 2), dtype=torch.int64, device="cuda")
    for _ in range(1 + args.reps):
        ctx.picture_ssim(a_s, a_o, refs, out=out)
    torch.cuda.synchronize()
    plan.append(["ssim", "hvq_ssim_kernel", 1 + args.reps, n, 2 * PIC_BYTES])
    for _ in range(1 + args.reps):
        _o, maps = ctx.picture_ssim(a_s, a_o, refs, out=out, maps=True)
    torch.cuda.synchronize()
    del maps
    plan.append(["ssim_maps", "hvq_ssim_kernel", 1 + args.reps, n, 2 * PIC_BYTES + 4 * windows])
    m = torch.empty((n, 3, 4), dtype=torch.int64, device="cuda")
    for _ in range(1 + args.reps):
        ctx.picture_metrics(a_s, a_o, refs, out=m)
    torch.cuda.synchronize()
    plan.append(["metrics", "hvq_metrics_kernel", 1 + args.reps, n, 2 * PIC_BYTES])
    ctx.close()
    print(json.dumps({"plan": plan}))


def trace_summary(trace_dir, printed, _earlier=None):
    plan = printed["plan"]
    cut = read_planned(trace_dir, [p[:3] for p in plan])
    if "error" in cut:
        return cut
    res = {}
    for label, _kernel, _count, n, per_pair in plan:
        part = cut[label][1:]                                                     # without the warm-up launch
        d = [l.ns for l in part]
        by = n * per_pair
        res[label] = {"kernel": part[0].shown, "pairs": n, **launch_stats(d), "bytes": by,
                      "of_peak_median": round(by / (statistics.median(d) * 1e-9) / PEAK, 3), **resources(part[0])}
    res["ssim_over_metrics"] = round(res["ssim"]["median_us"] / res["metrics"]["median_us"], 2)
    res["ssim_maps_over_metrics"] = round(res["ssim_maps"]["median_us"] / res["metrics"]["median_us"], 2)
    return res


def torch_route_ssim(torch, ua, ub):
    """uint8 [n, 3, H, W] twice -> float32 [n, 3]: the mean over the 8 x 8 windows, 4 samples apart, of the library's formula in means"""
    import torch.nn.functional as F
    a, b = ua.to(torch.float32), ub.to(torch.float32)
    pool = lambda x: F.avg_pool2d(x, 8, stride=4)
    ma, mb, m2, mab = pool(a), pool(b), pool(a * a + b * b), pool(a * b)
    c1, c2 = 416.0 / 4096.0, 235963.0 / 4096.0                                   # the integer constants over 64^2
    sq, cr = ma * ma + mb * mb, ma * mb
    q = ((2.0 * cr + c1) * (2.0 * (mab - cr) + c2)) / ((sq + c1) * (m2 - sq + c2))
    return q.mean(dim=(2, 3))


def child_route(args):
    from hvqm4_amd.metrics import ssim
    torch, ctx, sids = setup(args)
    res = {"size": f"{W}x{H}", "reps": args.reps, "rounds": args.rounds}
    a_s, a_o, refs = pairs(sids, args.per, False)
    n = len(a_s)
    b_s, b_o = [s for s, _k in refs], [k for _s, k in refs]
    out = torch.empty((n, 3, 2), dtype=torch.int64, device="cuda")
    ua = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
    ub = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
    keep = {}

    def call():
        ctx.picture_ssim(a_s, a_o, refs, out=out)

    def route():
        ctx.export(a_s, a_o, ua, "yuv444p")
        ctx.export(b_s, b_o, ub, "yuv444p")
        keep["ssim"] = torch_route_ssim(torch, ua, ub)

    timed(torch, call, args.warmup)
    timed(torch, route, args.warmup)
    diff = (ssim(out)[:, 0] - keep["ssim"][:, 0].to(torch.float64)).abs().max().item()
    rows = {"pairs": n, "call_ms": [], "route_ms": []}
    for _ in range(args.rounds):
        rows["call_ms"].append(round(timed(torch, call, args.reps), 4))
        rows["route_ms"].append(round(timed(torch, route, args.reps), 4))
    rows["call_median_ms"] = statistics.median(rows["call_ms"])
    rows["route_median_ms"] = statistics.median(rows["route_ms"])
    rows["speedup"] = round(rows["route_median_ms"] / rows["call_median_ms"], 2)
    rows["luma_mean_max_abs_difference"] = diff
    rows["luma_means_agree"] = bool(diff < 1e-3)
    rows["luma_mean_ssim_of_the_workload"] = round(ssim(out)[:, 0].mean().item(), 6)
    res["pairs_all"] = rows
    ctx.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    add_common_arguments(ap, children=("trace", "route"), reps=30, warmup=3, rounds=5, steps="trace,route", out_dir="ssim_bench_out")
    args = ap.parse_args()
    if args.child:
        return {"trace": child_trace, "route": child_route}[args.child](args)
    drive(args, {"trace": ("trace", trace_summary), "route": ("route", None)}, [sys.executable, os.path.abspath(__file__)])


if __name__ == "__main__":
    main()
