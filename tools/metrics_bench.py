"""Picture metrics (hvq_picture_metrics, Context.picture_metrics) on the GPU: 128 dense 640x480 4:2:0 streams, 8 resident pictures each.

Two measurements (steps of tools/benchlib.py):
  trace   the kernel trace of a child that launches, in a fixed order, the metrics of 1024 pairs (k, k - 1)
          (k - 1 taken inside the stream's 8 pictures, so picture 0 pairs with picture 7), of 128 pairs (the newest picture of every
          stream against its predecessor), and -- in the same process, on the same box -- the uint8 export of the same 1024 pictures
          (planar RGB and YUV 4:4:4), the yardstick for "bound by HBM".  One warm-up launch and `reps` launches each.  Kernel times
          are read from the trace: median with min-max; bytes = 2 x pic_bytes per pair (metrics), source planes read + destination
          written (export); share of 8 TB/s.
  route   the call against the route a user takes without it: export(..., "yuv444p") of both pictures, then per plane the int32
          difference, abs().sum() and pow(2).sum() in torch.  Both event-timed on one stream in alternating rounds, 1024 and 128 pairs;
          the two routes must agree on luma sad and sse (the chroma planes of the export are replicated to full size, so only luma
          is compared).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.benchlib import PEAK, add_common_arguments, drive, launch_stats, read_planned, resident, resources, timed  # noqa: E402

W, H = 640, 480
PIC_BYTES = W * H * 3 // 2


def setup(args):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    sids = resident(ctx, preset="dense", streams=args.streams, per=args.per, distinct=args.distinct)
    return torch, ctx, sids


def pairs(sids, per, newest_only):
    """(sids, ordinals, references): every picture against its predecessor inside the stream, or only the newest of every stream"""
    ks = [per - 1] if newest_only else list(range(per))
    a_s = [s for s in sids for _ in ks]
    a_o = [k for _ in sids for k in ks]
    refs = [(s, (k - 1) % per) for s in sids for k in ks]
    return a_s, a_o, refs


def child_trace(args):
    """the launches the trace is taken of, in the order trace_summary reads them by"""
    torch, ctx, sids = setup(args)
    plan = []
    for label, newest in (("metrics_all", False), ("metrics_newest", True)):
        a_s, a_o, refs = pairs(sids, args.per, newest)
        out = torch.empty((len(a_s), 3, 4), dtype=torch.int64, device="cuda")
        for _ in range(1 + args.reps):
            ctx.picture_metrics(a_s, a_o, refs, out=out)
        torch.cuda.synchronize()
        plan.append([label, "hvq_metrics_kernel", 1 + args.reps, len(a_s), 2 * PIC_BYTES])
    a_s, a_o, _refs = pairs(sids, args.per, False)
    for fmt in ("rgbp", "yuv444p"):
        u8 = torch.empty((len(a_s), 3, H, W), dtype=torch.uint8, device="cuda")
        for _ in range(1 + args.reps):
            ctx.export(a_s, a_o, u8, fmt)
        torch.cuda.synchronize()
        plan.append(["export_" + fmt, "hvq_yuv_rgb_kernel", 1 + args.reps, len(a_s), PIC_BYTES + 3 * W * H])
        del u8
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps({"plan": plan}))


def trace_summary(trace_dir, printed, _earlier=None):
    plan = printed["plan"]
    cut = read_planned(trace_dir, [p[:3] for p in plan])
    if "error" in cut:
        return cut
    res = {}
    for label, _kernel, _count, n, per_picture in plan:
        part = cut[label][1:]                                                     # without the warm-up launch
        d = sorted(l.ns for l in part)
        by = n * per_picture
        res[label] = {"kernel": part[0].shown, "pictures": n, **launch_stats(d), "bytes": by,
                      "of_peak_median": round(by / (statistics.median(d) * 1e-9) / PEAK, 3), "of_peak_best": round(by / (d[0] * 1e-9) / PEAK, 3),
                      **resources(part[0])}
    if "metrics_all" in res and "export_rgbp" in res:
        res["metrics_share_over_export_share"] = round(res["metrics_all"]["of_peak_median"] / res["export_rgbp"]["of_peak_median"], 2)
    return res


def child_route(args):
    torch, ctx, sids = setup(args)
    res = {"size": f"{W}x{H}", "reps": args.reps, "rounds": args.rounds}
    for label, newest in (("pairs_all", False), ("pairs_newest", True)):
        a_s, a_o, refs = pairs(sids, args.per, newest)
        n = len(a_s)
        b_s, b_o = [s for s, _k in refs], [k for _s, k in refs]
        out = torch.empty((n, 3, 4), dtype=torch.int64, device="cuda")
        ua = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
        ub = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
        keep = {}

        def call():
            ctx.picture_metrics(a_s, a_o, refs, out=out)

        def route():
            ctx.export(a_s, a_o, ua, "yuv444p")
            ctx.export(b_s, b_o, ub, "yuv444p")
            d = ua.to(torch.int32) - ub.to(torch.int32)
            keep["sad"] = d.abs().sum(dim=(2, 3))
            keep["sse"] = d.pow(2).sum(dim=(2, 3))

        timed(torch, call, args.warmup)
        timed(torch, route, args.warmup)
        agree = bool(torch.equal(out[:, 0, 2], keep["sad"][:, 0]) and torch.equal(out[:, 0, 3], keep["sse"][:, 0]))
        rows = {"pairs": n, "call_ms": [], "route_ms": []}
        for _ in range(args.rounds):
            rows["call_ms"].append(round(timed(torch, call, args.reps), 4))
            rows["route_ms"].append(round(timed(torch, route, args.reps), 4))
        rows["call_median_ms"] = statistics.median(rows["call_ms"])
        rows["route_median_ms"] = statistics.median(rows["route_ms"])
        rows["speedup"] = round(rows["route_median_ms"] / rows["call_median_ms"], 2)
        rows["luma_sad_and_sse_agree"] = agree
        res[label] = rows
        del out, ua, ub
        keep.clear()
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    add_common_arguments(ap, children=("trace", "route"), reps=30, warmup=3, rounds=5, steps="trace,route", out_dir="metrics_bench_out")
    args = ap.parse_args()
    if args.child:
        return {"trace": child_trace, "route": child_route}[args.child](args)
    drive(args, {"trace": ("trace", trace_summary), "route": ("route", None)}, [sys.executable, os.path.abspath(__file__)])


if __name__ == "__main__":
    main()
