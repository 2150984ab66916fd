"""Picture histograms (hvq_picture_histograms, Context.picture_histograms) on the GPU: 128 dense 640x480 4:2:0 streams, 8 resident pictures
each, 1024 pictures per call; natural content (the decoded pictures) and flat content (`src` tensors filled with one value: every lane of
every wave adds into the same bin), HVQ_HIST_VALUES and HVQ_HIST_ABSDIFF (natural: picture k against k - 1 inside the stream's 8
pictures; flat: one constant against another).

Two measurements (steps of tools/benchlib.py):
  calls   HIP-event timed on one stream, in alternating rounds: (a) the four histogram calls; (b) picture_metrics on the same pictures
          (against zeros: the bytes VALUES reads; against the predecessor: the bytes ABSDIFF reads) -- the project's streaming bound for
          reading those bytes; (c) the route a user takes without the call: export(..., "yuv444p") of the 1024 pictures, then ONE
          torch.bincount over all planes (each plane's values offset into bins of its own), which is kinder to the route than a
          bincount per plane.  The route's chroma counts are of the replicated planes, so only luma is compared with the call's.
  trace   the kernel trace of a child that launches the same six calls in a fixed order, one warm-up and `reps`
          launches each.  Kernel times are read from the trace: median with min-max; bytes = pic_bytes per picture and side; share of
          8 TB/s; the histogram kernel's time over the metrics kernel's for the same bytes.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.benchlib import PEAK, add_common_arguments, drive, launch_stats, picture_lists, read_planned, resident, resources, timed  # noqa: E402

W, H = 640, 480
PIC_BYTES = W * H * 3 // 2
FLAT_A, FLAT_B = 128, 100


def setup(args):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    sids = resident(ctx, preset="dense", streams=args.streams, per=args.per, distinct=args.distinct)
    return torch, ctx, sids


def workload(torch, ctx, sids, per):
    """label -> (callable, kernel name, sides read): the six calls over the same 1024 pictures"""
    a_s, a_o = picture_lists(sids, per)
    refs = [(s, (k - 1) % per) for s in sids for k in range(per)]
    n = len(a_s)
    flat_a = torch.full((n, PIC_BYTES), FLAT_A, dtype=torch.uint8, device="cuda")
    flat_b = torch.full((n, PIC_BYTES), FLAT_B, dtype=torch.uint8, device="cuda")
    src_a, ref_b, minus = list(flat_a), list(flat_b), [-1] * n
    hist = torch.empty((n, 3, 256), dtype=torch.int32, device="cuda")
    met = torch.empty((n, 3, 4), dtype=torch.int64, device="cuda")
    calls = {
        "values_natural": (lambda: ctx.picture_histograms(a_s, a_o, out=hist), "hvq_histogram_kernel", 1),
        "absdiff_natural": (lambda: ctx.picture_histograms(a_s, a_o, ref=refs, out=hist), "hvq_histogram_kernel", 2),
        "values_flat": (lambda: ctx.picture_histograms(a_s, minus, src=src_a, out=hist), "hvq_histogram_kernel", 1),
        "absdiff_flat": (lambda: ctx.picture_histograms(a_s, minus, ref=ref_b, src=src_a, out=hist), "hvq_histogram_kernel", 2),
        "metrics_zeros": (lambda: ctx.picture_metrics(a_s, a_o, out=met), "hvq_metrics_kernel", 1),
        "metrics_pairs": (lambda: ctx.picture_metrics(a_s, a_o, refs, out=met), "hvq_metrics_kernel", 2),
    }
    return calls, (a_s, a_o, refs, hist, met, flat_a, flat_b)


def child_calls(args):
    torch, ctx, sids = setup(args)
    calls, (a_s, a_o, _refs, hist, _met, _fa, _fb) = workload(torch, ctx, sids, args.per)
    n = len(a_s)
    u8 = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
    offs = (torch.arange(n * 3, dtype=torch.int64, device="cuda") * 256).view(n, 3, 1, 1)
    keep = {}

    def route():
        ctx.export(a_s, a_o, u8, "yuv444p")
        keep["h"] = torch.bincount((u8.to(torch.int64) + offs).view(-1), minlength=n * 3 * 256).view(n, 3, 256)

    fns = {k: v[0] for k, v in calls.items()}
    fns["route_export_bincount"] = route
    for fn in fns.values():
        timed(torch, fn, args.warmup)
    fns["values_natural"]()
    torch.cuda.synchronize()
    agree = bool(torch.equal(hist[:, 0].to(torch.int64), keep["h"][:, 0]))
    fns["values_flat"]()
    torch.cuda.synchronize()
    flat_ok = bool(hist[:, 0, FLAT_A].eq(W * H).all() and hist.sum().item() == n * PIC_BYTES)
    if not (agree and flat_ok):
        sys.exit(f"wrong counts (luma agrees with the route: {agree}, flat pictures counted right: {flat_ok}): nothing is timed")
    res = {"size": f"{W}x{H}", "pictures": n, "reps": args.reps, "rounds": args.rounds, "ms": {k: [] for k in fns}}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            res["ms"][k].append(round(timed(torch, fn, args.route_reps if k.startswith("route") else args.reps), 4))
    med = {k: statistics.median(v) for k, v in res["ms"].items()}
    res["median_ms"] = med
    res["route_over_values_natural"] = round(med["route_export_bincount"] / med["values_natural"], 1)
    res["values_natural_over_metrics_zeros"] = round(med["values_natural"] / med["metrics_zeros"], 2)
    res["absdiff_natural_over_metrics_pairs"] = round(med["absdiff_natural"] / med["metrics_pairs"], 2)
    res["values_flat_over_natural"] = round(med["values_flat"] / med["values_natural"], 2)
    res["absdiff_flat_over_natural"] = round(med["absdiff_flat"] / med["absdiff_natural"], 2)
    res["absdiff_over_values_per_byte_read"] = round(med["absdiff_natural"] / (2 * med["values_natural"]), 2)
    res["luma_agrees_with_the_route"] = agree
    res["flat_counts_right"] = flat_ok
    ctx.close()
    print(json.dumps(res))


def child_trace(args):
    """the launches the trace is taken of, in the order trace_summary reads them by"""
    torch, ctx, sids = setup(args)
    calls, _keep = workload(torch, ctx, sids, args.per)
    plan = []
    for label, (fn, kernel, sides) in calls.items():
        for _ in range(1 + args.reps):
            fn()
        torch.cuda.synchronize()
        plan.append([label, kernel, 1 + args.reps, args.streams * args.per, sides * PIC_BYTES])
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
        d = [l.ns for l in part]
        by = n * per_picture
        res[label] = {"kernel": part[0].shown, "pictures": n, **launch_stats(d), "bytes": by,
                      "of_peak_median": round(by / (statistics.median(d) * 1e-9) / PEAK, 3), **resources(part[0])}
    us = {k: v["median_us"] for k, v in res.items()}
    res["values_natural_over_metrics_zeros"] = round(us["values_natural"] / us["metrics_zeros"], 2)
    res["absdiff_natural_over_metrics_pairs"] = round(us["absdiff_natural"] / us["metrics_pairs"], 2)
    res["values_flat_over_natural"] = round(us["values_flat"] / us["values_natural"], 2)
    res["absdiff_flat_over_natural"] = round(us["absdiff_flat"] / us["absdiff_natural"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    add_common_arguments(ap, children=("calls", "trace"), reps=30, warmup=2, rounds=5, steps="calls,trace", out_dir="histogram_bench_out")
    ap.add_argument("--route-reps", type=int, default=3)
    args = ap.parse_args()
    if args.child:
        return {"calls": child_calls, "trace": child_trace}[args.child](args)
    drive(args, {"calls": ("calls", None), "trace": ("trace", trace_summary)}, [sys.executable, os.path.abspath(__file__)])


if __name__ == "__main__":
    main()
