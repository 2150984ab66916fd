"""Scaled pictures in slot layout (hvq_scale_pictures) on the GPU.

Two measurements (steps of tools/benchlib.py):
  calls   128 640x480 4:2:0 streams, 8 resident pictures each, 1024 pictures per call, on natural and dense content, scaled to 320x240
          (ratio 2), 160x120 (4), 224x168 (2.857), 24x16 (near the limit of 32), 640x480 (identity) and 640x480 at 4:4:4 (chroma
          enlargement): (a) scale_pictures, (b) picture_metrics against zeros on the same pictures -- it reads the same 1.5 B/px and
          writes almost nothing: the memory-bound floor of a reduction -- and (c) a torch route on a device copy of the same pictures: per
          plane adaptive_avg_pool2d on a float view, rounding, concatenation.  HIP-event timed per call on one stream in alternating
          rounds after a warm-up; medians over the rounds; the factors (a)/(b) and (c)/(a).  (a) must equal hvqm4_amd.scale on pictures
          read back; the torch route's largest difference from it is reported (float means, another rounding).
  trace   the kernel trace of a child that launches scale_pictures per shape and picture_metrics in a fixed order,
          one warm-up and `reps` launches each.  Kernel times are read from the trace: median with min-max per shape, the bytes the shape
          reads and writes over them, and the ratio to the metrics kernel.
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
SRC = (W, H, 2, 2)
PIC_BYTES = W * H * 3 // 2
SHAPES = [("320x240", (320, 240, 2, 2)), ("160x120", (160, 120, 2, 2)), ("224x168", (224, 168, 2, 2)), ("24x16", (24, 16, 2, 2)),
          ("640x480", (640, 480, 2, 2)), ("640x480_444", (640, 480, 1, 1))]


def torch_route(torch, copy, dst):
    """the scaled pictures the way a pipeline without the call gets them: float means per plane, rounded, concatenated"""
    from hvqm4_amd import scale
    n = copy.shape[0]
    out, at = [], 0
    for p, (nx, ny, mx, my) in enumerate(scale.plane_sizes(SRC, dst)):
        plane = copy[:, at:at + nx * ny].float().view(n, 1, ny, nx)
        at += nx * ny
        out.append(torch.floor(torch.nn.functional.adaptive_avg_pool2d(plane, (my, mx)) + 0.5).to(torch.uint8).view(n, -1))
    return torch.cat(out, dim=1)


def child_calls(args):
    import numpy as np
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch, scale
    res = {"size": f"{W}x{H}", "pictures": args.streams * args.per, "reps": args.reps, "rounds": args.rounds, "contents": {}}
    for preset in args.contents.split(","):
        ctx = batch.Context(0)
        a_s, a_o = picture_lists(resident(ctx, preset=preset, streams=args.streams, per=args.per, distinct=args.distinct), args.per)
        n = len(a_s)
        met = torch.empty((n, 3, 4), dtype=torch.int64, device="cuda")
        copy = torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
        probe = list(range(0, n, max(1, n // 8)))
        host = {i: ctx.read_picture(a_s[i], a_o[i]) for i in probe}
        for at in range(0, n, 64):                                  # the device copy the torch route works on
            copy[at:at + 64] = torch.from_numpy(np.stack([ctx.read_picture(a_s[i], a_o[i]) for i in range(at, min(n, at + 64))])).cuda()
        metrics = lambda: ctx.picture_metrics(a_s, a_o, None, out=met)
        timed(torch, metrics, args.warmup)
        shapes = {}
        for label, dst in SHAPES:
            out = torch.empty((n, scale.nbytes(*dst)), dtype=torch.uint8, device="cuda")
            call = lambda: ctx.scale_pictures(a_s, a_o, dst[:2], dst[2:], out=out)
            route = lambda: torch_route(torch, copy, dst)
            timed(torch, call, args.warmup)
            timed(torch, route, 1)
            got = out.cpu().numpy()
            agree = all(np.array_equal(got[i], scale.of_picture(host[i], SRC, dst)) for i in probe)
            off = int((route().to(torch.int16) - out.to(torch.int16)).abs().max())
            r = {"scale_ms": [], "metrics_ms": [], "torch_ms": []}
            for _ in range(args.rounds):
                r["scale_ms"].append(round(timed(torch, call, args.reps), 4))
                r["metrics_ms"].append(round(timed(torch, metrics, args.reps), 4))
                r["torch_ms"].append(round(timed(torch, route, max(1, args.reps // 5)), 4))
            for k in ("scale", "metrics", "torch"):
                r[k + "_median_ms"] = statistics.median(r[k + "_ms"])
            r["scale_over_metrics"] = round(r["scale_median_ms"] / r["metrics_median_ms"], 2)
            r["torch_over_scale"] = round(r["torch_median_ms"] / r["scale_median_ms"], 1)
            r["bytes_read_and_written"] = n * (PIC_BYTES + scale.nbytes(*dst))
            r["gb_per_s"] = round(r["bytes_read_and_written"] / (r["scale_median_ms"] * 1e-3) / 1e9, 1)
            r["equal_host_module"] = bool(agree)
            r["torch_route_largest_difference"] = off
            r["bodies"] = [scale.body(*s) for s in scale.plane_sizes(SRC, dst)]
            shapes[label] = r
        res["contents"][preset] = shapes
        ctx.close()
    print(json.dumps(res))


def child_trace(args):
    """the launches the trace is taken of: per shape 1 + reps of the scale kernel, then 1 + reps of the metrics kernel"""
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch, scale
    ctx = batch.Context(0)
    a_s, a_o = picture_lists(resident(ctx, preset=args.contents.split(",")[0], streams=args.streams, per=args.per, distinct=args.distinct), args.per)
    n = len(a_s)
    for _label, dst in SHAPES:
        out = torch.empty((n, scale.nbytes(*dst)), dtype=torch.uint8, device="cuda")
        for _ in range(1 + args.reps):
            ctx.scale_pictures(a_s, a_o, dst[:2], dst[2:], out=out)
        torch.cuda.synchronize()
    met = torch.empty((n, 3, 4), dtype=torch.int64, device="cuda")
    for _ in range(1 + args.reps):
        ctx.picture_metrics(a_s, a_o, None, out=met)
    torch.cuda.synchronize()
    ctx.close()
    print(json.dumps({"launches": 1 + args.reps, "pictures": n, "content": args.contents.split(",")[0]}))


def trace_summary(trace_dir, plan, _earlier=None):
    from hvqm4_amd import scale
    per = plan["launches"]
    cut = read_planned(trace_dir, [(label, "hvq_scale_kernel", per) for label, _dst in SHAPES] + [("hvq_metrics_kernel", "hvq_metrics_kernel", per)])
    if "error" in cut:
        return cut
    stats = lambda r: launch_stats(l.ns for l in r[1:])                               # without the warm-up launch
    res = {"pictures": plan["pictures"], "content": plan["content"], **resources(cut[SHAPES[0][0]][0])}
    m = stats(cut["hvq_metrics_kernel"])
    m["bytes"] = plan["pictures"] * PIC_BYTES
    m["of_peak_median"] = round(m["bytes"] / (m["median_us"] * 1e-6) / PEAK, 3)
    res["hvq_metrics_kernel"] = m
    for label, dst in SHAPES:
        s = stats(cut[label])
        s["bytes"] = plan["pictures"] * (PIC_BYTES + scale.nbytes(*dst))
        s["of_peak_median"] = round(s["bytes"] / (s["median_us"] * 1e-6) / PEAK, 3)
        s["over_metrics_kernel"] = round(s["median_us"] / m["median_us"], 2)
        res[label] = s
    return res


def main():
    ap = argparse.ArgumentParser()
    add_common_arguments(ap, children=("calls", "trace"), reps=20, warmup=3, rounds=5, steps="calls,trace", out_dir="scale_bench_out", out="--out")
    ap.add_argument("--contents", default="natural,dense")
    args = ap.parse_args()
    if args.child:
        return {"calls": child_calls, "trace": child_trace}[args.child](args)
    drive(args, {"calls": ("calls", None), "trace": ("trace", trace_summary)}, [sys.executable, os.path.abspath(__file__)])


if __name__ == "__main__":
    main()
