"""Filtered pictures in slot layout (hvq_filter_pictures) on the GPU.

Two measurements (steps of tools/benchlib.py):
  calls   128 640x480 4:2:0 streams, 8 resident pictures each, 1024 pictures per call, on natural content, through the binomial 3 x 3, a
          Gaussian of sigma 1.5 (radius 5), a Gaussian of radius 15, the Sobel magnitude on luma only, unsharp masking on luma only and
          the identity: (a) filter_pictures, (b) scale_pictures to the pictures' own geometry on the same pictures -- it reads and writes
          the same bytes: the memory floor of this operation --, (c) picture_metrics against zeros and (d) a torch route on a device copy
          of the same pictures: per plane a float view, F.pad(mode="replicate"), two F.conv2d per term, rounding, clamp, cast,
          concatenation.  HIP-event timed per call on one stream in alternating rounds after a warm-up; medians over the rounds; the
          factors (a)/(b) and (d)/(a).  (a) must equal hvqm4_amd.filters on pictures read back, and so must the torch route.
  trace   the kernel trace of a child that launches filter_pictures per filter, scale_pictures (identity) and
          picture_metrics in a fixed order, one warm-up and `reps` launches each.  Kernel times are read from the trace: median with
          min-max per filter, the bytes read and written over them, and the ratios to the scale identity and to the metrics kernel.
"""
import argparse
import json
import os
import statistics
import sys
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.benchlib import (PEAK, add_common_arguments, drive, launch_stats, optional_route, picture_lists, read_planned, resident, resources,  # noqa: E402
                            timed)

W, H = 640, 480
SRC = (W, H, 2, 2)
PIC_BYTES = W * H * 3 // 2


def the_filters():
    from hvqm4_amd import filters as F
    return [("binomial3", F.binomial(3)), ("gauss1.5_r5", F.gaussian(1.5, 5)), ("gauss5_r15", F.gaussian(5.0, 15)),
            ("sobelmag_luma", F.luma_only(F.gradient_magnitude("sobel"))), ("unsharp_luma", F.luma_only(F.unsharp(1.0, Fraction(1, 2)))),
            ("identity", F.identity())]


def torch_route(torch, copy, filt):
    """the filtered pictures the way a pipeline without the call gets them: planar float32 where every partial sum (an integer of at most
    255 gain) stays below 2^24 and float64 otherwise, replicate padding, two convolutions per term"""
    from hvqm4_amd import filters as F
    from hvqm4_amd import scale
    tf = torch.nn.functional
    n = copy.shape[0]
    out, at = [], 0
    for p, (nx, ny, _mx, _my) in enumerate(scale.plane_sizes(SRC, SRC)):
        pf = filt.chroma if p else filt.luma
        raw = copy[:, at:at + nx * ny]
        at += nx * ny
        if F.is_identity(pf):
            out.append(raw)
            continue
        dt = torch.float64 if F.gain(pf) * 255 >= 1 << 24 else torch.float32
        plane = raw.to(dt).view(n, 1, ny, nx)
        t = []
        for term in pf.terms:
            x = tf.pad(plane, (term.rx, term.rx, term.ry, term.ry), mode="replicate")
            x = tf.conv2d(x, torch.tensor(term.wx, dtype=dt, device="cuda").view(1, 1, 1, -1))
            t.append(tf.conv2d(x, torch.tensor(term.wy, dtype=dt, device="cuda").view(1, 1, -1, 1)))
        if len(t) == 1:
            t.append(torch.zeros_like(t[0]))
        s = t[0] + t[1] if pf.combine == F.SUM else (t[0] + t[1]).abs() if pf.combine == F.ABS_SUM else t[0].abs() + t[1].abs()
        half = 1 << (pf.shift - 1) if pf.shift else 0
        out.append((torch.floor((s + half) / (1 << pf.shift)) + pf.bias).clamp_(0, 255).to(torch.uint8).view(n, -1))
    return torch.cat(out, dim=1)


def setup(args):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    a_s, a_o = picture_lists(resident(ctx, preset=args.contents.split(",")[0], streams=args.streams, per=args.per, distinct=args.distinct), args.per)
    return torch, ctx, a_s, a_o


def child_calls(args):
    import numpy as np
    from hvqm4_amd import filters as F
    torch, ctx, a_s, a_o = setup(args)
    n = len(a_s)
    res = {"size": f"{W}x{H}", "pictures": n, "reps": args.reps, "rounds": args.rounds, "content": args.contents.split(",")[0], "filters": {}}
    met = torch.empty((n, 3, 4), dtype=torch.int64, device="cuda")
    copy = torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
    out = torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
    sout = torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
    probe = list(range(0, n, max(1, n // 8)))
    host = {i: ctx.read_picture(a_s[i], a_o[i]) for i in probe}
    for at in range(0, n, 64):                                  # the device copy the torch route works on
        copy[at:at + 64] = torch.from_numpy(np.stack([ctx.read_picture(a_s[i], a_o[i]) for i in range(at, min(n, at + 64))])).cuda()
    metrics = lambda: ctx.picture_metrics(a_s, a_o, None, out=met)
    ident = lambda: ctx.scale_pictures(a_s, a_o, (W, H), out=sout)
    timed(torch, metrics, args.warmup)
    timed(torch, ident, args.warmup)
    for label, f in the_filters():
        call = lambda: ctx.filter_pictures(a_s, a_o, f, out=out)
        timed(torch, call, args.warmup)
        got = out.cpu().numpy()
        agree = all(np.array_equal(got[i], F.of_picture(host[i], SRC, f)) for i in probe)
        route, off = optional_route(torch, lambda: torch_route(torch, copy, f))         # a torch build without this convolution
        if route:
            off = int((route().to(torch.int16) - out.to(torch.int16)).abs().max())
        r = {"filter_ms": [], "scale_identity_ms": [], "metrics_ms": [], "torch_ms": []}
        for _ in range(args.rounds):
            r["filter_ms"].append(round(timed(torch, call, args.reps), 4))
            r["scale_identity_ms"].append(round(timed(torch, ident, args.reps), 4))
            r["metrics_ms"].append(round(timed(torch, metrics, args.reps), 4))
            if route:
                r["torch_ms"].append(round(timed(torch, route, max(1, args.reps // 5)), 4))
        for k in ("filter", "scale_identity", "metrics", "torch"):
            r[k + "_median_ms"] = statistics.median(r[k + "_ms"]) if r[k + "_ms"] else None
        r["filter_over_scale_identity"] = round(r["filter_median_ms"] / r["scale_identity_median_ms"], 2)
        r["torch_over_filter"] = round(r["torch_median_ms"] / r["filter_median_ms"], 1) if route else None
        r["bytes_read_and_written"] = 2 * n * PIC_BYTES
        r["gb_per_s"] = round(r["bytes_read_and_written"] / (r["filter_median_ms"] * 1e-3) / 1e9, 1)
        r["equal_host_module"] = bool(agree)
        r["torch_route_largest_difference"] = off
        r["gain"] = [F.gain(f.luma), F.gain(f.chroma)]
        r["radii"] = [[(t.rx, t.ry) for t in p.terms] for p in (f.luma, f.chroma)]
        res["filters"][label] = r
    ctx.close()
    print(json.dumps(res))


def child_trace(args):
    """the launches the trace is taken of: per filter 1 + reps of the filter kernel, then of the scale kernel (identity), then of the
    metrics kernel"""
    torch, ctx, a_s, a_o = setup(args)
    n = len(a_s)
    out = torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
    for _label, f in the_filters():
        for _ in range(1 + args.reps):
            ctx.filter_pictures(a_s, a_o, f, out=out)
        torch.cuda.synchronize()
    for _ in range(1 + args.reps):
        ctx.scale_pictures(a_s, a_o, (W, H), out=out)
    torch.cuda.synchronize()
    met = torch.empty((n, 3, 4), dtype=torch.int64, device="cuda")
    for _ in range(1 + args.reps):
        ctx.picture_metrics(a_s, a_o, None, out=met)
    torch.cuda.synchronize()
    ctx.close()
    print(json.dumps({"launches": 1 + args.reps, "pictures": n, "content": args.contents.split(",")[0]}))


def trace_summary(trace_dir, plan, _earlier=None):
    per = plan["launches"]
    names = [label for label, _f in the_filters()]
    cut = read_planned(trace_dir, [(label, "hvq_filter_kernel", per) for label in names] +
                       [("hvq_scale_kernel_identity", "hvq_scale_kernel", per), ("hvq_metrics_kernel", "hvq_metrics_kernel", per)])
    if "error" in cut:
        return cut
    stats = lambda r: launch_stats(l.ns for l in r[1:])                               # without the warm-up launch
    res = {"pictures": plan["pictures"], "content": plan["content"], **resources(cut[names[0]][0])}
    m, s = stats(cut["hvq_metrics_kernel"]), stats(cut["hvq_scale_kernel_identity"])
    m["bytes"] = plan["pictures"] * PIC_BYTES
    s["bytes"] = 2 * plan["pictures"] * PIC_BYTES
    for d in (m, s):
        d["of_peak_median"] = round(d["bytes"] / (d["median_us"] * 1e-6) / PEAK, 3)
    res["hvq_metrics_kernel"], res["hvq_scale_kernel_identity"] = m, s
    for label in names:
        t = stats(cut[label])
        t["bytes"] = 2 * plan["pictures"] * PIC_BYTES
        t["of_peak_median"] = round(t["bytes"] / (t["median_us"] * 1e-6) / PEAK, 3)
        t["over_scale_identity_kernel"] = round(t["median_us"] / s["median_us"], 2)
        t["over_metrics_kernel"] = round(t["median_us"] / m["median_us"], 2)
        res[label] = t
    return res


def main():
    ap = argparse.ArgumentParser()
    add_common_arguments(ap, children=("calls", "trace"), reps=20, warmup=3, rounds=5, steps="calls,trace", out_dir="filter_bench_out", out="--out")
    ap.add_argument("--contents", default="natural")
    args = ap.parse_args()
    if args.child:
        return {"calls": child_calls, "trace": child_trace}[args.child](args)
    drive(args, {"calls": ("calls", None), "trace": ("trace", trace_summary)}, [sys.executable, os.path.abspath(__file__)])


if __name__ == "__main__":
    main()
