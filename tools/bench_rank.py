"""Rank filters on pictures in slot layout (hvq_rank_pictures) on the GPU.

Two measurements (steps of tools/benchlib.py):
  calls   128 640x480 4:2:0 streams, 8 resident pictures each, 1024 pictures per call, on natural content, through erode 3 x 3, erode of
          radius 7 and 15, the range of radius 2, the medians 3 x 3 and 5 x 5, the identity and the identity with the copy body switched
          off: (a) rank_pictures, and in the same session (b) scale_pictures to the pictures' own geometry -- it reads and writes the same
          bytes: the memory floor of this operation --, (c) filter_pictures with the binomial 3 x 3 and with a Gaussian of radius 15, and
          (d) a torch route on a device copy of some of the pictures (--route-pictures; its time is scaled to the call's pictures): per
          plane a float copy, F.pad(mode="replicate"), max_pool2d on the negated copy for an erosion, unfold + sort for a median.
          HIP-event timed per call on one stream in alternating rounds after a warm-up; medians over the rounds.  (a) must equal
          hvqm4_amd.rank on pictures read back, and so must the torch route.
  trace   the kernel trace of a child that launches rank_pictures per entry, then scale_pictures (identity), then filter_pictures
          (binomial 3 x 3, Gaussian radius 15) in a fixed order, one warm-up and `reps` launches each.  Kernel times are read from the
          trace: median with min-max per entry, every kernel as a multiple of the scale identity kernel, the ratios erode 15 / erode 1,
          erode 3 x 3 / binomial 3 x 3 and median 5 x 5 / median 3 x 3, and the one condition: the erode radius 15 kernel takes no longer
          than the Gaussian radius 15 filter kernel of the same session.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.benchlib import (PEAK, add_common_arguments, drive, launch_stats, optional_route, picture_lists, read_planned, resident, resources,  # noqa: E402
                            timed)

W, H = 640, 480
SRC = (W, H, 2, 2)
PIC_BYTES = W * H * 3 // 2
GENERAL = "identity_general"                       # the identity with hvq_rank_force_general: the min/max body at radius 0


def the_ranks():
    from hvqm4_amd import rank as R
    return [("erode1", R.erode(1)), ("erode7", R.erode(7)), ("erode15", R.erode(15)), ("range2", R.gradient(2)), ("median3", R.median(3)),
            ("median5", R.median(5)), ("identity", R.identity()), (GENERAL, R.identity())]


def the_filters():
    from hvqm4_amd import filters as F
    return [("binomial3", F.binomial(3)), ("gauss5_r15", F.gaussian(5.0, 15))]


def trace_plan():
    """(label, kernel) of the trace step's blocks in launch order"""
    return [(label, "hvq_rank_kernel") for label in ("erode1", "erode7", "erode15", "range2", "median3", "median5", "identity", GENERAL)] + \
           [("scale_identity", "hvq_scale_kernel"), ("binomial3", "hvq_filter_kernel"), ("gauss5_r15", "hvq_filter_kernel")]


def torch_route(torch, copy, rank):
    """the pictures the way a pipeline without the call gets them, per plane: a float copy, replicate padding, max_pool2d (on the negated
    copy for the minimum), unfold + sort for the median"""
    from hvqm4_amd import rank as R
    from hvqm4_amd import scale
    tf = torch.nn.functional
    n = copy.shape[0]
    out, at = [], 0
    for p, (nx, ny, _mx, _my) in enumerate(scale.plane_sizes(SRC, SRC)):
        pr = rank.chroma if p else rank.luma
        raw = copy[:, at:at + nx * ny]
        at += nx * ny
        if R.copies(pr):
            out.append(raw)
            continue
        x = tf.pad(raw.to(torch.float32).view(n, 1, ny, nx), (pr.rx, pr.rx, pr.ry, pr.ry), mode="replicate")
        k = (2 * pr.ry + 1, 2 * pr.rx + 1)
        if pr.op == R.MEDIAN:
            win = tf.unfold(x, k)                                      # [n, |W|, ny nx]
            y = win.sort(dim=1).values[:, (win.shape[1] - 1) // 2]
        else:
            hi = tf.max_pool2d(x, k, stride=1) if pr.op != R.MIN else None
            lo = -tf.max_pool2d(-x, k, stride=1) if pr.op != R.MAX else None
            y = lo if pr.op == R.MIN else hi if pr.op == R.MAX else hi - lo
        out.append(y.to(torch.uint8).view(n, -1))
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
    from hvqm4_amd import rank as R
    torch, ctx, a_s, a_o = setup(args)
    n = len(a_s)
    m = min(n, args.route_pictures)
    res = {"size": f"{W}x{H}", "pictures": n, "reps": args.reps, "rounds": args.rounds, "content": args.contents.split(",")[0], "route_pictures": m,
           "ranks": {}, "filters": {}}
    out = torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
    sout = torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
    fout = torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
    probe = list(range(0, n, max(1, n // 4)))
    host = {i: ctx.read_picture(a_s[i], a_o[i]) for i in probe}
    copy = torch.from_numpy(np.stack([ctx.read_picture(a_s[i], a_o[i]) for i in range(m)])).cuda()      # what the torch route works on
    ident = lambda: ctx.scale_pictures(a_s, a_o, (W, H), out=sout)
    filt = {label: (lambda f=f: ctx.filter_pictures(a_s, a_o, f, out=fout)) for label, f in the_filters()}
    timed(torch, ident, args.warmup)
    for call in filt.values():
        timed(torch, call, args.warmup)
    fms = {label: [] for label in filt}
    for label, r in the_ranks():
        was = ctx.rank_force_general(label == GENERAL)
        call = lambda: ctx.rank_pictures(a_s, a_o, r, out=out)
        timed(torch, call, args.warmup)
        got = out.cpu().numpy()
        agree = all(np.array_equal(got[i], R.of_picture(host[i], SRC, r)) for i in probe)
        route, off = (None, "not measured") if label in ("identity", GENERAL, "erode7") else optional_route(torch, lambda: torch_route(torch, copy, r))
        if route:
            off = int((route().to(torch.int16) - out[:m].to(torch.int16)).abs().max())
        t = {"rank_ms": [], "scale_identity_ms": [], "torch_ms": []}
        for _ in range(args.rounds):
            t["rank_ms"].append(round(timed(torch, call, args.reps), 4))
            t["scale_identity_ms"].append(round(timed(torch, ident, args.reps), 4))
            for fl, fcall in filt.items():
                fms[fl].append(round(timed(torch, fcall, args.reps), 4))
            if route:
                t["torch_ms"].append(round(timed(torch, route, 1) * n / m, 4))           # scaled from m pictures to the call's n
        ctx.rank_force_general(was)
        for k in ("rank", "scale_identity", "torch"):
            t[k + "_median_ms"] = statistics.median(t[k + "_ms"]) if t[k + "_ms"] else None
        t["rank_over_scale_identity"] = round(t["rank_median_ms"] / t["scale_identity_median_ms"], 2)
        t["torch_over_rank"] = round(t["torch_median_ms"] / t["rank_median_ms"], 1) if route else None
        t["bytes_read_and_written"] = 2 * n * PIC_BYTES
        t["gb_per_s"] = round(t["bytes_read_and_written"] / (t["rank_median_ms"] * 1e-3) / 1e9, 1)
        t["equal_host_module"] = bool(agree)
        t["torch_route_largest_difference"] = off
        res["ranks"][label] = t
    for fl, ms in fms.items():
        res["filters"][fl] = {"filter_ms": ms, "filter_median_ms": statistics.median(ms)}
    ctx.close()
    print(json.dumps(res))


def child_trace(args):
    """the launches the trace is taken of: per entry 1 + reps of the rank kernel, then of the scale kernel (identity), then of the filter
    kernel per filter"""
    torch, ctx, a_s, a_o = setup(args)
    n = len(a_s)
    out = torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
    for label, r in the_ranks():
        was = ctx.rank_force_general(label == GENERAL)
        for _ in range(1 + args.reps):
            ctx.rank_pictures(a_s, a_o, r, out=out)
        torch.cuda.synchronize()
        ctx.rank_force_general(was)
    for _ in range(1 + args.reps):
        ctx.scale_pictures(a_s, a_o, (W, H), out=out)
    torch.cuda.synchronize()
    for _label, f in the_filters():
        for _ in range(1 + args.reps):
            ctx.filter_pictures(a_s, a_o, f, out=out)
        torch.cuda.synchronize()
    ctx.close()
    print(json.dumps({"launches": 1 + args.reps, "pictures": n, "content": args.contents.split(",")[0]}))


def trace_summary(trace_dir, plan, _earlier=None):
    per = plan["launches"]
    cut = read_planned(trace_dir, [(label, kernel, per) for label, kernel in trace_plan()])
    if "error" in cut:
        return cut
    stats = lambda r: launch_stats(l.ns for l in r[1:])                               # without the warm-up launch
    res = {"pictures": plan["pictures"], "content": plan["content"], **resources(cut["erode1"][0])}
    floor = stats(cut["scale_identity"])
    for label, _kernel in trace_plan():
        t = stats(cut[label])
        t["bytes"] = 2 * plan["pictures"] * PIC_BYTES
        t["of_peak_median"] = round(t["bytes"] / (t["median_us"] * 1e-6) / PEAK, 3)
        t["over_scale_identity_kernel"] = round(t["median_us"] / floor["median_us"], 2)
        res[label] = t
    med = lambda label: res[label]["median_us"]
    res["ratios"] = {"erode15_over_erode1": round(med("erode15") / med("erode1"), 2), "erode1_over_binomial3": round(med("erode1") / med("binomial3"), 2),
                     "median5_over_median3": round(med("median5") / med("median3"), 2)}
    # the one condition, no tolerance: the sub-linear min of radius 15 against the linear filter's 31 taps a pass
    res["condition"] = {"what": "erode radius 15 kernel <= Gaussian radius 15 filter kernel, same session", "erode15_us": med("erode15"),
                        "gauss5_r15_us": med("gauss5_r15"), "holds": med("erode15") <= med("gauss5_r15")}
    return res


def main():
    ap = argparse.ArgumentParser()
    add_common_arguments(ap, children=("calls", "trace"), reps=20, warmup=3, rounds=5, steps="calls,trace", out_dir="rank_bench_out", out="--out")
    ap.add_argument("--contents", default="natural")
    ap.add_argument("--route-pictures", type=int, default=32, help="pictures the torch route works on (unfold of a 5 x 5 window takes 100 bytes a sample)")
    args = ap.parse_args()
    if args.child:
        return {"calls": child_calls, "trace": child_trace}[args.child](args)
    drive(args, {"calls": ("calls", None), "trace": ("trace", trace_summary)}, [sys.executable, os.path.abspath(__file__)])


if __name__ == "__main__":
    main()
