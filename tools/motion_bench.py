"""Motion fields (hvq_picture_motion, Context.picture_motion) on the GPU: 128 dense 640x480 4:2:0 streams, 8 resident pictures each, 1024
pairs per call, at B = 16 with R = 8 and R = 15 and at B = 8 with R = 8; three contents: natural (picture k against k - 1 inside the
stream's 8 pictures), flat (a flat reference in the caller's memory: every candidate of a block ties) and a picture against itself
(every cost is 0 at the zero vector).

Two measurements (steps of tools/benchlib.py):
  calls   HIP-event timed on one stream, in alternating rounds: (a) the nine motion calls; (b) the route a user takes without the call,
          on the natural pairs at each setting: export(..., "yuv444p") of both pictures, then per displacement abs of the shifted luma
          difference and avg_pool2d(B), and a running minimum of the packed tuple (cost, |dy| + |dx|, dy, dx) -- in chunks of pictures,
          so that the route's temporaries fit.  The fields of the route and of the call are compared before anything is timed.
  trace   the kernel trace of a child that launches the same nine calls in a fixed order, one warm-up and `reps`
          launches each.  Kernel times are read from the trace: median with min-max, beside the arithmetic estimate of the time the byte
          differences alone would take as 4-byte SAD lane operations at the VALU issue rate (blocks x candidates x B^2 / 4 lane
          operations; 256 CUs x 64 lanes per clock at 2.4 GHz), and the fraction of it reached.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.benchlib import add_common_arguments, drive, launch_stats, picture_lists, read_planned, resident, resources, timed  # noqa: E402

W, H = 640, 480
PIC_BYTES = W * H * 3 // 2
SETTINGS = [(16, 8), (16, 15), (8, 8)]
CONTENTS = ["natural", "flat", "itself"]
FLAT = 100
LANE_OPS_PER_S = 256 * 64 * 2.4e9


def setup(args):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    sids = resident(ctx, preset="dense", streams=args.streams, per=args.per, distinct=args.distinct)
    return torch, ctx, sids


def label(content, B, R):
    return f"{content}_b{B}_r{R}"


def workload(torch, ctx, sids, per):
    """label -> callable: the nine calls over the same 1024 pictures"""
    from hvqm4_amd.motion import blocks
    a_s, a_o = picture_lists(sids, per)
    n = len(a_s)
    flat = torch.full((PIC_BYTES,), FLAT, dtype=torch.uint8, device="cuda")
    refs = {"natural": [(s, (k - 1) % per) for s in sids for k in range(per)], "flat": [flat] * n, "itself": list(zip(a_s, a_o))}
    outs = {B: [torch.empty(blocks(W, H, B) + (4,), dtype=torch.int32, device="cuda") for _ in range(n)] for B in (8, 16)}
    calls = {}
    for B, R in SETTINGS:
        for c in CONTENTS:
            calls[label(c, B, R)] = (lambda c=c, B=B, R=R: ctx.picture_motion(a_s, a_o, refs[c], block=B, radius=R, out=outs[B]))
    return calls, (a_s, a_o, refs, outs, flat)


def torch_route(torch, ctx, a_s, a_o, refs, B, R, chunk):
    """the fields of resident pairs without the call -> int64 [n, rows, cols] packed keys (cost << 15 | L1 << 10 | dy + R << 5 | dx + R)"""
    import torch.nn.functional as F
    n, rows, cols = len(a_s), H // B, W // B
    keys = torch.empty((n, rows, cols), dtype=torch.int64, device="cuda")
    ua = torch.empty((chunk, 3, H, W), dtype=torch.uint8, device="cuda")
    ub = torch.empty((chunk, 3, H, W), dtype=torch.uint8, device="cuda")
    for at in range(0, n, chunk):
        m = min(chunk, n - at)
        ctx.export(a_s[at:at + m], a_o[at:at + m], ua[:m], "yuv444p")
        ctx.export([r[0] for r in refs[at:at + m]], [r[1] for r in refs[at:at + m]], ub[:m], "yuv444p")
        A, Bm = ua[:m, 0].to(torch.float32), ub[:m, 0].to(torch.float32)
        best = torch.full((m, rows, cols), 1 << 40, dtype=torch.int64, device="cuda")
        for dy in range(-R, R + 1):
            r0, r1 = max(0, -(dy // B)), min(rows - 1, (H - B - dy) // B)
            for dx in range(-R, R + 1):
                c0, c1 = max(0, -(dx // B)), min(cols - 1, (W - B - dx) // B)
                if r0 > r1 or c0 > c1:
                    continue
                d = (A[:, r0 * B:(r1 + 1) * B, c0 * B:(c1 + 1) * B] - Bm[:, r0 * B + dy:(r1 + 1) * B + dy, c0 * B + dx:(c1 + 1) * B + dx]).abs()
                cost = (F.avg_pool2d(d[:, None], B)[:, 0] * (B * B)).to(torch.int64)      # exact: sums below 2^24, B^2 a power of two
                key = cost << 15 | ((abs(dy) + abs(dx)) << 10 | (dy + R) << 5 | (dx + R))
                best[:, r0:r1 + 1, c0:c1 + 1] = torch.minimum(best[:, r0:r1 + 1, c0:c1 + 1], key)
        keys[at:at + m] = best
    return keys


def child_calls(args):
    torch, ctx, sids = setup(args)
    calls, (a_s, a_o, refs, outs, _flat) = workload(torch, ctx, sids, args.per)
    n = len(a_s)
    fns = dict(calls)
    for B, R in SETTINGS:
        fns[f"route_b{B}_r{R}"] = (lambda B=B, R=R: torch_route(torch, ctx, a_s, a_o, refs["natural"], B, R, args.chunk))
    agree = {}
    for B, R in SETTINGS:                                   # the call against the route, before anything is timed
        calls[label("natural", B, R)]()
        f = torch.stack(outs[B]).to(torch.int64)
        k = f[..., 2] << 15 | (f[..., 0].abs() + f[..., 1].abs()) << 10 | (f[..., 0] + R) << 5 | (f[..., 1] + R)
        agree[f"b{B}_r{R}"] = bool(torch.equal(k, torch_route(torch, ctx, a_s, a_o, refs["natural"], B, R, args.chunk)))
        calls[label("itself", B, R)]()
        torch.cuda.synchronize()
        agree[f"itself_b{B}_r{R}"] = bool(not torch.stack(outs[B]).any())
    if not all(agree.values()):
        sys.exit(f"wrong fields ({agree}): nothing is timed")
    for k, fn in calls.items():
        timed(torch, fn, args.warmup)
    res = {"size": f"{W}x{H}", "pictures": n, "reps": args.reps, "rounds": args.rounds, "route_chunk": args.chunk, "ms": {k: [] for k in fns}}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            res["ms"][k].append(round(timed(torch, fn, args.route_reps if k.startswith("route") else args.reps), 4))
    med = {k: statistics.median(v) for k, v in res["ms"].items()}
    res["median_ms"] = med
    for B, R in SETTINGS:
        res[f"route_over_call_b{B}_r{R}"] = round(med[f"route_b{B}_r{R}"] / med[label("natural", B, R)], 1)
    res["agrees_with_the_route"] = agree
    ctx.close()
    print(json.dumps(res))


def child_trace(args):
    """the launches the trace is taken of, in the order trace_summary reads them by"""
    torch, ctx, sids = setup(args)
    calls, _keep = workload(torch, ctx, sids, args.per)
    plan = []
    for lab, fn in calls.items():
        for _ in range(1 + args.reps):
            fn()
        torch.cuda.synchronize()
        plan.append([lab, 1 + args.reps, args.streams * args.per])
    ctx.close()
    print(json.dumps({"plan": plan}))


def estimate_ms(n, B, R):
    """the byte differences of every inside candidate as 4-byte SAD lane operations at the VALU issue rate (an estimate, not a measurement)"""
    rows, cols = H // B, W // B
    cand = sum(sum(1 for dy in range(-R, R + 1) if 0 <= r * B + dy and r * B + dy + B <= H) for r in range(rows)) * \
        sum(sum(1 for dx in range(-R, R + 1) if 0 <= c * B + dx and c * B + dx + B <= W) for c in range(cols))
    return n * cand * (B * B // 4) / LANE_OPS_PER_S * 1e3


def trace_summary(trace_dir, printed, _earlier=None):
    plan = printed["plan"]
    cut = read_planned(trace_dir, [(lab, "hvq_motion_kernel", count) for lab, count, _n in plan])
    if "error" in cut:
        return cut
    res = {}
    for lab, _count, n in plan:
        part = cut[lab][1:]                                                       # without the warm-up launch
        d = [l.ns for l in part]
        B, R = int(lab.split("_b")[1].split("_r")[0]), int(lab.split("_r")[1])
        est = estimate_ms(n, B, R)
        res[lab] = {"pictures": n, **launch_stats(d), "sad_estimate_us": round(est * 1e3, 1), "estimate_over_median": round(est * 1e6 / statistics.median(d), 3),
                    **resources(part[0])}
    return res


def main():
    ap = argparse.ArgumentParser()
    add_common_arguments(ap, children=("calls", "trace"), reps=10, warmup=2, rounds=3, steps="calls,trace", step_timeout=420, out_dir="motion_bench_out")
    ap.add_argument("--route-reps", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=128, help="pictures the torch route handles at a time")
    args = ap.parse_args()
    if args.child:
        return {"calls": child_calls, "trace": child_trace}[args.child](args)
    drive(args, {"calls": ("calls", None), "trace": ("trace", trace_summary)}, [sys.executable, os.path.abspath(__file__)])


if __name__ == "__main__":
    main()
