"""Corner detection on pictures in slot layout (hvq_corner_pictures) on the GPU.

Two measurements (steps of tools/benchlib.py), per content preset (--contents):
  calls   128 640x480 4:2:0 streams, 8 resident pictures each, 1024 pictures per call: (a) corner_pictures with harris(1, nms=3), every
          output including the response map, and in the same session (b) a torch route that computes the response map ALONE on a device
          copy of the luma of some of the pictures (--route-pictures; its time is scaled to the call's pictures): replicate padding, the
          Sobel pair by int64 slices, the products, the window sums by slices.  HIP-event timed per call on one stream in alternating
          rounds after a warm-up; medians over the rounds.  (a) must equal hvqm4_amd.corners on pictures read back, and the torch route
          must equal (a)'s response maps before either is timed.  Condition 1: (a) is faster.
  trace   the kernel trace of a child that launches corner_pictures per entry -- Harris at (r, nms) = (1, 3), (3, 3), (1, 0), (1, 7), the
          min-eigenvalue measure at (1, 3), all without the response map, and Harris at (1, 3) with it --, then filter_pictures (the Sobel magnitude on luma) and map_pictures (a table on luma), one
          warm-up and `reps` launches each.  Kernel times are read from the trace: median with min-max per kernel and entry; the tile
          launch beside the filter kernel, r = 3 over r = 1, nms = 7 over nms = 0, and launches 2 to 4 together beside the map kernel.
          No pass mark.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.benchlib import (add_common_arguments, drive, launch_stats, optional_route, picture_lists, read_planned, resident, resources,  # noqa: E402
                            timed)

W, H = 640, 480
SRC = (W, H, 2, 2)
PIC_BYTES = W * H * 3 // 2
CAP = 4096
CORNER_KERNELS = ("hvq_corner_tile_kernel", "hvq_corner_count_kernel", "hvq_corner_scan_kernel", "hvq_corner_list_kernel")
# (label, mode, radius, nms, with the response map): the ratios are taken of the launches WITHOUT the map, whose 8 bytes a sample would
# otherwise be most of launch 1; one entry with it says what it costs
ENTRIES = (("harris_r1_nms3", 0, 1, 3, False), ("harris_r3_nms3", 0, 3, 3, False), ("harris_r1_nms0", 0, 1, 0, False), ("harris_r1_nms7", 0, 1, 7, False),
           ("min_eigen_r1_nms3", 1, 1, 3, False), ("harris_r1_nms3_response", 0, 1, 3, True))


def rule_of(mode, radius, nms):
    from hvqm4_amd import corners as cr
    return cr.min_eigen(radius, nms=nms) if mode else cr.harris(radius, 10, nms=nms)


def trace_plan():
    """(label, kernel or the kernels of one call) of the trace step's blocks in launch order"""
    return [(label, CORNER_KERNELS) for label, _m, _r, _n, _q in ENTRIES] + [("sobel_magnitude", "hvq_filter_kernel"), ("map", "hvq_map_kernel")]


def flat_plan(per):
    plan = []
    for label, kernel in trace_plan():
        if isinstance(kernel, str):
            plan.append((label, kernel, per))
        else:
            plan += [(f"{label}/{r}/{k}", k, 1) for r in range(per) for k in kernel]
    return plan


def torch_route(torch, luma, radius=1, k=10):
    """the Harris response maps of `luma` uint8 [m, H, W] the way a pipeline without the call gets them -> int64 [m, H, W]"""
    tf = torch.nn.functional
    m, h, w = luma.shape
    p = tf.pad(luma.to(torch.float32).view(m, 1, h, w), (radius + 1,) * 4, mode="replicate").to(torch.int64).view(m, h + 2 * radius + 2, w + 2 * radius + 2)
    gx = (p[:, :-2, 2:] + 2 * p[:, 1:-1, 2:] + p[:, 2:, 2:]) - (p[:, :-2, :-2] + 2 * p[:, 1:-1, :-2] + p[:, 2:, :-2])
    gy = (p[:, 2:, :-2] + 2 * p[:, 2:, 1:-1] + p[:, 2:, 2:]) - (p[:, :-2, :-2] + 2 * p[:, :-2, 1:-1] + p[:, :-2, 2:])
    n = 2 * radius + 1

    def window(v):
        rows = sum(v[:, i:i + h, :] for i in range(n))
        return sum(rows[:, :, j:j + w] for j in range(n))
    A, B, C = window(gx * gx), window(gx * gy), window(gy * gy)
    T = A + C
    return 256 * (A * C - B * B) - k * T * T


def setup(args, preset):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    a_s, a_o = picture_lists(resident(ctx, preset=preset, streams=args.streams, per=args.per, distinct=args.distinct), args.per)
    return torch, ctx, a_s, a_o


def rooms(torch, n):
    """the outputs of a call of n pictures, allocated once"""
    return dict(mask=[t for t in torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")], points=[t for t in torch.empty((n, CAP + 1, 4), dtype=torch.int64, device="cuda")],
                rows=[t for t in torch.empty((n, (H + 1 + 3) // 4 * 4), dtype=torch.int32, device="cuda")[:, :H + 1]],      # rows of 484: 16-byte multiples
                response=[t for t in torch.empty((n, H, W), dtype=torch.int64, device="cuda")])


def child_calls(args):
    import numpy as np
    from hvqm4_amd import corners as cr
    res = {"size": f"{W}x{H}", "reps": args.reps, "rounds": args.rounds, "contents": {}}
    rule = cr.harris(1, 10, nms=3)
    for preset in args.contents.split(","):
        torch, ctx, a_s, a_o = setup(args, preset)
        n = len(a_s)
        m = min(n, args.route_pictures)
        out = rooms(torch, n)
        host = [ctx.read_picture(a_s[i], a_o[i]) for i in range(m)]
        luma = torch.from_numpy(np.stack([p[:W * H].reshape(H, W) for p in host])).cuda()      # what the torch route works on
        got = {}

        def call():
            got["r"] = ctx.corner_pictures(a_s, a_o, rule, cap=CAP, mask=out["mask"], points=out["points"], rows=out["rows"], response=out["response"])
        timed(torch, call, args.warmup)
        mask, points, rows, response = got["r"]
        probe = list(range(0, m, max(1, m // 4)))
        agree = True
        for i in probe:
            wm, wp, wr = cr.of_picture(host[i], SRC, rule, CAP)
            agree &= np.array_equal(mask[i].cpu().numpy(), wm) and np.array_equal(points[i][:wp.shape[0]].cpu().numpy(), wp) and np.array_equal(rows[i].cpu().numpy().view(np.uint32), wr)
        route, off = optional_route(torch, lambda: torch_route(torch, luma))
        equal = bool(all(torch.equal(r, response[i]) for i, r in enumerate(route()))) if route else None
        t = {"pictures": n, "route_pictures": m, "corners_ms": [], "torch_ms": [], "corners_per_picture_median": int(statistics.median(int(p[0, 0]) for p in points[:m]))}
        for _ in range(args.rounds):
            t["corners_ms"].append(round(timed(torch, call, args.reps), 4))
            if route:
                t["torch_ms"].append(round(timed(torch, route, 1) * n / m, 4))                 # scaled from m pictures to the call's n
        for k in ("corners", "torch"):
            t[k + "_median_ms"] = statistics.median(t[k + "_ms"]) if t[k + "_ms"] else None
        t["corners_spread"] = round(max(t["corners_ms"]) / min(t["corners_ms"]), 3)
        t["torch_over_corners"] = round(t["torch_median_ms"] / t["corners_median_ms"], 1) if route else None
        t["equal_host_module"] = bool(agree)
        t["torch_route_equal"] = equal
        t["torch_route_missing"] = off
        t["condition_1"] = {"what": "the call (everything, response included) is faster than the torch route to the response map alone, same session, first held == to it",
                            "holds": bool(route and equal and agree and min(t["torch_ms"]) > max(t["corners_ms"]))}
        res["contents"][preset] = t
        ctx.close()
    print(json.dumps(res))


def child_trace(args):
    """the launches the trace is taken of: per entry 1 + reps calls of corner_pictures (four kernels each), then of the filter kernel
    (Sobel magnitude on luma) and of the map kernel (a table on luma); the first content preset"""
    from hvqm4_amd import filters as F
    from hvqm4_amd import maps as M
    preset = args.contents.split(",")[0]
    torch, ctx, a_s, a_o = setup(args, preset)
    n = len(a_s)
    out = rooms(torch, n)
    pics = torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
    for _label, mode, radius, nms, with_map in ENTRIES:
        for _ in range(1 + args.reps):
            ctx.corner_pictures(a_s, a_o, rule_of(mode, radius, nms), cap=CAP, mask=out["mask"], points=out["points"], rows=out["rows"],
                                response=out["response"] if with_map else None)
        torch.cuda.synchronize()
    for call in (lambda: ctx.filter_pictures(a_s, a_o, F.luma_only(F.gradient_magnitude()), out=pics), lambda: ctx.map_pictures(a_s, a_o, M.invert().luma_only(), out=pics)):
        for _ in range(1 + args.reps):
            call()
        torch.cuda.synchronize()
    ctx.close()
    print(json.dumps({"launches": 1 + args.reps, "pictures": n, "content": preset}))


def trace_summary(trace_dir, plan, _earlier=None):
    per = plan["launches"]
    cut = read_planned(trace_dir, flat_plan(per), kernels=set(CORNER_KERNELS) | {"hvq_filter_kernel", "hvq_map_kernel"})
    if "error" in cut:
        return cut
    res = {"pictures": plan["pictures"], "content": plan["content"], "kernels": {k: resources(cut[f"{ENTRIES[0][0]}/0/{k}"][0]) for k in CORNER_KERNELS}}
    for label, kernel in trace_plan():
        if isinstance(kernel, str):
            res[label] = launch_stats(l.ns for l in cut[label][1:])                               # without the warm-up launch
            continue
        row = {k: launch_stats(cut[f"{label}/{r}/{k}"][0].ns for r in range(1, per)) for k in kernel}
        row["list_median_us"] = round(sum(row[k]["median_us"] for k in kernel[1:]), 1)            # launches 2 to 4 together
        res[label] = row
    tile = lambda label: res[label][CORNER_KERNELS[0]]["median_us"]
    res["ratios"] = {"tile_over_sobel_magnitude": round(tile("harris_r1_nms3") / res["sobel_magnitude"]["median_us"], 2),
                     "r3_over_r1": round(tile("harris_r3_nms3") / tile("harris_r1_nms3"), 2), "nms7_over_nms0": round(tile("harris_r1_nms7") / tile("harris_r1_nms0"), 2),
                     "response_map_over_none": round(tile("harris_r1_nms3_response") / tile("harris_r1_nms3"), 2),
                     "list_launches_over_map_kernel": round(res["harris_r1_nms3"]["list_median_us"] / res["map"]["median_us"], 2)}
    return res


def main():
    ap = argparse.ArgumentParser()
    add_common_arguments(ap, children=("calls", "trace"), reps=10, warmup=2, rounds=5, steps="calls,trace", out_dir="corner_bench_out", out="--out")
    ap.add_argument("--contents", default="natural,dense")
    ap.add_argument("--route-pictures", type=int, default=16, help="pictures the torch route works on (its int64 intermediates take some 100 bytes a sample)")
    args = ap.parse_args()
    if args.child:
        return {"calls": child_calls, "trace": child_trace}[args.child](args)
    drive(args, {"calls": ("calls", None), "trace": ("trace", trace_summary)}, [sys.executable, os.path.abspath(__file__)])


if __name__ == "__main__":
    main()
