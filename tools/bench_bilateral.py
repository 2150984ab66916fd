"""Bilateral filters on pictures in slot layout (hvq_bilateral_pictures) on the GPU.

Two measurements (steps of tools/benchlib.py), per content preset (--contents):
  calls   128 640x480 4:2:0 streams, 8 resident pictures each, 1024 pictures per call: (a) bilateral_pictures with the Gaussian set 1.5 /
          12 at radius 2, and in the same session (b) a torch route on a device copy of some of the pictures (--route-pictures; its time
          is scaled to the call's pictures): per plane replicate padding, unfold, the absolute difference to the centre, a gather from the
          range table, the weighted sums and an integer division -- the only way to these bytes without the call.  HIP-event timed per
          call on one stream in alternating rounds after a warm-up; medians over the rounds.  (a) must equal hvqm4_amd.bilateral on
          pictures read back, and the torch route must equal (a) byte for byte before either is timed.  Condition 1: (a) is faster.
  trace   the kernel trace of a child that launches bilateral_pictures per entry -- wide Gaussians (sigma 4, so that no tap rounds to 0)
          at the radii 1, 2, 3, 5, 7, the set of the calls step, the full square and the disc of radius 5 under one range table, the
          identity through both bodies, the calls step's set guided by another resident picture --, then scale_pictures (identity),
          filter_pictures (the Gaussian of radius 2) and rank_pictures (the 5 x 5 median) in a fixed order, one warm-up and `reps` launches
          each.  Kernel times are read from the trace: median with min-max per entry, the time per tap and 1024 pictures the radii
          imply, every kernel as a multiple of the scale identity kernel, and condition 2: the disc takes less kernel time than the
          square (the ratio stands beside the ratio of the tap counts).
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
GENERAL = "identity_general"                       # the identity with hvq_bilateral_force_general: the general body at radius 0
GUIDED = "gauss_r2_guided"
RADII = (1, 2, 3, 5, 7)


def the_sets():
    from hvqm4_amd import bilateral as B
    rng = B.bilateral(1.5, 12).luma.range
    square5 = B.from_tables(5, 5, [[1] * 6] * 6, list(rng))
    disc5 = B.disc(5, sigma_range=12.0)
    assert disc5.luma.range == rng
    return [(f"wide_r{r}", B.bilateral(4.0, 12, r)) for r in RADII] + \
           [("gauss_r2", B.bilateral(1.5, 12, 2)), ("square5", square5), ("disc5", disc5), ("identity", B.identity()), (GENERAL, B.identity()), (GUIDED, B.bilateral(1.5, 12, 2))]


def trace_plan():
    """(label, kernel) of the trace step's blocks in launch order"""
    return [(label, "hvq_bilateral_kernel") for label in [f"wide_r{r}" for r in RADII] + ["gauss_r2", "square5", "disc5", "identity", GENERAL, GUIDED]] + \
           [("scale_identity", "hvq_scale_kernel"), ("filter_gauss_r2", "hvq_filter_kernel"), ("median5", "hvq_rank_kernel")]


def torch_route(torch, copy, bil):
    """the pictures the way a pipeline without the call gets them, per plane: replicate padding, unfold, |difference| to the centre, the
    range table gathered, weighted sums, an integer division"""
    from hvqm4_amd import scale
    tf = torch.nn.functional
    n = copy.shape[0]
    out, at = [], 0
    for p, (nx, ny, _mx, _my) in enumerate(scale.plane_sizes(SRC, SRC)):
        pb = bil.chroma if p else bil.luma
        raw = copy[:, at:at + nx * ny]
        at += nx * ny
        x = tf.pad(raw.to(torch.float32).view(n, 1, ny, nx), (pb.rx, pb.rx, pb.ry, pb.ry), mode="replicate")
        win = tf.unfold(x, (2 * pb.ry + 1, 2 * pb.rx + 1)).to(torch.int64)                       # [n, taps, ny nx]
        spatial = torch.tensor([pb.spatial[8 * abs(j) + abs(i)] for j in range(-pb.ry, pb.ry + 1) for i in range(-pb.rx, pb.rx + 1)],
                               dtype=torch.int64, device=copy.device).view(1, -1, 1)
        rng = torch.tensor(list(pb.range), dtype=torch.int64, device=copy.device)
        w = rng[(win - raw.to(torch.int64).view(n, 1, -1)).abs()] * spatial
        den = w.sum(dim=1)
        num = (w * win).sum(dim=1)
        out.append(torch.div(num + torch.div(den, 2, rounding_mode="floor"), den, rounding_mode="floor").to(torch.uint8))
    return torch.cat(out, dim=1)


def setup(args, preset):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    a_s, a_o = picture_lists(resident(ctx, preset=preset, streams=args.streams, per=args.per, distinct=args.distinct), args.per)
    return torch, ctx, a_s, a_o


def _guide(a_s, a_o, per):
    """every picture guided by the next resident one of its stream"""
    return [(s, (o + 1) % per) for s, o in zip(a_s, a_o)]


def child_calls(args):
    import numpy as np
    from hvqm4_amd import bilateral as B
    res = {"size": f"{W}x{H}", "reps": args.reps, "rounds": args.rounds, "contents": {}}
    b = B.bilateral(1.5, 12, 2)
    for preset in args.contents.split(","):
        torch, ctx, a_s, a_o = setup(args, preset)
        n = len(a_s)
        m = min(n, args.route_pictures)
        out = torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
        probe = list(range(0, n, max(1, n // 4)))
        host = {i: ctx.read_picture(a_s[i], a_o[i]) for i in probe}
        copy = torch.from_numpy(np.stack([ctx.read_picture(a_s[i], a_o[i]) for i in range(m)])).cuda()  # what the torch route works on
        call = lambda: ctx.bilateral_pictures(a_s, a_o, b, out=out)
        timed(torch, call, args.warmup)
        got = out.cpu().numpy()
        agree = all(np.array_equal(got[i], B.of_picture(host[i], SRC, b)) for i in probe)
        route, off = optional_route(torch, lambda: torch_route(torch, copy, b))
        equal = bool(torch.equal(route(), out[:m])) if route else None
        t = {"pictures": n, "route_pictures": m, "bilateral_ms": [], "torch_ms": []}
        for _ in range(args.rounds):
            t["bilateral_ms"].append(round(timed(torch, call, args.reps), 4))
            if route:
                t["torch_ms"].append(round(timed(torch, route, 1) * n / m, 4))                    # scaled from m pictures to the call's n
        for k in ("bilateral", "torch"):
            t[k + "_median_ms"] = statistics.median(t[k + "_ms"]) if t[k + "_ms"] else None
        t["bilateral_spread"] = round(max(t["bilateral_ms"]) / min(t["bilateral_ms"]), 3)
        t["torch_over_bilateral"] = round(t["torch_median_ms"] / t["bilateral_median_ms"], 1) if route else None
        t["equal_host_module"] = bool(agree)
        t["torch_route_equal"] = equal
        t["torch_route_missing"] = off
        t["condition_1"] = {"what": "the call is faster than the torch route of the same session, which is first held == to it",
                            "holds": bool(route and equal and agree and min(t["torch_ms"]) > max(t["bilateral_ms"]))}
        res["contents"][preset] = t
        ctx.close()
    print(json.dumps(res))


def child_trace(args):
    """the launches the trace is taken of: per entry 1 + reps of the bilateral kernel, then of the scale kernel (identity), of the filter
    kernel (Gaussian radius 2) and of the rank kernel (median 5 x 5); the first content preset"""
    from hvqm4_amd import filters as F
    from hvqm4_amd import rank as R
    preset = args.contents.split(",")[0]
    torch, ctx, a_s, a_o = setup(args, preset)
    n = len(a_s)
    out = torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
    for label, b in the_sets():
        was = ctx.bilateral_force_general(label == GENERAL)
        guide = _guide(a_s, a_o, args.per) if label == GUIDED else None
        for _ in range(1 + args.reps):
            ctx.bilateral_pictures(a_s, a_o, b, guide=guide, out=out)
        torch.cuda.synchronize()
        ctx.bilateral_force_general(was)
    for call in (lambda: ctx.scale_pictures(a_s, a_o, (W, H), out=out), lambda: ctx.filter_pictures(a_s, a_o, F.gaussian(1.5, 2), out=out),
                 lambda: ctx.rank_pictures(a_s, a_o, R.median(5), out=out)):
        for _ in range(1 + args.reps):
            call()
        torch.cuda.synchronize()
    ctx.close()
    taps = {label: [b.luma.taps(), b.chroma.taps()] for label, b in the_sets()}
    print(json.dumps({"launches": 1 + args.reps, "pictures": n, "content": preset, "taps": taps}))


def trace_summary(trace_dir, plan, _earlier=None):
    per = plan["launches"]
    cut = read_planned(trace_dir, [(label, kernel, per) for label, kernel in trace_plan()])
    if "error" in cut:
        return cut
    stats = lambda r: launch_stats(l.ns for l in r[1:])                               # without the warm-up launch
    res = {"pictures": plan["pictures"], "content": plan["content"], **resources(cut["wide_r2"][0])}
    floor = stats(cut["scale_identity"])
    for label, _kernel in trace_plan():
        t = stats(cut[label])
        t["bytes"] = 2 * plan["pictures"] * PIC_BYTES
        t["of_peak_median"] = round(t["bytes"] / (t["median_us"] * 1e-6) / PEAK, 3)
        t["over_scale_identity_kernel"] = round(t["median_us"] / floor["median_us"], 2)
        if label in plan.get("taps", {}):
            t["taps_luma_chroma"] = plan["taps"][label]
        res[label] = t
    med = lambda label: res[label]["median_us"]
    # the time a tap costs: the slope between neighbouring radii, (2 r + 1)^2 taps in every plane
    res["us_per_tap"] = {f"r{a}_to_r{b}": round((med(f"wide_r{b}") - med(f"wide_r{a}")) / ((2 * b + 1) ** 2 - (2 * a + 1) ** 2), 2) for a, b in zip(RADII, RADII[1:])}
    res["ratios"] = {"identity_over_scale_identity": round(med("identity") / med("scale_identity"), 2), "gauss_r2_over_filter_gauss_r2": round(med("gauss_r2") / med("filter_gauss_r2"), 2),
                     "gauss_r2_over_median5": round(med("gauss_r2") / med("median5"), 2), "guided_over_unguided": round(med(GUIDED) / med("gauss_r2"), 2),
                     "identity_general_over_identity": round(med(GENERAL) / med("identity"), 2)}
    taps = plan.get("taps", {})
    res["condition_2"] = {"what": "the disc of radius 5 takes less kernel time than the full square of radius 5, same session", "disc5_us": med("disc5"), "square5_us": med("square5"),
                          "time_ratio": round(med("disc5") / med("square5"), 3), "tap_ratio": round(taps["disc5"][0] / taps["square5"][0], 3) if taps else None,
                          "holds": res["disc5"]["max_us"] < res["square5"]["min_us"]}
    return res


def main():
    ap = argparse.ArgumentParser()
    add_common_arguments(ap, children=("calls", "trace"), reps=10, warmup=2, rounds=5, steps="calls,trace", out_dir="bilateral_bench_out", out="--out")
    ap.add_argument("--contents", default="natural,dense")
    ap.add_argument("--route-pictures", type=int, default=16, help="pictures the torch route works on (unfold of a 5 x 5 window as int64 takes 200 bytes a sample)")
    args = ap.parse_args()
    if args.child:
        return {"calls": child_calls, "trace": child_trace}[args.child](args)
    drive(args, {"calls": ("calls", None), "trace": ("trace", trace_summary)}, [sys.executable, os.path.abspath(__file__)])


if __name__ == "__main__":
    main()
