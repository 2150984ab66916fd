"""Warped pictures in slot layout (hvq_warp_pictures) on the GPU: the measurement that sets the rule of hvq_wp_choose (hvq_warp.h).

Two measurements (steps of tools/benchlib.py):
  calls   128 640x480 4:2:0 streams, 8 resident pictures each, 1024 pictures per call, on natural content, through the identity, a
          half-sample translation, rotations by 5 and 45 degrees, the quarter turn into 480x640, zoom 1/2 into 320x240 and zoom 2, each
          under the chosen body, the forced direct body and the tiled body wherever LDS holds the box: (a) warp_pictures, (b)
          scale_pictures to the pictures' own geometry on the same pictures -- it reads and writes the same bytes: the memory floor of
          the identity --, (c) a torch route on a device copy of the same pictures: per plane a float view, affine_grid + grid_sample,
          rounding, cast, concatenation.  HIP-event timed per call on one stream in alternating rounds after a warm-up; medians over
          the rounds.  (a) must equal hvqm4_amd.warp on pictures read back under every body.
  trace   the kernel trace of a child that launches warp_pictures per map and body and scale_pictures (identity) in a
          fixed order, one warm-up and `reps` launches each; one configuration (the identity under the direct body) is repeated at the
          start, in the middle and at the end: the largest distance between the medians of its three blocks is the run-to-run spread.
          Kernel times are read from the trace: median with min-max per map and body, and per map whether the body the rule chose is
          no slower than the direct one plus the spread.
"""
import argparse
import json
import os
import statistics
import sys
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.benchlib import (add_common_arguments, drive, launch_stats, optional_route, picture_lists, read_planned, resident, resources,  # noqa: E402
                            timed)

W, H = 640, 480
SRC = (W, H, 2, 2)
BODIES = (("chosen", 0), ("direct", 1), ("tiled", 2))
SPREAD_AFTER = 3                                     # the spread block is repeated after the map of this index


def the_maps():
    """(label, Warp, target geometry)"""
    from hvqm4_amd import warp as wp
    c = (Fraction(W, 2), Fraction(H, 2))
    turn, size = wp.rotate90(1, W, H)
    return [("identity", wp.identity(), SRC), ("translate_half", wp.translate(Fraction(-1, 2), Fraction(-1, 2)), SRC), ("rotate5", wp.rotate(5, W, H), SRC),
            ("rotate45", wp.rotate(45, W, H), SRC), ("quarter_turn", turn, size + (2, 2)), ("zoom_half_to_320x240", wp.zoom(Fraction(1, 2)), (320, 240, 2, 2)),
            ("zoom2", wp.zoom(2, centre=c), SRC)]


def torch_route(torch, copy, w, tg, chunk=128):
    """the warped pictures the way a pipeline without the call gets them: per plane a float view, affine_grid + grid_sample (bilinear,
    align_corners=False: sample centres at integer + 1/2, as here), rounding, cast, concatenation"""
    from hvqm4_amd import warp as wp
    tf = torch.nn.functional
    outs = []
    for at0 in range(0, copy.shape[0], chunk):
        part = copy[at0:at0 + chunk]
        n = part.shape[0]
        out, at = [], 0
        for p in range(3):
            (hd, vd), (hs, vs) = wp._samplings(SRC, tg, p)
            nx, ny = wp.plane_dims(SRC, p)
            mx, my = wp.plane_dims(tg, p)
            a, b, cc = w.m00 / 65536 * hd / hs, w.m01 / 65536 * vd / hs, w.t0 / 65536 / hs
            d, e, ff = w.m10 / 65536 * hd / vs, w.m11 / 65536 * vd / vs, w.t1 / 65536 / vs
            theta = torch.tensor([[a * mx / nx, b * my / nx, (a * mx + b * my + 2 * cc) / nx - 1], [d * mx / ny, e * my / ny, (d * mx + e * my + 2 * ff) / ny - 1]],
                                 dtype=torch.float32, device="cuda")
            plane = part[:, at:at + nx * ny].to(torch.float32).view(n, 1, ny, nx)
            at += nx * ny
            grid = tf.affine_grid(theta.expand(n, 2, 3), (n, 1, my, mx), align_corners=False)
            s = tf.grid_sample(plane, grid, mode="bilinear", padding_mode="border", align_corners=False)
            out.append(torch.floor(s + 0.5).clamp_(0, 255).to(torch.uint8).view(n, -1))
        outs.append(torch.cat(out, dim=1))
    return torch.cat(outs, dim=0)


def setup(args):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    a_s, a_o = picture_lists(resident(ctx, preset=args.contents.split(",")[0], streams=args.streams, per=args.per, distinct=args.distinct), args.per)
    return torch, ctx, a_s, a_o


def child_calls(args):
    import numpy as np
    from hvqm4_amd import scale
    from hvqm4_amd import warp as wp
    torch, ctx, a_s, a_o = setup(args)
    n = len(a_s)
    pb = scale.nbytes(*SRC)
    res = {"size": f"{W}x{H}", "pictures": n, "reps": args.reps, "rounds": args.rounds, "content": args.contents.split(",")[0], "maps": {}}
    copy = torch.empty((n, pb), dtype=torch.uint8, device="cuda")
    sout = torch.empty((n, pb), dtype=torch.uint8, device="cuda")
    probe = list(range(0, n, max(1, n // 8)))
    host = {i: ctx.read_picture(a_s[i], a_o[i]) for i in probe}
    for at in range(0, n, 64):                                  # the device copy the torch route works on
        copy[at:at + 64] = torch.from_numpy(np.stack([ctx.read_picture(a_s[i], a_o[i]) for i in range(at, min(n, at + 64))])).cuda()
    ident = lambda: ctx.scale_pictures(a_s, a_o, (W, H), out=sout)
    timed(torch, ident, args.warmup)
    for label, w, tg in the_maps():
        out = torch.empty((n, scale.nbytes(*tg)), dtype=torch.uint8, device="cuda")
        call = lambda: ctx.warp_pictures(a_s, a_o, w, tg[:2], tg[2:], out=out)
        want = {i: wp.of_picture(host[i], SRC, w, tg) for i in probe}
        r = {"bodies_of_planes": [wp.body(w, SRC, tg, p) for p in (0, 1)], "target": list(tg), "scale_identity_ms": [], "torch_ms": []}
        agree = True
        for name, force in BODIES:
            ctx.warp_force_direct(force)
            timed(torch, call, args.warmup)
            got = out.cpu().numpy()
            agree = agree and all(np.array_equal(got[i], want[i]) for i in probe)
            r[name + "_ms"] = []
        route, off = optional_route(torch, lambda: torch_route(torch, copy, w, tg))     # a torch build without this sampler
        if route:
            off = int((route().to(torch.int16) - out.to(torch.int16)).abs().max())
        for _ in range(args.rounds):
            for name, force in BODIES:
                ctx.warp_force_direct(force)
                r[name + "_ms"].append(round(timed(torch, call, args.reps), 4))
            r["scale_identity_ms"].append(round(timed(torch, ident, args.reps), 4))
            if route:
                r["torch_ms"].append(round(timed(torch, route, max(1, args.reps // 10)), 4))
        ctx.warp_force_direct(0)
        for k in ("chosen", "direct", "tiled", "scale_identity", "torch"):
            r[k + "_median_ms"] = statistics.median(r[k + "_ms"]) if r[k + "_ms"] else None
        r["torch_over_chosen"] = round(r["torch_median_ms"] / r["chosen_median_ms"], 1) if route else None
        r["equal_host_module_under_every_body"] = bool(agree)
        r["torch_route_largest_difference"] = off
        res["maps"][label] = r
    ctx.close()
    print(json.dumps(res))


def child_trace(args):
    """the launches the trace is taken of, in this order: the spread block, per map and body 1 + reps of the warp kernel, the spread block
    again after the fourth map and at the end, then the scale kernel (identity)"""
    from hvqm4_amd import scale
    from hvqm4_amd import warp as wp
    torch, ctx, a_s, a_o = setup(args)
    n = len(a_s)
    out = torch.empty((n, scale.nbytes(W, H, 2, 2)), dtype=torch.uint8, device="cuda")

    def block(w, tg, force):
        ctx.warp_force_direct(force)
        o = out if tg == SRC else torch.empty((n, scale.nbytes(*tg)), dtype=torch.uint8, device="cuda")
        for _ in range(1 + args.reps):
            ctx.warp_pictures(a_s, a_o, w, tg[:2], tg[2:], out=o)
        torch.cuda.synchronize()
    block(wp.identity(), SRC, 1)
    for i, (_label, w, tg) in enumerate(the_maps()):
        for _name, force in BODIES:
            block(w, tg, force)
        if i == SPREAD_AFTER:
            block(wp.identity(), SRC, 1)
    block(wp.identity(), SRC, 1)
    ctx.warp_force_direct(0)
    for _ in range(1 + args.reps):
        ctx.scale_pictures(a_s, a_o, (W, H), out=out)
    torch.cuda.synchronize()
    ctx.close()
    print(json.dumps({"launches": 1 + args.reps, "pictures": n, "content": args.contents.split(",")[0]}))


def trace_summary(trace_dir, plan, _earlier=None):
    from hvqm4_amd import warp as wp
    maps = the_maps()
    blocks = ["spread0"]
    for i, (label, _w, _tg) in enumerate(maps):
        blocks += [f"{label}/{name}" for name, _f in BODIES] + (["spread1"] if i == SPREAD_AFTER else [])
    cut = read_planned(trace_dir, [(b, "hvq_warp_kernel", plan["launches"]) for b in blocks + ["spread2"]] +
                       [("hvq_scale_kernel_identity", "hvq_scale_kernel", plan["launches"])])
    if "error" in cut:
        return cut
    stats = lambda b: launch_stats(l.ns for l in cut[b][1:])                          # without the warm-up launch
    res = {"pictures": plan["pictures"], "content": plan["content"], **resources(cut["spread0"][0]), "maps": {}}
    spread_blocks = [stats("spread0"), stats("spread1"), stats("spread2")]
    med = [b["median_us"] for b in spread_blocks]
    res["spread"] = {"configuration": "identity, direct body", "blocks": spread_blocks, "spread_us": round(max(med) - min(med), 1)}
    res["hvq_scale_kernel_identity"] = stats("hvq_scale_kernel_identity")
    ok = True
    for label, w, tg in maps:
        m = {name: stats(f"{label}/{name}") for name, _f in BODIES}
        m["bodies_of_planes"] = [wp.body(w, SRC, tg, p) for p in (0, 1)]
        m["chosen_no_slower_than_direct_plus_spread"] = m["chosen"]["median_us"] <= m["direct"]["median_us"] + res["spread"]["spread_us"]
        m["tiled_minus_direct_us"] = round(m["tiled"]["median_us"] - m["direct"]["median_us"], 1)
        ok = ok and m["chosen_no_slower_than_direct_plus_spread"]
        res["maps"][label] = m
    res["rule_agrees"] = ok
    return res


def main():
    ap = argparse.ArgumentParser()
    add_common_arguments(ap, children=("calls", "trace"), reps=20, warmup=3, rounds=5, steps="calls,trace", out_dir="warp_bench_out", out="--out")
    ap.add_argument("--contents", default="natural")
    args = ap.parse_args()
    if args.child:
        return {"calls": child_calls, "trace": child_trace}[args.child](args)
    drive(args, {"calls": ("calls", None), "trace": ("trace", trace_summary)}, [sys.executable, os.path.abspath(__file__)])


if __name__ == "__main__":
    main()
