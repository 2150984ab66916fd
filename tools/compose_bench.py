"""Composed pictures in slot layout (hvq_compose_pictures) on the GPU: what the kernel costs against the memory it moves and against torch.

Two measurements (steps of tools/benchlib.py):
  calls   128 640x480 4:2:0 streams, 8 resident pictures each, 1024 pictures, on natural content.  The cases: a copy of every picture; the
          cross-fade of every picture with its neighbour; the average of 8 neighbours; the difference of two; a translucent 160x120
          inset at an odd chroma offset (the general body); 64 sheets of 4 x 4 cells of 160x120 from 1024 thumbnails (scale_pictures
          first, not timed); the copy and the cross-fade again with every layer through the general body.  Per case: (a)
          compose_pictures, (b) the yardstick: scale_pictures to the pictures' own geometry on the same pictures, which reads and
          writes each picture once, (c) a torch route on a device copy of the same pictures in planar YUV: slices per plane, int32
          tensor arithmetic, clamp, cast, concatenation.  HIP-event timed per call on one stream in alternating rounds after a
          warm-up; medians over the rounds.  (a) must equal hvqm4_amd.compose on targets read back.
  trace   the kernel trace of a child that launches every case and the yardstick in a fixed order, one warm-up and
          `reps` launches each.  Kernel times are read from the trace: median with min-max per case, and per case the multiple of
          `bytes ratio x yardstick` it takes (bytes ratio: the bytes the case reads and writes over the yardstick's).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.benchlib import (add_common_arguments, cut_by_plan, drive, launch_stats, picture_lists, read_kernel_trace, resident, resources,  # noqa: E402
                            timed)

W, H = 640, 480
SRC = (W, H, 2, 2)
CELL = (160, 120)
INSET_AT = (6, 10)                                   # chroma (3, 5): odd in both axes
# (label, force_general, bytes the case moves in units of one picture read or written once, per 1024 pictures: the yardstick moves 2048)
CASES = (("copy", 0, 2048), ("crossfade2", 0, 3072), ("average8", 0, 9216), ("difference", 0, 3072), ("overlay_inset", 0, 2048 + 2 * 64), ("mosaic4x4", 0, 128),
         ("copy_general", 1, 2048), ("crossfade2_general", 1, 3072))


def case_targets(label, n):
    """(targets, the call's pictures are the thumbnails) of a case over pictures 0 .. n - 1"""
    from hvqm4_amd import compose as cp
    nb = lambda i, k: (i + k) % n
    base = label.replace("_general", "")
    if base == "copy":
        return [cp.copy(SRC, i) for i in range(n)], False
    if base == "crossfade2":
        return [cp.crossfade(SRC, 0.3, a=i, b=nb(i, 1)) for i in range(n)], False
    if base == "average8":
        w = cp.average_weights(8)
        return [cp.Target((W, H), (2, 2), tuple(cp.Layer(nb(i, k), cp.ADD, w[k]) for k in range(8)), 16) for i in range(n)], False
    if base == "difference":
        return [cp.difference(SRC, 1, i, nb(i, 1)) for i in range(n)], False
    if base == "overlay_inset":
        return [cp.overlay(SRC, INSET_AT[0], INSET_AT[1], CELL, 128, base=i, top=nb(i, 1)) for i in range(n)], False
    if base == "mosaic4x4":
        return [cp.mosaic(4, 4, CELL, (2, 2), sources=range(16 * s, 16 * s + 16)) for s in range(n // 16)], True
    raise ValueError(label)


def planes_of(t, g):
    """the Y, U, V views [n, rows, columns] of a tensor [n, bytes] of pictures of geometry g"""
    w, h, hs, vs = g
    y, c = w * h, (w // hs) * (h // vs)
    return [t[:, :y].view(-1, h, w), t[:, y:y + c].view(-1, h // vs, w // hs), t[:, y + c:].view(-1, h // vs, w // hs)]


def torch_route(torch, label, copy, thumbs):
    """the composed pictures the way a pipeline without the call gets them"""
    from hvqm4_amd import compose as cp
    base = label.replace("_general", "")
    nxt = lambda k: torch.roll(copy, -k, 0)
    fin = lambda acc, shift, bias=0: (((acc + ((1 << (shift - 1)) if shift else 0)) >> shift) + bias).clamp_(0, 255).to(torch.uint8)
    if base == "copy":
        return copy.clone()
    if base == "crossfade2":
        k = cp.crossfade(SRC, 0.3).layers[1].weights()[0]
        return fin(copy.to(torch.int32) * (256 - k) + nxt(1).to(torch.int32) * k, 8)
    if base == "average8":
        w = cp.average_weights(8)
        acc = copy.to(torch.int32) * w[0]
        for k in range(1, 8):
            acc += nxt(k).to(torch.int32) * w[k]
        return fin(acc, 16)
    if base == "difference":
        return fin(copy.to(torch.int32) - nxt(1).to(torch.int32), 0, 128)
    if base == "overlay_inset":
        out = copy.clone()
        for p, (a, b) in enumerate(zip(planes_of(out, SRC), planes_of(nxt(1), SRC))):
            d = 2 if p else 1
            x, y, w, h = INSET_AT[0] // d, INSET_AT[1] // d, CELL[0] // d, CELL[1] // d
            a[:, y:y + h, x:x + w] = fin(a[:, y:y + h, x:x + w].to(torch.int32) * 128 + b[:, :h, :w].to(torch.int32) * 128, 8)
        return out
    if base == "mosaic4x4":
        out = []
        for pl in planes_of(thumbs, CELL + (2, 2)):
            n, h, w = pl.shape
            out.append(pl.view(n // 16, 4, 4, h, w).permute(0, 1, 3, 2, 4).reshape(n // 16, -1))
        return torch.cat(out, dim=1)
    raise ValueError(label)


def setup(args):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    a_s, a_o = picture_lists(resident(ctx, preset=args.contents.split(",")[0], streams=args.streams, per=args.per, distinct=args.distinct), args.per)
    n = len(a_s)
    thumbs = ctx.scale_pictures(a_s, a_o, CELL)
    cell_sid = ctx.open_stream(CELL[0], CELL[1], 2, 2, True, 3)          # never submitted to: it names the geometry of the thumbnails
    calls = {}
    for label, force, _b in CASES:
        targets, small = case_targets(label, n)
        out = torch.empty((len(targets), W * H * 3 // 2), dtype=torch.uint8, device="cuda")
        if small:
            rows = [thumbs[i] for i in range(n)]
            calls[label] = (lambda t=targets, o=out, r=rows: ctx.compose_pictures([cell_sid] * n, [-1] * n, t, src=r, out=o), out, targets, force)
        else:
            calls[label] = (lambda t=targets, o=out: ctx.compose_pictures(a_s, a_o, t, out=o), out, targets, force)
    return torch, ctx, a_s, a_o, thumbs, calls


def child_calls(args):
    import numpy as np
    from hvqm4_amd import compose as cp
    torch, ctx, a_s, a_o, thumbs, calls = setup(args)
    n = len(a_s)
    pb = W * H * 3 // 2
    res = {"size": f"{W}x{H}", "pictures": n, "reps": args.reps, "rounds": args.rounds, "content": args.contents.split(",")[0], "cases": {}}
    copy = torch.empty((n, pb), dtype=torch.uint8, device="cuda")
    for at in range(0, n, 64):                                  # the device copy the torch route works on
        copy[at:at + 64] = torch.from_numpy(np.stack([ctx.read_picture(a_s[i], a_o[i]) for i in range(at, min(n, at + 64))])).cuda()
    sout = torch.empty((n, pb), dtype=torch.uint8, device="cuda")
    ident = lambda: ctx.scale_pictures(a_s, a_o, (W, H), out=sout)
    timed(torch, ident, args.warmup)
    host_thumbs = None
    for label, _force, units in CASES:
        call, out, targets, force = calls[label]
        route = lambda: torch_route(torch, label, copy, thumbs)
        ctx.compose_force_general(force)
        timed(torch, call, args.warmup)
        got = out.cpu().numpy()
        probe = list(range(0, len(targets), max(1, len(targets) // 4)))
        agree = True
        for i in probe:
            used = sorted({l.source for l in targets[i].layers})
            if label.startswith("mosaic"):
                host_thumbs = thumbs.cpu().numpy() if host_thumbs is None else host_thumbs
                pics, geoms = {j: host_thumbs[j] for j in used}, [CELL + (2, 2)] * n
            else:
                pics, geoms = {j: ctx.read_picture(a_s[j], a_o[j]) for j in used}, [SRC] * n
            agree = agree and np.array_equal(got[i], cp.of_pictures([pics.get(j, b"") for j in range(n)], geoms, targets[i]))
        timed(torch, route, 1)
        r = {"targets": len(targets), "layers": sum(len(t.layers) for t in targets), "force_general": force, "bytes_ratio": round(units / 2048, 4),
             "compose_ms": [], "scale_identity_ms": [], "torch_ms": []}
        r["torch_route_largest_difference"] = int((route().to(torch.int16) - out.to(torch.int16)).abs().max())
        for _ in range(args.rounds):
            r["compose_ms"].append(round(timed(torch, call, args.reps), 4))
            r["scale_identity_ms"].append(round(timed(torch, ident, args.reps), 4))
            r["torch_ms"].append(round(timed(torch, route, max(1, args.reps // 5)), 4))
        for k in ("compose", "scale_identity", "torch"):
            r[k + "_median_ms"] = statistics.median(r[k + "_ms"])
        r["torch_over_compose_call"] = round(r["torch_median_ms"] / r["compose_median_ms"], 2)
        r["equal_host_module"] = bool(agree)
        res["cases"][label] = r
    ctx.compose_force_general(0)
    ctx.close()
    print(json.dumps(res))


def child_trace(args):
    """the launches the trace is taken of, in this order: per case 1 + reps of the compose kernel, then the scale kernel (identity)"""
    torch, ctx, a_s, a_o, _thumbs, calls = setup(args)
    torch.cuda.synchronize()
    for label, _f, _u in CASES:
        call, _out, _t, force = calls[label]
        ctx.compose_force_general(force)
        for _ in range(1 + args.reps):
            call()
        torch.cuda.synchronize()
    ctx.compose_force_general(0)
    out = torch.empty((len(a_s), W * H * 3 // 2), dtype=torch.uint8, device="cuda")
    for _ in range(1 + args.reps):
        ctx.scale_pictures(a_s, a_o, (W, H), out=out)
    torch.cuda.synchronize()
    ctx.close()
    print(json.dumps({"launches": 1 + args.reps, "pictures": len(a_s), "content": args.contents.split(",")[0]}))


def trace_summary(trace_dir, plan, earlier=None):
    calls = (earlier or {}).get("calls")
    per = plan["launches"]
    launches = read_kernel_trace(trace_dir, ("hvq_compose_kernel", "hvq_scale_kernel"))
    if isinstance(launches, dict):
        return launches
    blocks = [(label, "hvq_compose_kernel", per) for label, _f, _u in CASES] + [("hvq_scale_kernel_identity", "hvq_scale_kernel", per)]
    thumbnails = max(0, len(launches) - per * len(blocks))                            # the scale launches of the set-up come first
    cut = cut_by_plan(launches, [("set-up", "hvq_scale_kernel", thumbnails)] + blocks)
    if "error" in cut:
        return cut
    stats = lambda r: launch_stats(l.ns for l in r[1:])                               # without the warm-up launch
    res = {"pictures": plan["pictures"], "content": plan["content"], **resources(cut[CASES[0][0]][0]), "cases": {}}
    yard = stats(cut["hvq_scale_kernel_identity"])
    res["hvq_scale_kernel_identity"] = yard
    for label, force, units in CASES:
        m = stats(cut[label])
        m["force_general"] = force
        m["bytes_ratio"] = round(units / 2048, 4)
        m["multiple_of_bytes_ratio_x_yardstick"] = round(m["median_us"] / (units / 2048 * yard["median_us"]), 2)
        if calls and label in calls.get("cases", {}):
            m["torch_ms_over_kernel_ms"] = round(calls["cases"][label]["torch_median_ms"] * 1e3 / m["median_us"], 1)
        res["cases"][label] = m
    return res


def main():
    ap = argparse.ArgumentParser()
    add_common_arguments(ap, children=("calls", "trace"), reps=10, warmup=2, rounds=3, steps="calls,trace", out_dir="compose_bench_out", out="--out")
    ap.add_argument("--contents", default="natural")
    args = ap.parse_args()
    if args.child:
        return {"calls": child_calls, "trace": child_trace}[args.child](args)
    drive(args, {"calls": ("calls", None), "trace": ("trace", trace_summary)}, [sys.executable, os.path.abspath(__file__)])


if __name__ == "__main__":
    main()
