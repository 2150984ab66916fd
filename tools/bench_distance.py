"""Exact distance transforms of pictures in slot layout (hvq_distance_pictures, hvq_distance_mask, Context.disc_morph) on the GPU.

Two measurements (steps of tools/benchlib.py), both on 128 640x480 4:2:0 streams with 8 resident pictures each, 1024 pictures a call,
whose luma is binarised in the same process by Otsu tables (Context.equalize_pictures) and transformed through src=.  The presets: the
synthetic clips `natural` (under each metric) and `dense`, an all-background plane, a full plane under border = 1, and the worst case of
the outward search: a full plane whose only background sample is (0, 0).
  calls   time per call, HIP-event timed on one stream in alternating rounds after a warm-up, medians over the rounds, of
          distance_pictures per preset, of distance_mask in both modes, of disc_morph(opening_disc(5)), of the rectangular
          morph_pictures(opening(5)) and of scale_pictures to the pictures' own geometry (the identity kernel).  The host route of the same
          session: read_pictures of the 1024 pictures, then scipy.ndimage.distance_transform_edt of the 1024 luma masks on 16 host threads
          (where scipy is missing the line says so and there is no host route).  The results of the calls must equal hvqm4_amd.distance on
          probes read back.
  trace   the kernel trace of a child that makes the same calls in a fixed order, one warm-up and `reps` calls each.  Kernel times per
          launch are read from the trace: median with min-max, registers, LDS and scratch per kernel, and the two passes as multiples of
          their yardstick: the scale identity kernel scaled by bytes moved (the column pass reads 1 and 4 and writes 4 + 4 bytes a luma
          sample, the row pass reads 4 and writes 4; the identity moves 1.5 in and 1.5 out a luma sample).
The one condition -- distance_pictures (EUCLID2) per call on the natural preset is faster than the host route of the same session -- is
in the calls step.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.benchlib import (add_common_arguments, drive, launch_stats, picture_lists, read_planned, resident, resources, timed)  # noqa: E402

W, H = 640, 480
SRC = (W, H, 2, 2)
PIC_BYTES = W * H * 3 // 2
RADIUS = 5
# preset -> (the masks it reads, metric, border)
PRESETS = {"natural": ("natural", 0, 0), "natural_city": ("natural", 1, 0), "natural_chess": ("natural", 2, 0), "dense": ("dense", 0, 0), "background": ("background", 0, 0),
           "full_border": ("full", 0, 1), "far": ("far", 0, 0)}
DISTANCE_KERNELS = ("hvq_distance_column_kernel", "hvq_distance_row_kernel")
MASK_KERNEL = "hvq_distance_mask_kernel"
COLUMN_BYTES, ROW_BYTES, IDENTITY_BYTES = 13.0, 8.0, 3.0           # per luma sample


def trace_plan(reps):
    """(label, kernel, count) of the trace step's launches in their order"""
    plan = [("scale_identity", "hvq_scale_kernel", 1 + reps)]
    for p in PRESETS:
        for r in range(1 + reps):
            plan += [(f"{p}/{r}/{k}", k, 1) for k in DISTANCE_KERNELS]
    plan += [("mask_range", MASK_KERNEL, 1 + reps), ("mask_root", MASK_KERNEL, 1 + reps), ("select", "hvq_select_kernel", 1 + reps)]
    return plan


def setup(args):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch, distance, labels, maps, rank
    ctx = batch.Context(0)
    otsu = maps.Rule(maps.otsu().luma, maps.flat(128).luma)
    S = {"torch": torch, "ctx": ctx, "masks": {}, "lists": {}}
    for p in ("natural", "dense"):
        a_s, a_o = picture_lists(resident(ctx, preset=p, streams=args.streams, per=args.per, distinct=args.distinct), args.per)
        S["lists"][p] = (a_s, a_o)
        S["masks"][p] = ctx.equalize_pictures(a_s, a_o, otsu)
    n = len(S["lists"]["natural"][0])
    S["masks"]["background"] = torch.zeros((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
    S["masks"]["full"] = torch.full((n, PIC_BYTES), 255, dtype=torch.uint8, device="cuda")
    S["masks"]["far"] = torch.full((n, PIC_BYTES), 255, dtype=torch.uint8, device="cuda")
    S["masks"]["far"][:, 0] = 0
    S["n"] = n
    S["dist"] = torch.empty((n, H, W), dtype=torch.int32, device="cuda")                     # 1.26 GB for 1024 pictures
    S["labels"] = torch.zeros((n, H, W), dtype=torch.int32, device="cuda")                   # the select kernel's input: the yardstick of the mask call
    S["comps"] = torch.zeros((n, 2, 8), dtype=torch.int64, device="cuda")
    S["out"] = torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
    S["rule"] = {p: distance.Rule(0, 255, 255, m, b) for p, (_m, m, b) in PRESETS.items()}
    S["range"], S["root"] = distance.mask_range(RADIUS * RADIUS + 1), distance.mask_root()
    S["discs"] = distance.opening_disc(RADIUS)
    S["rects"] = [rank.luma_only(s) for s in rank.opening(RADIUS)]
    S["select"] = labels.select(area=50)
    torch.cuda.synchronize()
    return S


def the_calls(S):
    ctx, n = S["ctx"], S["n"]
    a_s = S["lists"]["natural"][0]
    dist = [S["dist"][i] for i in range(n)]
    labs, comps = [S["labels"][i] for i in range(n)], [S["comps"][i] for i in range(n)]
    natural = [S["masks"]["natural"][i] for i in range(n)]
    calls = {"scale_identity": lambda: ctx.scale_pictures(*S["lists"]["natural"], (W, H), out=S["out"])}
    for p, (m, _metric, _b) in PRESETS.items():
        rows = [S["masks"][m][i] for i in range(n)]
        calls["distance_" + p] = lambda rows=rows, p=p: ctx.distance_pictures(a_s, [-1] * n, S["rule"][p], src=rows, out=dist)
    calls["mask_range"] = lambda: ctx.distance_mask(a_s, dist, S["range"], out=S["out"])
    calls["mask_root"] = lambda: ctx.distance_mask(a_s, dist, S["root"], out=S["out"])
    calls["select"] = lambda: ctx.select_components(a_s, labs, comps, S["select"], out=S["out"])
    calls["disc_opening"] = lambda: ctx.disc_morph(a_s, [-1] * n, S["discs"], src=natural, out=S["out"])
    calls["rect_opening"] = lambda: ctx.morph_pictures(a_s, [-1] * n, S["rects"], src=natural, out=S["out"])
    return calls


TRACED = ["scale_identity"] + ["distance_" + p for p in PRESETS] + ["mask_range", "mask_root", "select"]


def child_calls(args):
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
    from hvqm4_amd import distance
    S = setup(args)
    torch, ctx, n = S["torch"], S["ctx"], S["n"]
    calls = the_calls(S)
    res = {"size": f"{W}x{H}", "pictures": n, "reps": args.reps, "rounds": args.rounds, "map_bytes": n * W * H * 4, "radius": RADIUS, "rows": {}}
    probe = [0, n // 2]
    checks, facts = {}, {}
    for p, (m, _metric, _b) in PRESETS.items():
        if p == "far":
            continue                                                 # the host module's dense product takes minutes on it; the GPU test holds that case
        calls["distance_" + p](); calls["mask_range"]()
        torch.cuda.synchronize()
        ok = True
        for i in probe:
            want = distance.of_picture(S["masks"][m][i].cpu().numpy(), SRC, S["rule"][p])
            ok = ok and np.array_equal(S["dist"][i].cpu().numpy().view(np.uint32), want)
            ok = ok and np.array_equal(S["out"][i].cpu().numpy(), distance.of_mask(want, S["range"], SRC))
        checks[p] = bool(ok)
        d = S["dist"].view(n, -1)
        facts[p] = {"foreground_share": round(float((d != 0).float().mean()), 4), "max_distance_median": float(d.max(dim=1).values.float().median())}
    calls["disc_opening"]()
    torch.cuda.synchronize()
    checks["disc_opening"] = bool(all(np.array_equal(S["out"][i].cpu().numpy(), distance.of_steps(S["masks"]["natural"][i].cpu().numpy(), SRC, S["discs"])) for i in probe[:1]))
    res["equal_host_module"], res["maps"] = checks, facts
    labels_ = list(calls)
    for label in labels_:
        timed(torch, calls[label], args.warmup)
    ms = {label: [] for label in labels_}
    for _ in range(args.rounds):
        for label in labels_:
            ms[label].append(round(timed(torch, calls[label], args.reps), 4))
    for label, v in ms.items():
        res["rows"][label] = {"ms": v, "median_ms": statistics.median(v)}
    med = lambda label: res["rows"][label]["median_ms"]
    res["disc_over_rect_opening"] = round(med("disc_opening") / med("rect_opening"), 2)
    res["far_over_natural"] = round(med("distance_far") / med("distance_natural"), 1)
    # the host route on the natural preset: the read-back, then the masks through scipy on 16 threads
    try:
        from scipy import ndimage
    except ImportError:
        res["host_route"] = "scipy is not installed: no host route, the condition is not judged"
        ctx.close()
        print(json.dumps(res))
        return
    a_s, a_o = S["lists"]["natural"]
    masks = S["masks"]["natural"].cpu().numpy()[:, :W * H].reshape(n, H, W)
    pool = ThreadPoolExecutor(16)
    host = []
    for _ in range(max(1, min(3, args.rounds))):
        t0 = time.perf_counter()
        ctx.read_pictures(a_s, a_o)
        t1 = time.perf_counter()
        edt = list(pool.map(lambda m: ndimage.distance_transform_edt(m == 255), masks[:n]))
        t2 = time.perf_counter()
        host.append((round((t1 - t0) * 1e3, 2), round((t2 - t1) * 1e3, 2)))
    pool.shutdown()
    calls["distance_natural"]()
    torch.cuda.synchronize()
    got = S["dist"][0].cpu().numpy().view(np.uint32)
    has_bg = bool((masks[0] != 255).any())
    res["host_values_equal"] = bool(np.array_equal(np.rint(edt[0] ** 2).astype(np.int64), got.astype(np.int64))) if has_bg else None
    host_ms = statistics.median(a + b for a, b in host)
    res["host_route"] = {"transform": "scipy.ndimage.distance_transform_edt", "threads": 16, "read_pictures_ms, edt_ms": host, "median_ms": round(host_ms, 2)}
    res["condition"] = {"what": "distance_pictures (EUCLID2) per call on the natural preset faster than read_pictures + scipy's EDT on 16 threads, same session",
                        "distance_ms": med("distance_natural"), "host_ms": round(host_ms, 2), "host_over_distance": round(host_ms / med("distance_natural"), 1),
                        "holds": med("distance_natural") < host_ms}
    ctx.close()
    print(json.dumps(res))


def child_trace(args):
    """the launches the trace is taken of, in trace_plan's order"""
    S = setup(args)
    calls = the_calls(S)
    sync = S["torch"].cuda.synchronize
    for label in TRACED:
        for _ in range(1 + args.reps):
            calls[label]()
        sync()
    S["ctx"].close()
    print(json.dumps({"launches": 1 + args.reps, "pictures": S["n"]}))


def trace_summary(trace_dir, plan, _earlier=None):
    per = plan["launches"]
    cut = read_planned(trace_dir, trace_plan(per - 1), kernels=set(DISTANCE_KERNELS) | {"hvq_scale_kernel", "hvq_select_kernel", MASK_KERNEL})
    if "error" in cut:
        return cut
    res = {"pictures": plan["pictures"], "kernels": {k: resources(cut[f"natural/0/{k}"][0]) for k in DISTANCE_KERNELS}}
    res["kernels"][MASK_KERNEL] = resources(cut["mask_range"][0])
    res["scale_identity"] = launch_stats(l.ns for l in cut["scale_identity"][1:])
    luma_share = res["scale_identity"]["median_us"] * (W * H) / PIC_BYTES           # the identity kernel's time for the luma samples alone
    per_byte = luma_share / (IDENTITY_BYTES * 2.0 / 3.0)                              # ... moves 2 bytes a luma sample: 1 in, 1 out
    res["yardstick_us"] = {"column": round(per_byte * COLUMN_BYTES, 1), "row": round(per_byte * ROW_BYTES, 1)}
    for p in PRESETS:
        row = {k: launch_stats(cut[f"{p}/{r}/{k}"][0].ns for r in range(1, per)) for k in DISTANCE_KERNELS}          # without the warm-up call
        row["sum_median_us"] = round(sum(row[k]["median_us"] for k in DISTANCE_KERNELS), 1)
        row["column_over_yardstick"] = round(row[DISTANCE_KERNELS[0]]["median_us"] / res["yardstick_us"]["column"], 2)
        row["row_over_yardstick"] = round(row[DISTANCE_KERNELS[1]]["median_us"] / res["yardstick_us"]["row"], 2)
        res[p] = row
    res["mask_range"] = launch_stats(l.ns for l in cut["mask_range"][1:])
    res["mask_root"] = launch_stats(l.ns for l in cut["mask_root"][1:])
    res["select"] = launch_stats(l.ns for l in cut["select"][1:])
    res["mask_range_over_select"] = round(res["mask_range"]["median_us"] / res["select"]["median_us"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    add_common_arguments(ap, children=("calls", "trace"), reps=5, warmup=2, rounds=5, steps="calls,trace", out_dir="distance_bench_out", out="--out")
    args = ap.parse_args()
    if args.child:
        return {"calls": child_calls, "trace": child_trace}[args.child](args)
    drive(args, {"calls": ("calls", None), "trace": ("trace", trace_summary)}, [sys.executable, os.path.abspath(__file__)])


if __name__ == "__main__":
    main()
