"""Summed-area tables of pictures in slot layout (hvq_integral_pictures, hvq_window_pictures, hvq_rect_sums, Context.adaptive_pictures) on
the GPU.

Two measurements (steps of tools/benchlib.py), both on 128 640x480 4:2:0 streams with 8 resident pictures each, 1024 pictures a call, of
the synthetic clip `natural`.
  calls   time per call, HIP-event timed on one stream in alternating rounds after a warm-up, medians over the rounds, of
          integral_pictures (sums alone; sums and squares), of window_pictures under MEAN at the radii 2, 15 and 100, under THRESHOLD at
          radius 25 with k = 0 and with k = 51, of adaptive_pictures(adaptive(25, c=7)), of rect_sums on 65 536 rectangles, of
          filter_pictures with the Gaussian of radius 15 and of scale_pictures to the pictures' own geometry (the identity kernel).  The
          host route of the same session: read_pictures of the 1024 pictures, then scipy.ndimage.uniform_filter (size 51, mode
          "constant", of the plane and of a plane of ones: the mean over the cut window) and the compare a > mean - 7 on 16 host threads
          (where scipy is missing the line says so and there is no host route).  The results of the calls must equal hvqm4_amd.integral on
          probes read back.
  trace   the kernel trace of a child that makes the same calls in a fixed order, one warm-up and `reps` calls each.  Kernel times per
          launch are read from the trace: median with min-max, registers, LDS and scratch per kernel, and the integral launches as
          multiples of their yardstick: the scale identity kernel scaled by bytes moved (sums alone: the row pass reads 1 and writes 4,
          the column pass reads 4 and writes 4 bytes a luma sample, 13; with squares 8 + 8 + 8 more, 39; the identity moves 1.5 in and
          1.5 out a luma sample).
Condition 1 -- adaptive_pictures(adaptive(25, c=7)) per call is faster than the host route of the same session -- is in the calls step;
condition 2 -- the two integral kernels (sums alone) plus the window kernel under MEAN at radius 15 take less kernel time than the filter
kernel under the Gaussian of radius 15 -- in the trace step.
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
RADIUS, C = 25, 7
NRECTS = 65536
INTEGRAL_KERNELS = ("hvq_integral_row_kernel", "hvq_integral_column_kernel")
WINDOW_KERNEL = "hvq_window_kernel"
RECT_KERNEL = "hvq_rect_kernel"
FILTER_KERNEL = "hvq_filter_kernel"
WINDOW_ROWS = ("mean_2", "mean_15", "mean_100", "threshold_k0", "threshold_k51")
SUMS_BYTES, BOTH_BYTES, IDENTITY_BYTES = 13.0, 39.0, 3.0          # per luma sample


def trace_plan(reps):
    """(label, kernel, count) of the trace step's launches in their order"""
    plan = [("scale_identity", "hvq_scale_kernel", 1 + reps), ("gauss15", FILTER_KERNEL, 1 + reps)]
    for label in ("integral_sums", "integral_both"):
        for r in range(1 + reps):
            plan += [(f"{label}/{r}/{k}", k, 1) for k in INTEGRAL_KERNELS]
    plan += [(label, WINDOW_KERNEL, 1 + reps) for label in WINDOW_ROWS]
    plan.append(("rects", RECT_KERNEL, 1 + reps))
    return plan


def setup(args):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch, filters, integral
    ctx = batch.Context(0)
    S = {"torch": torch, "ctx": ctx}
    a_s, a_o = picture_lists(resident(ctx, preset="natural", streams=args.streams, per=args.per, distinct=args.distinct), args.per)
    n = len(a_s)
    S["lists"], S["n"] = (a_s, a_o), n
    S["sums"] = torch.empty((n, H, W), dtype=torch.int32, device="cuda")                     # 1.26 GB for 1024 pictures
    S["squares"] = torch.empty((n, H, W), dtype=torch.int64, device="cuda")                  # 2.5 GB
    S["out"] = torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
    S["rules"] = {"mean_2": integral.mean(2), "mean_15": integral.mean(15), "mean_100": integral.mean(100), "threshold_k0": integral.adaptive(RADIUS, c=C),
                  "threshold_k51": integral.adaptive(RADIUS, c=C, k=51)}
    S["adaptive"] = integral.adaptive(RADIUS, c=C)
    S["gauss"] = filters.gaussian(5.0, 15)
    g = torch.Generator(device="cpu").manual_seed(3)
    x0 = torch.randint(0, W, (NRECTS,), generator=g); y0 = torch.randint(0, H, (NRECTS,), generator=g)
    x1 = torch.minimum(x0 + torch.randint(0, 200, (NRECTS,), generator=g), torch.tensor(W - 1)); y1 = torch.minimum(y0 + torch.randint(0, 200, (NRECTS,), generator=g), torch.tensor(H - 1))
    S["rects"] = torch.stack([torch.randint(0, n, (NRECTS,), generator=g), x0, y0, x1, y1], dim=1).to(torch.int32).cuda()
    S["dims"] = torch.tensor([[W, H]] * n, dtype=torch.int32).cuda()
    S["rect_out"] = torch.empty((NRECTS, 3), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return S


def the_calls(S):
    ctx, n = S["ctx"], S["n"]
    a_s, a_o = S["lists"]
    sums, squares = [S["sums"][i] for i in range(n)], [S["squares"][i] for i in range(n)]
    calls = {"scale_identity": lambda: ctx.scale_pictures(a_s, a_o, (W, H), out=S["out"]),
             "gauss15": lambda: ctx.filter_pictures(a_s, a_o, S["gauss"], out=S["out"]),
             "integral_sums": lambda: ctx.integral_pictures(a_s, a_o, 0, squares=False, out=(sums, None)),
             "integral_both": lambda: ctx.integral_pictures(a_s, a_o, 0, squares=True, out=(sums, squares))}
    for label in WINDOW_ROWS:
        calls[label] = lambda label=label: ctx.window_pictures(a_s, a_o, sums, squares, S["rules"][label], out=S["out"])
    calls["rects"] = lambda: ctx.rect_sums(S["rects"], sums, squares, dims=S["dims"], out=S["rect_out"])
    calls["adaptive"] = lambda: ctx.adaptive_pictures(a_s, a_o, S["adaptive"], out=S["out"])
    return calls


TRACED = ["scale_identity", "gauss15", "integral_sums", "integral_both"] + list(WINDOW_ROWS) + ["rects"]


def child_calls(args):
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
    from hvqm4_amd import integral
    S = setup(args)
    torch, ctx, n = S["torch"], S["ctx"], S["n"]
    a_s, a_o = S["lists"]
    calls = the_calls(S)
    res = {"size": f"{W}x{H}", "pictures": n, "reps": args.reps, "rounds": args.rounds, "table_bytes": {"sums": n * W * H * 4, "squares": n * W * H * 8}, "radius": RADIUS, "c": C,
           "rectangles": NRECTS, "rows": {}}
    probe = [0, n // 2]
    pics = ctx.read_pictures(a_s, a_o)
    host = [np.frombuffer(pics[i], dtype=np.uint8) if not isinstance(pics[i], np.ndarray) else pics[i].reshape(-1) for i in probe]
    checks = {}
    calls["integral_both"]()
    torch.cuda.synchronize()
    tabs = {i: integral.of_plane(h[:W * H].reshape(H, W)) for i, h in zip(probe, host)}
    checks["tables"] = bool(all(np.array_equal(S["sums"][i].cpu().numpy().view(np.uint32), tabs[i][0]) and np.array_equal(S["squares"][i].cpu().numpy().view(np.uint64), tabs[i][1])
                                for i in probe))
    for label in WINDOW_ROWS:
        calls[label]()
        torch.cuda.synchronize()
        checks[label] = bool(all(np.array_equal(S["out"][i].cpu().numpy(), integral.of_picture(h, SRC, S["rules"][label])) for i, h in zip(probe, host)))
    calls["adaptive"]()
    torch.cuda.synchronize()
    checks["adaptive"] = bool(all(np.array_equal(S["out"][i].cpu().numpy(), integral.of_picture(h, SRC, S["adaptive"])) for i, h in zip(probe, host)))
    calls["integral_both"](); calls["rects"]()
    torch.cuda.synchronize()
    rects = S["rects"].cpu().numpy()
    rows = np.flatnonzero(np.isin(rects[:, 0], probe))[:64]
    got = S["rect_out"].cpu().numpy().view(np.uint64)
    checks["rects"] = bool(all(tuple(int(v) for v in got[r]) == integral.rect(tabs[int(rects[r, 0])][0], tabs[int(rects[r, 0])][1], *[int(v) for v in rects[r, 1:]]) for r in rows))
    res["equal_host_module"] = checks
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
    res["mean_100_over_mean_2"] = round(med("mean_100") / med("mean_2"), 3)
    res["threshold_k51_over_k0"] = round(med("threshold_k51") / med("threshold_k0"), 3)
    try:
        from scipy import ndimage
    except ImportError:
        res["host_route"] = "scipy is not installed: no host route, condition 1 is not judged"
        ctx.close()
        print(json.dumps(res))
        return
    size = 2 * RADIUS + 1
    ones = ndimage.uniform_filter(np.ones((H, W), np.float64), size=size, mode="constant")

    def host_threshold(p):
        a = np.asarray(p).reshape(-1)[:W * H].reshape(H, W)
        mean = ndimage.uniform_filter(a.astype(np.float64), size=size, mode="constant") / ones
        return (a > mean - C).astype(np.uint8) * 255
    pool = ThreadPoolExecutor(16)
    route = []
    for _ in range(max(1, min(3, args.rounds))):
        t0 = time.perf_counter()
        got = ctx.read_pictures(a_s, a_o)
        t1 = time.perf_counter()
        masks = list(pool.map(host_threshold, [got[i] for i in range(n)]))
        t2 = time.perf_counter()
        route.append((round((t1 - t0) * 1e3, 2), round((t2 - t1) * 1e3, 2)))
    pool.shutdown()
    calls["adaptive"]()
    torch.cuda.synchronize()
    mine = S["out"][0].cpu().numpy()[:W * H].reshape(H, W)
    res["host_values_differ_share"] = round(float((masks[0] != mine).mean()), 6)      # the float route rounds at the boundary a == mean - c
    host_ms = statistics.median(a + b for a, b in route)
    res["host_route"] = {"filter": "scipy.ndimage.uniform_filter, size 51, mode constant, and a compare", "threads": 16, "read_pictures_ms, threshold_ms": route,
                         "median_ms": round(host_ms, 2)}
    res["condition_1"] = {"what": "adaptive_pictures(adaptive(25, c=7)) per call faster than read_pictures + scipy's uniform_filter + a compare on 16 threads, same session",
                          "adaptive_ms": med("adaptive"), "host_ms": round(host_ms, 2), "host_over_adaptive": round(host_ms / med("adaptive"), 1), "holds": med("adaptive") < host_ms}
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
    cut = read_planned(trace_dir, trace_plan(per - 1), kernels=set(INTEGRAL_KERNELS) | {"hvq_scale_kernel", FILTER_KERNEL, WINDOW_KERNEL, RECT_KERNEL})
    if "error" in cut:
        return cut
    res = {"pictures": plan["pictures"], "kernels": {k: resources(cut[f"integral_both/0/{k}"][0]) for k in INTEGRAL_KERNELS}}
    res["kernels"][WINDOW_KERNEL] = resources(cut["threshold_k51"][0])
    res["kernels"][RECT_KERNEL] = resources(cut["rects"][0])
    res["scale_identity"] = launch_stats(l.ns for l in cut["scale_identity"][1:])
    res["gauss15"] = launch_stats(l.ns for l in cut["gauss15"][1:])
    luma_share = res["scale_identity"]["median_us"] * (W * H) / PIC_BYTES           # the identity kernel's time for the luma samples alone
    per_byte = luma_share / (IDENTITY_BYTES * 2.0 / 3.0)                              # ... moves 2 bytes a luma sample: 1 in, 1 out
    res["yardstick_us"] = {"sums": round(per_byte * SUMS_BYTES, 1), "sums_and_squares": round(per_byte * BOTH_BYTES, 1)}
    for label, yard in (("integral_sums", "sums"), ("integral_both", "sums_and_squares")):
        row = {k: launch_stats(cut[f"{label}/{r}/{k}"][0].ns for r in range(1, per)) for k in INTEGRAL_KERNELS}          # without the warm-up call
        row["sum_median_us"] = round(sum(row[k]["median_us"] for k in INTEGRAL_KERNELS), 1)
        row["over_yardstick"] = round(row["sum_median_us"] / res["yardstick_us"][yard], 2)
        res[label] = row
    for label in WINDOW_ROWS + ("rects",):
        res[label] = launch_stats(l.ns for l in cut[label][1:])
    res["mean_100_over_mean_2"] = round(res["mean_100"]["median_us"] / res["mean_2"]["median_us"], 3)
    res["threshold_k51_over_k0"] = round(res["threshold_k51"]["median_us"] / res["threshold_k0"]["median_us"], 3)
    both = round(res["integral_sums"]["sum_median_us"] + res["mean_15"]["median_us"], 1)
    res["condition_2"] = {"what": "the integral kernels (sums alone) plus the window kernel under MEAN at radius 15 < the filter kernel under the Gaussian of radius 15, same session",
                          "integral_plus_mean15_us": both, "gauss15_us": res["gauss15"]["median_us"], "holds": both < res["gauss15"]["median_us"]}
    return res


def main():
    ap = argparse.ArgumentParser()
    add_common_arguments(ap, children=("calls", "trace"), reps=5, warmup=2, rounds=5, steps="calls,trace", out_dir="integral_bench_out", out="--out")
    args = ap.parse_args()
    if args.child:
        return {"calls": child_calls, "trace": child_trace}[args.child](args)
    drive(args, {"calls": ("calls", None), "trace": ("trace", trace_summary)}, [sys.executable, os.path.abspath(__file__)])


if __name__ == "__main__":
    main()
