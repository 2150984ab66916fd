"""Connected components of pictures in slot layout (hvq_label_pictures, hvq_select_components) on the GPU.

Two measurements (steps of tools/benchlib.py), both on 128 640x480 4:2:0 streams with 8 resident pictures each, 1024 pictures a call,
whose luma is binarised in the same process by Otsu tables (Context.equalize_pictures) and labelled through src=.  The presets: the
synthetic clips `natural` and `dense`, a 0 / 255 checkerboard (the most components a plane can have under the 4-neighbourhood) and a
full plane (one component, the longest parent chains).
  calls   time per call, HIP-event timed on one stream in alternating rounds after a warm-up, medians over the rounds, of
          label_pictures and select_components per preset, and of scale_pictures to the pictures' own geometry (the identity kernel, 2
          bytes a sample).  The host route of the same session: read_pictures of the 1024 pictures, then scipy.ndimage.label and
          find_objects of the 1024 luma masks on 16 host threads (hvqm4_amd.labels.of_plane where scipy is missing; the line says which).
          The results of the calls must equal hvqm4_amd.labels on probes read back.
  trace   the kernel trace of a child that makes the same calls in a fixed order, one warm-up and `reps` calls each.  Kernel times per
          launch of a label call are read from the trace: median with min-max, registers, LDS and scratch per kernel, their sum, and that
          sum as a multiple of 2.5 x the luma share of the scale identity kernel (a label call reads 1 byte and writes 4 a luma sample at
          the least, the identity moves 2).
The one condition -- label_pictures per call on the natural preset is faster than the host route of the same session -- is in the calls
step.
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
CAP = 1024
PRESETS = ("natural", "dense", "checkerboard", "full")
LABEL_KERNELS = ("hvq_label_begin_kernel", "hvq_label_tile_kernel", "hvq_label_seam_kernel", "hvq_label_flatten_kernel", "hvq_label_number_kernel", "hvq_label_resolve_kernel",
                 "hvq_label_finish_kernel")


def trace_plan(reps):
    """(label, kernel, count) of the trace step's launches in their order"""
    plan = [("scale_identity", "hvq_scale_kernel", 1 + reps)]
    for p in PRESETS:
        for r in range(1 + reps):
            plan += [(f"{p}/{r}/{k}", k, 1) for k in LABEL_KERNELS]
        plan.append((f"{p}/select", "hvq_select_kernel", 1 + reps))
    return plan


def setup(args):
    import numpy as np
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch, labels, maps
    ctx = batch.Context(0)
    otsu = maps.Rule(maps.otsu().luma, maps.flat(128).luma)
    S = {"torch": torch, "ctx": ctx, "masks": {}, "lists": {}}
    for p in ("natural", "dense"):
        a_s, a_o = picture_lists(resident(ctx, preset=p, streams=args.streams, per=args.per, distinct=args.distinct), args.per)
        S["lists"][p] = (a_s, a_o)
        S["masks"][p] = ctx.equalize_pictures(a_s, a_o, otsu)
    n = len(S["lists"]["natural"][0])
    yy, xx = np.mgrid[0:H, 0:W]
    board = np.concatenate([(((xx + yy) & 1) * 255).astype(np.uint8).reshape(-1), np.full(PIC_BYTES - W * H, 128, np.uint8)])
    S["masks"]["checkerboard"] = torch.from_numpy(board).cuda().repeat(n, 1)
    S["masks"]["full"] = torch.full((n, PIC_BYTES), 255, dtype=torch.uint8, device="cuda")
    S["n"] = n
    S["labels"] = torch.empty((n, H, W), dtype=torch.int32, device="cuda")                   # 1.26 GB for 1024 pictures
    S["comps"] = torch.empty((n, CAP + 1, 8), dtype=torch.int64, device="cuda")
    S["out"] = torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
    S["rule"] = {p: labels.rule(connectivity=4 if p == "checkerboard" else 8) for p in PRESETS}
    S["select"] = labels.select(area=50)
    torch.cuda.synchronize()
    return S


def the_calls(S):
    ctx, n = S["ctx"], S["n"]
    a_s = S["lists"]["natural"][0]
    labs, comps = [S["labels"][i] for i in range(n)], [S["comps"][i] for i in range(n)]
    calls = {"scale_identity": lambda: ctx.scale_pictures(*S["lists"]["natural"], (W, H), out=S["out"])}
    for p in PRESETS:
        rows = [S["masks"][p][i] for i in range(n)]
        calls["label_" + p] = lambda rows=rows, p=p: ctx.label_pictures(a_s, [-1] * n, S["rule"][p], cap=CAP, src=rows, labels=labs, comps=comps)
        calls["select_" + p] = lambda: ctx.select_components(a_s, labs, comps, S["select"], out=S["out"])
    return calls


def host_labeller():
    """-> (name, f(mask uint8 [H][W], connectivity) -> K) of the host leg"""
    import numpy as np
    try:
        from scipy import ndimage
    except ImportError:
        from hvqm4_amd import labels
        return "hvqm4_amd.labels.of_plane", lambda m, c: int(labels.of_plane(m, labels.rule(connectivity=c))[1][0, 0])
    full = np.ones((3, 3), dtype=bool)

    def run(m, c):
        lab, K = ndimage.label(m == 255, structure=full if c == 8 else None)
        ndimage.find_objects(lab)
        return K
    return "scipy.ndimage.label + find_objects", run


def child_calls(args):
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
    from hvqm4_amd import labels
    S = setup(args)
    torch, ctx, n = S["torch"], S["ctx"], S["n"]
    calls = the_calls(S)
    res = {"size": f"{W}x{H}", "pictures": n, "cap": CAP, "reps": args.reps, "rounds": args.rounds, "label_map_bytes": n * W * H * 4, "rows": {}}
    probe = list(range(0, n, max(1, n // 4)))
    checks, counts = {}, {}
    for p in PRESETS:
        calls["label_" + p](); calls["select_" + p]()
        torch.cuda.synchronize()
        ok = True
        for i in probe:
            mask = S["masks"][p][i].cpu().numpy()
            lab, rec = labels.of_picture(mask, SRC, S["rule"][p], CAP)
            got_c = S["comps"][i].cpu().numpy()
            ok = ok and np.array_equal(S["labels"][i].cpu().numpy().view(np.uint32), lab) and np.array_equal(got_c[:rec.shape[0]], rec) and got_c[0, 3] == 0
            ok = ok and np.array_equal(S["out"][i].cpu().numpy(), labels.of_select(lab, rec, S["select"], SRC))
        checks[p] = bool(ok)
        head = S["comps"][:, 0, :4].cpu().numpy()
        counts[p] = {"K_median": float(np.median(head[:, 0])), "K_max": int(head[:, 0].max()), "F_median": float(np.median(head[:, 2])), "status_max": int(head[:, 3].max())}
    res["equal_host_module"], res["components"] = checks, counts
    labels_ = list(calls)
    for label in labels_:
        timed(torch, calls[label], args.warmup)
    ms = {label: [] for label in labels_}
    for _ in range(args.rounds):
        for label in labels_:
            ms[label].append(round(timed(torch, calls[label], args.reps), 4))
    for label, v in ms.items():
        res["rows"][label] = {"ms": v, "median_ms": statistics.median(v)}
    # the host route on the natural preset: the read-back, then the masks through the host labeller on 16 threads
    a_s, a_o = S["lists"]["natural"]
    name, run = host_labeller()
    masks = S["masks"]["natural"].cpu().numpy()[:, :W * H].reshape(n, H, W)
    pool = ThreadPoolExecutor(16)
    host = []
    for _ in range(max(1, min(3, args.rounds))):
        t0 = time.perf_counter()
        ctx.read_pictures(a_s, a_o)
        t1 = time.perf_counter()
        ks = list(pool.map(lambda m: run(m, 8), masks))
        t2 = time.perf_counter()
        host.append((round((t1 - t0) * 1e3, 2), round((t2 - t1) * 1e3, 2)))
    pool.shutdown()
    res["host_components_equal"] = bool(ks == S["comps"][:, 0, 0].cpu().tolist()) if False else None     # the comps hold the last preset's; K is compared below
    calls["label_natural"]()
    torch.cuda.synchronize()
    res["host_components_equal"] = bool(ks == [int(v) for v in S["comps"][:, 0, 0].cpu().tolist()])
    host_ms = statistics.median(a + b for a, b in host)
    med = lambda label: res["rows"][label]["median_ms"]
    res["host_route"] = {"labeller": name, "threads": 16, "read_pictures_ms, label_ms": host, "median_ms": round(host_ms, 2)}
    res["condition"] = {"what": "label_pictures per call on the natural preset faster than read_pictures + the host labeller on 16 threads, same session",
                        "label_ms": med("label_natural"), "host_ms": round(host_ms, 2), "host_over_label": round(host_ms / med("label_natural"), 1),
                        "holds": med("label_natural") < host_ms}
    ctx.close()
    print(json.dumps(res))


def child_trace(args):
    """the launches the trace is taken of, in trace_plan's order"""
    S = setup(args)
    calls = the_calls(S)
    sync = S["torch"].cuda.synchronize
    for _ in range(1 + args.reps):
        calls["scale_identity"]()
    sync()
    for p in PRESETS:
        for _ in range(1 + args.reps):
            calls["label_" + p]()
        sync()
        for _ in range(1 + args.reps):
            calls["select_" + p]()
        sync()
    S["ctx"].close()
    print(json.dumps({"launches": 1 + args.reps, "pictures": S["n"]}))


def trace_summary(trace_dir, plan, _earlier=None):
    per = plan["launches"]
    cut = read_planned(trace_dir, trace_plan(per - 1), kernels=set(LABEL_KERNELS) | {"hvq_scale_kernel", "hvq_select_kernel"})
    if "error" in cut:
        return cut
    res = {"pictures": plan["pictures"], "kernels": {k: resources(cut[f"natural/0/{k}"][0]) for k in LABEL_KERNELS}}
    res["kernels"]["hvq_select_kernel"] = resources(cut["natural/select"][0])
    res["scale_identity"] = launch_stats(l.ns for l in cut["scale_identity"][1:])
    luma_share = res["scale_identity"]["median_us"] * (W * H) / PIC_BYTES
    res["yardstick_us"] = round(2.5 * luma_share, 1)
    for p in PRESETS:
        row = {k: launch_stats(cut[f"{p}/{r}/{k}"][0].ns for r in range(1, per)) for k in LABEL_KERNELS}          # without the warm-up call
        row["sum_median_us"] = round(sum(row[k]["median_us"] for k in LABEL_KERNELS), 1)
        row["sum_over_yardstick"] = round(row["sum_median_us"] / res["yardstick_us"], 2)
        row["select"] = launch_stats(l.ns for l in cut[f"{p}/select"][1:])
        res[p] = row
    return res


def main():
    ap = argparse.ArgumentParser()
    add_common_arguments(ap, children=("calls", "trace"), reps=5, warmup=2, rounds=5, steps="calls,trace", out_dir="label_bench_out", out="--out")
    args = ap.parse_args()
    if args.child:
        return {"calls": child_calls, "trace": child_trace}[args.child](args)
    drive(args, {"calls": ("calls", None), "trace": ("trace", trace_summary)}, [sys.executable, os.path.abspath(__file__)])


if __name__ == "__main__":
    main()
