"""Picture histograms (hvq_picture_histograms, Context.picture_histograms) on the GPU: 128 dense 640x480 4:2:0 streams, 8 resident pictures
each, 1024 pictures per call; natural content (the decoded pictures) and flat content (`src` tensors filled with one value: every lane of
every wave adds into the same bin), HVQ_HIST_VALUES and HVQ_HIST_ABSDIFF (natural: picture k against k - 1 inside the stream's 8
pictures; flat: one constant against another).

Two measurements, each a child process of this driver under its own `timeout`; a step that fails ends the run:
  calls   HIP-event timed on one stream, in alternating rounds: (a) the four histogram calls; (b) picture_metrics on the same pictures
          (against zeros: the bytes VALUES reads; against the predecessor: the bytes ABSDIFF reads) -- the project's streaming bound for
          reading those bytes; (c) the route a user takes without the call: export(..., "yuv444p") of the 1024 pictures, then ONE
          torch.bincount over all planes (each plane's values offset into bins of its own), which is kinder to the route than a
          bincount per plane.  The route's chroma counts are of the replicated planes, so only luma is compared with the call's.
  trace   rocprofv3 --kernel-trace --stats around a child that launches the same six calls in a fixed order, one warm-up and `reps`
          launches each.  Kernel times are read from the trace: median with min-max; bytes = pic_bytes per picture and side; share of
          8 TB/s; the histogram kernel's time over the metrics kernel's for the same bytes.
One JSON line per measurement on stdout and in --out-dir.  torch is imported before the library, so both share one HIP runtime."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12
W, H = 640, 480
PIC_BYTES = W * H * 3 // 2
FLAT_A, FLAT_B = 128, 100


def setup(args):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    from tools.export_bench import resident_streams
    ctx = batch.Context(0)
    sids = resident_streams(ctx, "420", args.streams, args.per, args.distinct, W, H)
    return torch, ctx, sids


def workload(torch, ctx, sids, per):
    """label -> (callable, kernel name, sides read): the six calls over the same 1024 pictures"""
    a_s = [s for s in sids for _ in range(per)]
    a_o = [k for _ in sids for k in range(per)]
    refs = [(s, (k - 1) % per) for s in sids for k in range(per)]
    n = len(a_s)
    flat_a = torch.full((n, PIC_BYTES), FLAT_A, dtype=torch.uint8, device="cuda")
    flat_b = torch.full((n, PIC_BYTES), FLAT_B, dtype=torch.uint8, device="cuda")
    src_a, ref_b, minus = list(flat_a), list(flat_b), [-1] * n
    hist = torch.empty((n, 3, 256), dtype=torch.int32, device="cuda")
    met = torch.empty((n, 3, 4), dtype=torch.int64, device="cuda")
    calls = {
        "values_natural": (lambda: ctx.picture_histograms(a_s, a_o, out=hist), "hvq_histogram_kernel", 1),
        "absdiff_natural": (lambda: ctx.picture_histograms(a_s, a_o, ref=refs, out=hist), "hvq_histogram_kernel", 2),
        "values_flat": (lambda: ctx.picture_histograms(a_s, minus, src=src_a, out=hist), "hvq_histogram_kernel", 1),
        "absdiff_flat": (lambda: ctx.picture_histograms(a_s, minus, ref=ref_b, src=src_a, out=hist), "hvq_histogram_kernel", 2),
        "metrics_zeros": (lambda: ctx.picture_metrics(a_s, a_o, out=met), "hvq_metrics_kernel", 1),
        "metrics_pairs": (lambda: ctx.picture_metrics(a_s, a_o, refs, out=met), "hvq_metrics_kernel", 2),
    }
    return calls, (a_s, a_o, refs, hist, met, flat_a, flat_b)


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def child_calls(args):
    torch, ctx, sids = setup(args)
    calls, (a_s, a_o, _refs, hist, _met, _fa, _fb) = workload(torch, ctx, sids, args.per)
    n = len(a_s)
    u8 = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
    offs = (torch.arange(n * 3, dtype=torch.int64, device="cuda") * 256).view(n, 3, 1, 1)
    keep = {}

    def route():
        ctx.export(a_s, a_o, u8, "yuv444p")
        keep["h"] = torch.bincount((u8.to(torch.int64) + offs).view(-1), minlength=n * 3 * 256).view(n, 3, 256)

    fns = {k: v[0] for k, v in calls.items()}
    fns["route_export_bincount"] = route
    for fn in fns.values():
        timed(torch, fn, args.warmup)
    fns["values_natural"]()
    torch.cuda.synchronize()
    agree = bool(torch.equal(hist[:, 0].to(torch.int64), keep["h"][:, 0]))
    fns["values_flat"]()
    torch.cuda.synchronize()
    flat_ok = bool(hist[:, 0, FLAT_A].eq(W * H).all() and hist.sum().item() == n * PIC_BYTES)
    if not (agree and flat_ok):
        sys.exit(f"wrong counts (luma agrees with the route: {agree}, flat pictures counted right: {flat_ok}): nothing is timed")
    res = {"size": f"{W}x{H}", "pictures": n, "reps": args.reps, "rounds": args.rounds, "ms": {k: [] for k in fns}}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            res["ms"][k].append(round(timed(torch, fn, args.route_reps if k.startswith("route") else args.reps), 4))
    med = {k: statistics.median(v) for k, v in res["ms"].items()}
    res["median_ms"] = med
    res["route_over_values_natural"] = round(med["route_export_bincount"] / med["values_natural"], 1)
    res["values_natural_over_metrics_zeros"] = round(med["values_natural"] / med["metrics_zeros"], 2)
    res["absdiff_natural_over_metrics_pairs"] = round(med["absdiff_natural"] / med["metrics_pairs"], 2)
    res["values_flat_over_natural"] = round(med["values_flat"] / med["values_natural"], 2)
    res["absdiff_flat_over_natural"] = round(med["absdiff_flat"] / med["absdiff_natural"], 2)
    res["absdiff_over_values_per_byte_read"] = round(med["absdiff_natural"] / (2 * med["values_natural"]), 2)
    res["luma_agrees_with_the_route"] = agree
    res["flat_counts_right"] = flat_ok
    ctx.close()
    print(json.dumps(res))


def child_trace(args):
    """the launches the trace is taken of, in the order trace_summary reads them by"""
    torch, ctx, sids = setup(args)
    calls, _keep = workload(torch, ctx, sids, args.per)
    plan = []
    for label, (fn, kernel, sides) in calls.items():
        for _ in range(1 + args.reps):
            fn()
        torch.cuda.synchronize()
        plan.append([label, kernel, 1 + args.reps, args.streams * args.per, sides * PIC_BYTES])
    ctx.close()
    print(json.dumps({"plan": plan}))


def trace_summary(trace_dir, plan):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return {"error": f"no kernel trace under {trace_dir}"}
    rows = []
    with open(files[0], newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name") or row.get("Name") or ""
            if "hvq_histogram_kernel" in name or "hvq_metrics_kernel" in name:
                rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"]), name.split("(")[0],
                             row.get("VGPR_Count"), row.get("LDS_Block_Size"), row.get("Scratch_Size")))
    rows.sort()
    if len(rows) != sum(p[2] for p in plan):
        return {"error": f"{len(rows)} launches of the two kernels in the trace, {sum(p[2] for p in plan)} planned"}
    res, at = {}, 0
    for label, kernel, count, n, per_picture in plan:
        part = rows[at + 1:at + count]                                            # without the warm-up launch
        at += count
        if any(kernel not in r[2] for r in part):
            return {"error": f"{label}: the launches in the trace are not in the planned order"}
        d = sorted(r[1] for r in part)
        by = n * per_picture
        med = statistics.median(d)
        res[label] = {"kernel": part[0][2], "pictures": n, "launches": len(d), "median_us": round(med / 1e3, 1), "min_us": round(d[0] / 1e3, 1),
                      "max_us": round(d[-1] / 1e3, 1), "bytes": by, "of_peak_median": round(by / (med * 1e-9) / PEAK, 3),
                      "vgprs": part[0][3], "lds": part[0][4], "scratch": part[0][5]}
    us = {k: v["median_us"] for k, v in res.items()}
    res["values_natural_over_metrics_zeros"] = round(us["values_natural"] / us["metrics_zeros"], 2)
    res["absdiff_natural_over_metrics_pairs"] = round(us["absdiff_natural"] / us["metrics_pairs"], 2)
    res["values_flat_over_natural"] = round(us["values_flat"] / us["values_natural"], 2)
    res["absdiff_flat_over_natural"] = round(us["absdiff_flat"] / us["absdiff_natural"], 2)
    return res


def run(cmd, limit, log):
    """one GPU step under its own time limit; a failed step ends the run"""
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, capture_output=True, text=True)
    with open(log, "w") as f:
        f.write(r.stdout + "\n--- stderr ---\n" + r.stderr[-20000:])
    if r.returncode:
        sys.exit(f"{' '.join(cmd[:6])} ... ended with status {r.returncode}: see {log}")
    return [l for l in r.stdout.splitlines() if l.startswith("{")][-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("calls", "trace"), default=None)
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--per", type=int, default=8, help="resident pictures per stream")
    ap.add_argument("--distinct", type=int, default=2, help="distinct clips dealt over the streams")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--route-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", default="calls,trace")
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out-dir", default="histogram_bench_out")
    args = ap.parse_args()
    if args.child:
        return {"calls": child_calls, "trace": child_trace}[args.child](args)
    os.makedirs(args.out_dir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    common = ["--streams", str(args.streams), "--per", str(args.per), "--distinct", str(args.distinct), "--reps", str(args.reps),
              "--route-reps", str(args.route_reps), "--warmup", str(args.warmup), "--rounds", str(args.rounds)]
    for step in args.steps.split(","):
        print(f"# step {step}", flush=True)
        if step == "trace":
            tdir = os.path.join(args.out_dir, "trace")
            line = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--"] + me + ["--child", "trace"] + common,
                       args.step_timeout, os.path.join(args.out_dir, "trace.log"))
            res = trace_summary(tdir, json.loads(line)["plan"])
            if "error" in res:
                sys.exit(f"trace: {res['error']}")
        elif step == "calls":
            res = json.loads(run(me + ["--child", "calls"] + common, args.step_timeout, os.path.join(args.out_dir, "calls.log")))
        else:
            sys.exit(f"unknown step {step}")
        line = json.dumps({step: res})
        print(line, flush=True)
        with open(os.path.join(args.out_dir, step + ".json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
