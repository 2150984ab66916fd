"""Picture metrics (hvq_picture_metrics, Context.picture_metrics) on the GPU: 128 dense 640x480 4:2:0 streams, 8 resident pictures each.

Two measurements, each a child process of this driver under its own `timeout`; a step that fails ends the run:
  trace   rocprofv3 --kernel-trace --stats around a child that launches, in a fixed order, the metrics of 1024 pairs (k, k - 1)
          (k - 1 taken inside the stream's 8 pictures, so picture 0 pairs with picture 7), of 128 pairs (the newest picture of every
          stream against its predecessor), and -- in the same process, on the same box -- the uint8 export of the same 1024 pictures
          (planar RGB and YUV 4:4:4), the yardstick for "bound by HBM".  One warm-up launch and `reps` launches each.  Kernel times
          are read from the trace: median with min-max; bytes = 2 x pic_bytes per pair (metrics), source planes read + destination
          written (export); share of 8 TB/s.
  route   the call against the route a user takes without it: export(..., "yuv444p") of both pictures, then per plane the int32
          difference, abs().sum() and pow(2).sum() in torch.  Both event-timed on one stream in alternating rounds, 1024 and 128 pairs;
          the two routes must agree on luma sad and sse (the chroma planes of the export are replicated to full size, so only luma
          is compared).
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


def setup(args):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    from tools.export_bench import resident_streams
    ctx = batch.Context(0)
    sids = resident_streams(ctx, "420", args.streams, args.per, args.distinct, W, H)
    return torch, ctx, sids


def pairs(sids, per, newest_only):
    """(sids, ordinals, references): every picture against its predecessor inside the stream, or only the newest of every stream"""
    ks = [per - 1] if newest_only else list(range(per))
    a_s = [s for s in sids for _ in ks]
    a_o = [k for _ in sids for k in ks]
    refs = [(s, (k - 1) % per) for s in sids for k in ks]
    return a_s, a_o, refs


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def child_trace(args):
    """the launches the trace is taken of, in the order trace_summary reads them by"""
    torch, ctx, sids = setup(args)
    plan = []
    for label, newest in (("metrics_all", False), ("metrics_newest", True)):
        a_s, a_o, refs = pairs(sids, args.per, newest)
        out = torch.empty((len(a_s), 3, 4), dtype=torch.int64, device="cuda")
        for _ in range(1 + args.reps):
            ctx.picture_metrics(a_s, a_o, refs, out=out)
        torch.cuda.synchronize()
        plan.append([label, "hvq_metrics_kernel", 1 + args.reps, len(a_s), 2 * PIC_BYTES])
    a_s, a_o, _refs = pairs(sids, args.per, False)
    for fmt in ("rgbp", "yuv444p"):
        u8 = torch.empty((len(a_s), 3, H, W), dtype=torch.uint8, device="cuda")
        for _ in range(1 + args.reps):
            ctx.export(a_s, a_o, u8, fmt)
        torch.cuda.synchronize()
        plan.append(["export_" + fmt, "hvq_yuv_rgb_kernel", 1 + args.reps, len(a_s), PIC_BYTES + 3 * W * H])
        del u8
        torch.cuda.empty_cache()
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
            if "hvq_metrics_kernel" in name or "hvq_yuv_rgb_kernel" in name:
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
                      "of_peak_best": round(by / (d[0] * 1e-9) / PEAK, 3), "vgprs": part[0][3], "lds": part[0][4], "scratch": part[0][5]}
    if "metrics_all" in res and "export_rgbp" in res:
        res["metrics_share_over_export_share"] = round(res["metrics_all"]["of_peak_median"] / res["export_rgbp"]["of_peak_median"], 2)
    return res


def child_route(args):
    torch, ctx, sids = setup(args)
    res = {"size": f"{W}x{H}", "reps": args.reps, "rounds": args.rounds}
    for label, newest in (("pairs_all", False), ("pairs_newest", True)):
        a_s, a_o, refs = pairs(sids, args.per, newest)
        n = len(a_s)
        b_s, b_o = [s for s, _k in refs], [k for _s, k in refs]
        out = torch.empty((n, 3, 4), dtype=torch.int64, device="cuda")
        ua = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
        ub = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
        keep = {}

        def call():
            ctx.picture_metrics(a_s, a_o, refs, out=out)

        def route():
            ctx.export(a_s, a_o, ua, "yuv444p")
            ctx.export(b_s, b_o, ub, "yuv444p")
            d = ua.to(torch.int32) - ub.to(torch.int32)
            keep["sad"] = d.abs().sum(dim=(2, 3))
            keep["sse"] = d.pow(2).sum(dim=(2, 3))

        timed(torch, call, args.warmup)
        timed(torch, route, args.warmup)
        agree = bool(torch.equal(out[:, 0, 2], keep["sad"][:, 0]) and torch.equal(out[:, 0, 3], keep["sse"][:, 0]))
        rows = {"pairs": n, "call_ms": [], "route_ms": []}
        for _ in range(args.rounds):
            rows["call_ms"].append(round(timed(torch, call, args.reps), 4))
            rows["route_ms"].append(round(timed(torch, route, args.reps), 4))
        rows["call_median_ms"] = statistics.median(rows["call_ms"])
        rows["route_median_ms"] = statistics.median(rows["route_ms"])
        rows["speedup"] = round(rows["route_median_ms"] / rows["call_median_ms"], 2)
        rows["luma_sad_and_sse_agree"] = agree
        res[label] = rows
        del out, ua, ub
        keep.clear()
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(res))


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
    ap.add_argument("--child", choices=("trace", "route"), default=None)
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--per", type=int, default=8, help="resident pictures per stream")
    ap.add_argument("--distinct", type=int, default=2, help="distinct clips dealt over the streams")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", default="trace,route")
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out-dir", default="metrics_bench_out")
    args = ap.parse_args()
    if args.child:
        return {"trace": child_trace, "route": child_route}[args.child](args)
    os.makedirs(args.out_dir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    common = ["--streams", str(args.streams), "--per", str(args.per), "--distinct", str(args.distinct), "--reps", str(args.reps),
              "--warmup", str(args.warmup), "--rounds", str(args.rounds)]
    for step in args.steps.split(","):
        print(f"# step {step}", flush=True)
        if step == "trace":
            tdir = os.path.join(args.out_dir, "trace")
            line = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--"] + me + ["--child", "trace"] + common,
                       args.step_timeout, os.path.join(args.out_dir, "trace.log"))
            res = trace_summary(tdir, json.loads(line)["plan"])
            if "error" in res:
                sys.exit(f"trace: {res['error']}")
        elif step == "route":
            res = json.loads(run(me + ["--child", "route"] + common, args.step_timeout, os.path.join(args.out_dir, "route.log")))
        else:
            sys.exit(f"unknown step {step}")
        line = json.dumps({step: res})
        print(line, flush=True)
        with open(os.path.join(args.out_dir, step + ".json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
