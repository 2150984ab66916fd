"""Windowed SSIM (hvq_picture_ssim, Context.picture_ssim) on the GPU: the workload of tools/metrics_bench.py -- 128 dense 640x480 4:2:0
streams, 8 resident pictures each, 1024 pairs (k, k - 1) (k - 1 taken inside the stream's 8 pictures).

Two measurements, each a child process of this driver under its own `timeout`; a step that fails ends the run:
  trace   rocprofv3 --kernel-trace --stats around a child that launches, in a fixed order, hvq_ssim_kernel without maps, with maps, and
          -- in the same process, on the same pairs -- hvq_metrics_kernel, the yardstick: it reads exactly the same bytes.  One warm-up
          launch and `reps` launches each.  Kernel times are read from the trace: median with min-max; bytes = 2 x pic_bytes per pair
          (plus the maps written); the two ratios to the metrics kernel.
  route   the call against the route a user takes without it: export(..., "yuv444p") of both pictures -> float32 -> the same windows by
          avg_pool2d(8, stride 4) on a, b, a^2 + b^2 and a b -> the formula -> the mean per plane.  Both event-timed on one stream in
          alternating rounds; the two must agree on the luma mean (the chroma planes of the export are replicated to full size, so
          only luma is compared, and the route's float32 variances only agree to about 1e-4).
One JSON line per measurement on stdout and in --out-dir.  torch is imported before the library, so both share one HIP runtime."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.metrics_bench import H, PEAK, PIC_BYTES, W, pairs, run, setup, timed      # noqa: E402

KERNELS = ("hvq_ssim_kernel", "hvq_metrics_kernel")


def child_trace(args):
    """the launches the trace is taken of, in the order trace_summary reads them by"""
    from hvqm4_amd.metrics import ssim_windows
    torch, ctx, sids = setup(args)
    a_s, a_o, refs = pairs(sids, args.per, False)
    n = len(a_s)
    windows = sum(r * c for r, c in ssim_windows(W, H, 2, 2))
    plan = []
    out = torch.empty((n, 3, 2), dtype=torch.int64, device="cuda")
    for _ in range(1 + args.reps):
        ctx.picture_ssim(a_s, a_o, refs, out=out)
    torch.cuda.synchronize()
    plan.append(["ssim", "hvq_ssim_kernel", 1 + args.reps, n, 2 * PIC_BYTES])
    for _ in range(1 + args.reps):
        _o, maps = ctx.picture_ssim(a_s, a_o, refs, out=out, maps=True)
    torch.cuda.synchronize()
    del maps
    plan.append(["ssim_maps", "hvq_ssim_kernel", 1 + args.reps, n, 2 * PIC_BYTES + 4 * windows])
    m = torch.empty((n, 3, 4), dtype=torch.int64, device="cuda")
    for _ in range(1 + args.reps):
        ctx.picture_metrics(a_s, a_o, refs, out=m)
    torch.cuda.synchronize()
    plan.append(["metrics", "hvq_metrics_kernel", 1 + args.reps, n, 2 * PIC_BYTES])
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
            if any(k in name for k in KERNELS):
                rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"]), name.split("(")[0],
                             row.get("VGPR_Count"), row.get("LDS_Block_Size"), row.get("Scratch_Size")))
    rows.sort()
    if len(rows) != sum(p[2] for p in plan):
        return {"error": f"{len(rows)} launches of the two kernels in the trace, {sum(p[2] for p in plan)} planned"}
    res, at = {}, 0
    for label, kernel, count, n, per_pair in plan:
        part = rows[at + 1:at + count]                                            # without the warm-up launch
        at += count
        if any(kernel not in r[2] for r in part):
            return {"error": f"{label}: the launches in the trace are not in the planned order"}
        d = sorted(r[1] for r in part)
        by = n * per_pair
        med = statistics.median(d)
        res[label] = {"kernel": part[0][2], "pairs": n, "launches": len(d), "median_us": round(med / 1e3, 1), "min_us": round(d[0] / 1e3, 1),
                      "max_us": round(d[-1] / 1e3, 1), "bytes": by, "of_peak_median": round(by / (med * 1e-9) / PEAK, 3),
                      "vgprs": part[0][3], "lds": part[0][4], "scratch": part[0][5]}
    res["ssim_over_metrics"] = round(res["ssim"]["median_us"] / res["metrics"]["median_us"], 2)
    res["ssim_maps_over_metrics"] = round(res["ssim_maps"]["median_us"] / res["metrics"]["median_us"], 2)
    return res


def torch_route_ssim(torch, ua, ub):
    """uint8 [n, 3, H, W] twice -> float32 [n, 3]: the mean over the 8 x 8 windows, 4 samples apart, of the library's formula in means"""
    import torch.nn.functional as F
    a, b = ua.to(torch.float32), ub.to(torch.float32)
    pool = lambda x: F.avg_pool2d(x, 8, stride=4)
    ma, mb, m2, mab = pool(a), pool(b), pool(a * a + b * b), pool(a * b)
    c1, c2 = 416.0 / 4096.0, 235963.0 / 4096.0                                   # the integer constants over 64^2
    sq, cr = ma * ma + mb * mb, ma * mb
    q = ((2.0 * cr + c1) * (2.0 * (mab - cr) + c2)) / ((sq + c1) * (m2 - sq + c2))
    return q.mean(dim=(2, 3))


def child_route(args):
    from hvqm4_amd.metrics import ssim
    torch, ctx, sids = setup(args)
    res = {"size": f"{W}x{H}", "reps": args.reps, "rounds": args.rounds}
    a_s, a_o, refs = pairs(sids, args.per, False)
    n = len(a_s)
    b_s, b_o = [s for s, _k in refs], [k for _s, k in refs]
    out = torch.empty((n, 3, 2), dtype=torch.int64, device="cuda")
    ua = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
    ub = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
    keep = {}

    def call():
        ctx.picture_ssim(a_s, a_o, refs, out=out)

    def route():
        ctx.export(a_s, a_o, ua, "yuv444p")
        ctx.export(b_s, b_o, ub, "yuv444p")
        keep["ssim"] = torch_route_ssim(torch, ua, ub)

    timed(torch, call, args.warmup)
    timed(torch, route, args.warmup)
    diff = (ssim(out)[:, 0] - keep["ssim"][:, 0].to(torch.float64)).abs().max().item()
    rows = {"pairs": n, "call_ms": [], "route_ms": []}
    for _ in range(args.rounds):
        rows["call_ms"].append(round(timed(torch, call, args.reps), 4))
        rows["route_ms"].append(round(timed(torch, route, args.reps), 4))
    rows["call_median_ms"] = statistics.median(rows["call_ms"])
    rows["route_median_ms"] = statistics.median(rows["route_ms"])
    rows["speedup"] = round(rows["route_median_ms"] / rows["call_median_ms"], 2)
    rows["luma_mean_max_abs_difference"] = diff
    rows["luma_means_agree"] = bool(diff < 1e-3)
    rows["luma_mean_ssim_of_the_workload"] = round(ssim(out)[:, 0].mean().item(), 6)
    res["pairs_all"] = rows
    ctx.close()
    print(json.dumps(res))


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
    ap.add_argument("--out-dir", default="ssim_bench_out")
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
