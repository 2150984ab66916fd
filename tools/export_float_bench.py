"""Float export (hvq_export_tensors, Context.export_float) on the GPU: 128 dense 640x480 4:2:0 streams, 8 resident pictures each.

Two measurements, each a child process of this driver under its own `timeout`:
  trace   rocprofv3 --kernel-trace --stats around a child that exports all 1024 pictures at their own size (the identity body) as
          float32 / float16 / bfloat16, and -- in the same process, on the same box -- as uint8 planar RGB and RGB24 through
          hvq_export_pictures.  Kernel times are read from the trace; bytes = source planes read + destination written; share of
          8 TB/s.
  route   the fused call against the route a user of the uint8 export takes: export(..., "rgbp"), .to(dtype), crop,
          F.interpolate(bilinear), normalise in torch (in place).  Both event-timed on one stream, alternating rounds, 640x480 ->
          same size and -> 224x224, float32 and float16.
  aa      the antialiased call (export_float(antialias=True), hvq_export_resampled) for 128 pictures (16 streams of 8) 640x480 ->
          224x224 and -> 320x240, float32 and float16, four legs: (a) the call as the library runs it (the tiled body at these shapes),
          (b) the same forced to the direct body (HVQ_FILTER_TRIANGLE_DIRECT: an argument for this tool and the tests, not a switch
          of the product), (c) the plain two-tap call at the same shapes, (d) the torch route export("rgbp") -> .float() ->
          F.interpolate(antialias=True) -> normalise.  Event-timed on one stream in alternating rounds.
  aa_trace  rocprofv3 --kernel-trace --stats around legs (a), (b), (c) in a fixed order: the kernel times of the legs.
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
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ES = {"float32": 4, "float16": 2, "bfloat16": 2}


def setup(args):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    from tools.export_bench import resident_streams
    ctx = batch.Context(0)
    sids = resident_streams(ctx, "420", args.streams, args.per, args.distinct, W, H)
    all_s = [s for s in sids for _ in range(args.per)]
    all_o = [k for _ in sids for k in range(args.per)]
    return torch, ctx, all_s, all_o


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def child_identity(args):
    """the launches the trace is taken of; the event-timed call rate (host-bound at 1024 destinations per call) goes to stdout"""
    torch, ctx, all_s, all_o = setup(args)
    n = len(all_s)
    res = {"pictures": n, "size": f"{W}x{H}", "reps": args.reps}
    for dt in ES:
        out = torch.empty((n, 3, H, W), dtype=getattr(torch, dt), device="cuda")
        fn = lambda: ctx.export_float(all_s, all_o, out, mean=MEAN, std=STD)
        timed(torch, fn, args.warmup)
        res[f"export_float_{dt}_call_ms"] = round(timed(torch, fn, args.reps), 4)
        del out
        torch.cuda.empty_cache()
    for fmt in ("rgbp", "rgb"):
        out = torch.empty((n, 3, H, W) if fmt == "rgbp" else (n, H, W, 3), dtype=torch.uint8, device="cuda")
        fn = lambda: ctx.export(all_s, all_o, out, fmt)
        timed(torch, fn, args.warmup)
        res[f"export_{fmt}_call_ms"] = round(timed(torch, fn, args.reps), 4)
        del out
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(res))


def child_route(args):
    torch, ctx, all_s, all_o = setup(args)
    import torch.nn.functional as F
    from hvqm4_amd.export import normalisation
    n = len(all_s)
    mul, add = normalisation(MEAN, STD)
    res = {"pictures": n, "source": f"{W}x{H}", "reps": args.reps, "rounds": args.rounds}
    u8 = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
    for hw in ((H, W), (224, 224)):
        for dt in ("float32", "float16"):
            td = getattr(torch, dt)
            m = torch.tensor(mul, dtype=td, device="cuda").view(1, 3, 1, 1)
            a = torch.tensor(add, dtype=td, device="cuda").view(1, 3, 1, 1)
            out = torch.empty((n, 3) + hw, dtype=td, device="cuda")
            keep = {}

            def fused():
                ctx.export_float(all_s, all_o, out, mean=MEAN, std=STD)

            def route():
                ctx.export(all_s, all_o, u8, "rgbp")
                x = u8.to(td)
                if hw != (H, W):
                    x = F.interpolate(x, size=hw, mode="bilinear", align_corners=False)
                keep["x"] = x.mul_(m).add_(a)

            timed(torch, fused, args.warmup)
            timed(torch, route, args.warmup)
            worst = float((out.float() - keep["x"].float()).abs().max())        # the two routes agree up to rounding
            rows = {"fused_ms": [], "route_ms": []}
            for _ in range(args.rounds):
                rows["fused_ms"].append(round(timed(torch, fused, args.reps), 4))
                rows["route_ms"].append(round(timed(torch, route, args.reps), 4))
            src = W * H * 3 // 2
            rows["fused_bytes"] = n * (src + 3 * hw[0] * hw[1] * ES[dt])
            rows["speedup"] = round(statistics.median(rows["route_ms"]) / statistics.median(rows["fused_ms"]), 2)
            rows["max_abs_difference"] = worst
            res[f"{hw[1]}x{hw[0]}_{dt}"] = rows
            del out, m, a
            keep.clear()
            torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(res))


AA_SHAPES = ((224, 224), (240, 320))
AA_DTYPES = ("float32", "float16")


def aa_setup(args):
    args.streams, args.per = args.aa_streams, 8
    return setup(args)


def aa_legs(torch, ctx, all_s, all_o, hw, dt):
    """the four legs of one shape and dtype as closures: {leg: (fn, result tensor getter)}"""
    import torch.nn.functional as F
    from hvqm4_amd.export import FILTER_TRIANGLE, FILTER_TRIANGLE_DIRECT, normalisation
    n = len(all_s)
    td = getattr(torch, dt)
    mul, add = normalisation(MEAN, STD)
    m = torch.tensor(mul, dtype=td, device="cuda").view(1, 3, 1, 1)
    a = torch.tensor(add, dtype=td, device="cuda").view(1, 3, 1, 1)
    outs = {k: torch.empty((n, 3) + hw, dtype=td, device="cuda") for k in "abc"}
    u8 = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
    keep = {}

    def leg_d():
        ctx.export(all_s, all_o, u8, "rgbp")
        keep["d"] = F.interpolate(u8.to(td), size=hw, mode="bilinear", align_corners=False, antialias=True).mul_(m).add_(a)

    legs = {"a_tiled": lambda: ctx._export_float(all_s, all_o, outs["a"], None, MEAN, STD, 1 / 255, FILTER_TRIANGLE),
            "b_direct": lambda: ctx._export_float(all_s, all_o, outs["b"], None, MEAN, STD, 1 / 255, FILTER_TRIANGLE_DIRECT),
            "c_plain": lambda: ctx.export_float(all_s, all_o, outs["c"], mean=MEAN, std=STD),
            "d_torch": leg_d}
    return legs, outs, keep


def child_aa(args):
    torch, ctx, all_s, all_o = aa_setup(args)
    from hvqm4_amd._lib import lib
    res = {"pictures": len(all_s), "source": f"{W}x{H}", "reps": args.reps, "rounds": args.rounds}
    for hw in AA_SHAPES:
        for dt in AA_DTYPES:
            legs, outs, keep = aa_legs(torch, ctx, all_s, all_o, hw, dt)
            for fn in legs.values():
                timed(torch, fn, args.warmup)
            rows = {k: [] for k in legs}
            for _ in range(args.rounds):
                for k, fn in legs.items():
                    rows[k].append(round(timed(torch, fn, args.reps), 4))
            out = {k + "_ms": v for k, v in rows.items()}
            out.update({k + "_median_ms": statistics.median(v) for k, v in rows.items()})
            out["tile_rows"] = lib().hvq_resample_tile_rows(W, H, hw[1], hw[0])
            out["bodies_equal_bits"] = bool(torch.equal(outs["a"], outs["b"]))
            out["max_abs_difference_to_torch"] = float((outs["a"].float() - keep["d"].float()).abs().max())
            res[f"{hw[1]}x{hw[0]}_{dt}"] = out
            del legs, outs, keep
            torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(res))


def child_aa_trace(args):
    """legs (a), (b), (c) in a fixed order, `reps` launches each after one warm-up launch: aa_trace_summary reads them by order"""
    torch, ctx, all_s, all_o = aa_setup(args)
    plan = []
    for hw in AA_SHAPES:
        for dt in AA_DTYPES:
            legs, outs, keep = aa_legs(torch, ctx, all_s, all_o, hw, dt)
            for k in ("a_tiled", "b_direct", "c_plain"):
                for _ in range(1 + args.reps):
                    legs[k]()
                torch.cuda.synchronize()
                plan.append([f"{hw[1]}x{hw[0]}_{dt}_{k}", 1 + args.reps])
            del legs, outs, keep
            torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps({"plan": plan}))


def aa_trace_summary(trace_dir, plan):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return {"error": f"no kernel trace under {trace_dir}"}
    rows = []
    with open(files[0], newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name") or row.get("Name") or ""
            if "hvq_yuv_resample_kernel" in name or "hvq_yuv_tensor_kernel" in name:
                rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"]), name.split("(")[0],
                             row.get("VGPR_Count"), row.get("LDS_Block_Size")))
    rows.sort()
    if len(rows) != sum(c for _l, c in plan):
        return {"error": f"{len(rows)} export launches in the trace, {sum(c for _l, c in plan)} planned"}
    res, at = {}, 0
    for label, count in plan:
        part = rows[at + 1:at + count]                                            # without the warm-up launch
        at += count
        d = sorted(r[1] for r in part)
        res[label] = {"kernel": part[0][2], "launches": len(d), "median_us": round(statistics.median(d) / 1e3, 1),
                      "min_us": round(d[0] / 1e3, 1), "max_us": round(d[-1] / 1e3, 1), "lds": part[0][4]}
    return res


def trace_summary(trace_dir, n):
    """median / min of every export kernel in the kernel trace -> share of 8 TB/s"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return {"error": f"no kernel trace under {trace_dir}"}
    dur = {}
    with open(files[0], newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name") or row.get("Name") or ""
            if "hvq_yuv_" in name:
                dur.setdefault(name, []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    src = W * H * 3 // 2
    per_px = {"<float>": 12, "<_Float16>": 6, "<hvq_bf16>": 6, "hvq_yuv_rgb_kernel": 3}
    res = {}
    for name, d in sorted(dur.items()):
        d = sorted(d)
        big = [x for x in d if x > 0.5 * d[-1]]                                   # the 1024-picture launches, not the warm-up of setup
        b = next((v for k, v in per_px.items() if k in name), None)
        if b is None:
            continue
        by = n * (src + b * W * H)
        med = statistics.median(big)
        res[name.split("(")[0]] = {"launches": len(big), "median_us": round(med / 1e3, 1), "min_us": round(big[0] / 1e3, 1), "bytes": by,
                                   "of_peak_median": round(by / (med * 1e-9) / PEAK, 3), "of_peak_best": round(by / (big[0] * 1e-9) / PEAK, 3)}
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
    ap.add_argument("--child", choices=("identity", "route", "aa", "aa_trace"), default=None)
    ap.add_argument("--aa-streams", type=int, default=16, help="streams of 8 resident pictures for the aa steps (16: 128 pictures)")
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--per", type=int, default=8, help="resident pictures per stream")
    ap.add_argument("--distinct", type=int, default=2, help="distinct clips dealt over the streams")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", default="trace,route")
    ap.add_argument("--step-timeout", type=int, default=400)
    ap.add_argument("--out-dir", default="export_float_bench_out")
    args = ap.parse_args()
    if args.child:
        return {"identity": child_identity, "route": child_route, "aa": child_aa, "aa_trace": child_aa_trace}[args.child](args)
    os.makedirs(args.out_dir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    common = ["--streams", str(args.streams), "--per", str(args.per), "--distinct", str(args.distinct), "--reps", str(args.reps),
              "--warmup", str(args.warmup), "--rounds", str(args.rounds), "--aa-streams", str(args.aa_streams)]
    for step in args.steps.split(","):
        print(f"# step {step}", flush=True)
        if step == "trace":
            tdir = os.path.join(args.out_dir, "trace")
            line = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--"] + me + ["--child", "identity"] + common,
                       args.step_timeout, os.path.join(args.out_dir, "trace.log"))
            res = {"calls": json.loads(line), "kernels": trace_summary(tdir, args.streams * args.per)}
        elif step == "route":
            res = json.loads(run(me + ["--child", "route"] + common, args.step_timeout, os.path.join(args.out_dir, "route.log")))
        elif step == "aa":
            res = json.loads(run(me + ["--child", "aa"] + common, args.step_timeout, os.path.join(args.out_dir, "aa.log")))
        elif step == "aa_trace":
            tdir = os.path.join(args.out_dir, "aa_trace")
            line = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--"] + me + ["--child", "aa_trace"] + common,
                       args.step_timeout, os.path.join(args.out_dir, "aa_trace.log"))
            res = aa_trace_summary(tdir, json.loads(line)["plan"])
        else:
            sys.exit(f"unknown step {step}")
        line = json.dumps({step: res})
        print(line, flush=True)
        with open(os.path.join(args.out_dir, step + ".json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
