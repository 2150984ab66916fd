"""Scaled pictures in slot layout (hvq_scale_pictures) on the GPU.

Two measurements, each a child process of this driver under its own `timeout`; a step that fails ends the run:
  calls   128 640x480 4:2:0 streams, 8 resident pictures each, 1024 pictures per call, on natural and dense content, scaled to 320x240
          (ratio 2), 160x120 (4), 224x168 (2.857), 24x16 (near the limit of 32), 640x480 (identity) and 640x480 at 4:4:4 (chroma
          enlargement): (a) scale_pictures, (b) picture_metrics against zeros on the same pictures -- it reads the same 1.5 B/px and
          writes almost nothing: the memory-bound floor of a reduction -- and (c) a torch route on a device copy of the same pictures: per
          plane adaptive_avg_pool2d on a float view, rounding, concatenation.  HIP-event timed per call on one stream in alternating
          rounds after a warm-up; medians over the rounds; the factors (a)/(b) and (c)/(a).  (a) must equal hvqm4_amd.scale on pictures
          read back; the torch route's largest difference from it is reported (float means, another rounding).
  trace   rocprofv3 --kernel-trace --stats around a child that launches scale_pictures per shape and picture_metrics in a fixed order,
          one warm-up and `reps` launches each.  Kernel times are read from the trace: median with min-max per shape, the bytes the shape
          reads and writes over them, and the ratio to the metrics kernel.
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
SRC = (W, H, 2, 2)
PIC_BYTES = W * H * 3 // 2
SHAPES = [("320x240", (320, 240, 2, 2)), ("160x120", (160, 120, 2, 2)), ("224x168", (224, 168, 2, 2)), ("24x16", (24, 16, 2, 2)),
          ("640x480", (640, 480, 2, 2)), ("640x480_444", (640, 480, 1, 1))]


def resident(ctx, preset, streams, per, distinct):
    from hvqm4_amd.container import video_pictures
    from hvqm4_amd.synth import SynthConfig, make_clip
    clips = [make_clip(SynthConfig(width=W, height=H, version="1.5", gop="IPBBPBBPBBPBBPBB", seed=1000 + i, preset=preset, sampling="420"))
             for i in range(distinct)]
    pics = [[(ft, bytes(p)) for ft, _d, p in video_pictures(c.data)][:per] for c in clips]
    sids = [ctx.open_stream(W, H, 2, 2, True, per + 2) for _ in range(streams)]
    a_s, a_t, a_p = [], [], []
    for k in range(per):
        for i, sid in enumerate(sids):
            ft, p = pics[i % distinct][k]
            a_s.append(sid); a_t.append(ft); a_p.append(p)
    ctx.submit_many(a_s, a_t, a_p, threads=16)
    ctx.flush()
    ctx.sync()
    return sids


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def torch_route(torch, copy, dst):
    """the scaled pictures the way a pipeline without the call gets them: float means per plane, rounded, concatenated"""
    from hvqm4_amd import scale
    n = copy.shape[0]
    out, at = [], 0
    for p, (nx, ny, mx, my) in enumerate(scale.plane_sizes(SRC, dst)):
        plane = copy[:, at:at + nx * ny].float().view(n, 1, ny, nx)
        at += nx * ny
        out.append(torch.floor(torch.nn.functional.adaptive_avg_pool2d(plane, (my, mx)) + 0.5).to(torch.uint8).view(n, -1))
    return torch.cat(out, dim=1)


def child_calls(args):
    import numpy as np
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch, scale
    res = {"size": f"{W}x{H}", "pictures": args.streams * args.per, "reps": args.reps, "rounds": args.rounds, "contents": {}}
    for preset in args.contents.split(","):
        ctx = batch.Context(0)
        sids = resident(ctx, preset, args.streams, args.per, args.distinct)
        a_s = [s for s in sids for _ in range(args.per)]
        a_o = [k for _ in sids for k in range(args.per)]
        n = len(a_s)
        met = torch.empty((n, 3, 4), dtype=torch.int64, device="cuda")
        copy = torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
        probe = list(range(0, n, max(1, n // 8)))
        host = {i: ctx.read_picture(a_s[i], a_o[i]) for i in probe}
        for at in range(0, n, 64):                                  # the device copy the torch route works on
            copy[at:at + 64] = torch.from_numpy(np.stack([ctx.read_picture(a_s[i], a_o[i]) for i in range(at, min(n, at + 64))])).cuda()
        metrics = lambda: ctx.picture_metrics(a_s, a_o, None, out=met)
        timed(torch, metrics, args.warmup)
        shapes = {}
        for label, dst in SHAPES:
            out = torch.empty((n, scale.nbytes(*dst)), dtype=torch.uint8, device="cuda")
            call = lambda: ctx.scale_pictures(a_s, a_o, dst[:2], dst[2:], out=out)
            route = lambda: torch_route(torch, copy, dst)
            timed(torch, call, args.warmup)
            timed(torch, route, 1)
            got = out.cpu().numpy()
            agree = all(np.array_equal(got[i], scale.of_picture(host[i], SRC, dst)) for i in probe)
            off = int((route().to(torch.int16) - out.to(torch.int16)).abs().max())
            r = {"scale_ms": [], "metrics_ms": [], "torch_ms": []}
            for _ in range(args.rounds):
                r["scale_ms"].append(round(timed(torch, call, args.reps), 4))
                r["metrics_ms"].append(round(timed(torch, metrics, args.reps), 4))
                r["torch_ms"].append(round(timed(torch, route, max(1, args.reps // 5)), 4))
            for k in ("scale", "metrics", "torch"):
                r[k + "_median_ms"] = statistics.median(r[k + "_ms"])
            r["scale_over_metrics"] = round(r["scale_median_ms"] / r["metrics_median_ms"], 2)
            r["torch_over_scale"] = round(r["torch_median_ms"] / r["scale_median_ms"], 1)
            r["bytes_read_and_written"] = n * (PIC_BYTES + scale.nbytes(*dst))
            r["gb_per_s"] = round(r["bytes_read_and_written"] / (r["scale_median_ms"] * 1e-3) / 1e9, 1)
            r["equal_host_module"] = bool(agree)
            r["torch_route_largest_difference"] = off
            r["bodies"] = [scale.body(*s) for s in scale.plane_sizes(SRC, dst)]
            shapes[label] = r
        res["contents"][preset] = shapes
        ctx.close()
    print(json.dumps(res))


def child_trace(args):
    """the launches the trace is taken of: per shape 1 + reps of the scale kernel, then 1 + reps of the metrics kernel"""
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch, scale
    ctx = batch.Context(0)
    sids = resident(ctx, args.contents.split(",")[0], args.streams, args.per, args.distinct)
    a_s = [s for s in sids for _ in range(args.per)]
    a_o = [k for _ in sids for k in range(args.per)]
    n = len(a_s)
    for _label, dst in SHAPES:
        out = torch.empty((n, scale.nbytes(*dst)), dtype=torch.uint8, device="cuda")
        for _ in range(1 + args.reps):
            ctx.scale_pictures(a_s, a_o, dst[:2], dst[2:], out=out)
        torch.cuda.synchronize()
    met = torch.empty((n, 3, 4), dtype=torch.int64, device="cuda")
    for _ in range(1 + args.reps):
        ctx.picture_metrics(a_s, a_o, None, out=met)
    torch.cuda.synchronize()
    ctx.close()
    print(json.dumps({"launches": 1 + args.reps, "pictures": n, "content": args.contents.split(",")[0]}))


def trace_summary(trace_dir, plan):
    from hvqm4_amd import scale
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return {"error": f"no kernel trace under {trace_dir}"}
    rows = {"hvq_scale_kernel": [], "hvq_metrics_kernel": []}
    with open(files[0], newline="") as f:
        for row in csv.DictReader(f):
            name = (row.get("Kernel_Name") or row.get("Name") or "").split("(")[0].strip()
            name = name[:-3] if name.endswith(".kd") else name
            k = name.split(" ")[-1]
            if k in rows:
                rows[k].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"]), row.get("VGPR_Count"), row.get("LDS_Block_Size"),
                                row.get("Scratch_Size")))
    per = plan["launches"]
    sc, mt = sorted(rows["hvq_scale_kernel"]), sorted(rows["hvq_metrics_kernel"])
    if len(sc) != per * len(SHAPES) or len(mt) != per:
        return {"error": f"{len(sc)} scale and {len(mt)} metrics launches in the trace, {per * len(SHAPES)} and {per} planned"}

    def stats(r):
        d = sorted(x[1] for x in r[1:])                                               # without the warm-up launch
        return {"launches": len(d), "median_us": round(statistics.median(d) / 1e3, 1), "min_us": round(d[0] / 1e3, 1), "max_us": round(d[-1] / 1e3, 1)}

    res = {"pictures": plan["pictures"], "content": plan["content"], "vgprs": sc[0][2], "lds": sc[0][3], "scratch": sc[0][4]}
    m = stats(mt)
    m["bytes"] = plan["pictures"] * PIC_BYTES
    m["of_peak_median"] = round(m["bytes"] / (m["median_us"] * 1e-6) / PEAK, 3)
    res["hvq_metrics_kernel"] = m
    for i, (label, dst) in enumerate(SHAPES):
        s = stats(sc[i * per:(i + 1) * per])
        s["bytes"] = plan["pictures"] * (PIC_BYTES + scale.nbytes(*dst))
        s["of_peak_median"] = round(s["bytes"] / (s["median_us"] * 1e-6) / PEAK, 3)
        s["over_metrics_kernel"] = round(s["median_us"] / m["median_us"], 2)
        res[label] = s
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
    ap.add_argument("--contents", default="natural,dense")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", default="calls,trace")
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out-dir", default="scale_bench_out")
    ap.add_argument("--out", default=None, help="all measurements as one JSON file (profiles/scale_bench.json)")
    args = ap.parse_args()
    if args.child:
        return {"calls": child_calls, "trace": child_trace}[args.child](args)
    os.makedirs(args.out_dir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    common = ["--streams", str(args.streams), "--per", str(args.per), "--distinct", str(args.distinct), "--reps", str(args.reps), "--warmup", str(args.warmup),
              "--rounds", str(args.rounds), "--contents", args.contents]
    everything = {}
    for step in args.steps.split(","):
        print(f"# step {step}", flush=True)
        if step == "calls":
            res = json.loads(run(me + ["--child", step] + common, args.step_timeout, os.path.join(args.out_dir, step + ".log")))
        elif step == "trace":
            tdir = os.path.join(args.out_dir, "trace")
            line = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--"] + me + ["--child", "trace"] + common,
                       args.step_timeout, os.path.join(args.out_dir, "trace.log"))
            res = trace_summary(tdir, json.loads(line))
            if "error" in res:
                sys.exit(f"trace: {res['error']}")
        else:
            sys.exit(f"unknown step {step}")
        everything[step] = res
        line = json.dumps({step: res})
        print(line, flush=True)
        with open(os.path.join(args.out_dir, step + ".json"), "w") as f:
            f.write(line + "\n")
        if args.out:
            with open(args.out, "w") as f:
                json.dump(everything, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
