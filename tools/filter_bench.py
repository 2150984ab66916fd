"""Filtered pictures in slot layout (hvq_filter_pictures) on the GPU.

Two measurements, each a child process of this driver under its own `timeout`; a step that fails ends the run:
  calls   128 640x480 4:2:0 streams, 8 resident pictures each, 1024 pictures per call, on natural content, through the binomial 3 x 3, a
          Gaussian of sigma 1.5 (radius 5), a Gaussian of radius 15, the Sobel magnitude on luma only, unsharp masking on luma only and
          the identity: (a) filter_pictures, (b) scale_pictures to the pictures' own geometry on the same pictures -- it reads and writes
          the same bytes: the memory floor of this operation --, (c) picture_metrics against zeros and (d) a torch route on a device copy
          of the same pictures: per plane a float view, F.pad(mode="replicate"), two F.conv2d per term, rounding, clamp, cast,
          concatenation.  HIP-event timed per call on one stream in alternating rounds after a warm-up; medians over the rounds; the
          factors (a)/(b) and (d)/(a).  (a) must equal hvqm4_amd.filters on pictures read back, and so must the torch route.
  trace   rocprofv3 --kernel-trace --stats around a child that launches filter_pictures per filter, scale_pictures (identity) and
          picture_metrics in a fixed order, one warm-up and `reps` launches each.  Kernel times are read from the trace: median with
          min-max per filter, the bytes read and written over them, and the ratios to the scale identity and to the metrics kernel.
One JSON line per measurement on stdout and in --out-dir.  torch is imported before the library, so both share one HIP runtime."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PEAK = 8.0e12
W, H = 640, 480
SRC = (W, H, 2, 2)
PIC_BYTES = W * H * 3 // 2


def the_filters():
    from hvqm4_amd import filters as F
    return [("binomial3", F.binomial(3)), ("gauss1.5_r5", F.gaussian(1.5, 5)), ("gauss5_r15", F.gaussian(5.0, 15)),
            ("sobelmag_luma", F.luma_only(F.gradient_magnitude("sobel"))), ("unsharp_luma", F.luma_only(F.unsharp(1.0, Fraction(1, 2)))),
            ("identity", F.identity())]


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def torch_route(torch, copy, filt):
    """the filtered pictures the way a pipeline without the call gets them: planar float32 where every partial sum (an integer of at most
    255 gain) stays below 2^24 and float64 otherwise, replicate padding, two convolutions per term"""
    from hvqm4_amd import filters as F
    from hvqm4_amd import scale
    tf = torch.nn.functional
    n = copy.shape[0]
    out, at = [], 0
    for p, (nx, ny, _mx, _my) in enumerate(scale.plane_sizes(SRC, SRC)):
        pf = filt.chroma if p else filt.luma
        raw = copy[:, at:at + nx * ny]
        at += nx * ny
        if F.is_identity(pf):
            out.append(raw)
            continue
        dt = torch.float64 if F.gain(pf) * 255 >= 1 << 24 else torch.float32
        plane = raw.to(dt).view(n, 1, ny, nx)
        t = []
        for term in pf.terms:
            x = tf.pad(plane, (term.rx, term.rx, term.ry, term.ry), mode="replicate")
            x = tf.conv2d(x, torch.tensor(term.wx, dtype=dt, device="cuda").view(1, 1, 1, -1))
            t.append(tf.conv2d(x, torch.tensor(term.wy, dtype=dt, device="cuda").view(1, 1, -1, 1)))
        if len(t) == 1:
            t.append(torch.zeros_like(t[0]))
        s = t[0] + t[1] if pf.combine == F.SUM else (t[0] + t[1]).abs() if pf.combine == F.ABS_SUM else t[0].abs() + t[1].abs()
        half = 1 << (pf.shift - 1) if pf.shift else 0
        out.append((torch.floor((s + half) / (1 << pf.shift)) + pf.bias).clamp_(0, 255).to(torch.uint8).view(n, -1))
    return torch.cat(out, dim=1)


def setup(args):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    from scale_bench import resident
    ctx = batch.Context(0)
    sids = resident(ctx, args.contents.split(",")[0], args.streams, args.per, args.distinct)
    a_s = [s for s in sids for _ in range(args.per)]
    a_o = [k for _ in sids for k in range(args.per)]
    return torch, ctx, a_s, a_o


def child_calls(args):
    import numpy as np
    from hvqm4_amd import filters as F
    torch, ctx, a_s, a_o = setup(args)
    n = len(a_s)
    res = {"size": f"{W}x{H}", "pictures": n, "reps": args.reps, "rounds": args.rounds, "content": args.contents.split(",")[0], "filters": {}}
    met = torch.empty((n, 3, 4), dtype=torch.int64, device="cuda")
    copy = torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
    out = torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
    sout = torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
    probe = list(range(0, n, max(1, n // 8)))
    host = {i: ctx.read_picture(a_s[i], a_o[i]) for i in probe}
    for at in range(0, n, 64):                                  # the device copy the torch route works on
        copy[at:at + 64] = torch.from_numpy(np.stack([ctx.read_picture(a_s[i], a_o[i]) for i in range(at, min(n, at + 64))])).cuda()
    metrics = lambda: ctx.picture_metrics(a_s, a_o, None, out=met)
    ident = lambda: ctx.scale_pictures(a_s, a_o, (W, H), out=sout)
    timed(torch, metrics, args.warmup)
    timed(torch, ident, args.warmup)
    for label, f in the_filters():
        call = lambda: ctx.filter_pictures(a_s, a_o, f, out=out)
        route = lambda: torch_route(torch, copy, f)
        timed(torch, call, args.warmup)
        got = out.cpu().numpy()
        agree = all(np.array_equal(got[i], F.of_picture(host[i], SRC, f)) for i in probe)
        try:                                                    # a torch build without this convolution: the route is reported as missing
            timed(torch, route, 1)
            off = int((route().to(torch.int16) - out.to(torch.int16)).abs().max())
        except RuntimeError as e:
            off, route = str(e)[:200], None
        r = {"filter_ms": [], "scale_identity_ms": [], "metrics_ms": [], "torch_ms": []}
        for _ in range(args.rounds):
            r["filter_ms"].append(round(timed(torch, call, args.reps), 4))
            r["scale_identity_ms"].append(round(timed(torch, ident, args.reps), 4))
            r["metrics_ms"].append(round(timed(torch, metrics, args.reps), 4))
            if route:
                r["torch_ms"].append(round(timed(torch, route, max(1, args.reps // 5)), 4))
        for k in ("filter", "scale_identity", "metrics", "torch"):
            r[k + "_median_ms"] = statistics.median(r[k + "_ms"]) if r[k + "_ms"] else None
        r["filter_over_scale_identity"] = round(r["filter_median_ms"] / r["scale_identity_median_ms"], 2)
        r["torch_over_filter"] = round(r["torch_median_ms"] / r["filter_median_ms"], 1) if route else None
        r["bytes_read_and_written"] = 2 * n * PIC_BYTES
        r["gb_per_s"] = round(r["bytes_read_and_written"] / (r["filter_median_ms"] * 1e-3) / 1e9, 1)
        r["equal_host_module"] = bool(agree)
        r["torch_route_largest_difference"] = off
        r["gain"] = [F.gain(f.luma), F.gain(f.chroma)]
        r["radii"] = [[(t.rx, t.ry) for t in p.terms] for p in (f.luma, f.chroma)]
        res["filters"][label] = r
    ctx.close()
    print(json.dumps(res))


def child_trace(args):
    """the launches the trace is taken of: per filter 1 + reps of the filter kernel, then of the scale kernel (identity), then of the
    metrics kernel"""
    torch, ctx, a_s, a_o = setup(args)
    n = len(a_s)
    out = torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")
    for _label, f in the_filters():
        for _ in range(1 + args.reps):
            ctx.filter_pictures(a_s, a_o, f, out=out)
        torch.cuda.synchronize()
    for _ in range(1 + args.reps):
        ctx.scale_pictures(a_s, a_o, (W, H), out=out)
    torch.cuda.synchronize()
    met = torch.empty((n, 3, 4), dtype=torch.int64, device="cuda")
    for _ in range(1 + args.reps):
        ctx.picture_metrics(a_s, a_o, None, out=met)
    torch.cuda.synchronize()
    ctx.close()
    print(json.dumps({"launches": 1 + args.reps, "pictures": n, "content": args.contents.split(",")[0]}))


def trace_summary(trace_dir, plan):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return {"error": f"no kernel trace under {trace_dir}"}
    rows = {"hvq_filter_kernel": [], "hvq_scale_kernel": [], "hvq_metrics_kernel": []}
    with open(files[0], newline="") as f:
        for row in csv.DictReader(f):
            name = (row.get("Kernel_Name") or row.get("Name") or "").split("(")[0].strip()
            name = name[:-3] if name.endswith(".kd") else name
            k = name.split(" ")[-1]
            if k in rows:
                rows[k].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"]), row.get("VGPR_Count"), row.get("LDS_Block_Size"),
                                row.get("Scratch_Size")))
    per = plan["launches"]
    names = [label for label, _f in the_filters()]
    fl, sc, mt = sorted(rows["hvq_filter_kernel"]), sorted(rows["hvq_scale_kernel"]), sorted(rows["hvq_metrics_kernel"])
    if len(fl) != per * len(names) or len(sc) != per or len(mt) != per:
        return {"error": f"{len(fl)} filter, {len(sc)} scale and {len(mt)} metrics launches in the trace, {per * len(names)}, {per} and {per} planned"}

    def stats(r):
        d = sorted(x[1] for x in r[1:])                                               # without the warm-up launch
        return {"launches": len(d), "median_us": round(statistics.median(d) / 1e3, 1), "min_us": round(d[0] / 1e3, 1), "max_us": round(d[-1] / 1e3, 1)}

    res = {"pictures": plan["pictures"], "content": plan["content"], "vgprs": fl[0][2], "lds": fl[0][3], "scratch": fl[0][4]}
    m, s = stats(mt), stats(sc)
    m["bytes"] = plan["pictures"] * PIC_BYTES
    s["bytes"] = 2 * plan["pictures"] * PIC_BYTES
    for d in (m, s):
        d["of_peak_median"] = round(d["bytes"] / (d["median_us"] * 1e-6) / PEAK, 3)
    res["hvq_metrics_kernel"], res["hvq_scale_kernel_identity"] = m, s
    for i, label in enumerate(names):
        t = stats(fl[i * per:(i + 1) * per])
        t["bytes"] = 2 * plan["pictures"] * PIC_BYTES
        t["of_peak_median"] = round(t["bytes"] / (t["median_us"] * 1e-6) / PEAK, 3)
        t["over_scale_identity_kernel"] = round(t["median_us"] / s["median_us"], 2)
        t["over_metrics_kernel"] = round(t["median_us"] / m["median_us"], 2)
        res[label] = t
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
    ap.add_argument("--contents", default="natural")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", default="calls,trace")
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out-dir", default="filter_bench_out")
    ap.add_argument("--out", default=None, help="all measurements as one JSON file (profiles/filter_bench.json)")
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
