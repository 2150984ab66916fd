"""Picture checksums (hvq_picture_checksums, Context.picture_checksums) on the GPU: 128 dense 640x480 4:2:0 streams, 8 resident pictures each,
1024 pictures per call.

Two measurements, each a child process of this driver under its own `timeout`; a step that fails ends the run:
  time    (a) picture_checksums, (b) picture_metrics against zeros on the same pictures -- existing code that reads the same bytes once --
          both HIP-event timed on one stream in alternating rounds after a warm-up, and (c) the route the call replaces: read_pictures
          into pinned memory, then zlib.crc32 and zlib.adler32 of every plane and picture on 16 host threads (wall clock: the route is
          host work).  (a) and (c) must give the same values.  Medians over the rounds; the factors (c)/(a) and (a)/(b).
  trace   rocprofv3 --kernel-trace --stats around a child that launches (a) and (b) in a fixed order, one warm-up and `reps` launches
          each.  Kernel times are read from the trace: median with min-max per kernel; bytes = pic_bytes per picture; share of 8 TB/s.
One JSON line per measurement on stdout and in --out-dir.  HVQM4_AMD_LIB names another build of the library (the byte steps and
ablations of hvq_checksum.hip: -DHVQ_CK_STEP=, -DHVQ_CK_ABLATE=); the line says which.  torch is imported before the library, so both
share one HIP runtime."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12
W, H = 640, 480
PIC_BYTES = W * H * 3 // 2
KERNELS = ("hvq_checksum_kernel", "hvq_checksum_finish_kernel", "hvq_metrics_kernel")


def setup(args):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    from tools.export_bench import resident_streams
    ctx = batch.Context(0)
    sids = resident_streams(ctx, "420", args.streams, args.per, args.distinct, W, H)
    a_s = [s for s in sids for _ in range(args.per)]
    a_o = [k for _ in sids for k in range(args.per)]
    return torch, ctx, a_s, a_o


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def host_checksums(pics, threads):
    """zlib on `threads` host threads (zlib releases the GIL): the eight values of every picture, as hvqm4_amd.checksums.of_bytes"""
    from concurrent.futures import ThreadPoolExecutor
    ny, nc = W * H, W * H // 4

    def one(i):
        m = memoryview(pics[i])
        planes = (m[:ny], m[ny:ny + nc], m[ny + nc:])
        return [zlib.crc32(p) for p in planes] + [zlib.crc32(m)] + [zlib.adler32(p) for p in planes] + [zlib.adler32(m)]

    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(one, range(len(pics)), chunksize=max(1, len(pics) // (4 * threads))))


def child_time(args):
    torch, ctx, a_s, a_o = setup(args)
    n = len(a_s)
    out = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    met = torch.empty((n, 3, 4), dtype=torch.int64, device="cuda")
    pinned = ctx.pinned_array((n, PIC_BYTES))
    keep = {}

    def call():
        ctx.picture_checksums(a_s, a_o, out=out)

    def metrics():
        ctx.picture_metrics(a_s, a_o, None, out=met)

    def route():
        ctx.read_pictures(a_s, a_o, out=pinned)
        keep["host"] = host_checksums(pinned, args.threads)

    timed(torch, call, args.warmup)
    timed(torch, metrics, args.warmup)
    route()
    agree = out.cpu().tolist() == keep["host"]
    res = {"size": f"{W}x{H}", "pictures": n, "bytes": n * PIC_BYTES, "reps": args.reps, "rounds": args.rounds, "host_threads": args.threads,
           "library": os.environ.get("HVQM4_AMD_LIB") or "in tree", "checksums_ms": [], "metrics_ms": [], "route_ms": [], "route_read_ms": []}
    for _ in range(args.rounds):
        res["checksums_ms"].append(round(timed(torch, call, args.reps), 4))
        res["metrics_ms"].append(round(timed(torch, metrics, args.reps), 4))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.read_pictures(a_s, a_o, out=pinned)
        t1 = time.perf_counter()
        keep["host"] = host_checksums(pinned, args.threads)
        t2 = time.perf_counter()
        res["route_ms"].append(round((t2 - t0) * 1e3, 3))
        res["route_read_ms"].append(round((t1 - t0) * 1e3, 3))
    for k in ("checksums", "metrics", "route", "route_read"):
        res[k + "_median_ms"] = statistics.median(res[k + "_ms"])
    res["route_over_checksums"] = round(res["route_median_ms"] / res["checksums_median_ms"], 1)
    res["checksums_over_metrics"] = round(res["checksums_median_ms"] / res["metrics_median_ms"], 2)
    res["checksums_gb_per_s"] = round(n * PIC_BYTES / (res["checksums_median_ms"] * 1e-3) / 1e9, 1)
    res["values_agree_with_zlib"] = bool(agree)
    ctx.close()
    print(json.dumps(res))


def child_trace(args):
    """the launches the trace is taken of, in the order trace_summary reads them by"""
    torch, ctx, a_s, a_o = setup(args)
    n = len(a_s)
    out = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    met = torch.empty((n, 3, 4), dtype=torch.int64, device="cuda")
    for _ in range(1 + args.reps):
        ctx.picture_checksums(a_s, a_o, out=out)
    torch.cuda.synchronize()
    for _ in range(1 + args.reps):
        ctx.picture_metrics(a_s, a_o, None, out=met)
    torch.cuda.synchronize()
    ctx.close()
    print(json.dumps({"launches": 1 + args.reps, "pictures": n}))


def trace_summary(trace_dir, plan):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return {"error": f"no kernel trace under {trace_dir}"}
    rows = {k: [] for k in KERNELS}
    with open(files[0], newline="") as f:
        for row in csv.DictReader(f):
            name = (row.get("Kernel_Name") or row.get("Name") or "").split("(")[0].strip()
            name = name[:-3] if name.endswith(".kd") else name
            for k in KERNELS:
                if name.split(" ")[-1] == k:
                    rows[k].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"]),
                                    row.get("VGPR_Count"), row.get("LDS_Block_Size"), row.get("Scratch_Size")))
    res = {"pictures": plan["pictures"], "library": os.environ.get("HVQM4_AMD_LIB") or "in tree"}
    for k in KERNELS:
        r = sorted(rows[k])
        if len(r) != plan["launches"]:
            return {"error": f"{len(r)} launches of {k} in the trace, {plan['launches']} planned"}
        d = sorted(x[1] for x in r[1:])                                           # without the warm-up launch
        med = statistics.median(d)
        by = plan["pictures"] * PIC_BYTES
        res[k] = {"launches": len(d), "median_us": round(med / 1e3, 1), "min_us": round(d[0] / 1e3, 1), "max_us": round(d[-1] / 1e3, 1),
                  "vgprs": r[0][2], "lds": r[0][3], "scratch": r[0][4]}
        if k != "hvq_checksum_finish_kernel":
            res[k].update({"bytes": by, "of_peak_median": round(by / (med * 1e-9) / PEAK, 3)})
    res["checksum_over_metrics_kernel"] = round((res[KERNELS[0]]["median_us"] + res[KERNELS[1]]["median_us"]) / res[KERNELS[2]]["median_us"], 2)
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
    ap.add_argument("--child", choices=("time", "trace"), default=None)
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--per", type=int, default=8, help="resident pictures per stream")
    ap.add_argument("--distinct", type=int, default=2, help="distinct clips dealt over the streams")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the route the call replaces")
    ap.add_argument("--steps", default="time,trace")
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out-dir", default="checksum_bench_out")
    args = ap.parse_args()
    if args.child:
        return {"time": child_time, "trace": child_trace}[args.child](args)
    os.makedirs(args.out_dir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    common = ["--streams", str(args.streams), "--per", str(args.per), "--distinct", str(args.distinct), "--reps", str(args.reps),
              "--warmup", str(args.warmup), "--rounds", str(args.rounds), "--threads", str(args.threads)]
    for step in args.steps.split(","):
        print(f"# step {step}", flush=True)
        if step == "time":
            res = json.loads(run(me + ["--child", "time"] + common, args.step_timeout, os.path.join(args.out_dir, "time.log")))
        elif step == "trace":
            tdir = os.path.join(args.out_dir, "trace")
            line = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--"] + me + ["--child", "trace"] + common,
                       args.step_timeout, os.path.join(args.out_dir, "trace.log"))
            res = trace_summary(tdir, json.loads(line))
            if "error" in res:
                sys.exit(f"trace: {res['error']}")
        else:
            sys.exit(f"unknown step {step}")
        line = json.dumps({step: res})
        print(line, flush=True)
        with open(os.path.join(args.out_dir, step + ".json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
