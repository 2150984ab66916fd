"""Picture checksums (hvq_picture_checksums, Context.picture_checksums) on the GPU: 128 dense 640x480 4:2:0 streams, 8 resident pictures each,
1024 pictures per call.

Two measurements (steps of tools/benchlib.py):
  time    (a) picture_checksums, (b) picture_metrics against zeros on the same pictures -- existing code that reads the same bytes once --
          both HIP-event timed on one stream in alternating rounds after a warm-up, and (c) the route the call replaces: read_pictures
          into pinned memory, then zlib.crc32 and zlib.adler32 of every plane and picture on 16 host threads (wall clock: the route is
          host work).  (a) and (c) must give the same values.  Medians over the rounds; the factors (c)/(a) and (a)/(b).
  trace   the kernel trace of a child that launches (a) and (b) in a fixed order, one warm-up and `reps` launches
          each.  Kernel times are read from the trace: median with min-max per kernel; bytes = pic_bytes per picture; share of 8 TB/s.
HVQM4_AMD_LIB names another build of the library (the byte steps and ablations of hvq_checksum.hip: -DHVQ_CK_STEP=, -DHVQ_CK_ABLATE=);
the line says which."""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.benchlib import PEAK, add_common_arguments, drive, launch_stats, picture_lists, read_per_kernel, resident, resources, timed  # noqa: E402

W, H = 640, 480
PIC_BYTES = W * H * 3 // 2
KERNELS = ("hvq_checksum_kernel", "hvq_checksum_finish_kernel", "hvq_metrics_kernel")


def setup(args):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    a_s, a_o = picture_lists(resident(ctx, preset="dense", streams=args.streams, per=args.per, distinct=args.distinct), args.per)
    return torch, ctx, a_s, a_o


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
    """the launches the trace is taken of: a call launches hvq_checksum_kernel and hvq_checksum_finish_kernel in turn"""
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


def trace_summary(trace_dir, plan, _earlier=None):
    cut = read_per_kernel(trace_dir, KERNELS, plan["launches"])
    if "error" in cut:
        return cut
    res = {"pictures": plan["pictures"], "library": os.environ.get("HVQM4_AMD_LIB") or "in tree"}
    for k, r in cut.items():
        d = [l.ns for l in r[1:]]                                                 # without the warm-up launch
        by = plan["pictures"] * PIC_BYTES
        res[k] = {**launch_stats(d), **resources(r[0])}
        if k != "hvq_checksum_finish_kernel":
            res[k].update({"bytes": by, "of_peak_median": round(by / (statistics.median(d) * 1e-9) / PEAK, 3)})
    res["checksum_over_metrics_kernel"] = round((res[KERNELS[0]]["median_us"] + res[KERNELS[1]]["median_us"]) / res[KERNELS[2]]["median_us"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    add_common_arguments(ap, children=("time", "trace"), reps=30, warmup=3, rounds=5, steps="time,trace", out_dir="checksum_bench_out")
    ap.add_argument("--threads", type=int, default=16, help="host threads of the route the call replaces")
    args = ap.parse_args()
    if args.child:
        return {"time": child_time, "trace": child_trace}[args.child](args)
    drive(args, {"time": ("time", None), "trace": ("trace", trace_summary)}, [sys.executable, os.path.abspath(__file__)])


if __name__ == "__main__":
    main()
