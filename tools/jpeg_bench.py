"""JPEG files of resident pictures (hvq_encode_jpeg, Context.encode_jpeg) on the GPU: 128 streams of 640x480 4:2:0, 8 resident pictures
each, 1024 pictures per call at quality 90, for the bench's dense and natural presets.

Two measurements, each a child process of this driver under its own `timeout`; a step that fails ends the run:
  calls   in alternating rounds: (a) the call, HIP-event timed on one stream, into buffers allocated once; (b) picture_metrics on the same
          pictures, the memory-bound yardstick (it reads every sample once); (c) the host route the call replaces: read_pictures of the same
          pictures into pinned memory (host clock: the call synchronises), and -- when Pillow is installed -- its JPEG encoder at the same
          quality and subsampling on 16 host threads over the planes read back (host clock; the chroma planes are repeated to full size
          first, the only form Pillow's encoder takes).  Without Pillow the PCIe time of read_pictures alone is the floor of the host route.
          The first files of the call are compared with hvqm4_amd.jpeg.encode of the pictures read back before anything is timed; the
          output bytes of a call are reported.
  trace   rocprofv3 --kernel-trace --stats around a child that makes `reps` calls per preset after a warm-up.  Kernel times per launch of
          a call (measure / lay out / emit) are read from the trace: median with min-max.
One JSON line per measurement on stdout and in --out-dir; --save merges them into one file (profiles/jpeg_bench.json).  torch is imported
before the library, so both share one HIP runtime."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 640, 480
PIC_BYTES = W * H * 3 // 2
QUALITY = 90
PRESETS = ["dense", "natural"]
LAUNCHES = ["measure", "layout", "emit"]


def resident_streams(ctx, preset, streams, per, distinct):
    """tools/export_bench.py's resident_streams for one of the bench's presets"""
    from hvqm4_amd.container import video_pictures
    from hvqm4_amd.synth import SynthConfig, make_clip
    clips = [make_clip(SynthConfig(width=W, height=H, version="1.5", gop="IPBBPBBPBBPBBPBB", seed=1000 + i, preset=preset, sampling="420")) for i in range(distinct)]
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


def setup(args):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    work = {}
    for preset in PRESETS:
        sids = resident_streams(ctx, preset, args.streams, args.per, args.distinct)
        work[preset] = ([s for s in sids for _ in range(args.per)], [k for _ in sids for k in range(args.per)])
    n = args.streams * args.per
    out = [torch.empty(2 * PIC_BYTES + 1024, dtype=torch.uint8, device="cuda") for _ in range(n)]
    lengths = torch.empty(n, dtype=torch.int64, device="cuda")
    return torch, ctx, work, out, lengths


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def pillow_encode(pics, threads):
    """Pillow's encoder over pictures read back (uint8 [n, PIC_BYTES]) -> (seconds, bytes), None without Pillow"""
    try:
        from PIL import Image
    except ImportError:
        return None
    import io
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np

    def one(p):
        y = p[:W * H].reshape(H, W)
        u = p[W * H:W * H + W * H // 4].reshape(H // 2, W // 2)
        v = p[W * H + W * H // 4:].reshape(H // 2, W // 2)
        full = np.stack([y, np.repeat(np.repeat(u, 2, 0), 2, 1), np.repeat(np.repeat(v, 2, 0), 2, 1)], -1)
        bio = io.BytesIO()
        Image.fromarray(full, "YCbCr").save(bio, "JPEG", quality=QUALITY, subsampling=2)
        return bio.tell()
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        sizes = list(ex.map(one, pics))
    return time.perf_counter() - t0, sum(sizes)


def child_calls(args):
    from hvqm4_amd import jpeg
    torch, ctx, work, out, lengths = setup(args)
    n = len(out)
    res = {"size": f"{W}x{H}", "pictures": n, "quality": QUALITY, "reps": args.reps, "rounds": args.rounds, "presets": {}}
    pinned = ctx.pinned_array((n, PIC_BYTES))
    for preset, (a_s, a_o) in work.items():
        call = lambda: ctx.encode_jpeg(a_s, a_o, quality=QUALITY, out=out, lengths=lengths)
        call()
        torch.cuda.synchronize()
        got = jpeg.files(out[:4], lengths[:4])
        back = ctx.read_pictures(a_s[:4], a_o[:4])
        if got != [jpeg.encode(back[i], W, H, QUALITY) for i in range(4)]:
            sys.exit(f"{preset}: the files are not hvqm4_amd.jpeg.encode's: nothing is timed")
        total = int(lengths.sum().item())
        met = lambda: ctx.picture_metrics(a_s, a_o)
        for fn in (call, met):
            timed(torch, fn, args.warmup)
        ms = {"encode_jpeg": [], "picture_metrics": [], "read_pictures": []}
        for _ in range(args.rounds):
            ms["encode_jpeg"].append(round(timed(torch, call, args.reps), 4))
            ms["picture_metrics"].append(round(timed(torch, met, args.reps), 4))
            t0 = time.perf_counter()
            ctx.read_pictures(a_s, a_o, out=pinned)
            ms["read_pictures"].append(round((time.perf_counter() - t0) * 1e3, 3))
        r = {"ms": ms, "median_ms": {k: statistics.median(v) for k, v in ms.items()}, "output_bytes": total, "bytes_per_picture": round(total / n),
             "compression": round(n * PIC_BYTES / total, 2)}
        pil = pillow_encode(pinned, 16)
        if pil is None:
            r["pillow"] = "Pillow is not installed here: read_pictures alone is the floor of the host route"
            r["host_route_ms"] = r["median_ms"]["read_pictures"]
        else:
            r["pillow_16_threads_ms"], r["pillow_output_bytes"] = round(pil[0] * 1e3, 1), pil[1]
            r["host_route_ms"] = round(r["median_ms"]["read_pictures"] + pil[0] * 1e3, 1)
        r["host_route_over_call"] = round(r["host_route_ms"] / r["median_ms"]["encode_jpeg"], 1)
        r["call_over_picture_metrics"] = round(r["median_ms"]["encode_jpeg"] / r["median_ms"]["picture_metrics"], 1)
        res["presets"][preset] = r
    ctx.close()
    print(json.dumps(res))


def child_trace(args):
    """the launches the trace is taken of, in the order trace_summary reads them by"""
    torch, ctx, work, out, lengths = setup(args)
    plan = []
    for preset, (a_s, a_o) in work.items():
        for _ in range(1 + args.reps):
            ctx.encode_jpeg(a_s, a_o, quality=QUALITY, out=out, lengths=lengths)
        torch.cuda.synchronize()
        plan.append([preset, 1 + args.reps])
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
            if "hvq_jpeg_" in name:
                rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"]), name.split("(")[0],
                             row.get("VGPR_Count"), row.get("LDS_Block_Size"), row.get("Scratch_Size")))
    rows.sort()
    if len(rows) != 3 * sum(p[1] for p in plan):
        return {"error": f"{len(rows)} JPEG launches in the trace, {3 * sum(p[1] for p in plan)} planned"}
    res, at = {}, 0
    for preset, count in plan:
        part = rows[at + 3:at + 3 * count]                                        # without the warm-up call
        at += 3 * count
        res[preset] = {}
        for i, lab in enumerate(LAUNCHES):
            mine = part[i::3]
            if ("layout" in mine[0][2]) != (lab == "layout"):
                return {"error": f"launch {i} of a call is {mine[0][2]}"}
            d = sorted(r[1] for r in mine)
            res[preset][lab] = {"kernel": mine[0][2], "launches": len(d), "median_us": round(statistics.median(d) / 1e3, 1), "min_us": round(d[0] / 1e3, 1),
                                "max_us": round(d[-1] / 1e3, 1), "vgprs": mine[0][3], "lds": mine[0][4], "scratch": mine[0][5]}
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", default="calls,trace")
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--out-dir", default="jpeg_bench_out")
    ap.add_argument("--save", default=None, help="write all steps as one JSON file")
    args = ap.parse_args()
    if args.child:
        return {"calls": child_calls, "trace": child_trace}[args.child](args)
    os.makedirs(args.out_dir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    common = ["--streams", str(args.streams), "--per", str(args.per), "--distinct", str(args.distinct), "--reps", str(args.reps),
              "--warmup", str(args.warmup), "--rounds", str(args.rounds)]
    merged = {}
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
        merged[step] = res
        line = json.dumps({step: res})
        print(line, flush=True)
        with open(os.path.join(args.out_dir, step + ".json"), "w") as f:
            f.write(line + "\n")
    if args.save:
        with open(args.save, "w") as f:
            json.dump(merged, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
