"""JPEG files of resident pictures (hvq_encode_jpeg, Context.encode_jpeg) on the GPU: 128 streams of 640x480 4:2:0, 8 resident pictures
each, 1024 pictures per call at quality 90, for the bench's dense and natural presets.

Two measurements (steps of tools/benchlib.py):
  calls   in alternating rounds: (a) the call, HIP-event timed on one stream, into buffers allocated once; (b) picture_metrics on the same
          pictures, the memory-bound yardstick (it reads every sample once); (c) the host route the call replaces: read_pictures of the same
          pictures into pinned memory (host clock: the call synchronises), and -- when Pillow is installed -- its JPEG encoder at the same
          quality and subsampling on 16 host threads over the planes read back (host clock; the chroma planes are repeated to full size
          first, the only form Pillow's encoder takes).  Without Pillow the PCIe time of read_pictures alone is the floor of the host route.
          The first files of the call are compared with hvqm4_amd.jpeg.encode of the pictures read back before anything is timed; the
          output bytes of a call are reported.
  trace   the kernel trace of a child that makes `reps` calls per preset after a warm-up.  Kernel times per launch of
          a call (measure / lay out / emit) are read from the trace: median with min-max.
--save merges the measurements into one file (profiles/jpeg_bench.json)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.benchlib import add_common_arguments, drive, launch_stats, picture_lists, read_planned, resident, resources, timed  # noqa: E402

W, H = 640, 480
PIC_BYTES = W * H * 3 // 2
QUALITY = 90
PRESETS = ["dense", "natural"]
LAUNCHES = ["measure", "layout", "emit"]
KERNELS = ("hvq_jpeg_code_kernel", "hvq_jpeg_layout_kernel")


def setup(args):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    work = {}
    for preset in PRESETS:
        work[preset] = picture_lists(resident(ctx, preset=preset, streams=args.streams, per=args.per, distinct=args.distinct), args.per)
    n = args.streams * args.per
    out = [torch.empty(2 * PIC_BYTES + 1024, dtype=torch.uint8, device="cuda") for _ in range(n)]
    lengths = torch.empty(n, dtype=torch.int64, device="cuda")
    return torch, ctx, work, out, lengths


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


def trace_summary(trace_dir, printed, _earlier=None):
    cut = read_planned(trace_dir, [(preset, None, 3 * count) for preset, count in printed["plan"]], KERNELS)    # three launches a call
    if "error" in cut:
        return cut
    res = {}
    for preset, part in cut.items():
        res[preset] = {}
        for i, lab in enumerate(LAUNCHES):
            mine = part[3 + i::3]                                                 # without the warm-up call
            if ("layout" in mine[0].shown) != (lab == "layout"):
                return {"error": f"launch {i} of a call is {mine[0].shown}"}
            res[preset][lab] = {"kernel": mine[0].shown, **launch_stats(l.ns for l in mine), **resources(mine[0])}
    return res


def main():
    ap = argparse.ArgumentParser()
    add_common_arguments(ap, children=("calls", "trace"), reps=10, warmup=2, rounds=3, steps="calls,trace", step_timeout=420, out_dir="jpeg_bench_out",
                         out="--save")
    args = ap.parse_args()
    if args.child:
        return {"calls": child_calls, "trace": child_trace}[args.child](args)
    drive(args, {"calls": ("calls", None), "trace": ("trace", trace_summary)}, [sys.executable, os.path.abspath(__file__)])


if __name__ == "__main__":
    main()
