"""Picture export (hvq_export_pictures) against the display epilogue, HIP-event timed on the GPU.

128 streams of 640x480 (the bench's dense preset), 8 resident pictures each, per sampling (4:2:0, 4:2:2, 4:4:4):
  * export of all 1024 pictures in each format (RGB24 output ~0.94 GB: far beyond the 256 MiB Infinity Cache);
  * 4:2:0 only: RGB24 export of the newest picture of every stream -- the 128 pictures hvq_rgb_bench converts -- alternated with
    hvq_rgb_bench itself, for the like-for-like A/B.
bytes = source plane bytes read + destination bytes written; fraction of 8 TB/s.  One JSON line on stdout (and --out).
torch is imported before the library, so both share one HIP runtime (hvqm4_amd.export.check_one_hip_runtime)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hvqm4_amd import batch  # noqa: E402
from tools.benchlib import PEAK, SAMPLINGS, picture_lists, resident, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--per", type=int, default=8, help="resident pictures per stream")
    ap.add_argument("--distinct", type=int, default=8, help="distinct clips dealt over the streams")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ab-rounds", type=int, default=5)
    ap.add_argument("--samplings", default="420,422,444")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.init()
    w, h = 640, 480
    res = {"streams": args.streams, "pictures": args.streams * args.per, "size": f"{w}x{h}", "reps": args.reps, "peak_bytes_per_s": PEAK}
    for sampling in args.samplings.split(","):
        ctx = batch.Context(0)
        sids = resident(ctx, preset="dense", sampling=sampling, streams=args.streams, per=args.per, distinct=args.distinct, w=w, h=h)
        hs, vs = SAMPLINGS[sampling]
        src = w * h + 2 * (w // (hs)) * (h // (vs))
        n = len(sids) * args.per
        all_s, all_o = picture_lists(sids, args.per)
        for fmt in ("rgb", "rgbp", "yuv444p"):
            out = torch.empty((n, h, w, 3) if fmt == "rgb" else (n, 3, h, w), dtype=torch.uint8, device="cuda")
            fn = lambda: ctx.export(all_s, all_o, out, fmt)
            timed(torch, fn, args.warmup)
            ms = timed(torch, fn, args.reps)
            by = n * (src + 3 * w * h)
            res[f"{sampling}_{fmt}_all"] = {"ms": round(ms, 4), "bytes": by, "tb_per_s": round(by / ms / 1e9, 3),
                                            "of_peak": round(by / ms / 1e9 / (PEAK / 1e12), 3)}
            del out
            torch.cuda.empty_cache()
        if sampling == "420":
            out = torch.empty((len(sids), h, w, 3), dtype=torch.uint8, device="cuda")
            fn = lambda: ctx.export(sids, [args.per - 1] * len(sids), out, "rgb")
            timed(torch, fn, args.warmup)
            ctx.rgb_bench(args.warmup)
            ab = {"export_ms": [], "rgb_bench_ms": []}
            for _ in range(args.ab_rounds):
                ab["export_ms"].append(round(timed(torch, fn, args.reps), 4))
                ms, by, npic = ctx.rgb_bench(args.reps)
                ab["rgb_bench_ms"].append(round(ms / args.reps, 4))
            by = len(sids) * (src + 3 * w * h)
            assert npic == len(sids) and by == ctx.rgb_bench(1)[1]
            ab["bytes"] = by
            ab["export_of_peak"] = [round(by / m / 1e9 / 8.0, 3) for m in ab["export_ms"]]
            ab["rgb_bench_of_peak"] = [round(by / m / 1e9 / 8.0, 3) for m in ab["rgb_bench_ms"]]
            res["420_rgb_newest_ab"] = ab
            # the newest pictures through both paths are the same bytes
            ref = torch.from_numpy(ctx.read_picture_rgb(sids[0], args.per - 1, w, h)).cuda()
            torch.cuda.synchronize()
            assert torch.equal(out[0], ref)
            del out
        ctx.close()
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
