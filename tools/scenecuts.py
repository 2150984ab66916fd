"""Scene cuts of .h4m clips by histogram distance: demux, decode and measure on the device, one line per picture in decode order -- ordinal,
frame type, the intersection of its luma histogram with its predecessor's (hvq_picture_histograms; 1 = the same distribution, towards 0 =
another scene), beside it the mean absolute luma difference from hvq_picture_metrics (the cruder measure: it also rises with motion inside
a scene), and CUT where the intersection falls below the threshold.  No picture is read back: what crosses PCIe is the bitstream one way
and 3 KiB + 96 bytes per picture the other.

    python tools/scenecuts.py clip.h4m [clip2.h4m ...] [--threshold T]

torch is imported before the library, so both share one HIP runtime."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAME_TYPES = {0x10: "I", 0x20: "P", 0x30: "B"}


def cut_lines(types, luma_hist, mad, threshold):
    """the lines of one clip: `luma_hist` integer [n, 256], `mad` the mean absolute luma difference from the predecessor, [n] (entry 0 is
    not printed: the first picture has no predecessor)"""
    from hvqm4_amd.histograms import intersection
    lines = [f"{0:6d} {types[0]}        -        -"]
    for k in range(1, len(types)):
        x = float(intersection(luma_hist[k], luma_hist[k - 1]))
        lines.append(f"{k:6d} {types[k]} {x:8.4f} {float(mad[k]):8.3f}" + (" CUT" if x < threshold else ""))
    return lines


def clip_measures(ctx, data):
    """-> (frame types, int32 CPU array [n, 256], float CPU array [n]) of one clip: its pictures decoded into a stream of their own"""
    from hvqm4_amd.container import parse_header, video_pictures
    from hvqm4_amd.metrics import mean_abs_diff, plane_samples
    hdr = parse_header(data)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    n = len(pics)
    sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, n + 3)
    for ft, p in pics:
        ctx.submit(sid, ft, p)
    ctx.flush()
    hist = ctx.picture_histograms([sid] * n, list(range(n)))
    met = ctx.picture_metrics([sid] * n, list(range(n)), [(sid, max(k - 1, 0)) for k in range(n)])
    mad = mean_abs_diff(met, plane_samples(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp))[:, 0]
    hist, mad = hist[:, 0].cpu().numpy(), mad.cpu().numpy()
    ctx.close_stream(sid)
    return [FRAME_TYPES.get(ft, f"{ft:#x}") for ft, _p in pics], hist, mad


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("clips", nargs="+", help=".h4m files")
    ap.add_argument("--threshold", type=float, default=0.5, help="a cut where the luma histogram intersection with the predecessor is below it")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    for path in args.clips:
        types, hist, mad = clip_measures(ctx, open(path, "rb").read())
        print(f"# {os.path.basename(path)}: {len(types)} pictures, threshold {args.threshold}")
        print("# ordinal type intersection mean_abs_diff")
        for line in cut_lines(types, hist, mad, args.threshold):
            print(line)
    ctx.close()


if __name__ == "__main__":
    main()
