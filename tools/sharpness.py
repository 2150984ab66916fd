"""How sharp (or how blocky) the pictures of an .h4m clip are: per picture the mean and the 99th percentile of the Sobel gradient
magnitude of luma, |d/dx| + |d/dy| divided by 4 and clamped to 255.  Demux, decode, filter and count on the device: the pictures go
through hvq_filter_pictures (hvqm4_amd.filters.gradient_magnitude, luma only) where they lie, the edge maps through
hvq_picture_histograms(src=) where they lie, and 3 x 256 counts per picture come back.

    python tools/sharpness.py clip.h4m

prints one line per picture in decode order, `<ordinal> <frame type> <mean> <p99>`, and the clip's mean of means.  torch is imported
before the library, so both share one HIP runtime."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAME_TYPES = {0x10: "I", 0x20: "P", 0x30: "B"}


def clip_sharpness(ctx, data):
    """-> (frame types, mean per picture, 99th percentile per picture) of one clip"""
    from hvqm4_amd import filters, histograms
    from hvqm4_amd.container import parse_header, video_pictures
    hdr = parse_header(data)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    n = len(pics)
    sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, n + 3)
    for ft, p in pics:
        ctx.submit(sid, ft, p)
    ctx.flush()
    edges = ctx.filter_pictures([sid] * n, list(range(n)), filters.luma_only(filters.gradient_magnitude("sobel")))
    hist = ctx.picture_histograms([sid] * n, [-1] * n, src=[edges[i] for i in range(n)]).cpu().numpy()[:, 0]      # the Y rows
    ctx.close_stream(sid)
    return [ft for ft, _p in pics], filters.sharpness(hist), histograms.percentile(hist, 99)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("clip", help="an .h4m file")
    args = ap.parse_args()
    data = open(args.clip, "rb").read()
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    types, mean, p99 = clip_sharpness(ctx, data)
    ctx.close()
    for k, (ft, m, p) in enumerate(zip(types, mean, p99)):
        print(f"{k:5d} {FRAME_TYPES.get(ft, 'X')} {m:8.3f} {int(p):3d}")
    print(f"{len(types)} pictures, mean {float(mean.mean()):.3f}")


if __name__ == "__main__":
    main()
