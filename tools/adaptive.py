"""Local thresholds of the pictures of an .h4m clip: per picture the summed-area tables of Y -> a threshold relative to the local mean
(and, with --k, the local deviation) -> optionally an opening, all on the device and nothing waited for in between:
hvq_integral_pictures -> hvq_window_pictures -> hvq_rank_pictures (two a step of the opening) -> hvq_encode_jpeg(src=) where the results
lie.

    python tools/adaptive.py clip.h4m outdir [--radius R] [--c C] [--k K] [--open R] [--quality Q]

It writes outdir/<ordinal>.jpg: Y 255 where a > mean + (K / 256) deviation - C over the window of radius R cut to the picture, else 0,
through an opening by the (2 R + 1)-square where asked, and prints per picture the share of samples that came out 255.  Where one
threshold a plane (tools/autolevels.py, Otsu) fails -- a page, a vignette, one lamp at night -- this one follows the light.  torch is
imported before the library, so both share one HIP runtime."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clip_adaptive(ctx, data, radius=25, c=7, k=0, opening=0, quality=90, files=True):
    """-> (geometry, per picture the share of Y samples that are 255, the JPEG files of the masks or None)"""
    from hvqm4_amd import integral, jpeg, rank
    from hvqm4_amd.container import parse_header, video_pictures
    hdr = parse_header(data)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    n = len(pics)
    sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, n + 3)
    for ft, p in pics:
        ctx.submit(sid, ft, p)
    ctx.flush()
    sids, ords = [sid] * n, list(range(n))
    mask = ctx.adaptive_pictures(sids, ords, integral.adaptive(radius, c=c, k=k))
    if opening:
        mask = ctx.morph_pictures(sids, [-1] * n, [rank.luma_only(s) for s in rank.opening(opening)], src=[mask[i] for i in range(n)])
    res = None
    if files:
        out, lengths = ctx.encode_jpeg(sids, [-1] * n, quality=quality, src=[mask[i] for i in range(n)])
        res = jpeg.files(out, lengths)
    luma = hdr.width * hdr.height
    shares = [float(v) for v in (mask[:, :luma] == 255).float().mean(dim=1).cpu()]
    ctx.close_stream(sid)
    return (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp), shares, res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("clip", help="an .h4m file")
    ap.add_argument("outdir")
    ap.add_argument("--radius", type=int, default=25, metavar="R", help="the window is (2 R + 1)-square, cut to the picture (0 .. 8191)")
    ap.add_argument("--c", type=int, default=7, metavar="C", help="-255 .. 255")
    ap.add_argument("--k", type=int, default=0, metavar="K", help="-1024 .. 1024, in 1/256 of the local deviation")
    ap.add_argument("--open", type=int, default=0, metavar="R", help="an opening of the mask by the (2 R + 1)-square")
    ap.add_argument("--quality", type=int, default=90)
    args = ap.parse_args()
    if not 0 <= args.radius <= 8191 or not -255 <= args.c <= 255 or not -1024 <= args.k <= 1024 or not 0 <= args.open <= 15:
        ap.error("--radius 0 .. 8191, --c -255 .. 255, --k -1024 .. 1024, --open 0 .. 15")
    data = open(args.clip, "rb").read()
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    geom, shares, files = clip_adaptive(ctx, data, args.radius, args.c, args.k, args.open, args.quality)
    ctx.close()
    os.makedirs(args.outdir, exist_ok=True)
    for k, f in enumerate(files):
        with open(os.path.join(args.outdir, f"{k:05d}.jpg"), "wb") as fh:
            fh.write(f)
        print(f"{k:5d} {100 * shares[k]:6.2f} % above the local threshold")
    print(f"{len(files)} pictures {geom[0]}x{geom[1]} -> {args.outdir}")


if __name__ == "__main__":
    main()
