"""The pictures of an .h4m clip despeckled and written as JPEG files.  Demux, decode, rank filter and encode on the device: the pictures
go through hvq_rank_pictures where they lie -- a median (the speckle and block-edge outliers of a vector-quantised codec vanish, edges
stay) and, if asked for, an opening of radius R on top (bright detail smaller than the window goes) --, the results through
hvq_encode_jpeg(src=) where they lie, and the files come back.

    python tools/despeckle.py clip.h4m outdir [--median 3|5] [--open R] [--quality Q]

writes outdir/<ordinal>.jpg per picture in decode order.  The chroma planes take the window that fits their sampling
(hvqm4_amd.rank.chroma_for).  torch is imported before the library, so both share one HIP runtime."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def steps_for(median, opening, h_samp, v_samp):
    """the rank steps of the command line for a clip of sampling (h_samp, v_samp)"""
    from hvqm4_amd import rank
    steps = [rank.chroma_for(rank.median(median), h_samp, v_samp)] if median else []
    if opening:
        steps += [rank.chroma_for(s, h_samp, v_samp) for s in rank.opening(opening)]
    return steps or [rank.identity()]


def clip_despeckled(ctx, data, median=3, opening=0, quality=90):
    """-> (geometry, the JPEG files as bytes) of one clip"""
    from hvqm4_amd import jpeg
    from hvqm4_amd.container import parse_header, video_pictures
    hdr = parse_header(data)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    n = len(pics)
    sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, n + 3)
    for ft, p in pics:
        ctx.submit(sid, ft, p)
    ctx.flush()
    clean = ctx.morph_pictures([sid] * n, list(range(n)), steps_for(median, opening, hdr.h_samp, hdr.v_samp))
    files, lengths = ctx.encode_jpeg([sid] * n, [-1] * n, quality=quality, src=[clean[i] for i in range(n)])
    out = jpeg.files(files, lengths)
    ctx.close_stream(sid)
    return (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp), out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("clip", help="an .h4m file")
    ap.add_argument("outdir")
    ap.add_argument("--median", type=int, choices=(0, 3, 5), default=3, help="the median's window (0: none)")
    ap.add_argument("--open", type=int, default=0, dest="opening", metavar="R", help="an opening of radius R behind the median (0: none)")
    ap.add_argument("--quality", type=int, default=90)
    args = ap.parse_args()
    if not 0 <= args.opening <= 15:
        ap.error("--open: 0 .. 15")
    data = open(args.clip, "rb").read()
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    geom, files = clip_despeckled(ctx, data, args.median, args.opening, args.quality)
    ctx.close()
    os.makedirs(args.outdir, exist_ok=True)
    for k, f in enumerate(files):
        with open(os.path.join(args.outdir, f"{k:05d}.jpg"), "wb") as fh:
            fh.write(f)
    print(f"{len(files)} pictures {geom[0]}x{geom[1]} -> {args.outdir}")


if __name__ == "__main__":
    main()
