"""The corners of the pictures of an .h4m clip: how many each has, the strongest of them, and, with an output directory, one JPEG file
per picture with the corners marked.  Demux, decode, corner detection, marking and encoding on the device: the pictures go through
hvq_corner_pictures where they lie, the mask through hvq_rank_pictures (a dilation of radius 2, so that a mark is a 5 x 5 square), the
marks over the picture through hvq_compose_pictures, the result through hvq_encode_jpeg(src=) -- one stream, no host synchronisation in
the chain -- and the lists and the files come back.

    python tools/corners.py clip.h4m [outdir] [--min-eigen] [--radius R] [--nms M] [--threshold T] [--top K]

prints K per picture and its --top strongest corners (x, y, R); with outdir it writes outdir/<ordinal>.jpg per picture in decode order.
torch is imported before the library, so both share one HIP runtime."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAP = 4096                                           # corners a picture's list has room for; K says how many there were
ALPHA = 192                                          # the weight of the marks over the picture, in 1/256ths


def rule_for(min_eigen=False, radius=1, nms=3, threshold=None):
    """the rule of the command line; threshold None: 1, every sample that is a corner at all"""
    from hvqm4_amd import corners as cr
    t = 1 if threshold is None else threshold
    return cr.min_eigen(radius, t, nms) if min_eigen else cr.harris(radius, 10, t, nms)


def marked(ctx, sid, n, geom, mask):
    """the n pictures of stream `sid` with their masks (dilated by 2) laid over them -> the pictures in slot layout, on the device"""
    from hvqm4_amd import compose, rank
    marks = ctx.rank_pictures([sid] * n, [-1] * n, rank.dilate(2), src=mask)
    targets = [compose.overlay(geom, 0, 0, geom[:2], ALPHA, base=2 * k, top=2 * k + 1) for k in range(n)]
    flat_s, flat_o, flat_src = [sid] * (2 * n), [], []
    for k in range(n):
        flat_o += [k, -1]
        flat_src += [None, marks[k]]
    return ctx.compose_pictures(flat_s, flat_o, targets, src=flat_src)


def clip_corners(ctx, data, rule=None, files=False, quality=90):
    """-> (geometry, the lists int64 [CAP + 1][4] as numpy arrays, the JPEG files as bytes or None) of one clip"""
    from hvqm4_amd import jpeg
    from hvqm4_amd.container import parse_header, video_pictures
    hdr = parse_header(data)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    n = len(pics)
    geom = (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)
    sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, n + 3)
    for ft, p in pics:
        ctx.submit(sid, ft, p)
    ctx.flush()
    mask, points, _rows = ctx.corner_pictures([sid] * n, list(range(n)), rule_for() if rule is None else rule, cap=CAP)
    out = None
    if files:
        both = marked(ctx, sid, n, geom, mask)
        bufs, lengths = ctx.encode_jpeg([sid] * n, [-1] * n, quality=quality, src=[both[k] for k in range(n)])
        out = jpeg.files(bufs, lengths)
    lists = [p.cpu().numpy() for p in points]
    ctx.close_stream(sid)
    return geom, lists, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("clip", help="an .h4m file")
    ap.add_argument("outdir", nargs="?", default=None)
    ap.add_argument("--min-eigen", action="store_true", help="the smaller eigenvalue (Shi-Tomasi) instead of Harris' measure")
    ap.add_argument("--radius", type=int, default=1, metavar="R", help="the structure window's radius, 1 .. 3")
    ap.add_argument("--nms", type=int, default=3, metavar="M", help="the suppression distance, 0 .. 7")
    ap.add_argument("--threshold", type=int, default=None, metavar="T", help="the least response of a corner (default 1)")
    ap.add_argument("--top", type=int, default=5, metavar="K", help="strongest corners printed per picture")
    ap.add_argument("--quality", type=int, default=90)
    args = ap.parse_args()
    if not 1 <= args.radius <= 3:
        ap.error("--radius: 1 .. 3")
    if not 0 <= args.nms <= 7:
        ap.error("--nms: 0 .. 7")
    if args.threshold is not None and args.threshold < 1:
        ap.error("--threshold: at least 1")
    data = open(args.clip, "rb").read()
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    from hvqm4_amd import corners as cr
    ctx = batch.Context(0)
    geom, lists, files = clip_corners(ctx, data, rule_for(args.min_eigen, args.radius, args.nms, args.threshold), args.outdir is not None, args.quality)
    ctx.close()
    for k, p in enumerate(lists):
        top = ", ".join(f"({x}, {y}) {r}" for x, y, r, _i in cr.strongest(p, args.top).tolist())
        print(f"{k:5d}: K {int(p[0, 0])}{' (the list holds ' + str(int(p[0, 1])) + ')' if p[0, 1] < p[0, 0] else ''}  {top}")
    if files is not None:
        os.makedirs(args.outdir, exist_ok=True)
        for k, f in enumerate(files):
            with open(os.path.join(args.outdir, f"{k:05d}.jpg"), "wb") as fh:
                fh.write(f)
        print(f"{len(files)} pictures {geom[0]}x{geom[1]} -> {args.outdir}")


if __name__ == "__main__":
    main()
