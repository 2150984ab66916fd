"""Disc morphology and distance fields of the pictures of an .h4m clip: per picture Otsu's threshold -> the exact squared Euclidean
distance transform -> a mask again, all on the device and nothing waited for in between: hvq_picture_histograms -> hvq_histogram_tables ->
hvq_map_pictures -> hvq_distance_pictures -> hvq_distance_mask (a pair a disc step), and with an outdir hvq_encode_jpeg(src=) where the
results lie.

    python tools/discmorph.py clip.h4m [outdir] [--open R | --close R | --erode R | --dilate R] [--field] [--quality Q]

With an outdir it writes outdir/<ordinal>.jpg: the Otsu mask through the disc step of radius R, or with --field the viewable distance
field min(255, isqrt(d)) of the mask's foreground.  Without one it prints per picture the largest inscribed radius of the mask's
foreground -- sqrt of the largest squared distance -- and its place.  torch is imported before the library, so both share one HIP runtime."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clip_discs(ctx, data, steps=None, field=False, quality=90, files=True):
    """-> (geometry, per picture (d, x, y) of the first largest squared distance of the Otsu mask's foreground, the JPEG files of the
    pictures behind `steps` (a list of distance (Rule, Mask) pairs) or of the field, or None)"""
    from hvqm4_amd import distance, jpeg, maps
    from hvqm4_amd.container import parse_header, video_pictures
    hdr = parse_header(data)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    n = len(pics)
    sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, n + 3)
    for ft, p in pics:
        ctx.submit(sid, ft, p)
    ctx.flush()
    sids, ords = [sid] * n, list(range(n))
    mask = ctx.equalize_pictures(sids, ords, maps.Rule(maps.otsu().luma, maps.flat(128).luma))
    rows = [mask[i] for i in range(n)]
    dist = ctx.distance_pictures(sids, [-1] * n, distance.rule(), src=rows)
    res = None
    if files:
        if field or not steps:
            shown = ctx.distance_mask(sids, dist, distance.mask_root())
        else:
            shown = ctx.disc_morph(sids, [-1] * n, steps, src=rows)
        out, lengths = ctx.encode_jpeg(sids, [-1] * n, quality=quality, src=[shown[i] for i in range(n)])
        res = jpeg.files(out, lengths)
    facts = [distance.max_inscribed(d.cpu().numpy()) for d in dist]
    ctx.close_stream(sid)
    return (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp), facts, res


def main():
    from hvqm4_amd import distance
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("clip", help="an .h4m file")
    ap.add_argument("outdir", nargs="?")
    how = ap.add_mutually_exclusive_group()
    for name, what in (("open", "an opening"), ("close", "a closing"), ("erode", "an erosion"), ("dilate", "a dilation")):
        how.add_argument("--" + name, type=int, metavar="R", help=what + " of the mask by the disc of radius R")
    ap.add_argument("--field", action="store_true", help="write the distance field, min(255, isqrt(d)), instead of a mask")
    ap.add_argument("--quality", type=int, default=90)
    args = ap.parse_args()
    steps = None
    for name, make in (("open", distance.opening_disc), ("close", distance.closing_disc), ("erode", distance.erode_disc), ("dilate", distance.dilate_disc)):
        r = getattr(args, name)
        if r is not None:
            if not 0 <= r <= 8192:
                ap.error(f"--{name}: 0 .. 8192")
            steps = distance.as_steps(make(r))
    if args.outdir and not steps and not args.field:
        ap.error("an outdir wants a disc step or --field")
    data = open(args.clip, "rb").read()
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    geom, facts, files = clip_discs(ctx, data, steps, args.field, args.quality, files=bool(args.outdir))
    ctx.close()
    if args.outdir:
        os.makedirs(args.outdir, exist_ok=True)
        for k, f in enumerate(files):
            with open(os.path.join(args.outdir, f"{k:05d}.jpg"), "wb") as fh:
                fh.write(f)
    else:
        for k, (d, x, y) in enumerate(facts):
            radius = "no background" if d == distance.NONE else f"radius {math.sqrt(d):7.2f} (d {d})"
            print(f"{k:5d} {radius} at ({x}, {y})")
    print(f"{len(facts)} pictures {geom[0]}x{geom[1]}" + (f" -> {args.outdir}" if args.outdir else ""))


if __name__ == "__main__":
    main()
