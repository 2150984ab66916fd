"""The objects of the pictures of an .h4m clip: per picture Otsu's threshold -> an opening -> connected components, all on the device and
nothing waited for in between: hvq_picture_histograms -> hvq_histogram_tables -> hvq_map_pictures -> hvq_rank_pictures (the opening) ->
hvq_label_pictures, and with --outdir hvq_select_components -> hvq_encode_jpeg(src=) where the masks lie.

    python tools/objects.py clip.h4m [--min-area N] [--open R] [--connectivity 4|8] [--outdir DIR] [--quality Q]

prints per picture K (the components of the cleaned mask), F (its white samples) and the boxes of the three largest components, and with
--outdir writes DIR/<ordinal>.jpg, the mask of the components of at least N samples (--min-area, default 1: all that have a record).
torch is imported before the library, so both share one HIP runtime."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAP = 1024                                           # records a picture: the components beyond them are counted in K, not described


def clip_objects(ctx, data, min_area=1, opening=1, connectivity=8, quality=90, files=True):
    """-> (geometry, per picture (K, F, [(area, x0, y0, x1, y1) of the three largest]), the JPEG files of the selected masks or None)"""
    from hvqm4_amd import jpeg, labels, maps, rank
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
    if opening:
        mask = ctx.morph_pictures(sids, [-1] * n, [rank.luma_only(s) for s in rank.opening(opening)], src=[mask[i] for i in range(n)])
    labs, comps = ctx.label_pictures(sids, [-1] * n, labels.rule(connectivity=connectivity), cap=CAP, src=[mask[i] for i in range(n)])
    res = None
    if files:
        picked = ctx.select_components(sids, labs, comps, labels.select(area=min_area))
        out, lengths = ctx.encode_jpeg(sids, [-1] * n, quality=quality, src=[picked[i] for i in range(n)])
        res = jpeg.files(out, lengths)
    facts = []
    for c in comps:
        rec = labels.records(c.cpu().numpy())
        if rec.status:
            raise RuntimeError("hvq_label_pictures reports an incomplete picture")
        facts.append((rec.K, rec.F, [tuple(int(v) for v in rec.rows[k - 1, :5]) for k in labels.largest(rec, 3)]))
    ctx.close_stream(sid)
    return (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp), facts, res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("clip", help="an .h4m file")
    ap.add_argument("--min-area", type=int, default=1, metavar="N", help="with --outdir: keep the components of at least N samples")
    ap.add_argument("--open", type=int, default=1, dest="opening", metavar="R", help="an opening of radius R on the mask (0: none)")
    ap.add_argument("--connectivity", type=int, default=8, choices=(4, 8))
    ap.add_argument("--outdir")
    ap.add_argument("--quality", type=int, default=90)
    args = ap.parse_args()
    if not 0 <= args.opening <= 15:
        ap.error("--open: 0 .. 15")
    if args.min_area < 0:
        ap.error("--min-area: not negative")
    data = open(args.clip, "rb").read()
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    geom, facts, files = clip_objects(ctx, data, args.min_area, args.opening, args.connectivity, args.quality, files=bool(args.outdir))
    ctx.close()
    for k, (K, F, top) in enumerate(facts):
        print(f"{k:5d} K {K:6d} F {F:8d} " + " ".join(f"[{a} at ({x0}, {y0}) .. ({x1}, {y1})]" for a, x0, y0, x1, y1 in top))
    if args.outdir:
        os.makedirs(args.outdir, exist_ok=True)
        for k, f in enumerate(files):
            with open(os.path.join(args.outdir, f"{k:05d}.jpg"), "wb") as fh:
                fh.write(f)
    print(f"{len(facts)} pictures {geom[0]}x{geom[1]}" + (f" -> {args.outdir}" if args.outdir else ""))


if __name__ == "__main__":
    main()
