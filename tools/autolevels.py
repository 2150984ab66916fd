"""The pictures of an .h4m clip through tables made of their own histograms, written as JPEG files.  Demux, decode, histograms, tables,
lookup and encode on the device, nothing waited for in between: hvq_picture_histograms -> hvq_histogram_tables -> hvq_map_pictures
(Context.equalize_pictures), the results through hvq_encode_jpeg(src=) where they lie, and the files come back.

    python tools/autolevels.py clip.h4m outdir [--equalize | --stretch LO:HI | --otsu [--open R]] [--quality Q]

writes outdir/<ordinal>.jpg per picture in decode order.  --equalize (the default) equalises the luma histogram; --stretch LO:HI clips
LO and HI per mille of the luma samples at the dark and the bright end and stretches what lies between to 0 .. 255; --otsu binarises
the luma plane at Otsu's threshold (chroma becomes 128: a grey mask), --open R cleans the mask with an opening of radius R
(Context.morph_pictures), and per picture the threshold and the count of 255-samples of the mask are printed, the count from
hvq_picture_histograms(src=) of the mask.  torch is imported before the library, so both share one HIP runtime."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rule_for(mode, lo=0, hi=0):
    """the rule of the command line: luma through the histogram, chroma as it is (a mask: grey)"""
    from hvqm4_amd import maps
    if mode == "equalize":
        return maps.equalize().luma_only()
    if mode == "stretch":
        return maps.stretch(lo, hi).luma_only()
    if mode == "otsu":
        return maps.Rule(maps.otsu().luma, maps.flat(128).luma)
    raise ValueError(f"mode {mode!r}: equalize, stretch or otsu")


def clip_levelled(ctx, data, mode="equalize", lo=0, hi=0, opening=0, quality=90):
    """-> (geometry, the JPEG files as bytes, per picture (threshold, 255-samples of the mask) under otsu, else None) of one clip"""
    from hvqm4_amd import jpeg, rank
    from hvqm4_amd.container import parse_header, video_pictures
    hdr = parse_header(data)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    n = len(pics)
    sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, n + 3)
    for ft, p in pics:
        ctx.submit(sid, ft, p)
    ctx.flush()
    sids, ords = [sid] * n, list(range(n))
    rule = rule_for(mode, lo, hi)
    facts = None
    if mode == "otsu":
        hist = ctx.picture_histograms(sids, ords)
        tables = ctx.histogram_tables(hist, rule)
        out = ctx.map_pictures(sids, ords, tables)
        if opening:
            out = ctx.morph_pictures(sids, [-1] * n, [rank.luma_only(s) for s in rank.opening(opening)], src=[out[i] for i in range(n)])
        counts = ctx.picture_histograms(sids, [-1] * n, src=[out[i] for i in range(n)])
        t = tables.cpu().numpy()[:, 0, :]
        c = counts.cpu().numpy()[:, 0, 255]
        facts = [(int((t[i] == 0).sum()) - 1, int(c[i])) for i in range(n)]          # the table is 0 up to t and 255 above it
    else:
        out = ctx.equalize_pictures(sids, ords, rule)
    files, lengths = ctx.encode_jpeg(sids, [-1] * n, quality=quality, src=[out[i] for i in range(n)])
    res = jpeg.files(files, lengths)
    ctx.close_stream(sid)
    return (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp), res, facts


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("clip", help="an .h4m file")
    ap.add_argument("outdir")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--equalize", action="store_true")
    g.add_argument("--stretch", metavar="LO:HI", help="per mille clipped at either end, each 0 .. 499")
    g.add_argument("--otsu", action="store_true")
    ap.add_argument("--open", type=int, default=0, dest="opening", metavar="R", help="with --otsu: an opening of radius R on the mask (0: none)")
    ap.add_argument("--quality", type=int, default=90)
    args = ap.parse_args()
    mode, lo, hi = "equalize", 0, 0
    if args.stretch:
        try:
            lo, hi = (int(v) for v in args.stretch.split(":"))
        except ValueError:
            ap.error("--stretch LO:HI: two integers")
        if not 0 <= lo <= 499 or not 0 <= hi <= 499:
            ap.error("--stretch: each 0 .. 499")
        mode = "stretch"
    elif args.otsu:
        mode = "otsu"
    if args.opening and mode != "otsu":
        ap.error("--open goes with --otsu")
    if not 0 <= args.opening <= 15:
        ap.error("--open: 0 .. 15")
    data = open(args.clip, "rb").read()
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    geom, files, facts = clip_levelled(ctx, data, mode, lo, hi, args.opening, args.quality)
    ctx.close()
    os.makedirs(args.outdir, exist_ok=True)
    for k, f in enumerate(files):
        with open(os.path.join(args.outdir, f"{k:05d}.jpg"), "wb") as fh:
            fh.write(f)
    for k, (t, c) in enumerate(facts or ()):
        print(f"{k:5d} threshold {t:3d} mask {c}")
    print(f"{len(files)} pictures {geom[0]}x{geom[1]} -> {args.outdir}")


if __name__ == "__main__":
    main()
