"""The pictures of an .h4m clip as JPEG files: demux, decode and encode on the device, one .jpg per picture in decode order
(hvq_encode_jpeg: baseline JFIF, the clip's own Y / Cb / Cr and sampling, no colour conversion, no resampling).  What crosses PCIe is the
bitstream one way and the compressed files the other; no decoded picture is read back.

    python tools/h4m2jpeg.py clip.h4m outdir [--quality Q] [--rotate {90,180,270}] [--size WxH | --fit N] [--sharpen AMOUNT[:SIGMA]]

writes outdir/<clip name>_<ordinal, 5 digits><frame type>.jpg.  --size WxH (multiples of 8) and --fit N (the largest size of the clip's
aspect inside N x N, hvqm4_amd.scale.fit) make thumbnails: the pictures are resampled where they lie (hvq_scale_pictures, the area
filter) and the scaled pictures encoded from there (encode_jpeg(src=...)); a stream of the thumbnails' geometry that nothing is submitted
to carries them.  --sharpen AMOUNT[:SIGMA] (AMOUNT a rational with a power-of-two denominator such as 1/2 or 0.75, SIGMA 1.0 unless given)
sharpens the luma of the pictures, after the scale if there is one, by unsharp masking where they lie (hvq_filter_pictures,
hvqm4_amd.filters.unsharp) and encodes from there: a reduced picture is soft.  --rotate D turns the pictures by D degrees
counter-clockwise where they lie, before everything else (hvq_warp_pictures, hvqm4_amd.warp.rotate90: an exact permutation of the
samples in 4:2:0 and 4:4:4); 90 and 270 exchange width and height, and --size / --fit then speak of the turned picture.  Without these options the files are what they always were.  torch is imported before the library, so both share one HIP
runtime."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAME_TYPES = {0x10: "I", 0x20: "P", 0x30: "B"}


def file_name(stem, k, ftype):
    return f"{stem}_{k:05d}{FRAME_TYPES.get(ftype, 'X')}.jpg"


def clip_files(ctx, data, quality, size=None, sharpen=None, rotate=None):
    """-> (frame types, files as bytes) of one clip: its pictures decoded into a stream of their own and encoded in one call; size =
    (w, h): scaled to that size first, on the device; sharpen = (amount, sigma): the luma unsharp-masked after that, on the device;
    rotate = 90, 180 or 270: turned counter-clockwise before either, on the device"""
    from hvqm4_amd import filters, jpeg, warp
    from hvqm4_amd.container import parse_header, video_pictures
    hdr = parse_header(data)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    n = len(pics)
    sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, n + 3)
    for ft, p in pics:
        ctx.submit(sid, ft, p)
    ctx.flush()
    if size is None and sharpen is None and rotate is None:
        buffers, lengths = ctx.encode_jpeg([sid] * n, list(range(n)), quality=quality)
        files = jpeg.files(buffers, lengths)
    else:
        src, turned_sid, tw, th = None, None, hdr.width, hdr.height
        if rotate is not None:
            turn, (tw, th) = warp.rotate90(rotate // 90, hdr.width, hdr.height)
            turned = ctx.warp_pictures([sid] * n, list(range(n)), turn, size=(tw, th))
            src = [turned[i] for i in range(n)]
            turned_sid = ctx.open_stream(tw, th, hdr.h_samp, hdr.v_samp, hdr.is15, 3)          # never submitted to: it names the geometry of src=
        w, h = size or (tw, th)
        carrier = ctx.open_stream(w, h, hdr.h_samp, hdr.v_samp, hdr.is15, 3)                   # likewise, for the geometry that is encoded
        if size is not None:
            scaled = ctx.scale_pictures([sid] * n, list(range(n)), size) if src is None else ctx.scale_pictures([turned_sid] * n, [-1] * n, size, src=src)
            src = [scaled[i] for i in range(n)]
        if sharpen is not None:
            unsharp = filters.luma_only(filters.unsharp(sharpen[1], sharpen[0]))
            sharp = ctx.filter_pictures([sid] * n, list(range(n)), unsharp) if src is None else ctx.filter_pictures([carrier] * n, [-1] * n, unsharp, src=src)
            src = [sharp[i] for i in range(n)]
        buffers, lengths = ctx.encode_jpeg([carrier] * n, [-1] * n, quality=quality, src=src)
        files = jpeg.files(buffers, lengths)
        ctx.close_stream(carrier)
        if turned_sid is not None:
            ctx.close_stream(turned_sid)
    ctx.close_stream(sid)
    return [ft for ft, _p in pics], files


def target_size(data, size, fit, error, rotate=None):
    """(w, h) of the thumbnails, or None without --size / --fit; error(message) on what the library would refuse; rotate 90 or 270:
    the clip's width and height change places first"""
    from hvqm4_amd import scale
    from hvqm4_amd.container import parse_header
    if not size and fit is None:
        return None
    hdr = parse_header(data)
    cw, ch = (hdr.height, hdr.width) if rotate in (90, 270) else (hdr.width, hdr.height)
    if size:
        try:
            w, h = (int(v) for v in size.lower().split("x"))
        except ValueError:
            error("--size takes WxH")
    else:
        if fit < 8:
            error("--fit takes 8 at least")
        w, h = scale.fit(cw, ch, fit, fit)
    try:
        scale.plane_sizes((cw, ch, hdr.h_samp, hdr.v_samp), (w, h, hdr.h_samp, hdr.v_samp))
    except ValueError as e:
        error(str(e))
    return w, h


def sharpen_option(text, error):
    """(amount as a Fraction, sigma) of --sharpen AMOUNT[:SIGMA], or None; error(message) on what hvqm4_amd.filters would refuse"""
    from fractions import Fraction
    from hvqm4_amd import filters
    if text is None:
        return None
    try:
        amount, _, sigma = text.partition(":")
        got = Fraction(amount), float(sigma) if sigma else 1.0
        filters.check(filters.unsharp(got[1], got[0]))
    except (ValueError, ZeroDivisionError) as e:
        error(f"--sharpen {text}: {e}")
    return got


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("clip", help="an .h4m file")
    ap.add_argument("outdir")
    ap.add_argument("--quality", type=int, default=90, help="1 .. 100, scaled as the IJG library does")
    ap.add_argument("--size", default=None, metavar="WxH", help="thumbnails of this size (multiples of 8)")
    ap.add_argument("--fit", type=int, default=None, metavar="N", help="thumbnails of the clip's aspect inside N x N")
    ap.add_argument("--rotate", type=int, default=None, choices=(90, 180, 270), help="turn the pictures counter-clockwise first")
    ap.add_argument("--sharpen", default=None, metavar="AMOUNT[:SIGMA]", help="unsharp masking of the luma after the scale, e.g. 1/2 or 0.75:1.5")
    args = ap.parse_args()
    if not 1 <= args.quality <= 100:
        ap.error("--quality takes 1 .. 100")
    if args.size and args.fit:
        ap.error("--size and --fit exclude each other")
    data = open(args.clip, "rb").read()
    size = target_size(data, args.size, args.fit, ap.error, args.rotate)
    sharpen = sharpen_option(args.sharpen, ap.error)
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    os.makedirs(args.outdir, exist_ok=True)
    stem = os.path.splitext(os.path.basename(args.clip))[0]
    ctx = batch.Context(0)
    types, files = clip_files(ctx, data, args.quality, size, sharpen, args.rotate)
    ctx.close()
    for k, (ft, f) in enumerate(zip(types, files)):
        with open(os.path.join(args.outdir, file_name(stem, k, ft)), "wb") as out:
            out.write(f)
    print(f"{len(files)} files, {sum(len(f) for f in files)} bytes, quality {args.quality} -> {args.outdir}")


if __name__ == "__main__":
    main()
