"""The pictures of an .h4m clip cleaned up with an edge-preserving filter and written as JPEG files.  Demux, decode, bilateral filter and
encode on the device: the pictures go through hvq_bilateral_pictures where they lie -- a bilateral filter of Gaussian weights (the block
edges and the noise of a vector-quantised codec are smoothed, the real edges stay), or with --surface a sigma filter ("surface blur": the
mean of the neighbours within T of the sample), K times over --, the results through hvq_encode_jpeg(src=) where they lie, and the files
come back.

    python tools/denoise.py clip.h4m outdir [--sigma-space S] [--sigma-range R] [--radius N] [--iterations K] [--surface T] [--quality Q]

writes outdir/<ordinal>.jpg per picture in decode order.  The chroma planes take the window that fits their sampling
(hvqm4_amd.bilateral.chroma_for).  torch is imported before the library, so both share one HIP runtime."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def steps_for(sigma_space, sigma_range, radius, iterations, surface, h_samp, v_samp):
    """the bilateral steps of the command line for a clip of sampling (h_samp, v_samp); radius None: from sigma_space; surface None: the
    Gaussian weights, otherwise the sigma filter of that threshold (its radius from sigma_space when none is given)"""
    from hvqm4_amd import bilateral as bl
    if surface is None:
        b = bl.bilateral(sigma_space, sigma_range, radius)
    else:
        b = bl.sigma_filter(bl.default_radius(sigma_space) if radius is None else radius, surface)
    return bl.iterate(bl.chroma_for(b, h_samp, v_samp), iterations)


def clip_denoised(ctx, data, sigma_space=1.5, sigma_range=12.0, radius=None, iterations=1, surface=None, quality=90):
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
    clean = ctx.smooth_pictures([sid] * n, list(range(n)), steps_for(sigma_space, sigma_range, radius, iterations, surface, hdr.h_samp, hdr.v_samp))
    files, lengths = ctx.encode_jpeg([sid] * n, [-1] * n, quality=quality, src=[clean[i] for i in range(n)])
    out = jpeg.files(files, lengths)
    ctx.close_stream(sid)
    return (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp), out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("clip", help="an .h4m file")
    ap.add_argument("outdir")
    ap.add_argument("--sigma-space", type=float, default=1.5, metavar="S", help="the spatial Gaussian's sigma, in luma samples")
    ap.add_argument("--sigma-range", type=float, default=12.0, metavar="R", help="the range Gaussian's sigma, in sample values")
    ap.add_argument("--radius", type=int, default=None, metavar="N", help="the window's radius, 0 .. 7 (default: from --sigma-space)")
    ap.add_argument("--iterations", type=int, default=1, metavar="K")
    ap.add_argument("--surface", type=int, default=None, metavar="T", help="a sigma filter of threshold T instead of the Gaussian weights")
    ap.add_argument("--quality", type=int, default=90)
    args = ap.parse_args()
    if args.radius is not None and not 0 <= args.radius <= 7:
        ap.error("--radius: 0 .. 7")
    if not 1 <= args.iterations <= 64:
        ap.error("--iterations: 1 .. 64")
    if args.surface is not None and not 0 <= args.surface <= 255:
        ap.error("--surface: 0 .. 255")
    data = open(args.clip, "rb").read()
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    geom, files = clip_denoised(ctx, data, args.sigma_space, args.sigma_range, args.radius, args.iterations, args.surface, args.quality)
    ctx.close()
    os.makedirs(args.outdir, exist_ok=True)
    for k, f in enumerate(files):
        with open(os.path.join(args.outdir, f"{k:05d}.jpg"), "wb") as fh:
            fh.write(f)
    print(f"{len(files)} pictures {geom[0]}x{geom[1]} -> {args.outdir}")


if __name__ == "__main__":
    main()
