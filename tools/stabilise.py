"""An .h4m clip stabilised against its own global motion, as JPEG files: demux, decode, motion search, warp and encode on the device.
Every picture is searched against its predecessor (hvq_picture_motion), the most frequent vector of each field is the camera's step
(hvqm4_amd.motion.global_motion), the steps add up to the camera's path, and every picture is moved back along that path
(hvq_warp_pictures with hvqm4_amd.warp.translate by the accumulated vector, replicated border) and encoded where it lies
(hvq_encode_jpeg(src=)).  Nothing is read back but the fields and the files.

    python tools/stabilise.py clip.h4m outdir [--quality Q] [--block {8,16}] [--radius R]

writes outdir/<clip name>_<ordinal, 5 digits><frame type>.jpg in decode order and prints the path.  torch is imported before the
library, so both share one HIP runtime."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from h4m2jpeg import file_name  # noqa: E402


def camera_path(fields):
    """the accumulated (dy, dx) per picture from the fields of pictures 1 .. n - 1 against their predecessors: picture k looks like
    picture 0 displaced by path[k]"""
    from hvqm4_amd import motion
    path = [(0, 0)]
    for f in fields:
        (dy, dx), _share = motion.global_motion(f)
        path.append((path[-1][0] + dy, path[-1][1] + dx))
    return path


def stabilised_files(ctx, data, quality=90, block=16, radius=8):
    """-> (frame types, the camera's path, files as bytes) of one clip"""
    from hvqm4_amd import jpeg, warp
    from hvqm4_amd.container import parse_header, video_pictures
    hdr = parse_header(data)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    n = len(pics)
    sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, n + 3)
    for ft, p in pics:
        ctx.submit(sid, ft, p)
    ctx.flush()
    fields = ctx.picture_motion([sid] * (n - 1), list(range(1, n)), [(sid, k - 1) for k in range(1, n)], block=block, radius=radius) if n > 1 else []
    path = camera_path([f.cpu().numpy() for f in fields])
    # picture k at (y, x) looks like picture 0 at (y + dy, x + dx): moved by (dy, dx), it lies where picture 0 lies
    steady = ctx.warp_pictures([sid] * n, list(range(n)), [warp.translate(dx, dy) for dy, dx in path])
    buffers, lengths = ctx.encode_jpeg([sid] * n, [-1] * n, quality=quality, src=[steady[i] for i in range(n)])
    files = jpeg.files(buffers, lengths)
    ctx.close_stream(sid)
    return [ft for ft, _p in pics], path, files


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("clip", help="an .h4m file")
    ap.add_argument("outdir")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--block", type=int, default=16, choices=(8, 16))
    ap.add_argument("--radius", type=int, default=8)
    args = ap.parse_args()
    data = open(args.clip, "rb").read()
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    os.makedirs(args.outdir, exist_ok=True)
    stem = os.path.splitext(os.path.basename(args.clip))[0]
    ctx = batch.Context(0)
    types, path, files = stabilised_files(ctx, data, args.quality, args.block, args.radius)
    ctx.close()
    for k, (ft, f) in enumerate(zip(types, files)):
        with open(os.path.join(args.outdir, file_name(stem, k, ft)), "wb") as out:
            out.write(f)
    print("path (dy, dx): " + " ".join(f"{dy},{dx}" for dy, dx in path))
    print(f"{len(files)} files, {sum(len(f) for f in files)} bytes -> {args.outdir}")


if __name__ == "__main__":
    main()
