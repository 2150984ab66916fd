"""Motion of .h4m clips by block matching: demux, decode and search on the device, one line per picture in decode order -- ordinal, frame
type, the global vector (dy, dx) of its motion field against its predecessor (hvq_picture_motion: the most frequent vector; the block
looks like the predecessor at that offset), the share of the blocks that have it, and the share of moving blocks (those the search
improved by at least --min-gain over the zero vector).  No picture is read back: what crosses PCIe is the bitstream one way and 16 bytes
per block the other.

    python tools/motionfield.py clip.h4m [clip2.h4m ...] [--block 8|16] [--radius R] [--min-gain G]

torch is imported before the library, so both share one HIP runtime."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAME_TYPES = {0x10: "I", 0x20: "P", 0x30: "B"}


def field_line(k, ftype, field, min_gain):
    """the line of picture k: `field` its motion field against its predecessor as a numpy array [rows, cols, 4], None for the first"""
    from hvqm4_amd.motion import global_motion, moving_mask
    if field is None:
        return f"{k:6d} {ftype}    -    -        -        -"
    (dy, dx), share = global_motion(field)
    return f"{k:6d} {ftype} {dy:+4d} {dx:+4d} {share:8.4f} {float(moving_mask(field, min_gain).mean()):8.4f}"


def clip_fields(ctx, data, block, radius):
    """-> (frame types, fields) of one clip: its pictures decoded into a stream of their own; fields[k] is None for k = 0"""
    from hvqm4_amd.container import parse_header, video_pictures
    hdr = parse_header(data)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    n = len(pics)
    sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, n + 3)
    for ft, p in pics:
        ctx.submit(sid, ft, p)
    ctx.flush()
    fields = ctx.picture_motion([sid] * (n - 1), list(range(1, n)), [(sid, k - 1) for k in range(1, n)], block=block, radius=radius) if n > 1 else []
    fields = [None] + [f.cpu().numpy() for f in fields]
    ctx.close_stream(sid)
    return [FRAME_TYPES.get(ft, f"{ft:#x}") for ft, _p in pics], fields


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("clips", nargs="+", help=".h4m files")
    ap.add_argument("--block", type=int, default=8, choices=(8, 16), help="block size (16 needs a width and height that are multiples of 16)")
    ap.add_argument("--radius", type=int, default=8, help="search radius, 0 .. 15")
    ap.add_argument("--min-gain", type=int, default=64, help="a block moves when its best vector costs at least this much less than (0, 0)")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    for path in args.clips:
        types, fields = clip_fields(ctx, open(path, "rb").read(), args.block, args.radius)
        print(f"# {os.path.basename(path)}: {len(types)} pictures, blocks of {args.block}, radius {args.radius}, moving at a gain of {args.min_gain}")
        print("# ordinal type dy dx share moving")
        for k, (t, f) in enumerate(zip(types, fields)):
            print(field_line(k, t, f, args.min_gain))
    ctx.close()


if __name__ == "__main__":
    main()
