"""Near-duplicate pictures of .h4m clips: demux, decode, hash and search on the device, one line per picture in decode order -- ordinal,
frame type, aHash, dHash and pHash (16 hex digits each; hvq_picture_hashes) and the first EARLIER picture whose hash lies within the
threshold, or `-` (hvq_hash_nearest in place on the chosen column).  No picture is read back: what crosses PCIe is the bitstream one
way and 48 bytes per picture the other.

    python tools/dedup.py clip.h4m [clip2.h4m ...] [--hash phash] [--threshold 10]

The records of the golden clips are in tests/golden/phash.json.  torch is imported before the library, so both share one HIP runtime."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAME_TYPES = {0x10: "I", 0x20: "P", 0x30: "B"}


def clip_records(ctx, data, column, threshold):
    """-> (frame types, records [n][4] as unsigned integers, duplicate_of [n]) of one clip: its pictures decoded into a stream of their own,
    hashed where they lie, and the column searched where the records lie"""
    from hvqm4_amd import phash
    from hvqm4_amd.container import parse_header, video_pictures
    hdr = parse_header(data)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, len(pics) + 3)
    for ft, p in pics:
        ctx.submit(sid, ft, p)
    ctx.flush()
    rec = ctx.picture_hashes([sid] * len(pics), list(range(len(pics))))
    near = ctx.hash_nearest(rec[:, column], threshold=threshold)
    dup = near[:, phash.FIRST_WITHIN].cpu().tolist()
    records = phash.as_uint64(rec.cpu().numpy()).tolist()
    ctx.close_stream(sid)
    return [FRAME_TYPES.get(ft, f"{ft:#x}") for ft, _p in pics], records, dup


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("clips", nargs="+", help=".h4m files")
    ap.add_argument("--hash", default="phash", choices=("ahash", "dhash", "phash"), help="the hash the duplicates are judged by")
    ap.add_argument("--threshold", type=int, default=10, help="bits two hashes may differ in, 0 .. 64")
    args = ap.parse_args()
    if not 0 <= args.threshold <= 64:
        ap.error("--threshold lies in 0 .. 64")
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    from hvqm4_amd.phash import DEDUP_HEADER, NAMES, dedup_lines
    ctx = batch.Context(0)
    for path in args.clips:
        types, records, dup = clip_records(ctx, open(path, "rb").read(), NAMES.index(args.hash), args.threshold)
        print(f"# {os.path.basename(path)}: {len(types)} pictures, {sum(d >= 0 for d in dup)} within {args.threshold} bits of an earlier one by {args.hash}")
        print(DEDUP_HEADER)
        for line in dedup_lines(range(len(types)), types, records, dup):
            print(line)
    ctx.close()


if __name__ == "__main__":
    main()
