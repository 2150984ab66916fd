"""framecrc for .h4m clips: demux, decode and checksum on the device, one line per picture in decode order -- ordinal, frame type, crc32 of
Y, U, V and of the picture, adler32 of Y, U, V and of the picture (zlib's; hvq_picture_checksums).  No picture is read back: what crosses
PCIe is the bitstream one way and 64 bytes per picture the other.

    python tools/framecrc.py clip.h4m [clip2.h4m ...]

The values of the golden clips are in tests/golden/checksums.json.  torch is imported before the library, so both share one HIP runtime."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAME_TYPES = {0x10: "I", 0x20: "P", 0x30: "B"}


def clip_records(ctx, data):
    """-> (frame types, int64 CPU tensor [n, 8]) of one clip: its pictures decoded into a stream of their own and checksummed where they lie"""
    from hvqm4_amd.container import parse_header, video_pictures
    hdr = parse_header(data)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, len(pics) + 3)
    for ft, p in pics:
        ctx.submit(sid, ft, p)
    ctx.flush()
    rec = ctx.picture_checksums([sid] * len(pics), list(range(len(pics)))).cpu()
    ctx.close_stream(sid)
    return [FRAME_TYPES.get(ft, f"{ft:#x}") for ft, _p in pics], rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("clips", nargs="+", help=".h4m files")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    from hvqm4_amd.checksums import FRAMECRC_HEADER, framecrc_lines
    ctx = batch.Context(0)
    for path in args.clips:
        types, rec = clip_records(ctx, open(path, "rb").read())
        print(f"# {os.path.basename(path)}: {len(types)} pictures")
        print(FRAMECRC_HEADER)
        for line in framecrc_lines(range(len(types)), types, rec.tolist()):
            print(line)
    ctx.close()


if __name__ == "__main__":
    main()
