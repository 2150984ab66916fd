"""The pictures of an .h4m clip as ONE JPEG contact sheet: demux, decode, scale, compose and encode on the device.  Every K-th picture is
reduced to a cell where it lies (hvq_scale_pictures, the area filter), the cells are laid row by row over a flat background into one
picture (hvq_compose_pictures, hvqm4_amd.compose.mosaic) and that picture is encoded from there (encode_jpeg(src=...)).  What crosses
PCIe is the bitstream one way and one compressed file the other; no decoded picture is read back.

    python tools/contactsheet.py clip.h4m out.jpg [--cols N] [--cell WxH] [--every K] [--gap G] [--quality Q]

--cols N: cells a row (default: the square root of their number, rounded up); --cell WxH: the size of a cell, multiples of 8 (default:
the largest of the clip's aspect inside 160 x 160); --every K: every K-th picture in decode order; --gap G: luma samples between the
cells, a multiple of the chroma sampling.  A sheet takes 255 cells at the most (a compose target has 256 layers, one is the
background).  torch is imported before the library, so both share one HIP runtime."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BACKGROUND = (16, 128, 128)
MAX_CELLS = 255


def layout(n, cols=None):
    """(cols, rows) of a sheet of n cells"""
    cols = cols or max(1, math.isqrt(n - 1) + 1)
    return cols, (n + cols - 1) // cols


def sheet_target(n, cols, cell, sampling, gap=0):
    """the compose.Target of a sheet of n cells: pictures 0 .. n - 1 of the call are the cells, picture n is the flat background"""
    from hvqm4_amd import compose
    cols, rows = layout(n, cols)
    return compose.mosaic(cols, rows, cell, sampling, gap, BACKGROUND, sources=range(n), flat=n)


def clip_sheet(ctx, data, quality=90, cols=None, cell=None, every=1, gap=0):
    """-> (the sheet's geometry, the file as bytes, the ordinals of its cells) of one clip"""
    import torch
    from hvqm4_amd import compose, jpeg, scale
    from hvqm4_amd.container import parse_header, video_pictures
    hdr = parse_header(data)
    sampling = (hdr.h_samp, hdr.v_samp)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    ordinals = list(range(0, len(pics), every))
    n = len(ordinals)
    if not 1 <= n <= MAX_CELLS:
        raise ValueError(f"{n} cells: a sheet takes 1 .. {MAX_CELLS} (--every)")
    cell = cell or scale.fit(hdr.width, hdr.height, 160, 160)
    target = sheet_target(n, cols, cell, sampling, gap)
    sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, len(pics) + 3)
    for ft, p in pics:
        ctx.submit(sid, ft, p)
    ctx.flush()
    cells = ctx.scale_pictures([sid] * n, ordinals, cell)
    # streams that nothing is submitted to name the geometries of the caller's memory: the cells, and the sheet
    cell_sid = ctx.open_stream(cell[0], cell[1], hdr.h_samp, hdr.v_samp, hdr.is15, 3)
    sheet_sid = ctx.open_stream(target.size[0], target.size[1], hdr.h_samp, hdr.v_samp, hdr.is15, 3)
    flat = torch.from_numpy(compose.flat_picture(target.size, sampling, BACKGROUND)).cuda()
    sheet = ctx.compose_pictures([cell_sid] * n + [sheet_sid], [-1] * (n + 1), [target], src=[cells[i] for i in range(n)] + [flat])
    buffers, lengths = ctx.encode_jpeg([sheet_sid], [-1], quality=quality, src=[sheet[0]])
    files = jpeg.files(buffers, lengths)
    for s in (sheet_sid, cell_sid, sid):
        ctx.close_stream(s)
    return target.geometry(), files[0], ordinals


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("clip", help="an .h4m file")
    ap.add_argument("out", help="the .jpg file to write")
    ap.add_argument("--cols", type=int, default=None, metavar="N", help="cells a row")
    ap.add_argument("--cell", default=None, metavar="WxH", help="the size of a cell (multiples of 8)")
    ap.add_argument("--every", type=int, default=1, metavar="K", help="every K-th picture")
    ap.add_argument("--gap", type=int, default=0, metavar="G", help="luma samples between the cells")
    ap.add_argument("--quality", type=int, default=90, help="1 .. 100, scaled as the IJG library does")
    args = ap.parse_args()
    if not 1 <= args.quality <= 100:
        ap.error("--quality takes 1 .. 100")
    if args.every < 1 or (args.cols is not None and args.cols < 1):
        ap.error("--every and --cols take 1 at least")
    cell = None
    if args.cell:
        try:
            cell = tuple(int(v) for v in args.cell.lower().split("x"))
            assert len(cell) == 2
        except (ValueError, AssertionError):
            ap.error("--cell takes WxH")
    data = open(args.clip, "rb").read()
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    try:
        geom, file, ordinals = clip_sheet(ctx, data, args.quality, args.cols, cell, args.every, args.gap)
    except ValueError as e:
        ctx.close()
        ap.error(str(e))
    ctx.close()
    with open(args.out, "wb") as out:
        out.write(file)
    print(f"{len(ordinals)} pictures, sheet {geom[0]}x{geom[1]}, {len(file)} bytes, quality {args.quality} -> {args.out}")


if __name__ == "__main__":
    main()
