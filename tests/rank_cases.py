"""The case tables that tests/test_rank_cpu.py (numpy module, plain-Python reference, CPU fake device) and tests/test_gpu_rank.py (the
kernel) share: the parameter sets, the shapes, the made pictures and the footprints to expect of single samples."""
import numpy as np

from hvqm4_amd import rank as R

SHAPES = ((64, 48, 2, 2), (48, 64, 1, 1), (296, 160, 2, 1))        # the golden ones; 148-wide chroma crosses a 64-column seam
SEAM_GEOM = SHAPES[2]
SMALLEST = (8, 8, 2, 2)                                            # the smallest geometry hvq_stream_open accepts: 4 x 4 chroma planes

# the five parameter sets of the fixture and of the golden-clip cases
FIVE = [("erode1", R.erode(1)), ("dilate3x1", R.dilate((3, 1))), ("range2", R.gradient(2)), ("median3", R.median(3)), ("median5", R.median(5))]
FOOTPRINT_RADII = [(1, 1), (7, 3), (15, 15), (0, 15), (15, 0)]
ALL_OPS = [R.erode((2, 1)), R.dilate((1, 2)), R.gradient((3, 3)), R.median(3), R.median(5)]


def plane_sizes(geom):
    w, h, hs, vs = geom
    return [(w, h), (w // hs, h // vs), (w // hs, h // vs)]


def nbytes(geom):
    return sum(pw * ph for pw, ph in plane_sizes(geom))


def seam_points(nx, ny, part, parts=3):
    """single samples at the columns 0, 1, 62, 63, 64, 65, 127, 128, last and the rows 0, 15, 16, 17, last that the plane has: pair (row
    i, column j) belongs to part (i + j) % parts, so that neighbouring footprints mostly stay apart"""
    cols = sorted({c for c in (0, 1, 62, 63, 64, 65, 127, 128, nx - 1) if c < nx})
    rows = sorted({r for r in (0, 15, 16, 17, ny - 1) if r < ny})
    return [(r, c) for i, r in enumerate(rows) for j, c in enumerate(cols) if (i + j) % parts == part]


def dotted(geom, part, background, dot):
    """a picture of `background` with single samples `dot` at seam_points of every plane -> (bytes as uint8, the points per plane)"""
    out, pts = [], []
    for pw, ph in plane_sizes(geom):
        a = np.full((ph, pw), background, dtype=np.uint8)
        p = seam_points(pw, ph, part)
        for r, c in p:
            a[r, c] = dot
        out.append(a.reshape(-1))
        pts.append(p)
    return np.concatenate(out), pts


def footprints(geom, pts, rx, ry, background, dot):
    """what MIN (dot 0 in 255) or MAX (dot 255 in 0) makes of dotted(): the rectangles [y - ry, y + ry] x [x - rx, x + rx] cut at the
    plane, painted without any window arithmetic"""
    out = []
    for (pw, ph), p in zip(plane_sizes(geom), pts):
        a = np.full((ph, pw), background, dtype=np.uint8)
        for r, c in p:
            a[max(r - ry, 0):min(r + ry, ph - 1) + 1, max(c - rx, 0):min(c + rx, pw - 1) + 1] = dot
        out.append(a.reshape(-1))
    return np.concatenate(out)


KINDS = ("check1", "check2", "ties", "random", "hramp", "vramp")


def made(geom, kind, k=0):
    """a made picture: 0 / 255 checkerboards of period 1 and 2 (a carry between the packed 16-bit halves shows there), random samples
    in 0 .. 3 (heavy ties), full-range random samples, a horizontal and a vertical ramp; in every plane"""
    out = []
    for p, (pw, ph) in enumerate(plane_sizes(geom)):
        y, x = np.mgrid[0:ph, 0:pw]
        rng = np.random.default_rng([k, p, pw, ph, KINDS.index(kind)])
        if kind == "check1":
            a = ((x + y + k) & 1) * 255
        elif kind == "check2":
            a = (((x >> 1) + (y >> 1) + k) & 1) * 255
        elif kind == "ties":
            a = rng.integers(0, 4, (ph, pw))
        elif kind == "random":
            a = rng.integers(0, 256, (ph, pw))
        elif kind == "hramp":
            a = x * 255 // max(pw - 1, 1)
        else:
            a = y * 255 // max(ph - 1, 1)
        out.append(a.astype(np.uint8).reshape(-1))
    return np.concatenate(out)


def table64():
    """64 distinct entries: every op, many radii, luma and chroma different"""
    out = []
    for i in range(64):
        op = i % 4
        if op == R.MEDIAN:
            luma = R.PlaneRank(R.MEDIAN, (i // 4) % 3, (i // 4) % 3)
            chroma = R.PlaneRank(R.MAX, i // 12, 0)
        else:
            luma = R.PlaneRank(op, i // 4, (i * 7) % 16)
            chroma = R.PlaneRank((op + 1) % 3, (i * 5) % 16, i // 4)
        out.append(R.Rank(luma, chroma))
    assert len(set(out)) == 64
    return out
