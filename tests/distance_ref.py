"""include/hvqm4_amd.h's text on hvq_distance_pictures and hvq_distance_mask, restated in plain Python with no numpy arithmetic and no
shared code with hvqm4_amd.distance: for every foreground sample the minimum over ALL background samples of the plane, plus the border
candidate.  Slow and obvious on purpose; the tests hold the module, the fake device and the GPU equal to it.

distance_by_rows is the same minimum taken row by row -- of a row's background samples only the one nearest in x can win, under each of
the three metrics -- for the planes that the brute force would take hours over (the golden clips of tests/golden/make_distance.py);
tests/test_distance_cpu.py holds the two equal on every small case."""
import bisect
import math

NONE = 0xFFFFFFFF
EUCLID2, CITY, CHESS = 0, 1, 2


def cost(metric, dx, dy):
    dx, dy = abs(dx), abs(dy)
    return dx * dx + dy * dy if metric == EUCLID2 else dx + dy if metric == CITY else max(dx, dy)


def _border(metric, x, y, nx, ny):
    e = min(x + 1, nx - x, y + 1, ny - y)
    return e * e if metric == EUCLID2 else e


def distance(plane, lo=255, hi=255, metric=EUCLID2, border=0):
    """plane: rows of samples -> rows of distances"""
    ny, nx = len(plane), len(plane[0])
    bg = [(x, y) for y in range(ny) for x in range(nx) if not lo <= int(plane[y][x]) <= hi]
    out = [[0] * nx for _ in range(ny)]
    for y in range(ny):
        for x in range(nx):
            if not lo <= int(plane[y][x]) <= hi:
                continue
            best = min((cost(metric, bx - x, by - y) for bx, by in bg), default=NONE)
            if border:
                best = min(best, _border(metric, x, y, nx, ny))
            out[y][x] = best
    return out


def distance_by_rows(plane, lo=255, hi=255, metric=EUCLID2, border=0):
    """the same values: per row of the plane the background sample nearest in x on either side"""
    ny, nx = len(plane), len(plane[0])
    rows = [[x for x in range(nx) if not lo <= int(plane[y][x]) <= hi] for y in range(ny)]
    out = [[0] * nx for _ in range(ny)]
    for y in range(ny):
        for x in range(nx):
            if not lo <= int(plane[y][x]) <= hi:
                continue
            best = NONE
            for by in range(ny):
                r = rows[by]
                k = bisect.bisect_left(r, x)
                if k < len(r):
                    best = min(best, cost(metric, r[k] - x, by - y))
                if k:
                    best = min(best, cost(metric, r[k - 1] - x, by - y))
            if border:
                best = min(best, _border(metric, x, y, nx, ny))
            out[y][x] = best
    return out


def mask(dist, mode=0, lo=0, hi=NONE, invert=0, chroma_samples=0):
    """the bytes of hvq_distance_mask for a Y map: Y, then 2 * chroma_samples bytes of 128.  mode 0 RANGE, 1 ROOT"""
    out = []
    for row in dist:
        for d in row:
            if mode == 1:
                out.append(min(255, math.isqrt(d)))
            else:
                out.append(255 if (lo <= d <= hi) != bool(invert) else 0)
    return bytes(out) + bytes([128]) * (2 * chroma_samples)


def erode_disc(plane, r):
    """rows of 0 / 255: a sample stays 255 when every sample of the plane within r of it is 255"""
    ny, nx = len(plane), len(plane[0])
    return [[255 if all(plane[py][px] == 255 for py in range(max(0, y - r), min(ny, y + r + 1)) for px in range(max(0, x - r), min(nx, x + r + 1))
                        if (px - x) ** 2 + (py - y) ** 2 <= r * r) else 0 for x in range(nx)] for y in range(ny)]


def dilate_disc(plane, r):
    """... becomes 255 when a 255 lies within r of it"""
    ny, nx = len(plane), len(plane[0])
    return [[255 if any(plane[py][px] == 255 for py in range(max(0, y - r), min(ny, y + r + 1)) for px in range(max(0, x - r), min(nx, x + r + 1))
                        if (px - x) ** 2 + (py - y) ** 2 <= r * r) else 0 for x in range(nx)] for y in range(ny)]
