"""The case tables that tests/test_bilateral_cpu.py (numpy module, plain-Python reference, CPU fake device) and
tests/test_gpu_bilateral.py (the kernel) share: the parameter sets, the shapes, the made pictures, the directed arithmetic set and the
footprints to expect of single samples."""
import numpy as np

from hvqm4_amd import bilateral as B
from tests.rank_cases import SEAM_GEOM, SHAPES, SMALLEST, made, nbytes, plane_sizes, seam_points  # noqa: F401 -- shared with the rank unit

# the five parameter sets of the fixture and of the golden-clip cases
FIVE = [("gauss1.5_12", B.bilateral(1.5, 12)), ("sigma2_10", B.sigma_filter(2, 10)), ("box3x1", B.box((3, 1))), ("disc3", B.disc(3)),
        ("luma_sigma3_20", B.luma_only(B.sigma_filter(3, 20)))]
FOOTPRINT_RADII = [(1, 1), (7, 3), (7, 7), (0, 7), (7, 0)]
ALL255 = B.from_tables(7, 7, [[255] * 8] * 8, [255] * 256)         # the largest weights: num + den / 2 reaches the header's bound


def random_set(seed, rx, ry, zeros=True):
    """random tables; with `zeros` about a third of the spatial factors (never the centre) and of the range entries (never the first)
    are 0"""
    rng = np.random.default_rng([seed, rx, ry])
    sp = rng.integers(1, 256, (8, 8))
    rg = rng.integers(1, 256, 256)
    if zeros:
        sp[rng.random((8, 8)) < 0.33] = 0
        rg[rng.random(256) < 0.33] = 0
        sp[0, 0] = max(int(sp[0, 0]), 1)
        rg[0] = max(int(rg[0]), 1)
    return B.plane_from_tables(rx, ry, sp.tolist(), rg.tolist())


def points(nx, ny, part, border, parts=3):
    """seam_points of the rank cases -- the columns 0, 1, 62 .. 65, 127, 128, last and the rows 0, 15, 16, 17, last that the plane has --
    those on the plane's border (`border`) or the others"""
    on = lambda r, c: r in (0, ny - 1) or c in (0, nx - 1)
    return [(r, c) for r, c in seam_points(nx, ny, part, parts) if on(r, c) == border]


def dotted(geom, part, background, dot, border):
    """a picture of `background` with single samples `dot` at points() of every plane -> (bytes as uint8, the points per plane)"""
    out, pts = [], []
    for pw, ph in plane_sizes(geom):
        a = np.full((ph, pw), background, dtype=np.uint8)
        p = points(pw, ph, part, border)
        for r, c in p:
            a[r, c] = dot
        out.append(a.reshape(-1))
        pts.append(p)
    return np.concatenate(out), pts


def footprints(geom, pts, rx, ry, background, dot):
    """what the box mean of radii (rx, ry) makes of dotted() with INTERIOR points: a dot that does not lie on the border is seen once by
    every target of its rectangle [y - ry, y + ry] x [x - rx, x + rx] cut at the plane (the replicated border holds background only), so
    a target under k rectangles is (k dot + (den - k) background + den / 2) / den with den = (2 rx + 1)(2 ry + 1): the rectangles are
    painted by counting, without any window arithmetic"""
    den = (2 * rx + 1) * (2 * ry + 1)
    out = []
    for (pw, ph), p in zip(plane_sizes(geom), pts):
        k = np.zeros((ph, pw), dtype=np.int64)
        for r, c in p:
            assert 0 < r < ph - 1 and 0 < c < pw - 1
            k[max(r - ry, 0):min(r + ry, ph - 1) + 1, max(c - rx, 0):min(c + rx, pw - 1) + 1] += 1
        out.append(((k * dot + (den - k) * background + den // 2) // den).astype(np.uint8).reshape(-1))
    return np.concatenate(out)


ARITH_GEOM = (40, 24, 2, 1)


def _planes_of(geom, fn):
    return np.concatenate([fn(pw, ph, p).astype(np.uint8).reshape(-1) for p, (pw, ph) in enumerate(plane_sizes(geom))])


def arithmetic():
    """the directed arithmetic set: (label, geometry, picture, Bilateral)"""
    g = ARITH_GEOM
    grid = lambda pw, ph: np.mgrid[0:ph, 0:pw]
    full = _planes_of(g, lambda pw, ph, p: np.full((ph, pw), 255))
    one254 = full.copy()
    for at in (0, 40 * 11 + 17, 40 * 24 + 20 * 23 + 19, len(full) - 1):
        one254[at] = 254
    check1 = _planes_of(g, lambda pw, ph, p: ((grid(pw, ph)[0] + grid(pw, ph)[1]) & 1) * 255)
    check2 = _planes_of(g, lambda pw, ph, p: (((grid(pw, ph)[0] >> 1) + (grid(pw, ph)[1] >> 1)) & 1) * 255)
    small = _planes_of(g, lambda pw, ph, p: np.random.default_rng([p, pw]).integers(0, 4, (ph, pw)))
    den1 = B.from_tables(7, 7, [[1] + [0] * 7] + [[0] * 8] * 7, [1])
    half_row = B.from_tables(1, 0, [[2, 1]], [1] * 256)               # den 4: {0, 1, 0} gives 2 / 4
    half_quad = B.from_tables(1, 1, [[4, 2], [2, 1]], [3] * 256)       # den 48
    return [("all255/255", g, full, ALL255), ("all255/check1", g, check1, ALL255), ("all255/check2", g, check2, ALL255), ("all255/one254", g, one254, ALL255),
            ("den1/random", g, made(g, "random", 2), den1), ("den1/check1", g, check1, den1), ("half/row", g, small, half_row), ("half/quad", g, small, half_quad),
            ("small/all255", g, small, ALL255), ("small/gauss", g, small, B.bilateral(2.0, 1.0, 4)), ("small/sigma", g, small, B.sigma_filter((7, 2), 1)),
            ("check1/gauss", g, check1, B.bilateral(1.5, 200.0))]


def step(geom, lo=40, hi=200):
    """a two-level step lo | hi down the middle of every plane"""
    return _planes_of(geom, lambda pw, ph, p: np.where(np.mgrid[0:ph, 0:pw][1] < pw // 2, lo, hi))


STEP_KEEPER = B.from_tables(7, 7, [[255] * 8] * 8, [255] * 100)     # range[d] = 0 for d >= 100, every other weight 255


def table64():
    """64 distinct sets: many radii, luma and chroma different, Gaussians, thresholds, discs and random tables with zeros"""
    out = []
    for i in range(64):
        kind = i % 4
        if kind == 0:
            luma, chroma = B.bilateral(0.5 + 0.1 * i, 4 + i, (i // 4) % 8).luma, random_set(i, (i * 3) % 8, i % 8)
        elif kind == 1:
            luma, chroma = B.sigma_filter(((i // 4) % 8, (i * 5) % 8), i).luma, B.box((i % 3, i % 5)).luma
        elif kind == 2:
            luma, chroma = random_set(i, i % 8, (i // 8) % 8), B.disc(1 + i % 7, threshold=i).luma
        else:
            luma, chroma = B.disc(1 + (i // 4) % 7, sigma_range=3.0 + i).luma, B.IDENTITY_PLANE
        out.append(B.Bilateral(luma, chroma))
    assert len(set(out)) == 64
    return out
