"""The planes and rules the corner tests share (tests/test_corner_cpu.py, tests/test_gpu_corners.py, tests/golden/make_corners.py).
threshold is 1 everywhere, except where a case is about the threshold.  numpy planes, uint8 [Ny][Nx], Nx a multiple of 4."""
import zlib

import numpy as np

from hvqm4_amd import corners as cr


def flat(ny, nx, v=77):
    return np.full((ny, nx), v, dtype=np.uint8)


def vertical_edge(ny, nx, at=None):
    a = np.zeros((ny, nx), dtype=np.uint8)
    a[:, (nx // 2 if at is None else at):] = 255
    return a


def checkerboard(ny, nx, block=1):
    y, x = np.mgrid[:ny, :nx]
    return (((y // block + x // block) & 1) * 255).astype(np.uint8)


def stripes4(ny, nx):
    """0, 0, 255, 255 along x: every |gx| is 1020, every gy 0"""
    return np.tile((((np.arange(nx) >> 1) & 1) * 255).astype(np.uint8), (ny, 1))


def quadrant(ny=24, nx=32, y0=10, x0=13):
    """255 for y >= y0, x >= x0: the header's known corner"""
    a = np.zeros((ny, nx), dtype=np.uint8)
    a[y0:, x0:] = 255
    return a


def blocks(ny, nx, at, size=3, v=255):
    """bright size x size blocks with their upper left samples at the (y, x) of `at`, cut to the plane"""
    a = np.zeros((ny, nx), dtype=np.uint8)
    for y, x in at:
        a[max(y, 0):y + size, max(x, 0):x + size] = v
    return a


def noise(ny, nx, seed):
    return np.random.default_rng(seed).integers(0, 256, (ny, nx), dtype=np.uint8)


def blobs(ny, nx, seed):
    """a few flat rectangles on a ramp: corners with wide flat surroundings, as natural pictures have"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:ny, :nx]
    a = ((x * 2 + y) & 255).astype(np.uint8)
    for _ in range(6):
        y0, x0 = int(rng.integers(0, ny)), int(rng.integers(0, nx))
        a[y0:y0 + int(rng.integers(2, 9)), x0:x0 + int(rng.integers(2, 12))] = int(rng.integers(0, 256))
    return a


# the rules every small plane goes through: both measures, every radius, every suppression distance the golden clips use
RULES = [cr.harris(r, 10, nms=m) for r in (1, 2, 3) for m in (0, 1, 3, 7)] + [cr.min_eigen(r, nms=m) for r in (1, 2, 3) for m in (0, 1, 3, 7)]
EXTREME = [cr.harris(3, 64, nms=1), cr.harris(3, 0, nms=1), cr.min_eigen(3, nms=1)]

# small planes for the plain-Python reference (a sample costs (2r + 1)^2 x 8 reads there)
SMALL = {
    "flat": flat(8, 12),
    "edge": vertical_edge(9, 12),
    "checker": checkerboard(12, 16),
    "checker2": checkerboard(12, 16, 2),
    "stripes": stripes4(9, 16),
    "quadrant": quadrant(14, 20, 6, 9),
    "noise": noise(13, 20, 1),
    "blobs": blobs(18, 24, 2),
    "narrow": noise(4, 4, 3),
    "square": blocks(16, 20, [(6, 8)], 4),
}


# ------------------------------------------------------------------------------------------------- pictures for the devices
TX, TY = 64, 16                                      # HVQ_CR_TX, HVQ_CR_TY
WIDE = (296, 160, 2, 1)                              # the 4:2:2 golden geometry: 4.6 x 10 tiles of luma
SEAM_COLUMNS = (0, 1, 62, 63, 64, 65, 127, 128, 295)
SEAM_ROWS = (0, 15, 16, 17, 159)


def nbytes(geom):
    w, h, hs, vs = geom
    return w * h + 2 * (w >> (hs == 2)) * (h >> (vs == 2))


def picture(geom, plane, a, seed):
    """a picture Y | U | V of random bytes whose plane `plane` is `a`"""
    pic = np.random.default_rng(seed).integers(0, 256, nbytes(geom), dtype=np.uint8)
    cr.plane_of(pic, geom, plane)[:] = a
    return pic


def seam_cases():
    """[(label, geom, picture, rule, response)]: one bright 3 x 3 block a picture, its upper left sample at every (row, column) of the
    seams, and one in the middle of a tile, (8 + 2 TY, 24 + 2 TX)"""
    r = cr.harris(1, 10, nms=3)
    at = [(y, x) for y in SEAM_ROWS for x in SEAM_COLUMNS] + [(8 + 2 * TY, 24 + 2 * TX)]
    return [(f"block at {p}", WIDE, picture(WIDE, 0, blocks(WIDE[1], WIDE[0], [p]), i), r, 0) for i, p in enumerate(at)]


def symmetric(ny, nx, seed):
    """a plane that is its own mirror image across the seam between its two middle columns, noise in blocks of 2 x 2"""
    half = np.repeat(np.repeat(noise(ny // 2, nx // 4, seed), 2, axis=0), 2, axis=1)
    return np.ascontiguousarray(np.concatenate([half, half[:, ::-1]], axis=1))


def small_bits(ny, nx, seed):
    """samples 0 and 1: the sums are small, so the radicand of the min-eigenvalue measure is a perfect square, or one less than one, at
    many samples"""
    return np.random.default_rng(seed).integers(0, 2, (ny, nx), dtype=np.uint8)


def tie_cases():
    sq = blocks(32, 128, [(10, 62)], 4)
    planes = [("square", sq), ("square, mirrored in x", sq[:, ::-1]), ("square, mirrored in y", sq[::-1]), ("square, mirrored in both", sq[::-1, ::-1]),
              ("symmetric across a seam", symmetric(32, 128, 4))]
    g = (128, 32, 1, 1)
    return [(f"{label}: {name}", g, picture(g, 0, np.ascontiguousarray(a), i), rule, 1)
            for i, (label, a) in enumerate(planes) for name, rule in (("harris", cr.harris(1, 10, nms=7)), ("min-eigen", cr.min_eigen(2, nms=7)))]


def arithmetic_cases():
    g = (72, 24, 1, 1)
    out = []
    for label, a in (("stripes", stripes4(24, 72)), ("2 x 2 checkerboard", checkerboard(24, 72, 2)), ("edge", vertical_edge(24, 72, 33)), ("bits", small_bits(24, 72, 6))):
        for name, rule in (("harris k 64 r 3", cr.harris(3, 64, nms=1)), ("harris k 0 r 3", cr.harris(3, 0, nms=1)), ("min-eigen r 3", cr.min_eigen(3, nms=1)),
                           ("min-eigen r 1", cr.min_eigen(1, nms=0))):
            out.append((f"{label}: {name}", g, picture(g, 2, a, len(out)), cr.Rule(2, rule.mode, rule.radius, rule.k, rule.nms, 0, 1), 1))
    return out


def narrow_cases():
    """8 x 8, whose chroma is 4 x 4 against a halo of 11: the smallest geometry a stream takes"""
    out = []
    for geom in ((8, 8, 2, 2), (8, 8, 1, 1), (16, 8, 2, 1)):
        for plane in range(3):
            ny, nx = cr.plane_shape(geom, plane)
            for rule in (cr.harris(3, 10, nms=7, plane=plane), cr.min_eigen(1, nms=0, plane=plane), cr.harris(1, 10, nms=3, plane=plane, margin=1)):
                out.append((f"{geom} plane {plane} {rule}", geom, picture(geom, plane, noise(ny, nx, len(out)), 50 + len(out)), rule, len(out) & 1))
    return out


def margin_cases():
    g = (72, 24, 2, 2)
    a = noise(24, 72, 9)
    return [(f"margin {m}", g, picture(g, 0, a, 3), cr.harris(1, 10, nms=1, margin=m), 0) for m in (0, 5, 11, 12, 36, 255)]


def threshold_cases():
    """a threshold equal to a corner's R, and that R + 1"""
    g = (72, 24, 2, 2)
    a = blobs(24, 72, 12)
    out = []
    for base in (cr.harris(1, 10, nms=3), cr.min_eigen(1, nms=3)):
        pts = cr.records(cr.of_plane(a, base)[1])
        assert pts.shape[0] >= 3
        R = int(np.sort(pts[:, 2])[pts.shape[0] // 2])
        for t in (R, R + 1):
            out.append((f"threshold {t}", g, picture(g, 0, a, 4), cr.Rule(0, base.mode, 1, base.k, 3, 0, t), 0))
    return out


def mixed_cases(n=60, nrules=64, seed=5):
    """-> (geoms, pictures, rules, which): n pictures of mixed geometries and contents under nrules distinct rules"""
    rng = np.random.default_rng(seed)
    geoms_all = [(64, 48, 2, 2), (48, 64, 1, 1), (72, 24, 2, 1), (8, 8, 2, 2), (136, 40, 2, 2)]
    rules = []
    while len(rules) < nrules:
        mode = int(rng.integers(0, 2))
        r = cr.Rule(int(rng.integers(0, 3)), mode, int(rng.integers(1, 4)), 0 if mode else int(rng.integers(0, 65)), int(rng.integers(0, 8)), int(rng.integers(0, 4)),
                    int(rng.integers(1, 1000)))
        if r not in rules:
            rules.append(r)
    geoms, pics, which = [], [], []
    for i in range(n):
        g = geoms_all[i % len(geoms_all)]
        w = int(rng.integers(0, nrules)) if i >= nrules else i % nrules
        ny, nx = cr.plane_shape(g, rules[w].plane)
        a = (noise, blobs, lambda y, x, s: checkerboard(y, x, 2))[i % 3](ny, nx, 100 + i)
        geoms.append(g); pics.append(picture(g, rules[w].plane, a, 200 + i)); which.append(w)
    return geoms, pics, rules, which


def device_cases():
    return seam_cases() + tie_cases() + arithmetic_cases() + narrow_cases() + margin_cases() + threshold_cases()


def cap_case():
    """(geom, picture, rule, K): a picture with a known number of corners, for cap in {0, 1, K - 1, K, K + 1}"""
    g = (72, 24, 2, 2)
    a = blobs(24, 72, 12)
    rule = cr.harris(1, 10, nms=3)
    return g, picture(g, 0, a, 4), rule, int(cr.of_plane(a, rule)[1][0, 0])


# ------------------------------------------------------------------------------------------------- tests/golden/corners.json
def fixture_rules():
    """the 72 rules of the fixture: every plane, both measures, r in {1, 2, 3}, nms in {0, 1, 3, 7}; threshold 1, k 10 under Harris"""
    return [cr.Rule(p, mode, r, 0 if mode else 10, m, 0, 1) for p in range(3) for mode in (0, 1) for r in (1, 2, 3) for m in (0, 1, 3, 7)]


def fixture_record(pic, geom, r):
    """K, rows[Ny] and the CRC-32 of the list, of the mask picture and of the row index"""
    mask, points, rows = cr.of_picture(pic, geom, r)
    return [int(points[0, 0]), int(rows[-1]), zlib.crc32(points.astype("<i8").tobytes()), zlib.crc32(mask.tobytes()), zlib.crc32(rows.astype("<u4").tobytes())]
