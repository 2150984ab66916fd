"""What the label tests share (tests/test_label_cpu.py, tests/test_gpu_label.py, tests/golden/make_label.py): the planes, the masks and
the seam shapes, and the pictures that carry them.  T_x x T_y is the tile of hvqm4_amd/csrc/hvq_desc.h; every shape here is laid out
relative to it, so that it crosses the seams wherever the tile is."""
import os
import re

import numpy as np

from hvqm4_amd import labels as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DESC = open(os.path.join(ROOT, "hvqm4_amd", "csrc", "hvq_desc.h")).read()
TX = int(re.search(r"#define HVQ_LB_TX\s+(\d+)u", _DESC).group(1))
TY = int(re.search(r"#define HVQ_LB_TY\s+(\d+)u", _DESC).group(1))
STEP = 8                                             # the smallest legal step of a width or a height (of a 4:4:4 plane)

# (geometry, plane): 8 x 8 and its 4 x 4 chroma; exactly one tile; a tile plus the smallest step in x, in y, in both; 72 x 24 and 136 x 40
# in the three samplings with each plane as the rule's plane
PLANES = ([((8, 8, 2, 2), 0), ((8, 8, 2, 2), 1), ((8, 8, 1, 1), 2), ((TX, TY, 1, 1), 0), ((2 * TX, 2 * TY, 2, 2), 2),
           ((TX + STEP, TY, 1, 1), 0), ((TX, TY + STEP, 1, 1), 0), ((TX + STEP, TY + STEP, 1, 1), 0)]
          + [((w, h, hs, vs), p) for w, h in ((72, 24), (136, 40)) for hs, vs in ((2, 2), (2, 1), (1, 1)) for p in (0, 1, 2)])
SEAM_PLANES = [((2 * TX + STEP, 2 * TY + STEP, 1, 1), 0), ((4 * TX + 2 * STEP, 4 * TY + 2 * STEP, 2, 2), 1)]
WIDE = ((8192, 8, 1, 1), 0)                          # rows of 8192 samples, 8 rows


def fill_masks(nx, ny, seed):
    """(label, uint8 [ny][nx], lo, hi): empty, full, both checkerboards, random masks at four densities, a random plane through windows"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:ny, 0:nx]
    out = [("empty", np.zeros((ny, nx), np.uint8), 255, 255), ("full", np.full((ny, nx), 255, np.uint8), 255, 255),
           ("check0", (((xx + yy) & 1) == 0).astype(np.uint8) * 255, 255, 255), ("check1", (((xx + yy) & 1) == 1).astype(np.uint8) * 255, 255, 255)]
    for d in (0.3, 0.5, 0.6, 0.8):
        out.append((f"random {d}", (rng.random((ny, nx)) < d).astype(np.uint8) * 255, 255, 255))
    noise = rng.integers(0, 256, (ny, nx), dtype=np.uint8)
    out += [("window 100 .. 180", noise, 100, 180), ("window 0 .. 90", noise, 0, 90), ("window 7 .. 7", noise & 15, 7, 7)]
    return out


def serpentine(nx, ny):
    """one sample wide: every second row whole, joined at alternating ends: one component that crosses every vertical seam on every
    second row"""
    m = np.zeros((ny, nx), np.uint8)
    m[0::2] = 255
    for k, y in enumerate(range(1, ny - 1, 2)):
        m[y, nx - 1 if k % 2 == 0 else 0] = 255
    return m


def spiral(nx, ny):
    """a square spiral, one sample wide, a gap of one between its turns"""
    m = np.zeros((ny, nx), np.uint8)
    x0, y0, x1, y1 = 0, 0, nx - 1, ny - 1
    x, y = 0, 0
    m[0, 0] = 255
    while x1 - x0 >= 2 and y1 - y0 >= 2:
        m[y0, x0:x1 + 1] = 255
        m[y0:y1 + 1, x1] = 255
        m[y1, x0 + 2:x1 + 1] = 255
        m[y0 + 2:y1 + 1, x0 + 2] = 255
        x0, y0, x1, y1 = x0 + 2, y0 + 2, x1 - 2, y1 - 2
        if x1 - x0 >= 2 and y1 - y0 >= 2:
            m[y0, x0] = 255
    return m


def comb(nx, ny):
    """teeth in every second column that join only on the last row"""
    m = np.zeros((ny, nx), np.uint8)
    m[:, 0::2] = 255
    m[ny - 1] = 255
    return m


def us(nx, ny):
    """a "U" per tile column: two arms from row 0 to the last row, joined there; label c + 1 on both arms of column c"""
    m = np.zeros((ny, nx), np.uint8)
    for c in range((nx + TX - 1) // TX):
        a, b = c * TX + 1, min(c * TX + TX - 3, nx - 2)
        m[:, a] = m[:, b] = 255
        m[ny - 1, a:b + 1] = 255
    return m


def diagonals(nx, ny, both):
    """lines of slope 1 (and -1) through the tile corners: components under 8, single samples under 4"""
    yy, xx = np.mgrid[0:ny, 0:nx]
    m = (xx - yy) % TY == 0
    if both:
        m |= (xx + yy) % TY == 0
    return m.astype(np.uint8) * 255


def corner_blobs(nx, ny, anti):
    """two 8 x 8 blobs that touch only diagonally across the tile corner (TX, TY)"""
    m = np.zeros((ny, nx), np.uint8)
    if anti:
        m[TY - 8:TY, TX:TX + 8] = 255
        m[TY:TY + 8, TX - 8:TX] = 255
    else:
        m[TY - 8:TY, TX - 8:TX] = 255
        m[TY:TY + 8, TX:TX + 8] = 255
    return m


def seam_masks(nx, ny):
    out = [("serpentine", serpentine(nx, ny)), ("serpentine transposed", np.ascontiguousarray(serpentine(ny, nx).T)), ("spiral", spiral(nx, ny)),
           ("comb", comb(nx, ny)), ("U per tile column", us(nx, ny)), ("diagonals", diagonals(nx, ny, False)), ("lattice", diagonals(nx, ny, True))]
    if nx >= TX + 8 and ny >= TY + 8:
        out += [("corner blobs", corner_blobs(nx, ny, False)), ("corner blobs, anti", corner_blobs(nx, ny, True))]
    return [(label, m, 255, 255) for label, m in out]


def wide_masks():
    nx, ny = 8192, 8
    row = np.zeros((ny, nx), np.uint8)
    row[3] = 255
    return [("one row through every tile", row, 255, 255), ("serpentine", serpentine(nx, ny), 255, 255)]


def nbytes(geom):
    w, h, hs, vs = geom
    return w * h + 2 * (w >> (hs == 2)) * (h >> (vs == 2))


def picture(geom, plane, mask, seed):
    """a picture Y | U | V of random bytes whose plane `plane` is `mask`"""
    pic = np.random.default_rng(seed).integers(0, 256, nbytes(geom), dtype=np.uint8)
    L.plane_of(pic, geom, plane)[:] = mask
    return pic


def cases(planes, masks_of, seed=0):
    """[(label, geom, picture, Rule)] over planes x masks x both connectivities"""
    out = []
    for gi, (geom, plane) in enumerate(planes):
        ny, nx = L.plane_shape(geom, plane)
        for mi, (label, mask, lo, hi) in enumerate(masks_of(nx, ny, seed + gi) if masks_of is fill_masks else masks_of(nx, ny)):
            pic = picture(geom, plane, mask, 1000 * gi + mi + seed)
            for conn in (4, 8):
                out.append((f"{geom} plane {plane}: {label}, {conn}", geom, pic, L.Rule(plane, lo, hi, conn)))
    return out


def small_cases():
    return cases(PLANES, fill_masks)


def seam_cases():
    return cases(SEAM_PLANES + [PLANES[-1]], seam_masks)


def wide_cases():
    geom, plane = WIDE
    return [(f"{geom}: {label}, {conn}", geom, picture(geom, plane, mask, 7), L.Rule(plane, lo, hi, conn)) for label, mask, lo, hi in wide_masks() for conn in (4, 8)]


def mixed_cases(n=300, nrules=64, seed=5):
    """n pictures of random bytes over the small geometries and `nrules` distinct rules -> (geoms, pictures, rules, which)"""
    rng = np.random.default_rng(seed)
    rules = []
    while len(rules) < nrules:
        lo = int(rng.integers(0, 200))
        r = L.Rule(int(rng.integers(0, 3)), lo, int(rng.integers(lo, 256)), int(rng.choice([4, 8])))
        if r not in rules:
            rules.append(r)
    geoms = [PLANES[int(rng.integers(0, len(PLANES)))][0] for _ in range(n)]
    pics = [(rng.integers(0, 256, nbytes(g), dtype=np.uint8) & np.uint8(rng.choice([255, 0xC0, 0x80]))) for g in geoms]
    which = [(i * 7) % nrules for i in range(n)]
    return geoms, pics, rules, which


def counted_cases(cap=32):
    """K = cap - 1, cap and cap + 1: the first K white squares of a checkerboard of 16 x 8 under the 4-neighbourhood"""
    geom = (16, 8, 1, 1)
    yy, xx = np.mgrid[0:8, 0:16]
    white = np.flatnonzero(((xx + yy) & 1).reshape(-1) == 0)
    out = []
    for K in (cap - 1, cap, cap + 1):
        m = np.zeros(128, np.uint8)
        m[white[:K]] = 255
        out.append((f"{K} single samples", geom, picture(geom, 0, m.reshape(8, 16), K), L.Rule(0, 255, 255, 4)))
    return out


# every range bound at its edge (the made mask of select_mask has areas 6, 10, 10, 1 and a large one), invert, and the open selection
SELECTS = [L.select(), L.select(area=2), L.select(area=(6, 6)), L.select(area=(7, 9)), L.select(area=(None, 10)), L.select(width=(10, 10)), L.select(width=(None, 1)),
           L.select(width=11), L.select(height=(3, 10)), L.select(height=11), L.select(height=(None, 1)), L.select(area=2, invert=True), L.select(invert=True)]


def select_mask():
    """136 x 40: components of area 6 (2 x 3), 10 (10 x 1), 10 (1 x 10), 1, and a large one with a hole over tile seams"""
    mask = np.zeros((40, 136), np.uint8)
    mask[1:4, 1:3] = 255
    mask[1, 8:18] = 255
    mask[6:16, 70] = 255
    mask[10, 3] = 255
    mask[20:38, 60:130] = 255
    mask[25:30, 62:66] = 0
    return mask
