"""What the distance tests share (tests/test_distance_cpu.py, tests/test_gpu_distance.py): the planes, the masks and the rules, and the
pictures that carry them.  COLS (the columns of a workgroup of the column pass), SPAN (the samples of a workgroup of the row pass) and
TILE (the samples of a tile of the mask call) are hvqm4_amd/csrc/hvq_desc.h's; the planes here are laid out relative to them, so that
they cross the seams wherever the constants put them."""
import os
import re

import numpy as np

from hvqm4_amd import distance as D
from hvqm4_amd import labels as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DESC = open(os.path.join(ROOT, "hvqm4_amd", "csrc", "hvq_desc.h")).read()


def _const(name):
    return int(re.search(r"#define " + name + r"\s+(\d+)u", _DESC).group(1))


COLS = _const("HVQ_DT_CLANES") * 4
SPAN = _const("HVQ_DT_SPAN")
LANES = _const("HVQ_DT_LANES")
TILE = _const("HVQ_MP_LANES") * _const("HVQ_MP_PER") * 4
STEP = 8                                             # the smallest legal step of a width or a height (of a 4:4:4 plane)
COMBOS = [(m, b) for m in (0, 1, 2) for b in (0, 1)]  # every metric under both borders


def _up(v):
    return (v + STEP - 1) // STEP * STEP


NX = 72                                              # a width that is no multiple of anything here
ROWS = SPAN // NX                                    # the rows of a workgroup of the row pass at that width
# (geometry, plane): 8 x 8 and its 4 x 4 chroma, 16 x 8, 24 x 16 -- small enough for the brute force
SMALL_PLANES = [((8, 8, 2, 2), 0), ((8, 8, 2, 2), 1), ((16, 8, 1, 1), 2), ((24, 16, 2, 1), 0)]
# 72 x 24 in the three samplings with each plane; one column group and a step; the rows of one row group and a step (which is also
# more samples than a tile of the mask call); two row groups and two tiles exactly
TILE_PLANES = ([((NX, 24, hs, vs), p) for hs, vs in ((2, 2), (2, 1), (1, 1)) for p in (0, 1, 2)]
               + [((COLS + STEP, 8, 1, 1), 0), ((2 * (COLS + STEP), 16, 2, 2), 1), ((NX, _up(ROWS + 1), 1, 1), 0), ((SPAN // 64, 128, 1, 1), 0)])
WIDE = ((8192, 8, 1, 1), 0)                          # rows of 8192 samples: a row group is ONE row (8 rows: no geometry has a plane of 8192 x 4)
FAR = ((200, 136, 1, 1), 0)                          # the long outward walk: one background sample in a corner
assert _up(ROWS + 1) * NX > TILE and COLS + STEP > COLS


def fill_masks(nx, ny, seed):
    """(label, uint8 [ny][nx], lo, hi): empty, full, a checkerboard, one background sample in each corner, one foreground sample, stripes
    whose period straddles a dword, random masks at three foreground densities, a random plane through windows"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:ny, 0:nx]
    out = [("empty", np.zeros((ny, nx), np.uint8), 255, 255), ("full", np.full((ny, nx), 255, np.uint8), 255, 255),
           ("check", (((xx + yy) & 1) == 0).astype(np.uint8) * 255, 255, 255)]
    for cx, cy in ((0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1)):
        m = np.full((ny, nx), 255, np.uint8)
        m[cy, cx] = 0
        out.append((f"background only at ({cx}, {cy})", m, 255, 255))
    m = np.zeros((ny, nx), np.uint8)
    m[ny // 2, nx // 3] = 255
    out.append(("one foreground sample", m, 255, 255))
    out += [("vertical stripes, period 3", ((xx % 3) != 0).astype(np.uint8) * 255, 255, 255), ("vertical stripes, period 5", ((xx % 5) < 3).astype(np.uint8) * 255, 255, 255),
            ("horizontal stripes, period 3", ((yy % 3) != 1).astype(np.uint8) * 255, 255, 255)]
    for d in (0.5, 0.9, 0.99):
        out.append((f"random {d}", (rng.random((ny, nx)) < d).astype(np.uint8) * 255, 255, 255))
    noise = rng.integers(0, 256, (ny, nx), dtype=np.uint8)
    out += [("window 100 .. 180", noise, 100, 180), ("window 0 .. 90", noise, 0, 90), ("window 7 .. 7", noise & 15, 7, 7)]
    return out


def nbytes(geom):
    w, h, hs, vs = geom
    return w * h + 2 * (w >> (hs == 2)) * (h >> (vs == 2))


def picture(geom, plane, mask, seed):
    """a picture Y | U | V of random bytes whose plane `plane` is `mask`"""
    pic = np.random.default_rng(seed).integers(0, 256, nbytes(geom), dtype=np.uint8)
    L.plane_of(pic, geom, plane)[:] = mask
    return pic


def cases(planes, every_combo, seed=0):
    """[(label, geom, picture, Rule)] over planes x masks, under every metric and border (every_combo) or under one of the six in turn"""
    out = []
    for gi, (geom, plane) in enumerate(planes):
        ny, nx = L.plane_shape(geom, plane)
        for mi, (label, mask, lo, hi) in enumerate(fill_masks(nx, ny, seed + gi)):
            pic = picture(geom, plane, mask, 1000 * gi + mi + seed)
            for m, b in (COMBOS if every_combo else [COMBOS[(gi + mi) % 6]]):
                out.append((f"{geom} plane {plane}: {label}, {D.METRICS[m]}, border {b}", geom, pic, D.Rule(plane, lo, hi, m, b)))
    return out


def small_cases():
    return cases(SMALL_PLANES, True)


def tile_cases():
    return cases(TILE_PLANES, False, seed=50)


def far_cases():
    """200 x 136: the only background sample in each corner, under every metric; border 1 once"""
    geom, plane = FAR
    out = []
    for k, (cx, cy) in enumerate(((0, 0), (199, 0), (0, 135), (199, 135))):
        m = np.full((136, 200), 255, np.uint8)
        m[cy, cx] = 0
        pic = picture(geom, plane, m, 70 + k)
        for metric in (0, 1, 2):
            out.append((f"{geom}: background only at ({cx}, {cy}), {D.METRICS[metric]}", geom, pic, D.Rule(0, 255, 255, metric, 0)))
    out.append((f"{geom}: background only at (199, 135), euclid2, border 1", geom, pic, D.Rule(0, 255, 255, 0, 1)))
    return out


def wide_cases():
    """foreground in the rows 2 and 5 only (the module's dense product is slow on rows this wide), background elsewhere"""
    geom, plane = WIDE
    rng = np.random.default_rng(8)
    xx = np.mgrid[0:8, 0:8192][1]
    rows = np.zeros((8, 8192), bool)
    rows[[2, 5]] = True
    lone = rows.copy()
    lone[:, 5000] = False
    lone[:, :3000] = False
    return [(f"{geom}: random 0.9, euclid2", geom, picture(geom, plane, (rows & (rng.random((8, 8192)) < 0.9)).astype(np.uint8) * 255, 7), D.Rule(0, 255, 255, 0, 0)),
            (f"{geom}: stripes of period 37, city, border 1", geom, picture(geom, plane, (rows & ((xx % 37) != 0)).astype(np.uint8) * 255, 8), D.Rule(0, 255, 255, 1, 1)),
            (f"{geom}: runs of 2000 and 3191 samples, chess", geom, picture(geom, plane, lone.astype(np.uint8) * 255, 9), D.Rule(0, 255, 255, 2, 0))]


def mixed_cases(n=60, nrules=64, seed=5):
    """n pictures of random bytes over the small and the 72 x 24 geometries and `nrules` distinct rules -> (geoms, pictures, rules, which)"""
    rng = np.random.default_rng(seed)
    rules = []
    while len(rules) < nrules:
        lo = int(rng.integers(0, 200))
        r = D.Rule(int(rng.integers(0, 3)), lo, int(rng.integers(lo, 256)), int(rng.integers(0, 3)), int(rng.integers(0, 2)))
        if r not in rules:
            rules.append(r)
    pool = SMALL_PLANES + TILE_PLANES[:9]
    geoms = [pool[int(rng.integers(0, len(pool)))][0] for _ in range(n)]
    pics = [(rng.integers(0, 256, nbytes(g), dtype=np.uint8) & np.uint8(rng.choice([255, 0xC0, 0x80]))) for g in geoms]
    which = [(i * 7) % nrules for i in range(n)]
    return geoms, pics, rules, which


# every mode, the range's bounds at their edges (the map of mask_picture holds 0, 1, 4, 9 and 10 among others), NONE, invert
MASKS = [D.mask_range(0), D.mask_range(1), D.mask_range(0, 0), D.mask_range(10, D.NONE), D.mask_range(4, 9), D.mask_range(5, 8), D.mask_range(D.NONE, D.NONE),
         D.mask_range(0, D.NONE - 1), D.mask_range(10, D.NONE, invert=True), D.mask_range(1, 4, invert=True), D.mask_root()]


def mask_picture():
    """136 x 40: a large blob with a hole, a line and a square, whose squared distances hold 0, 1, 4, 9 and 10; no plane this small reaches
    255^2, so the tests add made values for ROOT's last steps"""
    m = np.zeros((40, 136), np.uint8)
    m[2:38, 4:60] = 255
    m[10:14, 20:24] = 0
    m[5, 70:130] = 255
    m[20:31, 80:91] = 255
    return m


def morph_masks(nx, ny, seed):
    """0 / 255 masks for the disc steps: blobs, specks, holes and a frame that touches every edge"""
    rng = np.random.default_rng(seed)
    blobs = np.zeros((ny, nx), np.uint8)
    blobs[2:ny - 3, 3:nx // 2] = 255
    blobs[ny // 2, nx // 4] = 0
    blobs[1, nx - 4] = 255
    blobs[ny // 3:ny // 3 + 7, nx // 2 + 4:nx - 2] = 255
    frame = np.full((ny, nx), 255, np.uint8)
    frame[4:ny - 4, 4:nx - 4] = 0
    return [("blobs", blobs), ("frame", frame), ("random 0.7", (rng.random((ny, nx)) < 0.7).astype(np.uint8) * 255), ("empty", np.zeros((ny, nx), np.uint8)),
            ("full", np.full((ny, nx), 255, np.uint8))]
