"""What the integral tests share (tests/test_integral_cpu.py, tests/test_gpu_integral.py): the planes, the rules and the rectangles,
and the pictures that carry them.  CHUNK (the samples of a wave a step of the row pass), COLS (the columns of a workgroup of the column
pass), WAVES (the rows of a workgroup of the row pass) and the window tile TX x TY are hvqm4_amd/csrc/hvq_desc.h's; the planes here are
laid out relative to them, so that they cross the seams wherever the constants put them.

A geometry's width and height are multiples of 8, so a plane's are multiples of 4 (a subsampled chroma plane) or 8: there is no plane of
height 1 or 17 and none 68 x 17.  The smallest height is 4, which is one row group of the built shape exactly, and every height is whole
row groups; the window's seams are crossed by 72 x 24 (a tile and 8 either way) and by 136 x 40; a chunk and a dword is the 260 x 8
chroma plane of 520 x 8 in 4:2:2, which is also a column group and 4."""
import os
import re

import numpy as np

from hvqm4_amd import integral as I
from hvqm4_amd import labels as L
from tests.distance_cases import nbytes, picture  # noqa: F401  (a picture of random bytes whose plane is given)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DESC = open(os.path.join(ROOT, "hvqm4_amd", "csrc", "hvq_desc.h")).read()


def _const(name):
    return int(re.search(r"#define " + name + r"\s+(\d+)u", _DESC).group(1))


WAVE = _const("HVQ_IG_WAVE")
WAVES = _const("HVQ_IG_WAVES")
CHUNK = WAVE * 4
COLS = _const("HVQ_IG_CLANES") * 4
TX, TY = _const("HVQ_WN_TX"), _const("HVQ_WN_TY")

# (geometry, plane) for the tables: 4 x 4, 8 x 4, 8 x 8; one chunk, a chunk and a dword (a column group and 4), a chunk and 8; 72 x 24 in
# the three samplings with each plane; a window tile, 68 x 20; 8192 x 8: the carry across 32 chunks
TABLE_PLANES = ([((8, 8, 2, 2), 1), ((16, 8, 2, 2), 2), ((8, 8, 1, 1), 0), ((CHUNK, 8, 1, 1), 0), ((2 * (CHUNK + 4), 8, 2, 1), 1), ((CHUNK + 8, 8, 1, 1), 2)]
                + [((72, 24, hs, vs), p) for hs, vs in ((2, 2), (2, 1), (1, 1)) for p in (0, 1, 2)]
                + [((TX, TY, 1, 1), 0), ((2 * (TX + 4), 2 * (TY + 4), 2, 2), 1)])
WIDE = ((8192, 8, 1, 1), 0)
WRAP = (8192, 2064, 2, 2)                            # 255 everywhere: S(Nx - 1, Ny - 1) passes 2^32
# planes of Y's size for the windows: the smallest, a tile, a tile and 8 either way, a chunk and 8, two tiles and 8 across
WINDOW_PLANES = [((8, 8, 2, 2), 0), ((8, 8, 1, 1), 1), ((TX, TY, 2, 1), 0), ((TX + 8, TY + 8, 1, 1), 2), ((CHUNK + 8, 8, 2, 2), 0), ((2 * TX + 8, 2 * TY + 8, 2, 2), 0)]
BRUTE_PLANES = [((8, 8, 2, 2), 0), ((8, 8, 1, 1), 1), ((24, 16, 2, 1), 0)]     # small enough for the brute force
WINDOWS = [(0, 0), (1, 1), (7, 3), (0, 40), (40, 0), (25, 25), (8191, 8191)]
# every mode; THRESHOLD with k in {0, 51, -51}, c in {-3, 0, 7}, both inverts: (mode, k, c, invert)
SPECS = [(I.MEAN, 0, 0, 0), (I.DEVIATION, 0, 0, 0)] + [(I.THRESHOLD, k, c, inv) for k in (0, 51, -51) for c in (-3, 0, 7) for inv in (0, 1)]
assert len(SPECS) == 20 and TX + 8 > TX and CHUNK + 4 == COLS + 4


def fills(nx, ny, seed):
    """(label, uint8 [ny][nx]): the 0 / 255 checkerboard, all 0, all 255, random bytes, random bytes under a ramp of light"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:ny, 0:nx]
    ramp = (rng.integers(0, 96, (ny, nx)) + 160 * xx // max(1, nx - 1)).astype(np.uint8)
    return [("check", (((xx + yy) & 1) * 255).astype(np.uint8)), ("zeros", np.zeros((ny, nx), np.uint8)), ("all 255", np.full((ny, nx), 255, np.uint8)),
            ("random", rng.integers(0, 256, (ny, nx), dtype=np.uint8)), ("ramp", ramp)]


def table_cases(planes=None):
    """[(label, geom, picture, plane)] over planes x fills"""
    out = []
    for gi, (geom, plane) in enumerate(TABLE_PLANES if planes is None else planes):
        ny, nx = L.plane_shape(geom, plane)
        for fi, (label, a) in enumerate(fills(nx, ny, 300 + gi)):
            out.append((f"{geom} plane {plane}: {label}", geom, picture(geom, plane, a, 3000 + 10 * gi + fi), plane))
    return out


def wide_cases():
    """8192 x 8: random bytes, and all 255 (every chunk's carry at its largest)"""
    geom, plane = WIDE
    fs = fills(8192, 8, 77)
    return [(f"{geom}: {fs[k][0]}", geom, picture(geom, plane, fs[k][1], 3900 + k), plane) for k in (3, 2)]


def window_cases(planes=None, every=False):
    """[(label, geom, picture, Rule)] over planes x fills x windows; the specs in turn, so that every one meets every window (every: all
    20 specs under every window, for the brute force's smallest plane)"""
    out, turn = [], 0
    for gi, (geom, plane) in enumerate(WINDOW_PLANES if planes is None else planes):
        ny, nx = L.plane_shape(geom, plane)
        for fi, (label, a) in enumerate(fills(nx, ny, 500 + gi)):
            pic = picture(geom, plane, a, 5000 + 10 * gi + fi)
            for wi, (rx, ry) in enumerate(WINDOWS):
                for mode, k, c, inv in (SPECS if every else [SPECS[(turn + 3 * wi) % 20], SPECS[(turn + 3 * wi + 7) % 20]]):
                    out.append((f"{geom} plane {plane}: {label}, window ({rx}, {ry}), mode {mode}, k {k}, c {c}, invert {inv}", geom, pic,
                                I.Rule(plane, mode, rx, ry, k, c, inv)))
            turn += 1
    return out


def mixed_cases(n=60, nrules=64, seed=6):
    """n pictures of random bytes over the window geometries and `nrules` distinct rules -> (geoms, pictures, rules, which)"""
    rng = np.random.default_rng(seed)
    rules = []
    while len(rules) < nrules:
        mode, k, c, inv = SPECS[int(rng.integers(0, 20))]
        r = I.Rule(0, mode, int(rng.integers(0, 48)), int(rng.integers(0, 48)), k, c, inv)
        if r not in rules:
            rules.append(r)
    pool = [g for g, p in WINDOW_PLANES if p == 0]
    geoms = [pool[int(rng.integers(0, len(pool)))] for _ in range(n)]
    pics = [rng.integers(0, 256, nbytes(g), dtype=np.uint8) for g in geoms]
    which = [(i * 7) % nrules for i in range(n)]
    return geoms, pics, rules, which


def rect_cases(count=300, seed=9):
    """`count` rectangles over six pictures (the last one without a table of squares) -> (geoms, pictures, planes, rects int32 [count][5]):
    single samples, whole planes, random ones, and one of each refused kind: a corner outside the plane, x1 < x0, y1 < y0, a negative
    corner, an i of -1 and an i past the pictures.  More than 2^24 samples fit only the WRAP plane, whose test has that one"""
    rng = np.random.default_rng(seed)
    chosen = [TABLE_PLANES[k] for k in (0, 4, 6, 10, 14, 16)]
    geoms, planes = [g for g, _p in chosen], [p for _g, p in chosen]
    pics = [rng.integers(0, 256, nbytes(g), dtype=np.uint8) for g in geoms]
    shapes = [L.plane_shape(g, p) for g, p in chosen]
    rects = []
    for i, (ny, nx) in enumerate(shapes):
        rects += [(i, 0, 0, nx - 1, ny - 1), (i, 0, 0, 0, 0), (i, nx - 1, ny - 1, nx - 1, ny - 1), (i, nx - 1, 0, nx - 1, ny - 1), (i, 0, ny - 1, nx - 1, ny - 1)]
    ny, nx = shapes[2]
    rects += [(2, 0, 0, nx, ny - 1), (2, 0, 0, nx - 1, ny), (2, 5, 0, 4, 3), (2, 0, 3, 4, 2), (2, -1, 0, 4, 3), (2, 0, -1, 4, 3), (-1, 0, 0, 1, 1), (len(chosen), 0, 0, 1, 1),
              (2 ** 31 - 1, 0, 0, 1, 1), (2, 0, 0, 2 ** 31 - 1, 1)]
    while len(rects) < count:
        i = int(rng.integers(0, len(chosen)))
        ny, nx = shapes[i]
        x0, y0 = int(rng.integers(0, nx)), int(rng.integers(0, ny))
        rects.append((i, x0, y0, int(rng.integers(x0, nx)), int(rng.integers(y0, ny))))
    return geoms, pics, planes, np.array(rects, dtype=np.int32)
