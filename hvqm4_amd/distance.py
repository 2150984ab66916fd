"""Exact distance transforms of pictures in slot layout (hvq_distance_pictures / Context.distance_pictures, hvq_distance_mask /
Context.distance_mask, Context.disc_morph): the rules, the values to expect, and the helpers around a distance map.  numpy only.

A rule names a plane (0 Y, 1 U, 2 V), a window lo <= a <= hi of the samples that are foreground, a metric -- "euclid2" (squared
Euclidean), "city" (city block) or "chess" (chessboard) -- and whether the samples just outside the plane count as background
(border).  include/hvqm4_amd.h specifies the result: uint32 [Ny][Nx], 0 on the background, the exact integer distance to the nearest
background sample on the foreground, NONE where there is none.  of_plane computes it on the host with an algorithm of its own -- the
columns by running maxima of the last background row, the rows as a dense min-plus product of every row with the metric, no search and no
early end --, which shares nothing with the kernels' walks.  A geometry is (width, height, h_samp, v_samp).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .labels import plane_of, plane_shape

NONE = 0xFFFFFFFF                      # HVQ_DST_NONE
MAX_RULES = 64                         # HVQ_DST_MAX_RULES
MAX_MASKS = 64                         # HVQ_DSM_MAX
METRICS = ("euclid2", "city", "chess")  # HVQ_DST_EUCLID2, _CITY, _CHESS
RANGE, ROOT = 0, 1                     # HVQ_DSM_RANGE, _ROOT
_FAR = 1 << 20                         # a vertical distance that stands for "none": above every real one, its square fits int64


def _int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


@dataclass(frozen=True)
class Rule:
    """the foreground of one plane, the metric (an index of METRICS) and the border rule (0 or 1).  Hashable."""
    plane: int = 0
    lo: int = 255
    hi: int = 255
    metric: int = 0
    border: int = 0

    def struct(self):
        """the HvqDistanceRule of include/hvqm4_amd.h (ctypes)"""
        from ._lib import HvqDistanceRule
        check(self)
        return HvqDistanceRule(self.plane, self.lo, self.hi, self.metric, self.border)


def rule(plane: int = 0, lo: int = 255, hi: int = 255, metric="euclid2", border: bool = False) -> Rule:
    """the samples lo .. hi of `plane` under `metric` (a name of METRICS, or its index); the default reads an Otsu mask of Y"""
    if isinstance(metric, str):
        if metric not in METRICS:
            raise ValueError(f"metric {metric!r}: one of {METRICS}")
        metric = METRICS.index(metric)
    r = Rule(plane, lo, hi, metric, int(bool(border)))
    check(r)
    return r


def check(r: Rule) -> None:
    """ValueError for what hvq_distance_check refuses"""
    if not isinstance(r, Rule):
        raise ValueError(f"a distance.Rule, not {type(r).__name__}")
    if not _int(r.plane) or not 0 <= r.plane <= 2:
        raise ValueError(f"plane {r.plane!r}: 0 Y, 1 U, 2 V")
    if not _int(r.lo) or not _int(r.hi) or not 0 <= r.lo <= r.hi <= 255:
        raise ValueError(f"window {r.lo!r} .. {r.hi!r}: 0 <= lo <= hi <= 255")
    if not _int(r.metric) or not 0 <= r.metric <= 2:
        raise ValueError(f"metric {r.metric!r}: 0 euclid2, 1 city, 2 chess")
    if not _int(r.border) or r.border not in (0, 1):
        raise ValueError(f"border {r.border!r}: 0 or 1")


def complement(r: Rule) -> Rule:
    """the rule whose foreground is r's background, for a window that touches an end of 0 .. 255 (a mask's 255s, its 0s)"""
    check(r)
    if r.lo == 0 and r.hi < 255:
        return Rule(r.plane, r.hi + 1, 255, r.metric, r.border)
    if r.hi == 255 and r.lo > 0:
        return Rule(r.plane, 0, r.lo - 1, r.metric, r.border)
    raise ValueError(f"the complement of the window {r.lo} .. {r.hi} is no window")


def distance_bytes(geom, plane: int = 0) -> int:
    """hvq_distance_bytes: the bytes of the distance map of that plane"""
    ny, nx = plane_shape(geom, plane)
    return 4 * nx * ny


# ------------------------------------------------------------------------------------------------------------ the values
def _vertical(fg: np.ndarray, border: int) -> np.ndarray:
    """int64 [Ny][Nx]: the distance of every sample to the nearest background sample of its column (rows -1 and Ny under border),
    _FAR where the column has none: the running maximum of the last background row from above, the running minimum from below"""
    ny, nx = fg.shape
    rows = np.arange(ny, dtype=np.int64)[:, None]
    above = np.maximum.accumulate(np.where(fg, -_FAR, rows), axis=0)
    below = np.minimum.accumulate(np.where(fg, 2 * _FAR, rows)[::-1], axis=0)[::-1]
    if border:
        above = np.maximum(above, -1)
        below = np.minimum(below, ny)
    return np.minimum(np.minimum(rows - above, below - rows), _FAR)


def of_plane(a, r: Optional[Rule] = None) -> np.ndarray:
    """the distance map of a plane uint8 [Ny][Nx] -> uint32 [Ny][Nx]"""
    r = Rule() if r is None else r
    check(r)
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError("a plane is a uint8 array [Ny][Nx]")
    ny, nx = a.shape
    fg = (a >= r.lo) & (a <= r.hi)
    g = _vertical(fg, r.border)
    xs = np.arange(nx, dtype=np.int64)
    out = np.zeros((ny, nx), dtype=np.int64)
    cols = max(1, min(nx, (1 << 22) // nx))                                          # targets a block: cols x nx candidates a row
    for x0 in range(0, nx, cols):
        d = np.abs(xs[x0:x0 + cols, None] - xs[None, :])                             # [target][source]
        if r.metric == 0:
            d = d * d
        for y in range(ny):
            t = np.flatnonzero(fg[y, x0:x0 + cols])                                  # the background keeps its 0
            if not t.size:
                continue
            gy = g[y][None, :]
            c = d[t] + gy * gy if r.metric == 0 else d[t] + gy if r.metric == 1 else np.maximum(d[t], gy)
            out[y, x0 + t] = c.min(axis=1)
    if r.border:
        e = np.minimum(xs + 1, nx - xs)[None, :]
        out = np.minimum(out, e * e if r.metric == 0 else e)
    out[out >= (_FAR * _FAR if r.metric == 0 else _FAR)] = NONE                      # only a candidate made of _FAR gets there
    out[~fg] = 0
    return out.astype(np.uint32)


def of_picture(yuv, geom, r: Optional[Rule] = None) -> np.ndarray:
    """of_plane on the rule's plane of a picture Y | U | V of geometry `geom`"""
    r = Rule() if r is None else r
    check(r)
    return of_plane(plane_of(yuv, geom, r.plane), r)


# ------------------------------------------------------------------------------------------------------------ masks from distances
@dataclass(frozen=True)
class Mask:
    """an entry of hvq_distance_mask: RANGE with an inclusive range of distances and invert, or ROOT.  Hashable."""
    mode: int = RANGE
    lo: int = 0
    hi: int = NONE
    invert: int = 0

    def struct(self):
        """the HvqDistanceMask of include/hvqm4_amd.h (ctypes)"""
        from ._lib import HvqDistanceMask
        check_mask(self)
        return HvqDistanceMask(self.mode, self.lo, self.hi, self.invert)


def check_mask(m: Mask) -> None:
    """ValueError for what hvq_distance_mask_check refuses"""
    if not isinstance(m, Mask):
        raise ValueError(f"a distance.Mask, not {type(m).__name__}")
    if not _int(m.mode) or m.mode not in (RANGE, ROOT):
        raise ValueError(f"mode {m.mode!r}: 0 RANGE, 1 ROOT")
    if not _int(m.lo) or not _int(m.hi) or not 0 <= m.lo <= m.hi <= NONE:
        raise ValueError(f"range {m.lo!r} .. {m.hi!r}: 0 <= lo <= hi < 2^32")
    if not _int(m.invert) or m.invert not in (0, 1):
        raise ValueError(f"invert {m.invert!r}: 0 or 1")
    if m.mode == ROOT and (m.lo or m.hi or m.invert):
        raise ValueError("ROOT takes lo, hi and invert 0")


def mask_range(lo: int, hi: int = NONE, invert: bool = False) -> Mask:
    """Y 255 where lo <= d <= hi, else 0; invert swaps the two.  NONE is an ordinary value: hi = NONE includes it"""
    m = Mask(RANGE, lo, hi, int(bool(invert)))
    check_mask(m)
    return m


def mask_root() -> Mask:
    """Y min(255, isqrt(d)): the viewable field under euclid2"""
    return Mask(ROOT, 0, 0, 0)


def isqrt(v) -> np.ndarray:
    """the exact floor square root of uint32 values -> int64: the float64 root (53 bits hold a uint32), then a step of correction either
    way"""
    v = np.asarray(v).astype(np.int64) & NONE
    s = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    s = np.where(s * s > v, s - 1, s)
    return np.where((s + 1) * (s + 1) <= v, s + 1, s)


def _map(dist, geom) -> np.ndarray:
    w, h, _hs, _vs = geom
    return (np.asarray(dist).astype(np.int64) & NONE).reshape(h, w)                   # an int32 view of the map reads NONE as -1


def of_mask(dist, m: Mask, geom) -> np.ndarray:
    """the bytes hvq_distance_mask writes for one picture: `dist` the map [h][w] of its Y plane (uint32, or the int32 view)"""
    check_mask(m)
    d = _map(dist, geom)
    if m.mode == ROOT:
        y = np.minimum(255, isqrt(d)).astype(np.uint8)
    else:
        y = np.where(((d >= m.lo) & (d <= m.hi)) ^ bool(m.invert), 255, 0).astype(np.uint8)
    cy, cx = plane_shape(geom, 1)
    return np.concatenate([y.reshape(-1), np.full(2 * cx * cy, 128, dtype=np.uint8)])


# ------------------------------------------------------------------------------------------------------------ discs
def _radius(r) -> int:
    if not _int(r) or not 0 <= r <= 8192:
        raise ValueError(f"radius {r!r}: 0 .. 8192")
    return int(r)


def erode_disc(r: int) -> Tuple[Rule, Mask]:
    """a 0 / 255 mask of Y eroded by the disc of radius r: a sample stays 255 when every sample of the plane within r of it is 255
    (nothing outside the plane exists) -> the rule of the distance call and the mask of the call behind it"""
    r = _radius(r)
    return Rule(0, 255, 255, 0, 0), mask_range(r * r + 1, NONE)


def dilate_disc(r: int) -> Tuple[Rule, Mask]:
    """... dilated: a sample becomes 255 when a 255 lies within r of it: the distance of the complement, inverted"""
    r = _radius(r)
    return Rule(0, 0, 254, 0, 0), mask_range(r * r + 1, NONE, invert=True)


def opening_disc(r: int) -> List[Tuple[Rule, Mask]]:
    return [erode_disc(r), dilate_disc(r)]


def closing_disc(r: int) -> List[Tuple[Rule, Mask]]:
    return [dilate_disc(r), erode_disc(r)]


def as_steps(steps) -> List[Tuple[Rule, Mask]]:
    """one (Rule, Mask) pair or a list of them -> a checked list; the rules are of plane 0"""
    if isinstance(steps, tuple) and len(steps) == 2 and isinstance(steps[0], Rule):
        steps = [steps]
    steps = list(steps or ())
    if not steps:
        raise ValueError("no steps")
    for s in steps:
        if not isinstance(s, tuple) or len(s) != 2:
            raise ValueError("a step is a (distance.Rule, distance.Mask) pair")
        check(s[0])
        check_mask(s[1])
        if s[0].plane != 0:
            raise ValueError("a step's rule is of plane 0: the mask call reads a map of Y")
    return steps


def of_steps(yuv, geom, steps) -> np.ndarray:
    """the bytes Context.disc_morph leaves for one picture: every step is of_picture and of_mask of the result before it"""
    cur = np.asarray(np.frombuffer(yuv, dtype=np.uint8) if isinstance(yuv, (bytes, bytearray, memoryview)) else yuv, dtype=np.uint8).reshape(-1)
    for r, m in as_steps(steps):
        cur = of_mask(of_picture(cur, geom, r), m, geom)
    return cur


# ------------------------------------------------------------------------------------------------------------ reading a map
def max_inscribed(dist) -> Tuple[int, int, int]:
    """(d, x, y) of the first maximum of a map [Ny][Nx] in raster order: under euclid2 the largest disc inside the foreground has its
    centre there and the radius sqrt(d) (exclusive: the nearest background sample lies at exactly that distance)"""
    d = np.asarray(dist)
    if d.ndim != 2 or not d.size:
        raise ValueError("a map is an array [Ny][Nx]")
    d = d.astype(np.int64) & NONE
    i = int(np.argmax(d))
    return int(d.reshape(-1)[i]), i % d.shape[1], i // d.shape[1]


def signed(inside, outside) -> np.ndarray:
    """a signed field from the maps of a rule and of its complement -> int64: the distance to the background on the foreground, minus the
    distance to the foreground on the background (each is 0 where the other is not); NONE stays 2^32 - 1 in size"""
    a = np.asarray(inside).astype(np.int64) & NONE
    b = np.asarray(outside).astype(np.int64) & NONE
    if a.shape != b.shape:
        raise ValueError("the two maps differ in shape")
    if np.any((a != 0) & (b != 0)):
        raise ValueError("the maps are not of complementary windows: a sample is foreground in both")
    return a - b
