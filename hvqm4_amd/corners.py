"""Corners of pictures in slot layout (hvq_corner_pictures / Context.corner_pictures): the rules, the values to expect, and the helpers
around the list.  numpy only.

A rule names a plane (0 Y, 1 U, 2 V), a measure (Harris' with k in 1/256ths, or the smaller eigenvalue of the structure tensor), the
radius r of the (2r + 1)^2 structure window, the suppression distance nms, a margin and a threshold.  include/hvqm4_amd.h specifies the
result in exact integers: the mask picture (255 at corners of the analysed plane, the other planes 0 / 128), the row index uint32
[Ny + 1], the list int64 [cap + 1][4] -- row 0 {K, stored, status, 0}, row j {x, y, R, y Nx + x} in raster order -- and the response map
int64 [Ny][Nx].  response_of_plane and of_plane compute them on the host with an algorithm of their own -- shifted int64 slices of an
edge-padded plane, window sums by two cumulative sums, suppression by comparing shifted arrays of (R, -index) --, which shares nothing
with the kernels' tiles.  A geometry is (width, height, h_samp, v_samp).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .labels import plane_of, plane_shape

MAX_RULES = 64                         # HVQ_CRN_MAX_RULES
MAX_CAP = 1 << 20                      # HVQ_CRN_MAX_CAP
MAX_RADIUS = 3                         # HVQ_CRN_MAX_RADIUS
MAX_NMS = 7                            # HVQ_CRN_MAX_NMS
HARRIS = 0                             # HVQ_CRN_HARRIS
MIN_EIGEN = 1                          # HVQ_CRN_MIN_EIGEN
FIELDS = ("x", "y", "R", "index")
_NONE = np.iinfo(np.int64).min         # a position outside the plane: it beats nothing


def _int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


@dataclass(frozen=True)
class Rule:
    """one plane, the measure and what makes a sample a corner.  Hashable."""
    plane: int = 0
    mode: int = HARRIS
    radius: int = 1
    k: int = 10
    nms: int = 3
    margin: int = 0
    threshold: int = 1

    def struct(self):
        """the HvqCornerRule of include/hvqm4_amd.h (ctypes)"""
        from ._lib import HvqCornerRule
        check(self)
        return HvqCornerRule(self.plane, self.mode, self.radius, self.k, self.nms, self.margin, (0, 0), self.threshold)


def harris(radius: int = 1, k: int = 10, threshold: int = 1, nms: int = 3, margin: int = 0, plane: int = 0) -> Rule:
    """Harris' measure R = 256 (A C - B^2) - k T^2; k = 10 is the usual 0.04"""
    r = Rule(plane, HARRIS, radius, k, nms, margin, threshold)
    check(r)
    return r


def min_eigen(radius: int = 1, threshold: int = 1, nms: int = 3, margin: int = 0, plane: int = 0) -> Rule:
    """Shi and Tomasi's measure R = T - isqrt((A - C)^2 + 4 B^2): twice the smaller eigenvalue, rounded up"""
    r = Rule(plane, MIN_EIGEN, radius, 0, nms, margin, threshold)
    check(r)
    return r


def check(r: Rule) -> None:
    """ValueError for what hvq_corner_check refuses"""
    if not isinstance(r, Rule):
        raise ValueError(f"a corners.Rule, not {type(r).__name__}")
    if not _int(r.plane) or not 0 <= r.plane <= 2:
        raise ValueError(f"plane {r.plane!r}: 0 Y, 1 U, 2 V")
    if not _int(r.mode) or r.mode not in (HARRIS, MIN_EIGEN):
        raise ValueError(f"mode {r.mode!r}: 0 Harris, 1 min-eigenvalue")
    if not _int(r.radius) or not 1 <= r.radius <= MAX_RADIUS:
        raise ValueError(f"radius {r.radius!r} outside 1 .. {MAX_RADIUS}")
    if not _int(r.k) or not 0 <= r.k <= 64 or (r.mode == MIN_EIGEN and r.k):
        raise ValueError(f"k {r.k!r}: 0 .. 64 under Harris, 0 under min-eigenvalue")
    if not _int(r.nms) or not 0 <= r.nms <= MAX_NMS:
        raise ValueError(f"nms {r.nms!r} outside 0 .. {MAX_NMS}")
    if not _int(r.margin) or not 0 <= r.margin <= 255:
        raise ValueError(f"margin {r.margin!r} outside 0 .. 255")
    if not _int(r.threshold) or not 1 <= r.threshold < 1 << 63:
        raise ValueError(f"threshold {r.threshold!r}: at least 1, an int64")


def nbytes(geom, plane: int = 0, cap: int = 1024) -> Tuple[int, int, int, int]:
    """the bytes of the four outputs of one picture: (mask, points, rows, response) -- hvq_stream_pic_bytes, 32 (cap + 1),
    hvq_corner_rows_bytes, hvq_corner_response_bytes"""
    w, h, _hs, _vs = geom
    cy, cx = plane_shape(geom, 1)
    ny, nx = plane_shape(geom, plane)
    return w * h + 2 * cx * cy, 32 * (cap + 1), 4 * (ny + 1), 8 * nx * ny


# ------------------------------------------------------------------------------------------------------------ the values
def _isqrt(v: np.ndarray) -> np.ndarray:
    """the floor square roots of non-negative int64 values below 2^62"""
    s = np.sqrt(v.astype(np.float64)).astype(np.int64)
    for _ in range(2):
        s -= s * s > v
        s += (s + 1) * (s + 1) <= v
    return s


def response_of_plane(a, r: Optional[Rule] = None) -> np.ndarray:
    """every R of a plane uint8 [Ny][Nx] -> int64 [Ny][Nx]"""
    r = Rule() if r is None else r
    check(r)
    a = np.asarray(a)
    if a.ndim != 2 or a.dtype != np.uint8 or not a.size:
        raise ValueError("a plane is a uint8 array [Ny][Nx]")
    ny, nx = a.shape
    w = r.radius
    p = np.pad(a.astype(np.int64), w + 1, mode="edge")                # a* at the positions -w - 1 .. N + w
    gx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])      # at -w .. N + w - 1
    gy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])

    def window(v):
        c = np.zeros((v.shape[0] + 1, v.shape[1] + 1), dtype=np.int64)
        c[1:, 1:] = np.cumsum(np.cumsum(v, axis=0), axis=1)
        n = 2 * w + 1
        return c[n:, n:] - c[:-n, n:] - c[n:, :-n] + c[:-n, :-n]
    A, B, C = window(gx * gx), window(gx * gy), window(gy * gy)
    assert A.shape == (ny, nx)
    T = A + C
    if r.mode == HARRIS:
        return 256 * (A * C - B * B) - r.k * T * T
    return T - _isqrt((A - C) * (A - C) + 4 * B * B)


def of_plane(a, r: Optional[Rule] = None, cap: Optional[int] = None, response: Optional[np.ndarray] = None):
    """the corners of a plane uint8 [Ny][Nx] -> (mask uint8 [Ny][Nx], points int64 [stored + 1][4], rows uint32 [Ny + 1]); cap None:
    every corner.  `response`: response_of_plane's result, when the caller has it"""
    r = Rule() if r is None else r
    R = response_of_plane(a, r) if response is None else np.asarray(response, dtype=np.int64)
    ny, nx = R.shape
    m, g = r.nms, r.margin
    keep = R >= r.threshold
    inside = np.zeros((ny, nx), dtype=bool)
    if ny > 2 * g and nx > 2 * g:
        inside[g:ny - g, g:nx - g] = True
    keep &= inside
    if m and keep.any():
        P = np.full((ny + 2 * m, nx + 2 * m), _NONE, dtype=np.int64)
        P[m:m + ny, m:m + nx] = R
        for dy in range(-m, m + 1):
            for dx in range(-m, m + 1):
                if not dy and not dx:
                    continue
                Q = P[m + dy:m + dy + ny, m + dx:m + dx + nx]
                first = dy < 0 or (dy == 0 and dx < 0)                # (R, -index) of q above that of p
                keep &= ~((Q >= R) if first else (Q > R))
    mask = np.where(keep, 255, 0).astype(np.uint8)
    ys, xs = np.nonzero(keep)                                         # raster order
    K = int(ys.size)
    stored = K if cap is None else min(K, int(cap))
    points = np.zeros((stored + 1, 4), dtype=np.int64)
    points[0] = (K, stored, 0, 0)
    points[1:, 0] = xs[:stored]
    points[1:, 1] = ys[:stored]
    points[1:, 2] = R[ys[:stored], xs[:stored]]
    points[1:, 3] = ys[:stored].astype(np.int64) * nx + xs[:stored]
    rows = np.zeros(ny + 1, dtype=np.uint32)
    rows[1:] = np.cumsum(keep.sum(axis=1))
    return mask, points, rows


def of_picture(yuv, geom, r: Optional[Rule] = None, cap: Optional[int] = None):
    """of_plane on the rule's plane of a picture Y | U | V of geometry `geom` -> (the mask PICTURE uint8 [the picture's bytes], points,
    rows): the analysed plane 255 / 0, of the others Y 0, U and V 128"""
    r = Rule() if r is None else r
    check(r)
    mask, points, rows = of_plane(plane_of(yuv, geom, r.plane), r, cap)
    parts = []
    for p in range(3):
        ny, nx = plane_shape(geom, p)
        parts.append(mask.reshape(-1) if p == r.plane else np.full(nx * ny, 128 if p else 0, dtype=np.uint8))
    return np.concatenate(parts), points, rows


# ------------------------------------------------------------------------------------------------------------ the list
def records(points) -> np.ndarray:
    """the stored rows of one picture's list [cap + 1][4] (a numpy array, or a tensor on the host) -> int64 [stored][4]: x, y, R, index"""
    c = np.asarray(points).astype(np.int64, copy=False)
    if c.ndim != 2 or c.shape[1] != 4 or c.shape[0] < 1:
        raise ValueError("a list of corners is an array [cap + 1][4]")
    K, stored = int(c[0, 0]), int(c[0, 1])
    if not 0 <= stored <= min(K, c.shape[0] - 1):
        raise ValueError(f"row 0 says {stored} of {K} corners are stored, the list has room for {c.shape[0] - 1}")
    return c[1:stored + 1]


def strongest(points, k: int) -> np.ndarray:
    """the k stored corners of the largest R, the largest first, the smaller index first among equals -> int64 [<= k][4]"""
    rec = records(points)
    return rec[np.lexsort((rec[:, 3], -rec[:, 2]))[:max(int(k), 0)]]


def grid(points, cell: int) -> np.ndarray:
    """the strongest stored corner of every cell x cell square of the plane (the smaller index among equals), in raster order: an
    even spread for a fit -> int64 [cells with a corner][4]"""
    if not _int(cell) or cell < 1:
        raise ValueError(f"cell {cell!r}: at least 1")
    rec = records(points)
    if not rec.shape[0]:
        return rec
    cx, cy = rec[:, 0] // cell, rec[:, 1] // cell
    order = np.lexsort((rec[:, 3], -rec[:, 2], cx, cy))
    key = np.stack([cy[order], cx[order]], axis=1)
    first = np.ones(order.size, dtype=bool)
    first[1:] = (key[1:] != key[:-1]).any(axis=1)
    chosen = rec[order[first]]
    return chosen[np.argsort(chosen[:, 3], kind="stable")]
