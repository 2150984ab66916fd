"""Summed-area tables of pictures in slot layout (hvq_integral_pictures / Context.integral_pictures, hvq_window_pictures /
Context.window_pictures, hvq_rect_sums / Context.rect_sums, Context.adaptive_pictures): the rules, the values to expect, and the helpers
around a table.  numpy only.

A table is INCLUSIVE: S[y][x] is the sum of the plane over x' <= x, y' <= y, uint32 and so modulo 2^32; Q the same of the squares,
uint64.  include/hvqm4_amd.h specifies them and the three modes of a window rule: the mean rounded half up, the floor of the population
deviation, and a threshold relative to both.  The values here come from an algorithm of their own -- numpy.cumsum in uint64, masked to
32 bits for S; the boxes by slicing a padded exact table, the mean and the deviation by integer division and numpy's float root with a
step of correction either way --, which shares nothing with the kernels' prefix steps and binary digits.  A geometry is (width, height,
h_samp, v_samp).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .labels import plane_of, plane_shape

MEAN, DEVIATION, THRESHOLD = 0, 1, 2   # HVQ_WIN_MEAN, _DEVIATION, _THRESHOLD
MODES = ("mean", "deviation", "threshold")
MAX_RULES = 64                         # HVQ_WIN_MAX_RULES
MAX_RADIUS = 8191                      # HVQ_WIN_MAX_RADIUS
MAX_AREA = 1 << 24                     # the samples of a window, of a rectangle: 255 * 2^24 < 2^32
MAX_RECTS = 1 << 24                    # HVQ_RECT_MAX
_M32 = np.uint64(0xFFFFFFFF)


def _int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


@dataclass(frozen=True)
class Rule:
    """an entry of hvq_window_pictures: the plane the tables are of, the mode, the radii of the window, and THRESHOLD's k, c and invert.
    Hashable."""
    plane: int = 0
    mode: int = MEAN
    rx: int = 0
    ry: int = 0
    k: int = 0
    c: int = 0
    invert: int = 0

    def struct(self):
        """the HvqWindowRule of include/hvqm4_amd.h (ctypes)"""
        from ._lib import HvqWindowRule
        check(self)
        return HvqWindowRule(self.plane, self.mode, self.rx, self.ry, self.k, self.c, self.invert, 0)


def check(r: Rule) -> None:
    """ValueError for what hvq_window_check refuses"""
    if not isinstance(r, Rule):
        raise ValueError(f"an integral.Rule, not {type(r).__name__}")
    if not _int(r.plane) or not 0 <= r.plane <= 2:
        raise ValueError(f"plane {r.plane!r}: 0 Y, 1 U, 2 V")
    if not _int(r.mode) or not 0 <= r.mode <= 2:
        raise ValueError(f"mode {r.mode!r}: 0 MEAN, 1 DEVIATION, 2 THRESHOLD")
    if not _int(r.rx) or not _int(r.ry) or not 0 <= r.rx <= MAX_RADIUS or not 0 <= r.ry <= MAX_RADIUS:
        raise ValueError(f"radii {r.rx!r}, {r.ry!r}: 0 .. {MAX_RADIUS}")
    if not _int(r.k) or not -1024 <= r.k <= 1024:
        raise ValueError(f"k {r.k!r}: -1024 .. 1024")
    if not _int(r.c) or not -255 <= r.c <= 255:
        raise ValueError(f"c {r.c!r}: -255 .. 255")
    if not _int(r.invert) or r.invert not in (0, 1):
        raise ValueError(f"invert {r.invert!r}: 0 or 1")


def _radii(r):
    rx, ry = (r, r) if _int(r) else tuple(r)
    return rx, ry


def rule(mode, r, k: int = 0, c: int = 0, invert: bool = False, plane: int = 0) -> Rule:
    """`mode` (a name of MODES, or its index) over the window of radius r, or radii (rx, ry)"""
    if isinstance(mode, str):
        if mode not in MODES:
            raise ValueError(f"mode {mode!r}: one of {MODES}")
        mode = MODES.index(mode)
    rx, ry = _radii(r)
    out = Rule(plane, mode, rx, ry, k, c, int(bool(invert)))
    check(out)
    return out


def mean(r, plane: int = 0) -> Rule:
    """the local mean, rounded half up, over the window of radius r (or radii (rx, ry)) cut to the plane"""
    return rule(MEAN, r, plane=plane)


def deviation(r, plane: int = 0) -> Rule:
    """the floor of the local population standard deviation, 0 .. 127"""
    return rule(DEVIATION, r, plane=plane)


def adaptive(r, c: int = 0, k: int = 0, invert: bool = False, plane: int = 0) -> Rule:
    """255 where a > mean + (k / 256) deviation - c, else 0: k = 0 the "mean - C" rule, k != 0 Niblack's on the integer deviation"""
    return rule(THRESHOLD, r, k=k, c=c, invert=invert, plane=plane)


def needs_squares(r: Rule) -> bool:
    """does the rule read Q?"""
    return r.mode == DEVIATION or (r.mode == THRESHOLD and r.k != 0)


def nbytes(geom, plane: int = 0, order: int = 1) -> int:
    """hvq_integral_bytes: the bytes of the table of sums (order 1) or of squares (order 2) of that plane"""
    if order not in (1, 2):
        raise ValueError(f"order {order!r}: 1 sums, 2 squares")
    ny, nx = plane_shape(geom, plane)
    return 4 * order * nx * ny


# ------------------------------------------------------------------------------------------------------------ the tables
def _plane(a) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError("a plane is a uint8 array [Ny][Nx]")
    return a


def _exact(a, power: int) -> np.ndarray:
    """the inclusive table of a^power in uint64, nothing wrapped"""
    v = a.astype(np.uint64)
    return np.cumsum(np.cumsum(v * v if power == 2 else v, axis=0, dtype=np.uint64), axis=1, dtype=np.uint64)


def of_plane(a, squares: bool = True) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """the tables of a plane uint8 [Ny][Nx] -> (S uint32 [Ny][Nx], Q uint64 [Ny][Nx] or None)"""
    a = _plane(a)
    return (_exact(a, 1) & _M32).astype(np.uint32), (_exact(a, 2) if squares else None)


def padded(table) -> np.ndarray:
    """the (Ny + 1) x (Nx + 1) table of other libraries, a row and a column of zeros before the inclusive one: P[y][x] is the sum over
    x' < x, y' < y"""
    t = np.asarray(table)
    if t.ndim != 2:
        raise ValueError("a table is an array [Ny][Nx]")
    return np.pad(t, ((1, 0), (1, 0)))


def rect(sums, squares, x0: int, y0: int, x1: int, y1: int) -> Tuple[int, int, int]:
    """what hvq_rect_sums gives for the rectangle x0 .. x1, y0 .. y1 (inclusive) of the tables S (uint32, wrapped) and Q (uint64, or
    None) -> (count, S, Q); (0, 0, 0) for one that leaves the plane, is empty or holds more than 2^24 samples"""
    S = np.asarray(sums)
    ny, nx = S.shape
    if not (0 <= x0 <= x1 < nx and 0 <= y0 <= y1 < ny) or (x1 - x0 + 1) * (y1 - y0 + 1) > MAX_AREA:
        return 0, 0, 0
    P = padded(S.view(np.uint32) if S.dtype == np.int32 else S)
    s = (int(P[y1 + 1, x1 + 1]) - int(P[y0, x1 + 1]) - int(P[y1 + 1, x0]) + int(P[y0, x0])) % (1 << 32)
    q = 0
    if squares is not None:
        Pq = padded(np.asarray(squares))
        q = (int(Pq[y1 + 1, x1 + 1]) - int(Pq[y0, x1 + 1]) - int(Pq[y1 + 1, x0]) + int(Pq[y0, x0])) % (1 << 64)
    return (x1 - x0 + 1) * (y1 - y0 + 1), s, q


def of_rects(rects, tables, dims=None) -> np.ndarray:
    """what hvq_rect_sums writes: `rects` int [nrects][5] = (i, x0, y0, x1, y1), `tables` a list of (S, Q or None) a picture -> uint64
    [nrects][3]"""
    out = np.zeros((len(rects), 3), dtype=np.uint64)
    for r, (i, x0, y0, x1, y1) in enumerate(np.asarray(rects).tolist()):
        if 0 <= i < len(tables):
            out[r] = rect(tables[i][0], tables[i][1], x0, y0, x1, y1)
    return out


# ------------------------------------------------------------------------------------------------------------ the windows
def _boxes(a, rx: int, ry: int, power: int) -> np.ndarray:
    """int64-safe uint64 [Ny][Nx]: the sum of a^power over the window of every sample, cut to the plane"""
    ny, nx = a.shape
    P = padded(_exact(a, power))
    x0 = np.maximum(np.arange(nx) - rx, 0)
    x1 = np.minimum(np.arange(nx) + rx, nx - 1) + 1
    y0 = np.maximum(np.arange(ny) - ry, 0)[:, None]
    y1 = (np.minimum(np.arange(ny) + ry, ny - 1) + 1)[:, None]
    return P[y1, x1] - P[y0, x1] - P[y1, x0] + P[y0, x0]


def _counts(ny: int, nx: int, rx: int, ry: int) -> np.ndarray:
    w = np.minimum(np.arange(nx) + rx, nx - 1) - np.maximum(np.arange(nx) - rx, 0) + 1
    h = np.minimum(np.arange(ny) + ry, ny - 1) - np.maximum(np.arange(ny) - ry, 0) + 1
    return (h[:, None] * w[None, :]).astype(np.int64)


def _isqrt(v: np.ndarray) -> np.ndarray:
    """the exact floor square root of int64 values below 2^62: numpy's float root, then a step of correction either way"""
    s = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    s = np.where(s * s > v, s - 1, s)
    return np.where((s + 1) * (s + 1) <= v, s + 1, s)


def _deviation(S, Q, n) -> np.ndarray:
    # the largest d with (d n)^2 <= n Q - S^2 is floor(isqrt(n Q - S^2) / n); n Q may pass 2^63, so in uint64
    var = (n.astype(np.uint64) * Q.astype(np.uint64) - S.astype(np.uint64) * S.astype(np.uint64)).astype(np.int64)
    return _isqrt(var) // n


def of_window(a, r: Rule) -> np.ndarray:
    """what hvq_window_pictures writes into Y for a plane uint8 [Ny][Nx] -> uint8 [Ny][Nx]"""
    check(r)
    a = _plane(a)
    ny, nx = a.shape
    if min(2 * r.rx + 1, nx) * min(2 * r.ry + 1, ny) > MAX_AREA:
        raise ValueError(f"a window of {min(2 * r.rx + 1, nx)} x {min(2 * r.ry + 1, ny)} samples: a window holds 2^24")
    n = _counts(ny, nx, r.rx, r.ry)
    S = _boxes(a, r.rx, r.ry, 1).astype(np.int64)
    if r.mode == MEAN:
        return ((2 * S + n) // (2 * n)).astype(np.uint8)
    d = _deviation(S, _boxes(a, r.rx, r.ry, 2), n) if needs_squares(r) else np.zeros_like(n)
    if r.mode == DEVIATION:
        return d.astype(np.uint8)
    on = 256 * n * a.astype(np.int64) > 256 * S + r.k * d * n - 256 * r.c * n
    return np.where(on ^ bool(r.invert), 255, 0).astype(np.uint8)


def of_picture(yuv, geom, r: Rule) -> np.ndarray:
    """the bytes hvq_window_pictures writes for one picture Y | U | V of geometry `geom`: the result in Y, 128 in U and V.  The rule's
    plane must have the size of Y"""
    check(r)
    if plane_shape(geom, r.plane) != plane_shape(geom, 0):
        raise ValueError(f"plane {r.plane} of {geom} has not the size of Y: the result is written into Y")
    y = of_window(plane_of(np.asarray(yuv, dtype=np.uint8).reshape(-1), geom, r.plane), r)
    cy, cx = plane_shape(geom, 1)
    return np.concatenate([y.reshape(-1), np.full(2 * cx * cy, 128, dtype=np.uint8)])


# ------------------------------------------------------------------------------------------------------------ rectangles from boxes
def rects_of_boxes(comps):
    """the boxes of label_pictures' record tables as hvq_rect_sums' rectangles: `comps` a list of n tables [cap + 1][8] (torch tensors on
    the GPU: an expression on the device, no synchronisation; or numpy arrays) -> int32 [n * cap][5] = (i, x0, y0, x1, y1), row i * cap
    + k - 1 the box of record k of picture i; a row beyond the records stored is the empty rectangle (i, 0, 0, -1, -1), which gives
    (0, 0, 0)"""
    n = len(comps)
    if not n:
        raise ValueError("no record tables")
    if isinstance(comps[0], np.ndarray):
        t = np.stack([np.asarray(c) for c in comps]).astype(np.int64)
        cap = t.shape[1] - 1
        live = np.arange(1, cap + 1)[None, :] <= t[:, 0, 1][:, None]
        box = np.where(live[:, :, None], t[:, 1:, 1:5], np.array([0, 0, -1, -1]))
        idx = np.broadcast_to(np.arange(n)[:, None, None], (n, cap, 1))
        return np.concatenate([idx, box], axis=2).reshape(n * cap, 5).astype(np.int32)
    import torch
    t = torch.stack(list(comps))
    cap = t.shape[1] - 1
    live = torch.arange(1, cap + 1, device=t.device)[None, :] <= t[:, 0, 1][:, None]
    box = torch.where(live[:, :, None], t[:, 1:, 1:5], torch.tensor([0, 0, -1, -1], dtype=t.dtype, device=t.device))
    idx = torch.arange(n, device=t.device, dtype=t.dtype)[:, None, None].expand(n, cap, 1)
    return torch.cat([idx, box], dim=2).reshape(n * cap, 5).to(torch.int32).contiguous()
