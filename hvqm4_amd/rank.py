"""Rank filters on pictures in slot layout (hvq_rank_pictures / Context.rank_pictures, Context.morph_pictures): the operations, the
values to expect, and the helpers around them.  numpy only.

A picture is its bytes Y | U | V tightly packed.  Each plane goes through its PlaneRank, which include/hvqm4_amd.h specifies:
    W(y, x) = the (2 ry + 1)(2 rx + 1) samples a[cy(y + j - ry)][cx(x + i - rx)]                 (the border replicates the edge sample)
    MIN = min W;  MAX = max W;  RANGE = max W - min W;  MEDIAN = sorted(W)[(|W| - 1) / 2]
MIN, MAX and RANGE take radii 0 .. 15 per axis, MEDIAN 1 x 1, 3 x 3 or 5 x 5.  A geometry is (width, height, h_samp, v_samp).  A Rank
holds the plane operation of Y and that of U and V; the builders give both planes the same one, luma_only and chroma_for change the
chroma's.  Opening and closing are lists of steps: Context.morph_pictures runs them, of_steps gives their bytes.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence, Tuple, Union

import numpy as np

MIN, MAX, RANGE, MEDIAN = 0, 1, 2, 3   # HVQ_RNK_MIN, HVQ_RNK_MAX, HVQ_RNK_RANGE, HVQ_RNK_MEDIAN
MAX_RADIUS = 15                        # HVQ_RNK_MAX_RADIUS
MAX_RANKS = 64                         # HVQ_RNK_MAX_RANKS
_NAMES = {MIN: "MIN", MAX: "MAX", RANGE: "RANGE", MEDIAN: "MEDIAN"}


@dataclass(frozen=True)
class PlaneRank:
    op: int = MIN
    rx: int = 0
    ry: int = 0
    pad: int = 0

    def struct(self):
        """the HvqRankPlane of include/hvqm4_amd.h (ctypes)"""
        from ._lib import HvqRankPlane
        check_plane(self)
        return HvqRankPlane(self.op, self.rx, self.ry, self.pad)


@dataclass(frozen=True)
class Rank:
    """luma for Y, chroma for U and V (at their own resolution).  Hashable; equal when the plane operations are."""
    luma: PlaneRank
    chroma: PlaneRank

    def struct(self):
        """the HvqRank of include/hvqm4_amd.h (ctypes)"""
        from ._lib import HvqRank
        check(self)
        return HvqRank(self.luma.struct(), self.chroma.struct())


IDENTITY_PLANE = PlaneRank(MIN, 0, 0)


def _int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_plane(p: PlaneRank) -> None:
    """ValueError for what hvq_rank_check refuses in a plane"""
    if not isinstance(p, PlaneRank):
        raise ValueError(f"a plane rank, not {type(p).__name__}")
    if not _int(p.op) or p.op not in _NAMES:
        raise ValueError(f"op {p.op!r}: MIN, MAX, RANGE or MEDIAN")
    if not _int(p.rx) or not _int(p.ry) or not 0 <= p.rx <= MAX_RADIUS or not 0 <= p.ry <= MAX_RADIUS:
        raise ValueError(f"radius ({p.rx!r}, {p.ry!r}) outside 0 .. {MAX_RADIUS}")
    if p.op == MEDIAN and (p.rx != p.ry or p.rx > 2):
        raise ValueError(f"a median of radius ({p.rx}, {p.ry}): 1 x 1, 3 x 3 or 5 x 5")
    if p.pad != 0:
        raise ValueError(f"pad {p.pad!r}: 0")


def check(r: Rank) -> None:
    """ValueError for what hvq_rank_check refuses"""
    if not isinstance(r, Rank):
        raise ValueError(f"a rank.Rank, not {type(r).__name__}")
    check_plane(r.luma)
    check_plane(r.chroma)


def copies(p: PlaneRank) -> bool:
    """the plane operation leaves every sample as it is (the kernel's copy body takes it)"""
    return p.op != RANGE and p.rx == 0 and p.ry == 0


# ------------------------------------------------------------------------------------------------------------ the builders
def _radii(r) -> Tuple[int, int]:
    if _int(r):
        rx = ry = int(r)
    elif isinstance(r, (tuple, list)) and len(r) == 2 and all(_int(v) for v in r):
        rx, ry = int(r[0]), int(r[1])
    else:
        raise ValueError(f"radius {r!r}: an integer or (rx, ry)")
    if not 0 <= rx <= MAX_RADIUS or not 0 <= ry <= MAX_RADIUS:
        raise ValueError(f"radius ({rx}, {ry}) outside 0 .. {MAX_RADIUS}")
    return rx, ry


def _both(op: int, r) -> Rank:
    p = PlaneRank(op, *_radii(r))
    return Rank(p, p)


def erode(r=1) -> Rank:
    """the minimum of the (2 rx + 1) x (2 ry + 1) window; r: an integer or (rx, ry)"""
    return _both(MIN, r)


def dilate(r=1) -> Rank:
    """the maximum of the window"""
    return _both(MAX, r)


def gradient(r=1) -> Rank:
    """the morphological gradient: the maximum minus the minimum of the window (RANGE)"""
    return _both(RANGE, r)


def median(n: int = 3) -> Rank:
    """the n x n median, n = 3 or 5"""
    if n not in (3, 5):
        raise ValueError(f"median({n!r}): 3 or 5")
    return _both(MEDIAN, n // 2)


def identity() -> Rank:
    return Rank(IDENTITY_PLANE, IDENTITY_PLANE)


def luma_only(r: Rank) -> Rank:
    """r on Y, U and V copied"""
    check(r)
    return Rank(r.luma, IDENTITY_PLANE)


def chroma_for(r: Rank, h_samp: int, v_samp: int) -> Rank:
    """r with the chroma planes' radius adapted to their resolution: the luma radius divided by the sampling of each axis (rounded down),
    never below 1 where the luma radius is at least 1, so that the window covers about the same part of the picture in every plane.  A
    median stays square: the smaller of its two divided radii."""
    if (h_samp, v_samp) not in ((2, 2), (2, 1), (1, 1)):
        raise ValueError(f"sampling {(h_samp, v_samp)}: (2, 2), (2, 1) or (1, 1)")
    check(r)
    p = r.luma
    rx = max(1, p.rx // h_samp) if p.rx else 0
    ry = max(1, p.ry // v_samp) if p.ry else 0
    if p.op == MEDIAN:
        rx = ry = min(rx, ry)
    return Rank(p, PlaneRank(p.op, rx, ry))


def opening(r=1) -> List[Rank]:
    """erosion, then dilation: removes bright detail smaller than the window"""
    return [erode(r), dilate(r)]


def closing(r=1) -> List[Rank]:
    """dilation, then erosion: removes dark detail smaller than the window"""
    return [dilate(r), erode(r)]


# ------------------------------------------------------------------------------------------------------- the values to expect
def _windows(e: np.ndarray, n: int, size: int, axis: int):
    return [e[i:i + size, :] if axis == 0 else e[:, i:i + size] for i in range(n)]


def _extreme(a: np.ndarray, rx: int, ry: int, fn) -> np.ndarray:
    h = fn.reduce(_windows(np.pad(a, ((0, 0), (rx, rx)), mode="edge"), 2 * rx + 1, a.shape[1], 1))
    return fn.reduce(_windows(np.pad(h, ((ry, ry), (0, 0)), mode="edge"), 2 * ry + 1, a.shape[0], 0))


def of_plane(plane, p: PlaneRank) -> np.ndarray:
    """a plane (2-D uint8) through a plane operation -> uint8 of the same shape"""
    check_plane(p)
    a = np.asarray(plane)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError("a plane is a 2-D uint8 array")
    if p.op == MIN:
        return _extreme(a, p.rx, p.ry, np.minimum)
    if p.op == MAX:
        return _extreme(a, p.rx, p.ry, np.maximum)
    if p.op == RANGE:
        return _extreme(a, p.rx, p.ry, np.maximum) - _extreme(a, p.rx, p.ry, np.minimum)
    r = p.rx
    e = np.pad(a, ((r, r), (r, r)), mode="edge")
    ny, nx = a.shape
    w = np.stack([e[j:j + ny, i:i + nx] for j in range(2 * r + 1) for i in range(2 * r + 1)])
    return np.sort(w, axis=0)[(w.shape[0] - 1) // 2]


def of_picture(buf, geom, rank: Rank) -> np.ndarray:
    """the expected bytes of hvq_rank_pictures: the picture `buf` (Y | U | V of geometry geom = (w, h, h_samp, v_samp)) through `rank`
    -> uint8 [the picture's bytes]"""
    from .scale import planes
    check(rank)
    w, h, hs, vs = geom
    return np.concatenate([of_plane(a, rank.chroma if i else rank.luma).reshape(-1) for i, a in enumerate(planes(buf, w, h, hs, vs))])


def of_steps(buf, geom, steps: Sequence[Rank]) -> np.ndarray:
    """the expected bytes of Context.morph_pictures: the picture through every step in turn"""
    out = np.asarray(buf, dtype=np.uint8).reshape(-1)
    for s in steps:
        out = of_picture(out, geom, s)
    return out


def as_steps(steps: Union[Rank, Sequence[Rank]]) -> List[Rank]:
    """a Rank or a list of them -> the checked list of steps (at least one)"""
    steps = [steps] if isinstance(steps, Rank) else list(steps) if isinstance(steps, (list, tuple)) else None
    if not steps:
        raise ValueError("steps: a rank.Rank or a non-empty list of them")
    for s in steps:
        if not isinstance(s, Rank):
            raise ValueError(f"steps: an entry is a rank.Rank, not {type(s).__name__}")
        check(s)
    return steps
