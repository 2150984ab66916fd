"""Bilateral filters on pictures in slot layout (hvq_bilateral_pictures / Context.bilateral_pictures, Context.smooth_pictures): the
parameter sets, the values to expect, and the helpers around them.  numpy only.

A picture is its bytes Y | U | V tightly packed.  Each plane goes through its PlaneBilateral, which include/hvqm4_amd.h specifies:
    w(j, i) = spatial[|j|][|i|] * range[ |g[q] - g[y][x]| ],  q = (cy(y + j), cx(x + i))         (the border replicates the edge sample)
    out     = (sum w a[q] + den / 2) / den,  den = sum w                                          (exact integers, one rounding, half up)
for j in [-ry, ry] and i in [-rx, rx], radii 0 .. 7 per axis; g is the guide picture's plane, or a itself.  A geometry is (width,
height, h_samp, v_samp).  A Bilateral holds the set of Y and that of U and V; the builders give both planes the same one, luma_only and
chroma_for change the chroma's.  Repeated smoothing is a list of steps: Context.smooth_pictures runs it, of_steps gives its bytes.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

MAX_RADIUS = 7                         # HVQ_BIL_MAX_RADIUS
MAX_SETS = 64                          # HVQ_BIL_MAX_SETS


@dataclass(frozen=True)
class PlaneBilateral:
    """rx, ry: the radii; spatial: 64 bytes, [|j|][|i|] row by row; range: 256 bytes, by the guide's absolute difference"""
    rx: int
    ry: int
    spatial: bytes
    range: bytes
    pad: Tuple[int, int] = (0, 0)

    def struct(self):
        """the HvqBilateralPlane of include/hvqm4_amd.h (ctypes)"""
        from ._lib import HvqBilateralPlane
        check_plane(self)
        return HvqBilateralPlane.from_buffer_copy(np.array([self.rx, self.ry, 0, 0], dtype="<i4").tobytes() + self.spatial + self.range)

    def taps(self) -> int:
        """the taps of the window whose spatial factor is not 0"""
        return sum(1 for j in range(-self.ry, self.ry + 1) for i in range(-self.rx, self.rx + 1) if self.spatial[8 * abs(j) + abs(i)])


@dataclass(frozen=True)
class Bilateral:
    """luma for Y, chroma for U and V (at their own resolution).  Hashable; equal when the planes' sets are."""
    luma: PlaneBilateral
    chroma: PlaneBilateral

    def struct(self):
        """the HvqBilateral of include/hvqm4_amd.h (ctypes)"""
        from ._lib import HvqBilateral
        check(self)
        return HvqBilateral(self.luma.struct(), self.chroma.struct())


def _int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_plane(p: PlaneBilateral) -> None:
    """ValueError for what hvq_bilateral_check refuses in a plane, and for tables of another size"""
    if not isinstance(p, PlaneBilateral):
        raise ValueError(f"a plane set, not {type(p).__name__}")
    if not _int(p.rx) or not _int(p.ry) or not 0 <= p.rx <= MAX_RADIUS or not 0 <= p.ry <= MAX_RADIUS:
        raise ValueError(f"radius ({p.rx!r}, {p.ry!r}) outside 0 .. {MAX_RADIUS}")
    if not isinstance(p.spatial, bytes) or len(p.spatial) != 64 or not isinstance(p.range, bytes) or len(p.range) != 256:
        raise ValueError("tables: spatial is 64 bytes ([|j|][|i|]), range 256 bytes")
    if p.spatial[0] < 1 or p.range[0] < 1:
        raise ValueError(f"spatial[0][0] {p.spatial[0]}, range[0] {p.range[0]}: the centre tap has a weight, both at least 1")
    if not isinstance(p.pad, tuple) or len(p.pad) != 2 or p.pad != (0, 0):
        raise ValueError(f"pad {p.pad!r}: (0, 0)")


def check(b: Bilateral) -> None:
    """ValueError for what hvq_bilateral_check refuses"""
    if not isinstance(b, Bilateral):
        raise ValueError(f"a bilateral.Bilateral, not {type(b).__name__}")
    check_plane(b.luma)
    check_plane(b.chroma)


def copies(p: PlaneBilateral) -> bool:
    """the plane's set leaves every sample as it is by its radii alone (the kernel's copy body takes it)"""
    return p.rx == 0 and p.ry == 0


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


def _byte(v) -> int:
    if not _int(v) or not 0 <= v <= 255:
        raise ValueError(f"a table entry {v!r}: an integer 0 .. 255")
    return int(v)


def plane_from_tables(rx: int, ry: int, spatial, range_) -> PlaneBilateral:
    """spatial: rows [|j|][|i|] of at least (ry + 1) x (rx + 1) entries (what lies outside is not read and becomes 0); range_: up to 256
    entries by the guide's absolute difference (missing ones are 0)"""
    rx, ry = _radii((rx, ry))
    rows = [list(r) for r in spatial]
    if len(rows) < ry + 1 or any(len(r) < rx + 1 for r in rows[:ry + 1]):
        raise ValueError(f"spatial: at least {ry + 1} rows of {rx + 1} entries")
    sp = bytearray(64)
    for j in range(ry + 1):
        for i in range(rx + 1):
            sp[8 * j + i] = _byte(rows[j][i])
    rg = [_byte(v) for v in range_]
    if not 1 <= len(rg) <= 256:
        raise ValueError("range: 1 .. 256 entries")
    p = PlaneBilateral(rx, ry, bytes(sp), bytes(rg + [0] * (256 - len(rg))))
    check_plane(p)
    return p


def from_tables(rx: int, ry: int, spatial, range_) -> Bilateral:
    """the set of the given tables on all three planes"""
    p = plane_from_tables(rx, ry, spatial, range_)
    return Bilateral(p, p)


def _gauss_table(sigma: float, n: int, scale=1.0) -> List[int]:
    """round(255 exp(-(scale k)^2 / (2 sigma^2))) for k = 0 .. n - 1"""
    return [int(math.floor(255.0 * math.exp(-(scale * k) ** 2 / (2.0 * sigma * sigma)) + 0.5)) for k in range(n)]


def _gauss_spatial(sigma: float, rx: int, ry: int) -> List[List[int]]:
    return [[int(math.floor(255.0 * math.exp(-(i * i + j * j) / (2.0 * sigma * sigma)) + 0.5)) for i in range(rx + 1)] for j in range(ry + 1)]


def default_radius(sigma_space: float) -> int:
    """the radius a spatial sigma asks for: ceil(2 sigma), 1 .. 7"""
    return max(1, min(MAX_RADIUS, int(math.ceil(2.0 * sigma_space))))


def bilateral(sigma_space: float, sigma_range: float, radius=None) -> Bilateral:
    """the bilateral filter of Gaussian weights: spatial[j][i] = round(255 exp(-(i^2 + j^2) / (2 sigma_space^2))), range[d] = round(255
    exp(-d^2 / (2 sigma_range^2))).  radius: an integer or (rx, ry); default_radius(sigma_space) when not given"""
    if not sigma_space > 0 or not sigma_range > 0:
        raise ValueError(f"sigmas {sigma_space}, {sigma_range}: above 0")
    rx, ry = _radii(default_radius(sigma_space) if radius is None else radius)
    return from_tables(rx, ry, _gauss_spatial(sigma_space, rx, ry), _gauss_table(sigma_range, 256))


def sigma_filter(radius, threshold: int) -> Bilateral:
    """the sigma filter ("surface blur"): the mean of the window's samples that differ from the centre by `threshold` at the most"""
    rx, ry = _radii(radius)
    if not _int(threshold) or not 0 <= threshold <= 255:
        raise ValueError(f"threshold {threshold!r}: 0 .. 255")
    return from_tables(rx, ry, [[1] * (rx + 1)] * (ry + 1), [1] * (threshold + 1))


def box(radius) -> Bilateral:
    """the box mean (no edge is kept): every weight 1"""
    rx, ry = _radii(radius)
    return from_tables(rx, ry, [[1] * (rx + 1)] * (ry + 1), [1] * 256)


def disc(radius: int, sigma_range: Optional[float] = None, threshold: Optional[int] = None) -> Bilateral:
    """a disc window, the taps with i^2 + j^2 <= radius^2 + radius (the other corners are switched off), weight 1 each; the range table
    flat, a Gaussian of sigma_range, or 1 up to `threshold`"""
    if not _int(radius):
        raise ValueError(f"radius {radius!r}: an integer")
    r, _ = _radii(radius)
    if sigma_range is not None and threshold is not None:
        raise ValueError("disc: sigma_range or threshold, not both")
    sp = [[1 if i * i + j * j <= r * r + r else 0 for i in range(r + 1)] for j in range(r + 1)]
    if sigma_range is not None:
        if not sigma_range > 0:
            raise ValueError(f"sigma_range {sigma_range}: above 0")
        rg = _gauss_table(sigma_range, 256)
    elif threshold is not None:
        if not _int(threshold) or not 0 <= threshold <= 255:
            raise ValueError(f"threshold {threshold!r}: 0 .. 255")
        rg = [1] * (threshold + 1)
    else:
        rg = [1] * 256
    return from_tables(r, r, sp, rg)


IDENTITY_PLANE = PlaneBilateral(0, 0, bytes([1] + [0] * 63), bytes([1] + [0] * 255))


def identity() -> Bilateral:
    return Bilateral(IDENTITY_PLANE, IDENTITY_PLANE)


def luma_only(b: Bilateral) -> Bilateral:
    """b on Y, U and V copied"""
    check(b)
    return Bilateral(b.luma, IDENTITY_PLANE)


def chroma_for(b: Bilateral, h_samp: int, v_samp: int) -> Bilateral:
    """b with the chroma planes' window adapted to their resolution: the luma radius divided by the sampling of each axis (rounded down),
    never below 1 where the luma radius is at least 1, and the chroma tap (j, i) takes the spatial factor of the luma tap (j v_samp, i
    h_samp) -- the one that lies there in the picture (the last of the luma table where that leaves it): a Gaussian's sigma is
    divided by the sampling.  The range table stays."""
    if (h_samp, v_samp) not in ((2, 2), (2, 1), (1, 1)):
        raise ValueError(f"sampling {(h_samp, v_samp)}: (2, 2), (2, 1) or (1, 1)")
    check(b)
    p = b.luma
    rx = max(1, p.rx // h_samp) if p.rx else 0
    ry = max(1, p.ry // v_samp) if p.ry else 0
    sp = [[p.spatial[8 * min(j * v_samp, p.ry) + min(i * h_samp, p.rx)] for i in range(rx + 1)] for j in range(ry + 1)]
    return Bilateral(p, plane_from_tables(rx, ry, sp, p.range))


def iterate(b: Bilateral, n: int) -> List[Bilateral]:
    """b, n times: the steps of Context.smooth_pictures (repeated mild smoothing flattens more than one strong pass)"""
    check(b)
    if not _int(n) or n < 1:
        raise ValueError(f"iterate: {n!r} steps (at least 1)")
    return [b] * int(n)


def as_steps(steps: Union[Bilateral, Sequence[Bilateral]]) -> List[Bilateral]:
    """a Bilateral or a list of them -> the checked list of steps (at least one)"""
    steps = [steps] if isinstance(steps, Bilateral) else list(steps) if isinstance(steps, (list, tuple)) else None
    if not steps:
        raise ValueError("steps: a bilateral.Bilateral or a non-empty list of them")
    for s in steps:
        if not isinstance(s, Bilateral):
            raise ValueError(f"steps: an entry is a bilateral.Bilateral, not {type(s).__name__}")
        check(s)
    return steps


# ------------------------------------------------------------------------------------------------------- the values to expect
def of_plane(a, g, plane: PlaneBilateral) -> np.ndarray:
    """a plane (2-D uint8) with the guide plane g (None: a itself) through a plane's set -> uint8 of the same shape.  Whole shifted
    planes at a time: one pass per tap over uint64 sums"""
    check_plane(plane)
    a = np.asarray(a)
    g = a if g is None else np.asarray(g)
    if a.ndim != 2 or a.dtype != np.uint8 or g.shape != a.shape or g.dtype != np.uint8:
        raise ValueError("a plane and its guide are 2-D uint8 arrays of one shape")
    ny, nx = a.shape
    rx, ry = plane.rx, plane.ry
    ea = np.pad(a, ((ry, ry), (rx, rx)), mode="edge").astype(np.uint64)
    eg = np.pad(g, ((ry, ry), (rx, rx)), mode="edge").astype(np.int64)
    gc = g.astype(np.int64)
    rg = np.frombuffer(plane.range, dtype=np.uint8).astype(np.uint64)
    num = np.zeros((ny, nx), dtype=np.uint64)
    den = np.zeros((ny, nx), dtype=np.uint64)
    for j in range(-ry, ry + 1):
        for i in range(-rx, rx + 1):
            s = plane.spatial[8 * abs(j) + abs(i)]
            if not s:
                continue
            w = np.uint64(s) * rg[np.abs(eg[ry + j:ry + j + ny, rx + i:rx + i + nx] - gc)]
            den += w
            num += w * ea[ry + j:ry + j + ny, rx + i:rx + i + nx]
    return ((num + den // np.uint64(2)) // den).astype(np.uint8)


def of_picture(pic, geom, b: Bilateral, guide=None) -> np.ndarray:
    """the expected bytes of hvq_bilateral_pictures: the picture `pic` (Y | U | V of geometry geom = (w, h, h_samp, v_samp)) through
    `b`, guided by the picture `guide` of the same geometry (None: by itself) -> uint8 [the picture's bytes]"""
    from .scale import planes
    check(b)
    w, h, hs, vs = geom
    gp = [None] * 3 if guide is None else planes(guide, w, h, hs, vs)
    return np.concatenate([of_plane(a, gp[i], b.chroma if i else b.luma).reshape(-1) for i, a in enumerate(planes(pic, w, h, hs, vs))])


def of_steps(pic, geom, steps: Sequence[Bilateral], guide=None) -> np.ndarray:
    """the expected bytes of Context.smooth_pictures: the picture through every step in turn, every step under the same guide"""
    out = np.asarray(pic, dtype=np.uint8).reshape(-1)
    for s in steps:
        out = of_picture(out, geom, s, guide)
    return out
