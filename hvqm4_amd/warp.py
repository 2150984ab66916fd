"""Warped pictures in slot layout (hvq_warp_pictures / Context.warp_pictures): the maps, the values to expect, and the helpers around
them.  numpy only.

A picture is its bytes Y | U | V tightly packed (what read_picture returns, what a slot holds).  A Warp holds six Q16 integers (65536 =
1.0) that map TARGET luma coordinates to SOURCE luma coordinates, u = m00 x + m01 y + t0, v = m10 x + m11 y + t1, sample centres at
integer + 1/2 and chroma at the centre of its luma cell; every plane takes bilinear taps in exact integers with one rounding
(include/hvqm4_amd.h is the specification).  The builders are named for what the PICTURE does and store the inverse map: translate(3, 0)
moves the content three samples to the right.  A geometry is (width, height, h_samp, v_samp).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from fractions import Fraction
from typing import Sequence, Tuple

import numpy as np

from .scale import SAMPLINGS, nbytes, planes

ONE = 65536
MAX_SCALE = 32 * ONE             # HVQ_WARP_MAX_SCALE
REPLICATE, CONSTANT = 0, 1       # HVQ_WARP_REPLICATE, HVQ_WARP_CONSTANT
DIRECT, TILED = 0, 1             # HVQ_WARP_DIRECT, HVQ_WARP_TILED
TILE_W, TILE_H, LDS_DWORDS, TILED_ROWS = 64, 16, 4096, 8       # hvq_warp.h
INT32 = (-(1 << 31), (1 << 31) - 1)


@dataclass(frozen=True)
class Warp:
    """the inverse map of a picture, Q16, and what lies outside the source: border REPLICATE (the edge sample) or CONSTANT (fill =
    (Y, U, V))"""
    m00: int = ONE
    m01: int = 0
    m10: int = 0
    m11: int = ONE
    t0: int = 0
    t1: int = 0
    border: int = REPLICATE
    fill: Tuple[int, int, int] = (0, 128, 128)

    def coefficients(self) -> Tuple[int, int, int, int, int, int]:
        return (self.m00, self.m01, self.m10, self.m11, self.t0, self.t1)

    def to_struct(self):
        """the HvqWarp of the C interface"""
        from ._lib import HvqWarp
        check(self)
        s = HvqWarp(*self.coefficients(), self.border)
        for p in range(3):
            s.fill[p] = self.fill[p]
        s.pad = 0
        return s


def check(w: Warp) -> Warp:
    """ValueError for what hvq_warp_check refuses, and for what the record cannot hold"""
    if not isinstance(w, Warp):
        raise ValueError(f"a warp is a warp.Warp, not {type(w).__name__}")
    for name, v in zip(("m00", "m01", "m10", "m11", "t0", "t1"), w.coefficients()):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
            raise ValueError(f"warp: {name} = {v!r} is no integer")
        if name[0] == "m" and abs(int(v)) > MAX_SCALE:
            raise ValueError(f"warp: coefficient {name} = {v} beyond {MAX_SCALE} (a scale of 32)")
        if not INT32[0] <= int(v) <= INT32[1]:
            raise ValueError(f"warp: {name} = {v} does not fit 32 bits")
    if w.border not in (REPLICATE, CONSTANT):
        raise ValueError(f"warp: border {w.border!r} (REPLICATE or CONSTANT)")
    if not isinstance(w.fill, tuple) or len(w.fill) != 3 or any(not isinstance(v, (int, np.integer)) or not 0 <= v <= 255 for v in w.fill):
        raise ValueError(f"warp: fill {w.fill!r} (three values 0 .. 255)")
    return w


# ------------------------------------------------------------------------------------------------- exact arithmetic
def _frac(v) -> Fraction:
    return v if isinstance(v, Fraction) else Fraction(v)


def _q16(v: Fraction) -> int:
    return math.floor(v * ONE + Fraction(1, 2))


def _matrix(w: Warp):
    """the inverse map as 2 x 3 Fractions"""
    return [[Fraction(w.m00, ONE), Fraction(w.m01, ONE), Fraction(w.t0, ONE)], [Fraction(w.m10, ONE), Fraction(w.m11, ONE), Fraction(w.t1, ONE)]]


def _from_matrix(m, border=REPLICATE, fill=(0, 128, 128)) -> Warp:
    """one floor(v * 65536 + 1/2) per coefficient"""
    return check(Warp(_q16(m[0][0]), _q16(m[0][1]), _q16(m[1][0]), _q16(m[1][1]), _q16(m[0][2]), _q16(m[1][2]), border, tuple(fill)))


def _invert(m):
    (a, b, c), (d, e, f) = m
    det = a * e - b * d
    if det == 0:
        raise ValueError("the map is singular: it has no inverse")
    return [[e / det, -b / det, (b * f - c * e) / det], [-d / det, a / det, (c * d - a * f) / det]]


def _about(m, centre):
    """the linear part of m about `centre` instead of the origin"""
    cx, cy = _frac(centre[0]), _frac(centre[1])
    (a, b, _c), (d, e, _f) = m
    return [[a, b, cx - a * cx - b * cy], [d, e, cy - d * cx - e * cy]]


# ------------------------------------------------------------------------------------------------- the builders
def identity() -> Warp:
    """the picture as it is"""
    return Warp()


def translate(dx, dy) -> Warp:
    """the content moves dx samples to the right and dy down (fractions allowed: translate(-0.5, 0) averages neighbours)"""
    return _from_matrix([[1, 0, -_frac(dx)], [0, 1, -_frac(dy)]])


def flip_h(w: int) -> Warp:
    """the mirror image of a picture w wide: left and right change places"""
    return _from_matrix([[-1, 0, w], [0, 1, 0]])


def flip_v(h: int) -> Warp:
    """a picture h high upside down: top and bottom change places"""
    return _from_matrix([[1, 0, 0], [0, -1, h]])


def transpose() -> Warp:
    """rows become columns: the target of a w x h picture is h x w"""
    return _from_matrix([[0, 1, 0], [1, 0, 0]])


def rotate90(k: int, w: int, h: int) -> Tuple[Warp, Tuple[int, int]]:
    """a w x h picture turned by k quarter turns counter-clockwise, as numpy.rot90(plane, k) turns a plane -> (warp, (w', h') of
    the target): exact permutations of the samples wherever the chroma sampling is square"""
    k %= 4
    if k == 0:
        return identity(), (w, h)
    if k == 1:
        return _from_matrix([[0, -1, w], [1, 0, 0]]), (h, w)
    if k == 2:
        return _from_matrix([[-1, 0, w], [0, -1, h]]), (w, h)
    return _from_matrix([[0, 1, 0], [-1, 0, h]]), (h, w)


def rotate(degrees, w: int, h: int) -> Warp:
    """a w x h picture turned counter-clockwise by `degrees` about its centre, into a target of the same size"""
    q = _frac(degrees) / 90
    if q.denominator == 1:
        c, s = ((1, 0), (0, 1), (-1, 0), (0, -1))[int(q) % 4]
    else:
        r = math.radians(float(degrees))
        c, s = Fraction(math.cos(r)), Fraction(math.sin(r))
    return _from_matrix(_about([[c, -s, 0], [s, c, 0]], (Fraction(w, 2), Fraction(h, 2))))


def zoom(fx, fy=None, centre=(0, 0)) -> Warp:
    """the content grows by fx horizontally and fy (default fx) vertically about `centre`: zoom(2, centre=(w / 2, h / 2)) shows the
    middle of the picture twice as large; zoom(Fraction(1, 2)) into a target of half the size is a 2:1 reduction of the whole picture"""
    fx = _frac(fx)
    fy = fx if fy is None else _frac(fy)
    if fx == 0 or fy == 0:
        raise ValueError("a zoom by 0 has no inverse")
    return _from_matrix(_about([[1 / fx, 0, 0], [0, 1 / fy, 0]], centre))


def shear(kx, ky=0, centre=(0, 0)) -> Warp:
    """the content sheared about `centre`: a sample moves kx to the right for every row below the centre, and ky down for every column
    right of it"""
    inv = _invert([[1, _frac(kx), 0], [_frac(ky), 1, 0]])
    return _from_matrix(_about(inv, centre))


def affine(forward: Sequence[Sequence]) -> Warp:
    """the picture under the 2 x 3 FORWARD matrix (source luma coordinates -> target luma coordinates, as OpenCV's warpAffine takes
    it): inverted exactly, then rounded"""
    m = [[_frac(v) for v in row] for row in forward]
    if len(m) != 2 or any(len(r) != 3 for r in m):
        raise ValueError("a forward matrix has two rows of three")
    return _from_matrix(_invert(m))


def compose(first: Warp, second: Warp) -> Warp:
    """what `first` does to the picture, then what `second` does to the result, as one warp (border and fill of `second`): exact in
    Fractions, then one rounding per coefficient"""
    (a, b, c), (d, e, f) = _matrix(check(first))
    (p, q, r), (s, t, u) = _matrix(check(second))
    m = [[a * p + b * s, a * q + b * t, a * r + b * u + c], [d * p + e * s, d * q + e * t, d * r + e * u + f]]
    return _from_matrix(m, second.border, second.fill)


def invert(w: Warp) -> Warp:
    """the warp that undoes w (ValueError for a singular one)"""
    return _from_matrix(_invert(_matrix(check(w))), w.border, w.fill)


def with_border(w: Warp, border: int, fill=None) -> Warp:
    """w with another border rule (and fill)"""
    return check(replace(w, border=border, fill=w.fill if fill is None else tuple(int(v) for v in fill)))


def from_motion(vector) -> Warp:
    """the map under which the warped REFERENCE predicts the picture, for a vector (dy, dx) of picture_motion / motion.global_motion:
    the picture at (y, x) looks like the reference at (y + dy, x + dx)"""
    dy, dx = vector
    return translate(-int(dx), -int(dy))


# ------------------------------------------------------------------------------------------------- the values
def _samplings(src_geom, dst_geom, plane: int):
    if tuple(src_geom[2:]) not in SAMPLINGS or tuple(dst_geom[2:]) not in SAMPLINGS:
        raise ValueError(f"samplings {tuple(src_geom[2:])} -> {tuple(dst_geom[2:])}: each is one of {SAMPLINGS}")
    return ((dst_geom[2], dst_geom[3]), (src_geom[2], src_geom[3])) if plane else ((1, 1), (1, 1))


def plane_dims(geom, plane: int) -> Tuple[int, int]:
    """(samples a row, rows) of a plane of a geometry"""
    w, h, hs, vs = geom
    return (w >> (hs == 2), h >> (vs == 2)) if plane else (w, h)


def coords(w: Warp, src_geom, dst_geom, plane: int, saturate: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """(U8, V8), int64 [My, Mx]: the source position of every target sample of a plane in 1 / 256 of a sample of the source plane;
    saturate: to [-512, 256 Nx] and [-512, 256 Ny], which changes no value of the picture"""
    (hd, vd), (hs, vs) = _samplings(src_geom, dst_geom, plane)
    mx, my = plane_dims(dst_geom, plane)
    nx, ny = plane_dims(src_geom, plane)
    x = 2 * np.arange(mx, dtype=np.int64)[None, :] + 1
    y = 2 * np.arange(my, dtype=np.int64)[:, None] + 1
    nu = w.m00 * hd * x + w.m01 * vd * y + 2 * w.t0 - ONE * hs
    nv = w.m10 * hd * x + w.m11 * vd * y + 2 * w.t1 - ONE * vs
    u8, v8 = (nu + 256 * hs) >> (8 + hs), (nv + 256 * vs) >> (8 + vs)        # 512 h = 2^(8 + h) for h = 1, 2; >> floors
    if saturate:
        u8, v8 = np.clip(u8, -512, 256 * nx), np.clip(v8, -512, 256 * ny)
    return u8, v8


def of_plane(a, u8, v8, border: int = REPLICATE, fill: int = 0) -> np.ndarray:
    """the bilinear taps of plane a (2-D uint8) at the positions (U8, V8) -> uint8 of their shape"""
    a = np.asarray(a)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError("a plane is a 2-D uint8 array")
    ny, nx = a.shape
    u8, v8 = np.asarray(u8, dtype=np.int64), np.asarray(v8, dtype=np.int64)
    ix, iy, fx, fy = u8 >> 8, v8 >> 8, u8 & 255, v8 & 255
    wide = a.astype(np.int64)

    def tap(j, i):
        x, y = ix + i, iy + j
        t = wide[np.clip(y, 0, ny - 1), np.clip(x, 0, nx - 1)]
        if border == CONSTANT:
            t = np.where((x >= 0) & (x < nx) & (y >= 0) & (y < ny), t, int(fill))
        return t
    s = (256 - fy) * ((256 - fx) * tap(0, 0) + fx * tap(0, 1)) + fy * ((256 - fx) * tap(1, 0) + fx * tap(1, 1))
    return ((s + 32768) >> 16).astype(np.uint8)


def of_picture(buf, geom, w: Warp, target_geom=None, saturate: bool = False) -> np.ndarray:
    """the expected bytes of hvq_warp_pictures: the picture `buf` (Y | U | V of geometry `geom`) under w into target_geom (None: geom)
    -> uint8 [nbytes(*target_geom)]"""
    check(w)
    target_geom = tuple(geom) if target_geom is None else tuple(target_geom)
    tw, th = target_geom[:2]
    if tw < 8 or th < 8 or tw % 8 or th % 8 or tw > 8192 or th > 8192:
        raise ValueError(f"target {tw}x{th}: multiples of 8 up to 8192")
    out = []
    for p, a in enumerate(planes(buf, *geom)):
        u8, v8 = coords(w, geom, target_geom, p, saturate)
        out.append(of_plane(a, u8, v8, w.border, w.fill[p]).reshape(-1))
    got = np.concatenate(out)
    assert got.size == nbytes(*target_geom)
    return got


def body(w: Warp, src_geom, dst_geom, plane: int) -> int:
    """DIRECT or TILED: the body of the kernel a plane takes (hvq_warp_body; the arithmetic of hvq_warp.h restated); the values do
    not depend on it"""
    check(w)
    (hd, vd), (hs, vs) = _samplings(src_geom, dst_geom, plane)
    nx, ny = plane_dims(src_geom, plane)

    def span(a, b, s, n):
        d = abs(a) * (TILE_W - 1) + abs(b) * (TILE_H - 1)
        return min((((d + (1 << s) - 1) >> s) + 255 >> 8) + 2, n)
    au, bu, av, bv = 2 * w.m00 * hd, 2 * w.m01 * vd, 2 * w.m10 * hd, 2 * w.m11 * vd
    pitch = max(3, ((span(au, bu, 8 + hs, nx) + 6) >> 2) | 1)
    rows = span(av, bv, 8 + vs, ny)
    crossed = (abs(av) * (TILE_W - 1)) >> (8 + vs + 8)
    return TILED if pitch * rows <= LDS_DWORDS and crossed >= TILED_ROWS else DIRECT
