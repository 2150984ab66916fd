"""Separable integer filters on pictures in slot layout (hvq_filter_pictures / Context.filter_pictures): the filters, the values to
expect, and the helpers around them.  numpy only.

A picture is its bytes Y | U | V tightly packed.  Each plane goes through its PlaneFilter, a sum of one or two separable integer
kernels with one rounding, which include/hvqm4_amd.h specifies as exact integers:
    T_t[y][x] = sum_j sum_i wy_t[j] wx_t[i] a[cy(y + j - ry_t)][cx(x + i - rx_t)]        (correlation, borders replicate)
    S = T_0 + T_1 | |T_0 + T_1| | |T_0| + |T_1|;   out = clamp(((S + half) >> shift) + bias, 0, 255),  half = shift ? 1 << (shift - 1) : 0
A geometry is (width, height, h_samp, v_samp).  A Filter holds the plane filter of Y and that of U and V; the builders give both
planes the same one, luma_only and chroma_for change the chroma's.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from fractions import Fraction
from typing import Optional, Tuple

import numpy as np

MAX_RADIUS = 15                  # HVQ_FLT_MAX_RADIUS
MAX_TAPS = 31                    # HVQ_FLT_MAX_TAPS
MAX_SHIFT = 22                   # HVQ_FLT_MAX_SHIFT
MAX_GAIN = 1 << 22               # HVQ_FLT_MAX_GAIN
MAX_FILTERS = 64                 # HVQ_FLT_MAX_FILTERS
SUM, ABS_SUM, SUM_ABS = 0, 1, 2  # HVQ_FLT_SUM, HVQ_FLT_ABS_SUM, HVQ_FLT_SUM_ABS


@dataclass(frozen=True)
class Term:
    """one separable kernel: wx and wy are tuples of 2 r + 1 integers (int16), radius (len - 1) / 2 each"""
    wx: Tuple[int, ...]
    wy: Tuple[int, ...]

    @property
    def rx(self) -> int:
        return (len(self.wx) - 1) // 2

    @property
    def ry(self) -> int:
        return (len(self.wy) - 1) // 2


@dataclass(frozen=True)
class PlaneFilter:
    terms: Tuple[Term, ...]
    combine: int = SUM
    shift: int = 0
    bias: int = 0


@dataclass(frozen=True)
class Filter:
    """luma for Y, chroma for U and V (at their own resolution).  Hashable; equal when the plane filters are.  `recipe` remembers what a
    builder made (chroma_for reads it) and takes no part in the comparison."""
    luma: PlaneFilter
    chroma: PlaneFilter
    recipe: Optional[tuple] = field(default=None, compare=False)

    def to_struct(self):
        """the HvqFilter of include/hvqm4_amd.h (ctypes)"""
        from ._lib import HvqFilter
        check(self)
        s = HvqFilter()
        for dst, p in ((s.luma, self.luma), (s.chroma, self.chroma)):
            dst.terms, dst.combine, dst.shift, dst.bias = len(p.terms), p.combine, p.shift, p.bias
            for t, term in enumerate(p.terms):
                dst.term[t].rx, dst.term[t].ry = term.rx, term.ry
                for i, w in enumerate(term.wx):
                    dst.term[t].wx[i] = w
                for i, w in enumerate(term.wy):
                    dst.term[t].wy[i] = w
        return s


def _both(p: PlaneFilter, recipe=None) -> Filter:
    return Filter(p, p, recipe)


IDENTITY_PLANE = PlaneFilter((Term((1,), (1,)),))


def gain(p: PlaneFilter) -> int:
    """sum over the terms of (sum |wx|) (sum |wy|): 255 gain bounds every partial sum"""
    return sum(sum(abs(w) for w in t.wx) * sum(abs(w) for w in t.wy) for t in p.terms)


def check_plane(p: PlaneFilter) -> None:
    """ValueError for what hvq_filter_check refuses in a plane filter"""
    if not isinstance(p, PlaneFilter):
        raise ValueError(f"a plane filter, not {type(p).__name__}")
    if len(p.terms) not in (1, 2):
        raise ValueError(f"{len(p.terms)} terms: 1 or 2")
    if p.combine not in (SUM, ABS_SUM, SUM_ABS):
        raise ValueError(f"combine {p.combine}: SUM, ABS_SUM or SUM_ABS")
    if not 0 <= p.shift <= MAX_SHIFT:
        raise ValueError(f"shift {p.shift} outside 0 .. {MAX_SHIFT}")
    if not -255 <= p.bias <= 255:
        raise ValueError(f"bias {p.bias} outside -255 .. 255")
    for t in p.terms:
        for w in (t.wx, t.wy):
            if len(w) % 2 == 0 or len(w) > MAX_TAPS:
                raise ValueError(f"{len(w)} taps: an odd number up to {MAX_TAPS} (radius 0 .. {MAX_RADIUS})")
            if any(not -32768 <= v <= 32767 for v in w):
                raise ValueError("a tap is a 16-bit integer")
    if not 1 <= gain(p) <= MAX_GAIN:
        raise ValueError(f"a gain of {gain(p)}: 1 .. {MAX_GAIN}")


def check(f: Filter) -> None:
    """ValueError for what hvq_filter_check refuses"""
    if not isinstance(f, Filter):
        raise ValueError(f"a filters.Filter, not {type(f).__name__}")
    check_plane(f.luma)
    check_plane(f.chroma)


def is_identity(p: PlaneFilter) -> bool:
    """the plane filter leaves every sample as it is (the kernel's copy body takes it)"""
    t = p.terms[0]
    return len(p.terms) == 1 and len(t.wx) == 1 and len(t.wy) == 1 and p.bias == 0 and t.wx[0] * t.wy[0] == 1 << p.shift


# ------------------------------------------------------------------------------------------------------------ the builders
def identity() -> Filter:
    return _both(IDENTITY_PLANE, ("identity",))


def binomial_taps(n: int) -> Tuple[int, ...]:
    """row n - 1 of Pascal's triangle: n taps that sum to 2^(n - 1)"""
    if n < 1 or n % 2 == 0 or n > 11:
        raise ValueError(f"binomial({n}): an odd number of taps, 1 .. 11 (the gain of the 2-D kernel is 4^(n - 1) <= 2^22)")
    return tuple(math.comb(n - 1, k) for k in range(n))


def binomial(n: int = 3) -> Filter:
    """the n x n binomial blur: (1, 2, 1) / 4 in each axis for n = 3"""
    w = binomial_taps(n)
    return _both(PlaneFilter((Term(w, w),), SUM, 2 * (n - 1), 0), ("binomial", n))


def gaussian_taps(sigma: float, radius: Optional[int] = None, bits: int = 8) -> Tuple[int, ...]:
    """2 r + 1 integer taps of a Gaussian that sum to exactly 2^bits: with g_k = exp(-k^2 / (2 sigma^2)) for |k| <= r,
    w[k] = floor(2^bits g_k / sum g + 1/2) for k = 1 .. r, and the centre takes the rest, 2^bits - 2 sum w[k] (corrected, see below, in
    the rare case that this leaves it below w[1]).  Symmetric, non-increasing from the centre.  The default radius is
    min(15, ceil(3 sigma))."""
    if not sigma > 0:
        raise ValueError(f"sigma {sigma}: above 0")
    if radius is None:
        radius = min(MAX_RADIUS, int(math.ceil(3 * sigma)))
    if not 0 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius {radius} outside 0 .. {MAX_RADIUS}")
    if not 1 <= bits <= 14:
        raise ValueError(f"bits {bits} outside 1 .. 14")
    g = [math.exp(-k * k / (2.0 * sigma * sigma)) for k in range(radius + 1)]
    total = g[0] + 2.0 * sum(g[1:])
    side = [int(math.floor((1 << bits) * g[k] / total + 0.5)) for k in range(1, radius + 1)]
    centre = (1 << bits) - 2 * sum(side)
    # The side taps are rounded to nearest one by one and the centre absorbs all their errors: for a wide Gaussian at few bits it can
    # come out below its neighbours (sigma 3.25, 8 bits: .. 30 28 30 ..).  Then units move from the outer end of the neighbours' plateau
    # to the centre until it is the maximum again: the sum, the symmetry and the order of the side taps stay as they are.
    while side and centre < side[0]:
        k = max(i for i, w in enumerate(side) if w == side[0])
        side[k] -= 1
        centre += 2
    return tuple(side[::-1]) + (centre,) + tuple(side)


def _gaussian_plane(sx: float, sy: float, radius, bits) -> PlaneFilter:
    return PlaneFilter((Term(gaussian_taps(sx, radius, bits), gaussian_taps(sy, radius, bits)),), SUM, 2 * bits, 0)


def gaussian(sigma: float, radius: Optional[int] = None, bits: int = 8) -> Filter:
    """the Gaussian blur of standard deviation sigma (in samples of the plane it meets), weights of `bits` bits per axis"""
    return _both(_gaussian_plane(sigma, sigma, radius, bits), ("gaussian", float(sigma), radius, bits))


_SMOOTH = {"sobel": (1, 2, 1), "scharr": (3, 10, 3)}
_GRADIENT_SHIFT = {"sobel": 2, "scharr": 4}           # a straight full-swing edge answers 4 * 255 and 16 * 255


def _derivative(kind: str, axis: str) -> Term:
    if kind not in _SMOOTH:
        raise ValueError(f"kind {kind!r}: 'sobel' or 'scharr'")
    if axis not in ("x", "y"):
        raise ValueError(f"axis {axis!r}: 'x' or 'y'")
    d, s = (-1, 0, 1), _SMOOTH[kind]
    return Term(d, s) if axis == "x" else Term(s, d)


def sobel(axis: str = "x", shift: int = 3, bias: int = 128) -> Filter:
    """the Sobel derivative along `axis` (towards larger x / y is positive), 128 + d / 8 by default"""
    return _both(PlaneFilter((_derivative("sobel", axis),), SUM, shift, bias), ("sobel", axis))


def scharr(axis: str = "x", shift: int = 5, bias: int = 128) -> Filter:
    """the Scharr derivative along `axis`, 128 + d / 32 by default"""
    return _both(PlaneFilter((_derivative("scharr", axis),), SUM, shift, bias), ("scharr", axis))


def gradient_magnitude(kind: str = "sobel", shift: Optional[int] = None) -> Filter:
    """|d/dx| + |d/dy| of the Sobel or Scharr derivatives (two terms, SUM_ABS), divided by 4 (Sobel) or 16 (Scharr) by default: a
    straight full-swing edge gives 255"""
    sh = _GRADIENT_SHIFT.get(kind, 0) if shift is None else shift
    return _both(PlaneFilter((_derivative(kind, "x"), _derivative(kind, "y")), SUM_ABS, sh, 0), ("gradient_magnitude", kind))


def laplacian(shift: int = 3, bias: int = 128) -> Filter:
    """the 4-neighbour Laplacian as two terms, (1, -2, 1) along x plus (1, -2, 1) along y: 128 + L / 8 by default"""
    return _both(PlaneFilter((Term((1, -2, 1), (1,)), Term((1,), (1, -2, 1))), SUM, shift, bias), ("laplacian",))


def dog(sigma_a: float, sigma_b: float, bits: int = 8, gain_bits: int = 0, bias: int = 128) -> Filter:
    """a difference of Gaussians, G(sigma_a) - G(sigma_b), as two terms: bias + 2^gain_bits (G_a - G_b)"""
    if not 0 <= gain_bits <= 2 * bits:
        raise ValueError(f"gain_bits {gain_bits} outside 0 .. {2 * bits}")
    a, b = gaussian_taps(sigma_a, None, bits), gaussian_taps(sigma_b, None, bits)
    return _both(PlaneFilter((Term(a, a), Term(b, tuple(-w for w in b))), SUM, 2 * bits - gain_bits, bias), ("dog", float(sigma_a), float(sigma_b), bits))


def _unsharp_plane(sx: float, sy: float, amount: Fraction, radius, bits: int) -> PlaneFilter:
    p, den = amount.numerator, amount.denominator
    q = den.bit_length() - 1
    gx, gy = gaussian_taps(sx, radius, bits), gaussian_taps(sy, radius, bits)
    # ((den + p) 2^(2 bits) delta - p G) / (den 2^(2 bits)): the delta's weight is split over its two one-tap axes
    return PlaneFilter((Term((1 << bits,), ((den + p) << bits,)), Term(gx, tuple(-p * w for w in gy))), SUM, q + 2 * bits, 0)


def _amount(amount) -> Fraction:
    a = Fraction(amount)
    if a <= 0 or a.denominator & (a.denominator - 1):
        raise ValueError(f"amount {amount}: a positive rational with a power-of-two denominator")
    return a


def unsharp(sigma: float, amount=Fraction(1, 2), radius: Optional[int] = None, bits: int = 8) -> Filter:
    """unsharp masking, a + amount (a - G a) = (1 + amount) a - amount G a, as two terms with one rounding; `amount` is a rational
    with a power-of-two denominator (1/2, 0.75, 2, ...).  ValueError when the weights leave 16 bits or the gain 2^22: lower `bits`."""
    a = _amount(amount)
    return _both(_unsharp_plane(sigma, sigma, a, radius, bits), ("unsharp", float(sigma), a, radius, bits))


def luma_only(f: Filter) -> Filter:
    """f on Y, the identity on U and V"""
    return Filter(f.luma, IDENTITY_PLANE, f.recipe)


def chroma_for(f: Filter, h_samp: int, v_samp: int) -> Filter:
    """f with the chroma planes' filter adapted to their resolution: for a Gaussian (and the Gaussian of unsharp) sigma is divided by
    the sampling of each axis, the radius following it, so that the blur covers the same part of the picture in every plane; any
    other filter meets the chroma planes as it meets Y"""
    if (h_samp, v_samp) not in ((2, 2), (2, 1), (1, 1)):
        raise ValueError(f"sampling {(h_samp, v_samp)}: (2, 2), (2, 1) or (1, 1)")
    r = f.recipe
    if r and r[0] == "gaussian":
        _n, sigma, _radius, bits = r
        return Filter(f.luma, _gaussian_plane(sigma / h_samp, sigma / v_samp, None, bits), r)
    if r and r[0] == "unsharp":
        _n, sigma, amount, _radius, bits = r
        return Filter(f.luma, _unsharp_plane(sigma / h_samp, sigma / v_samp, amount, None, bits), r)
    return Filter(f.luma, f.luma, r)


# ------------------------------------------------------------------------------------------------------- the values to expect
def _correlate(a: np.ndarray, w, axis: int) -> np.ndarray:
    """sum_i w[i] a[.. clamp(k + i - r) ..] along `axis`, int64"""
    r = (len(w) - 1) // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    e = np.pad(a, pad, mode="edge")
    n = a.shape[axis]
    out = np.zeros(a.shape, dtype=np.int64)
    for i, v in enumerate(w):
        if v:
            out += v * (e[i:i + n, :] if axis == 0 else e[:, i:i + n])
    return out


def terms_of_plane(plane, p: PlaneFilter):
    """the exact T_t of a plane (2-D uint8), a list of int64 arrays"""
    a = np.asarray(plane)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError("a plane is a 2-D uint8 array")
    a = a.astype(np.int64)
    return [_correlate(_correlate(a, t.wx, 1), t.wy, 0) for t in p.terms]


def of_plane(plane, p: PlaneFilter) -> np.ndarray:
    """a plane (2-D uint8) through a plane filter -> uint8 of the same shape"""
    check_plane(p)
    t = terms_of_plane(plane, p)
    if len(t) == 1:
        t.append(np.zeros_like(t[0]))
    s = t[0] + t[1] if p.combine == SUM else np.abs(t[0] + t[1]) if p.combine == ABS_SUM else np.abs(t[0]) + np.abs(t[1])
    half = 1 << (p.shift - 1) if p.shift else 0
    return np.clip(((s + half) >> p.shift) + p.bias, 0, 255).astype(np.uint8)


def of_picture(buf, geom, filt: Filter) -> np.ndarray:
    """the expected bytes of hvq_filter_pictures: the picture `buf` (Y | U | V of geometry geom = (w, h, h_samp, v_samp)) through
    `filt` -> uint8 [the picture's bytes]"""
    from .scale import planes
    check(filt)
    w, h, hs, vs = geom
    return np.concatenate([of_plane(a, filt.chroma if i else filt.luma).reshape(-1) for i, a in enumerate(planes(buf, w, h, hs, vs))])


def sharpness(hist) -> np.ndarray:
    """the mean of a gradient-magnitude histogram as picture_histograms returns it (integer counts [..., 256]), float64 [...]: filter
    with luma_only(gradient_magnitude()), count with picture_histograms(src=), read the Y row.  Larger is sharper (or blockier)."""
    from .histograms import mean
    return mean(hist)
