"""Scaled pictures in slot layout (hvq_scale_pictures / Context.scale_pictures): the values to expect, and the helpers around them.
numpy only.

A picture is its bytes Y | U | V tightly packed (what read_picture returns, what a slot holds).  Each plane is resampled on its own by
the area filter with rational cell edges that include/hvqm4_amd.h specifies as exact integers:
    w(r, y) = max(0, min(m (y + 1), n (r + 1)) - max(m y, n r));  S = wy a wx^T;  out = (S + (D >> 1)) // D with D = Nx Ny
-- one rounding, half up.  A geometry is (width, height, h_samp, v_samp); a crop is (x, y, w, h) in luma samples of the source.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from .checksums import plane_bytes

MAX_RATIO = 32                   # HVQ_SCALE_MAX_RATIO: n <= 32 m for every plane and axis
DIRECT, TILED = 0, 1             # HVQ_SCALE_DIRECT, HVQ_SCALE_TILED
SAMPLINGS = ((2, 2), (2, 1), (1, 1))


def weights(n: int, m: int) -> np.ndarray:
    """int64 [m, n]: w[r, y] = max(0, min(m y + m, n r + n) - max(m y, n r)), the share (in units of 1 / m of a sample) of source
    sample y in target sample r when n samples become m.  Every row sums to n, every column to m."""
    y = np.arange(n, dtype=np.int64)[None, :]
    r = np.arange(m, dtype=np.int64)[:, None]
    return np.maximum(0, np.minimum(m * y + m, n * r + n) - np.maximum(m * y, n * r))


def magic(d: int) -> int:
    """ceil(2^64 / d): the multiplier the kernel divides by d with (hvq_sc_magic of hvq_scale.h)"""
    if not 1 < d <= 1 << 26:
        raise ValueError(f"a plane has 2 .. 2^26 samples, not {d}")
    return ((1 << 64) + d - 1) // d


def divide(v: int, d: int) -> int:
    """v // d the way the kernel computes it: the high 64 bits of v * magic(d).  Exact for v < 2^35 (hvq_scale.h: the proof)."""
    return ((int(v) & 0xFFFFFFFFFFFFFFFF) * magic(d)) >> 64


def of_plane(plane, mx: int, my: int) -> np.ndarray:
    """a plane (2-D uint8, ny x nx) resampled to my x mx -> uint8 [my, mx]"""
    a = np.asarray(plane)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError("a plane is a 2-D uint8 array")
    ny, nx = a.shape
    if mx < 1 or my < 1 or nx > MAX_RATIO * mx or ny > MAX_RATIO * my:
        raise ValueError(f"{nx} x {ny} -> {mx} x {my}: a reduction beyond {MAX_RATIO}, or no target")
    d = nx * ny
    # products of integers in float64 (BLAS): every partial sum is an integer of at most 255 nx ny < 2^34, exact below 2^53
    s = weights(ny, my).astype(np.float64) @ a.astype(np.float64) @ weights(nx, mx).T.astype(np.float64)
    return ((np.rint(s).astype(np.int64) + (d >> 1)) // d).astype(np.uint8)


def nbytes(width: int, height: int, h_samp: int = 2, v_samp: int = 2) -> int:
    """bytes of a picture of that geometry (hvq_scale_bytes)"""
    return sum(plane_bytes(width, height, h_samp, v_samp))


def planes(buf, w: int, h: int, hs: int = 2, vs: int = 2) -> List[np.ndarray]:
    """the Y, U, V views (2-D uint8) of a slot-layout buffer of a w x h picture with sampling (hs, vs)"""
    b = np.frombuffer(bytes(buf), dtype=np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else np.asarray(buf)
    if b.dtype != np.uint8:
        raise TypeError(f"a picture is uint8, not {b.dtype}")
    b = b.reshape(-1)
    sizes = plane_bytes(w, h, hs, vs)
    if b.size != sum(sizes):
        raise ValueError(f"{b.size} bytes, a {w}x{h} picture of sampling ({hs}, {vs}) has {sum(sizes)}")
    cw, ch = w >> (hs == 2), h >> (vs == 2)
    y, u = sizes[0], sizes[0] + sizes[1]
    return [b[:y].reshape(h, w), b[y:u].reshape(ch, cw), b[u:].reshape(ch, cw)]


def check_crop(crop, src_geom) -> Tuple[int, int, int, int]:
    """a crop (None: the whole picture) of a source geometry as (x, y, w, h), checked as the library checks it"""
    w, h, hs, vs = src_geom
    if crop is None:
        return 0, 0, w, h
    x, y, cw, ch = (int(v) for v in crop)
    if x < 0 or y < 0 or cw <= 0 or ch <= 0 or x + cw > w or y + ch > h:
        raise ValueError(f"crop {(x, y, cw, ch)} is empty or leaves the {w}x{h} picture")
    if x % hs or cw % hs or y % vs or ch % vs:
        raise ValueError(f"crop {(x, y, cw, ch)}: x values are multiples of {hs}, y values of {vs} (the source's sampling)")
    if cw < 8 or ch < 8:
        raise ValueError(f"crop {(x, y, cw, ch)}: a cropped source is 8 x 8 luma samples at least")
    return x, y, cw, ch


def plane_sizes(src_geom, dst_geom, crop=None) -> List[Tuple[int, int, int, int]]:
    """per plane (nx, ny, mx, my): the samples of the crop's part of the source plane and of the target plane; ValueError beyond the
    limits of hvq_scale_pictures"""
    w, h, hs, vs = src_geom
    dw, dh, dhs, dvs = dst_geom
    if (hs, vs) not in SAMPLINGS or (dhs, dvs) not in SAMPLINGS:
        raise ValueError(f"samplings {(hs, vs)} -> {(dhs, dvs)}: each is one of {SAMPLINGS}")
    if dw < 8 or dh < 8 or dw % 8 or dh % 8 or dw > 8192 or dh > 8192:
        raise ValueError(f"target {dw}x{dh}: multiples of 8 up to 8192")
    _x, _y, cw, ch = check_crop(crop, src_geom)
    out = []
    for p in range(3):
        sx, sy = (hs == 2, vs == 2) if p else (0, 0)
        tx, ty = (dhs == 2, dvs == 2) if p else (0, 0)
        nx, ny, mx, my = cw >> sx, ch >> sy, dw >> tx, dh >> ty
        if nx > MAX_RATIO * mx or ny > MAX_RATIO * my:
            raise ValueError(f"plane {p}: {nx} x {ny} -> {mx} x {my} is a reduction beyond {MAX_RATIO}")
        out.append((nx, ny, mx, my))
    return out


def of_picture(buf, src_geom, dst_geom, crop=None) -> np.ndarray:
    """the expected bytes of hvq_scale_pictures: the picture `buf` (Y | U | V of geometry src_geom = (w, h, h_samp, v_samp)), cropped
    and resampled to dst_geom -> uint8 [nbytes(*dst_geom)]"""
    w, h, hs, vs = src_geom
    sizes = plane_sizes(src_geom, dst_geom, crop)
    x, y, _cw, _ch = check_crop(crop, src_geom)
    out = []
    for p, (a, (nx, ny, mx, my)) in enumerate(zip(planes(buf, w, h, hs, vs), sizes)):
        px, py = (x >> (hs == 2), y >> (vs == 2)) if p else (x, y)
        out.append(of_plane(a[py:py + ny, px:px + nx], mx, my).reshape(-1))
    return np.concatenate(out)


def body(nx: int, ny: int, mx: int, my: int) -> int:
    """DIRECT or TILED: the body of the kernel a plane takes (hvq_scale_body); the values do not depend on it"""
    from ._lib import check, lib
    return check(lib().hvq_scale_body(nx, ny, mx, my))


def fit(w: int, h: int, max_w: int, max_h: int) -> Tuple[int, int]:
    """the largest target inside max_w x max_h with the aspect of w x h, each side rounded to the nearest multiple of 8 and never
    below 8 (nor above the box's own multiple of 8)"""
    if min(w, h, max_w, max_h) < 8:
        raise ValueError("sizes are 8 at least")
    if w * max_h >= h * max_w:                       # the width binds
        tw, th = max_w, h * max_w / w
    else:
        tw, th = w * max_h / h, max_h
    r8 = lambda v, cap: max(8, min(cap // 8 * 8, int(v / 8 + 0.5) * 8))
    return r8(tw, max_w), r8(th, max_h)


def pyramid(w: int, h: int, levels: int) -> List[Tuple[int, int]]:
    """`levels` sizes, each half the one before (rounded to the nearest multiple of 8, never below 8), starting at w x h: the
    targets of a multi-scale SSIM or a coarse-to-fine motion search"""
    if levels < 1:
        raise ValueError("a pyramid has one level at least")
    out = [(w, h)]
    r8 = lambda v: max(8, (v + 8) // 16 * 8)
    for _ in range(levels - 1):
        out.append((r8(out[-1][0]), r8(out[-1][1])))
    return out


def per_picture(value, n: int, width: int, what: str):
    """(one tuple of `width` integers per picture, whether they are all the same object) from None, one tuple, or a list of n tuples
    (None entries stay)"""
    scalar = lambda e: isinstance(e, (int, np.integer)) and not isinstance(e, bool)
    if value is None:
        return [None] * n, True
    if isinstance(value, (list, tuple)) and len(value) == width and all(scalar(v) for v in value):
        return [tuple(int(v) for v in value)] * n, True
    if not isinstance(value, (list, tuple)) or len(value) != n:
        raise ValueError(f"{what}: {width} integers, or a list of {n} such")
    out = []
    for v in value:
        if v is not None and not (isinstance(v, (list, tuple)) and len(v) == width and all(scalar(e) for e in v)):
            raise ValueError(f"{what}: an entry is {width} integers, not {v!r}")
        out.append(None if v is None else tuple(int(e) for e in v))
    return out, False
