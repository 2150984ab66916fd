"""Motion fields (hvq_picture_motion, Context.picture_motion): what to expect from two pictures on the host, and what the records mean.

A field is int32 [rows, cols, 4] = per block (dy, dx, cost, cost_zero): block (r, c) of picture a, B x B luma samples at (B r, B c), looks
most like the reference b at (B r + dy, B c + dx); cost is the sum of absolute differences there, cost_zero the one at (0, 0).  Full
search over |dy|, |dx| <= radius, only displacements whose block lies inside the picture; the smallest (cost, |dy| + |dx|, dy, dx) wins
(include/hvqm4_amd.h is the specification).  Everything here is numpy on the host and takes fields as numpy arrays (tensor.cpu().numpy()).
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

DY, DX, COST, COST_ZERO = 0, 1, 2, 3
BLOCK_SIZES = (8, 16)
MAX_RADIUS = 15                     # HVQ_MOTION_MAX_RADIUS
TILE = 64                           # HVQ_MV_TILE: luma samples of the side of the tile one workgroup searches
MAX_COST = 16 * 16 * 255


def blocks(width: int, height: int, block: int) -> Tuple[int, int]:
    """(rows, cols) of the field of a width x height picture: hvq_motion_blocks' dims.  ValueError for a block other than 8 or 16 and
    for a picture the blocks do not tile."""
    if block not in BLOCK_SIZES:
        raise ValueError(f"block {block}: 8 or 16")
    if width < block or height < block or width % block or height % block:
        raise ValueError(f"blocks of {block} do not tile a {width}x{height} picture")
    return height // block, width // block


def _luma(p, width: int, height: int, h_samp: int, v_samp: int, what: str) -> np.ndarray:
    from .metrics import plane_samples
    v = np.frombuffer(p, dtype=np.uint8) if isinstance(p, (bytes, bytearray, memoryview)) else np.asarray(p)
    if v.dtype != np.uint8:
        raise TypeError(f"{what} has dtype {v.dtype}, not uint8")
    want = sum(plane_samples(width, height, h_samp, v_samp))
    if v.size != want:
        raise ValueError(f"{what} has {v.size} bytes, a {width}x{height} picture sampled ({h_samp}, {v_samp}) has {want}")
    return v.reshape(-1)[:width * height].reshape(height, width)


def of_luma(ya: np.ndarray, yb: np.ndarray, block: int, radius: int) -> np.ndarray:
    """the field of two luma planes uint8 [height, width] -> int32 [rows, cols, 4]"""
    ya, yb = np.asarray(ya), np.asarray(yb)
    if ya.ndim != 2 or ya.shape != yb.shape or ya.dtype != np.uint8 or yb.dtype != np.uint8:
        raise ValueError("two uint8 planes of the same [height, width]")
    if not isinstance(radius, (int, np.integer)) or not 0 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius {radius} outside [0, {MAX_RADIUS}]")
    H, W = ya.shape
    rows, cols = blocks(W, H, block)
    B, R = block, int(radius)
    a, b = ya.astype(np.int32), yb.astype(np.int32)
    best = np.full((rows, cols), np.iinfo(np.int64).max, dtype=np.int64)       # cost << 15 | L1 << 10 | dy + R << 5 | dx + R
    zero = None
    for dy in range(-R, R + 1):
        r0, r1 = max(0, -(dy // B)), min(rows - 1, (H - B - dy) // B)          # the block rows whose displaced block is inside
        if r0 > r1:
            continue
        for dx in range(-R, R + 1):
            c0, c1 = max(0, -(dx // B)), min(cols - 1, (W - B - dx) // B)
            if c0 > c1:
                continue
            ys, xs = slice(r0 * B, (r1 + 1) * B), slice(c0 * B, (c1 + 1) * B)
            d = np.abs(a[ys, xs] - b[r0 * B + dy:(r1 + 1) * B + dy, c0 * B + dx:(c1 + 1) * B + dx])
            cost = d.reshape(r1 - r0 + 1, B, c1 - c0 + 1, B).sum(axis=(1, 3), dtype=np.int64)
            key = cost << 15 | (abs(dy) + abs(dx)) << 10 | (dy + R) << 5 | (dx + R)
            np.minimum(best[r0:r1 + 1, c0:c1 + 1], key, out=best[r0:r1 + 1, c0:c1 + 1])
            if dy == 0 and dx == 0:
                zero = cost
    out = np.empty((rows, cols, 4), dtype=np.int32)
    out[..., DY] = ((best >> 5) & 31) - R
    out[..., DX] = (best & 31) - R
    out[..., COST] = best >> 15
    out[..., COST_ZERO] = zero
    return out


def of_pictures(a, b, width: int, height: int, block: int, radius: int, h_samp: int = 2, v_samp: int = 2) -> np.ndarray:
    """the field hvq_picture_motion gives for picture `a` against reference `b`, both whole pictures (Y | U | V, bytes or uint8 arrays)
    of a width x height stream -> int32 [rows, cols, 4]"""
    return of_luma(_luma(a, width, height, h_samp, v_samp, "a"), _luma(b, width, height, h_samp, v_samp, "b"), block, radius)


def _field(field) -> np.ndarray:
    f = np.asarray(field)
    if f.ndim < 3 or f.shape[-1] != 4:
        raise ValueError(f"fields have shape [..., rows, cols, 4], not {f.shape}")
    if not np.issubdtype(f.dtype, np.integer):
        raise TypeError(f"fields hold integers, not {f.dtype}")
    return f


def magnitude(field) -> Tuple[np.ndarray, np.ndarray]:
    """(L1, Euclidean) length of every block's vector: int64 [..., rows, cols], float64 [..., rows, cols]"""
    f = _field(field).astype(np.int64)
    dy, dx = f[..., DY], f[..., DX]
    return np.abs(dy) + np.abs(dx), np.sqrt((dy * dy + dx * dx).astype(np.float64))


def global_motion(field) -> Tuple[Tuple[int, int], float]:
    """((dy, dx), share): the most frequent vector of ONE field [rows, cols, 4] and the share of the blocks that have it; among equally
    frequent vectors the smallest (|dy| + |dx|, dy, dx) wins -- the tie rule of the search"""
    f = _field(field)
    if f.ndim != 3 or f.shape[0] * f.shape[1] == 0:
        raise ValueError(f"one field [rows, cols, 4] with at least one block, not {f.shape}")
    v, cnt = np.unique(f[..., :2].reshape(-1, 2).astype(np.int64), axis=0, return_counts=True)
    order = sorted(range(len(v)), key=lambda i: (-int(cnt[i]), abs(int(v[i][0])) + abs(int(v[i][1])), int(v[i][0]), int(v[i][1])))
    i = order[0]
    return (int(v[i][0]), int(v[i][1])), float(cnt[i]) / float(f.shape[0] * f.shape[1])


def moving_mask(field, min_gain: int) -> np.ndarray:
    """bool [..., rows, cols]: the blocks the search improved by at least `min_gain`, cost_zero - cost >= min_gain"""
    f = _field(field).astype(np.int64)
    return f[..., COST_ZERO] - f[..., COST] >= min_gain


def compensate(b_luma, field, block: int) -> np.ndarray:
    """the luma predicted from the reference: uint8 [height, width], block (r, c) copied from b_luma at (B r + dy, B c + dx)"""
    f = _field(field)
    b = np.asarray(b_luma)
    if f.ndim != 3 or b.ndim != 2 or b.dtype != np.uint8 or b.shape != (f.shape[0] * block, f.shape[1] * block):
        raise ValueError(f"a field [rows, cols, 4] and a uint8 reference [{block} rows, {block} cols], not {f.shape} and {b.shape}")
    rows, cols = f.shape[:2]
    y = (np.arange(rows * block)[:, None] + np.repeat(f[..., DY].astype(np.int64), block, axis=0).repeat(block, axis=1))
    x = (np.arange(cols * block)[None, :] + np.repeat(f[..., DX].astype(np.int64), block, axis=0).repeat(block, axis=1))
    if y.min() < 0 or x.min() < 0 or y.max() >= b.shape[0] or x.max() >= b.shape[1]:
        raise ValueError("a vector of the field points outside the reference")
    return b[y, x]


def gain(field) -> float:
    """sum of cost_zero / sum of cost over one field or a stack of them: how much the vectors explain; inf when sum of cost is 0"""
    f = _field(field).astype(np.int64)
    c, z = int(f[..., COST].sum()), int(f[..., COST_ZERO].sum())
    return float("inf") if c == 0 else z / c
