"""Perceptual hashes of pictures and nearest-hash search (hvq_picture_hashes / Context.picture_hashes, hvq_hash_nearest /
Context.hash_nearest): what the records mean, and the values to expect.  numpy only.

A hash record is uint64 [4] = (ahash, dhash, phash, sum_y) of the luma plane, specified as exact integers in include/hvqm4_amd.h:
area grids with rational cell edges (nothing is rounded), aHash on 8 x 8 against the mean, dHash on 8 rows x 9 columns, pHash the
signs of the 8 x 8 low-frequency corner of an integer 32 x 32 DCT-II against their median.  A hash is 64 bits row-major, element
(r, c) is bit 63 - (8 r + c).  The device's tensors hold the bit patterns as int64; as_int64 / as_uint64 convert.

A nearest record is int32 [4] = (nearest, distance, within, first_within) per query hash (hvq_hash_nearest).
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

AHASH, DHASH, PHASH, SUM_Y = range(4)
NAMES = ("ahash", "dhash", "phash", "sum_y")
NEAREST, DISTANCE, WITHIN, FIRST_WITHIN = range(4)
NEAREST_NAMES = ("nearest", "distance", "within", "first_within")
NEAREST_TILE = 1024              # HVQ_HN_TILE of hvq_desc.h: database hashes a workgroup of hvq_hash_nearest stages at a time
NEAREST_MAX = 1 << 24            # most queries, and most database hashes, of one call
EMPTY = (-1, 65, 0, -1)          # the record of a query without a candidate

# C[k][n] = floor(4096 cos((2 n + 1) k pi / 64) + 0.5), rows k = 1 .. 7, n = 0 .. 15: committed constants (include/hvqm4_amd.h).
# C[0][n] = 4096, and C[k][31 - n] = (-1)^k C[k][n].
_HALF = (
    (4091, 4052, 3973, 3857, 3703, 3513, 3290, 3035, 2751, 2440, 2106, 1751, 1380, 995, 601, 201),
    (4076, 3920, 3612, 3166, 2598, 1931, 1189, 401, -401, -1189, -1931, -2598, -3166, -3612, -3920, -4076),
    (4052, 3703, 3035, 2106, 995, -201, -1380, -2440, -3290, -3857, -4091, -3973, -3513, -2751, -1751, -601),
    (4017, 3406, 2276, 799, -799, -2276, -3406, -4017, -4017, -3406, -2276, -799, 799, 2276, 3406, 4017),
    (3973, 3035, 1380, -601, -2440, -3703, -4091, -3513, -2106, -201, 1751, 3290, 4052, 3857, 2751, 995),
    (3920, 2598, 401, -1931, -3612, -4076, -3166, -1189, 1189, 3166, 4076, 3612, 1931, -401, -2598, -3920),
    (3857, 2106, -601, -3035, -4091, -3290, -995, 1751, 3703, 3973, 2440, -201, -2751, -4052, -3513, -1380),
)
TABLE = np.array([[4096] * 32] + [list(h) + [(-1) ** (k + 1) * v for v in h[::-1]] for k, h in enumerate(_HALF)], dtype=np.int64)
TABLE.setflags(write=False)


def weights(g: int, n: int) -> np.ndarray:
    """int64 [g, n]: w[r, y] = max(0, min(g y + g, n r + n) - max(g y, n r)), the share (in units of 1 / g of a sample) of sample
    y in cell r when n samples are divided into g equal cells.  Every row sums to n, every column to g."""
    y = np.arange(n, dtype=np.int64)[None, :]
    r = np.arange(g, dtype=np.int64)[:, None]
    return np.maximum(0, np.minimum(g * y + g, n * r + n) - np.maximum(g * y, n * r))


def grid(plane, gy: int, gx: int) -> np.ndarray:
    """the cell sums S[r][c] = sum wy(r, y) wx(c, x) a[y][x] of a plane (2-D uint8) on a grid of gy rows x gx columns -> int64
    [gy, gx].  Every cell has total weight W H."""
    a = np.asarray(plane)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError("a plane is a 2-D uint8 array")
    h, w = a.shape
    # products of integers in float64 (BLAS): every partial sum is an integer of at most 255 w h, exact below 2^53
    if 255 * w * h >= 1 << 53:
        return weights(gy, h) @ a.astype(np.int64) @ weights(gx, w).T
    s = weights(gy, h).astype(np.float64) @ a.astype(np.float64) @ weights(gx, w).T.astype(np.float64)
    return np.rint(s).astype(np.int64)


def dct_corner(m) -> np.ndarray:
    """F[k][l] = sum C[k][r] C[l][c] m[r][c] for 0 <= k, l < 8 of a 32 x 32 integer array, exact -> object array of Python integers
    (|F| < 2^46 for the means of a picture; an int64 would do there, the object array holds whatever it is given)"""
    m = np.asarray(m).astype(object)
    t = TABLE.astype(object)
    return t.dot(m).dot(t.T)


def _bits(b) -> int:
    v = 0
    for x in np.asarray(b).reshape(64):
        v = v << 1 | int(bool(x))
    return v


def of_plane(plane) -> List[int]:
    """[ahash, dhash, phash, sum_y] of a luma plane (2-D uint8, any size), as unsigned Python integers"""
    a = np.asarray(plane)
    h, w = a.shape
    s32 = grid(a, 32, 32)
    s8 = grid(a, 8, 8)
    d = grid(a, 8, 9)
    t = int(s8.sum())
    ahash = _bits(64 * s8 > t)
    dhash = _bits(d[:, 1:] > d[:, :-1])
    m = (16 * s32 + (w * h >> 1)) // (w * h)
    f = dct_corner(m).reshape(64)
    srt = sorted(int(v) for v in f)
    mid = srt[31] + srt[32]
    phash = _bits([2 * int(v) > mid for v in f])
    return [ahash, dhash, phash, t // 64]


def of_picture(picture, width: int, height: int, h_samp: int = 2, v_samp: int = 2) -> List[int]:
    """the record of a picture on the host: `picture` is its bytes Y | U | V (bytes, bytearray, memoryview or a uint8 numpy array) as
    read_picture returns them.  Only the luma plane enters; the sampling says how long the picture is."""
    from .checksums import plane_bytes
    buf = np.frombuffer(bytes(picture), dtype=np.uint8) if isinstance(picture, (bytes, bytearray, memoryview)) else np.asarray(picture)
    if buf.dtype != np.uint8:
        raise TypeError(f"a picture is uint8, not {buf.dtype}")
    sizes = plane_bytes(width, height, h_samp, v_samp)
    buf = buf.reshape(-1)
    if buf.size != sum(sizes):
        raise ValueError(f"{buf.size} bytes, a {width}x{height} picture of sampling ({h_samp}, {v_samp}) has {sum(sizes)}")
    return of_plane(buf[:sizes[0]].reshape(height, width))


def _u64(values) -> np.ndarray:
    a = values if isinstance(values, np.ndarray) else np.array(values, dtype=object)
    if a.dtype == object:
        return np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in a.reshape(-1)], dtype=np.uint64).reshape(a.shape)
    if a.dtype == np.uint64:
        return a
    return np.ascontiguousarray(a.astype(np.int64)).view(np.uint64)


def as_uint64(values) -> np.ndarray:
    """hashes as a uint64 numpy array: from unsigned Python integers, or from the int64 bit patterns a device tensor holds"""
    return _u64(values)


def as_int64(values) -> np.ndarray:
    """hashes as the int64 bit patterns a device tensor holds (numpy int64 array of the same shape)"""
    return np.ascontiguousarray(_u64(values)).view(np.int64)


def hamming(a, b):
    """popcount(a ^ b) of two hashes, or elementwise of two broadcastable arrays of hashes (unsigned values or int64 bit patterns)"""
    x = np.bitwise_xor(_u64(a), _u64(b))
    scalar = x.ndim == 0
    x = np.atleast_1d(x)
    d = np.unpackbits(np.ascontiguousarray(x).view(np.uint8).reshape(x.shape + (8,)), axis=-1).sum(axis=-1).astype(np.int32)
    return int(d[0]) if scalar else d


def hexes(record) -> List[str]:
    """the three hashes of a record as 16 hex digits each: read left to right, top to bottom"""
    return [f"{int(v) & 0xFFFFFFFFFFFFFFFF:016x}" for v in list(record)[:3]]


def nearest(q, db=None, self_offset: int = -1, threshold: int = 10) -> np.ndarray:
    """hvq_hash_nearest on the host -> int32 [nq, 4] = (nearest, distance, within, first_within).  The candidates of query i are
    all of db when self_offset < 0, otherwise those with j < self_offset + i.  db None: the queries themselves with self_offset 0
    (de-duplication in place).  nearest is the candidate with the smallest (distance, j); within counts the candidates with
    distance <= threshold, first_within is the smallest such j or -1; no candidate: (-1, 65, 0, -1)."""
    if db is None:
        db, self_offset = q, 0
    if not 0 <= threshold <= 64:
        raise ValueError(f"threshold {threshold} outside [0, 64]")
    qa, da = _u64(q).reshape(-1), _u64(db).reshape(-1)
    out = np.empty((qa.size, 4), dtype=np.int32)
    for i in range(qa.size):
        lim = da.size if self_offset < 0 else max(0, min(da.size, self_offset + i))
        if lim == 0:
            out[i] = EMPTY
            continue
        d = hamming(da[:lim], qa[i])
        j = int(np.argmin(d))                        # the first of equal distances
        ok = np.flatnonzero(d <= threshold)
        out[i] = (j, int(d[j]), ok.size, int(ok[0]) if ok.size else -1)
    return out


def duplicates(hashes, threshold: int = 10) -> List[int]:
    """for each picture of a sequence the first EARLIER one whose hash lies within `threshold` bits, or -1: a picture with an entry
    other than -1 is a near-duplicate to drop"""
    return nearest(hashes, None, 0, threshold)[:, FIRST_WITHIN].tolist()


def hash_views(queries, database=None, self_offset: int = -1):
    """what Context.hash_nearest hands to the library: ((q pointer, nq, q stride), (db pointer, ndb, db stride), self_offset).  A set
    of hashes is an int64 tensor [n], or [n, k] of which column 0 counts; the stride (in 64-bit words, at least 1) is the tensor's
    own, so records[:, PHASH] walks a column of picture_hashes' records.  database None: the queries themselves with self_offset 0.
    Raises TypeError / ValueError; the device is checked last, so the layout checks run on CPU tensors too."""
    import torch

    def view(t, what):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what} must be an int64 tensor, not {type(t).__name__}")
        if t.dtype != torch.int64:
            raise TypeError(f"{what} has dtype {t.dtype}, not torch.int64")
        if t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[1] < 1):
            raise ValueError(f"{what} must have shape [n] or [n, k], not {tuple(t.shape)}")
        n = int(t.shape[0])
        if n > NEAREST_MAX:
            raise ValueError(f"{what}: {n} hashes, one call takes {NEAREST_MAX} at the most")
        stride = int(t.stride(0)) if n > 1 else 1
        if stride < 1:
            raise ValueError(f"{what}: stride {stride} (hashes must lie at increasing addresses, at least one word apart)")
        if t.device.type != "cuda":
            raise ValueError(f"{what} is on {t.device}, not a GPU")
        return t.data_ptr(), n, stride

    if database is None:
        if self_offset not in (-1, 0):
            raise ValueError("database None means the queries themselves with self_offset 0")
        qv = view(queries, "queries")
        return qv, qv, 0
    return view(queries, "queries"), view(database, "database"), int(self_offset)


def dedup_lines(ordinals: Sequence[int], frame_types: Sequence, records, dup: Sequence[int]) -> List[str]:
    """one line per picture: ordinal, frame type, the three hashes in hex, and the earlier picture it duplicates or '-'
    (tools/dedup.py)"""
    lines = []
    for k, t, rec, d in zip(ordinals, frame_types, records, dup):
        lines.append(f"{k:6d} {t} " + " ".join(hexes(rec)) + (f" {d:6d}" if d >= 0 else "      -"))
    return lines


DEDUP_HEADER = "# ordinal type ahash dhash phash duplicate_of"
