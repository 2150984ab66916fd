"""Picture histograms (hvq_picture_histograms, Context.picture_histograms): what the records mean, and what to read from them.

A record is int32 [3 planes Y, U, V][256].  In HVQ_HIST_VALUES bin v counts the samples of the plane equal to v; in HVQ_HIST_ABSDIFF bin
d counts the positions where |a - b| equals d.  The helpers below are numpy on the host, take integer arrays of shape [..., 256] (one
histogram, a record, a batch of records: `.cpu().numpy()` of the tensor) and work on the last axis; counts are taken as exact integers
(int64), whatever integer type they come in.  of_picture gives the record to expect of a picture the caller has on the host.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

BINS = 256                          # HVQ_HIST_BINS
HIST_VALUES, HIST_ABSDIFF = 0, 1    # HVQ_HIST_VALUES, HVQ_HIST_ABSDIFF
WORKGROUP_UNITS = 1024              # HVQ_HG_CHUNK: 16-byte units of a plane one workgroup of the kernel counts before it flushes its bins

_V = np.arange(BINS, dtype=np.int64)


def _h(h) -> np.ndarray:
    a = np.asarray(h)
    if a.ndim < 1 or a.shape[-1] != BINS:
        raise ValueError(f"histograms have shape [..., {BINS}], not {tuple(a.shape)}")
    if a.dtype.kind not in "iu":
        raise TypeError(f"histograms are integer counts, not {a.dtype}")
    a = a.astype(np.int64)
    if (a < 0).any():
        raise ValueError("a histogram holds a negative count")
    return a


def samples(h) -> np.ndarray:
    """the number of samples counted, int64 [...]: the sum of the bins (the plane's sample count, in both modes)"""
    return _h(h).sum(-1)


def _nonempty(a: np.ndarray) -> np.ndarray:
    n = a.sum(-1)
    if (n == 0).any():
        raise ValueError("an empty histogram has no such statistic")
    return n


def mean(h) -> np.ndarray:
    """mean sample value, float64 [...]"""
    a = _h(h)
    return (a * _V).sum(-1) / _nonempty(a)


def variance(h) -> np.ndarray:
    """population variance of the sample values, float64 [...]: (N sum v^2 h - (sum v h)^2) / N^2, the numerator in exact integers"""
    a = _h(h)
    n = _nonempty(a)
    s1, s2 = (a * _V).sum(-1), (a * _V * _V).sum(-1)
    return (n * s2 - s1 * s1) / (n.astype(np.float64) * n)


def min_max(h):
    """(smallest, largest) value with a non-zero count, int64 [...] each"""
    a = _h(h)
    _nonempty(a)
    nz = a > 0
    return nz.argmax(-1).astype(np.int64), (BINS - 1 - nz[..., ::-1].argmax(-1)).astype(np.int64)


def _at_rank(a: np.ndarray, k: np.ndarray) -> np.ndarray:
    """the k-th smallest sample (k from 1): the smallest v whose cumulative count reaches k"""
    return (a.cumsum(-1) < k[..., None]).sum(-1).astype(np.int64)


def percentile(h, q) -> np.ndarray:
    """the q-th percentile of the samples, int64 [...], 0 <= q <= 100, by an exact integer rank rule: with N samples sorted ascending,
    x_1 <= ... <= x_N, the result is x_k with k = max(1, ceil(q N / 100)) -- the smallest value v such that at least q percent of the
    samples are <= v (the inverse of the empirical distribution function; numpy's method="inverted_cdf").  q N / 100 is evaluated in
    exact rational arithmetic on the value of q as given (an int, a Fraction, or the exact binary value of a float): percentile(h, 0)
    is the minimum, percentile(h, 100) the maximum, and the result is always a value that occurs."""
    a = _h(h)
    n = _nonempty(a)
    f = Fraction(q)
    if not 0 <= f <= 100:
        raise ValueError(f"percentile {q} outside [0, 100]")
    k = np.array([max(1, math.ceil(f * int(v) / 100)) for v in n.reshape(-1)], dtype=np.int64).reshape(n.shape)
    return _at_rank(a, k)


def median(h) -> np.ndarray:
    """the median of the samples, float64 [...]: the middle sample for an odd count, the mean of the two middle samples for an even one
    (numpy.median)"""
    a = _h(h)
    n = _nonempty(a)
    return (_at_rank(a, (n + 1) // 2) + _at_rank(a, n // 2 + 1)) / 2.0


def entropy_bits(h) -> np.ndarray:
    """Shannon entropy of the value distribution in bits per sample, float64 [...], in [0, 8]"""
    a = _h(h)
    p = a / _nonempty(a)[..., None].astype(np.float64)
    return -(p * np.log2(np.where(p > 0, p, 1.0))).sum(-1)


def cdf(h) -> np.ndarray:
    """the empirical distribution function, float64 [..., 256]: cdf[v] = the fraction of samples <= v; cdf[255] == 1"""
    a = _h(h)
    return a.cumsum(-1) / _nonempty(a)[..., None].astype(np.float64)


def equalize_lut(h) -> np.ndarray:
    """the histogram-equalisation table, uint8 [..., 256]: lut[v] = round(255 (C(v) - C_min) / (N - C_min)), 0 for v below the
    smallest occurring value, with C the cumulative counts and C_min the count of that smallest value (the rule of OpenCV's
    equalizeHist); the identity for a plane of a single value.  Rounding is half up, in exact integers."""
    a = _h(h)
    n = _nonempty(a)
    c = a.cumsum(-1)
    lo = min_max(a)[0]
    cmin = np.take_along_axis(c, lo[..., None], -1)
    den = n[..., None] - cmin
    num = np.maximum(c - cmin, 0) * 255
    lut = (2 * num + np.maximum(den, 1)) // (2 * np.maximum(den, 1))
    return np.where(den > 0, lut, _V).astype(np.uint8)


def otsu(h) -> np.ndarray:
    """Otsu's threshold, int64 [...]: the t in [0, 254] that maximises the between-class variance of the classes {v <= t} and {v > t},
    n0 n1 (m0 - m1)^2 / N^2; the smallest such t on a tie; 0 for a plane of a single value.  Compared in exact rational arithmetic."""
    a = _h(h)
    _nonempty(a)
    out = np.zeros(a.shape[:-1], dtype=np.int64)
    flat_out = out.reshape(-1)
    for i, row in enumerate(a.reshape(-1, BINS)):
        n, s = int(row.sum()), int((row * _V).sum())
        n0 = s0 = 0
        best, best_t = Fraction(-1), 0
        for t in range(BINS - 1):
            n0 += int(row[t]); s0 += t * int(row[t])
            n1 = n - n0
            if not n0 or not n1:
                continue
            d = s0 * n1 - (s - s0) * n0                     # n0 n1 (m0 - m1)
            score = Fraction(d * d, n0 * n1)
            if score > best:
                best, best_t = score, t
        flat_out[i] = best_t
    return out


def _pq(h1, h2):
    a, b = _h(h1), _h(h2)
    return a / _nonempty(a)[..., None].astype(np.float64), b / _nonempty(b)[..., None].astype(np.float64)


def intersection(h1, h2) -> np.ndarray:
    """histogram intersection of the two distributions, float64 [...]: sum min(p, q) with p = h1 / N1, q = h2 / N2; 1 for equal
    distributions, 0 for disjoint ones (1 - intersection is half the L1 distance; a scene cut drives it towards 0)"""
    p, q = _pq(h1, h2)
    return np.minimum(p, q).sum(-1)


def chi_square(h1, h2) -> np.ndarray:
    """symmetric chi-square distance of the two distributions, float64 [...]: sum (p - q)^2 / (p + q) over the bins where p + q > 0,
    with p = h1 / N1, q = h2 / N2; 0 for equal distributions, 2 for disjoint ones"""
    p, q = _pq(h1, h2)
    s = p + q
    return ((p - q) ** 2 / np.where(s > 0, s, 1.0)).sum(-1)


def max_abs_diff(h) -> np.ndarray:
    """of HVQ_HIST_ABSDIFF records: the largest |a - b| of the plane, int64 [...]"""
    return min_max(h)[1]


def sad(h) -> np.ndarray:
    """of HVQ_HIST_ABSDIFF records: sum |a - b| = sum d h[d], int64 [...] (picture_metrics' sad; of HVQ_HIST_VALUES records: sum_a)"""
    return (_h(h) * _V).sum(-1)


def sse(h) -> np.ndarray:
    """of HVQ_HIST_ABSDIFF records: sum (a - b)^2 = sum d^2 h[d], int64 [...] (picture_metrics' sse)"""
    return (_h(h) * _V * _V).sum(-1)


def psnr(h, peak: float = 255.0) -> np.ndarray:
    """of HVQ_HIST_ABSDIFF records: PSNR in dB, float64 [...]: 10 log10(peak^2 N / sse); inf where sse == 0"""
    a = _h(h)
    n, e = _nonempty(a).astype(np.float64), sse(a).astype(np.float64)
    with np.errstate(divide="ignore"):
        return np.where(e == 0, np.inf, 10.0 * np.log10(peak * peak * n / np.maximum(e, 1.0)))


def of_picture(yuv, width: int, height: int, h_samp: int = 2, v_samp: int = 2, ref=None) -> np.ndarray:
    """the record to expect of a picture on the host, int64 [3, 256]: `yuv` is its bytes Y | U | V (bytes or a uint8 array);
    `ref` None: the values of its samples, otherwise (a second such buffer) the absolute differences |yuv - ref|"""
    from .checksums import plane_bytes
    a = np.frombuffer(yuv, dtype=np.uint8) if isinstance(yuv, (bytes, bytearray, memoryview)) else np.asarray(yuv)
    sizes = plane_bytes(width, height, h_samp, v_samp)
    if a.dtype != np.uint8 or a.size != sum(sizes):
        raise ValueError(f"{a.size} elements of {a.dtype}, a {width}x{height} picture of sampling ({h_samp}, {v_samp}) has {sum(sizes)} bytes")
    v = a.reshape(-1).astype(np.int64)
    if ref is not None:
        b = np.frombuffer(ref, dtype=np.uint8) if isinstance(ref, (bytes, bytearray, memoryview)) else np.asarray(ref)
        if b.dtype != np.uint8 or b.size != a.size:
            raise ValueError(f"the reference has {b.size} elements of {b.dtype}, the picture has {a.size} bytes")
        v = np.abs(v - b.reshape(-1).astype(np.int64))
    out, at = np.zeros((3, BINS), dtype=np.int64), 0
    for p, n in enumerate(sizes):
        out[p] = np.bincount(v[at:at + n], minlength=BINS)
        at += n
    return out
