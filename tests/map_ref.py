"""The values of hvq_map_pictures and hvq_histogram_tables as include/hvqm4_amd.h states them, restated in plain Python: loops over
samples and bins, fractions.Fraction where the text divides (the percentile ranks, Otsu's scores).  No numpy arithmetic in the values.
Slow on purpose: it is what hvqm4_amd.maps, the fake device and the GPU are compared with."""
from fractions import Fraction
from math import ceil

IDENTITY, FLAT, EQUALIZE, STRETCH, OTSU = range(5)


def plane_sizes(geom):
    w, h, hs, vs = geom
    cw, ch = w >> (hs == 2), h >> (vs == 2)
    return [(w, h), (cw, ch), (cw, ch)]


def map_picture(yuv: bytes, geom, tables, planes: int = 7) -> bytes:
    """tables: three sequences of 256 entries (Y, U, V); a plane whose bit of `planes` is clear is copied"""
    out, at = bytearray(), 0
    for p, (pw, ph) in enumerate(plane_sizes(geom)):
        for a in yuv[at:at + pw * ph]:
            out.append(tables[p][a] if planes >> p & 1 else a)
        at += pw * ph
    assert at == len(yuv)
    return bytes(out)


def _kth(h, k):
    """x_k, k from 1: the smallest v with C(v) >= k"""
    c = 0
    for v in range(256):
        c += h[v]
        if c >= k:
            return v
    raise AssertionError("rank beyond the samples")


def otsu_threshold(h):
    n, s = sum(h), sum(v * h[v] for v in range(256))
    best, best_t = None, 0
    n0 = s0 = 0
    for t in range(255):
        n0 += h[t]                                  # the samples v <= t, and their sum
        s0 += t * h[t]
        n1, s1 = n - n0, s - s0                     # the samples v > t
        if n0 == 0 or n1 == 0:
            continue
        d = s0 * n1 - s1 * n0
        score = Fraction(d * d, n0 * n1)
        if best is None or score > best:            # the smallest t on a tie
            best, best_t = score, t
    return best_t


def table(h, kind, a=0, b=0):
    """the 256 entries of a plane whose bins are h (a list of 256 counts)"""
    h = [int(x) for x in h]
    assert len(h) == 256 and min(h) >= 0
    ident = list(range(256))
    if kind == IDENTITY:
        return ident
    if kind == FLAT:
        return [a] * 256
    n = sum(h)
    if n == 0:
        return ident
    if kind == EQUALIZE:
        cmin = next(x for x in h if x)
        d = n - cmin
        if d == 0:
            return ident
        out, c = [], 0
        for v in range(256):
            c += h[v]
            out.append((2 * 255 * max(c - cmin, 0) + d) // (2 * d))
        return out
    if kind == STRETCH:
        lo = _kth(h, max(1, ceil(Fraction(a * n, 1000))))
        hi = _kth(h, max(1, ceil(Fraction((1000 - b) * n, 1000))))
        if hi <= lo:
            return ident
        return [0 if v <= lo else 255 if v >= hi else (2 * 255 * (v - lo) + (hi - lo)) // (2 * (hi - lo)) for v in range(256)]
    assert kind == OTSU
    t = otsu_threshold(h)
    return [255 if v > t else 0 for v in range(256)]


def record_tables(rec, luma, chroma):
    """rec: three lists of 256 counts; luma, chroma: (kind, a, b) -> three lists of 256 entries"""
    return [table(rec[p], *(chroma if p else luma)) for p in range(3)]
