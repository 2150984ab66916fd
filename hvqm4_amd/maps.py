"""Lookup tables on pictures in slot layout (hvq_map_pictures / Context.map_pictures, hvq_histogram_tables / Context.histogram_tables,
Context.equalize_pictures): the tables, the rules that make tables of histogram records, and the values to expect.  numpy only.

A picture is its bytes Y | U | V tightly packed; a geometry is (width, height, h_samp, v_samp).  A Table holds one uint8 [256] per plane
and a picture goes through it sample by sample: out = table[plane][in], nothing is rounded (include/hvqm4_amd.h).  The builders are
named for what the picture becomes and give all three planes the same table; luma_only leaves U and V as they are.  A Rule says how the
GPU makes a table of a histogram record (equalize, stretch, otsu; flat and identity need no histogram): luma for Y, chroma for U and V,
each from its own histogram.  tables_of_records gives the tables to expect, built on hvqm4_amd.histograms.
"""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction
from typing import List, Sequence, Union

import numpy as np

TABLE_BYTES = 768                                              # HVQ_MAP_TABLE_BYTES
IDENTITY, FLAT, EQUALIZE, STRETCH, OTSU = 0, 1, 2, 3, 4        # HVQ_TBL_*
MAX_RULES = 64                                                 # HVQ_TBL_MAX_RULES
MAX_CLIP = 499                                                 # per mille, either end of STRETCH
_NAMES = {IDENTITY: "IDENTITY", FLAT: "FLAT", EQUALIZE: "EQUALIZE", STRETCH: "STRETCH", OTSU: "OTSU"}
_ID = bytes(range(256))


def _int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _lut(a) -> bytes:
    """256 table entries as bytes: a uint8 array [256], bytes, or 256 integers in 0 .. 255"""
    if isinstance(a, (bytes, bytearray)):
        b = bytes(a)
    else:
        arr = np.asarray(a)
        if arr.shape != (256,) or arr.dtype.kind not in "iu" or (arr < 0).any() or (arr > 255).any():
            raise ValueError("a table is 256 integers in 0 .. 255")
        b = arr.astype(np.uint8).tobytes()
    if len(b) != 256:
        raise ValueError(f"a table has 256 entries, not {len(b)}")
    return b


# ------------------------------------------------------------------------------------------------------------ tables
@dataclass(frozen=True)
class Table:
    """one table per plane, 256 bytes each.  Hashable; equal when the entries are."""
    y: bytes = _ID
    u: bytes = _ID
    v: bytes = _ID

    def __post_init__(self):
        for p in (self.y, self.u, self.v):
            if not isinstance(p, bytes) or len(p) != 256:
                raise ValueError("a Table holds three bytes objects of 256 entries (from_lut builds one of arrays)")

    def array(self) -> np.ndarray:
        """uint8 [3, 256]: the record of hvq_map_pictures"""
        return np.frombuffer(self.y + self.u + self.v, dtype=np.uint8).reshape(3, 256).copy()

    def luma_only(self) -> "Table":
        return Table(self.y, _ID, _ID)


def from_lut(y, u=None, v=None) -> Table:
    """a Table of arrays: `y` for Y; `u` for U (None: y's); `v` for V (None: u's)"""
    ty = _lut(y)
    tu = ty if u is None else _lut(u)
    return Table(ty, tu, tu if v is None else _lut(v))


def _all(f) -> Table:
    t = bytes(f(i) for i in range(256))
    return Table(t, t, t)


def identity() -> Table:
    return Table()


def invert() -> Table:
    """255 - v"""
    return _all(lambda i: 255 - i)


def flat_table(c: int) -> Table:
    """every sample becomes c"""
    if not _int(c) or not 0 <= c <= 255:
        raise ValueError(f"value {c!r} outside 0 .. 255")
    return _all(lambda i: int(c))


def threshold(t: int) -> Table:
    """255 where v > t, else 0 (t in 0 .. 255; Otsu's convention)"""
    if not _int(t) or not 0 <= t <= 255:
        raise ValueError(f"threshold {t!r} outside 0 .. 255")
    return _all(lambda i: 255 if i > t else 0)


def window(lo: int, hi: int) -> Table:
    """255 where lo <= v <= hi, else 0"""
    if not _int(lo) or not _int(hi) or not 0 <= lo <= hi <= 255:
        raise ValueError(f"window ({lo!r}, {hi!r}): 0 <= lo <= hi <= 255")
    return _all(lambda i: 255 if lo <= i <= hi else 0)


def _round_clip(x: Fraction) -> int:
    return min(255, max(0, (2 * x.numerator + x.denominator) // (2 * x.denominator)))        # half up, exact


def brightness_contrast(brightness=0, contrast=1) -> Table:
    """clip(round((v - 128) contrast + 128 + brightness)), rounded half up in exact rational arithmetic on the values as given"""
    b, c = Fraction(brightness), Fraction(contrast)
    return _all(lambda i: _round_clip((i - 128) * c + 128 + b))


def gamma(g: float) -> Table:
    """round(255 (v / 255) ** g), g > 0 (floating point: a table is built once on the host)"""
    if not g > 0:
        raise ValueError(f"gamma {g!r}: positive")
    return _all(lambda i: min(255, max(0, int(255.0 * (i / 255.0) ** float(g) + 0.5))))


def posterize(levels: int) -> Table:
    """`levels` (2 .. 256) equally wide bands of values, each shown as its band's share of 0 .. 255: (v levels // 256) 255 // (levels - 1)"""
    if not _int(levels) or not 2 <= levels <= 256:
        raise ValueError(f"{levels!r} levels: 2 .. 256")
    return _all(lambda i: (i * levels // 256) * 255 // (levels - 1))


def solarize(t: int = 128) -> Table:
    """v below t stays, from t on 255 - v"""
    if not _int(t) or not 0 <= t <= 256:
        raise ValueError(f"solarize {t!r}: 0 .. 256")
    return _all(lambda i: i if i < t else 255 - i)


def compose(t1: Table, t2: Table) -> Table:
    """first t1, then t2: t2[t1[v]] per plane"""
    return Table(*[bytes(b[a[i]] for i in range(256)) for a, b in ((t1.y, t2.y), (t1.u, t2.u), (t1.v, t2.v))])


def inverse(t: Table) -> Table:
    """the table of the inverse permutation of every plane; ValueError when a plane is no permutation"""
    out = []
    for p in (t.y, t.u, t.v):
        if len(set(p)) != 256:
            raise ValueError("a plane's table is no permutation")
        inv = bytearray(256)
        for i, x in enumerate(p):
            inv[x] = i
        out.append(bytes(inv))
    return Table(*out)


def luma_only(t):
    """the Table or Rule with U and V left as they are"""
    return t.luma_only()


def pack(tables: Sequence[Table]) -> np.ndarray:
    """uint8 [m, 3, 256]: the records of hvq_map_pictures one behind the other"""
    tables = list(tables)
    for t in tables:
        if not isinstance(t, Table):
            raise ValueError(f"an entry is a maps.Table, not {type(t).__name__}")
    return np.stack([t.array() for t in tables]) if tables else np.zeros((0, 3, 256), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------ rules
@dataclass(frozen=True)
class PlaneRule:
    kind: int = IDENTITY
    a: int = 0
    b: int = 0
    pad: int = 0

    def struct(self):
        """the HvqTablePlane of include/hvqm4_amd.h (ctypes)"""
        from ._lib import HvqTablePlane
        check_plane(self)
        return HvqTablePlane(self.kind, self.a, self.b, self.pad)


@dataclass(frozen=True)
class Rule:
    """luma for Y, chroma for U and V (each from its own histogram).  Hashable."""
    luma: PlaneRule
    chroma: PlaneRule

    def struct(self):
        """the HvqTableRule of include/hvqm4_amd.h (ctypes)"""
        from ._lib import HvqTableRule
        check(self)
        return HvqTableRule(self.luma.struct(), self.chroma.struct())

    def luma_only(self) -> "Rule":
        return Rule(self.luma, PlaneRule())


def check_plane(p: PlaneRule) -> None:
    """ValueError for what hvq_table_check refuses in a plane"""
    if not isinstance(p, PlaneRule):
        raise ValueError(f"a plane rule, not {type(p).__name__}")
    if not _int(p.kind) or p.kind not in _NAMES:
        raise ValueError(f"kind {p.kind!r}: IDENTITY, FLAT, EQUALIZE, STRETCH or OTSU")
    if not _int(p.a) or not _int(p.b):
        raise ValueError(f"a, b ({p.a!r}, {p.b!r}): integers")
    if p.pad != 0:
        raise ValueError(f"pad {p.pad!r}: 0")
    if p.kind == FLAT:
        if not 0 <= p.a <= 255 or p.b:
            raise ValueError(f"FLAT with a {p.a}, b {p.b}: a in 0 .. 255, b 0")
    elif p.kind == STRETCH:
        if not 0 <= p.a <= MAX_CLIP or not 0 <= p.b <= MAX_CLIP:
            raise ValueError(f"STRETCH with clips ({p.a}, {p.b}) outside 0 .. {MAX_CLIP} per mille")
    elif p.a or p.b:
        raise ValueError(f"{_NAMES[p.kind]} takes no a, b ({p.a}, {p.b})")


def check(r: Rule) -> None:
    """ValueError for what hvq_table_check refuses"""
    if not isinstance(r, Rule):
        raise ValueError(f"a maps.Rule, not {type(r).__name__}")
    check_plane(r.luma)
    check_plane(r.chroma)


def _rule(kind: int, a: int = 0, b: int = 0) -> Rule:
    p = PlaneRule(kind, a, b)
    check_plane(p)
    return Rule(p, p)


def equalize() -> Rule:
    """histogram equalisation: histograms.equalize_lut"""
    return _rule(EQUALIZE)


def stretch(lo: int = 0, hi: int = 0) -> Rule:
    """automatic levels: the sample at rank lo per mille becomes 0, the one at (1000 - hi) per mille 255, linear between (0 .. 499 each)"""
    return _rule(STRETCH, lo, hi)


def otsu() -> Rule:
    """binarise at Otsu's threshold: 255 where v > histograms.otsu, else 0"""
    return _rule(OTSU)


def flat(c: int) -> Rule:
    """every sample becomes c, whatever the histogram"""
    return _rule(FLAT, c)


def keep() -> Rule:
    """the identity, whatever the histogram"""
    return _rule(IDENTITY)


# ------------------------------------------------------------------------------------------------------------ the values to expect
def of_picture(yuv, geom, table: Table, planes: int = 7) -> np.ndarray:
    """the bytes hvq_map_pictures gives for a picture on the host, uint8 [bytes]: `yuv` its bytes Y | U | V, `planes` the mask of the
    planes that are looked up (the others are copied)"""
    from .checksums import plane_bytes
    if not isinstance(table, Table):
        raise ValueError(f"a maps.Table, not {type(table).__name__}")
    if not _int(planes) or not 1 <= planes <= 7:
        raise ValueError(f"planes {planes!r}: a mask of the bits 0 .. 2, not 0")
    a = np.frombuffer(yuv, dtype=np.uint8) if isinstance(yuv, (bytes, bytearray, memoryview)) else np.asarray(yuv)
    sizes = plane_bytes(*geom)
    if a.dtype != np.uint8 or a.size != sum(sizes):
        raise ValueError(f"{a.size} elements of {a.dtype}, a picture of geometry {tuple(geom)} has {sum(sizes)} bytes")
    a = a.reshape(-1)
    out, at, t = np.empty_like(a), 0, table.array()
    for p, n in enumerate(sizes):
        out[at:at + n] = t[p][a[at:at + n]] if planes >> p & 1 else a[at:at + n]
        at += n
    return out


def _plane_table(h: np.ndarray, r: PlaneRule) -> np.ndarray:
    from . import histograms as H
    ident = np.arange(256, dtype=np.uint8)
    if r.kind == IDENTITY:
        return ident
    if r.kind == FLAT:
        return np.full(256, r.a, dtype=np.uint8)
    if int(h.sum()) == 0:                                       # the device cannot raise what histograms raises
        return ident
    if r.kind == EQUALIZE:
        return H.equalize_lut(h)
    if r.kind == OTSU:
        t = int(H.otsu(h))
        return np.where(np.arange(256) > t, 255, 0).astype(np.uint8)
    lo, hi = int(H.percentile(h, Fraction(r.a, 10))), int(H.percentile(h, Fraction(1000 - r.b, 10)))
    if hi <= lo:
        return ident
    v = np.arange(256, dtype=np.int64)
    mid = (2 * 255 * (v - lo) + (hi - lo)) // (2 * (hi - lo))
    return np.where(v <= lo, 0, np.where(v >= hi, 255, mid)).astype(np.uint8)


def tables_of_records(hist, rules: Union[Rule, Sequence[Rule]]) -> np.ndarray:
    """the tables hvq_histogram_tables makes of HVQ_HIST_VALUES records, uint8 [n, 3, 256]: `hist` integer [n, 3, 256] (or one record
    [3, 256] -> [3, 256]), `rules` one Rule or one per record.  Built on histograms.equalize_lut, otsu and percentile; an empty
    histogram gives the identity."""
    h = np.asarray(hist)
    one = h.ndim == 2
    if one:
        h = h[None]
    if h.ndim != 3 or h.shape[1:] != (3, 256) or h.dtype.kind not in "iu":
        raise ValueError(f"records have shape [n, 3, 256] of integers, not {tuple(h.shape)} of {h.dtype}")
    h = h.astype(np.int64)
    rs: List[Rule] = [rules] * len(h) if isinstance(rules, Rule) else list(rules)
    if len(rs) != len(h):
        raise ValueError(f"{len(rs)} rules for {len(h)} records")
    out = np.empty((len(h), 3, 256), dtype=np.uint8)
    for i, r in enumerate(rs):
        check(r)
        for p in range(3):
            out[i, p] = _plane_table(h[i, p], r.chroma if p else r.luma)
    return out[0] if one else out
