"""Connected components of pictures in slot layout (hvq_label_pictures / Context.label_pictures, hvq_select_components /
Context.select_components): the rules, the values to expect, and the helpers around the records.  numpy only.

A rule names a plane (0 Y, 1 U, 2 V), a window lo <= a <= hi of the samples that are foreground, and the neighbourhood, 4 or 8.
include/hvqm4_amd.h specifies the result: components are numbered 1 .. K in ascending order of their first samples in raster order; the
label map is uint32 [Ny][Nx]; the record table is [cap + 1][8], row 0 {K, stored, F, status, 0, 0, 0, 0}, row k {area, x0, y0, x1, y1,
first, sum_x, sum_y}.  of_plane computes both on the host with an algorithm of its own -- runs of rows, a union-find over the runs, two
passes --, which shares nothing with the kernels' tiles.  A geometry is (width, height, h_samp, v_samp).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

MAX_RULES = 64                         # HVQ_LBL_MAX_RULES
MAX_CAP = 1 << 20                      # HVQ_LBL_MAX_CAP
INCOMPLETE = 1                         # HVQ_LBL_INCOMPLETE
MAX_SELECTS = 64                       # HVQ_SEL_MAX
FIELDS = ("area", "x0", "y0", "x1", "y1", "first", "sum_x", "sum_y")
_U32 = 0xFFFFFFFF


def _int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


@dataclass(frozen=True)
class Rule:
    """the foreground of one plane and its neighbourhood.  Hashable."""
    plane: int = 0
    lo: int = 255
    hi: int = 255
    connectivity: int = 8

    def struct(self):
        """the HvqLabelRule of include/hvqm4_amd.h (ctypes)"""
        from ._lib import HvqLabelRule
        check(self)
        return HvqLabelRule(self.plane, self.lo, self.hi, self.connectivity)


def rule(plane: int = 0, lo: int = 255, hi: int = 255, connectivity: int = 8) -> Rule:
    """the samples lo .. hi of `plane` under the 4- or 8-neighbourhood; the default reads an Otsu mask of Y"""
    r = Rule(plane, lo, hi, connectivity)
    check(r)
    return r


def check(r: Rule) -> None:
    """ValueError for what hvq_label_check refuses"""
    if not isinstance(r, Rule):
        raise ValueError(f"a labels.Rule, not {type(r).__name__}")
    if not _int(r.plane) or not 0 <= r.plane <= 2:
        raise ValueError(f"plane {r.plane!r}: 0 Y, 1 U, 2 V")
    if not _int(r.lo) or not _int(r.hi) or not 0 <= r.lo <= r.hi <= 255:
        raise ValueError(f"window {r.lo!r} .. {r.hi!r}: 0 <= lo <= hi <= 255")
    if not _int(r.connectivity) or r.connectivity not in (4, 8):
        raise ValueError(f"connectivity {r.connectivity!r}: 4 or 8")


def plane_shape(geom, plane: int) -> Tuple[int, int]:
    """(Ny, Nx) of a plane of a picture of geometry `geom`"""
    w, h, hs, vs = geom
    return (h >> (vs == 2), w >> (hs == 2)) if plane else (h, w)


def label_bytes(geom, plane: int = 0) -> int:
    """hvq_label_bytes: the bytes of the label map of that plane"""
    ny, nx = plane_shape(geom, plane)
    return 4 * nx * ny


def plane_of(yuv, geom, plane: int) -> np.ndarray:
    """plane `plane` of a picture Y | U | V as uint8 [Ny][Nx]"""
    a = np.frombuffer(yuv, dtype=np.uint8) if isinstance(yuv, (bytes, bytearray, memoryview)) else np.asarray(yuv, dtype=np.uint8).reshape(-1)
    w, h, _hs, _vs = geom
    ny, nx = plane_shape(geom, plane)
    cy, cx = plane_shape(geom, 1)
    if a.size != w * h + 2 * cx * cy:
        raise ValueError(f"{a.size} bytes, a picture of geometry {tuple(geom)} has {w * h + 2 * cx * cy}")
    off = 0 if plane == 0 else w * h + (plane - 1) * cx * cy
    return a[off:off + nx * ny].reshape(ny, nx)


# ------------------------------------------------------------------------------------------------------------ the values
def of_plane(a, r: Optional[Rule] = None, cap: Optional[int] = None):
    """the label map and the records of a plane uint8 [Ny][Nx] -> (uint32 [Ny][Nx], int64 [stored + 1][8]); cap None: every record.
    Runs of foreground per row, a union-find over the runs that links the later root to the earlier one, numbers in the order of the
    roots, then the runs' labels and sums."""
    r = Rule() if r is None else r
    check(r)
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError("a plane is a uint8 array [Ny][Nx]")
    if cap is not None and (not _int(cap) or not 0 <= cap <= MAX_CAP):
        raise ValueError(f"cap {cap!r} outside 0 .. {MAX_CAP}")
    ny, nx = a.shape
    fg = (a >= r.lo) & (a <= r.hi)
    edge = np.diff(np.pad(fg.astype(np.int8), ((0, 0), (1, 1))), axis=1)              # [Ny][Nx + 1]: +1 where a run starts, -1 behind its end
    ys, xs = np.nonzero(edge == 1)
    _ye, xe = np.nonzero(edge == -1)                                                  # run j: row ys[j], columns xs[j] .. xe[j] - 1, in raster order
    runs = int(xs.size)
    parent = list(range(runs))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    row_at = np.searchsorted(ys, np.arange(ny + 1)).tolist()
    reach = 1 if r.connectivity == 8 else 0
    s, e = xs.tolist(), xe.tolist()
    for y in range(1, ny):
        i, i1, j, j1 = row_at[y - 1], row_at[y], row_at[y], row_at[y + 1]
        while i < i1 and j < j1:
            if s[i] < e[j] + reach and s[j] < e[i] + reach:
                ri, rj = find(i), find(j)
                if ri != rj:
                    parent[max(ri, rj)] = min(ri, rj)
            if e[i] < e[j]:
                i += 1
            else:
                j += 1
    root = np.array([find(i) for i in range(runs)], dtype=np.int64)
    is_root = root == np.arange(runs)
    number = np.cumsum(is_root)                                                        # of a root: its rank among the roots, from 1
    lab = number[root] if runs else np.zeros(0, dtype=np.int64)
    K = int(is_root.sum())
    flat = np.zeros(ny * nx + 1, dtype=np.int64)
    np.add.at(flat, ys * nx + xs, lab)
    np.add.at(flat, ys * nx + xe, -lab)
    labels = np.cumsum(flat[:-1]).astype(np.uint32).reshape(ny, nx)
    length = (xe - xs).astype(np.int64)
    rec = np.zeros((K + 1, 8), dtype=np.int64)
    rec[1:, 1] = rec[1:, 2] = np.iinfo(np.int64).max
    np.add.at(rec[:, 0], lab, length)
    np.minimum.at(rec[:, 1], lab, xs)
    np.minimum.at(rec[:, 2], lab, ys)
    np.maximum.at(rec[:, 3], lab, xe - 1)
    np.maximum.at(rec[:, 4], lab, ys)
    rec[lab[is_root], 5] = (ys * nx + xs)[is_root]
    np.add.at(rec[:, 6], lab, (xs + xe - 1) * length // 2)
    np.add.at(rec[:, 7], lab, ys * length)
    stored = K if cap is None else min(K, cap)
    rec[0] = (K, stored, int(fg.sum()), 0, 0, 0, 0, 0)
    return labels, rec[:stored + 1].copy()


def of_picture(yuv, geom, r: Optional[Rule] = None, cap: Optional[int] = None):
    """of_plane on the rule's plane of a picture Y | U | V of geometry `geom`"""
    r = Rule() if r is None else r
    check(r)
    return of_plane(plane_of(yuv, geom, r.plane), r, cap)


# ------------------------------------------------------------------------------------------------------------ the records
@dataclass(frozen=True)
class Records:
    """a record table taken apart: K components, `stored` of them with a row, F foreground samples, the status, and rows int64 [stored][8]
    (FIELDS); rows[k - 1] belongs to label k"""
    K: int
    stored: int
    F: int
    status: int
    rows: np.ndarray

    def __getitem__(self, name: str) -> np.ndarray:
        return self.rows[:, FIELDS.index(name)]


def records(comps) -> Records:
    """a view of one picture's record table, [cap + 1][8] (a numpy array, or a tensor on the host)"""
    c = np.asarray(comps).astype(np.int64, copy=False)
    if c.ndim != 2 or c.shape[1] != 8 or c.shape[0] < 1:
        raise ValueError("a record table is an array [cap + 1][8]")
    K, stored, F, status = (int(v) for v in c[0, :4])
    if not 0 <= stored <= min(K, c.shape[0] - 1):
        raise ValueError(f"row 0 says {stored} of {K} records are stored, the table has room for {c.shape[0] - 1}")
    return Records(K, stored, F, status, c[1:stored + 1])


def centroids(rec: Records) -> np.ndarray:
    """float64 [stored][2]: (x, y) of every stored component"""
    return np.stack([rec["sum_x"] / rec["area"], rec["sum_y"] / rec["area"]], axis=1) if rec.stored else np.zeros((0, 2))


def boxes(rec: Records) -> np.ndarray:
    """int64 [stored][4]: (x0, y0, x1, y1), inclusive"""
    return rec.rows[:, 1:5]


def largest(rec: Records, n: int = 1) -> np.ndarray:
    """the labels of the n largest stored components, the largest first, the smaller label first among equals"""
    order = np.lexsort((np.arange(rec.stored), -rec["area"]))
    return order[:n] + 1


@dataclass(frozen=True)
class Select:
    """inclusive ranges of a record's area and of its box's width and height.  Hashable."""
    area_min: int = 0
    area_max: int = _U32
    w_min: int = 0
    w_max: int = _U32
    h_min: int = 0
    h_max: int = _U32
    invert: int = 0
    pad: int = 0

    def struct(self):
        """the HvqSelect of include/hvqm4_amd.h (ctypes)"""
        from ._lib import HvqSelect
        check_select(self)
        return HvqSelect(self.area_min, self.area_max, self.w_min, self.w_max, self.h_min, self.h_max, self.invert, self.pad)


def check_select(s: Select) -> None:
    """ValueError for what hvq_select_components refuses in an entry"""
    if not isinstance(s, Select):
        raise ValueError(f"a labels.Select, not {type(s).__name__}")
    for lo, hi, what in ((s.area_min, s.area_max, "area"), (s.w_min, s.w_max, "width"), (s.h_min, s.h_max, "height")):
        if not _int(lo) or not _int(hi) or not 0 <= lo <= hi <= _U32:
            raise ValueError(f"{what} {lo!r} .. {hi!r}: 0 <= min <= max < 2^32")
    if s.invert not in (0, 1) or isinstance(s.invert, bool):
        raise ValueError(f"invert {s.invert!r}: 0 or 1")
    if s.pad != 0:
        raise ValueError(f"pad {s.pad!r}: 0")


def _range(v, what):
    if v is None:
        return 0, _U32
    if _int(v):
        return int(v), _U32
    if isinstance(v, (tuple, list)) and len(v) == 2:
        return (0 if v[0] is None else v[0]), (_U32 if v[1] is None else v[1])
    raise ValueError(f"{what} {v!r}: a minimum, or (min, max) with None for an open end")


def select(area=None, width=None, height=None, invert: bool = False) -> Select:
    """the components whose area, box width and box height lie in their ranges: each a minimum, or (min, max), None for open.
    select(area=50) is area opening: the specks below 50 samples go"""
    s = Select(*_range(area, "area"), *_range(width, "width"), *_range(height, "height"), int(bool(invert)))
    check_select(s)
    return s


def of_select(labels, comps, sel: Select, geom) -> np.ndarray:
    """the bytes hvq_select_components writes for one picture: `labels` uint32 [h][w] of its Y plane, `comps` its record table"""
    check_select(sel)
    w, h, _hs, _vs = geom
    lab = np.asarray(labels).astype(np.int64).reshape(h, w)
    rec = records(comps)
    keep = np.zeros(max(int(lab.max(initial=0)), rec.stored) + 1, dtype=bool)
    if rec.stored:
        bw, bh = rec["x1"] - rec["x0"] + 1, rec["y1"] - rec["y0"] + 1
        keep[1:rec.stored + 1] = ((rec["area"] >= sel.area_min) & (rec["area"] <= sel.area_max) & (bw >= sel.w_min) & (bw <= sel.w_max)
                                  & (bh >= sel.h_min) & (bh <= sel.h_max))
    y = np.where(keep[lab] ^ bool(sel.invert), 255, 0).astype(np.uint8)
    cy, cx = plane_shape(geom, 1)
    return np.concatenate([y.reshape(-1), np.full(2 * cx * cy, 128, dtype=np.uint8)])
