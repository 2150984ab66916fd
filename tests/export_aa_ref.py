"""Helper (not a test): numpy restatement of the antialiased float export (include/hvqm4_amd.h, hvq_export_resampled with
HVQ_FILTER_TRIANGLE) on top of export_reference(..., "rgbp") of tests/test_export_cpu.py.  The tables are float64 with one rounding
per operation and one rounding to float32 at the end; the pixel sums are float32, one rounding per operation -- numpy fuses
nothing -- in the order of the specification, and every intermediate is asserted to be float32."""
import numpy as np

from tests.export_float_ref import bits_of, to_dtype  # noqa: F401  (re-exported: the tests take them from here)
from tests.test_export_cpu import export_reference

F32 = np.float32


def _f32(*arrays):
    for a in arrays:
        assert a.dtype == np.float32, a.dtype


def table(n_src: int, n_out: int):
    """(first, count, weights) of one axis as hvq_resample_table returns them: int32 [n_out], int32 [n_out], float32 CSR"""
    j = np.arange(n_out, dtype=np.float64)
    scale = np.float64(n_src) / np.float64(n_out)
    support = max(scale, np.float64(1.0))
    c = scale * (j + 0.5)
    first = np.maximum(np.trunc(c - support + 0.5).astype(np.int64), 0)
    end = np.minimum(np.trunc(c + support + 0.5).astype(np.int64), n_src)
    count = end - first
    assert (count >= 1).all()
    k = np.arange(int(count.max()), dtype=np.int64)[None, :]
    live = k < count[:, None]
    u = np.maximum(0.0, 1.0 - np.abs(((k + first[:, None]).astype(np.float64) - c[:, None] + 0.5) / support))
    u = np.where(live, u, 0.0)                                      # + 0.0 changes no bit of a sum of terms >= 0
    t = u[:, 0].copy()
    for col in range(1, u.shape[1]):                                # left to right: np.sum adds pairwise
        t = t + u[:, col]
    assert u.dtype == np.float64 and t.dtype == np.float64
    w = (u / t[:, None]).astype(np.float32)
    return first.astype(np.int32), count.astype(np.int32), w[live]


def _padded(n_src: int, n_out: int):
    """the table as (index [n_out, K], weight [n_out, K]) with zero weights past each count, the index kept inside the axis"""
    first, count, w = table(n_src, n_out)
    K = int(count.max())
    k = np.arange(K)[None, :]
    live = k < count[:, None]
    wp = np.zeros((n_out, K), dtype=np.float32)
    wp[live] = w
    idx = np.minimum(first[:, None].astype(np.int64) + k, n_src - 1)
    return idx, wp


def resize_planes_aa(p: np.ndarray, out_hw) -> np.ndarray:
    """float32 planes [3, ch, cw] -> [3, H, W]: h = P * w0, then h = h + P * wk along x; then the same along y.  A padded tap has
    weight +0 and every product is >= +0, so it changes no bit."""
    H, W = out_hw
    _f32(p)
    ch, cw = p.shape[1:]
    xi, xw = _padded(cw, W)
    yi, yw = _padded(ch, H)
    _f32(xw, yw)
    h = p[:, :, xi[:, 0]] * xw[:, 0]
    for k in range(1, xi.shape[1]):
        h = h + p[:, :, xi[:, k]] * xw[:, k]
        _f32(h)
    _f32(h)
    v = h[:, yi[:, 0], :] * yw[:, 0][None, :, None]
    for k in range(1, yi.shape[1]):
        v = v + h[:, yi[:, k], :] * yw[:, k][None, :, None]
        _f32(v)
    _f32(v)
    return v


def aa_from_planes(rgbp: np.ndarray, out_hw, crop=None, mul=(1, 1, 1), add=(0, 0, 0)) -> np.ndarray:
    """uint8 planar RGB [3, h, w] of a whole picture -> the normalised float32 result [3, H, W], before the conversion to the
    output type (tests that take several dtypes of one geometry share it)"""
    h, w = rgbp.shape[1:]
    x0, y0, cw, ch = crop if crop is not None else (0, 0, w, h)
    assert 0 <= x0 and 0 <= y0 and cw >= 1 and ch >= 1 and x0 + cw <= w and y0 + ch <= h
    v = resize_planes_aa(rgbp[:, y0:y0 + ch, x0:x0 + cw].astype(np.float32), out_hw)
    m = np.asarray(mul, dtype=np.float32).reshape(3, 1, 1)
    a = np.asarray(add, dtype=np.float32).reshape(3, 1, 1)
    with np.errstate(over="ignore"):
        o = v * m + a
    _f32(o)
    return o


def export_aa_reference(yuv, w, h, hs, vs, out_hw, crop=None, mul=(1, 1, 1), add=(0, 0, 0), dtype="float32") -> np.ndarray:
    """Y|U|V of a w x h picture of sampling (hs, vs) -> raw bits [3, H, W] of `dtype`, as export_float_reference"""
    return to_dtype(aa_from_planes(export_reference(yuv, w, h, hs, vs, "rgbp"), out_hw, crop, mul, add), dtype)
