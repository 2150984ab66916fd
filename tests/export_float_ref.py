"""Helper (not a test): numpy restatement of the float export's arithmetic (include/hvqm4_amd.h, hvq_export_tensors) on top of
export_reference(..., "rgbp") of tests/test_export_cpu.py.  Everything is float32 with one rounding per operation -- numpy fuses
nothing -- and every intermediate is asserted to be float32."""
import numpy as np

from tests.test_export_cpu import export_reference

F32 = np.float32


def _f32(*arrays):
    for a in arrays:
        assert a.dtype == np.float32, a.dtype


def taps(n_out: int, n_src: int):
    """(a, b, l) of every output index along one axis: half-sample centres, taps clamped to [0, n_src - 1]"""
    s = F32(n_src) / F32(n_out)                                     # the host's single division
    j = np.arange(n_out, dtype=np.float32)
    f = np.maximum((j + F32(0.5)) * s - F32(0.5), F32(0))
    _f32(f)
    a = np.minimum(np.floor(f).astype(np.int64), n_src - 1)
    b = np.minimum(a + 1, n_src - 1)
    l = f - a.astype(np.float32)
    _f32(l)
    return a, b, l


def resize_planes(p: np.ndarray, out_hw) -> np.ndarray:
    """float32 planes [3, ch, cw] -> [3, H, W]: horizontal blend first, the two products added left to right"""
    H, W = out_hw
    _f32(p)
    ch, cw = p.shape[1:]
    ya, yb, ly = taps(H, ch)
    xa, xb, lx = taps(W, cw)
    mx, my = F32(1) - lx, (F32(1) - ly)[:, None]
    ly = ly[:, None]
    top, bot = p[:, ya], p[:, yb]
    t = top[:, :, xa] * mx + top[:, :, xb] * lx
    b = bot[:, :, xa] * mx + bot[:, :, xb] * lx
    v = t * my + b * ly
    _f32(mx, my, t, b, v)
    return v


def to_dtype(o: np.ndarray, dtype: str) -> np.ndarray:
    """float32 -> the raw bits of the output type (uint32 / uint16 arrays): both 16-bit roundings are to nearest even"""
    _f32(o)
    if dtype == "float32":
        return np.ascontiguousarray(o).view(np.uint32)
    if dtype == "float16":
        with np.errstate(over="ignore"):
            return np.ascontiguousarray(o).astype(np.float16).view(np.uint16)
    if dtype == "bfloat16":
        import torch
        return torch.from_numpy(np.ascontiguousarray(o)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    raise ValueError(dtype)


def export_float_reference(yuv, w, h, hs, vs, out_hw, crop=None, mul=(1, 1, 1), add=(0, 0, 0), dtype="float32") -> np.ndarray:
    """Y|U|V of a w x h picture of sampling (hs, vs) -> raw bits [3, H, W] of `dtype`.  crop = (x, y, cw, ch) or None; mul / add are
    taken as float32."""
    x0, y0, cw, ch = crop if crop is not None else (0, 0, w, h)
    assert 0 <= x0 and 0 <= y0 and cw >= 1 and ch >= 1 and x0 + cw <= w and y0 + ch <= h
    p = export_reference(yuv, w, h, hs, vs, "rgbp")[:, y0:y0 + ch, x0:x0 + cw].astype(np.float32)
    v = resize_planes(p, out_hw)
    m = np.asarray(mul, dtype=np.float32).reshape(3, 1, 1)
    a = np.asarray(add, dtype=np.float32).reshape(3, 1, 1)
    with np.errstate(over="ignore"):
        o = v * m + a
    _f32(o)
    return to_dtype(o, dtype)


def bits_of(t) -> np.ndarray:
    """raw bits of a torch float tensor (any device), as export_float_reference returns them"""
    import torch
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32)
    return t.view(torch.int16).numpy().view(np.uint16)
