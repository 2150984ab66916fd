"""Export of resident pictures into torch tensors on the GPU (hvq_export_pictures, hvq_export_tensors).

torch is imported lazily: the rest of the package works without it.  Everything here that can refuse a destination does so
before the library is called, and the layout checks need no GPU.
"""
from __future__ import annotations

import ctypes as C
import os
import math
import struct
from typing import List, Optional, Sequence, Tuple

from ._lib import HVQ_E_STATE, HvqError

FORMATS = {"rgb": 0, "rgbp": 1, "yuv444p": 2}          # HVQ_FMT_RGB24, HVQ_FMT_RGBP, HVQ_FMT_YUV444P


class HvqExportDst(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("row_pitch", C.c_int64), ("plane_pitch", C.c_int64)]


def destinations(out, geoms: Sequence[Tuple[int, int]], fmt: str) -> List[Tuple[int, int, int]]:
    """(pointer, row pitch, plane pitch) in bytes for picture i of geometry geoms[i] = (w, h).  `out` is one uint8 tensor
    [N, H, W, 3] ("rgb") / [N, 3, H, W] (planar), or a list of N per-picture tensors [H, W, 3] / [3, H, W].  Views with larger
    strides are accepted; "rgb" needs channel stride 1 and pixel stride 3, planar formats a column stride of 1; pointers and
    pitches must be multiples of 4.  Raises TypeError / ValueError; the device is checked last, so the layout checks run on
    CPU tensors too."""
    import torch
    if fmt not in FORMATS:
        raise ValueError(f"fmt must be one of {sorted(FORMATS)}, not {fmt!r}")
    n = len(geoms)
    if isinstance(out, torch.Tensor):
        if out.dim() != 4:
            raise ValueError(f"a batch destination has 4 dimensions, not {out.dim()}")
        if out.shape[0] != n:
            raise ValueError(f"destination holds {out.shape[0]} pictures, {n} requested")
        if n and all(g == geoms[0] for g in geoms):
            # one layout for all pictures: check the first, the others lie a batch stride further
            ptr, row, plane = _destination(out[0], geoms[0], fmt, 0)
            if out.stride(0) & 3:
                raise ValueError(f"batch stride {out.stride(0)} is not a multiple of 4")
            return [(ptr + i * out.stride(0), row, plane) for i in range(n)]
        tensors = list(out.unbind(0))
    elif isinstance(out, (list, tuple)):
        tensors = list(out)
        if len(tensors) != n:
            raise ValueError(f"{len(tensors)} destinations for {n} pictures")
    else:
        raise TypeError("out must be a torch tensor or a list of tensors")
    return [_destination(t, g, fmt, i) for i, (t, g) in enumerate(zip(tensors, geoms))]


def _destination(t, geom, fmt: str, i: int) -> Tuple[int, int, int]:
    import torch
    w, h = geom
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"destination {i} is not a torch tensor")
    if t.dtype != torch.uint8:
        raise TypeError(f"destination {i} has dtype {t.dtype}, not torch.uint8")
    if t.dim() != 3:
        raise ValueError(f"destination {i} has {t.dim()} dimensions, not 3")
    if fmt == "rgb":
        if tuple(t.shape) != (h, w, 3):
            raise ValueError(f"destination {i} has shape {tuple(t.shape)}, picture needs ({h}, {w}, 3)")
        if t.stride(2) != 1 or t.stride(1) != 3:
            raise ValueError(f"destination {i}: HWC needs channel stride 1 and pixel stride 3, not {t.stride()}")
        row, plane = t.stride(0), 0
        if row < 3 * w:
            raise ValueError(f"destination {i}: rows overlap (row stride {row} < {3 * w})")
    else:
        if tuple(t.shape) != (3, h, w):
            raise ValueError(f"destination {i} has shape {tuple(t.shape)}, picture needs (3, {h}, {w})")
        if t.stride(2) != 1:
            raise ValueError(f"destination {i}: CHW needs column stride 1, not {t.stride()}")
        row, plane = t.stride(1), t.stride(0)
        if row < w or plane < row * h:
            raise ValueError(f"destination {i}: rows or planes overlap (strides {t.stride()})")
    ptr = t.data_ptr()
    if (ptr | row | plane) & 3:
        raise ValueError(f"destination {i}: pointer {ptr:#x}, row stride {row} and plane stride {plane} must be multiples of 4")
    if t.device.type != "cuda":
        raise ValueError(f"destination {i} is on {t.device}, not a GPU")
    return ptr, row, plane


FILTER_BILINEAR, FILTER_TRIANGLE, FILTER_TRIANGLE_DIRECT = 0, 1, 0x101      # HVQ_FILTER_*
DTYPES = {"float32": (0, 4), "float16": (1, 2), "bfloat16": (2, 2)}    # torch dtype name -> (HVQ_T_*, element size)
MAX_OUT = 16384


class HvqTensorDst(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("row_pitch", C.c_int64), ("plane_pitch", C.c_int64),
                ("out_w", C.c_int32), ("out_h", C.c_int32),
                ("crop_x", C.c_int32), ("crop_y", C.c_int32), ("crop_w", C.c_int32), ("crop_h", C.c_int32)]


def _f32(x: float) -> float:
    """a double rounded once to float32 (nearest even); OverflowError when it does not fit"""
    return struct.unpack("f", struct.pack("f", x))[0]


def normalisation(mean=(0, 0, 0), std=(1, 1, 1), scale: float = 1 / 255) -> Tuple[List[float], List[float]]:
    """(mul, add) of `o = v * mul[c] + add[c]`, v in 0..255: mul = scale / std and add = -mean / std, computed in double and rounded
    once to float32 -- (v * scale - mean) / std up to rounding.  ValueError for a zero or non-finite std, a non-finite mean or
    scale, or a result float32 cannot hold."""
    mean, std = [float(m) for m in mean], [float(d) for d in std]
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("mean and std have three entries, one per channel")
    scale = float(scale)
    if not math.isfinite(scale):
        raise ValueError(f"scale {scale} is not finite")
    mul, add = [], []
    for c in range(3):
        if not math.isfinite(std[c]) or std[c] == 0:
            raise ValueError(f"std[{c}] = {std[c]} must be finite and not zero")
        if not math.isfinite(mean[c]):
            raise ValueError(f"mean[{c}] = {mean[c]} is not finite")
        try:
            m, a = _f32(scale / std[c]), _f32(-mean[c] / std[c])
        except OverflowError:
            m = a = math.inf
        if not (math.isfinite(m) and math.isfinite(a)):
            raise ValueError(f"channel {c}: scale / std or mean / std does not fit float32")
        mul.append(m); add.append(a)
    return mul, add


def resample_table(n_src: int, n_out: int):
    """hvq_resample_table: the triangle filter's table of one axis (n_src = crop size, n_out = output size) as numpy arrays
    (first, count, weights) -- int32 [n_out], int32 [n_out], float32 [count.sum()]; the weights of output j start at
    count[:j].sum().  Host only: no GPU needed.  HvqError for sizes outside [1, 65535] / [1, 16384]."""
    import numpy as np
    from ._lib import check, lib
    n_src, n_out = int(n_src), int(n_out)
    need = C.c_size_t(0)
    check(lib().hvq_resample_table(n_src, n_out, None, None, None, 0, C.byref(need)))
    first, count = np.empty(n_out, dtype=np.int32), np.empty(n_out, dtype=np.int32)
    weights = np.empty(need.value, dtype=np.float32)
    i32, f32 = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    check(lib().hvq_resample_table(n_src, n_out, first.ctypes.data_as(i32), count.ctypes.data_as(i32), weights.ctypes.data_as(f32),
                                   need.value, C.byref(need)))
    return first, count, weights


def crops(crop, geoms: Sequence[Tuple[int, int]]) -> List[Tuple[int, int, int, int]]:
    """per-picture crop rectangles (x, y, w, h) in luma samples: None = whole pictures, one rectangle for all, or a list with one
    entry (or None) per picture.  ValueError for a rectangle that is empty or leaves its picture."""
    n = len(geoms)
    if crop is None:
        per = [None] * n
    elif len(crop) == 4 and all(isinstance(v, int) for v in crop):
        per = [tuple(crop)] * n
    else:
        per = list(crop)
        if len(per) != n:
            raise ValueError(f"{len(per)} crops for {n} pictures")
    out = []
    for i, (c, (w, h)) in enumerate(zip(per, geoms)):
        if c is None:
            out.append((0, 0, w, h))
            continue
        if len(c) != 4 or not all(isinstance(v, int) for v in c):
            raise ValueError(f"crop {i} is not four integers (x, y, w, h)")
        x, y, cw, ch = c
        if x < 0 or y < 0 or cw < 1 or ch < 1 or x + cw > w or y + ch > h:
            raise ValueError(f"crop {i} = {tuple(c)} is empty or outside the {w}x{h} picture")
        out.append((x, y, cw, ch))
    return out


def float_destinations(out, n: int) -> Tuple[int, List[Tuple[int, int, int, int, int]]]:
    """(HVQ_T_* of the common dtype, [(pointer, row pitch, plane pitch, W, H)] in bytes) for `n` pictures.  `out` is one float32 /
    float16 / bfloat16 tensor [N, 3, H, W] or a list of N tensors [3, H_i, W_i] of one dtype; their shapes pick the output sizes.
    Views with larger row / plane strides are accepted, the column stride must be 1; pointers and pitches need only the
    alignment of an element.  Raises TypeError / ValueError; the device is checked last."""
    import torch
    if isinstance(out, torch.Tensor):
        if out.dim() != 4:
            raise ValueError(f"a batch destination has 4 dimensions, not {out.dim()}")
        if out.shape[0] != n:
            raise ValueError(f"destination holds {out.shape[0]} pictures, {n} requested")
        if not n:
            return _float_dtype(out, 0)[0], []
        # one layout for all pictures: check the first, the others lie a batch stride further
        code, es = _float_dtype(out, 0)
        ptr, row, plane, w, h = _float_destination(out[0], es, 0)
        step = out.stride(0) * es
        return code, [(ptr + i * step, row, plane, w, h) for i in range(n)]
    if not isinstance(out, (list, tuple)):
        raise TypeError("out must be a torch tensor or a list of tensors")
    if len(out) != n:
        raise ValueError(f"{len(out)} destinations for {n} pictures")
    if not n:
        return 0, []
    code, es = _float_dtype(out[0], 0)
    for i, t in enumerate(out):
        if _float_dtype(t, i)[0] != code:
            raise TypeError(f"destination {i} has dtype {t.dtype}, destination 0 has {out[0].dtype}: one dtype per call")
    return code, [_float_destination(t, es, i) for i, t in enumerate(out)]


def _float_dtype(t, i: int) -> Tuple[int, int]:
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"destination {i} is not a torch tensor")
    name = str(t.dtype).replace("torch.", "")
    if name not in DTYPES:
        raise TypeError(f"destination {i} has dtype {t.dtype}, not float32, float16 or bfloat16")
    return DTYPES[name]


def _float_destination(t, es: int, i: int) -> Tuple[int, int, int, int, int]:
    if t.dim() != 3:
        raise ValueError(f"destination {i} has {t.dim()} dimensions, not 3")
    if t.shape[0] != 3:
        raise ValueError(f"destination {i} has {t.shape[0]} channels, not 3")
    h, w = int(t.shape[1]), int(t.shape[2])
    if not (1 <= w <= MAX_OUT and 1 <= h <= MAX_OUT):
        raise ValueError(f"destination {i}: output size {w}x{h} outside [1, {MAX_OUT}]")
    if t.stride(2) != 1:
        raise ValueError(f"destination {i}: CHW needs column stride 1, not {t.stride()}")
    row, plane = t.stride(1), t.stride(0)
    if row < w or plane < row * h:
        raise ValueError(f"destination {i}: rows or planes overlap (strides {t.stride()})")
    if t.device.type != "cuda":
        raise ValueError(f"destination {i} is on {t.device}, not a GPU")
    return t.data_ptr(), row * es, plane * es, w, h


_one_runtime = None


def check_one_hip_runtime() -> None:
    """Torch ships its own libamdhip64; the library links the system one.  Loaded by the same soname, the first one serves both
    -- unless the library was loaded before torch, which then maps a second runtime whose stream handles mean nothing to the
    library's.  Refuse that instead of handing a foreign stream over."""
    global _one_runtime
    if _one_runtime is None:
        paths = set()
        with open("/proc/self/maps") as f:
            for line in f:
                parts = line.split()
                if len(parts) >= 6 and os.path.basename(parts[5]).startswith("libamdhip64"):
                    paths.add(os.path.realpath(parts[5]))
        _one_runtime = sorted(paths)
    if len(_one_runtime) > 1:
        raise HvqError(HVQ_E_STATE, "two HIP runtimes are mapped (" + ", ".join(_one_runtime) + "): import torch before the "
                       "first use of hvqm4_amd, so that both share torch's")
