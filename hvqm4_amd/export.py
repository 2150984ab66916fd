"""Export of resident pictures into torch tensors on the GPU (hvq_export_pictures).

torch is imported lazily: the rest of the package works without it.  Everything here that can refuse a destination does so
before the library is called, and the layout checks need no GPU.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Sequence, Tuple

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
