"""Picture metrics (hvq_picture_metrics, Context.picture_metrics): the references of a call, and what the records mean.

A record is int64 [3 planes Y, U, V][4] = (sum_a, sum_b, sad, sse).  The helpers below are pure torch, take CPU or CUDA tensors of
shape [..., 3, 4] and never synchronise; torch is imported lazily, the rest of the package works without it.

A record of hvq_picture_ssim / Context.picture_ssim is int64 [3 planes][2] = (sum_f, windows): the sum of the fixed-point window values
(SSIM_ONE = 2^24 is 1.0) and the number of windows; ssim_windows, ssim, ssim_all and ssim_db belong to it.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, List, Optional, Tuple

SUM_A, SUM_B, SAD, SSE = 0, 1, 2, 3
SSIM_ONE = 1 << 24                  # HVQ_SSIM_ONE
SUM_F, WINDOWS = 0, 1


class HvqMetricsRef(C.Structure):
    _fields_ = [("stream", C.c_int32), ("ordinal", C.c_int32), ("ptr", C.c_void_p)]


def references(ref, n: int, pic_bytes: Callable[[int], int]) -> Optional[List[Tuple[int, int, Optional[int]]]]:
    """(stream, ordinal, pointer) of HvqMetricsRef for each of the `n` pictures of a call, or None when `ref` is None (all zeros).
    An entry of `ref` is None (zeros: (-1, 0, None)), a pair (sid, ordinal) of integers (a resident picture) or a contiguous uint8
    tensor of pic_bytes(i) elements whose address is a multiple of 16 (the caller's memory).  Raises TypeError / ValueError; the
    device of a tensor is checked last, so the layout checks run on CPU tensors too."""
    import torch
    if ref is None:
        return None
    if not isinstance(ref, (list, tuple)):
        raise TypeError("ref must be None or a list with one entry per picture")
    if len(ref) != n:
        raise ValueError(f"{len(ref)} references for {n} pictures")
    out = []
    for i, r in enumerate(ref):
        if r is None:
            out.append((-1, 0, None))
        elif isinstance(r, torch.Tensor):
            if r.dtype != torch.uint8:
                raise TypeError(f"reference {i} has dtype {r.dtype}, not torch.uint8")
            if not r.is_contiguous():
                raise ValueError(f"reference {i} is not contiguous")
            want = int(pic_bytes(i))
            if r.numel() != want:
                raise ValueError(f"reference {i} has {r.numel()} elements, the picture has {want} bytes")
            if r.data_ptr() & 15:
                raise ValueError(f"reference {i}: pointer {r.data_ptr():#x} must be a multiple of 16")
            if r.device.type != "cuda":
                raise ValueError(f"reference {i} is on {r.device}, not a GPU")
            out.append((-1, 0, r.data_ptr()))
        elif isinstance(r, (list, tuple)):
            if len(r) != 2 or not all(isinstance(v, int) and not isinstance(v, bool) for v in r):
                raise TypeError(f"reference {i} is not a pair of integers (sid, ordinal)")
            if r[0] < 0 or r[1] < 0:
                raise ValueError(f"reference {i} = {tuple(r)}: stream and ordinal are not negative")
            out.append((int(r[0]), int(r[1]), None))
        else:
            raise TypeError(f"reference {i} must be None, (sid, ordinal) or a uint8 tensor, not {type(r).__name__}")
    return out


def plane_samples(width: int, height: int, h_samp: int = 2, v_samp: int = 2) -> Tuple[int, int, int]:
    """samples of the planes Y, U, V of a width x height picture with chroma sampling (h_samp, v_samp), each 1 or 2"""
    if h_samp not in (1, 2) or v_samp not in (1, 2):
        raise ValueError(f"sampling ({h_samp}, {v_samp}): each is 1 or 2")
    if width < 1 or height < 1:
        raise ValueError(f"{width}x{height} is not a picture size")
    c = (width >> (h_samp == 2)) * (height >> (v_samp == 2))
    return width * height, c, c


def _counts(m, samples):
    import torch
    if m.shape[-2:] != (3, 4):
        raise ValueError(f"records have shape [..., 3, 4], not {tuple(m.shape)}")
    return torch.as_tensor(samples, dtype=torch.float64, device=m.device)


def psnr(m, samples, peak: float = 255.0):
    """PSNR per plane in dB, float64 [..., 3]: 10 log10(peak^2 samples / sse); inf where sse == 0.  `samples` = plane_samples(...),
    or anything that broadcasts against [..., 3]."""
    import torch
    cnt = _counts(m, samples)
    sse = m[..., SSE].to(torch.float64)
    db = 10.0 * torch.log10(peak * peak * cnt / sse.clamp_min(1.0))
    return torch.where(sse == 0, torch.full_like(db, float("inf")), db)


def mean_abs_diff(m, samples):
    """mean |a - b| per plane, float64 [..., 3] (the luma entry of consecutive pictures is ffmpeg's scene / mpdecimate measure)"""
    import torch
    return m[..., SAD].to(torch.float64) / _counts(m, samples)


def mean_var(m, samples):
    """(mean, variance) of a per plane, float64 [..., 3] each, from records taken against zeros (sum_b == 0: sse = sum a^2);
    the variance is that of the population, E[a^2] - E[a]^2, never below 0"""
    import torch
    cnt = _counts(m, samples)
    mean = m[..., SUM_A].to(torch.float64) / cnt
    var = (m[..., SSE].to(torch.float64) / cnt - mean * mean).clamp_min(0.0)
    return mean, var


def ssim_windows(width: int, height: int, h_samp: int = 2, v_samp: int = 2) -> Tuple[Tuple[int, int], Tuple[int, int], Tuple[int, int]]:
    """(rows, cols) of the 8 x 8 SSIM windows, 4 samples apart, of the planes Y, U, V: hvq_ssim_windows.  A plane below 8 samples in a
    direction has none: (0, cols) or (rows, 0)."""
    y, c, _c = plane_samples(width, height, h_samp, v_samp)
    cw = width >> (h_samp == 2)
    dims = ((height, width), (c // cw if cw else 0, cw), (c // cw if cw else 0, cw))
    return tuple((max(h // 4 - 1, 0), max(w // 4 - 1, 0)) for h, w in dims)


def _ssim_parts(rec):
    import torch
    if rec.shape[-2:] != (3, 2):
        raise ValueError(f"SSIM records have shape [..., 3, 2], not {tuple(rec.shape)}")
    return rec[..., SUM_F].to(torch.float64), rec[..., WINDOWS].to(torch.float64)


def ssim(rec):
    """mean SSIM per plane, float64 [..., 3]: sum_f / (2^24 windows); NaN for a plane without a window"""
    import torch
    f, n = _ssim_parts(rec)
    return torch.where(n == 0, torch.full_like(f, float("nan")), f / (SSIM_ONE * n.clamp_min(1.0)))


def ssim_all(rec, samples):
    """the mean over the planes weighted by their sample counts (what ffmpeg prints as "All"), float64 [...]; planes without a window
    are left out of both sums.  `samples` = plane_samples(...), or anything that broadcasts against [..., 3]."""
    import torch
    f, n = _ssim_parts(rec)
    cnt = torch.as_tensor(samples, dtype=torch.float64, device=rec.device) * (n > 0)
    return ((f / (SSIM_ONE * n.clamp_min(1.0))) * cnt).sum(-1) / cnt.sum(-1)


def ssim_db(x):
    """-10 log10(1 - x), inf at 1"""
    import torch
    x = torch.as_tensor(x, dtype=torch.float64)
    db = -10.0 * torch.log10((1.0 - x).clamp_min(1e-300))
    return torch.where(x >= 1.0, torch.full_like(db, float("inf")), db)
