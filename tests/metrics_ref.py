"""numpy restatement of hvq_picture_metrics (include/hvqm4_amd.h): from a picture's bytes (Y | U | V tightly packed) and geometry, in
int64, to the record layout int64 [3 planes Y, U, V][4] = (sum_a, sum_b, sum |a - b|, sum (a - b)^2).  Shared by the CPU and GPU tests."""
import numpy as np


def plane_sizes(w, h, hs, vs):
    """bytes of the planes Y, U, V for chroma sampling (h_samp, v_samp) = (hs, vs)"""
    c = (w >> int(hs == 2)) * (h >> int(vs == 2))
    return w * h, c, c


def metrics_reference(a, b, w, h, hs, vs):
    """a, b: uint8 [pic_bytes]; b = None: a picture of zeros"""
    sizes = plane_sizes(w, h, hs, vs)
    a = np.asarray(a, dtype=np.uint8).reshape(-1)
    assert a.size == sum(sizes), (a.size, sizes)
    b = np.zeros_like(a) if b is None else np.asarray(b, dtype=np.uint8).reshape(-1)
    assert b.size == a.size, (a.size, b.size)
    out = np.zeros((3, 4), dtype=np.int64)
    at = 0
    for p, n in enumerate(sizes):
        x, y = a[at:at + n].astype(np.int64), b[at:at + n].astype(np.int64)
        d = x - y
        out[p] = (x.sum(), y.sum(), np.abs(d).sum(), (d * d).sum())
        at += n
    return out


def adversarial_reference(a):
    """the buffer whose every difference from `a` is at least 128: 0 where a >= 128, else 255"""
    a = np.asarray(a, dtype=np.uint8)
    return np.where(a >= 128, 0, 255).astype(np.uint8)
