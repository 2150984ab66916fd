"""numpy restatement of hvq_picture_histograms (include/hvqm4_amd.h): from a picture's bytes (Y | U | V tightly packed) and geometry to
the record layout int64 [3 planes Y, U, V][256].  b = None: HVQ_HIST_VALUES, bin v counts the samples of a equal to v; otherwise
HVQ_HIST_ABSDIFF, bin d counts the positions where |a - b| equals d.  Shared by the CPU and GPU tests."""
import numpy as np

from tests.metrics_ref import plane_sizes


def histogram_reference(a, b, width, height, h_samp, v_samp):
    """a, b: uint8 [pic_bytes]; b = None: the values of a"""
    sizes = plane_sizes(width, height, h_samp, v_samp)
    a = np.asarray(a, dtype=np.uint8).reshape(-1)
    assert a.size == sum(sizes), (a.size, sizes)
    v = a
    if b is not None:
        b = np.asarray(b, dtype=np.uint8).reshape(-1)
        assert b.size == a.size, (a.size, b.size)
        v = np.abs(a.astype(np.int16) - b)
    out = np.zeros((3, 256), dtype=np.int64)
    at = 0
    for p, n in enumerate(sizes):
        out[p] = np.bincount(v[at:at + n], minlength=256)
        at += n
    return out
