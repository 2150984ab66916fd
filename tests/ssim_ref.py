"""numpy restatement of hvq_picture_ssim (include/hvqm4_amd.h): from two pictures' bytes (Y | U | V tightly packed) and geometry to the
record int64 [3 planes Y, U, V][2] = (sum_f, windows) and the three maps of window values q (float32 [rows, cols]).  The window integers
are int64, narrowed through int32 to float32 as the kernel converts them; the products and the quotient are float32, one rounding each;
f = rint(q * 2^24).  Shared by the CPU and GPU tests."""
import numpy as np

from tests.metrics_ref import plane_sizes

SSIM_ONE = 1 << 24
C1, C2 = 416, 235963


def plane_dims(w, h, hs, vs):
    """(height, width) of the planes Y, U, V"""
    cw, ch = w >> int(hs == 2), h >> int(vs == 2)
    return (h, w), (ch, cw), (ch, cw)


def window_dims(w, h, hs, vs):
    """(rows, cols) of the windows of the planes Y, U, V"""
    return tuple((max(ph // 4 - 1, 0), max(pw // 4 - 1, 0)) for ph, pw in plane_dims(w, h, hs, vs))


def ssim_plane(a, b):
    """a, b: uint8 [H, W], H and W multiples of 4 -> (q float32 [rows, cols], f int64 [rows, cols])"""
    h, w = a.shape
    assert h % 4 == 0 and w % 4 == 0 and a.shape == b.shape, (a.shape, b.shape)
    rows, cols = max(h // 4 - 1, 0), max(w // 4 - 1, 0)
    if rows == 0 or cols == 0:
        return np.zeros((rows, cols), dtype=np.float32), np.zeros((rows, cols), dtype=np.int64)
    a, b = a.astype(np.int64), b.astype(np.int64)
    blk = lambda x: x.reshape(h // 4, 4, w // 4, 4).sum(axis=(1, 3))
    win = lambda x: x[:-1, :-1] + x[:-1, 1:] + x[1:, :-1] + x[1:, 1:]
    s1, s2, ss, s12 = (win(blk(x)) for x in (a, b, a * a + b * b, a * b))
    assert s1.max() <= 16320 and s2.max() <= 16320 and ss.max() <= 8323200
    va = 64 * ss - s1 * s1 - s2 * s2
    co = 64 * s12 - s1 * s2
    A, B, C, D = 2 * s1 * s2 + C1, 2 * co + C2, s1 * s1 + s2 * s2 + C1, va + C2
    for v in (A, B, C, D):
        assert np.abs(v).max() < 2 ** 30, int(np.abs(v).max())              # they fit 32 bits, with room
    assert (A > 0).all() and (C > 0).all() and (D > 0).all() and (B % 2 != 0).all()
    f32 = lambda v: v.astype(np.int32).astype(np.float32)
    num, den = f32(A) * f32(B), f32(C) * f32(D)
    assert num.dtype == np.float32 and den.dtype == np.float32
    q = num / den
    assert q.dtype == np.float32
    f = np.rint(q * np.float32(SSIM_ONE)).astype(np.int64)
    return q, f


def ssim_reference(a, b, w, h, hs, vs):
    """a, b: uint8 [pic_bytes] -> (record int64 [3, 2], [q of Y, q of U, q of V])"""
    sizes = plane_sizes(w, h, hs, vs)
    a = np.asarray(a, dtype=np.uint8).reshape(-1)
    b = np.asarray(b, dtype=np.uint8).reshape(-1)
    assert a.size == sum(sizes) and b.size == a.size, (a.size, b.size, sizes)
    rec = np.zeros((3, 2), dtype=np.int64)
    maps = []
    at = 0
    for p, ((ph, pw), n) in enumerate(zip(plane_dims(w, h, hs, vs), sizes)):
        q, f = ssim_plane(a[at:at + n].reshape(ph, pw), b[at:at + n].reshape(ph, pw))
        rec[p] = (f.sum(), f.size)
        maps.append(q)
        at += n
    return rec, maps


def flat_maps(maps):
    """the three maps as the library lays them out: Y, U, V, each row-major, dense"""
    return np.concatenate([m.reshape(-1) for m in maps]).astype(np.float32) if maps else np.zeros(0, dtype=np.float32)


def checkerboard(w, h, hs, vs):
    """a picture whose every plane is a checkerboard of 0 and 255"""
    return np.concatenate([((np.add.outer(np.arange(ph), np.arange(pw)) & 1) * 255).astype(np.uint8).reshape(-1)
                           for ph, pw in plane_dims(w, h, hs, vs)])
