"""The corner values of include/hvqm4_amd.h restated in plain Python: ints, loops and math.isqrt, one sample at a time.  Slow on
purpose; it is what hvqm4_amd.corners, the fake device and the GPU are held to on small planes.  A plane is a list of rows of ints."""
import math

HARRIS, MIN_EIGEN = 0, 1


def sample(a, y, x):
    ny, nx = len(a), len(a[0])
    return a[min(max(y, 0), ny - 1)][min(max(x, 0), nx - 1)]


def gradient(a, y, x):
    gx = (sample(a, y - 1, x + 1) + 2 * sample(a, y, x + 1) + sample(a, y + 1, x + 1)
          - sample(a, y - 1, x - 1) - 2 * sample(a, y, x - 1) - sample(a, y + 1, x - 1))
    gy = (sample(a, y + 1, x - 1) + 2 * sample(a, y + 1, x) + sample(a, y + 1, x + 1)
          - sample(a, y - 1, x - 1) - 2 * sample(a, y - 1, x) - sample(a, y - 1, x + 1))
    assert abs(gx) <= 1020 and abs(gy) <= 1020
    return gx, gy


def sums(a, y, x, radius):
    A = B = C = 0
    for py in range(y - radius, y + radius + 1):
        for px in range(x - radius, x + radius + 1):
            gx, gy = gradient(a, py, px)
            A += gx * gx
            B += gx * gy
            C += gy * gy
    assert A < 1 << 26 and C < 1 << 26 and abs(B) < 1 << 26
    return A, B, C


def response(a, y, x, mode, radius, k):
    A, B, C = sums(a, y, x, radius)
    T = A + C
    if mode == HARRIS:
        R = 256 * (A * C - B * B) - k * T * T
        assert abs(R) < 1 << 61
    else:
        v = (A - C) * (A - C) + 4 * B * B
        assert v < 1 << 55
        R = T - math.isqrt(v)
        assert 0 <= R < 1 << 27
    assert abs(R) < 1 << 63
    return R


def response_map(a, mode, radius, k):
    return [[response(a, y, x, mode, radius, k) for x in range(len(a[0]))] for y in range(len(a))]


def corners(a, mode=HARRIS, radius=1, k=10, nms=3, margin=0, threshold=1, cap=None, R=None):
    """-> (mask rows of 0 / 255, points [stored + 1][4], rows [Ny + 1], R)"""
    ny, nx = len(a), len(a[0])
    R = response_map(a, mode, radius, k) if R is None else R
    mask = [[0] * nx for _ in range(ny)]
    found = []
    for y in range(ny):
        for x in range(nx):
            if not (margin <= x < nx - margin and margin <= y < ny - margin) or R[y][x] < threshold:
                continue
            beaten = False
            for qy in range(max(y - nms, 0), min(y + nms, ny - 1) + 1):
                for qx in range(max(x - nms, 0), min(x + nms, nx - 1) + 1):
                    if (qy, qx) == (y, x):
                        continue
                    if R[qy][qx] > R[y][x] or (R[qy][qx] == R[y][x] and qy * nx + qx < y * nx + x):
                        beaten = True
            if not beaten:
                mask[y][x] = 255
                found.append([x, y, R[y][x], y * nx + x])
    K = len(found)
    stored = K if cap is None else min(K, cap)
    rows = [0] * (ny + 1)
    for y in range(ny):
        rows[y + 1] = rows[y] + sum(1 for v in mask[y] if v)
    return mask, [[K, stored, 0, 0]] + found[:stored], rows, R
