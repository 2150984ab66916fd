"""include/hvqm4_amd.h's summed-area tables and window rules restated in plain Python: loops over the samples of every window,
math.isqrt for the deviation, Python's unbounded integers.  Shares nothing with hvqm4_amd.integral (numpy's cumsum) or with the kernels
(prefix steps, binary digits).  Lists of rows in, lists of rows out."""
import math


def tables(plane):
    """-> (S modulo 2^32, Q): the inclusive sums over x' <= x, y' <= y, the slow way"""
    ny, nx = len(plane), len(plane[0])
    S = [[0] * nx for _ in range(ny)]
    Q = [[0] * nx for _ in range(ny)]
    for y in range(ny):
        for x in range(nx):
            s = q = 0
            for yy in range(y + 1):
                for xx in range(x + 1):
                    s += plane[yy][xx]
                    q += plane[yy][xx] ** 2
            S[y][x], Q[y][x] = s % (1 << 32), q
    return S, Q


def tables_by_rows(plane):
    """the same by the recurrence T(x, y) = a + T(x - 1, y) + T(x, y - 1) - T(x - 1, y - 1), for planes the slow way cannot walk"""
    ny, nx = len(plane), len(plane[0])
    S = [[0] * nx for _ in range(ny)]
    Q = [[0] * nx for _ in range(ny)]
    for y in range(ny):
        for x in range(nx):
            for T, v in ((S, plane[y][x]), (Q, plane[y][x] ** 2)):
                T[y][x] = v + (T[y][x - 1] if x else 0) + (T[y - 1][x] if y else 0) - (T[y - 1][x - 1] if x and y else 0)
    return [[v % (1 << 32) for v in row] for row in S], Q


def box(plane, x, y, rx, ry):
    """(n, S, Q) of the window of (x, y) cut to the plane: every sample visited"""
    ny, nx = len(plane), len(plane[0])
    n = s = q = 0
    for yy in range(max(0, y - ry), min(ny - 1, y + ry) + 1):
        row = plane[yy]
        for xx in range(max(0, x - rx), min(nx - 1, x + rx) + 1):
            n += 1
            s += row[xx]
            q += row[xx] * row[xx]
    return n, s, q


def value(a, n, s, q, mode, k, c, invert):
    if mode == 0:
        return (2 * s + n) // (2 * n)
    d = math.isqrt(n * q - s * s) // n                # the largest d with (d n)^2 <= n Q - S^2
    assert (d * n) ** 2 <= n * q - s * s < ((d + 1) * n) ** 2 and 0 <= d <= 127
    if mode == 1:
        return d
    on = 256 * n * a > 256 * s + k * d * n - 256 * c * n
    return 255 if on != bool(invert) else 0


def window(plane, mode, rx, ry, k=0, c=0, invert=0):
    """what hvq_window_pictures writes into Y"""
    ny, nx = len(plane), len(plane[0])
    return [[value(plane[y][x], *box(plane, x, y, rx, ry), mode, k, c, invert) for x in range(nx)] for y in range(ny)]


def rect(plane, x0, y0, x1, y1):
    """(count, S, Q) of hvq_rect_sums for a rectangle of a plane, every sample visited; (0, 0, 0) for a refused one"""
    ny, nx = len(plane), len(plane[0])
    if not (0 <= x0 <= x1 < nx and 0 <= y0 <= y1 < ny) or (x1 - x0 + 1) * (y1 - y0 + 1) > 1 << 24:
        return 0, 0, 0
    s = q = 0
    for yy in range(y0, y1 + 1):
        for xx in range(x0, x1 + 1):
            s += plane[yy][xx]
            q += plane[yy][xx] ** 2
    return (x1 - x0 + 1) * (y1 - y0 + 1), s, q
