"""TEST INFRASTRUCTURE: an independent restatement of the hash records of include/hvqm4_amd.h (hvq_picture_hashes) and of
hvq_hash_nearest, for the tests to compare with.  Plain loops over Python integers (the grids), `fractions` as a second statement of
the grids (cell edges as rationals, for small pictures), Python integers for the DCT; the table comes from the formula, not from the
committed constants.  It does not import hvqm4_amd.phash.
"""
import math
from fractions import Fraction

MASK64 = (1 << 64) - 1


def table():
    """C[k][n] = floor(4096 cos((2 n + 1) k pi / 64) + 0.5), 8 x 32, from the formula"""
    return [[math.floor(4096 * math.cos((2 * n + 1) * k * math.pi / 64) + 0.5) for n in range(32)] for k in range(8)]


def tie_margin():
    """the smallest distance of 4096 cos(...) from a rounding tie over the whole table"""
    return min(abs((4096 * math.cos((2 * n + 1) * k * math.pi / 64)) % 1 - 0.5) for k in range(8) for n in range(32))


def axis(g, n):
    """per sample 0 <= y < n the list of (cell, weight) with weight > 0: weight = max(0, min(g y + g, n r + n) - max(g y, n r))"""
    out = []
    for y in range(n):
        cells = []
        for r in range(g * y // n, min(g - 1, (g * y + g - 1) // n) + 1):
            w = min(g * y + g, n * r + n) - max(g * y, n * r)
            if w > 0:
                cells.append((r, w))
        assert sum(w for _r, w in cells) == g
        out.append(cells)
    return out


def grid_simple(rows, gy, gx):
    """S[r][c] of a plane given as a list of rows of integers: sample by sample, straight from the formula"""
    h, w = len(rows), len(rows[0])
    ay, ax = axis(gy, h), axis(gx, w)
    s = [[0] * gx for _ in range(gy)]
    for y in range(h):
        for r, wy in ay[y]:
            for x in range(w):
                for c, wx in ax[x]:
                    s[r][c] += wy * wx * rows[y][x]
    return s


def spans(g, n):
    """per cell r the samples with a share in it, as (first, end, edges): the samples [first, end) lie wholly inside (weight g), `edges`
    lists the others as (sample, weight)"""
    out = []
    for r in range(g):
        full, edges = [], []
        for y in range(n * r // g, (n * (r + 1) + g - 1) // g):
            w = min(g * y + g, n * r + n) - max(g * y, n * r)
            assert w > 0
            (full if w == g else edges).append((y, w))
        first, end = (full[0][0], full[-1][0] + 1) if full else (0, 0)
        assert end - first == len(full)
        assert g * (end - first) + sum(w for _y, w in edges) == n
        out.append((first, end, edges))
    return out


def grid(rows, gy, gx):
    """S[r][c] of a plane given as a list of rows (lists of integers, or bytes): per row the sums of the runs of samples that lie wholly
    inside a cell, plus the weighted samples on the cell's edges; then the same for the rows of a row cell"""
    h, w = len(rows), len(rows[0])
    sx, ay = spans(gx, w), axis(gy, h)
    s = [[0] * gx for _ in range(gy)]
    for y in range(h):
        row = rows[y]
        line = [gx * sum(row[first:end]) + sum(wx * row[x] for x, wx in edges) for first, end, edges in sx]
        for r, wy in ay[y]:
            dst = s[r]
            for c in range(gx):
                dst[c] += wy * line[c]
    return s


def grid_fractions(rows, gy, gx):
    """the same cells from the definition: cell (r, c) is the rectangle [r H / gy, (r + 1) H / gy) x [c W / gx, (c + 1) W / gx) of the
    plane, every sample a unit square; the cell's integral of the picture, times gy gx"""
    h, w = len(rows), len(rows[0])
    s = [[0] * gx for _ in range(gy)]
    for r in range(gy):
        y0, y1 = Fraction(r * h, gy), Fraction((r + 1) * h, gy)
        for c in range(gx):
            x0, x1 = Fraction(c * w, gx), Fraction((c + 1) * w, gx)
            acc = Fraction(0)
            for y in range(math.floor(y0), math.ceil(y1)):
                oy = min(y1, y + 1) - max(y0, y)
                for x in range(math.floor(x0), math.ceil(x1)):
                    acc += oy * (min(x1, x + 1) - max(x0, x)) * rows[y][x]
            acc *= gy * gx
            assert acc.denominator == 1
            s[r][c] = int(acc)
    return s


def bits(flags):
    v = 0
    for f in flags:
        v = v << 1 | (1 if f else 0)
    return v


def record_of_cells(s32, s8, d, wh, cell_mod=None):
    """the record from the three grids.  cell_mod: reduce every cell modulo it first (what a 32-bit cell would hold), for the test
    that shows such a cell is wrong"""
    if cell_mod:
        s32 = [[v % cell_mod for v in row] for row in s32]
        s8 = [[v % cell_mod for v in row] for row in s8]
        d = [[v % cell_mod for v in row] for row in d]
    t = sum(sum(row) for row in s8)
    ahash = bits(64 * s8[r][c] > t for r in range(8) for c in range(8))
    dhash = bits(d[r][c + 1] > d[r][c] for r in range(8) for c in range(8))
    m = [[(16 * s32[r][c] + (wh >> 1)) // wh for c in range(32)] for r in range(32)]
    C = table()
    g = [[sum(C[l][c] * m[r][c] for c in range(32)) for l in range(8)] for r in range(32)]
    f = [sum(C[k][r] * g[r][l] for r in range(32)) for k in range(8) for l in range(8)]
    srt = sorted(f)
    phash = bits(2 * v > srt[31] + srt[32] for v in f)
    return [ahash, dhash, phash, t // 64]


def hash_reference(plane):
    """[ahash, dhash, phash, sum_y] of a luma plane: a 2-D array-like of 8-bit samples (numpy array or list of rows)"""
    rows = [row if isinstance(row, bytes) else bytes(bytearray(int(v) for v in row)) for row in plane]
    h, w = len(rows), len(rows[0])
    return record_of_cells(grid(rows, 32, 32), grid(rows, 8, 8), grid(rows, 8, 9), w * h)


def picture_reference(picture, width, height):
    """the record of a picture given as its bytes Y | U | V (any sampling: the luma plane comes first)"""
    data = bytes(picture)
    return hash_reference([data[y * width:(y + 1) * width] for y in range(height)])


def popcount(v):
    return bin(v & MASK64).count("1")


def nearest_reference(q, db, self_offset, threshold):
    """[nq][4] = (nearest, distance, within, first_within) by the definition, hashes as Python integers (any sign: 64 bits count)"""
    out = []
    for i, a in enumerate(q):
        lim = len(db) if self_offset < 0 else max(0, min(len(db), self_offset + i))
        best, within, first = (65, -1), 0, -1
        for j in range(lim):
            d = popcount(int(a) ^ int(db[j]))
            if (d, j) < best:
                best = (d, j)
            if d <= threshold:
                within += 1
                if first < 0:
                    first = j
        out.append([best[1], best[0], within, first])
    return out
