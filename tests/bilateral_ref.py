"""The values of hvq_bilateral_pictures restated from the text of include/hvqm4_amd.h in plain Python: one sample at a time, Python
integers, no numpy and nothing of the library.  For the small shapes only: radius 7 on a 64 x 48 plane is under a second.

A plane is a list of rows (bytes, or lists of integers); a set is (rx, ry, spatial, range) with spatial[|j|][|i|] and range[d] indexable
(as_ref makes one of a hvqm4_amd.bilateral.PlaneBilateral)."""


def as_ref(p):
    """hvqm4_amd.bilateral.PlaneBilateral -> (rx, ry, spatial as 8 rows of 8, range as a list of 256)"""
    return (p.rx, p.ry, [list(p.spatial[8 * j:8 * j + 8]) for j in range(8)], list(p.range))


def sample(a, g, y, x, rx, ry, spatial, rng):
    """out at (y, x): the header's Window, Weights and Value"""
    ny, nx = len(a), len(a[0])
    cy = lambda v: min(max(v, 0), ny - 1)
    cx = lambda v: min(max(v, 0), nx - 1)
    num = den = 0
    for j in range(-ry, ry + 1):
        for i in range(-rx, rx + 1):
            qy, qx = cy(y + j), cx(x + i)
            w = spatial[abs(j)][abs(i)] * rng[abs(g[qy][qx] - g[y][x])]
            assert 0 <= w <= 65025
            den += w
            num += w * a[qy][qx]
    assert den >= 1 and num + den // 2 < 2 ** 32, (num, den)
    out = (num + den // 2) // den
    assert 0 <= out <= 255
    return out


def bilateral_plane(a, g, rx, ry, spatial, rng):
    """a plane with the guide plane g (None: a itself) -> a list of rows of integers"""
    assert 0 <= rx <= 7 and 0 <= ry <= 7 and spatial[0][0] >= 1 and rng[0] >= 1
    g = a if g is None else g
    assert len(g) == len(a) and len(g[0]) == len(a[0])
    return [[sample(a, g, y, x, rx, ry, spatial, rng) for x in range(len(a[0]))] for y in range(len(a))]


def split(buf, geom):
    """a picture's bytes -> its three planes as lists of rows"""
    w, h, hs, vs = geom
    out, at = [], 0
    for pw, ph in ((w, h), (w // hs, h // vs), (w // hs, h // vs)):
        out.append([bytes(buf[at + r * pw:at + (r + 1) * pw]) for r in range(ph)])
        at += pw * ph
    assert at == len(buf)
    return out


def bilateral_picture(buf, geom, luma, chroma, guide=None):
    """a picture (bytes, Y | U | V) through the sets of its planes, guided by the picture `guide` (None: by itself) -> bytes"""
    gp = [None] * 3 if guide is None else split(guide, geom)
    out = bytearray()
    for p, a in enumerate(split(buf, geom)):
        for row in bilateral_plane(a, gp[p], *(chroma if p else luma)):
            out += bytes(row)
    return bytes(out)


def steps_picture(buf, geom, steps, guide=None):
    """the picture through every (luma, chroma) step in turn"""
    for luma, chroma in steps:
        buf = bilateral_picture(buf, geom, luma, chroma, guide)
    return buf
