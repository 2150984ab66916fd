"""The values of hvq_rank_pictures restated from the text of include/hvqm4_amd.h in plain Python: nested loops over Python integers and
sorted(window)[k], no numpy in the arithmetic.  Slow, and meant to be: everything else is compared with it by ==.

A plane is a list of rows (bytes or lists of integers).  A plane operation is (op, rx, ry).  A picture is bytes Y | U | V; a geometry
is (width, height, h_samp, v_samp)."""

MIN, MAX, RANGE, MEDIAN = 0, 1, 2, 3
MAX_RADIUS = 15


def check_plane(op, rx, ry):
    """the limits of the header; AssertionError beyond them"""
    assert op in (MIN, MAX, RANGE, MEDIAN)
    assert 0 <= rx <= MAX_RADIUS and 0 <= ry <= MAX_RADIUS
    if op == MEDIAN:
        assert rx == ry and rx in (0, 1, 2)


def window(rows, y, x, rx, ry):
    """W(y, x): the (2 ry + 1)(2 rx + 1) samples a[cy(y + j - ry)][cx(x + i - rx)]; a clamped coordinate counts as often as it occurs"""
    ny, nx = len(rows), len(rows[0])
    w = []
    for j in range(2 * ry + 1):
        row = rows[min(max(y + j - ry, 0), ny - 1)]
        for i in range(2 * rx + 1):
            w.append(row[min(max(x + i - rx, 0), nx - 1)])
    return w


def rank_of(w, op):
    if op == MIN:
        return min(w)
    if op == MAX:
        return max(w)
    if op == RANGE:
        return max(w) - min(w)
    return sorted(w)[(len(w) - 1) // 2]


def rank_plane(rows, op, rx, ry):
    """rows: ny rows of nx samples -> ny rows of nx samples (lists of integers)"""
    check_plane(op, rx, ry)
    return [[rank_of(window(rows, y, x, rx, ry), op) for x in range(len(rows[0]))] for y in range(len(rows))]


def plane_rows(data, geom):
    """the three planes of a picture as lists of rows (bytes)"""
    w, h, hs, vs = geom
    cw, ch = w // hs, h // vs
    assert len(data) == w * h + 2 * cw * ch
    out, at = [], 0
    for pw, ph in ((w, h), (cw, ch), (cw, ch)):
        out.append([data[at + y * pw:at + (y + 1) * pw] for y in range(ph)])
        at += pw * ph
    return out


def rank_picture(data, geom, luma, chroma):
    """-> bytes of the picture through the plane operations luma and chroma, (op, rx, ry) each: Y | U | V"""
    out = bytearray()
    for p, rows in enumerate(plane_rows(bytes(data), geom)):
        for line in rank_plane(rows, *(chroma if p else luma)):
            out += bytes(line)
    return bytes(out)


def steps_picture(data, geom, steps):
    """the picture through a list of (luma, chroma) steps in turn"""
    data = bytes(data)
    for luma, chroma in steps:
        data = rank_picture(data, geom, luma, chroma)
    return data


def as_ref(plane_rank):
    """a hvqm4_amd.rank.PlaneRank as this module's tuple"""
    return (plane_rank.op, plane_rank.rx, plane_rank.ry)
