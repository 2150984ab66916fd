"""The values of hvq_filter_pictures restated from the text of include/hvqm4_amd.h in plain Python: loops over Python integers, no
numpy in the arithmetic.  Slow, and meant to be: everything else is compared with it by ==.

A plane is a list of rows (bytes or lists of integers).  A plane filter is (terms, combine, shift, bias) with terms a list of (wx, wy),
each a sequence of 2 r + 1 integers.  A picture is bytes Y | U | V; a geometry is (width, height, h_samp, v_samp)."""

SUM, ABS_SUM, SUM_ABS = 0, 1, 2
MAX_RADIUS, MAX_SHIFT, MAX_GAIN = 15, 22, 1 << 22


def check_plane(terms, combine, shift, bias):
    """the limits of the header; AssertionError beyond them"""
    assert len(terms) in (1, 2)
    assert combine in (SUM, ABS_SUM, SUM_ABS) and 0 <= shift <= MAX_SHIFT and -255 <= bias <= 255
    gain = 0
    for wx, wy in terms:
        assert len(wx) % 2 == 1 and len(wy) % 2 == 1 and len(wx) <= 2 * MAX_RADIUS + 1 and len(wy) <= 2 * MAX_RADIUS + 1
        gain += sum(abs(w) for w in wx) * sum(abs(w) for w in wy)
    assert 1 <= gain <= MAX_GAIN
    return gain


def term_plane(rows, wx, wy):
    """T[y][x] = sum over j, i of wy[j] wx[i] a[cy(y + j - ry)][cx(x + i - rx)]: correlation, borders replicate"""
    ny, nx = len(rows), len(rows[0])
    rx, ry = (len(wx) - 1) // 2, (len(wy) - 1) // 2
    out = []
    for y in range(ny):
        line = []
        for x in range(nx):
            s = 0
            for j in range(2 * ry + 1):
                row = rows[min(max(y + j - ry, 0), ny - 1)]
                for i in range(2 * rx + 1):
                    s += wy[j] * wx[i] * row[min(max(x + i - rx, 0), nx - 1)]
            line.append(s)
        out.append(line)
    return out


def finish(t0, t1, combine, shift, bias):
    """S = combine(T0, T1); out = min(255, max(0, floor((S + h) / 2^shift) + bias)), h = shift ? 1 << (shift - 1) : 0"""
    s = t0 + t1 if combine == SUM else abs(t0 + t1) if combine == ABS_SUM else abs(t0) + abs(t1)
    h = 1 << (shift - 1) if shift else 0
    assert abs(s) + h < 1 << 31, "32-bit signed arithmetic serves everywhere"
    return min(255, max(0, (s + h) // (1 << shift) + bias))          # Python's // floors towards minus infinity


def filter_plane(rows, terms, combine, shift, bias):
    """rows: ny rows of nx samples -> ny rows of nx samples (lists of integers)"""
    check_plane(terms, combine, shift, bias)
    t = [term_plane(rows, wx, wy) for wx, wy in terms]
    ny, nx = len(rows), len(rows[0])
    return [[finish(t[0][y][x], t[1][y][x] if len(t) == 2 else 0, combine, shift, bias) for x in range(nx)] for y in range(ny)]


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


def filter_picture(data, geom, luma, chroma):
    """-> bytes of the filtered picture, Y | U | V; luma and chroma are plane filters (terms, combine, shift, bias)"""
    out = bytearray()
    for p, rows in enumerate(plane_rows(bytes(data), geom)):
        for line in filter_plane(rows, *(chroma if p else luma)):
            out += bytes(line)
    return bytes(out)


def as_ref(plane_filter):
    """a hvqm4_amd.filters.PlaneFilter as this module's tuple"""
    return ([(list(t.wx), list(t.wy)) for t in plane_filter.terms], plane_filter.combine, plane_filter.shift, plane_filter.bias)
