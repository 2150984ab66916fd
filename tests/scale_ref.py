"""The values of hvq_scale_pictures restated from the text of include/hvqm4_amd.h in plain Python: loops over Python integers, no
numpy in the arithmetic.  Slow, and meant to be: everything else is compared with it by ==.

A plane is a list of rows (bytes or lists of integers).  A picture is bytes Y | U | V; a geometry is (width, height, h_samp, v_samp);
a crop is (x, y, w, h) in luma samples of the source or None."""


def weight(n, m, r, y):
    """w(r, y) = max(0, min(m (y + 1), n (r + 1)) - max(m y, n r))"""
    return max(0, min(m * (y + 1), n * (r + 1)) - max(m * y, n * r))


def scale_plane(rows, mx, my):
    """rows: ny rows of nx samples -> my rows of mx samples (lists of integers)"""
    ny, nx = len(rows), len(rows[0])
    assert nx <= 32 * mx and ny <= 32 * my, "a reduction beyond 32 is refused"
    d = nx * ny
    wx = [[(x, weight(nx, mx, c, x)) for x in range(nx) if weight(nx, mx, c, x)] for c in range(mx)]
    wy = [[(y, weight(ny, my, r, y)) for y in range(ny) if weight(ny, my, r, y)] for r in range(my)]
    assert all(sum(w for _x, w in t) == nx for t in wx) and all(sum(w for _y, w in t) == ny for t in wy)
    out = []
    for r in range(my):
        line = []
        for c in range(mx):
            s = 0
            for y, a in wy[r]:
                row = rows[y]
                for x, b in wx[c]:
                    s += a * b * row[x]
            line.append((s + (d >> 1)) // d)
        out.append(line)
    return out


def plane_rows(data, src_geom):
    """the three planes of a picture as lists of rows (bytes)"""
    w, h, hs, vs = src_geom
    cw, ch = w // hs, h // vs
    assert len(data) == w * h + 2 * cw * ch
    out, at = [], 0
    for pw, ph in ((w, h), (cw, ch), (cw, ch)):
        out.append([data[at + y * pw:at + (y + 1) * pw] for y in range(ph)])
        at += pw * ph
    return out


def scale_picture(data, src_geom, dst_geom, crop=None):
    """-> bytes of the target picture, Y | U | V"""
    w, h, hs, vs = src_geom
    dw, dh, dhs, dvs = dst_geom
    x, y, cw, ch = crop if crop is not None else (0, 0, w, h)
    assert 0 <= x and 0 <= y and cw >= 8 and ch >= 8 and x + cw <= w and y + ch <= h
    assert x % hs == 0 and cw % hs == 0 and y % vs == 0 and ch % vs == 0
    out = bytearray()
    for p, rows in enumerate(plane_rows(bytes(data), src_geom)):
        sx, sy = (hs, vs) if p else (1, 1)
        tx, ty = (dhs, dvs) if p else (1, 1)
        part = [row[x // sx:(x + cw) // sx] for row in rows[y // sy:(y + ch) // sy]]
        for line in scale_plane(part, dw // tx, dh // ty):
            out += bytes(line)
    return bytes(out)


def tie_pictures():
    """the two 8 x 8 4:4:4 pictures of the header's known answers: every 2 x 2 block is {0, 0, 0, 2} (-> 1 at half size) and
    {0, 0, 0, 1} (-> 0)"""
    out = []
    for v in (2, 1):
        plane = bytes(v if (x & 1) and (y & 1) else 0 for y in range(16) for x in range(16))
        out.append(plane * 3)
    return out


TIE_GEOMETRY = (16, 16, 1, 1)
TIE_TARGET = (8, 8, 1, 1)
