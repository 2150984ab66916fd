"""The values of hvq_warp_pictures restated from the text of include/hvqm4_amd.h in plain Python: loops over Python integers, no numpy
in the arithmetic.  Slow, and meant to be: everything else is compared with it by ==.

A warp is (m00, m01, m10, m11, t0, t1, border, fill) with fill = (Y, U, V).  A plane is a list of rows (bytes or lists of integers).  A
picture is bytes Y | U | V; a geometry is (width, height, h_samp, v_samp)."""

REPLICATE, CONSTANT = 0, 1
MAX_SCALE = 32 * 65536


def check(warp):
    """the limits of the header; AssertionError beyond them"""
    m00, m01, m10, m11, t0, t1, border, fill = warp
    assert all(abs(m) <= MAX_SCALE for m in (m00, m01, m10, m11))
    assert all(-(1 << 31) <= t < 1 << 31 for t in (t0, t1))
    assert border in (REPLICATE, CONSTANT) and len(fill) == 3 and all(0 <= f <= 255 for f in fill)


def floor_div(a, b):
    return a // b                                                    # Python's // floors towards minus infinity


def position(warp, x, y, target_sampling, source_sampling):
    """(U8, V8) of target sample (x, y) of a plane whose target sampling is (hx', vy') and whose source sampling is (hx, vy)"""
    m00, m01, m10, m11, t0, t1 = warp[:6]
    hxd, vyd = target_sampling
    hx, vy = source_sampling
    nu = m00 * hxd * (2 * x + 1) + m01 * vyd * (2 * y + 1) + 2 * t0 - 65536 * hx
    nv = m10 * hxd * (2 * x + 1) + m11 * vyd * (2 * y + 1) + 2 * t1 - 65536 * vy
    return floor_div(nu + 256 * hx, 512 * hx), floor_div(nv + 256 * vy, 512 * vy)


def sample(rows, u8, v8, border, fill):
    """the value at (U8, V8) of a plane"""
    ny, nx = len(rows), len(rows[0])
    ix, iy = floor_div(u8, 256), floor_div(v8, 256)
    fx, fy = u8 - 256 * ix, v8 - 256 * iy
    assert 0 <= fx <= 255 and 0 <= fy <= 255

    def tap(j, i):
        x, y = ix + i, iy + j
        if border == REPLICATE:
            return rows[min(max(y, 0), ny - 1)][min(max(x, 0), nx - 1)]
        return rows[y][x] if 0 <= x < nx and 0 <= y < ny else fill
    s = (256 - fy) * ((256 - fx) * tap(0, 0) + fx * tap(0, 1)) + fy * ((256 - fx) * tap(1, 0) + fx * tap(1, 1))
    assert s + 32768 < 1 << 31
    return (s + 32768) >> 16


def warp_plane(rows, warp, mx, my, target_sampling=(1, 1), source_sampling=(1, 1), fill=0):
    """rows: Ny rows of Nx samples -> My rows of Mx samples (lists of integers)"""
    check(warp)
    out = []
    for y in range(my):
        line = []
        for x in range(mx):
            u8, v8 = position(warp, x, y, target_sampling, source_sampling)
            line.append(sample(rows, u8, v8, warp[6], fill))
        out.append(line)
    return out


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


def warp_picture(data, geom, warp, target_geom=None):
    """-> bytes of the warped picture of geometry target_geom (None: geom), Y | U | V"""
    target_geom = geom if target_geom is None else target_geom
    tw, th, ths, tvs = target_geom
    out = bytearray()
    for p, rows in enumerate(plane_rows(bytes(data), geom)):
        mx, my = (tw // ths, th // tvs) if p else (tw, th)
        ts, ss = ((ths, tvs), (geom[2], geom[3])) if p else ((1, 1), (1, 1))
        for line in warp_plane(rows, warp, mx, my, ts, ss, warp[7][p]):
            out += bytes(line)
    return bytes(out)


def as_ref(w):
    """a hvqm4_amd.warp.Warp as this module's tuple"""
    return (w.m00, w.m01, w.m10, w.m11, w.t0, w.t1, w.border, tuple(w.fill))
