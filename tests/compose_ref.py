"""The values of hvq_compose_pictures restated from the text of include/hvqm4_amd.h in plain Python: loops over Python integers, no numpy
in the arithmetic.  Slow, and meant to be: everything else is compared with it by ==.

A layer is (source, mode, (wY, wU, wV), rect, (dx, dy)) with rect = (sx, sy, w, h) in luma samples or None for the whole source.  A
target is ((w, h), (h_samp, v_samp), layers, shift, (biasY, biasU, biasV)).  A picture is bytes Y | U | V; a geometry is (width, height,
h_samp, v_samp)."""

PUT, ADD = 0, 1
MAX_LAYERS, MAX_GAIN, MAX_SHIFT = 256, 1 << 22, 22


def as_ref(target):
    """a hvqm4_amd.compose.Target as this module's tuple"""
    return (tuple(target.size), tuple(target.sampling), tuple((l.source, l.mode, l.weights(), l.rect, tuple(l.at)) for l in target.layers),
            target.shift, target.biases())


def plane_geometry(geom, p):
    w, h, hs, vs = geom
    return (w, h) if p == 0 else (w // hs, h // vs)


def planes(picture, geom):
    """the three planes of a picture as lists of rows"""
    out, at = [], 0
    for p in range(3):
        pw, ph = plane_geometry(geom, p)
        out.append([picture[at + y * pw:at + (y + 1) * pw] for y in range(ph)])
        at += pw * ph
    assert at == len(picture)
    return out


def floor_shift(v, shift):
    return v // (1 << shift)                                         # Python's // floors towards minus infinity


def finish(acc, shift, bias):
    h = 1 << (shift - 1) if shift else 0
    return min(255, max(0, floor_shift(acc + h, shift) + bias))


def compose_picture(pictures, geoms, target):
    """the bytes of one target: pictures[i] the bytes of the call's picture i, of geometry geoms[i]"""
    (w, h), (hs, vs), layers, shift, bias = target
    assert 0 <= shift <= MAX_SHIFT and all(-255 <= b <= 255 for b in bias) and len(layers) <= MAX_LAYERS
    split = {}
    out = bytearray()
    for p in range(3):
        hx, vy = (1, 1) if p == 0 else (hs, vs)
        recs = []
        for source, mode, weight, rect, (dx, dy) in layers:
            g = geoms[source]
            assert tuple(g[2:]) == (hs, vs), "a layer has its target's sampling"
            sx, sy, rw, rh = (0, 0, g[0], g[1]) if rect is None or rect[2] == 0 else rect
            assert mode in (PUT, ADD) and rw > 0 and rh > 0 and min(sx, sy, dx, dy) >= 0
            assert sx + rw <= g[0] and sy + rh <= g[1] and dx + rw <= w and dy + rh <= h, "nothing is clipped"
            assert all(v % hs == 0 for v in (sx, rw, dx)) and all(v % vs == 0 for v in (sy, rh, dy)), "the numbers divide exactly"
            if source not in split:
                split[source] = planes(pictures[source], g)
            recs.append((split[source][p], mode, weight[p], sx // hx, sy // vy, rw // hx, rh // vy, dx // hx, dy // vy))
        assert sum(abs(r[2]) for r in recs) <= MAX_GAIN
        pw, ph = plane_geometry((w, h, hs, vs), p)
        for y in range(ph):
            row = [r for r in recs if r[8] <= y < r[8] + r[6]]       # the layers that meet this row, in their order: the rest cannot cover a sample of it
            for x in range(pw):
                acc = 0
                for a, mode, wt, sx, sy, rw, rh, dx, dy in row:
                    if dx <= x < dx + rw and dy <= y < dy + rh:
                        s = a[y - dy + sy][x - dx + sx]
                        acc = (0 if mode == PUT else acc) + wt * s
                out.append(finish(acc, shift, bias[p]))
    return bytes(out)
