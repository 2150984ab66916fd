"""Recipes that the compose tests share (tests/test_compose_cpu.py, tests/test_gpu_compose.py, tests/golden/make_compose.py): lists of
hvqm4_amd.compose.Target over a flat list of pictures, built from a geometry alone.  No test of its own."""
from hvqm4_amd import compose as cp

SEAM_COLUMNS = (62, 64, 66, 126, 128, 130)            # around the seams of the kernel's 64-column tiles, in samples of a plane
SEAM_ROWS = (14, 16, 18)                              # around the seam of its 16-row tiles


def fixture_recipes(geom):
    """the fixture's recipes of a clip of geometry `geom` over two pictures (0: the clip's first, 1: its last): [(label, Target)].  The
    overlay lands at an odd chroma offset wherever the chroma is subsampled; the inset's rectangle starts at one"""
    w, h, hs, vs = geom
    return [("difference2", cp.difference(geom, 2)),
            ("crossfade0.3", cp.crossfade(geom, 0.3)),
            ("overlay77", cp.overlay(geom, 3 * hs, vs, (w // 2 // hs * hs - hs, h // 2 // vs * vs), 77)),
            ("inset", cp.inset(geom, hs, vs, rect=(hs, vs, w // 4 // hs * hs + hs, h // 4 // vs * vs + vs))),
            ("side_by_side", cp.side_by_side(geom))]


def seam_target(geom, a=0, b=1):
    """one target of the geometry of its two sources: picture a below, and over it rectangles of picture b whose right or left edge
    falls on SEAM_COLUMNS and whose lower or upper edge on SEAM_ROWS -- of the luma plane and of the chroma planes -- with source and
    destination offsets that walk through the residues mod 4; rectangles two samples wide, two high, and of one chroma sample"""
    w, h, hs, vs = geom
    layers = [cp.Layer(a)]
    xs = sorted({e * m for e in SEAM_COLUMNS for m in (1, hs) if e * m <= w and e * m % hs == 0})
    xs = xs or [hs * k for k in (5, 8, 11, 14)]                                # a plane too narrow for a seam: the residues still
    ys = sorted({e * m for e in SEAM_ROWS for m in (1, vs) if e * m <= h and e * m % vs == 0})
    k = 0
    for ex in xs:
        for ey in ys:
            for ends in (True, False):
                rw, rh = hs * (1 + k % 7), vs * (1 + k % 5)
                if k % 11 == 3:
                    rw = 2 * hs if hs == 1 else hs                            # two luma samples wide: one chroma sample where subsampled
                if k % 13 == 5:
                    rh = 2 * vs if vs == 1 else vs
                dx, dy = (ex - rw, ey - rh) if ends else (ex, ey)
                if dx < 0 or dy < 0 or dx + rw > w or dy + rh > h:
                    k += 1
                    continue
                sx, sy = min(hs * ((3 * k + k // 4) % 9), w - rw), min(vs * (k % 6), h - rh)
                mode = cp.PUT if k % 3 else cp.ADD
                layers.append(cp.Layer(b, mode, (1 + k % 2, 1, 1 + k % 3) if mode == cp.PUT else (-1, 1, -2), (sx, sy, rw, rh), (dx, dy)))
                k += 1
    for ex in xs:                                                              # the aligned body across a seam: whole dwords in every plane
        if ex % (4 * hs) == 0 and 4 * hs <= ex <= w - 4 * hs and 20 * vs <= h:
            layers.append(cp.Layer(b, cp.ADD, (1, -1, 2), (4 * hs, 2 * vs, 8 * hs, 6 * vs), (ex - 4 * hs, 13 * vs)))
    layers.append(cp.Layer(b, cp.PUT, 1, (0, 0, hs, vs), (w - hs, h - vs)))    # one chroma sample, in the last corner
    assert len(layers) <= cp.MAX_LAYERS
    return cp.Target((w, h), (hs, vs), tuple(layers), 0, (3, -2, 1))


def residues(target, p):
    """{(dx_p mod 4, (sx_p - dx_p) mod 4)} over the target's layers with a rectangle, in samples of plane p"""
    hs, vs = target.sampling if p else (1, 1)
    return {(l.at[0] // hs % 4, (l.rect[0] - l.at[0]) // hs % 4) for l in target.layers if l.rect is not None}


def order_targets(geom):
    """PUT over ADD over PUT with overlapping rectangles, and the same layers reversed"""
    w, h, hs, vs = geom
    q = lambda v, s: v // 4 // s * s
    layers = (cp.Layer(0, cp.PUT, 2),
              cp.Layer(1, cp.ADD, -1, (q(w, hs), q(h, vs), 2 * q(w, hs), 2 * q(h, vs)), (hs, vs)),
              cp.Layer(1, cp.PUT, (1, 2, 1), (0, 0, 2 * q(w, hs), q(h, vs)), (q(w, hs) + hs, q(h, vs) - vs)))
    return [cp.Target((w, h), (hs, vs), layers, 1, 7), cp.Target((w, h), (hs, vs), layers[::-1], 1, 7)]


def extreme_targets(sampling=(2, 2)):
    """over the pictures 0 (a 0 / 255 checkerboard of 128 x 128), 1 (the other checkerboard), 2 .. 257 (pictures of 8 x 8): gain exactly
    2^22 with shift 22, weights of both signs that cancel, bias +255 and -255, 256 layers in one target (a 16 x 16 mosaic of 8 x 8
    cells), count == 0"""
    big, half = ((128, 128), tuple(sampling)), cp.MAX_GAIN // 2
    return [cp.Target(*big, (cp.Layer(0, cp.ADD, half), cp.Layer(1, cp.ADD, half)), 22),
            cp.Target(*big, (cp.Layer(0, cp.ADD, cp.MAX_GAIN),), 22),
            cp.Target(*big, (cp.Layer(0, cp.ADD, half), cp.Layer(0, cp.ADD, -half)), 0, (1, 2, 3)),
            cp.Target(*big, (cp.Layer(0, cp.ADD, half), cp.Layer(1, cp.ADD, -half)), 21, 128),
            cp.Target(*big, (cp.Layer(0),), 0, 255),
            cp.Target(*big, (cp.Layer(1),), 0, (-255, -1, -254)),
            cp.mosaic(16, 16, (8, 8), tuple(sampling), sources=range(2, 258)),
            cp.Target(*big, (), 3, (16, 128, 240)),
            cp.Target(*big, (), 0, (-9, 0, 255))]


def shifted(t, by):
    """a target whose layers index the call's pictures `by` further on"""
    return cp.Target(t.size, t.sampling, tuple(cp.Layer(l.source + by, l.mode, l.weight, l.rect, l.at) for l in t.layers), t.shift, t.bias)


def flatten(targets):
    """the call of a list of targets whose layers stand one target behind the other -> (layers, [(Target, first, count)])"""
    layers, rows = [], []
    for t in targets:
        rows.append((t, len(layers), len(t.layers)))
        layers.extend(t.layers)
    return layers, rows
