"""The motion field of two pictures, restated from the text of include/hvqm4_amd.h (hvq_picture_motion) in numpy: every displacement of the
square |dy|, |dx| <= R in turn, for all blocks at once; the validity of a displacement per block from the four inequalities of the
header; the winner by comparing the tuples (cost, |dy| + |dx|, dy, dx) member by member.  No packed key, no tiles, no window: nothing of
the kernel's shape.  What the GPU, the fake device and hvqm4_amd.motion.of_pictures give is compared with this."""
import numpy as np

_cache = {}


def motion_reference(a, b, width, height, block, radius):
    """a, b: whole pictures (uint8, Y first) or luma planes of at least width * height bytes -> int32 [rows, cols, 4] = (dy, dx, cost,
    cost_zero)"""
    assert block in (8, 16) and 0 <= radius <= 15 and width % block == 0 and height % block == 0
    W, H, B, R = width, height, block, radius
    ya = np.asarray(a).reshape(-1)[:W * H].reshape(H, W).astype(np.int64)
    yb = np.asarray(b).reshape(-1)[:W * H].reshape(H, W).astype(np.int64)
    rows, cols = H // B, W // B
    y0 = (np.arange(rows) * B)[:, None]
    x0 = (np.arange(cols) * B)[None, :]
    big = 1 << 40
    w_cost = np.full((rows, cols), big, dtype=np.int64)
    w_l1 = np.full((rows, cols), big, dtype=np.int64)
    w_dy = np.full((rows, cols), big, dtype=np.int64)
    w_dx = np.full((rows, cols), big, dtype=np.int64)
    zero = None
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            valid = (0 <= y0 + dy) & (y0 + dy + B <= H) & (0 <= x0 + dx) & (x0 + dx + B <= W)
            if not valid.any():
                continue
            # b displaced: shifted[y][x] = b[y + dy][x + dx] where that lies inside, a value no valid block looks at elsewhere
            shifted = np.full((H, W), big, dtype=np.int64)
            ys0, ys1, xs0, xs1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            shifted[ys0:ys1, xs0:xs1] = yb[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
            cost = np.abs(ya - shifted).reshape(rows, B, cols, B).sum(axis=(1, 3))
            assert (cost[valid] <= B * B * 255).all()
            l1 = abs(dy) + abs(dx)
            less = (cost < w_cost) | ((cost == w_cost) & ((l1 < w_l1) | ((l1 == w_l1) & ((dy < w_dy) | ((dy == w_dy) & (dx < w_dx))))))
            take = valid & less
            w_cost = np.where(take, cost, w_cost)
            w_l1 = np.where(take, l1, w_l1)
            w_dy = np.where(take, dy, w_dy)
            w_dx = np.where(take, dx, w_dx)
            if dy == 0 and dx == 0:
                assert valid.all(), "(0, 0) is always a candidate"
                zero = cost
    return np.stack([w_dy, w_dx, w_cost, zero], axis=-1).astype(np.int32)


def cached(key, a, b, width, height, block, radius):
    """motion_reference, computed once per (key, block, radius) and never changed afterwards"""
    k = (key, block, radius)
    if k not in _cache:
        f = motion_reference(a, b, width, height, block, radius)
        f.setflags(write=False)
        _cache[k] = f
    return _cache[k]


def plant_cases():
    """the tie cases and the flat cases of the tests: (name, luma a, luma b, block, radius, expected record of block (1, 1) or None, the
    expected whole field or None).  Pictures are 32 x 32; block (1, 1) of a (B = 8, corner (8, 8)) is planted twice in random b, the copies
    apart from each other and neither at (0, 0)."""
    rng = np.random.default_rng(20261019)
    cases = []
    for name, first, second, winner in (("l1", (0, 5), (-4, -4), (0, 5)), ("dy", (-8, 0), (0, -8), (-8, 0)), ("dx", (0, -8), (0, 8), (0, -8))):
        a = rng.integers(0, 256, (32, 32), dtype=np.uint8)
        b = rng.integers(0, 256, (32, 32), dtype=np.uint8)
        for dy, dx in (first, second):
            b[8 + dy:16 + dy, 8 + dx:16 + dx] = a[8:16, 8:16]
        cases.append(("tie_" + name, a, b, 8, 8, (winner[0], winner[1], 0), None))
    for B in (8, 16):
        a, b = np.full((32, 32), 90, dtype=np.uint8), np.full((32, 32), 97, dtype=np.uint8)
        field = np.zeros((32 // B, 32 // B, 4), dtype=np.int32)
        field[..., 2:] = B * B * 7
        cases.append((f"flat{B}", a, b, B, 8, None, field))
    return cases
