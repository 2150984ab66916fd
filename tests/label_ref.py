"""include/hvqm4_amd.h's text on hvq_label_pictures and hvq_select_components, restated in plain Python with no numpy arithmetic and no
shared code with hvqm4_amd.labels: a raster scan, and a flood fill from every foreground sample that has no number yet.  Slow and
obvious on purpose; the tests hold the module, the fake device and the GPU equal to it."""

NEIGHBOURS = {4: ((-1, 0), (1, 0), (0, -1), (0, 1)), 8: ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))}


def label(plane, lo=255, hi=255, connectivity=8, cap=None):
    """plane: rows of samples -> (labels: rows of numbers, records: rows of eight integers, row 0 first, stored + 1 of them)"""
    ny, nx = len(plane), len(plane[0])
    fg = [[lo <= int(a) <= hi for a in row] for row in plane]
    lab = [[0] * nx for _ in range(ny)]
    rows = []
    K = 0
    for y in range(ny):
        for x in range(nx):
            if not fg[y][x] or lab[y][x]:
                continue
            K += 1                                      # the unnumbered foreground sample of the smallest raster index: a first sample
            lab[y][x] = K
            stack, filled = [(x, y)], []
            while stack:
                cx, cy = stack.pop()
                filled.append((cx, cy))
                for dx, dy in NEIGHBOURS[connectivity]:
                    px, py = cx + dx, cy + dy
                    if 0 <= px < nx and 0 <= py < ny and fg[py][px] and not lab[py][px]:
                        lab[py][px] = K
                        stack.append((px, py))
            xs, ys = [p[0] for p in filled], [p[1] for p in filled]
            rows.append([len(filled), min(xs), min(ys), max(xs), max(ys), y * nx + x, sum(xs), sum(ys)])
    stored = K if cap is None else min(K, cap)
    F = sum(sum(r) for r in fg)
    return lab, [[K, stored, F, 0, 0, 0, 0, 0]] + rows[:stored]


def select(lab, records, area=(0, 2 ** 32 - 1), width=(0, 2 ** 32 - 1), height=(0, 2 ** 32 - 1), invert=0, chroma_samples=0):
    """the bytes of hvq_select_components for a Y label map and its records: Y, then 2 * chroma_samples bytes of 128"""
    stored = records[0][1]
    out = []
    for row in lab:
        for k in row:
            sel = False
            if 1 <= k <= stored:
                a, x0, y0, x1, y1 = records[k][:5]
                sel = area[0] <= a <= area[1] and width[0] <= x1 - x0 + 1 <= width[1] and height[0] <= y1 - y0 + 1 <= height[1]
            out.append(255 if sel != bool(invert) else 0)
    return bytes(out) + bytes([128]) * (2 * chroma_samples)
