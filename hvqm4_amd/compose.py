"""Composition of pictures in slot layout (include/hvqm4_amd.h, hvq_compose_pictures): the layers and targets of a call, the library's
argument checks in its words, the expected bytes (numpy, host only), and builders named for what the picture becomes.

A call has a flat list of pictures; Layer.source indexes it.  A target is an ordered list of layers over a background of its bias:

    acc = 0;  for each layer that covers the sample, in order:  acc = (PUT ? 0 : acc) + weight * s
    out = clamp(((acc + half) >> shift) + bias)          half = shift ? 1 << (shift - 1) : 0: ONE rounding

The bias joins covered samples too: a background other than 0 under samples that are copied needs a flat picture as the lowest layer
(flat_picture gives its bytes, for src=)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from . import scale as sc

PUT, ADD = 0, 1                  # HVQ_CMP_PUT, HVQ_CMP_ADD
MAX_LAYERS = 256                 # HVQ_CMP_MAX_LAYERS: per target
MAX_TOTAL = 1 << 18              # HVQ_CMP_MAX_TOTAL: layers per call
MAX_GAIN = 1 << 22               # HVQ_CMP_MAX_GAIN: per target and plane, sum of |weight|
MAX_SHIFT = 22                   # HVQ_CMP_MAX_SHIFT
ALIGNED, GENERAL = 0, 1          # the bodies of the kernel (hvq_compose.h)

Geom = Tuple[int, int, int, int]  # width, height, h_samp, v_samp


def _three(v, what: str) -> Tuple[int, int, int]:
    if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
        return (int(v),) * 3
    if isinstance(v, (list, tuple)) and len(v) == 3 and all(isinstance(e, (int, np.integer)) and not isinstance(e, bool) for e in v):
        return tuple(int(e) for e in v)
    raise ValueError(f"{what}: an integer, or three (Y, U, V), not {v!r}")


@dataclass(frozen=True)
class Layer:
    """one layer: the rectangle `rect` = (sx, sy, w, h) in luma samples (None: the whole picture) of picture `source` of the call's flat
    list lands with its top-left at `at` = (dx, dy) of the target and replaces (PUT) or joins (ADD) what lies below, times `weight`
    (an integer, or three: Y, U, V)"""
    source: int
    mode: int = PUT
    weight: Union[int, Tuple[int, int, int]] = 1
    rect: Optional[Tuple[int, int, int, int]] = None
    at: Tuple[int, int] = (0, 0)

    def weights(self) -> Tuple[int, int, int]:
        return _three(self.weight, "weight")

    def numbers(self) -> Tuple[int, ...]:
        """the ten dwords of an HvqComposeLayer: mode, sx, sy, w, h, dx, dy, weight[3] (kept with the layer, which cannot change)"""
        n = self.__dict__.get("_numbers")
        if n is None:
            r = (0, 0, 0, 0) if self.rect is None else tuple(int(v) for v in self.rect)
            n = self.__dict__["_numbers"] = (int(self.mode),) + r + (int(self.at[0]), int(self.at[1])) + self.weights()
        return n


@dataclass(frozen=True)
class Target:
    """one composed picture: `size` = (w, h), `sampling` = (h_samp, v_samp), its layers from the lowest to the highest, the shift
    and the bias (an integer, or three: Y, U, V) of the finish"""
    size: Tuple[int, int]
    sampling: Tuple[int, int]
    layers: Tuple[Layer, ...]
    shift: int = 0
    bias: Union[int, Tuple[int, int, int]] = 0

    def biases(self) -> Tuple[int, int, int]:
        return _three(self.bias, "bias")

    def geometry(self) -> Geom:
        return (int(self.size[0]), int(self.size[1]), int(self.sampling[0]), int(self.sampling[1]))


def check_layer(layer: Layer) -> None:
    """hvq_compose_check"""
    if not isinstance(layer, Layer):
        raise ValueError(f"a layer is a compose.Layer, not {type(layer).__name__}")
    if layer.mode not in (PUT, ADD):
        raise ValueError(f"layer: mode {layer.mode}")
    if layer.rect is not None and len(layer.rect) != 4:
        raise ValueError(f"layer: rect {layer.rect!r} is (sx, sy, w, h) or None")
    if len(layer.at) != 2:
        raise ValueError(f"layer: at {layer.at!r} is (dx, dy)")
    _mode, sx, sy, w, h, dx, dy = layer.numbers()[:7]
    if min(sx, sy, w, h, dx, dy) < 0:
        raise ValueError(f"layer: a negative number in {sx}, {sy}, {w} x {h} -> {dx}, {dy}")
    if w == 0 and (sx or sy or h):
        raise ValueError("layer: w == 0 means the whole source and takes sx, sy and h as 0")
    if w > 0 and h == 0:
        raise ValueError(f"layer: the rectangle {w} x {h} is empty")
    if max(abs(v) for v in layer.weights()) >= 1 << 31:
        raise ValueError("layer: a weight is a 32-bit integer")


def _rect(layer: Layer, g: Geom) -> Tuple[int, int, int, int]:
    return (0, 0, g[0], g[1]) if layer.rect is None or layer.rect[2] == 0 else tuple(int(v) for v in layer.rect)


def check(target: Target, geoms: Sequence[Geom]) -> None:
    """what hvq_compose_pictures refuses of one target whose layers index pictures of the geometries `geoms`, as ValueError in the
    library's words"""
    if not isinstance(target, Target):
        raise ValueError(f"a target is a compose.Target, not {type(target).__name__}")
    w, h, hs, vs = target.geometry()
    if (hs, vs) not in sc.SAMPLINGS:
        raise ValueError(f"sampling {(hs, vs)}: one of {sc.SAMPLINGS}")
    if w < 8 or h < 8 or w % 8 or h % 8 or w > 8192 or h > 8192:
        raise ValueError(f"target {w}x{h}: multiples of 8 up to 8192")
    if not 0 <= target.shift <= MAX_SHIFT:
        raise ValueError(f"shift {target.shift} outside 0 .. {MAX_SHIFT}")
    for b in target.biases():
        if not -255 <= b <= 255:
            raise ValueError(f"bias {b} outside -255 .. 255")
    if len(target.layers) > MAX_LAYERS:
        raise ValueError(f"{len(target.layers)} layers, a target takes {MAX_LAYERS} at the most")
    gain = [0, 0, 0]
    for k, layer in enumerate(target.layers):
        check_layer(layer)
        if not 0 <= layer.source < len(geoms):
            raise ValueError(f"layer {k}: source {layer.source} of {len(geoms)} pictures")
        g = geoms[layer.source]
        sx, sy, rw, rh = _rect(layer, g)
        dx, dy = int(layer.at[0]), int(layer.at[1])
        if sx + rw > g[0] or sy + rh > g[1]:
            raise ValueError(f"layer {k}: the rectangle {sx}, {sy}, {rw} x {rh} leaves the {g[0]} x {g[1]} source")
        if (sx | rw | dx) % g[2] or (sy | rh | dy) % g[3]:
            raise ValueError(f"layer {k}: {sx}, {sy}, {rw} x {rh} -> {dx}, {dy} does not lie on the chroma samples of its source")
        if tuple(g[2:]) != (hs, vs):
            raise ValueError(f"layer {k}: its source has not the target's sampling {hs} x {vs} (scale it first)")
        if dx + rw > w or dy + rh > h:
            raise ValueError(f"layer {k}: {rw} x {rh} at {dx}, {dy} leaves the {w} x {h} target")
        for p, v in enumerate(layer.weights()):
            gain[p] += abs(v)
    for p in range(3):
        if gain[p] > MAX_GAIN:
            raise ValueError(f"plane {p}: a gain of {gain[p]} (at most {MAX_GAIN})")


def check_call(targets: Sequence[Target], geoms: Sequence[Geom]):
    """check() of every target of a call at once, vectorised over the layers of the call -> (int32 [layers] the picture of every
    layer, int32 [layers, 10] the layers' numbers, int32 [targets, 10] per target width, height, h_samp, v_samp, first, count, shift,
    bias[3]): the layers of the targets one target behind the other.  What a target is refused for is found here and said by check()"""
    def refuse(t):
        check(t, geoms)
        raise ValueError("a target that hvq_compose_pictures refuses")
    for t in targets:
        if type(t) is not Target:
            check(t, geoms)
    counts = [len(t.layers) for t in targets]
    flat = [l for t in targets for l in t.layers]
    nt, nl = len(targets), len(flat)
    try:
        rows = np.array([t.geometry() + (0, 0, t.shift) + t.biases() for t in targets], dtype=np.int64).reshape(nt, 10)
        if any(type(l) is not Layer for l in flat):
            raise TypeError
        source = np.array([l.source for l in flat], dtype=np.int64).reshape(nl)
        nums = np.array([l.numbers() for l in flat], dtype=np.int64).reshape(nl, 10)
    except (TypeError, ValueError, OverflowError):
        for t in targets:
            check(t, geoms)
        raise
    rows[:, 5] = counts
    rows[:, 4] = np.cumsum(rows[:, 5]) - rows[:, 5]
    w, h, hs, vs, shift = (rows[:, i] for i in (0, 1, 2, 3, 6))
    bad = ~(((hs == 2) & (vs == 2)) | ((hs == 2) & (vs == 1)) | ((hs == 1) & (vs == 1)))
    bad |= (w < 8) | (h < 8) | (w % 8 != 0) | (h % 8 != 0) | (w > 8192) | (h > 8192) | (shift < 0) | (shift > MAX_SHIFT) | (rows[:, 5] > MAX_LAYERS)
    bad |= (np.abs(rows[:, 7:10]) > 255).any(axis=1)
    if bad.any():
        refuse(targets[int(np.flatnonzero(bad)[0])])
    if nl:
        of = np.repeat(np.arange(nt), counts)
        g = np.array(geoms, dtype=np.int64).reshape(len(geoms), 4)
        lbad = (source < 0) | (source >= len(geoms))
        if not lbad.any():
            gw, gh, ghs, gvs = (g[source, i] for i in range(4))
            mode, sx, sy, rw, rh, dx, dy = (nums[:, i] for i in range(7))
            lbad = ((mode != PUT) & (mode != ADD)) | (nums[:, 1:7].min(axis=1) < 0) | ((rw == 0) & ((sx | sy | rh) != 0)) | ((rw > 0) & (rh == 0))
            lbad |= (np.abs(nums[:, 7:10]) >= 1 << 31).any(axis=1)
            whole = rw == 0
            rw, rh = np.where(whole, gw, rw), np.where(whole, gh, rh)
            lbad |= (sx + rw > gw) | (sy + rh > gh) | ((sx | rw | dx) % ghs != 0) | ((sy | rh | dy) % gvs != 0)
            lbad |= (ghs != hs[of]) | (gvs != vs[of]) | (dx + rw > w[of]) | (dy + rh > h[of])
        if lbad.any():
            refuse(targets[int(of[np.flatnonzero(lbad)[0]])])
        for p in range(3):
            gain = np.bincount(of, weights=np.abs(nums[:, 7 + p]).astype(np.float64), minlength=nt)      # exact: below 2^53
            if (gain > MAX_GAIN).any():
                refuse(targets[int(np.flatnonzero(gain > MAX_GAIN)[0])])
    return source.astype(np.int32), nums.astype(np.int32), rows.astype(np.int32)


def body(sx: int, dx: int, w: int) -> int:
    """ALIGNED or GENERAL: the body of the kernel a plane of a layer takes, from its numbers in samples of the plane (hvq_cp_body): aligned
    when dx, w and sx - dx are multiples of 4; the values do not depend on it"""
    return ALIGNED if (dx | w | (sx - dx)) & 3 == 0 else GENERAL


def nbytes(target: Target) -> int:
    return sc.nbytes(*target.geometry())


def of_pictures(pictures, geoms: Sequence[Geom], target: Target) -> np.ndarray:
    """the expected bytes of hvq_compose_pictures for one target: pictures[i] is the slot-layout buffer of the call's picture i, of
    geometry geoms[i] -> uint8 [nbytes(target)]"""
    check(target, geoms)
    w, h, hs, vs = target.geometry()
    views = {}
    out = []
    half = (1 << (target.shift - 1)) if target.shift else 0
    for p in range(3):
        xs, ys = (hs, vs) if p else (1, 1)
        acc = np.zeros((h // ys, w // xs), dtype=np.int64)
        for layer in target.layers:
            i = layer.source
            if i not in views:
                views[i] = sc.planes(pictures[i], *geoms[i])
            sx, sy, rw, rh = _rect(layer, geoms[i])
            dx, dy = layer.at
            s = views[i][p][sy // ys:(sy + rh) // ys, sx // xs:(sx + rw) // xs].astype(np.int64) * layer.weights()[p]
            d = acc[dy // ys:(dy + rh) // ys, dx // xs:(dx + rw) // xs]
            if layer.mode == PUT:
                d[...] = s
            else:
                d += s
        out.append(np.clip(((acc + half) >> target.shift) + target.biases()[p], 0, 255).astype(np.uint8).reshape(-1))
    return np.concatenate(out)


def flat_picture(size: Tuple[int, int], sampling: Tuple[int, int], colour=(16, 128, 128)) -> np.ndarray:
    """the bytes of a picture of one colour (Y, U, V): the lowest layer of a target whose background is not its bias"""
    y, u, v = sc.plane_bytes(size[0], size[1], *sampling)
    return np.concatenate([np.full(n, c, dtype=np.uint8) for n, c in zip((y, u, v), colour)])


# ---- builders: each returns a Target; `geom` = (w, h, h_samp, v_samp) of the sources, which index the call's flat pictures

def copy(geom: Geom, source: int = 0) -> Target:
    """the picture itself"""
    return Target(tuple(geom[:2]), tuple(geom[2:]), (Layer(source),))


def mosaic(cols: int, rows: int, cell: Tuple[int, int], sampling: Tuple[int, int], gap: int = 0, background=(16, 128, 128),
           sources: Optional[Sequence[int]] = None, flat: Optional[int] = None) -> Target:
    """a contact sheet: cols x rows cells of cell = (w, h), `gap` luma samples between them, cell k (row by row) from picture
    sources[k] (default: k; fewer than cols * rows leave the last cells empty).  The sheet is as wide and high as the cells and gaps
    need, rounded up to multiples of 8.  Where no cell lies the sheet shows `background`: from picture `flat` of the call, a flat
    picture of the sheet's geometry that goes below the cells (flat_picture), or, with flat None, from the bias -- which serves only
    where no cell lies anywhere (no sources) or the background is (0, 0, 0), because the bias joins the cells too."""
    if cols < 1 or rows < 1 or cols * rows > MAX_LAYERS - (flat is not None):
        raise ValueError(f"{cols} x {rows} cells: 1 .. {MAX_LAYERS} layers")
    cw, ch = cell
    hs, vs = sampling
    if gap < 0 or gap % hs or gap % vs:
        raise ValueError(f"gap {gap}: a multiple of the sampling {hs} x {vs}, 0 at least")
    r8 = lambda v: (v + 7) // 8 * 8
    size = (r8(cols * cw + (cols - 1) * gap), r8(rows * ch + (rows - 1) * gap))
    src = list(range(cols * rows)) if sources is None else list(sources)
    if len(src) > cols * rows:
        raise ValueError(f"{len(src)} pictures for {cols * rows} cells")
    whole = size == (cols * cw, rows * ch) and len(src) == cols * rows
    bg = tuple(int(v) for v in background)
    if flat is None and not whole and bg != (0, 0, 0) and src:
        raise ValueError("a background other than (0, 0, 0) beside the cells needs a flat picture below them (flat=, flat_picture)")
    layers = [] if flat is None else [Layer(flat)]
    layers += [Layer(s, PUT, 1, None, ((k % cols) * (cw + gap), (k // cols) * (ch + gap))) for k, s in enumerate(src)]
    return Target(size, tuple(sampling), tuple(layers), 0, bg if not src and flat is None else 0)


def side_by_side(geom: Geom, left: int = 0, right: int = 1) -> Target:
    """two pictures of one geometry next to each other"""
    w, h, hs, vs = geom
    return Target((2 * w, h), (hs, vs), (Layer(left), Layer(right, at=(w, 0))))


def inset(geom: Geom, x: int, y: int, rect: Optional[Tuple[int, int, int, int]] = None, base: int = 0, small: int = 1) -> Target:
    """picture in picture: picture `small` (or its rectangle `rect`) with its top-left at (x, y) of picture `base`"""
    return Target(tuple(geom[:2]), tuple(geom[2:]), (Layer(base), Layer(small, rect=rect, at=(x, y))))


def crossfade(geom: Geom, t: float, bits: int = 8, a: int = 0, b: int = 1) -> Target:
    """(1 - t) a + t b with t rounded to `bits` bits: weights 2^bits - k and k, k = round(t 2^bits), one rounding"""
    if not 0 <= t <= 1 or not 1 <= bits <= MAX_SHIFT:
        raise ValueError(f"t {t} in 0 .. 1, bits {bits} in 1 .. {MAX_SHIFT}")
    k = int(np.floor(t * (1 << bits) + 0.5))
    return Target(tuple(geom[:2]), tuple(geom[2:]), (Layer(a, ADD, (1 << bits) - k), Layer(b, ADD, k)), bits)


def average_weights(n: int, bits: int = 16) -> Tuple[int, ...]:
    """n integer weights that sum to exactly 2^bits: every weight but the middle one is 2^bits / n rounded to nearest, the middle one
    takes the rest (the construction of filters.gaussian_taps)"""
    if not 1 <= n <= MAX_LAYERS or not 8 <= bits <= MAX_SHIFT:
        raise ValueError(f"{n} pictures (1 .. {MAX_LAYERS}), {bits} bits (8 .. {MAX_SHIFT})")
    side = ((1 << bits) + n // 2) // n
    w = [side] * n
    w[n // 2] = (1 << bits) - side * (n - 1)
    return tuple(w)


def average(geom: Geom, n: int, bits: int = 16) -> Target:
    """the mean of pictures 0 .. n - 1, one rounding"""
    return Target(tuple(geom[:2]), tuple(geom[2:]), tuple(Layer(i, ADD, w) for i, w in enumerate(average_weights(n, bits))), bits)


def difference(geom: Geom, gain: int = 1, a: int = 0, b: int = 1) -> Target:
    """gain (a - b) + 128, clamped: the visible difference of two pictures"""
    return Target(tuple(geom[:2]), tuple(geom[2:]), (Layer(a, ADD, gain), Layer(b, ADD, -gain)), 0, 128)


def overlay(geom: Geom, x: int, y: int, size: Tuple[int, int], alpha: int, base: int = 0, top: int = 1) -> Target:
    """the top-left size = (w, h) of picture `top` blended with alpha / 256 over the region at (x, y) of picture `base`:
    (base (256 - alpha) + top alpha + 128) >> 8 there with one rounding, base elsewhere"""
    if not 0 <= alpha <= 256:
        raise ValueError(f"alpha {alpha} outside 0 .. 256")
    w, h = size
    return Target(tuple(geom[:2]), tuple(geom[2:]),
                  (Layer(base, PUT, 256), Layer(base, PUT, 256 - alpha, (x, y, w, h), (x, y)), Layer(top, ADD, alpha, (0, 0, w, h), (x, y))), 8)


def luma_only(geom: Geom, source: int = 0) -> Target:
    """the picture in grey: Y copied, U and V 128"""
    return Target(tuple(geom[:2]), tuple(geom[2:]), (Layer(source, PUT, (1, 0, 0)),), 0, (0, 128, 128))
