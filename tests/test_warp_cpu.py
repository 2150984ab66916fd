"""CPU: the values of hvq_warp_pictures.  tests/warp_ref.py restates include/hvqm4_amd.h in plain Python; hvqm4_amd.warp (numpy), the
fixture tests/golden/warp.json and the runtime on the CPU fake device (tests/native/fake_warp.cpp, which walks the kernel's grid and
phases with the kernel's own arithmetic of hvq_warp.h) are compared with it by ==.  The fake-device driver is a stand-alone program,
built and run plain and with ASan + UBSan as tests/test_filters_cpu.py builds its own; nothing is preloaded and no Python is involved
in the sanitised run."""
import hashlib
import json
import os
import zlib
from fractions import Fraction

import numpy as np
import pytest

import tests.test_fake_device as fd
from hvqm4_amd import warp as W
from tests import warp_ref as ref

NATIVE = fd.NATIVE
CXX_SOURCES = [s for s in fd.CXX_SOURCES if os.path.basename(s) != "fake_driver.cpp"] + \
              [os.path.join(NATIVE, "fake_warp.cpp"), os.path.join(NATIVE, "fake_warp_driver.cpp")]
FIXTURE = json.load(open(os.path.join(fd.GOLDEN, "warp.json")))
SAMPLINGS = ((2, 2), (2, 1), (1, 1))
T_MAX = (1 << 31) - 1
M_MAX = 1 << 21


def _centre(w, h):
    return (Fraction(w, 2), Fraction(h, 2))


def _maps(w, h):
    """name -> (Warp, target (w, h) or None for the source's): the maps of the seams, known, border and extreme cases for a w x h source"""
    c = _centre(w, h)
    out = {"identity": (W.identity(), None), "flip_h": (W.flip_h(w), None), "flip_v": (W.flip_v(h), None), "transpose": (W.transpose(), (h, w)),
           "half_shift": (W.translate(Fraction(-1, 2), 0), None), "reduce2": (W.zoom(Fraction(1, 2), 1), None), "shift_3_-5": (W.translate(3, -5), None),
           "shift_const": (W.with_border(W.translate(-2, 1), W.CONSTANT, (7, 99, 201)), None), "shear": (W.shear(Fraction(1, 4), Fraction(-1, 8), c), None),
           "negdet": (W.compose(W.flip_h(w), W.rotate(20, w, h)), None), "zero": (W.with_border(W.Warp(0, 0, 0, 0, 3 * 65536 + 77, 2 * 65536 + 200), W.REPLICATE), None)}
    for k in (1, 2, 3):
        t, size = W.rotate90(k, w, h)
        out[f"turn{k}"] = (t, size)
    for d in (Fraction(1, 2), 30, 45, Fraction(179, 2)):
        out[f"rot{float(d)}"] = (W.rotate(d, w, h), None)
        out[f"rot{float(d)}_const"] = (W.with_border(W.rotate(d, w, h), W.CONSTANT, (16, 240, 3)), None)
    for z in (Fraction(3, 4), Fraction(3, 2), 3, Fraction(1, 2)):
        out[f"zoom{float(z)}"] = (W.zoom(z, centre=c), None)
    # footprints wholly outside on each of the four sides, and straddling each edge and corner
    for name, (dx, dy) in {"out_left": (w + 3, 0), "out_right": (-w - 3, 0), "out_top": (0, h + 3), "out_bottom": (0, -h - 3), "edge_l": (Fraction(5, 2), 0),
                           "edge_r": (Fraction(-5, 2), 0), "edge_t": (0, Fraction(7, 4)), "edge_b": (0, Fraction(-7, 4)), "corner_tl": (Fraction(3, 2), Fraction(5, 4)),
                           "corner_br": (Fraction(-3, 2), Fraction(-5, 4)), "corner_tr": (Fraction(-9, 4), Fraction(1, 2)), "corner_bl": (Fraction(1, 4), Fraction(-11, 4))}.items():
        out[name] = (W.translate(dx, dy), None)
        out[name + "_const"] = (W.with_border(W.translate(dx, dy), W.CONSTANT, (1, 2, 3)), None)
    # the extremes: |m| = 2^21 on each coefficient alone, t = +-(2^31 - 1)
    for i, nm in enumerate(("m00", "m01", "m10", "m11")):
        for sgn in (1, -1):
            m = [0, 0, 0, 0]
            m[i] = sgn * M_MAX
            out[f"{nm}_{'max' if sgn > 0 else 'min'}"] = (W.Warp(m[0], m[1], m[2], m[3], 65536 * (w // 2) + 1234, 65536 * (h // 2) - 999, W.CONSTANT, (9, 8, 7)), None)
    for sgn in (1, -1):
        for b in (W.REPLICATE, W.CONSTANT):
            out[f"t0_{sgn}_{b}"] = (W.Warp(65536, 0, 0, 65536, sgn * T_MAX, 0, b, (50, 60, 70)), None)
            out[f"t1_{sgn}_{b}"] = (W.Warp(65536, 0, 0, 65536, 0, sgn * T_MAX, b, (50, 60, 70)), None)
            out[f"t_both_{sgn}_{b}"] = (W.Warp(-M_MAX, M_MAX, M_MAX, -M_MAX, sgn * T_MAX, -sgn * T_MAX, b, (50, 60, 70)), None)
    return out


def _picture(g, seed):
    return np.random.default_rng(seed).integers(0, 256, W.nbytes(*g), dtype=np.uint8)


def _both(pic, g, w, tg=None):
    got = W.of_picture(pic, g, w, tg)
    assert ref.warp_picture(pic.tobytes(), g, ref.as_ref(w), tg) == got.tobytes()
    return got


@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_module_equals_reference(sampling):
    """every map of the cases on 24 x 16 (chroma 12 or 24 wide) into the source's geometry, a turned one and another sampling"""
    g = (24, 16) + sampling
    pic = _picture(g, 1)
    for name, (w, size) in _maps(24, 16).items():
        tg = (size or g[:2]) + sampling
        _both(pic, g, w, tg)
    for other in SAMPLINGS:                                       # warp plus resize plus another sampling in one call
        _both(pic, g, W.rotate(30, 24, 16), (16, 8) + other)
        _both(pic, g, W.identity(), (24, 16) + other)


def test_known_answers():
    for s in SAMPLINGS:
        for wh in ((8, 8), (72, 24)):
            g = wh + s
            pic = _picture(g, 2)
            assert np.array_equal(W.of_picture(pic, g, W.identity()), pic), "the identity copies every plane in every sampling"
            pl = W.planes(pic, *g)
            got = W.planes(W.of_picture(pic, g, W.flip_h(g[0])), *g)
            assert all(np.array_equal(a[:, ::-1], b) for a, b in zip(pl, got)), "the exact mirror, in 2:1-sampled chroma alike"
            got = W.planes(W.of_picture(pic, g, W.flip_v(g[1])), *g)
            assert all(np.array_equal(a[::-1], b) for a, b in zip(pl, got))
            if s[0] == s[1]:
                tg = (g[1], g[0]) + s
                got = W.planes(W.of_picture(pic, g, W.transpose(), tg), *tg)
                assert all(np.array_equal(a.T, b) for a, b in zip(pl, got)), "the exact transpose"
                for k in (1, 2, 3):
                    t, size = W.rotate90(k, *wh)
                    got = W.planes(W.of_picture(pic, g, t, size + s), *(size + s))
                    assert all(np.array_equal(np.rot90(a, k), b) for a, b in zip(pl, got)), f"quarter turn {k}"
            flat = np.full(W.nbytes(*g), 201, dtype=np.uint8)
            for w, _size in _maps(*wh).values():
                if w.border == W.REPLICATE:
                    assert bool((W.of_picture(flat, g, w) == 201).all()), "a flat picture stays flat under REPLICATE"
    g = (24, 8, 1, 1)
    pic = _picture(g, 3)
    y = W.planes(pic, *g)[0].astype(int)
    half = W.Warp(t0=32768)
    assert half == W.translate(Fraction(-1, 2), 0)
    got = W.planes(_both(pic, g, half), *g)[0]
    assert np.array_equal(got[:, :-1], (y[:, :-1] + y[:, 1:] + 1) >> 1) and np.array_equal(got[:, -1], y[:, -1])
    red = W.Warp(m00=131072)
    got = W.planes(_both(pic, g, red, (8, 8, 1, 1)), 8, 8, 1, 1)[0]
    assert np.array_equal(got[:, :8], (y[:, 0:16:2] + y[:, 1:16:2] + 1) >> 1)
    mirror = W.Warp(m00=-65536, t0=65536 * 24)
    assert mirror == W.flip_h(24) and W.Warp(0, 65536, 65536, 0) == W.transpose()
    # integer translations against index arithmetic under both borders
    sh = W.translate(3, -5)
    got = W.planes(_both(pic, g, sh), *g)[0]
    xs, ys = np.clip(np.arange(24) - 3, 0, 23), np.clip(np.arange(8) + 5, 0, 7)
    assert np.array_equal(got, y[ys][:, xs])
    got = W.planes(_both(pic, g, W.with_border(sh, W.CONSTANT, (77, 0, 0))), *g)[0]
    want = np.full((8, 24), 77)
    want[:3, 3:] = y[5:, :21]
    assert np.array_equal(got, want)
    # an all-zero linear part is a constant picture
    z = W.Warp(0, 0, 0, 0, 5 * 65536 + 32768, 2 * 65536 + 32768)
    assert set(W.planes(_both(pic, g, z), *g)[0].reshape(-1).tolist()) == {int(y[2, 5])}


def test_saturating_the_positions_changes_no_value():
    """U8 to [-512, 256 Nx], V8 to [-512, 256 Ny]: at t = +-(2^31 - 1) and |m| = 2^21, and on every other map"""
    for s in SAMPLINGS:
        g = (24, 16) + s
        pic = _picture(g, 4)
        hit = 0
        for name, (w, size) in _maps(24, 16).items():
            tg = (size or g[:2]) + s
            assert np.array_equal(W.of_picture(pic, g, w, tg), W.of_picture(pic, g, w, tg, saturate=True)), name
            u, v = W.coords(w, g, tg, 1)
            hit += int(u.min() < -512 or u.max() > 256 * 24 or v.min() < -512 or v.max() > 256 * 16)
        assert hit >= 20, "the saturation was met"
    w = W.Warp(M_MAX, 0, 0, M_MAX, T_MAX, -T_MAX)
    u, v = W.coords(w, (8192, 8, 2, 2), (8192, 8, 2, 2), 0)
    assert int(u.max()) << 9 > 1 << 35 and int(v.min()) << 9 < -(1 << 31), "NU and NV need 64 bits before the shift and the saturation"


def test_struct_layout():
    import ctypes as C
    from hvqm4_amd._lib import HvqWarp, HvqWarpDst
    assert (C.sizeof(HvqWarp), C.sizeof(HvqWarpDst)) == (32, 24)
    assert (HvqWarp.border.offset, HvqWarp.fill.offset, HvqWarp.pad.offset, HvqWarpDst.width.offset, HvqWarpDst.v_samp.offset) == (24, 28, 31, 8, 20)
    s = W.with_border(W.Warp(1, -2, 3, -4, 5, -6), W.CONSTANT, (7, 8, 9)).to_struct()
    assert (s.m00, s.m01, s.m10, s.m11, s.t0, s.t1, s.border, list(s.fill), s.pad) == (1, -2, 3, -4, 5, -6, 1, [7, 8, 9], 0)
    assert W.Warp().fill == (0, 128, 128)


def test_builders():
    w, h = 72, 24
    for a in (W.flip_h(w), W.flip_v(h), W.rotate90(2, w, h)[0]):
        assert W.invert(a) == a and W.compose(a, a) == W.identity()
    assert W.invert(W.transpose()) == W.transpose() and W.compose(W.transpose(), W.transpose()) == W.identity()
    t1, s1 = W.rotate90(1, w, h)
    t3, s3 = W.rotate90(3, *s1)
    assert s1 == (h, w) and s3 == (w, h) and W.compose(t1, t3) == W.identity() and W.invert(t1) == t3
    assert W.compose(t1, W.rotate90(1, *s1)[0]) == W.rotate90(2, w, h)[0]
    assert W.compose(W.compose(t1, W.rotate90(1, *s1)[0]), W.compose(W.rotate90(1, w, h)[0], W.rotate90(1, *s1)[0])) == W.identity()
    assert W.compose(W.flip_h(w), W.flip_v(h)) == W.rotate90(2, w, h)[0]
    assert W.compose(W.transpose(), W.flip_v(w)) == t1, "a transpose, then upside down, is the quarter turn counter-clockwise"
    assert W.rotate90(0, w, h) == (W.identity(), (w, h)) and W.rotate90(5, w, h) == W.rotate90(1, w, h)
    assert W.rotate(90, 24, 24) == W.rotate90(1, 24, 24)[0] and W.rotate(180, w, h) == W.rotate90(2, w, h)[0] and W.rotate(0, w, h) == W.identity()
    assert W.compose(W.translate(3, -5), W.translate(-3, 5)) == W.identity() and W.invert(W.translate(3, -5)) == W.translate(-3, 5)
    assert W.translate(3, -5).coefficients() == (65536, 0, 0, 65536, -3 * 65536, 5 * 65536)
    assert W.from_motion((-5, 3)) == W.translate(-3, 5), "the picture at (y, x) looks like the reference at (y + dy, x + dx)"
    assert W.zoom(2).m00 == 32768 and W.zoom(Fraction(1, 2)).m00 == 131072 and W.invert(W.zoom(2)) == W.zoom(Fraction(1, 2))
    assert W.zoom(2, centre=(36, 12)).t0 == 18 * 65536
    assert W.affine([[1, 0, 3], [0, 1, -5]]) == W.translate(3, -5) and W.affine([[0, 1, 0], [1, 0, 0]]) == W.transpose()
    assert W.shear(Fraction(1, 4)).coefficients() == (65536, -16384, 0, 65536, 0, 0)
    assert W.invert(W.shear(Fraction(1, 4))) == W.shear(Fraction(-1, 4))
    r = W.rotate(30, w, h)
    assert abs(r.m00 - round(65536 * np.cos(np.pi / 6))) <= 1 and r.m01 == -32768 or abs(r.m01 + 32768) <= 1
    b = W.with_border(r, W.CONSTANT, (1, 2, 3))
    assert (b.border, b.fill, b.coefficients()) == (W.CONSTANT, (1, 2, 3), r.coefficients()) and W.compose(W.identity(), b).fill == (1, 2, 3)
    assert len({W.identity(), W.Warp(), W.flip_h(8)}) == 2
    for bad in (lambda: W.invert(W.Warp(0, 0, 0, 0)), lambda: W.zoom(0), lambda: W.zoom(Fraction(1, 64)), lambda: W.check(W.Warp(m01=M_MAX + 1)),
                lambda: W.check(W.Warp(border=2)), lambda: W.check(W.Warp(fill=(0, 0, 256))), lambda: W.check(W.Warp(t0=1 << 31)), lambda: W.translate(40000, 0),
                lambda: W.check(W.Warp(m00=1.0)), lambda: W.affine([[1, 0, 0]]), lambda: W.check("turn"), lambda: W.of_picture(np.zeros(96, np.uint8), (8, 8, 2, 2), W.identity(), (12, 8, 2, 2))):
        with pytest.raises(ValueError):
            bad()


def test_body_mirrors_the_library():
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, lib
    seen = set()
    for g in ((640, 480, 2, 2), (136, 40, 2, 1), (8, 8, 1, 1), (8192, 8, 2, 2)):
        for name, (w, size) in _maps(*g[:2]).items():
            for p in (0, 1):
                (hd, vd), (hs, vs) = W._samplings(g, g, p)
                nx, ny = W.plane_dims(g, p)
                got = lib().hvq_warp_body(C.byref(w.to_struct()), hd, vd, hs, vs, nx, ny)
                assert got == W.body(w, g, g, p), (g, name, p)
                seen.add(got)
    assert seen == {W.DIRECT, W.TILED}
    g = (640, 480, 2, 2)
    assert W.body(W.rotate90(1, 640, 480)[0], g, (480, 640, 2, 2), 0) == W.TILED, "the body for turns"
    assert W.body(W.identity(), g, g, 0) == W.DIRECT and W.body(W.zoom(Fraction(1, 32)), g, g, 0) == W.DIRECT, "a footprint LDS cannot hold"
    s = W.identity().to_struct()
    assert lib().hvq_warp_body(None, 1, 1, 1, 1, 8, 8) == HVQ_E_ARG and lib().hvq_warp_body(C.byref(s), 3, 1, 1, 1, 8, 8) == HVQ_E_ARG
    assert lib().hvq_warp_body(C.byref(s), 1, 1, 1, 1, 0, 8) == HVQ_E_ARG and lib().hvq_warp_body(C.byref(s), 1, 1, 1, 1, 8, 8193) == HVQ_E_ARG


# ------------------------------------------------------------------------------------------------- the fixture
def _clip_geometry(name):
    from hvqm4_amd.container import parse_header
    hdr = parse_header(open(os.path.join(fd.GOLDEN, fd.CLIPS[name]["file"]), "rb").read())
    return (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)


def _fixture_warps(geom):
    w, h, hs, vs = geom
    turn, (tw, th) = W.rotate90(1, w, h)
    return [("rotate7_constant", W.with_border(W.rotate(7, w, h), W.CONSTANT), geom), ("rotate90", turn, (tw, th, hs, vs)),
            ("zoom3/4_replicate", W.zoom(Fraction(3, 4), centre=_centre(w, h)), geom)]


def test_fixture_covers_every_golden_clip():
    assert set(FIXTURE["clips"]) == set(fd.CLIPS)
    for name, entry in FIXTURE["clips"].items():
        assert tuple(entry["geometry"]) == _clip_geometry(name)
        assert [(l, tuple(t)) for l, t, _c in entry["warps"]] == [(l, t) for l, _w, t in _fixture_warps(_clip_geometry(name))]


@pytest.mark.parametrize("name", sorted(FIXTURE["clips"]))
def test_fixture_equals_reference_and_module(name):
    entry = FIXTURE["clips"][name]
    g = tuple(entry["geometry"])
    pic = fd.oracle_pictures(name)[-1]
    assert hashlib.sha256(pic.tobytes()).hexdigest() == fd.CLIPS[name]["picture_sha256"][-1], "the fixture describes the manifest's picture"
    for (label, tg, crc), (label2, w, tg2) in zip(entry["warps"], _fixture_warps(g)):
        assert label == label2 and tuple(tg) == tg2
        got = W.of_picture(pic, g, w, tg2)
        assert zlib.crc32(got.tobytes()) == crc, (name, label)
        if g[0] * g[1] <= 64 * 48:                                          # plain Python: the small clips, every sampling among them
            assert ref.warp_picture(pic.tobytes(), g, ref.as_ref(w), tg2) == got.tobytes(), (name, label)


def test_the_reference_meets_clips_of_every_sampling():
    small = {tuple(e["geometry"])[2:] for e in FIXTURE["clips"].values() if e["geometry"][0] * e["geometry"][1] <= 64 * 48}
    assert small == {(2, 2), (2, 1), (1, 1)}


# ------------------------------------------------------------------------------------------------- argument checks without a device
class _NoDevice:
    """what Context.warp_pictures looks at before it reaches the library"""
    _geom = {0: (64, 48), 1: (24, 40), 2: (64, 48)}
    _h = None

    def __init__(self):
        self._geom4 = {}

    @staticmethod
    def pic_bytes(sid):
        return {0: 64 * 48 * 3 // 2, 1: 24 * 40 * 3 // 2, 2: 64 * 48 * 3}[sid]

    def _geometry(self, sid):
        from hvqm4_amd.batch import Context
        return Context._geometry(self, sid)


def test_arguments_are_checked_before_the_library_is_called():
    import torch
    from hvqm4_amd._lib import HVQ_E_ARG, HvqError
    from hvqm4_amd.batch import Context
    call = lambda *a, **k: Context.warp_pictures(_NoDevice(), *a, **k)
    w = W.rotate(30, 64, 48)
    nb = 64 * 48 * 3 // 2
    with pytest.raises(ValueError, match="ordinals"):
        call([0, 0], [0], w)
    with pytest.raises(HvqError) as e:
        call([0, 7], [0, 0], w)
    assert e.value.code == HVQ_E_ARG
    for bad in (None, "turn", [w], [w, None], w.coefficients()):
        with pytest.raises(ValueError, match="warp"):
            call([0, 0], [0, 1], bad)
    with pytest.raises(ValueError, match="coefficient"):
        call([0], [0], W.Warp(m10=-M_MAX - 1))
    with pytest.raises(ValueError, match="border"):
        call([0], [0], W.Warp(border=3))
    with pytest.raises(ValueError, match="fill"):
        call([0], [0], W.Warp(fill=(1, 2)))
    with pytest.raises(ValueError, match="target"):
        call([0], [0], w, size=(60, 48))
    with pytest.raises(ValueError, match="target"):
        call([0], [0], w, size=(8200, 48))
    with pytest.raises(ValueError, match="size"):
        call([0, 0], [0, 1], w, size=[(64, 48)])
    with pytest.raises(ValueError, match="sampling"):
        call([0], [0], w, sampling=(1, 2))
    with pytest.raises(ValueError, match="1 sources for 2 pictures"):
        call([0, 0], [0, 1], w, src=[None])
    good = torch.zeros(nb, dtype=torch.uint8)
    with pytest.raises(ValueError, match="elements"):
        call([1], [-1], w, src=[good])
    room = torch.zeros(nb + 64, dtype=torch.uint8)
    off = (-room.data_ptr()) % 16
    with pytest.raises(ValueError, match="ordinal -1"):
        call([0], [0], w, src=[room[off:off + nb]])
    with pytest.raises(ValueError, match="not a GPU"):
        call([0], [-1], w, src=[room[off:off + nb]])
    with pytest.raises(ValueError, match="out must be"):
        call([0, 0], [0, 1], w, out=torch.zeros((2, nb), dtype=torch.int32))
    with pytest.raises(ValueError, match="out must be"):
        call([0, 0], [0, 1], w, out=torch.zeros((2, nb + 16), dtype=torch.uint8))
    with pytest.raises(ValueError, match="out must be"):
        call([0, 0], [0, 1], w, out=[torch.zeros(nb, dtype=torch.uint8)] * 2)                          # one target geometry: one tensor
    with pytest.raises(ValueError, match="out must be a list"):
        call([0, 1], [0, 1], w, out=torch.zeros((2, nb), dtype=torch.uint8))                           # two geometries: a list
    with pytest.raises(ValueError, match=r"out\[1\]"):
        call([0, 1], [0, 1], w, out=[torch.zeros(nb, dtype=torch.uint8)] * 2)
    with pytest.raises(ValueError, match="not a GPU"):                                                  # one target for two source geometries: one tensor
        call([0, 1], [0, 1], w, size=(48, 64), sampling=(1, 1), out=torch.zeros((2, 48 * 64 * 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="not a GPU"):                                                  # the turned size, per picture
        call([0, 1], [0, 1], [W.rotate90(1, 64, 48)[0], W.rotate90(1, 24, 40)[0]], size=[(48, 64), (40, 24)],
             out=[torch.zeros(nb, dtype=torch.uint8), torch.zeros(24 * 40 * 3 // 2, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="multiple of 16"):
        room = torch.zeros(2 * nb + 64, dtype=torch.uint8)
        off = (-room.data_ptr()) % 16 + 8
        call([0, 0], [0, 1], w, out=room[off:off + 2 * nb].view(2, nb))
    with pytest.raises(ValueError, match="65535"):
        call([0] * 65536, [0] * 65536, w)


def test_the_library_without_a_device_still_checks_its_arguments():
    """no context can exist here, and the call says so before it looks at anything else; the host-only check works"""
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, HvqWarpDst, lib
    one = (C.c_int * 1)(0)
    w = W.identity().to_struct()
    dst = HvqWarpDst(16, 8, 8, 2, 2)
    assert lib().hvq_warp_pictures(None, 1, one, one, None, C.byref(w), C.byref(dst), None) == HVQ_E_ARG
    assert lib().hvq_warp_force_direct(None, 1) == HVQ_E_ARG
    assert lib().hvq_warp_check(None) == HVQ_E_ARG
    for name, (m, _size) in _maps(72, 24).items():
        assert lib().hvq_warp_check(C.byref(m.to_struct())) == 0, name
    for field, v in (("m00", 32 * 65536 + 1), ("m01", -32 * 65536 - 1), ("m10", 1 << 30), ("m11", -(1 << 31)), ("border", 2), ("border", -1), ("pad", 1)):
        s = W.identity().to_struct()
        setattr(s, field, v)
        assert lib().hvq_warp_check(C.byref(s)) == HVQ_E_ARG, field
    s = W.Warp(32 * 65536, -32 * 65536, 32 * 65536, -32 * 65536, T_MAX, -T_MAX - 1, W.CONSTANT, (255, 255, 255)).to_struct()
    assert lib().hvq_warp_check(C.byref(s)) == 0, "at the limits"


# ------------------------------------------------------------------------------------------------- the runtime on the CPU fake device
SAME, SWAP = (0, 0, 0, 0), (-1, -1, 0, 0)
DRIVER_WARPS = {                                       # name -> (Warp, target rule); the second and third keep the geometry (the reuse scenario chains them)
    "rot30_const": (W.with_border(W.Warp(56756, -32768, 32768, 56756, 700000, -500000), W.CONSTANT, (16, 240, 3)), SAME),
    "half_shift": (W.translate(Fraction(-1, 2), Fraction(1, 4)), SAME),
    "shear": (W.shear(Fraction(1, 4), Fraction(-1, 8)), SAME),
    "identity": (W.identity(), SAME),
    "transpose": (W.transpose(), SWAP),
    "turn_left": (W.Warp(0, -65536, 65536, 0, 65536 * 48, 0, W.CONSTANT, (200, 100, 50)), SWAP),     # exact on the 48-wide clips, shifted on others
    "rot45_to_104x56": (W.Warp(46341, -46341, 46341, 46341, 20 * 65536, -7 * 65536), (104, 56, 0, 0)),
    "rot89.5": (W.Warp(572, -65534, 65534, 572, 65536 * 40, 3000), SAME),
    "zoom3_to_420": (W.Warp(21845, 0, 0, 21845, 5 * 65536, 3 * 65536), (0, 0, 2, 2)),
    "reduce2_to_444": (W.Warp(131072, 0, 0, 131072, 0, 0, W.CONSTANT, (1, 2, 3)), (24, 16, 1, 1)),
    "negdet_to_422": (W.Warp(-60000, 25000, 20000, 61000, 65536 * 50, -65536 * 4), (0, 0, 2, 1)),
    "zero": (W.Warp(0, 0, 0, 0, 65536 * 5 + 100, 65536 * 2 + 40000), SAME),
    "m10_max": (W.Warp(0, 65536, M_MAX, 0, 0, -65536 * 100, W.CONSTANT, (9, 8, 7)), SAME),
    "m01_min_tmax": (W.Warp(65536, -M_MAX, 0, 65536, T_MAX, 0), SAME),
    "tmin_const": (W.Warp(65536, 0, 0, 65536, 0, -T_MAX, W.CONSTANT, (50, 60, 70)), SAME),
    "reduce40": (W.Warp(40 * 65536 // 2, 0, 0, 65536 * 12, 0, 0), (16, 8, 0, 0)),                   # a footprint LDS cannot hold
    "flip_both_out": (W.Warp(-65536, 0, 0, -65536, 65536 * 30, 65536 * 20, W.CONSTANT, (0, 128, 128)), SAME),
}


def _warps_txt():
    lines = []
    for name, (w, t) in DRIVER_WARPS.items():
        lines.append(" ".join(str(v) for v in (name,) + w.coefficients() + (w.border,) + w.fill + t))
    return "\n".join(lines) + "\n"


def _target(geom, rule):
    w, h, hs, vs = geom
    if rule[0] == -1:
        w, h = h, w
    elif rule[0] > 0:
        w, h = rule[:2]
    if rule[2] > 0:
        hs, vs = rule[2:]
    return (w, h, hs, vs)


@pytest.fixture(scope="module")
def drivers():
    return {kind: fd.build_driver(kind, "warp", "fake_warp_driver", CXX_SOURCES, __file__) for kind in fd.BUILDS}


_want = {}


def _source(source, form, k, geom):
    """the picture the driver warped, as the driver's line describes it"""
    n = W.nbytes(*geom)
    if form == "pic":
        return fd.oracle_pictures(source)[k].reshape(-1)
    if form == "inv":
        return 255 - fd.oracle_pictures(source)[k].reshape(-1)
    if form.startswith("warped:"):
        return _expected(source, "pic", k, geom, form.split(":", 1)[1])[1]
    if form == "synth":
        return ((((np.arange(n, dtype=np.uint64) + np.uint64(k)) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(13)).astype(np.uint8)
    if form == "flat":
        return np.full(n, k, dtype=np.uint8)
    if form == "check":
        w, h, hs, vs = geom
        out = []
        for pw, ph in ((w, h), (w // hs, h // vs), (w // hs, h // vs)):
            y, x = np.mgrid[0:ph, 0:pw]
            out.append((((x + y + k) & 1) * 255).astype(np.uint8).reshape(-1))
        return np.concatenate(out)
    raise AssertionError(form)


def _expected(source, form, k, geom, wname):
    key = (source, form, k, geom, wname)
    if key not in _want:
        w, rule = DRIVER_WARPS[wname]
        got = W.of_picture(_source(source, form, k, geom), geom, w, _target(geom, rule))
        _want[key] = (zlib.crc32(got.tobytes()), got)
    return _want[key]


def _run(exe, scenario, schedule, tmp_path):
    _, lines = fd.run_checked(exe, scenario, schedule, tmp_path, inputs={"warps.txt": _warps_txt()})
    P, R, S = {}, {}, {}
    for line in lines:
        f = line.split()
        if f[0] == "P":
            label, source, form, k, geom, wname, tg = f[1], f[2], f[3], int(f[4]), tuple(int(v) for v in f[5:9]), f[9], tuple(int(v) for v in f[10:14])
            assert int(f[15]) == 1, f"{label}: the bytes around the output of {source} {k} were written"
            assert tg == _target(geom, DRIVER_WARPS[wname][1])
            want = _expected(source, form, k, geom, wname)[0]
            assert int(f[14]) == want, f"{label}: picture {k} of {source} ({form}) {geom} through {wname}: crc {int(f[14]):08x}, want {want:08x}"
            P.setdefault(label, []).append((source, form, k, geom, wname))
        elif f[0] == "R":
            R[f[1]] = int(f[2])
        elif f[0] == "S":
            S[f[1]] = (int(f[2]), int(f[3]))
    return P, R, S


def _check_goldens(P, R, S):
    nf = len(DRIVER_WARPS)
    assert len(P["goldens/all"]) == 6 * nf and {fn for *_r, fn in P["goldens/all"]} == set(DRIVER_WARPS)
    assert {g[2:] for _s, _f, _k, g, _n in P["goldens/all"]} == {(2, 2), (2, 1), (1, 1)}
    assert any(g[0] > 128 and g[1] > 32 for _s, _f, _k, g, _n in P["goldens/all"]), "tile seams inside a plane"
    assert P["goldens/one"] == [P["goldens/all"][1]]
    assert R == {"goldens/n0": 0}


def _check_memory(P, R, S):
    assert P["memory"] == P["memory/nullstream"]
    forms = [f for _s, f, *_r in P["memory"]]
    assert forms.count("inv") == fd.n_pics("yuv422_64x48") and forms.count("check") == 7 * len(DRIVER_WARPS) and forms.count("flat") == 9
    geoms = {g for _s, f, _k, g, _n in P["memory"] if f == "synth"}
    assert {(8, 8, 2, 2), (8, 8, 2, 1), (8, 8, 1, 1), (72, 24, 2, 2), (24, 72, 2, 1), (136, 40, 2, 2), (104, 56, 1, 1), (8192, 8, 2, 2), (8, 8192, 2, 2)} == geoms


def _check_many(P, R, S):
    assert len(P["many"]) == 300 and P["many"] == P["many/again"]
    assert len({s for s, *_r in P["many"]}) == 8 and len({g for _s, _f, _k, g, _n in P["many"]}) >= 4 and len({n for *_r, n in P["many"]}) >= 10


def _check_body(P, R, S):
    assert P["body/chosen"] == P["body/direct"] == P["body/tiled"] == P["body/chosen_again"] and len(P["body/direct"]) == 5 * len(DRIVER_WARPS)
    assert R == {"body/force": 0, "body/force_tiled": 1, "body/unforce": 2}
    chosen = {W.body(DRIVER_WARPS[n][0], g, _target(g, DRIVER_WARPS[n][1]), p) for _s, _f, _k, g, n in P["body/chosen"] for p in (0, 1)}
    assert chosen == {W.DIRECT, W.TILED}, "at least one job chose each body"


def _check_reuse(P, R, S):
    from hvqm4_amd._lib import HVQ_E_STATE
    n, ne = fd.n_pics("gop64x48_15"), fd.n_pics("yuv444_64x48")
    g = _clip_geometry("gop64x48_15")
    names = list(DRIVER_WARPS)
    assert P["reuse"] == [("gop64x48_15", "pic", k, g, names[1]) for k in range(n)]
    assert R["reuse/evicted"] == HVQ_E_STATE, "the flushes did not hand the slots of the first pass on: the scenario tests nothing"
    assert P["reuse/chain"] == [("gop64x48_15", "warped:" + names[1], k, g, names[2]) for k in range(n)]
    assert P["reuse/late"] == P["reuse"]
    assert [(s, k) for s, _f, k, *_r in P["reuse/destroy"]] == [("yuv444_64x48", k) for k in range(ne)]


def _check_refused(P, R, S):
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_GEOMETRY, HVQ_E_STATE
    arg = ["null_context", "bad_stream", "bad_ordinal", "misaligned_src", "src_with_ordinal", "src_with_bad_stream", "minus_one_without_src", "null_ptr",
           "misaligned_ptr", "too_many", "null_warps", "null_dst", "force_null", "check_null"]
    spoiled = ["m00_above", "m01_below", "m10_above", "m11_below", "border_2", "border_negative", "pad"]
    want = {k: HVQ_E_ARG for k in arg + spoiled + ["check_" + s for s in spoiled]}
    want.update({"geometry_width": HVQ_E_GEOMETRY, "geometry_sampling": HVQ_E_GEOMETRY, "geometry_zero": HVQ_E_GEOMETRY})
    want.update({"evicted": HVQ_E_STATE, "queued": HVQ_E_STATE, "n0": 0, "check_good": 0, "check_limits": 0})
    assert R == {"refused/" + k: v for k, v in want.items()}
    same, total = S["refused"]
    assert same == total == 2 * 4608 + 16, "a refused call wrote its output"
    g = _clip_geometry("gop64x48_15")
    names = list(DRIVER_WARPS)
    assert P["refused/then_ok"] == [("gop64x48_15", "pic", 1, g, names[-1]), ("gop64x48_15", "pic", fd.n_pics("gop64x48_15") - 1, g, names[0])]


CHECKS = {"goldens": _check_goldens, "memory": _check_memory, "many": _check_many, "body": _check_body, "reuse": _check_reuse, "refused": _check_refused}


@pytest.mark.parametrize("schedule", ["eager", "late"])
@pytest.mark.parametrize("build", list(fd.BUILDS))
@pytest.mark.parametrize("scenario", list(CHECKS))
def test_fake_device_scenario(drivers, scenario, build, schedule, tmp_path):
    P, R, S = _run(drivers[build], scenario, schedule, tmp_path)
    CHECKS[scenario](P, R, S)


def test_the_existing_fake_builds_link_without_the_warp_body():
    """the source lists of the other drivers have no hvq_launch_warp: the runtime's reference is weak"""
    assert not any("fake_warp" in s for s in fd.CXX_SOURCES)
    text = open(os.path.join(fd.CSRC, "hvq_runtime.cpp")).read()
    decl = [l for l in text.splitlines() if "hvq_launch_warp(" in l and l.startswith("extern")]
    assert len(decl) == 1 and "weak" in decl[0]
