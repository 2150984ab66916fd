"""CPU: the values of hvq_compose_pictures.  tests/compose_ref.py restates include/hvqm4_amd.h in plain Python; hvqm4_amd.compose (numpy),
the committed fixture and the runtime on the CPU fake device (tests/native/fake_compose.cpp walks the kernel's grid with the arithmetic
of hvqm4_amd/csrc/hvq_compose.h) are compared with it by ==.  The fake-device driver is a stand-alone executable, built and run plain
and with ASan + UBSan as tests/test_warp_cpu.py builds its own; nothing is preloaded and no Python is involved in those runs."""
import ctypes as C
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

import tests.test_fake_device as fd
from hvqm4_amd import compose as cp
from hvqm4_amd import scale as sc
from tests import compose_cases as cases
from tests import compose_ref as ref

NATIVE = fd.NATIVE
CXX_SOURCES = [s for s in fd.CXX_SOURCES if os.path.basename(s) != "fake_driver.cpp"] + \
              [os.path.join(NATIVE, "fake_compose.cpp"), os.path.join(NATIVE, "fake_compose_driver.cpp")]
FIXTURE = json.load(open(os.path.join(fd.GOLDEN, "compose.json")))
SAMPLINGS = ((2, 2), (2, 1), (1, 1))


def _picture(g, seed):
    return np.random.default_rng(seed).integers(0, 256, sc.nbytes(*g), dtype=np.uint8)


def _both(pics, geoms, target):
    """the module's bytes, after they were found equal to the reference's"""
    got = cp.of_pictures(pics, geoms, target)
    assert ref.compose_picture([p.tobytes() for p in pics], geoms, ref.as_ref(target)) == got.tobytes()
    return got


# ------------------------------------------------------------------------------------------------- the module against the reference
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_module_equals_reference(sampling):
    g = (72, 40) + sampling
    small = (24, 16) + sampling
    pics = [_picture(g, 1), _picture(g, 2), _picture(small, 3)]
    geoms = [g, g, small]
    for label, t in cases.fixture_recipes(g):
        _both(pics, geoms, t)
    for t in cases.order_targets(g):
        _both(pics, geoms, t)
    _both(pics, geoms, cases.seam_target(g))
    _both(pics, geoms, cp.inset(g, 8, 6, base=1, small=2))
    _both(pics, geoms, cp.mosaic(2, 2, (24, 16), sampling, background=(0, 0, 0), sources=[2, 2, 2]))
    _both(pics, geoms, cp.average(g, 2))
    _both(pics, geoms, cp.luma_only(g, 1))
    a, b = (_both(pics, geoms, t) for t in cases.order_targets(g))
    assert not np.array_equal(a, b), "the order of the layers matters"


def test_known_answers():
    for sampling in SAMPLINGS:
        g = (24, 16) + sampling
        a, b = _picture(g, 5), _picture(g, 6)
        n = a.size
        assert np.array_equal(_both([a], [g], cp.copy(g)), a), "one whole PUT of weight 1, shift 0: the picture"
        two = cp.Target(g[:2], sampling, (cp.Layer(0, cp.ADD), cp.Layer(1, cp.ADD)), 1)
        assert np.array_equal(_both([a, b], [g, g], two), ((a.astype(int) + b + 1) >> 1).astype(np.uint8))
        assert np.array_equal(_both([a, a.copy()], [g, g], cp.difference(g)), np.full(n, 128, np.uint8)), "+1 and -1 with bias 128 on equal pictures"
        flat = cp.Target(g[:2], sampling, (), 5, (16, 128, 300 - 45))
        want = np.concatenate([np.full(k, v, np.uint8) for k, v in zip(sc.plane_bytes(*g), (16, 128, 255))])
        assert np.array_equal(_both([], [], flat), want), "count == 0: a flat picture of the bias"
        assert np.array_equal(_both([], [], cp.Target(g[:2], sampling, (), 0, -3)), np.zeros(n, np.uint8)), "the background is clamped"
    # the two negative ties of the filter text: acc -1, shift 1 -> 0; acc -3, shift 1 -> -1 (seen through a bias of 10)
    g = (8, 8, 1, 1)
    one, three = np.full(192, 1, np.uint8), np.full(192, 3, np.uint8)
    tie = lambda src: _both([src], [g], cp.Target((8, 8), (1, 1), (cp.Layer(0, cp.ADD, -1),), 1, 10))
    assert set(tie(one)) == {10} and set(tie(three)) == {9}
    assert ref.finish(-1, 1, 0) == 0 and ref.floor_shift(-3 + 1, 1) == -1
    # a PUT above ADDs discards them inside its rectangle only
    g = (16, 16, 2, 2)
    a, b = _picture(g, 7), _picture(g, 8)
    t = cp.Target((16, 16), (2, 2), (cp.Layer(0, cp.ADD, 3), cp.Layer(0, cp.ADD, 2), cp.Layer(1, cp.PUT, 1, (0, 0, 8, 8), (4, 6))))
    got = sc.planes(_both([a, b], [g, g], t), *g)
    pa, pb = sc.planes(a, *g), sc.planes(b, *g)
    for p, (x, y, w, h) in enumerate(((4, 6, 8, 8), (2, 3, 4, 4), (2, 3, 4, 4))):
        want = np.clip(5 * pa[p].astype(int), 0, 255)
        want[y:y + h, x:x + w] = pb[p][:h, :w]
        assert np.array_equal(got[p], want)
    # the translucent overlay: one rounding
    alpha = 77
    got = sc.planes(_both([a, b], [g, g], cp.overlay(g, 2, 4, (8, 6), alpha)), *g)
    for p, (x, y, w, h) in enumerate(((2, 4, 8, 6), (1, 2, 4, 3), (1, 2, 4, 3))):
        want = pa[p].astype(int)
        want[y:y + h, x:x + w] = (pa[p][y:y + h, x:x + w].astype(int) * (256 - alpha) + pb[p][:h, :w].astype(int) * alpha + 128) >> 8
        assert np.array_equal(got[p], want)


def test_struct_layout():
    from hvqm4_amd._lib import HvqComposeDst, HvqComposeLayer
    assert C.sizeof(HvqComposeLayer) == 40 and C.sizeof(HvqComposeDst) == 48
    assert [getattr(HvqComposeLayer, n).offset for n in ("mode", "sx", "sy", "w", "h", "dx", "dy", "weight")] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert [getattr(HvqComposeDst, n).offset for n in ("ptr", "width", "height", "h_samp", "v_samp", "first", "count", "shift", "bias")] == [0, 8, 12, 16, 20, 24, 28, 32, 36]
    assert cp.Layer(3, cp.ADD, (1, -2, 3), (2, 4, 6, 8), (10, 12)).numbers() == (1, 2, 4, 6, 8, 10, 12, 1, -2, 3)
    assert cp.Layer(0).numbers() == (0,) * 7 + (1, 1, 1)
    text = open(os.path.join(fd.ROOT, "include", "hvqm4_amd.h")).read()
    for name, v in (("HVQ_CMP_PUT", cp.PUT), ("HVQ_CMP_ADD", cp.ADD), ("HVQ_CMP_MAX_LAYERS", cp.MAX_LAYERS), ("HVQ_CMP_MAX_SHIFT", cp.MAX_SHIFT)):
        assert f"#define {name} {v} " in text or f"#define {name} {v}\n" in text or f"#define {name}  {v}" in text, name
    assert "#define HVQ_CMP_MAX_TOTAL  (1 << 18)" in text and cp.MAX_TOTAL == 1 << 18
    assert "#define HVQ_CMP_MAX_GAIN   (1 << 22)" in text and cp.MAX_GAIN == 1 << 22


def test_builders():
    g = (64, 48, 2, 2)
    a, b = _picture(g, 11), _picture(g, 12)
    for n in range(2, 17):
        w = cp.average_weights(n)
        assert sum(w) == 1 << 16 and len(w) == n and max(w) - min(w) <= n, n
        assert sum(l.weights()[0] for l in cp.average(g, n).layers) == 1 << cp.average(g, n).shift
    assert np.array_equal(_both([a] * 5, [g] * 5, cp.average(g, 5)), a), "the mean of equal pictures"
    mean = _both([a, b], [g, g], cp.average(g, 2))
    assert np.array_equal(mean, ((a.astype(int) + b + 1) >> 1).astype(np.uint8))
    assert np.array_equal(_both([a, b], [g, g], cp.crossfade(g, 0.0)), a) and np.array_equal(_both([a, b], [g, g], cp.crossfade(g, 1.0)), b)
    assert np.array_equal(_both([a, b], [g, g], cp.crossfade(g, 0.5)), mean)
    assert np.array_equal(_both([a], [g], cp.copy(g)), a)
    grey = sc.planes(_both([a], [g], cp.luma_only(g)), *g)
    assert np.array_equal(grey[0], sc.planes(a, *g)[0]) and set(grey[1].reshape(-1)) == set(grey[2].reshape(-1)) == {128}
    d = _both([a, b], [g, g], cp.difference(g, 2)).astype(int)
    assert np.array_equal(d, np.clip(2 * (a.astype(int) - b) + 128, 0, 255))
    sbs = cp.side_by_side(g)
    assert sbs.geometry() == (128, 48, 2, 2)
    got = sc.planes(_both([a, b], [g, g], sbs), 128, 48, 2, 2)
    for p in range(3):
        assert np.array_equal(got[p], np.hstack([sc.planes(a, *g)[p], sc.planes(b, *g)[p]]))
    small = (16, 8, 2, 2)
    s = _picture(small, 13)
    ins = sc.planes(_both([a, s], [g, small], cp.inset(g, 6, 10)), *g)
    assert np.array_equal(ins[0][10:18, 6:22], sc.planes(s, *small)[0]) and np.array_equal(ins[1][5:9, 3:11], sc.planes(s, *small)[1])
    assert np.array_equal(ins[0][:10], sc.planes(a, *g)[0][:10])
    # overlay equals the three-layer recipe of the header
    recipe = cp.Target((64, 48), (2, 2), (cp.Layer(0, cp.PUT, 256), cp.Layer(0, cp.PUT, 256 - 100, (6, 2, 20, 10), (6, 2)), cp.Layer(1, cp.ADD, 100, (0, 0, 20, 10), (6, 2))), 8)
    assert cp.overlay(g, 6, 2, (20, 10), 100) == recipe
    assert np.array_equal(_both([a, b], [g, g], cp.overlay(g, 6, 2, (20, 10), 0)), a), "alpha 0: the base"
    # the mosaic: cells row by row, the sheet rounded up to multiples of 8, the background from a flat picture or from the bias
    cell = (24, 8, 2, 2)
    cells = [_picture(cell, 20 + k) for k in range(5)]
    sheet = cp.mosaic(3, 2, (24, 8), (2, 2), gap=2, sources=range(5), flat=5)
    assert sheet.geometry() == (80, 24, 2, 2) and len(sheet.layers) == 6 and sheet.layers[5].at == (26, 10)
    bg = cp.flat_picture((80, 24), (2, 2), (16, 128, 240))
    got = sc.planes(_both(cells + [bg], [cell] * 5 + [(80, 24, 2, 2)], sheet), 80, 24, 2, 2)
    assert np.array_equal(got[0][10:18, 26:50], sc.planes(cells[4], *cell)[0]) and got[0][9, 30] == 16 and got[2][5, 39] == 240 and got[1][11, 39] == 128
    assert np.array_equal(got[1][5:9, 0:12], sc.planes(cells[3], *cell)[1])
    exact = cp.mosaic(2, 1, (24, 8), (2, 2))
    assert exact.geometry() == (48, 8, 2, 2) and exact.biases() == (0, 0, 0) and [l.source for l in exact.layers] == [0, 1]
    assert cp.mosaic(2, 2, (8, 8), (1, 1), sources=[], background=(1, 2, 3)).biases() == (1, 2, 3)
    with pytest.raises(ValueError, match="flat"):
        cp.mosaic(3, 2, (24, 8), (2, 2), gap=2)
    with pytest.raises(ValueError, match="gap"):
        cp.mosaic(3, 2, (24, 8), (2, 2), gap=1)
    with pytest.raises(ValueError, match="cells"):
        cp.mosaic(17, 16, (8, 8), (2, 2))
    with pytest.raises(ValueError, match="alpha"):
        cp.overlay(g, 0, 0, (8, 8), 257)
    with pytest.raises(ValueError, match="bits"):
        cp.crossfade(g, 0.5, bits=23)


def test_the_seam_recipe_meets_what_it_is_for():
    for g in ((64, 48, 2, 2), (48, 64, 1, 1), (296, 160, 2, 1)):
        t = cases.seam_target(g)
        cp.check(t, [g, g])
        assert any(l.rect and l.rect[2:] == (g[2], g[3]) for l in t.layers), "a rectangle of one chroma sample"
    t = cases.seam_target((296, 160, 2, 1))
    cols = {l.at[0] // 2 for l in t.layers if l.rect} | {(l.at[0] + l.rect[2]) // 2 for l in t.layers if l.rect}
    rows = {l.at[1] for l in t.layers if l.rect} | {l.at[1] + l.rect[3] for l in t.layers if l.rect}
    assert set(cases.SEAM_COLUMNS) <= cols and set(cases.SEAM_ROWS) <= rows, "the chroma planes' seams"
    assert {d for d, _s in cases.residues(t, 1)} == {0, 1, 2, 3} == {s for _d, s in cases.residues(t, 1)}
    assert {cp.body(l.rect[0] // 2, l.at[0] // 2, l.rect[2] // 2) for l in t.layers if l.rect} == {cp.ALIGNED, cp.GENERAL}
    t = cases.seam_target((48, 64, 1, 1))
    assert {d for d, _s in cases.residues(t, 0)} == {0, 1, 2, 3} == {s for _d, s in cases.residues(t, 0)}


# ------------------------------------------------------------------------------------------------- the fixture
def _clip_geometry(name):
    from hvqm4_amd.container import parse_header
    hdr = parse_header(open(os.path.join(fd.GOLDEN, fd.CLIPS[name]["file"]), "rb").read())
    return (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)


def test_fixture_covers_every_golden_clip():
    assert set(FIXTURE["clips"]) == set(fd.CLIPS)
    for name, entry in FIXTURE["clips"].items():
        g = _clip_geometry(name)
        assert tuple(entry["geometry"]) == g
        assert [(l, tuple(t)) for l, t, _c in entry["recipes"]] == [(l, t.geometry()) for l, t in cases.fixture_recipes(g)]
    assert {tuple(e["geometry"])[2:] for e in FIXTURE["clips"].values()} == set(SAMPLINGS)


@pytest.mark.parametrize("name", sorted(FIXTURE["clips"]))
def test_fixture_equals_module_and_reference(name):
    entry = FIXTURE["clips"][name]
    g = tuple(entry["geometry"])
    pics = fd.oracle_pictures(name)
    pair = [pics[0].reshape(-1), pics[-1].reshape(-1)]
    for k in (0, -1):
        assert hashlib.sha256(pics[k].tobytes()).hexdigest() == fd.CLIPS[name]["picture_sha256"][k], "the fixture describes the manifest's pictures"
    for (label, tg, crc), (label2, t) in zip(entry["recipes"], cases.fixture_recipes(g)):
        assert label == label2 and tuple(tg) == t.geometry()
        got = cp.of_pictures(pair, [g, g], t)
        assert zlib.crc32(got.tobytes()) == crc, (name, label)
        if g[0] * g[1] <= 64 * 48:                                          # plain Python again: the small clips, every sampling among them
            assert ref.compose_picture([p.tobytes() for p in pair], [g, g], ref.as_ref(t)) == got.tobytes(), (name, label)


# ------------------------------------------------------------------------------------------------- argument checks without a device
class _NoDevice:
    """what Context.compose_pictures looks at before it reaches the library"""
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


G0 = (64, 48, 2, 2)
BAD_TARGETS = {                                          # one case per refusal of the header's list that a Target can express
    "sampling": lambda: cp.Target((64, 48), (2, 2), (cp.Layer(2),)),                                  # a 4:4:4 source in a 4:2:0 target
    "leaves the 64 x 48 source": lambda: cp.Target((64, 48), (2, 2), (cp.Layer(0, rect=(56, 0, 16, 8)),)),
    "leaves the 64 x 48 target": lambda: cp.Target((64, 48), (2, 2), (cp.Layer(0, rect=(0, 0, 16, 8), at=(56, 0)),)),
    "leaves the 32 x 32 target": lambda: cp.Target((32, 32), (2, 2), (cp.Layer(0),)),
    "chroma samples": lambda: cp.Target((64, 48), (2, 2), (cp.Layer(0, rect=(1, 0, 16, 8)),)),
    "does not lie": lambda: cp.Target((64, 48), (2, 2), (cp.Layer(0, rect=(0, 0, 16, 8), at=(0, 3)),)),
    "is empty": lambda: cp.Target((64, 48), (2, 2), (cp.Layer(0, rect=(0, 0, 16, 0)),)),
    "whole source": lambda: cp.Target((64, 48), (2, 2), (cp.Layer(0, rect=(2, 0, 0, 0)),)),
    "negative": lambda: cp.Target((64, 48), (2, 2), (cp.Layer(0, rect=(0, 0, 16, 8), at=(-2, 0)),)),
    "mode": lambda: cp.Target((64, 48), (2, 2), (cp.Layer(0, mode=2),)),
    "gain": lambda: cp.Target((64, 48), (2, 2), (cp.Layer(0, cp.ADD, cp.MAX_GAIN), cp.Layer(1, cp.ADD, (0, -1, 0)))),
    "shift": lambda: cp.Target((64, 48), (2, 2), (), cp.MAX_SHIFT + 1),
    "bias": lambda: cp.Target((64, 48), (2, 2), (), 0, (0, 256, 0)),
    "bias -256": lambda: cp.Target((64, 48), (2, 2), (), 0, -256),
    "257 layers": lambda: cp.Target((64, 48), (2, 2), (cp.Layer(0, cp.ADD),) * 257),
    "target 60x48": lambda: cp.Target((60, 48), (2, 2), ()),
    "sampling \\(1, 2\\)": lambda: cp.Target((64, 48), (1, 2), ()),
    "source 5": lambda: cp.Target((64, 48), (2, 2), (cp.Layer(5),)),
    "weight": lambda: cp.Target((64, 48), (2, 2), (cp.Layer(0, weight=(1, 2)),)),
}


@pytest.mark.parametrize("what", sorted(BAD_TARGETS))
def test_a_bad_target_is_refused_before_the_library_is_called(what):
    from hvqm4_amd.batch import Context
    with pytest.raises(ValueError, match=what):
        Context.compose_pictures(_NoDevice(), [0, 0, 2], [0, 1, 0], [cp.copy(G0), BAD_TARGETS[what]()])


def test_arguments_are_checked_before_the_library_is_called():
    import torch
    from hvqm4_amd._lib import HVQ_E_ARG, HvqError
    from hvqm4_amd.batch import Context
    call = lambda *a, **k: Context.compose_pictures(_NoDevice(), *a, **k)
    t = cp.difference(G0)
    nb = 64 * 48 * 3 // 2
    with pytest.raises(ValueError, match="ordinals"):
        call([0, 0], [0], [t])
    with pytest.raises(HvqError) as e:
        call([0, 7], [0, 0], [t])
    assert e.value.code == HVQ_E_ARG
    for bad in (None, t, "sheet"):
        with pytest.raises(ValueError, match="targets"):
            call([0, 0], [0, 1], bad)
    with pytest.raises(ValueError, match="compose.Target"):
        call([0, 0], [0, 1], [t, None])
    with pytest.raises(ValueError, match="65535"):
        call([0, 0], [0, 1], [t] * 65536)
    with pytest.raises(ValueError, match=f"{1 << 18}"):
        call([0, 0], [0, 1], [cp.Target((64, 48), (2, 2), (cp.Layer(0, cp.ADD),) * 256)] * 1025)
    with pytest.raises(ValueError, match="1 sources for 2 pictures"):
        call([0, 0], [0, 1], [t], src=[None])
    room = torch.zeros(nb + 64, dtype=torch.uint8)
    off = (-room.data_ptr()) % 16
    with pytest.raises(ValueError, match="ordinal -1"):
        call([0, 0], [0, 1], [t], src=[None, room[off:off + nb]])
    with pytest.raises(ValueError, match="not a GPU"):
        call([0, 0], [0, -1], [t], src=[None, room[off:off + nb]])
    with pytest.raises(ValueError, match="out must be"):
        call([0, 0], [0, 1], [t, t], out=torch.zeros((2, nb), dtype=torch.int32))
    with pytest.raises(ValueError, match="out must be"):
        call([0, 0], [0, 1], [t, t], out=[torch.zeros(nb, dtype=torch.uint8)] * 2)                     # one target geometry: one tensor
    with pytest.raises(ValueError, match="out must be a list"):
        call([0, 0], [0, 1], [t, cp.side_by_side(G0)], out=torch.zeros((2, nb), dtype=torch.uint8))     # two geometries: a list
    with pytest.raises(ValueError, match=r"out\[1\]"):
        call([0, 0], [0, 1], [t, cp.side_by_side(G0)], out=[torch.zeros(nb, dtype=torch.uint8)] * 2)
    with pytest.raises(ValueError, match="not a GPU"):
        call([0, 0], [0, 1], [t, cp.side_by_side(G0)], out=[torch.zeros(nb, dtype=torch.uint8), torch.zeros(2 * nb, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="not a GPU"):                                                   # a call without pictures: flat targets
        call([], [], [cp.Target((64, 48), (2, 2), (), 0, 9)], out=torch.zeros((1, nb), dtype=torch.uint8))
    with pytest.raises(ValueError, match="multiple of 16"):
        room = torch.zeros(2 * nb + 64, dtype=torch.uint8)
        off = (-room.data_ptr()) % 16 + 8
        call([0, 0], [0, 1], [t, t], out=room[off:off + 2 * nb].view(2, nb))


def test_the_library_without_a_device_still_checks_its_arguments():
    """no context can exist here, and the call says so before it looks at anything else; the host-only check works"""
    from hvqm4_amd._lib import HVQ_E_ARG, HvqComposeDst, HvqComposeLayer, lib
    one = (C.c_int * 1)(0)
    l = HvqComposeLayer(0, 0, 0, 0, 0, 0, 0, (C.c_int32 * 3)(1, 1, 1))
    dst = HvqComposeDst(16, 8, 8, 2, 2, 0, 1, 0, (C.c_int32 * 3)(0, 0, 0))
    assert lib().hvq_compose_pictures(None, 1, one, one, None, C.byref(l), 1, C.byref(dst), None) == HVQ_E_ARG
    assert lib().hvq_compose_force_general(None, 1) == HVQ_E_ARG
    assert lib().hvq_compose_check(None) == HVQ_E_ARG
    assert lib().hvq_compose_check(C.byref(l)) == 0
    good = dict(mode=1, sx=2, sy=4, w=6, h=8, dx=10, dy=12)
    for field, v in (("mode", 2), ("mode", -1), ("sx", -1), ("sy", -2), ("w", -6), ("h", -8), ("dx", -1), ("dy", -1), ("h", 0), ("w", 0)):
        s = HvqComposeLayer(**good)
        assert lib().hvq_compose_check(C.byref(s)) == 0
        setattr(s, field, v)
        assert lib().hvq_compose_check(C.byref(s)) == HVQ_E_ARG, field
        with pytest.raises(ValueError):
            k = dict(good, **{field: v})
            cp.check_layer(cp.Layer(0, k["mode"], 1, (k["sx"], k["sy"], k["w"], k["h"]), (k["dx"], k["dy"])))
    s = HvqComposeLayer(1, 0, 0, 0, 0, 1 << 30, 5, (C.c_int32 * 3)(-(1 << 31), (1 << 31) - 1, 0))
    assert lib().hvq_compose_check(C.byref(s)) == 0, "weights and offsets are the call's business"


# ------------------------------------------------------------------------------------------------- the runtime on the CPU fake device
@pytest.fixture(scope="module")
def drivers():
    return {kind: fd.build_driver(kind, "compose", "fake_compose_driver", CXX_SOURCES, __file__) for kind in fd.BUILDS}


def _made(form, k, geom):
    n = sc.nbytes(*geom)
    if form == "synth":
        return ((((np.arange(n, dtype=np.uint64) + np.uint64(k)) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(13)).astype(np.uint8)
    if form == "flat":
        return np.full(n, k, dtype=np.uint8)
    assert form == "check"
    w, h, hs, vs = geom
    out = []
    for pw, ph in ((w, h), (w // hs, h // vs), (w // hs, h // vs)):
        y, x = np.mgrid[0:ph, 0:pw]
        out.append((((x + y + k) & 1) * 255).astype(np.uint8).reshape(-1))
    return np.concatenate(out)


class Script:
    """the text of a driver script, and beside it the pictures and the expected bytes of every call"""

    def __init__(self):
        self.lines, self.streams, self.pics, self.geoms, self.calls, self.bodies = [], [], [], [], {}, {}
        self._outs, self._counts = [], [0, 0]

    def clip(self, name):
        self.lines.append(f"CLIP {name}")
        self.streams.append((_clip_geometry(name), name))
        return len(self.streams) - 1

    def shape(self, g):
        self.lines.append("SHAPE %d %d %d %d" % g)
        self.streams.append((g, None))
        return len(self.streams) - 1

    def _pic(self, s, data):
        self.pics.append(np.asarray(data).reshape(-1))
        self.geoms.append(self.streams[s][0])
        return len(self.pics) - 1

    def pic(self, s, k):
        self.lines.append(f"PIC {s} {k}")
        return self._pic(s, fd.oracle_pictures(self.streams[s][1])[k])

    def mem(self, s, form, k, offset=0):
        self.lines.append(f"MEM {s} {form} {k} {offset}")
        g, name = self.streams[s]
        return self._pic(s, 255 - fd.oracle_pictures(name)[k].reshape(-1) if form == "inv" else _made(form, k, g))

    def out(self, s, call, target):
        self.lines.append(f"OUT {s} {call} {target}")
        assert sc.nbytes(*self.streams[s][0]) == self._outs[call][target].size
        return self._pic(s, self._outs[call][target])

    def force(self, on):
        self.lines.append(f"FORCE {int(on)}")
        self.forced = bool(on)

    forced = False

    def call(self, label, layers, rows, null=False):
        """rows: [(Target, first, count)]: a target's own layers are ignored, it takes layers[first : first + count]"""
        for l in layers:
            self.lines.append("L %d %d %d %d %d %d %d %d %d %d %d" % ((l.source,) + l.numbers()))
        want = []
        for t, first, count in rows:
            self.lines.append("T %d %d %d %d %d %d %d %d %d %d" % (t.geometry() + (t.shift,) + t.biases() + (first, count)))
            mine = cp.Target(t.size, t.sampling, tuple(layers[first:first + count]), t.shift, t.bias)
            want.append(cp.of_pictures(self.pics, self.geoms, mine))
            hs, vs = t.sampling
            for l in mine.layers:
                sx, dx, w = (l.rect[0], l.at[0], l.rect[2]) if l.rect and l.rect[2] else (0, l.at[0], self.geoms[l.source][0])
                for p in range(3):
                    d = hs if p else 1
                    self._counts[cp.GENERAL if self.forced else cp.body(sx // d, dx // d, w // d)] += 1
        self.lines.append(f"CALL {label} {int(null)}")
        self.calls[label] = [(t.geometry(), zlib.crc32(w.tobytes())) for (t, _f, _c), w in zip(rows, want)]
        self._outs.append(want)
        return len(self._outs) - 1

    def targets(self, label, targets, null=False):
        layers, rows = cases.flatten(targets)
        return self.call(label, layers, rows, null)

    def count(self, label):
        self.lines.append(f"COUNT {label}")
        self.bodies[label] = tuple(self._counts)
        self._counts = [0, 0]


_shift = cases.shifted


def script_goldens():
    """the fixture's recipes, the seams and the order on clips of the three samplings and of two with tile seams inside every plane"""
    s = Script()
    targets = []
    for name in ("crossplane420_64x48", "crossplane422_13_64x48", "crossplane444_48x64", "ragged24x40", "wide296x160", "yuv422_296x160"):
        st = s.clip(name)
        a, b = s.pic(st, 0), s.pic(st, fd.n_pics(name) - 1)
        assert b == a + 1
        g = s.streams[st][0]
        targets += [_shift(t, a) for _l, t in cases.fixture_recipes(g)] + [_shift(t, a) for t in cases.order_targets(g)]
        targets += [_shift(cases.seam_target(g), a), _shift(cp.copy(g), a), _shift(cp.luma_only(g, 1), a), _shift(cp.average(g, 2), a)]
    s.targets("goldens/all", targets)
    s.targets("goldens/one", targets[1:2])
    s.count("goldens")
    return s


def script_memory():
    """pictures in the caller's memory, at the start of an allocation and 16 bytes into one, mixed with resident ones; the extremes on
    checkerboards; the smallest geometry in the three samplings; on the caller's stream and on the null stream"""
    s = Script()
    name = "yuv422_64x48"
    st = s.clip(name)
    g = s.streams[st][0]
    targets = []
    for k in range(fd.n_pics(name)):
        a, b = s.mem(st, "inv", k, 16 if k & 1 else 0), s.pic(st, k)
        targets += [_shift(cp.crossfade(g, 0.25), a), _shift(cp.difference(g), a), _shift(cases.seam_target(g), a)]
    for sampling in SAMPLINGS:
        big, small = s.shape((128, 128) + sampling), s.shape((8, 8) + sampling)
        first = s.mem(big, "check", 0)
        s.mem(big, "check", 1)
        for k in range(256):
            s.mem(small, "synth" if k % 3 else "flat", k)
        targets += [_shift(t, first) for t in cases.extreme_targets(sampling)]
        targets += [_shift(cp.copy((8, 8) + sampling), first + 2 + 77), _shift(cp.difference((8, 8) + sampling, 3), first + 2)]
    s.targets("memory", targets)
    s.targets("memory/nullstream", targets, null=True)
    s.count("memory")
    return s


def script_many():
    """one launch, many shapes: 300 targets over the pictures of eight clips, with layer ranges that share layers; the same call twice"""
    s = Script()
    layers, spans = [], []
    for name in ("gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8", "i16", "natural128x96"):
        st = s.clip(name)
        g = s.streams[st][0]
        first = len(layers)
        pics = [s.pic(st, k) for k in range(fd.n_pics(name))]
        hs, vs = g[2:]
        for k, p in enumerate(pics * 2):                                        # ADD layers of weights 3, -1, 2, 1, ...: any run of them is a target
            layers.append(cp.Layer(p, cp.ADD, (3, -1, 2, 1)[k % 4]) if k % 3 else cp.Layer(p, cp.PUT, 2, (0, 0, g[0] // 2 // hs * hs, g[1] // 2 // vs * vs), (hs * (k % 3), vs * (k % 2))))
        spans.append((g, first, len(layers) - first))
    rows = []
    for i in range(300):
        g, first, n = spans[i % len(spans)]
        off, cnt = i // 8 % n, 1 + (i // 3) % 4
        cnt = min(cnt, n - off)
        rows.append((cp.Target(g[:2], g[2:], (), i % 3, ((i % 5) * 20 - 40, 0, i % 7)), first + off, cnt))
    rows.append((cp.Target((64, 48), (2, 2), (), 0, 77), 0, 0))
    s.call("many", layers, rows)
    s.call("many/again", layers, rows)
    s.count("many")
    return s


def script_body():
    """the same call under the chosen bodies, under the general body everywhere, and under the chosen ones again"""
    s = Script()
    targets = []
    for name in ("crossplane420_64x48", "crossplane444_48x64", "wide296x160", "yuv422_296x160"):
        st = s.clip(name)
        a, _b = s.pic(st, 0), s.pic(st, fd.n_pics(name) - 1)
        g = s.streams[st][0]
        targets += [_shift(t, a) for _l, t in cases.fixture_recipes(g)] + [_shift(cases.seam_target(g), a)]
    s.targets("body/chosen", targets)
    s.count("body/chosen")
    s.force(1)
    s.targets("body/general", targets)
    s.count("body/general")
    s.force(0)
    s.targets("body/chosen_again", targets)
    s.count("body/chosen_again")
    return s


def script_chain():
    """composed pictures straight into the next call as its sources, nothing waited for in between"""
    s = Script()
    st = s.clip("gop64x48_15")
    g = s.streams[st][0]
    pics = [s.pic(st, k) for k in range(4)]
    first = s.targets("chain/first", [_shift(cp.crossfade(g, 0.5), k) for k in range(3)] + [cp.side_by_side(g)])
    wide = s.shape((128, 48, 2, 2))
    o = [s.out(st, first, k) for k in range(3)]
    sheet = s.out(wide, first, 3)
    s.targets("chain/second", [cp.difference(g, 4, o[0], o[1]), cp.difference(g, 4, o[1], pics[3]),
                               cp.Target((128, 48), (2, 2), (cp.Layer(sheet), cp.Layer(o[2], cp.ADD, -1, at=(32, 0))), 0, 9)])
    s.count("chain")
    return s


SCRIPTS = {"goldens": script_goldens, "memory": script_memory, "many": script_many, "body": script_body, "chain": script_chain}
_scripts = {}


def _run(exe, scenario, schedule, tmp_path):
    script = None
    if scenario in SCRIPTS:
        if scenario not in _scripts:
            _scripts[scenario] = SCRIPTS[scenario]()
        script = _scripts[scenario]
    _, lines = fd.run_checked(exe, "script" if script else scenario, schedule, tmp_path,
                                inputs={"script.txt": "\n".join(script.lines) + "\n"} if script else None)
    P, R, S, B = {}, {}, {}, {}
    for line in lines:
        f = line.split()
        if f[0] == "P":
            assert int(f[8]) == 1, f"{f[1]}: the bytes around target {f[2]} were written"
            P.setdefault(f[1], []).append((tuple(int(v) for v in f[3:7]), int(f[7])))
            assert int(f[2]) == len(P[f[1]]) - 1
        elif f[0] == "R":
            R.setdefault(f[1], []).append(int(f[2]))
        elif f[0] == "S":
            S[f[1]] = (int(f[2]), int(f[3]))
        elif f[0] == "B":
            B[f[1]] = (int(f[2]), int(f[3]))
    if script:
        assert set(P) == set(script.calls)
        for label, want in script.calls.items():
            for i, (got, w) in enumerate(zip(P[label], want)):
                assert got == w, f"{label}: target {i}: geometry and crc {got}, want {w}"
            assert len(P[label]) == len(want)
        assert B == script.bodies, "the bodies that ran are the host rule's"
    return P, R, S, B


def _check_goldens(P, R, S, B):
    assert len(P["goldens/all"]) == 6 * 11 and P["goldens/one"] == P["goldens/all"][1:2]
    assert {g[2:] for g, _c in P["goldens/all"]} == set(SAMPLINGS) and min(B["goldens"]) > 0


def _check_memory(P, R, S, B):
    assert P["memory"] == P["memory/nullstream"] and len(P["memory"]) == 3 * fd.n_pics("yuv422_64x48") + 3 * (len(cases.extreme_targets()) + 2)


def _check_many(P, R, S, B):
    assert len(P["many"]) == 301 and P["many"] == P["many/again"]
    assert len({g for g, _c in P["many"]}) >= 5 and len({c for _g, c in P["many"]}) > 250


def _check_body(P, R, S, B):
    assert P["body/chosen"] == P["body/general"] == P["body/chosen_again"]
    assert R == {"force": [0, 1]}
    assert B["body/chosen"] == B["body/chosen_again"] and min(B["body/chosen"]) > 0, "at least one layer plane chose each body"
    assert B["body/general"] == (0, sum(B["body/chosen"]))


def _check_chain(P, R, S, B):
    assert len(P["chain/first"]) == 4 and len(P["chain/second"]) == 3


def _mean(pics, g, n):
    return [cp.of_pictures(pics, [g] * len(pics), cp.Target(g[:2], g[2:], (cp.Layer(k, cp.ADD), cp.Layer((k + 1) % n, cp.ADD)), 1)) for k in range(n)]


def _crcs(pictures, g):
    return [(g, zlib.crc32(p.tobytes())) for p in pictures]


def _check_reuse(P, R, S, B):
    from hvqm4_amd._lib import HVQ_E_STATE
    n, ne = fd.n_pics("gop64x48_15"), fd.n_pics("yuv444_64x48")
    g, ge = _clip_geometry("gop64x48_15"), _clip_geometry("yuv444_64x48")
    pics = [p.reshape(-1) for p in fd.oracle_pictures("gop64x48_15")]
    first = _mean(pics, g, n)
    assert P["reuse"] == _crcs(first, g) == P["reuse/late"]
    assert R["reuse/evicted"] == [HVQ_E_STATE], "the flushes did not hand the slots of the first pass on: the scenario tests nothing"
    chain = [cp.of_pictures(first, [g] * n, cp.Target(g[:2], g[2:], (cp.Layer(k, cp.ADD, 1), cp.Layer((k + 1) % n, cp.ADD, -1)), 0, 128)) for k in range(n)]
    assert P["reuse/chain"] == _crcs(chain, g)
    assert P["reuse/destroy"] == _crcs(_mean([p.reshape(-1) for p in fd.oracle_pictures("yuv444_64x48")], ge, ne), ge)


ARG_REFUSALS = ["null_context", "null_streams", "null_ordinals", "null_layers", "null_dst", "negative_layers", "negative_targets", "too_many_targets", "too_many_layers",
                "bad_stream", "bad_ordinal", "misaligned_src", "src_with_ordinal", "src_with_bad_stream", "minus_one_without_src", "null_ptr", "misaligned_ptr",
                "sampling_differs", "sampling_differs_target", "source_leaves_x", "source_leaves_y", "source_too_wide", "target_leaves_x", "target_leaves_y",
                "whole_leaves_target", "whole_in_smaller_target", "odd_sx", "odd_w", "odd_dx", "odd_sy", "odd_h", "odd_dy", "empty_h", "whole_with_sx", "negative_sx",
                "negative_dy", "negative_w", "mode_2", "mode_negative", "gain_above", "shift_above", "shift_negative", "bias_above", "bias_below", "first_negative",
                "count_negative", "range_beyond", "first_beyond", "unused_layer_checked", "too_many_in_target", "check_null", "check_mode", "force_null"]


def _check_refused(P, R, S, B):
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_GEOMETRY, HVQ_E_STATE
    want = {k: HVQ_E_ARG for k in ARG_REFUSALS}
    want.update({"geometry_width": HVQ_E_GEOMETRY, "geometry_sampling": HVQ_E_GEOMETRY, "geometry_zero": HVQ_E_GEOMETRY})
    want.update({"evicted": HVQ_E_STATE, "queued": HVQ_E_STATE, "n0": 0, "check_good": 0, "check_rect": 0})
    assert R == {"refused/" + k: [v] for k, v in want.items()}
    same, total = S["refused"]
    assert same == total == 2 * 4608 + 16, "a refused call wrote its output"
    g = _clip_geometry("gop64x48_15")
    assert P["refused/then_ok"] == _crcs(_mean([p.reshape(-1) for p in fd.oracle_pictures("gop64x48_15")[:2]], g, 2), g)


CHECKS = {"goldens": _check_goldens, "memory": _check_memory, "many": _check_many, "body": _check_body, "chain": _check_chain, "reuse": _check_reuse,
          "refused": _check_refused}


@pytest.mark.parametrize("schedule", ["eager", "late"])
@pytest.mark.parametrize("build", list(fd.BUILDS))
@pytest.mark.parametrize("scenario", list(CHECKS))
def test_fake_device_scenario(drivers, scenario, build, schedule, tmp_path):
    P, R, S, B = _run(drivers[build], scenario, schedule, tmp_path)
    CHECKS[scenario](P, R, S, B)


def test_the_existing_fake_builds_link_without_the_compose_body():
    """the source lists of the other drivers have no hvq_launch_compose: the runtime's reference is weak"""
    assert not any("fake_compose" in s for s in fd.CXX_SOURCES)
    text = open(os.path.join(fd.CSRC, "hvq_runtime.cpp")).read()
    decl = [l for l in text.splitlines() if "hvq_launch_compose(" in l and l.startswith("extern")]
    assert len(decl) == 1 and "__attribute__((weak))" in decl[0]
    # the call hands the symbol to the tail the slot-layout calls share, which refuses a null one before anything is enqueued
    assert "return slot_enqueue(c, hvq_launch_compose, " in text and "if (!launch) return fail(HVQ_E_NOGPU" in text
    for kind in fd.BUILDS:                                                       # the plain driver of tests/test_fake_device.py: built there, or here
        exe = fd.build_driver(kind, "fake", "fake_driver", fd.CXX_SOURCES, fd.__file__)
        assert os.path.exists(exe)
