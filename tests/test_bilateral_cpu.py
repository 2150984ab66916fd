"""CPU: the values of hvq_bilateral_pictures.  tests/bilateral_ref.py restates include/hvqm4_amd.h in plain Python; hvqm4_amd.bilateral
(numpy, whole shifted planes at a time), the fixture tests/golden/bilateral.json and the runtime on the CPU fake device
(tests/native/fake_bilateral.cpp, which walks the kernel's grid with the staging, the tap step and the division of hvq_bilateral.h) are
compared with it by ==.  The fake-device driver is a stand-alone program, built and run plain and with ASan + UBSan as
tests/test_rank_cpu.py builds its own; nothing is preloaded and no Python is involved in the sanitised run."""
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import pytest

import tests.test_fake_device as fd
from hvqm4_amd import bilateral as B
from tests import bilateral_cases as cases
from tests import bilateral_ref as ref

NATIVE = fd.NATIVE
CXX_SOURCES = [s for s in fd.CXX_SOURCES if os.path.basename(s) != "fake_driver.cpp"] + \
              [os.path.join(NATIVE, "fake_bilateral.cpp"), os.path.join(NATIVE, "fake_bilateral_driver.cpp")]
FIXTURE = json.load(open(os.path.join(fd.GOLDEN, "bilateral.json")))

PLANES = {"identity": B.IDENTITY_PLANE, "gauss": B.bilateral(1.5, 12).luma, "gauss7": B.bilateral(3.0, 25, 7).luma, "gauss3x1": B.bilateral(1.0, 8, (3, 1)).luma,
          "sigma2_10": B.sigma_filter(2, 10).luma, "sigma0x7": B.sigma_filter((0, 7), 30).luma, "sigma7x0": B.sigma_filter((7, 0), 3).luma, "box1": B.box(1).luma,
          "box7x3": B.box((7, 3)).luma, "disc3": B.disc(3).luma, "disc7": B.disc(7, sigma_range=20.0).luma, "disc5t": B.disc(5, threshold=16).luma,
          "all255": cases.ALL255.luma, "random7": cases.random_set(1, 7, 7), "random5x2": cases.random_set(2, 5, 2), "random0x6": cases.random_set(3, 0, 6),
          "random_nozeros": cases.random_set(4, 3, 3, zeros=False), "only_range0": B.plane_from_tables(4, 3, [[9] * 5] * 4, [7])}


def _ref_plane(a, g, p):
    rows = lambda v: None if v is None else [bytes(r) for r in np.asarray(v, dtype=np.uint8)]
    return np.array(ref.bilateral_plane(rows(a), rows(g), *ref.as_ref(p)), dtype=np.uint8)


def _both(a, p, g=None):
    """the module's answer, which must be the reference's, as lists"""
    a = np.array(a, dtype=np.uint8)
    g = None if g is None else np.array(g, dtype=np.uint8)
    got = B.of_plane(a, g, p)
    assert np.array_equal(got, _ref_plane(a, g, p))
    return got.tolist()


def _plane_contents(nx, ny, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:ny, 0:nx]
    return [rng.integers(0, 256, (ny, nx), dtype=np.uint8), rng.integers(0, 4, (ny, nx)).astype(np.uint8), (((x + y) & 1) * 255).astype(np.uint8),
            (x * 255 // max(nx - 1, 1)).astype(np.uint8)]


@pytest.mark.parametrize("name", sorted(PLANES))
def test_module_equals_reference(name):
    p = PLANES[name]
    for (nx, ny), seed in (((12, 8), 1), ((4, 4), 2), ((8, 20), 3)):           # 4 x 4 under radius 7: the clamp repeats
        planes = _plane_contents(nx, ny, seed)
        for k, a in enumerate(planes):
            assert np.array_equal(B.of_plane(a, None, p), _ref_plane(a, None, p)), (name, nx, ny)
            g = planes[(k + 1) % len(planes)]
            assert np.array_equal(B.of_plane(a, g, p), _ref_plane(a, g, p)), (name, nx, ny, "guided")


def test_module_equals_reference_on_the_largest_made_plane():
    a, g = _plane_contents(72, 40, 9)[0], _plane_contents(72, 40, 10)[0]
    for name in ("gauss7", "random7", "disc5t"):
        assert np.array_equal(B.of_plane(a, None, PLANES[name]), _ref_plane(a, None, PLANES[name])), name
    assert np.array_equal(B.of_plane(a, g, PLANES["random5x2"]), _ref_plane(a, g, PLANES["random5x2"]))


@pytest.mark.parametrize("geom", [(16, 8, 2, 2), (16, 8, 2, 1), (8, 16, 1, 1)])
def test_module_equals_reference_on_pictures_of_the_three_samplings(geom):
    pic, guide = cases.made(geom, "random", 5), cases.made(geom, "ties", 6)
    sets = (B.chroma_for(B.bilateral(2.0, 30, 4), *geom[2:]), B.luma_only(B.sigma_filter(3, 40)), B.Bilateral(cases.random_set(5, 2, 3), cases.random_set(6, 7, 1)))
    for b in sets:
        for gd in (None, guide):
            want = ref.bilateral_picture(pic.tobytes(), geom, ref.as_ref(b.luma), ref.as_ref(b.chroma), None if gd is None else gd.tobytes())
            assert B.of_picture(pic, geom, b, gd).tobytes() == want, (geom, gd is None)
    steps = B.iterate(sets[0], 2) + [sets[1]]
    assert B.of_steps(pic, geom, steps).tobytes() == ref.steps_picture(pic.tobytes(), geom, [(ref.as_ref(s.luma), ref.as_ref(s.chroma)) for s in steps])
    assert B.of_steps(pic, geom, steps, guide).tobytes() == ref.steps_picture(pic.tobytes(), geom, [(ref.as_ref(s.luma), ref.as_ref(s.chroma)) for s in steps], guide.tobytes())


def test_known_answers():
    """every known answer of the header, in the module and in the reference"""
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, (7, 9), dtype=np.uint8)
    g = rng.integers(0, 256, (7, 9), dtype=np.uint8)
    # radius 0 copies the plane
    for p in (B.IDENTITY_PLANE, B.plane_from_tables(0, 0, [[200]], [3] * 256), B.plane_from_tables(0, 0, [[1]], [255])):
        assert _both(a, p) == a.tolist() and _both(a, p, g) == a.tolist()
    # a flat plane stays flat under any tables
    flat = np.full((6, 7), 201, dtype=np.uint8)
    for name, p in PLANES.items():
        assert _both(flat, p) == flat.tolist() and _both(flat, p, g[:6, :7]) == flat.tolist(), name
    # a range table with only range[0] != 0 copies the plane under any radius and spatial table
    assert _both(a, PLANES["only_range0"]) == a.tolist()
    assert _both(a, B.plane_from_tables(7, 7, [[255] * 8] * 8, [1])) == a.tolist()
    # range all ones and spatial all ones: the box mean with replicated borders, rounded half up
    for rx, ry in ((1, 1), (2, 0), (0, 3), (7, 2)):
        e = np.pad(a.astype(np.int64), ((ry, ry), (rx, rx)), mode="edge")
        total = sum(e[j:j + 7, i:i + 9] for j in range(2 * ry + 1) for i in range(2 * rx + 1))
        n = (2 * rx + 1) * (2 * ry + 1)
        assert _both(a, B.box((rx, ry)).luma) == ((2 * total + n) // (2 * n)).tolist(), (rx, ry)
    # {0, 1, 0} under spatial[0] = {2, 1}, ry = 0 and a flat range table: 2 / 4 rounds up
    assert _both([[0, 1, 0]], B.plane_from_tables(1, 0, [[2, 1]], [1] * 256))[0][1] == 1
    assert _both([[0, 1, 0]], B.plane_from_tables(1, 0, [[2, 1]], [77] * 256))[0][1] == 1
    # a two-level step of 40 | 200 under range[d] = 0 for d >= 100 is left as it is, at radius 7 with every other weight 255
    step = np.where(np.mgrid[0:20, 0:24][1] < 12, 40, 200).astype(np.uint8)
    assert _both(step, cases.STEP_KEEPER.luma) == step.tolist()
    assert _both(step, cases.ALL255.luma) != step.tolist()
    # a flat guide makes the call a linear filter; with the quadrant {4, 2; 2, 1} it is the 3 x 3 binomial exactly
    quad = B.plane_from_tables(1, 1, [[4, 2], [2, 1]], [1] + [0] * 255)
    e = np.pad(a.astype(np.int64), 1, mode="edge")
    want = sum(w * e[j:j + 7, i:i + 9] for j, wj in enumerate((1, 2, 1)) for i, w in ((0, wj), (1, 2 * wj), (2, wj)))
    assert _both(a, quad, np.full((7, 9), 33, dtype=np.uint8)) == ((want + 8) >> 4).tolist()
    # a picture guided by a copy of itself equals the unguided call
    for name in ("gauss", "random7", "sigma2_10"):
        assert _both(a, PLANES[name], a.copy()) == _both(a, PLANES[name]), name


def _transposed(p):
    return B.plane_from_tables(p.ry, p.rx, [[p.spatial[8 * i + j] for i in range(8)] for j in range(8)], list(p.range))


@pytest.mark.parametrize("name", ["gauss3x1", "random5x2", "random0x6", "box7x3", "disc5t"])
def test_transposition_and_mirrors(name):
    """transposing the plane, the radii and spatial transposes the result; mirroring the plane mirrors it: module and reference"""
    p = PLANES[name]
    a, g = _plane_contents(12, 8, 11)[0], _plane_contents(12, 8, 12)[1]
    for gd in (None, g):
        out = np.array(_both(a, p, gd), dtype=np.uint8)
        assert _both(a.T.copy(), _transposed(p), None if gd is None else gd.T.copy()) == out.T.tolist()
        assert _both(a[:, ::-1].copy(), p, None if gd is None else gd[:, ::-1].copy()) == out[:, ::-1].tolist()
        assert _both(a[::-1].copy(), p, None if gd is None else gd[::-1].copy()) == out[::-1].tolist()


def test_cross_checks_against_the_filter_and_integral_modules():
    from hvqm4_amd import filters as F
    from hvqm4_amd import integral as I
    quad = B.from_tables(1, 1, [[4, 2], [2, 1]], [5] * 256)                # a flat range table: a linear filter
    for geom in cases.SHAPES[:2] + ((16, 8, 2, 1),):
        pic = cases.made(geom, "random", 21)
        assert np.array_equal(B.of_picture(pic, geom, quad), F.of_picture(pic, geom, F.binomial(3))), geom
    # box(r) == the integral unit's MEAN on the samples whose window does not touch the border
    a = _plane_contents(40, 24, 5)[0]
    for r in (1, 2, 5):
        got = B.of_plane(a, None, B.box(r).luma)
        assert np.array_equal(got[r:-r, r:-r], I.of_window(a, I.mean(r))[r:-r, r:-r]), r


@pytest.mark.parametrize("case", cases.arithmetic(), ids=lambda c: c[0])
def test_directed_arithmetic(case):
    _label, g, pic, b = case
    assert B.of_picture(pic, g, b).tobytes() == ref.bilateral_picture(pic.tobytes(), g, ref.as_ref(b.luma), ref.as_ref(b.chroma))


def test_the_directed_set_reaches_the_bounds_of_the_header():
    arith = {label: (g, pic, b) for label, g, pic, b in cases.arithmetic()}
    # all-255 tables at radius 7 on a plane of 255: num + den / 2 is the header's bound, and the answer is 255
    assert 225 * 65025 * 255 + 225 * 65025 // 2 == 3738124687 < 2 ** 32 and 225 * 65025 == 14630625
    g, pic, b = arith["all255/255"]
    assert b.luma.taps() == 225 and set(b.luma.spatial) == {255} and set(b.luma.range) == {255} and set(pic.tolist()) == {255}
    assert set(B.of_picture(pic, g, b).tolist()) == {255}
    assert set(B.of_picture(arith["all255/one254"][1], g, b).tolist()) == {255}, "one 254 among 225 samples of 255 rounds back up"
    # den == 1: the centre tap alone, weight 1
    g, pic, b = arith["den1/random"]
    assert b.luma.taps() == 1 and b.luma.spatial[0] == 1 and b.luma.range[0] == 1 and np.array_equal(B.of_picture(pic, g, b), pic)
    # ties exactly at one half occur and round up
    a = np.array([[0, 1, 0, 3, 2, 3, 0, 0]], dtype=np.uint8)
    assert _both(a, arith["half/row"][2].luma) == [[0, 1, 1, 2, 3, 2, 1, 0]]


def test_struct_layout():
    import ctypes as C
    from hvqm4_amd._lib import HvqBilateral, HvqBilateralPlane
    assert (C.sizeof(HvqBilateralPlane), C.sizeof(HvqBilateral)) == (336, 672)
    assert [(n, getattr(HvqBilateralPlane, n).offset) for n, _t in HvqBilateralPlane._fields_] == [("rx", 0), ("ry", 4), ("pad", 8), ("spatial", 16), ("range", 80)]
    assert HvqBilateral.luma.offset == 0 and HvqBilateral.chroma.offset == 336
    s = B.Bilateral(cases.random_set(1, 7, 3), cases.random_set(2, 0, 5)).struct()
    assert (s.luma.rx, s.luma.ry, s.luma.pad[0], s.luma.pad[1], s.chroma.rx, s.chroma.ry) == (7, 3, 0, 0, 0, 5)
    assert bytes(bytearray(s.luma.spatial[2])) == cases.random_set(1, 7, 3).spatial[16:24] and bytes(bytearray(s.chroma.range)) == cases.random_set(2, 0, 5).range
    assert (B.MAX_RADIUS, B.MAX_SETS) == (7, 64)
    header = open(os.path.join(fd.ROOT, "include", "hvqm4_amd.h")).read()
    for line in ("#define HVQ_BIL_MAX_RADIUS 7", "#define HVQ_BIL_MAX_SETS   64",
                 "typedef struct HvqBilateralPlane { int32_t rx, ry, pad[2]; uint8_t spatial[8][8]; uint8_t range[256]; } HvqBilateralPlane;",
                 "typedef struct HvqBilateral      { HvqBilateralPlane luma, chroma; } HvqBilateral;", "225 * 65025 * 255 + 7315312 = 3738124687 < 2^32"):
        assert line in header, line
    desc = open(os.path.join(fd.CSRC, "hvq_desc.h")).read()
    for line in ("#define HVQ_BL_PLANE_BYTES 336u", "#define HVQ_BL_SPATIAL_AT  16u", "#define HVQ_BL_RANGE_AT    80u", "#define HVQ_BL_MAX_R  7u"):
        assert line in desc, line


def test_builders():
    import math
    b = B.bilateral(1.5, 12)
    assert b.luma == b.chroma and (b.luma.rx, b.luma.ry) == (3, 3), "the radius rule: ceil(2 sigma)"
    sp = lambda p, j, i: p.spatial[8 * j + i]
    assert [sp(b.luma, 0, i) for i in range(5)] == [255, 204, 105, 35, 0] and sp(b.luma, 1, 1) == 164 and sp(b.luma, 3, 3) == 5 and sp(b.luma, 4, 0) == 0
    assert list(b.luma.range[:4]) == [255, 254, 251, 247] and b.luma.range[12] == 155 and b.luma.range[24] == 35 and b.luma.range[48] == 0 and b.luma.range[255] == 0
    for i in range(4):
        for j in range(4):
            assert sp(b.luma, j, i) == int(math.floor(255 * math.exp(-(i * i + j * j) / 4.5) + 0.5))
    assert [B.default_radius(s) for s in (0.1, 0.5, 0.6, 1.0, 1.5, 2.2, 3.5, 9.0)] == [1, 1, 2, 2, 3, 5, 7, 7]
    assert (B.bilateral(9.0, 5).luma.rx, B.bilateral(1.5, 12, 2).luma.rx, B.bilateral(1.5, 12, (1, 4)).luma.ry) == (7, 2, 4)
    s = B.sigma_filter((2, 1), 10).luma
    assert (s.rx, s.ry) == (2, 1) and s.taps() == 15 and s.range[:12] == bytes([1] * 11 + [0]) and sp(s, 1, 2) == 1 and sp(s, 2, 0) == 0 and sp(s, 0, 3) == 0
    assert B.box(2).luma.taps() == 25 and set(B.box(2).luma.range) == {1}
    d = B.disc(3).luma
    assert d.taps() == 37 and sp(d, 3, 0) == 1 and sp(d, 3, 1) == 1 and sp(d, 2, 2) == 1 and sp(d, 3, 2) == 0 and sp(d, 3, 3) == 0 and set(d.range) == {1}
    assert B.disc(5).luma.taps() == 97 and B.box(5).luma.taps() == 121
    assert B.disc(2, threshold=4).luma.range[:6] == bytes([1, 1, 1, 1, 1, 0]) and B.disc(2, sigma_range=12.0).luma.range == b.luma.range
    assert B.identity().luma == B.IDENTITY_PLANE and B.copies(B.identity().chroma) and not B.copies(B.box((0, 1)).luma)
    assert B.luma_only(b) == B.Bilateral(b.luma, B.IDENTITY_PLANE)
    # the chroma radius and spatial sigma follow the sampling
    wide = B.bilateral(3.0, 12, 6)
    assert B.chroma_for(wide, 2, 2).chroma == B.bilateral(1.5, 12, 3).luma and B.chroma_for(wide, 2, 2).luma == wide.luma
    c = B.chroma_for(wide, 2, 1).chroma
    assert (c.rx, c.ry) == (3, 6) and [sp(c, 0, i) for i in range(4)] == [sp(wide.luma, 0, 2 * i) for i in range(4)] and [sp(c, j, 0) for j in range(7)] == [sp(wide.luma, j, 0) for j in range(7)]
    assert B.chroma_for(wide, 1, 1).chroma == wide.luma
    one = B.chroma_for(B.box((1, 0)), 2, 2).chroma
    assert (one.rx, one.ry, one.taps()) == (1, 0, 3), "never below 1 where the luma radius is at least 1"
    assert B.chroma_for(B.sigma_filter(5, 9), 2, 1).chroma == B.sigma_filter((2, 5), 9).luma
    assert B.iterate(b, 3) == [b, b, b] and B.as_steps(b) == [b] and B.as_steps([b, wide]) == [b, wide]
    assert len({B.box(1), B.box((1, 1)), B.box(2)}) == 2 and hash(B.disc(3)) == hash(B.disc(3))
    t = B.from_tables(2, 1, [[9, 8, 7, 99], [6, 5, 4, 99], [99] * 4], [3, 2])
    assert (t.luma.rx, t.luma.ry) == (2, 1) and t.luma.spatial[:4] == bytes([9, 8, 7, 0]) and t.luma.spatial[8:12] == bytes([6, 5, 4, 0]) and t.luma.spatial[16] == 0
    assert t.luma.range[:3] == bytes([3, 2, 0]), "what lies outside the radii is not read and becomes 0"
    for bad in (lambda: B.box(8), lambda: B.box(-1), lambda: B.box((1, 2, 3)), lambda: B.box(1.5), lambda: B.bilateral(0, 5), lambda: B.bilateral(1, -1), lambda: B.bilateral(1, 1, 8),
                lambda: B.sigma_filter(1, 256), lambda: B.sigma_filter(1, -1), lambda: B.disc(3, 2.0, 4), lambda: B.disc((1, 2)), lambda: B.chroma_for(b, 1, 2),
                lambda: B.from_tables(1, 1, [[0, 1], [1, 1]], [1]), lambda: B.from_tables(1, 1, [[1, 1], [1, 1]], [0, 1]), lambda: B.from_tables(1, 1, [[1, 1]], [1]),
                lambda: B.from_tables(1, 0, [[1, 256]], [1]), lambda: B.from_tables(1, 0, [[1, 1]], [1] * 257), lambda: B.iterate(b, 0), lambda: B.as_steps([]),
                lambda: B.as_steps([b, None]), lambda: B.check(b.luma), lambda: B.check(B.Bilateral(B.PlaneBilateral(1, 1, b.luma.spatial, b.luma.range, (0, 1)), b.chroma)),
                lambda: B.check(B.Bilateral(b.luma, B.PlaneBilateral(1, 1, b.luma.spatial[:63], b.luma.range))), lambda: B.of_plane(np.zeros((2, 2)), None, b.luma),
                lambda: B.of_plane(np.zeros((2, 2), dtype=np.uint8), np.zeros((2, 3), dtype=np.uint8), b.luma)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------- the fixture
def _clip_geometry(name):
    from hvqm4_amd.container import parse_header
    hdr = parse_header(open(os.path.join(fd.GOLDEN, fd.CLIPS[name]["file"]), "rb").read())
    return (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)


def test_fixture_covers_every_golden_clip():
    assert set(FIXTURE["clips"]) == set(fd.CLIPS)
    for name, entry in FIXTURE["clips"].items():
        assert tuple(entry["geometry"]) == _clip_geometry(name)
        assert [l for l, _c in entry["sets"]] == [l for l, _b in cases.FIVE]


def test_the_generator_names_the_shared_parameter_sets():
    sys.path.insert(0, fd.GOLDEN)
    try:
        import make_bilateral
    finally:
        sys.path.remove(fd.GOLDEN)
    assert make_bilateral.SETS == [label for label, _b in cases.FIVE] and make_bilateral.cases is cases
    assert cases.FIVE[0][1] == B.bilateral(1.5, 12) and cases.FIVE[1][1] == B.sigma_filter(2, 10) and cases.FIVE[2][1] == B.box((3, 1)) and cases.FIVE[3][1] == B.disc(3)
    assert cases.FIVE[4][1].chroma == B.IDENTITY_PLANE and cases.FIVE[4][1].luma.rx > 0


@pytest.mark.parametrize("name", sorted(FIXTURE["clips"]))
def test_fixture_equals_module_and_reference(name):
    entry = FIXTURE["clips"][name]
    g = tuple(entry["geometry"])
    pic = fd.oracle_pictures(name)[0]
    assert hashlib.sha256(pic.tobytes()).hexdigest() == fd.CLIPS[name]["picture_sha256"][0], "the fixture describes the manifest's picture"
    for (label, crc), (label2, b) in zip(entry["sets"], cases.FIVE):
        assert label == label2
        got = B.of_picture(pic, g, b)
        assert zlib.crc32(got.tobytes()) == crc, (name, label)
        if g[0] * g[1] <= 32 * 32 or (name in ("yuv444_13_portrait48x64", "yuv422_64x48") and label == "gauss1.5_12"):      # plain Python again: small clips, and every sampling
            assert ref.bilateral_picture(pic.tobytes(), g, ref.as_ref(b.luma), ref.as_ref(b.chroma)) == got.tobytes(), (name, label)


# ------------------------------------------------------------------------------------------------- argument checks without a device
class _NoDevice:
    """what Context.bilateral_pictures looks at before it reaches the library"""
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

    def bilateral_pictures(self, *a, **k):
        from hvqm4_amd.batch import Context
        return Context.bilateral_pictures(self, *a, **k)


def test_arguments_are_checked_before_the_library_is_called():
    import torch
    from hvqm4_amd._lib import HVQ_E_ARG, HvqError
    from hvqm4_amd.batch import Context
    call = lambda *a, **k: Context.bilateral_pictures(_NoDevice(), *a, **k)
    b = B.box(1)
    nb = 64 * 48 * 3 // 2
    with pytest.raises(ValueError, match="ordinals"):
        call([0, 0], [0], b)
    with pytest.raises(HvqError) as e:
        call([0, 7], [0, 0], b)
    assert e.value.code == HVQ_E_ARG
    for bil in (None, "box", [b], [b, None], b.luma):
        with pytest.raises(ValueError, match="bil"):
            call([0, 0], [0, 1], bil)
    # every refusal of hvq_bilateral_check
    P = B.PlaneBilateral
    with pytest.raises(ValueError, match="radius"):
        call([0], [0], B.Bilateral(P(8, 0, b.luma.spatial, b.luma.range), b.chroma))
    with pytest.raises(ValueError, match="radius"):
        call([0], [0], B.Bilateral(b.luma, P(0, -1, b.luma.spatial, b.luma.range)))
    with pytest.raises(ValueError, match="centre tap"):
        call([0], [0], B.Bilateral(P(1, 1, bytes(64), b.luma.range), b.chroma))
    with pytest.raises(ValueError, match="centre tap"):
        call([0], [0], B.Bilateral(b.luma, P(1, 1, b.luma.spatial, bytes(256))))
    with pytest.raises(ValueError, match="pad"):
        call([0], [0], B.Bilateral(P(1, 1, b.luma.spatial, b.luma.range, (7, 0)), b.chroma))
    with pytest.raises(ValueError, match="pad"):
        call([0, 0], [0, 1], [b, B.Bilateral(b.luma, P(1, 1, b.luma.spatial, b.luma.range, (0, 1)))])
    with pytest.raises(ValueError, match="tables"):
        call([0], [0], B.Bilateral(P(1, 1, b.luma.spatial, b.luma.range[:255]), b.chroma))
    # and of the call
    with pytest.raises(ValueError, match="65 distinct"):
        call([0] * 65, list(range(65)), cases.table64() + [B.box((7, 6))])
    with pytest.raises(ValueError, match="not a GPU"):                       # 64 distinct ones (each given twice): on to the next check
        call([0] * 128, list(range(128)), cases.table64() * 2, out=torch.zeros((128, 4608), dtype=torch.uint8))
    with pytest.raises(ValueError, match="1 sources for 2 pictures"):
        call([0, 0], [0, 1], b, src=[None])
    good = torch.zeros(nb, dtype=torch.uint8)
    with pytest.raises(ValueError, match="elements"):
        call([1], [-1], b, src=[good])
    room = torch.zeros(nb + 64, dtype=torch.uint8)
    off = (-room.data_ptr()) % 16
    with pytest.raises(ValueError, match="ordinal -1"):
        call([0], [0], b, src=[room[off:off + nb]])
    with pytest.raises(ValueError, match="multiple of 16"):
        call([0], [-1], b, src=[room[off + 8:off + 8 + nb]])
    with pytest.raises(ValueError, match="not a GPU"):
        call([0], [-1], b, src=[room[off:off + nb]])
    # the guides: picture_metrics' forms
    with pytest.raises(TypeError, match="list"):
        call([0], [0], b, guide=5)
    with pytest.raises(ValueError, match="1 references for 2 pictures"):
        call([0, 0], [0, 1], b, guide=[None])
    with pytest.raises(TypeError, match="pair of integers"):
        call([0], [0], b, guide=[(0, 1, 2)])
    with pytest.raises(ValueError, match="not negative"):
        call([0], [0], b, guide=[(0, -1)])
    with pytest.raises(TypeError, match="dtype"):
        call([0], [0], b, guide=[torch.zeros(nb, dtype=torch.int8)])
    with pytest.raises(ValueError, match="elements"):
        call([0], [0], b, guide=[torch.zeros(nb + 16, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="multiple of 16"):
        call([0], [0], b, guide=[room[off + 8:off + 8 + nb]])
    with pytest.raises(ValueError, match="reference 1 is on cpu"):
        call([0, 0], [0, 1], b, guide=[None, room[off:off + nb]])
    with pytest.raises(ValueError, match="out must be"):
        call([0, 0], [0, 1], b, out=torch.zeros((2, nb), dtype=torch.int32))
    with pytest.raises(ValueError, match="out must be"):
        call([0, 0], [0, 1], b, out=torch.zeros((2, nb + 16), dtype=torch.uint8))
    with pytest.raises(ValueError, match="out must be a list"):
        call([0, 1], [0, 1], b, out=torch.zeros((2, nb), dtype=torch.uint8))                           # two geometries: a list
    with pytest.raises(ValueError, match=r"out\[1\]"):
        call([0, 1], [0, 1], b, out=[torch.zeros(nb, dtype=torch.uint8)] * 2)
    with pytest.raises(ValueError, match="not a GPU"):
        call([0, 0], [0, 1], b, guide=[None, (2, 0)], out=torch.zeros((2, nb), dtype=torch.uint8))
    with pytest.raises(ValueError, match="65535"):
        call([0] * 65536, [0] * 65536, b)
    # smooth_pictures: its steps, then bilateral_pictures' checks
    smooth = lambda *a, **k: Context.smooth_pictures(_NoDevice(), *a, **k)
    for steps in ([], None, [b, "box"], b.luma):
        with pytest.raises(ValueError, match="steps"):
            smooth([0], [0], steps)
    with pytest.raises(ValueError, match="pad"):
        smooth([0], [0], [b, B.Bilateral(P(1, 1, b.luma.spatial, b.luma.range, (7, 0)), b.chroma)])
    with pytest.raises(ValueError, match="not a GPU"):
        smooth([0, 0], [0, 1], B.iterate(b, 1), out=torch.zeros((2, nb), dtype=torch.uint8))


def _spoiled():
    """(label, HvqBilateral struct) for every refusal of hvq_bilateral_check, in the chroma plane of an otherwise good entry"""
    out = []

    def bad(label, spoil):
        s = B.bilateral(1.5, 12).struct()
        spoil(s.chroma)
        out.append((label, s))

    def member(name, value):
        return lambda p: setattr(p, name, value)

    def entry(name, at, value):
        def spoil(p):
            t = getattr(p, name)
            for i in at[:-1]:
                t = t[i]
            t[at[-1]] = value
        return spoil
    bad("radius 8", member("rx", 8))
    bad("radius 8 in y", member("ry", 8))
    bad("a negative radius", member("ry", -1))
    bad("a negative radius in x", member("rx", -3))
    bad("spatial[0][0] == 0", entry("spatial", (0, 0), 0))
    bad("range[0] == 0", entry("range", (0,), 0))
    bad("pad", entry("pad", (0,), 1))
    bad("a negative pad", entry("pad", (1,), -1))
    return out


def test_the_library_without_a_device_still_checks_its_arguments():
    """no context can exist here, and the call says so before it looks at anything else (HVQ_E_ARG, not HVQ_E_NOGPU); the host-only check
    works"""
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, lib
    one = (C.c_int * 1)(0)
    b = B.box(1).struct()
    dst = (C.c_void_p * 1)(16)
    assert lib().hvq_bilateral_pictures(None, 1, one, one, None, None, C.byref(b), 1, None, C.cast(dst, C.c_void_p), None) == HVQ_E_ARG
    assert lib().hvq_bilateral_force_general(None, 1) == HVQ_E_ARG
    assert lib().hvq_bilateral_check(None) == HVQ_E_ARG
    for name, p in PLANES.items():
        assert lib().hvq_bilateral_check(C.byref(B.Bilateral(p, B.IDENTITY_PLANE).struct())) == 0, name
        assert lib().hvq_bilateral_check(C.byref(B.Bilateral(B.IDENTITY_PLANE, p).struct())) == 0, name
    for entry in cases.table64():
        assert lib().hvq_bilateral_check(C.byref(entry.struct())) == 0
    for label, s in _spoiled():
        assert lib().hvq_bilateral_check(C.byref(s)) == HVQ_E_ARG, label
        s.luma, s.chroma = s.chroma, s.luma
        assert lib().hvq_bilateral_check(C.byref(s)) == HVQ_E_ARG, label + " (luma)"


# ------------------------------------------------------------------------------------------------- the runtime on the CPU fake device
DRIVER_SETS = {                                                             # the first is well formed with both radii below 7 (the driver's malformed ones derive from it)
    "gauss": B.bilateral(1.5, 12), "identity": B.identity(), "sigma2_10": B.sigma_filter(2, 10), "box3x1": B.box((3, 1)), "disc3": B.disc(3),
    "luma_sigma3": B.luma_only(B.sigma_filter(3, 20)), "all255": cases.ALL255, "gauss7x0": B.bilateral(4.0, 30, (7, 0)), "gauss0x7": B.bilateral(4.0, 30, (0, 7)),
    "random": B.Bilateral(cases.random_set(1, 7, 7), cases.random_set(2, 5, 2)), "chroma_only": B.Bilateral(B.IDENTITY_PLANE, cases.random_set(3, 4, 6)),
    "step_keeper": cases.STEP_KEEPER, "gauss6_422": B.chroma_for(B.bilateral(3.0, 20, 6), 2, 1), "weight0": B.from_tables(0, 0, [[9]], [9] * 256),
}


def _sets_txt():
    plane = lambda p: f"{p.rx} {p.ry} {p.spatial.hex()} {p.range.hex()}"
    return "".join(f"{name} {plane(b.luma)} {plane(b.chroma)}\n" for name, b in DRIVER_SETS.items())


@pytest.fixture(scope="module")
def drivers():
    return {kind: fd.build_driver(kind, "bilateral", "fake_bilateral_driver", CXX_SOURCES, __file__) for kind in fd.BUILDS}


_want = {}


def _source(source, form, k, geom):
    """the picture the driver worked on, as the driver's line describes it"""
    n = cases.nbytes(geom)
    if form == "pic":
        return fd.oracle_pictures(source)[k].reshape(-1)
    if form == "inv":
        return 255 - fd.oracle_pictures(source)[k].reshape(-1)
    if form.startswith("smoothed:"):
        return _expected(source, "pic", k, geom, form.split(":", 1)[1], "self")[1]
    if form == "synth":
        return ((((np.arange(n, dtype=np.uint64) + np.uint64(k)) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(13)).astype(np.uint8)
    if form == "flat":
        return np.full(n, k, dtype=np.uint8)
    if form == "check":
        out = []
        for pw, ph in cases.plane_sizes(geom):
            y, x = np.mgrid[0:ph, 0:pw]
            out.append((((x + y + k) & 1) * 255).astype(np.uint8).reshape(-1))
        return np.concatenate(out)
    raise AssertionError(form)


def _guide(gform, source, pic, geom):
    if gform == "self":
        return None
    if gform == "copy":
        return pic.copy()
    if gform == "inv":
        return 255 - pic
    if gform.startswith("res"):
        return fd.oracle_pictures(source)[int(gform[3:])].reshape(-1)
    if gform.startswith("flat"):
        return np.full(cases.nbytes(geom), int(gform[4:]), dtype=np.uint8)
    raise AssertionError(gform)


def _expected(source, form, k, geom, sname, gform):
    key = (source, form, k, geom, sname, gform)
    if key not in _want:
        pic = _source(source, form, k, geom)
        got = B.of_picture(pic, geom, DRIVER_SETS[sname], _guide(gform, source, pic, geom))
        _want[key] = (zlib.crc32(got.tobytes()), got)
    return _want[key]


def _run(exe, scenario, schedule, tmp_path):
    _, lines = fd.run_checked(exe, scenario, schedule, tmp_path, inputs={"sets.txt": _sets_txt()})
    P, Rc, S = {}, {}, {}
    for line in lines:
        f = line.split()
        if f[0] == "P":
            label, source, form, k, geom, sname, gform = f[1], f[2], f[3], int(f[4]), tuple(int(v) for v in f[5:9]), f[9], f[10]
            assert int(f[12]) == 1, f"{label}: the bytes around the output of {source} {k} were written"
            want = _expected(source, form, k, geom, sname, gform)[0]
            assert int(f[11]) == want, f"{label}: picture {k} of {source} ({form}) {geom} through {sname} guided by {gform}: crc {int(f[11]):08x}, want {want:08x}"
            P.setdefault(label, []).append((source, form, k, geom, sname, gform))
        elif f[0] == "R":
            Rc[f[1]] = int(f[2])
        elif f[0] == "S":
            S[f[1]] = (int(f[2]), int(f[3]))
    return P, Rc, S, fd.refusal_texts(lines)


def _check_memory(P, Rc, S, E):
    ns = len(DRIVER_SETS)
    assert P["memory"] == P["memory/nullstream"] and len(P["memory"]) == 2 * fd.n_pics("yuv422_64x48") + 7 * (2 * ns + 1)
    forms = [f for _s, f, *_r in P["memory"]]
    assert forms.count("inv") == fd.n_pics("yuv422_64x48") and forms.count("check") == 7 * ns and forms.count("flat") == 7
    geoms = {g for _s, f, _k, g, _n, _g in P["memory"] if f == "check"}
    assert {(8, 8, 2, 2), (8, 8, 2, 1), (8, 8, 1, 1), (72, 24, 2, 2), (136, 40, 2, 2)} <= geoms, "planes narrower than the halo and than the window"
    assert {gf for *_r, gf in P["memory"]} == {"self"}


def _check_guides(P, Rc, S, E):
    ns = len(DRIVER_SETS)
    assert P["guides"] == P["guides/general"] and len(P["guides"]) == 3 * (ns + 1)
    kinds = {gf.rstrip("0123456789") for *_r, gf in P["guides"]}
    assert kinds == {"self", "copy", "res", "flat", "inv"}
    assert {g[2:] for _s, _f, _k, g, _n, _g in P["guides"]} == {(2, 2), (2, 1), (1, 1)}
    assert any(g[0] > 128 for _s, _f, _k, g, _n, _g in P["guides"]), "tile seams inside a plane"
    assert Rc == {"guides/force": 0, "guides/unforce": 1}
    assert sum(1 for b in DRIVER_SETS.values() if B.copies(b.luma) or B.copies(b.chroma)) >= 4
    # guided by a copy of itself: the unguided bytes; another picture as the guide gives other bytes
    for source, form, k, geom, sname, gform in P["guides"]:
        if gform == "copy":
            assert _expected(source, form, k, geom, sname, gform)[0] == _expected(source, form, k, geom, sname, "self")[0]
            if gform == "inv":                                              # |(255 - a) - (255 - b)| == |a - b|: an inverted copy guides as the picture itself
                assert _expected(source, form, k, geom, sname, gform)[0] == _expected(source, form, k, geom, sname, "self")[0]
    assert any(gf.startswith("res") and _expected(s, f, k, g, n, gf)[0] != _expected(s, f, k, g, n, "self")[0] for s, f, k, g, n, gf in P["guides"]), "a guide changes the bytes"


def _check_reuse(P, Rc, S, E):
    from hvqm4_amd._lib import HVQ_E_STATE
    n, ne = fd.n_pics("gop64x48_15"), fd.n_pics("yuv444_64x48")
    g = _clip_geometry("gop64x48_15")
    names = list(DRIVER_SETS)
    assert P["reuse"] == [("gop64x48_15", "pic", k, g, names[1], f"res{(k + 1) % n}" if k & 1 else "self") for k in range(n)]
    assert Rc["reuse/evicted"] == HVQ_E_STATE and Rc["reuse/evicted_guide"] == HVQ_E_STATE, "the flushes did not hand the slots of the first pass on: the scenario tests nothing"
    assert P["reuse/chain"] == [("gop64x48_15", "smoothed:" + names[1], k, g, names[2], "self") for k in range(0, n, 2)]
    assert P["reuse/late"] == [("gop64x48_15", "pic", k, g, names[1], "self") for k in range(n)]
    assert [(s, k) for s, _f, k, *_r in P["reuse/destroy"]] == [("yuv444_64x48", k) for k in range(ne)]


def _check_refused(P, Rc, S, E):
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_STATE
    arg = ["null_context", "bad_stream", "bad_ordinal", "misaligned_src", "src_with_ordinal", "src_with_bad_stream", "minus_one_without_src", "null_dst",
           "misaligned_dst", "too_many", "null_sets", "nsets_0", "nsets_65", "which_high", "which_negative", "force_null", "check_null",
           "guide_other_geometry", "guide_stream_and_pointer", "guide_misaligned", "guide_stream_minus_2", "guide_bad_stream", "guide_bad_ordinal"]
    spoiled = ["radius_8", "radius_8_y", "radius_negative", "spatial_0", "range_0", "pad", "pad_1"]
    want = {k: HVQ_E_ARG for k in arg + spoiled + ["check_" + s for s in spoiled]}
    want.update({"evicted": HVQ_E_STATE, "queued": HVQ_E_STATE, "guide_evicted": HVQ_E_STATE, "guide_queued": HVQ_E_STATE, "n0": 0, "check_good": 0})
    assert Rc == {"refused/" + k: v for k, v in want.items()}
    # the guides are refused in picture_reference's words
    assert "has not the geometry of stream" in E["guide_other_geometry"] and "a resident reference takes no pointer" in E["guide_stream_and_pointer"]
    assert "reference 1: the pointer must be a multiple of 16" in E["guide_misaligned"] and "or zeros" in E["guide_stream_minus_2"]
    assert "set 1 of 1" in E["which_high"] and "65 sets" in E["nsets_65"] and "radii" in E["radius_8"] and "centre tap" in E["spatial_0"] and "pad" in E["pad_1"]
    same, total = S["refused"]
    assert same == total == 2 * 4608 + 16, "a refused call wrote its output"
    g = _clip_geometry("gop64x48_15")
    names = list(DRIVER_SETS)
    assert P["refused/then_ok"] == [("gop64x48_15", "pic", 1, g, names[63 % len(names)], "res2"), ("gop64x48_15", "pic", fd.n_pics("gop64x48_15") - 1, g, names[0], "self")]


CHECKS = {"memory": _check_memory, "guides": _check_guides, "reuse": _check_reuse, "refused": _check_refused}


@pytest.mark.parametrize("schedule", ["eager", "late"])
@pytest.mark.parametrize("build", list(fd.BUILDS))
@pytest.mark.parametrize("scenario", list(CHECKS))
def test_fake_device_scenario(drivers, scenario, build, schedule, tmp_path):
    CHECKS[scenario](*_run(drivers[build], scenario, schedule, tmp_path))


@pytest.mark.parametrize("schedule", ["eager", "late"])
def test_fake_device_without_the_bilateral_body_refuses(schedule, tmp_path):
    """a driver linked without fake_bilateral.cpp: the runtime's reference is weak, the call checks first and then says HVQ_E_NOGPU"""
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_NOGPU
    exe = fd.build_driver("plain", "bilateral_nogpu", "fake_bilateral_driver", [s for s in CXX_SOURCES if not s.endswith("fake_bilateral.cpp")], __file__)
    P, Rc, S, E = _run(exe, "nogpu", schedule, tmp_path)
    assert Rc == {"nogpu/bad_which": HVQ_E_ARG, "nogpu/bad_set": HVQ_E_ARG, "nogpu/bad_guide": HVQ_E_ARG, "nogpu/well_formed": HVQ_E_NOGPU, "nogpu/n0": 0}
    assert "no bilateral kernel" in E["well_formed"] and "hvq_bilateral.hip is not linked" in E["well_formed"]
    assert not P and S["nogpu"][0] == S["nogpu"][1] == 4608 + 512, "a refused call wrote its output"


def test_the_reuse_chain_is_two_steps_in_two_calls():
    """what `reuse/chain` computes is a chain through src=: the expected bytes of the second call are of_steps of the two entries"""
    names = list(DRIVER_SETS)
    pic = fd.oracle_pictures("gop64x48_15")[0].reshape(-1)
    g = _clip_geometry("gop64x48_15")
    assert np.array_equal(_expected("gop64x48_15", "smoothed:" + names[1], 0, g, names[2], "self")[1], B.of_steps(pic, g, [DRIVER_SETS[names[1]], DRIVER_SETS[names[2]]]))


def test_the_existing_fake_builds_link_without_the_bilateral_body():
    """the source lists of the other drivers have no hvq_launch_bilateral: the runtime's reference is weak"""
    assert not any("fake_bilateral" in s for s in fd.CXX_SOURCES)
    text = open(os.path.join(fd.CSRC, "hvq_runtime.cpp")).read()
    decl = [l for l in text.splitlines() if "hvq_launch_bilateral(" in l and l.startswith("extern")]
    assert len(decl) == 1 and "weak" in decl[0]
    exe = fd.build_driver("plain", "fake", "fake_driver", fd.CXX_SOURCES, fd.__file__)
    assert os.access(exe, os.X_OK)


# ------------------------------------------------------------------------------------------------- tools/bench_bilateral.py, tools/denoise.py
def _tool(name):
    sys.path.insert(0, os.path.join(fd.ROOT, "tools"))
    try:
        return __import__(name)
    finally:
        sys.path.remove(os.path.join(fd.ROOT, "tools"))


def _bench_trace(tmp_path, drop=0):
    sys.path.insert(0, fd.GOLDEN)
    try:
        import make_bench_tools as mk
    finally:
        sys.path.remove(fd.GOLDEN)
    tool = _tool("bench_bilateral")
    blocks = [mk.block(kernel) for _label, kernel in tool.trace_plan()]
    if drop:
        blocks[-1] = blocks[-1][:-drop]
    d = str(tmp_path / "trace")
    mk.write_trace(d, blocks)
    taps = {label: [b.luma.taps(), b.chroma.taps()] for label, b in tool.the_sets()}
    return tool, mk, d, {"launches": 1 + mk.REPS, "pictures": 1024, "content": "natural", "taps": taps}


def test_bench_bilateral_imports_without_a_gpu_and_reads_a_synthetic_trace(tmp_path):
    tool, mk, d, printed = _bench_trace(tmp_path)
    assert "torch" not in tool.__dict__ and callable(tool.main)
    labels = [label for label, _k in tool.trace_plan()]
    assert labels[:11] == ["wide_r1", "wide_r2", "wide_r3", "wide_r5", "wide_r7", "gauss_r2", "square5", "disc5", "identity", "identity_general", "gauss_r2_guided"]
    assert labels[11:] == ["scale_identity", "filter_gauss_r2", "median5"] and labels[:11] == [label for label, _b in tool.the_sets()]
    assert [printed["taps"][f"wide_r{r}"][0] for r in tool.RADII] == [(2 * r + 1) ** 2 for r in tool.RADII], "no tap of the wide Gaussians rounds to 0"
    assert printed["taps"]["square5"] == [121, 121] and printed["taps"]["disc5"] == [97, 97] and printed["taps"]["gauss_r2"] == [25, 25]
    res = tool.trace_summary(d, printed)
    assert "error" not in res, res
    # block b of the helper: a warm-up launch and three of base, base + 1234, base + 4321 ns, base = 100000 + 7919 b
    for b, label in enumerate(labels):
        base = 100_000 + 7_919 * b
        assert res[label]["launches"] == mk.REPS and res[label]["median_us"] == round((base + 1_234) / 1e3, 1), label
        assert res[label]["min_us"] == round(base / 1e3, 1) and res[label]["max_us"] == round((base + 4_321) / 1e3, 1), label
    med = lambda label: res[label]["median_us"]
    assert res["wide_r7"]["over_scale_identity_kernel"] == round(med("wide_r7") / med("scale_identity"), 2)
    assert res["us_per_tap"]["r1_to_r2"] == round((med("wide_r2") - med("wide_r1")) / 16, 2) and res["us_per_tap"]["r5_to_r7"] == round((med("wide_r7") - med("wide_r5")) / 104, 2)
    assert res["ratios"]["gauss_r2_over_median5"] == round(med("gauss_r2") / med("median5"), 2)
    assert res["ratios"]["guided_over_unguided"] == round(med("gauss_r2_guided") / med("gauss_r2"), 2)
    c = res["condition_2"]
    assert (c["disc5_us"], c["square5_us"], c["tap_ratio"]) == (med("disc5"), med("square5"), round(97 / 121, 3)) and c["holds"] is False, "the helper's disc block is the later, slower one"
    assert (res["vgprs"], res["lds"], res["scratch"]) == ("8", "0", "0")


def test_bench_bilateral_refuses_a_trace_with_one_launch_too_few(tmp_path):
    tool, _mk, d, printed = _bench_trace(tmp_path, drop=1)
    res = tool.trace_summary(d, printed)
    assert "error" in res and "planned" in res["error"]


def test_denoise_builds_its_steps_without_a_gpu():
    tool = _tool("denoise")
    assert "torch" not in tool.__dict__ and callable(tool.main) and callable(tool.clip_denoised)
    assert tool.steps_for(1.5, 12.0, None, 2, None, 2, 2) == [B.chroma_for(B.bilateral(1.5, 12.0), 2, 2)] * 2
    assert tool.steps_for(1.5, 12.0, 5, 1, None, 1, 1) == [B.bilateral(1.5, 12.0, 5)]
    assert tool.steps_for(3.0, 12.0, None, 1, 7, 2, 1) == [B.chroma_for(B.sigma_filter(6, 7), 2, 1)]
