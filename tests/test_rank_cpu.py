"""CPU: the values of hvq_rank_pictures.  tests/rank_ref.py restates include/hvqm4_amd.h in plain Python; hvqm4_amd.rank (numpy), the
fixture tests/golden/rank.json and the runtime on the CPU fake device (tests/native/fake_rank.cpp, which walks the kernel's grid with
the phases and the body choice of hvq_rank.h) are compared with it by ==.  The fake-device driver is a stand-alone program, built and run
plain and with ASan + UBSan as tests/test_compose_cpu.py builds its own; nothing is preloaded and no Python is involved in the
sanitised run."""
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import pytest

import tests.test_fake_device as fd
from hvqm4_amd import rank as R
from tests import rank_cases as cases
from tests import rank_ref as ref

NATIVE = fd.NATIVE
CXX_SOURCES = [s for s in fd.CXX_SOURCES if os.path.basename(s) != "fake_driver.cpp"] + \
              [os.path.join(NATIVE, "fake_rank.cpp"), os.path.join(NATIVE, "fake_rank_driver.cpp")]
FIXTURE = json.load(open(os.path.join(fd.GOLDEN, "rank.json")))

PLANES = {"identity": R.IDENTITY_PLANE, "max0": R.PlaneRank(R.MAX), "range0": R.PlaneRank(R.RANGE), "median1": R.PlaneRank(R.MEDIAN),
          "erode1": R.erode(1).luma, "erode2x0": R.erode((2, 0)).luma, "erode0x2": R.erode((0, 2)).luma, "erode15": R.erode(15).luma,
          "erode7x3": R.erode((7, 3)).luma, "dilate1": R.dilate(1).luma, "dilate3x1": R.dilate((3, 1)).luma, "dilate15x0": R.dilate((15, 0)).luma,
          "dilate0x15": R.dilate((0, 15)).luma, "dilate4": R.dilate(4).luma, "range1": R.gradient(1).luma, "range2": R.gradient(2).luma,
          "range15x7": R.gradient((15, 7)).luma, "median3": R.median(3).luma, "median5": R.median(5).luma}


def _ref_plane(a, p):
    return np.array(ref.rank_plane([bytes(r) for r in np.asarray(a, dtype=np.uint8)], *ref.as_ref(p)), dtype=np.uint8)


def _both(a, p):
    """the module's answer, which must be the reference's, as lists"""
    a = np.array(a, dtype=np.uint8)
    got = R.of_plane(a, p)
    assert np.array_equal(got, _ref_plane(a, p))
    return got.tolist()


def _plane_contents(nx, ny, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:ny, 0:nx]
    return [rng.integers(0, 256, (ny, nx), dtype=np.uint8), rng.integers(0, 4, (ny, nx)).astype(np.uint8), (((x + y) & 1) * 255).astype(np.uint8)]


@pytest.mark.parametrize("name", sorted(PLANES))
def test_module_equals_reference(name):
    p = PLANES[name]
    for (nx, ny), seed in (((12, 8), 1), ((4, 4), 2), ((8, 20), 3)):           # 4 x 4 under radius 15: the clamp repeats
        for a in _plane_contents(nx, ny, seed):
            assert np.array_equal(R.of_plane(a, p), _ref_plane(a, p)), (name, nx, ny)


@pytest.mark.parametrize("geom", [(16, 8, 2, 2), (16, 8, 2, 1), (8, 16, 1, 1)])
def test_module_equals_reference_on_pictures_of_the_three_samplings(geom):
    pic = cases.made(geom, "random", 5)
    for rank in (R.chroma_for(R.erode(2), *geom[2:]), R.luma_only(R.median(5)), R.Rank(R.median(3).luma, R.gradient((1, 2)).luma)):
        want = ref.rank_picture(pic.tobytes(), geom, ref.as_ref(rank.luma), ref.as_ref(rank.chroma))
        assert R.of_picture(pic, geom, rank).tobytes() == want, (geom, rank)
    steps = R.opening((2, 1))
    assert R.of_steps(pic, geom, steps).tobytes() == ref.steps_picture(pic.tobytes(), geom, [(ref.as_ref(s.luma), ref.as_ref(s.chroma)) for s in steps])


def test_known_answers():
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, (7, 9), dtype=np.uint8)
    # radius 0 copies the plane under MIN, MAX and MEDIAN, and gives all zeros under RANGE
    for op in (R.MIN, R.MAX, R.MEDIAN):
        assert _both(a, R.PlaneRank(op)) == a.tolist()
    assert _both(a, R.PlaneRank(R.RANGE)) == np.zeros((7, 9), dtype=int).tolist()
    # a flat plane stays flat, and RANGE of a flat plane is 0
    flat = np.full((6, 7), 201, dtype=np.uint8)
    for name, p in PLANES.items():
        assert _both(flat, p) == (np.zeros((6, 7), dtype=int) if p.op == R.RANGE else flat).tolist(), name
    # a single 0 in a plane of 255 under MIN: exactly the rectangle, cut at the plane; a 255 in zeros under MAX likewise
    for (y, x), (rx, ry) in (((3, 4), (2, 1)), ((0, 0), (1, 3)), ((6, 8), (15, 2)), ((2, 8), (0, 1)), ((5, 1), (3, 0))):
        dot = np.full((7, 9), 255, dtype=np.uint8)
        dot[y, x] = 0
        want = np.full((7, 9), 255, dtype=np.uint8)
        want[max(y - ry, 0):y + ry + 1, max(x - rx, 0):x + rx + 1] = 0
        assert _both(dot, R.PlaneRank(R.MIN, rx, ry)) == want.tolist(), (y, x, rx, ry)
        assert _both(255 - dot, R.PlaneRank(R.MAX, rx, ry)) == (255 - want).tolist(), (y, x, rx, ry)
    # a single outlier vanishes under MEDIAN 3 x 3
    out = np.full((5, 5), 17, dtype=np.uint8)
    out[2, 2] = 255
    assert _both(out, R.median(3).luma) == np.full((5, 5), 17).tolist()
    out[2, 2] = 0
    assert _both(out, R.median(3).luma) == np.full((5, 5), 17).tolist()
    # MEDIAN 3 x 3 of {0, 0, 0; 0, 255, 255; 255, 255, 255} at its centre is 255
    assert _both([[0, 0, 0], [0, 255, 255], [255, 255, 255]], R.median(3).luma)[1][1] == 255
    # at a corner of the plane the corner sample counts four times
    assert sorted(ref.window([[9, 1], [1, 1]], 0, 0, 1, 1)) == [1, 1, 1, 1, 1, 9, 9, 9, 9]
    assert _both([[9, 1], [1, 1]], R.median(3).luma)[0][0] == 1 and _both([[9, 9], [1, 1]], R.median(3).luma)[0][0] == 9
    assert (len(ref.window(a.tolist(), 0, 0, 2, 2)) - 1) // 2 == 12


@pytest.mark.parametrize("seed", range(3))
def test_identities_of_the_reference(seed):
    """the reference against itself, independent of any kernel"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (9, 11), dtype=np.uint8) if seed else rng.integers(0, 3, (9, 11)).astype(np.uint8) * 127
    rows = [bytes(r) for r in a]
    inv = [bytes(255 - v for v in r) for r in rows]
    for rx, ry in ((1, 1), (3, 0), (0, 2), (15, 4)):
        lo, hi = ref.rank_plane(rows, ref.MIN, rx, ry), ref.rank_plane(rows, ref.MAX, rx, ry)
        assert hi == [[255 - v for v in r] for r in ref.rank_plane(inv, ref.MIN, rx, ry)], "MAX == 255 - MIN(255 - .)"
        assert all(l <= v <= h for rl, rv, rh in zip(lo, rows, hi) for l, v, h in zip(rl, rv, rh)), "MIN <= a <= MAX"
        assert ref.rank_plane(rows, ref.RANGE, rx, ry) == [[h - l for l, h in zip(rl, rh)] for rl, rh in zip(lo, hi)]
        # a rectangle equals rows then columns
        assert lo == ref.rank_plane(ref.rank_plane(rows, ref.MIN, rx, 0), ref.MIN, 0, ry)
        assert hi == ref.rank_plane(ref.rank_plane(rows, ref.MAX, rx, 0), ref.MAX, 0, ry)
        # opening is idempotent
        opened = ref.rank_plane(lo, ref.MAX, rx, ry)
        assert ref.rank_plane(ref.rank_plane(opened, ref.MIN, rx, ry), ref.MAX, rx, ry) == opened
    for r in (1, 2):
        m = ref.rank_plane(rows, ref.MEDIAN, r, r)
        assert ref.rank_plane(inv, ref.MEDIAN, r, r) == [[255 - v for v in line] for line in m], "MEDIAN(255 - a) == 255 - MEDIAN(a)"


def test_struct_layout():
    import ctypes as C
    from hvqm4_amd._lib import HvqRank, HvqRankPlane
    assert (C.sizeof(HvqRankPlane), C.sizeof(HvqRank)) == (16, 32)
    assert [(n, getattr(HvqRankPlane, n).offset) for n, _t in HvqRankPlane._fields_] == [("op", 0), ("rx", 4), ("ry", 8), ("pad", 12)]
    assert HvqRank.luma.offset == 0 and HvqRank.chroma.offset == 16
    s = R.Rank(R.PlaneRank(R.RANGE, 7, 3), R.PlaneRank(R.MEDIAN, 2, 2)).struct()
    assert (s.luma.op, s.luma.rx, s.luma.ry, s.luma.pad, s.chroma.op, s.chroma.rx, s.chroma.ry, s.chroma.pad) == (2, 7, 3, 0, 3, 2, 2, 0)
    assert (R.MIN, R.MAX, R.RANGE, R.MEDIAN, R.MAX_RADIUS, R.MAX_RANKS) == (0, 1, 2, 3, 15, 64)
    header = open(os.path.join(fd.ROOT, "include", "hvqm4_amd.h")).read()
    for line in ("#define HVQ_RNK_MIN    0", "#define HVQ_RNK_MAX    1", "#define HVQ_RNK_RANGE  2", "#define HVQ_RNK_MEDIAN 3", "#define HVQ_RNK_MAX_RADIUS 15",
                 "#define HVQ_RNK_MAX_RANKS  64", "typedef struct HvqRankPlane { int32_t op, rx, ry, pad; } HvqRankPlane;"):
        assert line in header, line


def test_builders():
    assert R.erode(2) == R.Rank(R.PlaneRank(R.MIN, 2, 2), R.PlaneRank(R.MIN, 2, 2)) and R.erode((3, 1)).luma == R.PlaneRank(R.MIN, 3, 1)
    assert R.dilate(1).luma.op == R.MAX and R.gradient((0, 4)).chroma == R.PlaneRank(R.RANGE, 0, 4)
    assert R.median(3).luma == R.PlaneRank(R.MEDIAN, 1, 1) and R.median(5).chroma == R.PlaneRank(R.MEDIAN, 2, 2)
    assert R.identity().luma == R.IDENTITY_PLANE and R.copies(R.identity().chroma) and R.copies(R.PlaneRank(R.MEDIAN)) and not R.copies(R.PlaneRank(R.RANGE))
    assert R.luma_only(R.median(5)) == R.Rank(R.PlaneRank(R.MEDIAN, 2, 2), R.IDENTITY_PLANE)
    # the chroma radius follows the sampling and never drops below 1 when the luma radius is at least 1
    assert R.chroma_for(R.erode(6), 2, 2).chroma == R.PlaneRank(R.MIN, 3, 3) and R.chroma_for(R.erode(6), 2, 2).luma == R.erode(6).luma
    assert R.chroma_for(R.erode(6), 2, 1).chroma == R.PlaneRank(R.MIN, 3, 6)
    assert R.chroma_for(R.erode(6), 1, 1).chroma == R.PlaneRank(R.MIN, 6, 6)
    assert R.chroma_for(R.dilate(1), 2, 2).chroma == R.PlaneRank(R.MAX, 1, 1) and R.chroma_for(R.dilate((1, 0)), 2, 2).chroma == R.PlaneRank(R.MAX, 1, 0)
    assert R.chroma_for(R.gradient((5, 1)), 2, 1).chroma == R.PlaneRank(R.RANGE, 2, 1)
    assert R.chroma_for(R.median(5), 2, 2).chroma == R.PlaneRank(R.MEDIAN, 1, 1) and R.chroma_for(R.median(5), 2, 1).chroma == R.PlaneRank(R.MEDIAN, 1, 1)
    assert R.chroma_for(R.median(5), 1, 1).chroma == R.PlaneRank(R.MEDIAN, 2, 2) and R.chroma_for(R.median(3), 2, 2).chroma == R.PlaneRank(R.MEDIAN, 1, 1)
    assert R.opening(2) == [R.erode(2), R.dilate(2)] and R.closing((3, 1)) == [R.dilate((3, 1)), R.erode((3, 1))]
    assert len({R.erode(1), R.erode((1, 1)), R.dilate(1)}) == 2 and hash(R.median(3)) == hash(R.median(3))
    assert R.as_steps(R.erode(1)) == [R.erode(1)] and R.as_steps(R.opening(1)) == R.opening(1)
    for bad in (lambda: R.erode(16), lambda: R.erode(-1), lambda: R.dilate((1, 2, 3)), lambda: R.gradient(1.5), lambda: R.median(7), lambda: R.median(1),
                lambda: R.chroma_for(R.erode(1), 1, 2), lambda: R.check(R.Rank(R.PlaneRank(R.MEDIAN, 1, 2), R.IDENTITY_PLANE)),
                lambda: R.check(R.Rank(R.IDENTITY_PLANE, R.PlaneRank(R.MEDIAN, 3, 3))), lambda: R.check(R.Rank(R.PlaneRank(4), R.IDENTITY_PLANE)),
                lambda: R.check(R.Rank(R.PlaneRank(R.MIN, 0, 0, 1), R.IDENTITY_PLANE)), lambda: R.check(R.erode(1).luma), lambda: R.as_steps([]),
                lambda: R.as_steps([R.erode(1), None]), lambda: R.of_plane(np.zeros((2, 2)), R.IDENTITY_PLANE)):
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
        assert [l for l, _c in entry["sets"]] == [l for l, _r in cases.FIVE]


def test_the_generator_names_the_shared_parameter_sets():
    sys.path.insert(0, fd.GOLDEN)
    try:
        import make_rank
    finally:
        sys.path.remove(fd.GOLDEN)
    assert make_rank.SETS == [(label, ref.as_ref(r.luma)) for label, r in cases.FIVE] and all(r.luma == r.chroma for _l, r in cases.FIVE)


@pytest.mark.parametrize("name", sorted(FIXTURE["clips"]))
def test_fixture_equals_reference_and_module(name):
    entry = FIXTURE["clips"][name]
    g = tuple(entry["geometry"])
    pic = fd.oracle_pictures(name)[0]
    assert hashlib.sha256(pic.tobytes()).hexdigest() == fd.CLIPS[name]["picture_sha256"][0], "the fixture describes the manifest's picture"
    for (label, crc), (label2, r) in zip(entry["sets"], cases.FIVE):
        assert label == label2
        got = R.of_picture(pic, g, r)
        assert zlib.crc32(got.tobytes()) == crc, (name, label)
        if g[0] * g[1] <= 64 * 48:                                          # plain Python again: the small clips, every sampling among them
            assert ref.rank_picture(pic.tobytes(), g, ref.as_ref(r.luma), ref.as_ref(r.chroma)) == got.tobytes(), (name, label)


def test_the_reference_meets_clips_of_every_sampling():
    small = {tuple(e["geometry"])[2:] for e in FIXTURE["clips"].values() if e["geometry"][0] * e["geometry"][1] <= 64 * 48}
    assert small == {(2, 2), (2, 1), (1, 1)}


# ------------------------------------------------------------------------------------------------- argument checks without a device
class _NoDevice:
    """what Context.rank_pictures looks at before it reaches the library"""
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

    def rank_pictures(self, *a, **k):
        from hvqm4_amd.batch import Context
        return Context.rank_pictures(self, *a, **k)


def test_arguments_are_checked_before_the_library_is_called():
    import torch
    from hvqm4_amd._lib import HVQ_E_ARG, HvqError
    from hvqm4_amd.batch import Context
    call = lambda *a, **k: Context.rank_pictures(_NoDevice(), *a, **k)
    r = R.erode(1)
    with pytest.raises(ValueError, match="ordinals"):
        call([0, 0], [0], r)
    with pytest.raises(HvqError) as e:
        call([0, 7], [0, 0], r)
    assert e.value.code == HVQ_E_ARG
    for rank in (None, "erode", [r], [r, None], r.luma):
        with pytest.raises(ValueError, match="rank"):
            call([0, 0], [0, 1], rank)
    # every refusal of hvq_rank_check
    with pytest.raises(ValueError, match="op 4"):
        call([0], [0], R.Rank(R.PlaneRank(4), r.chroma))
    with pytest.raises(ValueError, match="op -1"):
        call([0], [0], R.Rank(r.luma, R.PlaneRank(-1)))
    with pytest.raises(ValueError, match="radius"):
        call([0], [0], R.Rank(R.PlaneRank(R.MIN, 16, 0), r.chroma))
    with pytest.raises(ValueError, match="radius"):
        call([0], [0], R.Rank(r.luma, R.PlaneRank(R.MAX, 0, -1)))
    with pytest.raises(ValueError, match="median"):
        call([0], [0], R.Rank(R.PlaneRank(R.MEDIAN, 1, 2), r.chroma))
    with pytest.raises(ValueError, match="median"):
        call([0], [0], R.Rank(r.luma, R.PlaneRank(R.MEDIAN, 3, 3)))
    with pytest.raises(ValueError, match="pad"):
        call([0], [0], R.Rank(R.PlaneRank(R.MIN, 1, 1, 7), r.chroma))
    with pytest.raises(ValueError, match="pad"):
        call([0, 0], [0, 1], [r, R.Rank(R.PlaneRank(R.MIN, 1, 1, 7), r.chroma)])
    # and of the call
    with pytest.raises(ValueError, match="65 distinct"):
        call([0] * 65, list(range(65)), cases.table64() + [R.Rank(R.PlaneRank(R.RANGE, 9, 9), R.PlaneRank(R.RANGE, 9, 8))])
    with pytest.raises(ValueError, match="not a GPU"):                       # 64 distinct ones (each given twice): on to the next check
        call([0] * 128, list(range(128)), cases.table64() * 2, out=torch.zeros((128, 4608), dtype=torch.uint8))
    with pytest.raises(ValueError, match="1 sources for 2 pictures"):
        call([0, 0], [0, 1], r, src=[None])
    good = torch.zeros(64 * 48 * 3 // 2, dtype=torch.uint8)
    with pytest.raises(ValueError, match="elements"):
        call([1], [-1], r, src=[good])
    room = torch.zeros(64 * 48 * 3 // 2 + 64, dtype=torch.uint8)
    off = (-room.data_ptr()) % 16
    with pytest.raises(ValueError, match="ordinal -1"):
        call([0], [0], r, src=[room[off:off + good.numel()]])
    with pytest.raises(ValueError, match="multiple of 16"):
        call([0], [-1], r, src=[room[off + 8:off + 8 + good.numel()]])
    with pytest.raises(ValueError, match="not a GPU"):
        call([0], [-1], r, src=[room[off:off + good.numel()]])
    nb = 64 * 48 * 3 // 2
    with pytest.raises(ValueError, match="out must be"):
        call([0, 0], [0, 1], r, out=torch.zeros((2, nb), dtype=torch.int32))
    with pytest.raises(ValueError, match="out must be"):
        call([0, 0], [0, 1], r, out=torch.zeros((2, nb + 16), dtype=torch.uint8))
    with pytest.raises(ValueError, match="out must be"):
        call([0, 0], [0, 1], r, out=[torch.zeros(nb, dtype=torch.uint8)] * 2)                          # one geometry: one tensor
    with pytest.raises(ValueError, match="out must be a list"):
        call([0, 1], [0, 1], r, out=torch.zeros((2, nb), dtype=torch.uint8))                           # two geometries: a list
    with pytest.raises(ValueError, match=r"out\[1\]"):
        call([0, 1], [0, 1], r, out=[torch.zeros(nb, dtype=torch.uint8)] * 2)
    with pytest.raises(ValueError, match="multiple of 16"):
        room = torch.zeros(2 * nb + 64, dtype=torch.uint8)
        off = (-room.data_ptr()) % 16 + 8
        call([0, 0], [0, 1], r, out=room[off:off + 2 * nb].view(2, nb))
    with pytest.raises(ValueError, match="not a GPU"):
        call([0, 0], [0, 1], r, out=torch.zeros((2, nb), dtype=torch.uint8))
    with pytest.raises(ValueError, match="65535"):
        call([0] * 65536, [0] * 65536, r)
    # morph_pictures: its steps, then rank_pictures' checks
    morph = lambda *a, **k: Context.morph_pictures(_NoDevice(), *a, **k)
    for steps in ([], None, [r, "dilate"], r.luma):
        with pytest.raises(ValueError, match="steps"):
            morph([0], [0], steps)
    with pytest.raises(ValueError, match="pad"):
        morph([0], [0], [r, R.Rank(R.PlaneRank(R.MIN, 1, 1, 7), r.chroma)])
    with pytest.raises(ValueError, match="not a GPU"):
        morph([0, 0], [0, 1], R.opening(1)[:1], out=torch.zeros((2, nb), dtype=torch.uint8))


def _spoiled():
    """(label, HvqRank struct) for every refusal of hvq_rank_check, in the chroma plane of an otherwise good entry"""
    out = []

    def bad(label, **members):
        s = R.erode(1).struct()
        for k, v in members.items():
            setattr(s.chroma, k, v)
        out.append((label, s))
    bad("op 4", op=4)
    bad("op -1", op=-1)
    bad("radius 16", rx=16)
    bad("radius 16 in y", ry=16)
    bad("a negative radius", ry=-1)
    bad("median with rx != ry", op=R.MEDIAN, rx=1, ry=2)
    bad("median of radius 3", op=R.MEDIAN, rx=3, ry=3)
    bad("median of radius 15", op=R.MEDIAN, rx=15, ry=15)
    bad("pad", pad=1)
    bad("a negative pad", pad=-1)
    return out


def test_the_library_without_a_device_still_checks_its_arguments():
    """no context can exist here, and the call says so before it looks at anything else (HVQ_E_ARG, not HVQ_E_NOGPU); the host-only check
    works"""
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, lib
    one = (C.c_int * 1)(0)
    r = R.erode(1).struct()
    dst = (C.c_void_p * 1)(16)
    assert lib().hvq_rank_pictures(None, 1, one, one, None, C.byref(r), 1, None, C.cast(dst, C.c_void_p), None) == HVQ_E_ARG
    assert lib().hvq_rank_force_general(None, 1) == HVQ_E_ARG
    assert lib().hvq_rank_check(None) == HVQ_E_ARG
    for name, p in PLANES.items():
        assert lib().hvq_rank_check(C.byref(R.Rank(p, R.IDENTITY_PLANE).struct())) == 0, name
        assert lib().hvq_rank_check(C.byref(R.Rank(R.IDENTITY_PLANE, p).struct())) == 0, name
    for entry in cases.table64():
        assert lib().hvq_rank_check(C.byref(entry.struct())) == 0, entry
    for label, s in _spoiled():
        assert lib().hvq_rank_check(C.byref(s)) == HVQ_E_ARG, label
        s.luma, s.chroma = s.chroma, s.luma
        assert lib().hvq_rank_check(C.byref(s)) == HVQ_E_ARG, label + " (luma)"


# ------------------------------------------------------------------------------------------------- the runtime on the CPU fake device
DRIVER_RANKS = {                                                            # the first is well formed with both radii below 15 (the driver's malformed ones derive from it)
    "erode1": R.erode(1), "identity": R.identity(), "dilate3x1": R.dilate((3, 1)), "range2": R.gradient(2), "median3": R.median(3), "median5": R.median(5),
    "erode15": R.erode(15), "dilate15x0": R.dilate((15, 0)), "erode0x15": R.erode((0, 15)), "range7x3": R.gradient((7, 3)), "dilate2": R.dilate(2),
    "erode5x6": R.erode((5, 6)), "range0": R.gradient(0), "max0": R.dilate(0), "median1": R.Rank(R.PlaneRank(R.MEDIAN), R.PlaneRank(R.MEDIAN)),
    "median5_luma": R.luma_only(R.median(5)), "mixed": R.Rank(R.median(3).luma, R.gradient((4, 9)).luma), "chroma_only": R.Rank(R.IDENTITY_PLANE, R.dilate((9, 4)).luma),
    "erode6_420": R.chroma_for(R.erode(6), 2, 2), "range15": R.gradient(15),
}


def _ranks_txt():
    return "".join(f"{name} {r.luma.op} {r.luma.rx} {r.luma.ry} {r.luma.pad} {r.chroma.op} {r.chroma.rx} {r.chroma.ry} {r.chroma.pad}\n" for name, r in DRIVER_RANKS.items())


@pytest.fixture(scope="module")
def drivers():
    return {kind: fd.build_driver(kind, "rank", "fake_rank_driver", CXX_SOURCES, __file__) for kind in fd.BUILDS}


_want = {}


def _source(source, form, k, geom):
    """the picture the driver worked on, as the driver's line describes it"""
    n = cases.nbytes(geom)
    if form == "pic":
        return fd.oracle_pictures(source)[k].reshape(-1)
    if form == "inv":
        return 255 - fd.oracle_pictures(source)[k].reshape(-1)
    if form.startswith("ranked:"):
        return _expected(source, "pic", k, geom, form.split(":", 1)[1])[1]
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


def _expected(source, form, k, geom, rname):
    key = (source, form, k, geom, rname)
    if key not in _want:
        got = R.of_picture(_source(source, form, k, geom), geom, DRIVER_RANKS[rname])
        _want[key] = (zlib.crc32(got.tobytes()), got)
    return _want[key]


def _run(exe, scenario, schedule, tmp_path):
    _, lines = fd.run_checked(exe, scenario, schedule, tmp_path, inputs={"ranks.txt": _ranks_txt()})
    P, Rc, S = {}, {}, {}
    for line in lines:
        f = line.split()
        if f[0] == "P":
            label, source, form, k, geom, rname = f[1], f[2], f[3], int(f[4]), tuple(int(v) for v in f[5:9]), f[9]
            assert int(f[11]) == 1, f"{label}: the bytes around the output of {source} {k} were written"
            want = _expected(source, form, k, geom, rname)[0]
            assert int(f[10]) == want, f"{label}: picture {k} of {source} ({form}) {geom} through {rname}: crc {int(f[10]):08x}, want {want:08x}"
            P.setdefault(label, []).append((source, form, k, geom, rname))
        elif f[0] == "R":
            Rc[f[1]] = int(f[2])
        elif f[0] == "S":
            S[f[1]] = (int(f[2]), int(f[3]))
    return P, Rc, S


def _check_goldens(P, Rc, S):
    nr = len(DRIVER_RANKS)
    assert len(P["goldens/all"]) == 6 * nr and {rn for *_r, rn in P["goldens/all"]} == set(DRIVER_RANKS)
    assert {g[2:] for _s, _f, _k, g, _n in P["goldens/all"]} == {(2, 2), (2, 1), (1, 1)}
    assert any(g[0] > 128 and g[1] > 32 for _s, _f, _k, g, _n in P["goldens/all"]), "tile seams inside a plane"
    assert P["goldens/one"] == [P["goldens/all"][1]]
    assert Rc == {"goldens/n0": 0}


def _check_memory(P, Rc, S):
    nr = len(DRIVER_RANKS)
    assert P["memory"] == P["memory/nullstream"] and len(P["memory"]) == 2 * fd.n_pics("yuv422_64x48") + 7 * (2 * nr + 1)
    forms = [f for _s, f, *_r in P["memory"]]
    assert forms.count("inv") == fd.n_pics("yuv422_64x48") and forms.count("check") == 7 * nr and forms.count("flat") == 7
    geoms = {g for _s, f, _k, g, _n in P["memory"] if f == "check"}
    assert {(8, 8, 2, 2), (8, 8, 2, 1), (8, 8, 1, 1), (72, 24, 2, 2), (136, 40, 2, 2)} <= geoms, "planes narrower than the halo and than the window"


def _check_many(P, Rc, S):
    assert len(P["many"]) == 300 and P["many"] == P["many/again"]
    assert len({s for s, *_r in P["many"]}) == 8 and len({g for _s, _f, _k, g, _n in P["many"]}) >= 4 and len({n for *_r, n in P["many"]}) >= 8


def _check_body(P, Rc, S):
    assert P["body/chosen"] == P["body/general"] == P["body/chosen_again"] and len(P["body/general"]) == 4 * len(DRIVER_RANKS)
    assert Rc == {"body/force": 0, "body/unforce": 1}
    assert sum(1 for r in DRIVER_RANKS.values() if R.copies(r.luma) or R.copies(r.chroma)) >= 5


def _check_reuse(P, Rc, S):
    from hvqm4_amd._lib import HVQ_E_STATE
    n, ne = fd.n_pics("gop64x48_15"), fd.n_pics("yuv444_64x48")
    g = _clip_geometry("gop64x48_15")
    names = list(DRIVER_RANKS)
    assert P["reuse"] == [("gop64x48_15", "pic", k, g, names[1]) for k in range(n)]
    assert Rc["reuse/evicted"] == HVQ_E_STATE, "the flushes did not hand the slots of the first pass on: the scenario tests nothing"
    assert P["reuse/chain"] == [("gop64x48_15", "ranked:" + names[1], k, g, names[2]) for k in range(n)]
    assert P["reuse/late"] == P["reuse"]
    assert [(s, k) for s, _f, k, *_r in P["reuse/destroy"]] == [("yuv444_64x48", k) for k in range(ne)]


def _check_refused(P, Rc, S):
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_STATE
    arg = ["null_context", "bad_stream", "bad_ordinal", "misaligned_src", "src_with_ordinal", "src_with_bad_stream", "minus_one_without_src", "null_dst",
           "misaligned_dst", "too_many", "null_ranks", "nranks_0", "nranks_65", "which_high", "which_negative", "force_null", "check_null"]
    spoiled = ["op_4", "op_negative", "radius_16", "radius_negative", "median_rx_ry", "median_radius_3", "pad"]
    want = {k: HVQ_E_ARG for k in arg + spoiled + ["check_" + s for s in spoiled]}
    want.update({"evicted": HVQ_E_STATE, "queued": HVQ_E_STATE, "n0": 0, "check_good": 0})
    assert Rc == {"refused/" + k: v for k, v in want.items()}
    same, total = S["refused"]
    assert same == total == 2 * 4608 + 16, "a refused call wrote its output"
    g = _clip_geometry("gop64x48_15")
    names = list(DRIVER_RANKS)
    assert P["refused/then_ok"] == [("gop64x48_15", "pic", 1, g, names[63 % len(names)]), ("gop64x48_15", "pic", fd.n_pics("gop64x48_15") - 1, g, names[0])]


CHECKS = {"goldens": _check_goldens, "memory": _check_memory, "many": _check_many, "body": _check_body, "reuse": _check_reuse, "refused": _check_refused}


@pytest.mark.parametrize("schedule", ["eager", "late"])
@pytest.mark.parametrize("build", list(fd.BUILDS))
@pytest.mark.parametrize("scenario", list(CHECKS))
def test_fake_device_scenario(drivers, scenario, build, schedule, tmp_path):
    P, Rc, S = _run(drivers[build], scenario, schedule, tmp_path)
    CHECKS[scenario](P, Rc, S)


def test_the_reuse_chain_is_an_opening_in_two_calls():
    """what `reuse/chain` computes is a chain through src=: the expected bytes of the second call are of_steps of the two entries"""
    names = list(DRIVER_RANKS)
    pic = fd.oracle_pictures("gop64x48_15")[0].reshape(-1)
    g = _clip_geometry("gop64x48_15")
    assert np.array_equal(_expected("gop64x48_15", "ranked:" + names[1], 0, g, names[2])[1], R.of_steps(pic, g, [DRIVER_RANKS[names[1]], DRIVER_RANKS[names[2]]]))


def test_the_existing_fake_builds_link_without_the_rank_body():
    """the source lists of the other drivers have no hvq_launch_rank: the runtime's reference is weak"""
    assert not any("fake_rank" in s for s in fd.CXX_SOURCES)
    text = open(os.path.join(fd.CSRC, "hvq_runtime.cpp")).read()
    decl = [l for l in text.splitlines() if "hvq_launch_rank(" in l and l.startswith("extern")]
    assert len(decl) == 1 and "weak" in decl[0]
    exe = fd.build_driver("plain", "fake", "fake_driver", fd.CXX_SOURCES, fd.__file__)
    assert os.access(exe, os.X_OK)


# ------------------------------------------------------------------------------------------------- tools/bench_rank.py
def _bench_rank():
    sys.path.insert(0, os.path.join(fd.ROOT, "tools"))
    try:
        import bench_rank
    finally:
        sys.path.remove(os.path.join(fd.ROOT, "tools"))
    return bench_rank


def _bench_trace(tmp_path, drop=0):
    sys.path.insert(0, fd.GOLDEN)
    try:
        import make_bench_tools as mk
    finally:
        sys.path.remove(fd.GOLDEN)
    tool = _bench_rank()
    blocks = [mk.block(kernel) for _label, kernel in tool.trace_plan()]
    if drop:
        blocks[-1] = blocks[-1][:-drop]
    d = str(tmp_path / "trace")
    mk.write_trace(d, blocks)
    per = 1 + mk.REPS
    return tool, mk, d, {"launches": per, "pictures": 1024, "content": "natural"}


def test_bench_rank_imports_without_a_gpu_and_reads_a_synthetic_trace(tmp_path):
    tool, mk, d, printed = _bench_trace(tmp_path)
    assert "torch" not in tool.__dict__ and callable(tool.main)
    labels = [label for label, _k in tool.trace_plan()]
    assert labels[:8] == ["erode1", "erode7", "erode15", "range2", "median3", "median5", "identity", "identity_general"]
    assert labels[8:] == ["scale_identity", "binomial3", "gauss5_r15"]
    res = tool.trace_summary(d, printed)
    assert "error" not in res, res
    # block b of the helper: a warm-up launch and three of base, base + 1234, base + 4321 ns, base = 100000 + 7919 b
    for b, label in enumerate(labels):
        base = 100_000 + 7_919 * b
        assert res[label]["launches"] == mk.REPS and res[label]["median_us"] == round((base + 1_234) / 1e3, 1), label
        assert res[label]["min_us"] == round(base / 1e3, 1) and res[label]["max_us"] == round((base + 4_321) / 1e3, 1), label
    med = lambda label: res[label]["median_us"]
    assert res["erode15"]["over_scale_identity_kernel"] == round(med("erode15") / med("scale_identity"), 2)
    assert res["ratios"]["erode15_over_erode1"] == round(med("erode15") / med("erode1"), 2)
    assert res["ratios"]["erode1_over_binomial3"] == round(med("erode1") / med("binomial3"), 2)
    assert res["ratios"]["median5_over_median3"] == round(med("median5") / med("median3"), 2)
    assert res["condition"]["erode15_us"] == med("erode15") and res["condition"]["gauss5_r15_us"] == med("gauss5_r15")
    assert res["condition"]["holds"] is (med("erode15") <= med("gauss5_r15"))
    assert (res["vgprs"], res["lds"], res["scratch"]) == ("8", "0", "0")


def test_bench_rank_refuses_a_trace_with_one_launch_too_few(tmp_path):
    tool, _mk, d, printed = _bench_trace(tmp_path, drop=1)
    res = tool.trace_summary(d, printed)
    assert "error" in res and "planned" in res["error"]


# ------------------------------------------------------------------------------------------------- the 5 x 5 median's network
def test_the_median_network_of_the_header_selects_the_median_of_sorted_columns():
    """the X / LO / HI lines of hvq_rk_med_select5, checked on all 6^5 0 / 1 patterns of sorted columns, are the ones
    tools/median_network.py derives; the column sort it assumes is the one hvq_rk_med_sort5 spells"""
    sys.path.insert(0, os.path.join(fd.ROOT, "tools"))
    try:
        import median_network as mn
    finally:
        sys.path.remove(os.path.join(fd.ROOT, "tools"))
    text = open(os.path.join(fd.CSRC, "hvq_rank.h")).read()
    body = text[text.index("#define X HVQ_RK_X"):text.index("#undef X")]
    ops = mn.parse(body)
    assert len(ops) == 79 and sum(2 if k == "X" else 1 for k, _a, _b in ops) == 134
    mn.check(ops, 12)
    assert "return hvq_rk_pack(v[12]);" in text
    cost, _name, derived, outw = mn.derive()
    assert (cost, outw, derived) == (134, 12, ops)
    sort5 = text[text.index("HvqRkPair v[5];"):text.index("S[HVQ_RK_SORTED * i + idx] = hvq_rk_pack(v[i]);\n    }\n}\n/* 3 x 3")]
    assert [(int(a), int(b)) for a, b in __import__("re").findall(r"HVQ_RK_X\((\d), (\d)\)", sort5)] == mn.SORT5
    for bits in __import__("itertools").product((0, 1), repeat=5):
        v = list(bits)
        for a, b in mn.SORT5:
            v[a], v[b] = min(v[a], v[b]), max(v[a], v[b])
        assert v == sorted(bits)
