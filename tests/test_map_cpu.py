"""CPU: the values of hvq_map_pictures and hvq_histogram_tables.  tests/map_ref.py restates include/hvqm4_amd.h in plain Python;
hvqm4_amd.maps (numpy, built on hvqm4_amd.histograms), the fixture tests/golden/map.json and the runtime on the CPU fake device
(tests/native/fake_map.cpp, which walks the kernels' grids with the functions of hvq_map.h) are compared with it by ==.  The fake-device
driver is a stand-alone program, built and run plain and with ASan + UBSan as tests/test_rank_cpu.py builds its own; nothing is preloaded
and no Python is involved in the sanitised run."""
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import pytest

import tests.test_fake_device as fd
from hvqm4_amd import histograms as H
from hvqm4_amd import maps as M
from tests import map_cases as cases
from tests import map_ref as ref

NATIVE = fd.NATIVE
CXX_SOURCES = [s for s in fd.CXX_SOURCES if os.path.basename(s) != "fake_driver.cpp"] + \
              [os.path.join(NATIVE, "fake_map.cpp"), os.path.join(NATIVE, "fake_histograms.cpp"), os.path.join(NATIVE, "fake_map_driver.cpp")]
FIXTURE = json.load(open(os.path.join(fd.GOLDEN, "map.json")))


def _lists(t: M.Table):
    return [list(t.y), list(t.u), list(t.v)]


def _as_ref(p: M.PlaneRule):
    return (p.kind, p.a, p.b)


def _ref_tables(rec, rule: M.Rule) -> np.ndarray:
    return np.array(ref.record_tables([[int(x) for x in rec[p]] for p in range(3)], _as_ref(rule.luma), _as_ref(rule.chroma)), dtype=np.uint8)


def _clip_geometry(name):
    from hvqm4_amd.container import parse_header
    hdr = parse_header(open(os.path.join(fd.GOLDEN, fd.CLIPS[name]["file"]), "rb").read())
    return (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)


# ------------------------------------------------------------------------------------------------- module and known answers
@pytest.mark.parametrize("geom", [(16, 8, 2, 2), (16, 8, 2, 1), (8, 16, 1, 1)])
def test_module_equals_reference_on_pictures_of_the_three_samplings(geom):
    pic = cases.made(geom, 5)
    for t in cases.tables(6):
        for planes in range(1, 8):
            assert M.of_picture(pic, geom, t, planes).tobytes() == ref.map_picture(pic.tobytes(), geom, _lists(t), planes), (geom, planes)


def test_known_answers():
    geom = (24, 16, 2, 2)
    pic = cases.made(geom, 3)
    assert M.of_picture(pic, geom, M.identity()).tobytes() == pic.tobytes() == ref.map_picture(pic.tobytes(), geom, _lists(M.identity()))
    assert np.array_equal(M.of_picture(pic, geom, M.invert()), 255 - pic)
    assert ref.map_picture(pic.tobytes(), geom, _lists(M.invert())) == (255 - pic).tobytes()
    t = cases.perm_table(9)
    assert len({t.y, t.u, t.v}) == 3, "distinct per plane"
    there = M.of_picture(pic, geom, t)
    assert not np.array_equal(there, pic) and np.array_equal(M.of_picture(there, geom, M.inverse(t)), pic)
    assert M.compose(t, M.inverse(t)) == M.identity() == M.compose(M.inverse(t), t)
    assert np.array_equal(M.of_picture(pic, geom, M.compose(t, M.invert())), 255 - there)
    flat = M.of_picture(pic, geom, M.flat_table(77))
    assert flat.tolist() == [77] * cases.nbytes(geom)
    only_y = M.of_picture(pic, geom, M.invert(), planes=1)
    assert np.array_equal(only_y[:24 * 16], 255 - pic[:24 * 16]) and np.array_equal(only_y[24 * 16:], pic[24 * 16:])
    assert np.array_equal(M.of_picture(pic, geom, M.invert().luma_only()), only_y)


def test_struct_layout():
    import ctypes as C
    from hvqm4_amd._lib import HvqTablePlane, HvqTableRule
    assert (C.sizeof(HvqTablePlane), C.sizeof(HvqTableRule)) == (16, 32)
    assert [(n, getattr(HvqTablePlane, n).offset) for n, _t in HvqTablePlane._fields_] == [("kind", 0), ("a", 4), ("b", 8), ("pad", 12)]
    assert HvqTableRule.luma.offset == 0 and HvqTableRule.chroma.offset == 16
    s = M.Rule(M.PlaneRule(M.STRETCH, 7, 3), M.PlaneRule(M.FLAT, 200)).struct()
    assert (s.luma.kind, s.luma.a, s.luma.b, s.luma.pad, s.chroma.kind, s.chroma.a, s.chroma.b, s.chroma.pad) == (3, 7, 3, 0, 1, 200, 0, 0)
    assert (M.IDENTITY, M.FLAT, M.EQUALIZE, M.STRETCH, M.OTSU, M.MAX_RULES, M.TABLE_BYTES) == (0, 1, 2, 3, 4, 64, 768)
    assert (ref.IDENTITY, ref.FLAT, ref.EQUALIZE, ref.STRETCH, ref.OTSU) == (0, 1, 2, 3, 4)
    header = open(os.path.join(fd.ROOT, "include", "hvqm4_amd.h")).read()
    for line in ("#define HVQ_MAP_TABLE_BYTES 768", "#define HVQ_TBL_IDENTITY 0", "#define HVQ_TBL_FLAT     1", "#define HVQ_TBL_EQUALIZE 2", "#define HVQ_TBL_STRETCH  3",
                 "#define HVQ_TBL_OTSU     4", "#define HVQ_TBL_MAX_RULES 64", "typedef struct HvqTablePlane { int32_t kind, a, b, pad; } HvqTablePlane;"):
        assert line in header, line
    assert M.pack(cases.tables(5)).shape == (5, 3, 256) and M.pack(cases.tables(5)).dtype == np.uint8 and M.pack([]).shape == (0, 3, 256)
    assert M.pack([cases.perm_table(2)]).tobytes() == cases.perm_table(2).y + cases.perm_table(2).u + cases.perm_table(2).v


def test_builders():
    v = np.arange(256)
    assert M.identity().array().tolist() == [list(range(256))] * 3 and M.invert().y == bytes(255 - i for i in range(256))
    assert M.threshold(100).array()[1].tolist() == np.where(v > 100, 255, 0).tolist() and set(M.threshold(255).y) == {0}
    assert M.window(10, 20).array()[2].tolist() == np.where((v >= 10) & (v <= 20), 255, 0).tolist()
    assert M.brightness_contrast() == M.identity() and M.brightness_contrast(10).y == bytes(min(255, i + 10) for i in range(256))
    assert M.brightness_contrast(0, 2).y == bytes(min(255, max(0, 2 * i - 128)) for i in range(256))
    assert M.brightness_contrast(0, 0.5).y[129] == 129 and M.brightness_contrast(0, 0.5).y[131] == 130      # 128.5 and 129.5 round half up
    assert M.gamma(1.0) == M.identity() and M.gamma(2.0).y[128] == int(255 * (128 / 255) ** 2 + 0.5) and M.gamma(0.5).y[255] == 255
    assert set(M.posterize(2).y) == {0, 255} and sorted(set(M.posterize(4).y)) == [0, 85, 170, 255] and M.posterize(256) == M.identity()
    assert M.solarize(128).y == bytes(i if i < 128 else 255 - i for i in range(256)) and M.solarize(0) == M.invert() and M.solarize(256) == M.identity()
    lut = (v * 7 % 256).astype(np.uint8)
    assert M.from_lut(lut) == M.Table(lut.tobytes(), lut.tobytes(), lut.tobytes())
    assert M.from_lut(lut, v) == M.Table(lut.tobytes(), bytes(range(256)), bytes(range(256))) and M.from_lut(lut, v, lut).v == lut.tobytes()
    assert M.luma_only(M.invert()) == M.Table(M.invert().y) and M.luma_only(M.otsu()) == M.Rule(M.PlaneRule(M.OTSU), M.PlaneRule())
    t1, t2 = cases.perm_table(3), cases.perm_table(4)
    assert M.compose(t1, t2).u == bytes(t2.u[t1.u[i]] for i in range(256))
    assert len({M.invert(), M.invert(), M.identity()}) == 2 and hash(cases.perm_table(1)) == hash(cases.perm_table(1))
    assert M.equalize() == M.Rule(M.PlaneRule(M.EQUALIZE), M.PlaneRule(M.EQUALIZE)) and M.stretch(5, 7).chroma == M.PlaneRule(M.STRETCH, 5, 7)
    assert M.stretch(lo=3).luma == M.PlaneRule(M.STRETCH, 3, 0) and M.flat(9).luma == M.PlaneRule(M.FLAT, 9) and M.equalize().luma_only().chroma == M.PlaneRule()
    assert len({M.otsu(), M.otsu(), M.equalize()}) == 2
    for r in cases.RULES.values():
        M.check(r)
    for bad in (lambda: M.threshold(256), lambda: M.threshold(-1), lambda: M.window(5, 4), lambda: M.gamma(0), lambda: M.posterize(1), lambda: M.posterize(257),
                lambda: M.solarize(257), lambda: M.flat_table(256), lambda: M.from_lut(np.arange(255)), lambda: M.from_lut(np.arange(256) * 2), lambda: M.from_lut(np.zeros(256)),
                lambda: M.Table(b"x"), lambda: M.inverse(M.flat_table(3)), lambda: M.pack([None]), lambda: M.stretch(500), lambda: M.stretch(0, -1), lambda: M.flat(256),
                lambda: M.flat(-1), lambda: M.check(M.Rule(M.PlaneRule(5), M.PlaneRule())), lambda: M.check(M.Rule(M.PlaneRule(), M.PlaneRule(M.OTSU, 1))),
                lambda: M.check(M.Rule(M.PlaneRule(M.EQUALIZE, 0, 1), M.PlaneRule())), lambda: M.check(M.Rule(M.PlaneRule(M.FLAT, 1, 1), M.PlaneRule())),
                lambda: M.check(M.Rule(M.PlaneRule(M.IDENTITY, 0, 0, 1), M.PlaneRule())), lambda: M.check(M.PlaneRule()), lambda: M.of_picture(np.zeros(96, np.uint8), (8, 8, 2, 2), M.identity(), 0),
                lambda: M.of_picture(np.zeros(96, np.uint8), (8, 8, 2, 2), M.identity(), 8), lambda: M.of_picture(np.zeros(95, np.uint8), (8, 8, 2, 2), M.identity()),
                lambda: M.tables_of_records(np.zeros((2, 3, 256), np.int64), [M.otsu()]), lambda: M.tables_of_records(np.zeros((3, 255), np.int64), M.otsu())):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------- tables of records
def _check_records(recs, label):
    """tables_of_records == the reference, rule by rule, and == the histogram module's own functions"""
    recs = np.asarray(recs)
    for name, rule in cases.RULES.items():
        got = M.tables_of_records(recs, rule)
        for i, rec in enumerate(recs):
            assert np.array_equal(got[i], _ref_tables(rec, rule)), (label, name, i)
    v = np.arange(256)
    eq, ot, st = M.tables_of_records(recs, M.equalize()), M.tables_of_records(recs, M.otsu()), M.tables_of_records(recs, M.stretch(10, 20))
    for i, rec in enumerate(recs):
        for p in range(3):
            if rec[p].sum() == 0:
                assert eq[i, p].tolist() == ot[i, p].tolist() == st[i, p].tolist() == list(range(256)), (label, i, p)
                continue
            assert np.array_equal(eq[i, p], H.equalize_lut(rec[p])), (label, i, p)
            assert np.array_equal(ot[i, p], np.where(v > int(H.otsu(rec[p])), 255, 0)), (label, i, p)
            lo, hi = int(H.percentile(rec[p], 1)), int(H.percentile(rec[p], 98))
            if hi > lo:
                assert st[i, p][lo] == 0 and st[i, p][hi] == 255 and (np.diff(st[i, p].astype(int)) >= 0).all(), (label, i, p)
            else:
                assert st[i, p].tolist() == list(range(256)), (label, i, p)


def test_tables_of_the_special_records():
    recs = dict(cases.special_records())
    _check_records(np.stack(list(recs.values())), "special")
    t = lambda label, rule: M.tables_of_records(recs[label], rule)
    assert t("single value", M.otsu())[0].tolist() == [0] + [255] * 255, "a single value: t = 0"
    assert t("single value", M.equalize())[0].tolist() == list(range(256)) and t("single value", M.stretch(0, 0))[0].tolist() == list(range(256))
    assert t("two values", M.equalize())[0][3] == 0 and t("two values", M.equalize())[0][200] == 255 and t("two values", M.otsu())[0][3:5].tolist() == [0, 255]
    assert t("two values", M.stretch(0, 0))[0][[3, 4, 199, 200]].tolist() == [0, 1, 254, 255]
    assert t("otsu tie", M.otsu())[0][10:12].tolist() == [0, 255], "every t in 10 .. 19 ties: the smallest wins"
    assert t("otsu tie", M.otsu())[1][0:2].tolist() == [0, 255] and t("otsu tie", M.otsu())[2][100:102].tolist() == [0, 255]
    assert t("empty", M.otsu()).tolist() == [list(range(256))] * 3 and t("empty", M.flat(9))[1].tolist() == [9] * 256
    assert t("2^26 between 0 and 255", M.otsu())[0][[0, 1, 254, 255]].tolist() == [0, 255, 255, 255]
    assert t("2^26 between 0 and 1", M.otsu())[0][[0, 1]].tolist() == [0, 255] and t("2^26 between 0 and 1", M.equalize())[0][[0, 1, 2]].tolist() == [0, 255, 255]
    assert t("hi <= lo", M.stretch(10, 10))[0].tolist() == list(range(256)) and t("hi <= lo", M.stretch(0, 0))[0][[50, 55, 60]].tolist() == [0, 128, 255]
    assert t("uniform", M.stretch(0, 0))[0].tolist() == list(range(256)) and t("uniform", M.stretch(499, 499))[0][[127, 128]].tolist() == [0, 255]


def test_tables_of_the_records_of_every_golden_picture():
    recs = []
    for name in sorted(fd.CLIPS):
        g = _clip_geometry(name)
        recs += [H.of_picture(p.reshape(-1), *g) for p in fd.oracle_pictures(name)[:2]]
    _check_records(np.stack(recs), "golden")


def test_tables_of_300_random_records():
    recs = cases.random_records()
    assert len(recs) == 300 and recs.sum(-1).max() == cases.MAX_N and (recs.sum(-1) == cases.MAX_N).sum() >= 300
    _check_records(recs, "random")


# ------------------------------------------------------------------------------------------------- the fixture
def test_fixture_covers_every_golden_clip_and_the_generator_names_the_shared_tables():
    assert set(FIXTURE["clips"]) == set(fd.CLIPS)
    sys.path.insert(0, fd.GOLDEN)
    try:
        import make_map
    finally:
        sys.path.remove(fd.GOLDEN)
    assert make_map.SETS == [(label, _lists(t)) for label, t in cases.FIVE]
    assert make_map.RULES == [(n, _as_ref(cases.RULES[n].luma)) for n in ("equalize", "stretch10_20", "otsu")] and all(cases.RULES[n].luma == cases.RULES[n].chroma for n, _r in make_map.RULES)
    for name, entry in FIXTURE["clips"].items():
        assert tuple(entry["geometry"]) == _clip_geometry(name)
        assert [l for l, _c in entry["sets"]] == [l for l, _t in cases.FIVE] and [l for l, _a, _b in entry["rules"]] == [l for l, _r in make_map.RULES]
    assert {tuple(e["geometry"])[2:] for e in FIXTURE["clips"].values()} == {(2, 2), (2, 1), (1, 1)}


@pytest.mark.parametrize("name", sorted(FIXTURE["clips"]))
def test_fixture_equals_module(name):
    entry = FIXTURE["clips"][name]
    g = tuple(entry["geometry"])
    pic = fd.oracle_pictures(name)[0].reshape(-1)
    assert hashlib.sha256(pic.tobytes()).hexdigest() == fd.CLIPS[name]["picture_sha256"][0], "the fixture describes the manifest's picture"
    for (label, crc), (_l, t) in zip(entry["sets"], cases.FIVE):
        assert zlib.crc32(M.of_picture(pic, g, t).tobytes()) == crc, (name, label)
    rec = H.of_picture(pic, *g)
    for label, tcrc, pcrc in entry["rules"]:
        t = M.tables_of_records(rec, cases.RULES[label])
        assert zlib.crc32(t.tobytes()) == tcrc, (name, label)
        assert zlib.crc32(M.of_picture(pic, g, M.from_lut(*t)).tobytes()) == pcrc, (name, label)


# ------------------------------------------------------------------------------------------------- argument checks without a device
class _NoDevice:
    """what Context.map_pictures looks at before it reaches the library"""
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
    call = lambda *a, **k: Context.map_pictures(_NoDevice(), *a, **k)
    t = M.invert()
    nb = 64 * 48 * 3 // 2
    with pytest.raises(ValueError, match="ordinals"):
        call([0, 0], [0], t)
    with pytest.raises(HvqError) as e:
        call([0, 7], [0, 0], t)
    assert e.value.code == HVQ_E_ARG
    for tables in (None, "invert", [t], [t, None], t.y, np.zeros((1, 3, 256), np.uint8)):
        with pytest.raises(ValueError, match="tables"):
            call([0, 0], [0, 1], tables)
    for planes in (0, 8, -1, True, 1.0, None):
        with pytest.raises(ValueError, match="planes"):
            call([0], [0], t, planes=planes)
    for bad in (torch.zeros((1, 3, 256), dtype=torch.int32), torch.zeros((1, 3, 255), dtype=torch.uint8), torch.zeros((3, 256), dtype=torch.uint8),
                torch.zeros((1, 3, 512), dtype=torch.uint8)[:, :, ::2], torch.zeros((3, 3, 256), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="tables"):
            call([0, 0], [0, 1], bad)
    room = torch.zeros(2 * 768 + 64, dtype=torch.uint8)
    off = (-room.data_ptr()) % 16
    with pytest.raises(ValueError, match="multiple of 16"):
        call([0, 0], [0, 1], room[off + 8:off + 8 + 1536].view(2, 3, 256))
    with pytest.raises(ValueError, match="tables is on cpu"):
        call([0, 0], [0, 1], room[off:off + 1536].view(2, 3, 256))
    with pytest.raises(ValueError, match="1 sources for 2 pictures"):
        call([0, 0], [0, 1], t, src=[None])
    good = torch.zeros(nb, dtype=torch.uint8)
    with pytest.raises(ValueError, match="elements"):
        call([1], [-1], t, src=[good])
    with pytest.raises(ValueError, match="ordinal -1"):
        call([0], [0], t, src=[good])
    with pytest.raises(ValueError, match="out must be"):
        call([0, 0], [0, 1], t, out=torch.zeros((2, nb), dtype=torch.int32))
    with pytest.raises(ValueError, match="out must be a list"):
        call([0, 1], [0, 1], t, out=torch.zeros((2, nb), dtype=torch.uint8))
    with pytest.raises(ValueError, match="not a GPU"):
        call([0, 0], [0, 1], [t, cases.perm_table(0)], out=torch.zeros((2, nb), dtype=torch.uint8))
    with pytest.raises(ValueError, match="65535"):
        call([0] * 65536, [0] * 65536, t)
    # histogram_tables
    tab = lambda *a, **k: Context.histogram_tables(_NoDevice(), *a, **k)
    hist = torch.zeros((2, 3, 256), dtype=torch.int32)
    for bad in (None, hist.long(), hist[:, :, :255], hist[0], torch.zeros((2, 3, 512), dtype=torch.int32)[:, :, ::2]):
        with pytest.raises(ValueError, match="hist"):
            tab(bad, M.otsu())
    for rules in (None, "otsu", [M.otsu()], [M.otsu(), None], M.otsu().luma):
        with pytest.raises(ValueError, match="rules"):
            tab(hist, rules)
    with pytest.raises(ValueError, match="kind"):
        tab(hist, M.Rule(M.PlaneRule(5), M.PlaneRule()))
    with pytest.raises(ValueError, match="STRETCH"):
        tab(hist, [M.otsu(), M.Rule(M.PlaneRule(M.STRETCH, 500), M.PlaneRule())])
    with pytest.raises(ValueError, match="FLAT"):
        tab(hist, M.Rule(M.PlaneRule(), M.PlaneRule(M.FLAT, 256)))
    with pytest.raises(ValueError, match="pad"):
        tab(hist, M.Rule(M.PlaneRule(M.OTSU, 0, 0, 1), M.PlaneRule()))
    with pytest.raises(ValueError, match="no a, b"):
        tab(hist, M.Rule(M.PlaneRule(M.OTSU, 0, 1), M.PlaneRule()))
    many = [M.Rule(M.PlaneRule(M.STRETCH, i, 1), M.PlaneRule()) for i in range(65)]
    with pytest.raises(ValueError, match="65 distinct"):
        tab(torch.zeros((65, 3, 256), dtype=torch.int32), many)
    with pytest.raises(ValueError, match="not a GPU"):
        tab(torch.zeros((128, 3, 256), dtype=torch.int32), many[:64] * 2)
    with pytest.raises(ValueError, match="65535"):
        tab(torch.zeros((65536, 3, 256), dtype=torch.int32), M.otsu())


def _spoiled():
    """(label, HvqTableRule struct) for every refusal of hvq_table_check, in the chroma plane of an otherwise good entry"""
    from hvqm4_amd._lib import HvqTablePlane
    out = []

    def bad(label, **members):
        s = M.equalize().struct()
        s.chroma = HvqTablePlane(0, 0, 0, 0)
        for k, v in members.items():
            setattr(s.chroma, k, v)
        out.append((label, s))
    bad("kind 5", kind=5)
    bad("kind -1", kind=-1)
    bad("flat 256", kind=M.FLAT, a=256)
    bad("flat -1", kind=M.FLAT, a=-1)
    bad("flat with b", kind=M.FLAT, a=1, b=1)
    bad("stretch a 500", kind=M.STRETCH, a=500)
    bad("stretch b 500", kind=M.STRETCH, b=500)
    bad("stretch a -1", kind=M.STRETCH, a=-1)
    bad("equalize with a", kind=M.EQUALIZE, a=1)
    bad("otsu with b", kind=M.OTSU, b=1)
    bad("identity with a", kind=M.IDENTITY, a=1)
    bad("pad", pad=1)
    bad("a negative pad", kind=M.OTSU, pad=-1)
    return out


def test_the_library_without_a_device_still_checks_its_arguments():
    """no context can exist here, and the calls say so before they look at anything else (HVQ_E_ARG, not HVQ_E_NOGPU); the host-only
    check works"""
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, lib
    one = (C.c_int * 1)(0)
    dst = (C.c_void_p * 1)(16)
    r = M.otsu().struct()
    assert lib().hvq_map_pictures(None, 1, one, one, None, C.c_void_p(16), 1, None, 7, C.cast(dst, C.c_void_p), None) == HVQ_E_ARG
    assert lib().hvq_histogram_tables(None, 1, C.c_void_p(16), C.byref(r), 1, None, C.c_void_p(16), None) == HVQ_E_ARG
    assert lib().hvq_table_check(None) == HVQ_E_ARG
    for name, rule in cases.RULES.items():
        assert lib().hvq_table_check(C.byref(rule.struct())) == 0, name
    for a in (0, 499):
        assert lib().hvq_table_check(C.byref(M.stretch(a, 499 - a).struct())) == 0
    for label, s in _spoiled():
        assert lib().hvq_table_check(C.byref(s)) == HVQ_E_ARG, label
        s.luma, s.chroma = s.chroma, s.luma
        assert lib().hvq_table_check(C.byref(s)) == HVQ_E_ARG, label + " (luma)"


# ------------------------------------------------------------------------------------------------- the runtime on the CPU fake device
NTABLES = 12
_TABLES = cases.tables(NTABLES)


@pytest.fixture(scope="module")
def drivers():
    return {kind: fd.build_driver(kind, "map", "fake_map_driver", CXX_SOURCES, __file__) for kind in fd.BUILDS}


@pytest.fixture(scope="module")
def records():
    """the records of the scenario `tables` and the tables to expect of them, rule by rule: [record][rule] uint8 [3, 256]"""
    recs = cases.all_records()
    per_rule = [M.tables_of_records(recs, rule) for rule in cases.RULES.values()]
    return recs, np.stack(per_rule, axis=1)


_want = {}


def _source(source, form, k, geom):
    if form == "pic":
        return fd.oracle_pictures(source)[k].reshape(-1)
    if form == "inv":
        return 255 - fd.oracle_pictures(source)[k].reshape(-1)
    if form in ("synth", "inplace"):
        return cases.synth(geom, k)
    raise AssertionError(form)


def _table(pic, geom, table, produced):
    if table.startswith("t"):
        return _TABLES[int(table[1:])]
    if table.startswith("o"):
        return M.from_lut(*produced[int(table[1:])])
    assert table.startswith("r:")
    return M.from_lut(*M.tables_of_records(H.of_picture(pic, *geom), cases.RULES[table[2:]]))


def _expected(source, form, k, geom, table, planes, produced):
    key = (source, form, k, geom, table, planes)
    if key not in _want:
        pic = _source(source, form, k, geom)
        _want[key] = zlib.crc32(M.of_picture(pic, geom, _table(pic, geom, table, produced), planes).tobytes())
    return _want[key]


def _run(exe, scenario, schedule, tmp_path, records):
    rules = "".join(f"{n} {r.luma.kind} {r.luma.a} {r.luma.b} {r.luma.pad} {r.chroma.kind} {r.chroma.a} {r.chroma.b} {r.chroma.pad}\n" for n, r in cases.RULES.items())
    out, lines = fd.run_checked(exe, scenario, schedule, tmp_path,
                                inputs={"rules.txt": rules, "tables.bin": M.pack(_TABLES).tobytes(), "records.bin": records[0].astype("<u4").tobytes()})
    produced = None
    if scenario == "tables":                                                   # == the expected tables first: the pictures then go through them
        produced = np.frombuffer((out / "tables_out.bin").read_bytes(), dtype=np.uint8).reshape(-1, 3, 256)
        want = records[1].reshape(-1, 3, 256)
        assert produced.shape == want.shape
        bad = np.flatnonzero((produced != want).any(axis=(1, 2)))
        assert not bad.size, f"record {bad[0] // len(cases.RULES)} through rule {list(cases.RULES)[bad[0] % len(cases.RULES)]}: {bad.size} tables differ"
    P, Rc, S = {}, {}, {}
    for line in lines:
        f = line.split()
        if f[0] == "P":
            label, source, form, k, geom, table, planes = f[1], f[2], f[3], int(f[4]), tuple(int(v) for v in f[5:9]), f[9], int(f[10])
            assert int(f[12]) == 1, f"{label}: the bytes around the output of {source} {k} were written"
            want = _expected(source, form, k, geom, table, planes, produced)
            assert int(f[11]) == want, f"{label}: picture {k} of {source} ({form}) {geom} through {table}, planes {planes}: crc {int(f[11]):08x}, want {want:08x}"
            P.setdefault(label, []).append((source, form, k, geom, table, planes))
        elif f[0] == "R":
            Rc[f[1]] = int(f[2])
        elif f[0] == "S":
            S[f[1]] = (int(f[2]), int(f[3]))
    return P, Rc, S, out


def _check_goldens(P, Rc, S, out, records):
    assert len(P["goldens/all"]) == 6 * NTABLES and {t for *_r, t, _p in P["goldens/all"]} == {f"t{i}" for i in range(NTABLES)}
    assert {g[2:] for _s, _f, _k, g, _t, _p in P["goldens/all"]} == {(2, 2), (2, 1), (1, 1)}
    assert any(g[0] * g[1] > 8192 for _s, _f, _k, g, _t, _p in P["goldens/all"]), "tile seams inside a plane"
    assert P["goldens/one"] == [P["goldens/all"][1]] and P["goldens/one"][0][4] == "t1"
    assert Rc == {"goldens/n0": 0}


def _check_memory(P, Rc, S, out, records):
    assert P["memory"] == P["memory/nullstream"] and len(P["memory"]) == 2 * fd.n_pics("yuv422_64x48") + 10 * 8
    forms = [f for _s, f, *_r in P["memory"]]
    assert forms.count("inv") == fd.n_pics("yuv422_64x48") and forms.count("synth") == forms.count("inplace") == 40
    geoms = {g for _s, f, _k, g, _t, _p in P["memory"] if f == "inplace"}
    assert {(8, 8, 2, 2), (8, 8, 2, 1), (8, 8, 1, 1), (72, 24, 2, 2), (136, 40, 2, 2), (136, 64, 2, 2), (216, 152, 2, 2), (8192, 8, 2, 2)} <= geoms


def _check_many(P, Rc, S, out, records):
    assert len(P["many"]) == 300 and P["many"] == P["many/again"]
    assert len({s for s, *_r in P["many"]}) == 8 and len({g for _s, _f, _k, g, _t, _p in P["many"]}) >= 4 and len({t for *_r, t, _p in P["many"]}) == NTABLES


def _check_planes(P, Rc, S, out, records):
    assert sorted(P) == [f"planes/{m}" for m in range(1, 8)]
    for m in range(1, 8):
        assert len(P[f"planes/{m}"]) == 8 and {p for *_r, p in P[f"planes/{m}"]} == {m}
        assert [r[:5] for r in P[f"planes/{m}"]] == [r[:5] for r in P["planes/7"]]


def _check_tables(P, Rc, S, out, records):
    n = len(records[0]) * len(cases.RULES)
    assert [(f, k, t) for _s, f, k, _g, t, _p in P["tables/map"]] == [("synth", i, f"o{i}") for i in range(n)]
    assert Rc == {"tables/n0": 0} and S == {"tables/guards": (512, 512)}


def _check_chain(P, Rc, S, out, records):
    from hvqm4_amd._lib import HVQ_E_STATE
    n, ne = fd.n_pics("gop64x48_15"), fd.n_pics("yuv444_64x48")
    g = _clip_geometry("gop64x48_15")
    names = list(cases.RULES)
    assert P["chain"] == [("gop64x48_15", "pic", k, g, "r:" + names[k % len(names)], 7) for k in range(n)]
    assert Rc == {"chain/evicted": HVQ_E_STATE, "chain/queued": HVQ_E_STATE}, "the flushes did not hand the slots of the first pass on: the scenario tests nothing"
    assert P["chain/late"] == P["chain"]
    assert [(s, k) for s, _f, k, *_r in P["chain/destroy"]] == [("yuv444_64x48", k) for k in range(ne)]
    got = np.frombuffer((out / "chain.bin").read_bytes(), dtype=np.uint8).reshape(-1, 3, 256)
    pics = fd.oracle_pictures("gop64x48_15")
    want = np.stack([M.tables_of_records(H.of_picture(pics[k].reshape(-1), *g), cases.RULES[names[k % len(names)]]) for k in range(n)])
    assert np.array_equal(got, want)


def _check_refused(P, Rc, S, out, records):
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_STATE
    arg = ["null_context", "bad_stream", "bad_ordinal", "misaligned_src", "src_with_ordinal", "src_with_bad_stream", "minus_one_without_src", "null_dst",
           "misaligned_dst", "too_many", "null_tables", "misaligned_tables", "ntables_0", "ntables_65536", "ntables_3_without_which", "which_high",
           "which_negative", "planes_0", "planes_8", "planes_negative", "t_null_context", "t_null_hist", "t_misaligned_hist", "t_null_tables", "t_misaligned_tables",
           "t_null_rules", "t_nrules_0", "t_nrules_65", "t_which_high", "t_which_negative", "t_too_many", "t_negative_n", "check_null"]
    spoiled = ["kind_5", "kind_negative", "flat_256", "flat_negative", "flat_b", "stretch_500", "stretch_b_500", "stretch_negative", "equalize_a", "otsu_b", "identity_a", "pad"]
    want = {k: HVQ_E_ARG for k in arg + spoiled + ["check_" + s for s in spoiled]}
    want.update({"evicted": HVQ_E_STATE, "queued": HVQ_E_STATE, "n0": 0, "t_n0": 0})
    want.update({"check_good_" + n: 0 for n in cases.RULES})
    assert Rc == {"refused/" + k: v for k, v in want.items()}
    same, total = S["refused"]
    assert same == total == 2 * 4608 + 16 + 2 * 768, "a refused call wrote its output"
    g = _clip_geometry("gop64x48_15")
    assert P["refused/then_ok"] == [("gop64x48_15", "pic", 1, g, f"t{NTABLES - 1}", 7), ("gop64x48_15", "pic", fd.n_pics("gop64x48_15") - 1, g, "t0", 7)]


CHECKS = {"goldens": _check_goldens, "memory": _check_memory, "many": _check_many, "planes": _check_planes, "tables": _check_tables, "chain": _check_chain,
          "refused": _check_refused}


@pytest.mark.parametrize("schedule", ["eager", "late"])
@pytest.mark.parametrize("build", list(fd.BUILDS))
@pytest.mark.parametrize("scenario", list(CHECKS))
def test_fake_device_scenario(drivers, records, scenario, build, schedule, tmp_path):
    P, Rc, S, out = _run(drivers[build], scenario, schedule, tmp_path, records)
    CHECKS[scenario](P, Rc, S, out, records)


def test_the_existing_fake_builds_link_without_the_map_bodies():
    """the source lists of the other drivers have no hvq_launch_map and no hvq_launch_tables: the runtime's references are weak"""
    assert not any("fake_map" in s for s in fd.CXX_SOURCES)
    text = open(os.path.join(fd.CSRC, "hvq_runtime.cpp")).read()
    for sym in ("hvq_launch_map(", "hvq_launch_tables("):
        decl = [l for l in text.splitlines() if sym in l and l.startswith("extern")]
        assert len(decl) == 1 and "weak" in decl[0], sym
    exe = fd.build_driver("plain", "fake", "fake_driver", fd.CXX_SOURCES, fd.__file__)
    assert os.access(exe, os.X_OK)


# ------------------------------------------------------------------------------------------------- tools/bench_map.py
def _bench_map():
    sys.path.insert(0, os.path.join(fd.ROOT, "tools"))
    try:
        import bench_map
    finally:
        sys.path.remove(os.path.join(fd.ROOT, "tools"))
    return bench_map


def _bench_trace(tmp_path, drop=0):
    sys.path.insert(0, fd.GOLDEN)
    try:
        import make_bench_tools as mk
    finally:
        sys.path.remove(fd.GOLDEN)
    tool = _bench_map()
    blocks = [mk.block(kernel) for _label, kernel in tool.trace_plan()]
    if drop:
        blocks[-1] = blocks[-1][:-drop]
    d = str(tmp_path / "trace")
    mk.write_trace(d, blocks)
    return tool, mk, d, {"launches": 1 + mk.REPS, "pictures": 1024}


def test_bench_map_imports_without_a_gpu_and_reads_a_synthetic_trace(tmp_path):
    tool, mk, d, printed = _bench_trace(tmp_path)
    assert "torch" not in tool.__dict__ and callable(tool.main)
    labels = [label for label, _k in tool.trace_plan()]
    assert labels == ["scale_identity", "rank_identity", "chain_histograms", "invert_shared", "distinct_tables", "luma_only", "inplace", "tables_identity", "tables_flat",
                      "tables_equalize", "tables_stretch", "tables_otsu", "chain_tables", "chain_map"]
    res = tool.trace_summary(d, printed)
    assert "error" not in res, res
    for b, label in enumerate(labels):                  # block b of the helper: a warm-up launch and three of base, base + 1234, base + 4321 ns
        base = 100_000 + 7_919 * b
        assert res[label]["launches"] == mk.REPS and res[label]["median_us"] == round((base + 1_234) / 1e3, 1), label
    med = lambda label: res[label]["median_us"]
    assert res["aim"]["map_over_rank_copy"] == round(med("invert_shared") / med("rank_identity"), 2)
    assert res["aim"]["met"] is (med("invert_shared") <= 1.5 * med("rank_identity"))
    assert res["ratios"]["map_over_scale_identity"] == round(med("invert_shared") / med("scale_identity"), 2)
    assert res["chain_kernels_us"] == round(med("chain_histograms") + med("chain_tables") + med("chain_map"), 1)


def test_bench_map_refuses_a_trace_with_one_launch_too_few(tmp_path):
    tool, _mk, d, printed = _bench_trace(tmp_path, drop=1)
    res = tool.trace_summary(d, printed)
    assert "error" in res and "planned" in res["error"]
