"""CPU: the values of hvq_distance_pictures and hvq_distance_mask.  tests/distance_ref.py restates include/hvqm4_amd.h in plain Python (a
brute force over the background samples plus the border candidate); hvqm4_amd.distance (numpy: running maxima down the columns, a dense
min-plus product along the rows), scipy where it is installed, the fixture tests/golden/distance.json and the runtime on the CPU fake
device (tests/native/fake_distance.cpp, which walks the launches' grids lane by lane with the functions of hvq_distance.h) are compared
with it by ==.  The fake-device driver is a stand-alone program, built and run plain and with ASan + UBSan as tests/test_label_cpu.py
builds its own; nothing is preloaded and no Python is involved in the sanitised run."""
import json
import math
import os
import zlib

import numpy as np
import pytest

import tests.test_fake_device as fd
from hvqm4_amd import distance as D
from hvqm4_amd import labels as L
from tests import distance_cases as cases
from tests import distance_ref as ref

NATIVE = fd.NATIVE
CXX_SOURCES = [s for s in fd.CXX_SOURCES if os.path.basename(s) != "fake_driver.cpp"] + \
              [os.path.join(NATIVE, "fake_distance.cpp"), os.path.join(NATIVE, "fake_distance_driver.cpp")]
FIXTURE = json.load(open(os.path.join(fd.GOLDEN, "distance.json")))


def _ref(plane, r: D.Rule, fn=ref.distance):
    return np.array(fn(plane.tolist(), r.lo, r.hi, r.metric, r.border), dtype=np.uint32)


def _same(label, plane, r, fn=ref.distance):
    got, want = D.of_plane(plane, r), _ref(plane, r, fn)
    assert got.dtype == np.uint32 and got.shape == plane.shape, label
    assert np.array_equal(got, want), label
    return got


# ------------------------------------------------------------------------------------------------- module against reference
def test_module_equals_the_brute_force_on_the_small_planes():
    cs = cases.small_cases()
    assert {(c[3].metric, c[3].border) for c in cs} == set(cases.COMBOS) and {c[3].plane for c in cs} == {0, 1, 2}
    for label, geom, pic, r in cs:
        plane = L.plane_of(pic, geom, r.plane)
        got = _same(label, plane, r)
        assert ref.distance_by_rows(plane.tolist(), r.lo, r.hi, r.metric, r.border) == got.tolist(), label       # the fixture's restatement
        assert np.array_equal(D.of_picture(pic, geom, r), got), label


def test_module_equals_the_reference_on_the_tile_planes_and_the_mixed_pictures():
    cs = cases.tile_cases()
    assert {(c[3].metric, c[3].border) for c in cs} == set(cases.COMBOS)
    for label, geom, pic, r in cs[::4]:
        _same(label, L.plane_of(pic, geom, r.plane), r, ref.distance_by_rows)
    geoms, pics, rules, which = cases.mixed_cases(60, 64)
    assert len(set(rules)) == 64 and len(pics) == 60
    for g, p, w in list(zip(geoms, pics, which))[::3]:
        _same((g, rules[w]), L.plane_of(p, g, rules[w].plane), rules[w], ref.distance_by_rows)


def test_known_answers():
    for m in range(3):
        for b in (0, 1):
            assert not _same("empty", np.zeros((5, 8), np.uint8), D.Rule(0, 255, 255, m, b)).any()
        assert (_same("full", np.full((5, 8), 255, np.uint8), D.Rule(0, 255, 255, m, 0)) == D.NONE).all()
    got = _same("full, border", np.full((5, 8), 255, np.uint8), D.rule(border=True))
    assert got.tolist() == [[1] * 8, [1, 4, 4, 4, 4, 4, 4, 1], [1, 4, 9, 9, 9, 9, 4, 1], [1, 4, 4, 4, 4, 4, 4, 1], [1] * 8]
    one = np.full((6, 8), 255, np.uint8)
    one[0, 0] = 0
    assert [int(_same("corner", one, D.rule(metric=m))[5, 7]) for m in D.METRICS] == [74, 12, 7]
    assert D.rule() == D.Rule(0, 255, 255, 0, 0) and D.rule(metric="chess", border=True) == D.Rule(0, 255, 255, 2, 1)
    assert D.max_inscribed(got) == (9, 2, 2) and D.max_inscribed(D.of_plane(one)) == (74, 7, 5)
    assert D.max_inscribed(np.array([[0, -1], [5, -1]], dtype=np.int32)) == (D.NONE, 1, 0)                        # the int32 view of a map
    inside, outside = D.of_plane(one), D.of_plane(one, D.complement(D.rule()))
    assert D.complement(D.rule()) == D.Rule(0, 0, 254, 0, 0) and D.complement(D.Rule(1, 0, 90, 1, 1)) == D.Rule(1, 91, 255, 1, 1)
    s = D.signed(inside, outside)
    assert s.dtype == np.int64 and s[0, 0] == -1 and s[5, 7] == 74 and s[0, 1] == 1
    with pytest.raises(ValueError):
        D.signed(inside, inside)
    with pytest.raises(ValueError):
        D.complement(D.Rule(0, 3, 9))


def test_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    seen = set()
    for label, geom, pic, r in cases.small_cases()[::5] + cases.tile_cases()[::2] + cases.far_cases()[::4]:
        plane = L.plane_of(pic, geom, r.plane)
        fg = (plane >= r.lo) & (plane <= r.hi)
        if fg.all() and not r.border:
            continue                                                # scipy has no answer for a plane without background
        f = np.pad(fg, 1) if r.border else fg                       # one ring of background, cropped again
        want = np.rint(ndi.distance_transform_edt(f) ** 2) if r.metric == 0 else ndi.distance_transform_cdt(f, "taxicab" if r.metric == 1 else "chessboard")
        want = want[1:-1, 1:-1] if r.border else want
        assert np.array_equal(D.of_plane(plane, r).astype(np.int64), want.astype(np.int64)), label
        seen.add((r.metric, r.border))
    assert seen == set(cases.COMBOS)


def test_isqrt_is_exact():
    k = np.arange(1, 11586, dtype=np.int64)                          # 11585^2 < 2^27 < 11586^2
    sq = k * k
    assert D.isqrt(sq).tolist() == k.tolist() and D.isqrt(sq - 1).tolist() == (k - 1).tolist() and D.isqrt(sq + 1).tolist() == k.tolist()
    for v in (0, 1, 2, 3, 2 ** 27, 65535 ** 2 - 1, 65535 ** 2, 2 ** 32 - 2, 2 ** 32 - 1):
        assert int(D.isqrt(np.uint32(v))) == math.isqrt(v), v
    assert int(D.isqrt(np.array([-1], dtype=np.int32))[0]) == 65535


def test_masks_and_discs():
    geom = (136, 40, 2, 2)
    dist = D.of_plane(cases.mask_picture())
    dist[0, 0], dist[0, 1], dist[39, 135] = D.NONE, 255 * 255 - 1, 255 * 255
    assert {0, 1, 4, 9, 10, D.NONE} <= set(dist.reshape(-1).tolist())
    for m in cases.MASKS:
        got = D.of_mask(dist, m, geom)
        assert got.tobytes() == ref.mask(dist.tolist(), m.mode, m.lo, m.hi, m.invert, chroma_samples=68 * 20), m
        assert np.array_equal(D.of_mask(dist.view(np.int32), m, geom), got), m
        assert got.size == cases.nbytes(geom) and (got[136 * 40:] == 128).all()
    root = D.of_mask(dist, D.mask_root(), geom)
    assert root[0] == 255 and root[1] == 254 and root[136 * 40 - 1] == 255
    assert {m.mode for m in cases.MASKS} == {0, 1} and {m.invert for m in cases.MASKS} == {0, 1}
    for bad in (D.Mask(2), D.Mask(0, 5, 4), D.Mask(0, -1, 4), D.Mask(0, 0, 2 ** 32), D.Mask(0, 0, 9, 2), D.Mask(0, 0, 9, True), D.Mask(1, 1, 1), D.Mask(1, 0, 9), D.Mask(1, 0, 0, 1)):
        with pytest.raises(ValueError):
            D.check_mask(bad)
    for bad in (D.Rule(3), D.Rule(-1), D.Rule(0, 9, 8), D.Rule(0, -1, 8), D.Rule(0, 0, 256), D.Rule(0, 0, 0, 3), D.Rule(0, 0, 0, -1), D.Rule(0, 0, 0, 0, 2), D.Rule(0, 0, 0, True)):
        with pytest.raises(ValueError):
            D.check(bad)
    with pytest.raises(ValueError):
        D.rule(metric="euclid")
    g = (24, 16, 2, 1)
    for label, mask in cases.morph_masks(24, 16, 3):
        pic = cases.picture(g, 0, mask, 4)
        rows = mask.tolist()
        for r in (0, 1, 2, 3, 5):
            er, di = ref.erode_disc(rows, r), ref.dilate_disc(rows, r)
            assert D.of_steps(pic, g, D.erode_disc(r))[:384].reshape(16, 24).tolist() == er, (label, r)
            assert D.of_steps(pic, g, D.dilate_disc(r))[:384].reshape(16, 24).tolist() == di, (label, r)
            assert D.of_steps(pic, g, D.opening_disc(r))[:384].reshape(16, 24).tolist() == ref.dilate_disc(er, r), (label, r)
            assert D.of_steps(pic, g, D.closing_disc(r))[:384].reshape(16, 24).tolist() == ref.erode_disc(di, r), (label, r)
            opened = D.of_steps(pic, g, D.opening_disc(r))
            assert np.array_equal(D.of_steps(opened, g, D.opening_disc(r)), opened), (label, r, "opening is idempotent")
            assert (opened[384:] == 128).all()
    assert D.distance_bytes((24, 16, 2, 2), 0) == 4 * 384 and D.distance_bytes((24, 16, 2, 1), 2) == 4 * 12 * 16
    with pytest.raises(ValueError):
        D.as_steps([(D.Rule(1), D.mask_root())])


def test_struct_layout():
    import ctypes as C
    from hvqm4_amd._lib import HvqDistanceMask, HvqDistanceRule
    assert (C.sizeof(HvqDistanceRule), C.sizeof(HvqDistanceMask)) == (32, 32)
    assert [(n, getattr(HvqDistanceRule, n).offset) for n, _t in HvqDistanceRule._fields_] == [("plane", 0), ("lo", 4), ("hi", 8), ("metric", 12), ("border", 16), ("pad", 20)]
    assert [(n, getattr(HvqDistanceMask, n).offset) for n, _t in HvqDistanceMask._fields_] == [("mode", 0), ("lo", 4), ("hi", 8), ("invert", 12), ("pad", 16)]
    s = D.Rule(2, 3, 200, 1, 1).struct()
    assert (s.plane, s.lo, s.hi, s.metric, s.border, list(s.pad)) == (2, 3, 200, 1, 1, [0, 0, 0])
    e = D.mask_range(5, D.NONE, invert=True).struct()
    assert (e.mode, e.lo, e.hi, e.invert, list(e.pad)) == (0, 5, 2 ** 32 - 1, 1, [0, 0, 0, 0])
    assert (D.NONE, D.MAX_RULES, D.MAX_MASKS, D.METRICS) == (2 ** 32 - 1, 64, 64, ("euclid2", "city", "chess"))
    header = open(os.path.join(fd.ROOT, "include", "hvqm4_amd.h")).read()
    for line in ("#define HVQ_DST_EUCLID2 0", "#define HVQ_DST_CITY    1", "#define HVQ_DST_CHESS   2", "#define HVQ_DST_NONE    0xFFFFFFFFu", "#define HVQ_DST_MAX_RULES 64",
                 "#define HVQ_DSM_RANGE 0", "#define HVQ_DSM_ROOT  1", "#define HVQ_DSM_MAX 64",
                 "typedef struct HvqDistanceRule { int32_t plane, lo, hi, metric, border, pad[3]; } HvqDistanceRule;",
                 "typedef struct HvqDistanceMask { uint32_t mode, lo, hi, invert, pad[4]; } HvqDistanceMask;",
                 "int64_t hvq_distance_bytes(int width, int height, int h_samp, int v_samp, int plane);"):
        assert line in header, line
    assert (cases.COLS, cases.SPAN, cases.LANES, cases.TILE) == (256, 8192, 256, 8192)
    assert f"HVQ_DT_SPAN = {cases.SPAN} samples" in header


def test_the_library_without_a_device_still_checks_its_arguments():
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, HvqDistanceMask, HvqDistanceRule, lib
    one = (C.c_int * 1)(0)
    ptr = (C.c_void_p * 1)(16)
    r = D.rule().struct()
    e = D.mask_range(1).struct()
    assert lib().hvq_distance_pictures(None, 1, one, one, None, C.byref(r), 1, None, C.cast(ptr, C.c_void_p), None) == HVQ_E_ARG
    assert lib().hvq_distance_mask(None, 1, one, C.cast(ptr, C.c_void_p), C.byref(e), 1, None, C.cast(ptr, C.c_void_p), None) == HVQ_E_ARG
    assert lib().hvq_distance_check(None) == HVQ_E_ARG and lib().hvq_distance_check(C.byref(r)) == 0
    assert lib().hvq_distance_mask_check(None) == HVQ_E_ARG and lib().hvq_distance_mask_check(C.byref(e)) == 0

    def rule(plane, lo, hi, metric, border, pad=(0, 0, 0)):
        return HvqDistanceRule(plane, lo, hi, metric, border, (C.c_int32 * 3)(*pad))

    def mask(mode, lo, hi, invert, pad=(0, 0, 0, 0)):
        return HvqDistanceMask(mode, lo, hi, invert, (C.c_uint32 * 4)(*pad))
    for bad in ((3, 0, 0, 0, 0), (-1, 0, 0, 0, 0), (0, 9, 8, 0, 0), (0, -1, 8, 0, 0), (0, 0, 256, 0, 0), (0, 0, 0, 3, 0), (0, 0, 0, -1, 0), (0, 0, 0, 0, 2), (0, 0, 0, 0, -1),
                (0, 0, 0, 0, 0, (1, 0, 0)), (0, 0, 0, 0, 0, (0, 1, 0)), (0, 0, 0, 0, 0, (0, 0, 1))):
        assert lib().hvq_distance_check(C.byref(rule(*bad))) == HVQ_E_ARG, bad
    for good in ((0, 0, 0, 0, 0), (2, 0, 255, 2, 1), (1, 255, 255, 1, 0)):
        assert lib().hvq_distance_check(C.byref(rule(*good))) == 0, good
    for bad in ((2, 0, 0, 0), (0, 5, 4, 0), (0, 0, 9, 2), (0, 0, 9, 0, (1, 0, 0, 0)), (0, 0, 9, 0, (0, 0, 0, 1)), (1, 1, 1, 0), (1, 0, 9, 0), (1, 0, 0, 1)):
        assert lib().hvq_distance_mask_check(C.byref(mask(*bad))) == HVQ_E_ARG, bad
    for good in ((0, 0, 0, 0), (0, 0, 2 ** 32 - 1, 1), (1, 0, 0, 0), (0, 2 ** 32 - 1, 2 ** 32 - 1, 0)):
        assert lib().hvq_distance_mask_check(C.byref(mask(*good))) == 0, good
    for geom in ((24, 16, 2, 2), (24, 16, 2, 1), (8, 8, 1, 1)):
        for p in range(3):
            assert lib().hvq_distance_bytes(*geom, p) == D.distance_bytes(geom, p)
    assert lib().hvq_distance_bytes(24, 16, 2, 2, 3) == HVQ_E_ARG and lib().hvq_distance_bytes(24, 17, 2, 2, 0) < 0


# ------------------------------------------------------------------------------------------------- the fixture
def _otsu_mask(pic, geom):
    from hvqm4_amd import histograms as H
    from hvqm4_amd import maps as M
    return M.of_picture(pic, geom, M.from_lut(*M.tables_of_records(H.of_picture(pic, *geom), M.otsu())))


@pytest.mark.parametrize("name", sorted(FIXTURE["clips"]))
def test_fixture_equals_module(name):
    from hvqm4_amd.container import parse_header
    hdr = parse_header(open(os.path.join(fd.GOLDEN, fd.CLIPS[name]["file"]), "rb").read())
    geom = (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)
    mask = _otsu_mask(fd.oracle_pictures(name)[0].reshape(-1), geom)
    want = FIXTURE["clips"][name]
    assert zlib.crc32(D.of_picture(mask, geom, D.rule()).astype("<u4").tobytes()) == want["euclid2"], name
    assert zlib.crc32(D.of_picture(mask, geom, D.rule(metric="chess", border=True)).astype("<u4").tobytes()) == want["chess_border"], name
    assert zlib.crc32(D.of_steps(mask, geom, D.opening_disc(3)).tobytes()) == want["opening3"], name


def test_fixture_covers_every_golden_clip():
    assert sorted(FIXTURE["clips"]) == sorted(fd.CLIPS)


# ------------------------------------------------------------------------------------------------- the runtime on the CPU fake device
@pytest.fixture(scope="module")
def drivers():
    return {kind: fd.build_driver(kind, "distance", "fake_distance_driver", CXX_SOURCES, __file__) for kind in fd.BUILDS}


def _inputs(scenario):
    """-> [(label, geom, picture, Rule, mask entry or -1)]"""
    if scenario == "cases":
        cs = cases.small_cases()[::2] + cases.tile_cases() + cases.far_cases()[::3] + cases.wide_cases()[:1]
        g = (136, 40, 2, 2)
        cs += [("mask picture", g, cases.picture(g, 0, cases.mask_picture(), 1), D.rule())] * len(cases.MASKS)
        return [c + ((i % len(cases.MASKS)) if c[3].plane == 0 else -1,) for i, c in enumerate(cs)]
    if scenario == "mixed":
        geoms, pics, rules, which = cases.mixed_cases()
        return [(f"mixed {i}", g, p, rules[w], (i % len(cases.MASKS)) if rules[w].plane == 0 else -1) for i, (g, p, w) in enumerate(zip(geoms, pics, which))]
    return [("first", (8, 8, 2, 2), cases.picture((8, 8, 2, 2), 0, np.zeros((8, 8), np.uint8), 0), D.rule(lo=128, border=True), 4)]


def _run(exe, scenario, schedule, tmp_path):
    items = _inputs(scenario)
    lines = [f"M {m.mode} {m.lo} {m.hi} {m.invert}" for m in cases.MASKS]
    lines += [f"P {g[0]} {g[1]} {g[2]} {g[3]} {r.plane} {r.lo} {r.hi} {r.metric} {r.border} {s}" for _l, g, _p, r, s in items]
    out, lines = fd.run_checked(exe, scenario if scenario in ("resident", "refused", "nogpu") else "cases", schedule, tmp_path,
                                inputs={"calls.txt": "\n".join(lines) + "\n", "pictures.bin": b"".join(p.tobytes() for _l, _g, p, _r, _s in items)})
    G, P, Rc, S = [], [], {}, {}
    for line in lines:
        f = line.split()
        if f[0] == "G":
            G.append((f[1], int(f[2]), int(f[3])))
        elif f[0] == "P":
            P.append((f[1], f[2], int(f[3])))
        elif f[0] == "R":
            Rc[f[1]] = int(f[2])
        elif f[0] == "S":
            S[f[1]] = (int(f[2]), int(f[3]))
    assert all(g == 1 for _w, _i, g in G), [x for x in G if x[2] != 1][:5]
    return items, G, P, Rc, S, out


def _compare(items, G, out):
    """dist.bin, mask.bin and chain.bin against the module, picture by picture"""
    dist = np.frombuffer((out / "dist.bin").read_bytes(), dtype="<u4")
    masked = np.frombuffer((out / "mask.bin").read_bytes(), dtype=np.uint8)
    chain = np.frombuffer((out / "chain.bin").read_bytes(), dtype="<u4")
    at = mat = cat = nmask = 0
    for label, geom, pic, r, s in items:
        want = D.of_picture(pic, geom, r)
        got = dist[at:at + want.size].reshape(want.shape)
        at += want.size
        assert np.array_equal(got, want), f"{label}: {int((got != want).sum())} distances differ"
        if s >= 0:
            wm = D.of_mask(want, cases.MASKS[s], geom)
            assert np.array_equal(masked[mat:mat + wm.size], wm), f"{label}: mask {s} differs"
            mat += wm.size
            wc = D.of_picture(wm, geom, D.rule())
            assert np.array_equal(chain[cat:cat + wc.size].reshape(wc.shape), wc), f"{label}: the distances of mask {s} differ"
            cat += wc.size
            nmask += 1
    assert at == dist.size and mat == masked.size and cat == chain.size
    assert sorted(G) == sorted([("dist", i, 1) for i in range(len(items))] + [("mask", i, 1) for i in range(nmask)] + [("chain", i, 1) for i in range(nmask)])


def _check_cases(items, G, P, Rc, S, out):
    _compare(items, G, out)
    assert Rc == {"cases/n0": 0, "cases/mask_n0": 0}
    assert {(it[3].metric, it[3].border) for it in items} == set(cases.COMBOS) and {it[3].plane for it in items} == {0, 1, 2}
    assert {it[4] for it in items} == set(range(-1, len(cases.MASKS)))


def _check_mixed(items, G, P, Rc, S, out):
    assert len(items) == 60 and len({it[3] for it in items}) == 60
    _compare(items, G, out)


def _check_resident(items, G, P, Rc, S, out):
    r0, s0 = items[0][3], items[0][4]
    assert len(P) == 18 and {f for _c, f, _k in P} == {"pic", "inv"}
    real = []
    for name, form, k in P:
        from hvqm4_amd.container import parse_header
        hdr = parse_header(open(os.path.join(fd.GOLDEN, fd.CLIPS[name]["file"]), "rb").read())
        pic = fd.oracle_pictures(name)[k].reshape(-1)
        plane = k % 3
        real.append((f"{name} {form} {k}", (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp), pic if form == "pic" else 255 - pic, D.Rule(plane, r0.lo, r0.hi, k % 3, r0.border),
                     s0 if plane == 0 else -1))
    assert {g[2:] for _l, g, _p, _r, _s in real} == {(2, 2), (2, 1), (1, 1)}
    _compare(real, G, out)


_DIST_REFUSED = ["null_context", "bad_stream", "bad_ordinal", "misaligned_src", "src_with_ordinal", "minus_one_without_src", "null_rules", "nrules_0", "nrules_65", "which_high",
                 "which_negative", "null_dist", "null_map", "misaligned_map", "too_many", "negative_n", "check_null"]
_RULE_REFUSED = ["plane_3", "plane_negative", "lo_above_hi", "lo_negative", "hi_256", "metric_3", "metric_negative", "border_2", "border_negative", "pad_0", "pad_2"]
_MASK_REFUSED = ["m_null_context", "m_bad_stream", "m_null_dist", "m_null_map", "m_misaligned_map", "m_null_sel", "m_nsel_0", "m_nsel_65", "m_which_high", "m_which_negative",
                 "m_null_dst", "m_null_destination", "m_misaligned_destination", "m_too_many", "m_negative_n", "check_m_null"]
_ENTRY_REFUSED = ["m_lo_above_hi", "m_mode_2", "m_invert_2", "m_pad_0", "m_pad_3", "m_root_lo", "m_root_hi", "m_root_invert"]


def _check_refused(items, G, P, Rc, S, out):
    from hvqm4_amd._lib import HVQ_E_ARG
    want = {k: HVQ_E_ARG for k in _DIST_REFUSED + _RULE_REFUSED + ["check_" + r for r in _RULE_REFUSED] + _MASK_REFUSED + _ENTRY_REFUSED + ["check_" + r for r in _ENTRY_REFUSED]}
    want.update({"check_good": 0, "check_m_good": 0, "then_ok": 0, "then_mask_ok": 0})
    assert Rc == {"refused/" + k: v for k, v in want.items()}
    same, total = S["refused"]
    assert same == total == 2 * (4 * 64 * 48 + 64 * 48 * 2), "a refused call wrote an output"


def _check_nogpu(items, G, P, Rc, S, out):
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_NOGPU
    assert Rc == {"nogpu/distance_bad_rule": HVQ_E_ARG, "nogpu/distance": HVQ_E_NOGPU, "nogpu/mask_bad_range": HVQ_E_ARG, "nogpu/mask": HVQ_E_NOGPU, "nogpu/n0": 0}
    assert S["nogpu"][0] == S["nogpu"][1] > 0


CHECKS = {"cases": _check_cases, "mixed": _check_mixed, "resident": _check_resident, "refused": _check_refused}


@pytest.mark.parametrize("schedule", ["eager", "late"])
@pytest.mark.parametrize("build", list(fd.BUILDS))
@pytest.mark.parametrize("scenario", list(CHECKS))
def test_fake_device_scenario(drivers, scenario, build, schedule, tmp_path):
    CHECKS[scenario](*_run(drivers[build], scenario, schedule, tmp_path))


@pytest.mark.parametrize("schedule", ["eager", "late"])
def test_fake_device_without_the_distance_bodies_refuses(schedule, tmp_path):
    """a driver linked without fake_distance.cpp: the runtime's references are weak, both calls check first and then say HVQ_E_NOGPU"""
    assert not any("fake_distance" in s for s in fd.CXX_SOURCES)
    exe = fd.build_driver("plain", "distance_nogpu", "fake_distance_driver", [s for s in CXX_SOURCES if not s.endswith("fake_distance.cpp")], __file__)
    _check_nogpu(*_run(exe, "nogpu", schedule, tmp_path))


# ------------------------------------------------------------------------------------------------- tools/bench_distance.py, tools/discmorph.py
def _tool(name):
    import importlib
    import sys
    sys.path.insert(0, fd.ROOT)
    return importlib.import_module("tools." + name)


def _bench_trace(tmp_path, drop=0):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_bench_tools", os.path.join(fd.GOLDEN, "make_bench_tools.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    bench = _tool("bench_distance")
    reps = 3
    blocks = [["hvq_scale_kernel"] * (1 + reps)]
    for _p in bench.PRESETS:
        blocks.append(list(bench.DISTANCE_KERNELS) * (1 + reps))
    blocks += [[bench.MASK_KERNEL] * (1 + reps), [bench.MASK_KERNEL] * (1 + reps), ["hvq_select_kernel"] * (1 + reps)]
    if drop:
        blocks[-1] = blocks[-1][:-drop]
    gen.write_trace(str(tmp_path), blocks)
    return bench, bench.trace_summary(str(tmp_path), {"launches": 1 + reps, "pictures": 1024})


def test_bench_distance_imports_without_a_gpu_and_reads_a_synthetic_trace(tmp_path):
    bench, res = _bench_trace(tmp_path)
    assert "error" not in res, res
    assert set(bench.PRESETS) <= set(res) and set(res["kernels"]) == set(bench.DISTANCE_KERNELS) | {bench.MASK_KERNEL}
    per_byte = res["scale_identity"]["median_us"] / 3.0                  # the identity kernel moves 1.5 bytes in and 1.5 out a luma sample
    assert res["yardstick_us"] == {"column": round(13 * per_byte, 1), "row": round(8 * per_byte, 1)}
    for p in bench.PRESETS:
        row = res[p]
        assert all(row[k]["launches"] == 3 for k in bench.DISTANCE_KERNELS), "the warm-up call is left out"
        assert row["sum_median_us"] == round(sum(row[k]["median_us"] for k in bench.DISTANCE_KERNELS), 1)
        assert row["row_over_yardstick"] == round(row["hvq_distance_row_kernel"]["median_us"] / res["yardstick_us"]["row"], 2)
    assert res["mask_range"]["launches"] == res["mask_root"]["launches"] == res["select"]["launches"] == 3


def test_bench_distance_refuses_a_trace_with_one_launch_too_few(tmp_path):
    _bench, res = _bench_trace(tmp_path, drop=1)
    assert list(res) == ["error"] and "planned" in res["error"]


def test_discmorph_imports_without_a_gpu():
    disc = _tool("discmorph")
    assert callable(disc.clip_discs)
