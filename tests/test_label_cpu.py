"""CPU: the values of hvq_label_pictures and hvq_select_components.  tests/label_ref.py restates include/hvqm4_amd.h in plain Python (a
raster scan and a flood fill); hvqm4_amd.labels (numpy: runs and a union-find), scipy where it is installed, the fixture
tests/golden/label.json and the runtime on the CPU fake device (tests/native/fake_label.cpp, which walks the launches' grids lane by lane
with the functions of hvq_label.h) are compared with it by ==.  The fake-device driver is a stand-alone program, built and run plain and
with ASan + UBSan as tests/test_map_cpu.py builds its own; nothing is preloaded and no Python is involved in the sanitised run."""
import json
import os
import zlib

import numpy as np
import pytest

import tests.test_fake_device as fd
from hvqm4_amd import labels as L
from tests import label_cases as cases
from tests import label_ref as ref

NATIVE = fd.NATIVE
CXX_SOURCES = [s for s in fd.CXX_SOURCES if os.path.basename(s) != "fake_driver.cpp"] + \
              [os.path.join(NATIVE, "fake_label.cpp"), os.path.join(NATIVE, "fake_label_driver.cpp")]
FIXTURE = json.load(open(os.path.join(fd.GOLDEN, "label.json")))


def _ref(plane, r: L.Rule, cap=None):
    lab, rec = ref.label(plane.tolist(), r.lo, r.hi, r.connectivity, cap)
    return np.array(lab, dtype=np.uint32), np.array(rec, dtype=np.int64)


def _same(label, plane, r, cap=None):
    got, want = L.of_plane(plane, r, cap), _ref(plane, r, cap)
    assert got[0].dtype == np.uint32 and got[1].dtype == np.int64 and got[0].shape == plane.shape, label
    assert np.array_equal(got[0], want[0]), label
    assert got[1].shape == want[1].shape and np.array_equal(got[1], want[1]), label
    return got


# ------------------------------------------------------------------------------------------------- module against reference
@pytest.mark.parametrize("group", ["small", "seam", "wide"])
def test_module_equals_reference(group):
    for label, geom, pic, r in getattr(cases, group + "_cases")():
        lab, rec = _same(label, L.plane_of(pic, geom, r.plane), r)
        assert int(rec[1:, 0].sum()) == int(rec[0, 2]), label                 # the areas add up to F
        again = L.of_picture(pic, geom, r)
        assert np.array_equal(again[0], lab) and np.array_equal(again[1], rec), label


def test_module_equals_reference_on_the_mixed_pictures_and_under_every_cap():
    geoms, pics, rules, which = cases.mixed_cases(60, 64)
    assert len(set(rules)) == 64
    for g, p, w in zip(geoms, pics, which):
        _same((g, rules[w]), L.plane_of(p, g, rules[w].plane), rules[w])
    board = L.plane_of(cases.small_cases()[4][2], (8, 8, 2, 2), 0)
    for cap in (33, 32, 31, 1, 0):
        lab, rec = _same(("cap", cap), board, L.rule(connectivity=4), cap)
        assert rec[0].tolist()[:3] == [32, min(32, cap), 32] and rec.shape[0] == min(32, cap) + 1 and int(lab.max()) == 32


def test_known_answers():
    nx, ny = 72, 24
    for conn in (4, 8):
        r = L.rule(connectivity=conn)
        lab, rec = _same("empty", np.zeros((ny, nx), np.uint8), r)
        assert rec.tolist() == [[0] * 8] and not lab.any()
        lab, rec = _same("full", np.full((ny, nx), 255, np.uint8), r)
        assert rec.tolist() == [[1, 1, nx * ny, 0, 0, 0, 0, 0], [nx * ny, 0, 0, nx - 1, ny - 1, 0, ny * nx * (nx - 1) // 2, nx * ny * (ny - 1) // 2]]
        assert (lab == 1).all()
        lab, rec = _same("two", np.array([[255, 0, 0, 0], [0, 255, 0, 0]], np.uint8), r)
        assert rec[0, 0] == (2 if conn == 4 else 1)
        u = cases.us(nx, ny)
        lab, rec = _same("U", u, r)
        assert rec[0, 0] == 2 and lab[0, 1] == 1 and lab[0, cases.TX - 3] == 1 and lab[0, cases.TX + 1] == 2
    yy, xx = np.mgrid[0:ny, 0:nx]
    board = (((xx + yy) & 1) == 1).astype(np.uint8) * 255
    lab, rec = _same("check, 4", board, L.rule(connectivity=4))
    assert rec[0].tolist()[:3] == [nx * ny // 2] * 3 and (rec[1:, 0] == 1).all()
    assert np.array_equal(lab[board == 255], np.arange(1, nx * ny // 2 + 1))
    lab, rec = _same("check, 8", board, L.rule(connectivity=8))
    assert rec[0, 0] == 1 and rec[1, 0] == nx * ny // 2
    odd = (((np.mgrid[0:3, 0:3][0] + np.mgrid[0:3, 0:3][1]) & 1) == 0).astype(np.uint8) * 255
    assert L.of_plane(np.pad(odd, ((0, 0), (0, 1))), L.rule(connectivity=4))[1][0, 0] == 5          # ceil(9 / 2) whites of a 3 x 3 board
    for label, mask, _lo, _hi in cases.seam_masks(2 * cases.TX + 8, 2 * cases.TY + 8):
        k4, k8 = (int(L.of_plane(mask, L.rule(connectivity=c))[1][0, 0]) for c in (4, 8))
        F = int((mask == 255).sum())
        want = {"serpentine": (1, 1), "serpentine transposed": (1, 1), "comb": (1, 1), "U per tile column": (3, 3), "lattice": (F, 1), "corner blobs": (2, 1),
                "corner blobs, anti": (2, 1)}.get(label)
        if want:
            assert (k4, k8) == want, label
        if label == "diagonals":
            assert k4 == F and k8 < F // 8


def test_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for label, geom, pic, r in cases.small_cases()[::3] + cases.seam_cases():
        plane = L.plane_of(pic, geom, r.plane)
        fg = (plane >= r.lo) & (plane <= r.hi)
        want, K = ndi.label(fg, structure=np.ones((3, 3)) if r.connectivity == 8 else None)
        lab, rec = L.of_plane(plane, r)
        assert K == rec[0, 0] and np.array_equal(lab, want.astype(np.uint32)), label
        for k, sl in enumerate(ndi.find_objects(want), 1):
            assert (sl[1].start, sl[0].start, sl[1].stop - 1, sl[0].stop - 1) == tuple(rec[k, 1:5]), (label, k)


def test_records_and_select():
    mask = np.zeros((16, 24), np.uint8)
    mask[1:4, 1:3] = 255            # 1: area 6, 2 x 3
    mask[1, 8:18] = 255             # 2: area 10, 10 x 1
    mask[6:16, 20] = 255            # 3: area 10, 1 x 10
    mask[10, 3] = 255               # 4: a speck
    geom = (24, 16, 2, 2)
    lab, rec = L.of_plane(mask, L.rule())
    R = L.records(rec)
    assert (R.K, R.stored, R.F, R.status) == (4, 4, 27, 0) and R["area"].tolist() == [6, 10, 10, 1]
    assert L.boxes(R).tolist() == [[1, 1, 2, 3], [8, 1, 17, 1], [20, 6, 20, 15], [3, 10, 3, 10]]
    assert L.centroids(R).tolist() == [[1.5, 2.0], [12.5, 1.0], [20.0, 10.5], [3.0, 10.0]]
    assert L.largest(R, 3).tolist() == [2, 3, 1] and L.largest(R, 9).tolist() == [2, 3, 1, 4]
    flat = [[int(v) for v in row] for row in lab]
    recs = rec.tolist()

    def both(sel, **kw):
        got = L.of_select(lab, rec, sel, geom)
        assert got.tobytes() == ref.select(flat, recs, chroma_samples=12 * 8, **kw)
        assert (got[24 * 16:] == 128).all() and got.size == cases.nbytes(geom)
        return sorted(set(lab.reshape(-1)[got[:24 * 16] == 255].tolist()))
    assert both(L.select()) == [1, 2, 3, 4]
    assert both(L.select(area=2), area=(2, 2 ** 32 - 1)) == [1, 2, 3]
    assert both(L.select(area=(6, 6)), area=(6, 6)) == [1] and both(L.select(area=(7, 9)), area=(7, 9)) == []
    assert both(L.select(width=(10, 10)), width=(10, 10)) == [2] and both(L.select(width=(None, 1)), width=(0, 1)) == [3, 4]
    assert both(L.select(height=(3, 10)), height=(3, 10)) == [1, 3] and both(L.select(height=11), height=(11, 2 ** 32 - 1)) == []
    assert both(L.select(area=2, invert=True), area=(2, 2 ** 32 - 1), invert=1) == [0, 4]
    lab2, rec2 = L.of_plane(mask, L.rule(), cap=2)                        # labels 3 and 4 have no record: not selected
    got = L.of_select(lab2, rec2, L.select(), geom)
    assert got.tobytes() == ref.select(flat, rec2.tolist(), chroma_samples=96) and sorted(set(lab2.reshape(-1)[got[:384] == 255].tolist())) == [1, 2]
    for bad in (dict(area=(5, 4)), dict(width=(2, 1)), dict(height=(-1, 1)), dict(area=2 ** 32)):
        with pytest.raises(ValueError):
            L.select(**bad)
    for bad in (L.Rule(3), L.Rule(-1), L.Rule(0, 9, 8), L.Rule(0, -1, 8), L.Rule(0, 0, 256), L.Rule(0, 0, 0, 6), L.Rule(0, 0, 0, True)):
        with pytest.raises(ValueError):
            L.check(bad)
    assert L.label_bytes((24, 16, 2, 2), 0) == 4 * 384 and L.label_bytes((24, 16, 2, 1), 2) == 4 * 12 * 16 and L.label_bytes((24, 16, 1, 1), 1) == 4 * 384


def test_struct_layout():
    import ctypes as C
    from hvqm4_amd._lib import HvqLabelRule, HvqSelect
    assert (C.sizeof(HvqLabelRule), C.sizeof(HvqSelect)) == (16, 32)
    assert [(n, getattr(HvqLabelRule, n).offset) for n, _t in HvqLabelRule._fields_] == [("plane", 0), ("lo", 4), ("hi", 8), ("connectivity", 12)]
    assert [(n, getattr(HvqSelect, n).offset) for n, _t in HvqSelect._fields_] == [(n, 4 * i) for i, n in enumerate(
        ("area_min", "area_max", "w_min", "w_max", "h_min", "h_max", "invert", "pad"))]
    s = L.Rule(2, 3, 200, 4).struct()
    assert (s.plane, s.lo, s.hi, s.connectivity) == (2, 3, 200, 4)
    e = L.select(area=(5, 9), width=3, height=(None, 7), invert=True).struct()
    assert (e.area_min, e.area_max, e.w_min, e.w_max, e.h_min, e.h_max, e.invert, e.pad) == (5, 9, 3, 2 ** 32 - 1, 0, 7, 1, 0)
    assert (L.MAX_RULES, L.MAX_CAP, L.INCOMPLETE, L.MAX_SELECTS, len(L.FIELDS)) == (64, 1 << 20, 1, 64, 8)
    header = open(os.path.join(fd.ROOT, "include", "hvqm4_amd.h")).read()
    for line in ("#define HVQ_LBL_MAX_RULES 64", "#define HVQ_LBL_MAX_CAP   (1 << 20)", "#define HVQ_LBL_INCOMPLETE 1", "#define HVQ_SEL_MAX 64",
                 "typedef struct HvqLabelRule { int32_t plane, lo, hi, connectivity; } HvqLabelRule;",
                 "typedef struct HvqSelect { uint32_t area_min, area_max, w_min, w_max, h_min, h_max, invert, pad; } HvqSelect;",
                 "int64_t hvq_label_bytes(int width, int height, int h_samp, int v_samp, int plane);"):
        assert line in header, line
    assert (cases.TX, cases.TY) == (64, 16)
    assert f"HVQ_LB_TX x HVQ_LB_TY = {cases.TX} x {cases.TY}" in header


def test_the_library_without_a_device_still_checks_its_arguments():
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, lib
    one = (C.c_int * 1)(0)
    ptr = (C.c_void_p * 1)(16)
    r = L.rule().struct()
    e = L.select().struct()
    assert lib().hvq_label_pictures(None, 1, one, one, None, C.byref(r), 1, None, C.cast(ptr, C.c_void_p), C.cast(ptr, C.c_void_p), 4, None) == HVQ_E_ARG
    assert lib().hvq_select_components(None, 1, one, C.cast(ptr, C.c_void_p), C.cast(ptr, C.c_void_p), 4, C.byref(e), 1, None, C.cast(ptr, C.c_void_p), None) == HVQ_E_ARG
    assert lib().hvq_label_check(None) == HVQ_E_ARG and lib().hvq_label_check(C.byref(r)) == 0
    from hvqm4_amd._lib import HvqLabelRule
    for bad in ((3, 0, 0, 8), (-1, 0, 0, 8), (0, 9, 8, 8), (0, -1, 8, 8), (0, 0, 256, 8), (0, 0, 0, 6), (0, 0, 0, 0)):
        assert lib().hvq_label_check(C.byref(HvqLabelRule(*bad))) == HVQ_E_ARG, bad
    for good in ((0, 0, 0, 4), (2, 0, 255, 8), (1, 255, 255, 4)):
        assert lib().hvq_label_check(C.byref(HvqLabelRule(*good))) == 0, good
    for geom in ((24, 16, 2, 2), (24, 16, 2, 1), (8, 8, 1, 1)):
        for p in range(3):
            assert lib().hvq_label_bytes(*geom, p) == L.label_bytes(geom, p)
    assert lib().hvq_label_bytes(24, 16, 2, 2, 3) == HVQ_E_ARG and lib().hvq_label_bytes(24, 17, 2, 2, 0) < 0


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
    for conn in (4, 8):
        lab, rec = L.of_picture(mask, geom, L.rule(connectivity=conn))
        want = FIXTURE["clips"][name][str(conn)]
        assert (zlib.crc32(lab.astype("<u4").tobytes()), zlib.crc32(rec.astype("<u8").tobytes()), int(rec[0, 0])) == (want["labels"], want["records"], want["K"]), (name, conn)


def test_fixture_covers_every_golden_clip():
    assert sorted(FIXTURE["clips"]) == sorted(fd.CLIPS)


# ------------------------------------------------------------------------------------------------- the runtime on the CPU fake device
@pytest.fixture(scope="module")
def drivers():
    return {kind: fd.build_driver(kind, "label", "fake_label_driver", CXX_SOURCES, __file__) for kind in fd.BUILDS}


def _inputs(scenario):
    """-> (cap, [(label, geom, picture, Rule, selection or -1)])"""
    if scenario == "cases":
        cs = cases.small_cases() + cases.seam_cases() + cases.wide_cases() + cases.counted_cases(32)
        cs += [("select mask", (136, 40, 2, 2), cases.picture((136, 40, 2, 2), 0, cases.select_mask(), 1), L.rule())] * len(cases.SELECTS)
        return 32, [c + ((i % len(cases.SELECTS)) if c[3].plane == 0 else -1,) for i, c in enumerate(cs)]
    if scenario == "cap0":
        return 0, [c + (i % 2 * 12 if c[3].plane == 0 else -1,) for i, c in enumerate(cases.counted_cases(32) + cases.small_cases()[:40])]
    if scenario == "mixed":
        geoms, pics, rules, which = cases.mixed_cases()
        return 64, [(f"mixed {i}", g, p, rules[w], (i % len(cases.SELECTS)) if rules[w].plane == 0 else -1) for i, (g, p, w) in enumerate(zip(geoms, pics, which))]
    return 8, [("first", (8, 8, 2, 2), cases.picture((8, 8, 2, 2), 0, np.zeros((8, 8), np.uint8), 0), L.rule(), 1)]


def _run(exe, scenario, schedule, tmp_path):
    cap, items = _inputs(scenario)
    lines = [f"cap {cap}"] + [f"S {s.area_min} {s.area_max} {s.w_min} {s.w_max} {s.h_min} {s.h_max} {s.invert}" for s in cases.SELECTS]
    lines += [f"P {g[0]} {g[1]} {g[2]} {g[3]} {r.plane} {r.lo} {r.hi} {r.connectivity} {s}" for _l, g, _p, r, s in items]
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
    return cap, items, G, P, Rc, S, out


def _compare(cap, items, G, out):
    """labels.bin, comps.bin and select.bin against the module, picture by picture"""
    labels = np.frombuffer((out / "labels.bin").read_bytes(), dtype="<u4")
    comps = np.frombuffer((out / "comps.bin").read_bytes(), dtype="<u8").reshape(len(items), cap + 1, 8)
    picked = np.frombuffer((out / "select.bin").read_bytes(), dtype=np.uint8)
    filler = int.from_bytes(b"\xa5" * 8, "little")
    at = sat = nsel = 0
    for i, (label, geom, pic, r, s) in enumerate(items):
        lab, rec = L.of_picture(pic, geom, r, cap)
        got = labels[at:at + lab.size].reshape(lab.shape)
        at += lab.size
        assert comps[i, 0, 3] == 0, f"{label}: status {comps[i, 0, 3]}"
        assert np.array_equal(got, lab), f"{label}: {int((got != lab).sum())} labels differ"
        assert np.array_equal(comps[i, :rec.shape[0]].astype(np.int64), rec), f"{label}: the records differ"
        assert (comps[i, rec.shape[0]:] == filler).all(), f"{label}: a row beyond `stored` was written"
        if s >= 0:
            want = L.of_select(lab, rec, cases.SELECTS[s], geom)
            assert np.array_equal(picked[sat:sat + want.size], want), f"{label}: selection {s} differs"
            sat += want.size
            nsel += 1
    assert at == labels.size and sat == picked.size
    assert sorted(G) == sorted([("labels", i, 1) for i in range(len(items))] + [("comps", i, 1) for i in range(len(items))] + [("select", i, 1) for i in range(nsel)])


def _check_cases(cap, items, G, P, Rc, S, out):
    _compare(cap, items, G, out)
    assert Rc == {"cases/n0": 0, "cases/select_n0": 0}
    assert len({it[3] for it in items}) > 8 and {it[3].plane for it in items} == {0, 1, 2}
    assert {int(L.of_picture(p, g, r)[1][0, 0]) for _l, g, p, r in cases.counted_cases(32)} == {31, 32, 33}


def _check_cap0(cap, items, G, P, Rc, S, out):
    assert cap == 0
    _compare(cap, items, G, out)


def _check_mixed(cap, items, G, P, Rc, S, out):
    assert len(items) == 300 and len({it[3] for it in items}) == 64
    _compare(cap, items, G, out)


def _check_resident(cap, items, G, P, Rc, S, out):
    r0, s0 = items[0][3], items[0][4]
    assert len(P) == 18 and {f for _c, f, _k in P} == {"pic", "inv"}
    real = []
    for name, form, k in P:
        from hvqm4_amd.container import parse_header
        hdr = parse_header(open(os.path.join(fd.GOLDEN, fd.CLIPS[name]["file"]), "rb").read())
        pic = fd.oracle_pictures(name)[k].reshape(-1)
        plane = k % 3
        real.append((f"{name} {form} {k}", (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp), pic if form == "pic" else 255 - pic, L.Rule(plane, r0.lo, r0.hi, r0.connectivity),
                     s0 if plane == 0 else -1))
    assert {g[2:] for _l, g, _p, _r, _s in real} == {(2, 2), (2, 1), (1, 1)}
    _compare(cap, real, G, out)


_LABEL_REFUSED = ["null_context", "bad_stream", "bad_ordinal", "misaligned_src", "src_with_ordinal", "minus_one_without_src", "null_rules", "nrules_0", "nrules_65", "which_high",
                  "which_negative", "cap_negative", "cap_beyond", "null_labels", "null_label_map", "misaligned_label_map", "null_comps", "null_record_table",
                  "misaligned_record_table", "too_many", "negative_n", "check_null"]
_RULE_REFUSED = ["plane_3", "plane_negative", "lo_above_hi", "lo_negative", "hi_256", "connectivity_6", "connectivity_0"]
_SELECT_REFUSED = ["s_null_context", "s_bad_stream", "s_null_labels", "s_null_label_map", "s_misaligned_label_map", "s_null_comps", "s_null_record_table", "s_misaligned_record_table",
                   "s_cap_negative", "s_cap_beyond", "s_null_sel", "s_nsel_0", "s_nsel_65", "s_which_high", "s_which_negative", "s_null_dst", "s_null_destination",
                   "s_misaligned_destination", "s_too_many", "s_negative_n", "s_area", "s_width", "s_height", "s_invert_2", "s_pad"]


def _check_refused(cap, items, G, P, Rc, S, out):
    from hvqm4_amd._lib import HVQ_E_ARG
    want = {k: HVQ_E_ARG for k in _LABEL_REFUSED + _RULE_REFUSED + ["check_" + r for r in _RULE_REFUSED] + _SELECT_REFUSED}
    want.update({"check_good": 0, "then_ok": 0, "then_select_ok": 0})
    assert Rc == {"refused/" + k: v for k, v in want.items()}
    same, total = S["refused"]
    assert same == total == 2 * (4 * 64 * 48 + 64 * 9 + 64 * 48 * 2), "a refused call wrote an output"


def _check_nogpu(cap, items, G, P, Rc, S, out):
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_NOGPU
    assert Rc == {"nogpu/label_bad_rule": HVQ_E_ARG, "nogpu/label": HVQ_E_NOGPU, "nogpu/select_bad_cap": HVQ_E_ARG, "nogpu/select": HVQ_E_NOGPU, "nogpu/n0": 0}
    assert S["nogpu"][0] == S["nogpu"][1] > 0


CHECKS = {"cases": _check_cases, "cap0": _check_cap0, "mixed": _check_mixed, "resident": _check_resident, "refused": _check_refused}


@pytest.mark.parametrize("schedule", ["eager", "late"])
@pytest.mark.parametrize("build", list(fd.BUILDS))
@pytest.mark.parametrize("scenario", list(CHECKS))
def test_fake_device_scenario(drivers, scenario, build, schedule, tmp_path):
    CHECKS[scenario](*_run(drivers[build], scenario, schedule, tmp_path))


@pytest.mark.parametrize("schedule", ["eager", "late"])
def test_fake_device_without_the_label_bodies_refuses(schedule, tmp_path):
    """a driver linked without fake_label.cpp: the runtime's references are weak, both calls check first and then say HVQ_E_NOGPU"""
    assert not any("fake_label" in s for s in fd.CXX_SOURCES)
    exe = fd.build_driver("plain", "label_nogpu", "fake_label_driver", [s for s in CXX_SOURCES if not s.endswith("fake_label.cpp")], __file__)
    _check_nogpu(*_run(exe, "nogpu", schedule, tmp_path))


# ------------------------------------------------------------------------------------------------- tools/bench_label.py, tools/objects.py
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
    bench = _tool("bench_label")
    reps = 3
    blocks = [["hvq_scale_kernel"] * (1 + reps)]
    for _p in bench.PRESETS:
        blocks += [list(bench.LABEL_KERNELS) * (1 + reps), ["hvq_select_kernel"] * (1 + reps)]
    if drop:
        blocks[-1] = blocks[-1][:-drop]
    gen.write_trace(str(tmp_path), blocks)
    return bench, bench.trace_summary(str(tmp_path), {"launches": 1 + reps, "pictures": 1024})


def test_bench_label_imports_without_a_gpu_and_reads_a_synthetic_trace(tmp_path):
    bench, res = _bench_trace(tmp_path)
    assert "error" not in res, res
    assert set(bench.PRESETS) <= set(res) and set(res["kernels"]) == set(bench.LABEL_KERNELS) | {"hvq_select_kernel"}
    luma = res["scale_identity"]["median_us"] * (640 * 480) / (640 * 480 * 3 // 2)
    assert res["yardstick_us"] == round(2.5 * luma, 1)
    for p in bench.PRESETS:
        row = res[p]
        assert all(row[k]["launches"] == 3 for k in bench.LABEL_KERNELS) and row["select"]["launches"] == 3, "the warm-up call is left out"
        assert row["sum_median_us"] == round(sum(row[k]["median_us"] for k in bench.LABEL_KERNELS), 1)
        assert row["sum_over_yardstick"] == round(row["sum_median_us"] / res["yardstick_us"], 2)


def test_bench_label_refuses_a_trace_with_one_launch_too_few(tmp_path):
    _bench, res = _bench_trace(tmp_path, drop=1)
    assert list(res) == ["error"] and "planned" in res["error"]


def test_objects_imports_without_a_gpu():
    objects = _tool("objects")
    assert objects.CAP == 1024 and callable(objects.clip_objects)
