"""CPU: the values of hvq_corner_pictures.  tests/corner_ref.py restates include/hvqm4_amd.h in plain Python (ints, loops, math.isqrt);
hvqm4_amd.corners (numpy: shifted slices, cumulative sums, shifted comparisons), the fixture tests/golden/corners.json and the runtime on
the CPU fake device (tests/native/fake_corner.cpp, which walks the launches' grids lane by lane with the functions of hvq_corner.h) are
compared with it by ==.  The fake-device driver is a stand-alone program, built and run plain and with ASan + UBSan as
tests/test_integral_cpu.py builds its own; nothing is preloaded and no Python is involved in the sanitised run."""
import json
import os
import zlib

import numpy as np
import pytest

import tests.test_fake_device as fd
from hvqm4_amd import corners as cr
from tests import corner_cases as cases
from tests import corner_ref as ref

NATIVE = fd.NATIVE
CXX_SOURCES = [s for s in fd.CXX_SOURCES if os.path.basename(s) != "fake_driver.cpp"] + \
              [os.path.join(NATIVE, "fake_corner.cpp"), os.path.join(NATIVE, "fake_corner_driver.cpp")]
FIXTURE = json.load(open(os.path.join(fd.GOLDEN, "corners.json")))


def _ref(a, r: cr.Rule, cap=None):
    mask, points, rows, R = ref.corners(a.tolist(), r.mode, r.radius, r.k, r.nms, r.margin, r.threshold, cap)
    return np.array(mask, dtype=np.uint8), np.array(points, dtype=np.int64).reshape(-1, 4), np.array(rows, dtype=np.uint32), np.array(R, dtype=np.int64)


def _same(label, a, r, cap=None):
    want = _ref(a, r, cap)
    got = cr.of_plane(a, r, cap) + (cr.response_of_plane(a, r),)
    assert [g.dtype for g in got] == [np.uint8, np.int64, np.uint32, np.int64], label
    for g, w, what in zip(got, want, ("mask", "points", "rows", "response")):
        assert g.shape == w.shape and np.array_equal(g, w), (label, what)
    return got


# ------------------------------------------------------------------------------------------------- module against reference
@pytest.mark.parametrize("name", sorted(cases.SMALL))
def test_module_equals_reference(name):
    for r in cases.RULES + cases.EXTREME:
        _same((name, r), cases.SMALL[name], r)


def test_module_equals_reference_under_margins_thresholds_and_caps():
    a = cases.SMALL["blobs"]
    K = int(cr.of_plane(a, cr.harris(1, 10, nms=1))[1][0, 0])
    assert K >= 3
    for cap in (0, 1, K - 1, K, K + 1):
        _m, p, _r, _R = _same(("cap", cap), a, cr.harris(1, 10, nms=1), cap)
        assert p[0].tolist() == [K, min(K, cap), 0, 0] and p.shape[0] == min(K, cap) + 1
    for margin in (1, 3, 9, 12, 255):
        _same(("margin", margin), a, cr.harris(1, 10, nms=2, margin=margin))
    assert cr.of_plane(a, cr.harris(1, 10, margin=9))[1][0, 0] == 0                       # half the plane's height
    pts = cr.records(cr.of_plane(a, cr.min_eigen(1, nms=2))[1])
    R = int(pts[pts.shape[0] // 2, 2])
    at, over = (_same(("threshold", t), a, cr.min_eigen(1, threshold=t, nms=2))[1] for t in (R, R + 1))
    assert R in at[1:, 2] and R not in over[1:, 2] and at[0, 0] > over[0, 0]


def test_module_of_picture_fills_the_other_planes():
    for geom, plane in (((24, 16, 2, 2), 0), ((24, 16, 2, 2), 1), ((24, 16, 2, 1), 2), ((8, 8, 1, 1), 1)):
        ny, nx = cr.plane_shape(geom, plane)
        a = cases.noise(ny, nx, plane)
        pic = cases.picture(geom, plane, a, 3)
        mask, points, rows = cr.of_picture(pic, geom, cr.harris(1, 10, nms=1, plane=plane))
        m, p, r = cr.of_plane(a, cr.harris(1, 10, nms=1, plane=plane))
        assert mask.size == cases.nbytes(geom) and np.array_equal(points, p) and np.array_equal(rows, r)
        for q in range(3):
            assert np.array_equal(cr.plane_of(mask, geom, q), m if q == plane else np.full(cr.plane_shape(geom, q), 128 if q else 0, np.uint8))
        assert cr.nbytes(geom, plane, 7) == (cases.nbytes(geom), 32 * 8, 4 * (ny + 1), 8 * nx * ny)


def test_known_answers():
    """the header's list, for both measures and r = 1, 2, 3"""
    ny, nx = 24, 32
    header = open(os.path.join(fd.ROOT, "include", "hvqm4_amd.h")).read()
    for r in (1, 2, 3):
        for rule in (cr.harris(r, 10, nms=1), cr.harris(r, 64, nms=1), cr.harris(r, 0, nms=0), cr.min_eigen(r, nms=1), cr.min_eigen(r, nms=0)):
            assert cr.of_plane(cases.flat(ny, nx), rule)[1].tolist() == [[0, 0, 0, 0]], rule
            R = cr.response_of_plane(cases.vertical_edge(ny, nx), rule)
            assert (R <= 0).all() and (rule.mode == cr.HARRIS or (R == 0).all()), rule
            assert cr.of_plane(cases.vertical_edge(ny, nx), rule)[1][0, 0] == 0
            R = cr.response_of_plane(cases.checkerboard(ny, nx), rule)
            assert (R[r + 2:ny - r - 2, r + 2:nx - r - 2] == 0).all(), rule
        for rule in (cr.harris(r, 10, nms=1), cr.min_eigen(r, nms=1)):
            pts = cr.records(cr.of_plane(cases.checkerboard(ny, nx), rule)[1])
            assert pts[:, :2].tolist() == [[0, 0], [nx - 1, 0], [0, ny - 1], [nx - 1, ny - 1]], rule
        assert (cr.response_of_plane(cases.stripes4(ny, nx), cr.min_eigen(r)) == 0).all()
    R = cr.response_of_plane(cases.stripes4(ny, nx), cr.harris(3, 64))
    assert int(R.min()) == -166330855434240000 == -64 * (49 * 1020 * 1020) ** 2 and int(R.min()).bit_length() == 58
    assert "-166 330 855 434 240 000" in header
    q = cases.quadrant()
    assert q.shape == (24, 32)
    assert cr.of_plane(q, cr.harris(1, 10, nms=3))[1].tolist() == [[1, 1, 0, 0], [13, 10, 2192466340080000, 10 * 32 + 13]]
    assert "2 192 466 340 080 000" in header
    assert cr.of_plane(q, cr.harris(2, 10, nms=3))[1][:, :2].tolist() == [[1, 1], [14, 11]]
    assert cr.of_plane(q, cr.harris(3, 10, nms=3))[1][:, :2].tolist() == [[1, 1], [15, 12]]
    for r in (1, 2, 3):                                                       # the reference agrees on a cut of the plane around the corner
        cut = q[4:20, 6:24]
        assert _ref(cut, cr.harris(r, 10, nms=3))[1].tolist() == cr.of_plane(cut, cr.harris(r, 10, nms=3))[1].tolist()


def test_the_arithmetic_planes_hold_both_kinds_of_radicand():
    """the min-eigenvalue radicand (A - C)^2 + 4 B^2 is a perfect square on the edge plane everywhere, and on the plane of 0 / 1 samples
    it is a perfect square at some samples and one less than one at others, at r = 1 and at r = 3: both roundings of isqrt are met"""
    import math
    items = {it[0]: it for it in cases.arithmetic_cases()}
    for r in (1, 3):
        for name, least_square, least_below in (("edge", 24 * 72, 0), ("bits", 20, 20)):
            _l, g, pic, rule, _q = items[f"{name}: min-eigen r {r}"]
            assert rule.mode == cr.MIN_EIGEN and rule.radius == r
            a = cr.plane_of(pic, g, rule.plane).tolist()
            v = [(A - C) ** 2 + 4 * B * B for y in range(len(a)) for x in range(len(a[0])) for A, B, C in (ref.sums(a, y, x, r),)]
            square = sum(1 for x in v if math.isqrt(x) ** 2 == x)
            below = sum(1 for x in v if x and math.isqrt(x + 1) ** 2 == x + 1)
            assert square >= least_square and below >= least_below, (name, r, square, below)


def test_seam_blocks_equal_the_block_in_the_middle_of_a_tile_shifted():
    """a block whose window, suppression distance and Sobel taps stay inside the plane sees nothing of where it lies"""
    cs = cases.seam_cases()
    r = cs[-1][3]
    ny, nx = cases.WIDE[1], cases.WIDE[0]
    my, mx = 8 + 2 * cases.TY, 24 + 2 * cases.TX
    mid = cr.records(cr.of_picture(cs[-1][2], cases.WIDE, r)[1])
    assert mid.shape[0] >= 1
    reach = r.nms + r.radius + 2
    shifted = 0
    for (y, x), (_l, g, pic, rule, _q) in zip([(y, x) for y in cases.SEAM_ROWS for x in cases.SEAM_COLUMNS], cs):
        pts = cr.records(cr.of_picture(pic, g, rule)[1])
        if y >= reach and x >= reach and y + 3 + reach <= ny and x + 3 + reach <= nx:
            want = mid + np.array([x - mx, y - my, 0, (y - my) * nx + (x - mx)])
            assert np.array_equal(pts, want), (y, x)
            shifted += 1
    assert shifted == 3 * 6                                                  # rows 15, 16, 17 x columns 62 .. 65, 127, 128


def test_records_strongest_and_grid():
    a = cases.blobs(24, 72, 12)
    _m, points, _r = cr.of_plane(a, cr.harris(1, 10, nms=1))
    rec = cr.records(points)
    assert rec.shape == (int(points[0, 1]), 4) and (np.diff(rec[:, 3]) > 0).all()
    top = cr.strongest(points, 5)
    order = sorted(rec.tolist(), key=lambda p: (-p[2], p[3]))
    assert top.tolist() == order[:5] and cr.strongest(points, 0).shape == (0, 4) and cr.strongest(points, 10 ** 6).tolist() == order
    g = cr.grid(points, 8)
    best = {}
    for p in order[::-1]:
        best[(p[1] // 8, p[0] // 8)] = p
    assert g.tolist() == sorted(best.values(), key=lambda p: p[3])
    assert cr.grid(np.array([[0, 0, 0, 0]]), 8).shape == (0, 4)
    with pytest.raises(ValueError):
        cr.records(np.array([[5, 3, 0, 0], [1, 1, 1, 1]]))
    with pytest.raises(ValueError):
        cr.grid(points, 0)


# ------------------------------------------------------------------------------------------------- the header and the library
def test_rule_struct_constants_and_header():
    import ctypes as C
    from hvqm4_amd._lib import HvqCornerRule
    assert C.sizeof(HvqCornerRule) == 40
    assert [(n, getattr(HvqCornerRule, n).offset) for n in ("plane", "mode", "radius", "k", "nms", "margin", "pad", "threshold")] == \
           [("plane", 0), ("mode", 4), ("radius", 8), ("k", 12), ("nms", 16), ("margin", 20), ("pad", 24), ("threshold", 32)]
    s = cr.Rule(2, cr.MIN_EIGEN, 3, 0, 7, 255, (1 << 62) + 5).struct()
    assert (s.plane, s.mode, s.radius, s.k, s.nms, s.margin, list(s.pad), s.threshold) == (2, 1, 3, 0, 7, 255, [0, 0], (1 << 62) + 5)
    assert (cr.MAX_RULES, cr.MAX_CAP, cr.MAX_RADIUS, cr.MAX_NMS, cr.HARRIS, cr.MIN_EIGEN) == (64, 1 << 20, 3, 7, 0, 1)
    assert cr.harris() == cr.Rule(0, 0, 1, 10, 3, 0, 1) and cr.min_eigen() == cr.Rule(0, 1, 1, 0, 3, 0, 1)
    header = open(os.path.join(fd.ROOT, "include", "hvqm4_amd.h")).read()
    for line in ("#define HVQ_CRN_MAX_RULES   64", "#define HVQ_CRN_MAX_CAP     (1 << 20)", "#define HVQ_CRN_MAX_RADIUS  3", "#define HVQ_CRN_MAX_NMS     7",
                 "#define HVQ_CRN_HARRIS      0", "#define HVQ_CRN_MIN_EIGEN   1",
                 "typedef struct HvqCornerRule { int32_t plane, mode, radius, k, nms, margin, pad[2]; int64_t threshold; } HvqCornerRule;",
                 "int64_t hvq_corner_rows_bytes(int width, int height, int h_samp, int v_samp, int plane);",
                 "int64_t hvq_corner_response_bytes(int width, int height, int h_samp, int v_samp, int plane);"):
        assert line in header, line
    for bad in (cr.Rule(3), cr.Rule(0, 2), cr.Rule(0, 0, 0), cr.Rule(0, 0, 4), cr.Rule(0, 0, 1, 65), cr.Rule(0, 1, 1, 10), cr.Rule(0, 0, 1, 10, 8),
                cr.Rule(0, 0, 1, 10, 3, 256), cr.Rule(0, 0, 1, 10, 3, 0, 0), cr.Rule(True), "rule"):
        with pytest.raises(ValueError):
            cr.check(bad)
    assert (cases.TX, cases.TY) == (64, 16)


_BAD_RULES = [(3, 0, 1, 10, 3, 0, (0, 0), 1), (-1, 0, 1, 10, 3, 0, (0, 0), 1), (0, 2, 1, 0, 3, 0, (0, 0), 1), (0, -1, 1, 0, 3, 0, (0, 0), 1), (0, 0, 0, 10, 3, 0, (0, 0), 1),
              (0, 0, 4, 10, 3, 0, (0, 0), 1), (0, 0, 1, 65, 3, 0, (0, 0), 1), (0, 0, 1, -1, 3, 0, (0, 0), 1), (0, 1, 1, 10, 3, 0, (0, 0), 1), (0, 0, 1, 10, 8, 0, (0, 0), 1),
              (0, 0, 1, 10, -1, 0, (0, 0), 1), (0, 0, 1, 10, 3, 256, (0, 0), 1), (0, 0, 1, 10, 3, -1, (0, 0), 1), (0, 0, 1, 10, 3, 0, (0, 0), 0), (0, 0, 1, 10, 3, 0, (0, 0), -7),
              (0, 0, 1, 10, 3, 0, (1, 0), 1), (0, 0, 1, 10, 3, 0, (0, 1), 1)]
_GOOD_RULES = [(0, 0, 1, 0, 0, 0, (0, 0), 1), (2, 0, 3, 64, 7, 255, (0, 0), 1 << 62), (1, 1, 3, 0, 7, 255, (0, 0), 1)]


def test_the_library_without_a_device_still_checks_its_arguments():
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, HvqCornerRule, lib
    one = (C.c_int * 1)(0)
    ptr = C.cast((C.c_void_p * 1)(16), C.c_void_p)
    r = cr.harris().struct()
    assert lib().hvq_corner_pictures(None, 1, one, one, None, C.byref(r), 1, None, ptr, ptr, ptr, None, 4, None) == HVQ_E_ARG
    assert lib().hvq_corner_check(None) == HVQ_E_ARG and lib().hvq_corner_check(C.byref(r)) == 0
    for bad in _BAD_RULES:
        assert lib().hvq_corner_check(C.byref(HvqCornerRule(*bad))) == HVQ_E_ARG, bad
    for good in _GOOD_RULES:
        assert lib().hvq_corner_check(C.byref(HvqCornerRule(*good))) == 0, good
    for geom in ((24, 16, 2, 2), (24, 16, 2, 1), (8, 8, 1, 1)):
        for p in range(3):
            _mask, _points, rows, response = cr.nbytes(geom, p)
            assert (lib().hvq_corner_rows_bytes(*geom, p), lib().hvq_corner_response_bytes(*geom, p)) == (rows, response)
    assert lib().hvq_corner_rows_bytes(24, 16, 2, 2, 3) == HVQ_E_ARG and lib().hvq_corner_response_bytes(24, 17, 2, 2, 0) < 0


# ------------------------------------------------------------------------------------------------- the fixture
_fixture_rules, fixture_record = cases.fixture_rules, cases.fixture_record


@pytest.mark.parametrize("name", sorted(FIXTURE["clips"]))
def test_fixture_equals_module(name):
    from hvqm4_amd.container import parse_header
    hdr = parse_header(open(os.path.join(fd.GOLDEN, fd.CLIPS[name]["file"]), "rb").read())
    geom = (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)
    pic = fd.oracle_pictures(name)[FIXTURE["picture"]].reshape(-1)
    rules = _fixture_rules()
    assert len(FIXTURE["clips"][name]) == len(rules) and FIXTURE["fields"] == ["K", "rows[Ny]", "crc32 points", "crc32 mask", "crc32 rows"]
    for r, want in zip(rules, FIXTURE["clips"][name]):
        assert fixture_record(pic, geom, r) == want, (name, r)
        assert want[0] == want[1]


def test_fixture_covers_the_three_samplings():
    assert sorted(FIXTURE["clips"]) == ["crossplane420_64x48", "crossplane444_48x64", "yuv422_296x160"]


# ------------------------------------------------------------------------------------------------- the runtime on the CPU fake device
@pytest.fixture(scope="module")
def drivers():
    return {kind: fd.build_driver(kind, "corner", "fake_corner_driver", CXX_SOURCES, __file__) for kind in fd.BUILDS}


def _inputs(scenario):
    """-> (cap, [(label, geom, picture, Rule, response)])"""
    if scenario == "cases":
        small = [(f"{name} {r}", (a.shape[1], a.shape[0], 1, 1), cases.picture((a.shape[1], a.shape[0], 1, 1), 0, a, i), r, i & 1)
                 for i, (name, a) in enumerate((n, cases.SMALL[n]) for n in ("blobs", "checker2")) for r in cases.RULES[i::2]
                 if a.shape[0] % 8 == 0 and a.shape[1] % 8 == 0]
        return 16, cases.device_cases() + small
    if scenario.startswith("cap"):
        g, pic, rule, K = cases.cap_case()
        return {"cap0": 0, "cap1": 1, "capK-1": K - 1, "capK": K, "capK+1": K + 1}[scenario], [("cap", g, pic, rule, 1)] + cases.narrow_cases()[:6]
    if scenario == "mixed":
        geoms, pics, rules, which = cases.mixed_cases()
        return 64, [(f"mixed {i}", g, p, rules[w], i % 3 == 0) for i, (g, p, w) in enumerate(zip(geoms, pics, which))]
    return 8, [("first", (8, 8, 2, 2), cases.picture((8, 8, 2, 2), 0, np.zeros((8, 8), np.uint8), 0), cr.harris(2, 10, nms=3), 0)]


def _run(exe, scenario, schedule, tmp_path):
    cap, items = _inputs(scenario)
    lines = [f"cap {cap}"]
    lines += [f"P {g[0]} {g[1]} {g[2]} {g[3]} {r.plane} {r.mode} {r.radius} {r.k} {r.nms} {r.margin} {r.threshold} {int(bool(q))}" for _l, g, _p, r, q in items]
    out, lines = fd.run_checked(exe, scenario if scenario in ("resident", "refused", "nogpu") else "cases", schedule, tmp_path,
                                inputs={"calls.txt": "\n".join(lines) + "\n", "pictures.bin": b"".join(p.tobytes() for _l, _g, p, _r, _q in items)})
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
    """mask.bin, points.bin, rows.bin and response.bin against the module, picture by picture"""
    masks = np.frombuffer((out / "mask.bin").read_bytes(), dtype=np.uint8)
    points = np.frombuffer((out / "points.bin").read_bytes(), dtype="<i8").reshape(len(items), cap + 1, 4)
    rows = np.frombuffer((out / "rows.bin").read_bytes(), dtype="<u4")
    resp = np.frombuffer((out / "response.bin").read_bytes(), dtype="<i8")
    filler = int.from_bytes(b"\xa5" * 8, "little", signed=True)
    mat = rat = qat = 0
    want_g = []
    for i, (label, geom, pic, r, q) in enumerate(items):
        mask, pts, idx = cr.of_picture(pic, geom, r, cap)
        assert np.array_equal(masks[mat:mat + mask.size], mask), f"{label}: {int((masks[mat:mat + mask.size] != mask).sum())} bytes of the mask differ"
        mat += mask.size
        assert np.array_equal(points[i, :pts.shape[0]], pts), f"{label}: the list differs: {points[i, :3].tolist()} for {pts[:3].tolist()}"
        assert (points[i, pts.shape[0]:] == filler).all(), f"{label}: a row beyond `stored` was written"
        assert np.array_equal(rows[rat:rat + idx.size], idx), f"{label}: the row index differs"
        rat += idx.size
        want_g += [("mask", i, 1), ("points", i, 1), ("rows", i, 1)]
        if q:
            R = cr.response_of_plane(cr.plane_of(pic, geom, r.plane), r)
            assert np.array_equal(resp[qat:qat + R.size].reshape(R.shape), R), f"{label}: the response map differs"
            qat += R.size
            want_g.append(("response", i, 1))
    assert (mat, rat, qat) == (masks.size, rows.size, resp.size)
    assert sorted(G) == sorted(want_g)


def _check_cases(cap, items, G, P, Rc, S, out):
    _compare(cap, items, G, out)
    assert Rc == {"cases/n0": 0}
    assert len({it[3] for it in items}) > 20 and {it[3].plane for it in items} == {0, 1, 2} and {it[3].mode for it in items} == {0, 1}
    assert {it[3].nms for it in items} >= {0, 1, 3, 7} and {it[3].radius for it in items} == {1, 2, 3}


def _check_cap(cap, items, G, P, Rc, S, out):
    K = cases.cap_case()[3]
    assert K >= 3 and cap in (0, 1, K - 1, K, K + 1)
    _compare(cap, items, G, out)


def _check_mixed(cap, items, G, P, Rc, S, out):
    assert len(items) == 60 and len({it[3] for it in items}) == 60
    _compare(cap, items, G, out)


def _check_resident(cap, items, G, P, Rc, S, out):
    r0 = items[0][3]
    assert len(P) == 18 and {f for _c, f, _k in P} == {"pic", "inv"}
    real = []
    for name, form, k in P:
        from hvqm4_amd.container import parse_header
        hdr = parse_header(open(os.path.join(fd.GOLDEN, fd.CLIPS[name]["file"]), "rb").read())
        pic = fd.oracle_pictures(name)[k].reshape(-1)
        real.append((f"{name} {form} {k}", (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp), pic if form == "pic" else 255 - pic,
                     cr.Rule(k % 3, r0.mode, r0.radius, r0.k, r0.nms, r0.margin, r0.threshold), form == "pic"))
    assert {g[2:] for _l, g, _p, _r, _q in real} == {(2, 2), (2, 1), (1, 1)}
    _compare(cap, real, G, out)


_CALL_REFUSED = ["null_context", "bad_stream", "bad_ordinal", "misaligned_src", "src_with_ordinal", "minus_one_without_src", "null_rules", "nrules_0", "nrules_65", "which_high",
                 "which_negative", "cap_negative", "cap_beyond", "null_masks", "null_mask", "misaligned_mask", "null_points", "null_point_list", "misaligned_point_list",
                 "null_rows", "null_row_index", "misaligned_row_index", "misaligned_response", "too_many", "negative_n", "check_null"]
_RULE_REFUSED = ["plane_3", "plane_negative", "mode_2", "mode_negative", "radius_0", "radius_4", "k_65", "k_negative", "k_under_min_eigen", "nms_8", "nms_negative",
                 "margin_256", "margin_negative", "threshold_0", "threshold_negative", "pad_0", "pad_1"]


def _check_refused(cap, items, G, P, Rc, S, out):
    from hvqm4_amd._lib import HVQ_E_ARG
    want = {k: HVQ_E_ARG for k in _CALL_REFUSED + _RULE_REFUSED + ["check_" + r for r in _RULE_REFUSED]}
    want.update({"check_good": 0, "then_ok": 0, "then_ok_without_response": 0})
    assert Rc == {"refused/" + k: v for k, v in want.items()}
    same, total = S["refused"]
    assert same == total == 2 * (64 * 48 * 2 + 32 * 9 + 4 * 64 + 8 * 64 * 48), "a refused call wrote an output"


def _check_nogpu(cap, items, G, P, Rc, S, out):
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_NOGPU
    assert Rc == {"nogpu/bad_rule": HVQ_E_ARG, "nogpu/bad_cap": HVQ_E_ARG, "nogpu/corners": HVQ_E_NOGPU, "nogpu/n0": 0}
    assert S["nogpu"][0] == S["nogpu"][1] > 0


CHECKS = {"cases": _check_cases, "cap0": _check_cap, "cap1": _check_cap, "capK-1": _check_cap, "capK": _check_cap, "capK+1": _check_cap, "mixed": _check_mixed,
          "resident": _check_resident, "refused": _check_refused}


@pytest.mark.parametrize("schedule", ["eager", "late"])
@pytest.mark.parametrize("build", list(fd.BUILDS))
@pytest.mark.parametrize("scenario", list(CHECKS))
def test_fake_device_scenario(drivers, scenario, build, schedule, tmp_path):
    CHECKS[scenario](*_run(drivers[build], scenario, schedule, tmp_path))


@pytest.mark.parametrize("schedule", ["eager", "late"])
def test_fake_device_without_the_corner_bodies_refuses(schedule, tmp_path):
    """a driver linked without fake_corner.cpp: the runtime's reference is weak, the call checks first and then says HVQ_E_NOGPU"""
    assert not any("fake_corner" in s for s in fd.CXX_SOURCES)
    exe = fd.build_driver("plain", "corner_nogpu", "fake_corner_driver", [s for s in CXX_SOURCES if not s.endswith("fake_corner.cpp")], __file__)
    _check_nogpu(*_run(exe, "nogpu", schedule, tmp_path))


# ------------------------------------------------------------------------------------------------- tools/bench_corners.py, tools/corners.py
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
    bench = _tool("bench_corners")
    reps = 3
    blocks = [[kernel] * (1 + reps) if isinstance(kernel, str) else list(kernel) * (1 + reps) for _label, kernel in bench.trace_plan()]
    if drop:
        blocks[-1] = blocks[-1][:-drop]
    gen.write_trace(str(tmp_path), blocks)
    return bench, bench.trace_summary(str(tmp_path), {"launches": 1 + reps, "pictures": 1024, "content": "natural"})


def test_bench_corners_imports_without_a_gpu_and_reads_a_synthetic_trace(tmp_path):
    bench, res = _bench_trace(tmp_path)
    assert "error" not in res, res
    for label, _kernel in bench.trace_plan():
        assert label in res, label
    row = res["harris_r1_nms3"]
    assert all(row[k]["launches"] == 3 for k in bench.CORNER_KERNELS), "the warm-up call is left out"
    assert row["list_median_us"] == round(sum(row[k]["median_us"] for k in bench.CORNER_KERNELS[1:]), 1)
    assert set(res["ratios"]) == {"tile_over_sobel_magnitude", "r3_over_r1", "nms7_over_nms0", "response_map_over_none", "list_launches_over_map_kernel"}


def test_bench_corners_refuses_a_trace_with_one_launch_too_few(tmp_path):
    _bench, res = _bench_trace(tmp_path, drop=1)
    assert list(res) == ["error"] and "planned" in res["error"]


def test_the_corner_tool_imports_without_a_gpu():
    tool = _tool("corners")
    assert tool.CAP == 4096 and callable(tool.clip_corners)
