"""CPU: the values of hvq_integral_pictures, hvq_window_pictures and hvq_rect_sums.  tests/integral_ref.py restates include/hvqm4_amd.h in
plain Python (every sample of every window visited, math.isqrt for the deviation); hvqm4_amd.integral (numpy's cumsum in uint64, then
masked), scipy where it is installed (a float route, compared away from the rounding boundaries), the fixture
tests/golden/integral.json and the runtime on the CPU fake device (tests/native/fake_integral.cpp, which walks the launches' grids lane
by lane with the functions of hvq_integral.h) are compared with it by ==.  The fake-device driver is a stand-alone program, built and
run plain and with ASan + UBSan as tests/test_distance_cpu.py builds its own; nothing is preloaded and no Python is involved in the
sanitised run."""
import json
import os
import zlib

import numpy as np
import pytest

import tests.test_fake_device as fd
from hvqm4_amd import integral as I
from hvqm4_amd import labels as L
from tests import integral_cases as cases
from tests import integral_ref as ref

NATIVE = fd.NATIVE
CXX_SOURCES = [s for s in fd.CXX_SOURCES if os.path.basename(s) != "fake_driver.cpp"] + \
              [os.path.join(NATIVE, "fake_integral.cpp"), os.path.join(NATIVE, "fake_integral_driver.cpp")]
FIXTURE = json.load(open(os.path.join(fd.GOLDEN, "integral.json")))


# ------------------------------------------------------------------------------------------------- module against reference
def test_module_equals_the_brute_force_on_the_small_planes():
    cs = cases.window_cases(cases.BRUTE_PLANES[:1], every=True) + cases.window_cases(cases.BRUTE_PLANES[1:])
    assert {(c[3].mode, c[3].k, c[3].c, c[3].invert) for c in cs} == set(cases.SPECS) and {(c[3].rx, c[3].ry) for c in cs} == set(cases.WINDOWS)
    for label, geom, pic, r in cs:
        plane = L.plane_of(pic, geom, r.plane)
        got = I.of_window(plane, r)
        assert got.dtype == np.uint8 and got.shape == plane.shape, label
        assert got.tolist() == ref.window(plane.tolist(), r.mode, r.rx, r.ry, r.k, r.c, r.invert), label
        want = I.of_picture(pic, geom, r)
        assert want.size == cases.nbytes(geom) and np.array_equal(want[:plane.size].reshape(plane.shape), got) and (want[plane.size:] == 128).all(), label


def test_tables_equal_the_slow_sums_and_the_recurrence():
    for label, geom, pic, plane in cases.table_cases(cases.TABLE_PLANES[:3]) + cases.table_cases([((24, 16, 2, 1), 0)]):
        a = L.plane_of(pic, geom, plane)
        S, Q = I.of_plane(a)
        assert S.dtype == np.uint32 and Q.dtype == np.uint64 and S.shape == Q.shape == a.shape, label
        slow = ref.tables(a.tolist())
        assert (S.tolist(), Q.tolist()) == slow and ref.tables_by_rows(a.tolist()) == slow, label
        assert I.of_plane(a, squares=False)[1] is None
    for label, geom, pic, plane in cases.table_cases()[::7]:
        a = L.plane_of(pic, geom, plane)
        S, Q = I.of_plane(a)
        assert (S.tolist(), Q.tolist()) == ref.tables_by_rows(a.tolist()), label


def test_rectangles_equal_the_visited_samples():
    geoms, pics, planes, rects = cases.rect_cases()
    assert rects.shape == (300, 5)
    planes_ = [L.plane_of(p, g, pl) for p, g, pl in zip(pics, geoms, planes)]
    tables = [I.of_plane(a, squares=i != len(pics) - 1) for i, a in enumerate(planes_)]
    got = I.of_rects(rects, tables)
    refused = 0
    for r, (i, x0, y0, x1, y1) in enumerate(rects.tolist()):
        want = ref.rect(planes_[i].tolist(), x0, y0, x1, y1) if 0 <= i < len(pics) else (0, 0, 0)
        if tables[i][1] is None if 0 <= i < len(pics) else False:
            want = (want[0], want[1], 0)
        assert tuple(int(v) for v in got[r]) == want, rects[r]
        refused += want[0] == 0
    assert refused == 10
    P = I.padded(tables[0][0])
    assert P.shape == (tables[0][0].shape[0] + 1, tables[0][0].shape[1] + 1) and not P[0].any() and not P[:, 0].any() and np.array_equal(P[1:, 1:], tables[0][0])


def test_against_scipy_away_from_the_rounding_boundaries():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(4)
    total = left_out = 0
    for ny, nx in ((40, 136), (24, 72), (64, 48)):
        a = rng.integers(0, 256, (ny, nx), dtype=np.uint8)
        for rx, ry in ((1, 1), (7, 3), (25, 25), (0, 5)):
            size = (2 * ry + 1, 2 * rx + 1)
            s = ndi.uniform_filter(a.astype(np.float64), size=size, mode="constant")
            n = ndi.uniform_filter(np.ones_like(a, dtype=np.float64), size=size, mode="constant")
            exact = s / n                                            # the zero padding scales both alike: the mean over the cut window
            keep = np.abs(exact + 0.5 - np.rint(exact + 0.5)) > 1e-6
            got = I.of_window(a, I.mean((rx, ry)))
            assert np.array_equal(got[keep], np.floor(exact + 0.5)[keep].astype(np.uint8)), (ny, nx, rx, ry)
            total += a.size
            left_out += int((~keep).sum())
    assert left_out <= total // 100, (left_out, total)


def test_known_answers():
    for v in (0, 1, 128, 255):
        a = np.full((16, 24), v, np.uint8)
        assert (I.of_window(a, I.mean((7, 3))) == v).all() and not I.of_window(a, I.deviation(5)).any()
        for c in (-255, -3, 0):
            assert not I.of_window(a, I.adaptive(9, c=c)).any() and (I.of_window(a, I.adaptive(9, c=c, invert=True)) == 255).all()
        for c in (1, 7, 255):
            assert (I.of_window(a, I.adaptive(9, c=c)) == 255).all()
    yy, xx = np.mgrid[0:16, 0:24]
    check = (((xx + yy) & 1) * 255).astype(np.uint8)
    d = I.of_window(check, I.deviation((1, 2)))
    n = ((np.minimum(xx + 1, 23) - np.maximum(xx - 1, 0) + 1) * (np.minimum(yy + 2, 15) - np.maximum(yy - 2, 0) + 1))
    assert (n % 2 == 0).any() and (n % 2 == 1).any() and (d[n % 2 == 0] == 127).all() and (d[n % 2 == 1] <= 127).all()
    a = np.random.default_rng(2).integers(0, 256, (16, 24), dtype=np.uint8)
    whole = (2 * int(a.sum()) + a.size) // (2 * a.size)
    for r in ((24, 16), (23, 15), (8191, 8191), (100, 4000)):
        assert (I.of_window(a, I.mean(r)) == whole).all(), r
    assert I.adaptive(25, c=7) == I.Rule(0, I.THRESHOLD, 25, 25, 0, 7, 0) and I.mean((7, 3), plane=2) == I.Rule(2, I.MEAN, 7, 3) and I.deviation(4) == I.rule("deviation", 4)
    assert not I.needs_squares(I.adaptive(25, c=7)) and I.needs_squares(I.adaptive(25, k=-1)) and I.needs_squares(I.deviation(1)) and not I.needs_squares(I.mean(1))
    for bad in (I.Rule(3), I.Rule(-1), I.Rule(0, 3), I.Rule(0, -1), I.Rule(0, 0, 8192), I.Rule(0, 0, 0, 8192), I.Rule(0, 0, -1), I.Rule(0, 2, 1, 1, 1025), I.Rule(0, 2, 1, 1, -1025),
                I.Rule(0, 2, 1, 1, 0, 256), I.Rule(0, 2, 1, 1, 0, -256), I.Rule(0, 2, 1, 1, 0, 0, 2), I.Rule(0, 2, 1, 1, 0, 0, True), I.Rule(0, True)):
        with pytest.raises(ValueError):
            I.check(bad)
    with pytest.raises(ValueError):
        I.rule("median", 3)
    with pytest.raises(ValueError):
        I.of_picture(np.zeros(cases.nbytes((24, 16, 2, 2)), np.uint8), (24, 16, 2, 2), I.mean(1, plane=1))


def test_the_table_wraps_and_the_rectangle_stays_exact():
    """8192 x 2064 of 255 in the module (about two seconds of numpy); the fake device runs this plane only in the plain build, see
    test_fake_device_wrap"""
    a = np.full((2064, 8192), 255, np.uint8)
    S, Q = I.of_plane(a)
    assert 255 * 8192 * 2064 == 4311613440 and int(S[-1, -1]) == 4311613440 % 2 ** 32 == 16646144 and int(Q[-1, -1]) == 255 * 255 * 8192 * 2064
    assert (2057 - 10 + 1) * (8191 - 100 + 1) == 16572416 <= I.MAX_AREA
    assert I.rect(S, Q, 100, 10, 8191, 2057) == (16572416, 255 * 16572416, 255 * 255 * 16572416)
    assert I.rect(S, Q, 0, 0, 8191, 2063) == (0, 0, 0) and I.rect(S, Q, 0, 0, 8191, 2047) == (1 << 24, 255 << 24, 255 * 255 << 24)
    assert I.rect(S.view(np.int32), None, 100, 10, 8191, 2057) == (16572416, 255 * 16572416, 0)


def test_struct_layout():
    import ctypes as C
    from hvqm4_amd._lib import HvqWindowRule
    assert C.sizeof(HvqWindowRule) == 32
    assert [(n, getattr(HvqWindowRule, n).offset) for n, _t in HvqWindowRule._fields_] == [("plane", 0), ("mode", 4), ("rx", 8), ("ry", 12), ("k", 16), ("c", 20), ("invert", 24), ("pad", 28)]
    s = I.Rule(2, 2, 40, 3, -51, 7, 1).struct()
    assert (s.plane, s.mode, s.rx, s.ry, s.k, s.c, s.invert, s.pad) == (2, 2, 40, 3, -51, 7, 1, 0)
    assert (I.MAX_RULES, I.MAX_RADIUS, I.MAX_AREA, I.MAX_RECTS, I.MODES) == (64, 8191, 1 << 24, 1 << 24, ("mean", "deviation", "threshold"))
    header = open(os.path.join(fd.ROOT, "include", "hvqm4_amd.h")).read()
    for line in ("#define HVQ_WIN_MEAN      0", "#define HVQ_WIN_DEVIATION 1", "#define HVQ_WIN_THRESHOLD 2", "#define HVQ_WIN_MAX_RULES 64", "#define HVQ_WIN_MAX_RADIUS 8191",
                 "#define HVQ_RECT_MAX (1 << 24)", "typedef struct HvqWindowRule { int32_t plane, mode, rx, ry, k, c, invert, pad; } HvqWindowRule;",
                 "int64_t hvq_integral_bytes(int width, int height, int h_samp, int v_samp, int plane, int order);"):
        assert line in header, line
    assert (cases.WAVE, cases.WAVES, cases.CHUNK, cases.COLS, cases.TX, cases.TY) == (64, 4, 256, 256, 64, 16)
    assert f"HVQ_IG_CHUNK = {cases.CHUNK} samples" in header


def test_the_library_without_a_device_still_checks_its_arguments():
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, HvqWindowRule, lib
    one = (C.c_int * 1)(0)
    ptr = (C.c_void_p * 1)(16)
    p = C.cast(ptr, C.c_void_p)
    r = I.mean(3).struct()
    assert lib().hvq_integral_pictures(None, 1, one, one, None, None, p, None, None) == HVQ_E_ARG
    assert lib().hvq_window_pictures(None, 1, one, one, None, p, None, C.byref(r), 1, None, p, None) == HVQ_E_ARG
    assert lib().hvq_rect_sums(None, 1, 1, p, p, None, p, p, None) == HVQ_E_ARG
    assert lib().hvq_window_check(None) == HVQ_E_ARG and lib().hvq_window_check(C.byref(r)) == 0
    for bad in ((3, 0, 1, 1, 0, 0, 0, 0), (-1, 0, 1, 1, 0, 0, 0, 0), (0, 3, 1, 1, 0, 0, 0, 0), (0, -1, 1, 1, 0, 0, 0, 0), (0, 0, 8192, 1, 0, 0, 0, 0), (0, 0, 1, 8192, 0, 0, 0, 0),
                (0, 0, -1, 1, 0, 0, 0, 0), (0, 2, 1, 1, 1025, 0, 0, 0), (0, 2, 1, 1, -1025, 0, 0, 0), (0, 2, 1, 1, 0, 256, 0, 0), (0, 2, 1, 1, 0, -256, 0, 0), (0, 2, 1, 1, 0, 0, 2, 0),
                (0, 2, 1, 1, 0, 0, -1, 0), (0, 0, 1, 1, 0, 0, 0, 1)):
        assert lib().hvq_window_check(C.byref(HvqWindowRule(*bad))) == HVQ_E_ARG, bad
    for good in ((0, 0, 0, 0, 0, 0, 0, 0), (2, 2, 8191, 8191, 1024, 255, 1, 0), (1, 1, 5, 0, -1024, -255, 0, 0), (0, 0, 3, 3, 51, 7, 1, 0)):
        assert lib().hvq_window_check(C.byref(HvqWindowRule(*good))) == 0, good
    for geom in ((24, 16, 2, 2), (24, 16, 2, 1), (8, 8, 1, 1)):
        for pl in range(3):
            for order in (1, 2):
                assert lib().hvq_integral_bytes(*geom, pl, order) == I.nbytes(geom, pl, order)
    assert lib().hvq_integral_bytes(24, 16, 2, 2, 3, 1) == HVQ_E_ARG and lib().hvq_integral_bytes(24, 16, 2, 2, 0, 3) == HVQ_E_ARG
    assert lib().hvq_integral_bytes(24, 16, 2, 2, 0, 0) == HVQ_E_ARG and lib().hvq_integral_bytes(24, 17, 2, 2, 0, 1) < 0
    with pytest.raises(ValueError):
        I.nbytes((24, 16, 2, 2), 0, 3)


def test_rects_of_boxes():
    comps = [np.zeros((4, 8), np.int64), np.zeros((4, 8), np.int64)]
    comps[0][0, :2] = (2, 2)
    comps[0][1, :5] = (6, 1, 2, 3, 3)
    comps[0][2, :5] = (1, 7, 7, 7, 7)
    comps[0][3, :5] = (9, 9, 9, 9, 9)                                # stale: beyond `stored`
    comps[1][0, :2] = (5, 3)                                         # more components than rows
    comps[1][1:, 1:5] = [(0, 0, 1, 1), (2, 2, 2, 2), (3, 0, 3, 5)]
    got = I.rects_of_boxes(comps)
    assert got.dtype == np.int32 and got.tolist() == [[0, 1, 2, 3, 3], [0, 7, 7, 7, 7], [0, 0, 0, -1, -1], [1, 0, 0, 1, 1], [1, 2, 2, 2, 2], [1, 3, 0, 3, 5]]
    torch = pytest.importorskip("torch")
    assert I.rects_of_boxes([torch.from_numpy(c) for c in comps]).tolist() == got.tolist()


# ------------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("name", sorted(FIXTURE["clips"]))
def test_fixture_equals_module(name):
    from hvqm4_amd.container import parse_header
    hdr = parse_header(open(os.path.join(fd.GOLDEN, fd.CLIPS[name]["file"]), "rb").read())
    geom = (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)
    pic = fd.oracle_pictures(name)[0].reshape(-1)
    want = FIXTURE["clips"][name]
    S, Q = I.of_plane(L.plane_of(pic, geom, 0))
    assert zlib.crc32(S.astype("<u4").tobytes()) == want["sums"] and zlib.crc32(Q.astype("<u8").tobytes()) == want["squares"], name
    for key, (mode, rx, ry, k, c, inv) in FIXTURE["windows"].items():
        assert zlib.crc32(I.of_picture(pic, geom, I.Rule(0, mode, rx, ry, k, c, inv)).tobytes()) == want[key], (name, key)


def test_fixture_covers_every_golden_clip():
    assert sorted(FIXTURE["clips"]) == sorted(fd.CLIPS)
    assert sorted(FIXTURE["windows"]) == ["adaptive_5_c7_k51", "deviation_2", "mean_7_3"]


# ------------------------------------------------------------------------------------------------- the runtime on the CPU fake device
@pytest.fixture(scope="module")
def drivers():
    return {kind: fd.build_driver(kind, "integral", "fake_integral_driver", CXX_SOURCES, __file__) for kind in fd.BUILDS}


def _inputs(scenario):
    """-> ([(label, geom, picture, plane, squares, Rule or None)], rects int32 [k][5])"""
    none = np.zeros((0, 5), np.int32)
    if scenario == "cases":
        tabs = cases.table_cases() + cases.wide_cases()
        items = [(lb, g, p, pl, int(i % 3 != 2), None) for i, (lb, g, p, pl) in enumerate(tabs)]
        items += [(lb, g, p, r.plane, 1 if I.needs_squares(r) or i % 4 == 0 else 0, r) for i, (lb, g, p, r) in enumerate(cases.window_cases()[::3])]
        return items, none
    if scenario == "mixed":
        geoms, pics, rules, which = cases.mixed_cases()
        return [(f"mixed {i}", g, p, 0, 1, rules[w]) for i, (g, p, w) in enumerate(zip(geoms, pics, which))], none
    if scenario == "rects":
        geoms, pics, planes, rects = cases.rect_cases()
        return [(f"rects {i}", g, p, pl, int(i != len(pics) - 1), None) for i, (g, p, pl) in enumerate(zip(geoms, pics, planes))], rects
    if scenario == "wrap":
        return [("wrap", cases.WRAP, np.full(cases.nbytes(cases.WRAP), 255, np.uint8), 0, 1, None)], np.array([(0, 100, 10, 8191, 2057), (0, 0, 0, 8191, 2063), (0, 0, 0, 8191, 2047),
                                                                                                              (1, 0, 0, 1, 1)], dtype=np.int32)
    rects = np.array([(i, x0, y0, 40, 40 + i) for i in range(18) for x0, y0 in ((0, 0), (3, 5))] + [(18, 0, 0, 1, 1)], dtype=np.int32)
    return [("first", (8, 8, 2, 2), np.zeros(cases.nbytes((8, 8, 2, 2)), np.uint8), 0, 1, I.adaptive((7, 3), c=7, k=51))], rects


def _run(exe, scenario, schedule, tmp_path, timeout=600):
    items, rects = _inputs(scenario)
    lines = []
    for _l, g, _p, plane, sq, r in items:
        r_ = r or I.Rule(plane)
        lines.append(f"P {g[0]} {g[1]} {g[2]} {g[3]} {plane} {sq} {int(r is not None)} {r_.mode} {r_.rx} {r_.ry} {r_.k} {r_.c} {r_.invert}")
    lines += ["R " + " ".join(str(v) for v in row) for row in rects.tolist()]
    out, lines = fd.run_checked(exe, scenario if scenario in ("resident", "refused", "nogpu") else "cases", schedule, tmp_path, timeout=timeout,
                                inputs={"calls.txt": "\n".join(lines) + "\n", "pictures.bin": b"".join(it[2].tobytes() for it in items)})
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
    return items, rects, G, P, Rc, S, out


def _compare(items, rects, G, out, tables=True):
    """sums.bin, squares.bin, window.bin and rects.bin against the module, picture by picture"""
    sums = np.fromfile(out / "sums.bin", dtype="<u4")
    squares = np.fromfile(out / "squares.bin", dtype="<u8")
    window = np.fromfile(out / "window.bin", dtype=np.uint8)
    at = qat = wat = nq = nw = 0
    made = []
    for label, geom, pic, plane, sq, r in items:
        a = L.plane_of(pic, geom, plane)
        S, Q = I.of_plane(a, squares=bool(sq))
        made.append((S, Q))
        assert np.array_equal(sums[at:at + S.size].reshape(S.shape), S), f"{label}: the table of sums differs"
        at += S.size
        if sq:
            assert np.array_equal(squares[qat:qat + Q.size].reshape(Q.shape), Q), f"{label}: the table of squares differs"
            qat += Q.size
            nq += 1
        if r is not None:
            want = I.of_picture(pic, geom, r)
            got = window[wat:wat + want.size]
            assert np.array_equal(got, want), f"{label}: {int((got != want).sum())} bytes differ"
            wat += want.size
            nw += 1
    assert at == sums.size and qat == squares.size and wat == window.size
    wantG = [("sums", i, 1) for i in range(len(items))] + [("squares", i, 1) for i in range(nq)] + [("window", i, 1) for i in range(nw)]
    if len(rects):
        got = np.fromfile(out / "rects.bin", dtype="<u8").reshape(-1, 3)
        assert np.array_equal(got, I.of_rects(rects, made)), "the rectangles differ"
        wantG.append(("rects", 0, 1))
    assert sorted(G) == sorted(wantG)
    return made


def _check_cases(items, rects, G, P, Rc, S, out):
    _compare(items, rects, G, out)
    assert Rc == {"cases/n0": 0, "cases/window_n0": 0, "cases/rects_0": 0}
    rules = [it[5] for it in items if it[5] is not None]
    assert {(r.mode, r.k, r.c, r.invert) for r in rules} == set(cases.SPECS) and {(r.rx, r.ry) for r in rules} == set(cases.WINDOWS)
    assert {it[3] for it in items} == {0, 1, 2} and {it[4] for it in items} == {0, 1}


def _check_mixed(items, rects, G, P, Rc, S, out):
    assert len(items) == 60 and len({it[5] for it in items}) == 60
    _compare(items, rects, G, out)


def _check_rects(items, rects, G, P, Rc, S, out):
    assert len(rects) == 300
    _compare(items, rects, G, out)


def _check_resident(items, rects, G, P, Rc, S, out):
    r0 = items[0][5]
    assert len(P) == 18 and {f for _c, f, _k in P} == {"pic", "inv"}
    real = []
    for name, form, k in P:
        from hvqm4_amd.container import parse_header
        hdr = parse_header(open(os.path.join(fd.GOLDEN, fd.CLIPS[name]["file"]), "rb").read())
        pic = fd.oracle_pictures(name)[k].reshape(-1)
        plane = k % 3 if hdr.h_samp == 1 else 0
        real.append((f"{name} {form} {k}", (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp), pic if form == "pic" else 255 - pic, plane, 1,
                     I.Rule(plane, r0.mode, r0.rx, r0.ry, r0.k, r0.c, r0.invert)))
    assert {g[2:] for _l, g, _p, _pl, _s, _r in real} == {(2, 2), (2, 1), (1, 1)} and {it[3] for it in real} == {0, 1, 2}
    _compare(real, rects, G, out)


_INTEGRAL_REFUSED = ["null_context", "bad_stream", "bad_ordinal", "misaligned_src", "src_with_ordinal", "minus_one_without_src", "plane_3", "plane_negative", "null_sums",
                     "null_table", "misaligned_table", "misaligned_squares", "too_many", "negative_n"]
_WINDOW_REFUSED = ["w_null_context", "w_bad_stream", "w_bad_ordinal", "w_misaligned_src", "w_null_sums", "w_null_table", "w_misaligned_table", "w_misaligned_squares",
                   "w_squares_needed", "w_squares_needed_one", "w_null_rules", "w_nrules_0", "w_nrules_65", "w_which_high", "w_which_negative", "w_null_dst", "w_null_destination",
                   "w_misaligned_destination", "w_too_many", "w_negative_n", "w_plane_not_of_y_size", "check_null"]
_RULE_REFUSED = ["r_plane_3", "r_plane_negative", "r_mode_3", "r_mode_negative", "r_rx_8192", "r_ry_8192", "r_rx_negative", "r_ry_negative", "r_k_1025", "r_k_low", "r_c_256",
                 "r_c_low", "r_invert_2", "r_invert_negative", "r_pad"]
_RECT_REFUSED = ["c_null_context", "c_n_0", "c_too_many", "c_negative_nrects", "c_too_many_rects", "c_null_rects", "c_misaligned_rects", "c_null_dims", "c_misaligned_dims",
                 "c_null_out", "c_misaligned_out", "c_null_sums", "c_null_table", "c_misaligned_table", "c_misaligned_squares"]


def _check_refused(items, rects, G, P, Rc, S, out):
    from hvqm4_amd._lib import HVQ_E_ARG
    want = {k: HVQ_E_ARG for k in _INTEGRAL_REFUSED + _WINDOW_REFUSED + _RULE_REFUSED + ["check_" + r for r in _RULE_REFUSED] + _RECT_REFUSED}
    want.update({"check_good": 0, "check_widest": 0, "then_ok": 0, "then_window_ok": 0, "then_window_without_squares_ok": 0, "then_rects_ok": 0})
    assert Rc == {"refused/" + k: v for k, v in want.items()}
    same, total = S["refused"]
    assert same == total == 2 * (12 * 64 * 48 + 64 * 48 * 2) + 96, "a refused call wrote an output"


def _check_nogpu(items, rects, G, P, Rc, S, out):
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_NOGPU
    assert Rc == {"nogpu/integral_bad_plane": HVQ_E_ARG, "nogpu/integral": HVQ_E_NOGPU, "nogpu/window_bad_rule": HVQ_E_ARG, "nogpu/window": HVQ_E_NOGPU,
                  "nogpu/rects_bad_out": HVQ_E_ARG, "nogpu/rects": HVQ_E_NOGPU, "nogpu/n0": 0}
    assert S["nogpu"][0] == S["nogpu"][1] > 0


CHECKS = {"cases": _check_cases, "mixed": _check_mixed, "rects": _check_rects, "resident": _check_resident, "refused": _check_refused}


@pytest.mark.parametrize("schedule", ["eager", "late"])
@pytest.mark.parametrize("build", list(fd.BUILDS))
@pytest.mark.parametrize("scenario", list(CHECKS))
def test_fake_device_scenario(drivers, scenario, build, schedule, tmp_path):
    CHECKS[scenario](*_run(drivers[build], scenario, schedule, tmp_path))


def test_fake_device_wrap(drivers, tmp_path):
    """the 8192 x 2064 plane of 255 on the fake device: in the plain build only, and under one schedule -- the sanitised build walks its
    17 million samples for a minute.  The table wraps, the rectangle of 16 572 416 samples stays exact, the whole plane is refused"""
    items, rects, G, _P, _Rc, _S, out = _run(drivers["plain"], "wrap", "eager", tmp_path)
    sums = np.fromfile(out / "sums.bin", dtype="<u4")
    squares = np.fromfile(out / "squares.bin", dtype="<u8")
    got = np.fromfile(out / "rects.bin", dtype="<u8").reshape(-1, 3)
    assert int(sums[-1]) == 16646144 and int(squares[-1]) == 255 * 255 * 8192 * 2064
    assert got.tolist() == [[16572416, 255 * 16572416, 255 * 255 * 16572416], [0, 0, 0], [1 << 24, 255 << 24, 255 * 255 << 24], [0, 0, 0]]
    xs = np.arange(1, 8193, dtype=np.uint64)
    for y in (0, 1, 1031, 2063):
        assert np.array_equal(sums[y * 8192:(y + 1) * 8192], ((xs * np.uint64(255 * (y + 1))) & np.uint64(0xFFFFFFFF)).astype(np.uint32)), y
    assert sorted(G) == [("rects", 0, 1), ("squares", 0, 1), ("sums", 0, 1)]


@pytest.mark.parametrize("schedule", ["eager", "late"])
def test_fake_device_without_the_integral_bodies_refuses(schedule, tmp_path):
    """a driver linked without fake_integral.cpp: the runtime's references are weak, the calls check first and then say HVQ_E_NOGPU"""
    assert not any("fake_integral" in s for s in fd.CXX_SOURCES)
    exe = fd.build_driver("plain", "integral_nogpu", "fake_integral_driver", [s for s in CXX_SOURCES if not s.endswith("fake_integral.cpp")], __file__)
    _check_nogpu(*_run(exe, "nogpu", schedule, tmp_path))


# ------------------------------------------------------------------------------------------------- tools/bench_integral.py, tools/adaptive.py
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
    bench = _tool("bench_integral")
    reps = 3
    blocks = [[k] * (1 + reps) if n == 1 + reps else [k] * n for _label, k, n in bench.trace_plan(reps)]
    if drop:
        blocks[-1] = blocks[-1][:-drop]
    gen.write_trace(str(tmp_path), blocks)
    return bench, bench.trace_summary(str(tmp_path), {"launches": 1 + reps, "pictures": 1024})


def test_bench_integral_imports_without_a_gpu_and_reads_a_synthetic_trace(tmp_path):
    bench, res = _bench_trace(tmp_path)
    assert "error" not in res, res
    assert set(res["kernels"]) == set(bench.INTEGRAL_KERNELS) | {bench.WINDOW_KERNEL, bench.RECT_KERNEL}
    per_byte = res["scale_identity"]["median_us"] / 3.0                  # the identity kernel moves 1.5 bytes in and 1.5 out a luma sample
    assert res["yardstick_us"] == {"sums": round(13 * per_byte, 1), "sums_and_squares": round(39 * per_byte, 1)}
    for label in ("integral_sums", "integral_both"):
        row = res[label]
        assert all(row[k]["launches"] == 3 for k in bench.INTEGRAL_KERNELS), "the warm-up call is left out"
        assert row["sum_median_us"] == round(sum(row[k]["median_us"] for k in bench.INTEGRAL_KERNELS), 1)
    for label in bench.WINDOW_ROWS:
        assert res[label]["launches"] == 3
    c2 = res["condition_2"]
    assert c2["integral_plus_mean15_us"] == round(res["integral_sums"]["sum_median_us"] + res["mean_15"]["median_us"], 1) and c2["holds"] == (c2["integral_plus_mean15_us"] < c2["gauss15_us"])


def test_bench_integral_refuses_a_trace_with_one_launch_too_few(tmp_path):
    _bench, res = _bench_trace(tmp_path, drop=1)
    assert list(res) == ["error"] and "planned" in res["error"]


def test_adaptive_imports_without_a_gpu():
    tool = _tool("adaptive")
    assert callable(tool.clip_adaptive)
