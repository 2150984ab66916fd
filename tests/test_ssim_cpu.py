"""CPU: windowed SSIM (hvq_picture_ssim, hvq_ssim_windows, Context.picture_ssim, hvqm4_amd/metrics.py) without a GPU.

  - tests/ssim_ref.py, the numpy restatement the GPU tests compare with, against windows small enough to work out by hand, and the helpers;
  - hvq_ssim_windows against metrics.ssim_windows; the argument checks of Context.picture_ssim that need no device;
  - the runtime's entry point linked UNCHANGED against the CPU fake device of tests/test_fake_device.py (its source lists and flags, with
    tests/native/fake_ssim_driver.cpp in the place of fake_driver.cpp and tests/native/fake_ssim.cpp added: a scalar body for
    hvq_launch_ssim that reaches memory only through fake_span, when it runs), under both schedules, plain and as a stand-alone
    AddressSanitizer + UndefinedBehaviorSanitizer program.  The driver judges nothing: every record and map it read back is compared here
    with ssim_ref on the oracle's pictures, bit for bit.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import tests.test_fake_device as fd
from tests.ssim_ref import SSIM_ONE, checkerboard, flat_maps, ssim_plane, ssim_reference, window_dims

NATIVE = fd.NATIVE
CXX_SOURCES = [s for s in fd.CXX_SOURCES if os.path.basename(s) != "fake_driver.cpp"] + \
              [os.path.join(NATIVE, "fake_ssim.cpp"), os.path.join(NATIVE, "fake_ssim_driver.cpp")]
SEVEN = ["gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8", "i16"]
ONE_BITS = np.float32(1.0).view(np.uint32)


# ------------------------------------------------------------------------------------------------- the reference, by hand
def test_reference_on_a_window_worked_out_by_hand():
    # 8 x 8, 4:2:0: Y all 10 against Y all 13: one luma window, no chroma window
    a = np.concatenate([np.full(64, 10), np.arange(16), np.full(16, 255)]).astype(np.uint8)
    b = np.concatenate([np.full(64, 13), np.zeros(16), np.zeros(16)]).astype(np.uint8)
    s1, s2, ss, s12 = 640, 832, 17216, 8320
    assert (s1, s2, ss, s12) == (64 * 10, 64 * 13, 64 * (100 + 169), 64 * 130)
    assert 64 * ss - s1 * s1 - s2 * s2 == 0 and 64 * s12 - s1 * s2 == 0                      # vars = covar = 0
    A, B, Cc, D = 2 * s1 * s2 + 416, 235963, s1 * s1 + s2 * s2 + 416, 235963
    assert (A, Cc) == (1065376, 1102240)
    q = (np.float32(A) * np.float32(B)) / (np.float32(Cc) * np.float32(D))
    assert q.dtype == np.float32
    rec, maps = ssim_reference(a, b, 8, 8, 2, 2)
    assert rec.dtype == np.int64 and rec.tolist() == [[int(np.rint(q * np.float32(SSIM_ONE))), 1], [0, 0], [0, 0]]
    assert [m.shape for m in maps] == [(1, 1), (0, 0), (0, 0)] and maps[0].dtype == np.float32
    assert maps[0].view(np.uint32)[0, 0] == q.view(np.uint32)
    assert abs(float(q) - 1065376 / 1102240) < 1e-7


def test_reference_identical_pictures_are_exactly_one():
    rng = np.random.default_rng(3)
    for w, h, hs, vs in ((64, 48, 2, 2), (24, 40, 2, 1), (48, 64, 1, 1)):
        n = w * h + 2 * (w >> (hs == 2)) * (h >> (vs == 2))
        a = rng.integers(0, 256, n, dtype=np.uint8)
        rec, maps = ssim_reference(a, a, w, h, hs, vs)
        dims = window_dims(w, h, hs, vs)
        assert rec.tolist() == [[r * c * SSIM_ONE, r * c] for r, c in dims]
        for m, d in zip(maps, dims):
            assert m.shape == d and (m.view(np.uint32) == ONE_BITS).all()


def test_reference_extremes():
    full, zero = np.full((16, 24), 255, np.uint8), np.zeros((16, 24), np.uint8)
    q, f = ssim_plane(full, zero)
    assert f.shape == (3, 5) and (f == 26).all()                                  # the tiny-q end: 416 * 235963 / (C D)
    board = checkerboard(24, 16, 1, 1)[:24 * 16].reshape(16, 24)
    q, f = ssim_plane(board, 255 - board)
    assert (f == -16717867).all() and (q < 0).all()                               # negative covar
    q, f = ssim_plane(full, full)
    assert (f == SSIM_ONE).all()                                                  # A = C = 532 685 216
    assert 2 * 16320 * 16320 + 416 == 532685216 < 2 ** 30


def test_reference_mean_equals_the_float64_mean():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (96, 128), dtype=np.uint8)
    b = np.clip(a.astype(int) + rng.integers(-8, 9, a.shape), 0, 255).astype(np.uint8)
    q, f = ssim_plane(a, b)
    assert f.sum() / (SSIM_ONE * f.size) == pytest.approx(q.astype(np.float64).mean(), abs=2.0 ** -25)


# ------------------------------------------------------------------------------------------------- geometry and helpers
def test_window_counts_of_the_library_and_of_python_agree():
    from hvqm4_amd import metrics
    from hvqm4_amd._lib import HVQ_E_GEOMETRY, lib
    for w, h in ((8, 8), (16, 16), (24, 40), (296, 160), (640, 480)):
        for hs, vs in ((2, 2), (2, 1), (1, 1)):
            dims = (C.c_int32 * 6)(*[-1] * 6)
            total = lib().hvq_ssim_windows(w, h, hs, vs, dims)
            got = tuple((dims[2 * p], dims[2 * p + 1]) for p in range(3))
            assert got == metrics.ssim_windows(w, h, hs, vs) == window_dims(w, h, hs, vs), (w, h, hs, vs)
            assert total == sum(r * c for r, c in got) == lib().hvq_ssim_windows(w, h, hs, vs, None)
    assert metrics.ssim_windows(8, 8, 2, 2) == ((1, 1), (0, 0), (0, 0))
    assert metrics.ssim_windows(8, 8, 2, 1) == ((1, 1), (1, 0), (1, 0))
    assert metrics.ssim_windows(640, 480, 2, 2) == ((119, 159), (59, 79), (59, 79))
    assert metrics.ssim_windows(640, 480) == metrics.ssim_windows(640, 480, 2, 2)
    assert metrics.ssim_windows(24, 40, 2, 2) == ((9, 5), (4, 2), (4, 2))
    for bad in ((100, 100, 2, 2), (640, 480, 1, 2), (0, 8, 2, 2), (16384, 8, 2, 2)):
        assert lib().hvq_ssim_windows(*bad, None) == HVQ_E_GEOMETRY, bad
    with pytest.raises(ValueError):
        metrics.ssim_windows(640, 480, 3, 1)


def test_helpers():
    import torch
    from hvqm4_amd import metrics
    assert metrics.SSIM_ONE == SSIM_ONE == 16777216
    rec = torch.tensor([[[SSIM_ONE, 1], [0, 0], [0, 0]],
                        [[3 * SSIM_ONE // 2, 2], [SSIM_ONE // 2, 1], [-SSIM_ONE // 4, 1]]], dtype=torch.int64)
    s = metrics.ssim(rec)
    assert s.dtype == torch.float64 and tuple(s.shape) == (2, 3)
    assert s[0, 0].item() == 1.0 and math.isnan(s[0, 1].item()) and math.isnan(s[0, 2].item())
    assert s[1].tolist() == [0.75, 0.5, -0.25]
    samples = metrics.plane_samples(8, 8, 2, 2)
    al = metrics.ssim_all(rec, samples)
    assert al.dtype == torch.float64 and tuple(al.shape) == (2,)
    assert al[0].item() == 1.0                                                   # the planes without a window are left out of both sums
    assert al[1].item() == pytest.approx((0.75 * 64 + 0.5 * 16 - 0.25 * 16) / 96, rel=1e-15)
    db = metrics.ssim_db(torch.tensor([1.0, 0.9, 0.0], dtype=torch.float64))
    assert math.isinf(db[0].item()) and db[0].item() > 0
    assert db[1].item() == pytest.approx(10.0, rel=1e-12) and db[2].item() == 0.0
    assert metrics.ssim_db(0.99).item() == pytest.approx(20.0, rel=1e-12)
    with pytest.raises(ValueError):
        metrics.ssim(torch.zeros((3, 4), dtype=torch.int64))
    # from a record of the reference
    a = np.random.default_rng(9).integers(0, 256, 64 * 48 * 3 // 2, dtype=np.uint8)
    r, maps = ssim_reference(a, 255 - a, 64, 48, 2, 2)
    got = metrics.ssim(torch.from_numpy(r))
    for p in range(3):
        assert got[p].item() == pytest.approx(maps[p].astype(np.float64).mean(), abs=2.0 ** -25)


# ------------------------------------------------------------------------------------------------- argument checks without a device
class _NoDevice:
    """what Context.picture_ssim looks at before it reaches the library"""
    _geom = {0: (64, 48), 1: (24, 40)}
    _h = None

    @staticmethod
    def pic_bytes(sid):
        return {0: 64 * 48 * 3 // 2, 1: 24 * 40 * 3 // 2}[sid]


def test_arguments_are_checked_before_the_library_is_called():
    import torch
    from hvqm4_amd._lib import HVQ_E_ARG, HvqError
    from hvqm4_amd.batch import Context
    call = lambda *a, **k: Context.picture_ssim(_NoDevice(), *a, **k)
    with pytest.raises(ValueError, match="ordinals"):
        call([0, 0], [0], [(0, 0)])
    with pytest.raises(HvqError) as e:
        call([0, 7], [0, 0], [(0, 0), (0, 0)])
    assert e.value.code == HVQ_E_ARG
    with pytest.raises(ValueError, match="needs a reference"):
        call([0], [0], None)
    with pytest.raises(TypeError):
        call([0], [0])                                                    # ref is required
    with pytest.raises(ValueError, match="reference 1 is None"):
        call([0, 0], [0, 1], [(0, 1), None])
    with pytest.raises(ValueError, match="1 references for 2 pictures"):
        call([0, 0], [0, 1], [(0, 0)])
    with pytest.raises(TypeError):
        call([0], [0], [(0, 1.5)])
    good = torch.zeros(64 * 48 * 3 // 2, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        call([0], [0], [good.to(torch.int8)])
    with pytest.raises(ValueError, match="elements"):
        call([1], [0], [good])
    room = torch.zeros(64 * 48 * 3 // 2 + 64, dtype=torch.uint8)
    off = (-room.data_ptr()) % 16
    with pytest.raises(ValueError, match="multiple of 16"):
        call([0], [0], [room[off + 8:off + 8 + good.numel()]])
    with pytest.raises(ValueError, match="not a GPU"):                    # the device is checked last
        call([0], [0], [room[off:off + good.numel()]])
    with pytest.raises(ValueError, match="out must be"):
        call([0], [0], [(0, 1)], out=torch.zeros((1, 3, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match="out must be"):
        call([0], [0], [(0, 1)], out=torch.zeros((1, 3, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match="not a GPU"):
        call([0], [0], [(0, 1)], out=torch.zeros((1, 3, 2), dtype=torch.int64))


def test_the_library_without_a_device_still_checks_its_arguments():
    from hvqm4_amd._lib import HVQ_E_ARG, lib
    one = (C.c_int * 1)(0)
    assert lib().hvq_picture_ssim(None, 1, one, one, None, None, None, None) == HVQ_E_ARG


def test_the_launch_is_a_weak_reference():
    """the source lists of tests/test_fake_device.py and tests/test_metrics_cpu.py have no hvq_launch_ssim: those builds must link"""
    assert not any("fake_ssim" in s for s in fd.CXX_SOURCES)
    text = open(os.path.join(fd.CSRC, "hvq_runtime.cpp")).read()
    decl = [l for l in text.splitlines() if "hvq_launch_ssim(" in l and l.startswith("extern")]
    assert len(decl) == 1 and "weak" in decl[0]


# ------------------------------------------------------------------------------------------------- the runtime on the CPU fake device
@pytest.fixture(scope="module")
def drivers():
    return {kind: fd.build_driver(kind, "ssim", "fake_ssim_driver", CXX_SOURCES, __file__) for kind in fd.BUILDS}


def _geometry(name):
    from hvqm4_amd.container import parse_header
    hdr = parse_header(open(os.path.join(fd.GOLDEN, fd.CLIPS[name]["file"]), "rb").read())
    return hdr.width, hdr.height, hdr.h_samp, hdr.v_samp


_want = {}


def _expected(clip_a, ka, form, clip_b, kb):
    key = (clip_a, ka, form, clip_b, kb)
    if key not in _want:
        a, b = fd.oracle_pictures(clip_a)[ka], fd.oracle_pictures(clip_b)[kb]
        if form == "inv":
            b = 255 - b
        rec, maps = ssim_reference(a, b, *_geometry(clip_a))
        _want[key] = (rec, flat_maps(maps).view(np.uint32))
    return _want[key]


def _run(exe, scenario, schedule, tmp_path):
    _, lines = fd.run_checked(exe, scenario, schedule, tmp_path)
    W, Q, R, S = {}, {}, {}, {}
    for line in lines:
        f = line.split()
        if f[0] in "WQ":
            label, key = f[1], (f[2], int(f[3]), f[4], f[5], int(f[6]))
            want_rec, want_map = _expected(*key)
            if f[0] == "W":
                got = np.array([int(v) for v in f[7:]], dtype=np.int64).reshape(3, 2)
                assert np.array_equal(got, want_rec), f"{label}: picture {key[1]} of {key[0]} against {key[2]} {key[3]} {key[4]}:\n{got}\nwant\n{want_rec}"
                W.setdefault(label, []).append(key)
            else:
                intact, guard, n = int(f[7]), int(f[8]), int(f[9])
                assert intact == guard > 0, f"{label}: {key}: the call wrote behind the map"
                got = np.array([int(v, 16) for v in f[10:]], dtype=np.uint32)
                assert n == got.size == want_map.size, (label, key, n, got.size, want_map.size)
                assert np.array_equal(got, want_map), f"{label}: {key}: {(got != want_map).sum()} of {n} map elements differ"
                Q.setdefault(label, []).append(key)
        elif f[0] == "R":
            R[f[1]] = int(f[2])
        elif f[0] == "S":
            S[f[1]] = (int(f[2]), int(f[3]))
    return W, Q, R, S, fd.refusal_texts(lines)


def _check_goldens(W, Q, R, S, E):
    n = {nm: fd.n_pics(nm) for nm in SEVEN}
    assert len({_geometry(nm)[2:] for nm in SEVEN}) == 3                   # 4:2:0, 4:2:2 and 4:4:4
    assert _geometry("ip8")[:2] == (8, 8) and _geometry("i16")[:2] == (16, 16)
    pairs = sorted([(nm, k, "pic", nm, k - 1) for nm in SEVEN for k in range(1, n[nm])] + [(nm, k, "pic", nm, k) for nm in SEVEN for k in range(n[nm])] +
                   [(nm, k, "inv", nm, k) for nm in SEVEN for k in range(n[nm])])
    assert sorted(W["goldens/maps"]) == sorted(Q["goldens/maps"]) == sorted(W["goldens/nomaps"]) == pairs
    assert "goldens/nomaps" not in Q
    mixed = W["goldens/mixed"]
    assert [m[0] for m in mixed] == SEVEN + SEVEN, "records come back in call order"
    assert [m[2] for m in mixed] == (["pic", "inv", "pic"] * 5)[:14]
    assert Q["goldens/mixed"] == mixed[1::2], "a map for every other pair"
    assert W["goldens/one"] == Q["goldens/one"] == [("yuv422_296x160", 1, "pic", "yuv422_296x160", 0)]
    # identical pictures: exactly one in every window
    for nm in SEVEN:
        rec, m = _expected(nm, 0, "pic", nm, 0)
        assert (rec[:, 0] == rec[:, 1] * SSIM_ONE).all() and (m == ONE_BITS).all()


def _check_reuse(W, Q, R, S, E):
    from hvqm4_amd._lib import HVQ_E_STATE
    n, ne = fd.n_pics("gop64x48_15"), fd.n_pics("yuv444_64x48")
    assert W["reuse"] == [("gop64x48_15", k, "pic", "gop64x48_15", (k + 1) % n) for k in range(n)]
    assert Q["reuse"] == W["reuse"][0::2]
    assert R["reuse/evicted"] == HVQ_E_STATE, "the flushes did not hand the slots of the first pass on: the scenario tests nothing"
    assert W["reuse/late"] == Q["reuse/late"] == [("gop64x48_15", k, "pic", "gop64x48_15", k - 1 if k else 0) for k in range(n)]
    assert W["reuse/destroy"] == Q["reuse/destroy"] == [("yuv444_64x48", k, "pic", "yuv444_64x48", k - 1 if k else 0) for k in range(ne)]


# what hvq_last_error_string() said after each call of `refused`, recorded from the runtime before the record frame: the
# order of the checks and their words are part of the interface.  A call that succeeds leaves the words of the refusal before it.
REFUSAL_TEXTS = {
    "refused/geometry": "reference 1: stream 1 (64 x 48, chroma shifts 1, 0) has not the geometry of stream 0 (64 x 48, 1, 1)",
    "refused/ptr_with_stream": "reference 1: a pointer together with stream 0 (a resident reference takes no pointer)",
    "refused/misaligned_ptr": "reference 1: the pointer must be a multiple of 16",
    "refused/bad_stream": "bad stream 99",
    "refused/bad_ordinal": "stream 0: bad picture ordinal 1000",
    "refused/bad_ref_stream": "bad stream 99",
    "refused/bad_ref_ordinal": "stream 0: bad picture ordinal -1",
    "refused/ref_stream_below_minus_one": "reference 1: stream -2 (a stream, or -1 for the caller's memory)",
    "refused/null_ref": "SSIM needs a reference for every picture (ref is NULL)",
    "refused/zeros_ref": "reference 1: SSIM against a picture of zeros means nothing (stream -1 needs a pointer)",
    "refused/null_out": "out must be a non-null multiple of 8",
    "refused/misaligned_out": "out must be a non-null multiple of 8",
    "refused/misaligned_map": "map 1: the pointer must be a multiple of 4",
    "refused/too_many": "65536 pictures: one call takes 65535 at the most (one grid row each)",
    "refused/evicted": "stream 2 picture 0 is no longer resident (slot reused, or the picture was dropped)",
    "refused/evicted_ref": "stream 2 picture 0 is no longer resident (slot reused, or the picture was dropped)",
    "refused/queued": "stream 0 picture 7 is queued but not flushed",
    "refused/null_context": "bad arguments",
}


def _check_refused(W, Q, R, S, E):
    for label, text in REFUSAL_TEXTS.items():
        assert E.get(label) == text, (label, E.get(label))
    assert set(E) == set(REFUSAL_TEXTS)
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_STATE
    want = {k: HVQ_E_ARG for k in ("geometry", "ptr_with_stream", "misaligned_ptr", "bad_stream", "bad_ordinal", "bad_ref_stream", "bad_ref_ordinal",
                                   "ref_stream_below_minus_one", "null_ref", "zeros_ref", "null_out", "misaligned_out", "misaligned_map", "too_many",
                                   "null_context")}
    want.update({k: HVQ_E_STATE for k in ("evicted", "evicted_ref", "queued")})
    assert R == {"refused/" + k: v for k, v in want.items()}
    same, total = S["refused"]
    windows = sum(r * c for r, c in window_dims(*_geometry("gop64x48_15")))
    assert same == total == (8 + 2 * 48 + 8) + 2 * (windows + 2) * 4, "a refused call wrote its output or a map"
    last = fd.n_pics("gop64x48_15") - 1
    assert W["refused/then_ok"] == [("gop64x48_15", 1, "pic", "gop64x48_15", 0), ("gop64x48_15", last, "pic", "gop64x48_15", last)]
    assert Q["refused/then_ok"] == W["refused/then_ok"][:1]


CHECKS = {"goldens": _check_goldens, "reuse": _check_reuse, "refused": _check_refused}


@pytest.mark.parametrize("schedule", ["eager", "late"])
@pytest.mark.parametrize("build", list(fd.BUILDS))
@pytest.mark.parametrize("scenario", list(CHECKS))
def test_fake_device_scenario(drivers, scenario, build, schedule, tmp_path):
    CHECKS[scenario](*_run(drivers[build], scenario, schedule, tmp_path))
