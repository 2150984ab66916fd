"""CPU: picture metrics (hvq_picture_metrics, Context.picture_metrics, hvqm4_amd/metrics.py) without a GPU.

  - tests/metrics_ref.py, the numpy restatement the GPU tests compare with, against planes small enough to sum by hand, and the helpers;
  - the argument checks of Context.picture_metrics that need no device;
  - the runtime's entry point linked UNCHANGED against the CPU fake device of tests/test_fake_device.py (its source lists and flags, with
    tests/native/fake_metrics_driver.cpp in the place of fake_driver.cpp and tests/native/fake_metrics.cpp added: a scalar body for
    hvq_launch_metrics that reaches memory only through fake_span, when it runs), under both schedules, plain and as a stand-alone
    AddressSanitizer + UndefinedBehaviorSanitizer program.  The driver judges nothing: every record it read back is compared here with
    metrics_ref on the oracle's pictures.
"""
import math
import os

import numpy as np
import pytest

import tests.test_fake_device as fd
from tests.metrics_ref import adversarial_reference, metrics_reference, plane_sizes

NATIVE = fd.NATIVE
CXX_SOURCES = [s for s in fd.CXX_SOURCES if os.path.basename(s) != "fake_driver.cpp"] + \
              [os.path.join(NATIVE, "fake_metrics.cpp"), os.path.join(NATIVE, "fake_metrics_driver.cpp")]
SIX = ["gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8"]


# ------------------------------------------------------------------------------------------------- the reference and the helpers
def test_reference_on_planes_summed_by_hand():
    # 8 x 8, 4:2:0: Y 64 samples of 10 against 13; U 0..15 against zeros; V 255 against 0
    a = np.concatenate([np.full(64, 10), np.arange(16), np.full(16, 255)]).astype(np.uint8)
    b = np.concatenate([np.full(64, 13), np.zeros(16), np.zeros(16)]).astype(np.uint8)
    want = [[640, 832, 192, 576], [120, 0, 120, 1240], [4080, 0, 4080, 1040400]]
    got = metrics_reference(a, b, 8, 8, 2, 2)
    assert got.dtype == np.int64 and got.tolist() == want
    # b against a: the sums swap, the differences stay
    assert metrics_reference(b, a, 8, 8, 2, 2).tolist() == [[832, 640, 192, 576], [0, 120, 120, 1240], [0, 4080, 4080, 1040400]]
    # zeros form: sum_b = 0, sad = sum_a, sse = sum a^2
    assert metrics_reference(a, None, 8, 8, 2, 2).tolist() == [[640, 0, 640, 6400], [120, 0, 120, 1240], [4080, 0, 4080, 1040400]]
    # a picture against itself
    assert metrics_reference(a, a, 8, 8, 2, 2)[:, 2:].tolist() == [[0, 0]] * 3


def test_reference_plane_sizes_follow_the_sampling():
    assert plane_sizes(16, 8, 2, 2) == (128, 32, 32)
    assert plane_sizes(16, 8, 2, 1) == (128, 64, 64)
    assert plane_sizes(16, 8, 1, 1) == (128, 128, 128)
    # 16 x 8, 4:2:2: U is 8 x 8 = 64 samples right behind the 128 of Y
    a = np.zeros(256, dtype=np.uint8)
    a[128:192] = 3
    a[192:] = 5
    assert metrics_reference(a, None, 16, 8, 2, 1).tolist() == [[0, 0, 0, 0], [192, 0, 192, 576], [320, 0, 320, 1600]]


def test_reference_full_scale_plane_and_the_adversarial_picture():
    w, h = 640, 480
    a = np.full(w * h * 3 // 2, 255, dtype=np.uint8)
    m = metrics_reference(a, None, w, h, 2, 2)
    assert m[0].tolist() == [w * h * 255, 0, w * h * 255, w * h * 65025] and m[0, 3] == 19975680000 > 2 ** 32
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, w * h * 3 // 2, dtype=np.uint8)
    b = adversarial_reference(a)
    assert (np.abs(a.astype(int) - b.astype(int)) >= 128).all()
    m = metrics_reference(a, b, w, h, 2, 2)
    assert m[0, 3] >= w * h * 128 * 128 == 5033164800 and m[0, 3] > 2 ** 32          # no 32-bit total holds it
    assert m[0, 2] >= w * h * 128
    # in int64 python arithmetic, sample by sample, on a slice small enough to loop over
    sl = slice(1000, 1400)
    assert metrics_reference(np.concatenate([a[sl], a[sl][:200]]), np.concatenate([b[sl], b[sl][:200]]), 20, 20, 2, 2)[0, 3] == \
        sum((int(x) - int(y)) ** 2 for x, y in zip(a[sl], b[sl]))


def test_helpers():
    import torch
    from hvqm4_amd import metrics
    assert metrics.plane_samples(640, 480, 2, 2) == (307200, 76800, 76800)
    assert metrics.plane_samples(640, 480, 2, 1) == (307200, 153600, 153600)
    assert metrics.plane_samples(24, 40, 1, 1) == (960, 960, 960)
    with pytest.raises(ValueError):
        metrics.plane_samples(640, 480, 3, 1)
    samples = metrics.plane_samples(8, 8, 2, 2)
    m = torch.tensor([[[640, 832, 192, 576], [120, 0, 120, 0], [4080, 0, 4080, 16]]], dtype=torch.int64)
    p = metrics.psnr(m, samples)
    assert p.dtype == torch.float64 and tuple(p.shape) == (1, 3)
    assert p[0, 0].item() == pytest.approx(10 * math.log10(65025 * 64 / 576), rel=1e-12)
    assert math.isinf(p[0, 1].item()) and p[0, 1].item() > 0
    assert p[0, 2].item() == pytest.approx(10 * math.log10(65025.0), rel=1e-12)              # sse == samples: mse 1
    d = metrics.mean_abs_diff(m, samples)
    assert d.dtype == torch.float64 and d[0].tolist() == [3.0, 7.5, 255.0]
    # against zeros: a plane of 10s; a plane half 0, half 2; a plane of 255s
    z = torch.tensor([[640, 0, 640, 6400], [16, 0, 16, 32], [4080, 0, 4080, 1040400]], dtype=torch.int64)
    mean, var = metrics.mean_var(z, samples)
    assert mean.tolist() == [10.0, 1.0, 255.0] and var.tolist() == [0.0, 1.0, 0.0]
    with pytest.raises(ValueError):
        metrics.psnr(torch.zeros((3, 3), dtype=torch.int64), samples)
    # values beyond 2^32 keep their digits
    big = torch.tensor([[0, 0, 0, 19975680000], [0, 0, 0, 1], [0, 0, 0, 1]], dtype=torch.int64)
    assert metrics.psnr(big, metrics.plane_samples(640, 480)).tolist()[0] == 0.0


# ------------------------------------------------------------------------------------------------- argument checks without a device
class _NoDevice:
    """what Context.picture_metrics looks at before it reaches the library"""
    _geom = {0: (64, 48), 1: (24, 40)}
    _h = None

    @staticmethod
    def pic_bytes(sid):
        return {0: 64 * 48 * 3 // 2, 1: 24 * 40 * 3 // 2}[sid]


def test_references_are_checked_before_the_library_is_called():
    import torch
    from hvqm4_amd._lib import HVQ_E_ARG, HvqError
    from hvqm4_amd.batch import Context
    from hvqm4_amd.metrics import references
    call = lambda *a, **k: Context.picture_metrics(_NoDevice(), *a, **k)
    with pytest.raises(ValueError, match="ordinals"):
        call([0, 0], [0])
    with pytest.raises(HvqError) as e:
        call([0, 7], [0, 0])
    assert e.value.code == HVQ_E_ARG
    with pytest.raises(ValueError, match="1 references for 2 pictures"):
        call([0, 0], [0, 1], ref=[None])
    with pytest.raises(TypeError):
        call([0], [0], ref="zeros")
    with pytest.raises(TypeError):
        call([0], [0], ref=[(0, 1, 2)])
    with pytest.raises(TypeError):
        call([0], [0], ref=[(0, 1.5)])
    with pytest.raises(ValueError):
        call([0], [0], ref=[(-1, 0)])
    with pytest.raises(TypeError):
        call([0], [0], ref=[3])
    good = torch.zeros(64 * 48 * 3 // 2, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        call([0], [0], ref=[good.to(torch.int8)])
    with pytest.raises(ValueError, match="elements"):
        call([1], [0], ref=[good])                                        # the bytes of stream 0's pictures for one of stream 1
    with pytest.raises(ValueError, match="contiguous"):
        call([0], [0], ref=[torch.zeros(64 * 48 * 3, dtype=torch.uint8)[::2]])
    room = torch.zeros(64 * 48 * 3 // 2 + 64, dtype=torch.uint8)
    off = (-room.data_ptr()) % 16
    with pytest.raises(ValueError, match="multiple of 16"):
        call([0], [0], ref=[room[off + 8:off + 8 + good.numel()]])
    with pytest.raises(ValueError, match="not a GPU"):                    # the device is checked last
        call([0], [0], ref=[room[off:off + good.numel()]])
    with pytest.raises(ValueError, match="out must be"):
        call([0], [0], out=torch.zeros((1, 3, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="out must be"):
        call([0], [0], out=torch.zeros((2, 3, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match="not a GPU"):
        call([0], [0], out=torch.zeros((1, 3, 4), dtype=torch.int64))
    # what the well-formed forms become
    assert references(None, 3, _NoDevice.pic_bytes) is None
    assert references([None, (1, 2), [0, 5]], 3, _NoDevice.pic_bytes) == [(-1, 0, None), (1, 2, None), (0, 5, None)]


def test_the_library_without_a_device_still_checks_its_arguments():
    """no context can exist here, and the call says so before it looks at anything else"""
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, lib
    one = (C.c_int * 1)(0)
    assert lib().hvq_picture_metrics(None, 1, one, one, None, None, None) == HVQ_E_ARG


# ------------------------------------------------------------------------------------------------- the runtime on the CPU fake device
@pytest.fixture(scope="module")
def drivers():
    return {kind: fd.build_driver(kind, "metrics", "fake_metrics_driver", CXX_SOURCES, __file__) for kind in fd.BUILDS}


def _geometry(name):
    from hvqm4_amd.container import parse_header
    hdr = parse_header(open(os.path.join(fd.GOLDEN, fd.CLIPS[name]["file"]), "rb").read())
    return hdr.width, hdr.height, hdr.h_samp, hdr.v_samp


_want = {}


def _expected(clip_a, ka, form, clip_b, kb):
    key = (clip_a, ka, form, clip_b, kb)
    if key not in _want:
        a = fd.oracle_pictures(clip_a)[ka]
        b = None if form == "zeros" else fd.oracle_pictures(clip_b)[kb]
        if form == "inv":
            b = 255 - b
        _want[key] = metrics_reference(a, b, *_geometry(clip_a))
    return _want[key]


def _run(exe, scenario, schedule, tmp_path):
    _, lines = fd.run_checked(exe, scenario, schedule, tmp_path)
    M, R, S = {}, {}, {}
    for line in lines:
        f = line.split()
        if f[0] == "M":
            label, clip_a, ka, form, clip_b, kb = f[1], f[2], int(f[3]), f[4], f[5], int(f[6])
            got = np.array([int(v) for v in f[7:]], dtype=np.uint64).astype(np.int64).reshape(3, 4)
            want = _expected(clip_a, ka, form, clip_b, kb)
            assert np.array_equal(got, want), f"{label}: picture {ka} of {clip_a} against {form} {clip_b} {kb}:\n{got}\nwant\n{want}"
            M.setdefault(label, []).append((clip_a, ka, form, clip_b, kb))
        elif f[0] == "R":
            R[f[1]] = int(f[2])
        elif f[0] == "S":
            S[f[1]] = (int(f[2]), int(f[3]))
    return M, R, S, fd.refusal_texts(lines)


def _check_goldens(M, R, S, E):
    n = {nm: fd.n_pics(nm) for nm in SIX}
    assert len({_geometry(nm)[2:] for nm in SIX}) == 3                    # 4:2:0, 4:2:2 and 4:4:4
    assert sorted(M["goldens/clip"]) == sorted(
        [(nm, k, "pic", nm, k - 1) for nm in SIX for k in range(1, n[nm])] + [(nm, k, "pic", nm, k) for nm in SIX for k in range(n[nm])] +
        [(nm, k, "zeros", "-", 0) for nm in SIX for k in range(n[nm])])
    assert sorted(M["goldens/nullref"]) == sorted((nm, k, "zeros", "-", 0) for nm in SIX for k in range(n[nm]))
    mixed = M["goldens/mixed"]
    assert [m[0] for m in mixed] == SIX + SIX, "records come back in call order"
    assert [m[2] for m in mixed] == ["pic", "zeros", "pic"] * 4
    assert M["goldens/one"] == [("yuv422_296x160", 1, "pic", "yuv422_296x160", 0)]


def _check_memory(M, R, S, E):
    na = fd.n_pics("yuv422_64x48")
    for label in ("memory", "memory/nullstream"):
        assert sorted(M[label]) == sorted(
            [("yuv422_64x48", k, "inv", "yuv422_64x48", k - 1 if k else 0) for k in range(na)] +
            [("yuv422_64x48", k, "pic", "yuv422_64x48", k) for k in range(na)] +
            [("ragged24x40", 1, "inv", "ragged24x40", 0), ("ragged24x40", 1, "zeros", "-", 0)])


def _check_reuse(M, R, S, E):
    from hvqm4_amd._lib import HVQ_E_STATE
    n, ne = fd.n_pics("gop64x48_15"), fd.n_pics("yuv444_64x48")
    assert sorted(M["reuse"]) == sorted([("gop64x48_15", k, "pic", "gop64x48_15", (k + 1) % n) for k in range(n)] +
                                        [("gop64x48_15", k, "zeros", "-", 0) for k in range(n)])
    assert R["reuse/evicted"] == HVQ_E_STATE, "the flushes did not hand the slots of the first pass on: the scenario tests nothing"
    assert M["reuse/late"] == [("gop64x48_15", k, "pic", "gop64x48_15", k - 1 if k else 0) for k in range(n)]
    assert M["reuse/destroy"] == [("yuv444_64x48", k, "zeros", "-", 0) for k in range(ne)]


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
    "refused/ref_stream_below_minus_one": "reference 1: stream -2 (a stream, or -1 for the caller's memory or zeros)",
    "refused/null_out": "out must be a non-null multiple of 8",
    "refused/misaligned_out": "out must be a non-null multiple of 8",
    "refused/too_many": "65536 pictures: one call takes 65535 at the most (one grid row each)",
    "refused/evicted": "stream 2 picture 0 is no longer resident (slot reused, or the picture was dropped)",
    "refused/evicted_ref": "stream 2 picture 0 is no longer resident (slot reused, or the picture was dropped)",
    "refused/queued": "stream 0 picture 7 is queued but not flushed",
}


def _check_refused(M, R, S, E):
    for label, text in REFUSAL_TEXTS.items():
        assert E.get(label) == text, (label, E.get(label))
    assert set(E) == set(REFUSAL_TEXTS)
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_STATE
    want = {"geometry": HVQ_E_ARG, "ptr_with_stream": HVQ_E_ARG, "misaligned_ptr": HVQ_E_ARG, "bad_stream": HVQ_E_ARG, "bad_ordinal": HVQ_E_ARG,
            "bad_ref_stream": HVQ_E_ARG, "bad_ref_ordinal": HVQ_E_ARG, "ref_stream_below_minus_one": HVQ_E_ARG, "null_out": HVQ_E_ARG,
            "misaligned_out": HVQ_E_ARG, "too_many": HVQ_E_ARG, "evicted": HVQ_E_STATE, "evicted_ref": HVQ_E_STATE, "queued": HVQ_E_STATE}
    assert R == {"refused/" + k: v for k, v in want.items()}
    same, total = S["refused"]
    assert same == total == 2 * 96 + 8, "a refused call wrote its output"
    assert M["refused/then_ok"] == [("gop64x48_15", 1, "pic", "gop64x48_15", 0), ("gop64x48_15", fd.n_pics("gop64x48_15") - 1, "zeros", "-", 0)]


CHECKS = {"goldens": _check_goldens, "memory": _check_memory, "reuse": _check_reuse, "refused": _check_refused}


@pytest.mark.parametrize("schedule", ["eager", "late"])
@pytest.mark.parametrize("build", list(fd.BUILDS))
@pytest.mark.parametrize("scenario", list(CHECKS))
def test_fake_device_scenario(drivers, scenario, build, schedule, tmp_path):
    CHECKS[scenario](*_run(drivers[build], scenario, schedule, tmp_path))


def test_the_existing_fake_build_links_without_the_metrics_body():
    """tests/test_fake_device.py's source list has no hvq_launch_metrics: the runtime's reference to it is weak"""
    assert not any("fake_metrics" in s for s in fd.CXX_SOURCES)
    text = open(os.path.join(fd.CSRC, "hvq_runtime.cpp")).read()
    decl = [l for l in text.splitlines() if "hvq_launch_metrics(" in l and l.startswith("extern")]
    assert len(decl) == 1 and "weak" in decl[0]
