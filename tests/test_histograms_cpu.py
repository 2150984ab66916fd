"""CPU: picture histograms (hvq_picture_histograms, Context.picture_histograms, hvqm4_amd/histograms.py) without a GPU.

  - tests/histograms_ref.py, the host restatement the GPU tests compare with, on a picture worked out by hand;
  - every helper of hvqm4_amd.histograms against a direct numpy computation on the expanded samples;
  - the identities the header states (sum of the bins = samples, sum v h = sum_a, sum d h = sad, sum d^2 h = sse) against
    tests/metrics_ref.py on the oracle's pictures of every golden clip;
  - the argument checks of Context.picture_histograms that need no device; the constants of histograms.py against hvq_desc.h;
  - the runtime's entry point linked UNCHANGED against the CPU fake device of tests/test_fake_device.py (its source lists and flags, with
    tests/native/fake_histograms_driver.cpp in the place of fake_driver.cpp and tests/native/fake_histograms.cpp added: a scalar body for
    hvq_launch_histograms that reaches memory only through fake_span, when it runs), under both schedules, plain and as a stand-alone
    AddressSanitizer + UndefinedBehaviorSanitizer program.  The driver judges nothing: every record it read back is compared here with
    histograms_ref on the oracle's pictures.
"""
import os
import re

import numpy as np
import pytest

import tests.test_fake_device as fd
from tests.histograms_ref import histogram_reference
from tests.metrics_ref import metrics_reference, plane_sizes

NATIVE = fd.NATIVE
CXX_SOURCES = [s for s in fd.CXX_SOURCES if os.path.basename(s) != "fake_driver.cpp"] + \
              [os.path.join(NATIVE, "fake_histograms.cpp"), os.path.join(NATIVE, "fake_histograms_driver.cpp")]
SIX = ["gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8"]


# ------------------------------------------------------------------------------------------------- the reference and the helpers
def test_reference_on_a_picture_worked_out_by_hand():
    # 8 x 8, 4:2:0: Y 60 samples of 1 and 4 of 200; U 16 samples of 0; V 0, 0, ..., 0, 255
    a = np.concatenate([np.full(60, 1), np.full(4, 200), np.zeros(16), np.zeros(15), [255]]).astype(np.uint8)
    got = histogram_reference(a, None, 8, 8, 2, 2)
    assert got.dtype == np.int64 and got.shape == (3, 256)
    want = np.zeros((3, 256), dtype=np.int64)
    want[0, 1], want[0, 200], want[1, 0], want[2, 0], want[2, 255] = 60, 4, 16, 15, 1
    assert (got == want).all()
    # against b: Y all 3 (|1 - 3| = 2 sixty times, |200 - 3| = 197 four times); U 0 against 255; V equal to a's
    b = np.concatenate([np.full(64, 3), np.full(16, 255), a[80:]]).astype(np.uint8)
    want = np.zeros((3, 256), dtype=np.int64)
    want[0, 2], want[0, 197], want[1, 255], want[2, 0] = 60, 4, 16, 16
    assert (histogram_reference(a, b, 8, 8, 2, 2) == want).all()
    assert (histogram_reference(b, a, 8, 8, 2, 2) == want).all(), "|a - b| is symmetric"
    # 4:2:2: U starts right behind Y and is half of it
    c = np.zeros(256, dtype=np.uint8)
    c[128] = 7
    r = histogram_reference(c, None, 16, 8, 2, 1)
    assert r[0, 0] == 128 and r[1, 0] == 63 and r[1, 7] == 1 and r[2, 0] == 64 and r.sum() == 256
    from hvqm4_amd import histograms as hg
    assert (hg.of_picture(a, 8, 8) == histogram_reference(a, None, 8, 8, 2, 2)).all()
    assert (hg.of_picture(a.tobytes(), 8, 8, 2, 2, ref=b.tobytes()) == histogram_reference(a, b, 8, 8, 2, 2)).all()
    with pytest.raises(ValueError):
        hg.of_picture(a[:-1], 8, 8)
    with pytest.raises(ValueError):
        hg.of_picture(a, 8, 8, ref=b[:-1])


def _sample_sets():
    """expanded samples the helpers are checked on: odd and even counts, a single value, two values, a bimodal and a uniform set"""
    rng = np.random.default_rng(5)
    sets = [np.array([7], dtype=np.int64), np.array([0, 255], dtype=np.int64), np.full(12, 200, dtype=np.int64),
            rng.integers(0, 256, 1001), rng.integers(0, 256, 640),
            np.concatenate([rng.normal(60, 10, 700), rng.normal(180, 15, 300)]).clip(0, 255).astype(np.int64),
            np.concatenate([np.full(5, 3), np.full(5, 9)]).astype(np.int64),
            rng.integers(100, 104, 77), np.arange(256).repeat(3)]
    return [np.sort(s.astype(np.int64)) for s in sets]


def test_helpers_against_numpy_on_the_expanded_samples():
    from hvqm4_amd import histograms as hg
    sets = _sample_sets()
    H = np.stack([np.bincount(s, minlength=256) for s in sets]).astype(np.int32)       # the tensor's dtype
    assert hg.BINS == 256 and (hg.HIST_VALUES, hg.HIST_ABSDIFF) == (0, 1)
    assert hg.samples(H).tolist() == [s.size for s in sets]
    assert np.allclose(hg.mean(H), [s.mean() for s in sets], rtol=1e-14, atol=0)
    assert np.allclose(hg.variance(H), [s.var() for s in sets], rtol=1e-11, atol=1e-12)
    lo, hi = hg.min_max(H)
    assert lo.tolist() == [s.min() for s in sets] and hi.tolist() == [s.max() for s in sets]
    assert np.array_equal(hg.median(H), np.array([np.median(s) for s in sets]))
    # the rank rule k = max(1, ceil(q N / 100)) is numpy's "inverted_cdf".  The q below make q N / 100 an exact binary fraction (0, 25, 50,
    # 75, 100 with q / 100 exact or N q / 100 an integer either way) or keep it at least 0.01 from an integer, so numpy's floating
    # q / 100 * N lands on the side the exact rule does
    for i, s in enumerate(sets):
        for q in (0, 25, 50, 75, 100, 10, 90, 99, 33.3, 0.5):
            exact = s.size * q / 100.0
            if q not in (0, 25, 50, 75, 100) and abs(exact - round(exact)) < 0.01:
                continue
            assert hg.percentile(H[i], q) == np.percentile(s, q, method="inverted_cdf"), (i, q)
            assert hg.percentile(H[i], q) == s[max(1, int(np.ceil(exact - 1e-9))) - 1], (i, q)
    assert hg.percentile(H, 50).shape == (len(sets),) and hg.percentile(H, 0).tolist() == lo.tolist() and hg.percentile(H, 100).tolist() == hi.tolist()
    with pytest.raises(ValueError):
        hg.percentile(H, 100.5)
    for i, s in enumerate(sets):
        _v, cnt = np.unique(s, return_counts=True)
        p = cnt / s.size
        assert abs(hg.entropy_bits(H[i]) - -(p * np.log2(p)).sum()) < 1e-12, i
        assert np.allclose(hg.cdf(H[i]), [(s <= v).mean() for v in range(256)], rtol=1e-15, atol=0), i
    assert hg.entropy_bits(H[0]) == 0 and abs(hg.entropy_bits(H[-1]) - 8.0) < 1e-12
    # equalisation: OpenCV's rule restated on the samples
    for i, s in enumerate(sets):
        lut = hg.equalize_lut(H[i])
        assert lut.dtype == np.uint8 and lut.shape == (256,)
        cmin = (s <= s.min()).sum()
        if cmin == s.size:
            assert lut.tolist() == list(range(256)), i
            continue
        want = [max(0, int(np.floor(((s <= v).sum() - cmin) * 255 / (s.size - cmin) + 0.5))) if v >= s.min() else 0 for v in range(256)]
        assert lut.tolist() == want, i
        assert lut[s.min()] == 0 and lut[s.max()] == 255 and (np.diff(lut.astype(int)) >= 0).all()
    # Otsu: brute force over the samples, in exact integers: n0 n1 (m0 - m1)^2 = (s0 n1 - s1 n0)^2 / (n0 n1)
    for i, s in enumerate(sets):
        best, best_t = -1.0, 0
        for t in range(255):
            c0, c1 = s[s <= t], s[s > t]
            if c0.size and c1.size:
                from fractions import Fraction
                score = Fraction(int(c0.sum() * c1.size - c1.sum() * c0.size) ** 2, int(c0.size * c1.size))
                if score > best:
                    best, best_t = score, t
        assert hg.otsu(H[i]) == best_t, i
    assert hg.otsu(H).shape == (len(sets),) and 60 < hg.otsu(H[5]) < 180 and hg.otsu(H[1]) == 0 and hg.otsu(H[6]) == 3
    # distances of normalised histograms
    for i in range(len(sets)):
        for j in range(len(sets)):
            p, q = H[i] / sets[i].size, H[j] / sets[j].size
            assert abs(hg.intersection(H[i], H[j]) - np.minimum(p, q).sum()) < 1e-15
            s_ = p + q
            assert abs(hg.chi_square(H[i], H[j]) - ((p - q)[s_ > 0] ** 2 / s_[s_ > 0]).sum()) < 1e-14
    assert hg.intersection(H[3], H[3]) == pytest.approx(1.0, abs=1e-15) and hg.chi_square(H[3], H[3]) == 0
    assert hg.intersection(H[0], H[2]) == 0 and hg.chi_square(H[0], H[2]) == pytest.approx(2.0, abs=1e-15)
    assert hg.intersection(H[2], 5 * H[2].astype(np.int64)) == pytest.approx(1.0, abs=1e-15), "normalised by the sample counts"
    # read as HVQ_HIST_ABSDIFF records
    assert hg.max_abs_diff(H).tolist() == hi.tolist()
    assert hg.sad(H).tolist() == [s.sum() for s in sets] and hg.sse(H).tolist() == [(s * s).sum() for s in sets]
    zero = np.zeros(256, dtype=np.int32)
    zero[0] = 99
    assert np.isinf(hg.psnr(zero)) and hg.max_abs_diff(zero) == 0
    assert np.allclose(hg.psnr(H[1:]), [10 * np.log10(255.0 ** 2 * s.size / (s * s).sum()) for s in sets[1:]], rtol=1e-14, atol=0)
    # refusals
    with pytest.raises(ValueError):
        hg.mean(np.zeros(256, dtype=np.int32))
    with pytest.raises(ValueError):
        hg.samples(np.zeros(255, dtype=np.int32))
    with pytest.raises(TypeError):
        hg.samples(np.zeros(256))
    with pytest.raises(ValueError):
        hg.samples(-np.ones(256, dtype=np.int32))


def test_constants_are_those_of_the_kernels_header():
    from hvqm4_amd import histograms as hg
    text = open(os.path.join(fd.CSRC, "hvq_desc.h")).read()
    val = {k: int(v) for k, v in re.findall(r"#define (HVQ_HG_(?:BINS|LANES|UNITS))\s+(\d+)u", text)}
    assert set(val) == {"HVQ_HG_BINS", "HVQ_HG_LANES", "HVQ_HG_UNITS"} and "#define HVQ_HG_CHUNK  (HVQ_HG_LANES * HVQ_HG_UNITS)" in text
    assert hg.BINS == val["HVQ_HG_BINS"] and hg.WORKGROUP_UNITS == val["HVQ_HG_LANES"] * val["HVQ_HG_UNITS"]
    head = open(os.path.join(fd.ROOT, "include", "hvqm4_amd.h")).read()
    assert re.search(r"#define HVQ_HIST_BINS\s+256\b", head) and re.search(r"#define HVQ_HIST_VALUES\s+0\b", head) and re.search(r"#define HVQ_HIST_ABSDIFF\s+1\b", head)


def test_scenecuts_lines():
    """tools/scenecuts.py's formatter: a cut where the luma histograms of neighbours stop overlapping, none where only the order of the
    samples changes"""
    from tools.scenecuts import cut_lines
    dark, bright = np.bincount(np.arange(40, 60).repeat(10), minlength=256), np.bincount(np.arange(180, 220).repeat(5), minlength=256)
    lines = cut_lines(["I", "P", "P", "I"], np.stack([dark, dark, bright, bright]), [0.0, 1.5, 140.25, 0.0], 0.5)
    assert [l.split() for l in lines] == [["0", "I", "-", "-"], ["1", "P", "1.0000", "1.500"], ["2", "P", "0.0000", "140.250", "CUT"],
                                          ["3", "I", "1.0000", "0.000"]]
    assert cut_lines(["I", "P"], np.stack([dark, bright]), [0, 1], 0.0)[1].endswith("1.000"), "no intersection lies below a threshold of 0"


# ------------------------------------------------------------------------------------------------- the identities, on the oracle's pictures
def _geometry(name):
    from hvqm4_amd.container import parse_header
    hdr = parse_header(open(os.path.join(fd.GOLDEN, fd.CLIPS[name]["file"]), "rb").read())
    return hdr.width, hdr.height, hdr.h_samp, hdr.v_samp


_want = {}


def _side(name, form, k):
    a = fd.oracle_pictures(name)[k]
    return 255 - a if form == "inv" else a


def _expected(name, aform, ak, bform, bk):
    key = (name, aform, ak, bform, bk)
    if key not in _want:
        _want[key] = histogram_reference(_side(name, aform, ak), None if bform == "none" else _side(name, bform, bk), *_geometry(name))
    return _want[key]


def test_identities_against_the_metrics_reference_on_every_golden_clip():
    from hvqm4_amd import histograms as hg
    assert len(fd.CLIPS) >= 30
    samplings = set()
    for name in fd.CLIPS:
        g = _geometry(name)
        samplings.add(g[2:])
        pics = fd.oracle_pictures(name)
        sizes = list(plane_sizes(*g))
        for k in range(len(pics)):
            m0 = metrics_reference(pics[k], None, *g)
            hv = _expected(name, "pic", k, "none", 0)
            assert hv.sum(-1).tolist() == sizes and hg.samples(hv).tolist() == sizes, (name, k)
            assert hg.sad(hv).tolist() == m0[:, 0].tolist(), (name, k)                        # sum v h = sum_a
            assert hg.sse(hv).tolist() == m0[:, 3].tolist(), (name, k)                        # against zeros, sse = sum a^2
            assert (hg.of_picture(pics[k], *g) == hv).all()
            j = max(k - 1, 0)
            m = metrics_reference(pics[k], pics[j], *g)
            hd = _expected(name, "pic", k, "pic", j)
            assert hd.sum(-1).tolist() == sizes, (name, k)
            assert hg.sad(hd).tolist() == m[:, 2].tolist() and hg.sse(hd).tolist() == m[:, 3].tolist(), (name, k)
            if j == k:
                assert hd[:, 0].tolist() == sizes and hd[:, 1:].sum() == 0
    assert len(samplings) == 3


# ------------------------------------------------------------------------------------------------- argument checks without a device
class _NoDevice:
    """what Context.picture_histograms looks at before it reaches the library"""
    _geom = {0: (64, 48), 1: (24, 40)}
    _h = None

    @staticmethod
    def pic_bytes(sid):
        return {0: 64 * 48 * 3 // 2, 1: 24 * 40 * 3 // 2}[sid]


def test_references_and_sources_are_checked_before_the_library_is_called():
    import torch
    from hvqm4_amd._lib import HVQ_E_ARG, HvqError
    from hvqm4_amd.batch import Context
    call = lambda *a, **k: Context.picture_histograms(_NoDevice(), *a, **k)
    with pytest.raises(ValueError, match="ordinals"):
        call([0, 0], [0])
    with pytest.raises(HvqError) as e:
        call([0, 7], [0, 0])
    assert e.value.code == HVQ_E_ARG
    good = torch.zeros(64 * 48 * 3 // 2, dtype=torch.uint8)
    room = torch.zeros(64 * 48 * 3 // 2 + 64, dtype=torch.uint8)
    off = (-room.data_ptr()) % 16
    # ref
    with pytest.raises(TypeError):
        call([0], [0], ref=(0, 1).__iter__())
    with pytest.raises(ValueError, match="1 references for 2 pictures"):
        call([0, 0], [0, 1], ref=[(0, 1)])
    with pytest.raises(ValueError, match="reference 1 is None"):
        call([0, 0], [0, 1], ref=[(0, 1), None])
    with pytest.raises(TypeError, match="pair of integers"):
        call([0], [0], ref=[(0, 1, 2)])
    with pytest.raises(ValueError, match="not negative"):
        call([0], [0], ref=[(-1, 0)])
    with pytest.raises(TypeError, match="uint8"):
        call([0], [0], ref=[good.to(torch.int8)])
    with pytest.raises(ValueError, match="elements"):
        call([1], [0], ref=[good])
    with pytest.raises(ValueError, match="contiguous"):
        call([0], [0], ref=[torch.zeros(64 * 48 * 3, dtype=torch.uint8)[::2]])
    with pytest.raises(ValueError, match="multiple of 16"):
        call([0], [0], ref=[room[off + 8:off + 8 + good.numel()]])
    with pytest.raises(ValueError, match="reference 0 is on cpu, not a GPU"):
        call([0], [0], ref=[room[off:off + good.numel()]])
    # src
    with pytest.raises(ValueError, match="1 sources for 2 pictures"):
        call([0, 0], [0, 1], src=[None])
    with pytest.raises(TypeError):
        call([0], [0], src="memory")
    with pytest.raises(TypeError, match="uint8"):
        call([0], [-1], src=[good.to(torch.int8)])
    with pytest.raises(ValueError, match="elements"):
        call([1], [-1], src=[good])
    with pytest.raises(ValueError, match="ordinal -1"):
        call([0], [0], src=[room[off:off + good.numel()]])
    with pytest.raises(ValueError, match="multiple of 16"):
        call([0], [-1], src=[room[off + 8:off + 8 + good.numel()]])
    with pytest.raises(ValueError, match="source 0 is on cpu, not a GPU"):
        call([0], [-1], src=[room[off:off + good.numel()]])
    # out
    with pytest.raises(ValueError, match="out must be"):
        call([0], [0], out=torch.zeros((1, 3, 256), dtype=torch.int64))
    with pytest.raises(ValueError, match="out must be"):
        call([0], [0], out=torch.zeros((2, 3, 256), dtype=torch.int32))
    with pytest.raises(ValueError, match="out must be"):
        call([0], [0], out=torch.zeros((1, 3, 512), dtype=torch.int32)[:, :, ::2])
    with pytest.raises(ValueError, match="not a GPU"):
        call([0], [0], out=torch.zeros((1, 3, 256), dtype=torch.int32))


def test_the_library_without_a_device_still_checks_its_arguments():
    """no context can exist here, and the call says so before it looks at anything else"""
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, lib
    one = (C.c_int * 1)(0)
    assert lib().hvq_picture_histograms(None, 1, one, one, None, 0, None, None, None) == HVQ_E_ARG
    assert lib().hvq_picture_histograms(None, 0, None, None, None, 1, None, None, None) == HVQ_E_ARG


# ------------------------------------------------------------------------------------------------- the runtime on the CPU fake device
@pytest.fixture(scope="module")
def drivers():
    return {kind: fd.build_driver(kind, "histograms", "fake_histograms_driver", CXX_SOURCES, __file__) for kind in fd.BUILDS}


def _run(exe, scenario, schedule, tmp_path):
    _, lines = fd.run_checked(exe, scenario, schedule, tmp_path)
    K, R, S = {}, {}, {}
    for line in lines:
        f = line.split()
        if f[0] == "H":
            label, name, aform, ak, bform, bk = f[1], f[2], f[3], int(f[4]), f[5], int(f[6])
            got = np.array(f[7:], dtype=np.int64).reshape(3, 256)
            want = _expected(name, aform, ak, bform, bk)
            assert (got == want).all(), f"{label}: picture {ak} ({aform}) of {name} against {bform} {bk}: bins {np.argwhere(got != want)[:8].tolist()} differ"
            K.setdefault(label, []).append((name, aform, ak, bform, bk))
        elif f[0] == "R":
            R[f[1]] = int(f[2])
        elif f[0] == "S":
            S[f[1]] = (int(f[2]), int(f[3]))
    return K, R, S, fd.refusal_texts(lines)


def _check_goldens(K, R, S, E):
    n = {nm: fd.n_pics(nm) for nm in SIX}
    assert len({_geometry(nm)[2:] for nm in SIX}) == 3                    # 4:2:0, 4:2:2 and 4:4:4
    assert K["goldens/values"] == [(nm, "pic", k, "none", 0) for nm in SIX for k in range(n[nm])]
    assert K["goldens/prev"] == [(nm, "pic", k, "pic", k - 1) for nm in SIX for k in range(1, n[nm])] and K["goldens/prev"]
    assert K["goldens/self"] == [(nm, "pic", k, "pic", k) for nm in SIX for k in range(n[nm])]
    for nm, _a, k, _b, _k in K["goldens/self"]:
        h = _expected(nm, "pic", k, "pic", k)
        assert h[:, 0].tolist() == list(plane_sizes(*_geometry(nm))) and h[:, 1:].sum() == 0
    assert K["goldens/mixed"] == [(nm, "pic", (r * 3 + 1) % n[nm], "none", 0) for r in range(2) for nm in SIX], "records come back in call order"
    assert K["goldens/one"] == [("yuv422_296x160", "pic", 1, "pic", 0)]
    assert R == {"goldens/n0": 0, "goldens/n0_absdiff": 0}


def _check_memory(K, R, S, E):
    na = fd.n_pics("yuv422_64x48")
    nm = "yuv422_64x48"
    assert K["memory/values"] == [x for k in range(na) for x in ((nm, "inv", k, "none", 0), (nm, "pic", k, "none", 0))] + [("ragged24x40", "inv", 1, "none", 0)]
    want = [x for k in range(na) for x in ((nm, "inv", k, "pic", (k + 1) % na), (nm, "pic", k, "inv", (k + 1) % na), (nm, "inv", k, "inv", (k + 2) % na))]
    want.append(("ragged24x40", "pic", 0, "inv", 1))
    assert K["memory/diffs"] == want and K["memory/nullstream"] == want


def _check_reuse(K, R, S, E):
    from hvqm4_amd._lib import HVQ_E_STATE
    n, ne = fd.n_pics("gop64x48_15"), fd.n_pics("yuv444_64x48")
    diffs = [("gop64x48_15", "pic", k, "pic", (k + 1) % n) for k in range(n)]
    assert K["reuse/values"] == [("gop64x48_15", "pic", k, "none", 0) for k in range(n)]
    assert K["reuse/diffs"] == diffs
    assert R["reuse/evicted"] == HVQ_E_STATE, "the flushes did not hand the slots of the first pass on: the scenario tests nothing"
    assert R["reuse/evicted_ref"] == HVQ_E_STATE
    assert K["reuse/late"] == diffs
    assert K["reuse/destroy"] == [("yuv444_64x48", "pic", k, "none", 0) for k in range(ne)]


# what hvq_last_error_string() said after each call of `refused`, recorded from the runtime before the record frame: the
# order of the checks and their words are part of the interface.  A call that succeeds leaves the words of the refusal before it.
REFUSAL_TEXTS = {
    "refused/null_context": "bad arguments",
    "refused/null_context_absdiff": "bad arguments",
    "refused/bad_mode": "bad mode 2",
    "refused/negative_mode": "bad mode -1",
    "refused/values_with_ref": "HVQ_HIST_VALUES takes no reference (ref must be NULL)",
    "refused/absdiff_without_ref": "HVQ_HIST_ABSDIFF needs a reference for every picture (ref is NULL)",
    "refused/absdiff_against_zeros": "reference 1: |a - 0| is a itself, HVQ_HIST_VALUES gives it (stream -1 needs a pointer)",
    "refused/absdiff_against_zeros_ordinal": "reference 1: |a - 0| is a itself, HVQ_HIST_VALUES gives it (stream -1 needs a pointer)",
    "refused/bad_stream": "bad stream 99",
    "refused/bad_ordinal": "stream 0: bad picture ordinal 1000",
    "refused/misaligned_src": "picture 1: the pointer must be a multiple of 16",
    "refused/src_with_ordinal": "picture 1: a pointer together with ordinal 1 (the caller's memory takes ordinal -1)",
    "refused/src_with_bad_stream": "bad stream 99",
    "refused/minus_one_without_src": "stream 0: bad picture ordinal -1",
    "refused/ref_bad_stream": "bad stream 99",
    "refused/ref_below_minus_one": "reference 1: stream -2 (a stream, or -1 for the caller's memory)",
    "refused/ref_bad_ordinal": "stream 0: bad picture ordinal 1000",
    "refused/ref_pointer_with_stream": "reference 1: a pointer together with stream 0 (a resident reference takes no pointer)",
    "refused/ref_misaligned": "reference 1: the pointer must be a multiple of 16",
    "refused/ref_other_geometry": "reference 1: stream 1 (64 x 48, chroma shifts 1, 0) has not the geometry of stream 0 (64 x 48, 1, 1)",
    "refused/null_out": "out must be a non-null multiple of 4",
    "refused/misaligned_out": "out must be a non-null multiple of 4",
    "refused/too_many": "65536 pictures: one call takes 65535 at the most (one grid row each)",
    "refused/evicted": "stream 2 picture 0 is no longer resident (slot reused, or the picture was dropped)",
    "refused/evicted_ref": "stream 2 picture 0 is no longer resident (slot reused, or the picture was dropped)",
    "refused/queued": "stream 0 picture 7 is queued but not flushed",
    "refused/queued_ref": "stream 0 picture 7 is queued but not flushed",
    "refused/n0": "stream 0 picture 7 is queued but not flushed",
}


def _check_refused(K, R, S, E):
    for label, text in REFUSAL_TEXTS.items():
        assert E.get(label) == text, (label, E.get(label))
    assert set(E) == set(REFUSAL_TEXTS)
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_STATE
    arg = ["null_context", "null_context_absdiff", "bad_mode", "negative_mode", "values_with_ref", "absdiff_without_ref", "absdiff_against_zeros",
           "absdiff_against_zeros_ordinal", "bad_stream", "bad_ordinal", "misaligned_src", "src_with_ordinal", "src_with_bad_stream",
           "minus_one_without_src", "ref_bad_stream", "ref_below_minus_one", "ref_bad_ordinal", "ref_pointer_with_stream", "ref_misaligned",
           "ref_other_geometry", "null_out", "misaligned_out", "too_many"]
    want = {k: HVQ_E_ARG for k in arg}
    want.update({"evicted": HVQ_E_STATE, "evicted_ref": HVQ_E_STATE, "queued": HVQ_E_STATE, "queued_ref": HVQ_E_STATE, "n0": 0})
    assert R == {"refused/" + k: v for k, v in want.items()}
    same, total = S["refused"]
    assert same == total == 2 * 3072 + 8, "a refused call wrote its output"
    last = fd.n_pics("gop64x48_15") - 1
    assert K["refused/then_ok"] == [("gop64x48_15", "pic", 1, "none", 0), ("gop64x48_15", "pic", last, "none", 0)]
    assert K["refused/then_ok_absdiff"] == [("gop64x48_15", "pic", 1, "pic", last)]


CHECKS = {"goldens": _check_goldens, "memory": _check_memory, "reuse": _check_reuse, "refused": _check_refused}


@pytest.mark.parametrize("schedule", ["eager", "late"])
@pytest.mark.parametrize("build", list(fd.BUILDS))
@pytest.mark.parametrize("scenario", list(CHECKS))
def test_fake_device_scenario(drivers, scenario, build, schedule, tmp_path):
    CHECKS[scenario](*_run(drivers[build], scenario, schedule, tmp_path))


def test_the_existing_fake_builds_link_without_the_histogram_body():
    """the source lists of the other drivers have no hvq_launch_histograms: the runtime's reference to it is weak"""
    assert not any("fake_histograms" in s for s in fd.CXX_SOURCES)
    text = open(os.path.join(fd.CSRC, "hvq_runtime.cpp")).read()
    decl = [l for l in text.splitlines() if "hvq_launch_histograms(" in l and l.startswith("extern")]
    assert len(decl) == 1 and "weak" in decl[0]
