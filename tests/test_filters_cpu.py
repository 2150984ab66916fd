"""CPU: the values of hvq_filter_pictures.  tests/filter_ref.py restates include/hvqm4_amd.h in plain Python; hvqm4_amd.filters (numpy), a
float64 convolution by torch that shares no code with either, the fixture tests/golden/filter.json and the runtime on the CPU fake
device (tests/native/fake_filter.cpp, which walks the kernel's grid and phases with the kernel's own index arithmetic) are compared with
it by ==.  The fake-device driver is a stand-alone program, built and run plain and with ASan + UBSan as tests/test_scale_cpu.py builds
its own; nothing is preloaded and no Python is involved in the sanitised run."""
import hashlib
import json
import os
import zlib
from fractions import Fraction

import numpy as np
import pytest

import tests.test_fake_device as fd
from hvqm4_amd import filters as F
from tests import filter_ref as ref

NATIVE = fd.NATIVE
CXX_SOURCES = [s for s in fd.CXX_SOURCES if os.path.basename(s) != "fake_driver.cpp"] + \
              [os.path.join(NATIVE, "fake_filter.cpp"), os.path.join(NATIVE, "fake_filter_driver.cpp")]
FIXTURE = json.load(open(os.path.join(fd.GOLDEN, "filter.json")))


def _plane(*terms, combine=F.SUM, shift=0, bias=0):
    return F.PlaneFilter(tuple(F.Term(tuple(wx), tuple(wy)) for wx, wy in terms), combine, shift, bias)


ONES31 = (1,) * 31
MAXGAIN = _plane(((1024, 0, 1024), (1024, 0, 1024)), shift=22)          # gain exactly 2^22; on a checkerboard all four taps meet 255
# every builder; then the shapes a builder does not give
PLANES = {
    "identity": F.identity().luma, "binomial3": F.binomial(3).luma, "binomial5": F.binomial(5).luma, "binomial11": F.binomial(11).luma,
    "gauss1.5": F.gaussian(1.5).luma, "gauss0.5": F.gaussian(0.5).luma, "gauss5_r15_b11": F.gaussian(5.0, 15, 11).luma,
    "gauss_chroma420": F.chroma_for(F.gaussian(1.5), 2, 2).chroma, "gauss_chroma422": F.chroma_for(F.gaussian(3.0), 2, 1).chroma,
    "sobel_x": F.sobel("x").luma, "sobel_y": F.sobel("y").luma, "scharr_x": F.scharr("x").luma, "scharr_y": F.scharr("y").luma,
    "sobel_mag": F.gradient_magnitude("sobel").luma, "scharr_mag": F.gradient_magnitude("scharr").luma, "laplacian": F.laplacian().luma,
    "dog": F.dog(1.0, 2.0).luma, "dog_gain": F.dog(0.8, 1.6, gain_bits=3).luma, "unsharp": F.unsharp(1.0, Fraction(1, 2)).luma,
    "unsharp_strong": F.unsharp(2.0, 3).luma, "unsharp_chroma": F.chroma_for(F.unsharp(2.0, Fraction(3, 4)), 2, 1).chroma,
    "asymmetric": _plane(((3, -1, 4, 1, -5), (9, 2, -6)), shift=2, bias=7),
    "shift_left": _plane(((1, 0, 0), (1,))), "shift_right": _plane(((0, 0, 1), (1,))), "shift_up": _plane(((1,), (1, 0, 0))), "shift_down": _plane(((1,), (0, 0, 1))),
    "rx0_ry15": _plane(((1,), ONES31), shift=5), "rx15_ry0": _plane((ONES31, (1,)), shift=5),
    "r15_both": _plane((tuple(range(1, 32)), tuple(range(31, 0, -1))), shift=18),
    "two_r15": _plane((ONES31, ONES31), (tuple((-1) ** i * 3 for i in range(31)), ONES31), combine=F.SUM_ABS, shift=10),
    "two_radii": _plane(((1, 2, 1), ONES31), (ONES31, (-1, 0, 1)), combine=F.ABS_SUM, shift=6),
    "sum_negative": _plane(((-1, -1, -1), (1, 1, 1)), ((1,), (2,)), combine=F.SUM, shift=1, bias=255),
    "abs_sum": _plane(((-1, 0, 1), (1, 2, 1)), ((1, 2, 1), (-1, 0, 1)), combine=F.ABS_SUM, shift=2),
    "sum_abs": _plane(((-1, 0, 1), (1, 2, 1)), ((1, 2, 1), (-1, 0, 1)), combine=F.SUM_ABS, shift=0),
    "shift0": _plane(((1, 1, 1), (1,))), "shift22": _plane(((2048,), (2048,)), shift=22), "shift22_small": _plane(((1,), (1,)), shift=22, bias=3),
    "bias_low": _plane(((1,), (1,)), bias=-255), "bias_high": _plane(((1,), (1,)), shift=1, bias=255),
    "tie_half": _plane(((-1,), (1,)), shift=1, bias=2),                     # S = -a: -1 -> 0, -3 -> -1
    "maxgain": MAXGAIN, "maxgain_negative": _plane(((-1024, 0, -1024), (1024, 0, 1024)), shift=22, bias=255),
    "maxgain_two": _plane(((1024, 0, 1024), (512, 0, 512)), ((-1024, 0, -1024), (512, 0, 512)), combine=F.SUM_ABS, shift=22),
}


def _contents(nx, ny, seed):
    """random, 0 / 255 at random, and the two checkerboards"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:ny, 0:nx]
    return [rng.integers(0, 256, (ny, nx), dtype=np.uint8), (rng.integers(0, 2, (ny, nx)) * 255).astype(np.uint8),
            (((x + y) & 1) * 255).astype(np.uint8), (((x + y + 1) & 1) * 255).astype(np.uint8)]


def _ref_plane(a, p):
    return np.array(ref.filter_plane([bytes(r) for r in a], *ref.as_ref(p)), dtype=np.uint8)


@pytest.mark.parametrize("name", sorted(PLANES))
def test_module_equals_reference(name):
    p = PLANES[name]
    for (nx, ny), seed in (((12, 8), 1), ((8, 8), 2)):                      # 8 x 8 under radius 15: the clamp repeats
        for a in _contents(nx, ny, seed):
            assert np.array_equal(F.of_plane(a, p), _ref_plane(a, p)), (name, nx, ny)


def test_the_cases_cover_what_the_issue_names():
    assert F.gain(MAXGAIN) == F.MAX_GAIN == ref.MAX_GAIN
    a = _contents(8, 8, 0)[2]
    t = F.terms_of_plane(a, MAXGAIN)[0]
    assert int(t.max()) == 255 << 22 and int(t.max()) + (1 << 21) < 1 << 31, "the sums reach the 32-bit bound"
    assert {p.combine for p in PLANES.values()} == {F.SUM, F.ABS_SUM, F.SUM_ABS}
    assert {0, 22} <= {p.shift for p in PLANES.values()} and {-255, 255} <= {p.bias for p in PLANES.values()}
    radii = {(t.rx, t.ry) for p in PLANES.values() for t in p.terms}
    assert {(0, 15), (15, 0), (15, 15)} <= radii
    assert any(t.wx != t.wx[::-1] for p in PLANES.values() for t in p.terms), "non-symmetric taps"
    assert any(len(p.terms) == 2 and p.terms[0].ry != p.terms[1].ry for p in PLANES.values()), "two terms of different radii"


@pytest.mark.parametrize("name", sorted(PLANES))
def test_terms_against_a_float64_convolution(name):
    """torch.nn.functional.conv2d in float64 on the replicate-padded plane gives every T_t exactly: all values are below 2^53"""
    import torch
    import torch.nn.functional as tf
    p = PLANES[name]
    for a in _contents(20, 9, 3)[:3]:
        for t, term in zip(F.terms_of_plane(a, p), p.terms):
            x = torch.from_numpy(a.astype(np.float64))[None, None]
            x = tf.pad(x, (term.rx, term.rx, term.ry, term.ry), mode="replicate")
            k = torch.tensor(term.wy, dtype=torch.float64)[:, None] * torch.tensor(term.wx, dtype=torch.float64)[None, :]
            got = tf.conv2d(x, k[None, None])[0, 0].numpy()                 # conv2d is correlation: nothing is flipped
            assert np.array_equal(got, t.astype(np.float64)), name
            want = [r for r in ref.term_plane([bytes(r) for r in a], list(term.wx), list(term.wy))]
            assert np.array_equal(got, np.array(want, dtype=np.float64)), name


def _both(a, p):
    got = F.of_plane(np.array(a, dtype=np.uint8), p)
    assert np.array_equal(got, _ref_plane(np.array(a, dtype=np.uint8), p))
    return got.tolist()


def test_known_answers():
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, (5, 6), dtype=np.uint8)
    assert _both(a, F.identity().luma) == a.tolist()
    assert _both(a, PLANES["shift_left"]) == a[:, [0, 0, 1, 2, 3, 4]].tolist(), "wx = {1, 0, 0}: out[x] = a[max(x - 1, 0)]"
    assert _both(a, PLANES["shift_right"]) == a[:, [1, 2, 3, 4, 5, 5]].tolist()
    assert _both(a, PLANES["shift_up"]) == a[[0, 0, 1, 2, 3], :].tolist()
    assert _both(a, PLANES["shift_down"]) == a[[1, 2, 3, 4, 4], :].tolist()
    flat = np.full((6, 7), 201, dtype=np.uint8)
    for name in ("binomial3", "binomial11", "gauss1.5", "gauss5_r15_b11", "unsharp", "unsharp_strong", "maxgain", "shift22"):
        p = PLANES[name]
        assert sum(sum(t.wx) * sum(t.wy) for t in p.terms) == 1 << p.shift, name
        assert _both(flat, p) == flat.tolist(), name
    dot = np.zeros((3, 3), dtype=np.uint8)
    dot[1, 1] = 16
    assert _both(dot, F.binomial(3).luma) == [[1, 2, 1], [2, 4, 2], [1, 2, 1]]
    assert _both(flat, F.sobel("x", shift=0, bias=128).luma) == np.full((6, 7), 128).tolist()
    assert _both(flat, F.sobel("x").luma) == np.full((6, 7), 128).tolist()
    # S = -1, shift 1 -> 0 and S = -3, shift 1 -> -1 (bias 2 makes them visible: 2 and 1)
    assert _both([[1, 3, 1, 3]], PLANES["tie_half"]) == [[2, 1, 2, 1]]
    assert ref.finish(-1, 0, ref.SUM, 1, 0) == 0 and ref.finish(-3, 0, ref.SUM, 1, 2) == 1 and (-3 + 1) // 2 == -1


@pytest.mark.parametrize("bits", range(6, 13))
def test_gaussian_taps(bits):
    for sigma in np.arange(0.5, 5.0001, 0.125):
        for radius in (None, 15):
            w = F.gaussian_taps(float(sigma), radius, bits)
            r = len(w) // 2
            assert r == (min(15, int(np.ceil(3 * sigma))) if radius is None else radius)
            assert sum(w) == 1 << bits, (sigma, bits)
            assert w == w[::-1], (sigma, bits)
            assert all(w[r + k] >= w[r + k + 1] for k in range(r)), (sigma, bits, w)
            assert w[r] > 0 and min(w) >= 0, (sigma, bits, w)
    # the formula of the documentation where the centre needs no correction
    w = F.gaussian_taps(1.5, None, 8)
    g = [np.exp(-k * k / 4.5) for k in range(6)]
    side = [int(np.floor(256 * g[k] / (g[0] + 2 * sum(g[1:])) + 0.5)) for k in range(1, 6)]
    assert list(w[6:]) == side and w[5] == 256 - 2 * sum(side)


def test_builders():
    assert F.binomial(3).luma.terms[0].wx == (1, 2, 1) and F.binomial(5).luma.terms[0].wy == (1, 4, 6, 4, 1) and F.binomial(5).luma.shift == 8
    assert F.luma_only(F.gaussian(2.0)).chroma == F.identity().luma and F.is_identity(F.identity().chroma) and not F.is_identity(F.binomial(3).luma)
    g = F.chroma_for(F.gaussian(3.0), 2, 1)
    assert g.luma == F.gaussian(3.0).luma
    assert g.chroma.terms[0].wx == F.gaussian_taps(1.5) and g.chroma.terms[0].wy == F.gaussian_taps(3.0)
    assert F.chroma_for(F.gaussian(3.0), 1, 1).chroma == F.gaussian(3.0).luma
    assert F.chroma_for(F.sobel("x"), 2, 2).chroma == F.sobel("x").luma
    u = F.unsharp(1.0, 0.5)
    assert u == F.unsharp(1.0, Fraction(1, 2)) and hash(u) == hash(F.unsharp(1.0, Fraction(1, 2))) and u != F.unsharp(1.0, 1)
    assert len({F.gaussian(1.0), F.gaussian(1.0), F.binomial(3)}) == 2
    m = F.gradient_magnitude()
    assert len(m.luma.terms) == 2 and m.luma.combine == F.SUM_ABS
    edge = np.zeros((4, 6), dtype=np.uint8)
    edge[:, 3:] = 255
    assert int(F.of_plane(edge, m.luma).max()) == 255 and int(F.of_plane(edge, F.sobel("x").luma).max()) == 255
    assert len(F.laplacian().luma.terms) == 2 and len(F.dog(1, 2).luma.terms) == 2
    for bad in (lambda: F.unsharp(1.0, Fraction(1, 3)), lambda: F.unsharp(1.0, 0), lambda: F.binomial(4), lambda: F.binomial(13), lambda: F.gaussian(0),
                lambda: F.gaussian(1.0, 16), lambda: F.sobel("z"), lambda: F.gradient_magnitude("prewitt"), lambda: F.chroma_for(F.binomial(3), 1, 2),
                lambda: F.check(F.gaussian(1.0, None, 12)), lambda: F.check(F.unsharp(1.0, 200))):
        with pytest.raises(ValueError):
            bad()
    hist = np.zeros((3, 256), dtype=np.int64)
    hist[0, 10] = 3
    hist[0, 30] = 1
    hist[1:, 0] = 1
    assert F.sharpness(hist).tolist() == [15.0, 0.0, 0.0]


def test_struct_layout():
    import ctypes as C
    from hvqm4_amd._lib import HvqFilter, HvqFilterTerm, HvqPlaneFilter
    assert (C.sizeof(HvqFilterTerm), C.sizeof(HvqPlaneFilter), C.sizeof(HvqFilter)) == (132, 280, 560)
    s = PLANES_FILTER("asymmetric").to_struct()
    assert (s.luma.terms, s.luma.shift, s.luma.bias, s.luma.term[0].rx, s.luma.term[0].ry) == (1, 2, 7, 2, 1)
    assert list(s.luma.term[0].wx)[:6] == [3, -1, 4, 1, -5, 0] and list(s.luma.term[0].wy)[:4] == [9, 2, -6, 0]


def PLANES_FILTER(name):
    return F.Filter(PLANES[name], PLANES[name])


# ------------------------------------------------------------------------------------------------- the fixture
def _clip_geometry(name):
    from hvqm4_amd.container import parse_header
    hdr = parse_header(open(os.path.join(fd.GOLDEN, fd.CLIPS[name]["file"]), "rb").read())
    return (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)


def _fixture_filters(hs, vs):
    return [("gauss1.5", F.chroma_for(F.gaussian(1.5), hs, vs)), ("unsharp1.0_1/2", F.luma_only(F.unsharp(1.0, Fraction(1, 2)))),
            ("sobelmag", F.luma_only(F.gradient_magnitude("sobel")))]


def test_fixture_covers_every_golden_clip():
    assert set(FIXTURE["clips"]) == set(fd.CLIPS)
    for name, entry in FIXTURE["clips"].items():
        assert tuple(entry["geometry"]) == _clip_geometry(name)
        assert [l for l, _c in entry["filters"]] == ["gauss1.5", "unsharp1.0_1/2", "sobelmag"]


@pytest.mark.parametrize("name", sorted(FIXTURE["clips"]))
def test_fixture_equals_reference_and_module(name):
    entry = FIXTURE["clips"][name]
    g = tuple(entry["geometry"])
    pic = fd.oracle_pictures(name)[-1]
    assert hashlib.sha256(pic.tobytes()).hexdigest() == fd.CLIPS[name]["picture_sha256"][-1], "the fixture describes the manifest's picture"
    for (label, crc), (label2, f) in zip(entry["filters"], _fixture_filters(*g[2:])):
        assert label == label2
        got = F.of_picture(pic, g, f)
        assert zlib.crc32(got.tobytes()) == crc, (name, label)
        if g[0] * g[1] <= 64 * 48:                                          # plain Python: the small clips, every sampling among them
            assert ref.filter_picture(pic.tobytes(), g, ref.as_ref(f.luma), ref.as_ref(f.chroma)) == got.tobytes(), (name, label)


def test_the_reference_meets_clips_of_every_sampling():
    small = {tuple(e["geometry"])[2:] for e in FIXTURE["clips"].values() if e["geometry"][0] * e["geometry"][1] <= 64 * 48}
    assert small == {(2, 2), (2, 1), (1, 1)}


# ------------------------------------------------------------------------------------------------- argument checks without a device
class _NoDevice:
    """what Context.filter_pictures looks at before it reaches the library"""
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
    call = lambda *a, **k: Context.filter_pictures(_NoDevice(), *a, **k)
    f = F.binomial(3)
    with pytest.raises(ValueError, match="ordinals"):
        call([0, 0], [0], f)
    with pytest.raises(HvqError) as e:
        call([0, 7], [0, 0], f)
    assert e.value.code == HVQ_E_ARG
    for filt in (None, "blur", [f], [f, None], f.luma):
        with pytest.raises(ValueError, match="filt"):
            call([0, 0], [0, 1], filt)
    with pytest.raises(ValueError, match="gain"):
        call([0], [0], F.Filter(f.luma, F.PlaneFilter((F.Term((2049,), (2048,)),), F.SUM, 22, 0)))
    with pytest.raises(ValueError, match="terms"):
        call([0], [0], F.Filter(F.PlaneFilter(()), f.chroma))
    with pytest.raises(ValueError, match="shift"):
        call([0], [0], F.Filter(F.PlaneFilter(f.luma.terms, F.SUM, 23, 0), f.chroma))
    with pytest.raises(ValueError, match="bias"):
        call([0], [0], F.Filter(f.luma, F.PlaneFilter(f.luma.terms, F.SUM, 4, 256)))
    with pytest.raises(ValueError, match="combine"):
        call([0], [0], F.Filter(f.luma, F.PlaneFilter(f.luma.terms, 3, 4, 0)))
    with pytest.raises(ValueError, match="taps"):
        call([0], [0], F.Filter(F.PlaneFilter((F.Term((1,) * 33, (1,)),)), f.chroma))
    with pytest.raises(ValueError, match="taps"):
        call([0], [0], F.Filter(F.PlaneFilter((F.Term((1, 1), (1,)),)), f.chroma))
    with pytest.raises(ValueError, match="65 distinct"):
        call([0] * 65, list(range(65)), [F.sobel("x", bias=b) for b in range(65)])
    with pytest.raises(ValueError, match="not a GPU"):                       # 64 distinct ones (each given twice): on to the next check
        call([0] * 128, list(range(128)), [F.sobel("x", bias=b % 64) for b in range(128)], out=torch.zeros((128, 4608), dtype=torch.uint8))
    with pytest.raises(ValueError, match="1 sources for 2 pictures"):
        call([0, 0], [0, 1], f, src=[None])
    good = torch.zeros(64 * 48 * 3 // 2, dtype=torch.uint8)
    with pytest.raises(ValueError, match="elements"):
        call([1], [-1], f, src=[good])
    room = torch.zeros(64 * 48 * 3 // 2 + 64, dtype=torch.uint8)
    off = (-room.data_ptr()) % 16
    with pytest.raises(ValueError, match="ordinal -1"):
        call([0], [0], f, src=[room[off:off + good.numel()]])
    with pytest.raises(ValueError, match="not a GPU"):
        call([0], [-1], f, src=[room[off:off + good.numel()]])
    nb = 64 * 48 * 3 // 2
    with pytest.raises(ValueError, match="out must be"):
        call([0, 0], [0, 1], f, out=torch.zeros((2, nb), dtype=torch.int32))
    with pytest.raises(ValueError, match="out must be"):
        call([0, 0], [0, 1], f, out=torch.zeros((2, nb + 16), dtype=torch.uint8))
    with pytest.raises(ValueError, match="out must be"):
        call([0, 0], [0, 1], f, out=[torch.zeros(nb, dtype=torch.uint8)] * 2)                          # one geometry: one tensor
    with pytest.raises(ValueError, match="out must be a list"):
        call([0, 1], [0, 1], f, out=torch.zeros((2, nb), dtype=torch.uint8))                           # two geometries: a list
    with pytest.raises(ValueError, match=r"out\[1\]"):
        call([0, 1], [0, 1], f, out=[torch.zeros(nb, dtype=torch.uint8)] * 2)
    with pytest.raises(ValueError, match="multiple of 16"):
        room = torch.zeros(2 * nb + 64, dtype=torch.uint8)
        off = (-room.data_ptr()) % 16 + 8
        call([0, 0], [0, 1], f, out=room[off:off + 2 * nb].view(2, nb))
    with pytest.raises(ValueError, match="not a GPU"):
        call([0, 0], [0, 1], f, out=torch.zeros((2, nb), dtype=torch.uint8))
    with pytest.raises(ValueError, match="not a GPU"):
        call([0, 1, 2], [0, 1, 2], [f, F.identity(), f], out=[torch.zeros(_NoDevice.pic_bytes(s), dtype=torch.uint8) for s in (0, 1, 2)])
    with pytest.raises(ValueError, match="65535"):
        call([0] * 65536, [0] * 65536, f)


def _spoiled():
    """(label, HvqFilter struct) for every refusal of hvq_filter_check, in the chroma plane of an otherwise good filter"""
    out = []

    def bad(label, spoil):
        s = F.binomial(3).to_struct()
        spoil(s.chroma)
        out.append((label, s))
    bad("terms 0", lambda p: setattr(p, "terms", 0))
    bad("terms 3", lambda p: setattr(p, "terms", 3))
    bad("radius 16", lambda p: setattr(p.term[0], "rx", 16))
    bad("radius -1", lambda p: setattr(p.term[0], "ry", -1))
    bad("a tap beyond the radius", lambda p: p.term[0].wx.__setitem__(3, 1))
    bad("the last tap beyond the radius", lambda p: p.term[0].wy.__setitem__(30, -1))
    bad("combine 3", lambda p: setattr(p, "combine", 3))
    bad("combine -1", lambda p: setattr(p, "combine", -1))
    bad("shift 23", lambda p: setattr(p, "shift", 23))
    bad("shift -1", lambda p: setattr(p, "shift", -1))
    bad("bias 256", lambda p: setattr(p, "bias", 256))
    bad("bias -256", lambda p: setattr(p, "bias", -256))

    def gain0(p):
        for i in range(3):
            p.term[0].wx[i] = 0
    bad("gain 0", gain0)

    def above(p):
        p.term[0].rx = p.term[0].ry = 0
        for i in range(3):
            p.term[0].wx[i] = p.term[0].wy[i] = 0
        p.term[0].wx[0], p.term[0].wy[0], p.shift = 2049, 2048, 22
    bad("gain above 2^22", above)
    return out


def test_the_library_without_a_device_still_checks_its_arguments():
    """no context can exist here, and the call says so before it looks at anything else; the host-only check works"""
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, lib
    one = (C.c_int * 1)(0)
    f = F.binomial(3).to_struct()
    dst = (C.c_void_p * 1)(16)
    assert lib().hvq_filter_pictures(None, 1, one, one, None, C.byref(f), 1, None, C.cast(dst, C.c_void_p), None) == HVQ_E_ARG
    assert lib().hvq_filter_force_filter(None, 1) == HVQ_E_ARG
    assert lib().hvq_filter_check(None) == HVQ_E_ARG
    for name, p in PLANES.items():
        assert lib().hvq_filter_check(C.byref(F.Filter(p, F.identity().luma).to_struct())) == 0, name
        assert lib().hvq_filter_check(C.byref(F.Filter(F.identity().luma, p).to_struct())) == 0, name
    for label, s in _spoiled():
        assert lib().hvq_filter_check(C.byref(s)) == HVQ_E_ARG, label
        s.luma, s.chroma = s.chroma, s.luma
        assert lib().hvq_filter_check(C.byref(s)) == HVQ_E_ARG, label + " (luma)"
    s = F.binomial(3).to_struct()                                           # a term that is not in use is not looked at
    s.luma.term[1].rx = 99
    s.luma.term[1].wx[30] = 7
    assert lib().hvq_filter_check(C.byref(s)) == 0
    at_limit = F.Filter(MAXGAIN, MAXGAIN).to_struct()
    assert lib().hvq_filter_check(C.byref(at_limit)) == 0


# ------------------------------------------------------------------------------------------------- the runtime on the CPU fake device
DRIVER_FILTERS = {                                                          # the first has a radius below 15 (the driver's malformed ones derive from it)
    "binomial3": F.binomial(3), "identity": F.identity(), "gauss1.5_420": F.chroma_for(F.gaussian(1.5), 2, 2), "gauss5_r15": F.gaussian(5.0, 15, 8),
    "sobel_x": F.sobel("x"), "scharr_y": F.scharr("y"), "sobel_mag_luma": F.luma_only(F.gradient_magnitude()), "laplacian": F.laplacian(),
    "dog": F.dog(1.0, 2.0), "unsharp_luma": F.luma_only(F.unsharp(1.0, Fraction(1, 2))), "chroma_only": F.Filter(F.identity().luma, F.binomial(5).luma),
    "asymmetric": F.Filter(PLANES["asymmetric"], PLANES["rx0_ry15"]), "two_r15": F.Filter(PLANES["two_r15"], PLANES["two_radii"]),
    "rx15": F.Filter(PLANES["rx15_ry0"], PLANES["r15_both"]), "abs_sum": F.Filter(PLANES["abs_sum"], PLANES["sum_negative"]),
    "maxgain": F.Filter(MAXGAIN, PLANES["maxgain_two"]), "tie_half": F.Filter(PLANES["tie_half"], PLANES["maxgain_negative"]),
    "shifts": F.Filter(PLANES["shift_left"], PLANES["shift_down"]),
}


def _filters_txt():
    lines = []
    for name, f in DRIVER_FILTERS.items():
        v = []
        for p in (f.luma, f.chroma):
            v += [len(p.terms), p.combine, p.shift, p.bias]
            for t in range(2):
                term = p.terms[t] if t < len(p.terms) else F.Term((0,), (0,))
                v += [term.rx, term.ry] + list(term.wx) + [0] * (31 - len(term.wx)) + list(term.wy) + [0] * (31 - len(term.wy))
        lines.append(name + " " + " ".join(str(x) for x in v))
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def drivers():
    return {kind: fd.build_driver(kind, "filter", "fake_filter_driver", CXX_SOURCES, __file__) for kind in fd.BUILDS}


_want = {}


def _source(source, form, k, geom):
    """the picture the driver filtered, as the driver's line describes it"""
    from hvqm4_amd import scale
    n = scale.nbytes(*geom)
    if form == "pic":
        return fd.oracle_pictures(source)[k].reshape(-1)
    if form == "inv":
        return 255 - fd.oracle_pictures(source)[k].reshape(-1)
    if form.startswith("filtered:"):
        return _expected(source, "pic", k, geom, form.split(":", 1)[1])[1]
    if form == "synth":
        return ((((np.arange(n, dtype=np.uint64) + np.uint64(k)) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(13)).astype(np.uint8)
    if form == "flat":
        return np.full(n, k, dtype=np.uint8)
    if form == "check":
        w, h, hs, vs = geom
        out = []
        for pw, ph in ((w, h), (w // hs, h // vs), (w // hs, h // vs)):
            y, x = np.mgrid[0:ph, 0:pw]
            out.append((((x + y + k) & 1) * 255).astype(np.uint8).reshape(-1))
        return np.concatenate(out)
    raise AssertionError(form)


def _expected(source, form, k, geom, fname):
    key = (source, form, k, geom, fname)
    if key not in _want:
        got = F.of_picture(_source(source, form, k, geom), geom, DRIVER_FILTERS[fname])
        _want[key] = (zlib.crc32(got.tobytes()), got)
    return _want[key]


def _run(exe, scenario, schedule, tmp_path):
    _, lines = fd.run_checked(exe, scenario, schedule, tmp_path, inputs={"filters.txt": _filters_txt()})
    P, R, S = {}, {}, {}
    for line in lines:
        f = line.split()
        if f[0] == "P":
            label, source, form, k, geom, fname = f[1], f[2], f[3], int(f[4]), tuple(int(v) for v in f[5:9]), f[9]
            assert int(f[11]) == 1, f"{label}: the bytes around the output of {source} {k} were written"
            want = _expected(source, form, k, geom, fname)[0]
            assert int(f[10]) == want, f"{label}: picture {k} of {source} ({form}) {geom} through {fname}: crc {int(f[10]):08x}, want {want:08x}"
            P.setdefault(label, []).append((source, form, k, geom, fname))
        elif f[0] == "R":
            R[f[1]] = int(f[2])
        elif f[0] == "S":
            S[f[1]] = (int(f[2]), int(f[3]))
    return P, R, S


def _check_goldens(P, R, S):
    nf = len(DRIVER_FILTERS)
    assert len(P["goldens/all"]) == 6 * nf and {fn for *_r, fn in P["goldens/all"]} == set(DRIVER_FILTERS)
    assert {g[2:] for _s, _f, _k, g, _n in P["goldens/all"]} == {(2, 2), (2, 1), (1, 1)}
    assert any(g[0] > 128 and g[1] > 32 for _s, _f, _k, g, _n in P["goldens/all"]), "tile seams inside a plane"
    assert P["goldens/one"] == [P["goldens/all"][1]]
    assert R == {"goldens/n0": 0}


def _check_memory(P, R, S):
    nf = len(DRIVER_FILTERS)
    assert P["memory"] == P["memory/nullstream"] and len(P["memory"]) == 2 * fd.n_pics("yuv422_64x48") + 7 * (2 * nf + 1)
    forms = [f for _s, f, *_r in P["memory"]]
    assert forms.count("inv") == fd.n_pics("yuv422_64x48") and forms.count("check") == 7 * nf and forms.count("flat") == 7
    geoms = {g for _s, f, _k, g, _n in P["memory"] if f == "check"}
    assert {(8, 8, 2, 2), (8, 8, 2, 1), (8, 8, 1, 1), (72, 24, 2, 2), (136, 40, 2, 2)} <= geoms
    assert ("synth", "check", 1, (8, 8, 2, 2), "maxgain") in P["memory"] or ("synth", "check", 0, (8, 8, 2, 2), "maxgain") in P["memory"]
    full = _expected("synth", "check", list(DRIVER_FILTERS).index("maxgain") & 1, (136, 40, 2, 2), "maxgain")[1]
    assert {0, 255} <= set(np.unique(full[:136 * 40]).tolist()), "the maximum-gain filter on the checkerboard reaches 255 2^22"


def _check_many(P, R, S):
    assert len(P["many"]) == 300 and P["many"] == P["many/again"]
    assert len({s for s, *_r in P["many"]}) == 8 and len({g for _s, _f, _k, g, _n in P["many"]}) >= 4 and len({n for *_r, n in P["many"]}) >= 8


def _check_body(P, R, S):
    assert P["body/chosen"] == P["body/filter"] == P["body/chosen_again"] and len(P["body/filter"]) == 4 * len(DRIVER_FILTERS)
    assert R == {"body/force": 0, "body/unforce": 1}
    assert sum(1 for f in DRIVER_FILTERS.values() if F.is_identity(f.luma) or F.is_identity(f.chroma)) >= 4


def _check_reuse(P, R, S):
    from hvqm4_amd._lib import HVQ_E_STATE
    n, ne = fd.n_pics("gop64x48_15"), fd.n_pics("yuv444_64x48")
    g = _clip_geometry("gop64x48_15")
    names = list(DRIVER_FILTERS)
    assert P["reuse"] == [("gop64x48_15", "pic", k, g, names[1]) for k in range(n)]
    assert R["reuse/evicted"] == HVQ_E_STATE, "the flushes did not hand the slots of the first pass on: the scenario tests nothing"
    assert P["reuse/chain"] == [("gop64x48_15", "filtered:" + names[1], k, g, names[2]) for k in range(n)]
    assert P["reuse/late"] == P["reuse"]
    assert [(s, k) for s, _f, k, *_r in P["reuse/destroy"]] == [("yuv444_64x48", k) for k in range(ne)]


def _check_refused(P, R, S):
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_STATE
    arg = ["null_context", "bad_stream", "bad_ordinal", "misaligned_src", "src_with_ordinal", "src_with_bad_stream", "minus_one_without_src", "null_dst",
           "misaligned_dst", "too_many", "null_filters", "nfilters_0", "nfilters_65", "which_high", "which_negative", "force_null", "check_null"]
    spoiled = ["terms_0", "terms_3", "radius_16", "radius_negative", "tap_beyond", "tap_beyond_y", "combine_3", "combine_negative", "shift_23", "shift_negative",
               "bias_256", "bias_minus_256", "gain_0", "gain_above"]
    want = {k: HVQ_E_ARG for k in arg + spoiled + ["check_" + s for s in spoiled]}
    want.update({"evicted": HVQ_E_STATE, "queued": HVQ_E_STATE, "n0": 0, "check_good": 0, "check_unused_term": 0})
    assert R == {"refused/" + k: v for k, v in want.items()}
    same, total = S["refused"]
    assert same == total == 2 * 4608 + 16, "a refused call wrote its output"
    g = _clip_geometry("gop64x48_15")
    names = list(DRIVER_FILTERS)
    assert P["refused/then_ok"] == [("gop64x48_15", "pic", 1, g, names[63 % len(names)]), ("gop64x48_15", "pic", fd.n_pics("gop64x48_15") - 1, g, names[0])]


CHECKS = {"goldens": _check_goldens, "memory": _check_memory, "many": _check_many, "body": _check_body, "reuse": _check_reuse, "refused": _check_refused}


@pytest.mark.parametrize("schedule", ["eager", "late"])
@pytest.mark.parametrize("build", list(fd.BUILDS))
@pytest.mark.parametrize("scenario", list(CHECKS))
def test_fake_device_scenario(drivers, scenario, build, schedule, tmp_path):
    P, R, S = _run(drivers[build], scenario, schedule, tmp_path)
    CHECKS[scenario](P, R, S)


def test_the_existing_fake_builds_link_without_the_filter_body():
    """the source lists of the other drivers have no hvq_launch_filter: the runtime's reference is weak"""
    assert not any("fake_filter" in s for s in fd.CXX_SOURCES)
    text = open(os.path.join(fd.CSRC, "hvq_runtime.cpp")).read()
    decl = [l for l in text.splitlines() if "hvq_launch_filter(" in l and l.startswith("extern")]
    assert len(decl) == 1 and "weak" in decl[0]
