"""CPU: scaled pictures in slot layout (hvq_scale_pictures / Context.scale_pictures, hvqm4_amd/scale.py) without a GPU.

  - hvqm4_amd.scale (numpy) equals tests/scale_ref.py (plain loops over Python integers, the text of include/hvqm4_amd.h) on random planes:
    identity, integer and non-integer reductions, enlargement, down in x with up in y; the rows of the weights sum to N;
  - the known answers of the header: identity, the k x k box mean rounded half up, replication, flat stays flat, the two tie pictures;
  - the division the kernel uses (the high 64 bits of v * ceil(2^64 / D)) against Python's // at the edges of every quotient for plane
    sizes up to 8192 x 8192 and on random sums, in Python (scale.divide) and in C (hvq_sc_div of hvq_scale.h, a stand-alone program);
  - tests/golden/scale.json equals both the reference and the module on the oracle's pictures, whose SHA-256 are manifest.json's;
  - the argument checks of Context.scale_pictures that need no device, and the library's without a device;
  - the runtime's entry point linked UNCHANGED against the CPU fake device of tests/test_fake_device.py (its source lists and flags, with
    tests/native/fake_scale_driver.cpp in the place of fake_driver.cpp and tests/native/fake_scale.cpp added: the kernel's two bodies
    walked lane by lane with its own index arithmetic, memory reached only through fake_span, when they run), under both schedules, plain
    and as a stand-alone AddressSanitizer + UndefinedBehaviorSanitizer program.  The driver judges nothing: every picture it read back is
    compared here with hvqm4_amd.scale.of_picture.
"""
import hashlib
import json
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

import tests.test_fake_device as fd
from tests import scale_ref as ref

NATIVE = fd.NATIVE
CXX_SOURCES = [s for s in fd.CXX_SOURCES if os.path.basename(s) != "fake_driver.cpp"] + \
              [os.path.join(NATIVE, "fake_scale.cpp"), os.path.join(NATIVE, "fake_scale_driver.cpp")]
FIXTURE = json.load(open(os.path.join(fd.GOLDEN, "scale.json")))
# (nx, ny) -> (mx, my): identity, integer and non-integer reductions, enlargement, down in x with up in y, the 32x limit
SIZES = [((24, 16), (24, 16)), ((24, 40), (16, 16)), ((24, 40), (8, 8)), ((40, 24), (24, 16)), ((128, 96), (56, 40)), ((64, 48), (32, 24)), ((64, 48), (16, 12)),
         ((8, 8), (264, 16)), ((16, 16), (40, 24)), ((128, 8), (56, 264)), ((8, 128), (264, 56)), ((37, 23), (12, 20)), ((256, 64), (8, 8)), ((4, 4), (12, 8))]


def _random_plane(nx, ny, seed):
    return np.random.default_rng(seed).integers(0, 256, (ny, nx), dtype=np.uint8)


def _ref_plane(a, mx, my):
    return np.array(ref.scale_plane([bytes(r) for r in a], mx, my), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------- the module against the reference
@pytest.mark.parametrize("src,dst", SIZES)
def test_module_equals_reference(src, dst):
    from hvqm4_amd import scale
    a = _random_plane(src[0], src[1], src[0] * 131 + dst[0])
    got = scale.of_plane(a, dst[0], dst[1])
    assert got.dtype == np.uint8 and got.shape == (dst[1], dst[0])
    assert np.array_equal(got, _ref_plane(a, dst[0], dst[1]))
    extreme = np.where(a >= 128, 255, 0).astype(np.uint8)
    assert np.array_equal(scale.of_plane(extreme, dst[0], dst[1]), _ref_plane(extreme, dst[0], dst[1]))


def test_the_sizes_cover_what_the_issue_names():
    pairs = {(s[0], d[0]) for s, d in SIZES} | {(s[1], d[1]) for s, d in SIZES}
    assert {(24, 16), (40, 24), (128, 56), (8, 264)} <= pairs
    assert any(s == d for s, d in SIZES) and any(s[0] > d[0] and s[1] < d[1] for s, d in SIZES) and any(s[0] == 32 * d[0] for s, d in SIZES)


def test_weights():
    from hvqm4_amd import scale
    for n, m in [(24, 16), (40, 24), (128, 56), (8, 264), (16, 16), (256, 8), (7, 5), (5, 7), (8192, 256)]:
        w = scale.weights(n, m)
        assert w.shape == (m, n) and w.dtype == np.int64 and w.min() >= 0
        assert (w.sum(axis=1) == n).all() and (w.sum(axis=0) == m).all()
        if n * m <= 4096:
            assert w.tolist() == [[ref.weight(n, m, r, y) for y in range(n)] for r in range(m)]
        taps = (w > 0).sum(axis=1).max()
        assert taps <= (n + m - 1) // m + 1 and (n > m or taps <= 2), "an enlargement has two taps at the most"


def test_known_answers():
    from hvqm4_amd import scale
    a = _random_plane(40, 24, 1)
    for f in (scale.of_plane, _ref_plane):
        assert np.array_equal(f(a, 40, 24), a), "M == N is the identity"
        for k in (2, 4, 8):
            box = a.reshape(24 // k, k, 40 // k, k).astype(np.int64).sum(axis=(1, 3))
            assert np.array_equal(f(a, 40 // k, 24 // k), (box + k * k // 2) // (k * k)), f"the {k} x {k} box mean, rounded half up"
        assert np.array_equal(f(a, 120, 48), np.repeat(np.repeat(a, 2, axis=0), 3, axis=1)), "an integer enlargement replicates samples"
        for v in (0, 1, 127, 255):
            flat = np.full((24, 40), v, dtype=np.uint8)
            for mx, my in ((40, 24), (16, 8), (56, 40), (8, 264), (24, 16)):
                assert (f(flat, mx, my) == v).all(), "a flat picture stays flat"
        assert f(np.array([[0, 0], [0, 2]], dtype=np.uint8), 1, 1).tolist() == [[1]] and f(np.array([[0, 0], [0, 1]], dtype=np.uint8), 1, 1).tolist() == [[0]]


def test_tie_pictures():
    from hvqm4_amd import scale
    two, one = ref.tie_pictures()
    assert ref.scale_picture(two, ref.TIE_GEOMETRY, ref.TIE_TARGET) == bytes([1]) * 192
    assert ref.scale_picture(one, ref.TIE_GEOMETRY, ref.TIE_TARGET) == bytes(192)
    assert scale.of_picture(two, ref.TIE_GEOMETRY, ref.TIE_TARGET).tolist() == [1] * 192
    assert scale.of_picture(one, ref.TIE_GEOMETRY, ref.TIE_TARGET).tolist() == [0] * 192


def test_pictures_samplings_and_crops():
    """of_picture against the reference: every pair of samplings, a crop with odd values on 4:4:4, chroma crop edges divided by the source
    sampling"""
    from hvqm4_amd import scale
    rng = np.random.default_rng(3)
    for src in ((32, 24, 2, 2), (32, 24, 2, 1), (32, 24, 1, 1)):
        pic = rng.integers(0, 256, scale.nbytes(*src), dtype=np.uint8)
        for to in scale.SAMPLINGS:
            for size, crop in (((16, 16), None), ((40, 8), None), ((8, 8), (src[2] * 3, src[3] * 5, 12 * src[2], 9 * src[3] if src[3] == 1 else 10))):
                dst = size + to
                got = scale.of_picture(pic, src, dst, crop)
                assert got.size == scale.nbytes(*dst)
                assert got.tobytes() == ref.scale_picture(pic.tobytes(), src, dst, crop), (src, dst, crop)
    y, u, v = scale.planes(np.arange(32 * 24 * 2, dtype=np.uint8), 32, 24, 2, 1)
    assert y.shape == (24, 32) and u.shape == v.shape == (24, 16) and u[0, 0] == (32 * 24) % 256
    for bad in ((1, 0, 16, 16), (0, 1, 16, 16), (0, 0, 15, 16), (0, 0, 6, 16), (24, 0, 16, 16), (0, 0, 0, 0), (-2, 0, 16, 16)):
        with pytest.raises(ValueError):
            scale.of_picture(np.zeros(scale.nbytes(32, 24), dtype=np.uint8), (32, 24, 2, 2), (16, 16, 2, 2), bad)
    with pytest.raises(ValueError, match="beyond 32"):
        scale.plane_sizes((528, 16, 2, 2), (16, 16, 2, 2))
    scale.plane_sizes((512, 16, 2, 2), (16, 16, 2, 2))
    with pytest.raises(ValueError, match="beyond 32"):
        scale.plane_sizes((512, 16, 1, 1), (16, 16, 2, 2))             # chroma: 512 -> 8


def test_fit_and_pyramid():
    from hvqm4_amd import scale
    assert scale.fit(640, 480, 56, 56) == (56, 40) and scale.fit(48, 64, 56, 56) == (40, 56) and scale.fit(64, 64, 56, 56) == (56, 56)
    assert scale.fit(8192, 8, 56, 56) == (56, 8) and scale.fit(296, 160, 160, 120) == (160, 88)
    for w, h, mw, mh in ((640, 480, 100, 100), (24, 40, 56, 56), (8, 8, 8, 8), (1920, 1080, 320, 320)):
        fw, fh = scale.fit(w, h, mw, mh)
        assert fw % 8 == 0 and fh % 8 == 0 and 8 <= fw <= mw and 8 <= fh <= mh
    assert scale.pyramid(640, 480, 5) == [(640, 480), (320, 240), (160, 120), (80, 64), (40, 32)]
    assert scale.pyramid(24, 40, 4) == [(24, 40), (16, 24), (8, 16), (8, 8)]
    assert scale.nbytes(64, 48) == 4608 and scale.nbytes(64, 48, 2, 1) == 6144 and scale.nbytes(64, 48, 1, 1) == 9216


# ------------------------------------------------------------------------------------------------- the division
def _plane_sizes_up_to_8192():
    sides = [4, 5, 7, 8, 12, 16, 24, 36, 40, 100, 148, 255, 256, 640, 1032, 2064, 4095, 4096, 8191, 8192]
    return sorted({a * b for a in sides for b in sides})


def test_division_against_python():
    from hvqm4_amd import scale
    rnd = random.Random(26)
    ds = _plane_sizes_up_to_8192()
    assert ds[0] == 16 and ds[-1] == 1 << 26
    for d in ds + [rnd.randrange(16, 1 << 26) for _ in range(300)]:
        m = scale.magic(d)
        assert m == -(-(1 << 64) // d) and m < 1 << 64
        h = d >> 1
        for k in list(range(0, 258)):
            for s in (k * d - 1, k * d, k * d + h - 1, k * d + h):
                if 0 <= s < 1 << 35:
                    assert scale.divide(s, d) == s // d, (s, d)
        for _ in range(40):
            s = rnd.randrange(0, 255 * d + 1) + h                       # what the kernel divides: S + (D >> 1)
            assert scale.divide(s, d) == s // d, (s, d)
    for d in (1, 0, (1 << 26) + 1):
        with pytest.raises(ValueError):
            scale.magic(d)


DIV_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "hvq_scale.h"
int main(int argc, char **argv)
{
    unsigned long long bad = 0, n = 0;
    for (int i = 1; i < argc; ++i) {
        const uint64_t d = strtoull(argv[i], nullptr, 10), h = d >> 1, m = hvq_sc_magic(d);
        for (uint64_t k = 0; k < 258; ++k) {
            const uint64_t at[4] = { k * d - 1, k * d, k * d + h - 1, k * d + h };
            for (uint64_t s : at) if (s < (1ull << 35)) { ++n; bad += hvq_sc_div(s, m) != s / d; }
        }
        uint64_t x = d * 0x9E3779B97F4A7C15ull + 1;
        for (int r = 0; r < 2000; ++r) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            const uint64_t s = x % (255 * d + 1) + h;
            ++n; bad += hvq_sc_div(s, m) != s / d;
        }
    }
    printf("%llu %llu\n", bad, n);
    return bad != 0;
}
"""


def test_division_in_c(tmp_path):
    """hvq_sc_magic / hvq_sc_div of hvq_scale.h, what the runtime and the fake device compile (the kernel has __umul64hi in the place of
    the 128-bit product): a stand-alone program, plain and sanitised"""
    src = tmp_path / "div.cpp"
    src.write_text(DIV_PROGRAM)
    ds = [str(d) for d in _plane_sizes_up_to_8192()]
    for kind, flags in fd.BUILDS.items():
        exe = str(tmp_path / ("div_" + kind))
        subprocess.run(["g++", "-std=c++17", "-O1", "-I" + fd.CSRC] + flags + [str(src), "-o", exe], check=True)
        r = subprocess.run([exe] + ds, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0 and not r.stderr, (kind, r.stdout, r.stderr[-2000:])
        bad, n = (int(v) for v in r.stdout.split())
        assert bad == 0 and n > 1000 * len(ds)


INDEX_PROGRAM = r"""
#include <cstdio>
#include <initializer_list>
#include "hvq_scale.h"
int main()
{
    unsigned long long bad = 0, n = 0;
    for (uint32_t m = 1; m <= 8192; ++m) {
        uint32_t mul, shift;
        hvq_sc_divisor(m, &mul, &shift);
        /* every multiple of m below 2^27 and the value before it when m is a plane's width or height (a multiple of 4); 4096 of them
           spread over the range otherwise; and the largest dividend */
        const uint32_t top = (1u << HVQ_SC_DIV_BITS) - 1u, step = (m & 3u) ? (top / m / 4096u + 1u) : 1u;
        for (uint32_t k = 1; k <= top / m; k += step) {
            n += 2;
            bad += hvq_sc_divm(k * m, mul, shift) != k;
            bad += hvq_sc_divm(k * m - 1u, mul, shift) != k - 1u;
        }
        ++n; bad += hvq_sc_divm(top, mul, shift) != top / m;
        /* the first and the last source of every target of m from 8192 and from a ragged n */
        if (!(m & 3u))
            for (uint32_t nn : { 8192u, 8191u, m, 5u * m + 3u > 8192u ? 37u : 5u * m + 3u })
                for (uint32_t r = 0; r < m; ++r) {
                    n += 2;
                    bad += hvq_sc_first(nn, m, r, mul, shift) != nn * r / m;
                    bad += hvq_sc_end(nn, m, r, mul, shift) != (nn * (r + 1u) + m - 1u) / m;
                }
    }
    printf("%llu %llu\n", bad, n);
    return bad != 0;
}
"""


def test_index_division_in_c(tmp_path):
    """hvq_sc_divisor / hvq_sc_divm of hvq_scale.h: the multiplication and shift in the place of n r / m, for every m up to 8192"""
    src = tmp_path / "index.cpp"
    src.write_text(INDEX_PROGRAM)
    for kind, flags in fd.BUILDS.items():
        exe = str(tmp_path / ("index_" + kind))
        subprocess.run(["g++", "-std=c++17", "-O2", "-I" + fd.CSRC] + flags + [str(src), "-o", exe], check=True)
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0 and not r.stderr, (kind, r.stdout, r.stderr[-2000:])
        bad, n = (int(v) for v in r.stdout.split())
        assert bad == 0 and n > 100_000_000


# ------------------------------------------------------------------------------------------------- the fixture
def _clip_geometry(name):
    from hvqm4_amd.container import parse_header
    hdr = parse_header(open(os.path.join(fd.GOLDEN, fd.CLIPS[name]["file"]), "rb").read())
    return (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)


def test_fixture_covers_every_golden_clip():
    from hvqm4_amd import scale
    assert set(FIXTURE["clips"]) == set(fd.CLIPS)
    labels = set()
    for name, entry in FIXTURE["clips"].items():
        g = tuple(entry["geometry"])
        assert g == _clip_geometry(name)
        want = [("half", scale.pyramid(g[0], g[1], 2)[1] + g[2:]), ("fit56", scale.fit(g[0], g[1], 56, 56) + g[2:])] + ([("to420", g[:2] + (2, 2))] if g[2:] != (2, 2) else [])
        assert [(l, tuple(d)) for l, d, _c in entry["targets"]] == want, name
        for _l, d, _c in entry["targets"]:
            assert all(nx <= 32 * mx and ny <= 32 * my for nx, ny, mx, my in scale.plane_sizes(g, tuple(d))), "the 32x limit"
        labels |= {l for l, _d, _c in entry["targets"]}
    assert labels == {"half", "fit56", "to420"}


@pytest.mark.parametrize("name", sorted(FIXTURE["clips"]))
def test_fixture_equals_reference_and_module(name):
    from hvqm4_amd import scale
    entry = FIXTURE["clips"][name]
    g = tuple(entry["geometry"])
    pic = fd.oracle_pictures(name)[-1]
    assert hashlib.sha256(pic.tobytes()).hexdigest() == fd.CLIPS[name]["picture_sha256"][-1], "the fixture describes the manifest's picture"
    for label, dst, crc in entry["targets"]:
        got = scale.of_picture(pic, g, tuple(dst))
        assert zlib.crc32(got.tobytes()) == crc, (name, label)
        assert ref.scale_picture(pic.tobytes(), g, tuple(dst)) == got.tobytes(), (name, label)


# ------------------------------------------------------------------------------------------------- argument checks without a device
class _NoDevice:
    """what Context.scale_pictures looks at before it reaches the library"""
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


class _Wide(_NoDevice):
    _geom = {0: (520, 8)}

    @staticmethod
    def pic_bytes(sid):
        return 520 * 8 * 3 // 2


def test_arguments_are_checked_before_the_library_is_called():
    import torch
    from hvqm4_amd._lib import HVQ_E_ARG, HvqError
    from hvqm4_amd.batch import Context
    call = lambda *a, **k: Context.scale_pictures(_NoDevice(), *a, **k)
    assert _NoDevice()._geometry(0) == (64, 48, 2, 2) and _NoDevice()._geometry(2) == (64, 48, 1, 1)
    with pytest.raises(ValueError, match="ordinals"):
        call([0, 0], [0], (32, 24))
    with pytest.raises(HvqError) as e:
        call([0, 7], [0, 0], (32, 24))
    assert e.value.code == HVQ_E_ARG
    for size in (None, (32,), [(32, 24)], (32, 24, 8), "32x24", [(32, 24), None]):
        with pytest.raises(ValueError, match="size"):
            call([0, 0], [0, 1], size)
    for size in ((36, 24), (32, 0), (8200, 24)):
        with pytest.raises(ValueError, match="multiples of 8"):
            call([0], [0], size)
    with pytest.raises(ValueError, match="samplings"):
        call([0], [0], (32, 24), sampling=(1, 2))
    with pytest.raises(ValueError, match="sampling"):
        call([0], [0], (32, 24), sampling=(2, 2, 2))
    for crop in ((1, 0, 32, 16), (0, 0, 32, 15), (0, 0, 6, 16), (40, 0, 32, 16), (0, 0, 0, 0), (-2, 0, 16, 16)):
        with pytest.raises(ValueError, match="crop"):
            call([0], [0], (32, 24), crop=crop)
    with pytest.raises(ValueError, match="crop"):
        call([0], [0], (32, 24), crop=(0, 0, 16))
    with pytest.raises(ValueError, match="beyond 32"):
        Context.scale_pictures(_Wide(), [0], [0], (16, 8))
    with pytest.raises(ValueError, match="not a GPU"):                      # 512 of the 520 samples: at the limit, and on to the next check
        Context.scale_pictures(_Wide(), [0], [0], (16, 8), crop=(0, 0, 512, 8), out=torch.zeros((1, 16 * 8 * 3 // 2), dtype=torch.uint8))
    with pytest.raises(ValueError, match="1 sources for 2 pictures"):
        call([0, 0], [0, 1], (32, 24), src=[None])
    good = torch.zeros(64 * 48 * 3 // 2, dtype=torch.uint8)
    with pytest.raises(ValueError, match="elements"):
        call([1], [-1], (32, 24), src=[good])
    with pytest.raises(ValueError, match="ordinal -1"):
        room = torch.zeros(64 * 48 * 3 // 2 + 64, dtype=torch.uint8)
        off = (-room.data_ptr()) % 16
        call([0], [0], (32, 24), src=[room[off:off + good.numel()]])
    with pytest.raises(ValueError, match="not a GPU"):
        call([0], [-1], (32, 24), src=[room[off:off + good.numel()]])
    nb = 32 * 24 * 3 // 2
    with pytest.raises(ValueError, match="out must be"):
        call([0, 0], [0, 1], (32, 24), out=torch.zeros((2, nb), dtype=torch.int32))
    with pytest.raises(ValueError, match="out must be"):
        call([0, 0], [0, 1], (32, 24), out=torch.zeros((2, nb + 16), dtype=torch.uint8))
    with pytest.raises(ValueError, match="out must be"):
        call([0, 0], [0, 1], (32, 24), out=[torch.zeros(nb, dtype=torch.uint8)] * 2)                    # one geometry: one tensor
    with pytest.raises(ValueError, match="out must be a list"):
        call([0, 0], [0, 1], [(32, 24), (16, 16)], out=torch.zeros((2, nb), dtype=torch.uint8))         # two geometries: a list
    with pytest.raises(ValueError, match=r"out\[1\]"):
        call([0, 0], [0, 1], [(32, 24), (16, 16)], out=[torch.zeros(nb, dtype=torch.uint8)] * 2)
    with pytest.raises(ValueError, match="multiple of 16"):
        room = torch.zeros(2 * nb + 64, dtype=torch.uint8)
        off = (-room.data_ptr()) % 16 + 8
        call([0, 0], [0, 1], (32, 24), out=room[off:off + 2 * nb].view(2, nb))
    with pytest.raises(ValueError, match="not a GPU"):
        call([0, 0], [0, 1], (32, 24), out=torch.zeros((2, nb), dtype=torch.uint8))
    with pytest.raises(ValueError, match="not a GPU"):
        call([0, 0], [0, 1], [(32, 24), (16, 16)], sampling=[None, (1, 1)], out=[torch.zeros(nb, dtype=torch.uint8), torch.zeros(16 * 16 * 3, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="65535"):
        call([0] * 65536, [0] * 65536, (32, 24))


def test_the_library_without_a_device_still_checks_its_arguments():
    """no context can exist here, and the calls say so before they look at anything else; the host-only entry points work"""
    import ctypes as C
    from hvqm4_amd import scale
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_GEOMETRY, HvqError, HvqScaleDst, lib
    one = (C.c_int * 1)(0)
    dst = (HvqScaleDst * 1)(HvqScaleDst(16, 32, 24, 2, 2, 0, 0, 0, 0))
    assert lib().hvq_scale_pictures(None, 1, one, one, None, C.cast(dst, C.c_void_p), None) == HVQ_E_ARG
    assert lib().hvq_scale_force_direct(None, 1) == HVQ_E_ARG
    assert C.sizeof(HvqScaleDst) == 40
    for w, h, hs, vs in ((64, 48, 2, 2), (64, 48, 2, 1), (64, 48, 1, 1), (8, 8, 2, 2), (8192, 8192, 1, 1)):
        assert lib().hvq_scale_bytes(w, h, hs, vs) == scale.nbytes(w, h, hs, vs)
    for w, h, hs, vs in ((60, 48, 2, 2), (64, 48, 1, 2), (0, 48, 2, 2), (8200, 48, 2, 2)):
        assert lib().hvq_scale_bytes(w, h, hs, vs) == HVQ_E_GEOMETRY
    assert scale.body(64, 48, 64, 48) == scale.DIRECT and scale.body(16, 16, 40, 24) == scale.DIRECT and scale.body(64, 48, 64, 104) == scale.DIRECT
    assert scale.body(64, 48, 32, 24) == scale.TILED and scale.body(128, 8, 56, 264) == scale.TILED and scale.body(256, 256, 8, 8) == scale.TILED
    for bad in ((264, 256, 8, 8), (256, 264, 8, 8), (0, 8, 8, 8), (8, 8, 8, 8193)):
        with pytest.raises(HvqError):
            scale.body(*bad)


# ------------------------------------------------------------------------------------------------- the runtime on the CPU fake device
@pytest.fixture(scope="module")
def drivers():
    return {kind: fd.build_driver(kind, "scale", "fake_scale_driver", CXX_SOURCES, __file__) for kind in fd.BUILDS}


_want = {}


def _source(source, form, k, geom):
    """the picture the driver scaled, as the driver's line describes it"""
    from hvqm4_amd import scale
    n = scale.nbytes(*geom)
    if form == "pic":
        return fd.oracle_pictures(source)[k].reshape(-1)
    if form == "inv":
        return 255 - fd.oracle_pictures(source)[k].reshape(-1)
    if form == "synth":
        return ((((np.arange(n, dtype=np.uint64) + np.uint64(k)) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(13)).astype(np.uint8)
    if form == "flat":
        return np.full(n, k, dtype=np.uint8)
    if form == "tie":
        i = np.arange(n)
        return np.where((i % geom[0] & 1) & (i // geom[0] & 1), k, 0).astype(np.uint8)
    raise AssertionError(form)


def _expected(source, form, k, sg, dg, crop):
    from hvqm4_amd import scale
    key = (source, form, k, sg, dg, crop)
    if key not in _want:
        if form == "scaled":                                       # picture k of the clip scaled to sg by an earlier call
            src = _expected(source, "pic", k, _clip_geometry(source), sg, None)[1]
        else:
            src = _source(source, form, k, sg)
        got = scale.of_picture(src, sg, dg, crop)
        _want[key] = (zlib.crc32(got.tobytes()), got)
    return _want[key]


def _run(exe, scenario, schedule, tmp_path):
    _, lines = fd.run_checked(exe, scenario, schedule, tmp_path)
    P, R, S = {}, {}, {}
    for line in lines:
        f = line.split()
        if f[0] == "P":
            label, source, form, k = f[1], f[2], f[3], int(f[4])
            sg, dg, crop = tuple(int(v) for v in f[5:9]), tuple(int(v) for v in f[9:13]), tuple(int(v) for v in f[13:17])
            crop = None if crop == (0, 0, 0, 0) else crop
            assert int(f[18]) == 1, f"{label}: the bytes behind the output of {source} {k} were written"
            want = _expected(source, form, k, sg, dg, crop)[0]
            assert int(f[17]) == want, f"{label}: picture {k} of {source} ({form}) {sg} -> {dg} crop {crop}: crc {int(f[17]):08x}, want {want:08x}"
            P.setdefault(label, []).append((source, form, k, sg, dg, crop))
        elif f[0] == "R":
            R[f[1]] = int(f[2])
        elif f[0] == "S":
            S[f[1]] = (int(f[2]), int(f[3]))
    return P, R, S


def _shapes_seen(items):
    from hvqm4_amd import scale
    sizes = [s for _src, _f, _k, sg, dg, crop in items for s in scale.plane_sizes(sg, dg, crop)]
    return {"identity": any(nx == mx and ny == my for nx, ny, mx, my in sizes), "integer": any(nx == 2 * mx and ny == 2 * my for nx, ny, mx, my in sizes),
            "noninteger": any(nx > mx and nx % mx for nx, ny, mx, my in sizes), "enlarge": any(nx < mx and ny < my for nx, ny, mx, my in sizes),
            "mixed": any(nx == mx and ny < my for nx, ny, mx, my in sizes), "seams": any(mx > 64 and my > 16 and nx % mx for nx, ny, mx, my in sizes),
            "crop": any(crop for *_r, crop in items), "sampling": any(sg[2:] != dg[2:] for _s, _f, _k, sg, dg, _c in items)}


def _check_goldens(P, R, S):
    assert len(P["goldens/all"]) == 25 and all(_shapes_seen(P["goldens/all"]).values()), _shapes_seen(P["goldens/all"])
    assert {sg[2:] for _s, _f, _k, sg, dg, _c in P["goldens/all"] if sg == dg} == {(2, 2), (2, 1), (1, 1)}, "identity in every sampling"
    assert P["goldens/one"] == [P["goldens/all"][7]]
    assert R == {"goldens/n0": 0}


def _check_memory(P, R, S):
    assert P["memory"] == P["memory/nullstream"] and len(P["memory"]) == 2 * fd.n_pics("yuv422_64x48") + 6
    forms = [f for _s, f, *_r in P["memory"]]
    assert forms.count("inv") == fd.n_pics("yuv422_64x48") + 1 and forms.count("tie") == 2 and forms.count("synth") == 2 and forms.count("flat") == 1
    tie = {k: _expected("synth", "tie", k, (16, 16, 1, 1), (8, 8, 1, 1), None)[1] for k in (1, 2)}
    assert (tie[2] == 1).all() and (tie[1] == 0).all()
    assert ("synth", "synth", 7, (256, 256, 2, 2), (8, 8, 2, 2), None) in P["memory"], "the 32x limit"


def _check_cells64(P, R, S):
    assert [(f, k) for _s, f, k, *_r in P["cells64"]] == [("synth", 64), ("flat", 255)]
    assert all(sg == (8192, 2064, 2, 2) and dg == (256, 72, 2, 2) for _s, _f, _k, sg, dg, _c in P["cells64"]) and 255 * 8192 * 2064 > 1 << 32
    assert (_expected("synth", "flat", 255, (8192, 2064, 2, 2), (256, 72, 2, 2), None)[1] == 255).all()


def _check_many(P, R, S):
    assert len(P["many"]) == 300 and P["many"] == P["many/again"]
    assert len({s for s, *_r in P["many"]}) == 8 and len({dg for *_r, dg, _c in P["many"]}) > 15 and sum(1 for *_r, c in P["many"] if c) >= 50
    assert all(_shapes_seen(P["many"])[k] for k in ("identity", "noninteger", "enlarge", "crop", "sampling", "seams"))


def _check_body(P, R, S):
    from hvqm4_amd import scale
    from hvqm4_amd._lib import HVQ_E_ARG
    assert P["body/chosen"] == P["body/direct"] == P["body/chosen_again"] and len(P["body/direct"]) == 26
    assert R == {"body/force": 0, "body/unforce": 1, "body/tiled": scale.TILED, "body/identity": scale.DIRECT, "body/enlarge": scale.DIRECT, "body/beyond": HVQ_E_ARG}
    assert P["body/direct"][-1][3:5] == ((256, 256, 2, 2), (8, 8, 2, 2)), "the forced direct body at the 32x limit"


def _check_reuse(P, R, S):
    from hvqm4_amd._lib import HVQ_E_STATE
    n, ne = fd.n_pics("gop64x48_15"), fd.n_pics("yuv444_64x48")
    g = _clip_geometry("gop64x48_15")
    assert P["reuse"] == [("gop64x48_15", "pic", k, g, (40, 24, 2, 2), None) for k in range(n)]
    assert R["reuse/evicted"] == HVQ_E_STATE, "the flushes did not hand the slots of the first pass on: the scenario tests nothing"
    assert P["reuse/chain"] == [("gop64x48_15", "scaled", k, (40, 24, 2, 2), (16, 16, 1, 1), None) for k in range(n)]
    assert P["reuse/late"] == P["reuse"]
    assert [(s, k) for s, _f, k, *_r in P["reuse/destroy"]] == [("yuv444_64x48", k) for k in range(ne)]


def _check_refused(P, R, S):
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_GEOMETRY, HVQ_E_STATE
    arg = ["null_context", "bad_stream", "bad_ordinal", "misaligned_src", "src_with_ordinal", "src_with_bad_stream", "minus_one_without_src", "null_ptr",
           "misaligned_ptr", "too_many", "beyond_32", "crop_empty", "crop_w0_with_offset", "crop_leaves_right", "crop_leaves_bottom", "crop_negative", "crop_odd_x",
           "crop_odd_h", "crop_narrow", "crop_low", "force_null"]
    want = {k: HVQ_E_ARG for k in arg}
    want.update({"geometry_width": HVQ_E_GEOMETRY, "geometry_sampling": HVQ_E_GEOMETRY, "bytes_geometry": HVQ_E_GEOMETRY, "evicted": HVQ_E_STATE, "queued": HVQ_E_STATE, "n0": 0})
    assert R == {"refused/" + k: v for k, v in want.items()}
    same, total = S["refused"]
    assert same == total == 2 * 1152 + 16, "a refused call wrote its output"
    g = _clip_geometry("gop64x48_15")
    assert P["refused/then_ok"] == [("gop64x48_15", "pic", 1, g, (32, 24, 2, 2), None), ("gop64x48_15", "pic", fd.n_pics("gop64x48_15") - 1, g, (32, 24, 2, 2), None)]


CHECKS = {"goldens": _check_goldens, "memory": _check_memory, "cells64": _check_cells64, "many": _check_many, "body": _check_body, "reuse": _check_reuse,
          "refused": _check_refused}


@pytest.mark.parametrize("schedule", ["eager", "late"])
@pytest.mark.parametrize("build", list(fd.BUILDS))
@pytest.mark.parametrize("scenario", list(CHECKS))
def test_fake_device_scenario(drivers, scenario, build, schedule, tmp_path):
    P, R, S = _run(drivers[build], scenario, schedule, tmp_path)
    CHECKS[scenario](P, R, S)


def test_the_existing_fake_builds_link_without_the_scale_body():
    """the source lists of the other drivers have no hvq_launch_scale: the runtime's reference is weak"""
    assert not any("fake_scale" in s for s in fd.CXX_SOURCES)
    text = open(os.path.join(fd.CSRC, "hvq_runtime.cpp")).read()
    decl = [l for l in text.splitlines() if "hvq_launch_scale(" in l and l.startswith("extern")]
    assert len(decl) == 1 and "weak" in decl[0]
