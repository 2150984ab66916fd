"""CPU: picture checksums (hvq_picture_checksums, Context.picture_checksums, hvqm4_amd/checksums.py) without a GPU.

  - tests/checksums_ref.py, the host restatement the GPU tests compare with, on a picture whose Adler values can be worked out by hand;
  - the combine helpers of the library against zlib on random splits, and beyond 2^32 bytes against the pure-Python ones;
  - tests/golden/checksums.json against checksums_ref on the oracle's pictures of every golden clip, whose SHA-256 are manifest.json's:
    the new fixture describes the pictures the old one does;
  - the argument checks of Context.picture_checksums that need no device;
  - the runtime's entry point linked UNCHANGED against the CPU fake device of tests/test_fake_device.py (its source lists and flags, with
    tests/native/fake_checksums_driver.cpp in the place of fake_driver.cpp and tests/native/fake_checksums.cpp added: a scalar body for
    hvq_launch_checksums that reaches memory only through fake_span, when it runs), under both schedules, plain and as a stand-alone
    AddressSanitizer + UndefinedBehaviorSanitizer program.  The driver judges nothing: every record it read back is compared here with
    checksums_ref on the oracle's pictures.
"""
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

import tests.test_fake_device as fd
from tests.checksums_ref import adler32_combine, checksums_reference, crc32_combine, plane_sizes

NATIVE = fd.NATIVE
CXX_SOURCES = [s for s in fd.CXX_SOURCES if os.path.basename(s) != "fake_driver.cpp"] + \
              [os.path.join(NATIVE, "fake_checksums.cpp"), os.path.join(NATIVE, "fake_checksums_driver.cpp")]
SIX = ["gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8"]
FIXTURE = json.load(open(os.path.join(fd.GOLDEN, "checksums.json")))


# ------------------------------------------------------------------------------------------------- the reference and the helpers
def test_reference_on_a_picture_worked_out_by_hand():
    # 8 x 8, 4:2:0: Y 64 samples of 1; U 16 samples of 0; V 0, 0, ..., 0, 255
    a = np.concatenate([np.full(64, 1), np.zeros(16), np.zeros(15), [255]]).astype(np.uint8)
    got = checksums_reference(a, 8, 8, 2, 2)
    assert got.dtype == np.int64 and got.shape == (8,)
    # Adler: lo = 1 + sum, hi = L + sum (L - i) d_i.  Y: 1 + 64, 64 + (64 + 63 + ... + 1); U: 1, 16; V: 1 + 255, 16 + 1 * 255
    assert got[4] == (64 + 64 * 65 // 2) << 16 | 65
    assert got[5] == 16 << 16 | 1
    assert got[6] == (16 + 255) << 16 | 256
    # the picture: lo = 1 + 64 + 255; hi = 96 + sum over Y of (96 - i) + 1 * 255
    assert got[7] == (96 + sum(96 - i for i in range(64)) + 255) << 16 | 320
    assert got[:4].tolist() == [zlib.crc32(bytes([1] * 64)), zlib.crc32(bytes(16)), zlib.crc32(bytes(15) + b"\xff"), zlib.crc32(a.tobytes())]
    assert got[1] == 0xECBB4B55                                  # crc32 of 16 zero bytes: the length-dependent term alone
    assert plane_sizes(16, 8, 2, 1) == (128, 64, 64) and plane_sizes(16, 8, 1, 1) == (128, 128, 128)
    # 4:2:2: U starts right behind Y
    b = np.zeros(256, dtype=np.uint8)
    b[128] = 7
    r = checksums_reference(b, 16, 8, 2, 1)
    assert r[5] == (64 + 64 * 7) << 16 | 8 and r[4] == 128 << 16 | 1 and r[6] == 64 << 16 | 1


def test_of_bytes_and_the_formatter():
    from hvqm4_amd import checksums as ck
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, 24 * 40 * 3 // 2, dtype=np.uint8)
    assert ck.of_bytes(a, 24, 40) == checksums_reference(a, 24, 40, 2, 2).tolist() == ck.of_bytes(a.tobytes(), 24, 40, 2, 2)
    assert ck.plane_bytes(640, 480) == (307200, 76800, 76800) and ck.plane_bytes(24, 40, 1, 1) == (960, 960, 960)
    assert (ck.CRC32_Y, ck.CRC32_U, ck.CRC32_V, ck.CRC32_PICTURE, ck.ADLER32_Y, ck.ADLER32_U, ck.ADLER32_V, ck.ADLER32_PICTURE) == tuple(range(8))
    with pytest.raises(ValueError):
        ck.of_bytes(a[:-1], 24, 40)
    with pytest.raises(ValueError):
        ck.plane_bytes(24, 40, 3, 1)
    lines = ck.framecrc_lines([0, 1], ["I", "P"], [[0, 1, 2, 3, 4, 5, 6, 0xFFFFFFFF], list(range(8, 16))])
    assert lines[0] == "     0 I 00000000 00000001 00000002 00000003 00000004 00000005 00000006 ffffffff"
    assert lines[1].split() == ["1", "P"] + [f"{v:08x}" for v in range(8, 16)]
    with pytest.raises(ValueError):
        ck.framecrc_lines([0], ["I"], [[1 << 32] + [0] * 7])


def test_combine_helpers_against_zlib_on_random_splits():
    from hvqm4_amd import checksums as ck
    rng = np.random.default_rng(11)
    data = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    cuts = [0, 1, 2, 15, 16, 17, 960, 1440, 4608, 65520, 65521, 65522, len(data) - 1, len(data)] + rng.integers(0, len(data), 12).tolist()
    for cut in cuts:                                             # len_b = len(data) - cut: 0 and 1 are among them
        a, b = data[:cut], data[cut:]
        for combine in (ck.crc32_combine, crc32_combine):
            assert combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(data), (cut, combine)
        for combine in (ck.adler32_combine, adler32_combine):
            assert combine(zlib.adler32(a), zlib.adler32(b), len(b)) == zlib.adler32(data), (cut, combine)
    # full-scale halves: planes of 0xFF
    ff = b"\xff" * 76800
    assert ck.adler32_combine(zlib.adler32(ff), zlib.adler32(ff), len(ff)) == zlib.adler32(ff + ff)
    assert ck.crc32_combine(zlib.crc32(ff), zlib.crc32(ff), len(ff)) == zlib.crc32(ff + ff)


def _zeros(nbytes):
    """(crc32, adler32) of `nbytes` zero bytes without hashing them: blocks of 2^j bytes, from zlib up to 2^16 and from doubling with the
    pure-Python combine beyond, joined along the bits of nbytes"""
    c, a = 0, 1                                                  # of no bytes
    bc, ba = zlib.crc32(b"\0"), zlib.adler32(b"\0")
    for j in range(nbytes.bit_length()):
        if j <= 16:
            bc, ba = zlib.crc32(bytes(1 << j)), zlib.adler32(bytes(1 << j))
        else:
            bc, ba = crc32_combine(bc, bc, 1 << (j - 1)), adler32_combine(ba, ba, 1 << (j - 1))
        if (nbytes >> j) & 1:
            c, a = crc32_combine(c, bc, 1 << j), adler32_combine(a, ba, 1 << j)
    return c, a


def test_combine_helpers_beyond_4_gib():
    """no buffer of that size is hashed: B is a run of zero bytes whose checksums come from zlib's at 2^16 bytes by doubling.  The library
    must agree with pure Python, and the result must not depend on where A | B | C is split"""
    from hvqm4_amd import checksums as ck
    assert _zeros(70001) == (zlib.crc32(bytes(70001)), zlib.adler32(bytes(70001))) and _zeros(0) == (0, 1)
    head, tail = b"hvqm4 pictures", b"are bit-exact"
    hc, ha, tc, ta = zlib.crc32(head), zlib.adler32(head), zlib.crc32(tail), zlib.adler32(tail)
    for big in ((1 << 32) + 12345, 1 << 33, (1 << 33) + 1, (1 << 40) + 65521):
        bc, ba = _zeros(big)
        assert ba == (big % 65521) << 16 | 1                     # zeros: lo stays 1, hi counts the bytes
        assert ck.crc32_combine(hc, bc, big) == crc32_combine(hc, bc, big) and ck.adler32_combine(ha, ba, big) == adler32_combine(ha, ba, big), big
        left_c = ck.crc32_combine(ck.crc32_combine(hc, bc, big), tc, len(tail))
        right_c = ck.crc32_combine(hc, ck.crc32_combine(bc, tc, len(tail)), big + len(tail))
        assert left_c == right_c == crc32_combine(crc32_combine(hc, bc, big), tc, len(tail)), big
        left_a = ck.adler32_combine(ck.adler32_combine(ha, ba, big), ta, len(tail))
        right_a = ck.adler32_combine(ha, ck.adler32_combine(ba, ta, len(tail)), big + len(tail))
        assert left_a == right_a == adler32_combine(adler32_combine(ha, ba, big), ta, len(tail)), big
    with pytest.raises(ValueError):
        ck.crc32_combine(0, 0, -1)


# ------------------------------------------------------------------------------------------------- the fixture
def _geometry(name):
    from hvqm4_amd.container import parse_header
    hdr = parse_header(open(os.path.join(fd.GOLDEN, fd.CLIPS[name]["file"]), "rb").read())
    return hdr.width, hdr.height, hdr.h_samp, hdr.v_samp


_want = {}


def _expected(name, k, form="pic"):
    key = (name, k, form)
    if key not in _want:
        a = fd.oracle_pictures(name)[k]
        _want[key] = checksums_reference(255 - a if form == "inv" else a, *_geometry(name)).tolist()
    return _want[key]


def test_fixture_equals_the_reference_on_the_oracles_pictures_of_every_golden_clip():
    assert set(FIXTURE["clips"]) == set(fd.MANIFEST["clips"]), "one entry per clip of manifest.json"
    assert len(fd.CLIPS) >= 30
    for name, c in fd.MANIFEST["clips"].items():
        rows = FIXTURE["clips"][name]
        assert len(rows) == len(c["frame_types"]) and all(len(r) == 8 and all(0 <= v < 1 << 32 for v in r) for r in rows), name
    for name, c in fd.CLIPS.items():
        pics = fd.oracle_pictures(name)
        assert [hashlib.sha256(p.tobytes()).hexdigest() for p in pics] == c["picture_sha256"], name
        assert FIXTURE["clips"][name] == [_expected(name, k) for k in range(len(pics))], name


# ------------------------------------------------------------------------------------------------- argument checks without a device
class _NoDevice:
    """what Context.picture_checksums looks at before it reaches the library"""
    _geom = {0: (64, 48), 1: (24, 40)}
    _h = None

    @staticmethod
    def pic_bytes(sid):
        return {0: 64 * 48 * 3 // 2, 1: 24 * 40 * 3 // 2}[sid]


def test_sources_are_checked_before_the_library_is_called():
    import torch
    from hvqm4_amd._lib import HVQ_E_ARG, HvqError
    from hvqm4_amd.batch import Context
    from hvqm4_amd.checksums import sources
    call = lambda *a, **k: Context.picture_checksums(_NoDevice(), *a, **k)
    with pytest.raises(ValueError, match="ordinals"):
        call([0, 0], [0])
    with pytest.raises(HvqError) as e:
        call([0, 7], [0, 0])
    assert e.value.code == HVQ_E_ARG
    with pytest.raises(ValueError, match="1 sources for 2 pictures"):
        call([0, 0], [0, 1], src=[None])
    with pytest.raises(TypeError):
        call([0], [0], src="memory")
    with pytest.raises(TypeError):
        call([0], [-1], src=[(0, 1)])
    good = torch.zeros(64 * 48 * 3 // 2, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        call([0], [-1], src=[good.to(torch.int8)])
    with pytest.raises(ValueError, match="elements"):
        call([1], [-1], src=[good])                                       # the bytes of stream 0's pictures for one of stream 1
    with pytest.raises(ValueError, match="contiguous"):
        call([0], [-1], src=[torch.zeros(64 * 48 * 3, dtype=torch.uint8)[::2]])
    room = torch.zeros(64 * 48 * 3 // 2 + 64, dtype=torch.uint8)
    off = (-room.data_ptr()) % 16
    with pytest.raises(ValueError, match="ordinal -1"):
        call([0], [0], src=[room[off:off + good.numel()]])
    with pytest.raises(ValueError, match="multiple of 16"):
        call([0], [-1], src=[room[off + 8:off + 8 + good.numel()]])
    with pytest.raises(ValueError, match="not a GPU"):                    # the device is checked last
        call([0], [-1], src=[room[off:off + good.numel()]])
    with pytest.raises(ValueError, match="out must be"):
        call([0], [0], out=torch.zeros((1, 8), dtype=torch.int32))
    with pytest.raises(ValueError, match="out must be"):
        call([0], [0], out=torch.zeros((2, 8), dtype=torch.int64))
    with pytest.raises(ValueError, match="not a GPU"):
        call([0], [0], out=torch.zeros((1, 8), dtype=torch.int64))
    assert sources(None, [0, 1, 2], _NoDevice.pic_bytes) is None
    assert sources([None, None], [3, 4], _NoDevice.pic_bytes) == [None, None]


def test_the_library_without_a_device_still_checks_its_arguments():
    """no context can exist here, and the call says so before it looks at anything else"""
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, lib
    one = (C.c_int * 1)(0)
    assert lib().hvq_picture_checksums(None, 1, one, one, None, None, None) == HVQ_E_ARG


# ------------------------------------------------------------------------------------------------- the runtime on the CPU fake device
@pytest.fixture(scope="module")
def drivers():
    return {kind: fd.build_driver(kind, "checksums", "fake_checksums_driver", CXX_SOURCES, __file__) for kind in fd.BUILDS}


def _run(exe, scenario, schedule, tmp_path):
    _, lines = fd.run_checked(exe, scenario, schedule, tmp_path)
    K, R, S = {}, {}, {}
    for line in lines:
        f = line.split()
        if f[0] == "C":
            label, name, k, form = f[1], f[2], int(f[3]), f[4]
            got = [int(v) for v in f[5:]]
            want = _expected(name, k, form)
            assert got == want, f"{label}: picture {k} of {name} ({form}):\n{got}\nwant\n{want}"
            K.setdefault(label, []).append((name, k, form))
        elif f[0] == "R":
            R[f[1]] = int(f[2])
        elif f[0] == "S":
            S[f[1]] = (int(f[2]), int(f[3]))
    return K, R, S, fd.refusal_texts(lines)


def _check_goldens(K, R, S, E):
    n = {nm: fd.n_pics(nm) for nm in SIX}
    assert len({_geometry(nm)[2:] for nm in SIX}) == 3                    # 4:2:0, 4:2:2 and 4:4:4
    assert K["goldens/clip"] == [(nm, k, "pic") for nm in SIX for k in range(n[nm])]
    assert K["goldens/clip"] and all(FIXTURE["clips"][nm][k] == _expected(nm, k) for nm, k, _f in K["goldens/clip"])
    assert K["goldens/mixed"] == [(nm, (r * 3 + 1) % n[nm], "pic") for r in range(2) for nm in SIX], "records come back in call order"
    assert K["goldens/one"] == [("yuv422_296x160", 1, "pic")]
    assert R == {"goldens/n0": 0}


def _check_memory(K, R, S, E):
    na = fd.n_pics("yuv422_64x48")
    want = [x for k in range(na) for x in (("yuv422_64x48", k, "inv"), ("yuv422_64x48", k, "pic"))] + [("ragged24x40", 1, "inv"), ("ragged24x40", 1, "pic")]
    assert K["memory"] == want and K["memory/nullstream"] == want


def _check_reuse(K, R, S, E):
    from hvqm4_amd._lib import HVQ_E_STATE
    n, ne = fd.n_pics("gop64x48_15"), fd.n_pics("yuv444_64x48")
    assert K["reuse"] == [("gop64x48_15", k, "pic") for k in range(n)]
    assert R["reuse/evicted"] == HVQ_E_STATE, "the flushes did not hand the slots of the first pass on: the scenario tests nothing"
    assert K["reuse/late"] == [("gop64x48_15", k, "pic") for k in range(n)]
    assert K["reuse/destroy"] == [("yuv444_64x48", k, "pic") for k in range(ne)]


def _check_backtoback(K, R, S, E):
    small = [("wide296x160", k, "pic") for k in range(2)]
    large = ([("gop64x48_15", k, "pic") for k in range(fd.n_pics("gop64x48_15"))] + [("wide296x160", k, "pic") for k in range(fd.n_pics("wide296x160"))]) * 6
    assert K["backtoback/small"] == small == K["backtoback/again"]
    assert K["backtoback/large"] == large == K["backtoback/large2"]
    assert len(large) * 96 > 4096 >= len(small) * 96 * 2, "the accumulators (96 bytes a picture, a page at first) had to grow with the small call queued"


# what hvq_last_error_string() said after each call of `refused`, recorded from the runtime before the record frame: the
# order of the checks and their words are part of the interface.  A call that succeeds leaves the words of the refusal before it.
REFUSAL_TEXTS = {
    "refused/null_context": "bad arguments",
    "refused/bad_stream": "bad stream 99",
    "refused/bad_ordinal": "stream 0: bad picture ordinal 1000",
    "refused/misaligned_src": "picture 1: the pointer must be a multiple of 16",
    "refused/src_with_ordinal": "picture 1: a pointer together with ordinal 1 (the caller's memory takes ordinal -1)",
    "refused/src_with_bad_stream": "bad stream 99",
    "refused/minus_one_without_src": "stream 0: bad picture ordinal -1",
    "refused/null_out": "out must be a non-null multiple of 8",
    "refused/misaligned_out": "out must be a non-null multiple of 8",
    "refused/too_many": "65536 pictures: one call takes 65535 at the most (one grid row each)",
    "refused/evicted": "stream 1 picture 0 is no longer resident (slot reused, or the picture was dropped)",
    "refused/queued": "stream 0 picture 7 is queued but not flushed",
    "refused/n0": "stream 0 picture 7 is queued but not flushed",
}


def _check_refused(K, R, S, E):
    for label, text in REFUSAL_TEXTS.items():
        assert E.get(label) == text, (label, E.get(label))
    assert set(E) == set(REFUSAL_TEXTS)
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_STATE
    want = {"null_context": HVQ_E_ARG, "bad_stream": HVQ_E_ARG, "bad_ordinal": HVQ_E_ARG, "misaligned_src": HVQ_E_ARG, "src_with_ordinal": HVQ_E_ARG,
            "src_with_bad_stream": HVQ_E_ARG, "minus_one_without_src": HVQ_E_ARG, "null_out": HVQ_E_ARG, "misaligned_out": HVQ_E_ARG,
            "too_many": HVQ_E_ARG, "evicted": HVQ_E_STATE, "queued": HVQ_E_STATE, "n0": 0}
    assert R == {"refused/" + k: v for k, v in want.items()}
    same, total = S["refused"]
    assert same == total == 2 * 64 + 8, "a refused call wrote its output"
    assert K["refused/then_ok"] == [("gop64x48_15", 1, "pic"), ("gop64x48_15", fd.n_pics("gop64x48_15") - 1, "pic")]


CHECKS = {"goldens": _check_goldens, "memory": _check_memory, "reuse": _check_reuse, "backtoback": _check_backtoback, "refused": _check_refused}


@pytest.mark.parametrize("schedule", ["eager", "late"])
@pytest.mark.parametrize("build", list(fd.BUILDS))
@pytest.mark.parametrize("scenario", list(CHECKS))
def test_fake_device_scenario(drivers, scenario, build, schedule, tmp_path):
    CHECKS[scenario](*_run(drivers[build], scenario, schedule, tmp_path))


def test_the_existing_fake_builds_link_without_the_checksum_body():
    """the source lists of the other drivers have no hvq_launch_checksums: the runtime's reference to it is weak"""
    assert not any("fake_checksums" in s for s in fd.CXX_SOURCES)
    text = open(os.path.join(fd.CSRC, "hvq_runtime.cpp")).read()
    decl = [l for l in text.splitlines() if "hvq_launch_checksums(" in l and l.startswith("extern")]
    assert len(decl) == 1 and "weak" in decl[0]
