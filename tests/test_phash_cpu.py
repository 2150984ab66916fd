"""CPU: perceptual hashes and nearest-hash search (hvq_picture_hashes / Context.picture_hashes, hvq_hash_nearest / Context.hash_nearest,
hvqm4_amd/phash.py) without a GPU.

  - the known answers of include/hvqm4_amd.h on tests/phash_ref.py (plain loops, fractions, Python integers) and on hvqm4_amd.phash (numpy);
  - the two agree on random pictures at 8x8, 16x8, 24x40, 72x56 and 296x160, and on the oracle's pictures of every golden clip, where both
    equal tests/golden/phash.json; the pictures' SHA-256 are manifest.json's: the fixtures describe the same pictures;
  - the grid identities, sum_y, the invariances under a + c, the committed table against the formula, its rows summing to 0;
  - nearest and duplicates on hand-made sets;
  - the argument checks of Context.picture_hashes / Context.hash_nearest that need no device, and the library's without a device;
  - the runtime's entry points linked UNCHANGED against the CPU fake device of tests/test_fake_device.py (its source lists and flags, with
    tests/native/fake_phash_driver.cpp in the place of fake_driver.cpp and tests/native/fake_phash.cpp added: scalar bodies for
    hvq_launch_hashes and hvq_launch_hash_nearest that reach memory only through fake_span, when they run), under both schedules, plain
    and as a stand-alone AddressSanitizer + UndefinedBehaviorSanitizer program.  The driver judges nothing: every record it read back is
    compared here with phash_ref.
"""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import tests.test_fake_device as fd
from tests import phash_ref as ref

NATIVE = fd.NATIVE
CXX_SOURCES = [s for s in fd.CXX_SOURCES if os.path.basename(s) != "fake_driver.cpp"] + \
              [os.path.join(NATIVE, "fake_phash.cpp"), os.path.join(NATIVE, "fake_phash_driver.cpp")]
SIX = ["gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8"]
FIXTURE = json.load(open(os.path.join(fd.GOLDEN, "phash.json")))
SIZES = [(8, 8), (16, 8), (24, 40), (72, 56), (296, 160)]


def fixture_record(name, k):
    a, d, p, s = FIXTURE["clips"][name][k]
    return [int(a, 16), int(d, 16), int(p, 16), s]


# ------------------------------------------------------------------------------------------------- the specification's known answers
def _both(plane):
    from hvqm4_amd import phash
    want = ref.hash_reference(plane)
    assert phash.of_plane(plane) == want
    return want


def test_known_answers():
    for w, h, v in ((8, 8, 1), (64, 48, 200), (24, 40, 255), (296, 160, 17)):
        assert _both(np.full((h, w), v, dtype=np.uint8)) == [0, 0, 0x8000000000000000, v * w * h], (w, h, v)
    # value 0: every F is 0, none lies above the median
    assert _both(np.zeros((48, 64), dtype=np.uint8)) == [0, 0, 0, 0]
    half = np.zeros((64, 64), dtype=np.uint8)
    half[:, :32] = 255
    a = _both(half)
    assert a[0] == 0xF0F0F0F0F0F0F0F0 and a[1] == 0 and a[3] == 255 * 32 * 64
    m = _both(np.ascontiguousarray(half[:, ::-1]))
    assert m[0] == 0x0F0F0F0F0F0F0F0F and m[1] == 0x1818181818181818 and m[3] == a[3]


def test_bit_order():
    """element (r, c) is bit 63 - (8 r + c): a picture whose top left 8th x 8th alone is bright sets the top bit of ahash"""
    from hvqm4_amd import phash
    p = np.zeros((64, 64), dtype=np.uint8)
    p[:8, :8] = 255
    assert _both(p)[0] == 1 << 63
    p = np.zeros((64, 64), dtype=np.uint8)
    p[56:, 56:] = 255
    assert _both(p)[0] == 1
    assert phash.hexes([1 << 63, 1, 0xF0F0F0F0F0F0F0F0, 7]) == ["8000000000000000", "0000000000000001", "f0f0f0f0f0f0f0f0"]
    assert ref.bits([True] + [False] * 63) == 1 << 63


def test_table_equals_the_formula_and_its_rows_sum_to_zero():
    from hvqm4_amd import phash
    t = ref.table()
    assert phash.TABLE.tolist() == t and phash.TABLE.shape == (8, 32)
    assert t[0] == [4096] * 32
    assert all(sum(row) == 0 for row in t[1:])
    assert all(t[k][31 - n] == (-1) ** k * t[k][n] for k in range(8) for n in range(32))
    assert ref.tie_margin() > 0.02
    assert t[1][:4] == [4091, 4052, 3973, 3857] and t[7][12:16] == [-2751, -4052, -3513, -1380]
    # the constants of the kernels and the fake device: hvq_phash.h holds the same half rows
    text = open(os.path.join(fd.CSRC, "hvq_phash.h")).read()
    rows = re.findall(r"\{ ((?:-?\d+, ){15}-?\d+) \},", text)
    assert [[int(v) for v in r.split(", ")] for r in rows] == [t[k][:16] for k in range(1, 8)]


@pytest.mark.parametrize("w,h", SIZES)
def test_module_equals_reference_on_random_pictures(w, h):
    from hvqm4_amd import phash
    rng = np.random.default_rng(w * 1000 + h)
    for kind in range(3):
        p = rng.integers(0, 256, (h, w), dtype=np.uint8) if kind == 0 else rng.integers(100, 104, (h, w), dtype=np.uint8) if kind == 1 else \
            (np.add.outer(np.arange(h) * 3, np.arange(w) * 2) % 256).astype(np.uint8)
        want = ref.hash_reference(p)
        assert phash.of_plane(p) == want
        assert want[3] == int(p.sum(dtype=np.int64)), "sum_y is the sum of luma"
        # of_picture: any sampling, chroma does not enter
        for hs, vs in ((2, 2), (2, 1), (1, 1)):
            c = (w >> (hs == 2)) * (h >> (vs == 2))
            pic = np.concatenate([p.reshape(-1), rng.integers(0, 256, 2 * c, dtype=np.uint8)])
            assert phash.of_picture(pic, w, h, hs, vs) == want == phash.of_picture(pic.tobytes(), w, h, hs, vs)
        assert ref.picture_reference(p.tobytes() + bytes(w * h // 2), w, h) == want


@pytest.mark.parametrize("w,h", SIZES[:4])
def test_grids_three_ways_and_the_two_identities(w, h):
    from hvqm4_amd import phash
    p = np.random.default_rng(w + h).integers(0, 256, (h, w), dtype=np.uint8)
    rows = p.tolist()
    g = {}
    for gy, gx in ((32, 32), (8, 8), (8, 9), (32, 9)):
        g[gy, gx] = ref.grid(rows, gy, gx)
        assert phash.grid(p, gy, gx).tolist() == g[gy, gx]
        if w * h <= 1000:
            assert ref.grid_fractions(rows, gy, gx) == g[gy, gx]
        assert ref.grid_simple(rows, gy, gx) == g[gy, gx]
        assert sum(map(sum, g[gy, gx])) == gy * gx * int(p.sum(dtype=np.int64))
    s32, s8, d, s329 = g[32, 32], g[8, 8], g[8, 9], g[32, 9]
    for r in range(8):
        for c in range(8):
            assert 16 * s8[r][c] == sum(s32[4 * r + i][4 * c + j] for i in range(4) for j in range(4))
        for c in range(9):
            assert 4 * d[r][c] == sum(s329[4 * r + i][c] for i in range(4))
    wts = phash.weights(32, h)
    assert wts.sum(axis=0).tolist() == [32] * h and wts.sum(axis=1).tolist() == [h] * 32
    with pytest.raises(ValueError):
        phash.grid(p.astype(np.int32), 8, 8)


def test_invariance_under_a_constant():
    from hvqm4_amd import phash
    rng = np.random.default_rng(5)
    p = rng.integers(40, 200, (56, 72), dtype=np.uint8)
    base = ref.hash_reference(p)
    for c in (1, 17, 55):
        q = (p + c).astype(np.uint8)
        got = ref.hash_reference(q)
        assert got[:2] == base[:2] and got[3] == base[3] + c * 72 * 56
        # phash too while F[0][0] stays above f_32: here it is the largest value by far
        assert got[2] == base[2] and got[2] >> 63 == 1
        assert phash.of_plane(q) == got


def test_fixture_equals_the_reference_and_the_module_on_the_oracles_pictures_of_every_golden_clip():
    from hvqm4_amd import phash
    from hvqm4_amd.container import parse_header
    assert set(FIXTURE["clips"]) == set(fd.MANIFEST["clips"]), "one entry per clip of manifest.json"
    for name, c in fd.MANIFEST["clips"].items():
        rows = FIXTURE["clips"][name]
        assert len(rows) == len(c["frame_types"]) and all(len(r) == 4 and all(re.fullmatch("[0-9a-f]{16}", v) for v in r[:3]) for r in rows), name
    for name, c in fd.CLIPS.items():
        hdr = parse_header(open(os.path.join(fd.GOLDEN, c["file"]), "rb").read())
        pics = fd.oracle_pictures(name)
        assert [hashlib.sha256(p.tobytes()).hexdigest() for p in pics] == c["picture_sha256"], name
        for k, p in enumerate(pics):
            want = ref.picture_reference(p.tobytes(), hdr.width, hdr.height)
            assert fixture_record(name, k) == want, (name, k)
            assert phash.of_picture(p, hdr.width, hdr.height, hdr.h_samp, hdr.v_samp) == want, (name, k)


# ------------------------------------------------------------------------------------------------- nearest and duplicates
def test_nearest_and_duplicates_on_hand_made_sets():
    from hvqm4_amd import phash
    A = 0xFFFF000000000000
    db = [A, A ^ 1, A ^ 3, A, A ^ (1 << 63), 0]
    q = [A, A ^ 2, 0xFFFFFFFFFFFFFFFF]
    got = phash.nearest(q, db, -1, 1)
    assert got.dtype == np.int32 and got.tolist() == ref.nearest_reference(q, db, -1, 1)
    # ties: A is at 0 and 3, the first wins; A ^ 2 has distance 1 to A (0, 3) and to A ^ 3 (2): candidate 0 wins
    assert got.tolist() == [[0, 0, 4, 0], [0, 1, 3, 0], [2, 46, 0, -1]]               # all ones: A ^ 3 has the most
    assert phash.nearest(q, db, -1, 0).tolist()[1] == [0, 1, 0, -1]
    assert phash.nearest(q, db, -1, 64).tolist()[2] == [2, 46, 6, 0]
    # earlier than me: query i sees j < self_offset + i
    inplace = phash.nearest(db, None, 0, 1)
    assert inplace.tolist() == ref.nearest_reference(db, db, 0, 1) == phash.nearest(db, db, 0, 1).tolist()
    assert inplace.tolist()[0] == [-1, 65, 0, -1] == list(phash.EMPTY)
    assert inplace.tolist()[3] == [0, 0, 2, 0] and inplace.tolist()[5] == [4, 15, 0, -1]
    assert phash.duplicates(db, 1) == [-1, 0, 1, 0, 0, -1]
    assert phash.duplicates(db, 0) == [-1, -1, -1, 0, -1, -1]
    block = phash.nearest(db[2:5], db, 2, 1)
    assert block.tolist() == inplace.tolist()[2:5] == ref.nearest_reference(db[2:5], db, 2, 1)
    assert phash.nearest(q, [], -1, 10).tolist() == [list(phash.EMPTY)] * 3 == ref.nearest_reference(q, [], -1, 10)
    assert phash.nearest([], db, -1, 10).shape == (0, 4)
    assert phash.nearest(db, db, 100, 1).tolist() == phash.nearest(db, db, -1, 1).tolist()
    with pytest.raises(ValueError):
        phash.nearest(q, db, -1, 65)
    # int64 bit patterns and unsigned values are the same hashes
    assert phash.nearest(phash.as_int64(q), phash.as_int64(db), -1, 1).tolist() == got.tolist()
    assert phash.as_uint64(phash.as_int64(db)).tolist() == db
    assert phash.hamming(A, A ^ 7) == 3 and phash.hamming(np.array(db, dtype=np.uint64), A).tolist() == [0, 1, 2, 0, 1, 16]
    rng = np.random.default_rng(9)
    rq, rdb = rng.integers(0, 1 << 12, 50).tolist(), rng.integers(0, 1 << 12, 70).tolist()       # 12 bits: many ties
    for off, thr in ((-1, 3), (0, 2), (5, 4)):
        assert phash.nearest(rq, rdb, off, thr).tolist() == ref.nearest_reference(rq, rdb, off, thr)
    lines = phash.dedup_lines([0, 1], ["I", "P"], [[1 << 63, 1, 2, 99], [3, 4, 5, 6]], [-1, 0])
    assert lines == ["     0 I 8000000000000000 0000000000000001 0000000000000002      -", "     1 P 0000000000000003 0000000000000004 0000000000000005      0"]


# ------------------------------------------------------------------------------------------------- argument checks without a device
class _NoDevice:
    """what Context.picture_hashes looks at before it reaches the library"""
    _geom = {0: (64, 48), 1: (24, 40)}
    _h = None

    @staticmethod
    def pic_bytes(sid):
        return {0: 64 * 48 * 3 // 2, 1: 24 * 40 * 3 // 2}[sid]


def test_arguments_are_checked_before_the_library_is_called():
    import torch
    from hvqm4_amd import phash
    from hvqm4_amd._lib import HVQ_E_ARG, HvqError
    from hvqm4_amd.batch import Context
    call = lambda *a, **k: Context.picture_hashes(_NoDevice(), *a, **k)
    with pytest.raises(ValueError, match="ordinals"):
        call([0, 0], [0])
    with pytest.raises(HvqError) as e:
        call([0, 7], [0, 0])
    assert e.value.code == HVQ_E_ARG
    with pytest.raises(ValueError, match="1 sources for 2 pictures"):
        call([0, 0], [0, 1], src=[None])
    good = torch.zeros(64 * 48 * 3 // 2, dtype=torch.uint8)
    with pytest.raises(ValueError, match="elements"):
        call([1], [-1], src=[good])
    room = torch.zeros(64 * 48 * 3 // 2 + 64, dtype=torch.uint8)
    off = (-room.data_ptr()) % 16
    with pytest.raises(ValueError, match="ordinal -1"):
        call([0], [0], src=[room[off:off + good.numel()]])
    with pytest.raises(ValueError, match="multiple of 16"):
        call([0], [-1], src=[room[off + 8:off + 8 + good.numel()]])
    with pytest.raises(ValueError, match="not a GPU"):
        call([0], [-1], src=[room[off:off + good.numel()]])
    with pytest.raises(ValueError, match="out must be"):
        call([0], [0], out=torch.zeros((1, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="out must be"):
        call([0], [0], out=torch.zeros((2, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match="not a GPU"):
        call([0], [0], out=torch.zeros((1, 4), dtype=torch.int64))
    # hash_nearest: the views
    near = lambda *a, **k: Context.hash_nearest(_NoDevice(), *a, **k)
    rec = torch.zeros((6, 4), dtype=torch.int64)
    with pytest.raises(TypeError, match="int64"):
        near(rec.to(torch.int32))
    with pytest.raises(TypeError):
        near([1, 2, 3])
    with pytest.raises(ValueError, match="shape"):
        near(torch.zeros((2, 2, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="stride"):
        near(rec[:1, 0].expand(6))                                          # six times the same word: stride 0
    with pytest.raises(ValueError, match="threshold"):
        near(rec[:, 0], threshold=65)
    with pytest.raises(ValueError, match="self_offset 0"):
        near(rec[:, 0], None, 3)
    with pytest.raises(ValueError, match="not a GPU"):
        near(rec[:, phash.PHASH])
    with pytest.raises(ValueError, match="not a GPU"):
        near(rec, rec[:, 1])
    # the constants the tests and the kernels share
    assert phash.NEAREST_TILE == 1024 and (phash.AHASH, phash.DHASH, phash.PHASH, phash.SUM_Y) == (0, 1, 2, 3)
    assert (phash.NEAREST, phash.DISTANCE, phash.WITHIN, phash.FIRST_WITHIN) == (0, 1, 2, 3)
    text = open(os.path.join(fd.CSRC, "hvq_desc.h")).read()
    assert re.search(r"#define HVQ_HN_TILE\s+(\d+)u", text).group(1) == str(phash.NEAREST_TILE)


def test_the_library_without_a_device_still_checks_its_arguments():
    """no context can exist here, and the calls say so before they look at anything else"""
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, lib
    one = (C.c_int * 1)(0)
    assert lib().hvq_picture_hashes(None, 1, one, one, None, None, None) == HVQ_E_ARG
    buf = (C.c_uint64 * 4)()
    assert lib().hvq_hash_nearest(None, buf, 1, 1, buf, 1, 1, -1, 10, buf, None) == HVQ_E_ARG


# ------------------------------------------------------------------------------------------------- the runtime on the CPU fake device
@pytest.fixture(scope="module")
def drivers():
    return {kind: fd.build_driver(kind, "phash", "fake_phash_driver", CXX_SOURCES, __file__) for kind in fd.BUILDS}


_want = {}


def _geometry(name):
    from hvqm4_amd.container import parse_header
    hdr = parse_header(open(os.path.join(fd.GOLDEN, fd.CLIPS[name]["file"]), "rb").read())
    return hdr.width, hdr.height


def _expected(name, k, form="pic"):
    key = (name, k, form)
    if key not in _want:
        a = fd.oracle_pictures(name)[k]
        _want[key] = ref.picture_reference((255 - a if form == "inv" else a).tobytes(), *_geometry(name))
    return _want[key]


def _run(exe, scenario, schedule, tmp_path):
    _, lines = fd.run_checked(exe, scenario, schedule, tmp_path)
    K, R, S, N = {}, {}, {}, {}
    for line in lines:
        f = line.split()
        if f[0] == "H":
            label, name, k, form = f[1], f[2], int(f[3]), f[4]
            got = [int(v) for v in f[5:]]
            want = _expected(name, k, form)
            assert got == want, f"{label}: picture {k} of {name} ({form}):\n{got}\nwant\n{want}"
            K.setdefault(label, []).append((name, k, form))
        elif f[0] == "R":
            R[f[1]] = int(f[2])
        elif f[0] == "S":
            S[f[1]] = (int(f[2]), int(f[3]))
        elif f[0] in "QD":
            N.setdefault(f[1], {"Q": [], "D": [], "N": []})[f[0]].append(int(f[3]))
        elif f[0] == "A":
            N[f[1]]["A"] = (int(f[2]), int(f[3]))
        elif f[0] == "N":
            N.setdefault(f[1], {"Q": [], "D": [], "N": []})["N"].append([int(v) for v in f[3:]])
    return K, R, S, N, fd.refusal_texts(lines)


def _check_goldens(K, R, S, N, E):
    n = {nm: fd.n_pics(nm) for nm in SIX}
    assert K["goldens/clip"] == [(nm, k, "pic") for nm in SIX for k in range(n[nm])]
    assert K["goldens/clip"] and all(fixture_record(nm, k) == _expected(nm, k) for nm, k, _f in K["goldens/clip"])
    assert K["goldens/mixed"] == [(nm, (r * 3 + 1) % n[nm], "pic") for r in range(2) for nm in SIX], "records come back in call order"
    assert K["goldens/one"] == [("yuv422_296x160", 1, "pic")]
    assert R == {"goldens/n0": 0}
    assert {_geometry(nm)[0] % 16 for nm in SIX} == {0, 8}, "rows of 16-byte and of 8-byte units"


def _check_memory(K, R, S, N, E):
    na = fd.n_pics("yuv422_64x48")
    want = [x for k in range(na) for x in (("yuv422_64x48", k, "inv"), ("yuv422_64x48", k, "pic"))] + [("ragged24x40", 1, "inv"), ("ragged24x40", 1, "pic")]
    assert K["memory"] == want and K["memory/nullstream"] == want


def _check_reuse(K, R, S, N, E):
    from hvqm4_amd._lib import HVQ_E_STATE
    n, ne = fd.n_pics("gop64x48_15"), fd.n_pics("yuv444_64x48")
    assert K["reuse"] == [("gop64x48_15", k, "pic") for k in range(n)]
    assert R["reuse/evicted"] == HVQ_E_STATE, "the flushes did not hand the slots of the first pass on: the scenario tests nothing"
    assert K["reuse/late"] == [("gop64x48_15", k, "pic") for k in range(n)]
    assert K["reuse/destroy"] == [("yuv444_64x48", k, "pic") for k in range(ne)]


def _check_backtoback(K, R, S, N, E):
    small = [("wide296x160", k, "pic") for k in range(2)]
    large = ([("gop64x48_15", k, "pic") for k in range(fd.n_pics("gop64x48_15"))] + [("wide296x160", k, "pic") for k in range(fd.n_pics("wide296x160"))]) * 6
    assert K["backtoback/small"] == small == K["backtoback/again"]
    assert K["backtoback/large"] == large == K["backtoback/large2"]
    assert len(large) > 2 * 2 * len(small), "the cells (twice the first call's at first) had to grow with the small call queued"


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
    "refused/too_many": "65536 pictures: one call takes 65535 at the most",
    "refused/evicted": "stream 1 picture 0 is no longer resident (slot reused, or the picture was dropped)",
    "refused/queued": "stream 0 picture 7 is queued but not flushed",
    "refused/n0": "stream 0 picture 7 is queued but not flushed",
    "refused/near_null_context": "bad arguments",
    "refused/near_null_q": "q must be a non-null multiple of 8",
    "refused/near_misaligned_q": "q must be a non-null multiple of 8",
    "refused/near_null_db": "db must be a non-null multiple of 8",
    "refused/near_misaligned_db": "db must be a non-null multiple of 8",
    "refused/near_null_out": "out must be a non-null multiple of 16",
    "refused/near_misaligned_out": "out must be a non-null multiple of 16",
    "refused/near_q_stride0": "strides 0 and 1: a stride counts 64-bit words and is at least 1",
    "refused/near_db_stride_negative": "strides 1 and -1: a stride counts 64-bit words and is at least 1",
    "refused/near_threshold65": "threshold 65 outside [0, 64]",
    "refused/near_threshold_negative": "threshold -1 outside [0, 64]",
    "refused/near_nq_negative": "-1 queries against 4 hashes: each count lies in [0, 16777216]",
    "refused/near_nq_too_many": "16777217 queries against 4 hashes: each count lies in [0, 16777216]",
    "refused/near_ndb_too_many": "4 queries against 16777217 hashes: each count lies in [0, 16777216]",
}


def _check_refused(K, R, S, N, E):
    for label, text in REFUSAL_TEXTS.items():
        assert E.get(label) == text, (label, E.get(label))
    assert set(E) == set(REFUSAL_TEXTS)
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_STATE
    want = {"null_context": HVQ_E_ARG, "bad_stream": HVQ_E_ARG, "bad_ordinal": HVQ_E_ARG, "misaligned_src": HVQ_E_ARG, "src_with_ordinal": HVQ_E_ARG,
            "src_with_bad_stream": HVQ_E_ARG, "minus_one_without_src": HVQ_E_ARG, "null_out": HVQ_E_ARG, "misaligned_out": HVQ_E_ARG,
            "too_many": HVQ_E_ARG, "evicted": HVQ_E_STATE, "queued": HVQ_E_STATE, "n0": 0}
    near = ["null_context", "null_q", "misaligned_q", "null_db", "misaligned_db", "null_out", "misaligned_out", "q_stride0", "db_stride_negative",
            "threshold65", "threshold_negative", "nq_negative", "nq_too_many", "ndb_too_many"]
    want.update({"near_" + k: HVQ_E_ARG for k in near})
    assert R == {"refused/" + k: v for k, v in want.items()}
    same, total = S["refused"]
    assert same == total == 2 * 32 + 8, "a refused call wrote its output"
    assert K["refused/then_ok"] == [("gop64x48_15", 1, "pic"), ("gop64x48_15", fd.n_pics("gop64x48_15") - 1, "pic")]


def _check_nearest(K, R, S, N, E):
    labels = ["all", "strides_thr0", "thr64", "inplace", "block", "offset_beyond", "ndb0", "one", "big", "big_block", "big_inplace"]
    assert R == {"nearest/nq0": 0}
    for lb in labels:
        c = N["nearest/" + lb]
        off, thr = c["A"]
        assert c["N"] == ref.nearest_reference(c["Q"], c["D"], off, thr), lb
        assert S["nearest/" + lb] == (4, 4), "the 16 bytes behind the records were written"
    assert N["nearest/inplace"]["N"][0] == [-1, 65, 0, -1] and N["nearest/ndb0"]["N"] == [[-1, 65, 0, -1]] * 80
    assert N["nearest/one"]["N"] == [[0, 0, 1, 0]]
    # the sets do exercise ties, duplicates and more than one workgroup and tile
    a = N["nearest/all"]
    assert len(set(a["D"])) < len(a["D"]) and any(r[2] > 1 for r in a["N"]) and any(r[2] == 0 for r in a["N"])
    assert len(N["nearest/big"]["Q"]) > 512 and len(N["nearest/big"]["D"]) > 2048
    assert N["nearest/block"]["N"][:60] == N["nearest/inplace"]["N"][10:70]
    # the records of a clip straight into the search, column by column
    n = fd.n_pics("gop64x48_15")
    assert K["nearest/records"] == [("gop64x48_15", k, "pic") for k in range(n)]
    for col in range(3):
        hashes = [_expected("gop64x48_15", k)[col] for k in range(n)]
        assert N[f"nearest/column{col}"]["N"] == ref.nearest_reference(hashes, hashes, 0, 12), col


CHECKS = {"goldens": _check_goldens, "memory": _check_memory, "reuse": _check_reuse, "backtoback": _check_backtoback, "refused": _check_refused,
          "nearest": _check_nearest}


@pytest.mark.parametrize("schedule", ["eager", "late"])
@pytest.mark.parametrize("build", list(fd.BUILDS))
@pytest.mark.parametrize("scenario", list(CHECKS))
def test_fake_device_scenario(drivers, scenario, build, schedule, tmp_path):
    CHECKS[scenario](*_run(drivers[build], scenario, schedule, tmp_path))


def test_the_existing_fake_builds_link_without_the_hash_bodies():
    """the source lists of the other drivers have no hvq_launch_hashes / hvq_launch_hash_nearest: the runtime's references are weak"""
    assert not any("fake_phash" in s for s in fd.CXX_SOURCES)
    text = open(os.path.join(fd.CSRC, "hvq_runtime.cpp")).read()
    for sym in ("hvq_launch_hashes(", "hvq_launch_hash_nearest("):
        decl = [l for l in text.splitlines() if sym in l and l.startswith("extern")]
        assert len(decl) == 1 and "weak" in decl[0], sym
