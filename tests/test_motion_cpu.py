"""CPU: motion fields (hvq_picture_motion, Context.picture_motion, hvqm4_amd/motion.py) without a GPU.

  - tests/motion_ref.py, the host restatement the GPU tests compare with, on cases worked out by hand: one block and one candidate, a
    picture against itself, a picture displaced by a known vector, flat pictures, and the three tie rules;
  - hvqm4_amd.motion.of_pictures against it, every helper of hvqm4_amd.motion against a direct computation;
  - the constants of motion.py against hvq_desc.h and the header; hvq_motion_blocks against blocks(), refusals included;
  - the argument checks of Context.picture_motion that need no device;
  - the runtime's entry point linked UNCHANGED against the CPU fake device of tests/test_fake_device.py (its source lists and flags, with
    tests/native/fake_motion_driver.cpp in the place of fake_driver.cpp and tests/native/fake_motion.cpp added: a scalar body for
    hvq_launch_motion that reaches memory only through fake_span, when it runs), under both schedules, plain and as a stand-alone
    AddressSanitizer + UndefinedBehaviorSanitizer program.  The driver judges nothing: every field it read back is compared here with
    motion_ref on the oracle's pictures.
"""
import os
import re

import numpy as np
import pytest

import tests.test_fake_device as fd
from tests.motion_ref import cached, motion_reference, plant_cases

NATIVE = fd.NATIVE
CXX_SOURCES = [s for s in fd.CXX_SOURCES if os.path.basename(s) != "fake_driver.cpp"] + \
              [os.path.join(NATIVE, "fake_motion.cpp"), os.path.join(NATIVE, "fake_motion_driver.cpp")]
SIX = ["gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8"]


# ------------------------------------------------------------------------------------------------- the reference, by hand
def test_reference_one_block_has_one_candidate():
    rng = np.random.default_rng(1)
    for B in (8, 16):
        a, b = rng.integers(0, 256, (B, B), dtype=np.uint8), rng.integers(0, 256, (B, B), dtype=np.uint8)
        f = motion_reference(a, b, B, B, B, 15)
        sad = int(np.abs(a.astype(int) - b.astype(int)).sum())
        assert f.dtype == np.int32 and f.shape == (1, 1, 4) and f[0, 0].tolist() == [0, 0, sad, sad]


def test_reference_picture_against_itself_is_all_zero():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (48, 64), dtype=np.uint8)
    for B, R in ((8, 15), (16, 8), (8, 0)):
        assert not motion_reference(a, a, 64, 48, B, R).any()


@pytest.mark.parametrize("B,R,dy,dx", [(8, 8, 3, -5), (16, 15, -15, 15), (8, 15, 0, 9), (16, 4, 4, 4), (8, 3, -3, 0)])
def test_reference_finds_a_known_displacement(B, R, dy, dx):
    """b random, a = b displaced: a[y][x] = b[y + dy][x + dx]; every block whose source lies inside the picture returns the vector at
    cost 0 (random bytes: no other candidate costs 0)"""
    rng = np.random.default_rng(3)
    H, W = 64, 80
    b = rng.integers(0, 256, (H, W), dtype=np.uint8)
    a = rng.integers(0, 256, (H, W), dtype=np.uint8)
    ys0, ys1, xs0, xs1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    a[ys0:ys1, xs0:xs1] = b[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
    f = motion_reference(a, b, W, H, B, R)
    inside = 0
    for r in range(H // B):
        for c in range(W // B):
            y, x = r * B + dy, c * B + dx
            if 0 <= y and y + B <= H and 0 <= x and x + B <= W:
                assert f[r, c, :3].tolist() == [dy, dx, 0], (r, c)
                inside += 1
            else:
                assert f[r, c, 2] > 0
    assert inside >= (H // B - 2) * (W // B - 2)


def test_reference_flat_pictures_and_tie_rules():
    for name, a, b, B, R, record, field in plant_cases():
        f = motion_reference(a, b, 32, 32, B, R)
        if field is not None:
            assert np.array_equal(f, field), name                   # every candidate ties: (0, 0) wins, cost B^2 |delta|
        else:
            assert f[1, 1, :3].tolist() == list(record), (name, f[1, 1].tolist())
            assert f[1, 1, 3] > 0
    assert [c[0] for c in plant_cases()] == ["tie_l1", "tie_dy", "tie_dx", "flat8", "flat16"]


# ------------------------------------------------------------------------------------------------- motion.py
def _geometry(name):
    from hvqm4_amd.container import parse_header
    hdr = parse_header(open(os.path.join(fd.GOLDEN, fd.CLIPS[name]["file"]), "rb").read())
    return hdr.width, hdr.height, hdr.h_samp, hdr.v_samp


def _expected(name, ak, bk, B, R):
    w, h = _geometry(name)[:2]
    pics = fd.oracle_pictures(name)
    return cached((name, ak, bk), pics[ak], pics[bk], w, h, B, R)


def test_of_pictures_is_the_reference():
    from hvqm4_amd import motion as mv
    for name, B, R in (("gop64x48_15", 8, 15), ("gop64x48_15", 16, 6), ("ragged24x40", 8, 15), ("yuv444_13_portrait48x64", 16, 15), ("ip8", 8, 2),
                       ("yuv422_296x160", 8, 3)):
        g = _geometry(name)
        pics = fd.oracle_pictures(name)
        got = mv.of_pictures(pics[1], pics[0].tobytes(), g[0], g[1], B, R, g[2], g[3])
        assert got.dtype == np.int32 and np.array_equal(got, _expected(name, 1, 0, B, R)), (name, B, R)
    for name, a, b, B, R, _rec, _f in plant_cases():
        assert np.array_equal(mv.of_luma(a, b, B, R), motion_reference(a, b, 32, 32, B, R)), name
    with pytest.raises(ValueError):
        mv.of_pictures(pics[1][:-1], pics[0], g[0], g[1], 8, 3, g[2], g[3])
    with pytest.raises(ValueError):
        mv.of_luma(a, b, 8, 16)
    with pytest.raises(ValueError):
        mv.of_luma(a, b[:16], 8, 3)


def test_helpers_against_direct_computation():
    from hvqm4_amd import motion as mv
    g = _geometry("gop64x48_15")
    pics = fd.oracle_pictures("gop64x48_15")
    W, H = g[:2]
    for B, R in ((8, 15), (16, 8)):
        f = _expected("gop64x48_15", 2, 1, B, R) if (B, R) == (8, 15) else motion_reference(pics[2], pics[1], W, H, B, R)
        rows, cols = mv.blocks(W, H, B)
        assert f.shape == (rows, cols, 4)
        l1, l2 = mv.magnitude(f)
        ya, yb = pics[2][:W * H].reshape(H, W), pics[1][:W * H].reshape(H, W)
        pred = mv.compensate(yb, f, B)
        assert pred.dtype == np.uint8 and pred.shape == (H, W)
        total = 0
        votes = {}
        for r in range(rows):
            for c in range(cols):
                dy, dx, cost, cz = (int(v) for v in f[r, c])
                assert l1[r, c] == abs(dy) + abs(dx) and l2[r, c] == pytest.approx((dy * dy + dx * dx) ** 0.5, abs=1e-12)
                src = yb[r * B + dy:(r + 1) * B + dy, c * B + dx:(c + 1) * B + dx]
                assert np.array_equal(pred[r * B:(r + 1) * B, c * B:(c + 1) * B], src)
                assert int(np.abs(ya[r * B:(r + 1) * B, c * B:(c + 1) * B].astype(int) - src.astype(int)).sum()) == cost
                total += cost
                votes[dy, dx] = votes.get((dy, dx), 0) + 1
        assert int(np.abs(ya.astype(int) - pred.astype(int)).sum()) == total == int(f[..., 2].sum()), "compensate, then SAD, is the sum of cost"
        top = max(votes.values())
        want = min((abs(v[0]) + abs(v[1]), v[0], v[1]) for v, k in votes.items() if k == top)
        vec, share = mv.global_motion(f)
        assert vec == want[1:] and share == top / (rows * cols)
        for thr in (0, 1, 50, 10 ** 6):
            assert np.array_equal(mv.moving_mask(f, thr), (f[..., 3].astype(int) - f[..., 2].astype(int)) >= thr)
        assert mv.moving_mask(f, 0).all() and not mv.moving_mask(f, 10 ** 6).any()
        assert mv.gain(f) == int(f[..., 3].sum()) / int(f[..., 2].sum()) >= 1.0
    # ties of global_motion: (0, -2) and (1, 1) and (-2, 0) twice each -> L1 equal, the one furthest up
    t = np.zeros((2, 3, 4), dtype=np.int32)
    t[..., :2] = [[(0, -2), (1, 1), (-2, 0)], [(-2, 0), (0, -2), (1, 1)]]
    assert mv.global_motion(t) == ((-2, 0), 2 / 6)
    t[0, 0, :2] = (0, 1)
    t[1, 1, :2] = (0, 1)
    assert mv.global_motion(t) == ((0, 1), 2 / 6), "then the shortest"
    still = np.zeros((3, 3, 4), dtype=np.int32)
    assert mv.gain(still) == float("inf") and mv.global_motion(still) == ((0, 0), 1.0)
    assert mv.magnitude(np.stack([t, t]))[0].shape == (2, 2, 3)
    with pytest.raises(ValueError):
        mv.compensate(np.zeros((16, 24), dtype=np.uint8), np.full((2, 3, 4), -1, dtype=np.int32), 8)        # points outside
    with pytest.raises(ValueError):
        mv.magnitude(np.zeros((3, 3), dtype=np.int32))
    with pytest.raises(TypeError):
        mv.magnitude(np.zeros((3, 3, 4)))
    with pytest.raises(ValueError):
        mv.global_motion(np.stack([t, t]))


def test_motionfield_lines():
    """tools/motionfield.py's formatter"""
    from tools.motionfield import field_line
    f = np.zeros((2, 2, 4), dtype=np.int32)
    f[..., :2] = (1, -2)
    f[0, 0] = (0, 0, 5, 5)
    f[1:, :, 2:] = (10, 90)
    assert field_line(3, "P", f, 16).split() == ["3", "P", "+1", "-2", "0.7500", "0.5000"]
    assert field_line(0, "I", None, 16).split() == ["0", "I", "-", "-", "-", "-"]


def test_constants_are_those_of_the_kernels_header():
    from hvqm4_amd import motion as mv
    text = open(os.path.join(fd.CSRC, "hvq_desc.h")).read()
    val = {k: int(v) for k, v in re.findall(r"#define (HVQ_MV_(?:LANES|TILE|MAX_RADIUS))\s+(\d+)u", text)}
    assert val == {"HVQ_MV_LANES": 256, "HVQ_MV_TILE": mv.TILE, "HVQ_MV_MAX_RADIUS": mv.MAX_RADIUS}
    assert "static_assert(sizeof(HvqMotionJob) == 48" in text
    head = open(os.path.join(fd.ROOT, "include", "hvqm4_amd.h")).read()
    assert re.search(r"#define HVQ_MOTION_MAX_RADIUS\s+15\b", head) and mv.MAX_RADIUS == 15 and mv.BLOCK_SIZES == (8, 16)
    assert (mv.DY, mv.DX, mv.COST, mv.COST_ZERO) == (0, 1, 2, 3) and mv.MAX_COST == 65280 < 1 << 16
    # the tuple packs into 31 bits
    assert (mv.MAX_COST << 15 | 30 << 10 | 30 << 5 | 30) < 1 << 31


def test_motion_blocks_of_the_library():
    import ctypes as C
    from hvqm4_amd import motion as mv
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_GEOMETRY, lib
    dims = (C.c_int32 * 2)()
    for w, h, hs, vs in [(64, 48, 2, 2), (296, 160, 2, 1), (48, 64, 1, 1), (24, 40, 2, 2), (8, 8, 2, 2), (320, 240, 2, 2), (640, 480, 2, 2)]:
        for B in (8, 16):
            rc = lib().hvq_motion_blocks(w, h, hs, vs, B, dims)
            if w % B or h % B:
                assert rc == HVQ_E_ARG, (w, h, B)
                with pytest.raises(ValueError):
                    mv.blocks(w, h, B)
            else:
                assert (dims[0], dims[1]) == mv.blocks(w, h, B) and rc == dims[0] * dims[1] == (w // B) * (h // B)
                assert lib().hvq_motion_blocks(w, h, hs, vs, B, None) == rc
    for B in (0, 4, 12, 32, -8):
        assert lib().hvq_motion_blocks(64, 48, 2, 2, B, dims) == HVQ_E_ARG
        with pytest.raises(ValueError):
            mv.blocks(64, 48, B)
    assert lib().hvq_motion_blocks(60, 48, 2, 2, 8, dims) == HVQ_E_GEOMETRY
    assert lib().hvq_motion_blocks(64, 48, 3, 2, 8, dims) == HVQ_E_GEOMETRY


# ------------------------------------------------------------------------------------------------- argument checks without a device
class _NoDevice:
    """what Context.picture_motion looks at before it reaches the library"""
    _geom = {0: (64, 48), 1: (24, 40)}
    _h = None

    @staticmethod
    def pic_bytes(sid):
        return {0: 64 * 48 * 3 // 2, 1: 24 * 40 * 3 // 2}[sid]


def test_arguments_are_checked_before_the_library_is_called():
    import torch
    from hvqm4_amd._lib import HVQ_E_ARG, HvqError
    from hvqm4_amd.batch import Context
    call = lambda *a, **k: Context.picture_motion(_NoDevice(), *a, **k)
    with pytest.raises(ValueError, match="ordinals"):
        call([0, 0], [0], [(0, 1)])
    with pytest.raises(HvqError) as e:
        call([0, 7], [0, 0], [(0, 1), (0, 1)])
    assert e.value.code == HVQ_E_ARG
    good = torch.zeros(64 * 48 * 3 // 2, dtype=torch.uint8)
    room = torch.zeros(64 * 48 * 3 // 2 + 64, dtype=torch.uint8)
    off = (-room.data_ptr()) % 16
    for B in (0, 4, 12, 32):
        with pytest.raises(ValueError, match="8 or 16"):
            call([0], [1], [(0, 0)], block=B)
    with pytest.raises(ValueError, match="do not tile"):
        call([0, 1], [1, 1], [(0, 0), (1, 0)], block=16)
    for R in (-1, 16, 2.0, True, None):
        with pytest.raises(ValueError, match="radius"):
            call([0], [1], [(0, 0)], radius=R)
    with pytest.raises(ValueError, match="needs a reference"):
        call([0], [0], None)
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
        call([1], [0], ref=[good], block=8)
    with pytest.raises(ValueError, match="multiple of 16"):
        call([0], [0], ref=[room[off + 8:off + 8 + good.numel()]])
    with pytest.raises(ValueError, match="reference 0 is on cpu, not a GPU"):
        call([0], [0], ref=[room[off:off + good.numel()]])
    # out
    with pytest.raises(ValueError, match="list of 1"):
        call([0], [0], [(0, 1)], block=8, out=torch.zeros((6, 8, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="list of 1"):
        call([0], [0], [(0, 1)], block=8, out=[])
    with pytest.raises(ValueError, match=r"out\[0\] must be"):
        call([0], [0], [(0, 1)], block=8, out=[torch.zeros((6, 8, 4), dtype=torch.int64)])
    with pytest.raises(ValueError, match=r"out\[0\] must be"):
        call([0], [0], [(0, 1)], block=16, out=[torch.zeros((6, 8, 4), dtype=torch.int32)])
    with pytest.raises(ValueError, match=r"out\[0\] must be"):
        call([1], [0], [(1, 1)], block=8, out=[torch.zeros((5, 3, 8), dtype=torch.int32)[:, :, ::2]])
    with pytest.raises(ValueError, match="not a GPU"):
        call([0], [0], [(0, 1)], block=8, out=[torch.zeros((6, 8, 4), dtype=torch.int32)])


def test_the_library_without_a_device_still_checks_its_arguments():
    """no context can exist here, and the call says so before it looks at anything else"""
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, lib
    one = (C.c_int * 1)(0)
    assert lib().hvq_picture_motion(None, 1, one, one, None, 8, 15, None, None) == HVQ_E_ARG
    assert lib().hvq_picture_motion(None, 0, None, None, None, 16, 0, None, None) == HVQ_E_ARG


# ------------------------------------------------------------------------------------------------- the runtime on the CPU fake device
@pytest.fixture(scope="module")
def drivers():
    return {kind: fd.build_driver(kind, "motion", "fake_motion_driver", CXX_SOURCES, __file__) for kind in fd.BUILDS}


def _run(exe, scenario, schedule, tmp_path):
    _, lines = fd.run_checked(exe, scenario, schedule, tmp_path)
    K, R, S, G = {}, {}, {}, {}
    for line in lines:
        f = line.split()
        if f[0] == "F":
            label, name, ak, bform, bk, B, Rad, rows, cols = f[1], f[2], int(f[3]), f[4], int(f[5]), int(f[6]), int(f[7]), int(f[8]), int(f[9])
            got = np.array(f[10:], dtype=np.int64).reshape(rows, cols, 4)
            want = _expected(name, ak, bk, B, Rad)
            assert got.shape == want.shape, (label, got.shape, want.shape)
            assert (got == want).all(), f"{label}: picture {ak} of {name} against {bform} {bk}, B {B} R {Rad}: records {np.argwhere((got != want).any(-1))[:8].tolist()} differ"
            K.setdefault(label, []).append((name, ak, bform, bk))
        elif f[0] == "R":
            R[f[1]] = int(f[2])
        elif f[0] == "S":
            S[f[1]] = (int(f[2]), int(f[3]))
        elif f[0] == "G":
            G[f[1]] = (int(f[2]), int(f[3]))
    assert len(G) == 1
    same, total = next(iter(G.values()))
    assert same == total > 0, "a call wrote outside its field"
    return K, R, S, fd.refusal_texts(lines)


def _check_goldens(K, R, S, E):
    n = {nm: fd.n_pics(nm) for nm in SIX}
    assert len({_geometry(nm)[2:] for nm in SIX}) == 3                    # 4:2:0, 4:2:2 and 4:4:4
    prev = [(nm, k, "pic", k - 1) for nm in SIX for k in range(1, n[nm])]
    assert K["goldens/b8r15"] == prev and K["goldens/b8r3"] == prev and len(prev) > 12
    tiled = [nm for nm in SIX if _geometry(nm)[0] % 16 == 0 and _geometry(nm)[1] % 16 == 0]
    assert tiled == ["gop64x48_15", "yuv444_13_portrait48x64"]
    assert K["goldens/b16r15"] == [(nm, k, "pic", k - 1) for nm in tiled for k in range(1, n[nm])]
    assert K["goldens/mixed"] == [(nm, (r * 2 + 1) % n[nm], "pic", ((r * 2 + 1) % n[nm] + n[nm] - 1) % n[nm]) for r in range(2) for nm in SIX], "fields come back in call order"
    assert K["goldens/self"] == [("yuv422_296x160", 1, "pic", 1)] and not _expected("yuv422_296x160", 1, 1, 8, 7).any()
    assert R == {"goldens/n0": 0}


def _check_memory(K, R, S, E):
    nm, na = "yuv422_64x48", fd.n_pics("yuv422_64x48")
    want = [x for k in range(na) for x in ((nm, k, "mem", (k + 1) % na), (nm, k, "pic", (k + 2) % na))]
    want += [("ragged24x40", 0, "mem", 1), ("ragged24x40", 2, "pic", 1)]
    assert K["memory/b8r15"] == want and K["memory/b8r0"] == want and K["memory/nullstream"] == want
    f = _expected(nm, 0, 1, 8, 0)
    assert not f[..., :2].any() and (f[..., 2] == f[..., 3]).all(), "R = 0: cost is cost_zero"


def _check_reuse(K, R, S, E):
    from hvqm4_amd._lib import HVQ_E_STATE
    n, ne = fd.n_pics("gop64x48_15"), fd.n_pics("yuv444_64x48")
    first = [("gop64x48_15", k, "pic", (k + 1) % n) for k in range(n)]
    assert K["reuse/first"] == first and K["reuse/first16"] == first
    assert R["reuse/evicted"] == HVQ_E_STATE, "the flushes did not hand the slots of the first pass on: the scenario tests nothing"
    assert R["reuse/evicted_ref"] == HVQ_E_STATE
    assert K["reuse/inflight_a"] == [("gop64x48_15", 2, "pic", n - 1)]
    assert K["reuse/inflight_b"] == [("gop64x48_15", n - 1, "pic", 4)]
    assert K["reuse/destroy"] == [("yuv444_64x48", k, "pic", k - 1) for k in range(1, ne)]


# what hvq_last_error_string() said after each call of `refused`, recorded from the runtime before the record frame: the
# order of the checks and their words are part of the interface.  A call that succeeds leaves the words of the refusal before it.
REFUSAL_TEXTS = {
    "refused/null_context": "bad arguments",
    "refused/block_4": "block 4 (8 or 16)",
    "refused/block_0": "block 0 (8 or 16)",
    "refused/block_32": "block 32 (8 or 16)",
    "refused/block_12": "block 12 (8 or 16)",
    "refused/radius_16": "radius 16 outside [0, 15]",
    "refused/radius_negative": "radius -1 outside [0, 15]",
    "refused/block_16_does_not_tile": "picture 1: blocks of 16 do not tile stream 2 (24 x 40)",
    "refused/without_ref": "motion needs a reference for every picture (ref is NULL)",
    "refused/against_zeros": "reference 1: motion against a picture of zeros means nothing (stream -1 needs a pointer)",
    "refused/against_zeros_ordinal": "reference 1: motion against a picture of zeros means nothing (stream -1 needs a pointer)",
    "refused/bad_stream": "bad stream 99",
    "refused/negative_stream": "bad stream -1",
    "refused/bad_ordinal": "stream 0: bad picture ordinal 1000",
    "refused/negative_ordinal": "stream 0: bad picture ordinal -1",
    "refused/ref_bad_stream": "bad stream 99",
    "refused/ref_below_minus_one": "reference 1: stream -2 (a stream, or -1 for the caller's memory)",
    "refused/ref_bad_ordinal": "stream 0: bad picture ordinal 1000",
    "refused/ref_pointer_with_stream": "reference 1: a pointer together with stream 0 (a resident reference takes no pointer)",
    "refused/ref_misaligned": "reference 1: the pointer must be a multiple of 16",
    "refused/ref_other_sampling": "reference 1: stream 1 (64 x 48, chroma shifts 1, 0) has not the geometry of stream 0 (64 x 48, 1, 1)",
    "refused/ref_other_size": "reference 1: stream 2 (24 x 40, chroma shifts 1, 1) has not the geometry of stream 0 (64 x 48, 1, 1)",
    "refused/null_out": "out is NULL",
    "refused/null_field": "field 1: the pointer must be a non-null multiple of 16",
    "refused/misaligned_field": "field 1: the pointer must be a non-null multiple of 16",
    "refused/too_many": "65536 pictures: one call takes 65535 at the most (one grid row each)",
    "refused/evicted": "stream 3 picture 0 is no longer resident (slot reused, or the picture was dropped)",
    "refused/evicted_ref": "stream 3 picture 0 is no longer resident (slot reused, or the picture was dropped)",
    "refused/queued": "stream 0 picture 7 is queued but not flushed",
    "refused/queued_ref": "stream 0 picture 7 is queued but not flushed",
    "refused/n0": "stream 0 picture 7 is queued but not flushed",
    "refused/n0_bad_block": "block 7 (8 or 16)",
    "blocks/64x48_8": "block 7 (8 or 16)",
    "blocks/64x48_16": "block 7 (8 or 16)",
    "blocks/24x40_16": "blocks of 16 do not tile a 24 x 40 picture",
    "blocks/64x48_12": "block 12 (8 or 16)",
    "blocks/geometry": "unsupported geometry 60x48 sampling 2x2",
}


def _check_refused(K, R, S, E):
    for label, text in REFUSAL_TEXTS.items():
        assert E.get(label) == text, (label, E.get(label))
    assert set(E) == set(REFUSAL_TEXTS)
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_GEOMETRY, HVQ_E_STATE
    arg = ["null_context", "block_4", "block_0", "block_32", "block_12", "radius_16", "radius_negative", "block_16_does_not_tile", "without_ref",
           "against_zeros", "against_zeros_ordinal", "bad_stream", "negative_stream", "bad_ordinal", "negative_ordinal", "ref_bad_stream",
           "ref_below_minus_one", "ref_bad_ordinal", "ref_pointer_with_stream", "ref_misaligned", "ref_other_sampling", "ref_other_size", "null_out",
           "null_field", "misaligned_field", "too_many", "n0_bad_block"]
    want = {"refused/" + k: HVQ_E_ARG for k in arg}
    want.update({"refused/evicted": HVQ_E_STATE, "refused/evicted_ref": HVQ_E_STATE, "refused/queued": HVQ_E_STATE, "refused/queued_ref": HVQ_E_STATE,
                 "refused/n0": 0})
    want.update({"blocks/64x48_8": 48, "blocks/64x48_8_rows": 6, "blocks/64x48_8_cols": 8, "blocks/64x48_16": 12, "blocks/24x40_16": HVQ_E_ARG,
                 "blocks/64x48_12": HVQ_E_ARG, "blocks/geometry": HVQ_E_GEOMETRY})
    assert R == want
    same, total = S["refused"]
    assert same == total == 2 * 48 * 16 + 16, "a refused call wrote a field"
    last = fd.n_pics("gop64x48_15") - 1
    assert K["refused/then_ok"] == [("gop64x48_15", 1, "pic", last), ("gop64x48_15", last, "pic", 0)]


CHECKS = {"goldens": _check_goldens, "memory": _check_memory, "reuse": _check_reuse, "refused": _check_refused}


@pytest.mark.parametrize("schedule", ["eager", "late"])
@pytest.mark.parametrize("build", list(fd.BUILDS))
@pytest.mark.parametrize("scenario", list(CHECKS))
def test_fake_device_scenario(drivers, scenario, build, schedule, tmp_path):
    CHECKS[scenario](*_run(drivers[build], scenario, schedule, tmp_path))


def test_the_existing_fake_builds_link_without_the_motion_body():
    """the source lists of the other drivers have no hvq_launch_motion: the runtime's reference to it is weak"""
    assert not any("fake_motion" in s for s in fd.CXX_SOURCES)
    text = open(os.path.join(fd.CSRC, "hvq_runtime.cpp")).read()
    decl = [l for l in text.splitlines() if "hvq_launch_motion(" in l and l.startswith("extern")]
    assert len(decl) == 1 and "weak" in decl[0]
