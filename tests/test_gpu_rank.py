"""GPU: rank filters in slot layout (hvq_rank_pictures / Context.rank_pictures, Context.morph_pictures) against hvqm4_amd.rank.of_picture
-- which tests/test_rank_cpu.py holds equal to tests/rank_ref.py, the plain-Python restatement of include/hvqm4_amd.h -- and against
footprints painted without any window arithmetic, compared with ==.  Every output is allocated with 256 sentinel bytes before and
behind it, which must stay untouched.  The shapes are those of the golden clips: 64 x 48 4:2:0, 48 x 64 4:4:4 and 296 x 160 4:2:2,
whose chroma planes are 148 wide, so that every plane crosses a seam of the kernel's 64-column tiles.  The cases run in ONE child
process that imports torch first (see tests/gpu_child.py); each test reports its case.  The child stops at the first HVQ_E_HIP or
HIP error: nothing more is started on a GPU that has reported a fault."""
import os
import sys
import zlib

import numpy as np
import pytest

from tests import gpu_child, gpu_kit
from tests.gpu_kit import ROOT, SENTINEL, check_bytes as _check, clip as _clip, decode as _decode, geom as _geom, golden as _golden

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300                                 # the cases take seconds each; a hung child is ended, not waited for


# ------------------------------------------------------------------------------------------------------------- child side
def _rank(torch, ctx, sids, ords, rank, src=None, steps=None):
    """one call (or morph_pictures with `steps`) into guarded rooms -> (list of uint8 tensors, guards)"""
    uniform = len({ctx._geometry(s) for s in set(sids)}) <= 1
    out, guards = gpu_kit.rooms(torch, [ctx.pic_bytes(s) for s in sids], uniform)
    got = ctx.morph_pictures(sids, ords, steps, out=out) if steps is not None else ctx.rank_pictures(sids, ords, rank, src, out)
    assert got is out
    return [out[i] for i in range(len(sids))], guards


_expected = {}


def _want(pic, geom, rank):
    """the expected bytes of one picture: computed once, shared by the cases that repeat it (the bodies), left unchanged"""
    from hvqm4_amd import rank as R
    key = (zlib.crc32(np.asarray(pic).tobytes()), geom, rank)
    if key not in _expected:
        _expected[key] = R.of_picture(pic, geom, rank)
    return _expected[key]


def _general(torch, ctx, sids, ords, ranks, src, got, what):
    """the same call with the copy body switched off: the same bytes; the setting is returned and restored"""
    was = ctx.rank_force_general(True)
    assert was is False, what
    again, guards = _rank(torch, ctx, sids, ords, ranks, src)
    torch.cuda.synchronize()
    assert ctx.rank_force_general(was) is True and ctx.rank_force_general(False) is False, what
    _check(torch, again, guards, [g.cpu().numpy() for g in got], what + ": the general body everywhere")


class _Uploaded(gpu_kit.Uploaded):
    def run(self, torch, ranks, what, wants=None, general=False):
        """the pictures in ONE call, ranks[i] for picture i, compared with `wants` (default: the module's bytes)"""
        got, guards = _rank(torch, self.ctx, self.sids, [-1] * len(self.sids), ranks, src=self.bufs)
        torch.cuda.synchronize()
        _check(torch, got, guards, wants if wants is not None else [_want(p, g, r) for p, g, r in zip(self.pics, self.geoms, ranks)], what)
        if general:
            _general(torch, self.ctx, self.sids, [-1] * len(self.sids), ranks, self.bufs, got, what)
        return got


def case_golden(torch, ctx):
    """every golden clip's pictures under erode 1, dilate (3, 1), range 2, median 3 and median 5; the identity beside them, and all of
    it again with the copy body switched off"""
    from hvqm4_amd import rank as R
    from tests import rank_cases as cases
    samplings = set()
    sets = [r for _l, r in cases.FIVE] + [R.identity(), R.luma_only(R.median(3))]
    for name, data, _hdr, _n in _golden():
        sid, hdr, n = _decode(ctx, data)
        g = _geom(hdr)
        samplings.add(g[2:])
        sids, ords, ranks = [sid] * (n * len(sets)), [k for k in range(n) for _ in sets], sets * n
        got, guards = _rank(torch, ctx, sids, ords, ranks)
        torch.cuda.synchronize()
        pics = [ctx.read_picture(sid, k) for k in range(n)]
        _check(torch, got, guards, [_want(pics[k], g, r) for k, r in zip(ords, ranks)], name)
        _general(torch, ctx, sids, ords, ranks, None, got, name)
        ctx.close_stream(sid)
    assert samplings == {(2, 2), (2, 1), (1, 1)}


def case_seams(torch, ctx):
    """296 x 160 4:2:2, planes of 255 with single zeros at the columns 0, 1, 62, 63, 64, 65, 127, 128, last and the rows 0, 15, 16, 17,
    last, under MIN with five radii, and the mirror case under MAX: the clipped rectangles exactly (window extent, axis swap, halo)"""
    from hvqm4_amd import rank as R
    from tests import rank_cases as cases
    g = cases.SEAM_GEOM
    pics, ranks, wants = [], [], []
    for rx, ry in cases.FOOTPRINT_RADII:
        for part in range(3):
            for build, bg, dot in ((R.erode, 255, 0), (R.dilate, 0, 255)):
                pic, pts = cases.dotted(g, part, bg, dot)
                assert all(len(p) >= 10 for p in pts)
                pics.append(pic); ranks.append(build((rx, ry))); wants.append(cases.footprints(g, pts, rx, ry, bg, dot))
    assert {c for _r, c in cases.seam_points(148, 160, 0) + cases.seam_points(148, 160, 1) + cases.seam_points(148, 160, 2)} == {0, 1, 62, 63, 64, 65, 127, 128, 147}
    up = _Uploaded(torch, ctx, pics, [g] * len(pics))
    up.run(torch, ranks, "footprints", wants=wants)
    for pic, r, w in zip(pics[:4], ranks[:4], wants[:4]):                        # the painted rectangles are what the module says too
        assert np.array_equal(_want(pic, g, r), w)
    up.close()


def case_narrow(torch, ctx):
    """planes narrower than the halo and than the window: radius 15 on the 32 x 24 and 24 x 32 chroma planes and on the smallest
    geometry hvq_stream_open accepts, through src=; both bodies"""
    from hvqm4_amd import rank as R
    from tests import rank_cases as cases
    geoms = [(64, 48, 2, 2), (48, 64, 2, 2), cases.SMALLEST, (8, 8, 2, 1), (8, 8, 1, 1)]
    ranks = [R.erode(15), R.dilate(15), R.gradient(15), R.erode((15, 0)), R.dilate((0, 15)), R.median(5), R.median(3), R.identity(), R.gradient(0)]
    pics, gs, rs = [], [], []
    for i, g in enumerate(geoms):
        for j, r in enumerate(ranks):
            pics.append(cases.made(g, "random" if j % 2 else "ties", i + j)); gs.append(g); rs.append(r)
    up = _Uploaded(torch, ctx, pics, gs)
    up.run(torch, rs, "narrow planes", general=True)
    up.close()


def case_packed(torch, ctx):
    """what leaks between the packed 16-bit halves shows: 0 / 255 checkerboards at periods 1 and 2 in every plane for all four ops,
    random planes with values in 0 .. 3 (heavy ties), full-range random planes, a horizontal and a vertical ramp"""
    from hvqm4_amd import rank as R
    from tests import rank_cases as cases
    assert {r.luma.op for r in cases.ALL_OPS} == {R.MIN, R.MAX, R.RANGE, R.MEDIAN}
    pics, gs, rs = [], [], []
    for g in cases.SHAPES:
        for kind in cases.KINDS:
            for j, r in enumerate(cases.ALL_OPS + [R.erode(15), R.dilate((8, 5))]):
                pics.append(cases.made(g, kind, j & 1)); gs.append(g); rs.append(r)
    up = _Uploaded(torch, ctx, pics, gs)
    up.run(torch, rs, "made pictures")
    up.close()


def case_planes(torch, ctx):
    """different luma and chroma entries: luma_only (chroma copied), and chroma RANGE with luma MEDIAN"""
    from hvqm4_amd import rank as R
    from tests import rank_cases as cases
    ranks = [R.luma_only(R.median(5)), R.luma_only(R.erode((4, 2))), R.Rank(R.median(3).luma, R.gradient((2, 3)).luma), R.Rank(R.median(5).luma, R.gradient(1).luma),
             R.Rank(R.IDENTITY_PLANE, R.dilate(3).luma), R.chroma_for(R.erode(6), 2, 1)]
    pics, gs, rs = [], [], []
    for i, g in enumerate(cases.SHAPES):
        for j, r in enumerate(ranks):
            pics.append(cases.made(g, "random", 10 * i + j)); gs.append(g); rs.append(r)
    up = _Uploaded(torch, ctx, pics, gs)
    got = up.run(torch, rs, "luma and chroma differ", general=True)
    g = cases.SHAPES[0]
    assert np.array_equal(got[0].cpu().numpy()[g[0] * g[1]:], pics[0][g[0] * g[1]:]), "luma_only copies the chroma planes"
    up.close()


def case_many(torch, ctx):
    """300 mixed pictures of the three shapes in one call with 64 distinct entries; separately, 65 entries are refused"""
    from hvqm4_amd import rank as R
    from hvqm4_amd._lib import HVQ_E_ARG
    from tests import rank_cases as cases
    table = cases.table64()
    base = {g: [cases.made(g, kind, 3) for kind in ("random", "ties", "check1")] for g in cases.SHAPES}
    pics, gs, rs = [], [], []
    for i in range(300):
        g = cases.SHAPES[i % 3]
        pics.append(base[g][(i // 3) % 3]); gs.append(g); rs.append(table[(i * 7 + i // 64) % 64])
    assert len(set(rs)) == 64
    up = _Uploaded(torch, ctx, pics, gs)
    up.run(torch, rs, "300 pictures, 64 entries")
    with pytest.raises(ValueError, match="65 distinct"):
        ctx.rank_pictures(up.sids[:65], [-1] * 65, table + [R.Rank(R.PlaneRank(R.RANGE, 9, 9), R.PlaneRank(R.RANGE, 9, 8))], src=up.bufs[:65])
    assert _raw(torch, ctx, [up.sids[0]] * 2, [-1, -1], [up.bufs[0].data_ptr()] * 2, [t.struct() for t in table] + [R.erode(1).struct()], which=[0, 64]) == (HVQ_E_ARG, True)
    up.close()


def case_sources(torch, ctx):
    """src= beside resident pictures; rank -> rank through src= equals of_steps(opening(2)); morph_pictures(closing((3, 1))) likewise;
    rank -> picture_checksums(src=) equals the CRC of the expected bytes"""
    from hvqm4_amd import rank as R
    sid, hdr, n = _decode(ctx, _clip("yuv422_296x160"))
    g = _geom(hdr)
    n = min(n, 6)
    pics = [ctx.read_picture(sid, k) for k in range(n)]
    inv = [255 - p for p in pics]
    bufs = [torch.from_numpy(p.copy()).cuda() for p in inv]
    r = R.chroma_for(R.gradient(4), *g[2:])
    sids, ords, src = [sid] * (2 * n), [k for k in range(n)] + [-1] * n, [None] * n + bufs
    got, guards = _rank(torch, ctx, sids, ords, r, src)
    torch.cuda.synchronize()
    _check(torch, got, guards, [_want(p, g, r) for p in pics + inv], "resident pictures and sources in one call")
    # two calls through src=, nothing waited for in between
    steps = R.opening(2)
    first = ctx.rank_pictures([sid] * n, list(range(n)), steps[0])
    second, guards = _rank(torch, ctx, [sid] * n, [-1] * n, steps[1], [first[i] for i in range(n)])
    sums = ctx.picture_checksums([sid] * n, [-1] * n, src=second)
    closed, cguards = _rank(torch, ctx, [sid] * n, list(range(n)), None, steps=R.closing((3, 1)))
    one, oguards = _rank(torch, ctx, [sid] * n, list(range(n)), None, steps=[R.median(3)])
    three = ctx.morph_pictures([sid] * n, list(range(n)), [R.erode(1), R.dilate(2), R.erode(1)])
    torch.cuda.synchronize()
    want = [R.of_steps(p, g, steps) for p in pics]
    _check(torch, second, guards, want, "rank -> rank through src=")
    assert [int(v) for v in sums.cpu().numpy()[:, 3]] == [zlib.crc32(w.tobytes()) for w in want], "rank -> picture_checksums(src=)"
    _check(torch, closed, cguards, [R.of_steps(p, g, R.closing((3, 1))) for p in pics], "morph_pictures(closing((3, 1)))")
    _check(torch, one, oguards, [_want(p, g, R.median(3)) for p in pics], "morph_pictures of one step")
    _check(torch, [three[i] for i in range(n)], [], [R.of_steps(p, g, [R.erode(1), R.dilate(2), R.erode(1)]) for p in pics], "three steps through two scratch tensors")
    ctx.close_stream(sid)


def _raw(torch, ctx, sids, ords, src, structs, which=None, nranks=None, count=None, ctx_h=None, ptr=None, null_ranks=False):
    """hvq_rank_pictures through the C ABI into sentinel-filled memory -> (return code, every byte still holds the sentinel).
    structs: the HvqRank table; ptr: the destination pointer of picture 0 instead of the room's"""
    import ctypes as C
    from hvqm4_amd._lib import HvqRank, lib
    n = len(sids)
    room = torch.full((n, 8192), SENTINEL, dtype=torch.uint8, device="cuda")
    a_d = (C.c_void_p * n)(*[(ptr if ptr is not None and i == 0 else room[i].data_ptr()) for i in range(n)])
    a_p = C.cast((C.c_void_p * n)(*src), C.c_void_p) if src is not None else None
    a_r = (HvqRank * len(structs))(*structs)
    a_w = C.cast((C.c_int * n)(*which), C.c_void_p) if which is not None else None
    rc = lib().hvq_rank_pictures(ctx._h if ctx_h is None else ctx_h, n if count is None else count, (C.c_int * n)(*sids), (C.c_int * n)(*ords), a_p,
                                 None if null_ranks else C.cast(a_r, C.c_void_p), len(structs) if nranks is None else nranks, a_w, C.cast(a_d, C.c_void_p),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, bool(room.eq(SENTINEL).all())


def case_refusals(torch, ctx):
    """every refusal of the header through the C entry leaves the destinations untouched, also those of the well-formed pictures of
    the same call"""
    import ctypes as C
    from hvqm4_amd import rank as R
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_STATE
    from hvqm4_amd.container import video_pictures
    from tests.test_rank_cpu import _spoiled
    data = _clip("gop64x48_15")
    sa, hdr, n = _decode(ctx, data)
    assert ctx.pic_bytes(sa) <= 8192
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    sd = ctx.open_stream(hdr.width, hdr.height, 2, 2, hdr.is15, 3)
    for ft, p in pics:
        ctx.submit(sd, ft, p)
    ctx.flush()                                                  # picture 0 of sd: its slot of the ring of 3 was reused
    sq = ctx.open_stream(hdr.width, hdr.height, 2, 2, hdr.is15, 3)
    mem = torch.zeros(ctx.pic_bytes(sa) + 32, dtype=torch.uint8, device="cuda")
    p16 = mem.data_ptr() + (-mem.data_ptr()) % 16
    good = R.erode(1).struct()
    two = [sa, sa]
    labels = [l for l, _s in _spoiled()]
    assert {"op 4", "radius 16", "a negative radius", "median with rx != ry", "median of radius 3", "pad"} <= set(labels)
    for label, s in _spoiled():                                  # every refusal of hvq_rank_check, in an entry of the table that no picture uses
        assert _raw(torch, ctx, two, [0, 1], None, [good, s], which=[0, 0]) == (HVQ_E_ARG, True), label
        assert _raw(torch, ctx, two, [0, 1], None, [s]) == (HVQ_E_ARG, True), label
    arg = [("bad stream", [sa, 99], [0, 0], None, {}), ("an ordinal that is not resident", two, [0, 1000], None, {}), ("negative ordinal", two, [0, -1], None, {}),
           ("misaligned src", two, [0, -1], [None, p16 + 8], {}), ("an ordinal with src", two, [0, 1], [None, p16], {}),
           ("src with a bad stream", [sa, 99], [0, -1], [None, p16], {}), ("which beyond the table", two, [0, 1], None, {"which": [0, 1]}),
           ("a negative which", two, [0, 1], None, {"which": [0, -1]}), ("nranks 0", two, [0, 1], None, {"nranks": 0}), ("nranks -1", two, [0, 1], None, {"nranks": -1}),
           ("null ranks", two, [0, 1], None, {"null_ranks": True}), ("null context", two, [0, 1], None, {"ctx_h": C.c_void_p(0)}),
           ("null dst", two, [0, 1], None, {"ptr": 0}), ("misaligned dst", two, [0, 1], None, {"ptr": p16 + 8})]
    for what, sids, ords, src, kw in arg:
        assert _raw(torch, ctx, sids, ords, src, [good], **kw) == (HVQ_E_ARG, True), what
    assert _raw(torch, ctx, two, [0, 1], None, [good] * 65, which=[0, 64]) == (HVQ_E_ARG, True), "nranks 65"
    assert _raw(torch, ctx, [sa], [0], None, [good], count=65536) == (HVQ_E_ARG, True), "n beyond 65535"
    assert _raw(torch, ctx, [sa], [0], None, [good], count=0) == (0, True), "n == 0 does nothing"
    # the HVQ_E_STATE cases: a dropped picture (its slot was reused), a picture queued but not flushed
    assert _raw(torch, ctx, [sa, sd], [0, 0], None, [good]) == (HVQ_E_STATE, True), "a dropped picture"
    ctx.submit(sq, pics[0][0], pics[0][1])
    assert _raw(torch, ctx, [sa, sq], [0, 0], None, [good]) == (HVQ_E_STATE, True), "queued but not flushed"
    ctx.flush()
    # the well-formed calls right after them work: a table of 64 with the last one used, and the method
    rc, untouched = _raw(torch, ctx, two, [0, 1], None, [good] * 64, which=[0, 63])
    assert rc == 0 and not untouched
    g = _geom(hdr)
    got, guards = _rank(torch, ctx, [sa, sd, sq], [1, len(pics) - 1, 0], R.median(3))
    torch.cuda.synchronize()
    three = [ctx.read_picture(s, o) for s, o in ((sa, 1), (sd, len(pics) - 1), (sq, 0))]
    _check(torch, got, guards, [_want(p, g, R.median(3)) for p in three], "after the refusals")
    for s in (sa, sd, sq):
        ctx.close_stream(s)


def case_tools(torch, ctx):
    """tools/despeckle.py on a golden clip: median, then an opening, then encode_jpeg(src=): the files of the expected pictures"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import despeckle
    from hvqm4_amd import jpeg
    from hvqm4_amd import rank as R
    from oracle import bridge
    data = _clip("yuv422_64x48")
    geom, files = despeckle.clip_despeckled(ctx, data, median=5, opening=2, quality=80)
    assert geom == (64, 48, 2, 1)
    steps = despeckle.steps_for(5, 2, 2, 1)
    assert steps == [R.chroma_for(R.median(5), 2, 1), R.chroma_for(R.erode(2), 2, 1), R.chroma_for(R.dilate(2), 2, 1)]
    pics = bridge.oracle_decode(data, len(files))
    for k, f in enumerate(files):
        assert f == jpeg.encode(R.of_steps(pics[k].reshape(-1), geom, steps), 64, 48, 80, 2, 1), k
    assert despeckle.steps_for(0, 0, 2, 2) == [R.identity()] and despeckle.steps_for(3, 0, 1, 1) == [R.median(3)]


CASES = ["golden", "seams", "narrow", "packed", "planes", "many", "sources", "refusals", "tools"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "rank", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_rank(case, child_results):
    gpu_child.report(case, child_results)
