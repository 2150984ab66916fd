"""GPU: corner detection (hvq_corner_pictures / Context.corner_pictures) against hvqm4_amd.corners -- which tests/test_corner_cpu.py holds
equal to tests/corner_ref.py, the plain-Python restatement of include/hvqm4_amd.h --, every comparison with ==.  Every output (mask,
list, row index, response map) is allocated with 256 sentinel bytes before and behind it, which must stay untouched; the rows of a list
beyond `stored` must keep the sentinel too.  The cases run in ONE child process that imports torch first (see tests/gpu_child.py); each
test reports its case.  The child stops at the first HVQ_E_HIP or HIP error: nothing more is started on a GPU that has reported a
fault."""
import os
import sys

import numpy as np
import pytest

from tests import gpu_child, gpu_kit
from tests.gpu_kit import GUARD, ROOT, SENTINEL, clip as _clip, decode as _decode, geom as _geom, golden_by_name as _golden

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300                                 # the cases take seconds each; a hung child is ended, not waited for
FILLER = int.from_bytes(bytes([SENTINEL]) * 8, "little", signed=True)


# ------------------------------------------------------------------------------------------------------------- child side
def _room(torch, nbytes, dtype, shape):
    """a tensor of `shape` between GUARD sentinel bytes, itself filled with the sentinel -> (tensor, the whole allocation)"""
    pad = (-nbytes) % 16
    whole = torch.full((GUARD + nbytes + pad + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    return whole[GUARD:GUARD + nbytes].view(dtype).view(shape), whole


def _corners(torch, ctx, sids, ords, rules, which=None, cap=16, src=None, response=None):
    """one call into guarded rooms -> (mask, points, rows, response or None, the allocations with the bytes of each output)"""
    from hvqm4_amd import corners as cr
    n = len(sids)
    table = [rules] * n if isinstance(rules, cr.Rule) else list(rules)
    per = [table[which[i]] if which is not None else table[i] for i in range(n)]
    response = [True] * n if response is None else response
    mask, points, rows, resp, wholes = [], [], [], [], []
    for i in range(n):
        g = ctx._geometry(sids[i])
        ny, nx = cr.plane_shape(g, per[i].plane)
        for lst, nb, dt, shape in ((mask, ctx.pic_bytes(sids[i]), torch.uint8, (ctx.pic_bytes(sids[i]),)), (points, 32 * (cap + 1), torch.int64, (cap + 1, 4)),
                                   (rows, 4 * (ny + 1), torch.int32, (ny + 1,)), (resp, 8 * nx * ny, torch.int64, (ny, nx))):
            t, whole = _room(torch, nb, dt, shape)
            lst.append(t); wholes.append((whole, nb))
    if all(response):
        got = ctx.corner_pictures(sids, ords, rules, which=which, cap=cap, src=src, mask=mask, points=points, rows=rows, response=resp)
        assert got[0] is not None and len(got) == 4
    else:                                                        # the C entry: NULL entries in the array of response maps
        import ctypes as C
        from hvqm4_amd._lib import HvqCornerRule, check, lib
        assert which is None and src is None
        distinct = list(dict.fromkeys(per))
        a_r = (HvqCornerRule * len(distinct))(*[r.struct() for r in distinct])
        arr = lambda ts: C.cast((C.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in ts]), C.c_void_p)
        check(lib().hvq_corner_pictures(ctx._h, n, (C.c_int * n)(*sids), (C.c_int * n)(*ords), None, C.cast(a_r, C.c_void_p), len(distinct),
                                        C.cast((C.c_int * n)(*[distinct.index(r) for r in per]), C.c_void_p), arr(mask), arr(points), arr(rows),
                                        arr([t if q else None for t, q in zip(resp, response)]), cap, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return mask, points, rows, resp, wholes, per, response


_expected = {}


def _want(pic, geom, rule, cap):
    """the expected values of one picture: computed once, shared by the cases that repeat it, left unchanged"""
    import zlib
    from hvqm4_amd import corners as cr
    key = (zlib.crc32(np.asarray(pic).tobytes()), tuple(geom), rule)
    if key not in _expected:
        R = cr.response_of_plane(cr.plane_of(pic, geom, rule.plane), rule)
        _expected[key] = (R,) + cr.of_plane(None, rule, None, response=R)
    R, mask, points, rows = _expected[key]
    parts = [mask.reshape(-1) if p == rule.plane else np.full(int(np.prod(cr.plane_shape(geom, p))), 128 if p else 0, dtype=np.uint8) for p in range(3)]
    stored = min(int(points[0, 0]), cap)
    pts = points[:stored + 1].copy()
    pts[0, 1] = stored
    return np.concatenate(parts), pts, rows, R


def _check(torch, ctx, result, pics, geoms, cap, what):
    mask, points, rows, resp, wholes, per, response = result
    torch.cuda.synchronize()
    for whole, nb in wholes:
        w = whole.cpu().numpy()
        assert (w[:GUARD] == SENTINEL).all() and (w[GUARD + nb:] == SENTINEL).all(), f"{what}: the bytes around an output were written"
    for i, (pic, g, r) in enumerate(zip(pics, geoms, per)):
        wm, wp, wr, wR = _want(pic, g, r, cap)
        gm, gp, gr = mask[i].cpu().numpy(), points[i].cpu().numpy(), rows[i].cpu().numpy().view(np.uint32)
        assert np.array_equal(gm, wm), f"{what}: picture {i} {r}: {int((gm != wm).sum())} bytes of the mask differ, first at {np.flatnonzero(gm != wm)[:1]}"
        assert np.array_equal(gr, wr), f"{what}: picture {i} {r}: the row index differs"
        assert np.array_equal(gp[:wp.shape[0]], wp), f"{what}: picture {i} {r}: the list differs: {gp[:3].tolist()} for {wp[:3].tolist()}"
        assert (gp[wp.shape[0]:] == FILLER).all(), f"{what}: picture {i}: a row beyond `stored` was written"
        if response[i]:
            gR = resp[i].cpu().numpy()
            assert np.array_equal(gR, wR), f"{what}: picture {i} {r}: {int((gR != wR).sum())} responses differ, first at {np.argwhere(gR != wR)[:1].tolist()}"
        else:
            assert (resp[i].cpu().numpy() == FILLER).all(), f"{what}: picture {i}: a response map that was not asked for was written"


def _uploaded(torch, ctx, items, cap, what, response=None):
    """[(label, geom, picture, rule, response)] through src= in ONE call"""
    up = gpu_kit.Uploaded(torch, ctx, [it[2] for it in items], [tuple(it[1]) for it in items])
    n = len(items)
    res = _corners(torch, ctx, up.sids, [-1] * n, [it[3] for it in items], cap=cap, src=up.bufs, response=response)
    _check(torch, ctx, res, up.pics, up.geoms, cap, what)
    up.close()
    return res


def case_golden(torch, ctx):
    """64 x 48 4:2:0, 48 x 64 4:4:4 and 296 x 160 4:2:2 where they lie: every plane, both measures, r in {1, 2, 3}, nms in {0, 1, 3, 7},
    with response maps; the fixture's K on the way"""
    import json
    from tests.corner_cases import fixture_rules as _fixture_rules
    fixture = json.load(open(os.path.join(ROOT, "tests", "golden", "corners.json")))
    rules = _fixture_rules()
    assert len(rules) == 72
    samplings = set()
    for name in ("crossplane420_64x48", "crossplane444_48x64", "yuv422_296x160"):
        data, _hdr, _n = _golden()[name]
        sid, hdr, n = _decode(ctx, data)
        g = _geom(hdr)
        samplings.add(g[2:])
        k = fixture["picture"]
        pic = ctx.read_picture(sid, k)
        for plane in range(3):                                       # 24 rules a call, one call per plane
            part = [r for r in rules if r.plane == plane]
            res = _corners(torch, ctx, [sid] * len(part), [k] * len(part), part, cap=64)
            _check(torch, ctx, res, [pic] * len(part), [g] * len(part), 64, f"{name} plane {plane}")
            for r, p in zip(part, res[1]):
                assert int(p[0, 0]) == fixture["clips"][name][rules.index(r)][0], (name, r)
        ctx.close_stream(sid)
    assert samplings == {(2, 2), (2, 1), (1, 1)}


def case_seams(torch, ctx):
    """296 x 160: single bright 3 x 3 blocks at the columns 0, 1, 62 .. 65, 127, 128, last and the rows 0, 15, 16, 17, last, one a
    picture, and one in the middle of a tile: == the module everywhere, and wherever the block's reach stays inside the plane its
    corners are the middle block's, shifted"""
    from tests import corner_cases as cases
    items = cases.seam_cases()
    res = _uploaded(torch, ctx, items, 16, "seams", response=[True] * len(items))
    mid = res[1][-1].cpu().numpy()
    K = int(mid[0, 0])
    assert K >= 1
    r = items[-1][3]
    reach, (ny, nx) = r.nms + r.radius + 2, (cases.WIDE[1], cases.WIDE[0])
    my, mx = 8 + 2 * cases.TY, 24 + 2 * cases.TX
    shifted = 0
    for i, (y, x) in enumerate((y, x) for y in cases.SEAM_ROWS for x in cases.SEAM_COLUMNS):
        if y >= reach and x >= reach and y + 3 + reach <= ny and x + 3 + reach <= nx:      # the block's reach stays inside the plane
            got = res[1][i].cpu().numpy()
            assert np.array_equal(got[:K + 1], mid[:K + 1] + np.array([[0] * 4] + [[x - mx, y - my, 0, (y - my) * nx + (x - mx)]] * K)), (y, x)
            shifted += 1
    assert shifted == 3 * 6                                      # rows 15, 16, 17 x columns 62 .. 65, 127, 128


def case_narrow(torch, ctx):
    """planes narrower than the halo: 8 x 8, whose chroma is 4 x 4 against a halo of 11 -- the smallest geometry a stream takes"""
    from tests import corner_cases as cases
    items = cases.narrow_cases()
    assert any(it[1] == (8, 8, 2, 2) and it[3].plane and it[3].nms + it[3].radius + 1 == 11 for it in items)
    _uploaded(torch, ctx, items, 16, "narrow planes")


def case_ties(torch, ctx):
    """a white 4 x 4 square and its mirror images under nms = 7: equal responses, the first in raster order survives; a plane that is
    mirror-symmetric across a tile seam"""
    from tests import corner_cases as cases
    items = cases.tie_cases()
    res = _uploaded(torch, ctx, items, 32, "ties")
    for it, p in zip(items, res[1]):
        if it[0].startswith("square"):
            assert int(p[0, 0]) == 1, it[0]


def case_arithmetic(torch, ctx):
    """the period-4 stripes and the 2 x 2 checkerboard at k = 64, r = 3; the edge, whose min-eigenvalue radicand is a perfect square
    everywhere; the plane of 0 / 1 samples, where it is a perfect square or one less than one at many samples"""
    from tests import corner_cases as cases
    items = cases.arithmetic_cases()
    res = _uploaded(torch, ctx, items, 32, "arithmetic")
    i = [it[0] for it in items].index("stripes: harris k 64 r 3")
    assert int(res[3][i].min()) == -166330855434240000


def case_cap(torch, ctx):
    """K against cap in {0, 1, K - 1, K, K + 1}: rows beyond `stored` stay untouched"""
    from tests import corner_cases as cases
    g, pic, rule, K = cases.cap_case()
    assert K >= 3
    for cap in (0, 1, K - 1, K, K + 1):
        res = _uploaded(torch, ctx, [("cap", g, pic, rule, 1)] * 2, cap, f"cap {cap}")
        assert res[1][0][0].tolist() == [K, min(K, cap), 0, 0]


def case_margin_and_thresholds(torch, ctx):
    """margins up to half the plane and beyond (K = 0); a threshold equal to a corner's R, and that R + 1"""
    from tests import corner_cases as cases
    items = cases.margin_cases() + cases.threshold_cases()
    res = _uploaded(torch, ctx, items, 128, "margins and thresholds")
    K = {it[0]: int(p[0, 0]) for it, p in zip(items, res[1])}
    assert K["margin 12"] == 0 and K["margin 36"] == 0 and K["margin 255"] == 0 and K["margin 0"] > K["margin 5"] > K["margin 11"] > 0
    t = [it[0] for it in cases.threshold_cases()]
    assert K[t[0]] == K[t[1]] + 1 and K[t[2]] == K[t[3]] + 1


def case_mixed(torch, ctx):
    """60 mixed pictures under 64 rules in one call, with which= and src=; every third with a response map through the C entry"""
    from tests import corner_cases as cases
    geoms, pics, rules, which = cases.mixed_cases()
    assert len(rules) == 64 and len(pics) == 60
    up = gpu_kit.Uploaded(torch, ctx, pics, geoms)
    res = _corners(torch, ctx, up.sids, [-1] * 60, rules, which=which, cap=64, src=up.bufs)
    _check(torch, ctx, res, pics, geoms, 64, "mixed")
    up.close()
    # resident pictures, some without a response map
    data, _hdr, _n = _golden()["yuv422_296x160"]
    sid, hdr, n = _decode(ctx, data)
    per = [rules[i % 64] for i in range(n)]
    res = _corners(torch, ctx, [sid] * n, list(range(n)), per, cap=64, response=[i % 3 == 0 for i in range(n)])
    _check(torch, ctx, res, [ctx.read_picture(sid, k) for k in range(n)], [_geom(hdr)] * n, 64, "resident, some response maps")
    ctx.close_stream(sid)


def case_chain(torch, ctx):
    """tools/corners.py on a golden clip: corners -> dilate -> overlay -> encode_jpeg(src=) against the same chain on the host modules"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import corners as tool
    from hvqm4_amd import compose, jpeg, rank
    from hvqm4_amd import corners as cr
    from oracle import bridge
    data = _clip("yuv422_64x48")
    rule = tool.rule_for(False, 1, 3, None)
    geom, lists, files = tool.clip_corners(ctx, data, rule, files=True, quality=80)
    assert geom == (64, 48, 2, 1) and rule == cr.harris(1, 10, nms=3)
    pics = bridge.oracle_decode(data, len(files))
    for k, f in enumerate(files):
        pic = pics[k].reshape(-1)
        mask, points, _rows = cr.of_picture(pic, geom, rule, tool.CAP)
        assert np.array_equal(lists[k][:points.shape[0]], points), k
        marks = rank.of_picture(mask, geom, rank.dilate(2))
        both = compose.of_pictures([pic, marks], [geom, geom], compose.overlay(geom, 0, 0, geom[:2], tool.ALPHA))
        assert f == jpeg.encode(both, 64, 48, 80, 2, 1), k


def case_refusals(torch, ctx):
    """a refused call leaves its outputs untouched, also those of the well-formed pictures of the same call"""
    import ctypes as C
    from hvqm4_amd import corners as cr
    from hvqm4_amd._lib import HVQ_E_ARG, HvqCornerRule, lib
    from tests.test_corner_cpu import _BAD_RULES
    sa, hdr, n = _decode(ctx, _clip("gop64x48_15"))
    pb = ctx.pic_bytes(sa)
    room = torch.full((2, pb + 32 * 9 + 4 * 52 + 8 * 64 * 48), SENTINEL, dtype=torch.uint8, device="cuda")
    base = [room[i].data_ptr() for i in range(2)]
    assert all(b % 16 == 0 for b in base)
    M, P, Y, Q = ([b + o for b in base] for o in (0, pb, pb + 288, pb + 288 + 208))
    mem = torch.zeros(pb + 32, dtype=torch.uint8, device="cuda")
    p16 = mem.data_ptr() + (-mem.data_ptr()) % 16
    good = cr.harris().struct()

    def raw(sids=(sa, sa), ords=(0, 1), src=None, rules=(good,), nrules=None, which=None, mask=M, points=P, rows=Y, response=Q, cap=8, count=2, ctx_h=None, null=()):
        arr = lambda v: None if v is None else C.cast((C.c_void_p * 2)(*v), C.c_void_p)
        a_r = (HvqCornerRule * len(rules))(*rules)
        rc = lib().hvq_corner_pictures(ctx._h if ctx_h is None else ctx_h, count, (C.c_int * 2)(*sids), (C.c_int * 2)(*ords), arr(src),
                                       None if "rules" in null else C.cast(a_r, C.c_void_p), len(rules) if nrules is None else nrules,
                                       None if which is None else C.cast((C.c_int * 2)(*which), C.c_void_p), arr(mask), arr(points), arr(rows), arr(response), cap,
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc, bool(room.eq(SENTINEL).all())
    for bad in _BAD_RULES:                                       # in an unused entry of the table and in a used one
        s = HvqCornerRule(*bad)
        assert raw(rules=(good, s), which=(0, 0)) == (HVQ_E_ARG, True), bad
        assert raw(rules=(s,)) == (HVQ_E_ARG, True), bad
    refused = [("bad stream", dict(sids=(sa, 99))), ("an ordinal that is not resident", dict(ords=(0, 1000))), ("a negative ordinal", dict(ords=(0, -1))),
               ("misaligned src", dict(ords=(0, -1), src=(None, p16 + 8))), ("an ordinal with src", dict(src=(None, p16))), ("which beyond the table", dict(which=(0, 1))),
               ("a negative which", dict(which=(0, -1))), ("nrules 0", dict(nrules=0)), ("nrules 65", dict(rules=(good,) * 65, which=(0, 0))), ("null rules", dict(null=("rules",))),
               ("null context", dict(ctx_h=C.c_void_p(0))), ("cap -1", dict(cap=-1)), ("cap beyond", dict(cap=cr.MAX_CAP + 1)), ("null masks", dict(mask=None)),
               ("a null mask", dict(mask=(M[0], None))), ("a misaligned mask", dict(mask=(M[0], M[1] + 8))), ("null points", dict(points=None)),
               ("a null list", dict(points=(None, P[1]))), ("a misaligned list", dict(points=(P[0] + 8, P[1]))), ("null rows", dict(rows=None)),
               ("a null row index", dict(rows=(Y[0], None))), ("a misaligned row index", dict(rows=(Y[0] + 4, Y[1]))), ("a misaligned response map", dict(response=(Q[0], Q[1] + 8))),
               ("65536 pictures", dict(count=65536)), ("-1 pictures", dict(count=-1))]
    for label, kw in refused:
        assert raw(**kw) == (HVQ_E_ARG, True), label
    assert raw(count=0) == (0, True)
    rc, untouched = raw()                                        # the well-formed call right after them works
    assert rc == 0 and not untouched
    g = _geom(hdr)
    for i in range(2):
        wm, wp, wr, wR = _want(ctx.read_picture(sa, i), g, cr.harris(), 8)
        got = room[i].cpu().numpy()
        assert np.array_equal(got[:pb], wm) and np.array_equal(got[pb:pb + 288].view("<i8").reshape(9, 4)[:wp.shape[0]], wp), i
        assert np.array_equal(got[pb + 288:pb + 288 + 4 * 49].view("<u4"), wr) and np.array_equal(got[pb + 496:].view("<i8").reshape(48, 64), wR), i
        assert (got[pb + 288 + 4 * 49:pb + 496] == SENTINEL).all()
    ctx.close_stream(sa)


CASES = ["golden", "seams", "narrow", "ties", "arithmetic", "cap", "margin_and_thresholds", "mixed", "chain", "refusals"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "corners", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_corners(case, child_results):
    gpu_child.report(case, child_results)
