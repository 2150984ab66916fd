"""GPU: bilateral filters in slot layout (hvq_bilateral_pictures / Context.bilateral_pictures, Context.smooth_pictures) against
hvqm4_amd.bilateral.of_picture -- which tests/test_bilateral_cpu.py holds equal to tests/bilateral_ref.py, the plain-Python restatement of
include/hvqm4_amd.h -- and against footprints painted without any window arithmetic, compared with ==.  Every output is allocated with
256 sentinel bytes before and behind it, which must stay untouched.  The shapes are those of the golden clips: 64 x 48 4:2:0, 48 x 64
4:4:4 and 296 x 160 4:2:2, whose chroma planes are 148 wide, so that every plane crosses a seam of the kernel's 64-column tiles; the
smallest geometry hvq_stream_open accepts; 8 x 8.  The cases run in ONE child process that imports torch first (see
tests/gpu_child.py); each test reports its case.  The child stops at the first HVQ_E_HIP or HIP error: nothing more is started on
a GPU that has reported a fault."""
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
def _bil(torch, ctx, sids, ords, bil, src=None, guide=None, steps=None):
    """one call (or smooth_pictures with `steps`) into guarded rooms -> (list of uint8 tensors, guards)"""
    uniform = len({ctx._geometry(s) for s in set(sids)}) <= 1
    out, guards = gpu_kit.rooms(torch, [ctx.pic_bytes(s) for s in sids], uniform)
    got = ctx.smooth_pictures(sids, ords, steps, guide=guide, out=out) if steps is not None else ctx.bilateral_pictures(sids, ords, bil, guide, src, out)
    assert got is out
    return [out[i] for i in range(len(sids))], guards


_expected = {}


def _want(pic, geom, bil, guide=None):
    """the expected bytes of one picture: computed once, shared by the cases that repeat it, left unchanged"""
    from hvqm4_amd import bilateral as B
    key = (zlib.crc32(np.asarray(pic).tobytes()), geom, bil, None if guide is None else zlib.crc32(np.asarray(guide).tobytes()))
    if key not in _expected:
        _expected[key] = B.of_picture(pic, geom, bil, guide)
    return _expected[key]


def _general(torch, ctx, sids, ords, bils, src, guide, got, what):
    """the same call with the copy body switched off: the same bytes; the setting is returned and restored"""
    was = ctx.bilateral_force_general(True)
    assert was is False, what
    again, guards = _bil(torch, ctx, sids, ords, bils, src, guide)
    torch.cuda.synchronize()
    assert ctx.bilateral_force_general(was) is True and ctx.bilateral_force_general(False) is False, what
    _check(torch, again, guards, [g.cpu().numpy() for g in got], what + ": the general body everywhere")


class _Uploaded(gpu_kit.Uploaded):
    def run(self, torch, bils, what, wants=None, general=False, guides=None):
        """the pictures in ONE call, bils[i] for picture i (guides[i]: None or a picture as numpy bytes), compared with `wants`
        (default: the module's bytes)"""
        n = len(self.sids)
        gbufs = None if guides is None else [None if g is None else torch.from_numpy(np.array(g, dtype=np.uint8)).cuda() for g in guides]
        got, guards = _bil(torch, self.ctx, self.sids, [-1] * n, bils, src=self.bufs, guide=gbufs)
        torch.cuda.synchronize()
        if wants is None:
            wants = [_want(p, g, b, None if guides is None else guides[i]) for i, (p, g, b) in enumerate(zip(self.pics, self.geoms, bils))]
        _check(torch, got, guards, wants, what)
        if general:
            _general(torch, self.ctx, self.sids, [-1] * n, bils, self.bufs, gbufs, got, what)
        return got


def case_golden(torch, ctx):
    """every golden clip's pictures under the five shared sets and the identity, and all of it again with the copy body switched off"""
    from hvqm4_amd import bilateral as B
    from tests import bilateral_cases as cases
    samplings = set()
    sets = [b for _l, b in cases.FIVE] + [B.identity()]
    assert sets[0] == B.bilateral(1.5, 12) and sets[1] == B.sigma_filter(2, 10) and sets[2] == B.box((3, 1)) and sets[3] == B.disc(3) and B.copies(sets[4].chroma)
    for name, data, _hdr, _n in _golden():
        sid, hdr, n = _decode(ctx, data)
        g = _geom(hdr)
        samplings.add(g[2:])
        sids, ords, bils = [sid] * (n * len(sets)), [k for k in range(n) for _ in sets], sets * n
        got, guards = _bil(torch, ctx, sids, ords, bils)
        torch.cuda.synchronize()
        pics = [ctx.read_picture(sid, k) for k in range(n)]
        _check(torch, got, guards, [_want(pics[k], g, b) for k, b in zip(ords, bils)], name)
        _general(torch, ctx, sids, ords, bils, None, None, got, name)
        ctx.close_stream(sid)
    assert samplings == {(2, 2), (2, 1), (1, 1)}


def case_seams(torch, ctx):
    """296 x 160 4:2:2, planes of zeros with single 255s at the columns 0, 1, 62, 63, 64, 65, 127, 128, last and the rows 0, 15, 16, 17,
    last, under flat tables with five radii, and the mirror case: for the interior points the clipped rectangles exactly, painted by
    counting; the points on the border against the module"""
    from hvqm4_amd import bilateral as B
    from tests import bilateral_cases as cases
    g = cases.SEAM_GEOM
    pics, bils, wants = [], [], []
    seen = set()
    for rx, ry in cases.FOOTPRINT_RADII:
        for part in range(3):
            for bg, dot in ((0, 255), (255, 0)):
                pic, pts = cases.dotted(g, part, bg, dot, border=False)
                assert all(len(p) >= 4 for p in pts)
                seen |= {c for p in pts[1:] for _r, c in p}
                pics.append(pic); bils.append(B.box((rx, ry))); wants.append(cases.footprints(g, pts, rx, ry, bg, dot))
                pic, pts = cases.dotted(g, part, bg, dot, border=True)
                seen |= {c for p in pts[1:] for _r, c in p}
                pics.append(pic); bils.append(B.box((rx, ry))); wants.append(_want(pic, g, B.box((rx, ry))))
    assert seen == {0, 1, 62, 63, 64, 65, 127, 128, 147}
    up = _Uploaded(torch, ctx, pics, [g] * len(pics))
    up.run(torch, bils, "footprints", wants=wants)
    for pic, b, w in zip(pics[:6:2], bils[:6:2], wants[:6:2]):                   # the painted rectangles are what the module says too
        assert np.array_equal(_want(pic, g, b), w)
    # a single interior 255 in zeros: (255 s + den / 2) / den inside its rectangle, 0 outside
    one = np.zeros(cases.nbytes(g), dtype=np.uint8)
    one[296 * 16 + 64] = 255
    got = up.ctx.bilateral_pictures(up.sids[:1], [-1], B.box((7, 3)), src=[torch.from_numpy(one).cuda()])
    torch.cuda.synchronize()
    y = got[0].cpu().numpy()[:296 * 160].reshape(160, 296)
    assert (255 + 105 // 2) // 105 == 2 and set(y[13:20, 57:72].reshape(-1).tolist()) == {2} and int(y.astype(np.int64).sum()) == 2 * 105
    up.close()


def case_narrow(torch, ctx):
    """planes narrower than the halo and than the window: radius 7 on the 32 x 24 and 24 x 32 chroma planes, on the smallest geometry
    hvq_stream_open accepts and on 8 x 8, through src=; both bodies"""
    from hvqm4_amd import bilateral as B
    from tests import bilateral_cases as cases
    geoms = [(64, 48, 2, 2), (48, 64, 2, 2), cases.SMALLEST, (8, 8, 2, 1), (8, 8, 1, 1)]
    bils = [B.bilateral(3.0, 30, 7), B.box(7), B.sigma_filter((7, 0), 40), B.sigma_filter((0, 7), 2), B.Bilateral(cases.random_set(8, 7, 7), cases.random_set(9, 7, 5)), B.disc(7, sigma_range=9.0),
            B.identity(), B.from_tables(0, 0, [[3]], [200] * 256)]
    pics, gs, bs = [], [], []
    for i, g in enumerate(geoms):
        for j, b in enumerate(bils):
            pics.append(cases.made(g, "random" if j % 2 else "ties", i + j)); gs.append(g); bs.append(b)
    up = _Uploaded(torch, ctx, pics, gs)
    up.run(torch, bs, "narrow planes", general=True)
    up.close()


def case_arithmetic(torch, ctx):
    """the directed arithmetic set: the largest weights on planes of 255 and on checkerboards, one 254 in 255s, den == 1, ties exactly
    at one half, planes valued 0 .. 3"""
    from tests import bilateral_cases as cases
    arith = cases.arithmetic()
    assert {l.split("/")[0] for l, *_r in arith} >= {"all255", "den1", "half", "small"}
    up = _Uploaded(torch, ctx, [pic for _l, _g, pic, _b in arith], [g for _l, g, _p, _b in arith])
    got = up.run(torch, [b for *_r, b in arith], "directed arithmetic")
    assert set(got[0].cpu().numpy().tolist()) == {255}
    up.close()


def case_guides(torch, ctx):
    """a copy of the picture by pointer as its guide == no guide; a resident guide of another ordinal; a flat guide == the linear filter
    (the {4, 2; 2, 1} quadrant: filters.binomial(3)); guided and unguided pictures mixed in one call"""
    from hvqm4_amd import bilateral as B
    from hvqm4_amd import filters as F
    sid, hdr, n = _decode(ctx, _clip("yuv422_296x160"))
    g = _geom(hdr)
    pics = [ctx.read_picture(sid, k) for k in range(n)]
    nb = ctx.pic_bytes(sid)
    b = B.chroma_for(B.bilateral(2.0, 10, 4), *g[2:])
    copies = [torch.from_numpy(p.copy()).cuda() for p in pics]
    flat = torch.full((nb,), 77, dtype=torch.uint8, device="cuda")
    quad = B.from_tables(1, 1, [[4, 2], [2, 1]], [255, 3] + [0] * 254)      # not linear without a guide: range falls to 0 at once
    sids, ords, bils, guide, wants = [], [], [], [], []
    for k in range(n):
        for gd, gpic in ((None, None), (copies[k], pics[k]), ((sid, (k + 1) % n), pics[(k + 1) % n])):
            sids.append(sid); ords.append(k); bils.append(b); guide.append(gd); wants.append(_want(pics[k], g, b, gpic))
        sids.append(sid); ords.append(k); bils.append(quad); guide.append(flat); wants.append(F.of_picture(pics[k], g, F.binomial(3)))
        sids.append(sid); ords.append(k); bils.append(quad); guide.append(None); wants.append(_want(pics[k], g, quad))
    got, guards = _bil(torch, ctx, sids, ords, bils, guide=guide)
    torch.cuda.synchronize()
    _check(torch, got, guards, wants, "guided and unguided pictures in one call")
    for k in range(n):
        assert torch.equal(got[5 * k], got[5 * k + 1]), "a copy of the picture as its guide"
        assert not torch.equal(got[5 * k], got[5 * k + 2]) and not torch.equal(got[5 * k + 3], got[5 * k + 4]), "another guide, other bytes"
    _general(torch, ctx, sids, ords, bils, None, guide, got, "guides")
    ctx.close_stream(sid)


def case_planes(torch, ctx):
    """different luma and chroma sets, luma_only copying the chroma planes"""
    from hvqm4_amd import bilateral as B
    from tests import bilateral_cases as cases
    bils = [B.luma_only(B.bilateral(2.0, 20, 5)), B.luma_only(B.box((4, 2))), B.Bilateral(B.disc(3).luma, B.sigma_filter((2, 6), 25).luma), B.Bilateral(B.IDENTITY_PLANE, B.bilateral(1.0, 9).luma),
             B.chroma_for(B.bilateral(3.0, 15, 6), 2, 1), B.Bilateral(cases.random_set(10, 6, 1), cases.random_set(11, 1, 6))]
    pics, gs, bs = [], [], []
    for i, g in enumerate(cases.SHAPES):
        for j, b in enumerate(bils):
            pics.append(cases.made(g, "random", 10 * i + j)); gs.append(g); bs.append(b)
    up = _Uploaded(torch, ctx, pics, gs)
    got = up.run(torch, bs, "luma and chroma differ", general=True)
    g = cases.SHAPES[0]
    assert np.array_equal(got[0].cpu().numpy()[g[0] * g[1]:], pics[0][g[0] * g[1]:]), "luma_only copies the chroma planes"
    assert not np.array_equal(got[0].cpu().numpy()[:g[0] * g[1]], pics[0][:g[0] * g[1]])
    up.close()


def case_many(torch, ctx):
    """300 mixed pictures of the three shapes in one call with 64 distinct sets, every third guided; separately, 65 sets are refused"""
    from hvqm4_amd import bilateral as B
    from hvqm4_amd._lib import HVQ_E_ARG
    from tests import bilateral_cases as cases
    table = cases.table64()
    shapes = (cases.SHAPES[0], cases.SHAPES[1], (72, 24, 2, 1))
    base = {g: [cases.made(g, kind, 3) for kind in ("random", "ties", "check1")] for g in shapes}
    pics, gs, bs, guides = [], [], [], []
    for i in range(300):
        g = shapes[i % 3]
        pics.append(base[g][(i // 3) % 3]); gs.append(g); bs.append(table[(i * 7 + i // 64) % 64])
        guides.append(base[g][(i // 3 + 1) % 3] if i % 3 == 2 else None)
    assert len(set(bs)) == 64
    up = _Uploaded(torch, ctx, pics, gs)
    up.run(torch, bs, "300 pictures, 64 sets", guides=guides)
    with pytest.raises(ValueError, match="65 distinct"):
        ctx.bilateral_pictures(up.sids[:65], [-1] * 65, table + [B.box((7, 6))], src=up.bufs[:65])
    assert _raw(torch, ctx, [up.sids[0]] * 2, [-1, -1], [up.bufs[0].data_ptr()] * 2, [t.struct() for t in table] + [B.box(1).struct()], which=[0, 64]) == (HVQ_E_ARG, True)
    up.close()


def case_sources(torch, ctx):
    """src= beside resident pictures; two calls through src= equal of_steps; smooth_pictures(iterate(b, 3)); bilateral ->
    picture_checksums(src=) equals the CRC of the expected bytes"""
    from hvqm4_amd import bilateral as B
    sid, hdr, n = _decode(ctx, _clip("yuv422_296x160"))
    g = _geom(hdr)
    n = min(n, 6)
    pics = [ctx.read_picture(sid, k) for k in range(n)]
    other = [np.roll(p, 7) for p in pics]
    bufs = [torch.from_numpy(p.copy()).cuda() for p in other]
    b = B.chroma_for(B.sigma_filter(4, 12), *g[2:])
    sids, ords, src = [sid] * (2 * n), [k for k in range(n)] + [-1] * n, [None] * n + bufs
    got, guards = _bil(torch, ctx, sids, ords, b, src)
    torch.cuda.synchronize()
    _check(torch, got, guards, [_want(p, g, b) for p in pics + other], "resident pictures and sources in one call")
    # two calls through src=, nothing waited for in between
    steps = [B.bilateral(1.5, 12), B.box(1)]
    first = ctx.bilateral_pictures([sid] * n, list(range(n)), steps[0])
    second, guards = _bil(torch, ctx, [sid] * n, [-1] * n, steps[1], [first[i] for i in range(n)])
    sums = ctx.picture_checksums([sid] * n, [-1] * n, src=second)
    three_steps = B.iterate(B.chroma_for(B.bilateral(1.5, 20, 2), *g[2:]), 3)
    thrice, tguards = _bil(torch, ctx, [sid] * n, list(range(n)), None, steps=three_steps)
    one, oguards = _bil(torch, ctx, [sid] * n, list(range(n)), None, steps=[B.disc(2)])
    guided = ctx.smooth_pictures([sid] * n, list(range(n)), B.iterate(B.sigma_filter(2, 6), 2), guide=[(sid, 0)] * n)
    torch.cuda.synchronize()
    want = [B.of_steps(p, g, steps) for p in pics]
    _check(torch, second, guards, want, "bilateral -> bilateral through src=")
    assert [int(v) for v in sums.cpu().numpy()[:, 3]] == [zlib.crc32(w.tobytes()) for w in want], "bilateral -> picture_checksums(src=)"
    _check(torch, thrice, tguards, [B.of_steps(p, g, three_steps) for p in pics], "smooth_pictures(iterate(b, 3))")
    _check(torch, one, oguards, [_want(p, g, B.disc(2)) for p in pics], "smooth_pictures of one step")
    _check(torch, [guided[i] for i in range(n)], [], [B.of_steps(p, g, B.iterate(B.sigma_filter(2, 6), 2), pics[0]) for p in pics], "two guided steps through two scratch tensors")
    ctx.close_stream(sid)


def _raw(torch, ctx, sids, ords, src, structs, which=None, nsets=None, count=None, ctx_h=None, ptr=None, null_sets=False, guide=None):
    """hvq_bilateral_pictures through the C ABI into sentinel-filled memory -> (return code, every byte still holds the sentinel).
    structs: the HvqBilateral table; ptr: the destination pointer of picture 0 instead of the room's; guide: (stream, ordinal, pointer)
    per picture"""
    import ctypes as C
    from hvqm4_amd._lib import HvqBilateral, lib
    from hvqm4_amd.metrics import HvqMetricsRef
    n = len(sids)
    room = torch.full((n, 8192), SENTINEL, dtype=torch.uint8, device="cuda")
    a_d = (C.c_void_p * n)(*[(ptr if ptr is not None and i == 0 else room[i].data_ptr()) for i in range(n)])
    a_p = C.cast((C.c_void_p * n)(*src), C.c_void_p) if src is not None else None
    a_g = C.cast((HvqMetricsRef * n)(*[HvqMetricsRef(s, o, p) for s, o, p in guide]), C.c_void_p) if guide is not None else None
    a_b = (HvqBilateral * len(structs))(*structs)
    a_w = C.cast((C.c_int * n)(*which), C.c_void_p) if which is not None else None
    rc = lib().hvq_bilateral_pictures(ctx._h if ctx_h is None else ctx_h, n if count is None else count, (C.c_int * n)(*sids), (C.c_int * n)(*ords), a_p, a_g,
                                      None if null_sets else C.cast(a_b, C.c_void_p), len(structs) if nsets is None else nsets, a_w, C.cast(a_d, C.c_void_p),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, bool(room.eq(SENTINEL).all())


def case_refusals(torch, ctx):
    """every refusal of the header through the C entry leaves the destinations untouched, also those of the well-formed pictures of
    the same call"""
    import ctypes as C
    from hvqm4_amd import bilateral as B
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_STATE
    from hvqm4_amd.container import video_pictures
    from tests.test_bilateral_cpu import _spoiled
    data = _clip("gop64x48_15")
    sa, hdr, n = _decode(ctx, data)
    assert ctx.pic_bytes(sa) <= 8192
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    sd = ctx.open_stream(hdr.width, hdr.height, 2, 2, hdr.is15, 3)
    for ft, p in pics:
        ctx.submit(sd, ft, p)
    ctx.flush()                                                  # picture 0 of sd: its slot of the ring of 3 was reused
    sq = ctx.open_stream(hdr.width, hdr.height, 2, 2, hdr.is15, 3)
    so, _ohdr, _on = _decode(ctx, _clip("yuv444_64x48"))         # another geometry
    mem = torch.zeros(ctx.pic_bytes(sa) + 32, dtype=torch.uint8, device="cuda")
    p16 = mem.data_ptr() + (-mem.data_ptr()) % 16
    good = B.bilateral(1.5, 12).struct()
    two = [sa, sa]
    labels = [l for l, _s in _spoiled()]
    assert {"radius 8", "a negative radius", "spatial[0][0] == 0", "range[0] == 0", "pad"} <= set(labels)
    for label, s in _spoiled():                                  # every refusal of hvq_bilateral_check, in an unused entry of the table and in a used one
        assert _raw(torch, ctx, two, [0, 1], None, [good, s], which=[0, 0]) == (HVQ_E_ARG, True), label
        assert _raw(torch, ctx, two, [0, 1], None, [s]) == (HVQ_E_ARG, True), label
    me = (-1, 0, None)
    arg = [("bad stream", [sa, 99], [0, 0], None, {}), ("an ordinal that is not resident", two, [0, 1000], None, {}), ("negative ordinal", two, [0, -1], None, {}),
           ("misaligned src", two, [0, -1], [None, p16 + 8], {}), ("an ordinal with src", two, [0, 1], [None, p16], {}),
           ("src with a bad stream", [sa, 99], [0, -1], [None, p16], {}), ("which beyond the table", two, [0, 1], None, {"which": [0, 1]}),
           ("a negative which", two, [0, 1], None, {"which": [0, -1]}), ("nsets 0", two, [0, 1], None, {"nsets": 0}), ("nsets -1", two, [0, 1], None, {"nsets": -1}),
           ("null sets", two, [0, 1], None, {"null_sets": True}), ("null context", two, [0, 1], None, {"ctx_h": C.c_void_p(0)}),
           ("null dst", two, [0, 1], None, {"ptr": 0}), ("misaligned dst", two, [0, 1], None, {"ptr": p16 + 8}),
           ("a guide of another geometry", two, [0, 1], None, {"guide": [me, (so, 0, None)]}), ("a guide with stream and pointer", two, [0, 1], None, {"guide": [me, (sa, 0, p16)]}),
           ("a misaligned guide", two, [0, 1], None, {"guide": [me, (-1, 0, p16 + 8)]}), ("a guide of stream -2", two, [0, 1], None, {"guide": [me, (-2, 0, None)]}),
           ("a guide of a bad stream", two, [0, 1], None, {"guide": [me, (99, 0, None)]}), ("a guide of a bad ordinal", two, [0, 1], None, {"guide": [me, (sa, 1000, None)]})]
    for what, sids, ords, src, kw in arg:
        assert _raw(torch, ctx, sids, ords, src, [good], **kw) == (HVQ_E_ARG, True), what
    assert _raw(torch, ctx, two, [0, 1], None, [good] * 65, which=[0, 64]) == (HVQ_E_ARG, True), "nsets 65"
    assert _raw(torch, ctx, [sa], [0], None, [good], count=65536) == (HVQ_E_ARG, True), "n beyond 65535"
    assert _raw(torch, ctx, [sa], [0], None, [good], count=0) == (0, True), "n == 0 does nothing"
    # the HVQ_E_STATE cases: a dropped picture (its slot was reused), as a source and as a guide; a picture queued but not flushed
    assert _raw(torch, ctx, [sa, sd], [0, 0], None, [good]) == (HVQ_E_STATE, True), "a dropped picture"
    assert _raw(torch, ctx, two, [0, 1], None, [good], guide=[me, (sd, 0, None)]) == (HVQ_E_STATE, True), "a dropped guide"
    ctx.submit(sq, pics[0][0], pics[0][1])
    assert _raw(torch, ctx, [sa, sq], [0, 0], None, [good]) == (HVQ_E_STATE, True), "queued but not flushed"
    assert _raw(torch, ctx, two, [0, 1], None, [good], guide=[me, (sq, 0, None)]) == (HVQ_E_STATE, True), "a guide queued but not flushed"
    ctx.flush()
    # the well-formed calls right after them work: a table of 64 with the last one used and a guide, and the method
    rc, untouched = _raw(torch, ctx, two, [0, 1], None, [good] * 64, which=[0, 63], guide=[me, (sa, 0, None)])
    assert rc == 0 and not untouched
    g = _geom(hdr)
    b = B.sigma_filter(2, 10)
    got, guards = _bil(torch, ctx, [sa, sd, sq], [1, len(pics) - 1, 0], b, guide=[None, (sa, 0), None])
    torch.cuda.synchronize()
    three = [ctx.read_picture(s, o) for s, o in ((sa, 1), (sd, len(pics) - 1), (sq, 0))]
    _check(torch, got, guards, [_want(three[0], g, b), _want(three[1], g, b, ctx.read_picture(sa, 0)), _want(three[2], g, b)], "after the refusals")
    for s in (sa, sd, sq, so):
        ctx.close_stream(s)


def case_tools(torch, ctx):
    """tools/denoise.py on a golden clip: three bilateral steps, then encode_jpeg(src=): the files of the expected pictures"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import denoise
    from hvqm4_amd import bilateral as B
    from hvqm4_amd import jpeg
    from oracle import bridge
    data = _clip("yuv422_64x48")
    geom, files = denoise.clip_denoised(ctx, data, sigma_space=2.0, sigma_range=15.0, radius=None, iterations=3, quality=80)
    assert geom == (64, 48, 2, 1)
    steps = denoise.steps_for(2.0, 15.0, None, 3, None, 2, 1)
    assert steps == [B.chroma_for(B.bilateral(2.0, 15.0, 4), 2, 1)] * 3
    pics = bridge.oracle_decode(data, len(files))
    for k, f in enumerate(files):
        assert f == jpeg.encode(B.of_steps(pics[k].reshape(-1), geom, steps), 64, 48, 80, 2, 1), k
    assert denoise.steps_for(1.5, 12.0, 2, 1, 9, 2, 2) == [B.chroma_for(B.sigma_filter(2, 9), 2, 2)]
    _g, surf = denoise.clip_denoised(ctx, data, radius=3, surface=8, quality=80)
    assert surf[0] == jpeg.encode(B.of_steps(pics[0].reshape(-1), geom, [B.chroma_for(B.sigma_filter(3, 8), 2, 1)]), 64, 48, 80, 2, 1)


CASES = ["golden", "seams", "narrow", "arithmetic", "guides", "planes", "many", "sources", "refusals", "tools"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "bilateral", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_bilateral(case, child_results):
    gpu_child.report(case, child_results)
