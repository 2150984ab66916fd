"""GPU: composed pictures in slot layout (hvq_compose_pictures / Context.compose_pictures) against tests/compose_ref.py, the plain-Python
restatement of include/hvqm4_amd.h, compared with ==.  Every output is allocated with 256 sentinel bytes before and behind it, which
must stay untouched.  The shapes are those of the golden clips: 64 x 48 4:2:0, 48 x 64 4:4:4 and 296 x 160 4:2:2, whose chroma planes
are 148 wide, so that every plane crosses a seam of the kernel's 64-column tiles.  The cases run in ONE child process that imports
torch first (see tests/gpu_child.py); each test reports its case.  The child stops at the first HVQ_E_HIP or HIP error: nothing
more is started on a GPU that has reported a fault."""
import json
import os
import sys
import zlib

import numpy as np
import pytest

from tests import gpu_child, gpu_kit
from tests.gpu_kit import GUARD, ROOT, SENTINEL, check_bytes as _check, clip as _clip, decode as _decode, geom as _geom

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300                                 # the cases take seconds each; a hung child is ended, not waited for
SHAPES = ((64, 48, 2, 2), (48, 64, 1, 1), (296, 160, 2, 1))


# ------------------------------------------------------------------------------------------------------------- child side
def _nbytes(g):
    from hvqm4_amd import scale
    return scale.nbytes(*g)


def _compose(torch, ctx, sids, ords, targets, src=None):
    """one call -> (list of uint8 tensors, guards)"""
    out, guards = gpu_kit.geometry_rooms(torch, [t.geometry() for t in targets])
    got = ctx.compose_pictures(sids, ords, targets, src, out)
    assert got is out
    return [out[i] for i in range(len(targets))], guards


def _contents(g, seed):
    """pictures of geometry g: random, and a 0 / 255 checkerboard in every plane"""
    rng = np.random.default_rng(seed)
    w, h, hs, vs = g
    board = []
    for pw, ph in ((w, h), (w // hs, h // vs), (w // hs, h // vs)):
        y, x = np.mgrid[0:ph, 0:pw]
        board.append((((x + y + seed) & 1) * 255).astype(np.uint8).reshape(-1))
    return rng.integers(0, 256, _nbytes(g), dtype=np.uint8), np.concatenate(board)


_expected = {}


def _want(pics, geoms, t):
    """the reference's bytes of one target: computed once, shared by the cases that repeat a target (the bodies), left unchanged"""
    from tests import compose_ref as ref
    used = sorted({l.source for l in t.layers})
    key = (t, tuple((i, geoms[i], zlib.crc32(np.asarray(pics[i]).tobytes())) for i in used))
    if key not in _expected:
        _expected[key] = ref.compose_picture([np.asarray(p).tobytes() if i in used else b"" for i, p in enumerate(pics)], geoms, ref.as_ref(t))
    return _expected[key]


class _Uploaded(gpu_kit.Uploaded):
    def run(self, torch, targets, what, general=None):
        """the targets in ONE call, compared with the reference; general: also under that setting of force_general, equal"""
        got, guards = _compose(torch, self.ctx, self.sids, [-1] * len(self.sids), targets, src=self.bufs)
        torch.cuda.synchronize()
        _check(torch, got, guards, [_want(self.pics, self.geoms, t) for t in targets], what)
        if general is not None:
            was = self.ctx.compose_force_general(general)
            again, guards = _compose(torch, self.ctx, self.sids, [-1] * len(self.sids), targets, src=self.bufs)
            torch.cuda.synchronize()
            assert self.ctx.compose_force_general(was) == bool(general)
            _check(torch, again, guards, [g.cpu().numpy() for g in got], what + ": the general body everywhere")
        return got


def _shift(t, by):
    from tests import compose_cases as cases
    return cases.shifted(t, by)


def case_identity(torch, ctx):
    """the copy recipe in every sampling, on the three shapes and on the smallest geometry: the source itself; both bodies"""
    from hvqm4_amd import compose as cp
    geoms = list(SHAPES) + [(8, 8) + s for s in ((2, 2), (2, 1), (1, 1))]
    pics = [_contents(g, 3 + i)[0] for i, g in enumerate(geoms)]
    up = _Uploaded(torch, ctx, pics, geoms)
    got = up.run(torch, [cp.copy(g, i) for i, g in enumerate(geoms)], "identity", general=True)
    for g, p in zip(got, pics):
        assert np.array_equal(g.cpu().numpy(), p), "the copy is not the picture"
    up.close()


def case_known(torch, ctx):
    """the known answers of the header"""
    from hvqm4_amd import compose as cp
    from hvqm4_amd import scale as sc
    for g in SHAPES:
        a, b = _contents(g, 11)[0], _contents(g, 12)[0]
        one, three = np.full(a.size, 1, np.uint8), np.full(a.size, 3, np.uint8)
        up = _Uploaded(torch, ctx, [a, b, a.copy(), one, three], [g] * 5)
        size, samp = g[:2], g[2:]
        hs, vs = samp
        over = cp.overlay(g, 3 * hs, vs, (16 * hs, 10 * vs), 77)
        put = cp.Target(size, samp, (cp.Layer(0, cp.ADD, 3), cp.Layer(0, cp.ADD, 2), cp.Layer(1, cp.PUT, 1, (0, 0, 8 * hs, 8 * vs), (3 * hs, 5 * vs))))
        targets = [cp.copy(g), cp.Target(size, samp, (cp.Layer(0, cp.ADD), cp.Layer(1, cp.ADD)), 1), cp.difference(g, 1, 0, 2),
                   cp.Target(size, samp, (cp.Layer(3, cp.ADD, -1),), 1, 10), cp.Target(size, samp, (cp.Layer(4, cp.ADD, -1),), 1, 10),
                   put, cp.Target(size, samp, (), 4, (16, 128, 255)), over]
        got = [t.cpu().numpy() for t in up.run(torch, targets, f"known answers {g}", general=True)]
        assert np.array_equal(got[0], a)
        assert np.array_equal(got[1], ((a.astype(int) + b + 1) >> 1).astype(np.uint8))
        assert set(got[2]) == {128} and set(got[3]) == {10} and set(got[4]) == {9}, "equal pictures; acc -1 -> 0 and acc -3 -> -1 under shift 1"
        pa, pb, pp, po = (sc.planes(v, *g) for v in (a, b, got[5], got[7]))
        for p in range(3):
            x, y, w, h = (3, 5, 8, 8) if p else (3 * hs, 5 * vs, 8 * hs, 8 * vs)
            want = np.clip(5 * pa[p].astype(int), 0, 255)
            want[y:y + h, x:x + w] = pb[p][:h, :w]
            assert np.array_equal(pp[p], want), "a PUT above ADDs discards them inside its rectangle only"
            x, y, w, h = (3, 1, 16, 10) if p else (3 * hs, vs, 16 * hs, 10 * vs)
            want = pa[p].astype(int)
            want[y:y + h, x:x + w] = (pa[p][y:y + h, x:x + w].astype(int) * (256 - 77) + pb[p][:h, :w].astype(int) * 77 + 128) >> 8
            assert np.array_equal(po[p], want), "the overlay: one rounding"
        assert np.array_equal(got[6], cp.flat_picture(size, samp, (16, 128, 255))), "count == 0"
        up.close()


def case_seams(torch, ctx):
    """rectangles whose edges fall around the tile seams, at offsets of every residue mod 4, two samples wide and high, of one chroma
    sample: both bodies, random pictures and checkerboards"""
    from tests import compose_cases as cases
    for g in SHAPES:
        r, c = _contents(g, 21)
        r2, c2 = _contents(g, 22)
        up = _Uploaded(torch, ctx, [r, r2, c, c2], [g] * 4)
        up.run(torch, [cases.seam_target(g, 0, 1), cases.seam_target(g, 2, 3), cases.seam_target(g, 1, 2)], f"seams {g}", general=True)
        up.close()


def case_order(torch, ctx):
    """PUT over ADD over PUT with overlapping rectangles; the same layers reversed give the other bytes"""
    from tests import compose_cases as cases
    for g in SHAPES:
        up = _Uploaded(torch, ctx, [_contents(g, 31)[0], _contents(g, 32)[0]], [g] * 2)
        a, b = up.run(torch, cases.order_targets(g), f"order {g}", general=True)
        assert not bool(a.eq(b).all()), "the order of the layers matters"
        up.close()


def case_extremes(torch, ctx):
    """gain exactly 2^22 on 0 / 255 checkerboards with shift 22, weights of both signs that cancel, bias +-255, 256 layers in one target
    (a 16 x 16 mosaic of 8 x 8 cells on 128 x 128), count == 0"""
    from tests import compose_cases as cases
    for s in ((2, 2), (2, 1), (1, 1)):
        big, small = (128, 128) + s, (8, 8) + s
        pics = [_contents(big, 0)[1], _contents(big, 1)[1]] + [_contents(small, 40 + k)[k % 2] for k in range(256)]
        up = _Uploaded(torch, ctx, pics, [big, big] + [small] * 256)
        got = up.run(torch, cases.extreme_targets(s), f"extremes {s}", general=True)
        both = got[0].cpu().numpy()
        assert set(both) == {128}, "0 and 255 at half the gain each: (255 * 2^21 + 2^21) >> 22"
        assert np.array_equal(got[1].cpu().numpy(), pics[0]), "the full gain with shift 22 copies"
        up.close()


def case_many(torch, ctx):
    """300 targets of mixed geometries, samplings and recipes over the pictures of several streams in one call, with layer ranges that
    share layers (the library's first / count, through the C entry), and the method's own flattening"""
    import ctypes as C
    from hvqm4_amd import compose as cp
    from hvqm4_amd._lib import HvqComposeDst, HvqComposeLayer, check, lib
    names = ["gop64x48_15", "yuv444_13_portrait48x64", "ragged24x40", "yuv422_64x48", "ip8", "i16", "yuv422_296x160"]
    streams = [_decode(ctx, _clip(nm)) for nm in names]
    sids, ords, layers, spans, pics, geoms = [], [], [], [], [], []
    for sid, hdr, n in streams:
        g = _geom(hdr)
        hs, vs = g[2:]
        first = len(layers)
        for k in range(2 * n):
            pics.append(ctx.read_picture(sid, k % n)); geoms.append(g); sids.append(sid); ords.append(k % n)
            i = len(pics) - 1
            layers.append(cp.Layer(i, cp.ADD, (3, -1, 2, 1)[k % 4]) if k % 3 else
                          cp.Layer(i, cp.PUT, 2, (0, 0, g[0] // 2 // hs * hs, g[1] // 2 // vs * vs), (hs * (k % 3), vs * (k % 2))))
        spans.append((g, first, len(layers) - first))
    rows = []
    for i in range(300):
        g, first, n = spans[i % 6 if i % 40 else 6]                             # the large clip now and then: the reference is plain Python
        off = i // 8 % n
        rows.append((g, first + off, min(1 + (i // 3) % 4, n - off), i % 3, ((i % 5) * 20 - 40, 0, i % 7)))
    assert len({r[0] for r in rows}) >= 6 and len({r[0][2:] for r in rows}) == 3
    nb = [_nbytes(r[0]) for r in rows]
    rooms = [torch.full((b + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for b in nb]
    a_l = (HvqComposeLayer * len(layers))(*[HvqComposeLayer(*l.numbers()[:7], (C.c_int32 * 3)(*l.weights())) for l in layers])
    a_d = (HvqComposeDst * 300)(*[HvqComposeDst(rm.data_ptr() + GUARD, *g, first, count, shift, (C.c_int32 * 3)(*bias)) for rm, (g, first, count, shift, bias) in zip(rooms, rows)])
    nl = len(layers)
    check(lib().hvq_compose_pictures(ctx._h, nl, (C.c_int * nl)(*sids), (C.c_int * nl)(*ords), None, C.cast(a_l, C.c_void_p), 300, C.cast(a_d, C.c_void_p),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    targets = [cp.Target(g[:2], g[2:], tuple(layers[first:first + count]), shift, bias) for g, first, count, shift, bias in rows]
    wants = [_want(pics, geoms, t) for t in targets]
    _check(torch, [rm[GUARD:GUARD + b] for rm, b in zip(rooms, nb)], [rm[:GUARD] for rm in rooms] + [rm[GUARD + b:] for rm, b in zip(rooms, nb)], wants, "many, shared ranges")
    got, guards = _compose(torch, ctx, sids, ords, targets)                    # the method: a list, the target geometries differ
    torch.cuda.synchronize()
    _check(torch, got, guards, wants, "many, the method")
    # one target geometry: one tensor [n, bytes], given and not given
    one = [t for t in targets if t.geometry() == (64, 48, 2, 2)][:12]
    got, guards = _compose(torch, ctx, sids, ords, one)
    fresh = ctx.compose_pictures(sids, ords, one)
    torch.cuda.synchronize()
    _check(torch, got, guards, [_want(pics, geoms, t) for t in one], "one tensor, given")
    assert tuple(fresh.shape) == (len(one), 4608)
    _check(torch, list(fresh), [], [_want(pics, geoms, t) for t in one], "one tensor, returned")
    for sid, _h, _n in streams:
        ctx.close_stream(sid)


def case_sources(torch, ctx):
    """layers from resident pictures, from src= memory (16 bytes into an allocation too) and from the outputs of scale_pictures,
    filter_pictures and warp_pictures, never read back in between, in one call"""
    from hvqm4_amd import compose as cp
    from hvqm4_amd import filters, scale, warp
    sid, hdr, n = _decode(ctx, _clip("yuv422_64x48"))
    big, hb, nbig = _decode(ctx, _clip("yuv422_296x160"))
    g, gb = _geom(hdr), _geom(hb)
    res = [ctx.read_picture(sid, k) for k in range(3)]
    inv = 255 - np.asarray(res[1]).reshape(-1)
    room = torch.zeros(inv.size + 32, dtype=torch.uint8, device="cuda")
    off = (-room.data_ptr()) % 16 + 16
    room[off:off + inv.size] = torch.from_numpy(inv).cuda()
    blur, turn = filters.gaussian(1.5), warp.flip_h(64)
    scaled = ctx.scale_pictures([big], [0], g[:2])
    filtered = ctx.filter_pictures([sid], [2], blur)
    warped = ctx.warp_pictures([sid], [0], turn)
    pics = [res[0], res[1], inv, scale.of_picture(ctx.read_picture(big, 0), gb, g), filters.of_picture(res[2], g, blur), warp.of_picture(res[0], g, turn)]
    sids, ords = [sid] * 6, [0, 1, -1, -1, -1, -1]
    src = [None, None, room[off:off + inv.size], scaled[0], filtered[0], warped[0]]
    hs, vs = g[2:]
    q = (8 * hs, 4 * vs, 14 * hs, 15 * vs)                                     # two cells a row, three rows, a margin of the bias between them
    sheet = cp.Target(g[:2], g[2:], tuple(cp.Layer(i, cp.PUT, 1, q, (16 * hs * (i % 2) + hs, 16 * vs * (i // 2))) for i in range(6)), 0, (0, 0, 0))
    targets = [cp.average(g, 6), sheet, cp.difference(g, 2, 3, 4), cp.overlay(g, hs, vs, (20 * hs, 9 * vs), 200, base=5, top=2)]
    got, guards = _compose(torch, ctx, sids, ords, targets, src=src)
    torch.cuda.synchronize()
    _check(torch, got, guards, [_want(pics, [g] * 6, t) for t in targets], "resident, src= and the outputs of scale, filter and warp")
    ctx.close_stream(sid)
    ctx.close_stream(big)


def case_golden(torch, ctx):
    """every clip of tests/golden/compose.json decoded on the GPU, its first and last picture through the fixture's recipes in one call"""
    from tests import compose_cases as cases
    fixture = json.load(open(os.path.join(ROOT, "tests", "golden", "compose.json")))["clips"]
    manifest = json.load(open(os.path.join(ROOT, "tests", "golden", "manifest.json")))["clips"]
    assert set(fixture) == {nm for nm, c in manifest.items() if "file" in c}
    sids, ords, targets, crcs, streams = [], [], [], [], []
    for name, entry in sorted(fixture.items()):
        sid, hdr, n = _decode(ctx, open(os.path.join(ROOT, "tests", "golden", manifest[name]["file"]), "rb").read())
        streams.append(sid)
        assert _geom(hdr) == tuple(entry["geometry"])
        first = len(sids)
        sids += [sid, sid]; ords += [0, n - 1]
        for (label, tg, crc), (label2, t) in zip(entry["recipes"], cases.fixture_recipes(_geom(hdr))):
            assert label == label2 and tuple(tg) == t.geometry()
            targets.append(_shift(t, first)); crcs.append((name, label, crc))
    got, guards = _compose(torch, ctx, sids, ords, targets)
    torch.cuda.synchronize()
    for g in guards:
        assert bool(g.eq(SENTINEL).all())
    for t, (name, label, crc) in zip(got, crcs):
        assert zlib.crc32(t.cpu().numpy().tobytes()) == crc, (name, label)
    for s in streams:
        ctx.close_stream(s)


def case_ordering(torch, ctx):
    """tests/test_gpu_warp.py's ordering: the composed pictures of batch k on a side stream beside batch k + 1 in flight, batch k + 2
    into batch k's slots behind the call; work queued behind the call on the same stream sees the result; a picture of the batch in
    flight"""
    from hvqm4_amd import compose as cp
    from hvqm4_amd.container import parse_header, video_pictures
    from oracle import bridge
    data = _clip("gop64x48_15")
    hdr = parse_header(data)
    g = _geom(hdr)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    assert len(pics) == 7                            # I P B B P B B
    dec = [p.reshape(-1) for p in bridge.oracle_decode(data, 7)]
    fade = lambda i, j: cp.crossfade(g, 0.25, a=i, b=j)
    sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, 6)
    b = [pics[0:3], pics[3:5], pics[5:7]]
    sub = lambda part: ctx.submit_many_device([sid] * len(part), [ft for ft, _p in part], [p for _f, p in part])
    side = torch.cuda.Stream()
    sub(b[0]); ctx.flush_begin()
    sub(b[1]); ctx.flush_next()                      # batch 0 ended, batch 1 in flight
    side.wait_stream(torch.cuda.current_stream())
    first = [fade(0, 1), fade(1, 2), fade(2, 0)]
    with torch.cuda.stream(side):
        got, guards = _compose(torch, ctx, [sid] * 3, [2, 0, 1], first)
        copy = torch.stack(got).clone()              # queued behind the call on the same stream: it sees the result
    sub(b[2]); ctx.flush_next()                      # batch 1 ended, batch 2 in flight
    ctx.flush_end()                                  # batch 2 reconstructed: picture 6 lies in picture 0's slot of the ring of 6
    second = [fade(0, 1), fade(1, 2), fade(2, 3), fade(3, 0)]
    late, lguards = _compose(torch, ctx, [sid] * 4, [3, 4, 5, 6], second)
    torch.cuda.synchronize()
    want = [_want([dec[2], dec[0], dec[1]], [g] * 3, t) for t in first]
    _check(torch, got, guards, want, "batch 0 beside batch 1")
    _check(torch, list(copy), [], want, "a copy queued behind the call")
    _check(torch, late, lguards, [_want(dec[3:7], [g] * 4, t) for t in second], "batches 1 and 2")
    sub(b[0]); ctx.flush_begin()                     # a picture of the batch in flight: the call ends that batch itself
    got, guards = _compose(torch, ctx, [sid, sid], [7 + 2, 7 + 0], [fade(0, 1)])
    torch.cuda.synchronize()
    _check(torch, got, guards, [_want([dec[2], dec[0]], [g] * 2, fade(0, 1))], "a picture of the batch in flight")
    ctx.close_stream(sid)


def case_refusals(torch, ctx):
    """every refusal of the header through the C entry leaves the destinations untouched, also those of the well-formed targets of the
    same call; the well-formed call right after works"""
    import ctypes as C
    from hvqm4_amd import compose as cp
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_GEOMETRY, HVQ_E_STATE, HvqComposeDst, HvqComposeLayer, lib
    from hvqm4_amd.container import video_pictures
    data = _clip("gop64x48_15")
    sa, hdr, n = _decode(ctx, data)
    s444, _h4, _n4 = _decode(ctx, _clip("yuv444_64x48"))
    g = _geom(hdr)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    sd = ctx.open_stream(hdr.width, hdr.height, 2, 2, hdr.is15, 3)
    for ft, p in pics:
        ctx.submit(sd, ft, p)
    ctx.flush()                                                  # picture 0 of sd: its slot of the ring of 3 was reused
    sq = ctx.open_stream(hdr.width, hdr.height, 2, 2, hdr.is15, 3)
    mem = torch.zeros(ctx.pic_bytes(sa) + 32, dtype=torch.uint8, device="cuda")
    p16 = mem.data_ptr() + (-mem.data_ptr()) % 16
    room = torch.full((2, 16384), SENTINEL, dtype=torch.uint8, device="cuda")

    def raw(change=None, sids=None, ords=None, src=None, nlayers=None, ntargets=None, ctx_h=None, null=()):
        """the good call -- two targets, three layers; target 0 takes layers 0 and 1, target 1 layers 1 and 2 -- after `change(layers,
        dst)` -> (return code, every byte still holds the sentinel)"""
        layers = [[0, 0, 0, 0, 0, 0, 0, 2, 2, 2], [1, 8, 8, 16, 16, 32, 16, 1, 1, 1], [1, 0, 0, 0, 0, 0, 0, -3, -3, -3]]
        dst = [[room[0].data_ptr(), 64, 48, 2, 2, 0, 2, 1, 0, 0, 0], [room[1].data_ptr(), 64, 48, 2, 2, 1, 2, 2, 128, 128, 128]]
        if change:
            change(layers, dst)
        sids, ords = sids or [sa, sa, sa], ords or [0, 1, 2]
        a_l = (HvqComposeLayer * len(layers))(*[HvqComposeLayer(*l[:7], (C.c_int32 * 3)(*l[7:])) for l in layers])
        a_d = (HvqComposeDst * 2)(*[HvqComposeDst(*d[:8], (C.c_int32 * 3)(*d[8:])) for d in dst])
        k = len(sids)
        rc = lib().hvq_compose_pictures(ctx._h if ctx_h is None else ctx_h, len(layers) if nlayers is None else nlayers,
                                        None if "streams" in null else (C.c_int * k)(*sids), None if "ordinals" in null else (C.c_int * k)(*ords),
                                        C.cast((C.c_void_p * k)(*src), C.c_void_p) if src is not None else None, None if "layers" in null else C.cast(a_l, C.c_void_p),
                                        2 if ntargets is None else ntargets, None if "dst" in null else C.cast(a_d, C.c_void_p), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc, bool(room.eq(SENTINEL).all())

    def setl(i, j, v):
        return lambda L, D: L[i].__setitem__(j, v)

    def setd(i, j, v):
        return lambda L, D: D[i].__setitem__(j, v)

    def both(*fs):
        return lambda L, D: [f(L, D) for f in fs]

    MODE, SX, SY, W, H, DX, DY, WY, WU, WV = range(10)
    PTR, TW, TH, HS, VS, FIRST, COUNT, SHIFT, B0, B1, B2 = range(11)
    arg = {"a 4:4:4 layer in a 4:2:0 target": dict(sids=[sa, sa, s444]), "a 4:2:0 layer in a 4:4:4 target": dict(change=both(setd(1, HS, 1), setd(1, VS, 1))),
           "the source rectangle leaves in x": dict(change=setl(1, SX, 56)), "the source rectangle leaves in y": dict(change=setl(1, SY, 40)),
           "the landing rectangle leaves in x": dict(change=setl(1, DX, 56)), "the landing rectangle leaves in y": dict(change=setl(1, DY, 40)),
           "a whole source in a smaller target": dict(change=both(setd(0, TW, 32), setd(0, TH, 32))), "a whole source moved out": dict(change=setl(0, DY, 2)),
           "odd sx": dict(change=setl(1, SX, 9)), "odd w": dict(change=setl(1, W, 15)), "odd dx": dict(change=setl(1, DX, 33)),
           "odd sy": dict(change=setl(1, SY, 9)), "odd h": dict(change=setl(1, H, 15)), "odd dy": dict(change=setl(1, DY, 17)),
           "an empty rectangle": dict(change=setl(1, H, 0)), "w == 0 with sx": dict(change=both(setl(1, W, 0), setl(1, H, 0), setl(1, SY, 0))),
           "negative sx": dict(change=setl(1, SX, -2)), "negative dy": dict(change=setl(1, DY, -2)), "negative w": dict(change=setl(1, W, -16)),
           "mode 2": dict(change=setl(2, MODE, 2)), "mode -1": dict(change=setl(0, MODE, -1)),
           "gain above 2^22 in U": dict(change=both(setl(1, WU, cp.MAX_GAIN - 2), setl(2, WU, -3))),
           "shift above": dict(change=setd(1, SHIFT, 23)), "shift negative": dict(change=setd(0, SHIFT, -1)),
           "bias above": dict(change=setd(1, B2, 256)), "bias below": dict(change=setd(0, B0, -256)),
           "first negative": dict(change=setd(1, FIRST, -1)), "count negative": dict(change=setd(1, COUNT, -1)), "range beyond nlayers": dict(change=setd(1, FIRST, 2)),
           "first beyond nlayers": dict(change=both(setd(1, FIRST, 4), setd(1, COUNT, 0))),
           "a layer of no target is checked": dict(change=both(setd(1, FIRST, 0), setd(1, COUNT, 1), setl(2, SX, 2))),
           "ntargets beyond 65535": dict(ntargets=65536), "nlayers beyond 2^18": dict(nlayers=cp.MAX_TOTAL + 1), "negative nlayers": dict(nlayers=-1),
           "null ptr": dict(change=setd(1, PTR, 0)), "misaligned ptr": dict(change=setd(1, PTR, room[1].data_ptr() + 8)),
           "bad stream": dict(sids=[sa, sa, 99]), "an ordinal that is not resident": dict(ords=[0, 1, 1000]), "negative ordinal": dict(ords=[0, 1, -1]),
           "misaligned src": dict(ords=[0, 1, -1], src=[None, None, p16 + 8]), "an ordinal with src": dict(src=[None, None, p16]),
           "src with a bad stream": dict(sids=[sa, sa, 99], ords=[0, 1, -1], src=[None, None, p16]),
           "null context": dict(ctx_h=C.c_void_p(0)), "null streams": dict(null=("streams",)), "null ordinals": dict(null=("ordinals",)),
           "null layers": dict(null=("layers",)), "null dst": dict(null=("dst",))}
    for what, kw in arg.items():
        assert raw(**kw) == (HVQ_E_ARG, True), what
    many = lambda L, D: (L.extend([[1, 0, 0, 0, 0, 0, 0, 1, 1, 1]] * 254), D[1].__setitem__(FIRST, 0), D[1].__setitem__(COUNT, 257))
    assert raw(change=many, sids=[sa] * 257, ords=[0] * 257) == (HVQ_E_ARG, True), "257 layers in a target"
    for bad in ((60, 48, 2, 2), (64, 48, 1, 2), (64, 48, 3, 1), (0, 0, 2, 2), (8200, 48, 2, 2)):
        assert raw(change=both(*[setd(1, TW + i, v) for i, v in enumerate(bad)])) == (HVQ_E_GEOMETRY, True), bad
    assert raw(ntargets=0) == (0, True), "ntargets == 0 does nothing"
    # the HVQ_E_STATE cases: a slot that was reused, a picture queued but not flushed
    assert raw(sids=[sa, sa, sd]) == (HVQ_E_STATE, True), "an evicted picture"        # ordinal 2 of the ring of 3 after 7 pictures
    ctx.submit(sq, pics[0][0], pics[0][1])
    assert raw(sids=[sa, sa, sq], ords=[0, 1, 0]) == (HVQ_E_STATE, True), "queued but not flushed"
    ctx.flush()
    # the well-formed calls right after them work: the gain at its limit, and the method
    rc, untouched = raw(change=both(setl(1, WU, cp.MAX_GAIN - 2), setl(2, WU, -2)))
    assert rc == 0 and not untouched
    t = cp.difference(g, 3)
    got, guards = _compose(torch, ctx, [sa, sd, sq], [1, len(pics) - 1, 0], [t, _shift(t, 1)])
    torch.cuda.synchronize()
    three = [ctx.read_picture(s, o) for s, o in ((sa, 1), (sd, len(pics) - 1), (sq, 0))]
    _check(torch, got, guards, [_want(three, [g] * 3, t), _want(three, [g] * 3, _shift(t, 1))], "after the refusals")
    for s in (sa, sd, sq, s444):
        ctx.close_stream(s)


def case_composition(torch, ctx):
    """scale -> compose (a sheet over a flat background) -> encode_jpeg(src=): the file of the expected sheet, which decodes to the
    sheet's size; compose of a, b with difference() -> picture_histograms(src=): the |a - b| histogram folded around 128"""
    from hvqm4_amd import compose as cp
    from hvqm4_amd import jpeg, scale
    sn, hn, nn = _decode(ctx, _clip("natural128x96"))
    g = _geom(hn)
    n = min(nn, 6)
    cell = (64, 48)
    cells = ctx.scale_pictures([sn] * n, list(range(n)), cell)
    sheet = cp.mosaic(3, 2, cell, g[2:], gap=4, sources=range(n), flat=n)
    sg = sheet.geometry()
    flat_np = cp.flat_picture(sheet.size, g[2:], (16, 128, 128))
    sc_sid = ctx.open_stream(cell[0], cell[1], g[2], g[3], True, 3)
    sh_sid = ctx.open_stream(sg[0], sg[1], g[2], g[3], True, 3)
    made = ctx.compose_pictures([sc_sid] * n + [sh_sid], [-1] * (n + 1), [sheet], src=[cells[i] for i in range(n)] + [torch.from_numpy(flat_np).cuda()])
    files, lengths = ctx.encode_jpeg([sh_sid], [-1], quality=85, src=[made[0]])
    diff = ctx.compose_pictures([sn, sn], [0, n - 1], [cp.difference(g)])
    hist = ctx.picture_histograms([sn], [-1], src=[diff[0]])
    absd = ctx.picture_histograms([sn], [0], ref=[(sn, n - 1)])
    torch.cuda.synchronize()
    pics = [ctx.read_picture(sn, k) for k in range(n)]
    small = [scale.of_picture(p, g, cell + g[2:]) for p in pics]
    want = _want(small + [flat_np], [cell + g[2:]] * n + [sg], sheet)
    _check(torch, [made[0]], [], [want], "scale -> compose")
    file = jpeg.files(files, lengths)[0]
    assert file == jpeg.encode(np.frombuffer(want, np.uint8), sg[0], sg[1], 85, g[2], g[3]), "compose -> encode_jpeg(src=)"
    try:                                             # an independent decoder, judged as tests/test_jpeg_cpu.py judges it: against its own encode
        import io
        from PIL import Image
    except ImportError:
        assert jpeg.segments(file)[-1][0] == 0xD9, "a JPEG file"
    else:
        from tests.test_jpeg_cpu import _decode_ycc, _psnr
        Y, U, V = scale.planes(np.frombuffer(want, np.uint8), *sg)
        im = _decode_ycc(Image, file)
        assert im.size == sg[:2] and im.mode == "YCbCr"
        full = np.stack([Y, np.repeat(np.repeat(U, sg[3], 0), sg[2], 1), np.repeat(np.repeat(V, sg[3], 0), sg[2], 1)], -1)
        bio = io.BytesIO()
        Image.fromarray(full, "YCbCr").save(bio, "JPEG", quality=85, subsampling={(1, 1): 0, (2, 1): 1, (2, 2): 2}[sg[2:]])
        ours, theirs = _psnr(np.asarray(im)[..., 0], Y), _psnr(np.asarray(_decode_ycc(Image, bio.getvalue()))[..., 0], Y)
        print(f"the sheet at quality 85: luma PSNR {ours:.2f} dB, Pillow's own encode {theirs:.2f} dB")
        assert ours >= theirs - 0.5, "the file decodes to the sheet"
    h, a = hist.cpu().numpy()[0].astype(np.int64), absd.cpu().numpy()[0].astype(np.int64)
    for p in range(3):                               # a - b = d shows as 128 + d: bin d of |a - b| is the bins 128 + d and 128 - d; 0, 1 and 255 hold |d| >= 127
        folded = np.array([h[p][128]] + [h[p][128 + d] + h[p][128 - d] for d in range(1, 127)])
        assert np.array_equal(folded, a[p][:127]), p
        assert h[p][0] + h[p][1] + h[p][255] == a[p][127:].sum(), p
    ctx.close_stream(sc_sid); ctx.close_stream(sh_sid); ctx.close_stream(sn)


def case_tools(torch, ctx):
    """tools/contactsheet.py on a golden clip: one valid JPEG of the expected size, the file of the expected sheet"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import contactsheet
    from hvqm4_amd import compose as cp
    from hvqm4_amd import jpeg, scale
    from oracle import bridge
    data = _clip("gop64x48_15")
    geom, file, ordinals = contactsheet.clip_sheet(ctx, data, 80, cols=2, cell=(32, 24), every=2, gap=2)
    assert ordinals == [0, 2, 4, 6] and geom == (72, 56, 2, 2)                 # 2 x 32 + 2 and 2 x 24 + 2, rounded up to multiples of 8
    pics = bridge.oracle_decode(data, 7)
    small = [scale.of_picture(pics[k], (64, 48, 2, 2), (32, 24, 2, 2)) for k in ordinals]
    target = contactsheet.sheet_target(4, 2, (32, 24), (2, 2), 2)
    want = cp.of_pictures(small + [cp.flat_picture((72, 56), (2, 2), contactsheet.BACKGROUND)], [(32, 24, 2, 2)] * 4 + [geom], target)
    assert file == jpeg.encode(want, 72, 56, 80, 2, 2)
    kinds = [s[0] for s in jpeg.segments(file)]
    assert kinds[0] == 0xD8 and kinds[-1] == 0xD9, "a whole JPEG file"
    assert contactsheet.layout(7) == (3, 3) and contactsheet.layout(16) == (4, 4) and contactsheet.layout(5, 5) == (5, 1)


CASES = ["identity", "known", "seams", "order", "extremes", "many", "sources", "golden", "ordering", "refusals", "composition", "tools"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "compose", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_compose(case, child_results):
    gpu_child.report(case, child_results)
