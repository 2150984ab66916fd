"""GPU: warped pictures in slot layout (hvq_warp_pictures / Context.warp_pictures) against hvqm4_amd.warp.of_picture, compared with ==
(tests/test_warp_cpu.py compares that module with tests/warp_ref.py, the plain-Python restatement of include/hvqm4_amd.h).  Every
output is allocated with 256 sentinel bytes before and behind it, which must stay untouched.  The cases run in ONE child process that
imports torch first (see tests/gpu_child.py); each test reports its case.  The child stops at the first HVQ_E_HIP or HIP error:
nothing more is started on a GPU that has reported a fault."""
import json
import os
import sys
import zlib
from fractions import Fraction

import numpy as np
import pytest

from tests import gpu_child
from tests.gpu_kit import ROOT, SENTINEL, check_bytes as _check, clip as _clip, decode as _decode, geom as _geom, geometry_rooms as _rooms

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300                                 # the cases take seconds each; a hung child is ended, not waited for
SAMPLINGS = ((2, 2), (2, 1), (1, 1))
T_MAX = (1 << 31) - 1
M_MAX = 1 << 21


# ------------------------------------------------------------------------------------------------------------- child side
def _nbytes(g):
    from hvqm4_amd import scale
    return scale.nbytes(*g)


def _warp(torch, ctx, sids, ords, targets, warps, src=None):
    """one call -> (list of n uint8 tensors, guards); targets: the target geometry of every picture"""
    out, guards = _rooms(torch, targets)
    got = ctx.warp_pictures(sids, ords, warps, [t[:2] for t in targets], [t[2:] for t in targets], src, out)
    assert got is out
    return [out[i] for i in range(len(targets))], guards


def _contents(g, seed):
    """pictures of geometry g: random, 0 / 255 at random, and a 0 / 255 checkerboard in every plane"""
    rng = np.random.default_rng(seed)
    n = _nbytes(g)
    w, h, hs, vs = g
    board = []
    for pw, ph in ((w, h), (w // hs, h // vs), (w // hs, h // vs)):
        y, x = np.mgrid[0:ph, 0:pw]
        board.append((((x + y + seed) & 1) * 255).astype(np.uint8).reshape(-1))
    return [rng.integers(0, 256, n, dtype=np.uint8), (rng.integers(0, 2, n) * 255).astype(np.uint8), np.concatenate(board)]


_expected = {}


def _want(g, pic, w, tg):
    from hvqm4_amd import warp as W
    key = (g, zlib.crc32(pic.tobytes()), w, tg)
    if key not in _expected:                          # computed once, shared by the cases that repeat a job (bodies), left unchanged
        _expected[key] = W.of_picture(pic, g, w, tg)
    return _expected[key]


def _upload_check(torch, ctx, jobs, what):
    """jobs: [(source geometry, picture as a uint8 array, Warp, target geometry)] through src= in ONE call, on streams nothing was
    decoded into"""
    sids = {}
    for g, _p, _w, _t in jobs:
        if g not in sids:
            sids[g] = ctx.open_stream(g[0], g[1], g[2], g[3], True, 3)
    bufs = [torch.from_numpy(np.array(p, dtype=np.uint8)).cuda() for _g, p, _w, _t in jobs]
    got, guards = _warp(torch, ctx, [sids[j[0]] for j in jobs], [-1] * len(jobs), [j[3] for j in jobs], [j[2] for j in jobs], src=bufs)
    torch.cuda.synchronize()
    _check(torch, got, guards, [_want(g, p, w, t) for g, p, w, t in jobs], what)
    for s in sids.values():
        ctx.close_stream(s)
    return got


def case_identity(torch, ctx):
    """the smallest geometry and 72 x 24 (one tile and a remainder in both axes) in the three samplings: the bytes themselves"""
    from hvqm4_amd import warp as W
    jobs = [((w, h) + s, _contents((w, h) + s, w)[0], W.identity(), (w, h) + s) for (w, h) in ((8, 8), (72, 24)) for s in SAMPLINGS]
    got = _upload_check(torch, ctx, jobs, "identity")
    for g, job in zip(got, jobs):
        assert np.array_equal(g.cpu().numpy(), job[1]), "identity is not the picture"


def _permutations(w, h, s):
    """(name, Warp, target geometry, what numpy does to a plane or None)"""
    from hvqm4_amd import warp as W
    out = [("flip_h", W.flip_h(w), (w, h) + s, lambda a: np.flip(a, 1)), ("flip_v", W.flip_v(h), (w, h) + s, lambda a: np.flip(a, 0)),
           ("transpose", W.transpose(), (h, w) + s, lambda a: a.T)]
    for k in (1, 2, 3):
        t, size = W.rotate90(k, w, h)
        out.append((f"turn{k}", t, size + s, lambda a, k=k: np.rot90(a, k)))
    return out


def _permutation_jobs():
    jobs, how = [], []
    for (w, h) in ((72, 24), (24, 72)):
        for s in SAMPLINGS:
            g = (w, h) + s
            pic = _contents(g, w + s[0] + s[1])[0]
            for name, t, tg, fn in _permutations(w, h, s):
                jobs.append((g, pic, t, tg))
                how.append((name, fn if s[0] == s[1] else None))     # 4:2:2: no permutation of the chroma samples under a turn, compared with the module
    return jobs, how


def case_permutations(torch, ctx):
    """the two mirrors, the transpose and the three quarter turns on 72 x 24 and 24 x 72: in 4:4:4 and 4:2:0 against np.flip / np.rot90
    per plane, in 4:2:2 against the module; yuv444_13_portrait48x64 decoded and turned to 64 x 48"""
    from hvqm4_amd import warp as W
    jobs, how = _permutation_jobs()
    got = _upload_check(torch, ctx, jobs, "permutations")
    for t, (g, pic, _w, tg), (name, fn) in zip(got, jobs, how):
        if fn is not None:
            want = np.concatenate([np.ascontiguousarray(fn(a)).reshape(-1) for a in W.planes(pic, *g)])
            assert np.array_equal(t.cpu().numpy(), want), (name, g)
    sid, hdr, n = _decode(ctx, _clip("yuv444_13_portrait48x64"))
    g = _geom(hdr)
    assert g == (48, 64, 1, 1)
    turn, size = W.rotate90(1, 48, 64)
    assert size == (64, 48)
    got, guards = _warp(torch, ctx, [sid] * n, list(range(n)), [(64, 48, 1, 1)] * n, turn)
    torch.cuda.synchronize()
    want = [np.concatenate([np.rot90(a, 1).reshape(-1) for a in W.planes(ctx.read_picture(sid, k), *g)]) for k in range(n)]
    _check(torch, got, guards, want, "the portrait clip turned upright")
    ctx.close_stream(sid)


def case_known(torch, ctx):
    """the half-sample shift, the 2:1 reduction, a flat picture, and integer translations against index arithmetic under both borders"""
    from hvqm4_amd import warp as W
    g = (72, 24, 1, 1)
    pic = _contents(g, 5)[0]
    y = pic[:72 * 24].reshape(24, 72).astype(int)
    flat = np.full(_nbytes(g), 201, dtype=np.uint8)
    sh = W.translate(3, -5)
    jobs = [(g, pic, W.Warp(t0=32768), g), (g, pic, W.Warp(m00=131072), (32, 24, 1, 1)), (g, flat, W.rotate(33, 72, 24), g), (g, flat, W.zoom(Fraction(1, 3)), g),
            (g, pic, sh, g), (g, pic, W.with_border(sh, W.CONSTANT, (77, 1, 2)), g)]
    got = [t.cpu().numpy() for t in _upload_check(torch, ctx, jobs, "known answers")]
    half = got[0][:72 * 24].reshape(24, 72)
    assert np.array_equal(half[:, :-1], (y[:, :-1] + y[:, 1:] + 1) >> 1) and np.array_equal(half[:, -1], y[:, -1]), "t0 = 32768"
    red = got[1][:32 * 24].reshape(24, 32)
    assert np.array_equal(red, (y[:, 0:64:2] + y[:, 1:64:2] + 1) >> 1), "m00 = 131072"
    assert bool((got[2] == 201).all()) and bool((got[3] == 201).all()), "a flat picture stays flat"
    xs, ys = np.clip(np.arange(72) - 3, 0, 71), np.clip(np.arange(24) + 5, 0, 23)
    assert np.array_equal(got[4][:72 * 24].reshape(24, 72), y[ys][:, xs]), "an integer translation, replicated border"
    want = np.full((24, 72), 77)
    want[:19, 3:] = y[5:, :69]
    assert np.array_equal(got[5][:72 * 24].reshape(24, 72), want), "an integer translation, constant border"


def _seam_maps(w, h):
    from hvqm4_amd import warp as W
    c = (Fraction(w, 2), Fraction(h, 2))
    maps = [W.rotate(d, w, h) for d in (Fraction(1, 2), 30, 45, Fraction(179, 2))] + [W.zoom(z, centre=c) for z in (Fraction(3, 4), Fraction(3, 2), 3, Fraction(1, 2))]
    maps += [W.shear(Fraction(1, 4), Fraction(-1, 8), c), W.compose(W.flip_h(w), W.rotate(20, w, h))]
    return [m if i & 1 else W.with_border(m, W.CONSTANT, (16, 240, 3)) for i, m in enumerate(maps)]


def _seam_jobs():
    jobs = []
    for s in ((2, 2), (1, 1)):
        g = (136, 40) + s
        for m in _seam_maps(136, 40):
            for c in _contents(g, 136):
                jobs += [(g, c, m, g), (g, c, m, (104, 56) + s)]
    return jobs


def case_seams(torch, ctx):
    """136 x 40 and 104 x 56 targets: three tile columns and rows, none full at the edge (a tile is 64 x 16); rotations by 0.5, 30, 45
    and 89.5 degrees, zooms 3/4, 3/2, 3 and 1/2, a shear and a negative determinant; random, 0 / 255 and checkerboard content"""
    from hvqm4_amd import warp as W
    assert (W.TILE_W, W.TILE_H) == (64, 16) and 136 > 2 * 64 and 136 % 64 and 40 > 2 * 16 and 40 % 16 and 104 % 64 and 56 > 3 * 16 and 56 % 16
    _upload_check(torch, ctx, _seam_jobs(), "tile seams")


def case_borders(torch, ctx):
    """footprints wholly outside on each of the four sides, and straddling each edge and corner; both borders, three distinct fill
    values, on 8 x 8 whose chroma is 4 wide"""
    from hvqm4_amd import warp as W
    moves = [(11, 0), (-11, 0), (0, 11), (0, -11), (Fraction(5, 2), 0), (Fraction(-5, 2), 0), (0, Fraction(7, 4)), (0, Fraction(-7, 4)),
             (Fraction(3, 2), Fraction(5, 4)), (Fraction(-3, 2), Fraction(-5, 4)), (Fraction(-9, 4), Fraction(1, 2)), (Fraction(1, 4), Fraction(-11, 4))]
    jobs = []
    for s in SAMPLINGS:
        g = (8, 8) + s
        pic = _contents(g, 8)[0]
        for dx, dy in moves:
            jobs += [(g, pic, W.translate(dx, dy), g), (g, pic, W.with_border(W.translate(dx, dy), W.CONSTANT, (1, 200, 77)), g)]
        jobs.append((g, pic, W.with_border(W.rotate(45, 8, 8), W.CONSTANT, (1, 200, 77)), g))
    got = _upload_check(torch, ctx, jobs, "borders")
    out = got[1].cpu().numpy()                        # wholly outside on the left, constant: the three fills
    assert set(out[:64].tolist()) == {1} and set(out[64:80].tolist()) == {200} and set(out[80:].tolist()) == {77}


def case_extremes(torch, ctx):
    """|m| = 2^21 on each coefficient alone, t = +-(2^31 - 1), an 8192 x 8 and an 8 x 8192 source, an all-zero linear part"""
    from hvqm4_amd import warp as W
    jobs = []
    for g in ((72, 24, 2, 2), (8192, 8, 2, 2), (8, 8192, 2, 1)):
        w, h = g[:2]
        pic = _contents(g, 3)[0]
        for i in range(4):
            for sgn in (1, -1):
                m = [0, 0, 0, 0]
                m[i] = sgn * M_MAX
                jobs.append((g, pic, W.Warp(m[0], m[1], m[2], m[3], 65536 * (w // 2) + 1234, 65536 * (h // 2) - 999, W.CONSTANT, (9, 8, 7)), (72, 24) + g[2:]))
        for sgn in (1, -1):
            for b in (W.REPLICATE, W.CONSTANT):
                jobs.append((g, pic, W.Warp(65536, 0, 0, 65536, sgn * T_MAX, -sgn * T_MAX, b, (50, 60, 70)), (72, 24) + g[2:]))
                jobs.append((g, pic, W.Warp(-M_MAX, M_MAX, M_MAX, -M_MAX, sgn * T_MAX, sgn * T_MAX, b, (50, 60, 70)), (72, 24) + g[2:]))
        jobs.append((g, pic, W.Warp(0, 0, 0, 0, 65536 * 5 + 100, 65536 * 2 + 40000), (72, 24) + g[2:]))
        jobs += [(g, pic, W.identity(), g), (g, pic, W.transpose(), (h, w) + g[2:]), (g, pic, W.rotate(1, w, h), g)]
    _upload_check(torch, ctx, jobs, "extremes")


def case_bodies(torch, ctx):
    """every seams and permutation job under the chosen body and under the forced direct body: the same bytes; at least one job chose
    each body"""
    from hvqm4_amd import warp as W
    jobs = _seam_jobs() + _permutation_jobs()[0]
    chosen = {W.body(w, g, tg, p) for g, _pic, w, tg in jobs for p in (0, 1)}
    assert chosen == {W.DIRECT, W.TILED}, chosen
    a = _upload_check(torch, ctx, jobs, "the chosen body")
    assert ctx.warp_force_direct(True) == 0
    try:
        b = _upload_check(torch, ctx, jobs, "the forced direct body")
        assert ctx.warp_force_direct(2) == 1
        c = _upload_check(torch, ctx, jobs, "the tiled body wherever LDS holds the box")
    finally:
        ctx.warp_force_direct(False)
    for x, y, z in zip(a, b, c):
        assert bool(x.eq(y).all()) and bool(x.eq(z).all())


def _ten_warps(w, h):
    from hvqm4_amd import warp as W
    c = (Fraction(w, 2), Fraction(h, 2))
    return [(W.identity(), None), (W.rotate90(1, w, h)[0], (h, w)), (W.rotate(7, w, h), None), (W.with_border(W.rotate(45, w, h), W.CONSTANT), None), (W.flip_h(w), None),
            (W.zoom(Fraction(1, 2)), (max(8, w // 16 * 8), max(8, h // 16 * 8))), (W.zoom(Fraction(3, 2), centre=c), None), (W.translate(Fraction(7, 2), -2), None),
            (W.transpose(), (h, w)), (W.shear(Fraction(1, 8), 0, c), (w, h))]


def case_many(torch, ctx):
    """one launch: 300 pictures of eight clips (more than four geometries), ten warps, mixed target sizes; both forms of out"""
    from hvqm4_amd import warp as W
    names = ["gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8", "i16", "natural128x96"]
    streams = {nm: _decode(ctx, _clip(nm)) for nm in names}
    sids, ords, geoms, warps, targets = [], [], [], [], []
    for i in range(300):
        sid, hdr, n = streams[names[i % len(names)]]
        g = _geom(hdr)
        w, size = _ten_warps(*g[:2])[(i // len(names) + i) % 10]
        sids.append(sid); ords.append(i % n); geoms.append(g); warps.append(w); targets.append((size or g[:2]) + g[2:])
    assert len(set(geoms)) >= 4 and len(set(warps)) >= 10 and len(set(targets)) > len(set(geoms))
    got, guards = _warp(torch, ctx, sids, ords, targets, warps)               # a list: the target geometries differ
    torch.cuda.synchronize()
    pics = {}
    wants = []
    for s, o, g, w, t in zip(sids, ords, geoms, warps, targets):
        if (s, o) not in pics:
            pics[s, o] = ctx.read_picture(s, o)
        wants.append(_want(g, pics[s, o], w, t))
    _check(torch, got, guards, wants, "many shapes")
    # one target geometry: one tensor [n, bytes], given and not given
    sid, hdr, n = streams["natural128x96"]
    g = _geom(hdr)
    k = [i % n for i in range(12)]
    w12 = [_ten_warps(128, 96)[i % 10][0] for i in range(12)]
    got, guards = _warp(torch, ctx, [sid] * 12, k, [g] * 12, w12)
    fresh = ctx.warp_pictures([sid] * 12, k, w12)
    torch.cuda.synchronize()
    want12 = [_want(g, pics.get((sid, o), None) if (sid, o) in pics else ctx.read_picture(sid, o), w, g) for o, w in zip(k, w12)]
    _check(torch, got, guards, want12, "one tensor, given")
    assert tuple(fresh.shape) == (12, _nbytes(g))
    _check(torch, list(fresh), [], want12, "one tensor, returned")
    for sid, _h, _n in streams.values():
        ctx.close_stream(sid)


def case_sources(torch, ctx):
    """src= from the caller's memory, 16 bytes into an allocation too, mixed with resident pictures in one call"""
    from hvqm4_amd import warp as W
    sid, hdr, n = _decode(ctx, _clip("yuv422_64x48"))
    g = _geom(hdr)
    pics = [ctx.read_picture(sid, k) for k in range(n)]
    w = W.with_border(W.rotate(30, 64, 48), W.CONSTANT)
    src, sids, ords, wants = [], [], [], []
    for k in range(n):
        inv = 255 - np.asarray(pics[k]).reshape(-1)
        room = torch.zeros(inv.size + 32, dtype=torch.uint8, device="cuda")
        off = (-room.data_ptr()) % 16 + (16 if k & 1 else 0)
        room[off:off + inv.size] = torch.from_numpy(inv).cuda()
        src += [room[off:off + inv.size], None]; sids += [sid, sid]; ords += [-1, k]
        wants += [W.of_picture(inv, g, w), W.of_picture(pics[k], g, w)]
    got, guards = _warp(torch, ctx, sids, ords, [g] * len(sids), w, src=src)
    torch.cuda.synchronize()
    _check(torch, got, guards, wants, "the caller's memory and resident pictures")
    ctx.close_stream(sid)


def _fixture_warps(geom):
    from hvqm4_amd import warp as W
    w, h, hs, vs = geom
    turn, (tw, th) = W.rotate90(1, w, h)
    return [("rotate7_constant", W.with_border(W.rotate(7, w, h), W.CONSTANT), geom), ("rotate90", turn, (tw, th, hs, vs)),
            ("zoom3/4_replicate", W.zoom(Fraction(3, 4), centre=(Fraction(w, 2), Fraction(h, 2))), geom)]


def case_golden(torch, ctx):
    """every clip of tests/golden/warp.json decoded on the GPU, its last picture through the fixture's three warps in one call"""
    fixture = json.load(open(os.path.join(ROOT, "tests", "golden", "warp.json")))["clips"]
    manifest = json.load(open(os.path.join(ROOT, "tests", "golden", "manifest.json")))["clips"]
    assert set(fixture) == {nm for nm, c in manifest.items() if "file" in c}
    sids, ords, targets, warps, crcs, streams = [], [], [], [], [], []
    for name, entry in sorted(fixture.items()):
        sid, hdr, n = _decode(ctx, open(os.path.join(ROOT, "tests", "golden", manifest[name]["file"]), "rb").read())
        streams.append(sid)
        assert _geom(hdr) == tuple(entry["geometry"])
        for (label, tg, crc), (label2, w, tg2) in zip(entry["warps"], _fixture_warps(_geom(hdr))):
            assert label == label2 and tuple(tg) == tg2
            sids.append(sid); ords.append(n - 1); targets.append(tg2); warps.append(w); crcs.append((name, label, crc))
    got, guards = _warp(torch, ctx, sids, ords, targets, warps)
    torch.cuda.synchronize()
    for g in guards:
        assert bool(g.eq(SENTINEL).all())
    for t, (name, label, crc) in zip(got, crcs):
        assert zlib.crc32(t.cpu().numpy().tobytes()) == crc, (name, label)
    for s in streams:
        ctx.close_stream(s)


def case_ordering(torch, ctx):
    """tests/test_gpu_scale.py's ordering: the warped pictures of batch k on a side stream beside batch k + 1 in flight, batch k + 2
    into batch k's slots behind the call; work queued behind the call on the same stream sees the result; a picture of the batch in
    flight"""
    from hvqm4_amd import warp as W
    from hvqm4_amd.container import parse_header, video_pictures
    from oracle import bridge
    data = _clip("gop64x48_15")
    hdr = parse_header(data)
    g, w = _geom(hdr), W.rotate(30, hdr.width, hdr.height)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    assert len(pics) == 7                            # I P B B P B B
    want = [W.of_picture(p, g, w) for p in bridge.oracle_decode(data, 7)]
    sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, 6)
    b = [pics[0:3], pics[3:5], pics[5:7]]
    sub = lambda part: ctx.submit_many_device([sid] * len(part), [ft for ft, _p in part], [p for _f, p in part])
    side = torch.cuda.Stream()
    sub(b[0]); ctx.flush_begin()
    sub(b[1]); ctx.flush_next()                      # batch 0 ended, batch 1 in flight
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got, guards = _warp(torch, ctx, [sid] * 3, [2, 0, 1], [g] * 3, w)
        copy = torch.stack(got).clone()              # queued behind the call on the same stream: it sees the result
    sub(b[2]); ctx.flush_next()                      # batch 1 ended, batch 2 in flight
    ctx.flush_end()                                  # batch 2 reconstructed: picture 6 lies in picture 0's slot of the ring of 6
    late, lguards = _warp(torch, ctx, [sid] * 4, [3, 4, 5, 6], [g] * 4, w)
    torch.cuda.synchronize()
    _check(torch, got, guards, [want[k] for k in (2, 0, 1)], "batch 0 beside batch 1")
    _check(torch, list(copy), [], [want[k] for k in (2, 0, 1)], "a copy queued behind the call")
    _check(torch, late, lguards, want[3:7], "batches 1 and 2")
    sub(b[0]); ctx.flush_begin()                     # a picture of the batch in flight: the call ends that batch itself
    got, guards = _warp(torch, ctx, [sid], [7 + 2], [g], w)
    torch.cuda.synchronize()
    _check(torch, got, guards, [want[2]], "a picture of the batch in flight")
    ctx.close_stream(sid)


def _raw(torch, ctx, sids, ords, src, structs, geoms, count=None, ctx_h=None, ptr=None, null_warps=False, null_dst=False):
    """hvq_warp_pictures through the C ABI into sentinel-filled memory -> (return code, every byte still holds the sentinel).
    structs: the HvqWarp of every picture; geoms: the target geometries; ptr: the destination pointer of picture 0 instead of the room's"""
    import ctypes as C
    from hvqm4_amd._lib import HvqWarp, HvqWarpDst, lib
    n = len(sids)
    room = torch.full((n, 8192), SENTINEL, dtype=torch.uint8, device="cuda")
    a_d = (HvqWarpDst * n)(*[HvqWarpDst(ptr if ptr is not None and i == 0 else room[i].data_ptr(), *geoms[i]) for i in range(n)])
    a_p = C.cast((C.c_void_p * n)(*src), C.c_void_p) if src is not None else None
    a_w = (HvqWarp * n)(*structs)
    rc = lib().hvq_warp_pictures(ctx._h if ctx_h is None else ctx_h, n if count is None else count, (C.c_int * n)(*sids), (C.c_int * n)(*ords), a_p,
                                 None if null_warps else C.cast(a_w, C.c_void_p), None if null_dst else C.cast(a_d, C.c_void_p),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, bool(room.eq(SENTINEL).all())


def case_refusals(torch, ctx):
    """every refusal of the header through the C entry leaves the destinations untouched, also those of the well-formed pictures of
    the same call; the well-formed call right after works"""
    import ctypes as C
    from hvqm4_amd import warp as W
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_GEOMETRY, HVQ_E_STATE
    from hvqm4_amd.container import video_pictures
    data = _clip("gop64x48_15")
    sa, hdr, n = _decode(ctx, data)
    g = _geom(hdr)
    assert ctx.pic_bytes(sa) <= 8192
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    sd = ctx.open_stream(hdr.width, hdr.height, 2, 2, hdr.is15, 3)
    for ft, p in pics:
        ctx.submit(sd, ft, p)
    ctx.flush()                                                  # picture 0 of sd: its slot of the ring of 3 was reused
    sq = ctx.open_stream(hdr.width, hdr.height, 2, 2, hdr.is15, 3)
    mem = torch.zeros(ctx.pic_bytes(sa) + 32, dtype=torch.uint8, device="cuda")
    p16 = mem.data_ptr() + (-mem.data_ptr()) % 16
    good = W.rotate(30, 64, 48).to_struct()
    two, gg = [sa, sa], [g, g]
    for field, v in (("m00", 32 * 65536 + 1), ("m01", -32 * 65536 - 1), ("m10", T_MAX), ("m11", -T_MAX - 1), ("border", 2), ("border", -1), ("pad", 1)):
        s = W.rotate(30, 64, 48).to_struct()
        setattr(s, field, v)
        assert _raw(torch, ctx, two, [0, 1], None, [good, s], gg) == (HVQ_E_ARG, True), (field, v)
    arg = [("bad stream", [sa, 99], [0, 0], None, {}), ("an ordinal that is not resident", two, [0, 1000], None, {}), ("negative ordinal", two, [0, -1], None, {}),
           ("misaligned src", two, [0, -1], [None, p16 + 8], {}), ("an ordinal with src", two, [0, 1], [None, p16], {}),
           ("src with a bad stream", [sa, 99], [0, -1], [None, p16], {}), ("null warps", two, [0, 1], None, {"null_warps": True}), ("null dst", two, [0, 1], None, {"null_dst": True}),
           ("null context", two, [0, 1], None, {"ctx_h": C.c_void_p(0)}), ("null ptr", two, [0, 1], None, {"ptr": 0}), ("misaligned ptr", two, [0, 1], None, {"ptr": p16 + 8})]
    for what, sids, ords, src, kw in arg:
        assert _raw(torch, ctx, sids, ords, src, [good, good], gg, **kw) == (HVQ_E_ARG, True), what
    for bad in ((60, 48, 2, 2), (64, 48, 1, 2), (64, 48, 3, 1), (0, 0, 2, 2), (8200, 48, 2, 2)):
        assert _raw(torch, ctx, two, [0, 1], None, [good, good], [g, bad]) == (HVQ_E_GEOMETRY, True), bad
    assert _raw(torch, ctx, [sa], [0], None, [good], [g], count=65536) == (HVQ_E_ARG, True), "n beyond 65535"
    assert _raw(torch, ctx, [sa], [0], None, [good], [g], count=0) == (0, True), "n == 0 does nothing"
    # the HVQ_E_STATE cases: a slot that was reused, a picture queued but not flushed
    assert _raw(torch, ctx, [sa, sd], [0, 0], None, [good, good], gg) == (HVQ_E_STATE, True), "an evicted picture"
    ctx.submit(sq, pics[0][0], pics[0][1])
    assert _raw(torch, ctx, [sa, sq], [0, 0], None, [good, good], gg) == (HVQ_E_STATE, True), "queued but not flushed"
    ctx.flush()
    # the well-formed calls right after them work: the coefficients at their limits, and the method
    lim = W.Warp(32 * 65536, -32 * 65536, 32 * 65536, -32 * 65536, T_MAX, -T_MAX - 1, W.CONSTANT, (255, 255, 255)).to_struct()
    rc, untouched = _raw(torch, ctx, two, [0, 1], None, [good, lim], gg)
    assert rc == 0 and not untouched
    w = W.rotate(30, 64, 48)
    got, guards = _warp(torch, ctx, [sa, sd, sq], [1, len(pics) - 1, 0], [g] * 3, w)
    torch.cuda.synchronize()
    _check(torch, got, guards, [W.of_picture(ctx.read_picture(s, o), g, w) for s, o in ((sa, 1), (sd, len(pics) - 1), (sq, 0))], "after the refusals")
    for s in (sa, sd, sq):
        ctx.close_stream(s)


def case_composition(torch, ctx):
    """picture_motion of a picture against a copy shifted by (3, -5) -> global_motion -> warp.from_motion -> warp_pictures(src=) ->
    picture_metrics against the original: the SAD numpy computes from warp.of_picture, 0 on the interior; the warped picture where it
    lies feeds encode_jpeg(src=) and scale_pictures(src=), nothing read back in between"""
    from hvqm4_amd import jpeg, motion, scale
    from hvqm4_amd import warp as W
    sn, hn, nn = _decode(ctx, _clip("natural128x96"))
    g = _geom(hn)
    w, h = g[:2]
    k = min(nn, 4) - 1
    pic = ctx.read_picture(sn, k)
    shifted = W.of_picture(pic, g, W.translate(-5, 3))            # the picture at (y, x) looks like this copy at (y + 3, x - 5)
    ref = torch.from_numpy(shifted).cuda()
    field = ctx.picture_motion([sn], [k], [ref], block=16, radius=8)[0]
    vector, share = motion.global_motion(field.cpu().numpy())
    assert vector == (3, -5) and share > 0.5, (vector, share)
    back = W.from_motion(vector)
    predicted = ctx.warp_pictures([sn], [-1], back, src=[ref])
    sad = ctx.picture_metrics([sn], [k], ref=[predicted[0]])
    turn, size = W.rotate90(1, w, h)
    st = ctx.open_stream(size[0], size[1], g[2], g[3], True, 3)   # carries the turned geometry; nothing is submitted to it
    turned = ctx.warp_pictures([sn], [k], turn, size=size)
    files, lengths = ctx.encode_jpeg([st], [-1], quality=85, src=[turned[0]])
    small = ctx.scale_pictures([st], [-1], (size[0] // 2 // 8 * 8, size[1] // 2), src=[turned[0]])
    torch.cuda.synchronize()
    want = W.of_picture(shifted, g, back)
    _check(torch, [predicted[0]], [], [want], "from_motion -> warp_pictures(src=)")
    a, b = W.planes(pic, *g), W.planes(want, *g)
    want_sad = [int(np.abs(x.astype(int) - y.astype(int)).sum()) for x, y in zip(a, b)]
    assert sad.cpu().numpy()[0, :, 2].tolist() == want_sad, "warp -> picture_metrics(ref=)"
    assert int(np.abs(a[0][8:-8, 8:-8].astype(int) - b[0][8:-8, 8:-8].astype(int)).sum()) == 0 and want_sad[0] > 0, "the prediction is exact on the interior"
    tg = size + g[2:]
    want_turned = W.of_picture(pic, g, turn, tg)
    assert jpeg.files(files, lengths) == [jpeg.encode(want_turned, size[0], size[1], 85, g[2], g[3])], "warp -> encode_jpeg(src=)"
    half = (size[0] // 2 // 8 * 8, size[1] // 2)
    _check(torch, [small[0]], [], [scale.of_picture(want_turned, tg, half + g[2:])], "warp -> scale_pictures(src=)")
    ctx.close_stream(st)
    ctx.close_stream(sn)


def case_tools(torch, ctx):
    """tools/h4m2jpeg.py --rotate: the files are those of the turned pictures; tools/stabilise.py: the first picture stays where it
    is, every picture is the clip's moved by the accumulated global vector"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import h4m2jpeg
    import stabilise
    from hvqm4_amd import jpeg, motion
    from hvqm4_amd import warp as W
    from oracle import bridge
    data = _clip("yuv444_13_portrait48x64")
    pics = bridge.oracle_decode(data, 4)
    _t, files = h4m2jpeg.clip_files(ctx, data, 80, None, None, 90)
    for f, p in zip(files, pics):
        turned = np.concatenate([np.rot90(a, 1).reshape(-1) for a in W.planes(p, 48, 64, 1, 1)])
        assert f == jpeg.encode(turned, 64, 48, 80, 1, 1), "--rotate 90"
    assert h4m2jpeg.target_size(data, None, 32, None, 90) == (32, 24) and h4m2jpeg.target_size(data, None, 32, None) == (24, 32)
    _t, small = h4m2jpeg.clip_files(ctx, data, 80, (32, 24), None, 270)
    assert len(small) == len(files) == len(pics) and all(len(a) < len(b) for a, b in zip(small, files))
    data = _clip("gop64x48_15")
    g = (64, 48, 2, 2)
    pics = bridge.oracle_decode(data, 7)
    types, path, files = stabilise.stabilised_files(ctx, data, 85, 16, 8)
    assert len(files) == len(path) == 7 and path[0] == (0, 0)
    want = [(0, 0)]
    for k in range(1, 7):
        (dy, dx), _s = motion.global_motion(motion.of_pictures(pics[k], pics[k - 1], 64, 48, 16, 8))
        want.append((want[-1][0] + dy, want[-1][1] + dx))
    assert path == want
    assert files == [jpeg.encode(W.of_picture(p, g, W.translate(dx, dy)), 64, 48, 85, 2, 2) for p, (dy, dx) in zip(pics, path)], "stabilise"


CASES = ["identity", "permutations", "known", "seams", "borders", "extremes", "bodies", "many", "sources", "golden", "ordering", "refusals", "composition", "tools"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "warp", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_warp(case, child_results):
    gpu_child.report(case, child_results)
