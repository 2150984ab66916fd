"""GPU: scaled pictures in slot layout (hvq_scale_pictures / Context.scale_pictures) against hvqm4_amd.scale.of_picture, compared with ==
(tests/test_scale_cpu.py compares that module with tests/scale_ref.py, the plain-Python restatement of include/hvqm4_amd.h).  Every
output is allocated with 256 sentinel bytes before and behind it, which must stay untouched.  The cases run in ONE child process that
imports torch first (see tests/gpu_child.py); each test reports its case.  The child stops at the first HVQ_E_HIP or HIP error: nothing
more is started on a GPU that has reported a fault."""
import json
import os
import sys

import numpy as np
import pytest

from tests import gpu_child, gpu_kit
from tests.gpu_kit import ROOT, SENTINEL, check_bytes as _check, clip as _clip, decode as _decode, geom as _geom

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300                                 # the cases take seconds each; a hung child is ended, not waited for


# ------------------------------------------------------------------------------------------------------------- child side
def _scale(torch, ctx, sids, ords, dsts, crops=None, src=None):
    """one call -> (list of n uint8 tensors, guards)"""
    dsts = [tuple(d) for d in dsts]
    out, guards = gpu_kit.geometry_rooms(torch, dsts)
    got = ctx.scale_pictures(sids, ords, [d[:2] for d in dsts], [d[2:] for d in dsts], crops, src, out)
    assert got is out
    return [out[i] for i in range(len(dsts))], guards


def _resident(torch, ctx, jobs, what):
    """jobs: [(clip name, picture ordinal or None for the last, target geometry or None for the source's, crop)] in ONE call; pictures
    read back for the expected bytes only after the call is queued"""
    from hvqm4_amd import scale
    streams = {}
    for name, _k, _d, _c in jobs:
        if name not in streams:
            streams[name] = _decode(ctx, _clip(name))
    sids, ords, dsts, crops, geoms = [], [], [], [], []
    for name, k, dst, crop in jobs:
        sid, hdr, n = streams[name]
        sids.append(sid); ords.append(n - 1 if k is None else k); geoms.append(_geom(hdr))
        dsts.append(tuple(dst) if dst is not None else _geom(hdr)); crops.append(crop)
    got, guards = _scale(torch, ctx, sids, ords, dsts, crops)
    torch.cuda.synchronize()
    pics = [ctx.read_picture(s, o) for s, o in zip(sids, ords)]
    wants = [scale.of_picture(p, g, d, c) for p, g, d, c in zip(pics, geoms, dsts, crops)]
    _check(torch, got, guards, wants, what)
    return streams, got, pics, (sids, ords, dsts, crops)


def _close(ctx, streams):
    for sid, _hdr, _n in streams.values():
        ctx.close_stream(sid)


def _upload(torch, ctx, pics, geom, dsts, crops=None):
    """pictures (uint8 arrays in slot layout of `geom`) through src= on a stream nothing was decoded into"""
    from hvqm4_amd import scale
    sid = ctx.open_stream(geom[0], geom[1], geom[2], geom[3], True, 3)
    bufs = [torch.from_numpy(np.array(p, dtype=np.uint8)).cuda() for p in pics]
    got, guards = _scale(torch, ctx, [sid] * len(pics), [-1] * len(pics), dsts, crops, src=bufs)
    torch.cuda.synchronize()
    ctx.close_stream(sid)
    return got, guards


def case_identity(torch, ctx):
    """each sampling: M == N gives the bytes read_picture returns"""
    from hvqm4_amd import scale
    names = ["crossplane420_64x48", "crossplane422_13_64x48", "crossplane444_48x64"]
    streams, got, pics, _call = _resident(torch, ctx, [(nm, None, None, None) for nm in names], "identity")
    assert {(_geom(h)[2:]) for _s, h, _n in streams.values()} == {(2, 2), (2, 1), (1, 1)}
    for g, p in zip(got, pics):
        assert np.array_equal(g.cpu().numpy(), np.asarray(p).reshape(-1)), "identity is not the picture"
    for _s, hdr, _n in streams.values():
        assert scale.body(hdr.width, hdr.height, hdr.width, hdr.height) == scale.DIRECT
    _close(ctx, streams)


def case_integer(torch, ctx):
    """ratios 2 and 4 on natural128x96, its first three pictures and its last"""
    n = 3
    jobs = [("natural128x96", k, dst, None) for k in (0, 1, 2, None) for dst in ((64, 48, 2, 2), (32, 24, 2, 2))]
    streams, _g, _p, _c = _resident(torch, ctx, jobs, "integer ratios")
    assert streams["natural128x96"][2] >= n
    _close(ctx, streams)


NONINTEGER = [("ragged24x40", None, (16, 16, 2, 2), None), ("ragged24x40", None, (8, 8, 2, 2), None), ("wide296x160", None, (104, 56, 2, 2), None),
              ("nest_exact280x152", None, (96, 56, 2, 2), None), ("portrait152x280", None, (56, 104, 2, 2), None)]
SAMPLING = [(nm, None, (w // d, h // d) + to, None)
            for nm, w, h, to in (("yuv444_64x48", 64, 48, (2, 2)), ("gop64x48_15", 64, 48, (1, 1)), ("yuv422_64x48", 64, 48, (2, 2))) for d in (1, 2)]


def case_noninteger(torch, ctx):
    """ratios that are no integers, tile seams (64 columns, 16 rows of targets) inside the picture"""
    from hvqm4_amd import scale
    streams, _g, _p, _c = _resident(torch, ctx, NONINTEGER, "non-integer ratios")
    assert scale.body(296, 160, 104, 56) == scale.TILED and 104 > 64 and 56 > 16 and 296 % 104 and 160 % 56
    _close(ctx, streams)


def case_enlarge(torch, ctx):
    """i16 -> 40 x 24 and 64 x 48 -> 64 x 104 (identity in x, up in y): the direct body"""
    from hvqm4_amd import scale
    streams, _g, _p, _c = _resident(torch, ctx, [("i16", None, (40, 24, 2, 2), None), ("gop64x48_15", 3, (64, 104, 2, 2), None)], "enlargement")
    assert scale.body(16, 16, 40, 24) == scale.DIRECT and scale.body(64, 48, 64, 104) == scale.DIRECT
    _close(ctx, streams)


def case_sampling(torch, ctx):
    """4:4:4 -> 4:2:0, 4:2:0 -> 4:4:4 and 4:2:2 -> 4:2:0, at the same size and at half size"""
    streams, _g, _p, _c = _resident(torch, ctx, SAMPLING, "sampling conversion")
    assert [(_geom(streams[nm][1])[2:], d[2:]) for nm, _k, d, _c2 in SAMPLING[::2]] == [((1, 1), (2, 2)), ((2, 2), (1, 1)), ((2, 1), (2, 2))]
    _close(ctx, streams)


def case_crops(torch, ctx):
    """a crop touching the right and bottom edges; odd offsets and sizes (legal for 4:4:4 only); a crop of exactly 8 x 8"""
    jobs = [("natural128x96", 2, (48, 40, 2, 2), (40, 24, 88, 72)), ("yuv444_64x48", None, (24, 16, 1, 1), (3, 5, 41, 33)),
            ("yuv444_64x48", 1, (64, 48, 2, 2), (23, 15, 41, 33)), ("natural128x96", 1, (8, 8, 2, 2), (120, 88, 8, 8)),
            ("natural128x96", 1, (16, 24, 2, 2), (62, 2, 8, 8))]
    streams, _g, _p, (sids, ords, dsts, crops) = _resident(torch, ctx, jobs, "crops")
    # the odd crop on a 4:2:0 stream is refused by the method and by the library
    from hvqm4_amd._lib import HVQ_E_ARG
    sid = streams["natural128x96"][0]
    with pytest.raises(ValueError):
        ctx.scale_pictures([sid], [0], (24, 16), crop=(3, 5, 41, 33))
    assert _raw(torch, ctx, [sid], [0], None, [((24, 16, 2, 2), (3, 5, 41, 33))])[0] == HVQ_E_ARG
    _close(ctx, streams)


def case_limit32(torch, ctx):
    """at the limit: 256 x 256 through src= -> 8 x 8 (33 x 33 taps where a cell straddles); just beyond it: refused"""
    from hvqm4_amd import scale
    from hvqm4_amd._lib import HVQ_E_ARG
    rng = np.random.default_rng(32)
    geom = (256, 256, 2, 2)
    pic = rng.integers(0, 256, scale.nbytes(*geom), dtype=np.uint8)
    got, guards = _upload(torch, ctx, [pic, pic], geom, [(8, 8, 2, 2), (8, 8, 1, 1)])
    _check(torch, got, guards, [scale.of_picture(pic, geom, d) for d in ((8, 8, 2, 2), (8, 8, 1, 1))], "256 x 256 -> 8 x 8")
    sid = ctx.open_stream(264, 256, 2, 2, True, 3)
    buf = torch.zeros(scale.nbytes(264, 256, 2, 2), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="beyond 32"):
        ctx.scale_pictures([sid], [-1], (8, 8), src=[buf])
    rc, untouched = _raw(torch, ctx, [sid], [-1], [buf.data_ptr()], [((8, 8, 2, 2), None)])
    assert rc == HVQ_E_ARG and untouched
    rc, untouched = _raw(torch, ctx, [sid], [-1], [buf.data_ptr()], [((8, 8, 2, 2), (0, 0, 256, 256))])      # the crop is within it
    assert rc == 0 and not untouched
    torch.cuda.synchronize()
    ctx.close_stream(sid)


def case_cells64(torch, ctx):
    """8192 x 2064 through src=, random and all 255, -> 256 x 72: a luma cell reaches 255 * 8192 * 2064 > 2^32, a 32-bit cell wraps"""
    from hvqm4_amd import scale
    geom, dst = (8192, 2064, 2, 2), (256, 72, 2, 2)
    assert 255 * geom[0] * geom[1] > 1 << 32
    rng = np.random.default_rng(64)
    rnd = rng.integers(0, 256, scale.nbytes(*geom), dtype=np.uint8)
    full = np.full(scale.nbytes(*geom), 255, dtype=np.uint8)
    got, guards = _upload(torch, ctx, [rnd, full], geom, [dst, dst])
    _check(torch, got, guards, [scale.of_picture(rnd, geom, dst), scale.of_picture(full, geom, dst)], "8192 x 2064 -> 256 x 72")
    assert bool(got[1].eq(255).all()), "all 255 stays all 255"


def case_ties(torch, ctx):
    """the two tie pictures: 2 x 2 blocks {0, 0, 0, 2} -> 1 (half rounds up) and {0, 0, 0, 1} -> 0"""
    from tests import scale_ref as ref
    pics = [np.frombuffer(p, dtype=np.uint8) for p in ref.tie_pictures()]
    got, guards = _upload(torch, ctx, pics, ref.TIE_GEOMETRY, [ref.TIE_TARGET] * 2)
    _check(torch, got, guards, [np.full(192, 1, dtype=np.uint8), np.zeros(192, dtype=np.uint8)], "ties")


def _many(ctx):
    """>= 300 pictures from every golden clip with mixed targets, samplings and crops"""
    from hvqm4_amd import scale
    manifest = json.load(open(os.path.join(ROOT, "tests", "golden", "manifest.json")))["clips"]
    names = [nm for nm, c in manifest.items() if "file" in c]
    streams = {nm: _decode(ctx, _clip(nm)) for nm in names}
    sids, ords, dsts, crops, geoms = [], [], [], [], []
    i = 0
    while len(sids) < 300 or i < len(names):
        nm = names[i % len(names)]
        sid, hdr, n = streams[nm]
        w, h, hs, vs = g = _geom(hdr)
        v = (i // len(names) + i) % 5
        crop = None
        if v == 0:
            dst = scale.pyramid(w, h, 2)[1] + (hs, vs)
        elif v == 1:
            dst = scale.fit(w, h, 56, 56) + (hs, vs)
        elif v == 2:
            dst = (w, h) + ((1, 1) if (hs, vs) == (2, 2) else (2, 2))
        elif v == 3:
            dst = (w + 8, max(8, h - 8), hs, vs)
        else:
            cw, ch = max(8, w // 2 // 2 * 2), max(8, h // 2 // 2 * 2)
            crop = (w - cw, h - ch, cw, ch)
            dst = (24, 16, 2, 1)
        sids.append(sid); ords.append(i % n); dsts.append(dst); crops.append(crop); geoms.append(g)
        i += 1
    return streams, sids, ords, dsts, crops, geoms


def case_many(torch, ctx):
    """one launch, many shapes: at least 300 pictures from every golden clip; the same call twice gives the same bits"""
    from hvqm4_amd import scale
    streams, sids, ords, dsts, crops, geoms = _many(ctx)
    assert len(sids) >= 300 and len(set(sids)) == len(streams) >= 30 and len(set(dsts)) > 20
    got, guards = _scale(torch, ctx, sids, ords, dsts, crops)
    again, guards2 = _scale(torch, ctx, sids, ords, dsts, crops)
    torch.cuda.synchronize()
    cache = {}
    wants = []
    for s, o, g, d, c in zip(sids, ords, geoms, dsts, crops):
        if (s, o) not in cache:
            cache[s, o] = ctx.read_picture(s, o)
        wants.append(scale.of_picture(cache[s, o], g, d, c))
    _check(torch, got, guards, wants, "many shapes")
    _check(torch, again, guards2, wants, "many shapes, again")
    _close(ctx, streams)


def case_body(torch, ctx):
    """the forced direct body equals the chosen one: the non-integer and the sampling cases, and the 32x limit"""
    from hvqm4_amd import scale
    jobs = NONINTEGER + SAMPLING
    streams, chosen, _p, (sids, ords, dsts, crops) = _resident(torch, ctx, jobs, "the chosen body")
    assert ctx.scale_force_direct(True) is False
    try:
        forced, guards = _scale(torch, ctx, sids, ords, dsts, crops)
        rng = np.random.default_rng(5)
        pic = rng.integers(0, 256, scale.nbytes(256, 256, 2, 2), dtype=np.uint8)
        lim, lguards = _upload(torch, ctx, [pic], (256, 256, 2, 2), [(8, 8, 2, 2)])
    finally:
        assert ctx.scale_force_direct(False) is True
    torch.cuda.synchronize()
    _check(torch, forced, guards, [c.cpu().numpy() for c in chosen], "the forced direct body")
    _check(torch, lim, lguards, [scale.of_picture(pic, (256, 256, 2, 2), (8, 8, 2, 2))], "the forced direct body at the limit")
    assert any(scale.body(*s) == scale.TILED for j in jobs for s in scale.plane_sizes(_geom(streams[j[0]][1]), j[2]))
    _close(ctx, streams)


def _raw(torch, ctx, sids, ords, src, dsts, count=None, ctx_h=None, ptr=None):
    """hvq_scale_pictures through the C ABI into sentinel-filled memory -> (return code, every byte still holds the sentinel).
    dsts: [(geometry, crop)]; ptr: the destination pointer of picture 0 instead of the room's"""
    import ctypes as C
    from hvqm4_amd._lib import HvqScaleDst, lib
    n = len(sids)
    room = torch.full((n, 65536), SENTINEL, dtype=torch.uint8, device="cuda")
    a_d = (HvqScaleDst * n)(*[HvqScaleDst((ptr if ptr is not None and i == 0 else room[i].data_ptr()), *g, *(c or (0, 0, 0, 0))) for i, (g, c) in enumerate(dsts)])
    a_p = C.cast((C.c_void_p * n)(*src), C.c_void_p) if src is not None else None
    rc = lib().hvq_scale_pictures(ctx._h if ctx_h is None else ctx_h, n if count is None else count, (C.c_int * n)(*sids), (C.c_int * n)(*ords), a_p,
                                  C.cast(a_d, C.c_void_p), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, bool(room.eq(SENTINEL).all())


def case_refusals(torch, ctx):
    """every refusal of the header leaves the destinations untouched, also those of the well-formed pictures of the same call"""
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_GEOMETRY, HVQ_E_STATE, lib
    from hvqm4_amd.container import video_pictures
    data = _clip("gop64x48_15")
    sa, hdr, n = _decode(ctx, data)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    sd = ctx.open_stream(hdr.width, hdr.height, 2, 2, hdr.is15, 3)
    for ft, p in pics:
        ctx.submit(sd, ft, p)
    ctx.flush()                                                  # picture 0 of sd: its slot of the ring of 3 was reused
    sq = ctx.open_stream(hdr.width, hdr.height, 2, 2, hdr.is15, 3)
    mem = torch.zeros(ctx.pic_bytes(sa) + 32, dtype=torch.uint8, device="cuda")
    p16 = mem.data_ptr() + (-mem.data_ptr()) % 16
    ok = ((32, 24, 2, 2), None)
    G = lambda *g: (tuple(g), None)
    K = lambda *c: ((32, 24, 2, 2), tuple(c))
    arg = [("bad stream", [sa, 99], [0, 0], None, [ok, ok]), ("an ordinal that is not resident", [sa, sa], [0, 1000], None, [ok, ok]),
           ("negative ordinal", [sa, sa], [0, -1], None, [ok, ok]), ("misaligned src", [sa, sa], [0, -1], [None, p16 + 8], [ok, ok]),
           ("src with an ordinal", [sa, sa], [0, 1], [None, p16], [ok, ok]), ("src with a bad stream", [sa, 99], [0, -1], [None, p16], [ok, ok]),
           ("an empty crop", [sa, sa], [0, 1], None, [ok, K(8, 8, 16, -8)]), ("crop_w == 0 with an offset", [sa, sa], [0, 1], None, [ok, K(2, 0, 0, 0)]),
           ("a crop that leaves the picture", [sa, sa], [0, 1], None, [ok, K(40, 0, 32, 16)]), ("a crop below it", [sa, sa], [0, 1], None, [ok, K(0, 40, 32, 16)]),
           ("a negative crop origin", [sa, sa], [0, 1], None, [ok, K(-2, 0, 32, 16)]), ("an odd crop x on 4:2:0", [sa, sa], [0, 1], None, [ok, K(1, 0, 32, 16)]),
           ("an odd crop height on 4:2:0", [sa, sa], [0, 1], None, [ok, K(0, 0, 32, 15)]), ("a crop narrower than 8", [sa, sa], [0, 1], None, [ok, K(0, 0, 6, 16)]),
           ("a crop lower than 8", [sa, sa], [0, 1], None, [ok, K(0, 0, 16, 6)])]
    for what, sids, ords, src, dsts in arg:
        assert _raw(torch, ctx, sids, ords, src, dsts) == (HVQ_E_ARG, True), what
    # N > 32 M: 64 x 48 cropped to 64 x 8 is fine at 8 x 8 (ratio 8), a target 8 wide from 264 is not -- see case_limit32; here in y: 48 -> 1 row does not exist
    # (a target is 8 at least), so the limit is reached through a larger stream
    big = ctx.open_stream(520, 8, 2, 2, True, 3)
    bmem = torch.zeros(520 * 8 * 3 // 2, dtype=torch.uint8, device="cuda")
    assert _raw(torch, ctx, [sa, big], [0, -1], [None, bmem.data_ptr()], [ok, ((16, 8, 2, 2), None)]) == (HVQ_E_ARG, True), "520 -> 16 is beyond 32"
    for what, g in (("a width that is no multiple of 8", (36, 24, 2, 2)), ("sampling 1 x 2", (32, 24, 1, 2)), ("a height of 0", (32, 0, 2, 2)), ("a width beyond 8192", (8200, 24, 2, 2))):
        assert _raw(torch, ctx, [sa, sa], [0, 1], None, [ok, G(*g)]) == (HVQ_E_GEOMETRY, True), what
    assert _raw(torch, ctx, [sa, sa], [0, 1], None, [ok, ok], ctx_h=C.c_void_p(0)) == (HVQ_E_ARG, True), "null context"
    assert _raw(torch, ctx, [sa, sa], [0, 1], None, [ok, ok], ptr=0) == (HVQ_E_ARG, True), "null ptr"
    assert _raw(torch, ctx, [sa, sa], [0, 1], None, [ok, ok], ptr=p16 + 8) == (HVQ_E_ARG, True), "misaligned ptr"
    assert _raw(torch, ctx, [sa], [0], None, [ok], count=65536) == (HVQ_E_ARG, True), "n beyond 65535"
    assert _raw(torch, ctx, [sa], [0], None, [ok], count=0) == (0, True), "n == 0 does nothing"
    assert lib().hvq_scale_bytes(36, 24, 2, 2) == HVQ_E_GEOMETRY and lib().hvq_scale_bytes(32, 24, 2, 1) == 32 * 24 * 2
    # the HVQ_E_STATE cases: a slot that was reused, a picture queued but not flushed
    assert _raw(torch, ctx, [sa, sd], [0, 0], None, [ok, ok]) == (HVQ_E_STATE, True), "an evicted picture"
    ctx.submit(sq, pics[0][0], pics[0][1])
    assert _raw(torch, ctx, [sa, sq], [0, 0], None, [ok, ok]) == (HVQ_E_STATE, True), "queued but not flushed"
    ctx.flush()
    # the well-formed call right after them works
    from hvqm4_amd import scale
    got, guards = _scale(torch, ctx, [sa, sd, sq], [1, len(pics) - 1, 0], [ok[0]] * 3)
    torch.cuda.synchronize()
    g = _geom(hdr)
    _check(torch, got, guards, [scale.of_picture(ctx.read_picture(s, o), g, ok[0]) for s, o in ((sa, 1), (sd, len(pics) - 1), (sq, 0))], "after the refusals")
    for s in (sa, sd, sq, big):
        ctx.close_stream(s)


def case_ordering(torch, ctx):
    """tests/test_gpu_phash.py's ordering: the scaled pictures of batch k on a side stream beside batch k + 1 in flight, batch k + 2 into
    batch k's slots behind the call; work queued behind the call on the same stream sees the result; a picture of the batch in flight"""
    from hvqm4_amd import scale
    from hvqm4_amd.container import parse_header, video_pictures
    from oracle import bridge
    data = _clip("gop64x48_15")
    hdr = parse_header(data)
    g, dst = _geom(hdr), (40, 24, 2, 2)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    assert len(pics) == 7                            # I P B B P B B
    want = [scale.of_picture(p, g, dst) for p in bridge.oracle_decode(data, 7)]
    sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, 6)
    b = [pics[0:3], pics[3:5], pics[5:7]]
    sub = lambda part: ctx.submit_many_device([sid] * len(part), [ft for ft, _p in part], [p for _f, p in part])
    side = torch.cuda.Stream()
    sub(b[0]); ctx.flush_begin()
    sub(b[1]); ctx.flush_next()                      # batch 0 ended, batch 1 in flight
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got, guards = _scale(torch, ctx, [sid] * 3, [2, 0, 1], [dst] * 3)
        copy = torch.stack(got).clone()              # queued behind the call on the same stream: it sees the result
    sub(b[2]); ctx.flush_next()                      # batch 1 ended, batch 2 in flight
    ctx.flush_end()                                  # batch 2 reconstructed: picture 6 lies in picture 0's slot of the ring of 6
    late, lguards = _scale(torch, ctx, [sid] * 4, [3, 4, 5, 6], [dst] * 4)
    torch.cuda.synchronize()
    _check(torch, got, guards, [want[k] for k in (2, 0, 1)], "batch 0 beside batch 1")
    _check(torch, list(copy), [], [want[k] for k in (2, 0, 1)], "a copy queued behind the call")
    _check(torch, late, lguards, want[3:7], "batches 1 and 2")
    sub(b[0]); ctx.flush_begin()                     # a picture of the batch in flight: the call ends that batch itself
    got, guards = _scale(torch, ctx, [sid], [7 + 2], [dst])
    torch.cuda.synchronize()
    _check(torch, got, guards, [want[2]], "a picture of the batch in flight")
    ctx.close_stream(sid)


def case_composition(torch, ctx):
    """the point of the feature: the scaled picture where it lies feeds picture_checksums(src=), encode_jpeg(src=) and picture_metrics
    (ref.ptr) through an open stream of the target geometry that nothing is submitted to"""
    from hvqm4_amd import checksums, jpeg, scale
    from tests.metrics_ref import metrics_reference
    sn, hn, nn = _decode(ctx, _clip("natural128x96"))
    sg, hg, ng = _decode(ctx, _clip("gop64x48_15"))                 # a resident stream of half natural's size
    dst = (64, 48, 2, 2)
    assert _geom(hg) == dst
    k = list(range(min(nn, ng, 4)))
    scaled = ctx.scale_pictures([sn] * len(k), k, dst[:2])
    assert tuple(scaled.shape) == (len(k), scale.nbytes(*dst))
    carrier = ctx.open_stream(*dst, True, 3)                       # never submitted to
    rows = [scaled[i] for i in range(len(k))]
    sums = ctx.picture_checksums([carrier] * len(k), [-1] * len(k), src=rows)
    files, lengths = ctx.encode_jpeg([carrier] * len(k), [-1] * len(k), quality=85, src=rows)
    met = ctx.picture_metrics([sg] * len(k), k, ref=rows)
    torch.cuda.synchronize()
    host = [scale.of_picture(ctx.read_picture(sn, i), _geom(hn), dst) for i in k]
    assert sums.cpu().tolist() == [checksums.of_bytes(h, *dst) for h in host], "picture_checksums(src=scaled)"
    assert jpeg.files(files, lengths) == [jpeg.encode(h, dst[0], dst[1], 85, dst[2], dst[3]) for h in host], "encode_jpeg(src=scaled)"
    want = np.stack([metrics_reference(ctx.read_picture(sg, i), h, *dst) for i, h in zip(k, host)])
    assert np.array_equal(met.cpu().numpy(), want), "picture_metrics against the scaled picture"
    for s in (sn, sg, carrier):
        ctx.close_stream(s)


def case_thumbnails(torch, ctx):
    """tools/h4m2jpeg.py: with a size, the files are jpeg.encode of the host-scaled pictures; without one, of the pictures themselves"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import h4m2jpeg
    from hvqm4_amd import jpeg, scale
    from oracle import bridge
    data = _clip("yuv422_64x48")
    size = h4m2jpeg.target_size(data, None, 40, None)
    assert size == (40, 32)
    types, thumbs = h4m2jpeg.clip_files(ctx, data, 80, size)
    _t, plain = h4m2jpeg.clip_files(ctx, data, 80)
    pics = bridge.oracle_decode(data, len(types))
    g = (64, 48, 2, 1)
    assert thumbs == [jpeg.encode(scale.of_picture(p, g, size + (2, 1)), size[0], size[1], 80, 2, 1) for p in pics]
    assert plain == [jpeg.encode(p, 64, 48, 80, 2, 1) for p in pics]


CASES = ["identity", "integer", "noninteger", "enlarge", "sampling", "crops", "limit32", "cells64", "ties", "many", "body", "refusals", "ordering",
         "composition", "thumbnails"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "scale", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_scale(case, child_results):
    gpu_child.report(case, child_results)
