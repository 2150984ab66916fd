"""GPU: filtered pictures in slot layout (hvq_filter_pictures / Context.filter_pictures) against hvqm4_amd.filters.of_picture, compared
with == (tests/test_filters_cpu.py compares that module with tests/filter_ref.py, the plain-Python restatement of include/hvqm4_amd.h).
Every output is allocated with 256 sentinel bytes before and behind it, which must stay untouched.  The cases run in ONE child process
that imports torch first (see tests/gpu_child.py); each test reports its case.  The child stops at the first HVQ_E_HIP or HIP
error: nothing more is started on a GPU that has reported a fault."""
import json
import os
import zlib
from fractions import Fraction

import numpy as np
import pytest

from tests import gpu_child
from tests.gpu_kit import ROOT, SENTINEL, check_bytes as _check, clip as _clip, decode as _decode, geom as _geom, geometry_rooms as _rooms

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300                                 # the cases take seconds each; a hung child is ended, not waited for
SAMPLINGS = ((2, 2), (2, 1), (1, 1))


# ------------------------------------------------------------------------------------------------------------- child side
def _nbytes(g):
    from hvqm4_amd import scale
    return scale.nbytes(*g)


def _filter(torch, ctx, sids, ords, geoms, filt, src=None):
    """one call -> (list of n uint8 tensors, guards)"""
    out, guards = _rooms(torch, geoms)
    got = ctx.filter_pictures(sids, ords, filt, src, out)
    assert got is out
    return [out[i] for i in range(len(geoms))], guards


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


def _upload_check(torch, ctx, jobs, what):
    """jobs: [(geometry, picture as a uint8 array, Filter)] through src= in ONE call, on streams nothing was decoded into"""
    from hvqm4_amd import filters as F
    sids = {}
    for g, _p, _f in jobs:
        if g not in sids:
            sids[g] = ctx.open_stream(g[0], g[1], g[2], g[3], True, 3)
    bufs = [torch.from_numpy(np.array(p, dtype=np.uint8)).cuda() for _g, p, _f in jobs]
    got, guards = _filter(torch, ctx, [sids[g] for g, _p, _f in jobs], [-1] * len(jobs), [g for g, _p, _f in jobs], [f for _g, _p, f in jobs], src=bufs)
    torch.cuda.synchronize()
    _check(torch, got, guards, [F.of_picture(p, g, f) for g, p, f in jobs], what)
    for s in sids.values():
        ctx.close_stream(s)
    return got


def _plane(*terms, combine=0, shift=0, bias=0):
    from hvqm4_amd import filters as F
    return F.PlaneFilter(tuple(F.Term(tuple(wx), tuple(wy)) for wx, wy in terms), combine, shift, bias)


def _same(p):
    from hvqm4_amd import filters as F
    return F.Filter(p, p)


def case_identity(torch, ctx):
    """the smallest geometry and 72 x 24 (one tile and a remainder in both axes) in the three samplings: the bytes themselves"""
    from hvqm4_amd import filters as F
    jobs = [((w, h) + s, c, F.identity()) for (w, h) in ((8, 8), (72, 24)) for s in SAMPLINGS for c in _contents((w, h) + s, w)[:1]]
    got = _upload_check(torch, ctx, jobs, "identity")
    for g, (_geom2, p, _f) in zip(got, jobs):
        assert np.array_equal(g.cpu().numpy(), p), "identity is not the picture"


def _radius_filters():
    ones = lambda r: (1,) * (2 * r + 1)
    ramp = lambda r: tuple(range(1, 2 * r + 2))
    out = []
    for r in (1, 7, 15):
        sh = (2 * r + 1).bit_length()
        out += [_same(_plane((ramp(r), (1,)), shift=sh + r.bit_length())), _same(_plane(((1,), ramp(r)), shift=sh + r.bit_length())),
                _same(_plane((ramp(r), ones(r)), shift=2 * sh + r.bit_length() - 1))]
    return out


def case_seams(torch, ctx):
    """136 x 40: three tile columns and rows, none full at the edge, under radius 1, 7 and 15 in each axis separately and together
    (non-symmetric taps); random, 0 / 255 and checkerboard content"""
    g = (136, 40, 2, 2)
    assert 136 > 2 * 64 and 136 % 64 and 40 > 2 * 16 and 40 % 16
    jobs = [(g, c, f) for f in _radius_filters() for c in _contents(g, 136)]
    _upload_check(torch, ctx, jobs, "tile seams")


def case_narrow(torch, ctx):
    """radius 15 on the smallest geometry: the chroma planes are 4 samples wide, far narrower than the halo"""
    from hvqm4_amd import filters as F
    fs = _radius_filters()[6:] + [F.gaussian(5.0, 15, 8), _same(_plane(((1,) * 31, (1,) * 31), (tuple((-1) ** i * 3 for i in range(31)), (1,) * 31), combine=F.SUM_ABS, shift=10))]
    jobs = [((8, 8) + s, c, f) for s in SAMPLINGS for f in fs for c in _contents((8, 8) + s, 8)]
    _upload_check(torch, ctx, jobs, "radius 15 on 8 x 8")


def case_orientation(torch, ctx):
    """the one-sample shift in each of the four directions: tap i meets the sample i - r to the right / below, the border replicates"""
    g = (72, 24, 1, 1)
    pic = _contents(g, 5)[0]
    shifts = {"left": _plane(((1, 0, 0), (1,))), "right": _plane(((0, 0, 1), (1,))), "up": _plane(((1,), (1, 0, 0))), "down": _plane(((1,), (0, 0, 1)))}
    got = _upload_check(torch, ctx, [(g, pic, _same(p)) for p in shifts.values()], "orientation")
    y = pic[:72 * 24].reshape(24, 72)
    idx = np.arange(72)
    want = {"left": y[:, np.maximum(idx - 1, 0)], "right": y[:, np.minimum(idx + 1, 71)], "up": y[np.maximum(np.arange(24) - 1, 0)], "down": y[np.minimum(np.arange(24) + 1, 23)]}
    for name, t in zip(shifts, got):
        assert np.array_equal(t.cpu().numpy()[:72 * 24].reshape(24, 72), want[name]), name


def case_signed(torch, ctx):
    """Sobel with bias 128; ABS_SUM; SUM_ABS with two terms; the Laplacian; unsharp clamping at 0 and 255; the two negative ties; the
    maximum-gain filter on the checkerboard"""
    from hvqm4_amd import filters as F
    g = (72, 24, 2, 2)
    sob = ((-1, 0, 1), (1, 2, 1)), ((1, 2, 1), (-1, 0, 1))
    fs = [F.sobel("x"), F.sobel("y"), F.scharr("x"), _same(_plane(*sob, combine=F.ABS_SUM, shift=2)), F.gradient_magnitude("sobel"), F.gradient_magnitude("scharr"),
          F.laplacian(), F.dog(1.0, 2.0), F.unsharp(1.0, 3), F.unsharp(2.0, Fraction(1, 2)),
          _same(_plane(((-1, -1, -1), (1, 1, 1)), ((1,), (2,)), shift=1, bias=255)), _same(_plane(((1,), (1,)), bias=-255))]
    jobs = [(g, c, f) for f in fs for c in _contents(g, 72)]
    got = _upload_check(torch, ctx, jobs, "signed sums")
    sharp = got[8 * 3 + 1].cpu().numpy()                       # unsharp(1.0, 3) on 0 / 255 content
    assert sharp.min() == 0 and sharp.max() == 255
    flat = np.full(_nbytes(g), 77, dtype=np.uint8)
    assert bool(_upload_check(torch, ctx, [(g, flat, F.sobel("x"))], "Sobel on a flat picture")[0].eq(128).all())
    # S = -a with shift 1: a = 1 -> S = -1 -> 0, a = 3 -> S = -3 -> -1; bias 2 makes both visible
    tie = _same(_plane(((-1,), (1,)), shift=1, bias=2))
    pic = np.tile(np.array([1, 3], dtype=np.uint8), _nbytes((8, 8, 1, 1)) // 2)
    t = _upload_check(torch, ctx, [((8, 8, 1, 1), pic, tie)], "the negative ties")[0].cpu().numpy()
    assert t.tolist() == [2, 1] * (t.size // 2)
    maxgain = _same(_plane(((1024, 0, 1024), (1024, 0, 1024)), shift=22))
    neg = _same(_plane(((-1024, 0, -1024), (1024, 0, 1024)), shift=22, bias=255))
    two = _same(_plane(((1024, 0, 1024), (512, 0, 512)), ((-1024, 0, -1024), (512, 0, 512)), combine=F.SUM_ABS, shift=22))
    assert F.gain(maxgain.luma) == F.gain(neg.luma) == F.gain(two.luma) == F.MAX_GAIN
    gm = (136, 40, 2, 2)
    boards = [_contents(gm, k)[2] for k in (0, 1)] + [np.full(_nbytes(gm), 255, dtype=np.uint8)]
    got = _upload_check(torch, ctx, [(gm, b, f) for f in (maxgain, neg, two) for b in boards], "the maximum gain")
    y = got[0].cpu().numpy()[:136 * 40]
    assert {0, 255} <= set(np.unique(y).tolist()), "255 * 2^22 is reached"


def case_chroma(torch, ctx):
    """luma only: the chroma bytes are the source's; chroma_for on 4:2:0, 4:2:2 and 4:4:4"""
    from hvqm4_amd import filters as F
    jobs, lumas = [], []
    for s in SAMPLINGS:
        g = (72, 24) + s
        pic = _contents(g, 3)[0]
        jobs += [(g, pic, F.luma_only(F.gaussian(2.0))), (g, pic, F.chroma_for(F.gaussian(3.0), *s)), (g, pic, F.chroma_for(F.unsharp(2.0, Fraction(3, 4)), *s)),
                 (g, pic, F.Filter(F.identity().luma, F.binomial(5).luma))]
        lumas.append((g, pic))
    got = _upload_check(torch, ctx, jobs, "chroma")
    for i, (g, pic) in enumerate(lumas):
        assert np.array_equal(got[4 * i].cpu().numpy()[72 * 24:], pic[72 * 24:]), "luma only changed the chroma planes"
        assert np.array_equal(got[4 * i + 3].cpu().numpy()[:72 * 24], pic[:72 * 24]), "chroma only changed the luma plane"
    assert F.chroma_for(F.gaussian(3.0), 2, 1).chroma.terms[0].wx == F.gaussian_taps(1.5) != F.gaussian_taps(3.0)


def _eight_filters():
    from hvqm4_amd import filters as F
    return [F.binomial(3), F.identity(), F.luma_only(F.gaussian(1.5)), F.gaussian(5.0, 15, 8), F.sobel("x"), F.luma_only(F.gradient_magnitude()), F.laplacian(),
            F.luma_only(F.unsharp(1.0, Fraction(1, 2))), F.dog(1.0, 2.0), F.chroma_for(F.gaussian(2.0), 2, 2)]


def case_many(torch, ctx):
    """one launch: 300 pictures of eight clips (more than four geometries) and ten filters chosen through `which`; both forms of out"""
    from hvqm4_amd import filters as F
    names = ["gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8", "i16", "natural128x96"]
    streams = {nm: _decode(ctx, _clip(nm)) for nm in names}
    fs = _eight_filters()
    sids, ords, geoms, filt = [], [], [], []
    for i in range(300):
        sid, hdr, n = streams[names[i % len(names)]]
        sids.append(sid); ords.append(i % n); geoms.append(_geom(hdr)); filt.append(fs[(i // len(names) + i) % len(fs)])
    assert len(set(geoms)) >= 4 and len(set(filt)) >= 8
    got, guards = _filter(torch, ctx, sids, ords, geoms, filt)               # a list: the geometries differ
    torch.cuda.synchronize()
    cache, wants = {}, []
    for s, o, g, f in zip(sids, ords, geoms, filt):
        if (s, o) not in cache:
            cache[s, o] = ctx.read_picture(s, o)
        if (s, o, f) not in cache:
            cache[s, o, f] = F.of_picture(cache[s, o], g, f)
        wants.append(cache[s, o, f])
    _check(torch, got, guards, wants, "many shapes")
    # one geometry: one tensor [n, bytes], given and not given
    sid, hdr, n = streams["natural128x96"]
    k = [i % n for i in range(12)]
    f12 = [fs[i % len(fs)] for i in range(12)]
    got, guards = _filter(torch, ctx, [sid] * 12, k, [_geom(hdr)] * 12, f12)
    fresh = ctx.filter_pictures([sid] * 12, k, f12)
    torch.cuda.synchronize()
    w12 = [cache.get((sid, o, f), None) if (sid, o, f) in cache else F.of_picture(ctx.read_picture(sid, o), _geom(hdr), f) for o, f in zip(k, f12)]
    _check(torch, got, guards, w12, "one tensor, given")
    assert tuple(fresh.shape) == (12, _nbytes(_geom(hdr)))
    _check(torch, list(fresh), [], w12, "one tensor, returned")
    for sid, _h, _n in streams.values():
        ctx.close_stream(sid)


def case_sources(torch, ctx):
    """src= from the caller's memory, 16 bytes into an allocation too, mixed with resident pictures in one call"""
    from hvqm4_amd import filters as F
    sid, hdr, n = _decode(ctx, _clip("yuv422_64x48"))
    g = _geom(hdr)
    pics = [ctx.read_picture(sid, k) for k in range(n)]
    f = F.chroma_for(F.gaussian(1.5), *g[2:])
    src, sids, ords, wants = [], [], [], []
    for k in range(n):
        inv = 255 - np.asarray(pics[k]).reshape(-1)
        room = torch.zeros(inv.size + 32, dtype=torch.uint8, device="cuda")
        off = (-room.data_ptr()) % 16 + (16 if k & 1 else 0)
        room[off:off + inv.size] = torch.from_numpy(inv).cuda()
        src += [room[off:off + inv.size], None]; sids += [sid, sid]; ords += [-1, k]
        wants += [F.of_picture(inv, g, f), F.of_picture(pics[k], g, f)]
    got, guards = _filter(torch, ctx, sids, ords, [g] * len(sids), f, src=src)
    torch.cuda.synchronize()
    _check(torch, got, guards, wants, "the caller's memory and resident pictures")
    ctx.close_stream(sid)


def _fixture_filters(hs, vs):
    from hvqm4_amd import filters as F
    return [("gauss1.5", F.chroma_for(F.gaussian(1.5), hs, vs)), ("unsharp1.0_1/2", F.luma_only(F.unsharp(1.0, Fraction(1, 2)))),
            ("sobelmag", F.luma_only(F.gradient_magnitude("sobel")))]


def case_golden(torch, ctx):
    """every clip of tests/golden/filter.json decoded on the GPU, its last picture through the fixture's three filters in one call"""
    fixture = json.load(open(os.path.join(ROOT, "tests", "golden", "filter.json")))["clips"]
    manifest = json.load(open(os.path.join(ROOT, "tests", "golden", "manifest.json")))["clips"]
    assert set(fixture) == {nm for nm, c in manifest.items() if "file" in c}
    sids, ords, geoms, filt, crcs, streams = [], [], [], [], [], []
    for name, entry in sorted(fixture.items()):
        sid, hdr, n = _decode(ctx, open(os.path.join(ROOT, "tests", "golden", manifest[name]["file"]), "rb").read())
        streams.append(sid)
        assert _geom(hdr) == tuple(entry["geometry"])
        for (label, crc), (label2, f) in zip(entry["filters"], _fixture_filters(hdr.h_samp, hdr.v_samp)):
            assert label == label2
            sids.append(sid); ords.append(n - 1); geoms.append(_geom(hdr)); filt.append(f); crcs.append((name, label, crc))
    got, guards = _filter(torch, ctx, sids, ords, geoms, filt)
    torch.cuda.synchronize()
    for g in guards:
        assert bool(g.eq(SENTINEL).all())
    for t, (name, label, crc) in zip(got, crcs):
        assert zlib.crc32(t.cpu().numpy().tobytes()) == crc, (name, label)
    for s in streams:
        ctx.close_stream(s)


def case_composition(torch, ctx):
    """the filtered picture where it lies feeds scale_pictures(src=) (a Gaussian pyramid level), picture_histograms(src=) (the
    sharpness measure) and encode_jpeg(src=) (the sharpened picture), nothing read back in between"""
    from hvqm4_amd import filters as F
    from hvqm4_amd import histograms, jpeg, scale
    sn, hn, nn = _decode(ctx, _clip("natural128x96"))
    g = _geom(hn)
    k = list(range(min(nn, 4)))
    host = [ctx.read_picture(sn, i) for i in k]
    blur, mag, sharp = F.chroma_for(F.gaussian(1.0), *g[2:]), F.luma_only(F.gradient_magnitude()), F.luma_only(F.unsharp(1.0, Fraction(1, 2)))
    half = scale.pyramid(g[0], g[1], 2)[1]
    blurred = ctx.filter_pictures([sn] * len(k), k, blur)
    level = ctx.scale_pictures([sn] * len(k), [-1] * len(k), half, src=[blurred[i] for i in range(len(k))])
    edges = ctx.filter_pictures([sn] * len(k), k, mag)
    hist = ctx.picture_histograms([sn] * len(k), [-1] * len(k), src=[edges[i] for i in range(len(k))])
    sharpened = ctx.filter_pictures([sn] * len(k), k, sharp)
    files, lengths = ctx.encode_jpeg([sn] * len(k), [-1] * len(k), quality=85, src=[sharpened[i] for i in range(len(k))])
    torch.cuda.synchronize()
    want_level = [scale.of_picture(F.of_picture(h, g, blur), g, half + g[2:]) for h in host]
    _check(torch, list(level), [], want_level, "filter -> scale_pictures(src=)")
    want_hist = np.stack([histograms.of_picture(F.of_picture(h, g, mag), *g) for h in host])
    assert np.array_equal(hist.cpu().numpy(), want_hist), "filter -> picture_histograms(src=)"
    assert np.array_equal(F.sharpness(hist.cpu().numpy())[:, 0], histograms.mean(want_hist)[:, 0])
    assert jpeg.files(files, lengths) == [jpeg.encode(F.of_picture(h, g, sharp), g[0], g[1], 85, g[2], g[3]) for h in host], "filter -> encode_jpeg(src=)"
    ctx.close_stream(sn)


def case_ordering(torch, ctx):
    """tests/test_gpu_scale.py's ordering: the filtered pictures of batch k on a side stream beside batch k + 1 in flight, batch k + 2
    into batch k's slots behind the call; work queued behind the call on the same stream sees the result; a picture of the batch in
    flight"""
    from hvqm4_amd import filters as F
    from hvqm4_amd.container import parse_header, video_pictures
    from oracle import bridge
    data = _clip("gop64x48_15")
    hdr = parse_header(data)
    g, f = _geom(hdr), F.gaussian(1.5)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    assert len(pics) == 7                            # I P B B P B B
    want = [F.of_picture(p, g, f) for p in bridge.oracle_decode(data, 7)]
    sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, 6)
    b = [pics[0:3], pics[3:5], pics[5:7]]
    sub = lambda part: ctx.submit_many_device([sid] * len(part), [ft for ft, _p in part], [p for _f, p in part])
    side = torch.cuda.Stream()
    sub(b[0]); ctx.flush_begin()
    sub(b[1]); ctx.flush_next()                      # batch 0 ended, batch 1 in flight
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got, guards = _filter(torch, ctx, [sid] * 3, [2, 0, 1], [g] * 3, f)
        copy = torch.stack(got).clone()              # queued behind the call on the same stream: it sees the result
    sub(b[2]); ctx.flush_next()                      # batch 1 ended, batch 2 in flight
    ctx.flush_end()                                  # batch 2 reconstructed: picture 6 lies in picture 0's slot of the ring of 6
    late, lguards = _filter(torch, ctx, [sid] * 4, [3, 4, 5, 6], [g] * 4, f)
    torch.cuda.synchronize()
    _check(torch, got, guards, [want[k] for k in (2, 0, 1)], "batch 0 beside batch 1")
    _check(torch, list(copy), [], [want[k] for k in (2, 0, 1)], "a copy queued behind the call")
    _check(torch, late, lguards, want[3:7], "batches 1 and 2")
    sub(b[0]); ctx.flush_begin()                     # a picture of the batch in flight: the call ends that batch itself
    got, guards = _filter(torch, ctx, [sid], [7 + 2], [g], f)
    torch.cuda.synchronize()
    _check(torch, got, guards, [want[2]], "a picture of the batch in flight")
    ctx.close_stream(sid)


def _raw(torch, ctx, sids, ords, src, structs, which=None, nfilters=None, count=None, ctx_h=None, ptr=None, null_filters=False):
    """hvq_filter_pictures through the C ABI into sentinel-filled memory -> (return code, every byte still holds the sentinel).
    structs: the HvqFilter table; ptr: the destination pointer of picture 0 instead of the room's"""
    import ctypes as C
    from hvqm4_amd._lib import HvqFilter, lib
    n = len(sids)
    room = torch.full((n, 8192), SENTINEL, dtype=torch.uint8, device="cuda")
    a_d = (C.c_void_p * n)(*[(ptr if ptr is not None and i == 0 else room[i].data_ptr()) for i in range(n)])
    a_p = C.cast((C.c_void_p * n)(*src), C.c_void_p) if src is not None else None
    a_f = (HvqFilter * len(structs))(*structs)
    a_w = C.cast((C.c_int * n)(*which), C.c_void_p) if which is not None else None
    rc = lib().hvq_filter_pictures(ctx._h if ctx_h is None else ctx_h, n if count is None else count, (C.c_int * n)(*sids), (C.c_int * n)(*ords), a_p,
                                   None if null_filters else C.cast(a_f, C.c_void_p), len(structs) if nfilters is None else nfilters, a_w, C.cast(a_d, C.c_void_p),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, bool(room.eq(SENTINEL).all())


def case_refusals(torch, ctx):
    """every refusal of the header through the C entry leaves the destinations untouched, also those of the well-formed pictures of
    the same call"""
    import ctypes as C
    from hvqm4_amd import filters as F
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_STATE
    from hvqm4_amd.container import video_pictures
    from tests.test_filters_cpu import _spoiled
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
    good = F.binomial(3).to_struct()
    two = [sa, sa]
    for label, s in _spoiled():                                  # every refusal of hvq_filter_check, in a filter of the table that no picture uses
        assert _raw(torch, ctx, two, [0, 1], None, [good, s], which=[0, 0]) == (HVQ_E_ARG, True), label
        assert _raw(torch, ctx, two, [0, 1], None, [s]) == (HVQ_E_ARG, True), label
    arg = [("bad stream", [sa, 99], [0, 0], None, {}), ("an ordinal that is not resident", two, [0, 1000], None, {}), ("negative ordinal", two, [0, -1], None, {}),
           ("misaligned src", two, [0, -1], [None, p16 + 8], {}), ("an ordinal with src", two, [0, 1], [None, p16], {}),
           ("src with a bad stream", [sa, 99], [0, -1], [None, p16], {}), ("which beyond the table", two, [0, 1], None, {"which": [0, 1]}),
           ("a negative which", two, [0, 1], None, {"which": [0, -1]}), ("nfilters 0", two, [0, 1], None, {"nfilters": 0}), ("nfilters -1", two, [0, 1], None, {"nfilters": -1}),
           ("null filters", two, [0, 1], None, {"null_filters": True}), ("null context", two, [0, 1], None, {"ctx_h": C.c_void_p(0)}),
           ("null dst", two, [0, 1], None, {"ptr": 0}), ("misaligned dst", two, [0, 1], None, {"ptr": p16 + 8})]
    for what, sids, ords, src, kw in arg:
        assert _raw(torch, ctx, sids, ords, src, [good], **kw) == (HVQ_E_ARG, True), what
    assert _raw(torch, ctx, two, [0, 1], None, [good] * 65, which=[0, 64]) == (HVQ_E_ARG, True), "nfilters 65"
    assert _raw(torch, ctx, [sa], [0], None, [good], count=65536) == (HVQ_E_ARG, True), "n beyond 65535"
    assert _raw(torch, ctx, [sa], [0], None, [good], count=0) == (0, True), "n == 0 does nothing"
    # the HVQ_E_STATE cases: a slot that was reused, a picture queued but not flushed
    assert _raw(torch, ctx, [sa, sd], [0, 0], None, [good]) == (HVQ_E_STATE, True), "an evicted picture"
    ctx.submit(sq, pics[0][0], pics[0][1])
    assert _raw(torch, ctx, [sa, sq], [0, 0], None, [good]) == (HVQ_E_STATE, True), "queued but not flushed"
    ctx.flush()
    # the well-formed calls right after them work: a table of 64 with the last one used, and the method
    rc, untouched = _raw(torch, ctx, two, [0, 1], None, [good] * 64, which=[0, 63])
    assert rc == 0 and not untouched
    g = _geom(hdr)
    got, guards = _filter(torch, ctx, [sa, sd, sq], [1, len(pics) - 1, 0], [g] * 3, F.binomial(3))
    torch.cuda.synchronize()
    _check(torch, got, guards, [F.of_picture(ctx.read_picture(s, o), g, F.binomial(3)) for s, o in ((sa, 1), (sd, len(pics) - 1), (sq, 0))], "after the refusals")
    for s in (sa, sd, sq):
        ctx.close_stream(s)


def case_bodies(torch, ctx):
    """identity planes through the copy body (chosen) and through the filter body (forced): the same bytes"""
    from hvqm4_amd import filters as F
    jobs = []
    for s in SAMPLINGS:
        for wh in ((8, 8), (72, 24), (264, 40)):                # 264 > 256: two tiles of the copy body side by side
            g = wh + s
            jobs += [(g, _contents(g, 9)[0], f) for f in (F.identity(), F.luma_only(F.binomial(3)), F.Filter(F.identity().luma, F.binomial(3).luma))]
    chosen = _upload_check(torch, ctx, jobs, "the chosen body")
    assert ctx.filter_force_filter(True) is False
    try:
        forced = _upload_check(torch, ctx, jobs, "the forced filter body")
    finally:
        assert ctx.filter_force_filter(False) is True
    for a, b in zip(chosen, forced):
        assert bool(a.eq(b).all())


CASES = ["identity", "seams", "narrow", "orientation", "signed", "chroma", "many", "sources", "golden", "composition", "ordering", "refusals", "bodies"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "filters", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_filters(case, child_results):
    gpu_child.report(case, child_results)
