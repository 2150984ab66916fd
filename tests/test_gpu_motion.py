"""GPU: motion fields (hvq_picture_motion, Context.picture_motion) against tests/motion_ref.py on the oracle's pictures and on caller
memory of chosen content, compared with ==: the records are exact integers.  The cases run in ONE child process that imports torch first
(see tests/gpu_child.py); each test reports its case.  The child stops at the first HVQ_E_HIP or HIP error: nothing more is started
on a GPU that has reported a fault.

Picture `a` of a call is always a resident picture, so it cannot be given chosen content; the reference `b` can (the caller's memory).  The
tie cases plant a block of a resident picture twice in random b.  The flat case uploads a flat b: every candidate of every block then
costs the same, sum |a - v|, whatever a holds, and (0, 0) must win everywhere -- the property flat-against-flat has (which
tests/test_motion_cpu.py checks on the reference itself)."""
import numpy as np
import pytest

from tests import gpu_child
from tests.gpu_kit import decode as _decode, golden_by_name as _golden, long_clip_data as _long_clip, oracle as _oracle

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300                                 # the cases take seconds each; a hung child is ended, not waited for
SENTINEL = 0x5A5A5A5A
GUARD = 16                                          # int32 elements: 64 bytes on either side of a field
SIX = ["gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8"]


# ------------------------------------------------------------------------------------------------------------- child side
_state = {}


def _want(key, a, b, hdr, B, R):
    from tests.motion_ref import cached
    return cached(key, a, b, hdr.width, hdr.height, B, R)


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(-1))
        raise AssertionError(f"{what}: {len(bad)} of {got.shape[0] * got.shape[1]} records differ, first at block {tuple(bad[0])}: got "
                             f"{got[tuple(bad[0])].tolist()}, want {want[tuple(bad[0])].tolist()}")


def _six(ctx):
    """the six clips decoded once for all cases: name -> (sid, hdr, n, the oracle's pictures)"""
    if "six" not in _state:
        g = _golden()
        _state["six"] = {}
        for name in SIX:
            data, hdr, n = g[name]
            sid, hdr, n = _decode(ctx, data)
            _state["six"][name] = (sid, hdr, n, _oracle(name, data, n))
    return _state["six"]


def _pairs(six, names=SIX):
    """every picture of the clips against its predecessor: (name, sid, hdr, k, yuv)"""
    return [(name, six[name][0], six[name][1], k, six[name][3]) for name in names for k in range(1, six[name][2])]


def _guarded(torch, dims):
    """fields between guards, all filled with the sentinel: (the buffers, the fields as views of them)"""
    bufs = [torch.full((2 * GUARD + r * c * 4,), SENTINEL, dtype=torch.int32, device="cuda") for r, c in dims]
    return bufs, [b[GUARD:GUARD + r * c * 4].view(r, c, 4) for b, (r, c) in zip(bufs, dims)]


def case_goldens(torch, ctx):
    """the six clips in ONE call of mixed geometries, each picture against its predecessor, B = 8, R = 15 (24 x 40: the radius exceeds the
    picture, the window is clipped on all four sides; 296 x 160: 37 block columns, the right edge tile is partial; 4:4:4 and 4:2:2: luma
    has nothing to do with the chroma layout) into sentinel-filled fields between guards; the same call twice; cost_zero sums to
    picture_metrics' Y sad"""
    from hvqm4_amd.motion import blocks
    six = _six(ctx)
    assert {(h.h_samp, h.v_samp) for _s, h, _n, _y in six.values()} == {(2, 2), (2, 1), (1, 1)}
    P = _pairs(six)
    sids, ords, refs = [p[1] for p in P], [p[3] for p in P], [(p[1], p[3] - 1) for p in P]
    bufs, fields = _guarded(torch, [blocks(p[2].width, p[2].height, 8) for p in P])
    got = ctx.picture_motion(sids, ords, refs, block=8, radius=15, out=fields)
    again = ctx.picture_motion(sids, ords, refs, block=8, radius=15)
    met = ctx.picture_metrics(sids, ords, refs)
    torch.cuda.synchronize()
    assert all(g is f for g, f in zip(got, fields))
    for (name, _sid, hdr, k, yuv), f, f2, buf, m in zip(P, got, again, bufs, met):
        _same(f, _want((name, k, k - 1), yuv[k], yuv[k - 1], hdr, 8, 15), (name, k, "B 8 R 15"))      # no record holds the sentinel: all are written
        assert buf[:GUARD].eq(SENTINEL).all() and buf[-GUARD:].eq(SENTINEL).all(), (name, k, "a guard was written")
        assert torch.equal(f, f2), (name, k, "the same call twice")
        assert int(f[..., 3].sum()) == int(m[0, 2]), (name, k, "cost_zero sums to the Y sad of picture_metrics")
    assert ctx.picture_motion([], [], []) == []


def case_radii(torch, ctx):
    """the same pairs at R = 0 (cost is cost_zero, every vector zero), R = 1 and R = 7"""
    six = _six(ctx)
    P = _pairs(six)
    sids, ords, refs = [p[1] for p in P], [p[3] for p in P], [(p[1], p[3] - 1) for p in P]
    got = {R: ctx.picture_motion(sids, ords, refs, block=8, radius=R) for R in (0, 1, 7)}
    torch.cuda.synchronize()
    for R, fields in got.items():
        for (name, _sid, hdr, k, yuv), f in zip(P, fields):
            _same(f, _want((name, k, k - 1), yuv[k], yuv[k - 1], hdr, 8, R), (name, k, f"B 8 R {R}"))
    for f in got[0]:
        assert not f[..., :2].any() and torch.equal(f[..., 2], f[..., 3])


def case_block16(torch, ctx):
    """B = 16 on the clips whose luma is a multiple of 16 in both directions; on the others the whole call is HVQ_E_ARG"""
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, lib
    from hvqm4_amd.metrics import HvqMetricsRef as Rf
    six = _six(ctx)
    tiled = [nm for nm in SIX if six[nm][1].width % 16 == 0 and six[nm][1].height % 16 == 0]
    others = [nm for nm in SIX if nm not in tiled]
    assert tiled == ["gop64x48_15", "yuv444_13_portrait48x64"] and len(others) == 4
    P = _pairs(six, tiled)
    sids, ords, refs = [p[1] for p in P], [p[3] for p in P], [(p[1], p[3] - 1) for p in P]
    got = ctx.picture_motion(sids, ords, refs, block=16, radius=15)
    small = ctx.picture_motion(sids, ords, refs, block=16, radius=2)
    torch.cuda.synchronize()
    for (name, _sid, hdr, k, yuv), f, f2 in zip(P, got, small):
        _same(f, _want((name, k, k - 1), yuv[k], yuv[k - 1], hdr, 16, 15), (name, k, "B 16 R 15"))
        _same(f2, _want((name, k, k - 1), yuv[k], yuv[k - 1], hdr, 16, 2), (name, k, "B 16 R 2"))
    # a stream that blocks of 16 do not tile, behind one they do: the library refuses the whole call and writes nothing
    out = torch.full((2, 64, 4), SENTINEL, dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for nm in others:
        sid = six[nm][0]
        s2, o2 = [six[tiled[0]][0], sid], [1, 1]
        r2 = (Rf * 2)(Rf(s2[0], 0, None), Rf(sid, 0, None))
        ptrs = (C.c_void_p * 2)(out[0].data_ptr(), out[1].data_ptr())
        rc = lib().hvq_picture_motion(ctx._h, 2, (C.c_int * 2)(*s2), (C.c_int * 2)(*o2), C.cast(r2, C.c_void_p), 16, 8, C.cast(ptrs, C.c_void_p), stream)
        assert rc == HVQ_E_ARG, (nm, rc)
        try:
            ctx.picture_motion(s2, o2, [(s2[0], 0), (sid, 0)], block=16)
        except ValueError:
            pass
        else:
            raise AssertionError((nm, "blocks of 16 were accepted"))
    torch.cuda.synchronize()
    assert out.eq(SENTINEL).all()


def case_tiles(torch, ctx):
    """one 320 x 240 pair at B = 16, R = 15: 5 x 4 workgroup tiles, the bottom row of tiles partial"""
    from tests import clips
    clip = clips.get([c for c in clips.MEDIUM if c[0] == "pselfref320x240"][0])
    yuv = _oracle("pselfref320x240", clip.data, clip.n_pictures)
    sid, hdr, _n = _decode(ctx, clip.data)
    assert (hdr.width, hdr.height) == (320, 240)
    got = ctx.picture_motion([sid], [1], [(sid, 0)], block=16, radius=15)
    torch.cuda.synchronize()
    _same(got[0], _want(("pselfref320x240", 1, 0), yuv[1], yuv[0], hdr, 16, 15), "320 x 240, B 16 R 15")
    assert tuple(got[0].shape) == (15, 20, 4)
    ctx.close_stream(sid)


def case_planted(torch, ctx):
    """the three tie cases (block (2, 3) of a resident picture planted twice in random b, B = 8, R = 8) and flat references, uploaded as the
    caller's memory; a picture against itself, resident and as a copy in the caller's memory"""
    from tests.motion_ref import motion_reference
    six = _six(ctx)
    sid, hdr, _n, yuv = six["gop64x48_15"]
    W, H = hdr.width, hdr.height
    a = yuv[2]
    ya = a[:W * H].reshape(H, W)
    y0, x0 = 16, 24
    assert len(np.unique(ya[y0:y0 + 8, x0:x0 + 8])) > 4, "the planted block has content"
    rng = np.random.default_rng(20261019)
    hosts, wins = [], []
    for first, second, winner in (((0, 5), (-4, -4), (0, 5)), ((-8, 0), (0, -8), (-8, 0)), ((0, -8), (0, 8), (0, -8))):
        b = rng.integers(0, 256, a.size, dtype=np.uint8)
        yb = b[:W * H].reshape(H, W)
        for dy, dx in (first, second):
            yb[y0 + dy:y0 + dy + 8, x0 + dx:x0 + dx + 8] = ya[y0:y0 + 8, x0:x0 + 8]
        hosts.append(b); wins.append(winner)
    for v in (0, 97, 255):
        hosts.append(np.full(a.size, v, dtype=np.uint8)); wins.append(None)
    hosts.append(a.copy()); wins.append("self")
    dev = [torch.from_numpy(b).cuda() for b in hosts]
    n = len(dev)
    got = ctx.picture_motion([sid] * n, [2] * n, dev, block=8, radius=8)
    got16 = ctx.picture_motion([sid] * n, [2] * n, dev, block=16, radius=15)
    itself = ctx.picture_motion([sid, sid], [2, 3], [(sid, 2), (sid, 3)], block=8, radius=15)
    torch.cuda.synchronize()
    for i, (b, win) in enumerate(zip(hosts, wins)):
        f = got[i].cpu().numpy()
        _same(got[i], motion_reference(a, b, W, H, 8, 8), ("planted", i, 8))
        _same(got16[i], motion_reference(a, b, W, H, 16, 15), ("planted", i, 16))
        if win == "self":
            assert not f.any() and not got16[i].any()
        elif win is None:                                      # flat b: every candidate ties, (0, 0) wins
            assert not f[..., :2].any() and (f[..., 2] == f[..., 3]).all() and not got16[i][..., :2].any()
        else:
            assert f[2, 3, :3].tolist() == [win[0], win[1], 0] and f[2, 3, 3] > 0, (i, f[2, 3].tolist())
    assert not itself[0].any() and not itself[1].any()


def case_ordering(torch, ctx):
    """on a non-default torch stream, nothing waited for: streaming with hvq_flush_next and a small ring -- the fields of batch k are
    queued beside batch k + 1 in flight, then later flushes rewrite the slots they read; a picture whose slot was reused is refused"""
    from hvqm4_amd._lib import HVQ_E_STATE, HvqError
    from hvqm4_amd.container import parse_header, video_pictures
    clip = _long_clip()
    hdr = parse_header(clip)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(clip)]
    yuv = _oracle("long640x480", clip, len(pics))
    side = torch.cuda.Stream()
    sid = ctx.open_stream(hdr.width, hdr.height, 2, 2, hdr.is15, 8)
    b = [pics[0:4], pics[4:8], pics[8:12]]
    sub = lambda part: ctx.submit_many_device([sid] * len(part), [ft for ft, _p in part], [p for _f, p in part])
    sub(b[0]); ctx.flush_begin()
    sub(b[1]); ctx.flush_next()                      # batch 0 ended, batch 1 in flight
    mem = torch.from_numpy(yuv[7].copy()).cuda()
    out = [torch.full((60, 80, 4), -1, dtype=torch.int32, device="cuda") for _ in range(3)]
    side.wait_stream(torch.cuda.current_stream())    # the outs and mem were filled on the current stream
    with torch.cuda.stream(side):
        got = ctx.picture_motion([sid] * 3, [1, 2, 3], [(sid, 0), (sid, 1), mem], block=8, radius=4, out=out)
    sub(b[2]); ctx.flush_next()                      # batch 1 ended, batch 2 in flight
    ctx.flush_end()                                  # batch 2 reconstructed into batch 0's slots
    torch.cuda.synchronize()
    for f, (k, j) in zip(got, ((1, 0), (2, 1), (3, 7))):
        _same(f, _want(("long640x480", k, j), yuv[k], yuv[j], hdr, 8, 4), ("flush_next", k, j))
    for kw in (dict(sids=[sid], ordinals=[0], ref=[(sid, 11)]), dict(sids=[sid], ordinals=[11], ref=[(sid, 1)])):
        try:
            ctx.picture_motion(block=8, radius=4, **kw)
        except HvqError as e:
            assert e.code == HVQ_E_STATE, (e, kw)
        else:
            raise AssertionError(("a picture whose slot was reused was not refused", kw))
    # a picture of the batch in flight as the reference: the call ends that batch itself
    sub(b[0]); ctx.flush_begin()
    got = ctx.picture_motion([sid], [11], [(sid, 12)], block=16, radius=4)
    torch.cuda.synchronize()
    _same(got[0], _want(("long640x480", 11, 0), yuv[11], yuv[0], hdr, 16, 4), "a reference of the batch in flight")
    ctx.close_stream(sid)


def case_refusals(torch, ctx):
    """each HVQ_E_ARG case of the specification (and the HVQ_E_STATE ones) leaves sentinel-filled fields untouched"""
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_STATE, HvqError, lib
    from hvqm4_amd.container import video_pictures
    from hvqm4_amd.metrics import HvqMetricsRef as Rf
    g = _golden()
    six = _six(ctx)
    sa, hdr, n, yuv = six["gop64x48_15"]
    sc = six["ragged24x40"][0]                                   # another size
    sb, _h, _n = _decode(ctx, g["yuv422_64x48"][0])              # the same size, another sampling
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(g["gop64x48_15"][0])]
    sd = ctx.open_stream(hdr.width, hdr.height, 2, 2, hdr.is15, 3)
    for ft, p in pics:
        ctx.submit(sd, ft, p)
    ctx.flush()                                                  # picture 0 of sd: its slot of the ring of 3 was reused
    last = len(pics) - 1
    out = torch.full((2, 6, 8, 4), SENTINEL, dtype=torch.int32, device="cuda")
    mem = torch.zeros(ctx.pic_bytes(sa) + 32, dtype=torch.uint8, device="cuda")
    p16 = mem.data_ptr() + (-mem.data_ptr()) % 16
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    o0, o1 = out[0].data_ptr(), out[1].data_ptr()

    def raw(sids, ords, refs, block=8, radius=15, dst=(o0, o1), count=None, handle=None, null_out=False):
        n_ = len(sids)
        a_r = C.cast((Rf * n_)(*[Rf(*r) for r in refs]), C.c_void_p) if refs is not None else None
        a_f = None if null_out else C.cast((C.c_void_p * n_)(*dst[:n_]), C.c_void_p)
        return lib().hvq_picture_motion(ctx._h if handle is None else handle[0], n_ if count is None else count, (C.c_int * n_)(*sids),
                                        (C.c_int * n_)(*ords), a_r, block, radius, a_f, stream)

    ok = [(sa, 1, None), (sa, 0, None)]
    two = dict(sids=[sa, sa], ords=[0, 1])
    arg = [("a NULL context", dict(two, refs=ok, handle=[None])),
           ("block 4", dict(two, refs=ok, block=4)), ("block 0", dict(two, refs=ok, block=0)), ("block 32", dict(two, refs=ok, block=32)),
           ("radius 16", dict(two, refs=ok, radius=16)), ("radius -1", dict(two, refs=ok, radius=-1)),
           ("without a ref", dict(two, refs=None)),
           ("against zeros", dict(two, refs=[ok[0], (-1, 0, None)])), ("against zeros, any ordinal", dict(two, refs=[ok[0], (-1, 5, None)])),
           ("another sampling", dict(two, refs=[ok[0], (sb, 1, None)])), ("another size", dict(two, refs=[ok[0], (sc, 1, None)])),
           ("ptr with stream >= 0", dict(two, refs=[ok[0], (sa, 0, p16)])), ("a misaligned reference", dict(two, refs=[ok[0], (-1, 0, p16 + 8)])),
           ("a bad reference stream", dict(two, refs=[ok[0], (99, 0, None)])), ("a bad reference ordinal", dict(two, refs=[ok[0], (sa, n, None)])),
           ("a reference stream below -1", dict(two, refs=[ok[0], (-2, 0, p16)])),
           ("a bad stream", dict(sids=[sa, 99], ords=[0, 0], refs=ok)), ("a bad ordinal", dict(sids=[sa, sa], ords=[0, 1000], refs=ok)),
           ("ordinal -1", dict(sids=[sa, sa], ords=[0, -1], refs=ok)),
           ("a null out", dict(two, refs=ok, null_out=True)), ("a null field", dict(two, refs=ok, dst=(o0, 0))),
           ("a misaligned field", dict(two, refs=ok, dst=(o0, o1 + 8))),
           ("n beyond the launch shape", dict(sids=[sa], ords=[0], refs=ok[:1], count=65536))]
    for what, kw in arg:
        assert raw(**kw) == HVQ_E_ARG, what
    assert raw([sd, sd], [last, 0], [(sd, last, None), (sd, last, None)]) == HVQ_E_STATE, "an evicted picture"
    assert raw([sd, sd], [last, last], [(sd, last, None), (sd, 0, None)]) == HVQ_E_STATE, "an evicted reference"
    assert raw([], [], None, count=0) == 0, "n == 0 is HVQ_OK"
    # through the Python layer: the library's refusals arrive as HvqError, the layer's own as ValueError
    outs = [out[0], out[1]]
    for code, kw in ((HVQ_E_ARG, dict(sids=[sa, sa], ordinals=[0, 1], ref=[(sa, 0), (sb, 1)])), (HVQ_E_ARG, dict(sids=[sa, sa], ordinals=[0, 1000], ref=[(sa, 0), (sa, 1)])),
                     (HVQ_E_STATE, dict(sids=[sd, sd], ordinals=[last, 0], ref=[(sd, last), (sd, last)])),
                     (HVQ_E_STATE, dict(sids=[sd, sd], ordinals=[last, last], ref=[(sd, last), (sd, 0)]))):
        try:
            ctx.picture_motion(block=8, radius=15, out=outs, **kw)
        except HvqError as e:
            assert e.code == code, (e, kw)
        else:
            raise AssertionError(("not refused", kw))
    short = mem[:ctx.pic_bytes(sa) - 16]
    for kw in (dict(ref=[(sa, 0), None]), dict(ref=[(sa, 0), mem[p16 - mem.data_ptr() + 8:][:ctx.pic_bytes(sa)]]), dict(ref=[(sa, 0), short]),
               dict(ref=None), dict(ref=[(sa, 0), (sa, 1)], radius=16), dict(ref=[(sa, 0), (sa, 1)], block=12)):
        try:
            ctx.picture_motion([sa, sa], [0, 1], out=outs, **dict(dict(block=8), **kw))
        except ValueError:
            pass
        else:
            raise AssertionError(("not refused by the Python layer", kw))
    torch.cuda.synchronize()
    assert out.eq(SENTINEL).all(), "a refused call wrote a field"
    # the well-formed call right after them works
    ctx.picture_motion([sa, sd], [1, last], [(sd, last), (sa, 0)], block=8, radius=15, out=outs)
    torch.cuda.synchronize()
    _same(out[0], _want(("gop64x48_15", 1, last), yuv[1], yuv[last], hdr, 8, 15), "after the refusals")
    _same(out[1], _want(("gop64x48_15", last, 0), yuv[last], yuv[0], hdr, 8, 15), "after the refusals, the ring of 3")
    for s in (sb, sd):
        ctx.close_stream(s)


CASES = ["goldens", "radii", "block16", "tiles", "planted", "ordering", "refusals"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "motion", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_motion(case, child_results):
    gpu_child.report(case, child_results)
