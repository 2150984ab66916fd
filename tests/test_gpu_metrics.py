"""GPU: picture metrics (hvq_picture_metrics, Context.picture_metrics) against tests/metrics_ref.py on the oracle's pictures, compared
with ==: the records are exact integers.  The cases run in ONE child process that imports torch first (see tests/gpu_child.py);
each test reports its case.  The child stops at the first HVQ_E_HIP or HIP error: nothing more is started on a GPU that has reported
a fault."""
import numpy as np
import pytest

from tests import gpu_child
from tests.gpu_kit import decode as _decode, golden_by_name as _golden, long_clip_data as _long_clip, oracle as _oracle, synth as _synth

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300                                 # the cases take seconds each; a hung child is ended, not waited for
SENTINEL = 0x5A5A5A5A5A5A5A5A


# ------------------------------------------------------------------------------------------------------------- child side
def _want(a, b, hdr):
    from tests.metrics_ref import metrics_reference
    return metrics_reference(a, b, hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)


def _same(got, wants, what):
    got = got.cpu().numpy()
    want = np.stack(wants) if len(wants) else np.zeros((0, 3, 4), dtype=np.int64)
    assert got.dtype == np.int64 and got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, "
                             f"want {want[tuple(bad[0])]}")


def case_goldens(torch, ctx):
    """every golden clip: every picture against its predecessor, against itself and against zeros; ref=None"""
    samplings = set()
    for name, (data, hdr, n) in _golden().items():
        yuv = _oracle(name, data, n)
        sid, hdr, n = _decode(ctx, data)
        samplings.add((hdr.h_samp, hdr.v_samp))
        sids, ords, refs, wants = [], [], [], []
        for k in range(n):
            forms = [((sid, k), yuv[k]), (None, None)] + ([((sid, k - 1), yuv[k - 1])] if k else [])
            for ref, b in forms:
                sids.append(sid); ords.append(k); refs.append(ref); wants.append(_want(yuv[k], b, hdr))
        got = ctx.picture_metrics(sids, ords, refs)
        zeros = ctx.picture_metrics([sid] * n, list(range(n)))
        torch.cuda.synchronize()
        _same(got, wants, name)
        _same(zeros, [_want(yuv[k], None, hdr) for k in range(n)], (name, "ref=None"))
        for k in range(n):                                     # a picture against itself
            assert got[3 * k - (1 if k else 0) + 0, :, 2:].eq(0).all(), (name, k)
        ctx.close_stream(sid)
    assert {(2, 2), (2, 1), (1, 1)} <= samplings, samplings


def case_mixed_batch(torch, ctx):
    """one call over the pictures of all golden clips, the three forms of reference interleaved; records in call order; n = 1"""
    streams = []
    for name, (data, hdr, n) in _golden().items():
        sid, hdr, n = _decode(ctx, data)
        streams.append((name, sid, hdr, n, _oracle(name, data, n)))
    sids, ords, refs, wants, keep = [], [], [], [], []
    i = 0
    for name, sid, hdr, n, yuv in streams:
        for k in range(n):
            form = i % 3
            other = (k + 1) % n
            if form == 0:
                ref, b = (sid, other), yuv[other]
            elif form == 1:
                ref, b = None, None
            else:
                ref = torch.from_numpy(ctx.read_pictures([sid], [other])[0]).cuda()
                keep.append(ref)
                b = yuv[other]
            sids.append(sid); ords.append(k); refs.append(ref); wants.append(_want(yuv[k], b, hdr))
            i += 1
    got = ctx.picture_metrics(sids, ords, refs)
    one = ctx.picture_metrics(sids[-1:], ords[-1:], refs[-1:])
    none = ctx.picture_metrics([], [])
    torch.cuda.synchronize()
    _same(got, wants, "mixed batch")
    _same(one, wants[-1:], "n = 1")
    assert tuple(none.shape) == (0, 3, 4)
    assert len({(h.width, h.height, h.h_samp, h.v_samp) for _n, _s, h, _c, _y in streams}) >= 8
    for _name, sid, _h, _n, _y in streams:
        ctx.close_stream(sid)


def case_cross_stream(torch, ctx):
    """the same clip decoded into two streams: sad = sse = 0 across them; two different clips of one geometry against the reference"""
    g = _golden()
    data, hdr, n = g["yuv422_64x48"]
    yuv = _oracle("yuv422_64x48", data, n)
    s0, hdr, n = _decode(ctx, data)
    s1, _h, _n = _decode(ctx, data)
    got = ctx.picture_metrics([s0] * n, list(range(n)), [(s1, k) for k in range(n)])
    torch.cuda.synchronize()
    _same(got, [_want(yuv[k], yuv[k], hdr) for k in range(n)], "one clip, two streams")
    assert got[:, :, 2:].eq(0).all() and got[:, :, 0].eq(got[:, :, 1]).all() and got[:, :, 0].gt(0).all()
    ctx.close_stream(s0); ctx.close_stream(s1)
    by_geom = {}
    for name, (data, hdr, n) in g.items():
        by_geom.setdefault((hdr.width, hdr.height, hdr.h_samp, hdr.v_samp), []).append(name)
    pairs = [v for v in by_geom.values() if len(v) >= 2]
    assert pairs, "no two golden clips share a geometry"
    checked = 0
    for names in pairs[:3]:
        na, nb = names[0], names[1]
        ya, yb = _oracle(na, *g[na][0::2]), _oracle(nb, *g[nb][0::2])
        sa, hdr, ca = _decode(ctx, g[na][0])
        sb, _h, cb = _decode(ctx, g[nb][0])
        m = min(ca, cb)
        got = ctx.picture_metrics([sa] * m, list(range(m)), [(sb, k) for k in range(m)])
        torch.cuda.synchronize()
        _same(got, [_want(ya[k], yb[k], hdr) for k in range(m)], (na, nb))
        checked += int(got[:, :, 3].sum().item() > 0)
        ctx.close_stream(sa); ctx.close_stream(sb)
    assert checked, "every pair of clips of one geometry decoded to the same pictures"


def case_caller_memory(torch, ctx):
    from hvqm4_amd.container import parse_header
    from tests.metrics_ref import adversarial_reference
    # a tensor built from read_pictures, and the same bytes 16 bytes into a larger allocation
    data, hdr, n = _golden()["wide296x160"]
    yuv = _oracle("wide296x160", data, n)
    sid, hdr, n = _decode(ctx, data)
    host = ctx.read_pictures([sid] * n, list(range(n)))
    assert np.array_equal(host, yuv)
    flat = [torch.from_numpy(host[(k + 1) % n]).cuda() for k in range(n)]
    pb = host.shape[1]
    room = torch.zeros(n * (pb + 64) + 64, dtype=torch.uint8, device="cuda")
    base = (-room.data_ptr()) % 16 + 16                       # 16 bytes past a 16-byte boundary of the allocation
    inside = []
    for k in range(n):
        view = room[base + k * (pb + 48):base + k * (pb + 48) + pb]
        assert view.data_ptr() % 16 == 0
        view.copy_(flat[k])
        inside.append(view)
    got = ctx.picture_metrics([sid] * n, list(range(n)), flat)
    got_in = ctx.picture_metrics([sid] * n, list(range(n)), inside)
    torch.cuda.synchronize()
    wants = [_want(yuv[k], yuv[(k + 1) % n], hdr) for k in range(n)]
    _same(got, wants, "a tensor per reference")
    _same(got_in, wants, "references inside a larger allocation")
    ctx.close_stream(sid)
    # 640 x 480, every difference at least 128: the luma sse does not fit 32 bits
    clip = _long_clip()
    hdr = parse_header(clip)
    yuv = _oracle("long640x480", clip, 12)
    sid, hdr, n = _decode(ctx, clip)
    adv = [adversarial_reference(yuv[k]) for k in (0, 5)]
    got = ctx.picture_metrics([sid, sid], [0, 5], [torch.from_numpy(a).cuda() for a in adv])
    torch.cuda.synchronize()
    wants = [_want(yuv[k], a, hdr) for k, a in zip((0, 5), adv)]
    assert all(w[0, 3] > 2 ** 32 and w[0, 3] >= 640 * 480 * 128 * 128 for w in wants)
    _same(got, wants, "adversarial 640x480")
    ctx.close_stream(sid)
    # 1280 x 64: rows wider than a workgroup's reach
    wide = _synth(1280, 64, "IP", 77)
    yuv = _oracle("wide1280x64", wide, 2)
    sid, hdr, n = _decode(ctx, wide)
    assert (hdr.width, hdr.height, n) == (1280, 64, 2)
    ref = [torch.from_numpy(yuv[0].copy()).cuda(), (sid, 0), None]
    got = ctx.picture_metrics([sid] * 3, [1, 1, 1], ref)
    torch.cuda.synchronize()
    _same(got, [_want(yuv[1], yuv[0], hdr), _want(yuv[1], yuv[0], hdr), _want(yuv[1], None, hdr)], "1280x64")
    ctx.close_stream(sid)


def case_overwrite_and_determinism(torch, ctx):
    """out full of 0xFF bytes is replaced whole; the same call twice into two buffers: identical bits"""
    clip = _long_clip()
    yuv = _oracle("long640x480", clip, 12)
    sid, hdr, n = _decode(ctx, clip)
    sids, ords = [sid] * (2 * n), list(range(n)) * 2
    refs = [(sid, (k + 1) % n) for k in range(n)] + [None] * n
    first = torch.full((2 * n, 3, 4), -1, dtype=torch.int64, device="cuda")                 # every byte 0xFF
    second = torch.full((2 * n, 3, 4), -1, dtype=torch.int64, device="cuda")
    assert ctx.picture_metrics(sids, ords, refs, out=first) is first
    ctx.picture_metrics(sids, ords, refs, out=second)
    torch.cuda.synchronize()
    _same(first, [_want(yuv[k], yuv[(k + 1) % n], hdr) for k in range(n)] + [_want(yuv[k], None, hdr) for k in range(n)], "overwrite")
    assert torch.equal(first, second)
    ctx.close_stream(sid)


def case_refusals(torch, ctx):
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_STATE, HvqError, lib
    from hvqm4_amd.container import video_pictures
    from hvqm4_amd.metrics import HvqMetricsRef as R
    g = _golden()
    sa, hdr, n = _decode(ctx, g["gop64x48_15"][0])
    sb, _h, _n = _decode(ctx, g["yuv422_64x48"][0])              # the same size, another sampling
    sc, _h, _n = _decode(ctx, g["ragged24x40"][0])               # another size
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(g["gop64x48_15"][0])]
    sd = ctx.open_stream(hdr.width, hdr.height, 2, 2, hdr.is15, 3)
    for ft, p in pics:
        ctx.submit(sd, ft, p)
    ctx.flush()                                                  # picture 0 of sd: its slot of the ring of 3 was reused
    last = len(pics) - 1
    out = torch.full((2, 3, 4), SENTINEL, dtype=torch.int64, device="cuda")
    mem = torch.zeros(ctx.pic_bytes(sa) + 32, dtype=torch.uint8, device="cuda")
    p16 = mem.data_ptr() + (-mem.data_ptr()) % 16
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(sids, ords, refs, dst=None, count=None):
        n_ = len(sids)
        a_r = C.cast((R * n_)(*[R(*r) for r in refs]), C.c_void_p) if refs is not None else None
        return lib().hvq_picture_metrics(ctx._h, n_ if count is None else count, (C.c_int * n_)(*sids), (C.c_int * n_)(*ords), a_r,
                                         C.c_void_p(out.data_ptr() if dst is None else dst), stream)

    Z = (-1, 0, None)
    arg = [("another sampling", [sa, sa], [0, 1], [Z, (sb, 1, None)]), ("another size", [sa, sa], [0, 1], [Z, (sc, 1, None)]),
           ("ptr with stream >= 0", [sa, sa], [0, 1], [Z, (sa, 0, p16)]), ("misaligned ptr", [sa, sa], [0, 1], [Z, (-1, 0, p16 + 8)]),
           ("bad stream", [sa, 99], [0, 0], None), ("bad ordinal", [sa, sa], [0, 1000], None), ("negative ordinal", [sa, sa], [0, -1], None),
           ("bad reference stream", [sa, sa], [0, 1], [Z, (99, 0, None)]), ("bad reference ordinal", [sa, sa], [0, 1], [Z, (sa, n, None)]),
           ("reference stream below -1", [sa, sa], [0, 1], [Z, (-2, 0, None)])]
    for what, sids, ords, refs in arg:
        assert raw(sids, ords, refs) == HVQ_E_ARG, what
    assert raw([sa, sa], [0, 1], None, dst=0) == HVQ_E_ARG, "null out"
    assert raw([sa, sa], [0, 1], None, dst=out.data_ptr() + 4) == HVQ_E_ARG, "misaligned out"
    assert raw([sa], [0], None, count=65536) == HVQ_E_ARG, "n beyond the launch shape"
    assert raw([sd, sd], [last, 0], None) == HVQ_E_STATE, "an evicted picture"
    assert raw([sd, sd], [last, last], [Z, (sd, 0, None)]) == HVQ_E_STATE, "an evicted reference"
    # through the Python layer: the library's refusals arrive as HvqError, the layer's own as ValueError
    for code, sids, ords, refs in ((HVQ_E_ARG, [sa, sa], [0, 1], [None, (sb, 1)]), (HVQ_E_ARG, [sa, sa], [0, 1000], None),
                                   (HVQ_E_STATE, [sd, sd], [last, 0], None), (HVQ_E_STATE, [sd, sd], [last, last], [None, (sd, 0)])):
        try:
            ctx.picture_metrics(sids, ords, refs, out=out)
        except HvqError as e:
            assert e.code == code, (e, sids, ords, refs)
        else:
            raise AssertionError(("not refused", sids, ords, refs))
    for refs in ([None, mem[p16 - mem.data_ptr() + 8:][:ctx.pic_bytes(sa)]], [None, mem[:ctx.pic_bytes(sa) - 16]]):
        try:
            ctx.picture_metrics([sa, sa], [0, 1], refs, out=out)
        except ValueError:
            pass
        else:
            raise AssertionError("a misaligned or short reference tensor was not refused")
    torch.cuda.synchronize()
    assert out.eq(SENTINEL).all(), "a refused call wrote its output"
    # the well-formed call right after them works
    ctx.picture_metrics([sa, sd], [1, last], [(sa, 0), None], out=out)
    torch.cuda.synchronize()
    yuv = _oracle("gop64x48_15", *g["gop64x48_15"][0::2])
    _same(out, [_want(yuv[1], yuv[0], hdr), _want(yuv[last], None, hdr)], "after the refusals")
    for s in (sa, sb, sc, sd):
        ctx.close_stream(s)


def case_ordering(torch, ctx):
    """on a non-default torch stream, nothing waited for: a call, then flushes that rewrite every slot it reads (the pattern of the
    slot-safety case of tests/test_gpu_export.py); then streaming: hvq_flush_next, metrics of batch k beside batch k + 1 in flight"""
    from hvqm4_amd.container import parse_header, video_pictures
    clip = _long_clip()
    hdr = parse_header(clip)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(clip)]
    yuv = _oracle("long640x480", clip, len(pics))
    w, h = hdr.width, hdr.height
    side = torch.cuda.Stream()
    sid = ctx.open_stream(w, h, 2, 2, hdr.is15, 3)
    for ft, p in pics[:3]:
        ctx.submit(sid, ft, p)
    ctx.flush()
    mem = torch.from_numpy(yuv[7].copy()).cuda()
    out = torch.full((4, 3, 4), -1, dtype=torch.int64, device="cuda")
    side.wait_stream(torch.cuda.current_stream())    # out and mem were filled on the current stream
    with torch.cuda.stream(side):
        got = ctx.picture_metrics([sid] * 4, [1, 2, 0, 2], [(sid, 0), (sid, 1), None, mem], out=out)
    for ft, p in pics[3:9]:
        ctx.submit(sid, ft, p)
    ctx.flush()                                      # rewrites every slot of the ring of 3
    ctx.replay(1)
    torch.cuda.synchronize()
    _same(got, [_want(yuv[1], yuv[0], hdr), _want(yuv[2], yuv[1], hdr), _want(yuv[0], None, hdr), _want(yuv[2], yuv[7], hdr)], "flush behind the call")
    ctx.close_stream(sid)
    # streaming: batch k measured while batch k + 1 is in flight; batch k + 2 reuses batch k's slots
    sid = ctx.open_stream(w, h, 2, 2, hdr.is15, 8)
    b = [pics[0:4], pics[4:8], pics[8:12]]
    sub = lambda part: ctx.submit_many_device([sid] * len(part), [ft for ft, _p in part], [p for _f, p in part])
    sub(b[0]); ctx.flush_begin()
    sub(b[1]); ctx.flush_next()                      # batch 0 ended, batch 1 in flight
    out = torch.full((4, 3, 4), -1, dtype=torch.int64, device="cuda")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ctx.picture_metrics([sid] * 4, [0, 1, 2, 3], [None, (sid, 0), (sid, 1), (sid, 2)], out=out)
    sub(b[2]); ctx.flush_next()                      # batch 1 ended, batch 2 in flight
    ctx.flush_end()                                  # batch 2 reconstructed into batch 0's slots
    torch.cuda.synchronize()
    _same(got, [_want(yuv[0], None, hdr)] + [_want(yuv[k], yuv[k - 1], hdr) for k in (1, 2, 3)], "flush_next")
    # a picture of the batch in flight as the reference: the call ends that batch itself
    sub(b[0]); ctx.flush_begin()
    got = ctx.picture_metrics([sid], [11], [(sid, 12)])
    torch.cuda.synchronize()
    _same(got, [_want(yuv[11], yuv[0], hdr)], "a reference of the batch in flight")
    for k in range(8, 12):
        assert np.array_equal(ctx.read_picture(sid, k), yuv[k]), k
    ctx.close_stream(sid)


CASES = ["goldens", "mixed_batch", "cross_stream", "caller_memory", "overwrite_and_determinism", "refusals", "ordering"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "metrics", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_metrics(case, child_results):
    gpu_child.report(case, child_results)
