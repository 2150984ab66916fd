"""GPU: picture histograms (hvq_picture_histograms, Context.picture_histograms) against tests/histograms_ref.py on the oracle's pictures
and on caller memory of chosen content, compared with ==: the records are exact integers.  The cases run in ONE child process that
imports torch first (see tests/gpu_child.py); each test reports its case.  The child stops at the first HVQ_E_HIP or HIP error:
nothing more is started on a GPU that has reported a fault."""
import numpy as np
import pytest

from tests import gpu_child
from tests.gpu_kit import decode as _decode, golden_by_name as _golden, long_clip_data as _long_clip, oracle as _oracle

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300                                 # the cases take seconds each; a hung child is ended, not waited for
SENTINEL = 0x5A5A5A5A


# ------------------------------------------------------------------------------------------------------------- child side
def _want(a, b, geom):
    from tests.histograms_ref import histogram_reference
    return histogram_reference(a, b, *geom)


def _g(hdr):
    return hdr.width, hdr.height, hdr.h_samp, hdr.v_samp


def _same(got, wants, what):
    got = got.cpu().numpy()
    want = np.stack(wants) if len(wants) else np.zeros((0, 3, 256), dtype=np.int64)
    assert got.dtype == np.int32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} bins differ, first at (record, plane, bin) {tuple(bad[0])}: got {got[tuple(bad[0])]}, "
                             f"want {want[tuple(bad[0])]}")


def case_goldens(torch, ctx):
    """every golden clip: every picture's values, and its differences from its predecessor and from itself"""
    from tests.metrics_ref import plane_sizes
    samplings = set()
    for name, (data, hdr, n) in _golden().items():
        yuv = _oracle(name, data, n)
        sid, hdr, n = _decode(ctx, data)
        samplings.add((hdr.h_samp, hdr.v_samp))
        every = list(range(n))
        values = ctx.picture_histograms([sid] * n, every)
        prev = ctx.picture_histograms([sid] * (n - 1), every[1:], ref=[(sid, k - 1) for k in every[1:]]) if n > 1 else None
        self_ = ctx.picture_histograms([sid] * n, every, ref=[(sid, k) for k in every])
        torch.cuda.synchronize()
        _same(values, [_want(yuv[k], None, _g(hdr)) for k in every], (name, "values"))
        if prev is not None:
            _same(prev, [_want(yuv[k], yuv[k - 1], _g(hdr)) for k in every[1:]], (name, "against the predecessor"))
        _same(self_, [_want(yuv[k], yuv[k], _g(hdr)) for k in every], (name, "against itself"))
        sizes = torch.tensor(plane_sizes(*_g(hdr)), dtype=torch.int32, device="cuda")
        assert self_[:, :, 0].eq(sizes).all() and self_[:, :, 1:].eq(0).all(), (name, "a picture against itself lies in bin 0")
        ctx.close_stream(sid)
    assert {(2, 2), (2, 1), (1, 1)} <= samplings, samplings


def _size_with(units, chroma):
    """(width, height), multiples of 8, of a 4:2:0 picture whose Y plane (chroma: whose U plane) is exactly `units` 16-byte units"""
    target = units * 16 * (4 if chroma else 1)
    for w in range(8, 8193, 8):
        if target % w == 0 and (target // w) % 8 == 0 and 8 <= target // w <= 8192:
            return w, target // w
    raise AssertionError(f"no picture has a plane of {units} units")


def case_shapes(torch, ctx):
    """the smallest shapes at which the kernel takes another path, filled through src with random bytes and with the ramp i % 256, in both
    modes: 8 x 8 (chroma is ONE unit, its workgroup all but one lane predicated off), 128 x 128 (Y exactly one chunk of 1024 units), 136 x
    128 (one chunk and 64 units), and around k times the units one workgroup counts before it flushes, WORKGROUP_UNITS = HVQ_HG_CHUNK of
    hvq_desc.h, for k = 1 and k = 3: a Y plane of exactly that, a Y plane of that + 4 units (widths and heights are multiples of 8: a Y
    plane grows in steps of 4 units) and a chroma plane of that + 1 unit, whose last workgroup counts a single unit"""
    from hvqm4_amd.histograms import WORKGROUP_UNITS as WU
    assert WU == 1024 and 128 * 128 == WU * 16 and 136 * 128 == (WU + 64) * 16, "the kernel's chunk changed: choose the fixed shapes again"
    sizes = [(8, 8), (128, 128), (136, 128)]
    for k in (1, 3):
        sizes += [_size_with(k * WU, False), _size_with(k * WU + 4, False), _size_with(k * WU + 1, True)]
        assert sizes[-3][0] * sizes[-3][1] == k * WU * 16 and sizes[-1][0] * sizes[-1][1] // 4 == (k * WU + 1) * 16
    rng = np.random.default_rng(2026)
    sids, srcs, refs, hosts, geoms = [], [], [], [], []
    for w, h in sizes:
        sid = ctx.open_stream(w, h, 2, 2, True, 3)
        nb = ctx.pic_bytes(sid)
        assert nb == w * h * 3 // 2
        ramp = (np.arange(nb) % 256).astype(np.uint8)
        for a, b in ((rng.integers(0, 256, nb, dtype=np.uint8), rng.integers(0, 256, nb, dtype=np.uint8)), (ramp, ramp[::-1].copy()),
                     (ramp, rng.integers(0, 256, nb, dtype=np.uint8))):
            sids.append(sid); hosts.append((a, b)); geoms.append((w, h, 2, 2))
            srcs.append(torch.from_numpy(a).cuda()); refs.append(torch.from_numpy(b).cuda())
    n = len(sids)
    values = ctx.picture_histograms(sids, [-1] * n, src=srcs)
    diffs = ctx.picture_histograms(sids, [-1] * n, ref=refs, src=srcs)
    torch.cuda.synchronize()
    _same(values, [_want(a, None, g) for (a, _b), g in zip(hosts, geoms)], "values of the edge shapes")
    _same(diffs, [_want(a, b, g) for (a, b), g in zip(hosts, geoms)], "differences of the edge shapes")
    for sid in sorted(set(sids)):
        ctx.close_stream(sid)


def case_contention(torch, ctx):
    """640 x 480 pictures in which every lane of every wave adds into the same bin: constants 0, 255 and 128 (one bin holds 307200 for Y:
    a 16-bit counter anywhere would overflow), 255 against 0 (everything in bin 255), and two alternating values"""
    sid = ctx.open_stream(640, 480, 2, 2, True, 3)
    nb, g = ctx.pic_bytes(sid), (640, 480, 2, 2)
    alt = np.tile(np.array([0, 255], dtype=np.uint8), nb // 2)
    host = [np.full(nb, v, dtype=np.uint8) for v in (0, 255, 128)] + [alt]
    dev = [torch.from_numpy(a).cuda() for a in host]
    values = ctx.picture_histograms([sid] * 4, [-1] * 4, src=dev)
    pairs = [(1, 0), (0, 1), (3, 0), (3, 2), (2, 2)]
    diffs = ctx.picture_histograms([sid] * len(pairs), [-1] * len(pairs), ref=[dev[b] for _a, b in pairs], src=[dev[a] for a, _b in pairs])
    torch.cuda.synchronize()
    _same(values, [_want(a, None, g) for a in host], "constant and alternating pictures")
    _same(diffs, [_want(host[a], host[b], g) for a, b in pairs], "differences of constant and alternating pictures")
    v = values.cpu().numpy()
    assert v[0, 0, 0] == v[1, 0, 255] == v[2, 0, 128] == 307200 > 65535 and v[3, 0, 0] == v[3, 0, 255] == 153600
    d = diffs.cpu().numpy()
    assert d[0, :, 255].tolist() == d[1, :, 255].tolist() == [307200, 76800, 76800] and d[4, :, 0].tolist() == [307200, 76800, 76800]
    ctx.close_stream(sid)


def case_mixed_batch(torch, ctx):
    """one call over the pictures of all golden clips interleaved with src pictures, resident and pointer references interleaved; records
    in call order; out= reuse over a sentinel; n = 1 and n = 0; the same call twice gives the same bits; sum d h and sum d^2 h equal the
    sad and sse of picture_metrics on the same pairs, sum h the plane's samples"""
    from tests.metrics_ref import plane_sizes
    streams = []
    for name, (data, hdr, n) in _golden().items():
        sid, hdr, n = _decode(ctx, data)
        streams.append((name, sid, hdr, n, _oracle(name, data, n)))
    rng = np.random.default_rng(7)
    sids, ords, srcs, refs, mrefs, wants_v, wants_d, keep, mem_a = [], [], [], [], [], [], [], [], []
    i = 0
    for name, sid, hdr, n, yuv in streams:
        for k in range(n):
            other = (k + 1) % n
            if i % 4 == 3:                                     # a picture in the caller's memory
                a = rng.integers(0, 256, yuv[k].size, dtype=np.uint8)
                t = torch.from_numpy(a).cuda()
                keep.append(t)
                sids.append(sid); ords.append(-1); srcs.append(t); mem_a.append(len(sids) - 1)
            else:
                a = yuv[k]
                sids.append(sid); ords.append(k); srcs.append(None)
            if i % 2:                                          # a reference in the caller's memory
                t = torch.from_numpy(yuv[other].copy()).cuda()
                keep.append(t)
                refs.append(t)
            else:
                refs.append((sid, other))
            wants_v.append(_want(a, None, _g(hdr))); wants_d.append(_want(a, yuv[other], _g(hdr)))
            i += 1
    n = len(sids)
    values = ctx.picture_histograms(sids, ords, src=srcs)
    out = torch.full((n, 3, 256), SENTINEL, dtype=torch.int32, device="cuda")
    assert ctx.picture_histograms(sids, ords, ref=refs, src=srcs, out=out) is out
    again = ctx.picture_histograms(sids, ords, ref=refs, src=srcs)
    one = ctx.picture_histograms(sids[-1:], ords[-1:], ref=refs[-1:], src=srcs[-1:])
    none = ctx.picture_histograms([], [])
    none_d = ctx.picture_histograms([], [], ref=[])
    # picture_metrics takes resident pictures as a: the pairs whose a is resident
    res = [j for j in range(n) if j not in mem_a]
    met = ctx.picture_metrics([sids[j] for j in res], [ords[j] for j in res], [refs[j] for j in res])
    torch.cuda.synchronize()
    _same(values, wants_v, "mixed batch, values")
    _same(out, wants_d, "mixed batch, differences into a sentinel-filled out")
    _same(one, wants_d[-1:], "n = 1")
    assert tuple(none.shape) == tuple(none_d.shape) == (0, 3, 256) and none.dtype == torch.int32
    assert torch.equal(out, again), "the same call twice"
    assert mem_a and len(res) > len(mem_a) and len({(h.width, h.height, h.h_samp, h.v_samp) for _n, _s, h, _c, _y in streams}) >= 8
    d = torch.arange(256, dtype=torch.int64, device="cuda")
    h64 = out.to(torch.int64)
    assert torch.equal((h64 * d).sum(-1)[res], met[:, :, 2]) and torch.equal((h64 * d * d).sum(-1)[res], met[:, :, 3])
    assert torch.equal((values.to(torch.int64) * d).sum(-1)[res], met[:, :, 0])
    geom = {sid: _g(hdr) for _n, sid, hdr, _c, _y in streams}
    counts = torch.tensor([plane_sizes(*geom[s]) for s in sids], dtype=torch.int64, device="cuda")
    assert torch.equal(h64.sum(-1), counts) and torch.equal(values.to(torch.int64).sum(-1), counts)
    for _name, sid, _h, _n, _y in streams:
        ctx.close_stream(sid)


def case_ordering(torch, ctx):
    """on a non-default torch stream, nothing waited for: streaming with hvq_flush_next and a small ring -- histograms of batch k are
    queued beside batch k + 1 in flight, then later flushes rewrite the slots they read; a picture whose slot was reused is refused"""
    from hvqm4_amd._lib import HVQ_E_STATE, HvqError
    from hvqm4_amd.container import parse_header, video_pictures
    clip = _long_clip()
    hdr = parse_header(clip)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(clip)]
    yuv = _oracle("long640x480", clip, len(pics))
    g = _g(hdr)
    side = torch.cuda.Stream()
    sid = ctx.open_stream(hdr.width, hdr.height, 2, 2, hdr.is15, 8)
    b = [pics[0:4], pics[4:8], pics[8:12]]
    sub = lambda part: ctx.submit_many_device([sid] * len(part), [ft for ft, _p in part], [p for _f, p in part])
    sub(b[0]); ctx.flush_begin()
    sub(b[1]); ctx.flush_next()                      # batch 0 ended, batch 1 in flight
    mem = torch.from_numpy(yuv[7].copy()).cuda()
    out_v = torch.full((4, 3, 256), -1, dtype=torch.int32, device="cuda")
    out_d = torch.full((4, 3, 256), -1, dtype=torch.int32, device="cuda")
    side.wait_stream(torch.cuda.current_stream())    # the outs and mem were filled on the current stream
    with torch.cuda.stream(side):
        got_v = ctx.picture_histograms([sid] * 4, [0, 1, 2, 3], out=out_v)
        got_d = ctx.picture_histograms([sid] * 4, [0, 1, 2, 3], ref=[mem, (sid, 0), (sid, 1), (sid, 2)], out=out_d)
    sub(b[2]); ctx.flush_next()                      # batch 1 ended, batch 2 in flight
    ctx.flush_end()                                  # batch 2 reconstructed into batch 0's slots
    torch.cuda.synchronize()
    _same(got_v, [_want(yuv[k], None, g) for k in range(4)], "flush_next, values")
    _same(got_d, [_want(yuv[0], yuv[7], g)] + [_want(yuv[k], yuv[k - 1], g) for k in (1, 2, 3)], "flush_next, differences")
    for kw in (dict(sids=[sid], ordinals=[0]), dict(sids=[sid], ordinals=[11], ref=[(sid, 1)])):
        try:
            ctx.picture_histograms(**kw)
        except HvqError as e:
            assert e.code == HVQ_E_STATE, (e, kw)
        else:
            raise AssertionError(("a picture whose slot was reused was not refused", kw))
    # a picture of the batch in flight as the reference: the call ends that batch itself
    sub(b[0]); ctx.flush_begin()
    got = ctx.picture_histograms([sid], [11], ref=[(sid, 12)])
    torch.cuda.synchronize()
    _same(got, [_want(yuv[11], yuv[0], g)], "a reference of the batch in flight")
    ctx.close_stream(sid)


def case_refusals(torch, ctx):
    """each HVQ_E_ARG case of the specification (and the HVQ_E_STATE ones) leaves a sentinel-filled out untouched"""
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
    out = torch.full((2, 3, 256), SENTINEL, dtype=torch.int32, device="cuda")
    mem = torch.zeros(ctx.pic_bytes(sa) + 32, dtype=torch.uint8, device="cuda")
    p16 = mem.data_ptr() + (-mem.data_ptr()) % 16
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    V, D = 0, 1

    def raw(sids, ords, mode, refs=None, srcs=None, dst=None, count=None, handle=None):
        n_ = len(sids)
        a_r = C.cast((R * n_)(*[R(*r) for r in refs]), C.c_void_p) if refs is not None else None
        a_p = C.cast((C.c_void_p * n_)(*srcs), C.c_void_p) if srcs is not None else None
        return lib().hvq_picture_histograms(ctx._h if handle is None else handle[0], n_ if count is None else count, (C.c_int * n_)(*sids),
                                            (C.c_int * n_)(*ords), a_p, mode, a_r, C.c_void_p(out.data_ptr() if dst is None else dst), stream)

    ok = [(sa, 1, None), (sa, 0, None)]
    arg = [("a NULL context", dict(sids=[sa, sa], ords=[0, 1], mode=V, handle=[None])),
           ("a bad mode", dict(sids=[sa, sa], ords=[0, 1], mode=2)), ("a negative mode", dict(sids=[sa, sa], ords=[0, 1], mode=-1, refs=ok)),
           ("VALUES with a ref", dict(sids=[sa, sa], ords=[0, 1], mode=V, refs=ok)),
           ("ABSDIFF without a ref", dict(sids=[sa, sa], ords=[0, 1], mode=D)),
           ("ABSDIFF against zeros", dict(sids=[sa, sa], ords=[0, 1], mode=D, refs=[ok[0], (-1, 0, None)])),
           ("ABSDIFF against zeros, any ordinal", dict(sids=[sa, sa], ords=[0, 1], mode=D, refs=[ok[0], (-1, 5, None)])),
           ("another sampling", dict(sids=[sa, sa], ords=[0, 1], mode=D, refs=[ok[0], (sb, 1, None)])),
           ("another size", dict(sids=[sa, sa], ords=[0, 1], mode=D, refs=[ok[0], (sc, 1, None)])),
           ("ptr with stream >= 0", dict(sids=[sa, sa], ords=[0, 1], mode=D, refs=[ok[0], (sa, 0, p16)])),
           ("a misaligned reference", dict(sids=[sa, sa], ords=[0, 1], mode=D, refs=[ok[0], (-1, 0, p16 + 8)])),
           ("a bad reference stream", dict(sids=[sa, sa], ords=[0, 1], mode=D, refs=[ok[0], (99, 0, None)])),
           ("a bad reference ordinal", dict(sids=[sa, sa], ords=[0, 1], mode=D, refs=[ok[0], (sa, n, None)])),
           ("a reference stream below -1", dict(sids=[sa, sa], ords=[0, 1], mode=D, refs=[ok[0], (-2, 0, p16)])),
           ("a bad stream", dict(sids=[sa, 99], ords=[0, 0], mode=V)), ("a bad ordinal", dict(sids=[sa, sa], ords=[0, 1000], mode=V)),
           ("ordinal -1 without src", dict(sids=[sa, sa], ords=[0, -1], mode=V)),
           ("a misaligned src", dict(sids=[sa, sa], ords=[0, -1], mode=V, srcs=[None, p16 + 8])),
           ("a src with an ordinal", dict(sids=[sa, sa], ords=[0, 1], mode=V, srcs=[None, p16])),
           ("a src with a bad stream", dict(sids=[sa, 99], ords=[0, -1], mode=V, srcs=[None, p16])),
           ("a null out", dict(sids=[sa, sa], ords=[0, 1], mode=V, dst=0)),
           ("a misaligned out", dict(sids=[sa, sa], ords=[0, 1], mode=V, dst=out.data_ptr() + 2)),
           ("n beyond the launch shape", dict(sids=[sa], ords=[0], mode=V, count=65536))]
    for what, kw in arg:
        assert raw(**kw) == HVQ_E_ARG, what
    assert raw([sd, sd], [last, 0], V) == HVQ_E_STATE, "an evicted picture"
    assert raw([sd, sd], [last, last], D, refs=[(sd, last, None), (sd, 0, None)]) == HVQ_E_STATE, "an evicted reference"
    assert raw([], [], V, count=0) == 0 and raw([], [], D, count=0) == 0, "n == 0 is HVQ_OK"
    # through the Python layer: the library's refusals arrive as HvqError, the layer's own as ValueError
    for code, kw in ((HVQ_E_ARG, dict(sids=[sa, sa], ordinals=[0, 1], ref=[(sa, 0), (sb, 1)])), (HVQ_E_ARG, dict(sids=[sa, sa], ordinals=[0, 1000])),
                     (HVQ_E_STATE, dict(sids=[sd, sd], ordinals=[last, 0])), (HVQ_E_STATE, dict(sids=[sd, sd], ordinals=[last, last], ref=[(sd, last), (sd, 0)]))):
        try:
            ctx.picture_histograms(out=out, **kw)
        except HvqError as e:
            assert e.code == code, (e, kw)
        else:
            raise AssertionError(("not refused", kw))
    short = mem[:ctx.pic_bytes(sa) - 16]
    for kw in (dict(ref=[(sa, 0), None]), dict(ref=[(sa, 0), mem[p16 - mem.data_ptr() + 8:][:ctx.pic_bytes(sa)]]), dict(ref=[(sa, 0), short]),
               dict(src=[None, short])):
        try:
            ctx.picture_histograms([sa, sa], [0, -1 if "src" in kw else 1], out=out, **kw)
        except ValueError:
            pass
        else:
            raise AssertionError(("not refused by the Python layer", kw))
    torch.cuda.synchronize()
    assert out.eq(SENTINEL).all(), "a refused call wrote its output"
    # the well-formed calls right after them work
    yuv = _oracle("gop64x48_15", *g["gop64x48_15"][0::2])
    ctx.picture_histograms([sa, sd], [1, last], out=out)
    torch.cuda.synchronize()
    _same(out, [_want(yuv[1], None, _g(hdr)), _want(yuv[last], None, _g(hdr))], "values after the refusals")
    ctx.picture_histograms([sa, sd], [1, last], ref=[(sd, last), (sa, 0)], out=out)
    torch.cuda.synchronize()
    _same(out, [_want(yuv[1], yuv[last], _g(hdr)), _want(yuv[last], yuv[0], _g(hdr))], "differences after the refusals")
    for s in (sa, sb, sc, sd):
        ctx.close_stream(s)


CASES = ["goldens", "shapes", "contention", "mixed_batch", "ordering", "refusals"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "histograms", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_histograms(case, child_results):
    gpu_child.report(case, child_results)
