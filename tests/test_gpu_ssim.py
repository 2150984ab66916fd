"""GPU: windowed SSIM (hvq_picture_ssim, Context.picture_ssim) against tests/ssim_ref.py on the oracle's pictures, records and maps
compared with == on the raw bits.  The cases run in ONE child process that imports torch first (see tests/gpu_child.py); each
test reports its case.  The child stops at the first HVQ_E_HIP or HIP error: nothing more is started on a GPU that has reported a
fault."""
import numpy as np
import pytest

from tests import gpu_child
from tests.gpu_kit import decode as _decode, golden_by_name as _golden, long_clip_data as _long_clip, oracle as _oracle, synth as _synth

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300                                 # the cases take seconds each; a hung child is ended, not waited for
SENTINEL = 0x5A5A5A5A5A5A5A5A
GUARD = 64                                          # sentinel floats behind a map


# ------------------------------------------------------------------------------------------------------------- child side
_cache = {}


def _want(a, b, hdr, key=None):
    """(record, flat map bits) of the reference; computed once per key"""
    from tests.ssim_ref import flat_maps, ssim_reference
    if key is not None and ("want", key) in _cache:
        return _cache["want", key]
    rec, maps = ssim_reference(a, b, hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)
    res = (rec, flat_maps(maps).view(np.uint32))
    if key is not None:
        _cache["want", key] = res
    return res


def _same(got, maps, wants, what):
    """got: int64 [n, 3, 2]; maps: None or a list of (None | triple of tensors); wants: list of (record, flat map bits)"""
    got = got.cpu().numpy()
    want = np.stack([w[0] for w in wants]) if len(wants) else np.zeros((0, 3, 2), dtype=np.int64)
    assert got.dtype == np.int64 and got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} record values differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, "
                             f"want {want[tuple(bad[0])]}")
    for i, tri in enumerate(maps or []):
        if tri is None:
            continue
        flat = np.concatenate([t.cpu().numpy().reshape(-1) for t in tri]).view(np.uint32)
        assert flat.shape == wants[i][1].shape, (what, i, flat.shape, wants[i][1].shape)
        if not np.array_equal(flat, wants[i][1]):
            bad = np.flatnonzero(flat != wants[i][1])
            raise AssertionError(f"{what}: pair {i}: {len(bad)} of {flat.size} map elements differ, first at {bad[0]}: got {flat[bad[0]]:#x}, "
                                 f"want {wants[i][1][bad[0]]:#x}")


def case_goldens(torch, ctx):
    """every golden clip: every picture against its predecessor, against itself and against 255 - picture in caller memory"""
    from tests.ssim_ref import SSIM_ONE
    samplings, smallest = set(), set()
    for name, (data, hdr, n) in _golden().items():
        yuv = _oracle(name, data, n)
        sid, hdr, n = _decode(ctx, data)
        samplings.add((hdr.h_samp, hdr.v_samp))
        sids, ords, refs, wants, selfs = [], [], [], [], []
        for k in range(n):
            inv = 255 - yuv[k]
            forms = [((sid, k), yuv[k], "self"), (torch.from_numpy(inv).cuda(), inv, "inv")] + ([((sid, k - 1), yuv[k - 1], "prev")] if k else [])
            for ref, b, form in forms:
                if form == "self":
                    selfs.append(len(sids))
                sids.append(sid); ords.append(k); refs.append(ref); wants.append(_want(yuv[k], b, hdr, (name, k, form)))
        got, maps = ctx.picture_ssim(sids, ords, refs, maps=True)
        plain = ctx.picture_ssim(sids, ords, refs)
        torch.cuda.synchronize()
        _same(got, maps, wants, name)
        _same(plain, None, wants, (name, "without maps"))
        for i in selfs:                                        # a picture against itself
            assert got[i, :, 0].eq(got[i, :, 1] << 24).all() and got[i, 0, 1].item() > 0, (name, i)
            assert all(t.eq(1.0).all() for t in maps[i]), (name, i)
        if name in ("ip8", "i16"):
            smallest.add(name)
            assert got[0, :, 1].tolist() == ([1, 0, 0] if name == "ip8" else [9, 1, 1]), (name, got[0])
            assert got[0, 0, 0].item() == got[0, 0, 1].item() * SSIM_ONE
        ctx.close_stream(sid)
    assert {(2, 2), (2, 1), (1, 1)} <= samplings, samplings
    assert smallest == {"ip8", "i16"}


def case_mixed_batch(torch, ctx):
    """one call over the pictures of all golden clips, the two forms of reference interleaved, a map for every other pair; n = 1; n = 0"""
    import ctypes as C
    from hvqm4_amd._lib import check, lib
    from hvqm4_amd.metrics import HvqMetricsRef as R
    streams = []
    for name, (data, hdr, n) in _golden().items():
        sid, hdr, n = _decode(ctx, data)
        streams.append((name, sid, hdr, n, _oracle(name, data, n)))
    sids, ords, refs, wants, keep = [], [], [], [], []
    for name, sid, hdr, n, yuv in streams:
        for k in range(n):
            other = (k + 1) % n
            if len(sids) % 2 == 0:
                ref = (sid, other)
            else:
                ref = torch.from_numpy(yuv[other].copy()).cuda()
                keep.append(ref)
            sids.append(sid); ords.append(k); refs.append(ref); wants.append(_want(yuv[k], yuv[other], hdr))
    n = len(sids)
    # through the C entry point: a map for every other pair and NULL for the rest
    out = torch.full((n, 3, 2), -1, dtype=torch.int64, device="cuda")
    bufs = [torch.full((len(w[1]),), float("nan"), dtype=torch.float32, device="cuda") if i % 2 else None for i, w in enumerate(wants)]
    a_r = (R * n)(*[R(r[0], r[1], None) if isinstance(r, tuple) else R(-1, 0, r.data_ptr()) for r in refs])
    a_m = (C.c_void_p * n)(*[b.data_ptr() if b is not None else None for b in bufs])
    check(lib().hvq_picture_ssim(ctx._h, n, (C.c_int * n)(*sids), (C.c_int * n)(*ords), C.cast(a_r, C.c_void_p), C.c_void_p(out.data_ptr()),
                                 C.cast(a_m, C.c_void_p), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    allmaps, maps = ctx.picture_ssim(sids, ords, refs, maps=True)
    one = ctx.picture_ssim(sids[-1:], ords[-1:], refs[-1:])
    none, nomaps = ctx.picture_ssim([], [], [], maps=True)
    torch.cuda.synchronize()
    _same(out, [(b,) if b is not None else None for b in bufs], wants, "mixed batch, every other pair with a map")
    _same(allmaps, maps, wants, "mixed batch")
    _same(one, None, wants[-1:], "n = 1")
    assert tuple(none.shape) == (0, 3, 2) and none.dtype == torch.int64 and nomaps == []
    assert len({(h.width, h.height, h.h_samp, h.v_samp) for _n, _s, h, _c, _y in streams}) >= 8
    for (_name, sid, hdr, _n, _y), tri in zip(streams[:1], maps[:1]):
        from hvqm4_amd.metrics import ssim_windows
        assert tuple(tuple(t.shape) for t in tri) == ssim_windows(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)
    for _name, sid, _h, _n, _y in streams:
        ctx.close_stream(sid)


def case_tile_edges(torch, ctx):
    """the smallest shapes that cross every tile boundary, each against its decoded predecessor and against caller memory holding a copy,
    the adversarial picture, all 255, all 0 and a checkerboard"""
    from tests.metrics_ref import adversarial_reference
    from tests.ssim_ref import checkerboard, window_dims
    data, hdr, n = _golden()["wide296x160"]
    clips = [("wide296x160", data, n, ((39, 73), (19, 36), (19, 36))),
             ("wide1280x64", _synth(1280, 64, "IP", 77), 2, ((15, 319), (7, 159), (7, 159))),
             ("long640x480", _long_clip(), 12, ((119, 159), (59, 79), (59, 79)))]
    for name, clip, n, dims in clips:
        yuv = _oracle(name, clip, n)
        sid, hdr, n = _decode(ctx, clip)
        assert window_dims(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp) == dims, (name, dims)
        k = n - 1
        a = yuv[k]
        mem = {"copy": a.copy(), "adversarial": adversarial_reference(a), "all255": np.full_like(a, 255), "all0": np.zeros_like(a),
               "checkerboard": checkerboard(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)}
        sids, ords, refs, wants = [sid], [k], [(sid, k - 1)], [_want(a, yuv[k - 1], hdr)]
        for form, b in mem.items():
            sids.append(sid); ords.append(k); refs.append(torch.from_numpy(b).cuda()); wants.append(_want(a, b, hdr))
        got, maps = ctx.picture_ssim(sids, ords, refs, maps=True)
        torch.cuda.synchronize()
        _same(got, maps, wants, name)
        assert got[:, :, 1].eq(torch.tensor([r * c for r, c in dims], device="cuda")).all(), (name, got[:, :, 1])
        assert got[1, :, 0].eq(got[1, :, 1] << 24).all(), (name, "a copy")
        ctx.close_stream(sid)


def case_overwrite_and_determinism(torch, ctx):
    """out and maps full of 0xFF bytes are replaced whole, the sentinels behind each map stay; the same call twice: identical bits"""
    from hvqm4_amd.metrics import HvqMetricsRef as R
    import ctypes as C
    from hvqm4_amd._lib import check, lib
    clip = _long_clip()
    yuv = _oracle("long640x480", clip, 12)
    sid, hdr, n = _decode(ctx, clip)
    sids, ords = [sid] * n, list(range(n))
    refs = [(sid, (k + 1) % n) for k in range(n)]
    wants = [_want(yuv[k], yuv[(k + 1) % n], hdr) for k in range(n)]
    nwin = len(wants[0][1])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    results = []
    for _round in range(2):
        out = torch.full((n, 3, 2), -1, dtype=torch.int64, device="cuda")                    # every byte 0xFF
        bufs = [torch.full((nwin + GUARD,), -1, dtype=torch.int32, device="cuda") for _k in range(n)]
        for b in bufs:
            b[nwin:] = 0x5A5A5A5A
        a_r = (R * n)(*[R(s, o, None) for s, o in refs])
        a_m = (C.c_void_p * n)(*[b.data_ptr() for b in bufs])
        check(lib().hvq_picture_ssim(ctx._h, n, (C.c_int * n)(*sids), (C.c_int * n)(*ords), C.cast(a_r, C.c_void_p), C.c_void_p(out.data_ptr()),
                                     C.cast(a_m, C.c_void_p), stream))
        results.append((out, bufs))
    torch.cuda.synchronize()
    for out, bufs in results:
        _same(out, [(b[:nwin].view(torch.float32),) for b in bufs], wants, "overwrite")
        assert all(b[nwin:].eq(0x5A5A5A5A).all() for b in bufs), "the call wrote behind a map"
    assert torch.equal(results[0][0], results[1][0])
    assert all(torch.equal(x, y) for x, y in zip(results[0][1], results[1][1]))
    given = torch.full((n, 3, 2), -1, dtype=torch.int64, device="cuda")
    assert ctx.picture_ssim(sids, ords, refs, out=given) is given
    torch.cuda.synchronize()
    assert torch.equal(given, results[0][0])
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
    yuv = _oracle("gop64x48_15", *g["gop64x48_15"][0::2])
    nwin = len(_want(yuv[1], yuv[0], hdr)[1])
    out = torch.full((2, 3, 2), SENTINEL, dtype=torch.int64, device="cuda")
    mapbuf = [torch.full((nwin + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _i in range(2)]
    mem = torch.zeros(ctx.pic_bytes(sa) + 32, dtype=torch.uint8, device="cuda")
    p16 = mem.data_ptr() + (-mem.data_ptr()) % 16
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(sids, ords, refs, dst=None, count=None, maps="good"):
        n_ = len(sids)
        a_r = C.cast((R * n_)(*[R(*r) for r in refs]), C.c_void_p) if refs is not None else None
        a_m = None if maps is None else C.cast((C.c_void_p * 2)(*(maps if maps != "good" else [b.data_ptr() for b in mapbuf])), C.c_void_p)
        return lib().hvq_picture_ssim(ctx._h, n_ if count is None else count, (C.c_int * n_)(*sids), (C.c_int * n_)(*ords), a_r,
                                      C.c_void_p(out.data_ptr() if dst is None else dst), a_m, stream)

    S0, S1 = (sa, 0, None), (sa, 1, None)
    arg = [("another sampling", [sa, sa], [0, 1], [S1, (sb, 1, None)]), ("another size", [sa, sa], [0, 1], [S1, (sc, 1, None)]),
           ("ptr with stream >= 0", [sa, sa], [0, 1], [S1, (sa, 0, p16)]), ("misaligned ptr", [sa, sa], [0, 1], [S1, (-1, 0, p16 + 8)]),
           ("bad stream", [sa, 99], [0, 0], [S1, S0]), ("bad ordinal", [sa, sa], [0, 1000], [S1, S0]), ("negative ordinal", [sa, sa], [0, -1], [S1, S0]),
           ("bad reference stream", [sa, sa], [0, 1], [S1, (99, 0, None)]), ("bad reference ordinal", [sa, sa], [0, 1], [S1, (sa, n, None)]),
           ("reference stream below -1", [sa, sa], [0, 1], [S1, (-2, 0, None)]),
           ("ref == NULL", [sa, sa], [0, 1], None), ("a zeros reference", [sa, sa], [0, 1], [S1, (-1, 0, None)])]
    for what, sids, ords, refs in arg:
        assert raw(sids, ords, refs) == HVQ_E_ARG, what
    assert raw([sa, sa], [0, 1], [S1, S0], dst=0) == HVQ_E_ARG, "null out"
    assert raw([sa, sa], [0, 1], [S1, S0], dst=out.data_ptr() + 4) == HVQ_E_ARG, "misaligned out"
    assert raw([sa, sa], [0, 1], [S1, S0], maps=[mapbuf[0].data_ptr(), mapbuf[1].data_ptr() + 2]) == HVQ_E_ARG, "misaligned map"
    assert raw([sa], [0], [S1], count=65536, maps=None) == HVQ_E_ARG, "n beyond the launch shape"
    L = (sd, last, None)
    assert raw([sd, sd], [last, 0], [L, L]) == HVQ_E_STATE, "an evicted picture"
    assert raw([sd, sd], [last, last], [L, (sd, 0, None)]) == HVQ_E_STATE, "an evicted reference"
    # through the Python layer: the library's refusals arrive as HvqError, the layer's own as ValueError
    for code, sids, ords, refs in ((HVQ_E_ARG, [sa, sa], [0, 1], [(sa, 1), (sb, 1)]), (HVQ_E_ARG, [sa, sa], [0, 1000], [(sa, 1), (sa, 0)]),
                                   (HVQ_E_STATE, [sd, sd], [last, 0], [(sd, last), (sd, last)]),
                                   (HVQ_E_STATE, [sd, sd], [last, last], [(sd, last), (sd, 0)])):
        try:
            ctx.picture_ssim(sids, ords, refs, out=out)
        except HvqError as e:
            assert e.code == code, (e, sids, ords, refs)
        else:
            raise AssertionError(("not refused", sids, ords, refs))
    for refs in (None, [(sa, 1), None], [(sa, 1), mem[p16 - mem.data_ptr() + 8:][:ctx.pic_bytes(sa)]], [(sa, 1), mem[:ctx.pic_bytes(sa) - 16]]):
        try:
            ctx.picture_ssim([sa, sa], [0, 1], refs, out=out)
        except ValueError:
            pass
        else:
            raise AssertionError("a missing, zeros, misaligned or short reference was not refused")
    torch.cuda.synchronize()
    assert out.eq(SENTINEL).all(), "a refused call wrote its output"
    assert all(b.eq(0x5A5A5A5A).all() for b in mapbuf), "a refused call wrote a map"
    # the well-formed call right after them works
    assert raw([sa, sd], [1, last], [S0, (sd, last, None)]) == 0
    torch.cuda.synchronize()
    wants = [_want(yuv[1], yuv[0], hdr), _want(yuv[last], yuv[last], hdr)]
    _same(out, [(b[:nwin].view(torch.float32),) for b in mapbuf], wants, "after the refusals")
    assert all(b[nwin:].eq(0x5A5A5A5A).all() for b in mapbuf)
    for s in (sa, sb, sc, sd):
        ctx.close_stream(s)


def case_ordering(torch, ctx):
    """on a non-default torch stream, nothing waited for: a call, then flushes that rewrite every slot it reads (the pattern of the
    slot-safety case of tests/test_gpu_metrics.py); then streaming: hvq_flush_next, SSIM of batch k beside batch k + 1 in flight"""
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
    out = torch.full((4, 3, 2), -1, dtype=torch.int64, device="cuda")
    side.wait_stream(torch.cuda.current_stream())    # out and mem were filled on the current stream
    with torch.cuda.stream(side):
        got, maps = ctx.picture_ssim([sid] * 4, [1, 2, 0, 2], [(sid, 0), (sid, 1), (sid, 0), mem], out=out, maps=True)
    for ft, p in pics[3:9]:
        ctx.submit(sid, ft, p)
    ctx.flush()                                      # rewrites every slot of the ring of 3
    ctx.replay(1)
    torch.cuda.synchronize()
    _same(got, maps, [_want(yuv[1], yuv[0], hdr), _want(yuv[2], yuv[1], hdr), _want(yuv[0], yuv[0], hdr), _want(yuv[2], yuv[7], hdr)],
          "flush behind the call")
    ctx.close_stream(sid)
    # streaming: batch k measured while batch k + 1 is in flight; batch k + 2 reuses batch k's slots
    sid = ctx.open_stream(w, h, 2, 2, hdr.is15, 8)
    b = [pics[0:4], pics[4:8], pics[8:12]]
    sub = lambda part: ctx.submit_many_device([sid] * len(part), [ft for ft, _p in part], [p for _f, p in part])
    sub(b[0]); ctx.flush_begin()
    sub(b[1]); ctx.flush_next()                      # batch 0 ended, batch 1 in flight
    out = torch.full((4, 3, 2), -1, dtype=torch.int64, device="cuda")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got, maps = ctx.picture_ssim([sid] * 4, [0, 1, 2, 3], [(sid, 3), (sid, 0), (sid, 1), (sid, 2)], out=out, maps=True)
    sub(b[2]); ctx.flush_next()                      # batch 1 ended, batch 2 in flight
    ctx.flush_end()                                  # batch 2 reconstructed into batch 0's slots
    torch.cuda.synchronize()
    _same(got, maps, [_want(yuv[0], yuv[3], hdr)] + [_want(yuv[k], yuv[k - 1], hdr) for k in (1, 2, 3)], "flush_next")
    # a picture of the batch in flight as the reference: the call ends that batch itself
    sub(b[0]); ctx.flush_begin()
    got = ctx.picture_ssim([sid], [11], [(sid, 12)])
    torch.cuda.synchronize()
    _same(got, None, [_want(yuv[11], yuv[0], hdr)], "a reference of the batch in flight")
    for k in range(8, 12):
        assert np.array_equal(ctx.read_picture(sid, k), yuv[k]), k
    ctx.close_stream(sid)


CASES = ["goldens", "mixed_batch", "tile_edges", "overwrite_and_determinism", "refusals", "ordering"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "ssim", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_ssim(case, child_results):
    gpu_child.report(case, child_results)
