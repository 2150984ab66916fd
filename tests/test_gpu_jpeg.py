"""GPU: JPEG files of resident pictures (hvq_encode_jpeg, Context.encode_jpeg) against tests/jpeg_ref.py on the oracle's pictures and on
caller memory of chosen content, compared with == on bytes: the file is specified exactly.  The cases run in ONE child process that imports
torch first (see tests/gpu_child.py); each test reports its case.  The child stops at the first HVQ_E_HIP or HIP error: nothing more
is started on a GPU that has reported a fault."""
import numpy as np
import pytest

from tests import gpu_child
from tests.gpu_kit import decode as _decode, golden_by_name as _golden, long_clip_data as _long_clip, oracle as _oracle

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300                                 # the cases take seconds each; a hung child is ended, not waited for
SENTINEL = 0x5A
GUARD = 64                                          # bytes on either side of a destination
SIX = ["gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8"]


# ------------------------------------------------------------------------------------------------------------- child side
_state = {}


def _want(key, pic, hdr, quality):
    from tests.jpeg_ref import cached
    return cached(key, pic, hdr.width, hdr.height, quality, hdr.h_samp, hdr.v_samp)


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


def _all(six):
    """every picture of the clips: (name, sid, hdr, k, yuv)"""
    return [(name, six[name][0], six[name][1], k, six[name][3]) for name in SIX for k in range(six[name][2])]


def _guarded(torch, caps):
    """destinations between guards, all filled with the sentinel: (the buffers, the destinations as views of them)"""
    bufs = [torch.full((2 * GUARD + c,), SENTINEL, dtype=torch.uint8, device="cuda") for c in caps]
    return bufs, [b[GUARD:GUARD + c] for b, c in zip(bufs, caps)]


def _check(torch, bufs, outs, lengths, wants, what):
    """every file is the expected one, the bytes behind it and the guards still hold the sentinel"""
    got = lengths.cpu().tolist()
    assert got == [len(w) for w in wants], (what, "lengths", got, [len(w) for w in wants])
    for i, (buf, out, want) in enumerate(zip(bufs, outs, wants)):
        host = buf.cpu().numpy()
        file = host[GUARD:GUARD + len(want)].tobytes()
        if file != want:
            at = next(j for j, (a, b) in enumerate(zip(file, want)) if a != b)
            raise AssertionError(f"{what}: file {i} differs from byte {at} of {len(want)}: got {file[at:at + 8].hex()}, want {want[at:at + 8].hex()}")
        assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + out.numel():] == SENTINEL).all(), (what, i, "a guard was written")
        assert (host[GUARD + len(want):GUARD + out.numel()] == SENTINEL).all(), (what, i, "bytes behind the file were written")


def case_goldens(torch, ctx):
    """the six clips: all pictures in ONE call of mixed geometries and samplings at quality 90 (24 x 40: luma and chroma padded both ways;
    296 x 160 at 4:2:2: 20 intervals, RST wraps past 7, a 148-wide chroma plane that is not whole blocks; 4:4:4; 8 x 8: one interval, no
    RST) into sentinel-filled buffers between guards; the same call twice"""
    from hvqm4_amd import jpeg
    six = _six(ctx)
    assert {(h.h_samp, h.v_samp) for _s, h, _n, _y in six.values()} == {(2, 2), (2, 1), (1, 1)}
    assert {(h.width, h.height) for _s, h, _n, _y in six.values()} >= {(24, 40), (296, 160), (8, 8)}
    P = _all(six)
    sids, ords = [p[1] for p in P], [p[3] for p in P]
    bufs, outs = _guarded(torch, [jpeg.bound(p[2].width, p[2].height, p[2].h_samp, p[2].v_samp) for p in P])
    got, lengths = ctx.encode_jpeg(sids, ords, quality=90, out=outs)
    again, lengths2 = ctx.encode_jpeg(sids, ords, quality=90)
    torch.cuda.synchronize()
    assert all(g is o for g, o in zip(got, outs)) and lengths.dtype == torch.int64
    wants = [_want((name, k), yuv[k], hdr, 90) for name, _sid, hdr, k, yuv in P]
    _check(torch, bufs, outs, lengths, wants, "goldens")
    assert jpeg.files(again, lengths2) == wants, "the same call twice, into buffers of the default size"
    assert all(a.numel() == 2 * ctx.pic_bytes(s) + 1024 for a, s in zip(again, sids))
    empty = ctx.encode_jpeg([], [])
    assert empty[0] == [] and empty[1].numel() == 0


def case_qualities(torch, ctx):
    """the same pictures at qualities 1, 50 and 100"""
    from hvqm4_amd import jpeg
    six = _six(ctx)
    P = _all(six)
    sids, ords = [p[1] for p in P], [p[3] for p in P]
    got = {q: ctx.encode_jpeg(sids, ords, quality=q) for q in (1, 50, 100)}
    torch.cuda.synchronize()
    for q, (bufs, lengths) in got.items():
        files = jpeg.files(bufs, lengths)
        for (name, _sid, hdr, k, yuv), f in zip(P, files):
            assert f == _want((name, k), yuv[k], hdr, q), (name, k, q)


def case_content(torch, ctx):
    """chosen content through src= on streams used only for their geometry: uniform noise at quality 100 (stuffing, long codes) at 4:2:0,
    4:2:2 (296 x 160) and 4:4:4, all-128, all-0 and all-255; the 128 basis sign patterns packed into one 64 x 128 4:4:4 picture"""
    from hvqm4_amd import jpeg
    from tests.jpeg_ref import basis_picture, jpeg_reference
    six = _six(ctx)
    rng = np.random.default_rng(20261019)
    items = []                                                      # (sid, hdr-like geometry, picture, quality)
    for name in ("gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40"):
        sid, hdr, _n, _y = six[name]
        items.append((sid, hdr, rng.integers(0, 256, ctx.pic_bytes(sid), dtype=np.uint8), 100))
    sid, hdr, _n, _y = six["gop64x48_15"]
    for v in (128, 0, 255):
        items.append((sid, hdr, np.full(ctx.pic_bytes(sid), v, dtype=np.uint8), 100))
    sb = ctx.open_stream(64, 128, 1, 1, hdr.is15, 3)
    dev = [torch.from_numpy(p).cuda() for _s, _h, p, _q in items]
    bufs, lengths = ctx.encode_jpeg([i[0] for i in items], [-1] * len(items), quality=100, src=dev)
    bdev = torch.from_numpy(basis_picture()).cuda()
    bb, bl = ctx.encode_jpeg([sb, sb], [-1, -1], quality=100, src=[bdev, bdev])
    b90, l90 = ctx.encode_jpeg([i[0] for i in items], [-1] * len(items), quality=90, src=dev)
    torch.cuda.synchronize()
    files, files90 = jpeg.files(bufs, lengths), jpeg.files(b90, l90)
    for i, ((_sid, h, pic, q), f, f9) in enumerate(zip(items, files, files90)):
        assert f == jpeg_reference(pic, h.width, h.height, 100, h.h_samp, h.v_samp), ("content", i, 100)
        assert f9 == jpeg_reference(pic, h.width, h.height, 90, h.h_samp, h.v_samp), ("content", i, 90)
    assert files[0].count(b"\xff\x00") > 0, "noise at quality 100 stuffs bytes"
    want = jpeg_reference(basis_picture(), 64, 128, 100, 1, 1)
    assert jpeg.files(bb, bl) == [want, want], "the basis sign patterns"
    ctx.close_stream(sb)


def case_wide(torch, ctx):
    """one 2048 x 16 4:2:0 picture of noise through src=: one interval of 128 MCUs needs several chunks of the workgroup, the bit position,
    the partial byte and the DC predictors carried across them"""
    from hvqm4_amd import jpeg
    from tests.jpeg_ref import jpeg_reference
    hdr = _six(ctx)["gop64x48_15"][1]
    sid = ctx.open_stream(2048, 16, 2, 2, hdr.is15, 3)
    rng = np.random.default_rng(11)
    pics = [rng.integers(0, 256, 2048 * 16 * 3 // 2, dtype=np.uint8), (np.arange(2048 * 16 * 3 // 2) // 5 % 251).astype(np.uint8)]
    dev = [torch.from_numpy(p).cuda() for p in pics]
    got = {q: ctx.encode_jpeg([sid, sid], [-1, -1], quality=q, src=dev) for q in (100, 75)}
    torch.cuda.synchronize()
    for q, (bufs, lengths) in got.items():
        assert jpeg.files(bufs, lengths) == [jpeg_reference(p, 2048, 16, q, 2, 2) for p in pics], ("wide", q)
    ctx.close_stream(sid)


def case_overflow(torch, ctx):
    """cap = the file's length - 1 for one picture of a call, exact for its neighbours: its length is the full one, its guards and the
    neighbours' files are intact; a second call with the reported length succeeds"""
    six = _six(ctx)
    sid, hdr, _n, yuv = six["gop64x48_15"]
    ords = [0, 1, 2, 3]
    wants = [_want(("gop64x48_15", k), yuv[k], hdr, 90) for k in ords]
    caps = [len(w) for w in wants]
    caps[1] -= 1
    bufs, outs = _guarded(torch, [-(-c // 16) * 16 for c in caps])         # views of `c` bytes below: the capacity is the view's length
    outs = [o[:c] for o, c in zip(outs, caps)]
    _o, lengths = ctx.encode_jpeg([sid] * 4, ords, quality=90, out=outs)
    torch.cuda.synchronize()
    assert lengths.cpu().tolist() == [len(w) for w in wants], "lengths[i] is the full length, whether or not the file fitted"
    for i, (buf, want) in enumerate(zip(bufs, wants)):
        host = buf.cpu().numpy()
        assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + caps[i]:] == SENTINEL).all(), (i, "a byte at or beyond cap was written")
        if i != 1:
            assert host[GUARD:GUARD + len(want)].tobytes() == want, (i, "a neighbour of the file that did not fit")
    need = lengths.cpu().tolist()
    bufs2, outs2 = _guarded(torch, [-(-c // 16) * 16 for c in need])
    outs2 = [o[:c] for o, c in zip(outs2, need)]
    _o, lengths2 = ctx.encode_jpeg([sid] * 4, ords, quality=90, out=outs2)
    torch.cuda.synchronize()
    _check(torch, bufs2, outs2, lengths2, wants, "overflow, the second call")


def case_refusals(torch, ctx):
    """the refusals leave every destination and the lengths untouched: a bad quality, a misaligned out, a cap too small for a header, a src
    with an ordinal"""
    import ctypes as C
    from hvqm4_amd import jpeg
    from hvqm4_amd._lib import HVQ_E_ARG, HvqError, lib
    six = _six(ctx)
    sa, hdr, _n, yuv = six["gop64x48_15"]
    room = -(-jpeg.bound(64, 48) // 16) * 16
    out = torch.full((2, room), SENTINEL, dtype=torch.uint8, device="cuda")
    lengths = torch.full((2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    mem = torch.zeros(ctx.pic_bytes(sa), dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    o0, o1 = out[0].data_ptr(), out[1].data_ptr()

    def raw(sids=(sa, sa), ords=(0, 1), src=None, quality=90, dst=(o0, o1), cap=(room, room), ln=lengths.data_ptr()):
        n = len(sids)
        a_p = None if src is None else C.cast((C.c_void_p * n)(*src), C.c_void_p)
        return lib().hvq_encode_jpeg(ctx._h, n, (C.c_int * n)(*sids), (C.c_int * n)(*ords), a_p, quality, C.cast((C.c_void_p * n)(*dst), C.c_void_p),
                                     C.cast((C.c_uint64 * n)(*cap), C.c_void_p), C.c_void_p(ln), stream)

    for what, kw in [("quality 0", dict(quality=0)), ("quality 101", dict(quality=101)), ("a misaligned out", dict(dst=(o0, o1 + 8))), ("a null out[i]", dict(dst=(o0, 0))),
                     ("cap below header + EOI", dict(cap=(room, 630))), ("src with an ordinal", dict(src=(None, mem.data_ptr()))),
                     ("misaligned lengths", dict(ln=lengths.data_ptr() + 4)), ("null lengths", dict(ln=0)), ("a bad ordinal", dict(ords=(0, 1000)))]:
        assert raw(**kw) == HVQ_E_ARG, what
    for kw in (dict(quality=0), dict(quality=101), dict(out=[out[0], out[1][8:]]), dict(out=[out[0], out[1][:630]]), dict(src=[None, mem])):
        try:
            ctx.encode_jpeg([sa, sa], [0, 1], **dict(dict(out=[out[0], out[1]], lengths=lengths), **kw))
        except (ValueError, HvqError):
            pass
        else:
            raise AssertionError(("not refused", kw))
    torch.cuda.synchronize()
    assert out.eq(SENTINEL).all() and lengths.eq(0x5A5A5A5A5A5A5A5A).all(), "a refused call wrote a destination or the lengths"
    # the well-formed call right after them works
    ctx.encode_jpeg([sa, sa], [0, 1], out=[out[0], out[1]], lengths=lengths)
    torch.cuda.synchronize()
    assert jpeg.files([out[0], out[1]], lengths) == [_want(("gop64x48_15", k), yuv[k], hdr, 90) for k in (0, 1)]


def case_ordering(torch, ctx):
    """on a non-default torch stream, nothing waited for: encode_jpeg right after the hvq_flush_next that ended the batch its pictures belong
    to, beside the next batch in flight, then later flushes rewrite the slots it read -- the same files as after a sync"""
    from hvqm4_amd import jpeg
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
    with torch.cuda.stream(side):
        early = ctx.encode_jpeg([sid] * 4, [0, 1, 2, 3], quality=90)
    sub(b[2]); ctx.flush_next()                      # batch 1 ended, batch 2 in flight
    ctx.flush_end()                                  # batch 2 reconstructed into batch 0's slots
    torch.cuda.synchronize()
    late = ctx.encode_jpeg([sid] * 2, [4, 5], quality=90)
    torch.cuda.synchronize()
    files = jpeg.files(*early)
    assert files == [jpeg.encode(yuv[k], hdr.width, hdr.height, 90) for k in range(4)], "right after flush_next"
    assert files[1] == _want(("long640x480", 1), yuv[1], hdr, 90), "640 x 480: two chunks an interval"
    assert jpeg.files(*late) == [jpeg.encode(yuv[k], hdr.width, hdr.height, 90) for k in (4, 5)], "after a sync"
    ctx.close_stream(sid)


CASES = ["goldens", "qualities", "content", "wide", "overflow", "refusals", "ordering"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "jpeg", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_jpeg(case, child_results):
    gpu_child.report(case, child_results)
