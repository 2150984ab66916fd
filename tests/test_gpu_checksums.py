"""GPU: picture checksums (hvq_picture_checksums, Context.picture_checksums) against tests/golden/checksums.json (the reference's pictures
through zlib) and against tests/checksums_ref.py on arbitrary bytes, compared with ==.  Nothing is read back except where a case says so.
The cases run in ONE child process that imports torch first (see tests/gpu_child.py); each test reports its case.  The child stops
at the first HVQ_E_HIP or HIP error: nothing more is started on a GPU that has reported a fault."""
import json
import os
import zlib

import numpy as np
import pytest

from tests import gpu_child
from tests.gpu_kit import ROOT, SEVEN_CLIPS as CLIPS, clip as _clip, decode as _decode

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300                                 # the cases take seconds each; a hung child is ended, not waited for
SENTINEL = 0x5A5A5A5A5A5A5A5A


# ------------------------------------------------------------------------------------------------------------- child side
_cache = {}


def _fixture():
    if "fixture" not in _cache:
        _cache["fixture"] = json.load(open(os.path.join(ROOT, "tests", "golden", "checksums.json")))["clips"]
    return _cache["fixture"]


def _same(got, wants, what):
    got = got.cpu().numpy()
    want = np.array(wants, dtype=np.int64).reshape(-1, 8)
    assert got.dtype == np.int64 and got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]:#x}, "
                             f"want {want[tuple(bad[0])]:#x}")


def case_goldens(torch, ctx):
    """seven golden clips of all three samplings in ONE call, their pictures interleaved: a 240-byte chroma plane (less than a workgroup's
    run), planes that end inside a run, planes of several workgroups.  Records == the fixture; no picture is read back"""
    from hvqm4_amd import checksums as ck
    fix = _fixture()
    streams, samplings, units = [], set(), set()
    for name in CLIPS:
        sid, hdr, n = _decode(ctx, _clip(name))
        assert n == len(fix[name]), name
        streams.append((name, sid, n))
        samplings.add((hdr.h_samp, hdr.v_samp))
        units |= {b // 16 for b in ck.plane_bytes(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)}
    assert samplings == {(2, 2), (2, 1), (1, 1)}, samplings
    assert min(units) == 15 and any(u > 1024 and u % 1024 for u in units) and max(units) > 2 * 1024, units
    sids, ords, wants = [], [], []
    for k in range(max(n for _nm, _s, n in streams)):           # round robin over the clips: mixed order
        for name, sid, n in streams[::-1] if k & 1 else streams:
            if k < n:
                sids.append(sid); ords.append(k); wants.append(fix[name][k])
    got = ctx.picture_checksums(sids, ords)
    one = ctx.picture_checksums(sids[-1:], ords[-1:])
    none = ctx.picture_checksums([], [])
    torch.cuda.synchronize()
    _same(got, wants, "seven clips in one call")
    _same(one, wants[-1:], "n = 1")
    assert tuple(none.shape) == (0, 8)
    assert got.ge(0).all() and got.lt(1 << 32).all()
    for _name, sid, _n in streams:
        ctx.close_stream(sid)


def _contents(nbytes, seed):
    rng = np.random.default_rng(seed)
    rnd = rng.integers(0, 256, nbytes, dtype=np.uint8)
    last = rnd.copy()
    last[-1] ^= 0x80                                             # only the last byte of V differs: nothing lies behind it
    return [("random", rnd), ("zeros", np.zeros(nbytes, dtype=np.uint8)), ("0xFF", np.full(nbytes, 255, dtype=np.uint8)), ("last byte", last)]


def case_caller_memory(torch, ctx):
    """arbitrary bytes through `src` at 64x48 and at 640x480 (a stream no picture was decoded into).  All 0xFF at 640x480 drives Adler's
    weighted sum of Y to 255 * 307200 * 307201 / 2 = 1.2e13: any 32-bit total fails.  All zeros leaves the length-dependent terms."""
    from tests.checksums_ref import checksums_reference
    assert 255 * 307200 * 307201 // 2 > 1 << 40
    for w, h in ((64, 48), (640, 480)):
        sid = ctx.open_stream(w, h, 2, 2, True, 3)
        nbytes = ctx.pic_bytes(sid)
        assert nbytes == w * h * 3 // 2
        cases = _contents(nbytes, 7 + w)
        bufs = [torch.from_numpy(a).cuda() for _l, a in cases]
        got = ctx.picture_checksums([sid] * len(bufs), [-1] * len(bufs), src=bufs)
        inside = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")         # 16 bytes into an allocation
        off = (-inside.data_ptr()) % 16 + 16
        inside[off:off + nbytes] = bufs[0]
        got_in = ctx.picture_checksums([sid], [-1], src=[inside[off:off + nbytes]])
        torch.cuda.synchronize()
        wants = [checksums_reference(a, w, h, 2, 2) for _l, a in cases]
        _same(got, wants, f"{w}x{h}: {[l for l, _a in cases]}")
        _same(got_in, wants[:1], f"{w}x{h}: inside an allocation")
        g = got.cpu().numpy()
        assert (g[0, :3] == g[3, :3]).tolist() == [True, True, False] and g[0, 3] != g[3, 3] and g[0, 7] != g[3, 7], "the last byte shows in V and in the picture"
        ctx.close_stream(sid)


def case_consistency(torch, ctx):
    """the picture's values follow from the planes' by the combine helpers; crc32_picture is zlib's crc32 of what read_picture returns"""
    from hvqm4_amd import checksums as ck
    name = "yuv422_296x160"
    sid, hdr, n = _decode(ctx, _clip(name))
    got = ctx.picture_checksums([sid] * n, list(range(n)))
    torch.cuda.synchronize()
    rec = got.cpu().numpy().tolist()
    _y, lu, lv = ck.plane_bytes(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)
    for k, r in enumerate(rec):
        assert r[ck.CRC32_PICTURE] == ck.crc32_combine(ck.crc32_combine(r[ck.CRC32_Y], r[ck.CRC32_U], lu), r[ck.CRC32_V], lv), k
        assert r[ck.ADLER32_PICTURE] == ck.adler32_combine(ck.adler32_combine(r[ck.ADLER32_Y], r[ck.ADLER32_U], lu), r[ck.ADLER32_V], lv), k
        pic = ctx.read_picture(sid, k)
        assert r[ck.CRC32_PICTURE] == zlib.crc32(pic.tobytes()) and r[ck.ADLER32_PICTURE] == zlib.adler32(pic.tobytes()), k
        assert r == ck.of_bytes(pic, hdr.width, hdr.height, hdr.h_samp, hdr.v_samp), k
    _same(got, _fixture()[name], name)
    ctx.close_stream(sid)


def case_determinism(torch, ctx):
    """the same call three times on a side stream, back to back (they share the library's accumulator), into buffers full of a sentinel:
    identical records, every byte replaced"""
    fix = _fixture()
    sa, _h, na = _decode(ctx, _clip("wide296x160"))
    sb, _h, nb = _decode(ctx, _clip("natural128x96"))
    sids, ords = [sa] * na + [sb] * nb, list(range(na)) + list(range(nb))
    outs = [torch.full((na + nb, 8), SENTINEL, dtype=torch.int64, device="cuda") for _ in range(3)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for o in outs:
            assert ctx.picture_checksums(sids, ords, out=o) is o
    torch.cuda.synchronize()
    for o in outs:
        _same(o, fix["wide296x160"] + fix["natural128x96"], "three calls")
        assert not o.eq(SENTINEL).any()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    ctx.close_stream(sa); ctx.close_stream(sb)


def case_ordering(torch, ctx):
    """streaming, nothing waited for: flush_next, the checksums of batch k on a side stream beside batch k + 1 in flight, batch k + 2 into
    batch k's slots behind the call"""
    from hvqm4_amd.container import parse_header, video_pictures
    name = "gop64x48_15"
    data = _clip(name)
    fix = _fixture()[name]
    hdr = parse_header(data)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    assert len(pics) == 7 == len(fix)                # I P B B P B B
    sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, 6)
    b = [pics[0:3], pics[3:5], pics[5:7]]
    sub = lambda part: ctx.submit_many_device([sid] * len(part), [ft for ft, _p in part], [p for _f, p in part])
    side = torch.cuda.Stream()
    sub(b[0]); ctx.flush_begin()
    sub(b[1]); ctx.flush_next()                      # batch 0 ended, batch 1 in flight
    out = torch.full((3, 8), -1, dtype=torch.int64, device="cuda")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ctx.picture_checksums([sid] * 3, [2, 0, 1], out=out)
    sub(b[2]); ctx.flush_next()                      # batch 1 ended, batch 2 in flight
    ctx.flush_end()                                  # batch 2 reconstructed: picture 6 lies in picture 0's slot of the ring of 6
    late = ctx.picture_checksums([sid] * 4, [3, 4, 5, 6])
    torch.cuda.synchronize()
    _same(got, [fix[k] for k in (2, 0, 1)], "batch 0 beside batch 1")
    _same(late, fix[3:7], "batches 1 and 2")
    # a picture of the batch in flight: the call ends that batch itself
    sub(b[0]); ctx.flush_begin()
    got = ctx.picture_checksums([sid], [7 + 2])
    torch.cuda.synchronize()
    _same(got, [fix[2]], "a picture of the batch in flight")
    ctx.close_stream(sid)


def case_refusals(torch, ctx):
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_STATE, HvqError, lib
    from hvqm4_amd.container import video_pictures
    name = "gop64x48_15"
    data = _clip(name)
    fix = _fixture()[name]
    sa, hdr, n = _decode(ctx, data)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    sd = ctx.open_stream(hdr.width, hdr.height, 2, 2, hdr.is15, 3)
    for ft, p in pics:
        ctx.submit(sd, ft, p)
    ctx.flush()                                                  # picture 0 of sd: its slot of the ring of 3 was reused
    last = len(pics) - 1
    out = torch.full((2, 8), SENTINEL, dtype=torch.int64, device="cuda")
    mem = torch.zeros(ctx.pic_bytes(sa) + 32, dtype=torch.uint8, device="cuda")
    p16 = mem.data_ptr() + (-mem.data_ptr()) % 16
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(sids, ords, src, dst=None, count=None, ctx_h=None):
        n_ = len(sids)
        a_p = C.cast((C.c_void_p * n_)(*src), C.c_void_p) if src is not None else None
        return lib().hvq_picture_checksums(ctx._h if ctx_h is None else ctx_h, n_ if count is None else count, (C.c_int * n_)(*sids),
                                           (C.c_int * n_)(*ords), a_p, C.c_void_p(out.data_ptr() if dst is None else dst), stream)

    arg = [("bad stream", [sa, 99], [0, 0], None), ("bad ordinal", [sa, sa], [0, 1000], None), ("negative ordinal", [sa, sa], [0, -1], None),
           ("misaligned src", [sa, sa], [0, -1], [None, p16 + 8]), ("src with an ordinal", [sa, sa], [0, 1], [None, p16]),
           ("src with a bad stream", [sa, 99], [0, -1], [None, p16])]
    for what, sids, ords, src in arg:
        assert raw(sids, ords, src) == HVQ_E_ARG, what
    assert raw([sa, sa], [0, 1], None, ctx_h=C.c_void_p(0)) == HVQ_E_ARG, "null context"
    assert raw([sa, sa], [0, 1], None, dst=0) == HVQ_E_ARG, "null out"
    assert raw([sa, sa], [0, 1], None, dst=out.data_ptr() + 4) == HVQ_E_ARG, "misaligned out"
    assert raw([sa], [0], None, count=65536) == HVQ_E_ARG, "n beyond the launch shape"
    assert raw([sd, sd], [last, 0], None) == HVQ_E_STATE, "an evicted picture"
    assert raw([sa], [0], None, dst=0, count=0) == 0, "n == 0 does nothing"
    for code, sids, ords in ((HVQ_E_ARG, [sa, sa], [0, 1000]), (HVQ_E_STATE, [sd, sd], [last, 0])):
        try:
            ctx.picture_checksums(sids, ords, out=out)
        except HvqError as e:
            assert e.code == code, (e, sids, ords)
        else:
            raise AssertionError(("not refused", sids, ords))
    for src, ords in (([None, mem[p16 - mem.data_ptr() + 8:][:ctx.pic_bytes(sa)]], [0, -1]), ([None, mem[:ctx.pic_bytes(sa) - 16]], [0, -1]),
                      ([None, mem[p16 - mem.data_ptr():][:ctx.pic_bytes(sa)]], [0, 1])):
        try:
            ctx.picture_checksums([sa, sa], ords, src=src, out=out)
        except ValueError:
            pass
        else:
            raise AssertionError("a misaligned or short source tensor, or one with an ordinal, was not refused")
    torch.cuda.synchronize()
    assert out.eq(SENTINEL).all(), "a refused call wrote its output"
    # the well-formed call right after them works
    ctx.picture_checksums([sa, sd], [1, last], out=out)
    torch.cuda.synchronize()
    _same(out, [fix[1], fix[last]], "after the refusals")
    ctx.close_stream(sa); ctx.close_stream(sd)


CASES = ["goldens", "caller_memory", "consistency", "determinism", "ordering", "refusals"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "checksums", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_checksums(case, child_results):
    gpu_child.report(case, child_results)
