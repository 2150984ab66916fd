"""GPU: perceptual hashes and nearest-hash search (hvq_picture_hashes / Context.picture_hashes, hvq_hash_nearest / Context.hash_nearest)
against tests/golden/phash.json (tests/phash_ref.py on the reference's pictures), against tests/phash_ref.py on arbitrary bytes, and
against hvqm4_amd.phash.nearest, compared with ==.  The cases run in ONE child process that imports torch first (see
tests/gpu_child.py); each test reports its case.  The child stops at the first HVQ_E_HIP or HIP error: nothing more is started on a
GPU that has reported a fault."""
import json
import os

import numpy as np
import pytest

from tests import gpu_child
from tests.gpu_kit import ROOT, SEVEN_CLIPS as CLIPS, clip as _clip, decode as _decode

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300                                 # the cases take seconds each; a hung child is ended, not waited for
SENTINEL = 0x5A5A5A5A5A5A5A5A
SENTINEL32 = 0x5A5A5A5A


# ------------------------------------------------------------------------------------------------------------- child side
_cache = {}


def _fixture():
    if "fixture" not in _cache:
        clips = json.load(open(os.path.join(ROOT, "tests", "golden", "phash.json")))["clips"]
        _cache["fixture"] = {nm: [[int(a, 16), int(d, 16), int(p, 16), s] for a, d, p, s in rows] for nm, rows in clips.items()}
    return _cache["fixture"]


def _same(got, wants, what):
    """records as unsigned integers against the reference's, =="""
    from hvqm4_amd import phash
    g = got.cpu().numpy()
    assert g.dtype == np.int64 and g.shape == (len(wants), 4), (what, g.dtype, g.shape, len(wants))
    rec = phash.as_uint64(g).tolist()
    if rec != [list(w) for w in wants]:
        bad = [(i, v) for i in range(len(wants)) for v in range(4) if rec[i][v] != wants[i][v]]
        i, v = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {4 * len(wants)} values differ, first at {(i, v)}: got {rec[i][v]:#x}, want {wants[i][v]:#x}")


def _near_same(got, want, what):
    g = got.cpu().numpy()
    w = np.asarray(want, dtype=np.int32).reshape(-1, 4)
    assert g.dtype == np.int32 and g.shape == w.shape, (what, g.dtype, g.shape, w.shape)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError(f"{what}: {len(bad)} of {g.size} values differ, first at {tuple(bad[0])}: got {g[bad[0][0]].tolist()}, want {w[bad[0][0]].tolist()}")


def case_goldens(torch, ctx):
    """the seven golden clips of tests/test_gpu_checksums.py, all three samplings, in ONE call, their pictures interleaved: a plane
    narrower than the grid (24 wide: 8-byte units, a sample feeds two cells), fractional cells (296 / 32 = 9.25 and 296 / 9), n = 1 and
    n = 0.  Records == the fixture; sum_y == sum_a of plane Y from picture_metrics on the same call list.  No picture is read back"""
    assert len(CLIPS) == 7
    fix = _fixture()
    streams, samplings, widths = [], set(), set()
    for name in CLIPS:
        sid, hdr, n = _decode(ctx, _clip(name))
        assert n == len(fix[name]), name
        streams.append((name, sid, n))
        samplings.add((hdr.h_samp, hdr.v_samp))
        widths.add(hdr.width)
    assert samplings == {(2, 2), (2, 1), (1, 1)}, samplings
    assert 24 in widths and 296 in widths
    sids, ords, wants = [], [], []
    for k in range(max(n for _nm, _s, n in streams)):           # round robin over the clips: mixed order
        for name, sid, n in streams[::-1] if k & 1 else streams:
            if k < n:
                sids.append(sid); ords.append(k); wants.append(fix[name][k])
    got = ctx.picture_hashes(sids, ords)
    one = ctx.picture_hashes(sids[-1:], ords[-1:])
    none = ctx.picture_hashes([], [])
    sums = ctx.picture_metrics(sids, ords)
    torch.cuda.synchronize()
    _same(got, wants, "seven clips in one call")
    _same(one, wants[-1:], "n = 1")
    assert tuple(none.shape) == (0, 4) and none.dtype == torch.int64
    assert torch.equal(got[:, 3], sums[:, 0, 0]), "sum_y is sum_a of plane Y"
    for _name, sid, _n in streams:
        ctx.close_stream(sid)


def _contents(w, h, seed):
    """luma planes: random, zeros, 0xFF, the half-and-half picture and its mirror, and the random one with its last sample changed"""
    rng = np.random.default_rng(seed)
    rnd = rng.integers(0, 256, (h, w), dtype=np.uint8)
    half = np.zeros((h, w), dtype=np.uint8)
    half[:, :w // 2] = 255
    last = rnd.copy()
    last[-1, -1] ^= 0x80
    return [("random", rnd), ("zeros", np.zeros((h, w), dtype=np.uint8)), ("0xFF", np.full((h, w), 255, dtype=np.uint8)), ("half", half),
            ("mirror", np.ascontiguousarray(half[:, ::-1])), ("last sample", last)]


def case_caller_memory(torch, ctx):
    """arbitrary pictures through `src` on streams nothing was decoded into: 8x8 (every sample feeds a 4 x 4 block of S32), 16x8,
    640x480 (exact 20 x 15 cells).  Chroma filled with different bytes must not change the record; a buffer that starts 16 bytes inside
    an allocation"""
    from tests.phash_ref import hash_reference
    for w, h in ((8, 8), (16, 8), (640, 480)):
        sid = ctx.open_stream(w, h, 2, 2, True, 3)
        nbytes = ctx.pic_bytes(sid)
        assert nbytes == w * h * 3 // 2
        cases = _contents(w, h, 7 + w)
        wants = [hash_reference(a) for _l, a in cases]
        pics = [np.concatenate([a.reshape(-1), np.full(w * h // 2, fill, dtype=np.uint8)]) for fill in (0, 0xC3) for _l, a in cases]
        bufs = [torch.from_numpy(p).cuda() for p in pics]
        got = ctx.picture_hashes([sid] * len(bufs), [-1] * len(bufs), src=bufs)
        inside = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")         # 16 bytes into an allocation
        off = (-inside.data_ptr()) % 16 + 16
        inside[off:off + nbytes] = bufs[0]
        got_in = ctx.picture_hashes([sid], [-1], src=[inside[off:off + nbytes]])
        torch.cuda.synchronize()
        _same(got, wants + wants, f"{w}x{h}: {[l for l, _a in cases]}, chroma 0 and 0xC3")
        _same(got_in, wants[:1], f"{w}x{h}: inside an allocation")
        labels = [l for l, _a in cases]
        assert wants[labels.index("zeros")] == [0, 0, 0, 0]
        assert wants[labels.index("0xFF")] == [0, 0, 1 << 63, 255 * w * h]
        assert wants[labels.index("last sample")][3] != wants[0][3], "the last sample shows in sum_y"
        if w == 640:
            assert wants[labels.index("half")][:2] == [0xF0F0F0F0F0F0F0F0, 0] and wants[labels.index("mirror")][0] == 0x0F0F0F0F0F0F0F0F
        ctx.close_stream(sid)


def case_cells64(torch, ctx):
    """one 8192 x 2064 picture through `src`: an all-0xFF cell is 255 * 8192 * 2064 = 4 311 613 440 > 2^32.  The left half is 255, the
    right half random in {252, 253}; the reference's record changes when its cells are reduced mod 2^32 (asserted here, on the host,
    first), so a 32-bit cell anywhere on the GPU's way shows"""
    from tests import phash_ref as ref
    w, h = 8192, 2064
    assert 255 * w * h == 4311613440 > 1 << 32
    rng = np.random.default_rng(64)
    y = np.empty((h, w), dtype=np.uint8)
    y[:, :w // 2] = 255
    y[:, w // 2:] = rng.integers(252, 254, (h, w // 2), dtype=np.uint8)
    data = y.tobytes()
    rows = [data[r * w:(r + 1) * w] for r in range(h)]
    grids = ref.grid(rows, 32, 32), ref.grid(rows, 8, 8), ref.grid(rows, 8, 9)
    assert max(max(r) for r in grids[0]) > 1 << 32
    want = ref.record_of_cells(*grids, w * h)
    narrow = ref.record_of_cells(*grids, w * h, cell_mod=1 << 32)
    assert [want[k] != narrow[k] for k in range(3)] == [True, True, True], "32-bit cells would give the same hashes: the case tests nothing"
    sid = ctx.open_stream(w, h, 2, 2, True, 3)
    pic = torch.empty(ctx.pic_bytes(sid), dtype=torch.uint8, device="cuda")
    pic[:w * h] = torch.from_numpy(y.reshape(-1)).cuda()
    pic[w * h:] = 0x80
    got = ctx.picture_hashes([sid], [-1], src=[pic])
    torch.cuda.synchronize()
    _same(got, [want], "8192x2064")
    ctx.close_stream(sid)


def _hashes(n, seed, bases=24):
    """n hashes a few bits away from a few bases: exact duplicates and equal distances at several j"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 1 << 63, bases, dtype=np.int64) * 2 + rng.integers(0, 2, bases, dtype=np.int64)
    h = base[rng.integers(0, bases, n)]
    for _ in range(3):
        flip = np.left_shift(np.int64(1), rng.integers(0, 64, n).astype(np.int64))
        h = np.where(rng.integers(0, 2, n) == 1, h ^ flip, h)
    return h.astype(np.int64)


def case_nearest(torch, ctx):
    """hash_nearest == phash.nearest: nq = ndb = 1; ndb one tile, one less and one more; nq = 257; ties and duplicates; self_offset 0 in
    place and k on a block; thresholds 0 and 64; ndb = 0; a sentinel behind the records"""
    from hvqm4_amd import phash
    T = phash.NEAREST_TILE
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    db = _hashes(T + 1, 1)
    q = np.concatenate([db[5:200], _hashes(62, 2)])                       # 257 queries: a second workgroup of one lane
    assert len(q) == 257 and len(set(db.tolist())) < len(db)
    d_db, d_q = dev(db), dev(q)
    runs = []
    for ndb in (T - 1, T, T + 1):
        for thr in (0, 3, 64):
            runs.append((f"ndb {ndb} thr {thr}", ctx.hash_nearest(d_q, d_db[:ndb], -1, thr), phash.nearest(q, db[:ndb], -1, thr)))
    runs.append(("one against one", ctx.hash_nearest(d_q[:1], d_db[:1]), phash.nearest(q[:1], db[:1], -1, 10)))
    runs.append(("in place", ctx.hash_nearest(d_db, None, threshold=2), phash.nearest(db, None, 0, 2)))
    runs.append(("in place, explicit", ctx.hash_nearest(d_db, d_db, 0, 2), phash.nearest(db, db, 0, 2)))
    runs.append(("a block at 5", ctx.hash_nearest(d_q[:195], d_db, 5, 2), phash.nearest(q[:195], db, 5, 2)))
    runs.append(("a block at 700", ctx.hash_nearest(d_db[700:], d_db, 700, 1), phash.nearest(db[700:], db, 700, 1)))
    runs.append(("ndb 0", ctx.hash_nearest(d_q, d_db[:0]), phash.nearest(q, db[:0], -1, 10)))
    # a sentinel-filled out with a guard behind it: untouched beyond 16 nq bytes
    room = torch.full((257 + 3, 4), SENTINEL32, dtype=torch.int32, device="cuda")
    assert ctx.hash_nearest(d_q, d_db, -1, 3, out=room[:257]).data_ptr() == room.data_ptr()
    none = ctx.hash_nearest(d_q[:0], d_db)
    torch.cuda.synchronize()
    for what, got, want in runs:
        _near_same(got, want, what)
    assert runs[4][1][0].tolist() != [-1, 65, 0, -1] and runs[10][1][0].tolist() == [-1, 65, 0, -1], "in place, query 0 has no candidate"
    assert runs[10][1].cpu().numpy().tolist() == runs[11][1].cpu().numpy().tolist()
    assert runs[12][1].cpu().numpy().tolist() == runs[10][1][5:200].cpu().numpy().tolist(), "a block sees what its queries see in place"
    assert runs[14][1].cpu().numpy().tolist() == [[-1, 65, 0, -1]] * 257
    w = runs[4][2]                                                        # ndb = T, thr 3: the set does exercise ties and first_within
    assert (w[:, 2] > 1).any() and (w[:, 3] != w[:, 0]).any() and (w[:, 1] == 0).any()
    _near_same(room[:257], phash.nearest(q, db, -1, 3), "into a view of a larger buffer")
    assert room[257:].eq(SENTINEL32).all(), "the records behind the last query were written"
    assert tuple(none.shape) == (0, 4) and none.dtype == torch.int32


def case_nearest_columns(torch, ctx):
    """stride 4 over a picture_hashes tensor, each of the three columns, queued right behind the hashes with nothing waited for; and a
    [n, k] view, of which column 0 counts"""
    from hvqm4_amd import phash
    name = "natural128x96"
    fix = _fixture()[name]
    sid, _hdr, n = _decode(ctx, _clip(name))
    rec = ctx.picture_hashes([sid] * n, list(range(n)))
    outs = [ctx.hash_nearest(rec[:, col], None, threshold=12) for col in range(3)]
    block = ctx.hash_nearest(rec[2:, phash.PHASH:], rec[:, phash.PHASH], 2, 12)
    torch.cuda.synchronize()
    _same(rec, fix, name)
    for col in range(3):
        _near_same(outs[col], phash.nearest([r[col] for r in fix], None, 0, 12), phash.NAMES[col])
    _near_same(block, phash.nearest([r[2] for r in fix[2:]], [r[2] for r in fix], 2, 12), "[n, k] view, a block")
    ctx.close_stream(sid)


def case_refusals(torch, ctx):
    """a refused call leaves a sentinel-filled out untouched"""
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
    out = torch.full((2, 4), SENTINEL, dtype=torch.int64, device="cuda")
    mem = torch.zeros(ctx.pic_bytes(sa) + 32, dtype=torch.uint8, device="cuda")
    p16 = mem.data_ptr() + (-mem.data_ptr()) % 16
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(sids, ords, src, dst=None, count=None, ctx_h=None):
        n_ = len(sids)
        a_p = C.cast((C.c_void_p * n_)(*src), C.c_void_p) if src is not None else None
        return lib().hvq_picture_hashes(ctx._h if ctx_h is None else ctx_h, n_ if count is None else count, (C.c_int * n_)(*sids),
                                        (C.c_int * n_)(*ords), a_p, C.c_void_p(out.data_ptr() if dst is None else dst), stream)

    arg = [("bad stream", [sa, 99], [0, 0], None), ("an ordinal that is not resident", [sa, sa], [0, 1000], None),
           ("negative ordinal", [sa, sa], [0, -1], None), ("misaligned src", [sa, sa], [0, -1], [None, p16 + 8]),
           ("src with an ordinal", [sa, sa], [0, 1], [None, p16]), ("src with a bad stream", [sa, 99], [0, -1], [None, p16])]
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
            ctx.picture_hashes(sids, ords, out=out)
        except HvqError as e:
            assert e.code == code, (e, sids, ords)
        else:
            raise AssertionError(("not refused", sids, ords))
    for src, ords in (([None, mem[p16 - mem.data_ptr() + 8:][:ctx.pic_bytes(sa)]], [0, -1]), ([None, mem[:ctx.pic_bytes(sa) - 16]], [0, -1]),
                      ([None, mem[p16 - mem.data_ptr():][:ctx.pic_bytes(sa)]], [0, 1])):
        try:
            ctx.picture_hashes([sa, sa], ords, src=src, out=out)
        except ValueError:
            pass
        else:
            raise AssertionError("a misaligned or short source tensor, or one with an ordinal, was not refused")
    # hvq_hash_nearest through the C ABI: q = db = the sentinel buffer's own words, out = the same buffer (16-byte aligned)
    o = out.data_ptr()
    assert o % 16 == 0

    def near(q=o, nq=2, qs=1, db=o, ndb=2, ds=1, thr=10, dst=o, ctx_h=None):
        return lib().hvq_hash_nearest(ctx._h if ctx_h is None else ctx_h, C.c_void_p(q), nq, qs, C.c_void_p(db), ndb, ds, -1, thr, C.c_void_p(dst), stream)

    for what, kw in (("null context", dict(ctx_h=C.c_void_p(0))), ("null q", dict(q=0)), ("misaligned q", dict(q=o + 4)), ("null db", dict(db=0)),
                     ("misaligned db", dict(db=o + 4)), ("null out", dict(dst=0)), ("misaligned out", dict(dst=o + 8)), ("a stride of 0", dict(qs=0)),
                     ("a negative stride", dict(ds=-4)), ("a threshold of 65", dict(thr=65)), ("a negative threshold", dict(thr=-1)),
                     ("nq < 0", dict(nq=-1)), ("nq beyond 2^24", dict(nq=(1 << 24) + 1)), ("ndb beyond 2^24", dict(ndb=(1 << 24) + 1))):
        assert near(**kw) == HVQ_E_ARG, what
    assert near(nq=0, q=0, dst=0) == 0, "nq == 0 does nothing"
    for kw in (dict(threshold=65), dict(threshold=-1)):
        try:
            ctx.hash_nearest(out[:, 0], **kw)
        except ValueError:
            pass
        else:
            raise AssertionError(("not refused", kw))
    torch.cuda.synchronize()
    assert out.eq(SENTINEL).all(), "a refused call wrote its output"
    # the well-formed call right after them works
    ctx.picture_hashes([sa, sd], [1, last], out=out)
    torch.cuda.synchronize()
    _same(out, [fix[1], fix[last]], "after the refusals")
    ctx.close_stream(sa); ctx.close_stream(sd)


def case_ordering(torch, ctx):
    """streaming, nothing waited for: flush_next, the hashes of batch k on a side stream beside batch k + 1 in flight, batch k + 2 into
    batch k's slots behind the call; hashes requested right after a flush equal those after a synchronisation"""
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
    out = torch.full((3, 4), -1, dtype=torch.int64, device="cuda")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ctx.picture_hashes([sid] * 3, [2, 0, 1], out=out)
    sub(b[2]); ctx.flush_next()                      # batch 1 ended, batch 2 in flight
    ctx.flush_end()                                  # batch 2 reconstructed: picture 6 lies in picture 0's slot of the ring of 6
    late = ctx.picture_hashes([sid] * 4, [3, 4, 5, 6])
    torch.cuda.synchronize()
    after = ctx.picture_hashes([sid] * 4, [3, 4, 5, 6])
    torch.cuda.synchronize()
    _same(got, [fix[k] for k in (2, 0, 1)], "batch 0 beside batch 1")
    _same(late, fix[3:7], "batches 1 and 2")
    assert torch.equal(late, after), "right after the flush and after a synchronisation"
    # a picture of the batch in flight: the call ends that batch itself
    sub(b[0]); ctx.flush_begin()
    got = ctx.picture_hashes([sid], [7 + 2])
    torch.cuda.synchronize()
    _same(got, [fix[2]], "a picture of the batch in flight")
    ctx.close_stream(sid)


def case_end_to_end(torch, ctx):
    """natural128x96: picture_hashes, then hash_nearest(database=None) on the pHash column where it lies; the duplicates found equal
    phash.duplicates of the host's records"""
    from hvqm4_amd import phash
    name = "natural128x96"
    sid, hdr, n = _decode(ctx, _clip(name))
    rec = ctx.picture_hashes([sid] * n, list(range(n)))
    near = {thr: ctx.hash_nearest(rec[:, phash.PHASH], threshold=thr) for thr in (4, 10, 24)}
    torch.cuda.synchronize()
    host = [phash.of_picture(ctx.read_picture(sid, k), hdr.width, hdr.height, hdr.h_samp, hdr.v_samp) for k in range(n)]
    _same(rec, host, name)
    for thr, got in near.items():
        assert got[:, phash.FIRST_WITHIN].cpu().tolist() == phash.duplicates([r[phash.PHASH] for r in host], thr), thr
    ctx.close_stream(sid)


CASES = ["goldens", "caller_memory", "cells64", "nearest", "nearest_columns", "refusals", "ordering", "end_to_end"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "phash", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_phash(case, child_results):
    gpu_child.report(case, child_results)
