"""GPU: lookup tables on pictures in slot layout (hvq_map_pictures / Context.map_pictures), tables from histogram records
(hvq_histogram_tables / Context.histogram_tables) and their chain (Context.equalize_pictures) against hvqm4_amd.maps -- which
tests/test_map_cpu.py holds equal to tests/map_ref.py, the plain-Python restatement of include/hvqm4_amd.h -- compared with ==.  Every
table that is not a known answer is a random permutation, distinct per plane and per picture.  Every output is allocated with 256
sentinel bytes before and behind it, which must stay untouched.  The shapes are the smallest that can go wrong: the golden clips, planes
of 8 x 8 (4 x 4 chroma), 72 x 24 and 136 x 40, planes of a tile, of a tile and 512 bytes and of a tile and four dwords (the kernel's tile
is 8192 consecutive bytes of a plane, the copy body's too), and rows of 8192.  The cases run in ONE child process that imports torch first
(see tests/gpu_child.py); each test reports its case.  The child stops at the first HVQ_E_HIP or HIP error: nothing more is started
on a GPU that has reported a fault."""
import os
import sys
import zlib

import numpy as np
import pytest

from tests import gpu_child, gpu_kit
from tests.gpu_kit import GUARD, ROOT, SENTINEL, check_bytes as _check, clip as _clip, decode as _decode, geom as _geom, golden as _golden, rooms as _rooms

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300                                 # the cases take seconds each; a hung child is ended, not waited for


# ------------------------------------------------------------------------------------------------------------- child side
def _map(torch, ctx, sids, ords, tables, planes=7, src=None, equalize=None):
    """one call (equalize_pictures with the rules `equalize`) into guarded rooms -> (list of uint8 tensors, guards)"""
    uniform = len({ctx._geometry(s) for s in set(sids)}) <= 1
    out, guards = _rooms(torch, [ctx.pic_bytes(s) for s in sids], uniform)
    got = ctx.equalize_pictures(sids, ords, equalize, src=src, out=out) if equalize is not None else ctx.map_pictures(sids, ords, tables, planes, src, out)
    assert got is out
    return [out[i] for i in range(len(sids))], guards


class _Uploaded(gpu_kit.Uploaded):
    def run(self, torch, tables, what, planes=7):
        """the pictures in ONE call, tables[i] for picture i, compared with the module's bytes"""
        from hvqm4_amd import maps as M
        got, guards = _map(torch, self.ctx, self.sids, [-1] * len(self.sids), tables, planes, src=self.bufs)
        torch.cuda.synchronize()
        _check(torch, got, guards, [M.of_picture(p, g, t, planes) for p, g, t in zip(self.pics, self.geoms, tables)], what)
        return got


def _made(geoms, per=2, first=0):
    """`per` made pictures of every geometry with a table of their own each: the known answers first, then permutations"""
    from tests import map_cases as cases
    pics, gs = [], []
    for i, g in enumerate(geoms):
        for j in range(per):
            pics.append(cases.made(g, 31 * i + j)); gs.append(g)
    return pics, gs, cases.tables(first + len(pics))[first:]


def case_golden(torch, ctx):
    """every golden clip's pictures, a table of its own for every picture: identity, inversion, a constant, then permutations"""
    from hvqm4_amd import maps as M
    from tests import map_cases as cases
    samplings = set()
    for name, data, _hdr, _n in _golden():
        sid, hdr, n = _decode(ctx, data)
        g = _geom(hdr)
        samplings.add(g[2:])
        tables = cases.tables(n)
        got, guards = _map(torch, ctx, [sid] * n, list(range(n)), tables)
        torch.cuda.synchronize()
        pics = [ctx.read_picture(sid, k).reshape(-1) for k in range(n)]
        _check(torch, got, guards, [M.of_picture(p, g, t) for p, t in zip(pics, tables)], name)
        ctx.close_stream(sid)
    assert samplings == {(2, 2), (2, 1), (1, 1)}


def case_seams(torch, ctx):
    """planes of exactly a tile (128 x 64), of a tile and 512 bytes, of a tile and four dwords (the 108 x 76 chroma of 216 x 152), of
    several tiles, and rows of 8192: every plane through a permutation of its own, and again with the chroma planes copied (the copy
    body over the same seams)"""
    from tests import map_cases as cases
    geoms = cases.SEAMS + [cases.WIDE]
    assert 128 * 64 == 8192 and 108 * 76 == 8192 + 16
    pics, gs, tables = _made(geoms, per=2, first=3)
    up = _Uploaded(torch, ctx, pics, gs)
    up.run(torch, tables, "seams")
    up.run(torch, tables, "seams, chroma copied", planes=1)
    up.run(torch, tables, "seams, luma copied", planes=6)
    up.close()


def case_narrow(torch, ctx):
    """the smallest geometry in the three samplings (chroma planes of 16 bytes: four lanes of one workgroup), 72 x 24 and 136 x 40"""
    from tests import map_cases as cases
    pics, gs, tables = _made(cases.SMALL, per=3)
    up = _Uploaded(torch, ctx, pics, gs)
    up.run(torch, tables, "narrow planes")
    up.close()


def case_which(torch, ctx):
    """the forms of `tables`: one Table; a list with repeats (shared records); a device tensor of 1 and of n records; and through the C
    entry an explicit `which` that permutes a table of n, and NULL with 1 and with n"""
    import ctypes as C
    from hvqm4_amd import maps as M
    from hvqm4_amd._lib import check, lib
    from tests import map_cases as cases
    g = (72, 24, 2, 2)
    n = 6
    pics = [cases.made(g, 50 + i) for i in range(n)]
    up = _Uploaded(torch, ctx, pics, [g] * n)
    t = [cases.perm_table(20 + i) for i in range(n)]
    one, guards = _map(torch, ctx, up.sids, [-1] * n, t[0], src=up.bufs)
    shared = [t[0], t[1], t[0], t[2], t[1], t[0]]
    rep, rguards = _map(torch, ctx, up.sids, [-1] * n, shared, src=up.bufs)
    dev = torch.from_numpy(M.pack(t)).cuda()
    each, eguards = _map(torch, ctx, up.sids, [-1] * n, dev, src=up.bufs)
    first, fguards = _map(torch, ctx, up.sids, [-1] * n, dev[3:4], src=up.bufs)
    torch.cuda.synchronize()
    _check(torch, one, guards, [M.of_picture(p, g, t[0]) for p in pics], "one Table")
    _check(torch, rep, rguards, [M.of_picture(p, g, s) for p, s in zip(pics, shared)], "a list with repeats")
    _check(torch, each, eguards, [M.of_picture(p, g, s) for p, s in zip(pics, t)], "a tensor of n records")
    _check(torch, first, fguards, [M.of_picture(p, g, t[3]) for p in pics], "a tensor of one record")
    which = [5, 3, 3, 0, 1, 4]
    out, wguards = _rooms(torch, [cases.nbytes(g)] * n, True)
    a_d = (C.c_void_p * n)(*[out[i].data_ptr() for i in range(n)])
    a_p = (C.c_void_p * n)(*[b.data_ptr() for b in up.bufs])
    check(lib().hvq_map_pictures(ctx._h, n, (C.c_int * n)(*up.sids), (C.c_int * n)(*([-1] * n)), C.cast(a_p, C.c_void_p), C.c_void_p(dev.data_ptr()), n,
                                 C.cast((C.c_int * n)(*which), C.c_void_p), 7, C.cast(a_d, C.c_void_p), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    _check(torch, [out[i] for i in range(n)], wguards, [M.of_picture(p, g, t[w]) for p, w in zip(pics, which)], "an explicit which")
    up.close()


def case_planes(torch, ctx):
    """each mask 1 .. 7 on pictures of the three samplings: the planes whose bit is clear equal the source"""
    from tests import map_cases as cases
    geoms = [(72, 24, 2, 2), (72, 24, 2, 1), (72, 24, 1, 1)]
    pics, gs, tables = _made(geoms, per=2, first=3)
    up = _Uploaded(torch, ctx, pics, gs)
    for planes in range(1, 8):
        got = up.run(torch, tables, f"planes {planes}", planes=planes)
        at = 0
        for p, (pw, ph) in enumerate([(72, 24), (36, 12), (36, 12)]):
            same = np.array_equal(got[0].cpu().numpy()[at:at + pw * ph], pics[0][at:at + pw * ph])
            assert same == (not planes >> p & 1), (planes, p)
            at += pw * ph
    up.close()


def case_inplace(torch, ctx):
    """out rows that ARE the src rows: pictures of every shape through a permutation in place, then through its inverse in place: the
    sources again, and the bytes around them untouched"""
    from hvqm4_amd import maps as M
    from tests import map_cases as cases
    geoms = cases.SMALL[:4] + cases.SEAMS[1:3]
    pics, gs, tables = _made(geoms, per=1, first=3)
    by_geom, sids = {}, []
    for g in gs:
        if g not in by_geom:
            by_geom[g] = ctx.open_stream(g[0], g[1], g[2], g[3], True, 3)
        sids.append(by_geom[g])
    rooms, guards = _rooms(torch, [cases.nbytes(g) for g in gs], False)
    for r, p in zip(rooms, pics):
        r.copy_(torch.from_numpy(p))
    n = len(pics)
    assert ctx.map_pictures(sids, [-1] * n, tables, src=rooms, out=rooms) is rooms
    torch.cuda.synchronize()
    _check(torch, rooms, guards, [M.of_picture(p, g, t) for p, g, t in zip(pics, gs, tables)], "in place")
    ctx.map_pictures(sids, [-1] * n, [M.inverse(t) for t in tables], src=rooms, out=rooms)
    torch.cuda.synchronize()
    _check(torch, rooms, guards, pics, "in place, and back through the inverse permutation")
    for s in by_geom.values():
        ctx.close_stream(s)


def case_guards(torch, ctx):
    """the bytes around every output, and around the table records of histogram_tables, stay: a call whose outputs lie back to back in one
    allocation, every one of them between sentinels of its own"""
    from hvqm4_amd import maps as M
    from tests import map_cases as cases
    g = (136, 40, 2, 1)
    nb, n = cases.nbytes(g), 5
    pics = [cases.made(g, 70 + i) for i in range(n)]
    up = _Uploaded(torch, ctx, pics, [g] * n)
    pitch = nb + GUARD
    assert pitch % 16 == 0
    room = torch.full((GUARD + n * pitch,), SENTINEL, dtype=torch.uint8, device="cuda")
    outs = [room[GUARD + i * pitch:GUARD + i * pitch + nb] for i in range(n)]
    sid2 = ctx.open_stream(8, 8, 2, 2, True, 3)                          # a second geometry: the list form of out
    small = torch.full((96 + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    sbuf = torch.from_numpy(cases.made((8, 8, 2, 2), 9)).cuda()
    tables = [cases.perm_table(40 + i) for i in range(n + 1)]
    ctx.map_pictures(up.sids + [sid2], [-1] * (n + 1), tables, src=up.bufs + [sbuf], out=outs + [small[GUARD:GUARD + 96]])
    troom = torch.full((2 * GUARD + n * 768,), SENTINEL, dtype=torch.uint8, device="cuda")
    hist = ctx.picture_histograms(up.sids, [-1] * n, src=up.bufs)
    tabs = troom[GUARD:GUARD + n * 768].view(n, 3, 256)
    assert ctx.histogram_tables(hist, M.otsu(), out=tabs) is tabs
    torch.cuda.synchronize()
    host = room.cpu().numpy()
    for i in range(n):
        assert np.array_equal(host[GUARD + i * pitch:GUARD + i * pitch + nb], M.of_picture(pics[i], g, tables[i])), i
        assert (host[GUARD + i * pitch + nb:GUARD + (i + 1) * pitch] == SENTINEL).all(), f"behind output {i}"
    assert (host[:GUARD] == SENTINEL).all()
    s = small.cpu().numpy()
    assert (s[:GUARD] == SENTINEL).all() and (s[GUARD + 96:] == SENTINEL).all()
    assert np.array_equal(s[GUARD:GUARD + 96], M.of_picture(cases.made((8, 8, 2, 2), 9), (8, 8, 2, 2), tables[n]))
    th = troom.cpu().numpy()
    assert (th[:GUARD] == SENTINEL).all() and (th[GUARD + n * 768:] == SENTINEL).all()
    up.close()
    ctx.close_stream(sid2)


def case_tables(torch, ctx):
    """the record list of tests/test_map_cpu.py -- a single value, two values, uniform, the Otsu tie, N == 0, N == 2^26 between 0 and
    255 and between 0 and 1, the STRETCH clips 0 / 0 and 499 / 499 and hi <= lo, 300 random records -- through every rule, == the
    reference (tests/map_ref.py) directly for the special records and the module (which the CPU test holds equal to it) for all"""
    from hvqm4_amd import maps as M
    from tests import map_cases as cases
    from tests import map_ref as ref
    recs = cases.all_records()
    nspecial = len(cases.special_records())
    names = list(cases.RULES)
    hist = torch.from_numpy(recs.astype(np.int32)).cuda()
    got = {name: ctx.histogram_tables(hist, cases.RULES[name]) for name in names}
    mixed_rules = [cases.RULES[names[i % len(names)]] for i in range(len(recs))]                # one call, a rule per record
    mixed = ctx.histogram_tables(hist, mixed_rules)
    torch.cuda.synchronize()
    for name in names:
        g = got[name].cpu().numpy()
        want = M.tables_of_records(recs, cases.RULES[name])
        bad = np.flatnonzero((g != want).any(axis=(1, 2)))
        assert not bad.size, f"rule {name}: {bad.size} records differ, first record {bad[0]}"
        r = cases.RULES[name]
        for i in range(nspecial):
            plain = ref.record_tables([[int(x) for x in recs[i][p]] for p in range(3)], (r.luma.kind, r.luma.a, r.luma.b), (r.chroma.kind, r.chroma.a, r.chroma.b))
            assert g[i].tolist() == plain, (name, i)
    assert np.array_equal(mixed.cpu().numpy(), np.stack([M.tables_of_records(recs[i], mixed_rules[i]) for i in range(len(recs))]))


def case_chain(torch, ctx):
    """equalize_pictures (default rule, stretch, per-picture rules) == histograms.of_picture -> tables_of_records -> of_picture on the
    host; and the segmentation chain histograms -> Otsu tables -> map -> morph_pictures(opening) -> picture_histograms(src=), step by
    step == the host modules"""
    from hvqm4_amd import histograms as Hs
    from hvqm4_amd import maps as M
    from hvqm4_amd import rank as R
    from tests import map_cases as cases
    sid, hdr, n = _decode(ctx, _clip("yuv422_296x160"))
    g = _geom(hdr)
    n = min(n, 6)
    sids, ords = [sid] * n, list(range(n))
    pics = [ctx.read_picture(sid, k).reshape(-1) for k in range(n)]
    recs = np.stack([Hs.of_picture(p, *g) for p in pics])

    def expect(rules):
        rs = [rules] * n if isinstance(rules, M.Rule) else rules
        return [M.of_picture(p, g, M.from_lut(*M.tables_of_records(recs[i], rs[i]))) for i, p in enumerate(pics)]
    default = ctx.equalize_pictures(sids, ords)
    levels, lguards = _map(torch, ctx, sids, ords, None, equalize=M.stretch(10, 20))
    each_rule = [list(cases.RULES.values())[i % len(cases.RULES)] for i in range(n)]
    each, eguards = _map(torch, ctx, sids, ords, None, equalize=each_rule)
    # the segmentation chain, nothing waited for in between
    hist = ctx.picture_histograms(sids, ords)
    mask_rule = M.Rule(M.otsu().luma, M.flat(128).luma)
    tables = ctx.histogram_tables(hist, mask_rule)
    mask = ctx.map_pictures(sids, ords, tables)
    steps = [R.luma_only(s) for s in R.opening(1)]
    cur = ctx.morph_pictures(sids, [-1] * n, steps, src=[mask[i] for i in range(n)])
    counts = ctx.picture_histograms(sids, [-1] * n, src=[cur[i] for i in range(n)])
    sums = ctx.picture_checksums(sids, [-1] * n, src=[cur[i] for i in range(n)])
    torch.cuda.synchronize()
    _check(torch, [default[i] for i in range(n)], [], expect(M.equalize().luma_only()), "equalize_pictures")
    _check(torch, levels, lguards, expect(M.stretch(10, 20)), "equalize_pictures(stretch)")
    _check(torch, each, eguards, expect(each_rule), "equalize_pictures, a rule per picture")
    assert np.array_equal(hist.cpu().numpy(), recs), "histograms"
    want_t = M.tables_of_records(recs, mask_rule)
    assert np.array_equal(tables.cpu().numpy(), want_t), "Otsu tables"
    t = [int(Hs.otsu(recs[i][0])) for i in range(n)]
    assert [int((want_t[i][0] == 0).sum()) - 1 for i in range(n)] == t
    want_mask = [M.of_picture(p, g, M.from_lut(*want_t[i])) for i, p in enumerate(pics)]
    _check(torch, [mask[i] for i in range(n)], [], want_mask, "the masks")
    want_open = [R.of_steps(m, g, steps) for m in want_mask]
    _check(torch, [cur[i] for i in range(n)], [], want_open, "the opened masks")
    assert np.array_equal(counts.cpu().numpy(), np.stack([Hs.of_picture(m, *g) for m in want_open])), "picture_histograms(src=) of the opened masks"
    assert [int(v) for v in sums.cpu().numpy()[:, 3]] == [zlib.crc32(m.tobytes()) for m in want_open]
    assert all(0 < int(c[0][255]) < g[0] * g[1] for c in counts.cpu().numpy()), "a mask of a natural picture has both classes"
    ctx.close_stream(sid)


def case_many(torch, ctx):
    """300 mixed pictures of seven shapes in one call, 64 distinct tables; the same call twice gives the same bytes"""
    from tests import map_cases as cases
    shapes = cases.SMALL[:5] + cases.SEAMS[1:3]
    table = cases.tables(64)
    base = {g: [cases.made(g, 90 + k) for k in range(3)] for g in shapes}
    pics, gs, ts = [], [], []
    for i in range(300):
        g = shapes[i % len(shapes)]
        pics.append(base[g][(i // 7) % 3]); gs.append(g); ts.append(table[(i * 7 + i // 64) % 64])
    assert len(set(ts)) == 64
    up = _Uploaded(torch, ctx, pics, gs)
    a = up.run(torch, ts, "300 pictures, 64 tables")
    b = up.run(torch, ts, "300 pictures again")
    assert all(bool((x == y).all()) for x, y in zip(a, b))
    up.close()


def _raw(torch, ctx, sids, ords, src, tables_ptr, ntables=1, which=None, planes=7, count=None, ctx_h=None, ptr=None):
    """hvq_map_pictures through the C ABI into sentinel-filled memory -> (return code, every byte still holds the sentinel)"""
    import ctypes as C
    from hvqm4_amd._lib import lib
    n = len(sids)
    room = torch.full((n, 8192), SENTINEL, dtype=torch.uint8, device="cuda")
    a_d = (C.c_void_p * n)(*[(ptr if ptr is not None and i == 0 else room[i].data_ptr()) for i in range(n)])
    a_p = C.cast((C.c_void_p * n)(*src), C.c_void_p) if src is not None else None
    a_w = C.cast((C.c_int * n)(*which), C.c_void_p) if which is not None else None
    rc = lib().hvq_map_pictures(ctx._h if ctx_h is None else ctx_h, n if count is None else count, (C.c_int * n)(*sids), (C.c_int * n)(*ords), a_p,
                                C.c_void_p(tables_ptr), ntables, a_w, planes, C.cast(a_d, C.c_void_p), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, bool(room.eq(SENTINEL).all())


def _raw_tables(torch, ctx, hist_ptr, structs, n=2, which=None, nrules=None, ctx_h=None, out_ptr=None, null_rules=False):
    """hvq_histogram_tables through the C ABI into sentinel-filled memory -> (return code, every byte still holds the sentinel)"""
    import ctypes as C
    from hvqm4_amd._lib import HvqTableRule, lib
    room = torch.full((2, 768), SENTINEL, dtype=torch.uint8, device="cuda")
    a_r = (HvqTableRule * len(structs))(*structs)
    a_w = C.cast((C.c_int * len(which))(*which), C.c_void_p) if which is not None else None
    rc = lib().hvq_histogram_tables(ctx._h if ctx_h is None else ctx_h, n, C.c_void_p(hist_ptr), None if null_rules else C.cast(a_r, C.c_void_p),
                                    len(structs) if nrules is None else nrules, a_w, C.c_void_p(room.data_ptr() if out_ptr is None else out_ptr),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, bool(room.eq(SENTINEL).all())


def case_refusals(torch, ctx):
    """every refusal of the header through the C entries leaves the destinations untouched, also those of the well-formed pictures of
    the same call"""
    import ctypes as C
    from hvqm4_amd import maps as M
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_STATE
    from hvqm4_amd.container import video_pictures
    from tests import map_cases as cases
    from tests.test_map_cpu import _spoiled
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
    tabs = torch.from_numpy(M.pack(cases.tables(4))).cuda()
    T = tabs.data_ptr()
    assert T % 16 == 0
    two = [sa, sa]
    arg = [("bad stream", [sa, 99], [0, 0], None, {}), ("an ordinal that is not resident", two, [0, 1000], None, {}), ("negative ordinal", two, [0, -1], None, {}),
           ("misaligned src", two, [0, -1], [None, p16 + 8], {}), ("an ordinal with src", two, [0, 1], [None, p16], {}),
           ("src with a bad stream", [sa, 99], [0, -1], [None, p16], {}), ("which beyond the table", two, [0, 1], None, {"which": [0, 1]}),
           ("a negative which", two, [0, 1], None, {"which": [0, -1]}), ("ntables 0", two, [0, 1], None, {"ntables": 0}), ("ntables -1", two, [0, 1], None, {"ntables": -1}),
           ("ntables 65536", two, [0, 1], None, {"ntables": 65536, "which": [0, 0]}), ("3 tables for 2 pictures without which", two, [0, 1], None, {"ntables": 3}),
           ("planes 0", two, [0, 1], None, {"planes": 0}), ("planes 8", two, [0, 1], None, {"planes": 8}), ("planes -1", two, [0, 1], None, {"planes": -1}),
           ("null context", two, [0, 1], None, {"ctx_h": C.c_void_p(0)}), ("null dst", two, [0, 1], None, {"ptr": 0}), ("misaligned dst", two, [0, 1], None, {"ptr": p16 + 8})]
    for what, sids, ords, src, kw in arg:
        assert _raw(torch, ctx, sids, ords, src, T, **kw) == (HVQ_E_ARG, True), what
    assert _raw(torch, ctx, two, [0, 1], None, 0) == (HVQ_E_ARG, True), "null tables"
    assert _raw(torch, ctx, two, [0, 1], None, T + 8) == (HVQ_E_ARG, True), "misaligned tables"
    assert _raw(torch, ctx, [sa], [0], None, T, count=65536) == (HVQ_E_ARG, True), "n beyond 65535"
    assert _raw(torch, ctx, [sa], [0], None, T, count=0) == (0, True), "n == 0 does nothing"
    # the HVQ_E_STATE cases: a dropped picture (its slot was reused), a picture queued but not flushed
    assert _raw(torch, ctx, [sa, sd], [0, 0], None, T) == (HVQ_E_STATE, True), "a dropped picture"
    ctx.submit(sq, pics[0][0], pics[0][1])
    assert _raw(torch, ctx, [sa, sq], [0, 0], None, T) == (HVQ_E_STATE, True), "queued but not flushed"
    ctx.flush()
    # hvq_histogram_tables
    hist = torch.zeros((2, 3, 256), dtype=torch.int32, device="cuda")
    Hp = hist.data_ptr()
    good = M.otsu().struct()
    for label, s in _spoiled():                                  # every refusal of hvq_table_check, in an entry of the table that no record uses
        assert _raw_tables(torch, ctx, Hp, [good, s], which=[0, 0]) == (HVQ_E_ARG, True), label
        assert _raw_tables(torch, ctx, Hp, [s]) == (HVQ_E_ARG, True), label
    for what, kw in (("null context", {"ctx_h": C.c_void_p(0)}), ("nrules 0", {"nrules": 0}), ("nrules -1", {"nrules": -1}), ("null rules", {"null_rules": True}),
                     ("which beyond the rules", {"which": [0, 1]}), ("a negative which", {"which": [-1, 0]}), ("n beyond 65535", {"n": 65536}), ("negative n", {"n": -1}),
                     ("null tables", {"out_ptr": 0}), ("misaligned tables", {"out_ptr": p16 + 8})):
        assert _raw_tables(torch, ctx, Hp, [good], **kw) == (HVQ_E_ARG, True), what
    assert _raw_tables(torch, ctx, Hp, [good] * 65, which=[0, 64]) == (HVQ_E_ARG, True), "nrules 65"
    assert _raw_tables(torch, ctx, 0, [good]) == (HVQ_E_ARG, True), "null hist"
    assert _raw_tables(torch, ctx, Hp + 4, [good]) == (HVQ_E_ARG, True), "misaligned hist"
    assert _raw_tables(torch, ctx, Hp, [good], n=0) == (0, True), "n == 0 does nothing"
    rc, untouched = _raw_tables(torch, ctx, Hp, [good] * 64, which=[0, 63])
    assert rc == 0 and not untouched
    # the well-formed calls right after them work: the last table of four used, and the method
    rc, untouched = _raw(torch, ctx, two, [0, 1], None, T, ntables=4, which=[0, 3])
    assert rc == 0 and not untouched
    g = _geom(hdr)
    t = cases.perm_table(77)
    got, guards = _map(torch, ctx, [sa, sd, sq], [1, len(pics) - 1, 0], t)
    torch.cuda.synchronize()
    three = [ctx.read_picture(s, o).reshape(-1) for s, o in ((sa, 1), (sd, len(pics) - 1), (sq, 0))]
    _check(torch, got, guards, [M.of_picture(p, g, t) for p in three], "after the refusals")
    for s in (sa, sd, sq):
        ctx.close_stream(s)


def case_tools(torch, ctx):
    """tools/autolevels.py on a golden clip: equalisation, levels and the opened Otsu mask through encode_jpeg(src=): the files of the
    expected pictures, and the printed facts"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import autolevels
    from hvqm4_amd import histograms as Hs
    from hvqm4_amd import jpeg
    from hvqm4_amd import maps as M
    from hvqm4_amd import rank as R
    from oracle import bridge
    data = _clip("yuv422_64x48")
    g = (64, 48, 2, 1)
    for mode, lo, hi in (("equalize", 0, 0), ("stretch", 10, 20)):
        geom, files, facts = autolevels.clip_levelled(ctx, data, mode, lo, hi, quality=80)
        assert geom == g and facts is None
        pics = bridge.oracle_decode(data, len(files))
        rule = autolevels.rule_for(mode, lo, hi)
        assert rule == (M.equalize().luma_only() if mode == "equalize" else M.stretch(10, 20).luma_only())
        for k, f in enumerate(files):
            p = pics[k].reshape(-1)
            assert f == jpeg.encode(M.of_picture(p, g, M.from_lut(*M.tables_of_records(Hs.of_picture(p, *g), rule))), 64, 48, 80, 2, 1), (mode, k)
    geom, files, facts = autolevels.clip_levelled(ctx, data, "otsu", opening=1, quality=80)
    for k, f in enumerate(files):
        p = pics[k].reshape(-1)
        rec = Hs.of_picture(p, *g)
        mask = M.of_picture(p, g, M.from_lut(*M.tables_of_records(rec, autolevels.rule_for("otsu"))))
        opened = R.of_steps(mask, g, [R.luma_only(s) for s in R.opening(1)])
        assert facts[k] == (int(Hs.otsu(rec[0])), int((opened[:64 * 48] == 255).sum())), k
        assert f == jpeg.encode(opened, 64, 48, 80, 2, 1), k


CASES = ["golden", "seams", "narrow", "which", "planes", "inplace", "guards", "tables", "chain", "many", "refusals", "tools"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "map", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_map(case, child_results):
    gpu_child.report(case, child_results)
