"""GPU: summed-area tables of pictures in slot layout (hvq_integral_pictures / Context.integral_pictures), local means, deviations and
thresholds from them (hvq_window_pictures / Context.window_pictures, Context.adaptive_pictures) and sums of rectangles in device memory
(hvq_rect_sums / Context.rect_sums) against hvqm4_amd.integral -- which tests/test_integral_cpu.py holds equal to tests/integral_ref.py,
the plain-Python restatement of include/hvqm4_amd.h -- compared with ==.  The planes, rules and rectangles are tests/integral_cases.py's:
4 x 4, 8 x 4, one chunk of the row pass, a chunk and a dword (which is a column group and 4), 72 x 24 in the three samplings with each
plane, 8192 x 8 for the carry across 32 chunks, the window's tile and planes past its seams, the checkerboard, all 0, all 255, random
planes; every window of the list under every mode, k, c and invert; 60 mixed pictures under 64 rules; 300 rectangles; and the 8192 x 2064
plane of 255 whose table wraps.  Every output is allocated with 256 sentinel bytes before and behind it, which must stay untouched.  The
cases run in ONE child process that imports torch first (see tests/gpu_child.py); each test reports its case.  The child stops at
the first HVQ_E_HIP or HIP error: nothing more is started on a GPU that has reported a fault."""
import json
import os
import sys

import numpy as np
import pytest

from tests import gpu_child
from tests.gpu_kit import GUARD, ROOT, SENTINEL, Uploaded as _uploaded, decode as _decode, golden as _golden

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300                                 # the cases take seconds each; a hung child is ended, not waited for


# ------------------------------------------------------------------------------------------------------------- child side
def _room(torch, nbytes, dtype, shape):
    """a tensor of `shape` inside an allocation of its own filled with the sentinel, GUARD bytes before and behind it -> (tensor, guards)"""
    room = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    return room[GUARD:GUARD + nbytes].view(dtype).view(shape), [room[:GUARD], room[GUARD + nbytes:]]


def _guards(guards, what):
    for g in guards:
        assert g.numel() == GUARD and bool(g.eq(SENTINEL).all()), f"{what}: the bytes around an output were written"


def _integral(torch, ctx, sids, ords, planes, squares=True, src=None):
    """one integral_pictures into guarded rooms -> (sums, squares or None, guards)"""
    from hvqm4_amd.labels import plane_shape
    sums, sq, guards = [], [], []
    for i in range(len(sids)):
        ny, nx = plane_shape(ctx._geometry(sids[i]), planes[i])
        t, g = _room(torch, 4 * nx * ny, torch.int32, (ny, nx))
        sums.append(t); guards += g
        if squares:
            t, g = _room(torch, 8 * nx * ny, torch.int64, (ny, nx))
            sq.append(t); guards += g
    got = ctx.integral_pictures(sids, ords, planes, squares=squares, src=src, out=(sums, sq if squares else None))
    assert all(a is b for a, b in zip(got[0], sums)) and (got[1] is None) == (not squares)
    return sums, (sq if squares else None), guards


def _window(torch, ctx, sids, ords, sums, squares, rules, which=None, src=None):
    nb = [ctx.pic_bytes(s) for s in sids]
    if len({ctx._geometry(s) for s in set(sids)}) <= 1:
        room, guards = _room(torch, sum(nb), torch.uint8, (len(nb), nb[0]))
        assert ctx.window_pictures(sids, ords, sums, squares, rules, which=which, src=src, out=room) is room
        return [room[i] for i in range(len(nb))], guards
    rooms = [_room(torch, b, torch.uint8, (b,)) for b in nb]
    out = [r[0] for r in rooms]
    ctx.window_pictures(sids, ords, sums, squares, rules, which=which, src=src, out=out)
    return out, [g for r in rooms for g in r[1]]


def _check_tables(sums, squares, guards, wants, what):
    _guards(guards, what if isinstance(what, str) else "tables")
    for i, (S, Q) in enumerate(wants):
        label = what[i] if isinstance(what, list) else f"{what}: picture {i}"
        got = sums[i].cpu().numpy().view(np.uint32)
        if not np.array_equal(got, S):
            bad = np.argwhere(got != S)
            raise AssertionError(f"{label}: {bad.shape[0]} of {got.size} sums differ, first at (y, x) = {tuple(bad[0])}: got {got[tuple(bad[0])]}, want {S[tuple(bad[0])]}")
        if squares is not None and Q is not None:
            gq = squares[i].cpu().numpy().view(np.uint64)
            if not np.array_equal(gq, Q):
                bad = np.argwhere(gq != Q)
                raise AssertionError(f"{label}: {bad.shape[0]} of {gq.size} sums of squares differ, first at (y, x) = {tuple(bad[0])}")


def _check_bytes(got, guards, wants, what):
    _guards(guards, what if isinstance(what, str) else "pictures")
    for i, (g, w) in enumerate(zip(got, wants)):
        g = g.cpu().numpy()
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            label = what[i] if isinstance(what, list) else f"{what}: picture {i}"
            raise AssertionError(f"{label}: {bad.size} of {g.size} bytes differ, first at {bad[0]}: got {g[bad[0]]}, want {w[bad[0]]}")


def case_tables(torch, ctx):
    """the tables of every plane of the list, with and without squares, and 8192 x 8: the carry across 32 chunks"""
    from hvqm4_amd import integral as I
    from hvqm4_amd import labels as L
    from tests import integral_cases as cases
    cs = cases.table_cases() + cases.wide_cases()
    up = _uploaded(torch, ctx, [c[2] for c in cs], [c[1] for c in cs])
    planes = [c[3] for c in cs]
    wants = [I.of_plane(L.plane_of(c[2], c[1], c[3])) for c in cs]
    sums, squares, guards = _integral(torch, ctx, up.sids, [-1] * len(cs), planes, src=up.bufs)
    alone, none, g2 = _integral(torch, ctx, up.sids, [-1] * len(cs), planes, squares=False, src=up.bufs)
    torch.cuda.synchronize()
    _check_tables(sums, squares, guards, wants, [c[0] for c in cs])
    _check_tables(alone, none, g2, wants, [c[0] + ", sums alone" for c in cs])
    up.close()


def case_windows(torch, ctx):
    """every window of the list under every mode, k, c and invert on the window planes and fills; integral -> window on one stream
    without a synchronisation; 64 distinct rules a call"""
    from hvqm4_amd import integral as I
    from tests import integral_cases as cases
    cs = cases.window_cases()
    assert {(c[3].mode, c[3].k, c[3].c, c[3].invert) for c in cs} == set(cases.SPECS) and {(c[3].rx, c[3].ry) for c in cs} == set(cases.WINDOWS)
    up = _uploaded(torch, ctx, [c[2] for c in cs], [c[1] for c in cs])
    sums, squares, guards = _integral(torch, ctx, up.sids, [-1] * len(cs), [c[3].plane for c in cs], src=up.bufs)
    calls, seen = [[]], set()
    for i, c in enumerate(cs):
        if c[3] not in seen and len(seen) == I.MAX_RULES:
            calls.append([])
            seen = set()
        seen.add(c[3])
        calls[-1].append(i)
    outs = {}
    for idx in calls:
        got, g = _window(torch, ctx, [up.sids[i] for i in idx], [-1] * len(idx), [sums[i] for i in idx], [squares[i] if I.needs_squares(cs[i][3]) else None for i in idx],
                         [cs[i][3] for i in idx], src=[up.bufs[i] for i in idx])
        guards += g
        outs.update(zip(idx, got))
    torch.cuda.synchronize()
    _check_bytes([outs[i] for i in range(len(cs))], guards, [I.of_picture(c[2], c[1], c[3]) for c in cs], [c[0] for c in cs])
    up.close()


def case_mixed(torch, ctx):
    """60 pictures of the window geometries under 64 rules in one call, through `which`; adaptive_pictures gives the same"""
    from hvqm4_amd import integral as I
    from tests import integral_cases as cases
    geoms, pics, rules, which = cases.mixed_cases()
    assert len(pics) == 60 and len(rules) == 64 and len(set(which)) == 60
    up = _uploaded(torch, ctx, pics, geoms)
    sums, squares, guards = _integral(torch, ctx, up.sids, [-1] * 60, [0] * 60, src=up.bufs)
    got, g = _window(torch, ctx, up.sids, [-1] * 60, sums, squares, rules, which=which, src=up.bufs)
    again = ctx.adaptive_pictures(up.sids, [-1] * 60, rules, which=which, src=up.bufs)
    torch.cuda.synchronize()
    wants = [I.of_picture(p, gm, rules[w]) for p, gm, w in zip(pics, geoms, which)]
    _check_bytes(got, guards + g, wants, "mixed")
    _check_bytes(again, [], wants, "mixed, adaptive_pictures")
    up.close()


def case_rects(torch, ctx):
    """300 rectangles in device memory over six pictures, the last without a table of squares: single samples, whole planes, random
    ones and one of each refused kind"""
    from hvqm4_amd import integral as I
    from hvqm4_amd import labels as L
    from tests import integral_cases as cases
    geoms, pics, planes, rects = cases.rect_cases()
    up = _uploaded(torch, ctx, pics, geoms)
    sums, squares, guards = _integral(torch, ctx, up.sids, [-1] * len(pics), planes, src=up.bufs)
    squares[-1] = None
    out, g = _room(torch, 24 * len(rects), torch.int64, (len(rects), 3))
    assert ctx.rect_sums(torch.from_numpy(rects).cuda(), sums, squares, out=out) is out
    torch.cuda.synchronize()
    _guards(guards + g, "rects")
    tables = [I.of_plane(L.plane_of(p, gm, pl), squares=i != len(pics) - 1) for i, (p, gm, pl) in enumerate(zip(pics, geoms, planes))]
    want = I.of_rects(rects, tables)
    got = out.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want), f"rectangles {np.flatnonzero((got != want).any(axis=1))[:8].tolist()} differ"
    assert int((want[:, 0] == 0).sum()) == 10
    up.close()


def case_wrap(torch, ctx):
    """the 8192 x 2064 plane of 255 through src=: S(Nx - 1, Ny - 1) = 4 311 613 440 mod 2^32 = 16 646 144, and the rectangle of 16 572 416
    samples still comes out exact; the whole plane, more than 2^24 samples, gives (0, 0, 0)"""
    from tests import integral_cases as cases
    g = cases.WRAP
    sid = ctx.open_stream(g[0], g[1], g[2], g[3], True, 3)
    pic = torch.full((cases.nbytes(g),), 255, dtype=torch.uint8, device="cuda")
    sums, squares, guards = _integral(torch, ctx, [sid], [-1], [0], src=[pic])
    rects = torch.tensor([(0, 100, 10, 8191, 2057), (0, 0, 0, 8191, 2063), (0, 0, 0, 8191, 2047), (1, 0, 0, 1, 1)], dtype=torch.int32).cuda()
    out = ctx.rect_sums(rects, sums, squares)
    torch.cuda.synchronize()
    _guards(guards, "wrap")
    assert int(sums[0][-1, -1]) & 0xFFFFFFFF == 16646144 and int(squares[0][-1, -1]) == 255 * 255 * 8192 * 2064
    assert out.cpu().tolist() == [[16572416, 255 * 16572416, 255 * 255 * 16572416], [0, 0, 0], [1 << 24, 255 << 24, 255 * 255 << 24], [0, 0, 0]]
    xs = np.arange(1, 8193, dtype=np.uint64)
    host = sums[0].cpu().numpy().view(np.uint32)
    ys = np.arange(1, 2065, dtype=np.uint64)
    assert np.array_equal(host, ((ys[:, None] * xs[None, :] * np.uint64(255)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)), "the wrapped table differs"
    ctx.close_stream(sid)


def case_chain(torch, ctx):
    """the golden clips through histograms -> adaptive_pictures -> morph_pictures -> label_pictures(src=) -> rects_of_boxes -> rect_sums,
    against the modules; the tables and a window against the fixture; one stream, no host synchronisation in between"""
    import zlib
    from hvqm4_amd import histograms as H
    from hvqm4_amd import integral as I
    from hvqm4_amd import labels as L
    from hvqm4_amd import rank as R
    fixture = json.load(open(os.path.join(ROOT, "tests", "golden", "integral.json")))
    rule = I.adaptive(5, c=7, k=51)
    assert fixture["windows"]["adaptive_5_c7_k51"] == [rule.mode, rule.rx, rule.ry, rule.k, rule.c, rule.invert]
    steps = [R.luma_only(s) for s in R.opening(1)]
    cap = 64
    seen = 0
    for name, data, _hdr, _n in _golden():
        sid, hdr, n = _decode(ctx, data)
        g = (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)
        sids, ords = [sid] * n, list(range(n))
        hist = ctx.picture_histograms(sids, ords)
        sums, squares, guards = _integral(torch, ctx, sids, ords, [0] * n)
        mask = ctx.adaptive_pictures(sids, ords, rule)
        opened = ctx.morph_pictures(sids, [-1] * n, steps, src=[mask[i] for i in range(n)])
        labs, comps = ctx.label_pictures(sids, [-1] * n, L.rule(), cap=cap, src=[opened[i] for i in range(n)])
        rects = I.rects_of_boxes(comps)
        out = ctx.rect_sums(rects, sums, squares)
        torch.cuda.synchronize()
        pics = ctx.read_pictures(sids, ords)
        assert np.array_equal(hist.cpu().numpy(), np.stack([H.of_picture(pics[k], *g) for k in range(n)])), f"{name}: histograms"
        tables = [I.of_plane(L.plane_of(pics[k], g, 0)) for k in range(n)]
        _check_tables(sums, squares, guards, tables, name)
        wants = [I.of_picture(pics[k], g, rule) for k in range(n)]
        _check_bytes([mask[k] for k in range(n)], [], wants, f"{name}: adaptive")
        if name in fixture["clips"]:
            want = fixture["clips"][name]
            assert zlib.crc32(sums[0].cpu().numpy().view(np.uint32).astype("<u4").tobytes()) == want["sums"], name
            assert zlib.crc32(squares[0].cpu().numpy().view(np.uint64).astype("<u8").tobytes()) == want["squares"], name
            assert zlib.crc32(mask[0].cpu().numpy().tobytes()) == want["adaptive_5_c7_k51"], name
            seen += 1
        host_rects = []
        for k in range(n):
            cur = wants[k]
            for s in steps:
                cur = R.of_picture(cur, g, s)
            assert np.array_equal(opened[k].cpu().numpy(), cur), f"{name}: opening, {k}"
            lab, rec = L.of_picture(cur, g, L.rule(), cap)
            assert np.array_equal(labs[k].cpu().numpy().view(np.uint32), lab) and np.array_equal(comps[k].cpu().numpy()[:rec.shape[0]], rec), f"{name}: labels, {k}"
            table = np.zeros((cap + 1, 8), np.int64)
            table[:rec.shape[0]] = rec
            host_rects.append(table)
        want_rects = I.rects_of_boxes(host_rects)
        assert np.array_equal(rects.cpu().numpy(), want_rects), f"{name}: rectangles of the boxes"
        assert np.array_equal(out.cpu().numpy().view(np.uint64), I.of_rects(want_rects, tables)), f"{name}: sums of the boxes"
        ctx.close_stream(sid)
    assert seen > 0


def case_refusals(torch, ctx):
    """HVQ_E_ARG leaves every output untouched; n == 0 does nothing; the well-formed call right after works"""
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, HvqWindowRule, lib
    from tests import integral_cases as cases
    geom = (72, 24, 2, 2)
    pic = cases.picture(geom, 0, cases.fills(72, 24, 1)[3][1], 9)
    up = _uploaded(torch, ctx, [pic, pic], [geom, geom])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nb = ctx.pic_bytes(up.sids[0])

    def rooms():
        return ([torch.full((24, 72), -7, dtype=torch.int32, device="cuda") for _ in range(2)], [torch.full((24, 72), -7, dtype=torch.int64, device="cuda") for _ in range(2)],
                [torch.full((nb,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2)], torch.full((4, 3), -7, dtype=torch.int64, device="cuda"))

    def untouched(r):
        torch.cuda.synchronize()
        return all(bool(t.eq(-7).all()) for t in r[0] + r[1] + [r[3]]) and all(bool(t.eq(SENTINEL).all()) for t in r[2])

    def arr(v):
        return C.cast((C.c_void_p * len(v))(*v), C.c_void_p)

    def ints(v):
        return None if v is None else C.cast((C.c_int * len(v))(*v), C.c_void_p)
    ok = up.bufs[0].data_ptr()
    srcs = [b.data_ptr() for b in up.bufs]

    def raw_integral(n=2, sids=None, ords=(-1, -1), src=None, planes=None, sums=None, squares=None, h=None):
        r = rooms()
        rc = lib().hvq_integral_pictures(ctx._h if h is None else h, n, (C.c_int * 2)(*(sids or up.sids)), (C.c_int * 2)(*ords), arr(srcs if src is None else src), ints(planes),
                                         arr([t.data_ptr() for t in r[0]] if sums is None else sums), arr([t.data_ptr() for t in r[1]] if squares is None else squares), stream)
        return rc, untouched(r)
    refused = [("bad stream", dict(sids=[up.sids[0], 99])), ("an ordinal with src", dict(ords=(-1, 0))), ("misaligned src", dict(src=[ok, ok + 8])), ("plane 3", dict(planes=[0, 3])),
               ("a negative plane", dict(planes=[-1, 0])), ("null table", dict(sums=[ok, 0])), ("misaligned table", dict(sums=[ok, ok + 4])), ("misaligned squares", dict(squares=[ok, ok + 8])),
               ("n beyond 65535", dict(n=65536)), ("negative n", dict(n=-1)), ("null context", dict(h=C.c_void_p(0)))]
    for what, kw in refused:
        assert raw_integral(**kw) == (HVQ_E_ARG, True), what
    assert raw_integral(n=0) == (0, True), "n == 0 does nothing"
    rc, same = raw_integral()
    assert rc == 0 and not same
    sums, squares, _g = _integral(torch, ctx, up.sids, [-1, -1], [0, 0], src=up.bufs)
    good = (0, 2, 5, 5, 51, 7, 0, 0)

    def raw_window(n=2, sids=None, ords=(-1, -1), src=None, sums_=None, squares_="given", rules=(good,), nrules=None, which=None, dst=None, h=None):
        r = rooms()
        a_r = (HvqWindowRule * len(rules))(*[HvqWindowRule(*e) for e in rules])
        sq = arr([t.data_ptr() for t in squares]) if squares_ == "given" else None if squares_ is None else arr(squares_)
        rc = lib().hvq_window_pictures(ctx._h if h is None else h, n, (C.c_int * 2)(*(sids or up.sids)), (C.c_int * 2)(*ords), arr(srcs if src is None else src),
                                       arr([t.data_ptr() for t in sums] if sums_ is None else sums_), sq, C.cast(a_r, C.c_void_p), len(rules) if nrules is None else nrules,
                                       ints(which), arr([t.data_ptr() for t in r[2]] if dst is None else dst), stream)
        return rc, untouched(r)
    refused = [("bad stream", dict(sids=[up.sids[0], 99])), ("an ordinal with src", dict(ords=(-1, 0))), ("misaligned src", dict(src=[ok, ok + 8])), ("nrules 0", dict(nrules=0)),
               ("nrules 65", dict(rules=(good,) * 65)), ("which beyond the rules", dict(which=[0, 1])), ("a negative which", dict(which=[-1, 0])), ("null table", dict(sums_=[0, ok])),
               ("misaligned table", dict(sums_=[ok, ok + 8])), ("misaligned squares", dict(squares_=[ok, ok + 8])), ("squares needed", dict(squares_=None)),
               ("squares needed by one", dict(squares_=[squares[0].data_ptr(), 0])), ("null dst", dict(dst=[ok, 0])), ("misaligned dst", dict(dst=[ok + 4, ok])),
               ("a plane that has not the size of Y", dict(rules=((1, 0, 1, 1, 0, 0, 0, 0),))), ("n beyond 65535", dict(n=65536)), ("null context", dict(h=C.c_void_p(0)))]
    for bad in ((3, 0, 1, 1, 0, 0, 0, 0), (0, 3, 1, 1, 0, 0, 0, 0), (0, 0, 8192, 1, 0, 0, 0, 0), (0, 0, 1, -1, 0, 0, 0, 0), (0, 2, 1, 1, 1025, 0, 0, 0), (0, 2, 1, 1, 0, -256, 0, 0),
                (0, 2, 1, 1, 0, 0, 2, 0), (0, 0, 1, 1, 0, 0, 0, 1)):
        refused.append((f"rule {bad} in an entry that no picture uses", dict(rules=(good, bad), which=[0, 0])))
    for what, kw in refused:
        assert raw_window(**kw) == (HVQ_E_ARG, True), what
    assert raw_window(n=0) == (0, True), "n == 0 does nothing"
    rc, same = raw_window()
    assert rc == 0 and not same
    rects = torch.tensor([(0, 0, 0, 3, 3), (1, 0, 0, 3, 3), (0, 1, 1, 2, 2), (1, 1, 1, 2, 2)], dtype=torch.int32).cuda()
    dims = torch.tensor([(72, 24), (72, 24)], dtype=torch.int32).cuda()

    def raw_rects(n=2, nrects=4, rects_=None, sums_=None, squares_=None, dims_=None, out=None, h=None):
        r = rooms()
        rc = lib().hvq_rect_sums(ctx._h if h is None else h, n, nrects, C.c_void_p(rects.data_ptr() if rects_ is None else rects_), arr([t.data_ptr() for t in sums] if sums_ is None else sums_),
                                 arr([t.data_ptr() for t in squares] if squares_ is None else squares_), C.c_void_p(dims.data_ptr() if dims_ is None else dims_),
                                 C.c_void_p(r[3].data_ptr() if out is None else out), stream)
        return rc, untouched(r)
    for what, kw in [("n 0", dict(n=0)), ("n beyond 65535", dict(n=65536)), ("negative nrects", dict(nrects=-1)), ("too many rectangles", dict(nrects=(1 << 24) + 1)),
                     ("null rects", dict(rects_=0)), ("misaligned rects", dict(rects_=rects.data_ptr() + 2)), ("null dims", dict(dims_=0)), ("misaligned dims", dict(dims_=dims.data_ptr() + 1)),
                     ("misaligned out", dict(out=ok + 4)), ("null table", dict(sums_=[ok, 0])), ("misaligned table", dict(sums_=[ok + 4, ok])), ("misaligned squares", dict(squares_=[ok, ok + 8])),
                     ("null context", dict(h=C.c_void_p(0)))]:
        assert raw_rects(**kw) == (HVQ_E_ARG, True), what
    assert raw_rects(nrects=0) == (0, True), "no rectangles: nothing is done"
    rc, same = raw_rects()
    assert rc == 0 and not same
    up.close()


def case_tools(torch, ctx):
    """tools/adaptive.py on a golden clip: the shares and the files, against the same chain of the modules"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import adaptive
    from hvqm4_amd import integral as I
    from hvqm4_amd import jpeg
    from hvqm4_amd import rank as R
    from oracle import bridge
    data = open(os.path.join(ROOT, "tests", "golden", "yuv422_64x48.h4m"), "rb").read()
    g = (64, 48, 2, 1)
    geom, shares, files = adaptive.clip_adaptive(ctx, data, radius=9, c=5, k=-51, opening=1, quality=80)
    assert geom == g and len(shares) == len(files) > 0
    pics = bridge.oracle_decode(data, len(files))
    for k, f in enumerate(files):
        cur = I.of_picture(pics[k].reshape(-1), g, I.adaptive(9, c=5, k=-51))
        for s in R.opening(1):
            cur = R.of_picture(cur, g, R.luma_only(s))
        assert f == jpeg.encode(cur, 64, 48, 80, 2, 1), k
        assert abs(shares[k] - float((cur[:64 * 48] == 255).mean())) < 1e-6, k
    _g, shares2, none = adaptive.clip_adaptive(ctx, data, radius=9, c=5, k=-51, opening=1, files=False)
    assert none is None and shares2 == shares


CASES = ["tables", "windows", "mixed", "rects", "wrap", "chain", "refusals", "tools"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "integral", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_integral(case, child_results):
    gpu_child.report(case, child_results)
