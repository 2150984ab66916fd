"""GPU: connected components of pictures in slot layout (hvq_label_pictures / Context.label_pictures) and masks from labels
(hvq_select_components / Context.select_components) against hvqm4_amd.labels -- which tests/test_label_cpu.py holds equal to
tests/label_ref.py, the plain-Python restatement of include/hvqm4_amd.h -- compared with ==.  The planes and masks are
tests/label_cases.py's: the smallest planes, planes of a tile and of a tile and a step, 72 x 24 and 136 x 40 in the three samplings, the
seam shapes, rows of 8192, K against cap, 300 mixed pictures under 64 rules.  Every output is allocated with 256 sentinel bytes before
and behind it, which must stay untouched, and a record table is filled with the sentinel: rows beyond `stored` keep it.  status == 0 is
asserted in every header row.  The cases run in ONE child process that imports torch first (see tests/gpu_child.py); each test
reports its case.  The child stops at the first HVQ_E_HIP or HIP error: nothing more is started on a GPU that has reported a fault."""
import os
import sys

import numpy as np
import pytest

from tests import gpu_child
from tests.gpu_kit import GUARD, ROOT, SENTINEL, Uploaded as _Uploaded, decode as _decode, golden as _golden

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300                                 # the cases take seconds each; a hung child is ended, not waited for


# ------------------------------------------------------------------------------------------------------------- child side
def _room(torch, nbytes, dtype, shape):
    """a tensor of `shape` inside an allocation of its own filled with the sentinel, GUARD bytes before and behind it -> (tensor, guards)"""
    room = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    return room[GUARD:GUARD + nbytes].view(dtype).view(shape), [room[:GUARD], room[GUARD + nbytes:]]


def _label(torch, ctx, sids, ords, rules, cap, src=None, which=None):
    """one label_pictures into guarded rooms -> (labels, comps, guards)"""
    from hvqm4_amd import labels as L
    n = len(sids)
    table = rules if which is not None else None
    labs, comps, guards = [], [], []
    for i in range(n):
        r = table[which[i]] if table is not None else rules[i] if isinstance(rules, list) else rules
        ny, nx = L.plane_shape(ctx._geometry(sids[i]), r.plane)
        t, g = _room(torch, 4 * nx * ny, torch.int32, (ny, nx))
        c, h = _room(torch, 64 * (cap + 1), torch.int64, (cap + 1, 8))
        labs.append(t); comps.append(c); guards += g + h
    got = ctx.label_pictures(sids, ords, rules, which=which, cap=cap, src=src, labels=labs, comps=comps)
    assert got[0] is not None and all(a is b for a, b in zip(got[0], labs)) and all(a is b for a, b in zip(got[1], comps))
    return labs, comps, guards


def _check(torch, labs, comps, guards, wants, what):
    """wants[i] = hvqm4_amd.labels' (labels, records of stored + 1 rows)"""
    for g in guards:
        assert g.numel() == GUARD and bool(g.eq(SENTINEL).all()), f"{what}: the bytes around an output were written"
    assert len(labs) == len(wants) == len(comps), what
    filler = int(np.frombuffer(bytes([SENTINEL] * 8), dtype="<i8")[0])
    for i, (t, c, (wl, wr)) in enumerate(zip(labs, comps, wants)):
        label = what[i] if isinstance(what, list) else f"{what}: picture {i}"
        got = t.cpu().numpy().view(np.uint32)
        rec = c.cpu().numpy()
        print(f"{label}: K {rec[0, 0]} stored {rec[0, 1]} F {rec[0, 2]} status {rec[0, 3]}", flush=True)
        assert rec[0, 3] == 0, f"{label}: status {rec[0, 3]}"
        assert rec[0].tolist() == wr[0].tolist(), f"{label}: row 0 {rec[0].tolist()}, want {wr[0].tolist()}"
        if not np.array_equal(got, wl):
            bad = np.argwhere(got != wl)
            raise AssertionError(f"{label}: {bad.shape[0]} of {got.size} labels differ, first at (y, x) = {tuple(bad[0])}: got {got[tuple(bad[0])]}, want {wl[tuple(bad[0])]}")
        stored = wr.shape[0] - 1
        assert np.array_equal(rec[:stored + 1], wr), f"{label}: records differ: row {int(np.flatnonzero((rec[:stored + 1] != wr).any(axis=1))[0])}"
        assert (rec[stored + 1:] == filler).all(), f"{label}: a row beyond `stored` was written"


def _run_cases(torch, ctx, cs, cap=4096):
    """every case in ONE call, a rule per picture"""
    from hvqm4_amd import labels as L
    up = _Uploaded(torch, ctx, [c[2] for c in cs], [c[1] for c in cs])
    rules = [c[3] for c in cs]
    assert len(set(rules)) <= L.MAX_RULES
    labs, comps, guards = _label(torch, ctx, up.sids, [-1] * len(cs), rules, cap, src=up.bufs)
    torch.cuda.synchronize()
    _check(torch, labs, comps, guards, [L.of_picture(c[2], c[1], c[3], cap) for c in cs], [c[0] for c in cs])
    up.close()


def case_small(torch, ctx):
    """8 x 8 and 4 x 4 planes, planes of a tile and of a tile and a step, 72 x 24 and 136 x 40 in the three samplings with each plane:
    empty, full, checkerboards, random masks, windows; both neighbourhoods"""
    from tests import label_cases as cases
    _run_cases(torch, ctx, cases.small_cases())


def case_seams(torch, ctx):
    """the seam shapes over 3 x 3 and 3 x 3 chroma tiles: serpentines, a spiral, a comb, a U per tile column, diagonals, corner blobs"""
    from tests import label_cases as cases
    _run_cases(torch, ctx, cases.seam_cases())


def case_wide(torch, ctx):
    """rows of 8192 samples: one row of foreground through 128 tiles, and the serpentine"""
    from tests import label_cases as cases
    _run_cases(torch, ctx, cases.wide_cases(), cap=16)


def case_cap(torch, ctx):
    """K = 32 against cap 33, 32, 31 and 0: the map is complete, the rows beyond `stored` keep the sentinel"""
    from hvqm4_amd import labels as L
    from tests import label_cases as cases
    label, geom, pic, _r = cases.small_cases()[4]
    assert "check0" in label and geom == (8, 8, 2, 2)
    r = L.rule(connectivity=4)
    up = _Uploaded(torch, ctx, [pic], [geom])
    for cap in (33, 32, 31, 0):
        labs, comps, guards = _label(torch, ctx, up.sids, [-1], r, cap, src=up.bufs)
        torch.cuda.synchronize()
        want = L.of_picture(pic, geom, r, cap)
        assert want[1][0].tolist()[:2] == [32, min(32, cap)]
        _check(torch, labs, comps, guards, [want], f"cap {cap}")
    up.close()


def case_mixed(torch, ctx):
    """300 pictures of the small geometries under 64 rules in one call, through `which`"""
    from hvqm4_amd import labels as L
    from tests import label_cases as cases
    geoms, pics, rules, which = cases.mixed_cases()
    assert len(pics) == 300 and len(rules) == 64 and set(which) == set(range(64))
    up = _Uploaded(torch, ctx, pics, geoms)
    labs, comps, guards = _label(torch, ctx, up.sids, [-1] * 300, rules, 64, src=up.bufs, which=which)
    torch.cuda.synchronize()
    _check(torch, labs, comps, guards, [L.of_picture(p, g, rules[w], 64) for p, g, w in zip(pics, geoms, which)], "mixed")
    up.close()


def _select(torch, ctx, sids, labs, comps, sel, which=None):
    nb = [ctx.pic_bytes(s) for s in sids]
    rooms = [_room(torch, b, torch.uint8, (b,)) for b in nb]
    out = [r[0] for r in rooms]
    uniform = len({ctx._geometry(s) for s in set(sids)}) <= 1
    if uniform:
        room, guards = _room(torch, sum(nb), torch.uint8, (len(nb), nb[0]))
        got = ctx.select_components(sids, labs, comps, sel, which=which, out=room)
        assert got is room
        return [room[i] for i in range(len(nb))], guards
    got = ctx.select_components(sids, labs, comps, sel, which=which, out=out)
    return out, [g for r in rooms for g in r[1]]


def _check_bytes(torch, got, guards, wants, what):
    for g in guards:
        assert g.numel() == GUARD and bool(g.eq(SENTINEL).all()), f"{what}: the bytes around an output were written"
    for i, (g, w) in enumerate(zip(got, wants)):
        g = g.cpu().numpy()
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError(f"{what}: picture {i}: {bad.size} of {g.size} bytes differ, first at {bad[0]}: got {g[bad[0]]}, want {w[bad[0]]}")


def case_select(torch, ctx):
    """every range bound at its edge, invert, labels beyond `stored`, chroma 128; label -> select on one stream without a
    synchronisation between them, against of_select of the module's labels"""
    from hvqm4_amd import labels as L
    from tests import label_cases as cases
    geom = (136, 40, 2, 2)
    mask = np.zeros((40, 136), np.uint8)
    mask[1:4, 1:3] = 255; mask[1, 8:18] = 255; mask[6:16, 70] = 255; mask[10, 3] = 255; mask[20:38, 60:130] = 255
    mask[25:30, 62:66] = 0
    pics = [cases.picture(geom, 0, mask, 1), cases.picture(geom, 0, cases.spiral(136, 40), 2), cases.picture((72, 24, 2, 1), 0, cases.fill_masks(72, 24, 3)[5][1], 3)]
    geoms = [geom, geom, (72, 24, 2, 1)]
    up = _Uploaded(torch, ctx, pics, geoms)
    r = L.rule()
    sels = [L.select(), L.select(area=2), L.select(area=(6, 6)), L.select(area=(7, 9)), L.select(area=(None, 10)), L.select(width=(10, 10)), L.select(width=(None, 1)),
            L.select(width=11), L.select(height=(3, 10)), L.select(height=11), L.select(height=(None, 1)), L.select(area=2, invert=True), L.select(invert=True)]
    for cap in (64, 2):
        wants = [L.of_picture(p, g, r, cap) for p, g in zip(pics, geoms)]
        labs, comps, guards = _label(torch, ctx, up.sids, [-1] * 3, r, cap, src=up.bufs)
        outs = [_select(torch, ctx, up.sids, labs, comps, s) for s in sels]                       # no synchronisation in between
        which = [0, 11, 4]
        outw = _select(torch, ctx, up.sids, labs, comps, sels, which=which)
        torch.cuda.synchronize()
        _check(torch, labs, comps, guards, wants, f"select, cap {cap}")
        for s, (got, g) in zip(sels, outs):
            _check_bytes(torch, got, g, [L.of_select(w[0], w[1], s, gm) for w, gm in zip(wants, geoms)], f"cap {cap}, {s}")
        _check_bytes(torch, outw[0], outw[1], [L.of_select(w[0], w[1], sels[k], gm) for w, gm, k in zip(wants, geoms, which)], f"cap {cap}, which")
    up.close()


def case_chain(torch, ctx):
    """the golden clips through histograms -> Otsu tables -> map -> opening -> label -> select -> checksums in one stream without a host
    synchronisation, against the same chain of the Python modules"""
    from hvqm4_amd import histograms as H
    from hvqm4_amd import labels as L
    from hvqm4_amd import maps as M
    from hvqm4_amd import rank as R
    sel = L.select(area=4)
    steps = [R.luma_only(s) for s in R.opening(1)]
    for name, data, _hdr, _n in _golden():
        sid, hdr, n = _decode(ctx, data)
        g = (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)
        sids, ords = [sid] * n, list(range(n))
        mask = ctx.equalize_pictures(sids, ords, M.otsu())
        opened = ctx.morph_pictures(sids, [-1] * n, steps, src=[mask[i] for i in range(n)])
        for conn in (4, 8):
            r = L.rule(connectivity=conn)
            labs, comps, guards = _label(torch, ctx, sids, [-1] * n, r, 256, src=[opened[i] for i in range(n)])
            got, g2 = _select(torch, ctx, sids, labs, comps, sel)
            torch.cuda.synchronize()
            wants, bytes_ = [], []
            for k in range(n):
                p = ctx.read_picture(sid, k).reshape(-1)
                m = M.of_picture(p, g, M.from_lut(*M.tables_of_records(H.of_picture(p, *g), M.otsu())))
                w = L.of_picture(R.of_steps(m, g, steps), g, r, 256)
                wants.append(w); bytes_.append(L.of_select(w[0], w[1], sel, g))
            _check(torch, labs, comps, guards, wants, f"{name}, {conn}")
            _check_bytes(torch, got, g2, bytes_, f"{name}, {conn}: select")
        ctx.close_stream(sid)


def case_refusals(torch, ctx):
    """HVQ_E_ARG leaves every output untouched; n == 0 does nothing; the well-formed call right after works"""
    import ctypes as C
    from hvqm4_amd import labels as L
    from hvqm4_amd._lib import HVQ_E_ARG, HvqLabelRule, HvqSelect, lib
    from tests import label_cases as cases
    geom = (72, 24, 2, 2)
    pic = cases.picture(geom, 0, cases.fill_masks(72, 24, 1)[5][1], 9)
    up = _Uploaded(torch, ctx, [pic, pic], [geom, geom])
    cap = 8
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def rooms():
        labs = [torch.full((24, 72), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
        comps = [torch.full((cap + 1, 8), -1, dtype=torch.int64, device="cuda") for _ in range(2)]
        dst = [torch.full((ctx.pic_bytes(up.sids[0]),), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2)]
        return labs, comps, dst

    def arr(v):
        return C.cast((C.c_void_p * len(v))(*v), C.c_void_p)

    def raw_label(n=2, sids=None, ords=(-1, -1), src=None, rules=((0, 255, 255, 8),), nrules=None, which=None, cap_=cap, lab=None, cmp_=None, h=None):
        labs, comps, _d = rooms()
        a_r = (HvqLabelRule * len(rules))(*[HvqLabelRule(*r) for r in rules])
        src = [b.data_ptr() for b in up.bufs] if src is None else src
        rc = lib().hvq_label_pictures(ctx._h if h is None else h, n, (C.c_int * 2)(*(sids or up.sids)), (C.c_int * 2)(*ords), arr(src), C.cast(a_r, C.c_void_p),
                                      len(rules) if nrules is None else nrules, None if which is None else C.cast((C.c_int * 2)(*which), C.c_void_p),
                                      arr([t.data_ptr() for t in labs] if lab is None else lab), arr([t.data_ptr() for t in comps] if cmp_ is None else cmp_), cap_, stream)
        torch.cuda.synchronize()
        return rc, all(bool(t.eq(-1).all()) for t in labs + comps)
    ok = up.bufs[0].data_ptr()
    refused = [("bad stream", dict(sids=[up.sids[0], 99])), ("an ordinal with src", dict(ords=(-1, 0))), ("misaligned src", dict(src=[ok, ok + 8])),
               ("nrules 0", dict(nrules=0)), ("nrules 65", dict(rules=((0, 255, 255, 8),) * 65)), ("which beyond the rules", dict(which=[0, 1])),
               ("a negative which", dict(which=[-1, 0])), ("cap -1", dict(cap_=-1)), ("cap beyond the most", dict(cap_=(1 << 20) + 1)), ("null labels", dict(lab=[ok, 0])),
               ("misaligned labels", dict(lab=[ok, ok + 4])), ("null comps", dict(cmp_=[0, ok])), ("misaligned comps", dict(cmp_=[ok + 8, ok])),
               ("n beyond 65535", dict(n=65536)), ("negative n", dict(n=-1)), ("null context", dict(h=C.c_void_p(0)))]
    for bad in ((3, 0, 0, 8), (-1, 0, 0, 8), (0, 9, 8, 8), (0, -1, 8, 8), (0, 0, 256, 8), (0, 0, 0, 6)):
        refused.append((f"rule {bad} in an entry that no picture uses", dict(rules=((0, 255, 255, 8), bad), which=[0, 0])))
    for what, kw in refused:
        assert raw_label(**kw) == (HVQ_E_ARG, True), what
    assert raw_label(n=0) == (0, True), "n == 0 does nothing"
    rc, untouched = raw_label()
    assert rc == 0 and not untouched
    # select
    r = L.rule()
    labs, comps, _g = _label(torch, ctx, up.sids, [-1, -1], r, cap, src=up.bufs)

    def raw_select(n=2, sids=None, sel=((0, 9, 0, 9, 0, 9, 0, 0),), nsel=None, which=None, cap_=cap, lab=None, cmp_=None, dst=None, h=None):
        _l, _c, out = rooms()
        a_e = (HvqSelect * len(sel))(*[HvqSelect(*e) for e in sel])
        rc = lib().hvq_select_components(ctx._h if h is None else h, n, (C.c_int * 2)(*(sids or up.sids)), arr([t.data_ptr() for t in labs] if lab is None else lab),
                                         arr([t.data_ptr() for t in comps] if cmp_ is None else cmp_), cap_, C.cast(a_e, C.c_void_p), len(sel) if nsel is None else nsel,
                                         None if which is None else C.cast((C.c_int * 2)(*which), C.c_void_p), arr([t.data_ptr() for t in out] if dst is None else dst), stream)
        torch.cuda.synchronize()
        return rc, all(bool(t.eq(SENTINEL).all()) for t in out)
    good = (0, 9, 0, 9, 0, 9, 0, 0)
    refused = [("bad stream", dict(sids=[up.sids[0], 99])), ("nsel 0", dict(nsel=0)), ("nsel 65", dict(sel=(good,) * 65)), ("which beyond", dict(which=[0, 1])),
               ("cap -1", dict(cap_=-1)), ("null labels", dict(lab=[0, ok])), ("misaligned comps", dict(cmp_=[ok, ok + 8])), ("null dst", dict(dst=[ok, 0])),
               ("misaligned dst", dict(dst=[ok + 4, ok])), ("n beyond 65535", dict(n=65536)), ("null context", dict(h=C.c_void_p(0)))]
    for bad in ((5, 4, 0, 9, 0, 9, 0, 0), (0, 9, 3, 2, 0, 9, 0, 0), (0, 9, 0, 9, 9, 0, 0, 0), (0, 9, 0, 9, 0, 9, 2, 0), (0, 9, 0, 9, 0, 9, 0, 1)):
        refused.append((f"selection {bad} in an entry that no picture uses", dict(sel=(good, bad), which=[0, 0])))
    for what, kw in refused:
        assert raw_select(**kw) == (HVQ_E_ARG, True), what
    assert raw_select(n=0) == (0, True), "n == 0 does nothing"
    rc, untouched = raw_select()
    assert rc == 0 and not untouched
    up.close()


def case_tools(torch, ctx):
    """tools/objects.py on a golden clip: the printed facts and the files of the selected masks, against the same chain of the modules"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import objects
    from hvqm4_amd import histograms as H
    from hvqm4_amd import jpeg
    from hvqm4_amd import labels as L
    from hvqm4_amd import maps as M
    from hvqm4_amd import rank as R
    from oracle import bridge
    data = open(os.path.join(ROOT, "tests", "golden", "yuv422_64x48.h4m"), "rb").read()
    g = (64, 48, 2, 1)
    geom, facts, files = objects.clip_objects(ctx, data, min_area=6, opening=1, connectivity=4, quality=80)
    assert geom == g and len(facts) == len(files) > 0
    pics = bridge.oracle_decode(data, len(files))
    rule = M.Rule(M.otsu().luma, M.flat(128).luma)
    for k, f in enumerate(files):
        p = pics[k].reshape(-1)
        mask = M.of_picture(p, g, M.from_lut(*M.tables_of_records(H.of_picture(p, *g), rule)))
        lab, rec = L.of_picture(R.of_steps(mask, g, [R.luma_only(s) for s in R.opening(1)]), g, L.rule(connectivity=4), objects.CAP)
        rc = L.records(rec)
        assert facts[k] == (rc.K, rc.F, [tuple(int(v) for v in rc.rows[j - 1, :5]) for j in L.largest(rc, 3)]), k
        assert f == jpeg.encode(L.of_select(lab, rec, L.select(area=6), g), 64, 48, 80, 2, 1), k
    geom, facts2, none = objects.clip_objects(ctx, data, opening=1, connectivity=4, files=False)
    assert none is None and facts2 == facts


CASES = ["small", "seams", "wide", "cap", "mixed", "select", "chain", "refusals", "tools"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "label", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_label(case, child_results):
    gpu_child.report(case, child_results)
