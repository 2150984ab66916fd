"""GPU: exact distance transforms of pictures in slot layout (hvq_distance_pictures / Context.distance_pictures), masks from distances
(hvq_distance_mask / Context.distance_mask) and disc morphology (Context.disc_morph) against hvqm4_amd.distance -- which
tests/test_distance_cpu.py holds equal to tests/distance_ref.py, the plain-Python restatement of include/hvqm4_amd.h -- compared with ==.
The planes and masks are tests/distance_cases.py's: the smallest planes, planes just past a column group, a row group and a mask tile,
72 x 24 in the three samplings with each plane, rows of 8192, one background sample in a corner of 200 x 136, every metric under both
borders, 60 mixed pictures under 64 rules.  Every output is allocated with 256 sentinel bytes before and behind it, which must stay
untouched.  The cases run in ONE child process that imports torch first (see tests/gpu_child.py); each test reports its case.  The
child stops at the first HVQ_E_HIP or HIP error: nothing more is started on a GPU that has reported a fault."""
import json
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


def _distance(torch, ctx, sids, ords, rules, src=None, which=None):
    """one distance_pictures into guarded rooms -> (maps, guards)"""
    from hvqm4_amd import distance as D
    maps, guards = [], []
    for i in range(len(sids)):
        r = rules[which[i]] if which is not None else rules[i] if isinstance(rules, list) else rules
        ny, nx = D.plane_shape(ctx._geometry(sids[i]), r.plane)
        t, g = _room(torch, 4 * nx * ny, torch.int32, (ny, nx))
        maps.append(t); guards += g
    got = ctx.distance_pictures(sids, ords, rules, which=which, src=src, out=maps)
    assert all(a is b for a, b in zip(got, maps))
    return maps, guards


def _guards(guards, what):
    for g in guards:
        assert g.numel() == GUARD and bool(g.eq(SENTINEL).all()), f"{what}: the bytes around an output were written"


def _check(torch, maps, guards, wants, what):
    _guards(guards, what if isinstance(what, str) else "cases")
    assert len(maps) == len(wants), what
    for i, (t, want) in enumerate(zip(maps, wants)):
        label = what[i] if isinstance(what, list) else f"{what}: picture {i}"
        got = t.cpu().numpy().view(np.uint32)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError(f"{label}: {bad.shape[0]} of {got.size} distances differ, first at (y, x) = {tuple(bad[0])}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")


def _run_cases(torch, ctx, cs):
    """every case, a rule per picture, in as few calls as their distinct rules allow (64 a call)"""
    from hvqm4_amd import distance as D
    up = _Uploaded(torch, ctx, [c[2] for c in cs], [c[1] for c in cs])
    calls, seen = [[]], set()
    for i, c in enumerate(cs):
        if c[3] not in seen and len(seen) == D.MAX_RULES:
            calls.append([])
            seen = set()
        seen.add(c[3])
        calls[-1].append(i)
    maps, guards = [], []
    for idx in calls:
        m, g = _distance(torch, ctx, [up.sids[i] for i in idx], [-1] * len(idx), [cs[i][3] for i in idx], src=[up.bufs[i] for i in idx])
        maps += m; guards += g
    torch.cuda.synchronize()
    _check(torch, maps, guards, [D.of_picture(c[2], c[1], c[3]) for c in cs], [c[0] for c in cs])
    up.close()


def case_small(torch, ctx):
    """8 x 8 and 4 x 4, 16 x 8 and 24 x 16 planes: empty, full, a checkerboard, one background sample in each corner, one foreground
    sample, stripes, random masks, windows; every metric under both borders"""
    from tests import distance_cases as cases
    _run_cases(torch, ctx, cases.small_cases())


def case_tiles(torch, ctx):
    """72 x 24 in the three samplings with each plane, a column group and a step, a row group and a step, two row groups exactly"""
    from tests import distance_cases as cases
    _run_cases(torch, ctx, cases.tile_cases())


def case_far(torch, ctx):
    """200 x 136 with its only background sample in a corner: the longest outward walks"""
    from tests import distance_cases as cases
    _run_cases(torch, ctx, cases.far_cases())


def case_wide(torch, ctx):
    """rows of 8192 samples: a row group is one row"""
    from tests import distance_cases as cases
    _run_cases(torch, ctx, cases.wide_cases())


def case_mixed(torch, ctx):
    """60 pictures of the small geometries under 64 rules in one call, through `which`"""
    from hvqm4_amd import distance as D
    from tests import distance_cases as cases
    geoms, pics, rules, which = cases.mixed_cases()
    assert len(pics) == 60 and len(rules) == 64 and len(set(which)) == 60
    up = _Uploaded(torch, ctx, pics, geoms)
    maps, guards = _distance(torch, ctx, up.sids, [-1] * 60, rules, src=up.bufs, which=which)
    torch.cuda.synchronize()
    _check(torch, maps, guards, [D.of_picture(p, g, rules[w]) for p, g, w in zip(pics, geoms, which)], "mixed")
    up.close()


def _mask(torch, ctx, sids, maps, m, which=None):
    nb = [ctx.pic_bytes(s) for s in sids]
    if len({ctx._geometry(s) for s in set(sids)}) <= 1:
        room, guards = _room(torch, sum(nb), torch.uint8, (len(nb), nb[0]))
        assert ctx.distance_mask(sids, maps, m, which=which, out=room) is room
        return [room[i] for i in range(len(nb))], guards
    rooms = [_room(torch, b, torch.uint8, (b,)) for b in nb]
    out = [r[0] for r in rooms]
    ctx.distance_mask(sids, maps, m, which=which, out=out)
    return out, [g for r in rooms for g in r[1]]


def _check_bytes(torch, got, guards, wants, what):
    _guards(guards, what)
    for i, (g, w) in enumerate(zip(got, wants)):
        g = g.cpu().numpy()
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError(f"{what}: picture {i}: {bad.size} of {g.size} bytes differ, first at {bad[0]}: got {g[bad[0]]}, want {w[bad[0]]}")


def case_mask(torch, ctx):
    """both modes, the range's bounds at their edges, invert, NONE, chroma 128; distance -> mask on one stream without a synchronisation
    between them, against of_mask of the module's distances; and a made map with ROOT's last steps"""
    from hvqm4_amd import distance as D
    from tests import distance_cases as cases
    geom = (136, 40, 2, 2)
    pics = [cases.picture(geom, 0, cases.mask_picture(), 1), cases.picture(geom, 0, np.full((40, 136), 255, np.uint8), 2),
            cases.picture((72, 24, 2, 1), 0, cases.fill_masks(72, 24, 3)[12][1], 3)]
    geoms = [geom, geom, (72, 24, 2, 1)]
    up = _Uploaded(torch, ctx, pics, geoms)
    r = D.rule()
    wants = [D.of_picture(p, g, r) for p, g in zip(pics, geoms)]
    assert (wants[1] == D.NONE).all()
    maps, guards = _distance(torch, ctx, up.sids, [-1] * 3, r, src=up.bufs)
    outs = [_mask(torch, ctx, up.sids, maps, m) for m in cases.MASKS]                                # no synchronisation in between
    which = [0, 10, 4]
    outw = _mask(torch, ctx, up.sids, maps, cases.MASKS, which=which)
    torch.cuda.synchronize()
    _check(torch, maps, guards, wants, "mask")
    for m, (got, g) in zip(cases.MASKS, outs):
        _check_bytes(torch, got, g, [D.of_mask(w, m, gm) for w, gm in zip(wants, geoms)], f"{m}")
    _check_bytes(torch, outw[0], outw[1], [D.of_mask(w, cases.MASKS[k], gm) for w, gm, k in zip(wants, geoms, which)], "which")
    made = np.arange(136 * 40, dtype=np.int64).reshape(40, 136) * 13 % (1 << 17)
    made[0, :6] = [0, 1, 255 * 255 - 1, 255 * 255, 2 ** 27, D.NONE]
    t = torch.from_numpy(made.astype(np.uint32).view(np.int32)).cuda()
    got, g = _mask(torch, ctx, up.sids[:1], [t], D.mask_root())
    torch.cuda.synchronize()
    _check_bytes(torch, got, g, [D.of_mask(made, D.mask_root(), geom)], "root of a made map")
    up.close()


def case_morph(torch, ctx):
    """disc_morph: erosions, dilations, openings and closings by discs of several radii, src= to src=, against of_steps"""
    from hvqm4_amd import distance as D
    from tests import distance_cases as cases
    geoms = [(72, 24, 2, 2)] * 5 + [(136, 40, 2, 1)] * 5
    pics = [cases.picture(g, 0, m, 20 + i) for g in ((72, 24, 2, 2), (136, 40, 2, 1)) for i, (_l, m) in enumerate(cases.morph_masks(g[0], g[1], 6))]
    up = _Uploaded(torch, ctx, pics, geoms)
    for steps in (D.erode_disc(2), D.dilate_disc(3), D.opening_disc(3), D.closing_disc(2), D.opening_disc(0), D.opening_disc(1) + D.closing_disc(4)):
        rooms = [_room(torch, b, torch.uint8, (b,)) for b in (ctx.pic_bytes(s) for s in up.sids)]
        got = ctx.disc_morph(up.sids, [-1] * 10, steps, src=up.bufs, out=[r[0] for r in rooms])
        torch.cuda.synchronize()
        _check_bytes(torch, got, [g for r in rooms for g in r[1]], [D.of_steps(p, g, steps) for p, g in zip(pics, geoms)], f"{steps}")
    up.close()


def case_chain(torch, ctx):
    """the golden clips through histograms -> Otsu tables -> map -> disc_morph(opening_disc(3)) -> checksums against the fixture, and
    distance -> RANGE mask -> label_pictures(src=): the result composes; one stream, no host synchronisation in between"""
    import zlib
    from hvqm4_amd import distance as D
    from hvqm4_amd import labels as L
    from hvqm4_amd import maps as M
    fixture = json.load(open(os.path.join(ROOT, "tests", "golden", "distance.json")))["clips"]
    seen = 0
    for name, data, _hdr, _n in _golden():
        sid, hdr, n = _decode(ctx, data)
        g = (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)
        sids, ords = [sid] * n, list(range(n))
        mask = ctx.equalize_pictures(sids, ords, M.otsu())
        rows = [mask[i] for i in range(n)]
        opened = ctx.disc_morph(sids, [-1] * n, D.opening_disc(3), src=rows)
        sums = ctx.picture_checksums(sids, [-1] * n, src=[opened[i] for i in range(n)])
        maps, guards = _distance(torch, ctx, sids, [-1] * n, D.rule(), src=rows)
        core, g2 = _mask(torch, ctx, sids, maps, D.mask_range(5))
        labs, comps = ctx.label_pictures(sids, [-1] * n, L.rule(), cap=64, src=core)
        torch.cuda.synchronize()
        host = mask.cpu().numpy()
        if name in fixture:
            assert zlib.crc32(opened[0].cpu().numpy().tobytes()) == fixture[name]["opening3"], name
            assert zlib.crc32(maps[0].cpu().numpy().view(np.uint32).astype("<u4").tobytes()) == fixture[name]["euclid2"], name
            seen += 1
        wants = [D.of_picture(host[k], g, D.rule()) for k in range(n)]
        _check(torch, maps, guards, wants, name)
        _check_bytes(torch, [opened[k] for k in range(n)], [], [D.of_steps(host[k], g, D.opening_disc(3)) for k in range(n)], f"{name}: opening")
        cores = [D.of_mask(w, D.mask_range(5), g) for w in wants]
        _check_bytes(torch, core, g2, cores, f"{name}: core")
        from hvqm4_amd import checksums
        assert sums.cpu().tolist() == [checksums.of_bytes(D.of_steps(host[k], g, D.opening_disc(3)), *g) for k in range(n)], f"{name}: checksums"
        for k in range(n):
            lab, rec = L.of_picture(cores[k], g, L.rule(), 64)
            assert np.array_equal(labs[k].cpu().numpy().view(np.uint32), lab) and np.array_equal(comps[k].cpu().numpy()[:rec.shape[0]], rec), f"{name}: labels of the core, {k}"
        ctx.close_stream(sid)
    assert seen > 0


def case_refusals(torch, ctx):
    """HVQ_E_ARG leaves every output untouched; n == 0 does nothing; the well-formed call right after works"""
    import ctypes as C
    from hvqm4_amd import distance as D
    from hvqm4_amd._lib import HVQ_E_ARG, HvqDistanceMask, HvqDistanceRule, lib
    from tests import distance_cases as cases
    geom = (72, 24, 2, 2)
    pic = cases.picture(geom, 0, cases.fill_masks(72, 24, 1)[12][1], 9)
    up = _Uploaded(torch, ctx, [pic, pic], [geom, geom])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def rooms():
        maps = [torch.full((24, 72), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
        dst = [torch.full((ctx.pic_bytes(up.sids[0]),), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2)]
        return maps, dst

    def arr(v):
        return C.cast((C.c_void_p * len(v))(*v), C.c_void_p)

    def rule(plane, lo, hi, metric, border, pad=(0, 0, 0)):
        return HvqDistanceRule(plane, lo, hi, metric, border, (C.c_int32 * 3)(*pad))

    def entry(mode, lo, hi, invert, pad=(0, 0, 0, 0)):
        return HvqDistanceMask(mode, lo, hi, invert, (C.c_uint32 * 4)(*pad))
    good = (0, 255, 255, 0, 0)

    def raw_distance(n=2, sids=None, ords=(-1, -1), src=None, rules=(good,), nrules=None, which=None, maps_=None, h=None):
        maps, _d = rooms()
        a_r = (HvqDistanceRule * len(rules))(*[rule(*r) for r in rules])
        src = [b.data_ptr() for b in up.bufs] if src is None else src
        rc = lib().hvq_distance_pictures(ctx._h if h is None else h, n, (C.c_int * 2)(*(sids or up.sids)), (C.c_int * 2)(*ords), arr(src), C.cast(a_r, C.c_void_p),
                                         len(rules) if nrules is None else nrules, None if which is None else C.cast((C.c_int * 2)(*which), C.c_void_p),
                                         arr([t.data_ptr() for t in maps] if maps_ is None else maps_), stream)
        torch.cuda.synchronize()
        return rc, all(bool(t.eq(-7).all()) for t in maps)
    ok = up.bufs[0].data_ptr()
    refused = [("bad stream", dict(sids=[up.sids[0], 99])), ("an ordinal with src", dict(ords=(-1, 0))), ("misaligned src", dict(src=[ok, ok + 8])),
               ("nrules 0", dict(nrules=0)), ("nrules 65", dict(rules=(good,) * 65)), ("which beyond the rules", dict(which=[0, 1])),
               ("a negative which", dict(which=[-1, 0])), ("null map", dict(maps_=[ok, 0])), ("misaligned map", dict(maps_=[ok, ok + 4])),
               ("n beyond 65535", dict(n=65536)), ("negative n", dict(n=-1)), ("null context", dict(h=C.c_void_p(0)))]
    for bad in ((3, 0, 0, 0, 0), (-1, 0, 0, 0, 0), (0, 9, 8, 0, 0), (0, -1, 8, 0, 0), (0, 0, 256, 0, 0), (0, 0, 0, 3, 0), (0, 0, 0, 0, 2), (0, 0, 0, 0, 0, (0, 1, 0))):
        refused.append((f"rule {bad} in an entry that no picture uses", dict(rules=(good, bad), which=[0, 0])))
    for what, kw in refused:
        assert raw_distance(**kw) == (HVQ_E_ARG, True), what
    assert raw_distance(n=0) == (0, True), "n == 0 does nothing"
    rc, untouched = raw_distance()
    assert rc == 0 and not untouched
    maps, _g = _distance(torch, ctx, up.sids, [-1, -1], D.rule(), src=up.bufs)
    mgood = (0, 1, 9, 0)

    def raw_mask(n=2, sids=None, sel=(mgood,), nsel=None, which=None, maps_=None, dst=None, h=None):
        _m, out = rooms()
        a_e = (HvqDistanceMask * len(sel))(*[entry(*e) for e in sel])
        rc = lib().hvq_distance_mask(ctx._h if h is None else h, n, (C.c_int * 2)(*(sids or up.sids)), arr([t.data_ptr() for t in maps] if maps_ is None else maps_),
                                     C.cast(a_e, C.c_void_p), len(sel) if nsel is None else nsel, None if which is None else C.cast((C.c_int * 2)(*which), C.c_void_p),
                                     arr([t.data_ptr() for t in out] if dst is None else dst), stream)
        torch.cuda.synchronize()
        return rc, all(bool(t.eq(SENTINEL).all()) for t in out)
    refused = [("bad stream", dict(sids=[up.sids[0], 99])), ("nsel 0", dict(nsel=0)), ("nsel 65", dict(sel=(mgood,) * 65)), ("which beyond", dict(which=[0, 1])),
               ("null map", dict(maps_=[0, ok])), ("misaligned map", dict(maps_=[ok, ok + 8])), ("null dst", dict(dst=[ok, 0])), ("misaligned dst", dict(dst=[ok + 4, ok])),
               ("n beyond 65535", dict(n=65536)), ("null context", dict(h=C.c_void_p(0)))]
    for bad in ((0, 5, 4, 0), (2, 0, 0, 0), (0, 0, 9, 2), (0, 0, 9, 0, (0, 0, 1, 0)), (1, 1, 1, 0), (1, 0, 9, 0), (1, 0, 0, 1)):
        refused.append((f"mask {bad} in an entry that no picture uses", dict(sel=(mgood, bad), which=[0, 0])))
    for what, kw in refused:
        assert raw_mask(**kw) == (HVQ_E_ARG, True), what
    assert raw_mask(n=0) == (0, True), "n == 0 does nothing"
    rc, untouched = raw_mask()
    assert rc == 0 and not untouched
    up.close()


def case_tools(torch, ctx):
    """tools/discmorph.py on a golden clip: the printed facts and the files, against the same chain of the modules"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import discmorph
    from hvqm4_amd import distance as D
    from hvqm4_amd import histograms as H
    from hvqm4_amd import jpeg
    from hvqm4_amd import maps as M
    from oracle import bridge
    data = open(os.path.join(ROOT, "tests", "golden", "yuv422_64x48.h4m"), "rb").read()
    g = (64, 48, 2, 1)
    steps = D.opening_disc(2)
    geom, facts, files = discmorph.clip_discs(ctx, data, steps, quality=80)
    _g, facts2, field = discmorph.clip_discs(ctx, data, None, field=True, quality=80)
    assert geom == g and len(facts) == len(files) == len(field) > 0 and facts2 == facts
    pics = bridge.oracle_decode(data, len(files))
    rule = M.Rule(M.otsu().luma, M.flat(128).luma)
    for k, f in enumerate(files):
        p = pics[k].reshape(-1)
        mask = M.of_picture(p, g, M.from_lut(*M.tables_of_records(H.of_picture(p, *g), rule)))
        dist = D.of_picture(mask, g, D.rule())
        assert facts[k] == D.max_inscribed(dist), k
        assert f == jpeg.encode(D.of_steps(mask, g, steps), 64, 48, 80, 2, 1), k
        assert field[k] == jpeg.encode(D.of_mask(dist, D.mask_root(), g), 64, 48, 80, 2, 1), k
    _g, facts3, none = discmorph.clip_discs(ctx, data, files=False)
    assert none is None and facts3 == facts


CASES = ["small", "tiles", "far", "wide", "mixed", "mask", "morph", "chain", "refusals", "tools"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "distance", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_distance(case, child_results):
    gpu_child.report(case, child_results)
