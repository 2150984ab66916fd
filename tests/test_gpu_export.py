"""GPU: picture export into torch tensors (hvq_export_pictures, Context.export), tolerance 0 everywhere.  The cases run in ONE child
process that imports torch first (see tests/gpu_child.py); each test reports its case.  The child stops at the first HVQ_E_HIP or HIP
error: nothing more is started on a GPU that has reported a fault."""
import os

import numpy as np
import pytest

from tests import gpu_child
from tests.gpu_kit import decode as _decode, golden as _golden, long_clip as _long_clip, pics as _pics, self_ref_clip as _self_ref_clip

pytestmark = pytest.mark.gpu

FMTS = ("rgb", "rgbp", "yuv444p")
CHILD_TIMEOUT = 900


# ------------------------------------------------------------------------------------------------------------- child side
def _alloc(torch, geom, fmt, n=None, fill=0):
    w, h = geom
    shape = (h, w, 3) if fmt == "rgb" else (3, h, w)
    if n is not None:
        shape = (n,) + shape
    return torch.full(shape, fill, dtype=torch.uint8, device="cuda")


def _want(data, n, hdr, fmt):
    from oracle import bridge
    from tests.test_export_cpu import export_reference
    yuv = bridge.oracle_decode(data, n)
    return np.stack([export_reference(yuv[k], hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, fmt) for k in range(n)])


def case_goldens(torch, ctx):
    samplings = set()
    for name, data, hdr, n in _golden():
        sid, hdr, n = _decode(ctx, data)
        samplings.add((hdr.h_samp, hdr.v_samp, hdr.is15))
        for fmt in FMTS:
            out = _alloc(torch, (hdr.width, hdr.height), fmt, n)
            ctx.export([sid] * n, list(range(n)), out, fmt)
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), _want(data, n, hdr, fmt)), (name, fmt)
            if fmt == "rgb" and (hdr.h_samp, hdr.v_samp) == (2, 2):
                for k in range(n):
                    assert np.array_equal(out[k].cpu().numpy(), ctx.read_picture_rgb(sid, k, hdr.width, hdr.height)), (name, k)
        ctx.close_stream(sid)
    assert {(2, 2), (2, 1), (1, 1)} <= {(a, b) for a, b, _v in samplings} and {True, False} <= {v for _a, _b, v in samplings}


def case_mixed_batch(torch, ctx):
    from tests.test_export_cpu import MANIFEST
    g = {name: (data, hdr, n) for name, data, hdr, n in _golden()}
    for names in (("gop64x48_15", "yuv422_64x48", "yuv444_13_portrait48x64", "i16"),              # every width % 16 == 0
                  ("wide296x160", "yuv422_296x160", "yuv444_64x48", "ragged24x40", "ip8")):      # and not
        streams = [(nm,) + _decode(ctx, g[nm][0]) for nm in names]
        sids, ords, geoms, wants = [], [], [], {}
        for nm, sid, hdr, n in streams:
            for k in range(n):
                sids.append(sid); ords.append(k); geoms.append((hdr.width, hdr.height))
        for fmt in FMTS:
            for nm, sid, hdr, n in streams:
                wants[nm] = _want(g[nm][0], n, hdr, fmt)
            outs = [_alloc(torch, geo, fmt) for geo in geoms]
            ctx.export(sids, ords, outs, fmt)
            torch.cuda.synchronize()
            i = 0
            for nm, sid, hdr, n in streams:
                for k in range(n):
                    assert np.array_equal(outs[i].cpu().numpy(), wants[nm][k]), (nm, k, fmt)
                    i += 1
        for _nm, sid, _h, _n in streams:
            ctx.close_stream(sid)
    assert MANIFEST


def case_pitched(torch, ctx):
    g = {name: (data, hdr, n) for name, data, hdr, n in _golden()}
    for nm in ("gop64x48_15", "yuv422_296x160", "yuv444_64x48"):
        data, hdr, n = g[nm]
        sid, hdr, n = _decode(ctx, data)
        w, h = hdr.width, hdr.height
        for fmt in FMTS:
            want = _want(data, n, hdr, fmt)
            if fmt == "rgb":
                canvas = torch.full((n, h + 8, w + 16, 3), 0xA5, dtype=torch.uint8, device="cuda")
                view = canvas[:, 4:4 + h, 8:8 + w]
                sel = (slice(None), slice(4, 4 + h), slice(8, 8 + w))
            else:
                canvas = torch.full((n, 4, h + 8, w + 16), 0xA5, dtype=torch.uint8, device="cuda")
                view = canvas[:, 1:4, 4:4 + h, 8:8 + w]
                sel = (slice(None), slice(1, 4), slice(4, 4 + h), slice(8, 8 + w))
            ctx.export([sid] * n, list(range(n)), view, fmt)
            torch.cuda.synchronize()
            got = canvas.cpu().numpy()
            assert np.array_equal(got[sel], want), (nm, fmt)
            rest = got.copy()
            rest[sel] = 0xA5
            assert (rest == 0xA5).all(), (nm, fmt, "bytes outside the picture area were written")
        ctx.close_stream(sid)


def case_no_host_sync(torch, ctx):
    from hvqm4_amd.container import parse_header, video_pictures
    from oracle import bridge
    from tests.test_export_cpu import export_reference
    clip = _long_clip()
    hdr = parse_header(clip.data)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(clip.data)]
    yuv = bridge.oracle_decode(clip.data, len(pics))
    w, h = hdr.width, hdr.height
    side = torch.cuda.Stream()
    # plain flushes: batch k = pictures 0..2 in a ring of 3, batch k + 1 rewrites every slot
    sid = ctx.open_stream(w, h, 2, 2, hdr.is15, 3)
    for ft, p in pics[:3]:
        ctx.submit(sid, ft, p)
    ctx.flush()
    outs = {fmt: _alloc(torch, (w, h), fmt, 3) for fmt in FMTS}
    side.wait_stream(torch.cuda.current_stream())   # the destinations were filled on the current stream
    with torch.cuda.stream(side):
        for fmt in FMTS:
            ctx.export([sid] * 3, [0, 1, 2], outs[fmt], fmt)
    for ft, p in pics[3:9]:
        ctx.submit(sid, ft, p)
    ctx.flush()
    torch.cuda.synchronize()
    for fmt in FMTS:
        for k in range(3):
            assert np.array_equal(outs[fmt][k].cpu().numpy(), export_reference(yuv[k], w, h, 2, 2, fmt)), ("flush", fmt, k)
    ctx.close_stream(sid)
    # streaming: batch k exported while batch k + 1 is in flight; batch k + 2 reuses batch k's slots
    sid = ctx.open_stream(w, h, 2, 2, hdr.is15, 8)
    b = [pics[0:4], pics[4:8], pics[8:12]]
    sub = lambda part: ctx.submit_many_device([sid] * len(part), [ft for ft, _p in part], [p for _f, p in part])
    sub(b[0]); ctx.flush_begin()
    sub(b[1]); ctx.flush_next()                    # batch 0 ended, batch 1 in flight
    outs = {fmt: _alloc(torch, (w, h), fmt, 4) for fmt in FMTS}
    side.wait_stream(torch.cuda.current_stream())   # the destinations were filled on the current stream
    with torch.cuda.stream(side):
        for fmt in FMTS:
            ctx.export([sid] * 4, [0, 1, 2, 3], outs[fmt], fmt)
    sub(b[2]); ctx.flush_next()                    # batch 1 ended, batch 2 in flight
    ctx.flush_end()                                # batch 2 reconstructed into batch 0's slots
    torch.cuda.synchronize()
    for fmt in FMTS:
        for k in range(4):
            assert np.array_equal(outs[fmt][k].cpu().numpy(), export_reference(yuv[k], w, h, 2, 2, fmt)), ("flush_next", fmt, k)
    for k in range(8, 12):
        assert np.array_equal(ctx.read_picture(sid, k), yuv[k]), k
    ctx.close_stream(sid)


def case_close_after_export(torch, ctx):
    clip = _long_clip()
    sid, hdr, n = _decode(ctx, clip.data)
    out = _alloc(torch, (hdr.width, hdr.height), "rgb", n)
    ctx.export([sid] * n, list(range(n)), out, "rgb")
    ctx.close_stream(sid)
    sid2, _h, _n = _decode(ctx, clip.data)         # a new ring, likely in the freed memory
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), _want(clip.data, n, hdr, "rgb"))
    ctx.close_stream(sid2)


def case_refusals(torch, ctx):
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_STATE, HvqError, lib
    from hvqm4_amd.export import HvqExportDst
    g = {name: (data, hdr, n) for name, data, hdr, n in _golden()}
    data, hdr, n = g["gop64x48_15"]
    w, h = hdr.width, hdr.height

    def refused(code, sids, ords, fmt="rgb"):
        out = _alloc(torch, (w, h), fmt, len(sids), fill=0xA5)
        try:
            ctx.export(sids, ords, out, fmt)
        except HvqError as e:
            assert e.code == code, e
        else:
            raise AssertionError(f"export of {list(zip(sids, ords))} was not refused")
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 0xA5).all(), "a refused export wrote its destination"

    from hvqm4_amd.container import video_pictures
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    sid = ctx.open_stream(w, h, 2, 2, hdr.is15, 3)
    for ft, p in pics[:2]:
        ctx.submit(sid, ft, p)
    ctx.flush()
    q = ctx.submit(sid, *pics[2])
    refused(HVQ_E_STATE, [sid, sid], [0, q])                                  # queued but not flushed (with a good one)
    for ft, p in pics[3:]:
        ctx.submit(sid, ft, p)
    ctx.flush()
    refused(HVQ_E_STATE, [sid], [0])                                          # slot reused
    refused(HVQ_E_ARG, [sid], [len(pics) + 5])                                # bad ordinal
    refused(HVQ_E_ARG, [sid + 100], [0])                                      # bad stream
    bad = _self_ref_clip(seed=9)
    bp = _pics(bad)
    sb = ctx.open_stream(bad.width, bad.height, 2, 2, True, 12)
    ctx.submit_many_device([sb] * len(bp), [ft for ft, _p in bp], [p for _f, p in bp])
    try:
        ctx.flush()
    except HvqError:
        pass
    else:
        raise AssertionError("the corrupt picture was not refused")
    refused(HVQ_E_STATE, [sb], [1])                                           # dropped by the rejection
    # destinations the library itself refuses (the Python front end refuses them earlier): nothing is enqueued
    last = len(pics) - 1
    buf = _alloc(torch, (w, h), "rgb", 1, fill=0xA5)
    base = buf.data_ptr()
    for d, fmt in ((HvqExportDst(base, 3 * w - 4, 0), 0),                     # row pitch below w*3
                   (HvqExportDst(base + 1, 0, 0), 0),                         # misaligned pointer
                   (HvqExportDst(base, 3 * w + 2, 0), 0),                     # misaligned pitch
                   (HvqExportDst(base, w, w * h - w), 1),                     # planes overlap
                   (HvqExportDst(None, 0, 0), 0),
                   (HvqExportDst(base, 0, 0), 7)):                            # bad format
        a_s, a_o = (C.c_int * 1)(sid), (C.c_int * 1)(last)
        rc = lib().hvq_export_pictures(ctx._h, 1, a_s, a_o, fmt, C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == HVQ_E_ARG, (rc, d.row_pitch, d.plane_pitch, fmt)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xA5).all()
    small = torch.full((h - 8, w, 3), 0xA5, dtype=torch.uint8, device="cuda")
    try:
        ctx.export([sid], [last], [small], "rgb")
    except ValueError:
        pass
    else:
        raise AssertionError("a destination too small for the picture was accepted")
    assert (small.cpu().numpy() == 0xA5).all()
    ctx.close_stream(sid); ctx.close_stream(sb)


def case_one_hip_runtime(torch, ctx):
    paths = {os.path.realpath(l.split()[5]) for l in open("/proc/self/maps")
             if len(l.split()) >= 6 and os.path.basename(l.split()[5]).startswith("libamdhip64")}
    assert len(paths) == 1, paths


CASES = ["goldens", "mixed_batch", "pitched", "no_host_sync", "close_after_export", "refusals", "one_hip_runtime"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "export", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_export(case, child_results):
    gpu_child.report(case, child_results)
