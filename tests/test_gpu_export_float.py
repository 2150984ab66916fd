"""GPU: float export (hvq_export_tensors, Context.export_float) against tests/export_float_ref.py, tolerance 0: every comparison is
of raw bits.  The cases run in ONE child process that imports torch first (see tests/gpu_child.py); each test reports its case.  The
child stops at the first HVQ_E_HIP or HIP error: nothing more is started on a GPU that has reported a fault.

The wide geometry (1280 samples, coordinates above 2^10) is synthesised here: tests/clips.py holds nothing that wide."""
import numpy as np
import pytest

from tests import gpu_child
from tests.gpu_kit import decode as _decode, golden_by_name as _golden, long_clip as _long_clip, pics as _pics, self_ref_clip as _self_ref_clip

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "float16", "bfloat16")
CHILD_TIMEOUT = 900
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SENTINEL = -7.5                                     # exact in all three types


# ------------------------------------------------------------------------------------------------------------- child side
def _norm(mean=MEAN, std=STD, scale=1 / 255):
    from hvqm4_amd.export import normalisation
    return normalisation(mean, std, scale)


def _want(yuv, hdr, out_hw, crop, dtype, mean=MEAN, std=STD, scale=1 / 255):
    from tests.export_float_ref import export_float_reference
    mul, add = _norm(mean, std, scale)
    return export_float_reference(yuv, hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, out_hw, crop, mul, add, dtype)


def _same(got_tensor, want_bits, what):
    from tests.export_float_ref import bits_of
    got = bits_of(got_tensor)
    if not np.array_equal(got, want_bits):
        bad = np.argwhere(got != want_bits)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ, first at {tuple(bad[0])}: "
                             f"got {got[tuple(bad[0])]:#x}, want {want_bits[tuple(bad[0])]:#x}")


def case_goldens(torch, ctx):
    from oracle import bridge
    samplings = set()
    for name, (data, hdr, n) in _golden().items():
        sid, hdr, n = _decode(ctx, data)
        samplings.add((hdr.h_samp, hdr.v_samp, hdr.is15))
        yuv = bridge.oracle_decode(data, n)
        w, h = hdr.width, hdr.height
        for dt in DTYPES:
            out = torch.full((n, 3, h, w), SENTINEL, dtype=getattr(torch, dt), device="cuda")
            ctx.export_float([sid] * n, list(range(n)), out, mean=MEAN, std=STD)
            torch.cuda.synchronize()
            for k in range(n):
                _same(out[k], _want(yuv[k], hdr, (h, w), None, dt), (name, dt, k))
        ctx.close_stream(sid)
    assert {(2, 2), (2, 1), (1, 1)} <= {(a, b) for a, b, _v in samplings} and {True, False} <= {v for _a, _b, v in samplings}


def _wide_clip():
    from hvqm4_amd.synth import SynthConfig, make_clip
    return make_clip(SynthConfig(width=1280, height=64, gop="IP", seed=77)).data


def _resample_one(torch, ctx, name, data, dtypes):
    from oracle import bridge
    sid, hdr, n = _decode(ctx, data)
    yuv = bridge.oracle_decode(data, n)
    w, h = hdr.width, hdr.height
    k = n - 1
    crops = [None, (3, 1, w - 7, h - 5), (w - 17, h - 13, 17, 13), (5, 0, w - 5, h)]       # odd offsets; right / bottom edges
    sizes = [(h // 2, w // 2), (37, 53), (2 * h, 2 * w), (224, 224)]
    count = 0
    for crop in crops:
        for hw in sizes:
            for dt in dtypes:
                out = torch.full((1, 3) + hw, SENTINEL, dtype=getattr(torch, dt), device="cuda")
                ctx.export_float([sid], [k], out, crop=crop, mean=MEAN, std=STD)
                torch.cuda.synchronize()
                _same(out[0], _want(yuv[k], hdr, hw, crop, dt), (name, crop, hw, dt))
                count += 1
    ctx.close_stream(sid)
    return count


def case_resampled(torch, ctx):
    g = _golden()
    count = 0
    for i, name in enumerate(("gop64x48_15", "yuv422_64x48", "yuv444_64x48", "ragged24x40", "yuv444_13_portrait48x64",
                              "portrait48x64", "wide296x160", "yuv422_296x160", "yuv444_296x160")):
        count += _resample_one(torch, ctx, name, g[name][0], DTYPES)
    count += _resample_one(torch, ctx, "synth1280x64", _wide_clip(), DTYPES)
    assert count == 10 * 4 * 4 * 3


def case_mixed_batch(torch, ctx):
    from oracle import bridge
    g = _golden()
    names = ("gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "yuv444_64x48", "ip8")
    streams = []
    for nm in names:
        sid, hdr, n = _decode(ctx, g[nm][0])
        streams.append((nm, sid, hdr, n, bridge.oracle_decode(g[nm][0], n)))
    for dt in DTYPES:
        sids, ords, crops, sizes, wants = [], [], [], [], []
        i = 0
        for nm, sid, hdr, n, yuv in streams:
            w, h = hdr.width, hdr.height
            for k in range(n):
                kind = i % 5
                crop = [None, (1, 1, w - 2, h - 2), (w // 2, h // 2, w // 2, h // 2), None, (3, 0, w - 3, h - 1)][kind]
                cw, ch = (w, h) if crop is None else crop[2:]
                hw = [(h, w), (ch, cw), (224, 224), (h // 2 + 1, 2 * w + 4), (31, 17)][kind]     # identity, cropped identity, resized
                sids.append(sid); ords.append(k); crops.append(crop); sizes.append(hw)
                wants.append((nm, k, _want(yuv[k], hdr, hw, crop, dt)))
                i += 1
        outs = [torch.full((3,) + hw, SENTINEL, dtype=getattr(torch, dt), device="cuda") for hw in sizes]
        ctx.export_float(sids, ords, outs, crop=crops, mean=MEAN, std=STD)
        torch.cuda.synchronize()
        for out, (nm, k, want), crop, hw in zip(outs, wants, crops, sizes):
            _same(out, want, (nm, k, dt, crop, hw))
    for _nm, sid, _h, _n, _y in streams:
        ctx.close_stream(sid)


def case_pitched(torch, ctx):
    from oracle import bridge
    from tests.export_float_ref import bits_of
    g = _golden()
    for nm in ("gop64x48_15", "yuv422_296x160", "yuv444_64x48"):
        data, hdr, n = g[nm]
        sid, hdr, n = _decode(ctx, data)
        yuv = bridge.oracle_decode(data, n)
        w, h = hdr.width, hdr.height
        for dt in DTYPES:
            for hw, crop, x_off in (((h, w), None, 8), ((h, w), None, 3), ((40, 56), (2, 2, w - 4, h - 4), 8), ((41, 55), None, 5)):
                H, W = hw
                canvas = torch.full((n, 4, H + 8, W + 16), SENTINEL, dtype=getattr(torch, dt), device="cuda")
                sent = bits_of(canvas[0, 0, 0, :1])[0]
                sel = (slice(None), slice(1, 4), slice(4, 4 + H), slice(x_off, x_off + W))
                ctx.export_float([sid] * n, list(range(n)), canvas[sel], crop=crop, mean=MEAN, std=STD)
                torch.cuda.synchronize()
                got = bits_of(canvas)
                for k in range(n):
                    assert np.array_equal(got[sel][k], _want(yuv[k], hdr, hw, crop, dt)), (nm, dt, hw, x_off, k)
                rest = got.copy()
                rest[sel] = sent
                assert (rest == sent).all(), (nm, dt, hw, x_off, "elements outside the view were written")
        ctx.close_stream(sid)


def case_store_forms(torch, ctx):
    """a 16-byte-aligned dense destination (vector stores) and an element-aligned one (a view one element into a canvas with an odd
    row pitch) hold the same values; so does an odd output width, which only the element form can store"""
    from oracle import bridge
    from tests.export_float_ref import bits_of
    g = _golden()
    for nm in ("gop64x48_15", "yuv444_64x48", "yuv422_296x160"):
        data, hdr, n = g[nm]
        sid, hdr, n = _decode(ctx, data)
        yuv = bridge.oracle_decode(data, n)
        w, h = hdr.width, hdr.height
        for dt in DTYPES:
            td = getattr(torch, dt)
            for hw, crop in (((h, w), None), ((48, 72), None), ((h - 2, w - 8), (8, 1, w - 8, h - 2)), ((h, w - 3), (3, 0, w - 3, h)),
                             ((33, 47), None)):
                H, W = hw
                dense = torch.full((1, 3, H, W), SENTINEL, dtype=td, device="cuda")
                assert dense.data_ptr() % 16 == 0
                canvas = torch.full((3, H + 1, W + 3), SENTINEL, dtype=td, device="cuda")
                view = canvas[:, 1:, 1:1 + W]
                assert view.data_ptr() % 16 != 0 or (W + 3) % 2
                ctx.export_float([sid], [n - 1], dense, crop=crop, mean=MEAN, std=STD)
                ctx.export_float([sid], [n - 1], [view], crop=crop, mean=MEAN, std=STD)
                torch.cuda.synchronize()
                want = _want(yuv[n - 1], hdr, hw, crop, dt)
                _same(dense[0], want, (nm, dt, hw, crop, "dense"))
                _same(view, want, (nm, dt, hw, crop, "element-aligned view"))
                got = bits_of(canvas)
                sent = bits_of(torch.full((1,), SENTINEL, dtype=td))[0]
                assert (got[:, 0] == sent).all() and (got[:, :, 0] == sent).all() and (got[:, :, 1 + W:] == sent).all(), (nm, dt, hw)
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
    side, side2 = torch.cuda.Stream(), torch.cuda.Stream()
    shapes = {"float32": (h, w), "float16": (224, 224), "bfloat16": (h // 2, w // 2)}
    alloc = lambda dt, n: torch.full((n, 3) + shapes[dt], SENTINEL, dtype=getattr(torch, dt), device="cuda")
    # plain flushes: export right after flush() with no synchronisation; the next flush rewrites every slot of the ring of 3, a
    # replay rewrites them again
    sid = ctx.open_stream(w, h, 2, 2, hdr.is15, 3)
    for ft, p in pics[:3]:
        ctx.submit(sid, ft, p)
    ctx.flush()
    outs = {dt: alloc(dt, 3) for dt in DTYPES}
    u8 = torch.zeros((3, 3, h, w), dtype=torch.uint8, device="cuda")
    side.wait_stream(torch.cuda.current_stream())    # the destinations were filled on the current stream
    side2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for dt in DTYPES:
            ctx.export_float([sid] * 3, [0, 1, 2], outs[dt], mean=MEAN, std=STD)
    with torch.cuda.stream(side2):                  # the uint8 export of the same pictures, on another stream, back to back
        ctx.export([sid] * 3, [0, 1, 2], u8, "rgbp")
    with torch.cuda.stream(side):
        again = alloc("float32", 3)
        ctx.export_float([sid] * 3, [0, 1, 2], again, mean=MEAN, std=STD)
    for ft, p in pics[3:9]:
        ctx.submit(sid, ft, p)
    ctx.flush()
    ctx.replay(2)
    torch.cuda.synchronize()
    for dt in DTYPES:
        for k in range(3):
            _same(outs[dt][k], _want(yuv[k], hdr, shapes[dt], None, dt), ("flush", dt, k))
    for k in range(3):
        _same(again[k], _want(yuv[k], hdr, shapes["float32"], None, "float32"), ("flush, after the uint8 export", k))
    for k in range(3):
        assert np.array_equal(u8[k].cpu().numpy(), export_reference(yuv[k], w, h, 2, 2, "rgbp")), ("uint8 beside float", k)
    ctx.close_stream(sid)
    # streaming: batch k exported while batch k + 1 is in flight; batch k + 2 reuses batch k's slots
    sid = ctx.open_stream(w, h, 2, 2, hdr.is15, 8)
    b = [pics[0:4], pics[4:8], pics[8:12]]
    sub = lambda part: ctx.submit_many_device([sid] * len(part), [ft for ft, _p in part], [p for _f, p in part])
    sub(b[0]); ctx.flush_begin()
    sub(b[1]); ctx.flush_next()                    # batch 0 ended, batch 1 in flight
    outs = {dt: alloc(dt, 4) for dt in DTYPES}
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for dt in DTYPES:
            ctx.export_float([sid] * 4, [0, 1, 2, 3], outs[dt], mean=MEAN, std=STD)
    sub(b[2]); ctx.flush_next()                    # batch 1 ended, batch 2 in flight
    ctx.flush_end()                                # batch 2 reconstructed into batch 0's slots
    torch.cuda.synchronize()
    for dt in DTYPES:
        for k in range(4):
            _same(outs[dt][k], _want(yuv[k], hdr, shapes[dt], None, dt), ("flush_next", dt, k))
    for k in range(8, 12):
        assert np.array_equal(ctx.read_picture(sid, k), yuv[k]), k
    ctx.close_stream(sid)


def case_refusals(torch, ctx):
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_STATE, HvqError, lib
    from hvqm4_amd.container import video_pictures
    from hvqm4_amd.export import HvqTensorDst
    from tests.export_float_ref import bits_of
    data, hdr, n = _golden()["gop64x48_15"]
    w, h = hdr.width, hdr.height

    def untouched(t):
        torch.cuda.synchronize()
        assert (bits_of(t) == bits_of(torch.full((1,), SENTINEL, dtype=t.dtype))[0]).all(), "a refused export wrote its destination"

    def refused(code, sids, ords, dt="float32"):
        out = torch.full((len(sids), 3, 24, 40), SENTINEL, dtype=getattr(torch, dt), device="cuda")
        try:
            ctx.export_float(sids, ords, out)
        except HvqError as e:
            assert e.code == code, e
        else:
            raise AssertionError(f"export_float of {list(zip(sids, ords))} was not refused")
        untouched(out)

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
    refused(HVQ_E_STATE, [sid], [0], "float16")                               # slot reused
    refused(HVQ_E_ARG, [sid], [len(pics) + 5])                                # bad ordinal
    refused(HVQ_E_ARG, [sid + 100], [0], "bfloat16")                          # bad stream
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
    # what the library itself refuses (the Python front end refuses most of it earlier): nothing is enqueued
    last = len(pics) - 1
    buf = torch.full((1, 3, h, w), SENTINEL, dtype=torch.float32, device="cuda")
    base = buf.data_ptr()
    one, zero = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    D = HvqTensorDst
    cases = [(D(base, 0, 0, w, h, 0, 0, 0, 0), 7, one, zero),                 # bad dtype
             (D(None, 0, 0, w, h, 0, 0, 0, 0), 0, one, zero),                 # null pointer
             (D(base, 0, 0, w, h, 0, 0, 0, 0), 0, (1.0, float("nan"), 1.0), zero),
             (D(base, 0, 0, w, h, 0, 0, 0, 0), 0, one, (0.0, 0.0, float("inf"))),
             (D(base, 0, 0, 0, h, 0, 0, 0, 0), 0, one, zero),                 # W < 1
             (D(base, 0, 0, w, -1, 0, 0, 0, 0), 0, one, zero),                # H < 1
             (D(base, 0, 0, 16385, 1, 0, 0, 0, 0), 0, one, zero),             # W above 16384
             (D(base, 0, 0, w, h, 1, 0, w, h), 0, one, zero),                 # crop leaves the picture on the right
             (D(base, 0, 0, w, h, 0, 1, w, h), 0, one, zero),                 # ... at the bottom
             (D(base, 0, 0, w, h, -1, 0, 8, 8), 0, one, zero),
             (D(base, 0, 0, w, h, 0, 0, 8, 0), 0, one, zero),                 # empty crop
             (D(base, 0, 0, w, h, 2, 0, 0, 0), 0, one, zero),                 # crop_w == 0 with an offset
             (D(base, 4 * w - 4, 0, w, h, 0, 0, 0, 0), 0, one, zero),         # row pitch below dense
             (D(base, 4 * w, 4 * w * h - 4, w, h, 0, 0, 0, 0), 0, one, zero), # planes overlap
             (D(base + 2, 0, 0, w, h, 0, 0, 0, 0), 0, one, zero),             # pointer not a multiple of the element size
             (D(base + 1, 0, 0, w, h, 0, 0, 0, 0), 1, one, zero),
             (D(base, 4 * w + 2, 0, w, h, 0, 0, 0, 0), 0, one, zero),         # pitch not a multiple of the element size
             (D(base, 2 * w + 1, 0, w, h, 0, 0, 0, 0), 2, one, zero)]
    for d, dtype, mul, add in cases:
        a_s, a_o = (C.c_int * 1)(sid), (C.c_int * 1)(last)
        rc = lib().hvq_export_tensors(ctx._h, 1, a_s, a_o, dtype, (C.c_float * 3)(*mul), (C.c_float * 3)(*add), C.byref(d),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == HVQ_E_ARG, (rc, dtype, mul, add, [getattr(d, f) for f, _t in D._fields_])
    a_s, a_o = (C.c_int * 1)(sid), (C.c_int * 1)(last)
    assert lib().hvq_export_tensors(ctx._h, 1, a_s, a_o, 0, None, None, C.byref(cases[0][0]), None) == HVQ_E_ARG
    untouched(buf)
    # and the well-formed call right after them works
    ctx.export_float([sid], [last], buf)
    torch.cuda.synchronize()
    assert not (bits_of(buf) == bits_of(torch.full((1,), SENTINEL))[0]).any()
    ctx.close_stream(sid); ctx.close_stream(sb)


def case_torch_sanity(torch, ctx):
    """F.interpolate on the uint8 export with the same normalisation: within 0.1 of a 0..255 unit, scaled by mul"""
    import torch.nn.functional as F
    g = _golden()
    mul, add = _norm()
    for nm in ("wide296x160", "yuv422_296x160", "yuv444_13_portrait48x64"):
        data, hdr, n = g[nm]
        sid, hdr, n = _decode(ctx, data)
        w, h = hdr.width, hdr.height
        u8 = torch.zeros((n, 3, h, w), dtype=torch.uint8, device="cuda")
        ctx.export([sid] * n, list(range(n)), u8, "rgbp")
        for hw, crop in (((h, w), None), ((224, 224), None), ((h // 2, w // 2), None), ((2 * h, 2 * w), None), ((50, 70), (3, 5, w - 9, h - 8))):
            out = torch.zeros((n, 3) + hw, dtype=torch.float32, device="cuda")
            ctx.export_float([sid] * n, list(range(n)), out, crop=crop, mean=MEAN, std=STD)
            src = u8.float()
            if crop:
                src = src[:, :, crop[1]:crop[1] + crop[3], crop[0]:crop[0] + crop[2]]
            ref = F.interpolate(src, size=hw, mode="bilinear", align_corners=False, antialias=False)
            m = torch.tensor(mul, device="cuda").view(1, 3, 1, 1)
            a = torch.tensor(add, device="cuda").view(1, 3, 1, 1)
            ref = ref * m + a
            torch.cuda.synchronize()
            worst = float(((out - ref).abs() / m).max())
            print(f"{nm} {hw} crop {crop}: worst difference {worst:.6f} of a 0..255 unit")
            assert worst <= 0.1, (nm, hw, crop, worst)
        ctx.close_stream(sid)


CASES = ["goldens", "resampled", "mixed_batch", "pitched", "store_forms", "no_host_sync", "refusals", "torch_sanity"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "export_float", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_export_float(case, child_results):
    gpu_child.report(case, child_results)
