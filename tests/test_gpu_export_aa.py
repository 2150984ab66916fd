"""GPU: antialiased float export (hvq_export_resampled with HVQ_FILTER_TRIANGLE, Context.export_float(antialias=True)) against
tests/export_aa_ref.py, tolerance 0: every comparison but torch_sanity is of raw bits.  The cases run in ONE child process that
imports torch first (see tests/gpu_child.py); each test reports its case.  The child stops at the first HVQ_E_HIP or HIP error:
nothing more is started on a GPU that has reported a fault.

Which body of the kernel a geometry takes (tiled: LDS, one barrier; direct: nested tap loops) is the host's decision,
hvq_resample_tile_rows; the cases assert through it that both ran, and body_agreement runs the same geometries through both."""
import numpy as np
import pytest

from tests import gpu_child
from tests.gpu_kit import decode as _decode, golden_by_name as _golden, long_clip as _long_clip

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "float16", "bfloat16")
CHILD_TIMEOUT = 420                                 # the cases take about a minute together; a hung child is ended, not waited for
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SENTINEL = -7.5                                     # exact in all three types


# ------------------------------------------------------------------------------------------------------------- child side
def _norm():
    from hvqm4_amd.export import normalisation
    return normalisation(MEAN, STD, 1 / 255)


def _rgbp(yuv, hdr):
    from tests.test_export_cpu import export_reference
    return export_reference(yuv, hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, "rgbp")


def _want32(rgbp, out_hw, crop):
    """the normalised float32 result: computed once per geometry, converted per dtype"""
    from tests.export_aa_ref import aa_from_planes
    mul, add = _norm()
    return aa_from_planes(rgbp, out_hw, crop, mul, add)


def _bits(o32, dtype):
    from tests.export_aa_ref import to_dtype
    return to_dtype(o32, dtype)


def _same(got_tensor, want_bits, what):
    from tests.export_aa_ref import bits_of
    got = bits_of(got_tensor)
    if not np.array_equal(got, want_bits):
        bad = np.argwhere(got != want_bits)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ, first at {tuple(bad[0])}: "
                             f"got {got[tuple(bad[0])]:#x}, want {want_bits[tuple(bad[0])]:#x}")


def _tile_rows(w, h, crop, hw):
    from hvqm4_amd._lib import lib
    cw, ch = (w, h) if crop is None else crop[2:]
    return lib().hvq_resample_tile_rows(cw, ch, hw[1], hw[0])


def _fresh(torch, shape, dt):
    return torch.full(shape, SENTINEL, dtype=getattr(torch, dt), device="cuda")


def _wide_clip():
    from hvqm4_amd.synth import SynthConfig, make_clip
    return make_clip(SynthConfig(width=1280, height=64, gop="IP", seed=77)).data


def case_goldens_identity(torch, ctx):
    """at picture size antialias=True is antialias=False bit for bit (every row of weights is [1, 0]), on every golden clip"""
    from tests.export_aa_ref import bits_of
    for name, (data, hdr, n) in _golden().items():
        sid, hdr, n = _decode(ctx, data)
        w, h = hdr.width, hdr.height
        for dt in DTYPES:
            plain, aa = _fresh(torch, (n, 3, h, w), dt), _fresh(torch, (n, 3, h, w), dt)
            ctx.export_float([sid] * n, list(range(n)), plain, mean=MEAN, std=STD)
            ctx.export_float([sid] * n, list(range(n)), aa, mean=MEAN, std=STD, antialias=True)
            torch.cuda.synchronize()
            assert np.array_equal(bits_of(aa), bits_of(plain)), (name, dt)
            assert not (bits_of(aa) == bits_of(torch.full((1,), SENTINEL, dtype=aa.dtype))[0]).all(), (name, dt)
        ctx.close_stream(sid)


def _downscale_one(torch, ctx, name, data, bodies):
    from oracle import bridge
    sid, hdr, n = _decode(ctx, data)
    k = n - 1
    rgbp = _rgbp(bridge.oracle_decode(data, n)[k], hdr)
    w, h = hdr.width, hdr.height
    crops = [None, (3, 1, w - 7, h - 5), (w - 17, h - 13, 17, 13)]               # odd offsets (the chroma index rule); right / bottom edges
    sizes = [(h // 2, w // 2), (37, 53), (7, w), (h, 9), (1, 1), (224, 224)]
    count = 0
    for crop in crops:
        for hw in sizes:
            body = _tile_rows(w, h, crop, hw)
            bodies.setdefault((name, crop is None, hw), body)
            want = _want32(rgbp, hw, crop)
            for dt in DTYPES:
                out = _fresh(torch, (1, 3) + hw, dt)
                ctx.export_float([sid], [k], out, crop=crop, mean=MEAN, std=STD, antialias=True)
                torch.cuda.synchronize()
                _same(out[0], _bits(want, dt), (name, crop, hw, dt, f"tile rows {body}"))
                count += 1
    ctx.close_stream(sid)
    return count


def case_downscale(torch, ctx):
    g = _golden()
    bodies, count = {}, 0
    for name in ("gop64x48_15", "yuv422_64x48", "yuv444_64x48", "ragged24x40", "portrait48x64", "wide296x160", "yuv422_296x160"):
        count += _downscale_one(torch, ctx, name, g[name][0], bodies)
    count += _downscale_one(torch, ctx, "synth1280x64", _wide_clip(), bodies)
    assert count == 8 * 3 * 6 * 3
    # both bodies ran, where the geometry says they must
    for name, (w, h) in (("wide296x160", (296, 160)), ("yuv422_296x160", (296, 160)), ("synth1280x64", (1280, 64))):
        assert bodies[(name, True, (1, 1))] == 0 and bodies[(name, True, (7, w))] == 0, (name, "direct body expected")
        assert bodies[(name, True, (h // 2, w // 2))] == 16, (name, "tiled body expected")
    vals = set(bodies.values())
    assert {0, 8, 16} <= vals, vals


def case_body_agreement(torch, ctx):
    """sizes just inside and just outside the tiled body's LDS bound, and at the step between its two tile heights; every size
    through the library's own choice and through the direct body alone: equal bits, and the restatement's"""
    from hvqm4_amd._lib import lib
    from hvqm4_amd.export import FILTER_TRIANGLE, FILTER_TRIANGLE_DIRECT
    from oracle import bridge
    from tests.export_aa_ref import bits_of
    data, hdr, n = _golden()["wide296x160"]
    sid, hdr, n = _decode(ctx, data)
    w, h = hdr.width, hdr.height
    assert (w, h) == (296, 160)
    rgbp = _rgbp(bridge.oracle_decode(data, n)[n - 1], hdr)
    q = lambda oh: lib().hvq_resample_tile_rows(w, h, 100, oh)
    inside = next(oh for oh in range(1, h) if q(oh))                             # the least output height the tiled body takes
    step = next(oh for oh in range(1, h) if q(oh) == 16)                         # ... with 16-row tiles
    assert q(inside) == 8 and q(inside - 1) == 0 and q(step - 1) == 8 and inside < step
    mul, add = _norm()
    for oh, body in ((inside - 1, 0), (inside, 8), (step - 1, 8), (step, 16)):
        want = _want32(rgbp, (oh, 100), None)
        for dt in DTYPES:
            auto, direct = _fresh(torch, (1, 3, oh, 100), dt), _fresh(torch, (1, 3, oh, 100), dt)
            ctx._export_float([sid], [n - 1], auto, None, MEAN, STD, 1 / 255, FILTER_TRIANGLE)
            ctx._export_float([sid], [n - 1], direct, None, MEAN, STD, 1 / 255, FILTER_TRIANGLE_DIRECT)
            torch.cuda.synchronize()
            assert np.array_equal(bits_of(auto), bits_of(direct)), (oh, body, dt, "the two bodies differ")
            _same(auto[0], _bits(want, dt), (oh, body, dt))
    ctx.close_stream(sid)


def case_upscale(torch, ctx):
    from oracle import bridge
    g = _golden()
    for name in ("gop64x48_15", "yuv422_296x160"):
        sid, hdr, n = _decode(ctx, g[name][0])
        rgbp = _rgbp(bridge.oracle_decode(g[name][0], n)[n - 1], hdr)
        w, h = hdr.width, hdr.height
        for hw in ((2 * h, 2 * w), (h + 1, w + 3)):
            assert _tile_rows(w, h, None, hw) == 0
            want = _want32(rgbp, hw, None)
            for dt in DTYPES:
                out = _fresh(torch, (1, 3) + hw, dt)
                ctx.export_float([sid], [n - 1], out, mean=MEAN, std=STD, antialias=True)
                torch.cuda.synchronize()
                _same(out[0], _bits(want, dt), (name, hw, dt))
        ctx.close_stream(sid)


def case_mixed_batch(torch, ctx):
    """one call, seven streams of different sizes and samplings; per picture identity, cropped identity, down (both tile heights),
    up and a huge ratio"""
    from oracle import bridge
    g = _golden()
    names = ("gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "yuv444_64x48", "ip8")
    streams = []
    for nm in names:
        sid, hdr, n = _decode(ctx, g[nm][0])
        yuv = bridge.oracle_decode(g[nm][0], n)
        streams.append((nm, sid, hdr, n, [_rgbp(yuv[k], hdr) for k in range(n)]))
    sids, ords, crops, sizes, wants, bodies = [], [], [], [], [], set()
    i = 0
    for nm, sid, hdr, n, planes in streams:
        w, h = hdr.width, hdr.height
        for k in range(n):
            kind = i % 7
            crop = [None, (1, 1, w - 2, h - 2), (w // 2, h // 2, w // 2, h // 2), None, (3, 0, w - 3, h - 1), None, None][kind]
            cw, ch = (w, h) if crop is None else crop[2:]
            hw = [(h, w), (ch, cw), (224, 224), (h // 2 + 1, 2 * w + 4), (31, 17), (max(h // 4, 1), max(w // 3, 1)), (2, 3)][kind]
            sids.append(sid); ords.append(k); crops.append(crop); sizes.append(hw)
            wants.append((nm, k, _want32(planes[k], hw, crop)))
            bodies.add(_tile_rows(w, h, crop, hw))
            i += 1
    assert {0, 8, 16} <= bodies, bodies
    for dt in DTYPES:
        outs = [_fresh(torch, (3,) + hw, dt) for hw in sizes]
        ctx.export_float(sids, ords, outs, crop=crops, mean=MEAN, std=STD, antialias=True)
        torch.cuda.synchronize()
        for out, (nm, k, want), crop, hw in zip(outs, wants, crops, sizes):
            _same(out, _bits(want, dt), (nm, k, dt, crop, hw))
    for _nm, sid, _h, _n, _p in streams:
        ctx.close_stream(sid)


def case_pitched_and_store_forms(torch, ctx):
    """views with larger row / plane pitches; 16-byte aligned (vector stores) and element-aligned pointers; output widths that are
    no multiple of the run: the same values, and nothing outside the described region changes"""
    from oracle import bridge
    from tests.export_aa_ref import bits_of
    g = _golden()
    for nm in ("gop64x48_15", "yuv422_296x160"):
        data, hdr, n = g[nm]
        sid, hdr, n = _decode(ctx, data)
        yuv = bridge.oracle_decode(data, n)
        planes = [_rgbp(yuv[k], hdr) for k in range(n)]
        w, h = hdr.width, hdr.height
        # (output size, crop, column offset of the view in its canvas): tiled and direct bodies, widths 40 / 41 / 9 / w + 8
        geoms = (((h // 2, 40), None, 8), ((h // 2, 40), None, 3), ((h // 2 - 1, 41), (2, 2, w - 4, h - 4), 8), ((h // 2, 9), None, 5),
                 ((h + 3, w + 8), None, 8), ((h + 3, w + 8), None, 1), ((2, 3), None, 4))
        for hw, crop, x_off in geoms:
            H, W = hw
            wants = [_want32(planes[k], hw, crop) for k in range(n)]
            for dt in DTYPES:
                canvas = _fresh(torch, (n, 4, H + 8, W + 16), dt)
                sent = bits_of(canvas[0, 0, 0, :1])[0]
                sel = (slice(None), slice(1, 4), slice(4, 4 + H), slice(x_off, x_off + W))
                ctx.export_float([sid] * n, list(range(n)), canvas[sel], crop=crop, mean=MEAN, std=STD, antialias=True)
                torch.cuda.synchronize()
                got = bits_of(canvas)
                for k in range(n):
                    assert np.array_equal(got[sel][k], _bits(wants[k], dt)), (nm, dt, hw, x_off, k)
                rest = got.copy()
                rest[sel] = sent
                assert (rest == sent).all(), (nm, dt, hw, x_off, "elements outside the view were written")
        ctx.close_stream(sid)


def case_refusals(torch, ctx):
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_STATE, HvqError, lib
    from hvqm4_amd.container import video_pictures
    from hvqm4_amd.export import HvqTensorDst
    from tests.export_aa_ref import bits_of
    data, hdr, n = _golden()["gop64x48_15"]
    w, h = hdr.width, hdr.height

    def untouched(t):
        torch.cuda.synchronize()
        assert (bits_of(t) == bits_of(torch.full((1,), SENTINEL, dtype=t.dtype))[0]).all(), "a refused export wrote its destination"

    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    sid = ctx.open_stream(w, h, 2, 2, hdr.is15, 3)
    for ft, p in pics:
        ctx.submit(sid, ft, p)
    ctx.flush()
    last = len(pics) - 1
    out = _fresh(torch, (2, 3, 24, 40), "float16")
    try:
        ctx.export_float([sid, sid], [last, 0], out, antialias=True)         # picture 0: its slot of the ring of 3 was reused
    except HvqError as e:
        assert e.code == HVQ_E_STATE, e
    else:
        raise AssertionError("a reused slot was not refused")
    untouched(out)
    buf = _fresh(torch, (1, 3, 24, 32), "float32")
    base = buf.data_ptr()
    one, zero = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    D = HvqTensorDst
    good = D(base, 0, 0, 32, 24, 0, 0, 0, 0)
    cases = [(good, 0, 2, one, zero), (good, 0, -1, one, zero), (good, 0, 0x100, one, zero), (good, 0, 0x102, one, zero),   # bad filter
             (good, 7, 1, one, zero),                                            # bad dtype
             (good, 0, 1, (1.0, float("nan"), 1.0), zero), (good, 0, 1, one, (0.0, 0.0, float("inf"))),
             (D(base, 0, 0, 32, 24, 1, 0, w, h), 0, 1, one, zero),               # crop leaves the picture on the right
             (D(base, 0, 0, 32, 24, 0, 1, w, h), 0, 1, one, zero),               # ... at the bottom
             (D(base, 0, 0, 32, 24, 0, 0, 8, 0), 0, 1, one, zero),               # empty crop
             (D(None, 0, 0, 32, 24, 0, 0, 0, 0), 0, 1, one, zero),
             (D(base, 0, 0, 16385, 1, 0, 0, 0, 0), 0, 1, one, zero),
             (D(base, 4 * 32 - 4, 0, 32, 24, 0, 0, 0, 0), 0, 1, one, zero),      # row pitch below dense
             (D(base + 2, 0, 0, 32, 24, 0, 0, 0, 0), 0, 1, one, zero)]           # pointer not a multiple of the element size
    for d, dtype, filt, mul, add in cases:
        a_s, a_o = (C.c_int * 1)(sid), (C.c_int * 1)(last)
        rc = lib().hvq_export_resampled(ctx._h, 1, a_s, a_o, dtype, filt, (C.c_float * 3)(*mul), (C.c_float * 3)(*add), C.byref(d),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == HVQ_E_ARG, (rc, dtype, filt, mul, add, [getattr(d, f) for f, _t in D._fields_])
    untouched(buf)
    # the well-formed call right after them works; filter 0 is the plain export
    ctx.export_float([sid], [last], buf, antialias=True)
    plain, fwd = _fresh(torch, (1, 3, 24, 32), "float32"), _fresh(torch, (1, 3, 24, 32), "float32")
    ctx.export_float([sid], [last], plain)
    ctx._export_float([sid], [last], fwd, None, (0, 0, 0), (1, 1, 1), 1 / 255, 0)
    torch.cuda.synchronize()
    assert not (bits_of(buf) == bits_of(torch.full((1,), SENTINEL))[0]).any()
    assert np.array_equal(bits_of(plain), bits_of(fwd)) and not np.array_equal(bits_of(plain), bits_of(buf))
    ctx.close_stream(sid)


def case_chain(torch, ctx):
    """export, export_float and export_float(antialias=True) back to back on one stream without a host synchronisation, then a
    flush that rewrites every slot: all three read their pictures whole (the shared export chain keeps the slots)"""
    from hvqm4_amd.container import parse_header, video_pictures
    from oracle import bridge
    from tests.export_float_ref import export_float_reference
    clip = _long_clip()
    hdr = parse_header(clip.data)
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(clip.data)]
    yuv = bridge.oracle_decode(clip.data, len(pics))
    w, h = hdr.width, hdr.height
    mul, add = _norm()
    sid = ctx.open_stream(w, h, 2, 2, hdr.is15, 3)
    for ft, p in pics[:3]:
        ctx.submit(sid, ft, p)
    ctx.flush()
    u8 = torch.zeros((3, 3, h, w), dtype=torch.uint8, device="cuda")
    plain = _fresh(torch, (3, 3, 120, 160), "float32")
    aa = {dt: _fresh(torch, (3, 3, 224, 224), dt) for dt in DTYPES}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())    # the destinations were filled on the current stream
    with torch.cuda.stream(side):
        ctx.export([sid] * 3, [0, 1, 2], u8, "rgbp")
        ctx.export_float([sid] * 3, [0, 1, 2], plain, mean=MEAN, std=STD)
        for dt in DTYPES:
            ctx.export_float([sid] * 3, [0, 1, 2], aa[dt], mean=MEAN, std=STD, antialias=True)
    for ft, p in pics[3:9]:
        ctx.submit(sid, ft, p)
    ctx.flush()                                      # rewrites every slot of the ring of 3
    ctx.replay(1)
    torch.cuda.synchronize()
    for k in range(3):
        planes = _rgbp(yuv[k], hdr)
        assert np.array_equal(u8[k].cpu().numpy(), planes), ("uint8", k)
        _same(plain[k], export_float_reference(yuv[k], w, h, 2, 2, (120, 160), None, mul, add, "float32"), ("plain", k))
        want = _want32(planes, (224, 224), None)
        for dt in DTYPES:
            _same(aa[dt][k], _bits(want, dt), ("antialias", dt, k))
    ctx.close_stream(sid)


def case_torch_sanity(torch, ctx):
    """F.interpolate(antialias=True) on the uint8 export with the same normalisation: within 0.1 of a 0..255 unit, scaled by mul"""
    import torch.nn.functional as F
    g = _golden()
    mul, add = _norm()
    for nm in ("wide296x160", "yuv422_296x160", "yuv444_13_portrait48x64"):
        data, hdr, n = g[nm]
        sid, hdr, n = _decode(ctx, data)
        w, h = hdr.width, hdr.height
        u8 = torch.zeros((n, 3, h, w), dtype=torch.uint8, device="cuda")
        ctx.export([sid] * n, list(range(n)), u8, "rgbp")
        for hw, crop in (((224, 224), None), ((h // 2, w // 2), None), ((20, 30), (3, 5, w - 9, h - 8))):
            out = torch.zeros((n, 3) + hw, dtype=torch.float32, device="cuda")
            ctx.export_float([sid] * n, list(range(n)), out, crop=crop, mean=MEAN, std=STD, antialias=True)
            src = u8.float()
            if crop:
                src = src[:, :, crop[1]:crop[1] + crop[3], crop[0]:crop[0] + crop[2]]
            ref = F.interpolate(src, size=hw, mode="bilinear", align_corners=False, antialias=True)
            m = torch.tensor(mul, device="cuda").view(1, 3, 1, 1)
            a = torch.tensor(add, device="cuda").view(1, 3, 1, 1)
            ref = ref * m + a
            torch.cuda.synchronize()
            worst = float(((out - ref).abs() / m).max())
            print(f"{nm} {hw} crop {crop}: worst difference {worst:.6f} of a 0..255 unit")
            assert worst <= 0.1, (nm, hw, crop, worst)
        ctx.close_stream(sid)


CASES = ["goldens_identity", "downscale", "body_agreement", "upscale", "mixed_batch", "pitched_and_store_forms", "refusals", "chain",
         "torch_sanity"]


# ------------------------------------------------------------------------------------------------------------ parent side
child_results = gpu_child.results_fixture(__name__, "export_aa", CHILD_TIMEOUT)


@pytest.mark.parametrize("case", CASES)
def test_export_aa(case, child_results):
    gpu_child.report(case, child_results)
