"""CPU: float export (hvq_export_tensors, Context.export_float).

* export_float_reference (tests/export_float_ref.py) restates the specification of include/hvqm4_amd.h in numpy float32; at the
  identity size with mul = 1, add = 0 it is export_reference's planar RGB as floats, exactly, on every golden clip.
* Its coordinate convention is torch's F.interpolate(mode="bilinear", align_corners=False): the two differ only in the float rounding
  of coordinates and the order of the blend.  Bound 0.1 in 0..255 units: the restatement against torch on exactly these sizes gave
  0.0035 at worst (0.0 at integer ratios); a half-sample or align_corners mistake shows as several units.
* The C entry point exists and refuses a NULL context.
* Context.export_float refuses malformed destinations, crops and normalisations before any library call, without a GPU.
* Known-answer ties of the float16 and bfloat16 roundings."""
import ctypes as C

import numpy as np
import pytest

from oracle import bridge
from tests.export_float_ref import bits_of, export_float_reference, resize_planes, to_dtype
from tests.test_export_cpu import export_reference, golden_clips

BOUND = 0.1


def test_identity_size_is_the_uint8_export_as_floats_on_every_golden():
    seen = 0
    for name, data, hdr, n in golden_clips():
        pics = bridge.oracle_decode(data, n)
        w, h = hdr.width, hdr.height
        for k in range(n):
            want = export_reference(pics[k], w, h, hdr.h_samp, hdr.v_samp, "rgbp").astype(np.float32)
            got = export_float_reference(pics[k], w, h, hdr.h_samp, hdr.v_samp, (h, w))
            assert got.dtype == np.uint32 and np.array_equal(got, want.view(np.uint32)), (name, k)
            seen += 1
        x0, y0, cw, ch = 3, 1, w - 4, h - 3                        # an odd-offset crop at its own size is the slice
        got = export_float_reference(pics[0], w, h, hdr.h_samp, hdr.v_samp, (ch, cw), crop=(x0, y0, cw, ch))
        assert np.array_equal(got, np.ascontiguousarray(want_slice(pics[0], hdr, x0, y0, cw, ch)).view(np.uint32)), name
    assert seen >= 100


def want_slice(yuv, hdr, x0, y0, cw, ch):
    return export_reference(yuv, hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, "rgbp")[:, y0:y0 + ch, x0:x0 + cw].astype(np.float32)


@pytest.mark.parametrize("src,out,crop", [
    ((48, 64), (24, 32), None), ((48, 64), (96, 128), None), ((48, 64), (37, 53), None),
    ((160, 296), (100, 177), None), ((480, 640), (224, 224), None), ((480, 640), (1080, 1920), None),
    ((480, 640), (224, 224), (37, 11, 403, 301)), ((160, 296), (64, 64), (200, 60, 96, 100)),
], ids=lambda v: "x".join(map(str, v)) if v else "whole")
def test_convention_is_torch_bilinear_align_corners_false(src, out, crop):
    import torch
    import torch.nn.functional as F
    h, w = src
    rng = np.random.default_rng(h * 7 + w + out[0])
    p = rng.integers(0, 256, (3, h, w)).astype(np.float32)
    if crop:
        x0, y0, cw, ch = crop
        p = np.ascontiguousarray(p[:, y0:y0 + ch, x0:x0 + cw])
    mine = resize_planes(p, out)
    ref = F.interpolate(torch.from_numpy(p)[None], size=out, mode="bilinear", align_corners=False, antialias=False)[0].numpy()
    worst = float(np.abs(mine - ref).max())
    print(f"{src} -> {out} crop {crop}: max abs difference {worst:.6f}")
    assert worst <= BOUND


def test_symbol_exists_and_refuses_a_null_context():
    from hvqm4_amd._lib import HVQ_E_ARG, lib
    l = lib()
    assert hasattr(l, "hvq_export_tensors")
    one = (C.c_float * 3)(1, 1, 1)
    assert l.hvq_export_tensors(None, 0, None, None, 0, one, one, None, None) == HVQ_E_ARG
    assert l.hvq_export_tensors(None, 1, None, None, 0, one, one, None, None) == HVQ_E_ARG


def test_struct_layout_matches_the_header():
    from hvqm4_amd.export import HvqTensorDst
    assert C.sizeof(HvqTensorDst) == 48
    assert [getattr(HvqTensorDst, f).offset for f in ("ptr", "row_pitch", "plane_pitch", "out_w", "out_h", "crop_x", "crop_y",
                                                      "crop_w", "crop_h")] == [0, 8, 16, 24, 28, 32, 36, 40, 44]


class _NoLibrary:
    """a Context that was never created: any library call would fail with an HvqError, not with the error under test"""

    def __new__(cls, geoms):
        from hvqm4_amd.batch import Context
        ctx = Context.__new__(Context)
        ctx._h = C.c_void_p()
        ctx._geom = dict(enumerate(geoms))
        return ctx


def test_export_float_validation_refuses_before_any_library_call():
    import torch
    w, h = 64, 48
    ctx = _NoLibrary([(w, h), (w, h)])
    ok = torch.zeros(3, 24, 32)

    def refused(exc, match, out, sids=(0,), **kw):
        with pytest.raises(exc, match=match):
            ctx.export_float(list(sids), [0] * len(sids), out, **kw)

    refused(ValueError, "not a GPU", [ok])                                       # well formed: refused for its device alone
    refused(ValueError, "not a GPU", torch.zeros(2, 3, h, w, dtype=torch.float16), sids=(0, 1))
    refused(ValueError, "not a GPU", [torch.zeros(3, 24, 32, dtype=torch.bfloat16)], crop=(1, 3, 63, 45))
    refused(ValueError, "not a GPU", [torch.zeros(3, 30, 40)[:, 3:27, 5:37]])     # a pitched view at element alignment
    refused(TypeError, "float32, float16 or bfloat16", [torch.zeros(3, 24, 32, dtype=torch.uint8)])
    refused(TypeError, "float32, float16 or bfloat16", [torch.zeros(3, 24, 32, dtype=torch.float64)])
    refused(TypeError, "one dtype", [ok, torch.zeros(3, 24, 32, dtype=torch.float16)], sids=(0, 1))
    refused(TypeError, "torch tensor", np.zeros((1, 3, 24, 32), np.float32))
    refused(TypeError, "not a torch tensor", [np.zeros((3, 24, 32), np.float32)])
    refused(ValueError, "dimensions", [torch.zeros(24, 32)])
    refused(ValueError, "dimensions", torch.zeros(3, 24, 32))                     # a batch tensor needs the N dimension
    refused(ValueError, "channels", [torch.zeros(4, 24, 32)])
    refused(ValueError, "channels", [torch.zeros(24, 32, 3)])                     # HWC
    refused(ValueError, "column stride", [torch.zeros(24, 32, 3).permute(2, 0, 1)])
    refused(ValueError, "column stride", [torch.zeros(3, 24, 64)[:, :, ::2]])
    refused(ValueError, "overlap", [torch.zeros(3, 1, 32).expand(3, 24, 32)])     # rows on top of each other
    refused(ValueError, "overlap", [torch.zeros(1, 24, 32).expand(3, 24, 32)])    # planes on top of each other
    refused(ValueError, "outside", [torch.zeros(3, 0, 32)])
    refused(ValueError, "pictures", torch.zeros(1, 3, 24, 32), sids=(0, 1))
    refused(ValueError, "destinations", [ok], sids=(0, 1))
    with pytest.raises(ValueError, match="ordinals"):
        ctx.export_float([0], [0, 1], [ok])
    for bad in ((0.0, 1, 1), (1, float("nan"), 1), (1, 1, float("inf"))):
        refused(ValueError, "std", [ok], std=bad)
    refused(ValueError, "mean", [ok], mean=(0, float("nan"), 0))
    refused(ValueError, "scale", [ok], scale=float("inf"))
    refused(ValueError, "float32", [ok], std=(1e-45, 1, 1), scale=1e10)           # scale / std overflows float32
    for bad in ((0, 0, w + 1, h), (1, 0, w, h), (0, 1, w, h), (-1, 0, 8, 8), (0, 0, 0, 8), (0, 0, 8, 0), (60, 40, 8, 8)):
        refused(ValueError, "crop", [ok], crop=bad)
    refused(ValueError, "crop", [ok, ok], sids=(0, 1), crop=[None, (0, 0, 65, 8)])
    refused(ValueError, "crops", [ok, ok], sids=(0, 1), crop=[None])
    refused(ValueError, "crop", [ok], crop=(0.5, 0, 8, 8))
    from hvqm4_amd._lib import HvqError
    with pytest.raises(HvqError, match="bad stream"):
        ctx.export_float([7], [0], [ok])
    ctx._h = C.c_void_p()                                                          # nothing to destroy


def test_normalisation_is_computed_in_double_and_rounded_once():
    from hvqm4_amd.export import normalisation
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    mul, add = normalisation(mean, std)
    for c in range(3):
        assert mul[c] == float(np.float32((1 / 255) / std[c])) and add[c] == float(np.float32(-mean[c] / std[c]))
    assert normalisation() == ([float(np.float32(1 / 255))] * 3, [0.0] * 3)
    assert normalisation(scale=1.0, std=(2, 4, 8), mean=(1, 1, 1)) == ([0.5, 0.25, 0.125], [-0.5, -0.25, -0.125])


def test_known_answer_ties_of_the_16_bit_roundings():
    f32 = lambda *v: np.array(v, dtype=np.float32)
    # float16: 11 significant bits -- above 2048 the spacing is 2, a tie goes to the even significand
    got = to_dtype(f32(2049, 2051, 2050.5, 2049.001, 65520, 65519.996, 2 ** -25, 2 ** -25 * 1.0001, -2049), "float16").view(np.float16)
    want = np.array([2048, 2052, 2050, 2050, np.inf, 65504, 0, 2 ** -24, -2048], dtype=np.float16)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    # bfloat16: 8 significant bits -- the raw bits are the top half of the float32, ties to the even top half
    src = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F80FFFF, 0x3F817FFF, 0x7F7FFFFF, 0xBF808000, 0x00008000, 0x00018000],
                   dtype=np.uint32).view(np.float32)
    want = np.array([0x3F80, 0x3F82, 0x3F81, 0x3F81, 0x3F81, 0x7F80, 0xBF80, 0x0000, 0x0002], dtype=np.uint16)
    assert np.array_equal(to_dtype(src, "bfloat16"), want)
    import torch
    assert np.array_equal(bits_of(torch.from_numpy(src).to(torch.bfloat16)), want)
    # the integer restatement of round-to-nearest-even the kernel uses, over a sweep of finite values and the infinities
    rng = np.random.default_rng(5)
    b = np.concatenate([rng.integers(0, 0x7F800000, 200000, dtype=np.uint32), rng.integers(0x80000000, 0xFF800000, 200000, dtype=np.uint32),
                        np.array([0x7F800000, 0xFF800000, 0x7F7FFFFF, 0, 0x80000000], dtype=np.uint32)])
    mine = ((b.astype(np.uint64) + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    assert np.array_equal(mine, to_dtype(b.view(np.float32), "bfloat16"))
