"""CPU: antialiased float export (hvq_export_resampled with HVQ_FILTER_TRIANGLE, Context.export_float(antialias=True)).

* hvq_resample_table (host only) equals the numpy table of tests/export_aa_ref.py exactly: first, count and the raw weight bits.
* Its length query, HVQ_E_ARG and HVQ_E_OVERFLOW; every count >= 1, first + count <= n_src, weights >= 0.
* At the crop's own size the restatement is export_float_reference bit for bit on every golden clip, in all three dtypes.
* Against torch's CPU F.interpolate(mode="bilinear", antialias=True, align_corners=False), which builds its weights in float32, the
  restatement stays within 0.01 of a 0..255 unit (about 2e-3 at worst when the bound was set: a margin of 5; a bound on the reference
  alone).
* Struct / enum values match the header, the new symbols are exported and refuse a NULL context.
* export_float(antialias=True) refuses malformed calls before any library call, on the cases of tests/test_export_float_cpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import bridge
from tests.export_aa_ref import export_aa_reference, resize_planes_aa, table
from tests.export_float_ref import export_float_reference
from tests.test_export_cpu import golden_clips

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(64, 32), (64, 23), (296, 53), (640, 224), (480, 224), (64, 128), (24, 50), (1280, 224), (64, 7), (64, 1), (1, 5), (65535, 1),
         (3, 16384)]
TORCH_BOUND = 0.01


@pytest.mark.parametrize("n_src,n_out", PAIRS, ids=lambda v: str(v))
def test_table_equals_the_numpy_table_exactly(n_src, n_out):
    from hvqm4_amd.export import resample_table
    first, count, w = resample_table(n_src, n_out)
    rf, rc, rw = table(n_src, n_out)
    assert first.dtype == np.int32 and count.dtype == np.int32 and w.dtype == np.float32
    assert np.array_equal(first, rf) and np.array_equal(count, rc)
    assert w.shape == rw.shape and np.array_equal(w.view(np.uint32), rw.view(np.uint32))
    assert (count >= 1).all() and (first >= 0).all() and (first.astype(np.int64) + count <= n_src).all()
    assert (w >= 0).all() and len(w) == int(count.sum())
    support = max(n_src / n_out, 1.0)
    assert int(count.max()) <= 2 * int(np.ceil(support)) + 1
    start = np.concatenate([[0], np.cumsum(count)])
    sums = np.add.reduceat(w.astype(np.float64), start[:-1])
    assert np.abs(sums - 1).max() < 1e-3 * max(1, count.max()) ** 0.5        # normalised rows (float32 rounding of each weight only)
    if n_src == n_out:
        assert (w.reshape(-1)[start[:-1]] == 1).all()


def test_identity_rows_are_one_zero():
    from hvqm4_amd.export import resample_table
    first, count, w = resample_table(48, 48)
    assert np.array_equal(first, np.arange(48)) and np.array_equal(count, [2] * 47 + [1])
    assert np.array_equal(w, np.array([1, 0] * 47 + [1], dtype=np.float32))


def test_length_query_and_refusals():
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_OVERFLOW, HVQ_OK, lib
    l = lib()
    need = C.c_size_t(0)
    assert l.hvq_resample_table(640, 224, None, None, None, 0, C.byref(need)) == HVQ_OK
    assert need.value == len(table(640, 224)[2])
    first, count = (C.c_int32 * 224)(), (C.c_int32 * 224)()
    w = (C.c_float * (need.value + 1))(*([-3.0] * (need.value + 1)))
    got = C.c_size_t(0)
    assert l.hvq_resample_table(640, 224, first, count, w, need.value - 1, C.byref(got)) == HVQ_E_OVERFLOW
    assert got.value == need.value and all(v == -3.0 for v in w), "a refused call writes no weight"
    assert l.hvq_resample_table(640, 224, first, count, w, need.value, None) == HVQ_OK
    assert w[need.value] == -3.0 and np.array_equal(np.frombuffer(w, dtype=np.float32)[:need.value], table(640, 224)[2])
    for n_src, n_out in ((0, 4), (-1, 4), (65536, 4), (4, 0), (4, -2), (4, 16385)):
        assert l.hvq_resample_table(n_src, n_out, None, None, None, 0, C.byref(need)) == HVQ_E_ARG, (n_src, n_out)
        assert l.hvq_resample_table(n_src, n_out, first, count, w, need.value, C.byref(need)) == HVQ_E_ARG, (n_src, n_out)
    assert l.hvq_resample_table(64, 32, None, None, None, 0, None) == HVQ_E_ARG          # a query with nowhere to answer
    assert l.hvq_resample_table(64, 32, None, None, w, 4096, None) == HVQ_E_ARG
    from hvqm4_amd._lib import HvqError
    from hvqm4_amd.export import resample_table
    with pytest.raises(HvqError):
        resample_table(65536, 1)


def test_body_choice_is_host_computable():
    """the tiled body takes downscales whose tiles' source rows fit its LDS rows; everything else goes the direct way"""
    from hvqm4_amd._lib import HVQ_E_ARG, lib
    q = lib().hvq_resample_tile_rows
    assert q(640, 480, 224, 224) == 16 and q(640, 480, 320, 240) == 16 and q(296, 160, 148, 80) == 16
    assert q(640, 480, 160, 120) == 8                                    # 4x: 16 rows need 17 * 4 + 1 source rows, 8 need 37
    assert q(296, 160, 1, 1) == 0 and q(296, 160, 296, 7) == 0 and q(1280, 64, 1280, 7) == 0 and q(1280, 64, 1, 1) == 0
    assert q(64, 48, 64, 48) == 0 and q(64, 48, 128, 96) == 0 and q(64, 48, 67, 49) == 0
    assert q(64, 48, 9, 48) == 16                                        # a downscale along x alone
    assert q(0, 48, 9, 48) == HVQ_E_ARG and q(64, 48, 9, 16385) == HVQ_E_ARG
    # the bound itself: the largest footprint of any tile against the rows of the table
    for ch, oh in ((160, 80), (160, 37), (160, 33), (160, 32), (160, 31), (160, 20), (160, 19), (480, 224), (59, 7), (13, 7)):
        first, count, _w = table(ch, oh)
        want = 0
        for th in (16, 8):
            worst = max(int(first[min(i0 + th, oh) - 1] + count[min(i0 + th, oh) - 1] - first[i0]) for i0 in range(0, oh, th))
            if worst <= 40:
                want = th
                break
        assert q(296, ch, 100, oh) == want, (ch, oh)


def test_identity_size_is_the_plain_export_bit_for_bit_on_every_golden():
    seen = 0
    for name, data, hdr, n in golden_clips():
        pics = bridge.oracle_decode(data, n)
        w, h = hdr.width, hdr.height
        mul, add = (0.017, 0.0175, 0.0174), (-2.1, -2.0, -1.8)
        for k in range(n):
            for dt in ("float32", "float16", "bfloat16"):
                want = export_float_reference(pics[k], w, h, hdr.h_samp, hdr.v_samp, (h, w), None, mul, add, dt)
                got = export_aa_reference(pics[k], w, h, hdr.h_samp, hdr.v_samp, (h, w), None, mul, add, dt)
                assert got.dtype == want.dtype and np.array_equal(got, want), (name, k, dt)
            seen += 1
        crop = (3, 1, w - 4, h - 3)
        want = export_float_reference(pics[0], w, h, hdr.h_samp, hdr.v_samp, (h - 3, w - 4), crop)
        assert np.array_equal(export_aa_reference(pics[0], w, h, hdr.h_samp, hdr.v_samp, (h - 3, w - 4), crop), want), name
    assert seen >= 100


@pytest.mark.parametrize("src,out", [((48, 64), (24, 32)), ((48, 64), (17, 23)), ((160, 296), (37, 53)), ((480, 640), (224, 224)),
                                     ((48, 64), (96, 128)), ((40, 24), (13, 50)), ((64, 1280), (7, 224)), ((48, 64), (48, 64)),
                                     ((48, 64), (1, 1))], ids=lambda v: "x".join(map(str, v)))
def test_restatement_is_torch_antialias_within_the_bound(src, out):
    import torch
    import torch.nn.functional as F
    h, w = src
    rng = np.random.default_rng(h * 7 + w + out[0])
    p = rng.integers(0, 256, (3, h, w)).astype(np.float32)
    mine = resize_planes_aa(p, out)
    ref = F.interpolate(torch.from_numpy(p)[None], size=out, mode="bilinear", align_corners=False, antialias=True)[0].numpy()
    worst = float(np.abs(mine - ref).max())
    print(f"{src} -> {out}: max abs difference {worst:.6f}")
    assert worst <= TORCH_BOUND


def test_symbols_exist_and_refuse_a_null_context():
    from hvqm4_amd._lib import HVQ_E_ARG, lib
    l = lib()
    assert hasattr(l, "hvq_export_resampled") and hasattr(l, "hvq_resample_table") and hasattr(l, "hvq_resample_tile_rows")
    one = (C.c_float * 3)(1, 1, 1)
    for filt in (0, 1, 0x101):
        assert l.hvq_export_resampled(None, 0, None, None, 0, filt, one, one, None, None) == HVQ_E_ARG
        assert l.hvq_export_resampled(None, 1, None, None, 0, filt, one, one, None, None) == HVQ_E_ARG
    assert l.hvq_export_resampled(None, 0, None, None, 0, 2, one, one, None, None) == HVQ_E_ARG


def test_values_match_the_header():
    from hvqm4_amd import export
    text = open(os.path.join(ROOT, "include", "hvqm4_amd.h")).read()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+(HVQ_FILTER_\w+)\s+(\w+)", text)}
    assert defs == {"HVQ_FILTER_BILINEAR": export.FILTER_BILINEAR, "HVQ_FILTER_TRIANGLE": export.FILTER_TRIANGLE,
                    "HVQ_FILTER_TRIANGLE_DIRECT": export.FILTER_TRIANGLE_DIRECT} == \
        {"HVQ_FILTER_BILINEAR": 0, "HVQ_FILTER_TRIANGLE": 1, "HVQ_FILTER_TRIANGLE_DIRECT": 0x101}
    assert C.sizeof(export.HvqTensorDst) == 48                      # hvq_export_resampled reuses it unchanged
    desc = open(os.path.join(ROOT, "hvqm4_amd", "csrc", "hvq_desc.h")).read()
    assert "sizeof(HvqResampleJob) == 96" in desc


class _NoLibrary:
    """a Context that was never created: any library call would fail with an HvqError, not with the error under test"""

    def __new__(cls, geoms):
        from hvqm4_amd.batch import Context
        ctx = Context.__new__(Context)
        ctx._h = C.c_void_p()
        ctx._geom = dict(enumerate(geoms))
        return ctx


def test_export_float_antialias_validation_refuses_before_any_library_call():
    import torch
    w, h = 64, 48
    ctx = _NoLibrary([(w, h), (w, h)])
    ok = torch.zeros(3, 24, 32)

    def refused(exc, match, out, sids=(0,), **kw):
        with pytest.raises(exc, match=match):
            ctx.export_float(list(sids), [0] * len(sids), out, antialias=True, **kw)

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
        ctx.export_float([0], [0, 1], [ok], antialias=True)
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
        ctx.export_float([7], [0], [ok], antialias=True)
    ctx._h = C.c_void_p()                                                          # nothing to destroy
