"""CPU: picture export (hvq_export_pictures, Context.export).

* export_reference restates the export kernel's arithmetic in numpy for the three samplings and the three formats; at 4:2:0 RGB24
  it equals the oracle's dumpRGB on every 4:2:0 golden clip, which ties the generalised kernel to the pinned reference.
* The C entry point exists and refuses a NULL context.
* Context.export refuses malformed destinations before any library call (hvqm4_amd.export.destinations, no GPU needed)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import bridge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MANIFEST = json.load(open(os.path.join(ROOT, "tests", "golden", "manifest.json")))


def export_reference(yuv: np.ndarray, w: int, h: int, hs: int, vs: int, fmt: str) -> np.ndarray:
    """Y|U|V of sampling (h_samp, v_samp) = (hs, vs) -> "rgb" [h, w, 3], "rgbp" / "yuv444p" [3, h, w].  Output sample (i, j) reads
    chroma [(i >> hshift) * (w >> wshift) + (j >> wshift)]; RGB in float32, one rounding per operation, floor, saturate."""
    ws, hsh = int(hs == 2), int(vs == 2)
    cw, ch = w >> ws, h >> hsh
    yuv = np.asarray(yuv, dtype=np.uint8)
    y = yuv[:w * h].reshape(h, w)
    u = yuv[w * h:w * h + cw * ch].reshape(ch, cw)
    v = yuv[w * h + cw * ch:w * h + 2 * cw * ch].reshape(ch, cw)
    rows, cols = np.arange(h) >> hsh, np.arange(w) >> ws
    uf, vf = u[rows][:, cols], v[rows][:, cols]
    if fmt == "yuv444p":
        return np.stack([y, uf, vf])
    f32 = np.float32
    yy = y.astype(f32)
    U = uf.astype(f32) - f32(128)
    V = vf.astype(f32) - f32(128)
    planes = (yy + f32(1.402) * V, (yy - f32(0.34414) * U) - f32(0.71414) * V, yy + f32(1.772) * U)
    out = np.stack([np.clip(np.floor(p), 0, 255).astype(np.uint8) for p in planes])
    assert all(p.dtype == np.float32 for p in planes)
    return out if fmt == "rgbp" else np.ascontiguousarray(out.transpose(1, 2, 0))


def golden_clips():
    from hvqm4_amd.container import parse_header
    for name, c in MANIFEST["clips"].items():
        if "file" not in c:                                     # catalogue entries without a committed file
            continue
        data = open(os.path.join(ROOT, "tests", "golden", c["file"]), "rb").read()
        yield name, data, parse_header(data), len(c["frame_types"])


def test_reference_restatement_equals_the_oracle_dumprgb_on_the_420_goldens():
    n420 = 0
    for name, data, hdr, n in golden_clips():
        if (hdr.h_samp, hdr.v_samp) != (2, 2):
            continue
        n420 += 1
        pics = bridge.oracle_decode(data, n)
        for k in range(n):
            mine = export_reference(pics[k], hdr.width, hdr.height, 2, 2, "rgb")
            want = bridge.oracle_rgb(pics[k], hdr.width, hdr.height).reshape(hdr.height, hdr.width, 3)
            assert np.array_equal(mine, want), (name, k)
            assert np.array_equal(export_reference(pics[k], hdr.width, hdr.height, 2, 2, "rgbp"), want.transpose(2, 0, 1))
    assert n420 >= 20


@pytest.mark.parametrize("hs,vs", [(2, 2), (2, 1), (1, 1)], ids=["420", "422", "444"])
def test_reference_restatement_index_rule(hs, vs):
    """chroma sample (i >> hshift, j >> wshift) serves output (i, j); Y passes through; a constant grey converts to itself"""
    w, h = 16, 8
    ws, hsh = int(hs == 2), int(vs == 2)
    cw, ch = w >> ws, h >> hsh
    rng = np.random.default_rng(hs * 10 + vs)
    yuv = rng.integers(0, 256, w * h + 2 * cw * ch, dtype=np.uint8)
    p = export_reference(yuv, w, h, hs, vs, "yuv444p")
    u = yuv[w * h:w * h + cw * ch].reshape(ch, cw)
    for i in range(h):
        for j in range(w):
            assert p[1, i, j] == u[i >> hsh, j >> ws]
    assert np.array_equal(p[0], yuv[:w * h].reshape(h, w))
    grey = np.concatenate([np.full(w * h, 77, np.uint8), np.full(2 * cw * ch, 128, np.uint8)])
    assert (export_reference(grey, w, h, hs, vs, "rgb") == 77).all()


def test_export_symbol_exists_and_refuses_a_null_context():
    from hvqm4_amd._lib import HVQ_E_ARG, lib
    l = lib()
    assert hasattr(l, "hvq_export_pictures")
    assert l.hvq_export_pictures(None, 0, None, None, 0, None, None) == HVQ_E_ARG
    assert l.hvq_export_pictures(None, 1, None, None, 0, None, None) == HVQ_E_ARG


def _dst(*args, **kw):
    from hvqm4_amd.export import destinations
    return destinations(*args, **kw)


def test_export_validation_refuses_malformed_destinations():
    import torch
    w, h = 64, 48
    g = [(w, h)]
    ok_hwc = torch.zeros(h, w, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="not a GPU"):                      # a well-formed CPU tensor: refused for its device alone
        _dst([ok_hwc], g, "rgb")
    with pytest.raises(ValueError, match="not a GPU"):
        _dst(torch.zeros(1, 3, h, w, dtype=torch.uint8), g, "rgbp")
    with pytest.raises(TypeError, match="uint8"):
        _dst([torch.zeros(h, w, 3, dtype=torch.float32)], g, "rgb")
    with pytest.raises(ValueError, match="dimensions"):
        _dst([torch.zeros(h * w * 3, dtype=torch.uint8)], g, "rgb")
    with pytest.raises(ValueError, match="dimensions"):
        _dst(torch.zeros(h, w, 3, dtype=torch.uint8), g, "rgb")            # a batch tensor needs the N dimension
    with pytest.raises(ValueError, match="shape"):
        _dst([torch.zeros(h, w, 4, dtype=torch.uint8)], g, "rgb")           # channel count 4
    with pytest.raises(ValueError, match="shape"):
        _dst([torch.zeros(4, h, w, dtype=torch.uint8)], g, "yuv444p")
    with pytest.raises(ValueError, match="shape"):
        _dst([torch.zeros(h, w, 3, dtype=torch.uint8)], g, "rgbp")          # HWC handed to a planar format
    with pytest.raises(ValueError, match="shape"):
        _dst([torch.zeros(h - 8, w, 3, dtype=torch.uint8)], g, "rgb")       # too small for the picture
    with pytest.raises(ValueError, match="stride"):
        _dst([torch.zeros(3, h, w, dtype=torch.uint8).permute(1, 2, 0)], g, "rgb")   # HWC view of planar memory
    canvas = torch.zeros(h, w + 1, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="multiples of 4"):
        _dst([canvas[:, :w]], g, "rgb")                                     # row pitch 195
    canvas = torch.zeros(h, w + 4, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="multiples of 4"):
        _dst([canvas[:, 1:w + 1]], g, "rgb")                                # pointer 3 bytes into a row
    with pytest.raises(ValueError, match="not a GPU"):
        _dst([canvas[:, 4:w + 4]], g, "rgb")                                # a legal crop: only the device is wrong
    with pytest.raises(ValueError, match="pictures"):
        _dst(torch.zeros(2, h, w, 3, dtype=torch.uint8), g, "rgb")          # N mismatch, batch tensor
    with pytest.raises(ValueError, match="destinations"):
        _dst([ok_hwc, ok_hwc], g, "rgb")                                    # N mismatch, list
    with pytest.raises(ValueError, match="fmt"):
        _dst([ok_hwc], g, "bgr")
    with pytest.raises(TypeError):
        _dst(np.zeros((h, w, 3), np.uint8), g, "rgb")


def test_export_struct_layout_matches_the_header():
    from hvqm4_amd.export import HvqExportDst
    assert C.sizeof(HvqExportDst) == 24
    assert (HvqExportDst.row_pitch.offset, HvqExportDst.plane_pitch.offset) == (8, 16)
