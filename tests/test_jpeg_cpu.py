"""CPU: JPEG files of pictures (hvq_encode_jpeg, Context.encode_jpeg, hvqm4_amd/jpeg.py) without a GPU.

  - tests/jpeg_ref.py, the host restatement the GPU tests compare with, against the header text: the 629 header bytes and the order of the
    segments, DRI, the RST markers, an all-128 picture, the sign patterns of the 64 basis functions (the range argument of the text), ZRLs;
  - hvqm4_amd.jpeg.encode against it on the oracle's pictures of six golden clips at four qualities; quant_tables, header, bound, segments;
  - the library's hvq_jpeg_header / hvq_jpeg_bound against the Python ones, its argument checks without a device, the argument checks of
    Context.encode_jpeg that need no device;
  - an independent decoder (Pillow, when it is installed): every file opens, has the stream's size, decodes in YCbCr, and at qualities 50
    and 90 loses no more than 0.5 dB of luma PSNR against Pillow's own encoder on the same planes;
  - the runtime's entry point linked UNCHANGED against the CPU fake device of tests/test_fake_device.py (its source lists and flags, with
    tests/native/fake_jpeg_driver.cpp in the place of fake_driver.cpp and tests/native/fake_jpeg.cpp added: scalar bodies of the three
    launches that reach memory only through fake_span, when they run), under both schedules, plain and as a stand-alone AddressSanitizer +
    UndefinedBehaviorSanitizer program.  The driver judges nothing: every file it read back is compared here with jpeg_ref on the oracle's
    pictures.  The same program checks the division helper of hvq_jpeg.h exhaustively.

The issue that asked for this feature says that the sign pattern of basis (7, 7) alone gives three ZRLs before coefficient 63.  It does
not: that pattern is a checkerboard, whose transform is non-zero at all 16 odd-odd frequencies (F[7][7] = 837, F[5][7] = 294, ... F[1][1] =
33), and at no quality does it code more than two ZRLs.  The three-ZRL case is tested on the basis function (7, 7) itself instead, sampled
at an amplitude of 100: at quality 50 coefficient 63 is then the block's only non-zero AC coefficient.
"""
import io
import math
import os
import re

import numpy as np
import pytest

import tests.test_fake_device as fd
from tests import jpeg_ref
from tests.jpeg_ref import cached, jpeg_reference

NATIVE = fd.NATIVE
CXX_SOURCES = [s for s in fd.CXX_SOURCES if os.path.basename(s) != "fake_driver.cpp"] + \
              [os.path.join(NATIVE, "fake_jpeg.cpp"), os.path.join(NATIVE, "fake_jpeg_driver.cpp")]
SIX = ["gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "ip8"]
QUALITIES = (1, 50, 90, 100)


def _geometry(name):
    from hvqm4_amd.container import parse_header
    hdr = parse_header(open(os.path.join(fd.GOLDEN, fd.CLIPS[name]["file"]), "rb").read())
    return hdr.width, hdr.height, hdr.h_samp, hdr.v_samp


def _expected(name, k, quality):
    w, h, hs, vs = _geometry(name)
    return cached((name, k), fd.oracle_pictures(name)[k], w, h, quality, hs, vs)


def _entropy(data):
    """the entropy data of a file, split at its RST markers: (the intervals, the markers)"""
    from hvqm4_amd.jpeg import segments
    segs = segments(data)
    sos = [s for s in segs if s[0] == 0xDA][0]
    cuts = [sos[1] + 2 + 2 + sos[2]] + [s[1] for s in segs if 0xD0 <= s[0] <= 0xD7 or s[0] == 0xD9]
    marks = [s[0] for s in segs if 0xD0 <= s[0] <= 0xD7]
    return [data[cuts[0]:cuts[1]]] + [data[a + 2:b] for a, b in zip(cuts[1:-1], cuts[2:])], marks


# ------------------------------------------------------------------------------------------------- the reference against the text
def test_reference_header_and_segment_order():
    from hvqm4_amd.jpeg import segments
    for w, h, hs, vs in [(64, 48, 2, 2), (296, 160, 2, 1), (48, 64, 1, 1), (24, 40, 2, 2), (8, 8, 2, 2)]:
        for q in QUALITIES:
            hd = jpeg_ref.header(w, h, hs, vs, q)
            assert len(hd) == 629 == jpeg_ref.HEADER_BYTES
            pic = np.full(w * h + 2 * (w // hs) * (h // vs), 77, dtype=np.uint8)
            f = jpeg_reference(pic, w, h, q, hs, vs)
            assert f[:629] == hd and f[-2:] == b"\xff\xd9"
            segs = segments(f)
            mw, mh = jpeg_ref.mcus(w, h, hs, vs)
            assert [s[0] for s in segs[:11]] == [0xD8, 0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
            assert [s[0] for s in segs[11:]] == [0xD0 + (j & 7) for j in range(mh - 1)] + [0xD9], "RST cycles mod 8, none behind the last interval"
            at = {m: o for m, o, _n in segs[:11]}
            assert f[at[0xE0] + 4:at[0xE0] + 18] == b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
            assert f[at[0xDD] + 4:at[0xDD] + 6] == mw.to_bytes(2, "big"), "DRI == mw"
            sof = f[at[0xC0] + 4:at[0xC0] + 4 + 15]
            assert sof == bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, hs << 4 | vs, 0, 2, 0x11, 1, 3, 0x11, 1])
            dht = [f[o + 4] for m, o, _n in segs[:11] if m == 0xC4]
            assert dht == [0x00, 0x10, 0x01, 0x11]
            dqt = [(f[o + 4], f[o + 5:o + 69]) for m, o, _n in segs[:11] if m == 0xDB]
            assert [d[0] for d in dqt] == [0, 1]
            assert list(dqt[0][1]) == [jpeg_ref.quant_table(jpeg_ref.Q_LUMA, q)[z] for z in jpeg_ref.ZIGZAG]
            assert f[at[0xDA] + 4:at[0xDA] + 14] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    # 296 x 160 at 4:2:2: 20 intervals, the markers wrap past 7
    assert jpeg_ref.mcus(296, 160, 2, 1) == (19, 20)


def test_reference_all_128_is_dc_size_0_and_eob_everywhere():
    for w, h, hs, vs in [(64, 48, 2, 2), (24, 40, 2, 2), (48, 64, 1, 1), (296, 160, 2, 1)]:
        pic = np.full(w * h + 2 * (w // hs) * (h // vs), 128, dtype=np.uint8)
        st = {}
        f = jpeg_reference(pic, w, h, 90, hs, vs, st)
        assert st["max_ac"] == 0 and st["max_dc"] == 0 and st["min_dc"] == 0 and st["max_dc_size"] == 0 and st["zrl"] == 0
        mw, mh = jpeg_ref.mcus(w, h, hs, vs)
        # Y: DC size 0 = 00, EOB = 1010; Cb, Cr: DC size 0 = 00, EOB = 00
        bits = ("001010" * (hs * vs) + "0000" * 2) * mw
        bits += "1" * (-len(bits) % 8)
        want = int(bits, 2).to_bytes(len(bits) // 8, "big").replace(b"\xff", b"\xff\x00")
        iv, marks = _entropy(f)
        assert iv == [want] * mh and len(marks) == mh - 1


def test_reference_sign_patterns_stay_within_the_coding_limits():
    """the range argument of the header text, on the sign pattern of every basis function and its inverse at quality 100 (Q = 1 everywhere:
    the coefficients are the transform's values)"""
    pats = jpeg_ref.basis_sign_patterns()
    worst_ac, lo, hi = 0, 0, 0
    for p in pats:
        F = jpeg_ref.fdct(p.astype(np.int64) - 128)
        worst_ac = max(worst_ac, int(np.abs(F.reshape(64)[1:]).max()))
        lo, hi = min(lo, int(F[0, 0])), max(hi, int(F[0, 0]))
    assert worst_ac == 1020 and (lo, hi) == (-1024, 1016)
    assert 1020 < 1 << 10 and hi - lo < 1 << 11, "AC sizes <= 10, DC difference sizes <= 11"
    st = {}
    f = jpeg_reference(jpeg_ref.basis_picture(), 64, 128, 100, 1, 1, st)           # jpeg_reference asserts the sizes itself
    assert st["max_ac"] == 1020 and st["max_ac_size"] == 10 and st["max_dc_size"] == 11 and st["zrl"] > 100
    assert f.count(b"\xff\x00") > 0, "the patterns produce stuffed bytes"
    # the checkerboard (the sign pattern of (7, 7)): non-zero at all 16 odd-odd frequencies, no ZRL at quality 100
    F = jpeg_ref.fdct(pats[126].astype(np.int64) - 128)
    assert F[7, 7] == 837 and all((F[k, l] != 0) == (k % 2 == 1 and l % 2 == 1) for k in range(8) for l in range(8) if (k, l) != (0, 0))


def test_reference_three_zrls_before_coefficient_63():
    """a block whose only non-zero AC coefficient is the last one: run 62 = ZRL ZRL ZRL, then (14, size), and no EOB"""
    y = np.array([[round(128 + 100 * math.cos((2 * r + 1) * 7 * math.pi / 16) * math.cos((2 * c + 1) * 7 * math.pi / 16)) for c in range(8)] for r in range(8)])
    pic = np.concatenate([y.reshape(-1), np.full(128, 128)]).astype(np.uint8)
    st = {}
    f = jpeg_reference(pic, 8, 8, 50, 1, 1, st)
    z = jpeg_ref.fdct(y.astype(np.int64) - 128).reshape(64)
    q = jpeg_ref.quant_table(jpeg_ref.Q_LUMA, 50)
    co = [int(np.sign(v)) * ((abs(int(v)) + (q[i] >> 1)) // q[i]) for i, v in enumerate(z)]
    assert [i for i, v in enumerate(co) if v] == [63] and st["zrl"] == 3
    ha, hd = jpeg_ref.huffman_codes(jpeg_ref.AC_LUMA), jpeg_ref.huffman_codes(jpeg_ref.DC_LUMA)
    v, s = co[63], abs(co[63]).bit_length()
    tok = [hd[0]] + [ha[0xF0]] * 3 + [ha[14 << 4 | s], (v if v > 0 else v + (1 << s) - 1, s)] + [(0, 2), (0, 2)] * 2      # then Cb, Cr: 00 00 each
    bits = "".join(format(c, f"0{n}b") for c, n in tok)
    bits += "1" * (-len(bits) % 8)
    iv, _m = _entropy(f)
    assert iv == [int(bits, 2).to_bytes(len(bits) // 8, "big").replace(b"\xff", b"\xff\x00")]


# ------------------------------------------------------------------------------------------------- jpeg.py
def test_encode_is_the_reference_on_the_golden_clips():
    from hvqm4_amd import jpeg
    assert len({_geometry(nm)[2:] for nm in SIX}) == 3                    # 4:2:0, 4:2:2 and 4:4:4
    assert {_geometry(nm)[:2] for nm in SIX} >= {(24, 40), (296, 160), (8, 8)}
    n = 0
    for name in SIX:
        w, h, hs, vs = _geometry(name)
        for k, pic in enumerate(fd.oracle_pictures(name)):
            for q in QUALITIES:
                got = jpeg.encode(pic, w, h, q, hs, vs)
                assert got == _expected(name, k, q), (name, k, q)
                assert got == jpeg.encode(pic.tobytes(), w, h, q, hs, vs)
                assert len(got) <= jpeg.bound(w, h, hs, vs)
                n += 1
    assert n >= 100
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 256, 2048 * 16 * 3 // 2, dtype=np.uint8)
    assert jpeg.encode(noise, 2048, 16, 100) == jpeg_reference(noise, 2048, 16, 100, 2, 2)
    assert jpeg.encode(jpeg_ref.basis_picture(), 64, 128, 100, 1, 1) == jpeg_reference(jpeg_ref.basis_picture(), 64, 128, 100, 1, 1)
    with pytest.raises(ValueError):
        jpeg.encode(noise[:-1], 2048, 16, 90)
    with pytest.raises(ValueError):
        jpeg.encode(noise, 2048, 16, 0)
    with pytest.raises(ValueError):
        jpeg.encode(noise, 2044, 16, 90)
    with pytest.raises(ValueError):
        jpeg.encode(noise, 2048, 16, 90, 1, 2)


def test_quant_tables_header_bound_segments():
    from hvqm4_amd import jpeg
    for q in (1, 49, 50, 100):
        ql, qc = jpeg.quant_tables(q)
        assert ql.dtype == np.uint8 and ql.shape == (64,) == qc.shape
        assert ql.tolist() == jpeg_ref.quant_table(jpeg_ref.Q_LUMA, q) and qc.tolist() == jpeg_ref.quant_table(jpeg_ref.Q_CHROMA, q)
    assert all((t == 255).all() for t in jpeg.quant_tables(1)) and all((t == 1).all() for t in jpeg.quant_tables(100))
    assert jpeg.quant_tables(50)[0].tolist() == jpeg_ref.Q_LUMA and jpeg.quant_tables(50)[1].tolist() == jpeg_ref.Q_CHROMA
    assert jpeg.quant_tables(49)[0][0] == (16 * 102 + 50) // 100
    for bad in (0, 101, -1, 50.0, True, None):
        with pytest.raises(ValueError):
            jpeg.quant_tables(bad)
    for w, h, hs, vs in [(64, 48, 2, 2), (296, 160, 2, 1), (48, 64, 1, 1), (24, 40, 2, 2), (8, 8, 2, 2)]:
        for q in QUALITIES:
            assert jpeg.header(w, h, q, hs, vs) == jpeg_ref.header(w, h, hs, vs, q)
        mw, mh = jpeg.mcus(w, h, hs, vs)
        blocks = mw * mh * (hs * vs + 2)
        assert jpeg.bound(w, h, hs, vs) <= 629 + 2 + 2 * (mh - 1) + 2 * -(-blocks * 64 * 26 // 8), "the bound the issue asks for, or tighter"
    f = _expected("gop64x48_15", 0, 90)
    assert [s[0] for s in jpeg.segments(f)][:2] == [0xD8, 0xE0] and jpeg.segments(f)[-1] == (0xD9, len(f) - 2, 0)
    for broken in (f[:-1], f[1:], f + b"\x00", f[:700]):
        with pytest.raises(ValueError):
            jpeg.segments(broken)


def test_header_and_bound_of_the_library():
    import ctypes as C
    from hvqm4_amd import jpeg
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_GEOMETRY, lib
    buf = (C.c_uint8 * 700)()
    n = C.c_size_t(0)
    for w, h, hs, vs in [(64, 48, 2, 2), (296, 160, 2, 1), (48, 64, 1, 1), (24, 40, 2, 2), (8, 8, 2, 2), (640, 480, 2, 2), (2048, 16, 2, 2)]:
        for q in (1, 49, 50, 90, 100):
            assert lib().hvq_jpeg_header(w, h, hs, vs, q, buf, 700, C.byref(n)) == 0 and n.value == 629
            assert bytes(buf[:629]) == jpeg.header(w, h, q, hs, vs), (w, h, hs, vs, q)
        assert lib().hvq_jpeg_bound(w, h, hs, vs) == jpeg.bound(w, h, hs, vs)
    assert lib().hvq_jpeg_header(64, 48, 2, 2, 90, buf, 629, None) == 0
    assert lib().hvq_jpeg_header(64, 48, 2, 2, 90, buf, 628, C.byref(n)) == HVQ_E_ARG
    assert lib().hvq_jpeg_header(64, 48, 2, 2, 90, None, 700, C.byref(n)) == HVQ_E_ARG
    for q in (0, 101, -3):
        assert lib().hvq_jpeg_header(64, 48, 2, 2, q, buf, 700, C.byref(n)) == HVQ_E_ARG
    assert lib().hvq_jpeg_header(60, 48, 2, 2, 90, buf, 700, C.byref(n)) == HVQ_E_GEOMETRY
    assert lib().hvq_jpeg_header(64, 48, 1, 2, 90, buf, 700, C.byref(n)) == HVQ_E_GEOMETRY
    assert lib().hvq_jpeg_bound(60, 48, 2, 2) == 0 and lib().hvq_jpeg_bound(64, 48, 3, 1) == 0
    head = open(os.path.join(fd.ROOT, "include", "hvqm4_amd.h")).read()
    assert re.search(r"#define HVQ_JPEG_HEADER\s+629\b", head)
    desc = open(os.path.join(fd.CSRC, "hvq_desc.h")).read()
    assert "sizeof(HvqJpegJob) == 64" in desc


def test_the_library_without_a_device_still_checks_its_arguments():
    """no context can exist here, and the call says so before it looks at anything else"""
    import ctypes as C
    from hvqm4_amd._lib import HVQ_E_ARG, lib
    one = (C.c_int * 1)(0)
    assert lib().hvq_encode_jpeg(None, 1, one, one, None, 90, None, None, None, None) == HVQ_E_ARG
    assert lib().hvq_encode_jpeg(None, 0, None, None, None, 90, None, None, None, None) == HVQ_E_ARG


class _NoDevice:
    """what Context.encode_jpeg looks at before it reaches the library"""
    _geom = {0: (64, 48), 1: (24, 40)}
    _h = None

    @staticmethod
    def pic_bytes(sid):
        return {0: 64 * 48 * 3 // 2, 1: 24 * 40 * 3 // 2}[sid]


def test_arguments_are_checked_before_the_library_is_called():
    import torch
    from hvqm4_amd._lib import HVQ_E_ARG, HvqError
    from hvqm4_amd.batch import Context
    call = lambda *a, **k: Context.encode_jpeg(_NoDevice(), *a, **k)
    with pytest.raises(ValueError, match="ordinals"):
        call([0, 0], [0])
    with pytest.raises(HvqError) as e:
        call([0, 7], [0, 0])
    assert e.value.code == HVQ_E_ARG
    for q in (0, 101, -1, 90.0, True, None):
        with pytest.raises(ValueError, match="quality"):
            call([0], [0], quality=q)
    room = torch.zeros(4096 + 64, dtype=torch.uint8)
    off = (-room.data_ptr()) % 16
    good = room[off:off + 4096]
    with pytest.raises(ValueError, match="list of 1"):
        call([0], [0], out=good)
    with pytest.raises(ValueError, match="list of 1"):
        call([0], [0], out=[])
    with pytest.raises(ValueError, match=r"out\[0\] must be"):
        call([0], [0], out=[good.to(torch.int8)])
    with pytest.raises(ValueError, match=r"out\[0\] must be"):
        call([0], [0], out=[good[:630]])
    with pytest.raises(ValueError, match=r"out\[0\] must be"):
        call([0], [0], out=[good[::2]])
    with pytest.raises(ValueError, match="multiple of 16"):
        call([0], [0], out=[room[off + 8:off + 8 + 4000]])
    with pytest.raises(ValueError, match="not a GPU"):
        call([0], [0], out=[good])
    pic = torch.zeros(64 * 48 * 3 // 2 + 64, dtype=torch.uint8)
    poff = (-pic.data_ptr()) % 16
    with pytest.raises(ValueError, match="ordinal"):
        call([0], [0], src=[pic[poff:poff + 4608]])
    with pytest.raises(ValueError, match="elements"):
        call([1], [-1], src=[pic[poff:poff + 4608]])
    with pytest.raises(ValueError, match="sources for"):
        call([0, 0], [0, 1], src=[None])
    with pytest.raises(ValueError, match="not a GPU"):
        call([0], [-1], src=[pic[poff:poff + 4608]])


# ------------------------------------------------------------------------------------------------- an independent decoder
def _psnr(a, b):
    m = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 99.0 if m == 0 else 10 * math.log10(255 * 255 / m)


def _decode_ycc(Image, data):
    im = Image.open(io.BytesIO(data))
    im.draft("YCbCr", None)
    im.load()
    return im


def test_an_independent_decoder_reads_the_files():
    """Pillow opens every file of the golden clips at the four qualities, sees the stream's size and decodes in YCbCr.  At qualities 50 and
    90, on the clips of 24 x 40 and more, the luma PSNR of the decoded file against the source is no more than 0.5 dB below that of
    Pillow's own encode of the same planes at the same quality and subsampling (8 x 8 pictures are left out of this comparison only: two
    to six blocks make PSNR noise).  Measured with the reference encoder alone on these clips (Pillow 12.2, libjpeg-turbo): the worst gap
    is 0.13 dB (ragged24x40 picture 0 at quality 90); on most pictures the two are within 0.05 dB of each other, either way."""
    Image = pytest.importorskip("PIL.Image")
    worst = (-99.0, None)
    for name in SIX:
        w, h, hs, vs = _geometry(name)
        for k, pic in enumerate(fd.oracle_pictures(name)):
            Y, U, V = jpeg_ref.planes(pic, w, h, hs, vs)
            for q in QUALITIES:
                im = _decode_ycc(Image, _expected(name, k, q))
                assert im.size == (w, h) and im.mode == "YCbCr", (name, k, q, im.size, im.mode)
                if q not in (50, 90) or w * h < 24 * 40:
                    continue
                ours = _psnr(np.asarray(im)[..., 0], Y)
                full = np.stack([Y, np.repeat(np.repeat(U, vs, 0), hs, 1), np.repeat(np.repeat(V, vs, 0), hs, 1)], -1)
                bio = io.BytesIO()
                Image.fromarray(full, "YCbCr").save(bio, "JPEG", quality=q, subsampling={(1, 1): 0, (2, 1): 1, (2, 2): 2}[(hs, vs)])
                theirs = _psnr(np.asarray(_decode_ycc(Image, bio.getvalue()))[..., 0], Y)
                print(f"{name} picture {k} quality {q}: luma PSNR {ours:.2f} dB, Pillow's own {theirs:.2f} dB")
                worst = max(worst, (theirs - ours, (name, k, q)))
                assert ours >= theirs - 0.5, (name, k, q, ours, theirs)
    print("worst gap", worst)


# ------------------------------------------------------------------------------------------------- the runtime on the CPU fake device
@pytest.fixture(scope="module")
def drivers():
    return {kind: fd.build_driver(kind, "jpeg", "fake_jpeg_driver", CXX_SOURCES, __file__) for kind in fd.BUILDS}


def _run(exe, scenario, schedule, tmp_path, extra=()):
    _, lines = fd.run_checked(exe, scenario, schedule, tmp_path, extra)
    K, R, S, G, Q = {}, {}, {}, {}, {}
    for line in lines:
        f = line.split()
        if f[0] == "J":
            label, name, k, form, q, cap, length, hexed, same, tail = f[1], f[2], int(f[3]), f[4], int(f[5]), int(f[6]), int(f[7]), f[8], int(f[9]), int(f[10])
            want = _expected(name, k, q)
            assert length == len(want), f"{label}: picture {k} of {name} at quality {q}: length {length}, the file has {len(want)} bytes"
            if length <= cap:
                got = bytes.fromhex(hexed)
                assert got == want, f"{label}: picture {k} of {name} ({form}) at quality {q}: the first difference is at byte {next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)}"
                assert tail == cap - length
            else:
                assert hexed == "-" and tail == cap
            assert same == tail, f"{label}: picture {k} of {name}: {tail - same} bytes behind the file (or of a file that did not fit) were written"
            K.setdefault(label, []).append((name, k, form, length <= cap))
        elif f[0] == "R":
            R[f[1]] = int(f[2])
        elif f[0] == "S":
            S[f[1]] = (int(f[2]), int(f[3]))
        elif f[0] == "G":
            G[f[1]] = (int(f[2]), int(f[3]))
        elif f[0] == "Q":
            Q[int(f[1]), int(f[2])] = [int(v) for v in f[3:]]
    assert len(G) == 1
    same, total = next(iter(G.values()))
    assert same == total > 0, "a call wrote outside its destination or its lengths"
    return K, R, S, Q, fd.refusal_texts(lines)


def _check_goldens(K, R, S, Q, E):
    n = {nm: fd.n_pics(nm) for nm in SIX}
    assert K["goldens/q90"] == [(nm, k, "pic", True) for nm in SIX for k in range(n[nm])] and len(K["goldens/q90"]) > 20
    assert K["goldens/mixed"] == [(nm, (r * 2 + 1) % n[nm], "pic", True) for r in range(2) for nm in SIX], "files come back in call order"
    two = [(nm, r % n[nm], "pic", True) for r in range(2) for nm in SIX]
    assert K["goldens/q1"] == two and K["goldens/q100"] == two
    assert R == {"goldens/n0": 0}


def _check_memory(K, R, S, Q, E):
    nm, na = "yuv422_64x48", fd.n_pics("yuv422_64x48")
    want = [x for k in range(na) for x in ((nm, (k + 1) % na, "mem", True), (nm, k, "pic", True))]
    want += [("ragged24x40", 1, "mem", True), ("ragged24x40", 2, "pic", True)]
    assert K["memory/q90"] == want and K["memory/q100"] == want and K["memory/nullstream"] == want


def _overflow_lengths():
    return [len(_expected("gop64x48_15", k, 90)) for k in range(4)]


def _check_overflow(K, R, S, Q, E):
    nm = "gop64x48_15"
    assert K["overflow/short"] == [(nm, 0, "pic", True), (nm, 1, "pic", False), (nm, 2, "pic", True), (nm, 3, "pic", True)]
    assert K["overflow/tiny"] == [(nm, k, "pic", False) for k in range(4)] and min(_overflow_lengths()) > 631
    assert K["overflow/again"] == [(nm, k, "pic", True) for k in range(4)]


# what hvq_last_error_string() said after each call of `refused`, recorded from the runtime before the record frame: the
# order of the checks and their words are part of the interface.  A call that succeeds leaves the words of the refusal before it.
REFUSAL_TEXTS = {
    "refused/null_context": "bad arguments",
    "refused/quality_0": "quality 0 outside [1, 100]",
    "refused/quality_101": "quality 101 outside [1, 100]",
    "refused/quality_negative": "quality -5 outside [1, 100]",
    "refused/null_out": "out or cap is NULL",
    "refused/null_cap": "out or cap is NULL",
    "refused/null_lengths": "lengths must be a non-null multiple of 8",
    "refused/misaligned_lengths": "lengths must be a non-null multiple of 8",
    "refused/null_destination": "file 1: the pointer must be a non-null multiple of 16",
    "refused/misaligned_destination": "file 1: the pointer must be a non-null multiple of 16",
    "refused/cap_630": "file 1: 630 bytes hold not even the header and EOI (631)",
    "refused/cap_0": "file 1: 0 bytes hold not even the header and EOI (631)",
    "refused/bad_stream": "bad stream 99",
    "refused/negative_stream": "bad stream -1",
    "refused/bad_ordinal": "stream 0: bad picture ordinal 1000",
    "refused/negative_ordinal": "stream 0: bad picture ordinal -1",
    "refused/src_with_ordinal": "picture 1: a pointer together with ordinal 1 (the caller's memory takes ordinal -1)",
    "refused/src_misaligned": "picture 1: the pointer must be a multiple of 16",
    "refused/src_bad_stream": "bad stream 99",
    "refused/too_many": "65536 pictures: one call takes 65535 at the most (one grid row each)",
    "refused/evicted": "stream 1 picture 0 is no longer resident (slot reused, or the picture was dropped)",
    "refused/queued": "stream 0 picture 7 is queued but not flushed",
    "refused/n0": "stream 0 picture 7 is queued but not flushed",
    "refused/n0_bad_quality": "quality 0 outside [1, 100]",
    "header/ok": "quality 0 outside [1, 100]",
    "header/no_len": "quality 0 outside [1, 100]",
    "header/short": "the header takes 629 bytes",
    "header/null": "the header takes 629 bytes",
    "header/quality": "quality 0 outside [1, 100]",
    "header/geometry": "unsupported geometry 60x48 sampling 2x2",
}


def _check_refused(K, R, S, Q, E):
    for label, text in REFUSAL_TEXTS.items():
        assert E.get(label) == text, (label, E.get(label))
    assert set(E) == set(REFUSAL_TEXTS)
    from hvqm4_amd import jpeg
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_GEOMETRY, HVQ_E_STATE
    arg = ["null_context", "quality_0", "quality_101", "quality_negative", "null_out", "null_cap", "null_lengths", "misaligned_lengths", "null_destination",
           "misaligned_destination", "cap_630", "cap_0", "bad_stream", "negative_stream", "bad_ordinal", "negative_ordinal", "src_with_ordinal",
           "src_misaligned", "src_bad_stream", "too_many", "n0_bad_quality"]
    want = {"refused/" + k: HVQ_E_ARG for k in arg}
    want.update({"refused/evicted": HVQ_E_STATE, "refused/queued": HVQ_E_STATE, "refused/n0": 0})
    want.update({"header/ok": 0, "header/len": 629, "header/no_len": 0, "header/short": HVQ_E_ARG, "header/null": HVQ_E_ARG, "header/quality": HVQ_E_ARG,
                 "header/geometry": HVQ_E_GEOMETRY, "bound/64x48": jpeg.bound(64, 48), "bound/geometry": 0})
    assert R == want
    same, total = S["refused"]
    assert same == total == 2 * (-(-jpeg.bound(64, 48) // 16) * 16) + 32, "a refused call wrote a destination or the lengths"
    last = fd.n_pics("gop64x48_15") - 1
    assert K["refused/then_ok"] == [("gop64x48_15", 1, "pic", True), ("gop64x48_15", last, "pic", True)]


def _check_helpers(K, R, S, Q, E):
    """the division helper against `/` for every numerator up to 1278 (|F| <= 1151 and Q >> 1 <= 127 lie below) and every Q in 1 .. 255"""
    assert R["helpers/div_max"] >= 1151 + 127 and R["helpers/tried"] == 255 * (R["helpers/div_max"] + 1)
    assert R["helpers/div_mismatches"] == 0 and R["helpers/quantise_mismatches"] == 0
    for q in (1, 49, 50, 100):
        assert Q[q, 0] == jpeg_ref.quant_table(jpeg_ref.Q_LUMA, q) and Q[q, 1] == jpeg_ref.quant_table(jpeg_ref.Q_CHROMA, q)


CHECKS = {"goldens": _check_goldens, "memory": _check_memory, "overflow": _check_overflow, "refused": _check_refused}


@pytest.mark.parametrize("schedule", ["eager", "late"])
@pytest.mark.parametrize("build", list(fd.BUILDS))
@pytest.mark.parametrize("scenario", list(CHECKS))
def test_fake_device_scenario(drivers, scenario, build, schedule, tmp_path):
    CHECKS[scenario](*_run(drivers[build], scenario, schedule, tmp_path, _overflow_lengths() if scenario == "overflow" else ()))


@pytest.mark.parametrize("build", list(fd.BUILDS))
def test_division_helper_and_quantisers_of_the_shared_header(drivers, build, tmp_path):
    _check_helpers(*_run(drivers[build], "helpers", "eager", tmp_path))


def test_the_existing_fake_builds_link_without_the_jpeg_body():
    """the source lists of the other drivers have no hvq_launch_jpeg: the runtime's reference to it is weak"""
    assert not any("fake_jpeg" in s for s in fd.CXX_SOURCES)
    text = open(os.path.join(fd.CSRC, "hvq_runtime.cpp")).read()
    decl = [l for l in text.splitlines() if "hvq_launch_jpeg(" in l and l.startswith("extern")]
    assert len(decl) == 1 and "weak" in decl[0]
    import tests.test_motion_cpu as mc
    assert not any("fake_jpeg" in s for s in mc.CXX_SOURCES)
