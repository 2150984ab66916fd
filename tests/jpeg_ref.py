"""The JPEG file of include/hvqm4_amd.h (hvq_encode_jpeg), restated from that text in plain numpy / Python with nothing of the kernels'
shape: full 8 x 8 sums with `//`-free Python integers for the division, no reciprocal, no even/odd halves, no LDS packing -- the bits of a
restart interval are accumulated in ONE Python integer.  The GPU, the fake device and hvqm4_amd.jpeg.encode are compared with it by ==.

It asserts what the text derives: AC sizes stay within 10 and DC difference sizes within 11."""
import math

import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
# ITU-T T.81 Annex K.1 and K.2
Q_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
Q_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
# Annex K.3 - K.6: (codes per length 1..16, symbols in code order)
_AC_TAIL = [r << 4 | s for r in range(16) for s in range(1, 11)]
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
            0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
            0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
            0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
            0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
            0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
            0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
              0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
              0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
              0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
              0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
              0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
              0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
assert sum(AC_LUMA[0]) == len(AC_LUMA[1]) == 162 == sum(AC_CHROMA[0]) == len(AC_CHROMA[1]) and sorted(AC_LUMA[1]) == sorted(AC_CHROMA[1]) == sorted(_AC_TAIL + [0, 0xf0])

# the table of the text, from its formula, against its printed rows
C = [[0] * 8 for _ in range(8)]
for _k in range(8):
    for _n in range(4):
        C[_k][_n] = math.floor((math.sqrt(1 / 8) if _k == 0 else 0.5) * math.cos((2 * _n + 1) * _k * math.pi / 16) * 8192 + 0.5)
        C[_k][7 - _n] = C[_k][_n] if _k % 2 == 0 else -C[_k][_n]
assert [r[:4] for r in C] == [[2896, 2896, 2896, 2896], [4017, 3406, 2276, 799], [3784, 1567, -1567, -3784], [3406, -799, -4017, -2276],
                              [2896, -2896, -2896, 2896], [2276, -4017, 799, 3406], [1567, -3784, 3784, -1567], [799, -2276, 3406, -4017]]
_CM = np.array(C, dtype=np.int64)

HEADER_BYTES = 629


def huffman_codes(table):
    """symbol -> (code, length), Annex C"""
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def quant_table(base, quality):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [min(255, max(1, (b * s + 50) // 100)) for b in base]


def fdct(x):
    """x: int64 [8, 8], level-shifted samples -> F[k][l], k the vertical frequency"""
    r = (x @ _CM.T + 1024) >> 11                    # r[y][k] = sum_n C[k][n] x[y][n]
    return (_CM @ r + 16384) >> 15                  # F[k][l] = sum_y C[k][y] r[y][l]


def mcus(width, height, h_samp, v_samp):
    return -(-width // (8 * h_samp)), -(-height // (8 * v_samp))


def header(width, height, h_samp, v_samp, quality):
    b = bytearray(b"\xff\xd8" + b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, base in enumerate((Q_LUMA, Q_CHROMA)):
        t = quant_table(base, quality)
        b += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(t[z] for z in ZIGZAG)
    b += b"\xff\xc0\x00\x11\x08" + height.to_bytes(2, "big") + width.to_bytes(2, "big") + b"\x03" + bytes([1, h_samp << 4 | v_samp, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        b += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([tc]) + bytes(bits) + bytes(vals)
    b += b"\xff\xdd\x00\x04" + mcus(width, height, h_samp, v_samp)[0].to_bytes(2, "big")
    b += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert len(b) == HEADER_BYTES
    return bytes(b)


def planes(picture, width, height, h_samp, v_samp):
    pic = np.frombuffer(bytes(picture), dtype=np.uint8) if not isinstance(picture, np.ndarray) else picture.reshape(-1)
    cw, ch = width // h_samp, height // v_samp
    assert pic.size == width * height + 2 * cw * ch, (pic.size, width, height, h_samp, v_samp)
    return (pic[:width * height].reshape(height, width), pic[width * height:width * height + cw * ch].reshape(ch, cw),
            pic[width * height + cw * ch:].reshape(ch, cw))


def jpeg_reference(picture, width, height, quality, h_samp=2, v_samp=2, stats=None):
    """the file, as bytes.  stats (a dict), if given, collects max |AC|, the DC range, the largest sizes and the ZRL count"""
    Y, U, V = planes(picture, width, height, h_samp, v_samp)
    mw, mh = mcus(width, height, h_samp, v_samp)
    pad = lambda p, h, w: np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge").astype(np.int64) - 128
    Y, U, V = pad(Y, mh * 8 * v_samp, mw * 8 * h_samp), pad(U, mh * 8, mw * 8), pad(V, mh * 8, mw * 8)
    q = (quant_table(Q_LUMA, quality), quant_table(Q_CHROMA, quality))
    hd, ha = (huffman_codes(DC_LUMA), huffman_codes(DC_CHROMA)), (huffman_codes(AC_LUMA), huffman_codes(AC_CHROMA))
    st = stats if stats is not None else {}
    for k in ("max_ac", "max_dc", "max_ac_size", "max_dc_size", "zrl"):
        st.setdefault(k, 0)
    st.setdefault("min_dc", 0)
    out = bytearray(header(width, height, h_samp, v_samp, quality))
    for my in range(mh):
        acc, nbits, pred = 0, 0, [0, 0, 0]
        for mx in range(mw):
            blocks = [(0, Y[(my * v_samp + j) * 8:(my * v_samp + j) * 8 + 8, (mx * h_samp + i) * 8:(mx * h_samp + i) * 8 + 8])
                      for j in range(v_samp) for i in range(h_samp)]
            blocks += [(1, U[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8]), (2, V[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8])]
            for comp, x in blocks:
                F = [int(v) for v in fdct(x).reshape(64)]
                st["max_ac"] = max(st["max_ac"], max(abs(v) for v in F[1:]))
                st["max_dc"], st["min_dc"] = max(st["max_dc"], F[0]), min(st["min_dc"], F[0])
                t = 0 if comp == 0 else 1
                co = [(1 if f > 0 else -1) * ((abs(f) + (q[t][i] >> 1)) // q[t][i]) for i, f in enumerate(F)]
                z = [co[i] for i in ZIGZAG]
                d = z[0] - pred[comp]
                pred[comp] = z[0]
                s = abs(d).bit_length()
                assert s <= 11, ("DC difference size", s)
                st["max_dc_size"] = max(st["max_dc_size"], s)
                code, length = hd[t][s]
                acc, nbits = acc << length | code, nbits + length
                if s:
                    acc, nbits = acc << s | (d if d > 0 else d + (1 << s) - 1), nbits + s
                run = 0
                for i in range(1, 64):
                    if z[i] == 0:
                        run += 1
                        continue
                    while run > 15:
                        code, length = ha[t][0xF0]
                        acc, nbits = acc << length | code, nbits + length
                        run -= 16
                        st["zrl"] += 1
                    s = abs(z[i]).bit_length()
                    assert s <= 10, ("AC size", s)
                    st["max_ac_size"] = max(st["max_ac_size"], s)
                    code, length = ha[t][run << 4 | s]
                    acc, nbits = acc << length | code, nbits + length
                    acc, nbits = acc << s | (z[i] if z[i] > 0 else z[i] + (1 << s) - 1), nbits + s
                    run = 0
                if run:                              # coefficient 63 is zero
                    code, length = ha[t][0x00]
                    acc, nbits = acc << length | code, nbits + length
        fill = -nbits % 8
        acc, nbits = acc << fill | ((1 << fill) - 1), nbits + fill
        out += acc.to_bytes(nbits // 8, "big").replace(b"\xff", b"\xff\x00")
        if my < mh - 1:
            out += bytes([0xFF, 0xD0 + (my & 7)])
    out += b"\xff\xd9"
    return bytes(out)


_cache = {}


def cached(key, picture, width, height, quality, h_samp, v_samp):
    """jpeg_reference, computed once per (key, quality): the tests share the expected files"""
    k = (key, width, height, quality, h_samp, v_samp)
    if k not in _cache:
        _cache[k] = jpeg_reference(picture, width, height, quality, h_samp, v_samp)
    return _cache[k]


def basis_sign_patterns():
    """the 128 blocks of the text's range argument: per basis function (k, l) samples 255 where the basis is positive and 0 elsewhere, and
    the inverse -> uint8 [128, 8, 8], the pattern of (k, l) at index 2 (8 k + l), its inverse behind it"""
    out = np.zeros((128, 8, 8), dtype=np.uint8)
    for k in range(8):
        for l in range(8):
            pos = np.outer(_CM[k], _CM[l]) > 0
            out[2 * (8 * k + l)] = np.where(pos, 255, 0)
            out[2 * (8 * k + l) + 1] = np.where(pos, 0, 255)
    return out


def basis_picture():
    """the 128 patterns as one 64 x 128 (W x H) 4:4:4 picture: Y holds them 8 a row, U the same shifted by one pattern, V by two"""
    p = basis_sign_patterns()
    plane = lambda sh: np.roll(p, sh, axis=0).reshape(16, 8, 8, 8).transpose(0, 2, 1, 3).reshape(128, 64)
    return np.concatenate([plane(0).reshape(-1), plane(1).reshape(-1), plane(2).reshape(-1)]).astype(np.uint8)
