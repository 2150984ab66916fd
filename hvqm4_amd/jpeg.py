"""Baseline JPEG files of pictures on the host (numpy only): what hvq_encode_jpeg / Context.encode_jpeg write on the GPU, byte for byte
(include/hvqm4_amd.h: the specification), and what a caller needs around that call.

    header(width, height, quality, h_samp, v_samp)   the 629 bytes in front of the entropy data
    bound(width, height, h_samp, v_samp)             a length no file of this geometry exceeds
    quant_tables(quality)                            (luminance, chrominance), natural order, uint8 [64] each
    encode(picture, width, height, quality, ...)     the expected file of a picture in slot layout (Y | U | V)
    files(buffers, lengths)                          the files of a Context.encode_jpeg call as bytes (synchronises)
    segments(file)                                   the marker walk of a file: [(marker, offset, payload length)]
"""
import numpy as np

HEADER_BYTES = 629
CODE_BITS = 26                      # the longest code with its value bits

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
# ITU-T T.81 Annex K.1, K.2 (natural order)
_QBASE = (np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]),
          np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32))
# Annex K.3 - K.6: codes per length 1..16 and the symbols in code order
_DC = ((bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), bytes(range(12))), (bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]), bytes(range(12))))
_AC = ((bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]), bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")),
       (bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]), bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a43444546474849"
    "4a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5"
    "c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))
_C = np.array([[2896, 2896, 2896, 2896], [4017, 3406, 2276, 799], [3784, 1567, -1567, -3784], [3406, -799, -4017, -2276],
               [2896, -2896, -2896, 2896], [2276, -4017, 799, 3406], [1567, -3784, 3784, -1567], [799, -2276, 3406, -4017]], dtype=np.int64)
_CM = np.concatenate([_C, _C[:, ::-1] * np.array([1, -1] * 4)[:, None]], axis=1)
_SIZE = np.array([int(v).bit_length() for v in range(4096)])


def _code_arrays(table):
    bits, vals = table
    code_of, len_of = np.zeros(256, dtype=np.int64), np.zeros(256, dtype=np.int64)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            code_of[vals[k]], len_of[vals[k]] = code, length
            code += 1
            k += 1
        code <<= 1
    return code_of, len_of


_DC_CODES = [_code_arrays(t) for t in _DC]
_AC_CODES = [_code_arrays(t) for t in _AC]


def _check_geometry(width, height, h_samp, v_samp):
    if (h_samp, v_samp) not in ((2, 2), (2, 1), (1, 1)):
        raise ValueError(f"sampling {h_samp} x {v_samp}: 2 x 2, 2 x 1 or 1 x 1")
    if width < 8 or height < 8 or width % 8 or height % 8 or width > 8192 or height > 8192:
        raise ValueError(f"{width} x {height}: multiples of 8 in [8, 8192]")


def _check_quality(quality):
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise ValueError(f"quality {quality!r}: an integer in [1, 100]")


def mcus(width, height, h_samp=2, v_samp=2):
    """(MCUs of a row, MCU rows = restart intervals)"""
    return -(-width // (8 * h_samp)), -(-height // (8 * v_samp))


def quant_tables(quality):
    _check_quality(quality)
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((b * s + 50) // 100, 1, 255).astype(np.uint8) for b in _QBASE)


def header(width, height, quality, h_samp=2, v_samp=2):
    _check_geometry(width, height, h_samp, v_samp)
    b = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, q in enumerate(quant_tables(quality)):
        b += b"\xff\xdb\x00\x43" + bytes([i]) + q[ZIGZAG].tobytes()
    b += b"\xff\xc0\x00\x11\x08" + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([3, 1, h_samp << 4 | v_samp, 0, 2, 0x11, 1, 3, 0x11, 1])
    for t in (0, 1):
        for cls, (bits, vals) in ((0x00, _DC[t]), (0x10, _AC[t])):
            b += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([cls | t]) + bits + vals
    b += b"\xff\xdd\x00\x04" + mcus(width, height, h_samp, v_samp)[0].to_bytes(2, "big")
    b += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert len(b) == HEADER_BYTES
    return bytes(b)


def bound(width, height, h_samp=2, v_samp=2):
    """hvq_jpeg_bound: header, EOI, RST markers, and per interval its blocks at CODE_BITS bits a coefficient, every byte stuffed"""
    _check_geometry(width, height, h_samp, v_samp)
    mw, mh = mcus(width, height, h_samp, v_samp)
    return HEADER_BYTES + 2 + 2 * (mh - 1) + 2 * mh * ((mw * (h_samp * v_samp + 2) * 64 * CODE_BITS + 7) // 8)


def _coefficients(plane, bw, bh, q):
    """a plane -> quantised coefficients int64 [bh, bw, 64] in zigzag order, the plane extended to bw x bh blocks by its last column and row"""
    p = np.pad(plane, ((0, bh * 8 - plane.shape[0]), (0, bw * 8 - plane.shape[1])), mode="edge").astype(np.int64) - 128
    x = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)                       # [bh, bw, y, n]
    r = (x @ _CM.T + 1024) >> 11                                            # [.., y, k]
    f = ((_CM @ r + 16384) >> 15).reshape(bh, bw, 64)
    qq = q.astype(np.int64)
    return (np.sign(f) * ((np.abs(f) + (qq >> 1)) // qq))[..., ZIGZAG]


def encode(picture, width, height, quality, h_samp=2, v_samp=2):
    """the file hvq_encode_jpeg writes for a picture in slot layout (bytes or a uint8 array of width * height + 2 chroma planes elements)"""
    _check_geometry(width, height, h_samp, v_samp)
    ql, qc = quant_tables(quality)
    pic = np.frombuffer(bytes(picture), dtype=np.uint8) if not isinstance(picture, np.ndarray) else np.ascontiguousarray(picture).reshape(-1)
    cw, ch = width // h_samp, height // v_samp
    if pic.dtype != np.uint8 or pic.size != width * height + 2 * cw * ch:
        raise ValueError(f"a {width} x {height} picture sampled {h_samp} x {v_samp} has {width * height + 2 * cw * ch} bytes, not {pic.size}")
    mw, mh = mcus(width, height, h_samp, v_samp)
    hv, bpm = h_samp * v_samp, h_samp * v_samp + 2
    zy = _coefficients(pic[:width * height].reshape(height, width), mw * h_samp, mh * v_samp, ql)
    zu = _coefficients(pic[width * height:width * height + cw * ch].reshape(ch, cw), mw, mh, qc)
    zv = _coefficients(pic[width * height + cw * ch:].reshape(ch, cw), mw, mh, qc)
    # coding order: [mh, mw, block of the MCU, 64]
    z = np.empty((mh, mw, bpm, 64), dtype=np.int64)
    z[:, :, :hv] = zy.reshape(mh, v_samp, mw, h_samp, 64).transpose(0, 2, 1, 3, 4).reshape(mh, mw, hv, 64)
    z[:, :, hv], z[:, :, hv + 1] = zu, zv
    # DC differences per component inside an interval
    dc = z[..., 0].copy()
    yd = dc[:, :, :hv].reshape(mh, mw * hv)
    yd[:, 1:] -= yd[:, :-1].copy()
    diff = np.empty_like(dc)
    diff[:, :, :hv] = yd.reshape(mh, mw, hv)
    for k in (hv, hv + 1):
        d = dc[:, :, k].copy()
        d[:, 1:] -= dc[:, :-1, k]
        diff[:, :, k] = d
    nblk = mw * bpm
    z = z.reshape(mh, nblk, 64)
    diff = diff.reshape(mh, nblk)
    tab = np.tile(np.array([0] * hv + [1, 1]), mw)
    out = bytearray(header(width, height, quality, h_samp, v_samp))
    pos = np.arange(CODE_BITS)
    for j in range(mh):
        zj, dj = z[j], diff[j]
        vals, lens, keys = [], [], []
        # DC tokens: key (block, 0, 0) and (block, 0, 1)
        ds = _SIZE[np.abs(dj)]
        for t in (0, 1):
            m = tab == t
            b = np.nonzero(m)[0]
            code, ln = _DC_CODES[t]
            vals += [code[ds[b]], np.where(dj[b] < 0, dj[b] + (1 << ds[b]) - 1, dj[b])]
            lens += [ln[ds[b]], ds[b]]
            keys += [b * 512, b * 512 + 1]
        # AC tokens
        b, k = np.nonzero(zj[:, 1:])
        k = k + 1
        v = zj[b, k]
        first = np.ones(b.size, dtype=bool)
        first[1:] = b[1:] != b[:-1]
        prev = np.zeros(b.size, dtype=np.int64)
        prev[1:] = k[:-1]
        prev[first] = 0
        run = k - prev - 1
        sz = _SIZE[np.abs(v)]
        if sz.size and sz.max() > 10:
            raise AssertionError("an AC coefficient beyond size 10")
        tb = tab[b]
        for t in (0, 1):
            code, ln = _AC_CODES[t]
            m = tb == t
            bm, km, rm, sm, vm = b[m], k[m], run[m], sz[m], v[m]
            for i in range(3):                                               # up to three ZRLs in front of a coefficient
                zr = rm >= 16 * (i + 1)
                vals.append(np.full(int(zr.sum()), code[0xF0])); lens.append(np.full(int(zr.sum()), ln[0xF0])); keys.append(bm[zr] * 512 + km[zr] * 8 + i)
            sym = (rm & 15) << 4 | sm
            vals += [code[sym], np.where(vm < 0, vm + (1 << sm) - 1, vm)]
            lens += [ln[sym], sm]
            keys += [bm * 512 + km * 8 + 3, bm * 512 + km * 8 + 4]
            # EOB behind the last coefficient of a block, unless coefficient 63 is non-zero
            eb = np.nonzero((zj[:, 63] == 0) & (tab == t))[0]
            vals.append(np.full(eb.size, code[0])); lens.append(np.full(eb.size, ln[0])); keys.append(eb * 512 + 511)
        vals, lens, keys = np.concatenate(vals), np.concatenate(lens), np.concatenate(keys)
        order = np.argsort(keys, kind="stable")
        vals, lens = vals[order], lens[order]
        bits = ((vals[:, None] >> np.maximum(lens[:, None] - 1 - pos, 0)) & 1).astype(np.uint8)[pos < lens[:, None]]
        bits = np.concatenate([bits, np.ones(-bits.size % 8, dtype=np.uint8)])
        out += np.packbits(bits).tobytes().replace(b"\xff", b"\xff\x00")
        if j < mh - 1:
            out += bytes([0xFF, 0xD0 + (j & 7)])
    out += b"\xff\xd9"
    return bytes(out)


def files(buffers, lengths):
    """the files of Context.encode_jpeg(...) -> (buffers, lengths) as a list of bytes.  Synchronises (reads the lengths back); raises
    ValueError with the needed length when a file did not fit its buffer: call encode_jpeg again with more room"""
    need = [int(v) for v in lengths.cpu().tolist()]
    if len(need) != len(buffers):
        raise ValueError(f"{len(buffers)} buffers but {len(need)} lengths")
    for i, (b, n) in enumerate(zip(buffers, need)):
        if n > b.numel():
            raise ValueError(f"file {i} needs {n} bytes, its buffer has {b.numel()}")
    return [b[:n].cpu().numpy().tobytes() for b, n in zip(buffers, need)]


def segments(data):
    """the marker walk of a file: [(marker byte, offset of the FF, payload length)], entropy data skipped (stuffed FF 00 is data, RSTn and
    EOI are markers); raises ValueError on anything that is not a well-formed sequence of segments from SOI to EOI at the last byte"""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    out, i = [(0xD8, 0, 0)], 2
    while True:
        if i + 2 > len(data) or data[i] != 0xFF:
            raise ValueError(f"no marker at {i}")
        m = data[i + 1]
        if m == 0xD9:
            out.append((m, i, 0))
            if i + 2 != len(data):
                raise ValueError(f"{len(data) - i - 2} bytes behind EOI")
            return out
        if 0xD0 <= m <= 0xD7:
            out.append((m, i, 0))
            i += 2
        else:
            if i + 4 > len(data):
                raise ValueError(f"a truncated segment at {i}")
            n = int.from_bytes(data[i + 2:i + 4], "big")
            out.append((m, i, n - 2))
            i += 2 + n
            if m != 0xDA:
                continue
        while True:                                                          # entropy data up to the next marker
            j = data.find(b"\xff", i)
            if j < 0 or j + 1 >= len(data):
                raise ValueError("entropy data runs to the end of the file")
            if data[j + 1] == 0:
                i = j + 2
                continue
            i = j
            break
