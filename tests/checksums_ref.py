"""Host restatement of hvq_picture_checksums (include/hvqm4_amd.h): from a picture's bytes (Y | U | V tightly packed) and geometry to the
record int64 [8] = (crc32 Y, U, V, picture, adler32 Y, U, V, picture), with zlib per plane and per picture; and zlib's two combine
functions in pure Python.  Shared by the CPU and GPU tests; it does not call the library."""
import zlib

import numpy as np

CRC_POLY = 0xEDB88320
ADLER_BASE = 65521


def plane_sizes(w, h, hs, vs):
    """bytes of the planes Y, U, V for chroma sampling (h_samp, v_samp) = (hs, vs)"""
    c = (w >> int(hs == 2)) * (h >> int(vs == 2))
    return w * h, c, c


def checksums_reference(a, w, h, hs, vs):
    """a: uint8 [pic_bytes] -> int64 [8]"""
    sizes = plane_sizes(w, h, hs, vs)
    data = np.ascontiguousarray(np.asarray(a, dtype=np.uint8).reshape(-1)).tobytes()
    assert len(data) == sum(sizes), (len(data), sizes)
    at, planes = 0, []
    for n in sizes:
        planes.append(data[at:at + n])
        at += n
    return np.array([zlib.crc32(p) for p in planes] + [zlib.crc32(data)] + [zlib.adler32(p) for p in planes] + [zlib.adler32(data)],
                    dtype=np.int64)


def _gf_mul(a, b):
    """a * b mod P, reflected: bit 31 is x^0"""
    p = 0
    for i in range(31, -1, -1):
        if (a >> i) & 1:
            p ^= b
        b = (b >> 1) ^ (CRC_POLY if b & 1 else 0)
    return p


def crc32_combine(crc_a, crc_b, len_b):
    """crc32(A | B) = crc32(A) * x^(8 len_b) ^ crc32(B)"""
    x, sq, n = 0x80000000, 0x00800000, len_b
    while n:
        if n & 1:
            x = _gf_mul(x, sq)
        sq = _gf_mul(sq, sq)
        n >>= 1
    return _gf_mul(crc_a, x) ^ crc_b


def adler32_combine(a, b, len_b):
    """every one of B's len_b running sums starts from A's low half instead of the seed 1"""
    a_lo, a_hi, b_lo, b_hi = a & 0xFFFF, a >> 16, b & 0xFFFF, b >> 16
    lo = (a_lo + b_lo - 1) % ADLER_BASE
    hi = (a_hi + b_hi + len_b * (a_lo - 1)) % ADLER_BASE
    return lo | (hi << 16)
