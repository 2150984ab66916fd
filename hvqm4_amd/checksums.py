"""Picture checksums (hvq_picture_checksums, Context.picture_checksums): what the records mean, and the values to expect.

A record is int64 [8] = (crc32 of Y, U, V and of the picture, adler32 of Y, U, V and of the picture): zlib's crc32 and adler32 of the
plane's bytes as they lie in the slot, and of the bytes Y | U | V that read_picture returns.  of_bytes gives the same eight values of a
picture the caller has on the host; the combine helpers give the checksum of A | B from those of A and B (a clip's running checksum
from its pictures', a picture's from its planes').
"""
from __future__ import annotations

import zlib
from typing import Callable, List, Optional, Sequence, Tuple

CRC32_Y, CRC32_U, CRC32_V, CRC32_PICTURE, ADLER32_Y, ADLER32_U, ADLER32_V, ADLER32_PICTURE = range(8)
NAMES = ("crc32_y", "crc32_u", "crc32_v", "crc32_picture", "adler32_y", "adler32_u", "adler32_v", "adler32_picture")


def crc32_combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """zlib's crc32_combine through hvq_crc32_combine: crc32(A | B) from crc32(A), crc32(B) and len(B)"""
    from ._lib import lib
    if len_b < 0:
        raise ValueError("len_b is negative")
    return int(lib().hvq_crc32_combine(crc_a & 0xFFFFFFFF, crc_b & 0xFFFFFFFF, len_b))


def adler32_combine(a: int, b: int, len_b: int) -> int:
    """zlib's adler32_combine through hvq_adler32_combine: adler32(A | B) from adler32(A), adler32(B) and len(B)"""
    from ._lib import lib
    if len_b < 0:
        raise ValueError("len_b is negative")
    return int(lib().hvq_adler32_combine(a & 0xFFFFFFFF, b & 0xFFFFFFFF, len_b))


def plane_bytes(width: int, height: int, h_samp: int = 2, v_samp: int = 2) -> Tuple[int, int, int]:
    """bytes of the planes Y, U, V of a width x height picture with chroma sampling (h_samp, v_samp), each 1 or 2"""
    if h_samp not in (1, 2) or v_samp not in (1, 2):
        raise ValueError(f"sampling ({h_samp}, {v_samp}): each is 1 or 2")
    if width < 1 or height < 1:
        raise ValueError(f"{width}x{height} is not a picture size")
    c = (width >> (h_samp == 2)) * (height >> (v_samp == 2))
    return width * height, c, c


def of_bytes(buf, width: int, height: int, h_samp: int = 2, v_samp: int = 2) -> List[int]:
    """the eight values of a picture on the host, with zlib: `buf` is its bytes Y | U | V (bytes, bytearray, memoryview or a uint8
    numpy array)"""
    data = bytes(memoryview(buf).cast("B")) if not isinstance(buf, (bytes, bytearray)) else bytes(buf)
    sizes = plane_bytes(width, height, h_samp, v_samp)
    if len(data) != sum(sizes):
        raise ValueError(f"{len(data)} bytes, a {width}x{height} picture of sampling ({h_samp}, {v_samp}) has {sum(sizes)}")
    at, planes = 0, []
    for n in sizes:
        planes.append(data[at:at + n])
        at += n
    return [zlib.crc32(p) for p in planes] + [zlib.crc32(data)] + [zlib.adler32(p) for p in planes] + [zlib.adler32(data)]


def sources(src, ordinals: Sequence[int], pic_bytes: Callable[[int], int]) -> Optional[List[Optional[int]]]:
    """the device pointers of hvq_picture_checksums' `src` for the pictures of a call, or None when `src` is None.  An entry of `src`
    is None (the resident picture) or a contiguous uint8 tensor of pic_bytes(i) elements whose address is a multiple of 16, with
    ordinal -1.  Raises TypeError / ValueError; the device of a tensor is checked last, so the layout checks run on CPU tensors too."""
    import torch
    n = len(ordinals)
    if src is None:
        return None
    if not isinstance(src, (list, tuple)):
        raise TypeError("src must be None or a list with one entry per picture")
    if len(src) != n:
        raise ValueError(f"{len(src)} sources for {n} pictures")
    out: List[Optional[int]] = []
    for i, t in enumerate(src):
        if t is None:
            out.append(None)
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"source {i} must be None or a uint8 tensor, not {type(t).__name__}")
        if t.dtype != torch.uint8:
            raise TypeError(f"source {i} has dtype {t.dtype}, not torch.uint8")
        if not t.is_contiguous():
            raise ValueError(f"source {i} is not contiguous")
        want = int(pic_bytes(i))
        if t.numel() != want:
            raise ValueError(f"source {i} has {t.numel()} elements, the picture has {want} bytes")
        if ordinals[i] != -1:
            raise ValueError(f"source {i} comes with ordinal {ordinals[i]}: a picture in the caller's memory takes ordinal -1")
        if t.data_ptr() & 15:
            raise ValueError(f"source {i}: pointer {t.data_ptr():#x} must be a multiple of 16")
        if t.device.type != "cuda":
            raise ValueError(f"source {i} is on {t.device}, not a GPU")
        out.append(t.data_ptr())
    return out


def framecrc_lines(ordinals: Sequence[int], frame_types: Sequence, records) -> List[str]:
    """one line per picture: ordinal, frame type, the eight values in hex (tools/framecrc.py).  `records`: [n][8] integers."""
    lines = []
    for k, t, rec in zip(ordinals, frame_types, records):
        v = [int(x) for x in rec]
        if len(v) != 8 or any(x < 0 or x >> 32 for x in v):
            raise ValueError(f"picture {k}: a record is eight values in [0, 2^32)")
        lines.append(f"{k:6d} {t} " + " ".join(f"{x:08x}" for x in v))
    return lines


FRAMECRC_HEADER = "# ordinal type " + " ".join(NAMES)
