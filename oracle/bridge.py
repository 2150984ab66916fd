"""ctypes loaders for the two CPU checkers (test infrastructure only)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import List, Optional, Tuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SO = os.path.join(HERE, "_ref", "libh4mref.so")
ORACLE_SO = os.path.join(HERE, "libhvqoracle.so")

# probe column order of ref_decode_clip (matches hvqm4_amd.synth stream indices)
PROBE_STREAMS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19]


def build(target: str = "all") -> None:
    subprocess.check_call(["make", "-C", HERE, target], stdout=subprocess.DEVNULL)


def have_ref() -> bool:
    return os.path.exists(REF_SO)


_ref = None


def ref():
    global _ref
    if _ref is None:
        lib = C.CDLL(REF_SO)
        lib.ref_decode_clip.restype = C.c_int
        lib.ref_decode_clip.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
        lib.ref_picsize.restype = C.c_uint32
        lib.ref_picsize.argtypes = [C.c_char_p, C.c_size_t]
        lib.ref_time_clip.restype = C.c_double
        lib.ref_time_clip.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_uint64)]
        lib.ref_buffsize.restype = C.c_uint32
        lib.ref_buffsize.argtypes = [C.c_uint16, C.c_uint16, C.c_uint8, C.c_uint8]
        lib.ref_rgb.restype = C.c_int
        lib.ref_rgb.argtypes = [C.c_void_p, C.c_uint16, C.c_uint16, C.c_void_p, C.c_char_p]
        _ref = lib
    return _ref


def ref_decode(data: bytes, n_pictures: int, probe: bool = False):
    """-> (pictures uint8[n, picsize], probe int32[n, 20] | None) from the compiled reference"""
    lib = ref()
    ps = lib.ref_picsize(data, len(data))
    out = np.zeros((n_pictures, ps), dtype=np.uint8)
    pr = np.full((n_pictures, 20), -2, dtype=np.int32) if probe else None
    n = lib.ref_decode_clip(data, len(data), out.ctypes.data, out.nbytes,
                            pr.ctypes.data if probe else None, n_pictures)
    if n != n_pictures:
        raise RuntimeError(f"reference decoded {n} pictures, expected {n_pictures}")
    return out, pr


REF_V3_SO = os.path.join(HERE, "_ref", "libh4mref_v3.so")
_ref_fast = None


def ref_fast_flags() -> Optional[str]:
    """-march flag of the build ref_time uses on this host (None: the portable build)"""
    try:
        flags = open("/proc/cpuinfo").read()
    except OSError:
        return None
    ok = all(f" {k}" in flags for k in ("avx2", "bmi2", "fma"))
    return "-march=x86-64-v3" if ok and os.path.exists(REF_V3_SO) else None


def ref_time(data: bytes, reps: int) -> Tuple[float, int]:
    """decode-call time of the reference over `reps` passes (the -march=x86-64-v3 build where the CPU allows it)"""
    global _ref_fast
    lib = ref()
    if ref_fast_flags():
        if _ref_fast is None:
            _ref_fast = C.CDLL(REF_V3_SO)
            _ref_fast.ref_time_clip.restype = C.c_double
            _ref_fast.ref_time_clip.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_uint64)]
        lib = _ref_fast
    px = C.c_uint64(0)
    t = lib.ref_time_clip(data, len(data), reps, C.byref(px))
    return t, px.value


_orc = None


def oracle():
    global _orc
    if _orc is None:
        if not os.path.exists(ORACLE_SO):
            build("oracle")
        lib = C.CDLL(ORACLE_SO)
        lib.hvqo_create.restype = C.c_void_p
        lib.hvqo_create.argtypes = [C.c_int] * 5
        lib.hvqo_destroy.argtypes = [C.c_void_p]
        lib.hvqo_picsize.restype = C.c_uint32
        lib.hvqo_picsize.argtypes = [C.c_void_p]
        lib.hvqo_decode_ipic.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
        lib.hvqo_decode_ppic.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p]
        lib.hvqo_decode_bpic.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hvqo_decode_clip.restype = C.c_int
        lib.hvqo_decode_clip.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
        lib.hvqo_time_clip.restype = C.c_double
        lib.hvqo_time_clip.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_uint64)]
        lib.hvqo_weight_block.argtypes = [C.c_void_p] + [C.c_uint8] * 5
        lib.hvqo_motion_comp.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int]
        lib.hvqo_tables.argtypes = [C.c_void_p, C.c_void_p]
        lib.hvqo_yuv420_to_rgb.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        lib.hvqo_nest.restype = C.c_void_p
        lib.hvqo_nest.argtypes = [C.c_void_p]
        lib.hvqc_create.restype = C.c_void_p
        lib.hvqc_create.argtypes = [C.c_int] * 5
        lib.hvqc_destroy.argtypes = [C.c_void_p]
        lib.hvqc_picsize.restype = C.c_uint32
        lib.hvqc_picsize.argtypes = [C.c_void_p]
        lib.hvqo_check_picture.restype = C.c_uint32
        lib.hvqo_check_picture.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _orc = lib
    return _orc


# ---- the checked oracle (hvq_oracle_chk.c): one guarded decode per picture, a class instead of a wild read
C_MEM, C_MAP, C_EMPTY, C_TREE, C_HANG, C_RULES = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
CLASS_NAMES = ((C_TREE, "tree"), (C_RULES, "rules"), (C_HANG, "hang"), (C_MEM, "mem"), (C_MAP, "map"), (C_EMPTY, "empty"))


def class_name(cls: int) -> str:
    """the class a refusal reports for the mask `cls`, in the order the product reports its flags (malformed, capped, clamped)"""
    for bit, name in CLASS_NAMES:
        if cls & bit:
            return name
    return "defined"


class Report(C.Structure):
    _fields_ = [("cls", C.c_uint32), ("past_bits", C.c_uint32), ("cross", C.c_uint32)]


class CheckedPlayer:
    """The checked oracle with the player's picture rotation (h4m:2087-2137).  `check` decodes a picture against the current
    references WITHOUT moving the rotation (into a private copy of the picture being written) and returns (class mask, report,
    picture or None); `advance` decodes the stream's own picture and rotates."""

    def __init__(self, width: int, height: int, samp_h: int, samp_v: int, is15: bool):
        self.lib = oracle()
        self.o = self.lib.hvqc_create(width, height, samp_h, samp_v, 1 if is15 else 0)
        self.ps = self.lib.hvqc_picsize(self.o)
        self.buf = [np.zeros(self.ps, dtype=np.uint8) for _ in range(3)]     # past, present, future

    def close(self) -> None:
        if self.o:
            self.lib.hvqc_destroy(self.o)
            self.o = None

    def refs(self, ft: int):
        """(past, present, future) as the decode of a picture of type `ft` sees them"""
        b = self.buf
        return (b[0], b[1], b[2]) if ft == 0x30 else (b[2], b[1], b[0])

    def check(self, ft: int, pic: bytes):
        past, present, future = self.refs(ft)
        out = present.copy()
        rep = Report()
        cls = self.lib.hvqo_check_picture(self.o, ft, pic, len(pic), out.ctypes.data, past.ctypes.data, future.ctypes.data, C.byref(rep))
        return cls, rep, (out if cls == 0 else None)

    def advance(self, ft: int, pic: bytes) -> np.ndarray:
        b = self.buf
        if ft != 0x30:
            b[0], b[2] = b[2], b[0]
        rep = Report()
        cls = self.lib.hvqo_check_picture(self.o, ft, pic, len(pic), b[1].ctypes.data, b[0].ctypes.data, b[2].ctypes.data, C.byref(rep))
        if cls:
            raise RuntimeError(f"the stream's own picture is not defined: {class_name(cls)}")
        out = b[1].copy()
        if ft != 0x30:
            b[1], b[2] = b[2], b[1]
        return out


def clip_picsize(data: bytes) -> int:
    w = int.from_bytes(data[0x34:0x36], "big")
    h = int.from_bytes(data[0x36:0x38], "big")
    ss = data[0x38] * data[0x39]
    return w * h * (ss + 2) // ss


def oracle_decode(data: bytes, n_pictures: int) -> np.ndarray:
    """-> pictures uint8[n, picsize] (decode order) from this repo's CPU restatement"""
    lib = oracle()
    ps = clip_picsize(data)
    out = np.zeros((n_pictures, ps), dtype=np.uint8)
    n = lib.hvqo_decode_clip(data, len(data), out.ctypes.data, out.nbytes, n_pictures)
    if n != n_pictures:
        raise RuntimeError(f"oracle decoded {n} pictures, expected {n_pictures}")
    return out


def oracle_time(data: bytes, reps: int) -> Tuple[float, int]:
    px = C.c_uint64(0)
    t = oracle().hvqo_time_clip(data, len(data), reps, C.byref(px))
    return t, px.value


def ref_rgb(yuv: np.ndarray, w: int, h: int) -> np.ndarray:
    """RGB24 of a 4:2:0 picture through the reference's own dumpRGB"""
    import tempfile
    out = np.zeros(w * h * 3, dtype=np.uint8)
    yuv = np.ascontiguousarray(yuv)
    with tempfile.TemporaryDirectory() as d:
        rc = ref().ref_rgb(yuv.ctypes.data, w, h, out.ctypes.data, os.path.join(d, "x.ppm").encode())
    if rc:
        raise RuntimeError(f"ref_rgb failed: {rc}")
    return out


def oracle_rgb(yuv: np.ndarray, w: int, h: int) -> np.ndarray:
    out = np.zeros(w * h * 3, dtype=np.uint8)
    yuv = np.ascontiguousarray(yuv)
    oracle().hvqo_yuv420_to_rgb(yuv.ctypes.data, w, h, out.ctypes.data)
    return out
