"""Batched, device-resident decode path (include/hvqm4_amd.h) -- thin ctypes layer."""
from __future__ import annotations

import ctypes as C
import weakref
from typing import List, Optional

import numpy as np

from ._lib import HVQ_E_ARG, HvqComposeDst, HvqComposeLayer, HvqError, HvqScaleDst, HvqStats, HvqWarp, HvqWarpDst, check, lib

# HvqScaleDst as a numpy record: a pointer and eight int32 (width, height, h_samp, v_samp, crop_x, crop_y, crop_w, crop_h)
_SCALE_DST = np.dtype([("ptr", np.uint64), ("rest", np.int32, (8,))])
assert _SCALE_DST.itemsize == C.sizeof(HvqScaleDst)
# HvqWarp (six coefficients and the border; fill[3] and pad) and HvqWarpDst (a pointer; width, height, h_samp, v_samp) likewise
_WARP = np.dtype([("m", np.int32, (7,)), ("fill", np.uint8, (4,))])
_WARP_DST = np.dtype([("ptr", np.uint64), ("rest", np.int32, (4,))])
assert _WARP.itemsize == C.sizeof(HvqWarp) == 32 and _WARP_DST.itemsize == C.sizeof(HvqWarpDst) == 24
# HvqComposeLayer (ten dwords) and HvqComposeDst (a pointer; width, height, h_samp, v_samp, first, count, shift, bias[3]) likewise
_COMPOSE_DST = np.dtype([("ptr", np.uint64), ("rest", np.int32, (10,))])
assert C.sizeof(HvqComposeLayer) == 40 and _COMPOSE_DST.itemsize == C.sizeof(HvqComposeDst) == 48


class Context:
    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        self._geom = {}                                    # stream id -> (width, height), for export()
        self._geom4 = {}                                   # stream id -> (width, height, h_samp, v_samp), filled by _geometry
        check(lib().hvq_context_create(device, C.byref(self._h)))

    def set_launch_queues(self, n: int) -> None:
        """1 or 2 launch queues for this context's batches (hvq_context_set_launch_queues); 1 when two contexts share the GPU"""
        check(lib().hvq_context_set_launch_queues(self._h, n))

    def set_group_bytes(self, nbytes: int) -> None:
        """reuse window a launch group of this context's batches may span (hvq_context_set_group_bytes); 0: batches are never split"""
        check(lib().hvq_context_set_group_bytes(self._h, nbytes))

    def launch_groups(self) -> int:
        """launch groups of the last flushed batch (hvq_context_launch_groups), 0: nothing flushed"""
        return check(lib().hvq_context_launch_groups(self._h))

    def open_stream(self, width: int, height: int, h_samp: int = 2, v_samp: int = 2, is15: bool = True,
                    nslots: int = 4) -> int:
        sid = check(lib().hvq_stream_open(self._h, width, height, h_samp, v_samp, int(is15), nslots))
        self._geom[sid] = (width, height)
        return sid

    def close_stream(self, sid: int) -> None:
        check(lib().hvq_stream_close(self._h, sid))
        self._geom.pop(sid, None)
        self._geom4.pop(sid, None)

    def set_parse_threads(self, sid: int, threads: int) -> int:
        """host threads that share the parse of ONE picture of this stream (hvq_stream_set_parse_threads); returns the count in effect"""
        return check(lib().hvq_stream_set_parse_threads(self._h, sid, threads))

    def submit(self, sid: int, frame_type: int, picture: bytes) -> int:
        return check(lib().hvq_stream_submit(self._h, sid, frame_type, picture, len(picture)))

    def submit_many(self, sids, frame_types, pictures, threads: int = 1):
        """parse `pictures` on a host thread pool (per-stream order kept) and queue them in list order"""
        n = len(pictures)
        a_s = (C.c_int * n)(*sids)
        a_t = (C.c_int * n)(*frame_types)
        a_p = (C.c_char_p * n)(*pictures)
        a_l = (C.c_size_t * n)(*[len(p) for p in pictures])
        a_o = (C.c_int * n)()
        check(lib().hvq_submit_many(self._h, n, a_s, a_t, a_p, a_l, threads, a_o))
        return list(a_o)

    def submit_many_device(self, sids, frame_types, pictures, defer: bool = False):
        """queue raw bitstreams; flush() parses them on the GPU (no host entropy parse at all).  defer=True
        (hvq_submit_many_device_async): the copy into the pinned arena runs on a worker thread of the library and the call returns at
        once; the pictures are kept alive here until the next flush_begin / sync joins the worker"""
        n = len(pictures)
        a_s = (C.c_int * n)(*sids)
        a_t = (C.c_int * n)(*frame_types)
        a_p = (C.c_char_p * n)(*pictures)
        a_l = (C.c_size_t * n)(*[len(p) for p in pictures])
        a_o = (C.c_int * n)()
        fn = lib().hvq_submit_many_device_async if defer else lib().hvq_submit_many_device
        check(fn(self._h, n, a_s, a_t, a_p, a_l, a_o))
        if defer:
            self._submit_keep = (a_p, pictures)
        return list(a_o)

    def arena_reserve(self, nbytes: int):
        """hvq_arena_reserve: a writable uint8 view of `nbytes` of the pinned arena the library uploads from (zero-copy submit);
        valid until submit_many_arena / the next flush_begin"""
        import numpy as np
        ptr = C.c_void_p()
        check(lib().hvq_arena_reserve(self._h, nbytes, C.byref(ptr)))
        return np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(ptr.value))

    @staticmethod
    def arena_stride(length: int) -> int:
        return int(lib().hvq_arena_stride(length))

    def submit_many_arena(self, sids, frame_types, offsets, lengths):
        """queue pictures the caller wrote into the reservation itself (picture i at offsets[i], lengths[i] bytes): no copy"""
        n = len(offsets)
        a_s = (C.c_int * n)(*sids)
        a_t = (C.c_int * n)(*frame_types)
        a_f = (C.c_size_t * n)(*offsets)
        a_l = (C.c_size_t * n)(*lengths)
        a_o = (C.c_int * n)()
        check(lib().hvq_submit_many_arena(self._h, n, a_s, a_t, a_f, a_l, a_o))
        return list(a_o)

    def flush(self) -> None:
        check(lib().hvq_flush(self._h))

    def flush_begin(self) -> None:
        """first half of a flush (uploads + entropy-parse kernel queued); the next batch may be submitted before flush_end"""
        check(lib().hvq_flush_begin(self._h))

    def flush_end(self) -> None:
        check(lib().hvq_flush_end(self._h))

    def flush_next(self) -> None:
        """streaming step: end the batch in flight and begin the queued one, the queued batch's parse kernel launched first
        (hvq_flush_next); equals flush_end() + flush_begin() in effect"""
        check(lib().hvq_flush_next(self._h))

    def sync(self) -> None:
        check(lib().hvq_sync(self._h))

    def replay(self, reps: int) -> float:
        ms = C.c_float(0)
        check(lib().hvq_replay(self._h, reps, C.byref(ms)))
        return float(ms.value)

    def replay_stage(self, reps: int, what: int = 1) -> float:
        """hvq_replay_stage: what = 1 queue build + reconstruction per repetition, 2 queue build only, 0 = replay"""
        ms = C.c_float(0)
        check(lib().hvq_replay_stage(self._h, reps, what, C.byref(ms)))
        return float(ms.value)

    def pic_bytes(self, sid: int) -> int:
        return int(lib().hvq_stream_pic_bytes(self._h, sid))

    def read_picture(self, sid: int, ordinal: int) -> np.ndarray:
        out = np.empty(self.pic_bytes(sid), dtype=np.uint8)
        check(lib().hvq_read_picture(self._h, sid, ordinal, out.ctypes.data, out.nbytes))
        return out

    def read_picture_rgb(self, sid: int, ordinal: int, width: int, height: int) -> np.ndarray:
        """RGB24 (h, w, 3) of a resident picture: the reference player's dumpRGB on the GPU"""
        out = np.empty(width * height * 3, dtype=np.uint8)
        check(lib().hvq_read_picture_rgb(self._h, sid, ordinal, out.ctypes.data, out.nbytes))
        return out.reshape(height, width, 3)

    def convert_yuv420_rgb(self, yuv: np.ndarray, width: int, height: int) -> np.ndarray:
        """the reference player's dumpRGB (h4m:897-926) on a host picture (Y|U|V 4:2:0) -> RGB24 (h, w, 3)"""
        yuv = np.ascontiguousarray(yuv, dtype=np.uint8)
        assert yuv.size == width * height * 3 // 2
        out = np.empty(width * height * 3, dtype=np.uint8)
        check(lib().hvq_convert_yuv420_rgb(self._h, yuv.ctypes.data, width, height, out.ctypes.data))
        return out.reshape(height, width, 3)

    def read_pictures(self, sids, ordinals, out: Optional[np.ndarray] = None) -> np.ndarray:
        """bulk readback (hvq_read_pictures): one synchronisation for all of them -> uint8[n, pic_bytes] (all streams of one size)"""
        n = len(sids)
        nb = self.pic_bytes(sids[0]) if n else 0
        if out is None:
            out = np.empty((n, nb), dtype=np.uint8)
        a_s = (C.c_int * n)(*sids)
        a_o = (C.c_int * n)(*ordinals)
        a_d = (C.c_void_p * n)(*[out.ctypes.data + i * out.strides[0] for i in range(n)])
        check(lib().hvq_read_pictures(self._h, n, a_s, a_o, a_d))
        return out

    def pinned_array(self, shape) -> np.ndarray:
        """uint8 array in pinned host memory (hvq_pinned_alloc).  The memory lives as long as the array or any view of it: it is
        freed when the last of them is collected, not when the context closes."""
        nbytes = int(np.prod(shape))
        p = lib().hvq_pinned_alloc(nbytes)
        if not p:
            raise MemoryError("hvq_pinned_alloc failed: " + lib().hvq_last_error_string().decode(errors="replace"))
        buf = (C.c_uint8 * nbytes).from_address(p)
        weakref.finalize(buf, lib().hvq_pinned_free, p)         # numpy views keep `buf` alive through their base
        return np.frombuffer(buf, dtype=np.uint8).reshape(shape)

    def picture_device_ptr(self, sid: int, ordinal: int) -> int:
        ptr = C.c_void_p()
        check(lib().hvq_picture_device_ptr(self._h, sid, ordinal, C.byref(ptr)))
        return int(ptr.value or 0)

    # ---- what the calls on resident pictures share (export() and everything below it): each check where the calls have it, in their
    # order.  Static, and named through the class: the methods also run on a stand-in that has only _geom, _h and pic_bytes
    @staticmethod
    def _pictures(geom, sids, ordinals, limit: bool = False) -> int:
        """the picture list of a call on a context whose open streams are `geom`'s keys -> n.  limit: a call of several jobs a picture
        refuses more than 65535 pictures here, and looks at every distinct stream once"""
        n = len(sids)
        if len(ordinals) != n:
            raise ValueError(f"{n} streams but {len(ordinals)} ordinals")
        if limit and n > 65535:
            raise ValueError(f"{n} pictures: one call takes 65535 at the most")
        for s in (set(sids) if limit else sids):
            if s not in geom:
                raise HvqError(HVQ_E_ARG, f"bad stream {s}")
        return n

    @staticmethod
    def _out_tensor(out, shape, dtype, device="cuda", name="out", align=0):
        """the tensor a call writes: a new one, or the caller's after its checks (the device is checked last)"""
        import torch
        if out is None:
            return torch.empty(shape, dtype=dtype, device=device)
        if not isinstance(out, torch.Tensor) or out.dtype != dtype or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {str(dtype).replace('torch.', '')} tensor of shape {tuple(shape)}")
        if align and out.data_ptr() & (align - 1):
            raise ValueError(f"{name}: pointer {out.data_ptr():#x} must be a multiple of {align}")
        if out.device.type != "cuda":
            raise ValueError(f"{name} is on {out.device}, not a GPU")
        return out

    @staticmethod
    def _out_list(out, n, check):
        """the caller's list of n tensors that a call writes -> a list; check(i, t) raises on a tensor the call does not take (the device
        is checked last)"""
        if not isinstance(out, (list, tuple)) or len(out) != n:
            raise ValueError(f"out must be a list of {n} tensors")
        for i, t in enumerate(out):
            check(i, t)
            if t.device.type != "cuda":
                raise ValueError(f"out[{i}] is on {t.device}, not a GPU")
        return list(out)

    @staticmethod
    def _no_zeros(refs, why):
        """the references of a call that takes no picture of zeros; why: the call's words for it"""
        for i, r in enumerate(refs or ()):
            if r[0] < 0 and r[2] is None:
                raise ValueError(f"reference {i} is None: {why}")

    @staticmethod
    def _slot_outputs(out, nb, uniform, differ):
        """the pictures in slot layout that a call writes, nb[i] bytes each: one uint8 tensor [n, bytes] when the geometries are one
        (`uniform`), a list of n otherwise; a new one, or the caller's after its checks -> (out, its device, uint64[n] the pictures'
        addresses).  differ: what differs when a list is asked for, for the message"""
        import torch
        n = len(nb)
        width = nb[0] if n else 0
        if out is None:
            out = torch.empty((n, width), dtype=torch.uint8, device="cuda") if uniform else [torch.empty(b, dtype=torch.uint8, device="cuda") for b in nb]
        if uniform:
            if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (n, width) or not out.is_contiguous():
                raise ValueError(f"out must be a contiguous uint8 tensor of shape ({n}, {width})")
            device = out.device
            where = np.arange(n, dtype=np.uint64) * np.uint64(width) + np.uint64(out.data_ptr())       # rows of a multiple of 16 bytes
        else:
            if not isinstance(out, (list, tuple)) or len(out) != n:
                raise ValueError(f"out must be a list of {n} tensors (the {differ} differ)")
            for i, t in enumerate(out):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1 or t.shape[0] != nb[i] or not t.is_contiguous():
                    raise ValueError(f"out[{i}] must be a contiguous uint8 tensor of shape ({nb[i]},)")
            device = out[0].device if n else torch.device("cuda")
            where = np.array([t.data_ptr() for t in out], dtype=np.uint64)
            if len({t.get_device() for t in out}) > 1:
                raise ValueError("out: the tensors lie on different devices")
        if n and int(np.bitwise_and(where, np.uint64(15)).max()):
            i = int(np.flatnonzero(np.bitwise_and(where, np.uint64(15)))[0])
            raise ValueError(f"out: the pointer of picture {i}, {int(where[i]):#x}, must be a multiple of 16")
        if device.type != "cuda":
            raise ValueError(f"out is on {device}, not a GPU")
        return out, device, where

    @staticmethod
    def _slot_frame(ctx, sids, ordinals, src, out):
        """what the calls that write pictures of the sources' own geometry share (filter, rank, map), after their own checks: the
        sources and _slot_outputs -> (ptrs, out, device, where)"""
        from .checksums import sources
        streams = set(sids)
        pb = {s: ctx.pic_bytes(s) for s in streams}                        # a call usually repeats few streams: each is looked at once
        ptrs = sources(src, ordinals, lambda i: pb[sids[i]])
        uniform = len({ctx._geometry(s) for s in streams}) <= 1
        return (ptrs,) + Context._slot_outputs(out, [pb[s] for s in sids], uniform, "geometries")

    @staticmethod
    def _table_which(arg, n, cls, name, kind, most=None, nouns=None, also=""):
        """one `cls` for all n pictures (or records), or a list of n -> (table, which): equal entries share an entry of `table`, which
        `which` indexes per picture (None: the one for all).  For the messages: name, the argument's; kind, the class's; also, what
        else the argument may be; and `most` distinct entries (None: any number) called `nouns`"""
        if isinstance(arg, cls):
            return [arg], None
        if not isinstance(arg, (list, tuple)) or len(arg) != n:
            raise ValueError(f"{name}: one {kind}, {'' if also else 'or '}a list of {n}{also}")
        index, table, which = {}, [], []
        for e in arg:
            if not isinstance(e, cls):
                raise ValueError(f"{name}: an entry is a {kind}, not {type(e).__name__}")
            if e not in index:
                index[e] = len(table)
                table.append(e)
            which.append(index[e])
        if most is not None and len(table) > most:
            raise ValueError(f"{len(table)} distinct {nouns}: one call takes {most} at the most")
        return table, which

    @staticmethod
    def _which_array(which, n):
        """_table_which's `which` -> int[n], or None"""
        return None if which is None else C.cast((C.c_int * n)(*which), C.c_void_p)

    @staticmethod
    def _target_shapes(geoms, sids, wanted, one, shape):
        """the target shapes of a call (scale, warp).  A call usually repeats few: each distinct (source geometry, *what is wanted of
        picture i) is looked at once, by shape(*key) -> a tuple.  geoms: _geometry per stream; wanted: lists of one entry per
        picture; one: every list repeats one entry.  -> (shapes, column): the tuples by key, and column(j) = element j of picture i's
        tuple for every i (broadcast: the bare element where all pictures share it)"""
        n = len(sids)
        if n and one and len(set(geoms.values())) == 1:
            keys = [(geoms[sids[0]],) + tuple(v[0] for v in wanted)] * n
            distinct = keys[:1]
        else:
            keys = list(zip(map(geoms.__getitem__, sids), *wanted))
            distinct = set(keys)
        shapes = {key: shape(*key) for key in distinct}

        def column(j, broadcast=False):
            if len(shapes) == 1:
                v = shapes[keys[0]][j]
                return v if broadcast else [v] * n
            return [shapes[k][j] for k in keys]
        return shapes, column

    @staticmethod
    def _ref_array(refs):
        """metrics.references' result -> HvqMetricsRef[n], or None"""
        from .metrics import HvqMetricsRef
        return None if refs is None else C.cast((HvqMetricsRef * len(refs))(*[HvqMetricsRef(s, o, p) for s, o, p in refs]), C.c_void_p)

    @staticmethod
    def _ptr_array(ptrs):
        """checksums.sources' result, or any list of addresses -> void *[n], or None"""
        return None if ptrs is None else C.cast((C.c_void_p * len(ptrs))(*ptrs), C.c_void_p)

    @staticmethod
    def _launch_args(device, sids, ordinals):
        """once everything is checked: one HIP runtime in the process, then (int[n] streams, int[n] ordinals, torch's current stream of
        `device`; None: no stream)"""
        import torch
        from .export import check_one_hip_runtime
        check_one_hip_runtime()
        stream = None if device is None else torch.cuda.current_stream(device).cuda_stream
        return (C.c_int * len(sids))(*sids), (C.c_int * len(ordinals))(*ordinals), C.c_void_p(stream)

    def export(self, sids, ordinals, out, fmt: str = "rgb") -> None:
        """hvq_export_pictures: resident pictures into uint8 CUDA tensors, in one launch on torch's current stream of `out`'s
        device, without a host synchronisation.  fmt "rgb" -> [H, W, 3], "rgbp" (RGB planar) and "yuv444p" -> [3, H, W]; `out` is
        one tensor [N, ...] (pictures of one geometry) or a list of N tensors; views with larger row / plane strides are fine.
        Work queued on that stream afterwards sees the pictures; the library keeps their slots from being rewritten before the
        export has read them."""
        import torch
        from .export import FORMATS, HvqExportDst, destinations
        n = Context._pictures(self._geom, sids, ordinals)
        geoms = [self._geom[s] for s in sids]
        dsts = destinations(out, geoms, fmt)
        dev = out.device if isinstance(out, torch.Tensor) else (out[0].device if n else torch.device("cuda"))
        a_s, a_o, stream = Context._launch_args(dev, sids, ordinals)
        a_d = (HvqExportDst * n)(*[HvqExportDst(p, r, pl) for p, r, pl in dsts])
        check(lib().hvq_export_pictures(self._h, n, a_s, a_o, FORMATS[fmt], C.cast(a_d, C.c_void_p), stream))

    def export_float(self, sids, ordinals, out, *, crop=None, mean=(0, 0, 0), std=(1, 1, 1), scale: float = 1 / 255,
                     antialias: bool = False) -> None:
        """hvq_export_tensors: resident pictures as the float tensors a network eats -- crop, bilinear resize (half-sample centres
        as F.interpolate(mode="bilinear", align_corners=False, antialias=False), taps clamped to the crop), (v * scale - mean) / std
        per channel and the conversion to `out`'s dtype, planar RGB, in one launch on torch's current stream of `out`'s device.
        `out` is one float32 / float16 / bfloat16 tensor [N, 3, H, W] or a list of N tensors [3, H_i, W_i]: their shapes pick the
        output sizes (H, W equal to the crop's: no resampling, normalise only).  `crop`: None (whole pictures), one (x, y, w, h)
        in luma samples for all, or a list per picture.  The arithmetic is specified in include/hvqm4_amd.h: v is the uint8
        sample export(..., "rgbp") gives, as a float, and the call computes v * mul + add with mul = scale / std and
        add = -mean / std rounded once to float32.  Ordering and slot safety are export()'s.
        antialias=True resizes with hvq_export_resampled's triangle filter instead -- F.interpolate(..., antialias=True),
        torchvision's Resize default: the filter to take when the output is smaller than the crop.  Same destinations, crops and
        normalisation; at the crop's own size the same bits."""
        from .export import FILTER_TRIANGLE
        self._export_float(sids, ordinals, out, crop, mean, std, scale, FILTER_TRIANGLE if antialias else None)

    def _export_float(self, sids, ordinals, out, crop, mean, std, scale, filt) -> None:
        """export_float; filt = None: hvq_export_tensors, else hvq_export_resampled with that HVQ_FILTER_* (tools and tests pass
        FILTER_TRIANGLE_DIRECT)"""
        import torch
        from .export import HvqTensorDst, crops, float_destinations, normalisation
        n = Context._pictures(self._geom, sids, ordinals)
        mul, add = normalisation(mean, std, scale)
        rects = crops(crop, [self._geom[s] for s in sids])
        dtype, dsts = float_destinations(out, n)
        dev = out.device if isinstance(out, torch.Tensor) else (out[0].device if n else torch.device("cuda"))
        a_s, a_o, stream = Context._launch_args(dev, sids, ordinals)
        a_d = (HvqTensorDst * n)(*[HvqTensorDst(p, r, pl, w, h, *rect) for (p, r, pl, w, h), rect in zip(dsts, rects)])
        if filt is None:
            check(lib().hvq_export_tensors(self._h, n, a_s, a_o, dtype, (C.c_float * 3)(*mul), (C.c_float * 3)(*add),
                                           C.cast(a_d, C.c_void_p), stream))
        else:
            check(lib().hvq_export_resampled(self._h, n, a_s, a_o, dtype, int(filt), (C.c_float * 3)(*mul), (C.c_float * 3)(*add),
                                             C.cast(a_d, C.c_void_p), stream))

    def picture_metrics(self, sids, ordinals, ref=None, out=None):
        """hvq_picture_metrics: per plane (Y, U, V) the exact integers sum_a, sum_b, sum |a - b| and sum (a - b)^2 of resident
        pictures a = (sids[i], ordinals[i]) against their references, in one launch on torch's current stream, without a host
        synchronisation -> int64 CUDA tensor [n, 3, 4] (`out`, if given: such a tensor, contiguous; it is overwritten whole).
        `ref`: None (every picture against zeros: sum, sum of squares -> mean and variance) or a list with one entry per picture:
        None (zeros), (sid, ordinal) -- a resident picture of the same geometry, of any stream -- or a contiguous uint8 CUDA tensor of
        pic_bytes(sid) elements laid out as the pictures are (Y | U | V; the caller keeps it alive until the work has run).
        hvqm4_amd.metrics turns the records into PSNR, mean absolute difference, mean and variance.  Ordering and slot safety are
        export()'s."""
        import torch
        from .metrics import references
        n = Context._pictures(self._geom, sids, ordinals)
        refs = references(ref, n, lambda i: self.pic_bytes(sids[i]))
        out = Context._out_tensor(out, (n, 3, 4), torch.int64)
        a_s, a_o, stream = Context._launch_args(out.device, sids, ordinals)
        check(lib().hvq_picture_metrics(self._h, n, a_s, a_o, Context._ref_array(refs), C.c_void_p(out.data_ptr()), stream))
        return out

    def picture_ssim(self, sids, ordinals, ref, out=None, maps=False):
        """hvq_picture_ssim: windowed SSIM (8 x 8 windows 4 samples apart, the arithmetic of x264 / ffmpeg's ssim filter, specified in
        include/hvqm4_amd.h) of resident pictures a = (sids[i], ordinals[i]) against their references, in one launch on torch's
        current stream, without a host synchronisation -> int64 CUDA tensor [n, 3, 2] = per plane (sum_f, windows) (`out`, if given:
        such a tensor, contiguous; it is overwritten whole).  `ref` is required: a list with one entry per picture, (sid, ordinal)
        -- a resident picture of the same geometry -- or a contiguous uint8 CUDA tensor of pic_bytes(sid) elements laid out as the
        pictures are.  maps=True: -> (out, maps), maps a list of n triples of float32 CUDA tensors [rows_p, cols_p], the window
        values of Y, U, V (views of one allocation per pair).  hvqm4_amd.metrics.ssim / ssim_all / ssim_db read the records.
        Ordering and slot safety are export()'s."""
        import torch
        from .metrics import references
        n = Context._pictures(self._geom, sids, ordinals)
        if ref is None:
            raise ValueError("picture_ssim needs a reference for every picture (SSIM against zeros means nothing)")
        refs = references(ref, n, lambda i: self.pic_bytes(sids[i]))
        Context._no_zeros(refs, "SSIM against zeros means nothing")
        out = Context._out_tensor(out, (n, 3, 2), torch.int64)
        a_s, a_o, stream = Context._launch_args(out.device, sids, ordinals)
        views, a_m = None, None
        if maps:
            views, ptrs = [], []
            for s in sids:
                dims = self._ssim_dims(s)
                buf = torch.empty(sum(r * c for r, c in dims), dtype=torch.float32, device=out.device)
                at, tri = 0, []
                for r, c in dims:
                    tri.append(buf[at:at + r * c].view(r, c))
                    at += r * c
                views.append(tuple(tri))
                ptrs.append(buf.data_ptr())
            a_m = Context._ptr_array(ptrs)
        check(lib().hvq_picture_ssim(self._h, n, a_s, a_o, Context._ref_array(refs), C.c_void_p(out.data_ptr()), a_m, stream))
        return (out, views) if maps else out

    def picture_checksums(self, sids, ordinals, src=None, out=None):
        """hvq_picture_checksums: zlib's CRC-32 and Adler-32 of every plane and of the whole picture (the bytes read_picture returns)
        of resident pictures (sids[i], ordinals[i]), computed on the device on torch's current stream, without a host
        synchronisation and without moving a picture -> int64 CUDA tensor [n, 8] = (crc32 Y, U, V, picture, adler32 Y, U, V,
        picture) (`out`, if given: such a tensor, contiguous; it is overwritten whole).  hvqm4_amd.checksums names the columns and
        gives the expected values of pictures on the host.  `src`: None, or a list with one entry per picture: None (the resident
        picture) or a contiguous uint8 CUDA tensor of pic_bytes(sid) elements laid out as the pictures of `sid` are (Y | U | V),
        checksummed instead; its ordinal must be -1 and the caller keeps it alive until the work has run.  Ordering and slot safety
        are export()'s."""
        import torch
        from .checksums import sources
        n = Context._pictures(self._geom, sids, ordinals)
        ptrs = sources(src, ordinals, lambda i: self.pic_bytes(sids[i]))
        out = Context._out_tensor(out, (n, 8), torch.int64)
        a_s, a_o, stream = Context._launch_args(out.device, sids, ordinals)
        check(lib().hvq_picture_checksums(self._h, n, a_s, a_o, Context._ptr_array(ptrs), C.c_void_p(out.data_ptr()), stream))
        return out

    def picture_hashes(self, sids, ordinals, src=None, out=None):
        """hvq_picture_hashes: three 64-bit perceptual hashes of the luma plane of resident pictures (sids[i], ordinals[i]) -- aHash,
        dHash and pHash as include/hvqm4_amd.h specifies them, exact integers -- and the sum of the luma samples, computed on the
        device on torch's current stream, without a host synchronisation and without moving a picture -> int64 CUDA tensor [n, 4] =
        (ahash, dhash, phash, sum_y) holding the bit patterns (`out`, if given: such a tensor, contiguous; it is overwritten whole).
        hvqm4_amd.phash names the columns, gives the expected values of pictures on the host and the Hamming distances; hash_nearest
        searches the records where they lie.  `src` as in picture_checksums: None, or per picture None (the resident picture) or a
        contiguous uint8 CUDA tensor of pic_bytes(sid) elements hashed instead, with ordinal -1.  Ordering and slot safety are
        export()'s."""
        import torch
        from .checksums import sources
        n = Context._pictures(self._geom, sids, ordinals)
        ptrs = sources(src, ordinals, lambda i: self.pic_bytes(sids[i]))
        out = Context._out_tensor(out, (n, 4), torch.int64)
        a_s, a_o, stream = Context._launch_args(out.device, sids, ordinals)
        check(lib().hvq_picture_hashes(self._h, n, a_s, a_o, Context._ptr_array(ptrs), C.c_void_p(out.data_ptr()), stream))
        return out

    def hash_nearest(self, queries, database=None, self_offset=-1, threshold=10, out=None):
        """hvq_hash_nearest: for every query hash the nearest database hash by Hamming distance, how many lie within `threshold` bits
        and the first such, on torch's current stream, without a host synchronisation -> int32 CUDA tensor [nq, 4] = (nearest,
        distance, within, first_within) (`out`, if given: such a tensor, contiguous, 16-byte aligned).  `queries`, `database`: int64
        CUDA tensors [n], or [n, k] of which column 0 counts; the stride is the tensor's own, so records[:, phash.PHASH] searches one
        column of picture_hashes' records where it lies.  self_offset < 0: every database hash is a candidate; otherwise query i sees
        candidates j < self_offset + i ("earlier than me").  database None: the queries themselves with self_offset 0, which is
        de-duplication of a sequence -- column first_within is then hvqm4_amd.phash.duplicates.  A query without a candidate gets
        (-1, 65, 0, -1)."""
        import torch
        from .phash import hash_views
        if not 0 <= threshold <= 64:
            raise ValueError(f"threshold {threshold} outside [0, 64]")
        (qp, nq, qs), (dp, ndb, ds), off = hash_views(queries, database, self_offset)
        out = Context._out_tensor(out, (nq, 4), torch.int32, device=queries.device, align=16)
        stream = Context._launch_args(out.device, (), ())[2]
        check(lib().hvq_hash_nearest(self._h, C.c_void_p(qp), nq, qs, C.c_void_p(dp) if ndb else None, ndb, ds, off, threshold,
                                     C.c_void_p(out.data_ptr()), stream))
        return out

    def picture_histograms(self, sids, ordinals, ref=None, src=None, out=None):
        """hvq_picture_histograms: per plane (Y, U, V) the 256-bin histogram of resident pictures a = (sids[i], ordinals[i]), in one
        launch on torch's current stream, without a host synchronisation -> int32 CUDA tensor [n, 3, 256] (`out`, if given: such a
        tensor, contiguous; it is overwritten whole).  `ref` None: bin v counts the samples equal to v (HVQ_HIST_VALUES).  `ref` a
        list with one entry per picture, (sid, ordinal) -- a resident picture of the same geometry, of any stream -- or a contiguous
        uint8 CUDA tensor of pic_bytes(sid) elements laid out as the pictures are: bin d counts the positions where |a - b| equals d
        (HVQ_HIST_ABSDIFF); an entry None is refused.  `src` as in picture_checksums: None, or per picture None (the resident
        picture) or a uint8 CUDA tensor counted instead, with ordinal -1.  hvqm4_amd.histograms reads the records (percentiles,
        Otsu, equalisation, histogram distances, maximum error).  Ordering and slot safety are export()'s."""
        import torch
        from .checksums import sources
        from .histograms import BINS, HIST_ABSDIFF, HIST_VALUES
        from .metrics import references
        n = Context._pictures(self._geom, sids, ordinals)
        refs = references(ref, n, lambda i: self.pic_bytes(sids[i]))
        Context._no_zeros(refs, "|a - 0| is a itself, ref=None gives its histogram")
        ptrs = sources(src, ordinals, lambda i: self.pic_bytes(sids[i]))
        out = Context._out_tensor(out, (n, 3, BINS), torch.int32)
        a_s, a_o, stream = Context._launch_args(out.device, sids, ordinals)
        check(lib().hvq_picture_histograms(self._h, n, a_s, a_o, Context._ptr_array(ptrs), HIST_VALUES if refs is None else HIST_ABSDIFF,
                                           Context._ref_array(refs), C.c_void_p(out.data_ptr()), stream))
        return out

    def picture_motion(self, sids, ordinals, ref, block=16, radius=8, out=None):
        """hvq_picture_motion: the block-matching motion field (full search on luma, specified in include/hvqm4_amd.h) of resident
        pictures a = (sids[i], ordinals[i]) against their references, in one launch on torch's current stream, without a host
        synchronisation -> a list of n int32 CUDA tensors [rows, cols, 4] = per block (dy, dx, cost, cost_zero): the block looks like
        the reference at (y + dy, x + dx) (`out`, if given: such a list, every tensor contiguous; they are overwritten whole).  `ref`
        is required: a list with one entry per picture, (sid, ordinal) -- a resident picture of the same geometry -- or a contiguous
        uint8 CUDA tensor of pic_bytes(sid) elements laid out as the pictures are.  `block` is 8 or 16 (16 only on streams whose width
        and height are multiples of 16), `radius` 0 .. 15.  hvqm4_amd.motion reads the fields on the host.  Ordering and slot safety
        are export()'s."""
        import torch
        from .metrics import references
        from .motion import MAX_RADIUS, blocks
        n = Context._pictures(self._geom, sids, ordinals)
        if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= MAX_RADIUS:
            raise ValueError(f"radius {radius!r}: an integer in [0, {MAX_RADIUS}]")
        dims = [blocks(self._geom[s][0], self._geom[s][1], block) for s in sids]
        if ref is None:
            raise ValueError("picture_motion needs a reference for every picture (motion against zeros means nothing)")
        refs = references(ref, n, lambda i: self.pic_bytes(sids[i]))
        Context._no_zeros(refs, "motion against zeros means nothing")
        if out is None:
            out = [torch.empty((r, c, 4), dtype=torch.int32, device="cuda") for r, c in dims]
        else:
            def field(i, t):
                r, c = dims[i]
                if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (r, c, 4) or not t.is_contiguous():
                    raise ValueError(f"out[{i}] must be a contiguous int32 tensor of shape ({r}, {c}, 4)")
            out = Context._out_list(out, n, field)
        a_s, a_o, stream = Context._launch_args(out[0].device if n else None, sids, ordinals)
        a_f = Context._ptr_array([t.data_ptr() for t in out])
        check(lib().hvq_picture_motion(self._h, n, a_s, a_o, Context._ref_array(refs), block, radius, a_f, stream))
        return out

    def encode_jpeg(self, sids, ordinals, quality=90, src=None, out=None, lengths=None):
        """hvq_encode_jpeg: each picture (sids[i], ordinals[i]) as one complete baseline JPEG (JFIF) file (specified byte for byte in
        include/hvqm4_amd.h) in device memory, on torch's current stream, without a host synchronisation -> (buffers, lengths): n uint8
        CUDA tensors, file i at the start of buffers[i], and an int64 CUDA tensor [n] of the files' lengths.  A length larger than its
        buffer says that the file did not fit (nothing of it was written): call again with that much room.  hvqm4_amd.jpeg.files turns the
        pair into bytes on the host.  `out`, if given: a list of n contiguous uint8 CUDA tensors whose data pointers are multiples of 16,
        of 631 elements at least (default: 2 * pic_bytes(sid) + 1024 each); `lengths`: a contiguous int64 CUDA tensor [n].  `src`, if
        given: a list with one entry per picture, None or a contiguous uint8 CUDA tensor of pic_bytes(sid) elements laid out as the
        pictures are; that memory is encoded in the picture's place and ordinals[i] must be -1.  Ordering and slot safety are export()'s."""
        import torch
        from .checksums import sources
        n = Context._pictures(self._geom, sids, ordinals)
        if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
            raise ValueError(f"quality {quality!r}: an integer in [1, 100]")
        ptrs = sources(src, ordinals, lambda i: self.pic_bytes(sids[i]))
        if out is None:
            out = [torch.empty(2 * self.pic_bytes(s) + 1024, dtype=torch.uint8, device="cuda") for s in sids]
        else:
            def file(i, t):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous() or t.numel() < 631:
                    raise ValueError(f"out[{i}] must be a contiguous one-dimensional uint8 tensor of 631 elements at least")
                if t.data_ptr() % 16:
                    raise ValueError(f"out[{i}]: the data pointer must be a multiple of 16")
            out = Context._out_list(out, n, file)
        lengths = Context._out_tensor(lengths, (n,), torch.int64, name="lengths")
        if not n:
            return out, lengths
        a_s, a_o, stream = Context._launch_args(lengths.device, sids, ordinals)
        a_f = Context._ptr_array([t.data_ptr() for t in out])
        a_c = C.cast((C.c_uint64 * n)(*[t.numel() for t in out]), C.c_void_p)
        check(lib().hvq_encode_jpeg(self._h, n, a_s, a_o, Context._ptr_array(ptrs), quality, a_f, a_c, C.c_void_p(lengths.data_ptr()), stream))
        return out, lengths

    def _geometry(self, sid):
        """(width, height, h_samp, v_samp) of an open stream"""
        g = self._geom4.get(sid)
        if g is None:
            w, h = self._geom[sid][:2]
            y = w * h
            c = (self.pic_bytes(sid) - y) // 2
            g = self._geom4[sid] = (w, h) + {y // 4: (2, 2), y // 2: (2, 1), y: (1, 1)}[c]
        return g

    def scale_force_direct(self, on: bool) -> bool:
        """hvq_scale_force_direct: every later scale_pictures of this context takes the direct body of the kernel (False: the chosen
        one again) -> the setting before.  The values do not depend on it: for tests that compare the two with =="""
        return bool(check(lib().hvq_scale_force_direct(self._h, int(bool(on)))))

    def scale_pictures(self, sids, ordinals, size, sampling=None, crop=None, src=None, out=None):
        """hvq_scale_pictures: resident pictures (sids[i], ordinals[i]) resampled plane by plane with the area filter (exact integers,
        one rounding: include/hvqm4_amd.h) into uint8 pictures of another geometry IN SLOT LAYOUT (Y | U | V), on torch's current
        stream, without a host synchronisation and without moving a picture.  `size`: (w, h), or one such pair per picture;
        `sampling`: None (the source's), (h_samp, v_samp), or one per picture (None entries: the source's); `crop`: None (the whole
        picture), (x, y, w, h) in luma samples, or one per picture.  -> when every target geometry is the same one uint8 CUDA tensor
        [n, bytes], otherwise a list of n 1-D uint8 CUDA tensors (`out`, if given: of that same form, contiguous, rows 16-byte
        aligned; it is overwritten whole).  Whatever takes src= or ref.ptr takes a row of the result, with an open stream of the
        target geometry to carry it.  hvqm4_amd.scale gives the expected bytes (of_picture), the plane views and the target sizes
        (fit, pyramid).  `src` as in picture_checksums.  Ordering and slot safety are export()'s."""
        from . import scale as sc
        from .checksums import sources
        n = Context._pictures(self._geom, sids, ordinals, limit=True)
        streams = set(sids)
        sizes, one_size = sc.per_picture(size, n, 2, "size")
        if n and (sizes[0] is None if one_size else any(v is None for v in sizes)):
            raise ValueError("size: every picture needs a target size")
        samplings, one_sampling = sc.per_picture(sampling, n, 2, "sampling")
        crops, one_crop = sc.per_picture(crop, n, 4, "crop")
        def shape(g, sz, sm, cr):
            dst = sz + (sm or g[2:])
            sc.plane_sizes(g, dst, cr)                                    # ValueError beyond the library's limits
            return dst, sc.nbytes(*dst), dst + (cr or (0, 0, 0, 0))
        geoms = {s: self._geometry(s) for s in streams}
        shapes, column = Context._target_shapes(geoms, sids, (sizes, samplings, crops), one_size and one_sampling and one_crop, shape)
        ptrs = sources(src, ordinals, lambda i: self.pic_bytes(sids[i]))
        uniform = len({v[0] for v in shapes.values()}) == 1
        out, device, where = Context._slot_outputs(out, column(1), uniform, "target geometries")
        if not n:
            return out
        a_s, a_o, stream = Context._launch_args(device, sids, ordinals)
        a_d = np.empty(n, dtype=_SCALE_DST)                                  # HvqScaleDst[n]
        a_d["ptr"] = where
        a_d["rest"] = column(2, broadcast=True)
        check(lib().hvq_scale_pictures(self._h, n, a_s, a_o, Context._ptr_array(ptrs), C.c_void_p(a_d.ctypes.data), stream))
        return out

    def filter_force_filter(self, on: bool) -> bool:
        """hvq_filter_force_filter: every later filter_pictures of this context runs identity planes through the filter body of the
        kernel instead of the copy body (False: the chosen one again) -> the setting before.  The values do not depend on it: for
        tests that compare the two with =="""
        return bool(check(lib().hvq_filter_force_filter(self._h, int(bool(on)))))

    def filter_pictures(self, sids, ordinals, filt, src=None, out=None):
        """hvq_filter_pictures: resident pictures (sids[i], ordinals[i]) through separable integer filters (exact integers, one
        rounding: include/hvqm4_amd.h) into uint8 pictures of their own geometry IN SLOT LAYOUT (Y | U | V), on torch's current
        stream, without a host synchronisation and without moving a picture.  `filt`: one hvqm4_amd.filters.Filter, or a list of one
        per picture (equal ones share an entry of the call's table; more than 64 distinct ones: ValueError).  -> when every geometry is
        the same one uint8 CUDA tensor [n, bytes], otherwise a list of n 1-D uint8 CUDA tensors (`out`, if given: of that same form,
        contiguous, rows 16-byte aligned; it is overwritten whole and must not overlap a source).  Whatever takes src= or ref.ptr
        takes a row of the result.  hvqm4_amd.filters builds the filters and gives the expected bytes (of_picture).  `src` as in
        picture_checksums.  Ordering and slot safety are export()'s."""
        from . import filters as fl
        n = Context._pictures(self._geom, sids, ordinals, limit=True)
        table, which = Context._table_which(filt, n, fl.Filter, "filt", "filters.Filter", fl.MAX_FILTERS, "filters")
        for f in table:
            fl.check(f)                                                    # ValueError beyond the library's limits
        ptrs, out, device, where = Context._slot_frame(self, sids, ordinals, src, out)
        if not n:
            return out
        a_s, a_o, stream = Context._launch_args(device, sids, ordinals)
        from ._lib import HvqFilter
        a_f = (HvqFilter * len(table))(*[f.to_struct() for f in table])
        a_w = Context._which_array(which, n)
        a_d = C.c_void_p(where.ctypes.data)                                  # void *[n]
        check(lib().hvq_filter_pictures(self._h, n, a_s, a_o, Context._ptr_array(ptrs), C.cast(a_f, C.c_void_p), len(table), a_w, a_d, stream))
        return out

    def rank_force_general(self, on: bool) -> bool:
        """hvq_rank_force_general: every later rank_pictures of this context runs the planes that are copied through the min/max body
        of the kernel instead of the copy body (False: the chosen one again) -> the setting before.  The values do not depend on it:
        for tests that compare the two with =="""
        return bool(check(lib().hvq_rank_force_general(self._h, int(bool(on)))))

    def rank_pictures(self, sids, ordinals, rank, src=None, out=None):
        """hvq_rank_pictures: resident pictures (sids[i], ordinals[i]) through rank filters -- erosion, dilation, the range, the 3 x 3
        or 5 x 5 median: samples are selected, nothing is rounded (include/hvqm4_amd.h) -- into uint8 pictures of their own geometry IN
        SLOT LAYOUT (Y | U | V), on torch's current stream, without a host synchronisation and without moving a picture.  `rank`: one
        hvqm4_amd.rank.Rank, or a list of one per picture (equal ones share an entry of the call's table; more than 64 distinct ones:
        ValueError).  -> when every geometry is the same one uint8 CUDA tensor [n, bytes], otherwise a list of n 1-D uint8 CUDA
        tensors (`out`, if given: of that same form, contiguous, rows 16-byte aligned; it is overwritten whole and must not overlap a
        source).  Whatever takes src= or ref.ptr takes a row of the result.  hvqm4_amd.rank builds the operations and gives the
        expected bytes (of_picture).  `src` as in picture_checksums.  Ordering and slot safety are export()'s."""
        from . import rank as rk
        n = Context._pictures(self._geom, sids, ordinals, limit=True)
        table, which = Context._table_which(rank, n, rk.Rank, "rank", "rank.Rank", rk.MAX_RANKS, "ranks")
        for r in table:
            rk.check(r)                                                    # ValueError beyond the library's limits
        ptrs, out, device, where = Context._slot_frame(self, sids, ordinals, src, out)
        if not n:
            return out
        a_s, a_o, stream = Context._launch_args(device, sids, ordinals)
        from ._lib import HvqRank
        a_r = (HvqRank * len(table))(*[r.struct() for r in table])
        a_w = Context._which_array(which, n)
        a_d = C.c_void_p(where.ctypes.data)                                  # void *[n]
        check(lib().hvq_rank_pictures(self._h, n, a_s, a_o, Context._ptr_array(ptrs), C.cast(a_r, C.c_void_p), len(table), a_w, a_d, stream))
        return out

    def morph_pictures(self, sids, ordinals, steps, out=None, src=None):
        """resident pictures (sids[i], ordinals[i]) through a list of rank steps (hvqm4_amd.rank.opening / closing, or any list of
        rank.Rank), one rank_pictures a step on torch's current stream: the first from the resident pictures, every later one from the
        result before it through src=.  The results between the steps alternate between two scratch tensors of the output's form; the
        last lands in `out` (rank_pictures' rules; default: a new one).  No host synchronisation.  -> rank_pictures' return forms.
        `src` as in rank_pictures: the first step then reads the caller's memory (a mask of map_pictures, say).  hvqm4_amd.rank.of_steps
        gives the expected bytes."""
        from . import rank as rk
        steps = rk.as_steps(steps)
        n = len(sids)
        cur = spare = None
        for k, step in enumerate(steps):
            dst = out if k == len(steps) - 1 else spare
            if cur is None:
                res = self.rank_pictures(sids, ordinals, step, src=src, out=dst)
            else:
                res = self.rank_pictures(sids, [-1] * n, step, src=[cur[i] for i in range(n)], out=dst)
            spare, cur = cur, res
        return cur

    def bilateral_force_general(self, on: bool) -> bool:
        """hvq_bilateral_force_general: every later bilateral_pictures of this context runs the planes of radius 0 through the general
        body of the kernel instead of the copy body (False: the chosen one again) -> the setting before.  The values do not depend on
        it: for tests that compare the two with =="""
        return bool(check(lib().hvq_bilateral_force_general(self._h, int(bool(on)))))

    def bilateral_pictures(self, sids, ordinals, bil, guide=None, src=None, out=None):
        """hvq_bilateral_pictures: resident pictures (sids[i], ordinals[i]) through bilateral filters -- a weighted mean whose weights
        are a spatial table times a range table of the guide's difference, exact integers with one rounding (include/hvqm4_amd.h) --
        into uint8 pictures of their own geometry IN SLOT LAYOUT (Y | U | V), on torch's current stream, without a host synchronisation
        and without moving a picture.  `bil`: one hvqm4_amd.bilateral.Bilateral, or a list of one per picture (equal ones share an
        entry of the call's table; more than 64 distinct ones: ValueError).  `guide`: None (every picture guides itself) or a list of
        one entry per picture as picture_metrics' `ref` -- None (itself), (sid, ordinal) (a resident picture of the same geometry) or
        a uint8 CUDA tensor in slot layout.  Return forms and `out` are rank_pictures'; whatever takes src= or ref.ptr takes a row of
        the result.  hvqm4_amd.bilateral builds the sets and gives the expected bytes (of_picture).  `src` as in picture_checksums.
        Ordering and slot safety are export()'s."""
        from . import bilateral as bl
        from .metrics import references
        n = Context._pictures(self._geom, sids, ordinals, limit=True)
        table, which = Context._table_which(bil, n, bl.Bilateral, "bil", "bilateral.Bilateral", bl.MAX_SETS, "sets")
        for b in table:
            bl.check(b)                                                    # ValueError beyond the library's limits
        refs = references(guide, n, lambda i: self.pic_bytes(sids[i]))
        ptrs, out, device, where = Context._slot_frame(self, sids, ordinals, src, out)
        if not n:
            return out
        a_s, a_o, stream = Context._launch_args(device, sids, ordinals)
        from ._lib import HvqBilateral
        a_b = (HvqBilateral * len(table))(*[b.struct() for b in table])
        a_w = Context._which_array(which, n)
        a_d = C.c_void_p(where.ctypes.data)                                  # void *[n]
        check(lib().hvq_bilateral_pictures(self._h, n, a_s, a_o, Context._ptr_array(ptrs), Context._ref_array(refs), C.cast(a_b, C.c_void_p), len(table),
                                           a_w, a_d, stream))
        return out

    def smooth_pictures(self, sids, ordinals, steps, guide=None, out=None):
        """resident pictures (sids[i], ordinals[i]) through a list of bilateral steps (hvqm4_amd.bilateral.iterate, or any list of
        bilateral.Bilateral), one bilateral_pictures a step on torch's current stream: the first from the resident pictures, every later
        one from the result before it through src=, every step under `guide`.  The results between the steps alternate between two
        scratch tensors of the output's form; the last lands in `out` (rank_pictures' rules; default: a new one).  No host
        synchronisation.  -> rank_pictures' return forms.  hvqm4_amd.bilateral.of_steps gives the expected bytes."""
        from . import bilateral as bl
        steps = bl.as_steps(steps)
        n = len(sids)
        cur = spare = None
        for k, step in enumerate(steps):
            dst = out if k == len(steps) - 1 else spare
            if cur is None:
                res = self.bilateral_pictures(sids, ordinals, step, guide=guide, out=dst)
            else:
                res = self.bilateral_pictures(sids, [-1] * n, step, guide=guide, src=[cur[i] for i in range(n)], out=dst)
            spare, cur = cur, res
        return cur

    def map_pictures(self, sids, ordinals, tables, planes=7, src=None, out=None):
        """hvq_map_pictures: resident pictures (sids[i], ordinals[i]) through lookup tables, out = table[plane][in], nothing rounded
        (include/hvqm4_amd.h), into uint8 pictures of their own geometry IN SLOT LAYOUT (Y | U | V), on torch's current stream, without
        a host synchronisation and without moving a picture.  `tables`: one hvqm4_amd.maps.Table, a list of one per picture (equal
        ones share a record), or a uint8 CUDA tensor [m, 3, 256] with m 1 (for all) or n (one each), contiguous, 16-byte aligned: it
        is read when the work runs, so an earlier call on the stream (histogram_tables) may write it, and the caller keeps it alive
        until then.  `planes`: the mask of the planes that are looked up (1 Y, 2 U, 4 V); the others are copied.  Return forms and
        `out` are rank_pictures', except that an `out` row may BE the `src` row of the same picture (in place).  hvqm4_amd.maps builds
        tables and gives the expected bytes (of_picture).  `src` as in picture_checksums.  Ordering and slot safety are export()'s."""
        import torch
        from . import maps
        n = Context._pictures(self._geom, sids, ordinals, limit=True)
        if isinstance(planes, bool) or not isinstance(planes, int) or not 1 <= planes <= 7:
            raise ValueError(f"planes {planes!r}: a mask of the bits 0 .. 2, not 0")
        which = None
        if isinstance(tables, torch.Tensor):
            if tables.dtype != torch.uint8 or tables.dim() != 3 or tuple(tables.shape[1:]) != (3, 256) or not tables.is_contiguous():
                raise ValueError("tables must be a contiguous uint8 tensor of shape (m, 3, 256)")
            if n and tables.shape[0] not in (1, n):
                raise ValueError(f"{tables.shape[0]} tables for {n} pictures: 1, or one per picture")
            if tables.data_ptr() & 15:
                raise ValueError(f"tables: pointer {tables.data_ptr():#x} must be a multiple of 16")
            if tables.device.type != "cuda":
                raise ValueError(f"tables is on {tables.device}, not a GPU")
            dev_tables = tables
        else:
            records, which = Context._table_which(tables, n, maps.Table, "tables", "maps.Table", also=", or a uint8 CUDA tensor [m, 3, 256]")
            dev_tables = None
        ptrs, out, device, where = Context._slot_frame(self, sids, ordinals, src, out)
        if not n:
            return out
        if dev_tables is None:
            dev_tables = torch.from_numpy(maps.pack(records)).to(device)         # uploaded on the current stream, in front of the launch; torch frees it in stream order
        a_s, a_o, stream = Context._launch_args(device, sids, ordinals)
        a_w = Context._which_array(which, n)
        a_d = C.c_void_p(where.ctypes.data)                                  # void *[n]
        check(lib().hvq_map_pictures(self._h, n, a_s, a_o, Context._ptr_array(ptrs), C.c_void_p(dev_tables.data_ptr()), int(dev_tables.shape[0]), a_w,
                                     planes, a_d, stream))
        return out

    def histogram_tables(self, hist, rules, out=None):
        """hvq_histogram_tables: tables from the histogram records where they lie -- `hist` is picture_histograms' result without a
        reference, an int32 CUDA tensor [n, 3, 256] -- in one launch on torch's current stream, without a host synchronisation ->
        uint8 CUDA tensor [n, 3, 256] (`out`, if given: such a tensor, contiguous, 16-byte aligned; it is overwritten whole), which
        map_pictures takes as it is.  `rules`: one hvqm4_amd.maps.Rule (equalize(), stretch(), otsu(), flat(c)) or a list of one per
        record (more than 64 distinct ones: ValueError).  hvqm4_amd.maps.tables_of_records gives the expected tables."""
        import torch
        from . import maps
        if not isinstance(hist, torch.Tensor) or hist.dtype != torch.int32 or hist.dim() != 3 or tuple(hist.shape[1:]) != (3, 256) or not hist.is_contiguous():
            raise ValueError("hist must be a contiguous int32 tensor of shape (n, 3, 256)")
        n = int(hist.shape[0])
        if n > 65535:
            raise ValueError(f"{n} records: one call takes 65535 at the most")
        if hist.data_ptr() & 15:
            raise ValueError(f"hist: pointer {hist.data_ptr():#x} must be a multiple of 16")
        table, which = Context._table_which(rules, n, maps.Rule, "rules", "maps.Rule", maps.MAX_RULES, "rules")
        for r in table:
            maps.check(r)
        if hist.device.type != "cuda":
            raise ValueError(f"hist is on {hist.device}, not a GPU")
        out = Context._out_tensor(out, (n, 3, 256), torch.uint8, device=hist.device, align=16)
        if not n:
            return out
        stream = Context._launch_args(out.device, (), ())[2]
        from ._lib import HvqTableRule
        a_r = (HvqTableRule * len(table))(*[r.struct() for r in table])
        a_w = Context._which_array(which, n)
        check(lib().hvq_histogram_tables(self._h, n, C.c_void_p(hist.data_ptr()), C.cast(a_r, C.c_void_p), len(table), a_w, C.c_void_p(out.data_ptr()), stream))
        return out

    def equalize_pictures(self, sids, ordinals, rules=None, src=None, out=None):
        """resident pictures (sids[i], ordinals[i]) through tables made of their own histograms: picture_histograms ->
        histogram_tables(rules) -> map_pictures, three launches on torch's current stream, no host synchronisation; the histogram and
        table tensors are scratch.  `rules`: histogram_tables' (default: hvqm4_amd.maps.equalize().luma_only(), equalisation of Y with
        U and V as they are); maps.stretch() gives automatic levels, maps.otsu() a mask.  `src`, `out` and the return forms are
        map_pictures'.  The expected bytes: maps.of_picture with maps.tables_of_records of histograms.of_picture."""
        from . import maps
        if rules is None:
            rules = maps.equalize().luma_only()
        hist = self.picture_histograms(sids, ordinals, src=src)
        tables = self.histogram_tables(hist, rules)
        return self.map_pictures(sids, ordinals, tables, src=src, out=out)      # torch frees the scratch in stream order

    def label_pictures(self, sids, ordinals, rules=None, which=None, cap=1024, src=None, labels=None, comps=None):
        """hvq_label_pictures: the connected components of one plane of the resident pictures (sids[i], ordinals[i]) -- which samples
        are foreground, the neighbourhood and the numbering are include/hvqm4_amd.h's --, on torch's current stream, without a host
        synchronisation and without moving a picture.  `rules`: one hvqm4_amd.labels.Rule (default labels.rule(): the 255s of Y under
        the 8-neighbourhood, an Otsu mask), a list of one per picture (equal ones share an entry; more than 64 distinct ones:
        ValueError), or a list of distinct rules together with `which`, one index per picture.  -> (labels, comps): lists of n CUDA
        tensors, labels[i] int32 [Ny, Nx] of the rule's plane (0 background, k component k), comps[i] int64 [cap + 1, 8] (row 0: K,
        stored, F, status; row k: area, x0, y0, x1, y1, first, sum_x, sum_y; rows beyond `stored` keep what they held).  `labels` /
        `comps`, if given: such lists, contiguous, 16-byte aligned; `cap` is then the comps' room.  hvqm4_amd.labels gives the expected
        values (of_picture) and reads the records (records, centroids, boxes, largest).  `src` as in picture_checksums.  Ordering and
        slot safety are export()'s."""
        import torch
        from . import labels as lb
        n = Context._pictures(self._geom, sids, ordinals, limit=True)
        if which is not None:
            table = [rules] if isinstance(rules, lb.Rule) else list(rules or ())
            if not table or len(table) > lb.MAX_RULES:
                raise ValueError(f"{len(table)} rules: one call takes 1 .. {lb.MAX_RULES}")
            which = [int(k) for k in which]
            if len(which) != n or any(not 0 <= k < len(table) for k in which):
                raise ValueError(f"which: {n} indices into the {len(table)} rules")
        else:
            table, which = Context._table_which(lb.Rule() if rules is None else rules, n, lb.Rule, "rules", "labels.Rule", lb.MAX_RULES, "rules")
        for r in table:
            lb.check(r)
        if isinstance(cap, bool) or not isinstance(cap, int) or not 0 <= cap <= lb.MAX_CAP:
            raise ValueError(f"cap {cap!r} outside 0 .. {lb.MAX_CAP}")
        from .checksums import sources
        ptrs = sources(src, ordinals, lambda i: self.pic_bytes(sids[i]))
        shapes = [lb.plane_shape(self._geometry(sids[i]), table[which[i] if which else 0].plane) for i in range(n)]

        def taken(given, name, shape, dtype):
            if given is None:
                return [torch.empty(shape(i), dtype=dtype, device="cuda") for i in range(n)]

            def one(i, t):
                if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape(i)) or not t.is_contiguous():
                    raise ValueError(f"{name}[{i}] must be a contiguous {str(dtype).replace('torch.', '')} tensor of shape {tuple(shape(i))}")
                if t.data_ptr() & 15:
                    raise ValueError(f"{name}[{i}]: pointer {t.data_ptr():#x} must be a multiple of 16")
            try:
                return Context._out_list(given, n, one)
            except ValueError as e:
                raise ValueError(str(e).replace("out", name)) from None
        labels = taken(labels, "labels", lambda i: shapes[i], torch.int32)
        comps = taken(comps, "comps", lambda i: (cap + 1, 8), torch.int64)
        if not n:
            return labels, comps
        a_s, a_o, stream = Context._launch_args(labels[0].device, sids, ordinals)
        from ._lib import HvqLabelRule
        a_r = (HvqLabelRule * len(table))(*[r.struct() for r in table])
        a_w = Context._which_array(which, n)
        a_l = Context._ptr_array([t.data_ptr() for t in labels])
        a_c = Context._ptr_array([t.data_ptr() for t in comps])
        check(lib().hvq_label_pictures(self._h, n, a_s, a_o, Context._ptr_array(ptrs), C.cast(a_r, C.c_void_p), len(table), a_w, a_l, a_c, cap, stream))
        return labels, comps

    def corner_pictures(self, sids, ordinals, rules=None, which=None, cap=1024, src=None, mask=None, points=None, rows=None, response=None):
        """hvq_corner_pictures: the corners of one plane of the resident pictures (sids[i], ordinals[i]) -- the measure, the suppression
        and the order of the list are include/hvqm4_amd.h's --, on torch's current stream, without a host synchronisation and without
        moving a picture.  `rules`: one hvqm4_amd.corners.Rule (default corners.harris(): Y, radius 1, k 10, nms 3, threshold 1), a list
        of one per picture (equal ones share an entry; more than 64 distinct ones: ValueError), or a list of distinct rules together
        with `which`, one index per picture.  -> (mask, points, rows): lists of n CUDA tensors, mask[i] uint8 [pic_bytes] IN SLOT LAYOUT
        (255 at the corners of the rule's plane; it goes wherever `src=` goes), points[i] int64 [cap + 1, 4] (row 0: K, stored, status,
        0; row j: x, y, R, index, in raster order; rows beyond `stored` keep what they held), rows[i] int32 [Ny + 1] (the corners above
        each row).  `response`: True, or a list of int64 [Ny, Nx] tensors: every R of the plane, returned as a fourth list.  `mask` /
        `points` / `rows`, if given: such lists, contiguous, 16-byte aligned; `cap` is then the points' room.  hvqm4_amd.corners gives
        the expected values (of_picture, response_of_plane) and reads the list (records, strongest, grid).  `src` as in
        picture_checksums.  Ordering and slot safety are export()'s."""
        import torch
        from . import corners as cr
        n = Context._pictures(self._geom, sids, ordinals, limit=True)
        if which is not None:
            table = [rules] if isinstance(rules, cr.Rule) else list(rules or ())
            if not table or len(table) > cr.MAX_RULES:
                raise ValueError(f"{len(table)} rules: one call takes 1 .. {cr.MAX_RULES}")
            which = [int(k) for k in which]
            if len(which) != n or any(not 0 <= k < len(table) for k in which):
                raise ValueError(f"which: {n} indices into the {len(table)} rules")
        else:
            table, which = Context._table_which(cr.Rule() if rules is None else rules, n, cr.Rule, "rules", "corners.Rule", cr.MAX_RULES, "rules")
        for r in table:
            cr.check(r)
        if isinstance(cap, bool) or not isinstance(cap, int) or not 0 <= cap <= cr.MAX_CAP:
            raise ValueError(f"cap {cap!r} outside 0 .. {cr.MAX_CAP}")
        from .checksums import sources
        ptrs = sources(src, ordinals, lambda i: self.pic_bytes(sids[i]))
        shapes = [cr.plane_shape(self._geometry(sids[i]), table[which[i] if which else 0].plane) for i in range(n)]

        def taken(given, name, shape, dtype):
            if given is None:
                return [torch.empty(shape(i), dtype=dtype, device="cuda") for i in range(n)]

            def one(i, t):
                if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape(i)) or not t.is_contiguous():
                    raise ValueError(f"{name}[{i}] must be a contiguous {str(dtype).replace('torch.', '')} tensor of shape {tuple(shape(i))}")
                if t.data_ptr() & 15:
                    raise ValueError(f"{name}[{i}]: pointer {t.data_ptr():#x} must be a multiple of 16")
            try:
                return Context._out_list(given, n, one)
            except ValueError as e:
                raise ValueError(str(e).replace("out", name)) from None
        mask = taken(mask, "mask", lambda i: (self.pic_bytes(sids[i]),), torch.uint8)
        points = taken(points, "points", lambda i: (cap + 1, 4), torch.int64)
        rows = taken(rows, "rows", lambda i: (shapes[i][0] + 1,), torch.int32)
        asked = response is not None and response is not False
        if asked:
            response = taken(None if response is True else response, "response", lambda i: shapes[i], torch.int64)
        if not n:
            return (mask, points, rows, response) if asked else (mask, points, rows)
        a_s, a_o, stream = Context._launch_args(mask[0].device, sids, ordinals)
        from ._lib import HvqCornerRule
        a_r = (HvqCornerRule * len(table))(*[r.struct() for r in table])
        a_w = Context._which_array(which, n)
        a_m = Context._ptr_array([t.data_ptr() for t in mask])
        a_p = Context._ptr_array([t.data_ptr() for t in points])
        a_y = Context._ptr_array([t.data_ptr() for t in rows])
        a_q = Context._ptr_array([t.data_ptr() for t in response]) if asked else None
        check(lib().hvq_corner_pictures(self._h, n, a_s, a_o, Context._ptr_array(ptrs), C.cast(a_r, C.c_void_p), len(table), a_w, a_m, a_p, a_y, a_q, cap,
                                        stream))
        return (mask, points, rows, response) if asked else (mask, points, rows)

    def select_components(self, sids, labels, comps, select, which=None, out=None):
        """hvq_select_components: label maps and record tables of the Y planes (label_pictures' results under a rule with plane 0) back
        into uint8 pictures IN SLOT LAYOUT of the geometries of sids[i]: Y 255 where the sample's component has a record and its
        area, box width and box height lie in `select`'s ranges, else 0 (invert swaps the two), U and V 128.  `select`: one
        hvqm4_amd.labels.Select (labels.select(area=50): the specks below 50 samples go), a list of one per picture, or a list of
        distinct ones together with `which`.  labels and comps are read when the work runs on torch's current stream: label ->
        select needs no host synchronisation.  Return forms and `out` are rank_pictures'; whatever takes src= takes a row of the
        result.  hvqm4_amd.labels.of_select gives the expected bytes."""
        import torch
        from . import labels as lb
        n = Context._pictures(self._geom, sids, [0] * len(sids), limit=True)
        if which is not None:
            table = [select] if isinstance(select, lb.Select) else list(select or ())
            if not table or len(table) > lb.MAX_SELECTS:
                raise ValueError(f"{len(table)} selections: one call takes 1 .. {lb.MAX_SELECTS}")
            which = [int(k) for k in which]
            if len(which) != n or any(not 0 <= k < len(table) for k in which):
                raise ValueError(f"which: {n} indices into the {len(table)} selections")
        else:
            table, which = Context._table_which(select, n, lb.Select, "select", "labels.Select", lb.MAX_SELECTS, "selections")
        for e in table:
            lb.check_select(e)
        if not isinstance(labels, (list, tuple)) or not isinstance(comps, (list, tuple)) or len(labels) != n or len(comps) != n:
            raise ValueError(f"labels and comps must be lists of {n} tensors")
        cap = int(comps[0].shape[0]) - 1 if n else 0
        for i in range(n):
            w, h = self._geometry(sids[i])[:2]
            t, c = labels[i], comps[i]
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (h, w) or not t.is_contiguous() or t.data_ptr() & 15:
                raise ValueError(f"labels[{i}] must be a contiguous, 16-byte aligned int32 tensor of shape ({h}, {w})")
            if not isinstance(c, torch.Tensor) or c.dtype != torch.int64 or tuple(c.shape) != (cap + 1, 8) or not c.is_contiguous() or c.data_ptr() & 15:
                raise ValueError(f"comps[{i}] must be a contiguous, 16-byte aligned int64 tensor of shape ({cap + 1}, 8)")
            if t.device.type != "cuda" or c.device.type != "cuda":
                raise ValueError(f"labels[{i}] / comps[{i}] are not on a GPU")
        pb = [self.pic_bytes(s) for s in sids]
        uniform = len({self._geometry(s) for s in set(sids)}) <= 1
        out, device, where = Context._slot_outputs(out, pb, uniform, "geometries")
        if not n:
            return out
        a_s, _a_o, stream = Context._launch_args(device, sids, ())
        from ._lib import HvqSelect
        a_e = (HvqSelect * len(table))(*[e.struct() for e in table])
        a_w = Context._which_array(which, n)
        a_l = Context._ptr_array([t.data_ptr() for t in labels])
        a_c = Context._ptr_array([t.data_ptr() for t in comps])
        a_d = C.c_void_p(where.ctypes.data)                                  # void *[n]
        check(lib().hvq_select_components(self._h, n, a_s, a_l, a_c, cap, C.cast(a_e, C.c_void_p), len(table), a_w, a_d, stream))
        return out

    @staticmethod
    def _explicit_table(entries, which, n, cls, most, nouns):
        """a list of distinct `cls` together with `which`, one index per picture -> (table, which) after their checks"""
        table = [entries] if isinstance(entries, cls) else list(entries or ())
        if not table or len(table) > most:
            raise ValueError(f"{len(table)} {nouns}: one call takes 1 .. {most}")
        which = [int(k) for k in which]
        if len(which) != n or any(not 0 <= k < len(table) for k in which):
            raise ValueError(f"which: {n} indices into the {len(table)} {nouns}")
        return table, which

    def distance_pictures(self, sids, ordinals, rules=None, which=None, src=None, out=None):
        """hvq_distance_pictures: the exact distance transform of one plane of the resident pictures (sids[i], ordinals[i]) -- which
        samples are foreground, the metric, the border rule and the values are include/hvqm4_amd.h's --, on torch's current stream,
        without a host synchronisation and without moving a picture.  `rules`: one hvqm4_amd.distance.Rule (default distance.rule():
        the 255s of Y, squared Euclidean, nothing outside the plane: an Otsu mask), a list of one per picture (equal ones share an
        entry; more than 64 distinct ones: ValueError), or a list of distinct rules together with `which`, one index per picture.
        -> a list of n CUDA tensors int32 [Ny, Nx] of the rule's plane, viewed from the uint32 memory: 0 on the background, the distance
        on the foreground, and distance.NONE (no background at all) reads as -1.  `out`, if given: such a list, contiguous, 16-byte
        aligned.  hvqm4_amd.distance gives the expected values (of_picture) and reads a map (max_inscribed, signed).  `src` as in
        picture_checksums.  Ordering and slot safety are export()'s."""
        import torch
        from . import distance as ds
        n = Context._pictures(self._geom, sids, ordinals, limit=True)
        if which is not None:
            table, which = Context._explicit_table(rules, which, n, ds.Rule, ds.MAX_RULES, "rules")
        else:
            table, which = Context._table_which(ds.Rule() if rules is None else rules, n, ds.Rule, "rules", "distance.Rule", ds.MAX_RULES, "rules")
        for r in table:
            ds.check(r)
        from .checksums import sources
        ptrs = sources(src, ordinals, lambda i: self.pic_bytes(sids[i]))
        shapes = [ds.plane_shape(self._geometry(sids[i]), table[which[i] if which else 0].plane) for i in range(n)]
        if out is None:
            out = [torch.empty(shapes[i], dtype=torch.int32, device="cuda") for i in range(n)]
        else:
            def one(i, t):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != tuple(shapes[i]) or not t.is_contiguous():
                    raise ValueError(f"out[{i}] must be a contiguous int32 tensor of shape {tuple(shapes[i])}")
                if t.data_ptr() & 15:
                    raise ValueError(f"out[{i}]: pointer {t.data_ptr():#x} must be a multiple of 16")
            out = Context._out_list(out, n, one)
        if not n:
            return out
        a_s, a_o, stream = Context._launch_args(out[0].device, sids, ordinals)
        from ._lib import HvqDistanceRule
        a_r = (HvqDistanceRule * len(table))(*[r.struct() for r in table])
        a_w = Context._which_array(which, n)
        a_d = Context._ptr_array([t.data_ptr() for t in out])
        check(lib().hvq_distance_pictures(self._h, n, a_s, a_o, Context._ptr_array(ptrs), C.cast(a_r, C.c_void_p), len(table), a_w, a_d, stream))
        return out

    def distance_mask(self, sids, dist, mask, which=None, out=None):
        """hvq_distance_mask: distance maps of the Y planes (distance_pictures' results under a rule with plane 0) back into uint8
        pictures IN SLOT LAYOUT of the geometries of sids[i]: under a distance.mask_range(lo, hi) Y 255 where lo <= d <= hi, else 0
        (invert swaps the two), under distance.mask_root() Y min(255, isqrt(d)); U and V 128.  `mask`: one hvqm4_amd.distance.Mask, a
        list of one per picture, or a list of distinct ones together with `which`.  The maps are read when the work runs on torch's
        current stream: distance -> mask needs no host synchronisation.  Return forms and `out` are rank_pictures'; whatever takes
        src= takes a row of the result.  hvqm4_amd.distance.of_mask gives the expected bytes."""
        import torch
        from . import distance as ds
        n = Context._pictures(self._geom, sids, [0] * len(sids), limit=True)
        if which is not None:
            table, which = Context._explicit_table(mask, which, n, ds.Mask, ds.MAX_MASKS, "masks")
        else:
            table, which = Context._table_which(mask, n, ds.Mask, "mask", "distance.Mask", ds.MAX_MASKS, "masks")
        for e in table:
            ds.check_mask(e)
        if not isinstance(dist, (list, tuple)) or len(dist) != n:
            raise ValueError(f"dist must be a list of {n} tensors")
        for i in range(n):
            w, h = self._geometry(sids[i])[:2]
            t = dist[i]
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (h, w) or not t.is_contiguous() or t.data_ptr() & 15:
                raise ValueError(f"dist[{i}] must be a contiguous, 16-byte aligned int32 tensor of shape ({h}, {w})")
            if t.device.type != "cuda":
                raise ValueError(f"dist[{i}] is not on a GPU")
        pb = [self.pic_bytes(s) for s in sids]
        uniform = len({self._geometry(s) for s in set(sids)}) <= 1
        out, device, where = Context._slot_outputs(out, pb, uniform, "geometries")
        if not n:
            return out
        a_s, _a_o, stream = Context._launch_args(device, sids, ())
        from ._lib import HvqDistanceMask
        a_e = (HvqDistanceMask * len(table))(*[e.struct() for e in table])
        a_w = Context._which_array(which, n)
        a_l = Context._ptr_array([t.data_ptr() for t in dist])
        a_d = C.c_void_p(where.ctypes.data)                                  # void *[n]
        check(lib().hvq_distance_mask(self._h, n, a_s, a_l, C.cast(a_e, C.c_void_p), len(table), a_w, a_d, stream))
        return out

    def disc_morph(self, sids, ordinals, steps, src=None, out=None):
        """resident pictures (sids[i], ordinals[i]) through a list of disc steps (hvqm4_amd.distance.erode_disc / dilate_disc /
        opening_disc / closing_disc: (Rule, Mask) pairs of any radius), a distance_pictures and a distance_mask a step on torch's
        current stream: the first from the resident pictures (or `src`, a mask of map_pictures, say), every later one from the result
        before it through src=.  All steps share one list of maps; the results between them alternate between two scratch tensors of the
        output's form; the last lands in `out` (rank_pictures' rules; default: a new one).  No host synchronisation.  -> rank_pictures'
        return forms.  hvqm4_amd.distance.of_steps gives the expected bytes."""
        from . import distance as ds
        steps = ds.as_steps(steps)
        n = len(sids)
        maps = cur = spare = None
        for k, (r, m) in enumerate(steps):
            if cur is None:
                maps = self.distance_pictures(sids, ordinals, r, src=src, out=maps)
            else:
                maps = self.distance_pictures(sids, [-1] * n, r, src=[cur[i] for i in range(n)], out=maps)
            res = self.distance_mask(sids, maps, m, out=out if k == len(steps) - 1 else spare)
            spare, cur = cur, res
        return cur

    @staticmethod
    def _tables(given, name, n, shapes, dtype, optional=False):
        """the caller's list of n tables (int32 [Ny, Nx] of S, viewed from the uint32 memory, or int64 of Q), contiguous and 16-byte
        aligned, on a GPU; optional: an entry may be None -> their addresses (0 for None)"""
        import torch
        if not isinstance(given, (list, tuple)) or len(given) != n:
            raise ValueError(f"{name} must be a list of {n} tensors")
        for i, t in enumerate(given):
            if t is None and optional:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shapes[i]) or not t.is_contiguous() or t.data_ptr() & 15:
                raise ValueError(f"{name}[{i}] must be a contiguous, 16-byte aligned {str(dtype).replace('torch.', '')} tensor of shape {tuple(shapes[i])}")
            if t.device.type != "cuda":
                raise ValueError(f"{name}[{i}] is not on a GPU")
        return [0 if t is None else t.data_ptr() for t in given]

    def integral_pictures(self, sids, ordinals, planes=0, squares=True, src=None, out=None):
        """hvq_integral_pictures: the inclusive summed-area tables of one plane of the resident pictures (sids[i], ordinals[i]) -- the
        values are include/hvqm4_amd.h's --, on torch's current stream, without a host synchronisation and without moving a picture.
        `planes`: 0 Y, 1 U, 2 V, one for all or a list of one per picture.  -> (sums, squares): lists of n CUDA tensors, sums[i] int32
        [Ny, Nx] viewed from the uint32 memory (modulo 2^32: a rectangle of at most 2^24 samples comes out exact from the wrapped
        corners), squares[i] int64 [Ny, Nx]; `squares` False: no tables of squares, the second list is None.  `out`, if given: such a
        pair of lists (the second None without squares), contiguous, 16-byte aligned.  hvqm4_amd.integral gives the expected values
        (of_plane), the padded view and the sum of a rectangle.  `src` as in picture_checksums.  Ordering and slot safety are
        export()'s."""
        import torch
        from .labels import plane_shape
        n = Context._pictures(self._geom, sids, ordinals, limit=True)
        planes = [planes] * n if isinstance(planes, int) and not isinstance(planes, bool) else [int(p) for p in planes]
        if len(planes) != n or any(not 0 <= p <= 2 for p in planes):
            raise ValueError(f"planes: 0 Y, 1 U, 2 V, one for all or {n} of them")
        from .checksums import sources
        ptrs = sources(src, ordinals, lambda i: self.pic_bytes(sids[i]))
        shapes = [plane_shape(self._geometry(sids[i]), planes[i]) for i in range(n)]
        if out is None:
            sums = [torch.empty(shapes[i], dtype=torch.int32, device="cuda") for i in range(n)]
            sq = [torch.empty(shapes[i], dtype=torch.int64, device="cuda") for i in range(n)] if squares else None
        else:
            if not isinstance(out, (list, tuple)) or len(out) != 2:
                raise ValueError("out must be a pair (sums, squares) of lists")
            sums, sq = list(out[0]), (list(out[1]) if squares else None)
            if squares is False and out[1] is not None:
                raise ValueError("out: tables of squares without squares=True")
        p_s = Context._tables(sums, "sums", n, shapes, torch.int32)
        p_q = Context._tables(sq, "squares", n, shapes, torch.int64) if squares else None
        if not n:
            return sums, sq
        a_s, a_o, stream = Context._launch_args(sums[0].device, sids, ordinals)
        a_p = C.cast((C.c_int * n)(*planes), C.c_void_p)
        check(lib().hvq_integral_pictures(self._h, n, a_s, a_o, Context._ptr_array(ptrs), a_p, Context._ptr_array(p_s), Context._ptr_array(p_q), stream))
        return sums, sq

    def window_pictures(self, sids, ordinals, sums, squares, rules, which=None, src=None, out=None):
        """hvq_window_pictures: the tables of integral_pictures (of the rule's plane, which must have the size of Y) and the pictures
        (sids[i], ordinals[i]) back into uint8 pictures IN SLOT LAYOUT of the geometries of sids[i]: Y the local mean, the local
        deviation or the threshold of the rule over its window cut to the plane, U and V 128.  `rules`: one hvqm4_amd.integral.Rule
        (integral.mean / deviation / adaptive), a list of one per picture (equal ones share an entry; more than 64 distinct ones:
        ValueError), or a list of distinct ones together with `which`.  `squares`: None, or a list whose entries may be None, where no
        rule needs them.  The tables are read when the work runs on torch's current stream: integral -> window needs no host
        synchronisation.  Return forms and `out` are rank_pictures'; whatever takes src= takes a row of the result.
        hvqm4_amd.integral.of_picture gives the expected bytes.  `src` as in picture_checksums."""
        import torch
        from . import integral as ig
        n = Context._pictures(self._geom, sids, ordinals, limit=True)
        if which is not None:
            table, which = Context._explicit_table(rules, which, n, ig.Rule, ig.MAX_RULES, "rules")
        else:
            table, which = Context._table_which(rules, n, ig.Rule, "rules", "integral.Rule", ig.MAX_RULES, "rules")
        for r in table:
            ig.check(r)
        shapes = []
        for i in range(n):
            w, h = self._geometry(sids[i])[:2]
            shapes.append((h, w))
        p_s = Context._tables(sums, "sums", n, shapes, torch.int32)
        p_q = None if squares is None else Context._tables(squares, "squares", n, shapes, torch.int64, optional=True)
        ptrs, out, device, where = Context._slot_frame(self, sids, ordinals, src, out)
        if not n:
            return out
        a_s, a_o, stream = Context._launch_args(device, sids, ordinals)
        from ._lib import HvqWindowRule
        a_r = (HvqWindowRule * len(table))(*[r.struct() for r in table])
        a_w = Context._which_array(which, n)
        a_d = C.c_void_p(where.ctypes.data)                                  # void *[n]
        check(lib().hvq_window_pictures(self._h, n, a_s, a_o, Context._ptr_array(ptrs), Context._ptr_array(p_s), Context._ptr_array(p_q), C.cast(a_r, C.c_void_p),
                                        len(table), a_w, a_d, stream))
        return out

    def rect_sums(self, rects, sums, squares=None, dims=None, out=None):
        """hvq_rect_sums: `rects`, a CUDA tensor int32 [nrects, 5] = (i, x0, y0, x1, y1) with inclusive corners (integral.rects_of_boxes
        makes them of label_pictures' records on the device), against the tables of integral_pictures -> a CUDA tensor int64 [nrects,
        3] = (count, S, Q), Q 0 where picture i has no table of squares; (0, 0, 0) for a rectangle that leaves its plane, is empty,
        holds more than 2^24 samples or names no picture.  `dims`: a CUDA tensor int32 [n, 2] = (Nx, Ny); default: of the tables' shapes,
        uploaded by this call (a caller that repeats the call keeps the tensor).  On torch's current stream, no host synchronisation.  hvqm4_amd.integral.of_rects gives the expected values."""
        import torch
        n = len(sums)
        if not 1 <= n <= 65535:
            raise ValueError(f"{n} pictures: one call takes 1 .. 65535")
        if not isinstance(rects, torch.Tensor) or rects.dtype != torch.int32 or rects.dim() != 2 or rects.shape[1] != 5 or not rects.is_contiguous() or rects.device.type != "cuda":
            raise ValueError("rects must be a contiguous int32 CUDA tensor of shape (nrects, 5)")
        nrects = int(rects.shape[0])
        shapes = [tuple(t.shape) if isinstance(t, torch.Tensor) else () for t in sums]
        p_s = Context._tables(sums, "sums", n, shapes, torch.int32)
        p_q = None if squares is None else Context._tables(squares, "squares", n, shapes, torch.int64, optional=True)
        if dims is None:
            dims = torch.tensor([[s[1], s[0]] for s in shapes], dtype=torch.int32).to(rects.device, non_blocking=False)
        elif not isinstance(dims, torch.Tensor) or dims.dtype != torch.int32 or tuple(dims.shape) != (n, 2) or not dims.is_contiguous() or dims.device.type != "cuda":
            raise ValueError(f"dims must be a contiguous int32 CUDA tensor of shape ({n}, 2)")
        out = Context._out_tensor(out, (nrects, 3), torch.int64, name="out", align=8)
        if not nrects:
            return out
        _a_s, _a_o, stream = Context._launch_args(rects.device, (), ())
        check(lib().hvq_rect_sums(self._h, n, nrects, C.c_void_p(rects.data_ptr()), Context._ptr_array(p_s), Context._ptr_array(p_q), C.c_void_p(dims.data_ptr()),
                                  C.c_void_p(out.data_ptr()), stream))
        return out

    def adaptive_pictures(self, sids, ordinals, rules, which=None, src=None, out=None):
        """resident pictures (sids[i], ordinals[i]) through integral_pictures and window_pictures on torch's current stream, the tables
        in scratch tensors that torch's allocator takes back behind the stream's work: local thresholds (integral.adaptive), means
        and deviations with no host synchronisation.  Tables of squares are made only where a rule needs them.  `rules`, `which`, `src`
        and `out` are window_pictures'.  hvqm4_amd.integral.of_picture gives the expected bytes."""
        from . import integral as ig
        n = len(sids)
        flat = [rules] if isinstance(rules, ig.Rule) else list(rules or ())
        for r in flat:
            ig.check(r)
        per = [flat[which[i]] for i in range(n)] if which is not None else (flat * n if isinstance(rules, ig.Rule) else flat)
        if len(per) != n:
            raise ValueError(f"rules: one integral.Rule, or a list of {n}, or a list of distinct ones together with which")
        sums, squares = self.integral_pictures(sids, ordinals, [r.plane for r in per], squares=any(ig.needs_squares(r) for r in per), src=src)
        return self.window_pictures(sids, ordinals, sums, squares, rules, which=which, src=src, out=out)

    def warp_force_direct(self, on) -> int:
        """hvq_warp_force_direct: every later warp_pictures of this context takes the direct body of the kernel (False / 0: the chosen
        one again; 2: the tiled one wherever LDS holds the box, for the measurement that sets the rule) -> the setting before.  The
        values do not depend on it: for tests that compare the bodies with =="""
        return check(lib().hvq_warp_force_direct(self._h, int(on)))

    def warp_pictures(self, sids, ordinals, warp, size=None, sampling=None, src=None, out=None):
        """hvq_warp_pictures: resident pictures (sids[i], ordinals[i]) through a per-picture affine map with bilinear taps (exact
        integers, one rounding: include/hvqm4_amd.h) into uint8 pictures of a target geometry IN SLOT LAYOUT (Y | U | V), on torch's
        current stream, without a host synchronisation and without moving a picture.  `warp`: one hvqm4_amd.warp.Warp, or a list of
        one per picture; `size`: None (the source's), (w, h), or one per picture (None entries: the source's); `sampling`: likewise
        with (h_samp, v_samp).  -> when every target geometry is the same one uint8 CUDA tensor [n, bytes], otherwise a list of n 1-D
        uint8 CUDA tensors (`out`, if given: of that same form, contiguous, rows 16-byte aligned; it is overwritten whole and must
        not overlap a source).  Whatever takes src= or ref.ptr takes a row of the result, with an open stream of the target geometry
        to carry it.  hvqm4_amd.warp builds the maps and gives the expected bytes (of_picture).  `src` as in picture_checksums.
        Ordering and slot safety are export()'s."""
        from . import scale as sc
        from . import warp as wp
        from .checksums import sources
        n = Context._pictures(self._geom, sids, ordinals, limit=True)
        streams = set(sids)
        if isinstance(warp, wp.Warp):
            warps = None                                                   # one map for all: one row, broadcast
            wp.check(warp)
        else:
            if not isinstance(warp, (list, tuple)) or len(warp) != n:
                raise ValueError(f"warp: one warp.Warp, or a list of {n}")
            warps = list(warp)
            for w in {id(w): w for w in warps}.values():
                wp.check(w)                                                # ValueError beyond the library's limits
        sizes, one_size = sc.per_picture(size, n, 2, "size")
        samplings, one_sampling = sc.per_picture(sampling, n, 2, "sampling")
        def shape(g, sz, sm):
            dst = (sz or g[:2]) + (sm or g[2:])
            if dst[2:] not in sc.SAMPLINGS:
                raise ValueError(f"sampling {dst[2:]}: one of {sc.SAMPLINGS}")
            if dst[0] < 8 or dst[1] < 8 or dst[0] % 8 or dst[1] % 8 or dst[0] > 8192 or dst[1] > 8192:
                raise ValueError(f"target {dst[0]}x{dst[1]}: multiples of 8 up to 8192")
            return dst, sc.nbytes(*dst)
        geoms = {s: self._geometry(s) for s in streams}
        shapes, column = Context._target_shapes(geoms, sids, (sizes, samplings), one_size and one_sampling, shape)
        pb = {s: self.pic_bytes(s) for s in streams}
        ptrs = sources(src, ordinals, lambda i: pb[sids[i]])
        uniform = len({v[0] for v in shapes.values()}) <= 1
        out, device, where = Context._slot_outputs(out, column(1), uniform, "target geometries")
        if not n:
            return out
        a_s, a_o, stream = Context._launch_args(device, sids, ordinals)
        a_w = np.empty(n, dtype=_WARP)                                       # HvqWarp[n]
        a_w["m"] = warp.coefficients() + (warp.border,) if warps is None else [w.coefficients() + (w.border,) for w in warps]
        a_w["fill"] = warp.fill + (0,) if warps is None else [w.fill + (0,) for w in warps]
        a_d = np.empty(n, dtype=_WARP_DST)                                   # HvqWarpDst[n]
        a_d["ptr"] = where
        a_d["rest"] = column(0, broadcast=True)
        check(lib().hvq_warp_pictures(self._h, n, a_s, a_o, Context._ptr_array(ptrs), C.c_void_p(a_w.ctypes.data), C.c_void_p(a_d.ctypes.data), stream))
        return out

    def compose_force_general(self, on: bool) -> bool:
        """hvq_compose_force_general: every later compose_pictures of this context takes the general body of the kernel for every
        layer (False: the chosen one again) -> the setting before.  The values do not depend on it: for tests that compare the two
        with =="""
        return bool(check(lib().hvq_compose_force_general(self._h, int(bool(on)))))

    def compose_pictures(self, sids, ordinals, targets, src=None, out=None):
        """hvq_compose_pictures: pictures built from layers of the resident pictures (sids[i], ordinals[i]) -- the call's flat list,
        which compose.Layer.source indexes; a picture that several layers use stands in it once -- with exact integers and one rounding
        (include/hvqm4_amd.h), IN SLOT LAYOUT (Y | U | V), on torch's current stream, without a host synchronisation and without
        moving a picture.  `targets`: a list of hvqm4_amd.compose.Target.  -> when every target geometry is the same one uint8 CUDA
        tensor [len(targets), bytes], otherwise a list of 1-D uint8 CUDA tensors (`out`, if given: of that same form, contiguous,
        rows 16-byte aligned; it is overwritten whole and must not overlap a source).  Whatever takes src= or ref.ptr takes a row of
        the result, with an open stream of the target geometry to carry it.  hvqm4_amd.compose builds the targets and gives the
        expected bytes (of_pictures).  `src` as in picture_checksums.  Ordering and slot safety are export()'s."""
        from . import compose as cp
        from . import scale as sc
        from .checksums import sources
        n = Context._pictures(self._geom, sids, ordinals)
        if not isinstance(targets, (list, tuple)):
            raise ValueError("targets: a list of compose.Target")
        nt = len(targets)
        if nt > 65535:
            raise ValueError(f"{nt} targets: one call takes 65535 at the most")
        by_stream = {s: self._geometry(s) for s in set(sids)}
        geoms = [by_stream[s] for s in sids]
        source, nums, rows = cp.check_call(targets, geoms)                  # ValueError beyond the library's limits
        nl = len(source)
        if nl > cp.MAX_TOTAL:
            raise ValueError(f"{nl} layers: one call takes {cp.MAX_TOTAL} at the most")
        pb = {s: self.pic_bytes(s) for s in by_stream}
        ptrs = sources(src, ordinals, lambda i: pb[sids[i]])
        dst_geoms = [tuple(r) for r in rows[:, :4].tolist()]
        uniform = len(set(dst_geoms)) <= 1
        nb = [sc.nbytes(*dst_geoms[0])] * nt if uniform and nt else [sc.nbytes(*g) for g in dst_geoms]
        out, device, where = Context._slot_outputs(out, nb, uniform, "target geometries")
        if not nt:
            return out
        _s, _o, stream = Context._launch_args(device, (), ())
        # the call's flat arrays: layer l reads picture source[l] of the method's list
        a_s = np.ascontiguousarray(np.asarray(sids, dtype=np.int32).reshape(n)[source])
        a_o = np.ascontiguousarray(np.asarray(ordinals, dtype=np.int32).reshape(n)[source])
        a_p = None if ptrs is None else np.ascontiguousarray(np.array([p or 0 for p in ptrs], dtype=np.uint64).reshape(n)[source])
        a_l = np.ascontiguousarray(nums)                                     # HvqComposeLayer[nlayers]
        a_d = np.empty(nt, dtype=_COMPOSE_DST)                               # HvqComposeDst[ntargets]
        a_d["ptr"] = where
        a_d["rest"] = rows
        as_int = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        check(lib().hvq_compose_pictures(self._h, nl, as_int(a_s), as_int(a_o), None if a_p is None else C.c_void_p(a_p.ctypes.data),
                                         C.c_void_p(a_l.ctypes.data), nt, C.c_void_p(a_d.ctypes.data), stream))
        return out

    def _ssim_dims(self, sid):
        """((rows, cols) of the SSIM windows of Y, U, V) of a stream: hvq_ssim_windows on its geometry"""
        from .metrics import ssim_windows
        w, h = self._geom[sid][:2]
        y = w * h
        c = (self.pic_bytes(sid) - y) // 2
        hs, vs = {y // 4: (2, 2), y // 2: (2, 1), y: (1, 1)}[c]
        return ssim_windows(w, h, hs, vs)

    def rgb_bench(self, reps: int):
        """-> (gpu_ms, bytes_per_rep, pictures): batched display epilogue over the newest picture of every stream"""
        ms, by, n = C.c_float(0), C.c_uint64(0), C.c_uint32(0)
        check(lib().hvq_rgb_bench(self._h, reps, C.byref(ms), C.byref(by), C.byref(n)))
        return float(ms.value), int(by.value), int(n.value)

    def h2d_probe(self, nbytes: int, reps: int = 8) -> float:
        """GB/s of pinned-host -> device copies of `nbytes` on the copy stream (the PCIe bound of streaming from host memory)"""
        g = C.c_double(0)
        check(lib().hvq_h2d_probe(self._h, int(nbytes), int(reps), C.byref(g)))
        return float(g.value)

    def stats(self) -> HvqStats:
        st = HvqStats()
        check(lib().hvq_get_stats(self._h, C.byref(st)))
        return st

    def close(self):
        if self._h:
            lib().hvq_context_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decode_clip(ctx: Context, data: bytes, nslots: Optional[int] = None, gpu_parse: bool = False,
                flush_every: Optional[int] = None) -> np.ndarray:
    """Decode a whole .h4m through the batched path; returns uint8[n_pictures, pic_bytes] (decode order).
    gpu_parse: entropy-parse on the GPU (hvq_submit_many_device); flush_every: flush after that many pictures."""
    from .container import parse_header, video_pictures
    hdr = parse_header(data)
    pics = list(video_pictures(data))
    sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15,
                          nslots if nslots is not None else len(pics) + 3)
    step = flush_every or len(pics)
    for at in range(0, len(pics), step):
        part = pics[at:at + step]
        if gpu_parse:
            ctx.submit_many_device([sid] * len(part), [ft for ft, _d, _p in part], [bytes(p) for _f, _d, p in part])
        else:
            for ft, _disp, pic in part:
                ctx.submit(sid, ft, pic)
        ctx.flush()
    out = np.stack([ctx.read_picture(sid, i) for i in range(len(pics))])
    ctx.close_stream(sid)
    return out


class PairedContexts:
    """The streaming subset of Context over TWO contexts of one GPU, driven by one thread: streams are dealt to the contexts in turn, a
    submit splits its pictures by their stream's context, flush_next() advances context A, then context B.  While the call waits for
    one context's parse results the other context's kernels run, and the two half-size parse kernels stay out of phase (one context's
    pictures in the scalar chains while the other's are in the all-thread passes or being reconstructed): 169-173 Gpixel/s against
    158-160 for the same 128 dense streams in one context (profiles/r05_flush_next.txt 6; INTEGRATION.md "Two contexts per GPU" is the
    same recipe in C).  Stream ids are the pair's own."""

    def __init__(self, device: int = 0):
        self._ctx = [Context(device), Context(device)]
        for c in self._ctx:
            c.set_launch_queues(1)                         # the two contexts are each other's second queue
        self._where = []                                   # pair stream id -> (context index, stream id inside it)

    def open_stream(self, width: int, height: int, h_samp: int = 2, v_samp: int = 2, is15: bool = True, nslots: int = 4) -> int:
        k = len(self._where) & 1
        self._where.append((k, self._ctx[k].open_stream(width, height, h_samp, v_samp, is15, nslots)))
        return len(self._where) - 1

    def submit_many_device(self, sids, frame_types, pictures, defer: bool = False):
        """as Context.submit_many_device; the returned ordinals are per stream, as there"""
        part = ([], [], [], []), ([], [], [], [])
        for i, sid in enumerate(sids):
            k, inner = self._where[sid]
            part[k][0].append(inner); part[k][1].append(frame_types[i]); part[k][2].append(pictures[i]); part[k][3].append(i)
        ords = [0] * len(sids)
        for k in (0, 1):
            if part[k][0]:
                for i, o in zip(part[k][3], self._ctx[k].submit_many_device(part[k][0], part[k][1], part[k][2], defer=defer)):
                    ords[i] = o
        return ords

    def flush_begin(self) -> None:
        for c in self._ctx:
            c.flush_begin()

    def flush_next(self) -> None:
        for c in self._ctx:
            c.flush_next()

    def flush_end(self) -> None:
        for c in self._ctx:
            c.flush_end()

    def flush(self) -> None:
        self.flush_begin()
        self.flush_end()

    def sync(self) -> None:
        for c in self._ctx:
            c.sync()

    def read_picture(self, sid: int, ordinal: int) -> np.ndarray:
        k, inner = self._where[sid]
        return self._ctx[k].read_picture(inner, ordinal)

    def stats(self):
        return [c.stats() for c in self._ctx]

    def close(self) -> None:
        for c in self._ctx:
            c.close()

