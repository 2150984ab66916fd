"""Loader for the product's C-ABI library (hvqm4_amd/libhvqm4_amd.so).

The library is the product: HIP kernels + host parse + runtime.  It is built in-tree by
`make -C hvqm4_amd/csrc` (or `__graft_entry__.build()`); importing this module with the
library missing is an error -- there is no Python or CPU fallback for the pixel path.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HVQM4_AMD_LIB") or os.path.join(HERE, "libhvqm4_amd.so")   # override: ablation builds only

HVQ_OK, HVQ_E_ARG, HVQ_E_OVERFLOW, HVQ_E_GEOMETRY, HVQ_E_NOGPU, HVQ_E_HIP, HVQ_E_STATE, HVQ_E_CONTAINER = 0, -1, -2, -3, -4, -5, -6, -7
HVQ_E_UNSUPPORTED = -8
ERROR_NAMES = {HVQ_E_ARG: "HVQ_E_ARG", HVQ_E_OVERFLOW: "HVQ_E_OVERFLOW", HVQ_E_GEOMETRY: "HVQ_E_GEOMETRY",
               HVQ_E_NOGPU: "HVQ_E_NOGPU", HVQ_E_HIP: "HVQ_E_HIP", HVQ_E_STATE: "HVQ_E_STATE",
               HVQ_E_CONTAINER: "HVQ_E_CONTAINER", HVQ_E_UNSUPPORTED: "HVQ_E_UNSUPPORTED"}

HVQM4_VIDEOSTATE_SIZE = 28120
HVQM4_VIDEOSTATE_PADDING = 28097


class HvqError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERROR_NAMES.get(code, code)}: {msg}")
        self.code = code


class VideoState(C.Structure):
    _fields_ = [("opaque0", C.c_uint8 * HVQM4_VIDEOSTATE_PADDING),
                ("padding", C.c_uint8 * 3),
                ("opaque1", C.c_uint8 * (HVQM4_VIDEOSTATE_SIZE - HVQM4_VIDEOSTATE_PADDING - 3))]


class SeqObj(C.Structure):                       # h4m_audio_decode.c:516-523
    _fields_ = [("state", C.POINTER(VideoState)), ("width", C.c_uint16), ("height", C.c_uint16),
                ("h_samp", C.c_uint8), ("v_samp", C.c_uint8)]


class VideoInfo(C.Structure):                    # h4m_audio_decode.c:533-540
    _fields_ = [("hres", C.c_uint16), ("vres", C.c_uint16), ("h_samp", C.c_uint8), ("v_samp", C.c_uint8),
                ("video_mode", C.c_uint8)]


class HvqH4mInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("header_size", "body_size", "blocks", "video_frames", "audio_frames",
                                          "usec_per_frame", "max_frame_size", "pic_bytes")] + \
               [("width", C.c_uint16), ("height", C.c_uint16), ("h_samp", C.c_uint8), ("v_samp", C.c_uint8),
                ("video_mode", C.c_uint8), ("is_1_5", C.c_uint8)]


class HvqH4mIter(C.Structure):
    _fields_ = [("pos", C.c_size_t), ("block_end", C.c_size_t)] + \
               [(n, C.c_uint32) for n in ("block", "v_left", "a_left", "video_seen", "gop_start", "in_block")]


class HvqStats(C.Structure):
    _fields_ = [("pictures", C.c_uint64), ("luma_pixels", C.c_uint64), ("algorithmic_bytes", C.c_uint64),
                ("descriptor_bytes", C.c_uint64), ("launches", C.c_uint32), ("workgroups", C.c_uint32),
                ("parse_seconds", C.c_double), ("flags_or", C.c_uint32), ("gpu_parsed", C.c_uint32),
                ("gpu_parse_ms", C.c_double), ("gpu_parse_retried", C.c_uint32), ("dropped", C.c_uint32),
                ("launch_queues", C.c_uint32), ("queue_bytes", C.c_uint64), ("copy_bytes", C.c_uint64), ("copy_seconds", C.c_double)]


class HvqScaleDst(C.Structure):                 # include/hvqm4_amd.h: a destination of hvq_scale_pictures
    _fields_ = [("ptr", C.c_void_p)] + [(n, C.c_int32) for n in ("width", "height", "h_samp", "v_samp", "crop_x", "crop_y", "crop_w", "crop_h")]


class HvqFilterTerm(C.Structure):               # include/hvqm4_amd.h: one separable kernel of a plane's filter
    _fields_ = [("rx", C.c_int32), ("ry", C.c_int32), ("wx", C.c_int16 * 31), ("wy", C.c_int16 * 31)]


class HvqPlaneFilter(C.Structure):
    _fields_ = [("terms", C.c_int32), ("combine", C.c_int32), ("shift", C.c_int32), ("bias", C.c_int32), ("term", HvqFilterTerm * 2)]


class HvqFilter(C.Structure):                   # a filter of hvq_filter_pictures: luma for Y, chroma for U and V
    _fields_ = [("luma", HvqPlaneFilter), ("chroma", HvqPlaneFilter)]


class HvqRankPlane(C.Structure):                # include/hvqm4_amd.h: a plane's rank operation (HVQ_RNK_*) and its radii
    _fields_ = [("op", C.c_int32), ("rx", C.c_int32), ("ry", C.c_int32), ("pad", C.c_int32)]


class HvqRank(C.Structure):                     # an entry of hvq_rank_pictures: luma for Y, chroma for U and V
    _fields_ = [("luma", HvqRankPlane), ("chroma", HvqRankPlane)]


class HvqBilateralPlane(C.Structure):           # include/hvqm4_amd.h: a plane's radii, its spatial table [|j|][|i|] and its range table
    _fields_ = [("rx", C.c_int32), ("ry", C.c_int32), ("pad", C.c_int32 * 2), ("spatial", (C.c_uint8 * 8) * 8), ("range", C.c_uint8 * 256)]


class HvqBilateral(C.Structure):                # an entry of hvq_bilateral_pictures: luma for Y, chroma for U and V
    _fields_ = [("luma", HvqBilateralPlane), ("chroma", HvqBilateralPlane)]


class HvqTablePlane(C.Structure):               # include/hvqm4_amd.h: a plane's table kind (HVQ_TBL_*) and its parameters
    _fields_ = [("kind", C.c_int32), ("a", C.c_int32), ("b", C.c_int32), ("pad", C.c_int32)]


class HvqTableRule(C.Structure):                # an entry of hvq_histogram_tables: luma for Y, chroma for U and V
    _fields_ = [("luma", HvqTablePlane), ("chroma", HvqTablePlane)]


class HvqLabelRule(C.Structure):               # include/hvqm4_amd.h: the foreground window of a plane and the neighbourhood (4 or 8)
    _fields_ = [("plane", C.c_int32), ("lo", C.c_int32), ("hi", C.c_int32), ("connectivity", C.c_int32)]


class HvqCornerRule(C.Structure):              # include/hvqm4_amd.h: the plane, the measure (HVQ_CRN_*), the window radius, k, nms, margin, threshold
    _fields_ = [(n, C.c_int32) for n in ("plane", "mode", "radius", "k", "nms", "margin")] + [("pad", C.c_int32 * 2), ("threshold", C.c_int64)]


class HvqSelect(C.Structure):                   # an entry of hvq_select_components: inclusive ranges of area, box width and box height
    _fields_ = [(n, C.c_uint32) for n in ("area_min", "area_max", "w_min", "w_max", "h_min", "h_max", "invert", "pad")]


class HvqDistanceRule(C.Structure):            # include/hvqm4_amd.h: the foreground window of a plane, the metric (HVQ_DST_*) and the border rule
    _fields_ = [(n, C.c_int32) for n in ("plane", "lo", "hi", "metric", "border")] + [("pad", C.c_int32 * 3)]


class HvqDistanceMask(C.Structure):            # an entry of hvq_distance_mask: the mode (HVQ_DSM_*), an inclusive range of distances, invert
    _fields_ = [(n, C.c_uint32) for n in ("mode", "lo", "hi", "invert")] + [("pad", C.c_uint32 * 4)]


class HvqWindowRule(C.Structure):              # include/hvqm4_amd.h: an entry of hvq_window_pictures: the plane of the tables, the mode (HVQ_WIN_*), the radii, k, c, invert
    _fields_ = [(n, C.c_int32) for n in ("plane", "mode", "rx", "ry", "k", "c", "invert", "pad")]


class HvqWarp(C.Structure):                     # include/hvqm4_amd.h: the map of a picture of hvq_warp_pictures, Q16, target -> source
    _fields_ = [(n, C.c_int32) for n in ("m00", "m01", "m10", "m11", "t0", "t1", "border")] + [("fill", C.c_uint8 * 3), ("pad", C.c_uint8)]


class HvqWarpDst(C.Structure):                  # a destination of hvq_warp_pictures: HvqScaleDst without the crop
    _fields_ = [("ptr", C.c_void_p)] + [(n, C.c_int32) for n in ("width", "height", "h_samp", "v_samp")]


class HvqComposeLayer(C.Structure):             # include/hvqm4_amd.h: a layer of hvq_compose_pictures, luma samples
    _fields_ = [(n, C.c_int32) for n in ("mode", "sx", "sy", "w", "h", "dx", "dy")] + [("weight", C.c_int32 * 3)]


class HvqComposeDst(C.Structure):               # a target of hvq_compose_pictures: its geometry, its layers, the finish
    _fields_ = [("ptr", C.c_void_p)] + [(n, C.c_int32) for n in ("width", "height", "h_samp", "v_samp", "first", "count", "shift")] + [("bias", C.c_int32 * 3)]


# every symbol include/hvqm4.h and include/hvqm4_amd.h declare: (restype, argtypes)
SYMBOLS = {
    "HVQM4InitDecoder": (None, []),
    "HVQM4InitSeqObj": (None, [C.POINTER(SeqObj), C.POINTER(VideoInfo)]),
    "HVQM4BuffSize": (C.c_uint32, [C.POINTER(SeqObj)]),
    "HVQM4SetBuffer": (None, [C.POINTER(SeqObj), C.c_void_p]),
    "HVQM4DecodeIpic": (None, [C.POINTER(SeqObj), C.c_char_p, C.c_void_p]),
    "HVQM4DecodePpic": (None, [C.POINTER(SeqObj), C.c_char_p, C.c_void_p, C.c_void_p]),
    "HVQM4DecodeBpic": (None, [C.POINTER(SeqObj), C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "HVQM4GetLastError": (C.c_int, []),
    "HVQM4GetLastErrorString": (C.c_char_p, []),
    "HVQM4SetVersion15": (None, [C.POINTER(SeqObj), C.c_int]),
    "HVQM4ReleaseBuffer": (None, [C.POINTER(SeqObj)]),
    "HVQM4SetMaxFrameSize": (None, [C.POINTER(SeqObj), C.c_uint32]),
    "hvq_context_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "hvq_context_destroy": (None, [C.c_void_p]),
    "hvq_context_set_launch_queues": (C.c_int, [C.c_void_p, C.c_int]),
    "hvq_context_set_group_bytes": (C.c_int, [C.c_void_p, C.c_uint64]),
    "hvq_context_launch_groups": (C.c_int, [C.c_void_p]),
    "hvq_launch_group_default_bytes": (C.c_uint64, []),
    "hvq_launch_group_plan": (C.c_uint32, [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_int32),
                                           C.c_uint64, C.c_uint32, C.POINTER(C.c_uint16), C.POINTER(C.c_uint64)]),
    "hvq_stream_open": (C.c_int, [C.c_void_p] + [C.c_int] * 6),
    "hvq_stream_close": (C.c_int, [C.c_void_p, C.c_int]),
    "hvq_stream_ring_bytes": (C.c_uint64, [C.c_int] * 5),
    "hvq_stream_submit": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    "hvq_submit_many": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_char_p),
                                  C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_int)]),
    "hvq_submit_many_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_char_p),
                                         C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "hvq_submit_many_device_async": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_char_p),
                                               C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "hvq_arena_reserve": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "hvq_arena_stride": (C.c_size_t, [C.c_size_t]),
    "hvq_submit_many_arena": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t),
                                        C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "hvq_flush": (C.c_int, [C.c_void_p]),
    "hvq_flush_begin": (C.c_int, [C.c_void_p]),
    "hvq_flush_end": (C.c_int, [C.c_void_p]),
    "hvq_flush_next": (C.c_int, [C.c_void_p]),
    "hvq_sync": (C.c_int, [C.c_void_p]),
    "hvq_replay": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "hvq_replay_stage": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "hvq_read_picture": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "hvq_stream_pic_bytes": (C.c_uint32, [C.c_void_p, C.c_int]),
    "hvq_read_picture_rgb": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "hvq_rgb_bench": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "hvq_convert_yuv420_rgb": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "hvq_read_pictures": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    "hvq_stream_set_parse_threads": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "hvq_h2d_probe": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_double)]),
    "hvq_pinned_alloc": (C.c_void_p, [C.c_size_t]),
    "hvq_pinned_free": (None, [C.c_void_p]),
    "hvq_picture_device_ptr": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "hvq_export_pictures": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_void_p,
                                      C.c_void_p]),
    "hvq_export_tensors": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_float),
                                     C.POINTER(C.c_float), C.c_void_p, C.c_void_p]),
    "hvq_export_resampled": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int,
                                       C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_void_p]),
    "hvq_picture_metrics": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p]),
    "hvq_ssim_windows": (C.c_int, [C.c_int] * 4 + [C.c_void_p]),
    "hvq_picture_ssim": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "hvq_picture_checksums": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p]),
    "hvq_picture_histograms": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "hvq_motion_blocks": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "hvq_picture_motion": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p]),
    "hvq_jpeg_header": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "hvq_jpeg_bound": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "hvq_encode_jpeg": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "hvq_picture_hashes": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p]),
    "hvq_hash_nearest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p,
                                   C.c_void_p]),
    "hvq_scale_pictures": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p]),
    "hvq_scale_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "hvq_scale_body": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "hvq_scale_force_direct": (C.c_int, [C.c_void_p, C.c_int]),
    "hvq_filter_check": (C.c_int, [C.c_void_p]),
    "hvq_filter_pictures": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "hvq_filter_force_filter": (C.c_int, [C.c_void_p, C.c_int]),
    "hvq_rank_check": (C.c_int, [C.c_void_p]),
    "hvq_rank_pictures": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "hvq_rank_force_general": (C.c_int, [C.c_void_p, C.c_int]),
    "hvq_bilateral_check": (C.c_int, [C.c_void_p]),
    "hvq_bilateral_pictures": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "hvq_bilateral_force_general": (C.c_int, [C.c_void_p, C.c_int]),
    "hvq_map_pictures": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                   C.c_void_p]),
    "hvq_table_check": (C.c_int, [C.c_void_p]),
    "hvq_histogram_tables": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hvq_label_check": (C.c_int, [C.c_void_p]),
    "hvq_label_bytes": (C.c_int64, [C.c_int] * 5),
    "hvq_label_pictures": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int, C.c_void_p]),
    "hvq_select_components": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "hvq_corner_check": (C.c_int, [C.c_void_p]),
    "hvq_corner_rows_bytes": (C.c_int64, [C.c_int] * 5),
    "hvq_corner_response_bytes": (C.c_int64, [C.c_int] * 5),
    "hvq_corner_pictures": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "hvq_distance_check": (C.c_int, [C.c_void_p]),
    "hvq_distance_bytes": (C.c_int64, [C.c_int] * 5),
    "hvq_distance_pictures": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "hvq_distance_mask_check": (C.c_int, [C.c_void_p]),
    "hvq_distance_mask": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hvq_integral_bytes": (C.c_int64, [C.c_int] * 6),
    "hvq_integral_pictures": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hvq_window_check": (C.c_int, [C.c_void_p]),
    "hvq_window_pictures": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "hvq_rect_sums": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hvq_warp_check": (C.c_int, [C.c_void_p]),
    "hvq_warp_pictures": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hvq_warp_body": (C.c_int, [C.c_void_p] + [C.c_int] * 6),
    "hvq_warp_force_direct": (C.c_int, [C.c_void_p, C.c_int]),
    "hvq_compose_check": (C.c_int, [C.c_void_p]),
    "hvq_compose_pictures": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hvq_compose_force_general": (C.c_int, [C.c_void_p, C.c_int]),
    "hvq_crc32_combine": (C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint64]),
    "hvq_adler32_combine": (C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint64]),
    "hvq_resample_table": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_size_t,
                                     C.POINTER(C.c_size_t)]),
    "hvq_resample_tile_rows": (C.c_int, [C.c_int] * 4),
    "hvq_get_stats": (C.c_int, [C.c_void_p, C.POINTER(HvqStats)]),
    "hvq_debug_table_divisions": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "hvq_last_error_string": (C.c_char_p, []),
    "hvq_h4m_header": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(HvqH4mInfo)]),
    "hvq_h4m_begin": (None, [C.POINTER(HvqH4mIter)]),
    "hvq_h4m_next": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(HvqH4mIter), C.POINTER(C.c_int), C.POINTER(C.c_uint32),
                               C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "hvq_parser_create": (C.c_void_p, [C.c_int] * 5),
    "hvq_parser_destroy": (None, [C.c_void_p]),
    "hvq_parser_blob_bound": (C.c_size_t, [C.c_void_p]),
    "hvq_parser_pic_bytes": (C.c_uint32, [C.c_void_p]),
    "hvq_picture_length": (C.c_int, [C.c_char_p, C.c_int, C.c_uint32, C.POINTER(C.c_size_t)]),
    "hvq_parser_set_threads": (C.c_int, [C.c_void_p, C.c_int]),
    "hvq_parser_last_flags": (C.c_uint32, [C.c_void_p]),
    "hvq_parse_picture": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                    C.POINTER(C.c_size_t)]),
}

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `make -C hvqm4_amd/csrc` "
                "(hipcc --offload-arch=gfx950).  The HVQM4 reconstruction path is GPU-only; "
                "there is no CPU fallback.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            try:
                fn = getattr(l, name)
            except AttributeError:
                if not os.environ.get("HVQM4_AMD_LIB"):
                    raise                      # the product library must export every symbol the headers declare (tests/test_abi.py)
                continue                       # an older build named for an A/B experiment: it simply lacks the newer entry points
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc: int) -> int:
    if rc < 0:
        raise HvqError(rc, lib().hvq_last_error_string().decode(errors="replace"))
    return rc
