"""Device-resident batch encode/decode (charls_amd.h part 2) on torch tensors, plus frame sharding across ranks.

torch supplies HBM allocations, the current HIP stream and torch.distributed (backend "nccl" = RCCL over xGMI);
all coding work happens inside libcharls_amd.so.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import capi


class CodecParams(C.Structure):  # charls_amd_codec_params (include/charls_amd.h)
    _fields_ = [("frame_info", capi.FrameInfo), ("near_lossless", C.c_int32), ("interleave_mode", C.c_int32),
                ("color_transformation", C.c_int32), ("preset_coding_parameters", capi.PcParameters),
                ("encoding_options", C.c_uint32), ("restart_interval", C.c_uint32)]


class DeviceShard(C.Structure):  # charls_amd_device_shard
    _fields_ = [("device", C.c_int32), ("frame_count", C.c_uint32), ("d_frames", C.c_void_p), ("d_streams", C.c_void_p),
                ("hip_stream", C.c_void_p)]


class Gather(C.Structure):  # charls_amd_gather
    _fields_ = [("root_shard", C.c_uint32), ("d_gathered", C.c_void_p), ("capacity_bytes", C.c_size_t),
                ("offsets", C.POINTER(C.c_uint64)), ("total_bytes", C.POINTER(C.c_uint64)), ("transport", C.c_int32)]


class FrameSource(C.Structure):  # charls_amd_frame_source
    _fields_ = [("params", CodecParams), ("d_pixels", C.c_void_p), ("stride", C.c_uint32), ("reserved", C.c_uint32),
                ("max_stream_bytes", C.c_uint64)]


class FrameDest(C.Structure):  # charls_amd_frame_dest
    _fields_ = [("d_pixels", C.c_void_p), ("capacity_bytes", C.c_uint64), ("stride", C.c_uint32), ("reserved", C.c_uint32)]


TRANSPORT_AUTO, TRANSPORT_RCCL, TRANSPORT_PEER_COPIES = 0, 1, 2


def _bind(lib):
    l = lib.lib
    if getattr(l, "_batch_bound", False):
        return l
    l.charls_amd_encode_batch_device.argtypes = [C.POINTER(CodecParams), C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32,
                                                 C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_int32),
                                                 C.c_void_p]
    l.charls_amd_encode_batch_device.restype = C.c_int32
    l.charls_amd_decode_batch_device.argtypes = [C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64), C.c_void_p,
                                                 C.c_size_t, C.c_uint32, C.POINTER(CodecParams), C.POINTER(C.c_int32),
                                                 C.c_void_p]
    l.charls_amd_decode_batch_device.restype = C.c_int32
    l.charls_amd_last_timings.argtypes = [C.POINTER(C.c_double), C.c_int32]
    l.charls_amd_last_timings.restype = C.c_int32
    l.charls_amd_set_encode_engine.argtypes = [C.c_int32]
    l.charls_amd_set_encode_engine.restype = C.c_int32
    l.charls_amd_set_workspace_limit.argtypes = [C.c_uint64]
    l.charls_amd_set_workspace_limit.restype = C.c_int32
    l.charls_amd_release_work_areas.argtypes = []
    l.charls_amd_release_work_areas.restype = C.c_int32
    l.charls_amd_work_area_bytes.argtypes = []
    l.charls_amd_work_area_bytes.restype = C.c_uint64
    l.charls_amd_encode_batch_devices.argtypes = [C.POINTER(CodecParams), C.c_uint32, C.POINTER(DeviceShard), C.c_size_t,
                                                  C.c_uint32, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_int32),
                                                  C.POINTER(Gather)]
    l.charls_amd_encode_batch_devices.restype = C.c_int32
    l.charls_amd_decode_batch_devices.argtypes = [C.c_uint32, C.POINTER(DeviceShard), C.c_size_t, C.POINTER(C.c_uint64),
                                                  C.c_size_t, C.c_uint32, C.POINTER(CodecParams), C.POINTER(C.c_int32)]
    l.charls_amd_decode_batch_devices.restype = C.c_int32
    u64p, i32p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    l.charls_amd_index_size_bound.argtypes = [C.POINTER(CodecParams), C.c_uint32, C.POINTER(C.c_size_t)]
    l.charls_amd_index_size_bound.restype = C.c_int32
    l.charls_amd_decode_batch_device_and_index.argtypes = [C.c_uint32, C.c_void_p, C.c_size_t, u64p, C.c_void_p, C.c_size_t, C.c_uint32,
                                                           C.c_uint32, C.c_void_p, C.c_size_t, u64p, C.POINTER(CodecParams), i32p,
                                                           C.c_void_p]
    l.charls_amd_decode_batch_device_and_index.restype = C.c_int32
    l.charls_amd_decode_batch_device_indexed.argtypes = [C.c_uint32, C.c_void_p, C.c_size_t, u64p, C.c_void_p, C.c_size_t, u64p,
                                                         C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(CodecParams), i32p, C.c_void_p]
    l.charls_amd_decode_batch_device_indexed.restype = C.c_int32
    l.charls_amd_decode_rows_batch_device.argtypes = [C.c_uint32, C.c_void_p, C.c_size_t, u64p, C.c_void_p, C.c_size_t, u64p, u32p, u32p,
                                                      C.c_void_p, C.c_size_t, C.c_uint32, i32p, C.c_void_p]
    l.charls_amd_decode_rows_batch_device.restype = C.c_int32
    l.charls_amd_index_counters.argtypes = [u64p, C.c_int32]
    l.charls_amd_index_counters.restype = C.c_int32
    l.charls_amd_pack_streams_device.argtypes = [C.c_uint32, C.c_void_p, C.c_size_t, u64p, C.c_void_p, C.c_size_t, C.c_uint32, u64p,
                                                 C.c_void_p]
    l.charls_amd_pack_streams_device.restype = C.c_int32
    l.charls_amd_encode_batch_device_packed.argtypes = [C.POINTER(CodecParams), C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32,
                                                        C.c_void_p, C.c_size_t, C.c_uint32, C.c_size_t, u64p, u64p, i32p, C.c_void_p]
    l.charls_amd_encode_batch_device_packed.restype = C.c_int32
    l.charls_amd_decode_batch_device_packed.argtypes = [C.c_uint32, C.c_void_p, u64p, u64p, C.c_void_p, C.c_size_t, C.c_uint32,
                                                        C.POINTER(CodecParams), i32p, C.c_void_p]
    l.charls_amd_decode_batch_device_packed.restype = C.c_int32
    l.charls_amd_probe_batch_device_packed.argtypes = [C.c_uint32, C.c_void_p, u64p, u64p, C.POINTER(CodecParams), u64p, i32p, C.c_void_p]
    l.charls_amd_probe_batch_device_packed.restype = C.c_int32
    l.charls_amd_decode_batch_device_ragged.argtypes = [C.c_uint32, C.c_void_p, u64p, u64p, C.POINTER(FrameDest), C.POINTER(CodecParams),
                                                        i32p, C.c_void_p]
    l.charls_amd_decode_batch_device_ragged.restype = C.c_int32
    l.charls_amd_encode_batch_device_ragged.argtypes = [C.c_uint32, C.POINTER(FrameSource), C.c_void_p, C.c_size_t, C.c_uint32, u64p, u64p,
                                                        i32p, C.c_void_p]
    l.charls_amd_encode_batch_device_ragged.restype = C.c_int32
    l.charls_amd_measure_batch_device.argtypes = [C.POINTER(CodecParams), C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32, i32p, C.c_uint32,
                                                  u64p, C.c_void_p]
    l.charls_amd_measure_batch_device.restype = C.c_int32
    l.charls_amd_encode_batch_device_budget.argtypes = [C.POINTER(CodecParams), C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32, u64p, i32p,
                                                        C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32, u64p, u64p, i32p, i32p, C.c_void_p]
    l.charls_amd_encode_batch_device_budget.restype = C.c_int32
    l.charls_amd_measure_counters.argtypes = [u64p, C.c_int32]
    l.charls_amd_measure_counters.restype = C.c_int32
    l.charls_amd_decode_batch_device_salvage.argtypes = [C.c_uint32, C.c_void_p, u64p, u64p, C.POINTER(FrameDest), C.c_uint32,
                                                         C.POINTER(CodecParams), C.POINTER(capi.SalvageReport), C.c_void_p, C.c_size_t,
                                                         i32p, C.c_void_p]
    l.charls_amd_decode_batch_device_salvage.restype = C.c_int32
    l.charls_amd_salvage_counters.argtypes = [u64p, C.c_int32]
    l.charls_amd_salvage_counters.restype = C.c_int32
    if hasattr(l, "charls_amd_decode_batch_device_salvage_indexed"):  # (an A/B tool may load a build from before part 2h)
        l.charls_amd_decode_batch_device_salvage_indexed.argtypes = [C.c_uint32, C.c_void_p, u64p, u64p, C.c_void_p, C.c_size_t, u64p,
                                                                     C.POINTER(FrameDest), C.c_uint32, C.c_uint32,
                                                                     C.POINTER(CodecParams), C.POINTER(capi.SalvageReport), C.c_void_p,
                                                                     C.c_size_t, i32p, C.c_void_p]
        l.charls_amd_decode_batch_device_salvage_indexed.restype = C.c_int32
        l.charls_amd_salvage_index_counters.argtypes = [u64p, C.c_int32]
        l.charls_amd_salvage_index_counters.restype = C.c_int32
    if hasattr(l, "charls_amd_encode_batch_host_ragged"):  # (part 2i; an A/B tool may load a build from before it)
        l.charls_amd_host_alloc.argtypes = [C.c_size_t]
        l.charls_amd_host_alloc.restype = C.c_void_p
        l.charls_amd_host_free.argtypes = [C.c_void_p]
        l.charls_amd_host_free.restype = None
        l.charls_amd_host_register.argtypes = [C.c_void_p, C.c_size_t]
        l.charls_amd_host_register.restype = C.c_int32
        l.charls_amd_host_unregister.argtypes = [C.c_void_p]
        l.charls_amd_host_unregister.restype = C.c_int32
        l.charls_amd_probe_batch_host_packed.argtypes = [C.c_uint32, C.c_void_p, u64p, u64p, C.POINTER(CodecParams), u64p, i32p]
        l.charls_amd_probe_batch_host_packed.restype = C.c_int32
        l.charls_amd_encode_batch_host_ragged.argtypes = [C.c_uint32, C.POINTER(FrameSource), C.c_void_p, C.c_size_t, C.c_uint32, u64p, u64p, i32p]
        l.charls_amd_encode_batch_host_ragged.restype = C.c_int32
        l.charls_amd_decode_batch_host_ragged.argtypes = [C.c_uint32, C.c_void_p, u64p, u64p, C.POINTER(FrameDest), C.POINTER(CodecParams), i32p]
        l.charls_amd_decode_batch_host_ragged.restype = C.c_int32
        l.charls_amd_encode_batch_host.argtypes = [C.POINTER(CodecParams), C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t,
                                                   C.c_uint32, C.c_size_t, u64p, u64p, i32p]
        l.charls_amd_encode_batch_host.restype = C.c_int32
        l.charls_amd_decode_batch_host.argtypes = [C.c_uint32, C.c_void_p, u64p, u64p, C.c_void_p, C.c_size_t, C.c_uint32,
                                                   C.POINTER(CodecParams), i32p]
        l.charls_amd_decode_batch_host.restype = C.c_int32
        l.charls_amd_host_counters.argtypes = [u64p, C.c_int32]
        l.charls_amd_host_counters.restype = C.c_int32
    if hasattr(l, "charls_amd_transcode_batch_device"):  # (part 2j; an A/B tool may load a build from before it)
        spec_p = C.POINTER(capi.TranscodeSpec)
        l.charls_amd_transcode_batch_device.argtypes = [C.c_uint32, C.c_void_p, u64p, u64p, spec_p, C.c_uint32, C.c_void_p, C.c_size_t,
                                                        C.c_uint32, u64p, u64p, C.POINTER(CodecParams), i32p, C.c_void_p]
        l.charls_amd_transcode_batch_device.restype = C.c_int32
        l.charls_amd_transcode_batch_host.argtypes = [C.c_uint32, C.c_void_p, u64p, u64p, spec_p, C.c_uint32, C.c_void_p, C.c_size_t,
                                                      C.c_uint32, u64p, u64p, C.POINTER(CodecParams), i32p]
        l.charls_amd_transcode_batch_host.restype = C.c_int32
        l.charls_amd_transcode_counters.argtypes = [u64p, C.c_int32]
        l.charls_amd_transcode_counters.restype = C.c_int32
    if hasattr(l, "charls_amd_encode_batch_device_ragged_budget"):  # (part 2k; an A/B tool may load a build from before it)
        spec_p = C.POINTER(capi.TranscodeSpec)
        l.charls_amd_measure_batch_device_ragged.argtypes = [C.c_uint32, C.POINTER(FrameSource), i32p, C.c_uint32, u64p, i32p, C.c_void_p]
        l.charls_amd_measure_batch_device_ragged.restype = C.c_int32
        l.charls_amd_encode_batch_device_ragged_budget.argtypes = [C.c_uint32, C.POINTER(FrameSource), u64p, i32p, C.c_uint32, C.c_void_p,
                                                                   C.c_size_t, C.c_uint32, u64p, u64p, i32p, i32p, C.c_void_p]
        l.charls_amd_encode_batch_device_ragged_budget.restype = C.c_int32
        l.charls_amd_transcode_batch_device_budget.argtypes = [C.c_uint32, C.c_void_p, u64p, u64p, spec_p, C.c_uint32, u64p, i32p, C.c_uint32,
                                                               C.c_void_p, C.c_size_t, C.c_uint32, u64p, u64p, i32p, C.POINTER(CodecParams),
                                                               i32p, C.c_void_p]
        l.charls_amd_transcode_batch_device_budget.restype = C.c_int32
        l.charls_amd_transcode_batch_host_budget.argtypes = [C.c_uint32, C.c_void_p, u64p, u64p, spec_p, C.c_uint32, u64p, i32p, C.c_uint32,
                                                             C.c_void_p, C.c_size_t, C.c_uint32, u64p, u64p, i32p, C.POINTER(CodecParams), i32p]
        l.charls_amd_transcode_batch_host_budget.restype = C.c_int32
    if hasattr(l, "charls_amd_index_batch_device_packed"):  # (part 2l; an A/B tool may load a build from before it)
        l.charls_amd_index_batch_device_packed.argtypes = [C.c_uint32, C.c_void_p, u64p, u64p, C.POINTER(FrameDest), C.c_uint32, C.c_void_p,
                                                           C.c_size_t, u64p, C.POINTER(CodecParams), i32p, C.c_void_p]
        l.charls_amd_index_batch_device_packed.restype = C.c_int32
        l.charls_amd_decode_batch_device_ragged_indexed.argtypes = [C.c_uint32, C.c_void_p, u64p, u64p, C.c_void_p, C.c_size_t, u64p,
                                                                    C.POINTER(FrameDest), C.POINTER(CodecParams), i32p, C.c_void_p]
        l.charls_amd_decode_batch_device_ragged_indexed.restype = C.c_int32
        l.charls_amd_decode_rows_batch_device_ragged.argtypes = [C.c_uint32, C.c_void_p, u64p, u64p, C.c_void_p, C.c_size_t, u64p, u32p, u32p,
                                                                 C.POINTER(FrameDest), i32p, C.c_void_p]
        l.charls_amd_decode_rows_batch_device_ragged.restype = C.c_int32
        l.charls_amd_index_batch_host.argtypes = [C.c_uint32, C.c_void_p, u64p, u64p, C.c_uint32, C.c_void_p, C.c_size_t, u64p,
                                                  C.POINTER(CodecParams), i32p]
        l.charls_amd_index_batch_host.restype = C.c_int32
    if hasattr(l, "charls_amd_decode_rows_batch_device_ragged_markers"):  # (part 2m; an A/B tool may load a build from before it)
        l.charls_amd_decode_rows_batch_device_ragged_markers.argtypes = l.charls_amd_decode_rows_batch_device_ragged.argtypes
        l.charls_amd_decode_rows_batch_device_ragged_markers.restype = C.c_int32
        l.charls_amd_band_marker_counters.argtypes = [u64p, C.c_int32]
        l.charls_amd_band_marker_counters.restype = C.c_int32
    l._batch_bound = True
    return l


def estimated_destination_size(width, height, bits, components) -> int:
    """charls_jpegls_encoder_get_estimated_destination_size (reference src/charls_jpegls_encoder.cpp:103-114)."""
    raw = width * height * components * ((bits + 7) // 8)
    return raw + raw // 16 + 1024 + 34


@dataclass
class EncodedBatch:
    streams: "torch.Tensor"  # (frames, pitch) uint8 on the device; frame f's .jls is streams[f, :sizes[f]]
    sizes: np.ndarray        # uint64, host
    errcs: np.ndarray        # int32, host
    gpu_ms: tuple            # (total, dominant kernel)


def last_timings(lib=None):
    l = _bind(lib or capi.load_product())
    buf = (C.c_double * 8)()
    n = l.charls_amd_last_timings(buf, 8)
    return tuple(buf[i] for i in range(n))


def encode_batch(frames, *, bits_per_sample=8, component_count=1, interleave_mode=0, near_lossless=0,
                 color_transformation=0, preset=(0, 0, 0, 0, 0), encoding_options=0, restart_interval=0, streams=None,
                 lib=None) -> EncodedBatch:
    """frames: contiguous torch tensor on the GPU, (F, H, W) / (F, C, H, W) for ILV_NONE or (F, H, W, C) otherwise,
    dtype uint8 (<= 8 bit) or int16/uint16 (9..16 bit).  restart_interval (lines, 0 = none) is this library's extension:
    the intervals of a frame are coded in parallel and separated by RSTm markers."""
    import torch
    lib = lib or capi.load_product()
    l = _bind(lib)
    assert frames.is_cuda and frames.is_contiguous()
    count = frames.shape[0]
    if component_count == 1 or interleave_mode == 0:
        height, width = frames.shape[-2], frames.shape[-1]
    else:
        height, width = frames.shape[1], frames.shape[2]
    frame_pitch = frames[0].numel() * frames.element_size()
    if streams is None:
        pitch = (estimated_destination_size(width, height, bits_per_sample, component_count) + 255) & ~255
        streams = torch.empty((count, pitch), dtype=torch.uint8, device=frames.device)
    assert streams.is_contiguous() and streams.shape[0] == count
    p = CodecParams(capi.FrameInfo(width, height, bits_per_sample, component_count), near_lossless, interleave_mode,
                    color_transformation, capi.PcParameters(*preset), encoding_options, restart_interval)
    sizes = np.zeros(count, dtype=np.uint64)
    errcs = np.zeros(count, dtype=np.int32)
    stream = torch.cuda.current_stream(frames.device).cuda_stream
    rc = l.charls_amd_encode_batch_device(C.byref(p), count, frames.data_ptr(), frame_pitch, 0, streams.data_ptr(),
                                          streams.shape[1], sizes.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          errcs.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_encode_batch_device")
    return EncodedBatch(streams, sizes, errcs, last_timings(lib))


def decode_batch(streams, sizes, out, *, lib=None):
    """streams: (F, pitch) uint8 device tensor; sizes: host uint64 array; out: preallocated device tensor whose [f] slice
    receives frame f in the reference's user layout. Returns (params, errcs, gpu_ms)."""
    import torch
    lib = lib or capi.load_product()
    l = _bind(lib)
    assert streams.is_cuda and streams.is_contiguous() and out.is_cuda and out.is_contiguous()
    count = streams.shape[0]
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    errcs = np.zeros(count, dtype=np.int32)
    p = CodecParams()
    frame_pitch = out[0].numel() * out.element_size()
    stream = torch.cuda.current_stream(streams.device).cuda_stream
    rc = l.charls_amd_decode_batch_device(count, streams.data_ptr(), streams.shape[1],
                                          sizes.ctypes.data_as(C.POINTER(C.c_uint64)), out.data_ptr(), frame_pitch, 0,
                                          C.byref(p), errcs.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_decode_batch_device")
    return p, errcs, last_timings(lib)


# ---- the seek-point index in the batch API (charls_amd.h part 2c): indexes are host bytes, everything else stays in HBM ----

def index_size_bound(width, height, bits_per_sample=8, component_count=1, interleave_mode=0, near_lossless=0,
                     lines_per_seek_point=64, *, color_transformation=0, preset=(0, 0, 0, 0, 0), restart_interval=0, lib=None) -> int:
    """charls_amd_index_size_bound: what get_index_size gives for a stream with these parameters.  Needs no GPU."""
    l = _bind(lib or capi.load_product())
    p = CodecParams(capi.FrameInfo(width, height, bits_per_sample, component_count), near_lossless, interleave_mode,
                    color_transformation, capi.PcParameters(*preset), 0, restart_interval)
    out = C.c_size_t(0)
    rc = l.charls_amd_index_size_bound(C.byref(p), lines_per_seek_point, C.byref(out))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_index_size_bound")
    return int(out.value)


def seek_launches(lib=None) -> int:
    """charls_amd_index_counters [3]: launches of the seek kernels so far (a batch call is one per group of scans)."""
    l = _bind(lib or capi.load_product())
    out = (C.c_uint64 * 4)()
    n = l.charls_amd_index_counters(out, 4)
    assert n == 4
    return int(out[3])


def _pack_indexes(indexes, count):
    """[bytes or None] -> (host uint8 array (count, pitch), pitch, uint64 sizes); None / b"" = no index."""
    assert len(indexes) == count
    pitch = max([len(x) for x in indexes if x] + [16])
    packed = np.zeros((count, pitch), dtype=np.uint8)
    sizes = np.zeros(count, dtype=np.uint64)
    for f, x in enumerate(indexes):
        if x:
            packed[f, :len(x)] = np.frombuffer(x, dtype=np.uint8)
            sizes[f] = len(x)
    return packed, pitch, sizes


def _index_pitch_for(out, lines, lib):
    """The largest index of a frame that fills out[f]: (H, W), planar (C, H, W) or interleaved (H, W, C), 8 or 16 bit."""
    bits = 16 if out.element_size() == 2 else 8
    shape = tuple(out.shape[1:])
    if len(shape) not in (2, 3):
        raise ValueError("index_pitch is needed: the frames' geometry cannot be read from the shape of `out`")
    if len(shape) == 2:
        cases = [(shape[1], shape[0], 1, 0)]
    else:
        cases = [(shape[2], shape[1], shape[0], 0)] + ([(shape[1], shape[0], shape[2], 2)] if shape[2] <= 4 else [])
    return max(index_size_bound(w, h, bits, c, ilv, 0, lines, lib=lib) for w, h, c, ilv in cases)


def decode_batch_and_index(streams, sizes, out, lines_per_seek_point=64, *, index_pitch=None, stride=0, frame_pitch=None, lib=None):
    """charls_amd_decode_batch_device_and_index: decode_batch that also builds every frame's seek-point index.
    index_pitch: bytes kept per index (at least index_size_bound of every frame; by default that of a frame that fills
    out[f]).  Returns (params, errcs, [index bytes]); the index of a frame that failed is b""."""
    import torch
    lib = lib or capi.load_product()
    l = _bind(lib)
    if index_pitch is None:
        index_pitch = _index_pitch_for(out, lines_per_seek_point, lib)
    assert streams.is_cuda and streams.is_contiguous() and out.is_cuda
    count = streams.shape[0]
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    errcs = np.zeros(count, dtype=np.int32)
    index_sizes = np.zeros(count, dtype=np.uint64)
    indexes = np.zeros((count, int(index_pitch)), dtype=np.uint8)
    p = CodecParams()
    if frame_pitch is None:
        frame_pitch = out[0].numel() * out.element_size()
    stream = torch.cuda.current_stream(streams.device).cuda_stream
    rc = l.charls_amd_decode_batch_device_and_index(count, streams.data_ptr(), streams.shape[1], sizes.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                    out.data_ptr(), frame_pitch, stride, lines_per_seek_point, indexes.ctypes.data,
                                                    int(index_pitch), index_sizes.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(p),
                                                    errcs.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_decode_batch_device_and_index")
    return p, errcs, [indexes[f, :int(index_sizes[f])].tobytes() for f in range(count)]


def decode_batch_indexed(streams, sizes, indexes, out, *, stride=0, frame_pitch=None, lib=None):
    """charls_amd_decode_batch_device_indexed: decode_batch through seek-point indexes (a list of bytes; None or b"" = that
    frame decodes the ordinary way).  Returns (params, errcs)."""
    import torch
    lib = lib or capi.load_product()
    l = _bind(lib)
    assert streams.is_cuda and streams.is_contiguous() and out.is_cuda
    count = streams.shape[0]
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    errcs = np.zeros(count, dtype=np.int32)
    packed, pitch, index_sizes = _pack_indexes(indexes, count)
    p = CodecParams()
    if frame_pitch is None:
        frame_pitch = out[0].numel() * out.element_size()
    stream = torch.cuda.current_stream(streams.device).cuda_stream
    rc = l.charls_amd_decode_batch_device_indexed(count, streams.data_ptr(), streams.shape[1], sizes.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                  packed.ctypes.data, pitch, index_sizes.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                  out.data_ptr(), frame_pitch, stride, C.byref(p),
                                                  errcs.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_decode_batch_device_indexed")
    return p, errcs


def decode_rows_batch(streams, sizes, indexes, first_rows, row_counts, bands, *, stride=0, band_pitch=None, lib=None):
    """charls_amd_decode_rows_batch_device: rows [first_rows[f], first_rows[f] + row_counts[f]) of frame f into bands[f]
    (decode_rows' layout), through the frame's index where indexes[f] is one, from the top otherwise.  Returns errcs."""
    import torch
    lib = lib or capi.load_product()
    l = _bind(lib)
    assert streams.is_cuda and streams.is_contiguous() and bands.is_cuda
    count = streams.shape[0]
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    first_rows = np.ascontiguousarray(first_rows, dtype=np.uint32)
    row_counts = np.ascontiguousarray(row_counts, dtype=np.uint32)
    assert len(first_rows) == count and len(row_counts) == count
    errcs = np.zeros(count, dtype=np.int32)
    packed, pitch, index_sizes = _pack_indexes(indexes, count)
    if band_pitch is None:
        band_pitch = bands[0].numel() * bands.element_size()
    stream = torch.cuda.current_stream(streams.device).cuda_stream
    rc = l.charls_amd_decode_rows_batch_device(count, streams.data_ptr(), streams.shape[1], sizes.ctypes.data_as(C.POINTER(C.c_uint64)),
                                               packed.ctypes.data, pitch, index_sizes.ctypes.data_as(C.POINTER(C.c_uint64)),
                                               first_rows.ctypes.data_as(C.POINTER(C.c_uint32)), row_counts.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               bands.data_ptr(), band_pitch, stride, errcs.ctypes.data_as(C.POINTER(C.c_int32)),
                                               C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_decode_rows_batch_device")
    return errcs


# ---- packed streams (charls_amd.h part 2d): one device buffer, a host table of offsets ------------------------------------

@dataclass
class PackedBatch:
    packed: "torch.Tensor"   # 1-D uint8 on the device; frame f's .jls is packed[offsets[f]:offsets[f] + sizes[f]]
    offsets: np.ndarray      # uint64, host, frames + 1 elements; offsets[-1] is the total
    sizes: np.ndarray        # uint64, host
    errcs: np.ndarray        # int32, host (None from pack_streams)


def pack_streams(streams, sizes, *, alignment=1, packed=None, capacity=None, lib=None) -> PackedBatch:
    """charls_amd_pack_streams_device: the (F, pitch) slot tensor of encode_batch into the packed form.  packed: a 1-D uint8
    device tensor to fill (by default one of exactly the total is made); capacity: what the call may use of it."""
    import torch
    lib = lib or capi.load_product()
    l = _bind(lib)
    assert streams.is_cuda and streams.is_contiguous()
    count = streams.shape[0]
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    assert len(sizes) == count
    if packed is None:
        total, step = 0, max(int(alignment), 1)  # (an alignment the call refuses: it says so itself)
        for s in sizes:
            total = -(-(total + int(s)) // step) * step
        packed = torch.empty(max(total, 16), dtype=torch.uint8, device=streams.device)
        if capacity is None:
            capacity = total
    assert packed.is_cuda and packed.is_contiguous()
    if capacity is None:
        capacity = packed.numel()
    offsets = np.zeros(count + 1, dtype=np.uint64)
    stream = torch.cuda.current_stream(streams.device).cuda_stream
    rc = l.charls_amd_pack_streams_device(count, streams.data_ptr(), streams.shape[1] if streams.dim() == 2 else 0,
                                          sizes.ctypes.data_as(C.POINTER(C.c_uint64)), packed.data_ptr(), int(capacity), alignment,
                                          offsets.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_pack_streams_device")
    return PackedBatch(packed, offsets, sizes, None)


def encode_batch_packed(frames, packed, *, alignment=1, max_stream_bytes=0, capacity=None, bits_per_sample=8, component_count=1,
                        interleave_mode=0, near_lossless=0, color_transformation=0, preset=(0, 0, 0, 0, 0), encoding_options=0,
                        restart_interval=0, lib=None) -> PackedBatch:
    """charls_amd_encode_batch_device_packed: encode_batch without slots -- the streams go back to back into `packed` (a 1-D
    uint8 device tensor; capacity: what the call may use of it, by default all).  frames as for encode_batch."""
    import torch
    lib = lib or capi.load_product()
    l = _bind(lib)
    assert frames.is_cuda and frames.is_contiguous() and packed.is_cuda and packed.is_contiguous()
    count = frames.shape[0]
    if component_count == 1 or interleave_mode == 0:
        height, width = frames.shape[-2], frames.shape[-1]
    else:
        height, width = frames.shape[1], frames.shape[2]
    frame_pitch = frames[0].numel() * frames.element_size() if count else 0
    p = CodecParams(capi.FrameInfo(width, height, bits_per_sample, component_count), near_lossless, interleave_mode,
                    color_transformation, capi.PcParameters(*preset), encoding_options, restart_interval)
    offsets = np.zeros(count + 1, dtype=np.uint64)
    sizes = np.zeros(count, dtype=np.uint64)
    errcs = np.zeros(count, dtype=np.int32)
    stream = torch.cuda.current_stream(frames.device).cuda_stream
    rc = l.charls_amd_encode_batch_device_packed(C.byref(p), count, frames.data_ptr(), frame_pitch, 0, packed.data_ptr(),
                                                 packed.numel() if capacity is None else int(capacity), alignment, int(max_stream_bytes),
                                                 offsets.ctypes.data_as(C.POINTER(C.c_uint64)), sizes.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                 errcs.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_encode_batch_device_packed")
    return PackedBatch(packed, offsets, sizes, errcs)


def decode_batch_packed(packed, offsets, sizes, out, *, stride=0, frame_pitch=None, lib=None):
    """charls_amd_decode_batch_device_packed: decode_batch with frame f's stream at packed[offsets[f]:offsets[f] + sizes[f]]
    (offsets: host uint64, at least len(sizes) elements, any order).  Returns (params, errcs, gpu_ms)."""
    import torch
    lib = lib or capi.load_product()
    l = _bind(lib)
    assert packed.is_cuda and packed.is_contiguous() and out.is_cuda
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    count = len(sizes)
    assert len(offsets) >= count
    errcs = np.zeros(count, dtype=np.int32)
    p = CodecParams()
    if frame_pitch is None:
        frame_pitch = out[0].numel() * out.element_size() if count else 0
    stream = torch.cuda.current_stream(packed.device).cuda_stream
    rc = l.charls_amd_decode_batch_device_packed(count, packed.data_ptr(), offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                 sizes.ctypes.data_as(C.POINTER(C.c_uint64)), out.data_ptr(), frame_pitch, stride,
                                                 C.byref(p), errcs.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_decode_batch_device_packed")
    return p, errcs, last_timings(lib)


# ---- ragged frames (charls_amd.h part 2e): a table entry per frame, tensors that need not share an allocation --------------

def codec_params(width, height, bits_per_sample=8, component_count=1, interleave_mode=0, near_lossless=0, *, color_transformation=0,
                 preset=(0, 0, 0, 0, 0), encoding_options=0, restart_interval=0) -> CodecParams:
    return CodecParams(capi.FrameInfo(width, height, bits_per_sample, component_count), near_lossless, interleave_mode,
                       color_transformation, capi.PcParameters(*preset), encoding_options, restart_interval)


def _row_stride(t, planar):
    """The `stride` argument for tensor t: 0 (minimal) for a contiguous one; for a view -- a tile cut out of an image -- the
    bytes from row to row: (H, W) and (H, W, C) views with contiguous rows, (C, H, W) views whose planes follow each other."""
    if t.is_contiguous():
        return 0
    if t.dim() == 3 and planar:
        assert t.stride(2) == 1 and t.stride(0) == t.stride(1) * t.shape[1], "a planar view's planes must follow each other"
        return t.stride(1) * t.element_size()
    assert t.dim() in (2, 3) and t.stride(-1) == 1 and (t.dim() == 2 or t.stride(1) == t.shape[2]), "a view's rows must be contiguous"
    return t.stride(0) * t.element_size()


def probe_packed(packed, offsets, sizes, *, lib=None):
    """charls_amd_probe_batch_device_packed: what the streams packed[offsets[f]:offsets[f] + sizes[f]] hold, without decoding
    them.  Returns (params -- a ctypes array of CodecParams --, frame_bytes uint64, errcs); probe, then allocate, then decode."""
    import torch
    lib = lib or capi.load_product()
    l = _bind(lib)
    assert packed.is_cuda and packed.is_contiguous()
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    count = len(sizes)
    assert len(offsets) >= count
    params = (CodecParams * max(count, 1))()
    frame_bytes = np.zeros(count, dtype=np.uint64)
    errcs = np.zeros(count, dtype=np.int32)
    stream = torch.cuda.current_stream(packed.device).cuda_stream
    rc = l.charls_amd_probe_batch_device_packed(count, packed.data_ptr(), offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                sizes.ctypes.data_as(C.POINTER(C.c_uint64)), params,
                                                frame_bytes.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                errcs.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_probe_batch_device_packed")
    return params, frame_bytes, errcs


def _frame_dests(outs, strides, capacities):
    dests = (FrameDest * max(len(outs), 1))()
    for f, t in enumerate(outs):
        assert t.is_cuda
        assert strides is not None or t.is_contiguous() or t.dim() == 2, "a 3-D view: say its row stride (planar or interleaved?)"
        stride = strides[f] if strides is not None else _row_stride(t, False)
        if capacities is not None:
            capacity = int(capacities[f])
        elif t.is_contiguous():
            capacity = t.numel() * t.element_size()
        else:  # the view's extent: to the end of its last row
            capacity = (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()
        dests[f] = FrameDest(t.data_ptr(), capacity, int(stride), 0)
    return dests


def decode_batch_ragged(packed, offsets, sizes, outs, *, strides=None, capacities=None, lib=None):
    """charls_amd_decode_batch_device_ragged: frame f of the packed streams into outs[f], a device tensor of its own (any
    allocation, any shape of enough bytes; a view with padded rows states them through its strides).  strides / capacities:
    per-frame overrides (bytes).  Returns (params -- a ctypes array, one CodecParams per frame --, errcs, gpu_ms)."""
    import torch
    lib = lib or capi.load_product()
    l = _bind(lib)
    assert packed.is_cuda and packed.is_contiguous()
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    count = len(sizes)
    assert len(offsets) >= count and len(outs) == count
    dests = _frame_dests(outs, strides, capacities)
    params = (CodecParams * max(count, 1))()
    errcs = np.zeros(count, dtype=np.int32)
    stream = torch.cuda.current_stream(packed.device).cuda_stream
    rc = l.charls_amd_decode_batch_device_ragged(count, packed.data_ptr(), offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                 sizes.ctypes.data_as(C.POINTER(C.c_uint64)), dests, params,
                                                 errcs.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_decode_batch_device_ragged")
    return params, errcs, last_timings(lib)


@dataclass
class SalvagedBatch:
    params: object       # ctypes array, one CodecParams per frame
    errcs: np.ndarray    # int32: what decode_batch_ragged reports
    reports: object      # ctypes array, one capi.SalvageReport per frame (state 1: the destination is usable)
    status: np.ndarray   # (frames, status_pitch) uint8, one byte per (scan, interval) of a salvaged frame; None when not asked for
    gpu_ms: tuple        # last_timings: round 1's (total, dominant kernel); with a round 2, what that round took (host clock)


def decode_batch_salvage(packed, offsets, sizes, outs, fill_value=0, *, strides=None, capacities=None, status_pitch=0, lib=None) -> SalvagedBatch:
    """charls_amd_decode_batch_device_salvage: decode_batch_ragged, and for the frames it fails on that have restart
    intervals the intact intervals, with fill_value in the rows of the lost ones (reports[f].state == 1).  status_pitch > 0:
    also the status byte of every (scan, interval): 0 kept, 1 unclaimed, 2 not decodable to its exact length, 3 scan not reached."""
    import torch
    lib = lib or capi.load_product()
    l = _bind(lib)
    assert packed.is_cuda and packed.is_contiguous()
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    count = len(sizes)
    assert len(offsets) >= count and len(outs) == count
    dests = _frame_dests(outs, strides, capacities)
    params = (CodecParams * max(count, 1))()
    reports = (capi.SalvageReport * max(count, 1))()
    errcs = np.zeros(count, dtype=np.int32)
    status = np.full((max(count, 1), status_pitch), 0xFF, dtype=np.uint8) if status_pitch else None
    stream = torch.cuda.current_stream(packed.device).cuda_stream
    rc = l.charls_amd_decode_batch_device_salvage(count, packed.data_ptr(), offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                  sizes.ctypes.data_as(C.POINTER(C.c_uint64)), dests, int(fill_value), params, reports,
                                                  status.ctypes.data if status is not None else None, status_pitch,
                                                  errcs.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_decode_batch_device_salvage")
    return SalvagedBatch(params, errcs, reports, status, last_timings(lib))


def salvage_counters(lib=None):
    """charls_amd_salvage_counters: (frames salvaged, intervals kept, intervals lost, launches of the salvage kernels),
    process-wide since the library was loaded."""
    l = _bind(lib or capi.load_product())
    out = (C.c_uint64 * 4)()
    n = l.charls_amd_salvage_counters(out, 4)
    assert n == 4
    return tuple(int(out[i]) for i in range(4))


SALVAGE_PREFIX = 1  # CHARLS_AMD_SALVAGE_PREFIX


def decode_batch_salvage_indexed(packed, offsets, sizes, outs, indexes=None, fill_value=0, *, flags=0, strides=None, capacities=None,
                                 status_pitch=0, lib=None) -> SalvagedBatch:
    """charls_amd_decode_batch_device_salvage_indexed: decode_batch_salvage, and for the frames it leaves failed that have a
    seek-point index (indexes[f]: bytes, or None) the intervals between seek points that decode to the next point's state
    (reports[f].state == 1; status 0 kept and proven, 4 kept on the index's word, 2 lost, 3 not reached); with
    flags=SALVAGE_PREFIX a frame without a usable index keeps the rows in front of its first error (state 3; status per
    scan: 0 whole, 5 prefix, 3 not reached).  Build the index while the stream is sound (decode_batch_and_index)."""
    import torch
    lib = lib or capi.load_product()
    l = _bind(lib)
    assert packed.is_cuda and packed.is_contiguous()
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    count = len(sizes)
    assert len(offsets) >= count and len(outs) == count
    indexes = [None] * count if indexes is None else list(indexes)
    assert len(indexes) == count
    index_sizes = np.array([0 if i is None else len(i) for i in indexes], dtype=np.uint64).reshape(count)
    pitch = max([int(v) for v in index_sizes] + [1])
    table = np.zeros((max(count, 1), pitch), dtype=np.uint8)
    for f, i in enumerate(indexes):
        if i is not None:
            table[f, :len(i)] = np.frombuffer(bytes(i), dtype=np.uint8)
    if count == 0:
        index_sizes = np.zeros(1, dtype=np.uint64)
    dests = _frame_dests(outs, strides, capacities)
    params = (CodecParams * max(count, 1))()
    reports = (capi.SalvageReport * max(count, 1))()
    errcs = np.zeros(count, dtype=np.int32)
    status = np.full((max(count, 1), status_pitch), 0xFF, dtype=np.uint8) if status_pitch else None
    stream = torch.cuda.current_stream(packed.device).cuda_stream
    rc = l.charls_amd_decode_batch_device_salvage_indexed(count, packed.data_ptr(), offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                          sizes.ctypes.data_as(C.POINTER(C.c_uint64)), table.ctypes.data, pitch,
                                                          index_sizes.ctypes.data_as(C.POINTER(C.c_uint64)), dests, int(fill_value),
                                                          int(flags), params, reports,
                                                          status.ctypes.data if status is not None else None, status_pitch,
                                                          errcs.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_decode_batch_device_salvage_indexed")
    return SalvagedBatch(params, errcs, reports, status, last_timings(lib))


def salvage_index_counters(lib=None):
    """charls_amd_salvage_index_counters: (frames salvaged by index, intervals kept proven, kept on the index, lost, frames
    salvaged by prefix, launches), process-wide since the library was loaded."""
    l = _bind(lib or capi.load_product())
    out = (C.c_uint64 * 6)()
    n = l.charls_amd_salvage_index_counters(out, 6)
    assert n == 6
    return tuple(int(out[i]) for i in range(6))


def encode_batch_ragged(frames, params, packed, *, alignment=1, strides=None, max_stream_bytes=None, capacity=None, lib=None) -> PackedBatch:
    """charls_amd_encode_batch_device_ragged: frames[f] -- a device tensor of its own: any allocation, the same tensor more
    than once, a view into a larger image (a tile: its row stride is read from the view) -- coded with params[f] (CodecParams,
    see codec_params; one CodecParams serves every frame).  The streams go back to back into `packed` in this order.  strides
    / max_stream_bytes: per-frame overrides (bytes; 0 = minimal / part 1's estimate)."""
    import torch
    lib = lib or capi.load_product()
    l = _bind(lib)
    assert packed.is_cuda and packed.is_contiguous()
    count = len(frames)
    if isinstance(params, CodecParams):
        params = [params] * count
    assert len(params) == count
    sources = (FrameSource * max(count, 1))()
    for f, t in enumerate(frames):
        assert t.is_cuda
        stride = strides[f] if strides is not None else _row_stride(t, params[f].interleave_mode == 0)
        sources[f] = FrameSource(params[f], t.data_ptr(), int(stride), 0, int(max_stream_bytes[f]) if max_stream_bytes is not None else 0)
    offsets = np.zeros(count + 1, dtype=np.uint64)
    sizes = np.zeros(count, dtype=np.uint64)
    errcs = np.zeros(count, dtype=np.int32)
    stream = torch.cuda.current_stream(packed.device).cuda_stream
    rc = l.charls_amd_encode_batch_device_ragged(count, sources, packed.data_ptr(), packed.numel() if capacity is None else int(capacity),
                                                 alignment, offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                 sizes.ctypes.data_as(C.POINTER(C.c_uint64)), errcs.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_encode_batch_device_ragged")
    return PackedBatch(packed, offsets, sizes, errcs)


# ---- host memory (charls_amd.h part 2i): numpy arrays or CPU torch tensors in, host bytes out, the copies inside the call ---

class _PinnedBlock:
    """Memory of charls_amd_host_alloc, freed when the last array that looks at it is gone."""

    def __init__(self, l, nbytes):
        self._l, self.address = l, l.charls_amd_host_alloc(nbytes)
        if not self.address:
            raise MemoryError("charls_amd_host_alloc: no usable device, or no memory")
        self.__array_interface__ = {"data": (self.address, False), "shape": (nbytes,), "typestr": "|u1", "version": 3}

    def __del__(self):
        if getattr(self, "address", None):
            self._l.charls_amd_host_free(self.address)
            self.address = None


def host_alloc(nbytes, *, lib=None) -> np.ndarray:
    """charls_amd_host_alloc: a uint8 array of pinned host memory (view it as another dtype, slice it, reshape it)."""
    l = _bind(lib or capi.load_product())
    return np.asarray(_PinnedBlock(l, int(nbytes)))


def _host(x):
    """(address, shape, strides in bytes, bytes per element) of a numpy array or a CPU torch tensor."""
    if isinstance(x, np.ndarray):
        return x.ctypes.data, x.shape, x.strides, x.itemsize
    assert not x.is_cuda, "host memory: a numpy array or a CPU tensor"
    return x.data_ptr(), tuple(x.shape), tuple(s * x.element_size() for s in x.stride()), x.element_size()


def _host_contiguous(x):
    address, shape, strides, item = _host(x)
    expect = item
    for n, s in zip(reversed(shape), reversed(strides)):
        assert n == 1 or s == expect, "host memory that is one contiguous block"
        expect *= n
    return address, expect  # (address, bytes)


def _host_rows(x, planar):
    """(address, stride argument, extent in bytes) of one frame: a contiguous array (stride 0), or a view with padded rows --
    (H, W) and (H, W, C) views with contiguous rows, (C, H, W) views whose planes follow each other."""
    address, shape, strides, item = _host(x)
    if len(shape) == 3 and planar:
        assert strides[2] == item and strides[0] == strides[1] * shape[1], "a planar view's planes must follow each other"
        row, rows, stride = shape[2] * item, shape[0] * shape[1], strides[1]
    elif len(shape) == 3:
        assert strides[2] == item and strides[1] == shape[2] * item, "a view's rows must be contiguous"
        row, rows, stride = shape[1] * shape[2] * item, shape[0], strides[0]
    else:
        assert len(shape) == 2 and strides[1] == item, "a view's rows must be contiguous"
        row, rows, stride = shape[1] * item, shape[0], strides[0]
    return address, (0 if stride == row else stride), (stride * (rows - 1) + row if rows else 0)


def host_register(x, *, lib=None):
    """charls_amd_host_register: pins the memory of a contiguous array the caller owns (undo with host_unregister)."""
    l = _bind(lib or capi.load_product())
    address, nbytes = _host_contiguous(x)
    rc = l.charls_amd_host_register(address, nbytes)
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_host_register")


def host_unregister(x, *, lib=None):
    l = _bind(lib or capi.load_product())
    rc = l.charls_amd_host_unregister(_host_contiguous(x)[0])
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_host_unregister")


def host_counters(lib=None):
    """charls_amd_host_counters: (calls, windows, bytes up, bytes down, pageable bytes staged, device bytes held, pinned bytes held)."""
    l = _bind(lib or capi.load_product())
    out = (C.c_uint64 * 7)()
    n = l.charls_amd_host_counters(out, 7)
    assert n == 7
    return tuple(int(out[i]) for i in range(7))


def _tables(offsets, sizes):
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    assert len(offsets) >= len(sizes)
    return offsets, sizes, len(sizes)


def probe_host(packed, offsets, sizes, *, lib=None):
    """charls_amd_probe_batch_host_packed: probe_packed on host bytes; needs no GPU.  Returns (params, frame_bytes, errcs)."""
    l = _bind(lib or capi.load_product())
    offsets, sizes, count = _tables(offsets, sizes)
    params = (CodecParams * max(count, 1))()
    frame_bytes = np.zeros(count, dtype=np.uint64)
    errcs = np.zeros(count, dtype=np.int32)
    u64p = C.POINTER(C.c_uint64)
    rc = l.charls_amd_probe_batch_host_packed(count, _host_contiguous(packed)[0], offsets.ctypes.data_as(u64p), sizes.ctypes.data_as(u64p), params,
                                              frame_bytes.ctypes.data_as(u64p), errcs.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_probe_batch_host_packed")
    return params, frame_bytes, errcs


def encode_batch_host_ragged(frames, params, packed, *, alignment=1, strides=None, max_stream_bytes=None, capacity=None, lib=None) -> PackedBatch:
    """charls_amd_encode_batch_host_ragged: encode_batch_ragged with frames[f] and `packed` in HOST memory -- numpy arrays or
    CPU tensors, pinned or pageable, views with padded rows (their row stride is read from the view)."""
    l = _bind(lib or capi.load_product())
    count = len(frames)
    if isinstance(params, CodecParams):
        params = [params] * count
    assert len(params) == count
    sources = (FrameSource * max(count, 1))()
    for f, x in enumerate(frames):
        if strides is not None:  # (the caller says where the rows are: x may be any view that starts at the first row)
            address, stride = _host(x)[0], strides[f]
        else:
            address, stride, _ = _host_rows(x, params[f].interleave_mode == 0)
        sources[f] = FrameSource(params[f], address, int(stride), 0, int(max_stream_bytes[f]) if max_stream_bytes is not None else 0)
    offsets = np.zeros(count + 1, dtype=np.uint64)
    sizes = np.zeros(count, dtype=np.uint64)
    errcs = np.zeros(count, dtype=np.int32)
    address, nbytes = _host_contiguous(packed)
    u64p = C.POINTER(C.c_uint64)
    rc = l.charls_amd_encode_batch_host_ragged(count, sources, address, nbytes if capacity is None else int(capacity), alignment,
                                               offsets.ctypes.data_as(u64p), sizes.ctypes.data_as(u64p), errcs.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_encode_batch_host_ragged")
    return PackedBatch(packed, offsets, sizes, errcs)


def decode_batch_host_ragged(packed, offsets, sizes, outs, *, strides=None, capacities=None, lib=None):
    """charls_amd_decode_batch_host_ragged: decode_batch_ragged with `packed` and outs[f] in HOST memory.  Returns (params --
    one CodecParams per frame --, errcs)."""
    l = _bind(lib or capi.load_product())
    offsets, sizes, count = _tables(offsets, sizes)
    assert len(outs) == count
    dests = (FrameDest * max(count, 1))()
    for f, x in enumerate(outs):
        address, shape, byte_strides, item = _host(x)
        extent = (sum((n - 1) * s for n, s in zip(shape, byte_strides)) + item) if all(shape) else 0  # to the end of the last row
        if strides is not None:
            stride = strides[f]
        elif _is_contiguous(shape, byte_strides, item):
            stride = 0
        else:
            assert len(shape) == 2 and byte_strides[1] == item, "a 3-D view: say its row stride (planar or interleaved?)"
            stride = byte_strides[0]
        dests[f] = FrameDest(address, int(capacities[f]) if capacities is not None else extent, int(stride), 0)
    params = (CodecParams * max(count, 1))()
    errcs = np.zeros(count, dtype=np.int32)
    u64p = C.POINTER(C.c_uint64)
    rc = l.charls_amd_decode_batch_host_ragged(count, _host_contiguous(packed)[0], offsets.ctypes.data_as(u64p), sizes.ctypes.data_as(u64p), dests,
                                               params, errcs.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_decode_batch_host_ragged")
    return params, errcs


def _is_contiguous(shape, byte_strides, item):
    expect = item
    for n, s in zip(reversed(shape), reversed(byte_strides)):
        if n != 1 and s != expect:
            return False
        expect *= n
    return True


def encode_batch_host(frames, packed, *, alignment=1, max_stream_bytes=0, capacity=None, bits_per_sample=8, component_count=1,
                      interleave_mode=0, near_lossless=0, color_transformation=0, preset=(0, 0, 0, 0, 0), encoding_options=0,
                      restart_interval=0, width=None, height=None, stride=0, frame_pitch=None, lib=None) -> PackedBatch:
    """charls_amd_encode_batch_host: encode_batch_packed with `frames` -- (F, ...) as for encode_batch -- and `packed` in HOST
    memory.  width / height / stride / frame_pitch: frames with padded rows, or at some pitch of a byte array."""
    l = _bind(lib or capi.load_product())
    address, shape, byte_strides, item = _host(frames)
    assert _is_contiguous(shape, byte_strides, item)
    count = shape[0]
    if width is None or height is None:
        height, width = (shape[-2], shape[-1]) if component_count == 1 or interleave_mode == 0 else (shape[1], shape[2])
    if frame_pitch is None:
        frame_pitch = byte_strides[0] if count else 0
    p = codec_params(int(width), int(height), bits_per_sample, component_count, interleave_mode, near_lossless,
                     color_transformation=color_transformation, preset=preset, encoding_options=encoding_options, restart_interval=restart_interval)
    offsets = np.zeros(count + 1, dtype=np.uint64)
    sizes = np.zeros(count, dtype=np.uint64)
    errcs = np.zeros(count, dtype=np.int32)
    to, nbytes = _host_contiguous(packed)
    u64p = C.POINTER(C.c_uint64)
    rc = l.charls_amd_encode_batch_host(C.byref(p), count, address, int(frame_pitch), int(stride), to, nbytes if capacity is None else int(capacity),
                                        alignment, int(max_stream_bytes), offsets.ctypes.data_as(u64p), sizes.ctypes.data_as(u64p),
                                        errcs.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_encode_batch_host")
    return PackedBatch(packed, offsets, sizes, errcs)


def decode_batch_host(packed, offsets, sizes, out, *, stride=0, frame_pitch=None, lib=None):
    """charls_amd_decode_batch_host: decode_batch_packed with `packed` and `out` -- (F, ...) -- in HOST memory.  Returns
    (params, errcs)."""
    l = _bind(lib or capi.load_product())
    offsets, sizes, count = _tables(offsets, sizes)
    address, shape, byte_strides, item = _host(out)
    assert _is_contiguous(shape, byte_strides, item)
    if frame_pitch is None:
        frame_pitch = byte_strides[0] if count else 0
    errcs = np.zeros(count, dtype=np.int32)
    p = CodecParams()
    u64p = C.POINTER(C.c_uint64)
    rc = l.charls_amd_decode_batch_host(count, _host_contiguous(packed)[0], offsets.ctypes.data_as(u64p), sizes.ctypes.data_as(u64p), address,
                                        int(frame_pitch), int(stride), C.byref(p), errcs.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_decode_batch_host")
    return p, errcs


# ---- re-coding a packed blob (charls_amd.h part 2j): decode and encode again in one call, restart intervals / NEAR replaced --

@dataclass
class TranscodedBatch:
    packed: object           # the output blob (a device tensor, or host memory); frame f's .jls is packed[offsets[f]:offsets[f] + sizes[f]]
    offsets: np.ndarray      # uint64, host, frames + 1 elements; offsets[-1] is the total
    sizes: np.ndarray        # uint64, host
    errcs: np.ndarray        # int32, host
    params: object           # ctypes array, one CodecParams per frame: what frame f was coded with


def _transcode_tables(offsets, sizes, specs):
    offsets, sizes, count = _tables(offsets, sizes)
    if isinstance(specs, capi.TranscodeSpec):
        specs = [specs]
    table = (capi.TranscodeSpec * max(len(specs), 1))(*specs)
    return offsets, sizes, count, table, len(specs)


def transcode_batch(packed_in, offsets, sizes, specs, packed_out, *, alignment=1, capacity=None, lib=None) -> TranscodedBatch:
    """charls_amd_transcode_batch_device: every stream packed_in[offsets[f]:offsets[f] + sizes[f]] decoded and coded again into
    `packed_out` (1-D uint8 device tensors) with the fields replaced that specs names (capi.transcode_spec: one for every
    frame, or a list with one per frame)."""
    import torch
    lib = lib or capi.load_product()
    l = _bind(lib)
    assert packed_in.is_cuda and packed_in.is_contiguous() and packed_out.is_cuda and packed_out.is_contiguous()
    offsets, sizes, count, table, spec_count = _transcode_tables(offsets, sizes, specs)
    offsets_out = np.zeros(count + 1, dtype=np.uint64)
    sizes_out = np.zeros(count, dtype=np.uint64)
    errcs = np.zeros(count, dtype=np.int32)
    params = (CodecParams * max(count, 1))()
    stream = torch.cuda.current_stream(packed_in.device).cuda_stream
    u64p = C.POINTER(C.c_uint64)
    rc = l.charls_amd_transcode_batch_device(count, packed_in.data_ptr(), offsets.ctypes.data_as(u64p), sizes.ctypes.data_as(u64p), table,
                                             spec_count, packed_out.data_ptr(), packed_out.numel() if capacity is None else int(capacity),
                                             alignment, offsets_out.ctypes.data_as(u64p), sizes_out.ctypes.data_as(u64p), params,
                                             errcs.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_transcode_batch_device")
    return TranscodedBatch(packed_out, offsets_out, sizes_out, errcs, params)


def transcode_batch_host(packed_in, offsets, sizes, specs, packed_out, *, alignment=1, capacity=None, lib=None) -> TranscodedBatch:
    """charls_amd_transcode_batch_host: transcode_batch with both blobs in HOST memory (numpy arrays or CPU tensors, pinned or
    pageable)."""
    l = _bind(lib or capi.load_product())
    offsets, sizes, count, table, spec_count = _transcode_tables(offsets, sizes, specs)
    offsets_out = np.zeros(count + 1, dtype=np.uint64)
    sizes_out = np.zeros(count, dtype=np.uint64)
    errcs = np.zeros(count, dtype=np.int32)
    params = (CodecParams * max(count, 1))()
    to, nbytes = _host_contiguous(packed_out)
    u64p = C.POINTER(C.c_uint64)
    rc = l.charls_amd_transcode_batch_host(count, _host_contiguous(packed_in)[0], offsets.ctypes.data_as(u64p), sizes.ctypes.data_as(u64p), table,
                                           spec_count, to, nbytes if capacity is None else int(capacity), alignment,
                                           offsets_out.ctypes.data_as(u64p), sizes_out.ctypes.data_as(u64p), params,
                                           errcs.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_transcode_batch_host")
    return TranscodedBatch(packed_out, offsets_out, sizes_out, errcs, params)


# ---- encoding to a byte budget (charls_amd.h part 2f): sizes without streams, NEAR picked per frame ------------------------

def _uniform_frames(frames, width, height, frame_pitch, component_count, interleave_mode):
    """(count, width, height, frame pitch in bytes) of a batch tensor as encode_batch takes it; width / height / frame_pitch
    given by the caller win (frames with padded rows, frames at some offset of a byte tensor)."""
    count = frames.shape[0]
    if width is None or height is None:
        if component_count == 1 or interleave_mode == 0:
            height, width = frames.shape[-2], frames.shape[-1]
        else:
            height, width = frames.shape[1], frames.shape[2]
    if frame_pitch is None:
        frame_pitch = frames[0].numel() * frames.element_size() if count else 0
    return count, int(width), int(height), int(frame_pitch)


def measure_batch(frames, near_candidates, *, bits_per_sample=8, component_count=1, interleave_mode=0, color_transformation=0,
                  preset=(0, 0, 0, 0, 0), encoding_options=0, restart_interval=0, stride=0, width=None, height=None, frame_pitch=None,
                  lib=None) -> np.ndarray:
    """charls_amd_measure_batch_device: sizes[f, c] = the bytes of frame f's complete .jls at NEAR near_candidates[c], what
    encode_batch_packed reports for it, without writing any stream.  frames as for encode_batch."""
    import torch
    lib = lib or capi.load_product()
    l = _bind(lib)
    assert frames.is_cuda and frames.is_contiguous()
    count, width, height, frame_pitch = _uniform_frames(frames, width, height, frame_pitch, component_count, interleave_mode)
    nears = np.ascontiguousarray(near_candidates, dtype=np.int32)
    p = CodecParams(capi.FrameInfo(width, height, bits_per_sample, component_count), 0, interleave_mode, color_transformation,
                    capi.PcParameters(*preset), encoding_options, restart_interval)
    sizes = np.zeros((count, len(nears)), dtype=np.uint64)
    stream = torch.cuda.current_stream(frames.device).cuda_stream
    rc = l.charls_amd_measure_batch_device(C.byref(p), count, frames.data_ptr(), frame_pitch, int(stride), nears.ctypes.data_as(C.POINTER(C.c_int32)),
                                           len(nears), sizes.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_measure_batch_device")
    return sizes


def encode_batch_budget(frames, budgets, near_candidates, packed, *, alignment=1, capacity=None, bits_per_sample=8, component_count=1,
                        interleave_mode=0, color_transformation=0, preset=(0, 0, 0, 0, 0), encoding_options=0, restart_interval=0,
                        stride=0, width=None, height=None, frame_pitch=None, lib=None):
    """charls_amd_encode_batch_device_budget: every frame coded at the first NEAR of near_candidates (the order given is the
    order of preference) whose complete stream has at most budgets[f] bytes, the streams back to back in `packed` as
    encode_batch_packed places them.  Returns (PackedBatch, nears): nears[f] = -1, sizes[f] = 0 and errcs[f] =
    destination_too_small for a frame that no candidate fits."""
    import torch
    lib = lib or capi.load_product()
    l = _bind(lib)
    assert frames.is_cuda and frames.is_contiguous() and packed.is_cuda and packed.is_contiguous()
    count, width, height, frame_pitch = _uniform_frames(frames, width, height, frame_pitch, component_count, interleave_mode)
    nears = np.ascontiguousarray(near_candidates, dtype=np.int32)
    budgets = np.ascontiguousarray(budgets, dtype=np.uint64)
    assert len(budgets) == count
    p = CodecParams(capi.FrameInfo(width, height, bits_per_sample, component_count), 0, interleave_mode, color_transformation,
                    capi.PcParameters(*preset), encoding_options, restart_interval)
    offsets = np.zeros(count + 1, dtype=np.uint64)
    sizes = np.zeros(count, dtype=np.uint64)
    chosen = np.zeros(count, dtype=np.int32)
    errcs = np.zeros(count, dtype=np.int32)
    stream = torch.cuda.current_stream(frames.device).cuda_stream
    u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    rc = l.charls_amd_encode_batch_device_budget(C.byref(p), count, frames.data_ptr(), frame_pitch, int(stride), budgets.ctypes.data_as(u64p),
                                                 nears.ctypes.data_as(i32p), len(nears), packed.data_ptr(),
                                                 packed.numel() if capacity is None else int(capacity), alignment,
                                                 offsets.ctypes.data_as(u64p), sizes.ctypes.data_as(u64p), chosen.ctypes.data_as(i32p),
                                                 errcs.ctypes.data_as(i32p), C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_encode_batch_device_budget")
    return PackedBatch(packed, offsets, sizes, errcs), chosen


# ---- byte budgets for ragged frames and for re-coding (charls_amd.h part 2k) ------------------------------------------------

def _frame_sources(frames, params, strides):
    count = len(frames)
    if isinstance(params, CodecParams):
        params = [params] * count
    assert len(params) == count
    sources = (FrameSource * max(count, 1))()
    for f, t in enumerate(frames):
        assert t.is_cuda
        stride = strides[f] if strides is not None else _row_stride(t, params[f].interleave_mode == 0)
        sources[f] = FrameSource(params[f], t.data_ptr(), int(stride), 0, 0)
    return sources, count


def measure_batch_ragged(frames, params, near_candidates, *, strides=None, lib=None):
    """charls_amd_measure_batch_device_ragged: (sizes, errcs) -- sizes[f, c] = the bytes of frame f's complete .jls at NEAR
    near_candidates[c], frames and params as for encode_batch_ragged (near_lossless is not looked at); errcs[f] is the code
    measure_batch raises for a batch of this one frame, its row zeroed then."""
    import torch
    l = _bind(lib or capi.load_product())
    sources, count = _frame_sources(frames, params, strides)
    nears = np.ascontiguousarray(near_candidates, dtype=np.int32)
    sizes = np.zeros((count, len(nears)), dtype=np.uint64)
    errcs = np.zeros(count, dtype=np.int32)
    stream = torch.cuda.current_stream(frames[0].device).cuda_stream if count else 0
    rc = l.charls_amd_measure_batch_device_ragged(count, sources, nears.ctypes.data_as(C.POINTER(C.c_int32)), len(nears),
                                                  sizes.ctypes.data_as(C.POINTER(C.c_uint64)), errcs.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_measure_batch_device_ragged")
    return sizes, errcs


def encode_batch_ragged_budget(frames, params, budgets, near_candidates, packed, *, alignment=1, strides=None, capacity=None, lib=None):
    """charls_amd_encode_batch_device_ragged_budget: encode_batch_ragged with every frame coded at the first NEAR of
    near_candidates whose complete stream has at most budgets[f] bytes.  Returns (PackedBatch, nears) as encode_batch_budget
    does; a frame whose parameters the encoder refuses with any candidate has that code in errcs[f]."""
    import torch
    l = _bind(lib or capi.load_product())
    assert packed.is_cuda and packed.is_contiguous()
    sources, count = _frame_sources(frames, params, strides)
    nears = np.ascontiguousarray(near_candidates, dtype=np.int32)
    budgets = np.ascontiguousarray(budgets, dtype=np.uint64)
    assert len(budgets) == count
    offsets = np.zeros(count + 1, dtype=np.uint64)
    sizes = np.zeros(count, dtype=np.uint64)
    chosen = np.zeros(count, dtype=np.int32)
    errcs = np.zeros(count, dtype=np.int32)
    stream = torch.cuda.current_stream(packed.device).cuda_stream
    u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    rc = l.charls_amd_encode_batch_device_ragged_budget(count, sources, budgets.ctypes.data_as(u64p), nears.ctypes.data_as(i32p), len(nears),
                                                        packed.data_ptr(), packed.numel() if capacity is None else int(capacity), alignment,
                                                        offsets.ctypes.data_as(u64p), sizes.ctypes.data_as(u64p), chosen.ctypes.data_as(i32p),
                                                        errcs.ctypes.data_as(i32p), C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_encode_batch_device_ragged_budget")
    return PackedBatch(packed, offsets, sizes, errcs), chosen


def _transcode_budget(call, name, blob_in, offsets, sizes, specs, budgets, near_candidates, packed_out, blob_out, nbytes, alignment, capacity,
                      tail):
    offsets, sizes, count, table, spec_count = _transcode_tables(offsets, sizes, specs)
    nears = np.ascontiguousarray(near_candidates, dtype=np.int32)
    budgets = np.ascontiguousarray(budgets, dtype=np.uint64)
    assert len(budgets) == count
    offsets_out = np.zeros(count + 1, dtype=np.uint64)
    sizes_out = np.zeros(count, dtype=np.uint64)
    chosen = np.zeros(count, dtype=np.int32)
    errcs = np.zeros(count, dtype=np.int32)
    params = (CodecParams * max(count, 1))()
    u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    rc = call(count, blob_in, offsets.ctypes.data_as(u64p), sizes.ctypes.data_as(u64p), table, spec_count, budgets.ctypes.data_as(u64p),
              nears.ctypes.data_as(i32p), len(nears), blob_out, nbytes if capacity is None else int(capacity), alignment,
              offsets_out.ctypes.data_as(u64p), sizes_out.ctypes.data_as(u64p), chosen.ctypes.data_as(i32p), params,
              errcs.ctypes.data_as(i32p), *tail)
    if rc != 0:
        raise capi.JpegLSError(rc, name)
    return TranscodedBatch(packed_out, offsets_out, sizes_out, errcs, params), chosen


def transcode_batch_budget(packed_in, offsets, sizes, specs, budgets, near_candidates, packed_out, *, alignment=1, capacity=None, lib=None):
    """charls_amd_transcode_batch_device_budget: transcode_batch with every frame re-coded at the first NEAR of near_candidates
    -- relative to the DECODED pixels -- whose complete stream has at most budgets[f] bytes; specs must not set NEAR.  Returns
    (TranscodedBatch, nears); nears[f] = -1 for a frame that was not coded."""
    import torch
    l = _bind(lib or capi.load_product())
    assert packed_in.is_cuda and packed_in.is_contiguous() and packed_out.is_cuda and packed_out.is_contiguous()
    stream = torch.cuda.current_stream(packed_in.device).cuda_stream
    return _transcode_budget(l.charls_amd_transcode_batch_device_budget, "charls_amd_transcode_batch_device_budget", packed_in.data_ptr(),
                             offsets, sizes, specs, budgets, near_candidates, packed_out, packed_out.data_ptr(), packed_out.numel(), alignment,
                             capacity, (C.c_void_p(stream),))


def transcode_batch_host_budget(packed_in, offsets, sizes, specs, budgets, near_candidates, packed_out, *, alignment=1, capacity=None, lib=None):
    """charls_amd_transcode_batch_host_budget: transcode_batch_budget with both blobs in HOST memory (numpy arrays or CPU
    tensors, pinned or pageable)."""
    l = _bind(lib or capi.load_product())
    to, nbytes = _host_contiguous(packed_out)
    return _transcode_budget(l.charls_amd_transcode_batch_host_budget, "charls_amd_transcode_batch_host_budget",
                             _host_contiguous(packed_in)[0], offsets, sizes, specs, budgets, near_candidates, packed_out, to, nbytes, alignment,
                             capacity, ())


# ---- the seek-point index on packed streams (charls_amd.h part 2l) ---------------------------------------------------------

def _index_table(count, index_pitch, indexes_out):
    """The host table the indexes of a build go to: (count, pitch) uint8, the caller's own where it brings one."""
    if indexes_out is None:
        return np.zeros((max(count, 1), int(index_pitch)), dtype=np.uint8)
    assert indexes_out.dtype == np.uint8 and indexes_out.ndim == 2 and indexes_out.flags["C_CONTIGUOUS"]
    assert indexes_out.shape[0] >= count and indexes_out.shape[1] == int(index_pitch)
    return indexes_out


def index_pitch_of(params, errcs, lines_per_seek_point, *, lib=None) -> int:
    """The largest charls_amd_index_size_bound of the frames a probe describes (probe_packed / probe_host): an index_pitch
    that holds every frame's index."""
    l = _bind(lib or capi.load_product())
    most = 16
    for f, e in enumerate(errcs):
        if e != 0 or params[f].frame_info.width == 0:
            continue
        out = C.c_size_t(0)
        if l.charls_amd_index_size_bound(C.byref(params[f]), lines_per_seek_point, C.byref(out)) == 0:
            most = max(most, int(out.value))
    return most


def index_batch_packed(packed, offsets, sizes, lines_per_seek_point=64, *, outs=None, strides=None, capacities=None, index_pitch=None,
                       indexes_out=None, lib=None):
    """charls_amd_index_batch_device_packed: the seek-point index of every stream of a packed blob.  outs=None is the
    index-only build (no frame is allocated or written); with outs -- device tensors as decode_batch_ragged takes them --
    the frames are decoded as well.  index_pitch: bytes kept per index (by default what a probe of the blob says the largest
    needs); indexes_out: a (frames, index_pitch) uint8 host array of the caller's to build into.
    Returns (params -- a ctypes array --, errcs, [index bytes]); the index of a frame that failed is b""."""
    import torch
    lib = lib or capi.load_product()
    l = _bind(lib)
    assert packed.is_cuda and packed.is_contiguous()
    offsets, sizes, count = _tables(offsets, sizes)
    if index_pitch is None:
        probed, _, probe_errcs = probe_packed(packed, offsets, sizes, lib=lib)
        index_pitch = index_pitch_of(probed, probe_errcs, lines_per_seek_point, lib=lib)
    assert outs is None or len(outs) == count
    dests = _frame_dests(outs, strides, capacities) if outs is not None else None
    table = _index_table(count, index_pitch, indexes_out)
    index_sizes = np.zeros(max(count, 1), dtype=np.uint64)
    params = (CodecParams * max(count, 1))()
    errcs = np.zeros(count, dtype=np.int32)
    u64p = C.POINTER(C.c_uint64)
    stream = torch.cuda.current_stream(packed.device).cuda_stream
    rc = l.charls_amd_index_batch_device_packed(count, packed.data_ptr(), offsets.ctypes.data_as(u64p), sizes.ctypes.data_as(u64p), dests,
                                                lines_per_seek_point, table.ctypes.data, int(index_pitch), index_sizes.ctypes.data_as(u64p),
                                                params, errcs.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_index_batch_device_packed")
    return params, errcs, [table[f, :int(index_sizes[f])].tobytes() for f in range(count)]


def index_batch_host(packed, offsets, sizes, lines_per_seek_point=64, *, index_pitch=None, indexes_out=None, lib=None):
    """charls_amd_index_batch_host: the index-only build of index_batch_packed with the blob in HOST memory (a numpy array or a
    CPU tensor, pinned or pageable).  Returns (params, errcs, [index bytes])."""
    lib = lib or capi.load_product()
    l = _bind(lib)
    offsets, sizes, count = _tables(offsets, sizes)
    if index_pitch is None:
        probed, _, probe_errcs = probe_host(packed, offsets, sizes, lib=lib)
        index_pitch = index_pitch_of(probed, probe_errcs, lines_per_seek_point, lib=lib)
    table = _index_table(count, index_pitch, indexes_out)
    index_sizes = np.zeros(max(count, 1), dtype=np.uint64)
    params = (CodecParams * max(count, 1))()
    errcs = np.zeros(count, dtype=np.int32)
    u64p = C.POINTER(C.c_uint64)
    rc = l.charls_amd_index_batch_host(count, _host_contiguous(packed)[0], offsets.ctypes.data_as(u64p), sizes.ctypes.data_as(u64p),
                                       lines_per_seek_point, table.ctypes.data, int(index_pitch), index_sizes.ctypes.data_as(u64p), params,
                                       errcs.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_index_batch_host")
    return params, errcs, [table[f, :int(index_sizes[f])].tobytes() for f in range(count)]


def decode_batch_ragged_indexed(packed, offsets, sizes, indexes, outs, *, strides=None, capacities=None, lib=None):
    """charls_amd_decode_batch_device_ragged_indexed: decode_batch_ragged through seek-point indexes (a list of bytes; None or
    b"" = that frame decodes the ordinary way).  Returns (params -- a ctypes array --, errcs)."""
    import torch
    lib = lib or capi.load_product()
    l = _bind(lib)
    assert packed.is_cuda and packed.is_contiguous()
    offsets, sizes, count = _tables(offsets, sizes)
    assert len(outs) == count
    table, pitch, index_sizes = _pack_indexes(indexes, count)
    dests = _frame_dests(outs, strides, capacities)
    params = (CodecParams * max(count, 1))()
    errcs = np.zeros(count, dtype=np.int32)
    u64p = C.POINTER(C.c_uint64)
    stream = torch.cuda.current_stream(packed.device).cuda_stream
    rc = l.charls_amd_decode_batch_device_ragged_indexed(count, packed.data_ptr(), offsets.ctypes.data_as(u64p), sizes.ctypes.data_as(u64p),
                                                         table.ctypes.data, pitch, index_sizes.ctypes.data_as(u64p), dests, params,
                                                         errcs.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_decode_batch_device_ragged_indexed")
    return params, errcs


def decode_rows_batch_ragged(packed, offsets, sizes, indexes, first_rows, row_counts, bands, *, strides=None, capacities=None, lib=None):
    """charls_amd_decode_rows_batch_device_ragged: rows [first_rows[f], first_rows[f] + row_counts[f]) of frame f of the packed
    streams into bands[f], a device tensor of its own (decode_rows' layout), through the frame's index where indexes[f] is
    one, from the top otherwise.  Returns errcs."""
    return _decode_rows_ragged("charls_amd_decode_rows_batch_device_ragged", packed, offsets, sizes, indexes, first_rows, row_counts, bands,
                               strides, capacities, lib)


def decode_rows_batch_ragged_markers(packed, offsets, sizes, indexes, first_rows, row_counts, bands, *, strides=None, capacities=None,
                                     lib=None):
    """charls_amd_decode_rows_batch_device_ragged_markers (part 2m): decode_rows_batch_ragged, with the frames that have restart
    intervals -- and no seek points -- decoded through their restart markers: only the intervals the band meets, all frames'
    in one launch.  Bands and errcs are those of decode_rows_batch_ragged on a stream that decodes whole.  Returns errcs."""
    return _decode_rows_ragged("charls_amd_decode_rows_batch_device_ragged_markers", packed, offsets, sizes, indexes, first_rows, row_counts,
                               bands, strides, capacities, lib)


def _decode_rows_ragged(name, packed, offsets, sizes, indexes, first_rows, row_counts, bands, strides, capacities, lib):
    import torch
    lib = lib or capi.load_product()
    l = _bind(lib)
    assert packed.is_cuda and packed.is_contiguous()
    offsets, sizes, count = _tables(offsets, sizes)
    first_rows = np.ascontiguousarray(first_rows, dtype=np.uint32)
    row_counts = np.ascontiguousarray(row_counts, dtype=np.uint32)
    assert len(first_rows) == count and len(row_counts) == count and len(bands) == count
    table, pitch, index_sizes = _pack_indexes(indexes, count)
    dests = _frame_dests(bands, strides, capacities)
    errcs = np.zeros(count, dtype=np.int32)
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    stream = torch.cuda.current_stream(packed.device).cuda_stream
    rc = getattr(l, name)(count, packed.data_ptr(), offsets.ctypes.data_as(u64p), sizes.ctypes.data_as(u64p), table.ctypes.data, pitch,
                          index_sizes.ctypes.data_as(u64p), first_rows.ctypes.data_as(u32p), row_counts.ctypes.data_as(u32p), dests,
                          errcs.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(stream))
    if rc != 0:
        raise capi.JpegLSError(rc, name)
    return errcs


def measure_counters(lib=None):
    """charls_amd_measure_counters: (scans sized by the measuring kernels, launches of them, scans sized by coding them for
    real), process-wide since the library was loaded."""
    l = _bind(lib or capi.load_product())
    out = (C.c_uint64 * 3)()
    n = l.charls_amd_measure_counters(out, 3)
    assert n == 3
    return tuple(int(out[i]) for i in range(3))


def set_workspace_limit(nbytes: int, lib=None):
    """HBM the library may keep for its work areas (process-wide; 0 = a quarter of the device)."""
    _bind(lib or capi.load_product()).charls_amd_set_workspace_limit(int(nbytes))


def release_work_areas(lib=None):
    """Frees the calling thread's work areas (they are re-allocated on demand)."""
    _bind(lib or capi.load_product()).charls_amd_release_work_areas()


def work_area_bytes(lib=None) -> int:
    return int(_bind(lib or capi.load_product()).charls_amd_work_area_bytes())


def set_encode_engine(engine: int, lib=None):
    """0 automatic, 1 one-wavefront-per-scan kernel, 2 parallel lossless pipeline."""
    rc = _bind(lib or capi.load_product()).charls_amd_set_encode_engine(engine)
    if rc:
        raise capi.JpegLSError(rc, "charls_amd_set_encode_engine")


# ---- multi-GPU: frames are the sharding unit; the only exchange is the final bitstream gather -------------

def encode_batch_devices(frame_shards, stream_shards, *, bits_per_sample=8, gather_to=None, transport=TRANSPORT_AUTO, lib=None):
    """One process, several GPUs (charls_amd_encode_batch_devices): frame_shards[s] / stream_shards[s] are contiguous device
    tensors of shard s on ITS device -- (F_s, H, W) single-component frames and (F_s, pitch) uint8 slots, same H, W and
    pitch everywhere.  gather_to = (root shard index, uint8 device tensor on the root's device): the streams of all shards
    are brought together there, back to back in frame order.  Returns (sizes, errcs, offsets or None, total or None)."""
    lib = lib or capi.load_product()
    l = _bind(lib)
    n = len(frame_shards)
    height, width = frame_shards[0].shape[-2], frame_shards[0].shape[-1]
    frame_pitch = int(np.prod(frame_shards[0].shape[1:])) * frame_shards[0].element_size()
    pitch = stream_shards[0].shape[1]
    shards = (DeviceShard * n)()
    total = 0
    for s in range(n):
        f, st = frame_shards[s], stream_shards[s]
        assert f.is_cuda and f.is_contiguous() and st.is_contiguous() and st.shape[1] == pitch and st.device == f.device
        shards[s] = DeviceShard(f.device.index or 0, f.shape[0], f.data_ptr(), st.data_ptr(), None)
        total += f.shape[0]
    p = CodecParams(capi.FrameInfo(width, height, bits_per_sample, 1), 0, 0, 0, capi.PcParameters(0, 0, 0, 0, 0), 0, 0)
    sizes = np.zeros(total, dtype=np.uint64)
    errcs = np.zeros(total, dtype=np.int32)
    offsets = total_bytes = None
    g = None
    if gather_to is not None:
        root, buf = gather_to
        offsets = np.zeros(total, dtype=np.uint64)
        total_bytes = C.c_uint64(0)
        g = Gather(root, buf.data_ptr(), buf.numel(), offsets.ctypes.data_as(C.POINTER(C.c_uint64)), C.pointer(total_bytes), transport)
    rc = l.charls_amd_encode_batch_devices(C.byref(p), n, shards, frame_pitch, 0, pitch, sizes.ctypes.data_as(C.POINTER(C.c_uint64)),
                                           errcs.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(g) if g is not None else None)
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_encode_batch_devices")
    return sizes, errcs, offsets, (int(total_bytes.value) if total_bytes is not None else None)


def decode_batch_devices(stream_shards, sizes, out_shards, *, lib=None):
    """charls_amd_decode_batch_devices: shard s decodes stream_shards[s] (F_s, pitch) into out_shards[s] on its device."""
    lib = lib or capi.load_product()
    l = _bind(lib)
    n = len(stream_shards)
    shards = (DeviceShard * n)()
    total = 0
    for s in range(n):
        st, o = stream_shards[s], out_shards[s]
        shards[s] = DeviceShard(st.device.index or 0, st.shape[0], o.data_ptr(), st.data_ptr(), None)
        total += st.shape[0]
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    errcs = np.zeros(total, dtype=np.int32)
    p = CodecParams()
    frame_pitch = int(np.prod(out_shards[0].shape[1:])) * out_shards[0].element_size()
    rc = l.charls_amd_decode_batch_devices(n, shards, stream_shards[0].shape[1], sizes.ctypes.data_as(C.POINTER(C.c_uint64)),
                                           frame_pitch, 0, C.byref(p), errcs.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise capi.JpegLSError(rc, "charls_amd_decode_batch_devices")
    return p, errcs


def shard_range(total: int, rank: int, world: int):
    """Contiguous block of frame indices owned by `rank` (sizes differ by at most one)."""
    base, extra = divmod(total, world)
    start = rank * base + min(rank, extra)
    return start, start + base + (1 if rank < extra else 0)


def gather_streams(streams, sizes, dst=0, group=None, chunk_frames=32, sink=None):
    """Variable-length gather of the encoded frames to rank `dst` (RCCL on GPU tensors, gloo on CPU tensors): an all-gather
    of the per-frame byte counts, then the payload point to point in rounds of `chunk_frames` frames per rank -- every
    frame is ONE send of exactly its bytes (`streams[f, :sizes[f]]` is contiguous, nothing is packed, padded or copied on
    the sending side), the sends / receives of a round are posted together (dist.batch_isend_irecv = one ncclGroup), and
    rank dst receives into a buffer per source rank that is re-used from round to round (the payload of a big batch does
    not have to fit rank dst's HBM at once).  `sink(rank, first_frame, tensor, sizes)` is called on dst for every received
    piece (its own frames are handed over as views, they never move); without a sink the pieces are kept and returned.
    Returns on dst: (list of per-rank lists of (first_frame, uint8 tensor (n, >= max size of the piece)), per-rank size
    arrays); elsewhere: (None, per-rank size arrays)."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    dev = streams.device
    counts = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
    dist.all_gather(counts, torch.tensor([len(sizes)], dtype=torch.int64, device=dev), group=group)
    counts = [int(c.item()) for c in counts]
    max_count = max(counts)
    mine = torch.zeros(max(max_count, 1), dtype=torch.int64, device=dev)
    mine[:len(sizes)] = torch.as_tensor(np.asarray(sizes, dtype=np.int64), device=dev)
    all_sizes = [torch.zeros(max(max_count, 1), dtype=torch.int64, device=dev) for _ in range(world)]
    dist.all_gather(all_sizes, mine, group=group)
    all_sizes = [s[:c].cpu().numpy().astype(np.uint64) for s, c in zip(all_sizes, counts)]
    kept = [[] for _ in range(world)] if rank == dst else None
    for first in range(0, max_count, chunk_frames):
        if rank != dst:
            ops = [dist.P2POp(dist.isend, streams[f, :int(sizes[f])], dst, group)
                   for f in range(first, min(first + chunk_frames, len(sizes))) if int(sizes[f]) > 0]
            for req in (dist.batch_isend_irecv(ops) if ops else []):
                req.wait()
            continue
        ops, pieces = [], []
        for r in range(world):
            m = max(0, min(chunk_frames, counts[r] - first))
            if m == 0:
                continue
            sz = all_sizes[r][first:first + m]
            if r == rank:
                pieces.append((r, streams[first:first + m], sz))
                continue
            longest = -(-max(int(sz.max()), 1) // 65536) * 65536  # few distinct buffer sizes -> re-used blocks
            part = torch.empty((m, longest), dtype=torch.uint8, device=dev)
            ops += [dist.P2POp(dist.irecv, part[f, :int(sz[f])], r, group) for f in range(m) if int(sz[f]) > 0]
            pieces.append((r, part, sz))
        for req in (dist.batch_isend_irecv(ops) if ops else []):
            req.wait()
        for r, part, sz in pieces:
            if sink is not None:
                sink(r, first, part, sz)
            else:
                kept[r].append((first, part))
    return kept, all_sizes
