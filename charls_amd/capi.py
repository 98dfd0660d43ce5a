"""ctypes binding of the CharLS C ABI (``charls_jpegls_encoder_*`` / ``charls_jpegls_decoder_*``).

The binding is library-agnostic on purpose: the same class drives

* ``charls_amd/lib/libcharls_amd.so`` -- this repository's MI355X engine (the product), and
* ``oracle/_ref/libcharls_ref.so``    -- the reference compiled from /root/reference (tests / cpu_baseline only),

because both export the interface declared in the reference's ``include/charls/charls_jpegls_encoder.h:24-316`` and
``include/charls/charls_jpegls_decoder.h:24-293``.  The Python classes mirror the reference's header-only C++ wrappers
(``include/charls/jpegls_encoder.hpp:58-449``, ``jpegls_decoder.hpp:108-570``): same method names, same argument
meaning, errors surface as :class:`JpegLSError` carrying the ``charls_jpegls_errc`` value.

There is no CPU fallback here: if the product library is missing, :func:`load_product` raises.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCT_LIB = os.path.join(_HERE, "lib", "libcharls_amd.so")


class JpegLSError(RuntimeError):
    def __init__(self, errc: int, where: str = ""):
        self.errc = int(errc)
        super().__init__(f"charls_jpegls_errc={self.errc} in {where}")


class FrameInfo(C.Structure):  # include/charls/public_types.h:983-1000 (16 bytes)
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("bits_per_sample", C.c_int32),
                ("component_count", C.c_int32)]


class PcParameters(C.Structure):  # include/charls/public_types.h:1003-1021 (20 bytes)
    _fields_ = [("maximum_sample_value", C.c_int32), ("threshold1", C.c_int32), ("threshold2", C.c_int32),
                ("threshold3", C.c_int32), ("reset_value", C.c_int32)]


class SpiffHeader(C.Structure):  # include/charls/public_types.h:934-980 (40 bytes)
    _fields_ = [("profile_id", C.c_int32), ("component_count", C.c_int32), ("height", C.c_uint32),
                ("width", C.c_uint32), ("color_space", C.c_int32), ("bits_per_sample", C.c_int32),
                ("compression_type", C.c_int32), ("resolution_units", C.c_int32),
                ("vertical_resolution", C.c_uint32), ("horizontal_resolution", C.c_uint32)]


class SalvageReport(C.Structure):  # charls_amd_salvage_report (include/charls_amd.h part 2g; product library only)
    _fields_ = [("state", C.c_uint32), ("intervals", C.c_uint32), ("intervals_lost", C.c_uint32), ("rows_lost", C.c_uint32),
                ("first_lost_row", C.c_uint32), ("reserved", C.c_uint32)]

    def astuple(self):
        return (self.state, self.intervals, self.intervals_lost, self.rows_lost, self.first_lost_row, self.reserved)


TRANSCODE_NEAR, TRANSCODE_RESTART_INTERVAL, TRANSCODE_PRESET, TRANSCODE_ENCODING_OPTIONS = 1, 2, 4, 8


class TranscodeSpec(C.Structure):  # charls_amd_transcode_spec (include/charls_amd.h part 2j; product library only)
    _fields_ = [("set", C.c_uint32), ("near_lossless", C.c_int32), ("restart_interval", C.c_uint32),
                ("preset_coding_parameters", PcParameters), ("encoding_options", C.c_uint32), ("reserved", C.c_uint32)]


def transcode_spec(near_lossless=None, restart_interval=None, preset=None, encoding_options=None) -> TranscodeSpec:
    """A spec that replaces exactly the fields given (None: the source stream's value stays)."""
    s = TranscodeSpec()
    if near_lossless is not None:
        s.set |= TRANSCODE_NEAR
        s.near_lossless = int(near_lossless)
    if restart_interval is not None:
        s.set |= TRANSCODE_RESTART_INTERVAL
        s.restart_interval = int(restart_interval)
    if preset is not None:
        s.set |= TRANSCODE_PRESET
        s.preset_coding_parameters = PcParameters(*preset)
    if encoding_options is not None:
        s.set |= TRANSCODE_ENCODING_OPTIONS
        s.encoding_options = int(encoding_options)
    return s


class MappingTableInfo(C.Structure):  # include/charls/public_types.h:1024-1034 (12 bytes)
    _fields_ = [("table_id", C.c_int32), ("entry_size", C.c_int32), ("data_size", C.c_uint32)]


ENCODER_SYMBOLS = [
    "create", "destroy", "set_frame_info", "set_near_lossless", "set_encoding_options", "set_interleave_mode",
    "set_preset_coding_parameters", "set_color_transformation", "set_mapping_table_id",
    "get_estimated_destination_size", "set_destination_buffer", "write_standard_spiff_header", "write_spiff_header",
    "write_spiff_entry", "write_spiff_end_of_directory_entry", "write_comment", "write_application_data",
    "write_mapping_table", "encode_from_buffer", "encode_components_from_buffer", "create_abbreviated_format",
    "get_bytes_written", "rewind"]
DECODER_SYMBOLS = [
    "create", "destroy", "set_source_buffer", "read_spiff_header", "read_header", "get_frame_info",
    "get_near_lossless", "get_interleave_mode", "get_preset_coding_parameters", "get_color_transformation",
    "get_destination_size", "decode_to_buffer", "at_comment", "at_application_data"]
DECODER_SYMBOLS2 = [
    "get_compressed_data_format", "get_mapping_table_id", "find_mapping_table_index", "get_mapping_table_count",
    "get_mapping_table_info", "get_mapping_table_data"]
MISC_SYMBOLS = ["charls_get_error_message", "charls_get_jpegls_category", "charls_get_version_string",
                "charls_get_version_number", "charls_validate_spiff_header"]


def all_abi_symbols() -> list[str]:
    """The 48 exported names of the reference (src/charls.version:1-21)."""
    return ([f"charls_jpegls_encoder_{s}" for s in ENCODER_SYMBOLS] +
            [f"charls_jpegls_decoder_{s}" for s in DECODER_SYMBOLS] +
            [f"charls_decoder_{s}" for s in DECODER_SYMBOLS2] + MISC_SYMBOLS)


@dataclass
class Header:
    width: int
    height: int
    bits_per_sample: int
    component_count: int
    near_lossless: int
    interleave_mode: int
    color_transformation: int
    preset: tuple


class CharLSLibrary:
    """One loaded implementation of the CharLS C ABI."""

    def __init__(self, path: str):
        if not os.path.exists(path):
            raise FileNotFoundError(f"CharLS-ABI library not found: {path}")
        self.path = path
        self.lib = C.CDLL(path)
        L = self.lib
        vp, sz, u32, i32 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int32
        L.charls_jpegls_encoder_create.restype = vp
        L.charls_jpegls_encoder_destroy.argtypes = [vp]
        L.charls_jpegls_encoder_destroy.restype = None
        L.charls_jpegls_decoder_create.restype = vp
        L.charls_jpegls_decoder_destroy.argtypes = [vp]
        L.charls_jpegls_decoder_destroy.restype = None
        sig = {
            "charls_jpegls_encoder_set_frame_info": [vp, C.POINTER(FrameInfo)],
            "charls_jpegls_encoder_set_near_lossless": [vp, i32],
            "charls_jpegls_encoder_set_encoding_options": [vp, u32],
            "charls_jpegls_encoder_set_interleave_mode": [vp, i32],
            "charls_jpegls_encoder_set_preset_coding_parameters": [vp, C.POINTER(PcParameters)],
            "charls_jpegls_encoder_set_color_transformation": [vp, i32],
            "charls_jpegls_encoder_set_mapping_table_id": [vp, i32, i32],
            "charls_jpegls_encoder_get_estimated_destination_size": [vp, C.POINTER(sz)],
            "charls_jpegls_encoder_set_destination_buffer": [vp, vp, sz],
            "charls_jpegls_encoder_write_standard_spiff_header": [vp, i32, i32, u32, u32],
            "charls_jpegls_encoder_write_spiff_header": [vp, C.POINTER(SpiffHeader)],
            "charls_jpegls_encoder_write_spiff_entry": [vp, u32, vp, sz],
            "charls_jpegls_encoder_write_spiff_end_of_directory_entry": [vp],
            "charls_jpegls_encoder_write_comment": [vp, vp, sz],
            "charls_jpegls_encoder_write_application_data": [vp, i32, vp, sz],
            "charls_jpegls_encoder_write_mapping_table": [vp, i32, i32, vp, sz],
            "charls_jpegls_encoder_encode_from_buffer": [vp, vp, sz, u32],
            "charls_jpegls_encoder_encode_components_from_buffer": [vp, vp, sz, i32, u32],
            "charls_jpegls_encoder_create_abbreviated_format": [vp],
            "charls_jpegls_encoder_get_bytes_written": [vp, C.POINTER(sz)],
            "charls_jpegls_encoder_rewind": [vp],
            "charls_jpegls_decoder_set_source_buffer": [vp, vp, sz],
            "charls_jpegls_decoder_read_spiff_header": [vp, C.POINTER(SpiffHeader), C.POINTER(i32)],
            "charls_jpegls_decoder_read_header": [vp],
            "charls_jpegls_decoder_get_frame_info": [vp, C.POINTER(FrameInfo)],
            "charls_jpegls_decoder_get_near_lossless": [vp, i32, C.POINTER(i32)],
            "charls_jpegls_decoder_get_interleave_mode": [vp, i32, C.POINTER(i32)],
            "charls_jpegls_decoder_get_preset_coding_parameters": [vp, i32, C.POINTER(PcParameters)],
            "charls_jpegls_decoder_get_color_transformation": [vp, C.POINTER(i32)],
            "charls_jpegls_decoder_get_destination_size": [vp, u32, C.POINTER(sz)],
            "charls_jpegls_decoder_decode_to_buffer": [vp, vp, sz, u32],
            "charls_jpegls_decoder_at_comment": [vp, vp, vp],
            "charls_jpegls_decoder_at_application_data": [vp, vp, vp],
            "charls_decoder_get_compressed_data_format": [vp, C.POINTER(i32)],
            "charls_decoder_get_mapping_table_id": [vp, i32, C.POINTER(i32)],
            "charls_decoder_find_mapping_table_index": [vp, i32, C.POINTER(i32)],
            "charls_decoder_get_mapping_table_count": [vp, C.POINTER(i32)],
            "charls_decoder_get_mapping_table_info": [vp, i32, C.POINTER(MappingTableInfo)],
            "charls_decoder_get_mapping_table_data": [vp, i32, vp, sz],
            "charls_validate_spiff_header": [C.POINTER(SpiffHeader), C.POINTER(FrameInfo)],
        }
        for name, argtypes in sig.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = i32
        L.charls_get_error_message.argtypes = [i32]
        L.charls_get_error_message.restype = C.c_char_p
        L.charls_get_version_string.restype = C.c_char_p
        L.charls_get_version_number.argtypes = [C.POINTER(i32)] * 3
        L.charls_get_version_number.restype = None

    # -- helpers -----------------------------------------------------------------------------------------------
    def _check(self, rc: int, where: str):
        if rc != 0:
            raise JpegLSError(rc, where)

    @staticmethod
    def _buf(a):
        """(pointer, nbytes, keepalive) of a bytes-like / ndarray."""
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a)
            return a.ctypes.data, a.nbytes, a
        b = (C.c_ubyte * len(a)).from_buffer_copy(bytes(a))
        return C.addressof(b), len(a), b

    def error_message(self, errc: int) -> str:
        return self.lib.charls_get_error_message(errc).decode()

    # -- jpegls_encoder::encode convenience (include/charls/jpegls_encoder.hpp:58-110) --------------------------
    def encode(self, image, *, width=None, height=None, bits_per_sample=8, component_count=1, near_lossless=0,
               interleave_mode=0, color_transformation=0, preset=None, encoding_options=0, stride=0,
               destination_size=None, restart_interval=0, destination=None):
        """Encode `image` (ndarray or bytes, user layout of SURVEY 8a row a20) to a .jls byte string.
        restart_interval != 0 uses charls_amd_jpegls_encoder_set_restart_interval (product library only).
        destination: a preallocated uint8 ndarray to encode into -- the methodology of the reference's cli/benchmark.cpp:60-90
        (destination allocated outside the measurement loop, handle inside); the result is then a VIEW of it, not a copy."""
        L = self.lib
        if isinstance(image, np.ndarray) and (width is None or height is None):
            if interleave_mode == 0 and component_count > 1:
                height, width = image.shape[1], image.shape[2]
            else:
                height, width = image.shape[0], image.shape[1]
        enc = L.charls_jpegls_encoder_create()
        if not enc:
            raise MemoryError
        try:
            fi = FrameInfo(width, height, bits_per_sample, component_count)
            self._check(L.charls_jpegls_encoder_set_frame_info(enc, C.byref(fi)), "set_frame_info")
            self._check(L.charls_jpegls_encoder_set_near_lossless(enc, near_lossless), "set_near_lossless")
            self._check(L.charls_jpegls_encoder_set_interleave_mode(enc, interleave_mode), "set_interleave_mode")
            if color_transformation:
                self._check(L.charls_jpegls_encoder_set_color_transformation(enc, color_transformation),
                            "set_color_transformation")
            if encoding_options:
                self._check(L.charls_jpegls_encoder_set_encoding_options(enc, encoding_options),
                            "set_encoding_options")
            if preset is not None:
                pc = PcParameters(*preset)
                self._check(L.charls_jpegls_encoder_set_preset_coding_parameters(enc, C.byref(pc)), "set_pc")
            if restart_interval:
                fn = L.charls_amd_jpegls_encoder_set_restart_interval
                fn.argtypes = [C.c_void_p, C.c_uint32]
                fn.restype = C.c_int32
                self._check(fn(enc, restart_interval), "set_restart_interval")
            if destination_size is None:
                n = C.c_size_t()
                self._check(L.charls_jpegls_encoder_get_estimated_destination_size(enc, C.byref(n)), "estimate")
                destination_size = n.value
            dst = destination if destination is not None else np.empty(destination_size, dtype=np.uint8)
            self._check(L.charls_jpegls_encoder_set_destination_buffer(enc, dst.ctypes.data, dst.nbytes), "set_dest")
            ptr, nbytes, keep = self._buf(image)
            self._check(L.charls_jpegls_encoder_encode_from_buffer(enc, ptr, nbytes, stride), "encode_from_buffer")
            n = C.c_size_t()
            self._check(L.charls_jpegls_encoder_get_bytes_written(enc, C.byref(n)), "get_bytes_written")
            del keep
            return dst[:n.value] if destination is not None else dst[:n.value].tobytes()
        finally:
            L.charls_jpegls_encoder_destroy(enc)

    # -- jpegls_decoder::decode convenience (include/charls/jpegls_decoder.hpp:108-180) --------------------------
    def read_header(self, data) -> Header:
        L = self.lib
        dec = L.charls_jpegls_decoder_create()
        try:
            ptr, n, keep = self._buf(data)
            self._check(L.charls_jpegls_decoder_set_source_buffer(dec, ptr, n), "set_source_buffer")
            self._check(L.charls_jpegls_decoder_read_header(dec), "read_header")
            return self._header(dec)
        finally:
            L.charls_jpegls_decoder_destroy(dec)

    def _header(self, dec) -> Header:
        L = self.lib
        fi = FrameInfo()
        self._check(L.charls_jpegls_decoder_get_frame_info(dec, C.byref(fi)), "get_frame_info")
        near, ilv, ct = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(L.charls_jpegls_decoder_get_near_lossless(dec, 0, C.byref(near)), "get_near")
        self._check(L.charls_jpegls_decoder_get_interleave_mode(dec, 0, C.byref(ilv)), "get_ilv")
        self._check(L.charls_jpegls_decoder_get_color_transformation(dec, C.byref(ct)), "get_ct")
        pc = PcParameters()
        self._check(L.charls_jpegls_decoder_get_preset_coding_parameters(dec, 0, C.byref(pc)), "get_pc")
        return Header(fi.width, fi.height, fi.bits_per_sample, fi.component_count, near.value, ilv.value, ct.value,
                      (pc.maximum_sample_value, pc.threshold1, pc.threshold2, pc.threshold3, pc.reset_value))

    def decode(self, data, stride=0, destination_size=None, out=None, index=None):
        """Decode a .jls byte string. Returns (Header, uint8 ndarray of the raw destination bytes).
        out: a preallocated uint8 ndarray to decode into (cli/benchmark.cpp:40-55: allocated outside the loop).
        index: a seek-point index of this stream (decode_with_index; product library only): decode through it."""
        if index is not None:
            return self.decode_indexed(data, index, stride)
        L = self.lib
        dec = L.charls_jpegls_decoder_create()
        if not dec:
            raise MemoryError
        try:
            ptr, n, keep = self._buf(data)
            self._check(L.charls_jpegls_decoder_set_source_buffer(dec, ptr, n), "set_source_buffer")
            self._check(L.charls_jpegls_decoder_read_header(dec), "read_header")
            hdr = self._header(dec)
            if destination_size is None:
                sz = C.c_size_t()
                self._check(L.charls_jpegls_decoder_get_destination_size(dec, stride, C.byref(sz)), "get_dest_size")
                destination_size = sz.value
            if out is None:
                out = np.zeros(destination_size, dtype=np.uint8)
            self._check(L.charls_jpegls_decoder_decode_to_buffer(dec, out.ctypes.data, out.nbytes, stride),
                        "decode_to_buffer")
            del keep
            return hdr, out
        finally:
            L.charls_jpegls_decoder_destroy(dec)

    # -- seek-point index (charls_amd_jpegls_decoder_*index*, decode_rows; product library only) ------------------------
    def _index_fns(self):
        L, vp, sz, u32, i32 = self.lib, C.c_void_p, C.c_size_t, C.c_uint32, C.c_int32
        if getattr(self, "_index_ready", False):
            return L
        for name, args in (("charls_amd_jpegls_decoder_get_index_size", [vp, u32, C.POINTER(sz)]),
                           ("charls_amd_jpegls_decoder_decode_to_buffer_and_index", [vp, vp, sz, u32, u32, vp, sz, C.POINTER(sz)]),
                           ("charls_amd_jpegls_decoder_set_index", [vp, vp, sz]),
                           ("charls_amd_jpegls_decoder_decode_rows", [vp, u32, u32, vp, sz, u32])):
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = i32
        self._index_ready = True
        return L

    def _open(self, data):
        L = self.lib
        dec = L.charls_jpegls_decoder_create()
        if not dec:
            raise MemoryError
        ptr, n, keep = self._buf(data)
        try:
            self._check(L.charls_jpegls_decoder_set_source_buffer(dec, ptr, n), "set_source_buffer")
            self._check(L.charls_jpegls_decoder_read_header(dec), "read_header")
        except Exception:
            L.charls_jpegls_decoder_destroy(dec)
            raise
        return dec, keep

    def set_index(self, dec, index):
        L = self._index_fns()
        iptr, ilen, ikeep = self._buf(index)
        self._check(L.charls_amd_jpegls_decoder_set_index(dec, iptr, ilen), "set_index")
        del ikeep

    def decode_with_index(self, data, lines_per_seek_point=64, stride=0):
        """decode_to_buffer that also builds the seek-point index: (Header, raw destination bytes, index bytes)."""
        L = self._index_fns()
        dec, keep = self._open(data)
        try:
            hdr = self._header(dec)
            sz = C.c_size_t()
            self._check(L.charls_jpegls_decoder_get_destination_size(dec, stride, C.byref(sz)), "get_dest_size")
            out = np.zeros(sz.value, dtype=np.uint8)
            isz = C.c_size_t()
            self._check(L.charls_amd_jpegls_decoder_get_index_size(dec, lines_per_seek_point, C.byref(isz)), "get_index_size")
            index = np.zeros(max(isz.value, 1), dtype=np.uint8)
            written = C.c_size_t()
            self._check(L.charls_amd_jpegls_decoder_decode_to_buffer_and_index(
                dec, out.ctypes.data, out.nbytes, stride, lines_per_seek_point, index.ctypes.data, isz.value, C.byref(written)),
                "decode_to_buffer_and_index")
            del keep
            return hdr, out, index[:written.value].tobytes()
        finally:
            L.charls_jpegls_decoder_destroy(dec)

    def decode_indexed(self, data, index, stride=0):
        """decode_to_buffer through a seek-point index (set_index first): (Header, raw destination bytes)."""
        L = self._index_fns()
        dec, keep = self._open(data)
        try:
            hdr = self._header(dec)
            self.set_index(dec, index)
            sz = C.c_size_t()
            self._check(L.charls_jpegls_decoder_get_destination_size(dec, stride, C.byref(sz)), "get_dest_size")
            out = np.zeros(sz.value, dtype=np.uint8)
            self._check(L.charls_jpegls_decoder_decode_to_buffer(dec, out.ctypes.data, out.nbytes, stride), "decode_to_buffer")
            del keep
            return hdr, out
        finally:
            L.charls_jpegls_decoder_destroy(dec)

    def decode_salvage(self, data, fill_value=0, stride=0, status_capacity=None):
        """charls_amd_jpegls_decoder_decode_to_buffer_salvage (product library only): (Header, raw destination bytes,
        SalvageReport, status bytes, errc).  errc is what decode_to_buffer returns; with report.state == 1 the destination holds
        the intact restart intervals and fill_value elsewhere.  status_capacity: room for the status bytes (default: enough)."""
        L = self.lib
        fn = L.charls_amd_jpegls_decoder_decode_to_buffer_salvage
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(SalvageReport), C.c_void_p, C.c_size_t]
        fn.restype = C.c_int32
        dec, keep = self._open(data)
        try:
            hdr = self._header(dec)
            sz = C.c_size_t()
            self._check(L.charls_jpegls_decoder_get_destination_size(dec, stride, C.byref(sz)), "get_dest_size")
            out = np.zeros(sz.value, dtype=np.uint8)
            if status_capacity is None:
                status_capacity = hdr.component_count * hdr.height
            status = np.full(max(status_capacity, 1), 0xFF, dtype=np.uint8)
            report = SalvageReport()
            rc = fn(dec, out.ctypes.data, out.nbytes, stride, fill_value, C.byref(report), status.ctypes.data, status_capacity)
            del keep
            return hdr, out, report, status[:status_capacity], rc
        finally:
            L.charls_jpegls_decoder_destroy(dec)

    def decode_salvage_indexed(self, data, index=None, fill_value=0, flags=0, stride=0, status_capacity=None):
        """charls_amd_jpegls_decoder_decode_to_buffer_salvage_indexed (product library only), after set_index where `index`
        is given: (Header, raw destination bytes, SalvageReport, status bytes, errc).  With report.state 1 or 3 the
        destination holds the salvaged frame."""
        L = self._index_fns()
        fn = L.charls_amd_jpegls_decoder_decode_to_buffer_salvage_indexed
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(SalvageReport), C.c_void_p,
                       C.c_size_t]
        fn.restype = C.c_int32
        dec, keep = self._open(data)
        try:
            hdr = self._header(dec)
            if index is not None:
                self.set_index(dec, index)
            sz = C.c_size_t()
            self._check(L.charls_jpegls_decoder_get_destination_size(dec, stride, C.byref(sz)), "get_dest_size")
            out = np.zeros(sz.value, dtype=np.uint8)
            if status_capacity is None:
                status_capacity = hdr.component_count * hdr.height
            status = np.full(max(status_capacity, 1), 0xFF, dtype=np.uint8)
            report = SalvageReport()
            rc = fn(dec, out.ctypes.data, out.nbytes, stride, fill_value, flags, C.byref(report), status.ctypes.data, status_capacity)
            del keep
            return hdr, out, report, status[:status_capacity], rc
        finally:
            L.charls_jpegls_decoder_destroy(dec)

    def decode_rows(self, data, first_row, row_count, index=None, stride=0):
        """Rows [first_row, first_row + row_count) in decode_to_buffer's layout for a frame of row_count rows (planar
        frames: one band per component).  With `index`, from the seek point at or before first_row."""
        L = self._index_fns()
        dec, keep = self._open(data)
        try:
            hdr = self._header(dec)
            if index is not None:
                self.set_index(dec, index)
            bps = (hdr.bits_per_sample + 7) // 8
            row = hdr.width * bps * (hdr.component_count if hdr.interleave_mode != 0 else 1)
            st = stride or row
            scans = hdr.component_count if hdr.interleave_mode == 0 else 1
            out = np.zeros(st * row_count * scans - (st - row), dtype=np.uint8)
            self._check(L.charls_amd_jpegls_decoder_decode_rows(dec, first_row, row_count, out.ctypes.data, out.nbytes, stride),
                        "decode_rows")
            del keep
            return out
        finally:
            L.charls_jpegls_decoder_destroy(dec)


_product = None


def load_product() -> CharLSLibrary:
    """Load this repository's engine. Raises if it has not been built -- there is no fallback."""
    global _product
    if _product is None:
        if not os.path.exists(PRODUCT_LIB):
            raise RuntimeError(
                f"{PRODUCT_LIB} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). charls_amd has no CPU fallback.")
        if "torch" not in sys.modules:
            # torch brings a HIP runtime of its own under the SONAME this library links (/opt/rocm's libamdhip64); the one
            # that is loaded first serves both, and torch does not find its device on the other one.  Every Python user of
            # this binding (tests, bench, tools) uses torch for device memory sooner or later: it goes first.
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        _product = CharLSLibrary(PRODUCT_LIB)
    return _product


KNOB_UNSET = -(1 << 63)


def set_knob(name: str, value, lib: CharLSLibrary | None = None) -> None:
    """charls_amd_debug_set_knob: a test / measurement knob of the engine (charls_amd/csrc/device/knobs.h); value None clears
    it.  The environment variables of the same names are read once, when the library first looks at a knob."""
    L = (lib or load_product()).lib
    L.charls_amd_debug_set_knob.argtypes = [C.c_char_p, C.c_int64]
    L.charls_amd_debug_set_knob.restype = C.c_int32
    rc = L.charls_amd_debug_set_knob(name.encode(), KNOB_UNSET if value is None else int(value))
    if rc != 0:
        raise JpegLSError(rc, f"charls_amd_debug_set_knob({name})")


def engine_counters(lib: CharLSLibrary | None = None) -> dict:
    """charls_amd_engine_counters: what the coalescer of the host-pointer ABI did, and pipeline scans without a work area."""
    L = (lib or load_product()).lib
    L.charls_amd_engine_counters.argtypes = [C.POINTER(C.c_uint64), C.c_int32]
    L.charls_amd_engine_counters.restype = C.c_int32
    out = (C.c_uint64 * 10)()
    n = L.charls_amd_engine_counters(out, 10)
    assert n >= 5
    names = ("calls", "launches", "merged_calls", "largest_launch", "pipeline_fallback_scans", "split_launches", "idle_pool_bytes",
             "deferred_free_bytes", "idle_releases", "exact_retry_scans")
    return dict(zip(names[:n], (int(v) for v in out[:n])))


def index_counters(lib: CharLSLibrary | None = None) -> dict:
    """charls_amd_index_counters: scans decoded from seek points, wavefronts launched from them, scans whose index did not
    hold and that were decoded from the top."""
    L = (lib or load_product()).lib
    L.charls_amd_index_counters.argtypes = [C.POINTER(C.c_uint64), C.c_int32]
    L.charls_amd_index_counters.restype = C.c_int32
    out = (C.c_uint64 * 3)()
    n = L.charls_amd_index_counters(out, 3)
    return dict(zip(("scans_from_points", "intervals", "fallback_scans")[:n], (int(v) for v in out[:n])))


def transcode_counters(lib: CharLSLibrary | None = None) -> tuple:
    """charls_amd_transcode_counters: (frames re-coded, windows, frames refused for a mapping table, frames behind the one that
    met the capacity), process-wide since the library was loaded.  The calls themselves: batch.transcode_batch / _host and, to a
    byte budget (part 2k), batch.transcode_batch_budget / _host_budget."""
    L = (lib or load_product()).lib
    L.charls_amd_transcode_counters.argtypes = [C.POINTER(C.c_uint64), C.c_int32]
    L.charls_amd_transcode_counters.restype = C.c_int32
    out = (C.c_uint64 * 4)()
    n = L.charls_amd_transcode_counters(out, 4)
    assert n == 4
    return tuple(int(v) for v in out)


def band_marker_counters(lib: CharLSLibrary | None = None) -> dict:
    """charls_amd_band_marker_counters (part 2m): frames that took the marker route of batch.decode_rows_batch_ragged_markers,
    intervals decoded on it, frames that fell back after starting it, launches it made; process-wide."""
    L = (lib or load_product()).lib
    L.charls_amd_band_marker_counters.argtypes = [C.POINTER(C.c_uint64), C.c_int32]
    L.charls_amd_band_marker_counters.restype = C.c_int32
    out = (C.c_uint64 * 4)()
    n = L.charls_amd_band_marker_counters(out, 4)
    assert n == 4
    return dict(zip(("frames", "intervals", "fallback_frames", "launches"), (int(v) for v in out)))
