"""The calls of charls_amd.h part 2i (host memory) without a GPU: what they refuse for the whole call is refused before a
device is asked for (the answer is invalid_argument here, where no device exists, not device_unavailable) and writes
nothing, a call without frames succeeds, both library names export the calls, and charls_amd_probe_batch_host_packed -- which
runs on the host alone -- says about every stream under tests/golden what a fresh part-1 decoder says."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import common
from charls_amd import batch, capi

INVALID_ARGUMENT = 101
LIB_DIR = os.path.join(common.ROOT, "charls_amd", "lib")
NAMES = ["charls_amd_host_alloc", "charls_amd_host_free", "charls_amd_host_register", "charls_amd_host_unregister",
         "charls_amd_probe_batch_host_packed", "charls_amd_encode_batch_host_ragged", "charls_amd_decode_batch_host_ragged",
         "charls_amd_encode_batch_host", "charls_amd_decode_batch_host", "charls_amd_host_counters"]

u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def lib():
    return capi.load_product()


@pytest.fixture(scope="module")
def l(lib):
    return batch._bind(lib)


class Tables:
    """Valid host tables and host memory for a call over n frames of 16 x 8."""

    def __init__(self, n):
        self.n = n
        self.offsets = np.full(n + 1, 77, dtype=np.uint64)
        self.sizes = np.full(max(n, 1), 10, dtype=np.uint64)
        self.errcs = np.full(max(n, 1), -1, dtype=np.int32)
        self.bytes = np.zeros(max(n, 1), dtype=np.uint64)
        self.pixels = np.full((max(n, 1), 8, 16), 0x5A, dtype=np.uint8)
        self.packed = np.full(4096, 0xA5, dtype=np.uint8)
        self.params = (batch.CodecParams * max(n, 1))()
        self.sources = (batch.FrameSource * max(n, 1))()
        self.dests = (batch.FrameDest * max(n, 1))()
        for f in range(n):
            self.sources[f] = batch.FrameSource(batch.codec_params(16, 8), self.pixels[f].ctypes.data, 0, 0, 0)
            self.dests[f] = batch.FrameDest(self.pixels[f].ctypes.data, 128, 0, 0)

    def o(self):
        return self.offsets.ctypes.data_as(u64p)

    def s(self):
        return self.sizes.ctypes.data_as(u64p)

    def e(self):
        return self.errcs.ctypes.data_as(i32p)

    def b(self):
        return self.bytes.ctypes.data_as(u64p)

    def p(self):
        return self.packed.ctypes.data

    def untouched(self):
        return bool((self.offsets == 77).all() and (self.errcs == -1).all() and (self.pixels == 0x5A).all() and (self.packed == 0xA5).all())


def test_null_tables(l):
    t = Tables(2)
    probe = [2, t.p(), t.o(), t.s(), t.params, t.b(), t.e()]
    for at in (1, 2, 3, 4, 5, 6):
        args = list(probe)
        args[at] = None
        assert l.charls_amd_probe_batch_host_packed(*args) == INVALID_ARGUMENT, at
    decode = [2, t.p(), t.o(), t.s(), t.dests, t.params, t.e()]
    for at in (1, 2, 3, 4, 6):
        args = list(decode)
        args[at] = None
        assert l.charls_amd_decode_batch_host_ragged(*args) == INVALID_ARGUMENT, at
    encode = [2, t.sources, t.p(), 4096, 1, t.o(), t.s(), t.e()]
    for at in (1, 2, 5, 6, 7):
        args = list(encode)
        args[at] = None
        assert l.charls_amd_encode_batch_host_ragged(*args) == INVALID_ARGUMENT, at
    p = batch.codec_params(16, 8)
    encode = [C.byref(p), 2, t.pixels.ctypes.data, 128, 0, t.p(), 4096, 1, 0, t.o(), t.s(), t.e()]
    for at in (0, 2, 5, 9, 10, 11):
        args = list(encode)
        args[at] = None
        assert l.charls_amd_encode_batch_host(*args) == INVALID_ARGUMENT, at
    decode = [2, t.p(), t.o(), t.s(), t.pixels.ctypes.data, 128, 0, None, t.e()]
    for at in (1, 2, 3, 4, 8):
        args = list(decode)
        args[at] = None
        assert l.charls_amd_decode_batch_host(*args) == INVALID_ARGUMENT, at
    assert t.untouched()  # nothing was done


def test_reserved_and_null_pixels(l):
    for bad in (0, 2):
        t = Tables(3)
        t.sources[bad].reserved = 1
        assert l.charls_amd_encode_batch_host_ragged(3, t.sources, t.p(), 4096, 1, t.o(), t.s(), t.e()) == INVALID_ARGUMENT
        t.dests[bad].reserved = 7
        assert l.charls_amd_decode_batch_host_ragged(3, t.p(), t.o(), t.s(), t.dests, t.params, t.e()) == INVALID_ARGUMENT
        t = Tables(3)
        t.sources[bad].d_pixels = None
        assert l.charls_amd_encode_batch_host_ragged(3, t.sources, t.p(), 4096, 1, t.o(), t.s(), t.e()) == INVALID_ARGUMENT
        t.dests[bad].d_pixels = None  # (with a capacity that is not 0)
        assert l.charls_amd_decode_batch_host_ragged(3, t.p(), t.o(), t.s(), t.dests, t.params, t.e()) == INVALID_ARGUMENT
        assert t.untouched()


@pytest.mark.parametrize("alignment", [0, 3, 8192])
def test_offset_alignment(l, alignment):
    for n in (0, 2):
        t = Tables(n)
        assert l.charls_amd_encode_batch_host_ragged(n, t.sources, t.p(), 4096, alignment, t.o(), t.s(), t.e()) == INVALID_ARGUMENT
        p = batch.codec_params(16, 8)
        assert l.charls_amd_encode_batch_host(C.byref(p), n, t.pixels.ctypes.data, 128, 0, t.p(), 4096, alignment, 0, t.o(), t.s(),
                                              t.e()) == INVALID_ARGUMENT
        assert t.untouched()


def test_no_frames(l):
    t = Tables(0)
    assert l.charls_amd_encode_batch_host_ragged(0, t.sources, None, 0, 16, t.o(), t.s(), t.e()) == 0
    assert t.offsets[0] == 0
    t.offsets[0] = 77
    p = batch.codec_params(16, 8)
    assert l.charls_amd_encode_batch_host(C.byref(p), 0, None, 0, 0, None, 0, 2, 0, t.o(), t.s(), t.e()) == 0
    assert t.offsets[0] == 0
    assert l.charls_amd_decode_batch_host_ragged(0, None, t.o(), t.s(), t.dests, None, t.e()) == 0
    assert l.charls_amd_decode_batch_host(0, None, t.o(), t.s(), None, 0, 0, None, t.e()) == 0
    assert l.charls_amd_probe_batch_host_packed(0, None, t.o(), t.s(), t.params, t.b(), t.e()) == 0
    assert (t.errcs == -1).all()


def test_counters_are_a_plain_host_call(l):
    out = (C.c_uint64 * 9)(*([99] * 9))
    assert l.charls_amd_host_counters(out, 9) == 7 and out[7] == 99
    assert l.charls_amd_host_counters(out, 3) == 3
    assert l.charls_amd_host_counters(None, 7) == 0
    l.charls_amd_host_free(None)  # a no-op


@pytest.mark.parametrize("library", ["libcharls_amd.so", "libcharls.so.3"])
def test_both_library_names_export_the_calls(library):
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB_DIR, library)], capture_output=True, text=True).stdout.split("\n")
    exported = {line.split()[-1] for line in names if line.strip()}
    assert set(NAMES) <= exported


# ---- the probe against part 1 -------------------------------------------------------------------------------------------------

def _streams():
    """Every .jls under tests/golden, and of a few of them truncated and corrupted copies."""
    out = []
    for path in sorted(glob.glob(os.path.join(common.GOLDEN, "**", "*.jls"), recursive=True)):
        with open(path, "rb") as f:
            out.append((os.path.relpath(path, common.GOLDEN), f.read()))
    assert any("abbreviated_tables" in name for name, _ in out)  # the table-only stream: read_header succeeds, no frame
    rng = np.random.default_rng(7)
    for name, data in list(out)[::5]:
        for cut in (0, 1, 2, 3, 11, len(data) // 4):
            out.append((f"{name}[:{cut}]", data[:cut]))
        for _ in range(3):  # a byte of the first 40 -- the marker segments -- set to something else
            at = int(rng.integers(0, min(40, len(data))))
            out.append((f"{name}[{at}]^", data[:at] + bytes([data[at] ^ int(rng.integers(1, 256))]) + data[at + 1:]))
    return out


def _part_one(lib, data):
    """(errc, frame_info tuple, near, interleave mode, destination size) of a fresh part-1 decoder on `data`."""
    L = lib.lib
    dec = L.charls_jpegls_decoder_create()
    try:
        ptr, n, keep = lib._buf(data)  # noqa: F841 (keep: the bytes stay while the decoder looks at them)
        rc = L.charls_jpegls_decoder_set_source_buffer(dec, ptr, n)
        if rc == 0:
            rc = L.charls_jpegls_decoder_read_header(dec)
        if rc != 0:
            return rc, None
        info, size = capi.FrameInfo(), C.c_size_t(0)
        if L.charls_jpegls_decoder_get_frame_info(dec, C.byref(info)) != 0 or info.component_count == 0:
            return 0, None  # (an abbreviated table stream: the header is read, and there is no frame)
        near, mode = C.c_int32(0), C.c_int32(0)
        assert L.charls_jpegls_decoder_get_near_lossless(dec, 0, C.byref(near)) == 0
        assert L.charls_jpegls_decoder_get_interleave_mode(dec, 0, C.byref(mode)) == 0
        assert L.charls_jpegls_decoder_get_destination_size(dec, 0, C.byref(size)) == 0
        return 0, ((info.width, info.height, info.bits_per_sample, info.component_count), near.value, mode.value, size.value)
    finally:
        L.charls_jpegls_decoder_destroy(dec)


def test_probe_says_what_a_part_one_decoder_says(lib):
    streams = _streams()
    offsets, blob = [], bytearray(b"\x00" * 3)  # (odd offsets, streams back to back)
    for _, data in streams:
        offsets.append(len(blob))
        blob += data
    packed = np.frombuffer(bytes(blob) + b"\x00", dtype=np.uint8)
    sizes = [len(data) for _, data in streams]
    params, frame_bytes, errcs = batch.probe_host(packed, offsets, sizes, lib=lib)
    seen = set()
    for f, (name, data) in enumerate(streams):
        rc, frame = _part_one(lib, data)
        assert errcs[f] == rc, name
        fi = params[f].frame_info
        got = ((fi.width, fi.height, fi.bits_per_sample, fi.component_count), params[f].near_lossless, params[f].interleave_mode, int(frame_bytes[f]))
        assert got == (frame if frame is not None else ((0, 0, 0, 0), 0, 0, 0)), name
        seen.add((rc != 0, frame is None))
    assert seen == {(False, False), (False, True), (True, True)}  # frames, the table-only stream, failures
