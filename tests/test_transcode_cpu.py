"""The calls of charls_amd.h part 2j (re-coding a packed blob) without a GPU: what they refuse for the whole call is refused
before a device is asked for -- the answer is the code itself here, where no device exists, not device_unavailable -- and writes
nothing, a call without frames succeeds, the counters do not move, and both library names export the calls."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import common
from charls_amd import batch, capi

INVALID_ARGUMENT, INVALID_ARGUMENT_SIZE = 101, 110
LIB_DIR = os.path.join(common.ROOT, "charls_amd", "lib")
NAMES = ["charls_amd_transcode_batch_device", "charls_amd_transcode_batch_host", "charls_amd_transcode_counters"]

u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def lib():
    return capi.load_product()


@pytest.fixture(scope="module")
def l(lib):
    return batch._bind(lib)


class Tables:
    """Valid host tables for a call over n frames, every output filled with a canary.  The blobs are host memory: the device
    form only looks at the pointers for NULL before it asks for a device."""

    def __init__(self, n, spec_count=1):
        self.n = n
        self.offsets_in = np.arange(max(n, 1), dtype=np.uint64) * 100
        self.sizes_in = np.full(max(n, 1), 100, dtype=np.uint64)
        self.specs = (capi.TranscodeSpec * max(spec_count, 1))()
        for k in range(spec_count):
            self.specs[k] = capi.transcode_spec(restart_interval=8)
        self.spec_count = spec_count
        self.blob_in = np.full(4096, 0x3C, dtype=np.uint8)
        self.blob_out = np.full(4096, 0xA5, dtype=np.uint8)
        self.offsets_out = np.full(n + 1, 77, dtype=np.uint64)
        self.sizes_out = np.full(max(n, 1), 78, dtype=np.uint64)
        self.errcs = np.full(max(n, 1), -1, dtype=np.int32)
        self.params = (batch.CodecParams * max(n, 1))()
        for f in range(max(n, 1)):
            self.params[f].near_lossless = 79

    def args(self, alignment=1):
        return [self.n, self.blob_in.ctypes.data, self.offsets_in.ctypes.data_as(u64p), self.sizes_in.ctypes.data_as(u64p), self.specs,
                self.spec_count, self.blob_out.ctypes.data, self.blob_out.nbytes, alignment, self.offsets_out.ctypes.data_as(u64p),
                self.sizes_out.ctypes.data_as(u64p), self.params, self.errcs.ctypes.data_as(i32p)]

    def untouched(self):
        return bool((self.offsets_out == 77).all() and (self.sizes_out == 78).all() and (self.errcs == -1).all() and
                    (self.blob_out == 0xA5).all() and (self.blob_in == 0x3C).all() and
                    all(self.params[f].near_lossless == 79 for f in range(max(self.n, 1))))


def both(l, t, alignment=1):
    """The device form and the host form on the same arguments: the code both return."""
    args = t.args(alignment)
    device = l.charls_amd_transcode_batch_device(*args, None)
    host = l.charls_amd_transcode_batch_host(*args)
    assert device == host, (device, host)
    return device


def counters(l):
    out = (C.c_uint64 * 4)()
    assert l.charls_amd_transcode_counters(out, 4) == 4
    return tuple(out)


def test_null_tables_and_blobs(l):
    before = counters(l)
    for at in (1, 2, 3, 4, 6, 9, 10, 11, 12):
        t = Tables(2)
        args = t.args()
        args[at] = None
        assert l.charls_amd_transcode_batch_device(*args, None) == INVALID_ARGUMENT, at
        assert l.charls_amd_transcode_batch_host(*args) == INVALID_ARGUMENT, at
        assert t.untouched(), at
    assert counters(l) == before


@pytest.mark.parametrize("frames, spec_count", [(3, 0), (3, 2), (3, 4), (2, 3), (0, 2)])
def test_spec_count_is_one_or_the_frame_count(l, frames, spec_count):
    t = Tables(frames, spec_count)
    assert both(l, t) == INVALID_ARGUMENT
    assert t.untouched()


@pytest.mark.parametrize("bit", [16, 32, 1 << 31])
def test_an_undefined_set_bit(l, bit):
    for spec_count, bad in ((1, 0), (3, 0), (3, 2)):
        t = Tables(3, spec_count)
        t.specs[bad].set |= bit
        assert both(l, t) == INVALID_ARGUMENT
        assert t.untouched()


def test_reserved_must_be_zero(l):
    for spec_count, bad in ((1, 0), (3, 1), (3, 2)):
        t = Tables(3, spec_count)
        t.specs[bad].reserved = 1
        assert both(l, t) == INVALID_ARGUMENT
        assert t.untouched()


@pytest.mark.parametrize("alignment", [0, 3, 24, 8192])
def test_offset_alignment(l, alignment):
    for n in (0, 2):
        t = Tables(n)
        assert both(l, t, alignment) == INVALID_ARGUMENT
        assert t.untouched()


def test_an_offset_plus_size_that_overflows(l):
    for bad in (0, 2):
        t = Tables(3)
        t.offsets_in[bad] = (1 << 64) - 50
        assert both(l, t) == INVALID_ARGUMENT_SIZE
        assert t.untouched()


def test_no_frames_is_success(l):
    before = counters(l)
    for spec_count in (0, 1):
        t = Tables(0, spec_count)
        args = t.args(16)
        args[1] = args[6] = None  # (no frames: no blobs)
        args[7] = 0
        assert l.charls_amd_transcode_batch_device(*args, None) == 0
        assert t.offsets_out[0] == 0
        t.offsets_out[0] = 77
        assert l.charls_amd_transcode_batch_host(*args) == 0
        assert t.offsets_out[0] == 0
        assert (t.errcs == -1).all() and (t.sizes_out == 78).all()
    assert counters(l) == before


def test_counters_are_a_plain_host_call(l, lib):
    out = (C.c_uint64 * 6)(*([99] * 6))
    assert l.charls_amd_transcode_counters(out, 6) == 4 and out[4] == 99
    assert l.charls_amd_transcode_counters(out, 2) == 2
    assert l.charls_amd_transcode_counters(None, 4) == 0
    assert len(capi.transcode_counters(lib)) == 4


def test_the_spec_is_forty_bytes(l):
    """uint32, int32, uint32, five int32 of the preset parameters, the encoding options, uint32: no padding."""
    assert C.sizeof(capi.TranscodeSpec) == 40
    s = capi.transcode_spec(near_lossless=2, restart_interval=16)
    assert s.set == capi.TRANSCODE_NEAR | capi.TRANSCODE_RESTART_INTERVAL and s.near_lossless == 2 and s.restart_interval == 16
    assert capi.transcode_spec().set == 0
    assert capi.transcode_spec(preset=(255, 9, 9, 9, 31), encoding_options=1).set == capi.TRANSCODE_PRESET | capi.TRANSCODE_ENCODING_OPTIONS


@pytest.mark.parametrize("library", ["libcharls_amd.so", "libcharls.so.3"])
def test_both_library_names_export_the_calls(library):
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB_DIR, library)], capture_output=True, text=True).stdout.split("\n")
    exported = {line.split()[-1] for line in names if line.strip()}
    assert set(NAMES) <= exported


def test_the_identity_list_is_the_plain_goldens():
    """The goldens the GPU test expects back byte for byte under set = 0 are exactly the reference-written ones whose container
    the batch encoder writes: picked here, on the CPU, by walking their marker segments."""
    import json
    import test_gpu_transcode as gpu
    with open(os.path.join(common.GOLDEN, "cases.json")) as f:
        cases = [c for c in json.load(f) if c.get("file", "").startswith("small/") and c["errc"] == 0]
    assert len(cases) > 60
    plain = sorted(c["name"] for c in cases if gpu.is_plain(gpu.golden(c["name"]), c))
    assert plain == sorted(gpu.PLAIN_GOLDENS)
