"""The calls of charls_amd.h part 2e without a GPU: what they refuse for the whole call is refused before a device is asked
for (the answer is invalid_argument here, where no device exists, not device_unavailable), a call without frames succeeds,
and both library names export the three entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import common
from charls_amd import batch, capi

INVALID_ARGUMENT = 101
LIB_DIR = os.path.join(common.ROOT, "charls_amd", "lib")
NAMES = ["charls_amd_probe_batch_device_packed", "charls_amd_decode_batch_device_ragged", "charls_amd_encode_batch_device_ragged"]
SOMEWHERE = 0x1000  # a non-NULL "device pointer": no call below gets as far as touching it

u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def l():
    return batch._bind(capi.load_product())


class Tables:
    """Valid host tables for a call over n frames."""

    def __init__(self, n):
        self.n = n
        self.offsets = np.full(n + 1, 77, dtype=np.uint64)
        self.sizes = np.full(max(n, 1), 10, dtype=np.uint64)
        self.errcs = np.full(max(n, 1), -1, dtype=np.int32)
        self.bytes = np.zeros(max(n, 1), dtype=np.uint64)
        self.params = (batch.CodecParams * max(n, 1))()
        self.sources = (batch.FrameSource * max(n, 1))()
        self.dests = (batch.FrameDest * max(n, 1))()
        for f in range(n):
            self.sources[f] = batch.FrameSource(batch.codec_params(16, 8), SOMEWHERE, 0, 0, 0)
            self.dests[f] = batch.FrameDest(SOMEWHERE, 128, 0, 0)

    def o(self):
        return self.offsets.ctypes.data_as(u64p)

    def s(self):
        return self.sizes.ctypes.data_as(u64p)

    def e(self):
        return self.errcs.ctypes.data_as(i32p)

    def b(self):
        return self.bytes.ctypes.data_as(u64p)


def test_null_tables(l):
    t = Tables(2)
    probe = [2, SOMEWHERE, t.o(), t.s(), t.params, t.b(), t.e(), None]
    for at in (2, 3, 4, 5, 6):
        args = list(probe)
        args[at] = None
        assert l.charls_amd_probe_batch_device_packed(*args) == INVALID_ARGUMENT, at
    decode = [2, SOMEWHERE, t.o(), t.s(), t.dests, t.params, t.e(), None]
    for at in (2, 3, 4, 6):
        args = list(decode)
        args[at] = None
        assert l.charls_amd_decode_batch_device_ragged(*args) == INVALID_ARGUMENT, at
    encode = [2, t.sources, SOMEWHERE, 1 << 20, 1, t.o(), t.s(), t.e(), None]
    for at in (1, 5, 6, 7):
        args = list(encode)
        args[at] = None
        assert l.charls_amd_encode_batch_device_ragged(*args) == INVALID_ARGUMENT, at
    assert (t.offsets == 77).all() and (t.errcs == -1).all()  # nothing was done


def test_reserved_must_be_zero(l):
    for bad in (0, 2):
        t = Tables(3)
        t.sources[bad].reserved = 1
        assert l.charls_amd_encode_batch_device_ragged(3, t.sources, SOMEWHERE, 1 << 20, 1, t.o(), t.s(), t.e(), None) == INVALID_ARGUMENT
        t.dests[bad].reserved = 7
        assert l.charls_amd_decode_batch_device_ragged(3, SOMEWHERE, t.o(), t.s(), t.dests, t.params, t.e(), None) == INVALID_ARGUMENT
        assert (t.offsets == 77).all() and (t.errcs == -1).all()


@pytest.mark.parametrize("alignment", [0, 3, 8192])
def test_offset_alignment(l, alignment):
    for n in (0, 2):
        t = Tables(n)
        assert l.charls_amd_encode_batch_device_ragged(n, t.sources, SOMEWHERE, 1 << 20, alignment, t.o(), t.s(), t.e(), None) == INVALID_ARGUMENT
        assert (t.offsets == 77).all()


def test_no_frames(l):
    t = Tables(0)
    assert l.charls_amd_encode_batch_device_ragged(0, t.sources, None, 0, 16, t.o(), t.s(), t.e(), None) == 0
    assert t.offsets[0] == 0
    assert l.charls_amd_decode_batch_device_ragged(0, None, t.o(), t.s(), t.dests, None, t.e(), None) == 0
    assert l.charls_amd_probe_batch_device_packed(0, None, t.o(), t.s(), t.params, t.b(), t.e(), None) == 0
    assert (t.errcs == -1).all()


@pytest.mark.parametrize("library", ["libcharls_amd.so", "libcharls.so.3"])
def test_both_library_names_export_the_calls(library):
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB_DIR, library)], capture_output=True, text=True).stdout.split("\n")
    exported = {line.split()[-1] for line in names if line.strip()}
    assert set(NAMES) <= exported
