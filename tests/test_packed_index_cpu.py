"""The calls of charls_amd.h part 2l (the seek-point index on packed streams) without a GPU: what they refuse for the whole
call is refused before a device is asked for -- the answer is the code itself here, where no device exists, not
device_unavailable -- and writes nothing; a call without frames succeeds; both library names export the calls."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import common
from charls_amd import batch, capi

INVALID_ARGUMENT, INVALID_ARGUMENT_SIZE = 101, 110
LIB_DIR = os.path.join(common.ROOT, "charls_amd", "lib")
NAMES = ["charls_amd_index_batch_device_packed", "charls_amd_decode_batch_device_ragged_indexed",
         "charls_amd_decode_rows_batch_device_ragged", "charls_amd_index_batch_host"]
CALLS = ["index", "index_only", "indexed", "rows", "host"]

u64p, u32p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def l():
    return batch._bind(capi.load_product())


class Tables:
    """Valid host tables for a call over n frames, every array the calls write filled with a sentinel.  Blob and pixels are
    host memory: the device forms only look at the pointers for NULL before they ask for a device."""

    def __init__(self, n):
        self.n, m = n, max(n, 1)
        self.blob = np.full(4096, 0x3C, dtype=np.uint8)
        self.pixels = np.full(4096, 0xA5, dtype=np.uint8)
        self.offsets = np.arange(m, dtype=np.uint64) * 100
        self.sizes = np.full(m, 100, dtype=np.uint64)
        self.dests = (batch.FrameDest * m)()
        for f in range(m):
            self.dests[f] = batch.FrameDest(self.pixels.ctypes.data + 512 * f, 512, 0, 0)
        self.indexes = np.full((m, 64), 0xC3, dtype=np.uint8)
        self.index_sizes = np.full(m, 77, dtype=np.uint64)  # (an input of the two decoding calls: must come back as it went)
        self.first_rows = np.zeros(m, dtype=np.uint32)
        self.row_counts = np.ones(m, dtype=np.uint32)
        self.errcs = np.full(m, -1, dtype=np.int32)
        self.params = (batch.CodecParams * m)()
        for f in range(m):
            self.params[f].near_lossless = 79

    def call(self, l, which, lines=4, **replace):
        a = dict(blob=self.blob.ctypes.data, offsets=self.offsets.ctypes.data_as(u64p), sizes=self.sizes.ctypes.data_as(u64p),
                 dests=self.dests, indexes=self.indexes.ctypes.data, index_sizes=self.index_sizes.ctypes.data_as(u64p),
                 first_rows=self.first_rows.ctypes.data_as(u32p), row_counts=self.row_counts.ctypes.data_as(u32p),
                 params=self.params, errcs=self.errcs.ctypes.data_as(i32p))
        a.update(replace)
        if which in ("index", "index_only"):
            return l.charls_amd_index_batch_device_packed(self.n, a["blob"], a["offsets"], a["sizes"], a["dests"] if which == "index" else None,
                                                          lines, a["indexes"], 64, a["index_sizes"], a["params"], a["errcs"], None)
        if which == "indexed":
            return l.charls_amd_decode_batch_device_ragged_indexed(self.n, a["blob"], a["offsets"], a["sizes"], a["indexes"], 64, a["index_sizes"],
                                                                   a["dests"], a["params"], a["errcs"], None)
        if which == "rows":
            return l.charls_amd_decode_rows_batch_device_ragged(self.n, a["blob"], a["offsets"], a["sizes"], a["indexes"], 64, a["index_sizes"],
                                                                a["first_rows"], a["row_counts"], a["dests"], a["errcs"], None)
        return l.charls_amd_index_batch_host(self.n, a["blob"], a["offsets"], a["sizes"], lines, a["indexes"], 64, a["index_sizes"], a["params"],
                                             a["errcs"])

    def untouched(self):
        m = max(self.n, 1)
        return bool((self.errcs == -1).all() and (self.index_sizes == 77).all() and (self.indexes == 0xC3).all() and
                    (self.pixels == 0xA5).all() and (self.blob == 0x3C).all() and all(self.params[f].near_lossless == 79 for f in range(m)))


TABLES_OF = {"index": ["offsets", "sizes", "index_sizes", "errcs", "blob", "indexes"],
             "index_only": ["offsets", "sizes", "index_sizes", "errcs", "blob", "indexes"],
             "indexed": ["offsets", "sizes", "index_sizes", "errcs", "blob", "indexes", "dests"],
             "rows": ["offsets", "sizes", "index_sizes", "errcs", "blob", "indexes", "dests", "first_rows", "row_counts"],
             "host": ["offsets", "sizes", "index_sizes", "errcs", "blob", "indexes"]}


@pytest.mark.parametrize("which", CALLS)
def test_null_tables(l, which):
    for name in TABLES_OF[which]:
        t = Tables(2)
        assert t.call(l, which, **{name: None}) == INVALID_ARGUMENT, name
        assert t.untouched(), name


@pytest.mark.parametrize("which", ["index", "index_only", "host"])
def test_no_lines_per_seek_point(l, which):
    for n in (0, 2):
        t = Tables(n)
        assert t.call(l, which, lines=0) == INVALID_ARGUMENT
        assert t.untouched()


@pytest.mark.parametrize("which", ["index", "indexed", "rows"])
def test_reserved_must_be_zero(l, which):
    for bad in (0, 2):
        t = Tables(3)
        t.dests[bad].reserved = 1
        assert t.call(l, which) == INVALID_ARGUMENT
        assert t.untouched()


@pytest.mark.parametrize("which", ["index", "indexed", "rows"])
def test_no_pixels_with_a_capacity(l, which):
    for bad in (0, 2):
        t = Tables(3)
        t.dests[bad].d_pixels = None
        assert t.call(l, which) == INVALID_ARGUMENT
        assert t.untouched()


@pytest.mark.parametrize("which", CALLS)
def test_an_offset_plus_size_that_overflows(l, which):
    for bad in (0, 2):
        t = Tables(3)
        t.offsets[bad] = (1 << 64) - 50
        assert t.call(l, which) == INVALID_ARGUMENT_SIZE
        assert t.untouched()


@pytest.mark.parametrize("which", CALLS)
def test_no_frames_is_success(l, which):
    t = Tables(0)
    assert t.call(l, which, blob=None, indexes=None) == 0  # (no frames: no blob, no indexes)
    assert t.untouched()


@pytest.mark.parametrize("library", ["libcharls_amd.so", "libcharls.so.3"])
def test_both_library_names_export_the_calls(library):
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB_DIR, library)], capture_output=True, text=True).stdout.split("\n")
    exported = {line.split()[-1] for line in names if line.strip()}
    assert set(NAMES) <= exported


def test_the_python_layer_has_the_four_calls():
    for name in ("index_batch_packed", "decode_batch_ragged_indexed", "decode_rows_batch_ragged", "index_batch_host"):
        assert callable(getattr(batch, name))
