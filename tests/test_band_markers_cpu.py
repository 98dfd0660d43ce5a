"""charls_amd_decode_rows_batch_device_ragged_markers (charls_amd.h part 2m) without a GPU: what it refuses for the whole call is
refused before a device is asked for -- the answer is the code itself here, where no device exists, not device_unavailable --
and writes nothing; a call without frames succeeds; both library names export the call and its counters, and the counters
answer.  Then tests/band_plan: the pure planning of the route (charls_amd/csrc/host/band_plan.h) as a stand-alone program,
built plain and with the host compiler's sanitizers and run directly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import common
from charls_amd import batch, capi

INVALID_ARGUMENT, INVALID_ARGUMENT_SIZE = 101, 110
LIB_DIR = os.path.join(common.ROOT, "charls_amd", "lib")
NAMES = ["charls_amd_decode_rows_batch_device_ragged_markers", "charls_amd_band_marker_counters"]

u64p, u32p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def l():
    return batch._bind(capi.load_product())


class Tables:
    """Valid host tables for a call over n frames, every array the call writes filled with a sentinel.  Blob and bands are host
    memory: the call only looks at the pointers for NULL before it asks for a device."""

    def __init__(self, n):
        self.n, m = n, max(n, 1)
        self.blob = np.full(4096, 0x3C, dtype=np.uint8)
        self.pixels = np.full(4096, 0xA5, dtype=np.uint8)
        self.offsets = np.arange(m, dtype=np.uint64) * 100
        self.sizes = np.full(m, 100, dtype=np.uint64)
        self.bands = (batch.FrameDest * m)()
        for f in range(m):
            self.bands[f] = batch.FrameDest(self.pixels.ctypes.data + 512 * f, 512, 0, 0)
        self.indexes = np.full((m, 64), 0xC3, dtype=np.uint8)
        self.index_sizes = np.full(m, 77, dtype=np.uint64)
        self.first_rows = np.zeros(m, dtype=np.uint32)
        self.row_counts = np.ones(m, dtype=np.uint32)
        self.errcs = np.full(m, -1, dtype=np.int32)

    def call(self, l, **replace):
        a = dict(blob=self.blob.ctypes.data, offsets=self.offsets.ctypes.data_as(u64p), sizes=self.sizes.ctypes.data_as(u64p),
                 bands=self.bands, indexes=self.indexes.ctypes.data, index_sizes=self.index_sizes.ctypes.data_as(u64p),
                 first_rows=self.first_rows.ctypes.data_as(u32p), row_counts=self.row_counts.ctypes.data_as(u32p),
                 errcs=self.errcs.ctypes.data_as(i32p))
        a.update(replace)
        return l.charls_amd_decode_rows_batch_device_ragged_markers(self.n, a["blob"], a["offsets"], a["sizes"], a["indexes"], 64,
                                                                    a["index_sizes"], a["first_rows"], a["row_counts"], a["bands"], a["errcs"],
                                                                    None)

    def untouched(self):
        return bool((self.errcs == -1).all() and (self.index_sizes == 77).all() and (self.indexes == 0xC3).all() and
                    (self.pixels == 0xA5).all() and (self.blob == 0x3C).all())


def test_null_tables(l):
    for name in ["offsets", "sizes", "index_sizes", "errcs", "blob", "indexes", "bands", "first_rows", "row_counts"]:
        t = Tables(2)
        assert t.call(l, **{name: None}) == INVALID_ARGUMENT, name
        assert t.untouched(), name
    t = Tables(2)
    t.index_sizes[:] = 0  # (no frame has an index: `indexes` may be NULL, and the call gets as far as asking for a device)
    assert t.call(l, indexes=None) != INVALID_ARGUMENT


def test_reserved_must_be_zero_and_no_pixels_with_a_capacity(l):
    for bad in (0, 2):
        t = Tables(3)
        t.bands[bad].reserved = 1
        assert t.call(l) == INVALID_ARGUMENT and t.untouched()
        t = Tables(3)
        t.bands[bad].d_pixels = None
        assert t.call(l) == INVALID_ARGUMENT and t.untouched()


def test_an_offset_plus_size_that_overflows(l):
    for bad in (0, 2):
        t = Tables(3)
        t.offsets[bad] = (1 << 64) - 50
        assert t.call(l) == INVALID_ARGUMENT_SIZE and t.untouched()


def test_the_checks_are_those_of_the_ragged_band_call(l):
    """Argument for argument: whatever one call answers for a whole call without a device, the other answers."""
    def both(t, **replace):
        a = dict(blob=t.blob.ctypes.data, indexes=t.indexes.ctypes.data, bands=t.bands)
        a.update(replace)
        args = (t.n, a["blob"], t.offsets.ctypes.data_as(u64p), t.sizes.ctypes.data_as(u64p), a["indexes"], 64,
                t.index_sizes.ctypes.data_as(u64p), t.first_rows.ctypes.data_as(u32p), t.row_counts.ctypes.data_as(u32p), a["bands"],
                t.errcs.ctypes.data_as(i32p), None)
        return l.charls_amd_decode_rows_batch_device_ragged(*args), l.charls_amd_decode_rows_batch_device_ragged_markers(*args)

    for replace in ({}, {"blob": None}, {"indexes": None}, {"bands": None}):
        for n in (0, 1, 3):
            old, new = both(Tables(n), **replace)
            assert old == new, (replace, n)


def test_no_frames_is_success(l):
    t = Tables(0)
    assert t.call(l, blob=None, indexes=None) == 0
    assert t.untouched()


@pytest.mark.parametrize("library", ["libcharls_amd.so", "libcharls.so.3"])
def test_both_library_names_export_the_two_symbols(library):
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB_DIR, library)], capture_output=True, text=True).stdout.split("\n")
    exported = {line.split()[-1] for line in names if line.strip()}
    assert set(NAMES) <= exported


def test_the_counters_answer(l):
    out = (C.c_uint64 * 6)(*([9] * 6))
    assert l.charls_amd_band_marker_counters(out, 6) == 4 and list(out)[4:] == [9, 9]
    three = (C.c_uint64 * 4)(*([9] * 4))
    assert l.charls_amd_band_marker_counters(three, 3) == 3 and three[3] == 9
    assert l.charls_amd_band_marker_counters(None, 4) == 0 and l.charls_amd_band_marker_counters(out, 0) == 0
    before = capi.band_marker_counters()
    assert set(before) == {"frames", "intervals", "fallback_frames", "launches"}
    Tables(0).call(l, blob=None, indexes=None)
    assert capi.band_marker_counters() == before  # (a call without frames counts nothing)
    assert callable(batch.decode_rows_batch_ragged_markers)


# ---- tests/band_plan: the planning header under the host compiler, plain and with sanitizers

def _build_and_run(tmp_path, name, extra_flags):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra_flags,
                           "-I" + os.path.join(common.ROOT, "charls_amd", "csrc"),
                           os.path.join(common.ROOT, "tests", "band_plan", "band_plan_test.cpp"), "-o", str(exe)])
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)


def test_band_plan(tmp_path):
    r = _build_and_run(tmp_path, "band_plan_test", [])
    assert r.returncode == 0 and "band plan ok" in r.stdout and "FAILED" not in r.stdout, r.stdout + r.stderr


def test_band_plan_under_address_and_undefined_behavior_sanitizers(tmp_path):
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull], input="int main(){return 0;}",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("this g++ has no libasan / libubsan")
    r = _build_and_run(tmp_path, "band_plan_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert r.returncode == 0 and "band plan ok" in r.stdout and "FAILED" not in r.stdout, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
