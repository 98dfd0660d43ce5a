"""The salvage calls of charls_amd.h part 2g without a GPU: what the batch call refuses for the whole call is refused before a
device is asked for (invalid_argument here, where no device exists, not device_unavailable) and nothing is written; a call
without frames succeeds; both library names export the three entry points; and the claim rule of tests/salvage_model.py
agrees with the cases worked by hand in the header's terms."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import common
import salvage_model as sm
from charls_amd import batch, capi

INVALID_ARGUMENT = 101
LIB_DIR = os.path.join(common.ROOT, "charls_amd", "lib")
NAMES = ["charls_amd_decode_batch_device_salvage", "charls_amd_jpegls_decoder_decode_to_buffer_salvage", "charls_amd_salvage_counters"]
SOMEWHERE = 0x1000  # a non-NULL "device pointer": no call below gets as far as touching it

u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def l():
    return batch._bind(capi.load_product())


class Tables:
    """Valid host tables for a call over n frames."""

    def __init__(self, n):
        self.offsets = np.full(n + 1, 77, dtype=np.uint64)
        self.sizes = np.full(max(n, 1), 10, dtype=np.uint64)
        self.errcs = np.full(max(n, 1), -1, dtype=np.int32)
        self.params = (batch.CodecParams * max(n, 1))()
        self.reports = (capi.SalvageReport * max(n, 1))()
        self.status = np.full((max(n, 1), 8), 0xEE, dtype=np.uint8)
        self.dests = (batch.FrameDest * max(n, 1))()
        for f in range(max(n, 1)):
            self.dests[f] = batch.FrameDest(SOMEWHERE, 128, 0, 0)
            self.reports[f] = capi.SalvageReport(9, 9, 9, 9, 9, 9)

    def args(self, n):
        return [n, SOMEWHERE, self.offsets.ctypes.data_as(u64p), self.sizes.ctypes.data_as(u64p), self.dests, 0, self.params, self.reports,
                self.status.ctypes.data, 8, self.errcs.ctypes.data_as(i32p), None]

    def untouched(self):
        return (self.offsets == 77).all() and (self.errcs == -1).all() and (self.status == 0xEE).all() and \
            all(r.astuple() == (9,) * 6 for r in self.reports)


def test_whole_call_errors_come_before_a_device_is_asked_for(l):
    t = Tables(2)
    for at in (2, 3, 4, 7, 10):  # offsets, sizes, dests, reports, errcs
        args = t.args(2)
        args[at] = None
        assert l.charls_amd_decode_batch_device_salvage(*args) == INVALID_ARGUMENT, at
    args = t.args(2)
    args[9] = 0  # a status array without a pitch
    assert l.charls_amd_decode_batch_device_salvage(*args) == INVALID_ARGUMENT
    args = t.args(2)
    args[1] = None  # no streams
    assert l.charls_amd_decode_batch_device_salvage(*args) == INVALID_ARGUMENT
    for bad in (0, 1):
        t.dests[bad].reserved = 3
        assert l.charls_amd_decode_batch_device_salvage(*t.args(2)) == INVALID_ARGUMENT
        t.dests[bad].reserved = 0
    t.dests[1] = batch.FrameDest(None, 16, 0, 0)
    assert l.charls_amd_decode_batch_device_salvage(*t.args(2)) == INVALID_ARGUMENT
    assert t.untouched()


def test_no_frames(l):
    t = Tables(0)
    args = t.args(0)
    args[1] = None
    assert l.charls_amd_decode_batch_device_salvage(*args) == 0
    args[8], args[9] = None, 0  # and without a status array
    assert l.charls_amd_decode_batch_device_salvage(*args) == 0
    assert t.untouched()


def test_counters_respect_the_capacity(l):
    out = (C.c_uint64 * 6)(*([7] * 6))
    assert l.charls_amd_salvage_counters(out, 6) == 4 and list(out)[4:] == [7, 7]
    assert l.charls_amd_salvage_counters(out, 2) == 2 and l.charls_amd_salvage_counters(None, 4) == 0
    before = batch.salvage_counters()
    t = Tables(0)
    assert l.charls_amd_decode_batch_device_salvage(*t.args(0)) == 0
    assert batch.salvage_counters() == before


def test_part_one_call_checks_its_arguments():
    L = capi.load_product().lib
    fn = L.charls_amd_jpegls_decoder_decode_to_buffer_salvage
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(capi.SalvageReport), C.c_void_p, C.c_size_t]
    fn.restype = C.c_int32
    report = capi.SalvageReport()
    out = np.zeros(64, dtype=np.uint8)
    assert fn(None, out.ctypes.data, 64, 0, 0, C.byref(report), None, 0) == INVALID_ARGUMENT
    L.charls_jpegls_decoder_create.restype = C.c_void_p
    dec = L.charls_jpegls_decoder_create()
    try:
        assert fn(dec, out.ctypes.data, 64, 0, 0, None, None, 0) == INVALID_ARGUMENT
        assert fn(dec, out.ctypes.data, 64, 0, 0, C.byref(report), None, 5) == INVALID_ARGUMENT
        assert fn(dec, out.ctypes.data, 64, 0, 0, C.byref(report), None, 0) == 100  # invalid_operation: no header was read
    finally:
        L.charls_jpegls_decoder_destroy.argtypes = [C.c_void_p]
        L.charls_jpegls_decoder_destroy(dec)


@pytest.mark.parametrize("library", ["libcharls_amd.so", "libcharls.so.3"])
def test_both_library_names_export_the_calls(library):
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB_DIR, library)], capture_output=True, text=True).stdout.split("\n")
    exported = {line.split()[-1] for line in names if line.strip()}
    assert set(NAMES) <= exported


# ---- the claim rule, N = 20 ----------------------------------------------------------------------------------------------

N = 20
SOUND = [k % 8 for k in range(N - 1)]


def _claimed(piece_of):
    return {j: k for j, k in enumerate(piece_of) if k is not None}


def test_model_intact():
    p, q, piece_of = sm.claims(SOUND, N)
    assert (len(SOUND), p, q) == (19, 19, 19) and piece_of == list(range(N))


def test_model_marker_deleted():
    numbers = SOUND[:5] + SOUND[6:]
    p, q, piece_of = sm.claims(numbers, N)
    assert (len(numbers), p, q) == (18, 5, 13)
    assert _claimed(piece_of) == {**{j: j for j in range(5)}, **{j: j - 1 for j in range(7, 20)}}  # only 5 and 6 unclaimed


def test_model_marker_with_the_wrong_number():
    numbers = SOUND[:9] + [(SOUND[9] + 3) % 8] + SOUND[10:]
    p, q, piece_of = sm.claims(numbers, N)
    assert (len(numbers), p, q) == (19, 9, 9)
    assert sorted(set(range(N)) - set(_claimed(piece_of))) == [9, 10]  # a marker that cannot be trusted bounds neither neighbour
    assert all(k == j for j, k in _claimed(piece_of).items())


def test_model_spurious_marker():
    numbers = SOUND[:2] + [5] + SOUND[2:]  # FF D5 behind marker 1
    p, q, piece_of = sm.claims(numbers, N)
    assert (len(numbers), p, q) == (20, 2, 17)
    assert sorted(set(range(N)) - set(_claimed(piece_of))) == [2]
    assert _claimed(piece_of) == {0: 0, 1: 1, **{j: j + 1 for j in range(3, 20)}}


def test_model_spurious_marker_with_the_expected_number():
    numbers = SOUND[:4] + [4] + SOUND[4:]  # a marker carrying 4 behind marker 3: inside interval 4
    p, q, piece_of = sm.claims(numbers, N)
    assert (len(numbers), p, q) == (20, 5, 15)
    # piece 4, the first half of interval 4, claims interval 4 (and fails the judgement); 5 .. 19 are claimed from behind
    assert _claimed(piece_of) == {**{j: j for j in range(5)}, **{j: j + 1 for j in range(5, 20)}}


def test_model_eight_markers_deleted_in_a_row():
    numbers = SOUND[:3] + SOUND[11:]
    p, q, piece_of = sm.claims(numbers, N)
    assert (len(numbers), p, q) == (11, 11, 11)
    assert _claimed(piece_of) == {0: 0, 19: 11}  # every other piece has two different claims; nothing is misplaced


def test_model_cut_off_behind_a_marker():
    numbers = SOUND[:7]
    p, q, piece_of = sm.claims(numbers, N)
    assert (len(numbers), p, q) == (7, 7, 0)
    assert _claimed(piece_of) == {j: j for j in range(7)}


def test_model_more_markers_than_are_recorded():
    numbers = [k % 8 for k in range(N + 12)]
    p, q, piece_of = sm.claims(numbers, N)
    assert (p, q) == (19, 0) and _claimed(piece_of) == {j: j for j in range(19)}
