"""The segment-hash kernel on the CPU harness (segment_hash.hip compiled for the host, tests/emu/emu_hash_driver.cpp) against the
library's host function (host/segment_hash.h, exposed by the same driver): every length around the 8-byte word, the 16-byte
load and the 2048-byte trip, at every kind of misalignment, with random, all-0xFF and all-zero bytes, many jobs per launch,
and a canary behind the output array.  Test infrastructure only."""
import ctypes as C
import os

import numpy as np
import pytest

import emu_bind

LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 511, 512, 513, 4095, 4096, 4097]
# trip boundaries of the kernel (128 words): a whole trip, one with a lone tail behind it, one word short of a trip
TRIP_LENGTHS = [1016, 1023, 1024, 1025, 1032, 2047, 2048, 2049, 2056]
OFFSETS = [0, 1, 5, 15]
CANARY = 0xA5A5A5A5A5A5A5A5


class HashJob(C.Structure):  # must mirror charls_amd/csrc/device/seek_decode.h
    _fields_ = [("offset", C.c_uint64), ("bytes", C.c_uint64)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = emu_bind._build_and_load("emu_hash_driver.cpp", os.path.join(emu_bind.ROOT, "tests", "_emu_build", "libjls_emu_hash.so"))
        assert _lib.emu_sizeof_hash_job() == C.sizeof(HashJob)
        _lib.emu_host_segment_hash.restype = C.c_uint64
        _lib.emu_host_segment_hash.argtypes = [C.c_void_p, C.c_size_t]
    return _lib


def _aligned(nbytes, fill):
    """A buffer whose byte 64 lies on a 64-byte boundary, with 64 bytes of margin on either side."""
    raw = np.empty(nbytes + 192, dtype=np.uint8)
    start = (-raw.ctypes.data) % 64 + 64
    raw[:] = 0x5A
    view = raw[start:start + nbytes]
    view[:] = fill
    return raw, view, start


def _run(raw, jobs):
    L = lib()
    n = len(jobs)
    arr = (HashJob * n)(*[HashJob(o, b) for o, b in jobs])
    out = np.full(n + 2, CANARY, dtype=np.uint64)
    L.emu_segment_hash(C.c_void_p(raw.ctypes.data), arr, C.c_void_p(out.ctypes.data), n)
    assert out[n] == CANARY and out[n + 1] == CANARY
    return [int(v) for v in out[:n]]


def _host(raw, offset, nbytes):
    return int(lib().emu_host_segment_hash(C.c_void_p(raw.ctypes.data + offset), nbytes))


@pytest.mark.parametrize("fill", ["random", "ff", "zero"])
def test_kernel_equals_host_function(fill):
    """All lengths x all misalignments in ONE launch per kind of bytes."""
    span = max(LENGTHS + TRIP_LENGTHS) + 16
    rng = np.random.default_rng(11)
    data = {"random": rng.integers(0, 256, span, dtype=np.uint8), "ff": 0xFF, "zero": 0}[fill]
    raw, _, start = _aligned(span, data)
    jobs = [(start + off, n) for n in LENGTHS + TRIP_LENGTHS for off in OFFSETS]
    got = _run(raw, jobs)
    for (o, n), v in zip(jobs, got):
        assert v == _host(raw, o, n), (o - start, n)


def test_segments_side_by_side_do_not_mix():
    """Jobs that touch one another (the end of one in the 16-byte granule the next starts in), a job of length 0 between
    them, and the same bytes at two misalignments giving the same value."""
    rng = np.random.default_rng(12)
    raw, view, start = _aligned(4096, rng.integers(0, 256, 4096, dtype=np.uint8))
    view[2000:2300] = view[100:400]
    jobs = [(start + 3, 1000), (start + 1003, 0), (start + 1003, 997), (start + 100, 300), (start + 2000, 300), (start, 4096)]
    got = _run(raw, jobs)
    for (o, n), v in zip(jobs, got):
        assert v == _host(raw, o, n)
    assert got[3] == got[4]
    assert len({got[0], got[1], got[2], got[3], got[5]}) == 5


def test_length_is_part_of_the_value():
    """Zero bytes of different lengths differ (n is folded into the seed), and a byte behind the end does not count."""
    raw, view, start = _aligned(64, 0)
    a = _run(raw, [(start, n) for n in (0, 1, 8, 9, 16)])
    assert len(set(a)) == 5
    view[9] = 0xFF
    assert _run(raw, [(start, 9)])[0] == a[3]
