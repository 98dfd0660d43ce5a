"""The segmented copy kernel of the packed-stream calls on the CPU harness (pack_streams.hip compiled for the host,
tests/emu/emu_pack_driver.cpp) against numpy slicing, in a canary-filled arena of which every byte outside the jobs' extents
must survive: every length around the 16-byte granule, the 256-byte row and the workgroup trip, at every source misalignment
x every destination misalignment, with every kind of padding; jobs that share one destination granule; a job of length 0
between two others; many jobs per launch, more than the grid has rows.  Test infrastructure only."""
import ctypes as C
import os

import numpy as np
import pytest

import emu_bind

CANARY = 0xC7
SMALL_LENGTHS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257]
PADS = [0, 1, 15, 4095]  # 4095: alignment - 1 of the largest offset alignment the calls take


class PackJob(C.Structure):  # must mirror charls_amd/csrc/device/pack_streams.h
    _fields_ = [("src_offset", C.c_uint64), ("dst_offset", C.c_uint64), ("bytes", C.c_uint64), ("pad_bytes", C.c_uint32),
                ("reserved", C.c_uint32)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = emu_bind._build_and_load("emu_pack_driver.cpp", os.path.join(emu_bind.ROOT, "tests", "_emu_build", "libjls_emu_pack.so"))
        assert _lib.emu_sizeof_pack_job() == C.sizeof(PackJob)
        _lib.emu_pack_trip_bytes.restype = C.c_uint64
    return _lib


def trip_bytes():
    return int(lib().emu_pack_trip_bytes())


def _aligned(nbytes, fill):
    """(raw, start): raw[start] lies on a 64-byte boundary and has 64 bytes of margin on either side of nbytes bytes."""
    raw = np.empty(nbytes + 192, dtype=np.uint8)
    start = (-raw.ctypes.data) % 64 + 64
    raw[:] = fill
    return raw, start


def _run(src_raw, dst_raw, jobs, shares, rows):
    """Runs the kernel on `jobs` [(src_offset, dst_offset, bytes, pad)] -- offsets from the raw arrays' first bytes -- and
    compares the whole destination arena with what numpy slicing makes of the same jobs."""
    expected = dst_raw.copy()
    for so, do, n, pad in jobs:
        expected[do:do + n] = src_raw[so:so + n]
        expected[do + n:do + n + pad] = 0
    arr = (PackJob * len(jobs))(*[PackJob(so, do, n, pad, 0) for so, do, n, pad in jobs])
    lib().emu_pack_streams(C.c_void_p(src_raw.ctypes.data), C.c_void_p(dst_raw.ctypes.data), arr, len(jobs), shares, rows)
    bad = np.flatnonzero(dst_raw != expected)
    assert bad.size == 0, f"first differing byte of the arena: {int(bad[0])} of {dst_raw.size} ({bad.size} differ)"


def _cross(lengths, pads, shares, rows, seed):
    """Every length x every source misalignment x every destination misalignment x every pad, each job in a stretch of its
    own with canary bytes between it and its neighbours, all in ONE launch."""
    rng = np.random.default_rng(seed)
    longest = max(lengths)
    src_raw, s0 = _aligned(longest + 64, 0)
    src_raw[:] = rng.integers(0, 256, src_raw.size, dtype=np.uint8)
    extent = sum((n + p + 48) for n in lengths for p in pads) * 256
    dst_raw, d0 = _aligned(extent, CANARY)
    jobs, at = [], d0
    for n in lengths:
        for pad in pads:
            for smis in range(16):
                for dmis in range(16):
                    at = (at + 15) // 16 * 16 + 16 + dmis  # (d0 is aligned: the address's misalignment is dmis)
                    jobs.append((s0 + 16 * (smis % 3) + smis, at, n, pad))
                    at += n + pad
    assert at <= d0 + extent
    _run(src_raw, dst_raw, jobs, shares, rows)


@pytest.mark.parametrize("shares,rows", [(1, 3), (2, 5)])
def test_small_lengths_at_every_alignment(shares, rows):
    _cross(SMALL_LENGTHS, PADS, shares, rows, 21)


@pytest.mark.parametrize("shares", [1, 3])
def test_lengths_around_the_workgroup_trip(shares):
    """One byte less than, exactly, and one byte more than what one workgroup trip moves -- and twice that, so that the
    grid-stride loop takes a second trip with one share and splits the trips with three."""
    t = trip_bytes()
    assert t == 16384
    _cross([t - 1, t, t + 1, 2 * t + 17], [0, 4095], shares, 4, 22)


def test_jobs_that_share_a_destination_granule():
    """Three jobs of 3, 5 and 2 bytes inside ONE destination granule and a long job that starts in the same granule; then a
    job of length 0 between two jobs that abut; then more tiny jobs in the long job's last granule.  Nothing but the jobs'
    own bytes may change: the neighbours in the granule are other jobs' bytes."""
    rng = np.random.default_rng(23)
    src_raw, s0 = _aligned(70000, 0)
    src_raw[:] = rng.integers(0, 256, src_raw.size, dtype=np.uint8)
    for shift in range(16):
        dst_raw, d0 = _aligned(70000, CANARY)
        at = d0 + shift
        jobs = []
        for n, pad, so in [(3, 0, 5), (5, 0, 100), (2, 0, 9), (40000 + shift, 0, 1003), (0, 0, 77), (7, 1, 31), (0, 3, 2), (1, 0, 3),
                           (1, 0, 4), (1, 0, 5), (20, 15, 6)]:
            jobs.append((s0 + so, at, n, pad))
            at += n + pad
        _run(src_raw, dst_raw, jobs, 2, 3)


def test_many_jobs_back_to_back():
    """2000 jobs of random lengths laid out by the offset rule at alignments 1, 2 and 16, back to back (no canary between
    them: the padding is the gap), sources at slot pitch 301 -- more jobs than the grid has rows."""
    rng = np.random.default_rng(24)
    count, pitch = 2000, 301
    src_raw, s0 = _aligned(count * pitch, 0)
    src_raw[:] = rng.integers(0, 256, src_raw.size, dtype=np.uint8)
    sizes = rng.integers(0, pitch + 1, count)
    sizes[::7] = 0
    for alignment in (1, 2, 16):
        dst_raw, d0 = _aligned(count * (pitch + 16), CANARY)
        jobs, at = [], 0
        for f in range(count):
            n = int(sizes[f])
            if n == 0:
                continue
            nxt = -(-(at + n) // alignment) * alignment
            jobs.append((s0 + f * pitch, d0 + 3 + at, n, nxt - at - n))  # (+ 3: the blob itself starts at an odd address)
            at = nxt
        _run(src_raw, dst_raw, jobs, 1, 7)
