"""decode_scans_wave_emit without a destination (charls_amd.h part 2l: the index-only build) on the CPU harness
(scan_seek_decode.hip compiled for the host, tests/emu/emu_seek_driver.cpp).

A scan whose ScanDesc::pixels is null is decoded in full and stores no row; a seek point is the wavefront's state -- the LDS
line, not the stored row --, so the points and the ScanResult must equal those of the run with a destination, byte for byte:
the 30 cases of test_emu_seek_index.py (widths 1-33, heights 7-20, 2/8/12/16 bit, 1-4 components, every interleave mode,
NEAR 0-3, K in 1/3/4/6) and one of 70 x 9, whose line spans more than 64 lanes.
Before part 2l the kernel stored through the null pointer: this file cannot run on such a build.  Test infrastructure only."""
import ctypes as C

import numpy as np
import pytest

import emu_bind
from test_emu_seek_index import CASES, Scan, lib

WIDE = (dict(width=70, height=9, bits=8, comps=1, ilv=0, near=0, seed=77, kind="mixed", preset=None), 4)


def _emit_without_pixels(s, K):
    keep = []
    desc = s.desc(np.zeros(1, dtype=np.uint8), keep)  # (make_desc wants an array: the pointer is cleared below)
    desc[0].pixels = None
    points = np.zeros(max(1, (s.height - 1) // K) * s.point_bytes, dtype=np.uint8)
    res = (emu_bind.ScanResult * 1)()
    lib().emu_seek_emit(desc, res, points.ctypes.data_as(C.c_void_p), K)
    return (res[0].errc, res[0].flags, res[0].bytes), points


@pytest.mark.parametrize("case", CASES + [WIDE], ids=[f"s{i}" for i in range(len(CASES))] + ["wide"])
def test_points_and_result_do_not_depend_on_a_destination(case):
    p, K = case
    s = Scan(**p)
    _, want_r, want_points = s.emit(K)
    assert want_r[0] == 0
    got_r, got_points = _emit_without_pixels(s, K)
    assert got_r == want_r
    assert got_points.tobytes() == want_points.tobytes()
    if s.height > K:
        assert want_points.any()  # (the comparison is of real points, not of two untouched buffers)
