"""Seek points of the exact decoder on the CPU harness (scan_seek_decode.hip compiled for the host, tests/emu/emu_seek_driver.cpp):
  * decode_scans_wave_emit decodes exactly as decode_scans_wave (rows and ScanResult);
  * resuming every interval from its seek point gives the same rows, every interval ends in exactly the next point's state,
    and the last one reports the bytes the plain decoder consumed;
  * a tampered seek point (a context byte, a line sample, the reader one bit away, two points swapped, the points of
    another image) makes the interval that starts from it or ends at it report a mismatch.
Streams from the oracle's encoder.  Test infrastructure only."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import emu_bind
import jls_container
import oracle_bind as ob
from charls_amd import synth
from test_emu_serial_kernels import _stream_copy

MISMATCH, CHECKED = 2, 4
COMPARE, END = 1, 2
LINE_OFF = 2992


class SeekWork(C.Structure):  # must mirror charls_amd/csrc/device/seek_decode.h
    _fields_ = [("scan", C.c_uint32), ("first_row", C.c_uint32), ("end_row", C.c_uint32), ("store_from", C.c_uint32),
                ("mode", C.c_uint32), ("row_base", C.c_uint32), ("from_point", C.c_uint64), ("to_point", C.c_uint64)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = emu_bind._build_and_load("emu_seek_driver.cpp", os.path.join(emu_bind.ROOT, "tests", "_emu_build", "libjls_emu_seek.so"))
        assert _lib.emu_sizeof_seek_work() == C.sizeof(SeekWork)
        _lib.emu_seek_point_bytes.restype = C.c_size_t
    return _lib


class Scan:
    """Scan 0 of an oracle-coded frame, ready for the kernels."""

    def __init__(self, width, height, bits, comps, ilv, near, seed, kind="mixed", preset=None):
        img = synth.frame_numpy(width, height, seed=seed, bits=bits, components=comps, kind=kind, interleaved=ilv != 0)
        self.jls = ob.encode(img, width=width, height=height, bits_per_sample=bits, component_count=comps, near_lossless=near,
                             interleave_mode=ilv, preset=preset, destination_size=8 * width * height * comps + 4096)
        cont = jls_container.parse(self.jls)
        self.pc = jls_container.validated_pc(cont.pc, bits, near)
        self.width, self.height, self.bits, self.near, self.ilv = width, height, bits, near, ilv
        self.comps = comps if ilv != 0 else 1
        self.planes = 1 if ilv == 0 else comps
        self.row = width * ((bits + 7) // 8) * (comps if ilv != 0 else 1)
        self.stream = _stream_copy(self.jls, cont.scans[0].data_start)
        self.point_bytes = lib().emu_seek_point_bytes(width, self.planes, int(bits > 8))

    def desc(self, pixels, keep):
        return (emu_bind.ScanDesc * 1)(emu_bind.make_desc(self.width, self.height, self.comps, self.ilv, self.bits, self.near, 0,
                                                          self.pc, 0, pixels, self.row, self.stream, keep))

    def plain(self):
        keep, px = [], np.zeros(self.row * self.height, dtype=np.uint8)
        res = (emu_bind.ScanResult * 1)()
        lib().emu_decode_scans_wave(self.desc(px, keep), res)
        return px, (res[0].errc, res[0].flags, res[0].bytes)

    def emit(self, K):
        keep, px = [], np.zeros(self.row * self.height, dtype=np.uint8)
        points = np.zeros(max(1, (self.height - 1) // K) * self.point_bytes, dtype=np.uint8)
        res = (emu_bind.ScanResult * 1)()
        lib().emu_seek_emit(self.desc(px, keep), res, points.ctypes.data_as(C.c_void_p), K)
        return px, (res[0].errc, res[0].flags, res[0].bytes), points

    def resume(self, K, points):
        n = (self.height - 1) // K + 1
        work = (SeekWork * n)()
        for i in range(n):
            last = i + 1 == n
            work[i] = SeekWork(0, i * K, min(self.height, (i + 1) * K), i * K, END if last else COMPARE, 0,
                               (i - 1) * self.point_bytes if i else 0, 0 if last else i * self.point_bytes)
        keep, px = [], np.zeros(self.row * self.height, dtype=np.uint8)
        res = (emu_bind.ScanResult * n)()
        lib().emu_seek_resume(self.desc(px, keep), work, res, n, points.ctypes.data_as(C.c_void_p))
        return px, [(r.errc, r.flags, r.bytes) for r in res]


def _case(seed):
    rng = random.Random(seed)
    bits = rng.choice([2, 8, 12, 16])
    comps = rng.choice([1, 2, 3, 4])
    ilv = 0 if comps == 1 else rng.choice([0, 1, 2])
    near = min(rng.choice([0, 0, 1, 2, 3]), ((1 << bits) - 1) // 2)
    preset = None
    if rng.random() < 0.3 and bits == 8:
        preset = (0, 5, 11, 40, rng.choice([32, 64, 100]))
    return dict(width=rng.choice([1, 5, 17, 33]), height=rng.choice([7, 13, 20]), bits=bits, comps=comps, ilv=ilv, near=near,
                seed=rng.randrange(1000), kind=rng.choice(["mixed", "noise", "zero"]), preset=preset), rng.choice([1, 3, 4, 6])


CASES = [_case(s) for s in range(30)]


@pytest.mark.parametrize("case", CASES, ids=[f"s{i}" for i in range(len(CASES))])
def test_emit_and_resume_match_the_plain_decoder(case):
    p, K = case
    s = Scan(**p)
    want, want_r = s.plain()
    assert want_r[0] == 0
    px, r, points = s.emit(K)
    assert r == want_r
    assert px.tobytes() == want.tobytes()
    got, results = s.resume(K, points)
    assert got.tobytes() == want.tobytes()
    for e, f, _ in results[:-1]:
        assert e == 0 and f & CHECKED and not f & MISMATCH
    assert results[-1] == want_r


def _points(s, K):
    return s.emit(K)[2]


@pytest.mark.parametrize("how", ["context", "sample", "position", "swap", "foreign"])
def test_tampered_points_are_caught_by_their_interval(how):
    K = 4
    s = Scan(48, 24, 8, 1, 0, 0, seed=11)
    points = _points(s, K).copy()
    pb = s.point_bytes
    j = 2  # the tampered point: interval j ends at it, interval j + 1 starts from it (0-based: point j starts row (j + 1) K)
    if how == "context":
        points[j * pb + 7 * 8] ^= 0x04  # A of context 7
    elif how == "sample":
        points[j * pb + LINE_OFF + 20] ^= 0x01
    elif how == "position":
        at = j * pb + pb - 24 + 16
        points[at] = points[at] - 1 if points[at] > 0 else 1
    elif how == "swap":
        a, b = points[j * pb:(j + 1) * pb].copy(), points[(j + 2) * pb:(j + 3) * pb].copy()
        points[j * pb:(j + 1) * pb], points[(j + 2) * pb:(j + 3) * pb] = b, a
    else:
        points = _points(Scan(48, 24, 8, 1, 0, 0, seed=12), K)
    _, results = s.resume(K, points)
    caught = [i for i, (e, f, _) in enumerate(results[:-1]) if e != 0 or f & MISMATCH]
    assert j in caught or j + 1 in caught, (how, results)
