"""The two kernels behind the salvage decode through the seek-point index (charls_amd.h part 2h) on the CPU harness
(tests/emu/emu_salvage_index_driver.cpp: scan_seek_decode.hip and salvage_intervals.hip compiled for the host):
  * decode_scans_wave_resume's prefix mode reports the row of the first error at the row the oracle stops at -- on a seeded
    sweep of damaged streams over every form and damage operator of tests/test_gpu_salvage_index.py -- and an item that ends
    sound is as kResumeEnd;
  * judge_and_fill's new criteria keep only checked, matching, error-free results, fill from the named row on, and touch
    nothing but lost rows in a canary arena (rows at odd bases, 8 and 16 bit, the widths of test_emu_salvage.py's fill test);
  * with today's argument values judge_and_fill gives part 2g's verdicts (tests/test_emu_salvage.py and
    tests/test_emu_seek_index.py run both kernels on all their cases with today's values as well);
  * seek points of a sound stream, the stream damaged, every interval resumed and judged as the host does it: the status
    bytes and pixels of tests/salvage_index_model.py.
Streams from the oracle's encoder, seek points from the emulated emit kernel.  Test infrastructure only."""
import ctypes as C
import os
import random
import struct

import numpy as np
import pytest

import emu_bind
import jls_container
import oracle_bind as ob
import salvage_index_model as sim
import strided
from test_emu_seek_index import SeekWork
from test_emu_serial_kernels import _stream_copy

DESC = np.dtype(emu_bind.ScanDesc)
RESULT = np.dtype(emu_bind.ScanResult)
BAND, COMPARE, END, PREFIX_MODE = 0, 1, 2, 3
WIDE, BY_INDEX, BY_PREFIX = 1, 2, 4
ENDS_IN_NEXT_POINT = 0xFFFFFFFFFFFFFFFF

# name -> (width, height, bits, components, interleave mode, NEAR): the one-scan forms of tests/test_gpu_salvage_index.py (a
# planar frame's scans are scans of one component: the first form)
FRAMES = {
    "gray8": (70, 40, 8, 1, 0, 0),
    "gray12": (70, 40, 12, 1, 0, 0),
    "gray8_near2": (70, 40, 8, 1, 0, 2),
    "rgb_line": (35, 24, 8, 3, 1, 0),
    "rgb_sample": (35, 24, 8, 3, 2, 0),
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = emu_bind._build_and_load("emu_salvage_index_driver.cpp",
                                        os.path.join(emu_bind.ROOT, "tests", "_emu_build", "libjls_emu_salvage_index.so"))
        assert _lib.emu_sizeof_seek_work() == C.sizeof(SeekWork) and _lib.emu_sizeof_scan_result() == RESULT.itemsize
        _lib.emu_seek_point_bytes.restype = _lib.emu_seek_reader_off.restype = C.c_size_t
        _lib.emu_ends_in_next_point.restype = C.c_uint64
        assert _lib.emu_mode_prefix() == PREFIX_MODE and _lib.emu_rule_by_index() == BY_INDEX and _lib.emu_rule_by_prefix() == BY_PREFIX
        assert _lib.emu_ends_in_next_point() == ENDS_IN_NEXT_POINT
        vp, u32 = C.c_void_p, C.c_uint32
        _lib.emu_salvage_judge.argtypes = [vp, u32, u32, vp, vp, vp, u32, u32, C.c_uint64]
        _lib.emu_salvage_judge.restype = None
    return _lib


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


class Coded:
    """An oracle-coded frame of one scan, its seek points from the emulated emit kernel and the index they make."""

    def __init__(self, name, K=4, seed=7):
        w, h, bits, comps, ilv, near = FRAMES[name]
        g = strided.Geometry(w, h, bits, comps, ilv)
        self.g, self.K, self.near = g, K, near
        self.jls = ob.encode(strided.mixed(g, seed), near_lossless=near, **g.kw())
        cont = jls_container.parse(self.jls)
        self.pc = jls_container.validated_pc(cont.pc, bits, near)
        self.start, self.end = cont.scans[0].data_start, cont.scans[0].data_end
        self.planes = 1 if ilv == 0 else comps
        self.N = -(-h // K)
        self.point_bytes = lib().emu_seek_point_bytes(w, self.planes, int(bits > 8))
        self.points = np.zeros(max(1, self.N - 1) * self.point_bytes, dtype=np.uint8)
        keep, px = [], np.zeros(g.row * h, dtype=np.uint8)
        res = (emu_bind.ScanResult * 1)()
        lib().emu_seek_emit(self.desc(px, self.jls, keep), res, _ptr(self.points), K)
        assert (res[0].errc, res[0].bytes) == (0, self.end - self.start)
        head = b"JLSSEEK\0" + struct.pack("<IIIIiiii", 1, K, w, h, bits, comps, ilv, near) + \
            struct.pack("<iiiii", self.pc[1], self.pc[2], self.pc[3], self.pc[4], 0) + struct.pack("<III", 1, self.point_bytes, 0)
        index = head + struct.pack("<QQII", self.end - self.start, 0, self.N - 1, 0) + self.points[:(self.N - 1) * self.point_bytes].tobytes()
        self.sound = sim.sound(self.jls, index)
        assert px.tobytes() == self.sound.pixels

    def desc(self, pixels, data, keep, stride=None):
        g = self.g
        return (emu_bind.ScanDesc * 1)(emu_bind.make_desc(g.width, g.height, g.comps if g.ilv else 1, g.ilv, g.bits, self.near, 0, self.pc, 0,
                                                          pixels, stride or g.row, _stream_copy(data, self.start), keep))

    def resume(self, data, work, pixels=None):
        """The work items on the scan of `data`: (pixels, [(errc, flags, bytes)])."""
        n = len(work)
        items = (SeekWork * n)(*work)
        keep = []
        px = np.full(self.g.row * self.g.height, 0xA5, dtype=np.uint8) if pixels is None else pixels
        res = (emu_bind.ScanResult * n)()
        lib().emu_seek_resume(self.desc(px, data, keep), items, res, n, _ptr(self.points))
        return px, [(r.errc, r.flags, r.bytes) for r in res]

    def from_the_top(self, data, mode):
        return self.resume(data, [SeekWork(0, 0, self.g.height, 0, mode, 0, 0, 0)])


_coded = {}


def coded(name, K=4) -> Coded:
    if (name, K) not in _coded:
        _coded[name, K] = Coded(name, K)
    return _coded[name, K]


# ---- the resume kernel's prefix mode ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(FRAMES))
def test_prefix_mode_on_a_sound_stream_is_resume_end(name):
    c = coded(name)
    px_end, r_end = c.from_the_top(c.jls, END)
    px, r = c.from_the_top(c.jls, PREFIX_MODE)
    assert r == r_end == [(0, 1, c.end - c.start)]
    assert px.tobytes() == px_end.tobytes() == c.sound.pixels


def _damaged(c: Coded, k, rng):
    s = c.sound
    op = k % 3
    places = [i for i in range(s.intervals) if sim.has_room(s, 0, i, (4, 16, 0)[op])]
    j = places[rng.randrange(len(places))]
    return sim.zero4(s, j) if op == 0 else (sim.overwrite16(s, j, k) if op == 1 else sim.cut(s, j))


def test_prefix_rows_equal_the_oracles_on_a_seeded_sweep():
    """225 damaged streams, every form, every operator: the row count the kernel reports is the count of rows the oracle wrote
    before it raised, and those rows are the oracle's.  (A disagreement would be a finding about the exact decoder's error
    detection.)"""
    rng = random.Random(77)
    names = list(FRAMES)
    compared, wrong = 0, []
    for k in range(225):
        c = coded(names[k % len(names)])
        d = _damaged(c, k // len(names), rng)
        rc, _ = sim.oracle_leaves(d.data, len(c.sound.pixels), 0)
        if rc == 0:
            continue  # (damage the reference cannot see either)
        rows, left = sim.oracle_rows(c.sound, d.data)
        px, [(errc, flags, count)] = c.from_the_top(d.data, PREFIX_MODE)
        compared += 1
        n = rows[0] * c.g.row
        if errc == 0 or count != rows[0] or px[:n].tobytes() != left[:n] or not (px[n:] == 0xA5).all():
            wrong.append((k, names[k % len(names)], errc, count, rows[0]))
    assert compared >= 200 and not wrong, (compared, wrong[:5])


def test_other_modes_report_no_rows():
    """An error under today's modes leaves bytes 0, as ever."""
    c = coded("gray8")
    d = sim.zero4(c.sound, 5)
    for mode in (BAND, COMPARE, END):
        _, [(errc, _, count)] = c.resume(d.data, [SeekWork(0, 0, c.g.height, 0, mode, 0, 0, 0)])
        assert errc != 0 and count == 0


# ---- judge_and_fill's criteria ---------------------------------------------------------------------------------------------

def _judge(results, expect, status, rule, *, lines=2, w=24, short=1, fill=0x3C):
    """One scan of len(results) intervals of `lines` rows (the last `short` rows short) of w bytes: (status, rows filled)."""
    N = len(results)
    height = N * lines - short
    arena = np.full(N * lines * w + 64, 0xA5, dtype=np.uint8)
    first = (-arena.ctypes.data) % 16 + 16
    parents = np.zeros(1, dtype=DESC)
    parents[0] = (w, height, 1, 0, 8, 0, 0, 3, 7, 21, 64, lines, arena.ctypes.data + first, w, 0, 100, 0)
    res = np.zeros(N, dtype=RESULT)
    res[:] = results
    exp = np.array(expect, dtype=np.uint64)
    st = np.array(status, dtype=np.uint8)
    lib().emu_salvage_judge(_ptr(parents), N, 1, _ptr(res), _ptr(exp), _ptr(st), fill, rule, w)
    body = arena[first:first + height * w].reshape(height, w)
    assert (arena[:first] == 0xA5).all() and (arena[first + height * w:] == 0xA5).all()
    filled, sample = [], fill & 0xFF
    for r in range(height):
        assert (body[r] == sample).all() or (body[r] == 0xA5).all(), r
        if (body[r] == sample).all():
            filled.append(r)
    return st.tolist(), filled


def test_index_criterion_keeps_only_checked_matching_error_free_results():
    E = ENDS_IN_NEXT_POINT
    results = [(0, 1 | 4, 0),      # compared, equal: kept
               (0, 1, 0),          # not compared: lost
               (0, 1 | 4 | 2, 0),  # compared, different: lost
               (5, 1 | 4, 0),      # an error: lost
               (0, 1 | 4, 77),     # kept (the count means nothing between points)
               (0, 1 | 2, 0),      # different and not marked as compared: lost
               (0, 1 | 4, 0),      # not launched by the host: stays 3
               (0, 1, 50)]         # the last interval: the scan ended where the index says
    status, filled = _judge(results, [E] * 7 + [50], [0, 0, 0, 0, 0, 0, 3, 0], BY_INDEX)
    assert status == [0, 2, 2, 2, 0, 2, 3, 0]
    assert filled == [2, 3, 4, 5, 6, 7, 10, 11, 12, 13]
    for last, verdict in (((0, 1, 49), 2), ((0, 1, 51), 2), ((5, 1, 50), 2), ((0, 1 | 4, 50), 0), ((0, 1, 0), 2)):
        status, filled = _judge([(0, 5, 0), last], [E, 50], [0, 0], BY_INDEX)
        assert status == [0, verdict] and filled == ([2] if verdict else [])


def test_flag_bit_2_is_undecided_under_part_2g_and_checked_under_the_index():
    """seek::kSeekChecked has the value of fast::kFastRetry."""
    results, expect = [(0, 4, 50), (0, 1 | 4, 50)], [50, 50]
    assert _judge(results, expect, [0, 0], 0)[0] == [2, 2]
    assert _judge(results, [ENDS_IN_NEXT_POINT] * 2, [0, 0], BY_INDEX)[0] == [0, 0]


def test_todays_values_give_part_2gs_verdicts():
    """tests/test_emu_salvage.py's judge case, on this library, for wide = 0 and 1."""
    results = [(0, 0, 50), (0, 0, 49), (0, 0, 51), (5, 0, 50), (0, 4, 50), (0, 8, 50), (0, 0, 0), (0, 3, 50), (4, 0, 0)]
    expect = [50] * 6 + [0] + [50] * 2
    for wide in (0, 1):
        status, filled = _judge(results, expect, [0] * 6 + [1] + [0] * 2, wide, fill=0x3C3C)
        assert status == [0, 2, 2, 2, 2, 2, 1, 0, 2]
        assert filled == [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16]


def test_prefix_criterion_fills_from_the_named_row():
    """One interval per scan, its length the scan's height."""
    for named, want_status, first_filled in ((0, 5, 0), (1, 5, 1), (6, 5, 6), (7, 5, 7), (9, 5, 7)):
        status, filled = _judge([(5, 1, named)], [0], [0], BY_PREFIX, lines=7, short=0)
        assert status == [want_status] and filled == list(range(first_filled, 7)), named
    assert _judge([(0, 1, 123)], [0], [0], BY_PREFIX, lines=7, short=0) == ([0], [])            # the scan ended: whole
    assert _judge([(0, 1, 123)], [0], [3], BY_PREFIX, lines=7, short=0) == ([3], list(range(7)))  # not reached: all rows


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("width", [1, 15, 16, 17, 150])
def test_new_criteria_touch_nothing_but_the_lost_rows(bits, width):
    """Two scans of 11 rows at every stride class and base (16-bit rows at odd bases too: the fill stores bytes).  Index rule:
    intervals of 4, some lost.  Prefix rule: scan 0 from row 5 on, scan 1 not reached."""
    g = strided.Geometry(width, 11, bits, 2, 0)
    fill = 0x5B if bits == 8 else 0x1C7
    sample = bytes([fill]) if bits == 8 else fill.to_bytes(2, "little")
    wide = WIDE if bits > 8 else 0
    E = ENDS_IN_NEXT_POINT
    row = g.row
    for stride in (row, row + 1, row + 13, ((row + 15) & ~15) + 16):
        for base in strided.BASES:
            lay = strided.Layout(g, stride, strided.need(g, stride), base, 1, tight=True)
            for rule in (BY_INDEX, BY_PREFIX):
                arena = lay.blank()
                lines, N = (4, 3) if rule == BY_INDEX else (11, 1)
                parents = np.zeros(2, dtype=DESC)
                for c in range(2):
                    parents[c] = (width, g.height, 1, 0, bits, 0, 0, 3, 7, 21, 64, lines, arena.ctypes.data + lay.row_offset(0, c * g.height),
                                  stride, 0, 100, 0)
                results = np.zeros((2, N), dtype=RESULT)
                if rule == BY_INDEX:
                    results[:] = [[(0, 5, 0), (0, 7, 0), (0, 1, 9)], [(3, 5, 0), (0, 5, 0), (0, 1, 10)]]
                    expect = np.array([[E, E, 10], [E, E, 10]], dtype=np.uint64)
                    status = np.array([[0, 0, 0], [0, 3, 0]], dtype=np.uint8)
                    want_status = [[0, 2, 2], [2, 3, 0]]
                    lost_rows = [(0, r) for r in range(4, 11)] + [(1, r) for r in range(0, 8)]
                else:
                    results[:] = [[(5, 1, 5)], [(0, 1, 0)]]
                    expect = np.zeros((2, 1), dtype=np.uint64)
                    status = np.array([[0], [3]], dtype=np.uint8)
                    want_status = [[5], [3]]
                    lost_rows = [(0, r) for r in range(5, 11)] + [(1, r) for r in range(11)]
                want = arena.copy()
                for c, r in lost_rows:
                    at = lay.row_offset(0, c * g.height + r)
                    want[at:at + row] = np.frombuffer(sample * width, dtype=np.uint8)
                lib().emu_salvage_judge(_ptr(parents), N, 2, _ptr(results), _ptr(expect), _ptr(status), fill, wide | rule, row)
                bad = np.flatnonzero(arena != want)
                assert bad.size == 0, f"rule {rule} stride {stride} base {base}: first wrong byte at {int(bad[0])} = {lay.where(int(bad[0]))}"
                assert status.tolist() == want_status


# ---- from seek points to verdicts, as the host does it ---------------------------------------------------------------------------

def _salvage(c: Coded, data, fill):
    """The host's work list for one scan: an interval whose point puts the reader beyond the bytes that are left is an idle
    item with status 3.  Returns (status, pixels)."""
    s, g, pb = c.sound, c.g, c.point_bytes
    reader_at = lib().emu_seek_reader_off(g.width, c.planes, int(g.bits > 8))
    left = len(data) - c.start
    work, status, expect = [], [], []
    for i in range(c.N):
        last = i + 1 == c.N
        launched = i == 0 or struct.unpack_from("<Q", c.points, (i - 1) * pb + reader_at)[0] <= left
        work.append(SeekWork(0, i * c.K, min(g.height, (i + 1) * c.K), i * c.K, END if last else COMPARE, 0, (i - 1) * pb if i else 0,
                             0 if last else i * pb) if launched else SeekWork(0, 0, 0, 0, BAND, 0, 0, 0))
        status.append(0 if launched else 3)
        expect.append(c.end - c.start if last else ENDS_IN_NEXT_POINT)
    px = np.full(g.row * g.height, 0xA5, dtype=np.uint8)
    _, results = c.resume(data, work, px)
    parents = np.zeros(1, dtype=DESC)
    parents[0] = (g.width, g.height, g.comps if g.ilv else 1, g.ilv, g.bits, c.near, 0, c.pc[1], c.pc[2], c.pc[3], c.pc[4] & 0xFF, c.K,
                  px.ctypes.data, g.row, 0, left, 0)
    res = np.zeros(c.N, dtype=RESULT)
    res[:] = results
    st, ex = np.array(status, dtype=np.uint8), np.array(expect, dtype=np.uint64)
    lib().emu_salvage_judge(_ptr(parents), c.N, 1, _ptr(res), _ptr(ex), _ptr(st), fill, (WIDE if g.bits > 8 else 0) | BY_INDEX, g.row)
    return st, px


END_TO_END = [("gray8", 4, lambda s: sim.zero4(s, 5)), ("gray8", 4, lambda s: sim.zero4(s, 0)), ("gray8", 4, lambda s: sim.overwrite16(s, 9, 4)),
              ("gray8", 7, lambda s: sim.cut(s, 3)), ("gray8", 7, lambda s: sim.zero4(s, 5)), ("gray12", 4, lambda s: sim.zero4(s, 4)),
              ("gray12", 4, lambda s: sim.cut(s, 6)), ("gray8_near2", 4, lambda s: sim.overwrite16(s, 2, 8)),
              ("rgb_line", 4, lambda s: sim.merge(s, sim.zero4(s, 1), sim.zero4(s, 4))), ("rgb_sample", 4, lambda s: sim.zero4(s, 5)),
              ("rgb_sample", 4, lambda s: sim.cut(s, 2))]


@pytest.mark.parametrize("k", range(len(END_TO_END)))
def test_intervals_are_kept_and_lost_as_the_model_says(k):
    name, K, make = END_TO_END[k]
    c = coded(name, K)
    d = make(c.sound)
    assert sim.oracle_leaves(d.data, len(c.sound.pixels), 0)[0] != 0
    fill = 0x5B if c.g.bits == 8 else 0x1C7
    status, px = _salvage(c, d.data, fill)
    exp = sim.expected_index(c.sound, d.raw, fill)
    assert status.tolist() == d.raw[0].tolist()
    assert px.tobytes() == exp.pixels
    # the sound stream: every interval kept
    status, px = _salvage(c, c.jls, fill)
    assert not status.any() and px.tobytes() == c.sound.pixels
