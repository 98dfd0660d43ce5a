"""The salvage kernels on the CPU harness (salvage_intervals.hip compiled for the host, tests/emu/emu_salvage_driver.cpp):
the marker search and the planner against the pure-Python model of tests/salvage_model.py, the judge with fabricated
results of the interval scans, the fill in a canary arena of which every byte outside the lost rows must survive.
Test infrastructure only."""
import ctypes as C
import os

import numpy as np
import pytest

import emu_bind
import salvage_model as sm
import strided

DESC = np.dtype(emu_bind.ScanDesc)
RESULT = np.dtype(emu_bind.ScanResult)


class Segment(C.Structure):  # must mirror salvage::Segment (salvage_intervals.hip)
    _fields_ = [("end", C.c_uint64), ("marks", C.c_uint32), ("overflow", C.c_uint32)]


SEGMENT = np.dtype(Segment)
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = emu_bind._build_and_load("emu_salvage_driver.cpp", os.path.join(emu_bind.ROOT, "tests", "_emu_build", "libjls_emu_salvage.so"))
        assert _lib.emu_sizeof_scan_result() == RESULT.itemsize and _lib.emu_sizeof_segment() == SEGMENT.itemsize
        assert DESC.itemsize == C.sizeof(emu_bind.ScanDesc)
        vp, u32 = C.c_void_p, C.c_uint32
        _lib.emu_salvage_find.argtypes = [vp, vp, u32, vp, u32]
        _lib.emu_salvage_plan.argtypes = _lib.emu_salvage_plan_replayed.argtypes = [vp, vp, u32, vp, u32, vp, vp, vp, vp, u32]
        _lib.emu_salvage_judge.argtypes = [vp, u32, u32, vp, vp, vp, u32, u32, C.c_uint64]
        for fn in (_lib.emu_salvage_find, _lib.emu_salvage_plan, _lib.emu_salvage_plan_replayed, _lib.emu_salvage_judge):
            fn.restype = None
    return _lib


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


HEIGHT_LINES, STRIDE = 3, 40  # rows per interval and the pixel stride of the planner's fabricated scans


def _plan(sequences, N, *, last_rows=2, cap=None, dead=()):
    """Runs plan_salvage on one fabricated scan per marker-number sequence (all with N intervals) and compares every
    sub-descriptor, expected length, provisional status byte and (p, q) with the model.  The markers of a scan are given to
    the planner as the search would have recorded them: at most `cap` = N + 7, `overflow` set when there were more.
    `dead`: indices of scans without a stream (not reached)."""
    cap = N + 7 if cap is None else cap
    scans = len(sequences)
    height = (N - 1) * HEIGHT_LINES + last_rows
    rng = np.random.default_rng(N * 1000 + scans)
    longest = max(len(s) for s in sequences)
    room = 8 * (longest + 2) + 16  # bytes per scan: pieces of 1..6 bytes, a marker behind each
    arena = np.full(scans * room + 64, 0x11, dtype=np.uint8)
    base = arena.ctypes.data
    parents = np.zeros(scans, dtype=DESC)
    marks = np.zeros((scans, cap), dtype=np.uint32)
    segments = np.zeros(scans, dtype=SEGMENT)
    layouts = []
    for s, numbers in enumerate(sequences):
        at, positions = 0, []
        lengths = rng.integers(1, 7, len(numbers) + 1)
        for k, n in enumerate(numbers):
            at += int(lengths[k])
            arena[s * room + at], arena[s * room + at + 1] = 0xFF, 0xD0 + n
            positions.append(at)
            at += 2
        end = at + int(lengths[-1])
        arena[s * room + end], arena[s * room + end + 1] = 0xFF, 0xD9
        capacity = 0 if s in dead else end + 2 + int(rng.integers(0, 3))
        parents[s] = (8, height, 1, 0, 8, 0, 0, 3, 7, 21, 64, HEIGHT_LINES, 0x100000 + s * 0x10000, STRIDE, base + s * room, capacity, 0)
        recorded = positions[:cap]
        marks[s, :len(recorded)] = recorded
        segments[s] = (0 if s in dead else end, 0 if s in dead else len(recorded), int(len(positions) > cap and s not in dead))
        layouts.append((positions, end, capacity))
    subs = np.zeros((scans, N), dtype=DESC)
    expect = np.full((scans, N), 0xEE, dtype=np.uint64)
    status = np.full((scans, N), 0xEE, dtype=np.uint8)
    counts = np.zeros((scans, 2), dtype=np.uint32)
    lib().emu_salvage_plan(_ptr(parents), _ptr(marks), cap, _ptr(segments), N, _ptr(subs), _ptr(expect), _ptr(status), _ptr(counts), scans)
    cache = {}
    for s, numbers in enumerate(sequences):
        positions, end, capacity = layouts[s]
        if s in dead:
            assert (status[s] == sm.NOT_REACHED).all() and (subs[s]["height"] == 0).all() and (subs[s]["stream_capacity"] == 0).all()
            continue
        key = tuple(numbers)
        if key not in cache:
            cache[key] = sm.claims(numbers, N, cap)
        p, q, piece_of = cache[key]
        assert (int(counts[s, 0]), int(counts[s, 1])) == (p, q), (N, numbers)
        recorded = positions[:cap]
        starts = [0] + [m + 2 for m in recorded]
        ends = recorded + [end]
        for j in range(N):
            d, k = subs[s, j], piece_of[j]
            assert d["restart_interval"] == 0 and d["pixel_stride"] == STRIDE and d["width"] == 8
            assert d["pixels"] == parents[s]["pixels"] + j * HEIGHT_LINES * STRIDE
            if k is None:
                assert (status[s, j], d["height"], d["stream_capacity"], expect[s, j]) == (sm.UNCLAIMED, 0, 0, 0), (N, numbers, j)
                continue
            want_rows = HEIGHT_LINES if j + 1 < N else last_rows
            assert (status[s, j], d["height"]) == (sm.KEPT, want_rows), (N, numbers, j)
            assert d["stream"] == base + s * room + starts[k], (N, numbers, j, k)
            assert d["stream_capacity"] == min(ends[k] + 2, capacity) - starts[k], (N, numbers, j, k)
            assert expect[s, j] == ends[k] - starts[k], (N, numbers, j, k)


def _plan_all_of_length(N, length, replayed=True):
    """Every sequence of `length` marker numbers on a scan of N intervals, in launches of 2^18 scans: pieces of 2 bytes, so
    piece k starts at 4k and its marker at 4k + 2.  Compared with the model as arrays."""
    codes = np.indices((8,) * length, dtype=np.uint8).reshape(length, -1).T if length else np.zeros((1, 0), dtype=np.uint8)
    cap, last_rows = N + 7, 2
    room, end = 4 * length + 4, 4 * length + 2
    run = lib().emu_salvage_plan_replayed if replayed else lib().emu_salvage_plan
    for first in range(0, len(codes), 1 << 18):
        chunk = codes[first:first + (1 << 18)]
        scans = len(chunk)
        arena = np.full((scans, room), 0x11, dtype=np.uint8)
        arena[:, 2:end:4] = 0xFF
        arena[:, 3:end:4] = 0xD0 + chunk
        arena[:, end], arena[:, end + 1] = 0xFF, 0xD9
        parents = np.zeros(scans, dtype=DESC)
        parents[:] = (8, (N - 1) * HEIGHT_LINES + last_rows, 1, 0, 8, 0, 0, 3, 7, 21, 64, HEIGHT_LINES, 0, STRIDE, 0, room, 0)
        parents["pixels"] = 0x100000 + 0x1000 * np.arange(scans, dtype=np.uint64)
        parents["stream"] = arena.ctypes.data + room * np.arange(scans, dtype=np.uint64)
        marks = np.zeros((scans, cap), dtype=np.uint32)
        marks[:, :length] = 2 + 4 * np.arange(length, dtype=np.uint32)
        segments = np.zeros(scans, dtype=SEGMENT)
        segments["end"], segments["marks"] = end, length
        subs = np.zeros((scans, N), dtype=DESC)
        expect = np.full((scans, N), 0xEE, dtype=np.uint64)
        status = np.full((scans, N), 0xEE, dtype=np.uint8)
        counts = np.zeros((scans, 2), dtype=np.uint32)
        run(_ptr(parents), _ptr(marks), cap, _ptr(segments), N, _ptr(subs), _ptr(expect), _ptr(status), _ptr(counts), scans)
        want_counts = np.zeros((scans, 2), dtype=np.uint32)
        want_piece = np.full((scans, N), -1, dtype=np.int64)
        for s, numbers in enumerate(chunk.tolist()):
            p, q, piece_of = sm.claims(numbers, N)
            want_counts[s] = p, q
            want_piece[s] = [-1 if k is None else k for k in piece_of]
        claimed = want_piece >= 0
        rows = np.where(np.arange(N) + 1 < N, HEIGHT_LINES, last_rows)
        assert np.array_equal(counts, want_counts), (N, length)
        assert np.array_equal(status, np.where(claimed, sm.KEPT, sm.UNCLAIMED)), (N, length)
        assert np.array_equal(subs["height"], np.where(claimed, rows, 0)), (N, length)
        assert np.array_equal(subs["stream_capacity"], np.where(claimed, 4, 0)), (N, length)  # (the piece and the marker behind it)
        assert np.array_equal(expect, np.where(claimed, 2, 0)), (N, length)
        assert np.array_equal(subs["stream"][claimed], (parents["stream"][:, None] + 4 * want_piece.astype(np.uint64))[claimed]), (N, length)
        assert np.array_equal(subs["pixels"], parents["pixels"][:, None] + np.arange(N, dtype=np.uint64) * HEIGHT_LINES * STRIDE)
        assert (subs["restart_interval"] == 0).all() and (subs["pixel_stride"] == STRIDE).all()


def test_planner_exhaustively_up_to_six_intervals():
    """Every sequence of marker numbers of length <= N + 1, N = 2 .. 6 (2.7 million scans), with the lanes of the planner run one
    after the other (emu_salvage_driver.cpp) -- and, up to N = 4, with a thread per lane as well: the two ways must not differ."""
    for N in range(2, 7):
        for length in range(N + 2):
            _plan_all_of_length(N, length)
            if N <= 4:
                _plan_all_of_length(N, length, replayed=False)


def _edits(N, count, seed):
    """Seeded random edits of the sound sequence 0, 1, .. N - 2 (mod 8): deletions, renumberings and insertions, single and
    in runs, at places that put the first mismatch and the matching suffix on either side of the 64-marker chunks."""
    rng = np.random.default_rng(seed)
    sound = [k % 8 for k in range(N - 1)]
    out = [sound]
    for _ in range(count):
        seq = list(sound)
        for _ in range(int(rng.integers(1, 4))):
            kind = int(rng.integers(0, 4))
            at = int(rng.integers(0, len(seq) + 1))
            if kind == 0 and seq:
                del seq[min(at, len(seq) - 1)]
            elif kind == 1 and seq:
                seq[min(at, len(seq) - 1)] = int(rng.integers(0, 8))
            elif kind == 2:
                seq.insert(at, int(rng.integers(0, 8)))
            elif seq:
                run = int(rng.integers(2, 10))
                del seq[min(at, len(seq) - 1):min(at, len(seq) - 1) + run]
        out.append(seq[:N + 7])
    return out


@pytest.mark.parametrize("N", [8, 9, 16, 17, 20, 63, 64, 65, 129, 150])
def test_planner_on_random_edits(N):
    _plan(_edits(N, 300, seed=N), N, last_rows=1 if N % 2 else 3)


def test_planner_hand_worked_cases_and_a_dead_scan():
    N = 20
    sound = [k % 8 for k in range(N - 1)]
    cases = [sound, sound[:5] + sound[6:], sound[:9] + [3] + sound[10:], sound[:2] + [5] + sound[2:], sound[:4] + [4] + sound[4:],
             sound[:3] + sound[11:], sound[:7], sound]
    _plan(cases, N, dead=(7,))


@pytest.mark.parametrize("N", [5, 64, 70])
def test_planner_overflow_beyond_the_cap(N):
    """More than N + 7 markers: the recorded ones count as all of them and nothing is claimed from the back."""
    sound = [k % 8 for k in range(N - 1)]
    longer = [k % 8 for k in range(N + 20)]
    cases = [longer, longer[:N + 8], sound + [7] * 9, [(k + 1) % 8 for k in range(N + 9)], longer[:N + 7]]
    for numbers in cases[:-1]:
        p, q, _ = sm.claims(numbers, N)
        assert q == 0 and p <= N - 1
    _plan(cases, N)


# ---- the marker search ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mis", [0, 1, 7, 15])
def test_search_reports_markers_end_and_overflow(mis):
    rng = np.random.default_rng(40 + mis)
    cap = 12
    streams = []
    for kind in range(6):
        body = bytearray(rng.integers(0, 0x7F, 3000 if kind != 5 else 40, dtype=np.uint8).tobytes())
        n_marks = (5, 12, 13, 30, 0, 3)[kind]
        places = sorted(rng.choice(np.arange(4, len(body) - 8, 4), n_marks, replace=False).tolist()) if n_marks else []
        for i, at in enumerate(places):
            body[at], body[at + 1] = 0xFF, 0xD0 + (i + kind) % 8
        if kind in (0, 2):  # the segment ends at a marker that is no RSTm; restart markers behind it do not count
            end = len(body) - 3 if kind == 0 else places[-1] + 2
            body[end], body[end + 1] = 0xFF, 0xD9 if kind == 0 else 0xDA
            if kind == 0:
                body[end + 2] = 0xFF
        else:
            end = len(body)
            if kind == 3:
                body[-1] = 0xFF  # a lone 0xFF as the last byte of the source is no marker
        streams.append((bytes(body), places, end))
    room = 3200
    arena = np.full(len(streams) * room + 64, 0x22, dtype=np.uint8)
    first = (-arena.ctypes.data) % 16 + 16 + mis
    descs = np.zeros(len(streams), dtype=DESC)
    for s, (body, _, _) in enumerate(streams):
        arena[first + s * room:first + s * room + len(body)] = np.frombuffer(body, dtype=np.uint8)
        descs[s] = (8, 8, 1, 0, 8, 0, 0, 3, 7, 21, 64, 1, 0, 8, arena.ctypes.data + first + s * room, len(body), 0)
    marks = np.full((len(streams), cap), 0xEEEEEEEE, dtype=np.uint32)
    segments = np.zeros(len(streams), dtype=SEGMENT)
    lib().emu_salvage_find(_ptr(descs), _ptr(marks), cap, _ptr(segments), len(streams))
    for s, (body, places, end) in enumerate(streams):
        inside = [p for p in places if p < end]
        assert int(segments[s]["end"]) == end, s
        assert int(segments[s]["marks"]) == min(len(inside), cap) and int(segments[s]["overflow"]) == int(len(inside) > cap), s
        assert marks[s, :min(len(inside), cap)].tolist() == inside[:cap], s
        assert (marks[s, min(len(inside), cap):] == 0xEEEEEEEE).all()


# ---- the judge -------------------------------------------------------------------------------------------------------

def test_judge_keeps_only_exact_clean_results():
    """Fabricated results of eight interval scans: exact and clean; one byte short; one byte long; an error code with the
    exact count; each undecided flag; unclaimed; a harmless flag (kept)."""
    N, lines, w = 9, 2, 24
    arena = np.full(N * lines * w + 64, 0xA5, dtype=np.uint8)
    first = (-arena.ctypes.data) % 16 + 16
    parents = np.zeros(1, dtype=DESC)
    parents[0] = (w, N * lines - 1, 1, 0, 8, 0, 0, 3, 7, 21, 64, lines, arena.ctypes.data + first, w, 0, 100, 0)
    results = np.zeros(N, dtype=RESULT)
    expect = np.full(N, 50, dtype=np.uint64)
    status = np.zeros(N, dtype=np.uint8)
    results[:] = [(0, 0, 50), (0, 0, 49), (0, 0, 51), (5, 0, 50), (0, 4, 50), (0, 8, 50), (0, 0, 0), (0, 3, 50), (4, 0, 0)]
    status[6] = sm.UNCLAIMED
    expect[6] = 0
    want = [sm.KEPT, sm.NOT_EXACT, sm.NOT_EXACT, sm.NOT_EXACT, sm.NOT_EXACT, sm.NOT_EXACT, sm.UNCLAIMED, sm.KEPT, sm.NOT_EXACT]
    before = arena.copy()
    lib().emu_salvage_judge(_ptr(parents), N, 1, _ptr(results), _ptr(expect), _ptr(status), 0x3C, 0, w)
    assert status.tolist() == want
    expected = before
    for j, verdict in enumerate(want):
        rows = lines if j + 1 < N else lines - 1  # the last interval is one row short
        if verdict != sm.KEPT:
            expected[first + j * lines * w:first + (j * lines + rows) * w] = 0x3C
    assert np.array_equal(arena, expected)


# ---- the fill --------------------------------------------------------------------------------------------------------

def _strides(row):
    up = (row + 15) & ~15
    return [row, row + 1, row + 13, up + 16]


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("width", [1, 15, 16, 17, 150])
def test_fill_touches_nothing_but_the_lost_rows(bits, width):
    """Two scans (a planar frame's planes) of 11 rows in intervals of 4 -- the last interval has 3 --, some intervals lost, at
    every stride class and base: the lost rows hold the fill value, little-endian by byte position; every other byte of the
    arena -- kept rows, gaps between rows, guard bands -- survives."""
    g = strided.Geometry(width, 11, bits, 2, 0)
    lines, N = 4, 3
    fill = 0x5B if bits == 8 else 0x1C7
    sample = bytes([fill]) if bits == 8 else fill.to_bytes(2, "little")
    lost = {(0, 1), (0, 2), (1, 0)}  # (scan, interval); scan 1 interval 1 is unclaimed (lost too), the rest are kept
    for stride in _strides(g.row):
        for base in strided.BASES:
            lay = strided.Layout(g, stride, strided.need(g, stride), base, 1, tight=True)
            arena = lay.blank()
            parents = np.zeros(2, dtype=DESC)
            for c in range(2):
                parents[c] = (width, g.height, 1, 0, bits, 0, 0, 3, 7, 21, 64, lines, arena.ctypes.data + lay.row_offset(0, c * g.height), stride,
                              0, 100, 0)
            results = np.zeros((2, N), dtype=RESULT)
            results["bytes"] = 10
            expect = np.full((2, N), 10, dtype=np.uint64)
            status = np.zeros((2, N), dtype=np.uint8)
            for c, j in lost:
                results[c, j]["errc"] = 5
            status[1, 1] = sm.UNCLAIMED
            want = arena.copy()
            for c, j in lost | {(1, 1)}:
                for r in range(j * lines, min((j + 1) * lines, g.height)):
                    at = lay.row_offset(0, c * g.height + r)
                    want[at:at + g.row] = np.frombuffer(sample * width, dtype=np.uint8)
            lib().emu_salvage_judge(_ptr(parents), N, 2, _ptr(results), _ptr(expect), _ptr(status), fill, int(bits > 8), g.row)
            bad = np.flatnonzero(arena != want)
            assert bad.size == 0, f"stride {stride} base {base}: first wrong byte at {int(bad[0])} = {lay.where(int(bad[0]))}"
            assert status.tolist() == [[0, 2, 2], [2, 1, 0]]
