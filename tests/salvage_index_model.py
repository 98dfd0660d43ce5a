"""Salvage decode through the seek-point index (charls_amd.h part 2h) as a model, for the tests (test_salvage_index_cpu.py,
test_gpu_salvage_index.py).  Nothing here comes from the code under test:

  * the sound pixels are the oracle's decode of the sound stream;
  * the byte range of every interval comes from the reader positions an index holds (the layouts of host/seek_index.h and
    device/seek_decode.h, read here with struct): interval i of a scan runs from the position of point i to that of point
    i + 1, the first from 0 and the last to the segment's length;
  * the damage operators place their damage at least MARGIN bytes from both ends of an interval's range -- the reader's
    64-bit cache is part of the state that is compared, so bytes nearer to a seek point belong to two intervals -- and the
    expectation is then exact: that interval is lost (2), the intervals above it are proven (0), those below are kept on
    the index's word (4), kept rows are the sound rows and lost rows the fill;
  * the prefix expectation is the oracle's own behaviour: what it leaves in a buffer before it raises."""
from __future__ import annotations

import ctypes as C
import random
import struct
from dataclasses import dataclass

import numpy as np

KEPT, LOST, NOT_REACHED, ON_INDEX, PREFIX = 0, 2, 3, 4, 5
NONE = 0xFFFFFFFF
MARGIN = 16

INDEX_HEADER, INDEX_SCAN, LINE_OFF, READER_BYTES = 72, 24, 2992, 24


# ---- the index ------------------------------------------------------------------------------------------------------------

@dataclass
class IndexView:
    lines: int           # K
    width: int
    height: int
    bits: int
    components: int
    ilv: int
    point_bytes: int
    segments: list       # per scan: the length of its entropy-coded segment
    positions: list      # per scan: the reader position of every seek point, from the segment's first byte


def read_index(index: bytes) -> IndexView:
    assert index[:8] == b"JLSSEEK\0"
    version, lines, width, height, bits, comps, ilv = struct.unpack_from("<IIIIiii", index, 8)
    scans, point_bytes = struct.unpack_from("<II", index, 60)
    assert version == 1
    planes = 1 if ilv == 0 else comps
    line = (planes * (width + 2) * (2 if bits > 8 else 1) + 7) & ~7
    assert point_bytes == LINE_OFF + line + READER_BYTES
    segments, counts = [], []
    for c in range(scans):
        length, _, points, _ = struct.unpack_from("<QQII", index, INDEX_HEADER + c * INDEX_SCAN)
        segments.append(length)
        counts.append(points)
    at = INDEX_HEADER + scans * INDEX_SCAN
    positions = []
    for c in range(scans):
        here = []
        for _ in range(counts[c]):
            here.append(struct.unpack_from("<Q", index, at + point_bytes - READER_BYTES)[0])
            at += point_bytes
        positions.append(here)
    assert at == len(index)
    return IndexView(lines, width, height, bits, comps, ilv, point_bytes, segments, positions)


@dataclass
class Sound:
    """A sound stream, its index, and where its intervals lie."""
    jls: bytes
    index: bytes
    view: IndexView
    pixels: bytes        # the oracle's decode, rows packed
    starts: list         # per scan: offset of its first entropy-coded byte in jls
    headers: list        # per scan: offset of its SOS marker
    row_bytes: int       # of one row of one scan

    @property
    def scans(self):
        return len(self.starts)

    @property
    def intervals(self):
        return -(-self.view.height // self.view.lines)

    def rows_of(self, i):
        return min(self.view.lines, self.view.height - i * self.view.lines)

    def span(self, c, i):
        """[a, b): the bytes of jls between the reader positions that bound interval i of scan c."""
        pos = [0] + self.view.positions[c] + [self.view.segments[c]]
        return self.starts[c] + pos[i], self.starts[c] + pos[i + 1]


def sound(jls: bytes, index: bytes) -> Sound:
    import jls_container
    import oracle_bind as ob
    view = read_index(index)
    cont = jls_container.parse(jls)
    starts = [s.data_start for s in cont.scans]
    headers = []
    for c, s in enumerate(cont.scans):
        headers.append(jls.rfind(b"\xff\xda", 0 if c == 0 else cont.scans[c - 1].data_end, s.data_start))
        assert s.data_end - s.data_start == view.segments[c], (c, s.data_end - s.data_start, view.segments[c])
    assert len(starts) == len(view.segments) and all(len(p) == -(-view.height // view.lines) - 1 for p in view.positions)
    bps = 2 if view.bits > 8 else 1
    row = view.width * bps * (1 if view.ilv == 0 else view.components)
    return Sound(jls, index, view, ob.decode(jls)[1].tobytes(), starts, headers, row)


# ---- damage ---------------------------------------------------------------------------------------------------------------

@dataclass
class Damaged:
    data: bytes
    raw: np.ndarray      # scans x N: KEPT, LOST or NOT_REACHED per interval, before kept ones below a loss become ON_INDEX


def _room(s: Sound, c, j, count):
    a, b = s.span(c, j)
    lo, hi = a + MARGIN, b - MARGIN - count
    assert lo <= hi, f"interval {j} of scan {c} has {b - a} bytes: no room for {count} with the margin"
    return lo, hi


def has_room(s: Sound, c, j, count):
    a, b = s.span(c, j)
    return a + MARGIN <= b - MARGIN - count


def _blank(s: Sound):
    return np.full((s.scans, s.intervals), KEPT, dtype=np.uint8)


def merge(s: Sound, *damages):
    """Several damages of one stream (none of them a cut or a destroyed header)."""
    data = bytearray(s.jls)
    raw = _blank(s)
    for d in damages:
        assert len(d.data) == len(s.jls)
        for k, (x, y) in enumerate(zip(d.data, s.jls)):
            if x != y:
                data[k] = x
        raw = np.maximum(raw, d.raw)
    return Damaged(bytes(data), raw)


def zero4(s: Sound, j, scan=0):
    """Four zero bytes in the middle of interval j."""
    lo, hi = _room(s, scan, j, 4)
    at = (lo + hi) // 2
    while at <= hi and s.jls[at:at + 4] == bytes(4):
        at += 1
    assert at <= hi
    data = bytearray(s.jls)
    data[at:at + 4] = bytes(4)
    raw = _blank(s)
    raw[scan, j] = LOST
    return Damaged(bytes(data), raw)


def overwrite16(s: Sound, j, seed, scan=0):
    """Sixteen bytes from a seeded generator somewhere in interval j."""
    lo, hi = _room(s, scan, j, 16)
    rng = random.Random(seed)
    at = rng.randint(lo, hi)
    noise = bytes(rng.randrange(256) for _ in range(16))
    assert noise != s.jls[at:at + 16]
    data = bytearray(s.jls)
    data[at:at + 16] = noise
    raw = _blank(s)
    raw[scan, j] = LOST
    return Damaged(bytes(data), raw)


def cut(s: Sound, j, scan=0):
    """The stream ends in the middle of interval j and is closed with FF D9 (never a bare cut: the oracle's documented
    deviation).  Every interval that starts below the cut is not reached, and so is every later scan."""
    lo, hi = _room(s, scan, j, 0)
    at = (lo + hi) // 2
    while at > lo and s.jls[at - 1] == 0xFF:
        at -= 1
    raw = _blank(s)
    raw[scan, j] = LOST
    raw[scan, j + 1:] = NOT_REACHED
    raw[scan + 1:, :] = NOT_REACHED
    return Damaged(s.jls[:at] + b"\xff\xd9", raw)


def destroy_sos(s: Sound, scan=1):
    """The SOS marker segment of `scan` overwritten: an EOI marker and zeros.  That scan and the ones behind it are not
    reached."""
    a, b = s.headers[scan], s.starts[scan]
    data = bytearray(s.jls)
    data[a:b] = b"\xff\xd9" + bytes(b - a - 2)
    raw = _blank(s)
    raw[scan:, :] = NOT_REACHED
    return Damaged(bytes(data), raw)


# ---- expectations ---------------------------------------------------------------------------------------------------------

@dataclass
class Expected:
    status: np.ndarray   # scans x N (index mode), scans (prefix mode)
    pixels: bytes
    report: tuple        # (state, intervals, intervals_lost, rows_lost, first_lost_row, reserved)
    alternatives: list = None  # prefix mode: every (status, report) that says the same about every row (expected_prefix)


def _sample(s: Sound, fill):
    return int(fill).to_bytes(2, "little") if s.view.bits > 8 else bytes([fill])


def statuses(raw):
    """Kept intervals below a lost one are kept on the index's word."""
    out = raw.copy()
    for c in range(raw.shape[0]):
        proven = True
        for i in range(raw.shape[1]):
            if raw[c, i] == KEPT and not proven:
                out[c, i] = ON_INDEX
            proven = proven and raw[c, i] == KEPT
    return out


def expected_index(s: Sound, raw, fill) -> Expected:
    status = statuses(raw)
    out = bytearray(s.pixels)
    sample = _sample(s, fill)
    plane = s.view.height * s.row_bytes
    lost = rows_lost = 0
    first = NONE
    for c in range(s.scans):
        for i in range(s.intervals):
            if status[c, i] in (KEPT, ON_INDEX):
                continue
            a = c * plane + i * s.view.lines * s.row_bytes
            n = s.rows_of(i) * s.row_bytes
            out[a:a + n] = sample * (n // len(sample))
            lost += 1
            rows_lost += s.rows_of(i)
            first = min(first, i * s.view.lines)
    return Expected(status, bytes(out), (1, s.scans * s.intervals, lost, rows_lost, first, 0))


def oracle_leaves(data: bytes, size: int, background: int):
    """(errc, what jls_oracle_decode leaves in a buffer of `size` bytes that held `background`)."""
    import oracle_bind as ob
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.full(size, background, dtype=np.uint8)
    q = ob.Params()
    rc = ob.lib().jls_oracle_decode(src.ctypes.data, src.nbytes, out.ctypes.data, out.nbytes, 0, C.byref(q))
    return rc, out.tobytes()


def oracle_rows(s: Sound, data: bytes):
    """Per scan: how many leading rows the oracle wrote before it raised -- the rows on which a decode into zeros and a
    decode into 0xFF agree -- and the rows themselves."""
    rc0, zeros = oracle_leaves(data, len(s.pixels), 0x00)
    rc1, ones = oracle_leaves(data, len(s.pixels), 0xFF)
    assert rc0 == rc1 and rc0 != 0
    plane = s.view.height * s.row_bytes
    rows = []
    for c in range(s.scans):
        r = 0
        while r < s.view.height:
            a = c * plane + r * s.row_bytes
            if zeros[a:a + s.row_bytes] != ones[a:a + s.row_bytes]:
                break
            r += 1
        rows.append(r)
    return rows, zeros


def expected_prefix(s: Sound, data: bytes, fill) -> Expected:
    """Scan c fails after r rows: scans before it are whole, its rows [0, r) are the oracle's, the rest is fill.  The rows
    and the pixels are exact.  Which scan failed cannot be read off a buffer where a scan has all its rows and the next one
    none -- the error came behind the last row of the one (5 with r = height), in the first row of the other (5 with
    r = 0), or no header of the other was found (the one whole, the other 3): `alternatives` lists the (status, report)
    pairs that say the same about every row, `status` and `report` are the first of them."""
    rows, left = oracle_rows(s, data)
    h, S = s.view.height, s.scans
    c = next((k for k in range(S) if rows[k] < h), None)
    assert all(r == 0 for r in rows[(S if c is None else c) + 1:])
    forms = []
    if c is None:
        forms = [[KEPT] * (S - 1) + [PREFIX], [KEPT] * S]
    elif rows[c] > 0 or c == 0:
        forms = [[KEPT] * c + [PREFIX] + [NOT_REACHED] * (S - c - 1)]
    else:
        forms = [[KEPT] * c + [PREFIX] + [NOT_REACHED] * (S - c - 1), [KEPT] * (c - 1) + [PREFIX] + [NOT_REACHED] * (S - c),
                 [KEPT] * c + [NOT_REACHED] * (S - c)]
    sample = _sample(s, fill)
    plane = h * s.row_bytes
    keep = sum(rows[:S if c is None else c + 1]) * s.row_bytes
    assert keep == (S * plane if c is None else c * plane + rows[c] * s.row_bytes)
    n = len(s.pixels) - keep
    pixels = left[:keep] + sample * (n // len(sample))
    rows_lost = S * h - sum(rows)
    first = NONE if rows_lost == 0 else min(r for r in rows if r < h)
    alternatives = [(np.array(f, dtype=np.uint8), (3, S, sum(1 for v in f if v != KEPT), rows_lost, first, 0)) for f in forms]
    return Expected(alternatives[0][0], pixels, alternatives[0][1], alternatives)


def prefix_matches(exp: Expected, status, report, reserved=0):
    """Is (status, report) one of the forms the oracle's buffer admits?"""
    return any(list(status) == st.tolist() and tuple(report) == rp[:5] + (reserved,) for st, rp in exp.alternatives)
