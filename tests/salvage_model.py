"""The salvage decode of charls_amd.h part 2g as a model, for the tests (tests/test_salvage_cpu.py, test_emu_salvage.py,
test_gpu_salvage.py).  Nothing here comes from the code under test:

  * the claim rule -- which piece of a damaged entropy-coded segment is which restart interval -- in pure Python, written
    the way the header words it (claims are collected, then conflicting ones are struck), not the way the kernel computes it;
  * a builder that puts a DRI stream together from the oracle's coding of every interval as an image of its own;
  * the damage operators of the tests, and what a salvage decode of the damaged stream must return: status bytes, report,
    pixels (the oracle's rows in kept intervals, the fill value elsewhere)."""
from __future__ import annotations

import copy
from dataclasses import dataclass, field

import numpy as np

KEPT, UNCLAIMED, NOT_EXACT, NOT_REACHED = 0, 1, 2, 3
NONE = 0xFFFFFFFF


# ---- the claim rule ----------------------------------------------------------------------------------------------------

def claims(numbers, n_intervals, cap=None):
    """numbers: n_k of the markers FF D0+n_k found in the segment, in order.  Returns (p, q, piece_of): piece_of[j] is the
    piece that claims interval j, or None.  At most `cap` (default N + 7) markers are recorded: with more, the recorded
    ones count as all of them and q = 0."""
    N = n_intervals
    cap = N + 7 if cap is None else cap
    overflow = len(numbers) > cap
    numbers = list(numbers[:cap])
    M = len(numbers)
    most = min(M, N - 1)
    p = 0
    while p < most and numbers[p] == p % 8:
        p += 1
    q = 0
    if not overflow:
        while q < most and numbers[M - 1 - q] == (N - 2 - q) % 8:
            q += 1
    claimed_by_piece = {}  # piece -> set of intervals
    for k in range(p):
        claimed_by_piece.setdefault(k, set()).add(k)
    for t in range(q):
        claimed_by_piece.setdefault(M - t, set()).add(N - 1 - t)
    pieces_of_interval = {}  # interval -> set of pieces
    for piece, wants in claimed_by_piece.items():
        if len(wants) != 1:
            continue  # a piece with two different claims claims nothing
        pieces_of_interval.setdefault(next(iter(wants)), set()).add(piece)
    piece_of = [None] * N
    for interval, pieces in pieces_of_interval.items():
        if len(pieces) == 1:  # an interval claimed by two different pieces is claimed by none
            piece_of[interval] = next(iter(pieces))
    return p, q, piece_of


# ---- streams -----------------------------------------------------------------------------------------------------------

@dataclass
class Scan:
    header: bytes           # the SOS marker segment
    pieces: list            # the entropy-coded bytes of every interval
    numbers: list           # of the markers between them
    tail: bytes = b""       # bytes between the last piece and the next scan's header (none in a sound stream)


@dataclass
class Built:
    prefix: bytes           # SOI .. DRI, up to the first SOS
    scans: list
    height: int
    interval: int
    row_bytes: int          # of one row of one scan in the destination
    pixels: bytes           # the oracle's decode of the sound stream
    kw: dict = field(default_factory=dict)  # of the oracle's encoder for ONE interval of ONE scan (without height)
    end: bytes = b"\xff\xd9"

    @property
    def intervals(self):
        return -(-self.height // self.interval)

    def assemble(self) -> bytes:
        out = bytearray(self.prefix)
        for s in self.scans:
            out += s.header
            for k, piece in enumerate(s.pieces):
                out += piece
                if k < len(s.numbers):
                    out += bytes([0xFF, 0xD0 + s.numbers[k]])
            out += s.tail
        return bytes(out + self.end)

    def copy(self):
        return copy.deepcopy(self)


def build(img, interval, *, bits=8, comps=1, ilv=0, near=0):
    """img: (H, W) for one component, (C, H, W) planar (ilv 0), (H, W, C) interleaved.  The stream any encoder would write
    with DRI = interval: the oracle's coding of every interval as an image of its own, FF D0+(k mod 8) between them."""
    import jls_container
    import oracle_bind as ob
    planar = comps > 1 and ilv == 0
    h, w = (img.shape[1], img.shape[2]) if planar else (img.shape[0], img.shape[1])
    kw = dict(bits_per_sample=bits, component_count=comps, interleave_mode=ilv, near_lossless=near)
    full = ob.encode(np.ascontiguousarray(img), width=w, height=h, **kw)
    cont = jls_container.parse(full)
    first_sos = full.rfind(b"\xff\xda", 0, cont.scans[0].data_start)
    prefix = full[:first_sos] + b"\xff\xdd\x00\x04" + interval.to_bytes(2, "big")
    n = -(-h // interval)
    scans, header_at = [], first_sos
    sub_kw = dict(kw, component_count=1) if planar else kw
    for c, sc in enumerate(cont.scans):
        pieces = []
        for j in range(n):
            rows = img[c, j * interval:(j + 1) * interval] if planar else img[j * interval:(j + 1) * interval]
            s = ob.encode(np.ascontiguousarray(rows), width=w, height=rows.shape[0], **sub_kw)
            ssc = jls_container.parse(s).scans[0]
            pieces.append(s[ssc.data_start:ssc.data_end])
        scans.append(Scan(full[header_at:sc.data_start], pieces, [k % 8 for k in range(n - 1)]))
        header_at = sc.data_end
    bps = (bits + 7) // 8
    b = Built(prefix, scans, h, interval, w * bps * (1 if planar or comps == 1 else comps), b"", dict(sub_kw, width=w))
    b.pixels = ob.decode(b.assemble())[1].tobytes()
    return b


# ---- damage ------------------------------------------------------------------------------------------------------------
# Every operator returns a damaged COPY of the stream's structure; scan 0 unless `scan` says otherwise.

def delete_marker(b: Built, k, scan=0):
    b = b.copy()
    s = b.scans[scan]
    s.pieces[k:k + 2] = [s.pieces[k] + s.pieces[k + 1]]
    del s.numbers[k]
    return b


def delete_markers(b: Built, first, count, scan=0):
    for _ in range(count):
        b = delete_marker(b, first, scan)
    return b


def renumber_marker(b: Built, k, number, scan=0):
    b = b.copy()
    assert b.scans[scan].numbers[k] != number
    b.scans[scan].numbers[k] = number
    return b


def insert_marker(b: Built, j, number, scan=0):
    """FF D0+number in the middle of piece j (at a place where it does not follow a 0xFF)."""
    b = b.copy()
    s = b.scans[scan]
    piece = s.pieces[j]
    at = len(piece) // 2
    while at > 0 and piece[at - 1] == 0xFF:
        at -= 1
    assert 0 < at < len(piece)
    s.pieces[j:j + 1] = [piece[:at], piece[at:]]
    s.numbers.insert(j, number)
    return b


def zero_bytes(b: Built, j, scan=0, count=4):
    """`count` zero bytes in the middle of piece j."""
    b = b.copy()
    s = b.scans[scan]
    piece = bytearray(s.pieces[j])
    at = (len(piece) - count) // 2
    assert at > 0 and bytes(piece[at:at + count]) != bytes(count)
    piece[at:at + count] = bytes(count)
    s.pieces[j] = bytes(piece)
    return b


def cut_inside(b: Built, j, scan=0):
    """The stream ends in the middle of piece j."""
    b = b.copy()
    s = b.scans[scan]
    s.pieces[j + 1:] = []
    s.numbers[j:] = []
    piece = s.pieces[j][:len(s.pieces[j]) // 2]
    while piece and piece[-1] == 0xFF:
        piece = piece[:-1]
    s.pieces[j] = piece
    b.scans[scan + 1:] = []
    b.end = b""
    return b


def cut_behind_marker(b: Built, k, scan=0):
    """The stream ends behind marker k."""
    b = b.copy()
    s = b.scans[scan]
    s.pieces[k + 1:] = [b""]
    s.numbers[k + 1:] = []
    b.scans[scan + 1:] = []
    b.end = b""
    return b


def destroy_sos(b: Built, scan=1):
    """The SOS marker segment of `scan` overwritten: an EOI marker and zeros."""
    b = b.copy()
    b.scans[scan].header = b"\xff\xd9" + bytes(len(b.scans[scan].header) - 2)
    return b


# ---- what a salvage decode of a damaged stream returns --------------------------------------------------------------------

@dataclass
class Expected:
    status: np.ndarray      # scans x N
    pixels: bytes           # the destination, rows packed
    report: tuple           # (state, intervals, intervals_lost, rows_lost, first_lost_row, reserved)
    claimed_damaged: list   # (scan, interval, piece bytes) of claimed pieces that are not the interval's own bytes


def _segment(data: bytes, start: int):
    """The markers FF D0..D7 of the segment that starts at `start` and where it ends."""
    marks, at = [], start
    while at + 1 < len(data):
        if data[at] == 0xFF and data[at + 1] >= 0x80:
            if not 0xD0 <= data[at + 1] <= 0xD7:
                return marks, at
            marks.append(at)
            at += 2
        else:
            at += 1
    return marks, len(data)


def expected(sound: Built, damaged: Built, fill_value, *, sos_valid=None) -> Expected:
    """What the salvage call returns for damaged.assemble(): the segments and their pieces are read from the BYTES, as the
    header describes them; a claimed piece is kept exactly when it is the sound stream's coding of the interval it claims
    (the tests assert with the oracle that every other claimed piece does not decode)."""
    data = damaged.assemble()
    N, scans = sound.intervals, len(sound.scans)
    status = np.full((scans, N), NOT_REACHED, dtype=np.uint8)
    claimed_damaged = []
    at = len(damaged.prefix)
    for c in range(scans):
        header = sound.scans[c].header
        if c >= len(damaged.scans) or data[at:at + len(header)] != header:
            break  # no valid SOS here: the scans from this one on are not reached
        start = at + len(header)
        marks, end = _segment(data, start)
        numbers = [data[m + 1] - 0xD0 for m in marks]
        _, _, piece_of = claims(numbers, N)
        marks = marks[:N + 7]
        bounds = [start] + [m + 2 for m in marks]
        ends = marks + [end]
        for j in range(N):
            k = piece_of[j]
            if k is None:
                status[c, j] = UNCLAIMED
                continue
            piece = data[bounds[k]:ends[k]]
            if piece == sound.scans[c].pieces[j]:
                status[c, j] = KEPT
            else:
                status[c, j] = NOT_EXACT
                claimed_damaged.append((c, j, piece))
        at = end
    rows_of = [min(sound.interval, sound.height - j * sound.interval) for j in range(N)]
    plane = sound.height * sound.row_bytes
    out = bytearray(sound.pixels)
    wide = sound.kw["bits_per_sample"] > 8
    sample = int(fill_value).to_bytes(2, "little") if wide else bytes([fill_value])
    rows_lost, first_lost = 0, NONE
    for c in range(scans):
        for j in range(N):
            if status[c, j] == KEPT:
                continue
            a = c * plane + j * sound.interval * sound.row_bytes
            n = rows_of[j] * sound.row_bytes
            out[a:a + n] = sample * (n // len(sample))
            rows_lost += rows_of[j]
            first_lost = min(first_lost, j * sound.interval)
    lost = int((status != KEPT).sum())
    return Expected(status, bytes(out), (1, scans * N, lost, rows_lost, first_lost, 0), claimed_damaged)


def wrapped(sound: Built, piece: bytes, rows: int) -> bytes:
    """`piece` as the scan data of an image of its own with `rows` rows (what the oracle is asked to decode)."""
    import jls_container
    import oracle_bind as ob
    kw = dict(sound.kw)
    w = kw.pop("width")
    comps = kw["component_count"]
    shape = (rows, w) if comps == 1 else (rows, w, comps)
    blank = np.zeros(shape, dtype=np.uint16 if kw["bits_per_sample"] > 8 else np.uint8)
    s = ob.encode(blank, width=w, height=rows, **kw)
    sc = jls_container.parse(s).scans[0]
    return s[:sc.data_start] + piece + b"\xff\xd9"
