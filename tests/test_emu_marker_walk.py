"""The marker walk of the restart-interval decoder (restart_intervals_decode.hip: find_restart_markers) on the CPU, through
the emulator's emu_find_restart_markers, against a numpy model on synthetic bytes: markers on every boundary the walk has --
a lane's 16 bytes, a chunk of 1 KB, a trip of 4 KB --, every misalignment of the first byte, the lengths around a trip, the end
of the segment, markers that are no RSTm, max_marks, and what may be read.  The cases hold whatever body the kernel has: they
are what keeps a rewrite of the walk in place."""
import ctypes as C

import numpy as np
import pytest

import emu_bind

TOO_MANY = 0xFFFFFFFF


def model(data: np.ndarray):
    """Offsets of the RSTm markers in front of the first marker that is no RSTm: 0xFF followed by a byte >= 0x80, both inside."""
    if data.size < 2:
        return []
    at = np.flatnonzero((data[:-1] == 0xFF) & (data[1:] >= 0x80))
    rst = (data[at + 1] & 0xF8) == 0xD0
    other = np.flatnonzero(~rst)
    return [int(v) for v in (at[:other[0]] if other.size else at)]


def walk(data: np.ndarray, max_marks: int, misalign: int = 0):
    """The kernel on `data` placed `misalign` bytes behind a 16-byte boundary of an arena.  Every byte of the arena that is not
    source is canary, in front of the source and behind the granule that holds its last byte: FF D0 pairs, so that a walk
    which took one of them for a source byte -- the byte behind a last 0xFF, say -- would list a marker the model does not
    have; and nothing of the arena may change."""
    n = int(data.size)
    granules = (misalign + max(n, 1) + 15) // 16
    raw = np.tile(np.array([0xFF, 0xD0], dtype=np.uint8), granules * 8 + 64)
    base = (-raw.ctypes.data) % 16
    raw[base + misalign:base + misalign + n] = data
    before = raw.copy()
    keep = []
    pix = np.zeros(8 * 16, dtype=np.uint8)
    d = emu_bind.make_desc(8, 16, 1, 0, 8, 0, 0, (255, 3, 7, 21, 64), 4, pix, 8, raw, keep)
    d.stream = raw.ctypes.data + base + misalign
    d.stream_capacity = n
    marks = np.full(max(max_marks, 1) + 4, 0xEEEEEEEE, dtype=np.uint32)
    counts = np.full(1, 0x12345678, dtype=np.uint32)
    emu_bind.lib().emu_find_restart_markers(C.byref(d), marks.ctypes.data_as(C.c_void_p), C.c_uint32(max_marks),
                                            counts.ctypes.data_as(C.c_void_p), 1)
    assert (raw == before).all()
    assert (marks[max_marks:] == 0xEEEEEEEE).all(), "a mark beyond max_marks was written"
    count = int(counts[0])
    return count, None if count == TOO_MANY else [int(m) for m in marks[:count]]


def quiet(n: int, seed: int) -> np.ndarray:
    """Bytes without a marker: no 0xFF is followed by a byte >= 0x80, but 0xFF bytes there are (FF 7F, FF 00)."""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, size=n, dtype=np.uint8)
    ff = np.flatnonzero(data[:-1] == 0xFF) if n > 1 else np.array([], dtype=np.int64)
    data[ff + 1] &= 0x7F
    if n and data[-1] == 0xFF:
        data[-1] = 0x7E
    return data


def put(data: np.ndarray, at: int, code: int):
    data[at] = 0xFF
    data[at + 1] = code
    if at > 0 and data[at - 1] == 0xFF:
        data[at - 1] = 0x7E  # (FF FF would be a fill byte: another marker)


def expect(data, max_marks=64, misalign=0):
    want = model(data)
    got = walk(data, max_marks, misalign)
    assert got == ((len(want), want) if len(want) <= max_marks else (TOO_MANY, None)), (got, want)
    return want


@pytest.mark.parametrize("misalign", range(16))
def test_every_misalignment_of_the_first_byte(misalign):
    data = quiet(13000, misalign)
    # the first source byte; then, counted from the 16-byte boundary in front of it, the 0xFF on the last byte of a lane's 16, on
    # the first, on the last of a chunk, on the first, on the last of a trip, on the first, and on the last of the third trip
    places = [0] + [at - misalign for at in (47, 64, 1023, 2048, 4095, 8192, 12287)]
    for k, at in enumerate(places):
        put(data, at, 0xD0 + (k & 7))
    assert expect(data, 64, misalign) == places


@pytest.mark.parametrize("boundary", [16, 1024, 4096, 8192])
@pytest.mark.parametrize("back", [1, 0])
def test_marker_across_and_behind_a_boundary(boundary, back):
    """0xFF on byte boundary - 1 (its number in the next lane, chunk or trip) and on byte boundary."""
    data = quiet(3 * 4096 + 5, boundary + back)
    put(data, boundary - back, 0xD3)
    assert expect(data) == [boundary - back]


@pytest.mark.parametrize("n", [0, 1, 2, 3, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 8193, 12287, 12288, 12289])
@pytest.mark.parametrize("misalign", [0, 5, 15])
def test_lengths_around_a_trip_and_the_end_of_the_segment(n, misalign):
    data = quiet(n, n)
    assert expect(data, 8, misalign) == []
    if n >= 2:
        tail = data.copy()
        put(tail, n - 2, 0xD5)  # an RSTm in the last two bytes
        assert expect(tail, 8, misalign) == [n - 2]
    if n >= 1:
        ends_on_ff = data.copy()
        ends_on_ff[n - 1] = 0xFF  # FF as the very last byte: no marker, whatever lies behind it (the bait: D0)
        if n >= 2 and ends_on_ff[n - 2] == 0xFF:
            ends_on_ff[n - 2] = 0x7E
        assert expect(ends_on_ff, 8, misalign) == []
    if n >= 3:
        both = data.copy()
        put(both, 0, 0xD0)
        both[n - 1] = 0xFF
        if both[n - 2] == 0xFF and n - 2 != 0:
            both[n - 2] = 0x7E
        assert expect(both, 8, misalign) == [0]


def test_another_marker_stops_the_walk_within_a_trip():
    data = quiet(3 * 4096, 7)
    put(data, 100, 0xD0)
    put(data, 102, 0xD9)   # directly behind an RSTm
    put(data, 104, 0xD1)   # same lane, same chunk
    put(data, 1500, 0xD2)  # next chunk of the same trip
    put(data, 5000, 0xD3)  # next trip
    assert expect(data) == [100]
    data = quiet(3 * 4096, 8)
    put(data, 4100, 0xD0)
    put(data, 5200, 0xD1)
    put(data, 6300, 0xC0)  # a marker that is no RSTm in the third chunk of a trip ...
    put(data, 6310, 0xD2)  # ... in front of RSTm bytes of the same lane, of later lanes and of the last chunk
    put(data, 6900, 0xD3)
    put(data, 7300, 0xD4)
    assert expect(data) == [4100, 5200]
    data = quiet(2 * 4096, 9)
    data[0] = 0xFF
    data[1] = 0xFF  # a fill byte is "another marker"
    data[2] = 0xD0
    assert expect(data) == []
    for code in (0x80, 0xCF, 0xD8, 0xFE):
        data = quiet(5000, code)
        put(data, 4095, code)
        put(data, 4200, 0xD0)
        assert expect(data) == []


def test_stuffed_pairs_are_no_markers():
    data = quiet(2 * 4096, 11)
    for at in (15, 16, 1023, 1024, 4095, 4096, 5000):
        data[at] = 0xFF
        data[at + 1] = 0x7F if at % 2 else 0x00
        if data[at - 1] == 0xFF:
            data[at - 1] = 0x7E
    put(data, 6000, 0xD0)
    assert expect(data) == [6000]


def test_max_marks():
    data = quiet(3 * 4096, 13)
    places = [10, 11 + 16, 1023, 1030, 4095, 4097, 4099, 8190, 9000, 12286]
    for k, at in enumerate(places):
        put(data, at, 0xD0 + (k & 7))
    assert model(data) == places
    assert walk(data, len(places)) == (len(places), places)
    assert walk(data, len(places) + 3) == (len(places), places)
    assert walk(data, len(places) - 1) == (TOO_MANY, None)  # exceeded by one
    assert walk(data, 1) == (TOO_MANY, None)
    assert walk(data, 0) == (TOO_MANY, None)
    # ... markers behind the one that ends the segment do not count towards it
    put(data, 4200, 0xD9)
    assert walk(data, 7) == (7, places[:7])


def test_dense_markers_keep_their_order():
    """Every lane of several chunks lists marks: the ordered append across lanes, chunks and trips."""
    data = quiet(3 * 4096 + 77, 17)
    places = list(range(3, data.size - 2, 7))
    for k, at in enumerate(places):
        put(data, at, 0xD0 + (k & 7))
    assert expect(data, len(places), 9) == places
