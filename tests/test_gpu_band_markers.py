"""Row bands through restart markers (charls_amd.h part 2m): charls_amd_decode_rows_batch_device_ragged_markers against
charls_amd_decode_rows_batch_device_ragged and against the pixels.

Streams are coded by this library's ragged encoder with restart intervals; what they hold is what the oracle decodes from
them (which, lossless, is the source).  Bands go to a canary buffer, a region per entry -- a base off a 16-byte boundary, padded
rows, the smallest legal capacity -- and the whole buffer is compared: the rows of every band, and every byte that is no row.
  * every one of the 153 bands of a 33 x 17 frame in one call, at restart intervals of 1, 2, 5 and 16 lines;
  * a frame whose markers wrap around RST7;
  * wide samples, planar / line / sample interleaved colour, near-lossless, 16-bit rows at an odd address (no route: the existing
    path's result), each with a band of inner intervals only, one with two edges and one inside a single interval;
  * strides R + 1, roundup(R, 16) + 16 and the smallest capacity;
  * a batch that mixes frames on the route with frames that never take it;
  * damage: outside the band (the one difference from the existing call), inside it, to a marker, to a marker's number, a
    stream cut short -- decodes that return an error code, nothing else;
  * the edge area is a work area, and without room for it the frames come back right the existing way.
GPU only."""
import numpy as np
import pytest

import jls_container
import oracle_bind as ob
import strided
from charls_amd import batch, capi, synth

pytestmark = pytest.mark.gpu

SUCCESS, INVALID_ARGUMENT = 0, 101
CANARY = strided.CANARY
GUARD = 64


@pytest.fixture(scope="module")
def lib():
    L = capi.load_product()
    assert L.lib.charls_amd_device_status() == 0
    return L


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def G(width, height, bits=8, comps=1, ilv=0):
    return strided.Geometry(width, height, bits, comps, ilv)


_coded = {}


def coded(torch, lib, g, ri, near=0, seed=1):
    """(stream, pixels): the ragged encoder's stream of a `mixed` frame with a restart interval of `ri` lines (0: none) and
    the oracle's decode of it.  Coded once per parameter set, shared, never changed."""
    key = (g, ri, near, seed)
    if key not in _coded:
        img = synth.frame_numpy(g.width, g.height, seed=seed, bits=g.bits, components=g.comps, kind="mixed", interleaved=g.ilv != 0)
        frame = torch.from_numpy(img.view(np.int16) if img.dtype == np.uint16 else img).cuda().contiguous()
        packed = torch.zeros(8 * g.packed + 4096, dtype=torch.uint8, device="cuda")
        p = batch.codec_params(g.width, g.height, g.bits, g.comps, g.ilv, near, restart_interval=ri)
        got = batch.encode_batch_ragged([frame], p, packed, lib=lib)
        torch.cuda.synchronize()
        assert got.errcs.tolist() == [SUCCESS]
        stream = packed[:int(got.sizes[0])].cpu().numpy().tobytes()
        assert jls_container.parse(stream).restart_interval == ri
        pixels = ob.decode(stream)[1].tobytes()
        if near == 0:
            assert pixels == img.tobytes()
        _coded[key] = (stream, pixels)
    return _coded[key]


def band_rows(pixels, g, first, count):
    """The band's rows in decode_rows' layout: (scans * count, R)."""
    a = np.frombuffer(pixels, dtype=np.uint8).reshape(g.rows, g.row)
    scans = g.comps if g.ilv == 0 else 1
    return np.concatenate([a[c * g.height + first:c * g.height + first + count] for c in range(scans)])


def pack(torch, streams):
    """The distinct streams back to back (alignment 1; an entry that repeats a stream repeats its offset), 16 readable bytes
    behind the last."""
    at, blob = {}, b""
    for s in streams:
        if s not in at:
            at[s] = len(blob)
            blob += s
    offsets = np.array([at[s] for s in streams], dtype=np.uint64)
    sizes = np.array([len(s) for s in streams], dtype=np.uint64)
    return torch.from_numpy(np.frombuffer(blob + bytes(16), dtype=np.uint8).copy()).cuda(), offsets, sizes


class Entry:
    def __init__(self, stream, g, first, count, *, pixels=None, stride=None, base=None, capacity=None, index=None):
        self.stream, self.g, self.first, self.count, self.pixels, self.index = stream, g, first, count, pixels, index
        self.scans = g.comps if g.ilv == 0 else 1
        self.stride = g.row + (2 if g.bits > 8 else 3) if stride is None else stride
        self.base = (2 if g.bits > 8 else 1) if base is None else base
        self.need = max(self.stride * count * self.scans - (self.stride - g.row), 0)
        self.capacity = self.need if capacity is None else capacity


def run(torch, lib, call, entries):
    """(errcs, the canary buffer on the host, where every entry's region starts)."""
    blob, offsets, sizes = pack(torch, [e.stream for e in entries])
    at, size = [], 0
    for e in entries:
        at.append(size + GUARD + e.base)
        size += (GUARD + e.base + max(e.need, e.capacity) + GUARD + 15) & ~15
    device = torch.full((size,), CANARY, dtype=torch.uint8, device="cuda")
    assert device.data_ptr() % 16 == 0
    errcs = call(blob, offsets, sizes, [e.index for e in entries], [e.first for e in entries], [e.count for e in entries],
                 [device[a:] for a in at], strides=[e.stride for e in entries], capacities=[e.capacity for e in entries], lib=lib)
    torch.cuda.synchronize()
    return errcs, device.cpu().numpy(), at


ARGUMENT_ERRORS = (INVALID_ARGUMENT, strided.INVALID_ARGUMENT_SIZE, strided.INVALID_ARGUMENT_STRIDE)


def expected(entries, at, size, errcs, got):
    """The buffer as it must be: the rows of every band that came back with success, canaries everywhere else.  Of a band that
    was refused for its arguments nothing is written.  The rows of a band whose decode failed may hold anything (a first
    attempt may have written them): they are taken from `got`."""
    want = np.full(size, CANARY, dtype=np.uint8)
    for e, a, errc in zip(entries, at, errcs):
        if errc in ARGUMENT_ERRORS:
            continue
        rows = band_rows(e.pixels, e.g, e.first, e.count) if errc == SUCCESS else None
        for r in range(e.scans * e.count):
            span = slice(a + r * e.stride, a + r * e.stride + e.g.row)
            want[span] = rows[r] if rows is not None else got[span]
    return want


def both(torch, lib, entries):
    """The new call and the existing one on the same entries: ((errcs, buffer), (errcs, buffer)), each buffer held against
    the pixels of the bands that succeeded and against its canaries."""
    out = []
    for call in (batch.decode_rows_batch_ragged_markers, batch.decode_rows_batch_ragged):
        errcs, got, at = run(torch, lib, call, entries)
        want = expected(entries, at, got.size, errcs, got)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (call.__name__, errcs.tolist(), bad[:8].tolist(), at)
        out.append((errcs.tolist(), got))
    return out


def same(torch, lib, entries):
    """Both calls agree errc for errc, and -- both buffers being what `expected` says -- byte for byte but for the rows of the
    bands whose decode failed.  Returns the errcs."""
    (new_errcs, new_got), (old_errcs, old_got) = both(torch, lib, entries)
    assert new_errcs == old_errcs
    if all(e == SUCCESS or e in ARGUMENT_ERRORS for e in new_errcs):
        assert new_got.tobytes() == old_got.tobytes()
    return new_errcs


def met(e, ri):
    return (e.first + e.count - 1) // ri - e.first // ri + 1


# ---- every band of a frame ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ri", [1, 2, 5, 16])
def test_every_band_of_a_frame_in_one_call(torch, lib, ri):
    g = G(33, 17)
    stream, pixels = coded(torch, lib, g, ri)
    entries = [Entry(stream, g, first, count, pixels=pixels) for first in range(17) for count in range(1, 17 - first + 1)]
    assert len(entries) == 153
    before = capi.band_marker_counters(lib)
    new_errcs, new_got, _ = run(torch, lib, batch.decode_rows_batch_ragged_markers, entries)
    after = capi.band_marker_counters(lib)
    old_errcs, old_got, at = run(torch, lib, batch.decode_rows_batch_ragged, entries)
    assert new_errcs.tolist() == [SUCCESS] * 153 and old_errcs.tolist() == [SUCCESS] * 153
    want = expected(entries, at, new_got.size, new_errcs, new_got)
    assert new_got.tobytes() == want.tobytes()      # the source rows, and every canary
    assert new_got.tobytes() == old_got.tobytes()   # byte for byte the existing call
    assert after["frames"] - before["frames"] == 153
    assert after["intervals"] - before["intervals"] == sum(met(e, ri) for e in entries)
    assert after["fallback_frames"] == before["fallback_frames"]
    # one marker search (one scan ordinal) and one decode launch (one kernel specialisation) for all 153
    assert after["launches"] - before["launches"] == 2


def test_marker_numbers_wrap(torch, lib):
    g = G(33, 40)
    stream, pixels = coded(torch, lib, g, 2)
    body = stream[jls_container.parse(stream).scans[0].data_start:]
    assert sum(1 for i in range(len(body) - 1) if body[i] == 0xFF and 0xD0 <= body[i + 1] <= 0xD7) == 19
    entries = [Entry(stream, g, first, count, pixels=pixels) for first, count in [(0, 3), (15, 2), (16, 2), (17, 4), (38, 2), (0, 40)]]
    before = capi.band_marker_counters(lib)
    assert same(torch, lib, entries) == [SUCCESS] * 6
    after = capi.band_marker_counters(lib)
    assert after["frames"] - before["frames"] == 6 and after["fallback_frames"] == before["fallback_frames"]


# ---- kinds -------------------------------------------------------------------------------------------------------------------

BANDS = [(4, 8), (2, 9), (5, 2)]  # at 4 lines per interval: inner intervals only, two edges around an inner one, inside one interval
KINDS = {
    "gray12": (G(33, 17, 12), 0, {}, True),
    "gray16": (G(33, 17, 16), 0, {}, True),
    "gray16_odd": (G(33, 17, 16), 0, dict(base=1, stride=2 * 33 + 3), False),  # the serial kernels: no route
    "rgb_planar": (G(33, 17, 8, 3, 0), 0, {}, True),
    "rgb_line": (G(33, 17, 8, 3, 1), 0, {}, True),
    "rgb_sample": (G(33, 17, 8, 3, 2), 0, {}, True),
    "rgb16_planar": (G(19, 17, 16, 3, 0), 0, {}, True),
    "near3": (G(33, 17), 3, {}, True),
    "near3_rgb_sample": (G(33, 17, 8, 3, 2), 3, {}, True),
}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_kinds(torch, lib, kind):
    g, near, where, on_route = KINDS[kind]
    stream, pixels = coded(torch, lib, g, 4, near)
    entries = [Entry(stream, g, first, count, pixels=pixels, **where) for first, count in BANDS]
    before = capi.band_marker_counters(lib)
    assert same(torch, lib, entries) == [SUCCESS] * 3
    after = capi.band_marker_counters(lib)
    scans = g.comps if g.ilv == 0 else 1
    assert after["frames"] - before["frames"] == (3 if on_route else 0)
    assert after["intervals"] - before["intervals"] == (scans * sum(met(e, 4) for e in entries) if on_route else 0)
    assert after["fallback_frames"] == before["fallback_frames"]
    if on_route:
        # a marker search per scan ordinal, then ONE decode launch, edges and inner intervals together: what picks a kernel looks
        # at an address only for 16-bit rows at odd ones, and the bands of wide samples here lie at even addresses and strides
        # as the edge area does
        assert after["launches"] - before["launches"] == scans + 1


# ---- strides -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g", [G(33, 17), G(33, 17, 16), G(33, 17, 8, 3, 0), G(33, 17, 8, 3, 2)], ids=["gray8", "gray16", "planar", "sample"])
def test_strides_and_the_smallest_capacity(torch, lib, g):
    stream, pixels = coded(torch, lib, g, 4)
    up = (g.row + 15) & ~15
    entries = []
    for stride in (g.row + (2 if g.bits > 8 else 1), up + 16, g.row):
        for base in ((0, 2) if g.bits > 8 else (0, 1)):
            entries += [Entry(stream, g, first, count, pixels=pixels, stride=stride, base=base) for first, count in BANDS + [(16, 1), (0, 17)]]
    before = capi.band_marker_counters(lib)
    assert same(torch, lib, entries) == [SUCCESS] * len(entries)  # (every byte that is no row of a band is a canary still)
    after = capi.band_marker_counters(lib)
    assert after["frames"] - before["frames"] == len(entries) and after["fallback_frames"] == before["fallback_frames"]
    # a capacity one byte below the band, a stride one byte below the row: that frame alone, and nothing of it is written
    short = [Entry(stream, g, 2, 9, pixels=pixels), Entry(stream, g, 2, 9, pixels=pixels), Entry(stream, g, 2, 9, pixels=pixels, stride=g.row - 1),
             Entry(stream, g, 2, 9, pixels=pixels)]
    short[1].capacity -= 1
    errcs = same(torch, lib, short)
    assert errcs == [SUCCESS, strided.INVALID_ARGUMENT_SIZE, strided.INVALID_ARGUMENT_STRIDE, SUCCESS]


# ---- a mixed batch -----------------------------------------------------------------------------------------------------------

def test_mixed_batch(torch, lib):
    g = G(33, 17)
    restart_a, pixels_a = coded(torch, lib, g, 4, seed=11)
    restart_b, pixels_b = coded(torch, lib, G(40, 23, 8, 3, 0), 3, seed=12)
    plain, pixels_plain = coded(torch, lib, g, 0, seed=13)
    indexed, pixels_indexed = coded(torch, lib, g, 0, seed=14)
    tall, pixels_tall = coded(torch, lib, g, 17, seed=15)       # the interval is the frame: no marker
    taller, pixels_taller = coded(torch, lib, g, 40, seed=16)   # an interval beyond the frame
    blob, offsets, sizes = pack(torch, [indexed])
    _, errcs, built = batch.index_batch_packed(blob, offsets, sizes, 4, lib=lib)
    assert errcs.tolist() == [SUCCESS] and len(built[0]) > 96  # an index with seek points
    _, errcs, pointless = batch.index_batch_packed(*pack(torch, [restart_a]), 4, lib=lib)
    assert errcs.tolist() == [SUCCESS] and 0 < len(pointless[0]) <= 96  # the index of a restart stream: no seek points
    entries = [
        Entry(restart_a, g, 2, 9, pixels=pixels_a),
        Entry(plain, g, 2, 9, pixels=pixels_plain),
        Entry(indexed, g, 5, 7, pixels=pixels_indexed, index=built[0]),
        Entry(restart_b, G(40, 23, 8, 3, 0), 7, 11, pixels=pixels_b),
        Entry(tall, g, 2, 9, pixels=pixels_tall),
        Entry(taller, g, 0, 17, pixels=pixels_taller),
        Entry(restart_a[:10], g, 2, 9, pixels=pixels_a),               # a truncated header
        Entry(restart_a, g, 16, 5, pixels=pixels_a),                   # a band beyond the height
        Entry(restart_a, g, 0, 17, pixels=pixels_a, index=pointless[0]),  # an index without seek points: the route all the same
    ]
    on_route = 3
    before = capi.band_marker_counters(lib)
    (new_errcs, new_got), (old_errcs, old_got) = both(torch, lib, entries)
    after = capi.band_marker_counters(lib)
    assert new_errcs == old_errcs and new_got.tobytes() == old_got.tobytes()
    assert [e == SUCCESS for e in new_errcs] == [True, True, True, True, True, True, False, False, True]
    assert new_errcs[7] == INVALID_ARGUMENT
    assert after["frames"] - before["frames"] == on_route and after["fallback_frames"] == before["fallback_frames"]


# ---- damage ------------------------------------------------------------------------------------------------------------------

class Damaged:
    """33 x 40 at 4 lines per interval: ten intervals, nine markers."""

    def __init__(self, torch, lib):
        self.g = G(33, 40)
        self.stream, self.pixels = coded(torch, lib, self.g, 4, seed=21)
        start = jls_container.parse(self.stream).scans[0].data_start
        s = self.stream
        self.marks = [i for i in range(start, len(s) - 1) if s[i] == 0xFF and 0xD0 <= s[i + 1] <= 0xD7]
        assert len(self.marks) == 9 and [s[m + 1] for m in self.marks] == [0xD0 + (k & 7) for k in range(9)]
        self.bounds = [start] + [m + 2 for m in self.marks]  # where interval j starts
        self.ends = self.marks + [len(s) - 2]                # ... and ends (the EOI behind the last)

    def zeroed(self, interval):
        """Four bytes in the middle of the interval zeroed, at least 4 bytes away from any marker."""
        a, b = self.bounds[interval], self.ends[interval]
        assert b - a >= 12 + 4
        mid = (a + b) // 2 - 2
        assert mid - a >= 4 and b - (mid + 4) >= 4 and any(self.stream[mid:mid + 4])
        return self.stream[:mid] + bytes(4) + self.stream[mid + 4:]


@pytest.fixture(scope="module")
def damaged(torch, lib):
    return Damaged(torch, lib)


BAND = (17, 6)  # rows 17 .. 22: intervals 4 and 5, both edges


def test_damage_outside_the_band_is_not_looked_at(torch, lib, damaged):
    d = damaged
    entries = [Entry(d.zeroed(8), d.g, *BAND, pixels=d.pixels),   # below the band
               Entry(d.zeroed(1), d.g, *BAND, pixels=d.pixels),   # above it
               Entry(d.stream, d.g, *BAND, pixels=d.pixels)]
    before = capi.band_marker_counters(lib)
    (new_errcs, _), (old_errcs, _) = both(torch, lib, entries)  # (`both` holds the rows of every success against the sound pixels)
    after = capi.band_marker_counters(lib)
    assert new_errcs == [SUCCESS, SUCCESS, SUCCESS]
    assert old_errcs[0] != SUCCESS and old_errcs[1] != SUCCESS and old_errcs[2] == SUCCESS  # the contract's one difference
    assert after["frames"] - before["frames"] == 3 and after["fallback_frames"] == before["fallback_frames"]


def test_damage_inside_a_band_interval(torch, lib, damaged):
    d = damaged
    for interval in (4, 5):
        entries = [Entry(d.stream, d.g, *BAND, pixels=d.pixels), Entry(d.zeroed(interval), d.g, *BAND, pixels=d.pixels)]
        before = capi.band_marker_counters(lib)
        errcs = same(torch, lib, entries)
        after = capi.band_marker_counters(lib)
        assert errcs[0] == SUCCESS and errcs[1] != SUCCESS
        assert after["frames"] - before["frames"] == 2 and after["fallback_frames"] - before["fallback_frames"] == 1


@pytest.mark.parametrize("what", ["marker_gone", "wrong_number", "cut_short"])
def test_damaged_markers_and_a_short_stream_go_the_existing_way(torch, lib, damaged, what):
    d = damaged
    m = d.marks[2]  # above the band
    broken = {"marker_gone": d.stream[:m] + b"\x00\x00" + d.stream[m + 2:],
              "wrong_number": d.stream[:m + 1] + bytes([0xD5]) + d.stream[m + 2:],
              "cut_short": d.stream[:(d.bounds[8] + d.ends[8]) // 2]}[what]
    entries = [Entry(broken, d.g, *BAND, pixels=d.pixels), Entry(d.stream, d.g, *BAND, pixels=d.pixels)]
    before = capi.band_marker_counters(lib)
    errcs = same(torch, lib, entries)
    after = capi.band_marker_counters(lib)
    assert errcs[1] == SUCCESS  # (one frame's failure never changes another frame's result)
    assert errcs[0] != SUCCESS
    assert after["frames"] - before["frames"] == 2 and after["fallback_frames"] - before["fallback_frames"] == 1


# ---- work areas --------------------------------------------------------------------------------------------------------------

def test_the_edge_area_is_a_work_area(torch, lib):
    g = G(512, 64)
    stream, pixels = coded(torch, lib, g, 16, seed=31)
    entries = [Entry(stream, g, 8, 16, pixels=pixels), Entry(stream, g, 16, 16, pixels=pixels)]  # two edges of 16 rows; none
    batch.release_work_areas(lib)
    held = batch.work_area_bytes(lib)
    before = capi.band_marker_counters(lib)
    errcs, got, at = run(torch, lib, batch.decode_rows_batch_ragged_markers, entries)
    assert errcs.tolist() == [SUCCESS, SUCCESS] and got.tobytes() == expected(entries, at, got.size, errcs, got).tobytes()
    assert capi.band_marker_counters(lib)["frames"] - before["frames"] == 2
    assert batch.work_area_bytes(lib) >= held + 2 * 16 * 512
    batch.release_work_areas(lib)
    assert batch.work_area_bytes(lib) <= held
    # no room for one edge (a quarter of the limit is less than the 256 bytes an edge takes at the least): the frame with edges
    # goes the existing way, the one without them the route
    batch.set_workspace_limit(512, lib)
    try:
        before = capi.band_marker_counters(lib)
        errcs, got, at = run(torch, lib, batch.decode_rows_batch_ragged_markers, entries)
        after = capi.band_marker_counters(lib)
    finally:
        batch.set_workspace_limit(0, lib)
        batch.release_work_areas(lib)
    assert errcs.tolist() == [SUCCESS, SUCCESS] and got.tobytes() == expected(entries, at, got.size, errcs, got).tobytes()
    assert after["frames"] - before["frames"] == 1 and after["fallback_frames"] == before["fallback_frames"]
