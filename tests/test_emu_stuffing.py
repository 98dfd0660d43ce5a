"""The stuffing corpus (tests/stuffing.py) through the emulated kernels: every reader and writer of the 0xFF stuffing, compiled
for the host (tests/emu), on streams that have a 0xFF in every second to fourth byte -- eight stuffed bits in a 16-byte lane, a
0xFF as the last byte of a lane, of a chunk, as the first coded byte and as the last data byte -- at every misalignment of the
stream's first byte.  tests/test_stuffing_census_cpu.py asserts from the oracle's bytes that the streams reach these cases.

Everything is compared for equality with the oracle: pixels, ScanResult.bytes against the segment's length, errc 0, encoded
bytes.

The thread-per-lane emulation costs seconds a scan, so the work is split into many cases: the single-scan decoders take one
(frame, misalignment) pair a case, every frame at all 16; the group decoder takes the frames of a geometry in 16 rounds, which
move every frame through all 16 (ROUNDS); the seek test resumes every interval, a part of them a case.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import emu_bind
import oracle_bind as ob
import stuffing as st
import test_emu_container as container
import test_emu_group_measure as measure
import test_emu_restart as restart
import test_emu_salvage as salvage
import test_emu_seek_index as seek
from test_emu_corners import Scan, one_by_one
from test_emu_decode_paths import BYTEWISE, DELETE_TRIPS, REFILLS
from test_emu_group_decode import _encode_group, _launch, _launch_pixels

CORPUS = st.CORPUS
TOO_SMALL = 3

_scans = {}


def scans(name, misalignment=None):
    if (name, misalignment) not in _scans:
        cc = st.coded(name)
        _scans[name, misalignment] = [Scan(cc.corner, i, s.data_start, s.data_end, cc.jls, cc.pixels, misalignment)
                                      for i, s in enumerate(cc.scans)]
    return _scans[name, misalignment]


def check_decoded(launch, all_scans, flags=0):
    """`launch(descs)` -> results for `all_scans` at once: errc 0, no flag (the wave decoder: its own, 1), the segment's length,
    the oracle's pixels."""
    keep, outs, descs = [], [], []
    for s in all_scans:
        out, d = s.decode_desc(keep)
        assert d.stream % 16 == s.stream.ctypes.data % 16
        outs.append(out)
        descs.append(d)
    res = launch(descs)
    for s, r, out in zip(all_scans, res, outs):
        where = (s.c.name, s.index, s.stream.ctypes.data % 16)
        assert (r.errc, r.flags, r.bytes) == (0, flags, len(s.segment)), where + (r.errc, r.flags, r.bytes, len(s.segment))
        assert out.tobytes() == s.want, where


def dense(route):
    return st.route_frames(route, "emu", dense=True)


# ---- single-scan decoders -----------------------------------------------------------------------------------------------------

def alignment_cases(route):
    """Every dense frame of the route at every misalignment of its first coded byte, a case each."""
    return [pytest.param(n, m, id=f"{n}-{m}") for n in dense(route) for m in st.MISALIGNMENTS]


@pytest.mark.parametrize("name,m", alignment_cases("fast_decode"))
def test_fast_decoder(name, m):
    """DenseBits::refill of scan_fast_decode.hip: chunks of 1024 bytes."""
    check_decoded(one_by_one("emu_decode_scans_fast"), scans(name, m))


@pytest.mark.parametrize("name,m", alignment_cases("exact_decode"))
def test_wave_decoder(name, m):
    """The exact reader of scan_wave_decode.hip: the 8-byte fill behind any_ff, the byte loop with --valid, end_scan and
    consumed_bytes walking back over 7- and 8-bit bytes."""
    check_decoded(one_by_one("emu_decode_scans_wave"), scans(name, m), flags=1)


@pytest.mark.parametrize("name", dense("serial_decode"))
def test_serial_decoder(name):
    """scan_serial.hip's copy of the exact reader: every frame at every misalignment (a lane, milliseconds)."""
    for m in st.MISALIGNMENTS:
        check_decoded(one_by_one("emu_decode_scans_serial"), scans(name, m))


# ---- the group decoder --------------------------------------------------------------------------------------------------------

GROUPS = (8, 16, 32)
ROUNDS = 16   # launches per geometry: each moves every frame's misalignment on by one and takes the next G


def group_cases():
    """A geometry with several frames: 16 rounds.  A geometry with one frame (the tall flat frames, the odd NEARs): a launch per
    G, with the frame at all 16 misalignments side by side in it."""
    out = []
    for key, names in st.batches(st.route_frames("group_decode", "emu"), "thresholds").items():
        if len(names) > 1:
            out += [pytest.param(names, r, None, id=f"{st.batch_id(key)}-r{r}") for r in range(ROUNDS)]
        else:
            out += [pytest.param(names, None, g, id=f"{st.batch_id(key)}-g{g}") for g in GROUPS]
    return out


def mixed(names, r):
    """The frames of one geometry and one set of thresholds in the corpus' order -- dense frames between their partners --, frame
    j at misalignment 3 j + r."""
    return [s for j, n in enumerate(names) for s in scans(n, (3 * j + r) % 16)]


def test_the_rounds_put_every_frame_at_every_misalignment():
    assert all({(3 * j + r) % 16 for r in range(ROUNDS)} == set(st.MISALIGNMENTS) for j in range(16))


@pytest.mark.parametrize("names,r,group", group_cases())
def test_group_decoder_mixed_wavefronts(names, r, group):
    """refill and refill_bytewise of scan_group_decode.hip.  Lanes with 8 delete trips share a wavefront with lanes that have
    none (`while (__any(...))`), and the flat partner's scan ends while its neighbours are in mid-stream, which sends them to
    the bytewise path (`__all(...)`).  Over the 16 rounds of a geometry every frame stands at every misalignment, and at
    five of them or more with each G; a frame that is alone in its geometry stands at all 16 with every G."""
    L = emu_bind.lib()
    if r is None:
        all_scans = [s for m in st.MISALIGNMENTS for s in scans(names[0], m)]
    else:
        group, all_scans = GROUPS[r % 3], mixed(names, r)
    check_decoded(lambda descs: _launch(L, descs, group), all_scans)


def test_group_decoder_four_wavefronts_a_workgroup():
    """decode_scans_group<S, 32, 1, 4>: eight scans, dense ones and partners, fill the four wavefronts of one workgroup."""
    L = emu_bind.lib()
    names = next(v for k, v in st.batches(st.route_frames("group_decode", "emu"), "thresholds").items() if k[:3] == (128, 96, 8))
    all_scans = (mixed(names, 1) + mixed(names, 8))[:8]

    def waves(descs):
        n = len(descs)
        res = (emu_bind.ScanResult * n)()
        assert L.emu_decode_scans_group_waves((emu_bind.ScanDesc * n)(*descs), res, n, 32, 4) == 0
        return res
    check_decoded(waves, all_scans)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", ["ramp_8", "ramp_8n"])
def test_a_pure_ramp_costs_eight_delete_trips_a_refill(name, group):
    """The path-counting build on a launch of a pure ramp alone, at misalignment 0: every 128-bit refill meets a lane with eight
    stuffed bits, so the delete loop makes 8 trips each time -- not "once or twice" --, and the bytewise refill is for the two
    ends of the stream."""
    L = emu_bind.profile_lib()
    keep = []
    s, = scans(name, 0)
    out, d = s.decode_desc(keep)
    res = (emu_bind.ScanResult * 1)()
    counts = (C.c_ulonglong * 32)()
    assert L.emu_profile_decode_group((emu_bind.ScanDesc * 1)(d), res, 1, group, counts) == 0
    assert (res[0].errc, res[0].flags, res[0].bytes) == (0, 0, len(s.segment)) and out.tobytes() == s.want
    assert counts[REFILLS] - counts[BYTEWISE] >= 1
    assert counts[BYTEWISE] <= 2
    assert counts[DELETE_TRIPS] == 8 * (counts[REFILLS] - counts[BYTEWISE]), list(counts)[:17]


# ---- pixel decoders -----------------------------------------------------------------------------------------------------------

def pixel_cases():
    out = []
    for key, names in st.batches(st.route_frames("pixel_decode", "emu"), "thresholds").items():
        if key[1] > 600 or key[:2] == (16, 2400):
            continue   # (the 4096- and 2400-line frames: the group decoder's; their 600-line likes are here)
        out += [pytest.param(names, g, id=f"{st.batch_id(key)}-g{g}") for g in (8, 32)]
    return out


@pytest.mark.parametrize("names,group", pixel_cases())
def test_pixel_decoders(names, group):
    """scan_group_pixels.hip shares the refill: sample-interleaved lossless frames, near-lossless gray and line-interleaved ones,
    dense frames between their partners."""
    check_decoded(lambda descs: _launch_pixels(emu_bind.lib(), descs, group), mixed(names, group))


# ---- seek points --------------------------------------------------------------------------------------------------------------

class SeekScan(seek.Scan):
    """tests/test_emu_seek_index.py's harness on scan 0 of a frame of the corpus."""

    def __init__(self, name, misalignment):
        s = scans(name, misalignment)[0]
        c = s.c
        self.pc, self.width, self.height, self.bits, self.near, self.ilv = s.pc, c.width, c.height, c.bits, c.near, c.ilv
        self.comps, self.planes, self.row, self.stream = s.nc, s.nc, s.stride, s.stream
        self.point_bytes = seek.lib().emu_seek_point_bytes(c.width, self.planes, int(c.bits > 8))

    def resume_some(self, K, points, which):
        """As resume(), for the intervals `which` (600 wavefronts of the harness cost 18 s: a test takes a part of them);
        returns the pixels and the results."""
        n = (self.height - 1) // K + 1
        work = (seek.SeekWork * len(which))()
        for k, i in enumerate(which):
            last = i + 1 == n
            work[k] = seek.SeekWork(0, i * K, min(self.height, (i + 1) * K), i * K, seek.END if last else seek.COMPARE, 0,
                                    (i - 1) * self.point_bytes if i else 0, 0 if last else i * self.point_bytes)
        keep, px = [], np.zeros(self.row * self.height, dtype=np.uint8)
        res = (emu_bind.ScanResult * len(which))()
        seek.lib().emu_seek_resume(self.desc(px, keep), work, res, len(which), points.ctypes.data_as(C.c_void_p))
        return px, [(r.errc, r.flags, r.bytes) for r in res]


_emitted = {}


def emitted(name, K):
    """The frame's scan at misalignment 5, its harness, and what decode_scans_wave_emit gave with a point every K lines: once
    per (frame, K), shared and left unchanged."""
    if (name, K) not in _emitted:
        s = SeekScan(name, 5)
        _emitted[name, K] = (scans(name, 5)[0], s) + s.emit(K)
    return _emitted[name, K]


PARTS = {1: 6, 7: 1}   # the intervals of a frame are resumed in so many tests: 100 wavefronts of the harness each at K = 1


@pytest.mark.parametrize("K,part", [(K, p) for K, n in PARTS.items() for p in range(n)])
@pytest.mark.parametrize("name", st.SEEK_FLAT)
def test_every_interval_resumed_from_its_point_ends_in_the_next_point_s_state(name, K, part):
    """Resume on the tall flat frames, a line a bit: EVERY interval, resumed from its point, gives the oracle's rows and ends in
    exactly the next point's state; the last one reports the plain decoder's bytes."""
    sc, s, _, r, points = emitted(name, K)
    n = (s.height - 1) // K + 1
    which = list(range(n))[part::PARTS[K]]
    got, results = s.resume_some(K, points, which)
    rows = np.frombuffer(sc.want, dtype=np.uint8).reshape(s.height, s.row)
    for i, res in zip(which, results):
        assert got.reshape(s.height, s.row)[i * K:(i + 1) * K].tobytes() == rows[i * K:(i + 1) * K].tobytes(), i
        if i + 1 == n:
            assert res == r
        else:
            assert res[0] == 0 and res[1] & seek.CHECKED and not res[1] & seek.MISMATCH, (i, res)


def test_the_parts_hold_every_interval():
    for K, n in PARTS.items():
        assert sorted(i for p in range(n) for i in list(range(600))[p::n]) == list(range(600))


@pytest.mark.parametrize("K", [1, 7])
@pytest.mark.parametrize("name", st.SEEK_FLAT)
def test_seek_points_inside_seven_bit_bytes(name, K):
    """Emit on the tall flat frames: decode_scans_wave_emit decodes as the plain decoder does, and its points stand where they
    are wanted."""
    sc, s, px, r, points = emitted(name, K)
    assert r == (0, 1, len(sc.segment)) and px.tobytes() == sc.want
    if st.is_specked(name):
        return
    # a test of the test: the points stand at 7 bit phases or more, and some of them in a byte that follows a 0xFF
    where = [st.current_byte(sc.segment, p, v) for p, _, v in st.reader_states(points, s.point_bytes)]
    assert len({phase for _, phase in where}) >= 7, sorted({phase for _, phase in where})
    assert any(phase and b and sc.segment[b - 1] == 0xFF for b, phase in where)
    assert all(b < len(sc.segment) for b, _ in where)


# ---- restart intervals, salvage, scan end -------------------------------------------------------------------------------------

@pytest.mark.parametrize("lines", st.RESTART_LINES)
@pytest.mark.parametrize("name", st.RESTART_FRAMES)
def test_restart_marker_search_and_interval_descriptors(name, lines):
    """find_restart_markers and build_decode_intervals of restart_intervals_decode.hip, and the search of salvage_intervals.hip,
    on intervals that end in FF xx: the RSTm is the third 0xFF-led pair in a row."""
    seg, at = st.dri_scan(name, lines)
    c = CORPUS[name]
    body = seg + b"\xff\xd9"
    n = len(at) + 1
    for m in st.MISALIGNMENTS:
        assert restart._find(body, n - 1, m) == (n - 1, at), m
    # the descriptors
    keep = []
    buf = np.frombuffer(body + bytes(64), dtype=np.uint8).copy()
    nc = 1 if c.ilv == 0 else c.comps
    stride = c.width * nc * (2 if c.bits > 8 else 1)
    pix = np.zeros(stride * c.height, dtype=np.uint8)
    parent = emu_bind.make_desc(c.width, c.height, nc, c.ilv, c.bits, c.near, 0, st.corners.coding_parameters(c), lines, pix, stride, buf, keep)
    parent.stream_capacity = len(body)
    marks = np.array(at, dtype=np.uint32)
    subs = (emu_bind.ScanDesc * n)()
    emu_bind.lib().emu_build_decode_intervals(C.byref(parent), marks.ctypes.data_as(C.c_void_p), C.c_uint32(n), subs, 1)
    starts = [0] + [a + 2 for a in at]
    assert [s.stream - parent.stream for s in subs] == starts
    assert [s.stream_capacity for s in subs] == [e + 2 - b for b, e in zip(starts, at + [len(seg)])]
    assert [s.height for s in subs] == [min(lines, c.height - j * lines) for j in range(n)]
    # salvage_intervals.hip's search: the same markers, and the segment's end
    arena = np.full(len(body) + 128, 0x22, dtype=np.uint8)
    for m in (0, 9, 15):
        first = (-arena.ctypes.data) % 16 + 16 + m
        arena[first:first + len(body)] = np.frombuffer(body, dtype=np.uint8)
        descs = np.zeros(1, dtype=salvage.DESC)
        descs[0] = (8, 8, 1, 0, 8, 0, 0, 3, 7, 21, 64, 1, 0, 8, arena.ctypes.data + first, len(body), 0)
        found = np.full((1, n + 7), 0xEEEEEEEE, dtype=np.uint32)
        segments = np.zeros(1, dtype=salvage.SEGMENT)
        salvage.lib().emu_salvage_find(salvage._ptr(descs), salvage._ptr(found), n + 7, salvage._ptr(segments), 1)
        assert (int(segments[0]["end"]), int(segments[0]["marks"]), int(segments[0]["overflow"])) == (len(seg), n - 1, 0), m
        assert found[0, :n - 1].tolist() == at


@pytest.mark.parametrize("kernel", ["emu_decode_scans_wave", "emu_decode_scans_serial"])
@pytest.mark.parametrize("name,lines", [("ramp_8", 16), ("ramp_8_specks100", 7), ("ramp_8n_specks30", 16), ("ramp_16_specks30", 7)])
def test_salvage_of_an_interval_damaged_inside_ff_7f(name, lines, kernel):
    """The salvage kernels on a restart-interval stream with four zero bytes over an FF 7F FF 7F of interval 3: the search and the
    planner of salvage_intervals.hip give the sub-scans, an emulated exact decoder decodes every claimed one, judge_and_fill gets
    those results.  Status bytes and pixels are tests/salvage_model.py's: interval 3 is lost and filled, its neighbours, which end
    in FF xx in front of their RSTm, are kept."""
    c = CORPUS[name]
    sound = salvage.sm.build(c.img, lines, bits=c.bits, near=c.near)
    damaged = st.zero_in_stretch(sound, 3)
    fill = 0x1C7 if c.bits > 8 else 0x5B
    exp = salvage.sm.expected(sound, damaged, fill)
    N = sound.intervals
    assert exp.status[0].tolist() == [salvage.sm.NOT_EXACT if j == 3 else salvage.sm.KEPT for j in range(N)]
    data = damaged.assemble()
    start = len(damaged.prefix) + len(damaged.scans[0].header)
    body = np.frombuffer(data[start:] + bytes(64), dtype=np.uint8).copy()
    keep = []
    stride = c.width * (2 if c.bits > 8 else 1)
    pix = np.full(stride * c.height, 0xA5, dtype=np.uint8)
    parent = emu_bind.make_desc(c.width, c.height, 1, 0, c.bits, c.near, 0, st.corners.coding_parameters(c), lines, pix, stride, body, keep)
    parent.stream_capacity = len(data) - start
    parents = np.frombuffer(bytes(parent), dtype=salvage.DESC).copy()
    S = salvage.lib()
    cap = N + 7
    marks = np.zeros((1, cap), dtype=np.uint32)
    segments = np.zeros(1, dtype=salvage.SEGMENT)
    S.emu_salvage_find(salvage._ptr(parents), salvage._ptr(marks), cap, salvage._ptr(segments), 1)
    assert (int(segments[0]["marks"]), int(segments[0]["overflow"])) == (N - 1, 0)
    subs = np.zeros((1, N), dtype=salvage.DESC)
    expect = np.zeros((1, N), dtype=np.uint64)
    status = np.full((1, N), 0xEE, dtype=np.uint8)
    counts = np.zeros((1, 2), dtype=np.uint32)
    S.emu_salvage_plan(salvage._ptr(parents), salvage._ptr(marks), cap, salvage._ptr(segments), N, salvage._ptr(subs), salvage._ptr(expect),
                       salvage._ptr(status), salvage._ptr(counts), 1)
    assert (status == salvage.sm.KEPT).all()   # (provisional: the markers are sound, every interval is claimed)
    assert expect[0].tolist() == [len(p) for p in damaged.scans[0].pieces]
    results = np.zeros((1, N), dtype=salvage.RESULT)
    for j in range(N):
        d = emu_bind.ScanDesc.from_buffer_copy(subs[0, j].tobytes())
        d.line_scratch = parent.line_scratch
        r = (emu_bind.ScanResult * 1)()
        getattr(emu_bind.lib(), kernel)((emu_bind.ScanDesc * 1)(d), r, 1)
        results[0, j] = (r[0].errc, r[0].flags, r[0].bytes)
    S.emu_salvage_judge(salvage._ptr(parents), N, 1, salvage._ptr(results), salvage._ptr(expect), salvage._ptr(status), fill, int(c.bits > 8),
                        stride)
    assert status.tolist() == exp.status.tolist()
    assert pix.tobytes() == exp.pixels


@pytest.mark.parametrize("kernel,flags", [("emu_decode_scans_wave", 1), ("emu_decode_scans_serial", 0)])
@pytest.mark.parametrize("name", st.RESTART_FRAMES)
def test_exact_readers_cross_restart_markers_behind_ff_xx(name, kernel, flags):
    """restart_marker of the exact reader and of its copy in scan_serial.hip, 7 lines an interval."""
    lines = 7
    seg, _ = st.dri_scan(name, lines)
    jls = st.dri_stream(name, lines)
    c = CORPUS[name]
    s = Scan(c, 0, jls.index(seg), jls.index(seg) + len(seg), jls, st.dri_pixels(name, lines), 11)
    keep = []
    out, d = s.decode_desc(keep)
    d.restart_interval = lines
    res = (emu_bind.ScanResult * 1)()
    getattr(emu_bind.lib(), kernel)((emu_bind.ScanDesc * 1)(d), res, 1)
    assert (res[0].errc, res[0].flags, res[0].bytes) == (0, flags, len(seg))
    assert out.tobytes() == s.want


@pytest.mark.parametrize("name", ["ramp_8_specks30", "ramp_8_specks100", "line3_8", "sample3_8_specks10", "ramp_16_specks30"])
def test_restart_interval_encoder(name):
    """restart_intervals_encode.hip joins privately coded intervals that end in FF xx: the oracle's intervals, RSTm between.
    (The harness has this encode for lossless scans.)"""
    lines = 7
    c = CORPUS[name]
    want, _ = st.dri_scan(name, lines)
    keep = []
    nc = 1 if c.ilv == 0 else c.comps
    stride = c.width * nc * (2 if c.bits > 8 else 1)
    pix = np.frombuffer(c.img.tobytes(), dtype=np.uint8).copy()
    out = np.zeros(len(want) + 100, dtype=np.uint8)
    d = emu_bind.make_desc(c.width, c.height, nc, c.ilv, c.bits, c.near, 0, st.corners.coding_parameters(c), lines, pix, stride, out, keep)
    res = (emu_bind.ScanResult * 1)()
    emu_bind.lib().emu_encode_with_restart_intervals(C.byref(d), res, 1, C.c_uint64(stride * lines * 4 + 256))
    assert (res[0].errc, res[0].flags, res[0].bytes) == (0, 0, len(want))
    assert out[:len(want)].tobytes() == want


@pytest.mark.parametrize("name", list(CORPUS))
def test_scan_end_finder(name):
    """find_scan_end of container_kernels.hip on every stream of the corpus, from every start alignment: the first marker
    behind the entropy-coded segment (EOI, or the next scan's SOS), not one of the stuffed 0xFF bytes before it."""
    cc = st.coded(name)
    pieces, stretches, want, at = [], [], [], 0
    for s in cc.scans:
        tail = cc.jls[s.data_start:]
        for m in st.MISALIGNMENTS:
            pad = (-at) % 64 + m
            pieces.append(bytes(pad) + tail)
            stretches.append((at + pad, at + pad + len(tail)))
            want.append(at + pad + s.data_end - s.data_start)
            at += pad + len(tail)
    buf = np.frombuffer(b"".join(pieces) + bytes(64), dtype=np.uint8).copy()
    assert container._search(buf, stretches) == want


# ---- encoders -----------------------------------------------------------------------------------------------------------------
#
# Capacity.  A destination one byte shorter than the segment is destination_too_small, one with 8 bytes to spare succeeds.  In
# between the serial and the group encoder follow the reference's writer, which wants four free bytes at every flush: the
# oracle, pinned to the reference, refuses a destination of exactly the segment's length for these frames, and the kernels'
# verdict is the oracle's size by size (oracle_verdict).  Nothing is ever written behind the destination.

ROOMS = (8, -1, 0, 1, 2, 3, 4)
_verdicts = {}


def oracle_verdict(s, room):
    """What the oracle says to a destination that ends `room` bytes behind the entropy-coded segment of scan `s`: 0, TOO_SMALL,
    or None where it cannot say.  (A plane of a planar frame is coded as an image of its own: the same segment.  The oracle
    writes EOI behind the segment, so with less than 2 bytes of room its refusal may be EOI's: there the verdict is known only
    where 2 bytes are refused too -- a writer that refuses a destination refuses every shorter one.)"""
    c = s.c
    key = (c.name, s.index, max(room, 2))
    if key not in _verdicts:
        planar = c.comps > 1 and c.ilv == 0
        img, kw = (np.ascontiguousarray(c.img[s.index]), dict(c.kw(), component_count=1)) if planar else (c.img, c.kw())
        jls = ob.encode(img, destination_size=8 * img.nbytes + 4096, **kw)
        end = st.jls_container.parse(jls).scans[0].data_end
        assert jls[end - len(s.segment):end] == s.segment and len(jls) == end + 2
        try:
            assert ob.encode(img, destination_size=end + key[2], **kw) == jls
            _verdicts[key] = 0
        except ob.OracleError as e:
            _verdicts[key] = e.errc
    v = _verdicts[key]
    return v if room >= 2 or v == TOO_SMALL else None


def check_encoded(launch, all_scans, room=64, oracle=False):
    """`room`: bytes of the destination beyond the segment.  `oracle`: the verdict is the oracle's for a destination of that
    size."""
    keep, outs, descs = [], [], []
    for s in all_scans:
        out, d = s.encode_desc(keep)
        d.stream_capacity = len(s.segment) + room
        outs.append(out)
        descs.append(d)
    res = launch(descs)
    for s, r, out in zip(all_scans, res, outs):
        what = (s.c.name, s.index, room, r.errc, r.flags, r.bytes, len(s.segment))
        assert not out[len(s.segment) + room:].any(), ("wrote behind the destination",) + what
        want = TOO_SMALL if room < 0 else 0 if room >= 8 else oracle_verdict(s, room) if oracle else None
        assert want is None or r.errc == want, what + ("the oracle:", want)
        assert r.errc in (0, TOO_SMALL), what
        if r.errc == 0:
            assert r.bytes == len(s.segment) and out[:r.bytes].tobytes() == s.segment, what
    return descs, res, keep


def serial(descs):
    res = (emu_bind.ScanResult * len(descs))()
    emu_bind.lib().emu_encode_scans_serial((emu_bind.ScanDesc * len(descs))(*descs), res, len(descs))
    return res


@pytest.mark.parametrize("name", st.route_frames("serial_encode", "emu", dense=True))
def test_serial_encoder_and_its_capacity(name):
    """scan_serial.hip's writer: the oracle's bytes."""
    for room in ROOMS:
        check_encoded(serial, scans(name), room, oracle=True)


FORMS = [("0", None), ("1", None), ("2", ("64", "0")), ("2", ("64", "64"))]   # stage E: stuff_scan, block form, speculative form


def set_form(monkeypatch, form, geometry):
    monkeypatch.setenv("CHARLS_AMD_BLOCK_STUFFING", form)
    if geometry:
        monkeypatch.setenv("CHARLS_AMD_SPEC_CHUNK", geometry[0])
        monkeypatch.setenv("CHARLS_AMD_SPEC_WARM", geometry[1])


def tile_cases():
    names = st.route_frames("tile_encode", "emu", dense=True)
    return [pytest.param(v, f, id=f"{st.batch_id(k)}-form{i}") for k, v in st.batches(names, "parameters").items() for i, f in enumerate(FORMS)]


def tile(descs):
    n = len(descs)
    res = (emu_bind.ScanResult * n)()
    emu_bind.tile_lib().emu_encode_tile_pipeline((emu_bind.ScanDesc * n)(*descs), res, n, 64, 32, 8, 8, 24)
    return res


@pytest.mark.parametrize("names,form", tile_cases())
def test_tile_pipeline_in_every_form_of_stage_e(monkeypatch, names, form):
    """The raw bit stream of a ramp is ones: stage E (stuff_scan, block_stuffing.hip, speculative_stuffing.hip with chunks of
    64 bytes, without and with warm-up) stuffs a bit into every second byte."""
    set_form(monkeypatch, *form)
    check_encoded(tile, [s for n in names for s in scans(n)], room=64)


@pytest.mark.parametrize("name,rooms", [("ramp_8", (-1, 0, 1, 2, 3, 4)), ("flat_1x600_zeros", (-1, 0, 4)), ("flat_2x597_255", (-1, 0, 4)),
                                        ("ramp_16_specks30", (-1, 0, 4))])
def test_tile_pipeline_capacity(monkeypatch, name, rooms):
    """One byte less than the segment is destination_too_small in every form of stage E and the exact length succeeds; up to
    three bytes more the forms give stuff_scan's verdict (errc, flags, bytes: the zone in which the host runs the exact kernel
    again, tests/test_emu_block_stuffing.py, test_capacity_verdicts_agree), and whoever reports success without that flag has
    written the oracle's bytes."""
    s, = scans(name)
    verdicts = {}
    for form, geometry in FORMS:
        set_form(monkeypatch, form, geometry)
        for room in rooms:
            keep = []
            out, d = s.encode_desc(keep)
            d.stream_capacity = len(s.segment) + room
            r, = tile([d])
            verdicts[form, geometry, room] = (r.errc, r.flags, r.bytes)
            assert not out[len(s.segment) + room:].any(), "wrote behind the destination"
            if room < 0:
                assert r.errc == TOO_SMALL, (form, geometry)
            else:
                assert r.errc == 0, (form, geometry, room)
            if room == 4:
                assert r.flags == 0, (form, geometry)
            if r.errc == 0 and r.flags == 0:
                assert out[:r.bytes].tobytes() == s.segment, (form, geometry, room)
            assert verdicts[form, geometry, room] == verdicts["0", None, room], (form, geometry, room)


def group_encode_cases():
    names = st.route_frames("group_encode", "emu", dense=True)
    return [pytest.param(i, v, id=st.batch_id(k)) for i, (k, v) in enumerate(st.batches(names, "parameters").items())]


@pytest.mark.parametrize("i,names", group_encode_cases())
def test_group_encoder_its_measuring_form_and_capacity(i, names):
    """The RingWriter of scan_group_encode.hip, and the measuring form, which has to count the stuffed bits: the measured size is
    the oracle's."""
    group = (8, 16, 64)[i % 3]
    all_scans = [s for n in names for s in scans(n)]
    L = emu_bind.lib()
    c = all_scans[0].c
    # (a launch of the harness costs seconds per thousand lines: every size on the small geometries, three on the others)
    for room in (ROOMS[1:] if c.width * c.height * c.comps <= 10000 else (-1, 3)) + ROOMS[:1]:
        descs, res, keep = check_encoded(lambda descs: _encode_group(L, descs, group), all_scans, room, oracle=True)
    n = len(descs)
    canaries = []
    for d in descs:
        canary = np.full(64, measure.CANARY, dtype=np.uint8)
        canaries.append(canary)
        d.stream, d.stream_capacity, d.line_scratch = canary.ctypes.data, 0, None
    measured = (emu_bind.ScanResult * n)()
    assert measure.measure_lib().emu_measure_pixels_group((emu_bind.ScanDesc * n)(*descs), measured, n, group) == 0
    assert [(m.errc, m.bytes) for m in measured] == [(0, len(s.segment)) for s in all_scans]
    assert all((c == measure.CANARY).all() for c in canaries)
