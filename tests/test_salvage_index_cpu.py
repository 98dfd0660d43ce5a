"""The calls of charls_amd.h part 2h without a GPU: what the batch call refuses for the whole call is refused before a device
is asked for (invalid_argument here, where no device exists, not device_unavailable) and nothing is written; a call without
frames succeeds; both library names export the three entry points and the header declares them; and the model of
tests/salvage_index_model.py agrees with cases worked by hand."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import common
import oracle_bind as ob
import salvage_index_model as sim
from charls_amd import batch, capi, synth

INVALID_ARGUMENT = 101
LIB_DIR = os.path.join(common.ROOT, "charls_amd", "lib")
NAMES = ["charls_amd_decode_batch_device_salvage_indexed", "charls_amd_jpegls_decoder_decode_to_buffer_salvage_indexed",
         "charls_amd_salvage_index_counters"]
SOMEWHERE = 0x1000  # a non-NULL "device pointer": no call below gets as far as touching it

u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def l():
    return batch._bind(capi.load_product())


class Tables:
    """Valid host tables for a call over n frames."""

    def __init__(self, n):
        m = max(n, 1)
        self.offsets = np.full(n + 1, 77, dtype=np.uint64)
        self.sizes = np.full(m, 10, dtype=np.uint64)
        self.indexes = np.full((m, 16), 0xDD, dtype=np.uint8)
        self.index_sizes = np.full(m, 16, dtype=np.uint64)
        self.errcs = np.full(m, -1, dtype=np.int32)
        self.params = (batch.CodecParams * m)()
        self.reports = (capi.SalvageReport * m)()
        self.status = np.full((m, 8), 0xEE, dtype=np.uint8)
        self.dests = (batch.FrameDest * m)()
        for f in range(m):
            self.dests[f] = batch.FrameDest(SOMEWHERE, 128, 0, 0)
            self.reports[f] = capi.SalvageReport(9, 9, 9, 9, 9, 9)

    def args(self, n, flags=0):
        return [n, SOMEWHERE, self.offsets.ctypes.data_as(u64p), self.sizes.ctypes.data_as(u64p), self.indexes.ctypes.data, 16,
                self.index_sizes.ctypes.data_as(u64p), self.dests, 0, flags, self.params, self.reports, self.status.ctypes.data, 8,
                self.errcs.ctypes.data_as(i32p), None]

    def untouched(self):
        return (self.offsets == 77).all() and (self.errcs == -1).all() and (self.status == 0xEE).all() and \
            (self.index_sizes == 16).all() and all(r.astuple() == (9,) * 6 for r in self.reports)


def test_whole_call_errors_come_before_a_device_is_asked_for(l):
    fn = l.charls_amd_decode_batch_device_salvage_indexed
    t = Tables(2)
    for at in (2, 3, 6, 7, 11, 14):  # offsets, sizes, index_sizes, dests, reports, errcs
        args = t.args(2)
        args[at] = None
        assert fn(*args) == INVALID_ARGUMENT, at
    args = t.args(2)
    args[4] = None  # index sizes that are not 0 without indexes
    assert fn(*args) == INVALID_ARGUMENT
    for flags in (2, 3, 0x80000000, 0xFFFFFFFE):  # bits above bit 0
        assert fn(*t.args(2, flags)) == INVALID_ARGUMENT, flags
    args = t.args(2)
    args[13] = 0  # a status array without a pitch
    assert fn(*args) == INVALID_ARGUMENT
    args = t.args(2)
    args[1] = None  # no streams
    assert fn(*args) == INVALID_ARGUMENT
    for bad in (0, 1):
        t.dests[bad].reserved = 3
        assert fn(*t.args(2)) == INVALID_ARGUMENT
        t.dests[bad].reserved = 0
    t.dests[1] = batch.FrameDest(None, 16, 0, 0)
    assert fn(*t.args(2)) == INVALID_ARGUMENT
    assert t.untouched()


def test_no_frames(l):
    fn = l.charls_amd_decode_batch_device_salvage_indexed
    t = Tables(0)
    for flags in (0, 1):
        args = t.args(0, flags)
        args[1] = None
        assert fn(*args) == 0
        args[4] = None  # and without indexes
        args[12], args[13] = None, 0  # and without a status array
        assert fn(*args) == 0
    assert fn(*t.args(0, 2)) == INVALID_ARGUMENT  # (the flags are checked all the same)
    assert t.untouched()


def test_counters_respect_the_capacity(l):
    out = (C.c_uint64 * 8)(*([7] * 8))
    assert l.charls_amd_salvage_index_counters(out, 8) == 6 and list(out)[6:] == [7, 7]
    assert l.charls_amd_salvage_index_counters(out, 2) == 2 and l.charls_amd_salvage_index_counters(None, 6) == 0
    before = batch.salvage_index_counters()
    t = Tables(0)
    assert l.charls_amd_decode_batch_device_salvage_indexed(*t.args(0)) == 0
    assert batch.salvage_index_counters() == before


def test_part_one_call_checks_its_arguments():
    L = capi.load_product().lib
    fn = L.charls_amd_jpegls_decoder_decode_to_buffer_salvage_indexed
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(capi.SalvageReport), C.c_void_p,
                   C.c_size_t]
    fn.restype = C.c_int32
    report = capi.SalvageReport()
    out = np.zeros(64, dtype=np.uint8)
    assert fn(None, out.ctypes.data, 64, 0, 0, 0, C.byref(report), None, 0) == INVALID_ARGUMENT
    L.charls_jpegls_decoder_create.restype = C.c_void_p
    dec = L.charls_jpegls_decoder_create()
    try:
        assert fn(dec, out.ctypes.data, 64, 0, 0, 0, None, None, 0) == INVALID_ARGUMENT
        assert fn(dec, out.ctypes.data, 64, 0, 0, 2, C.byref(report), None, 0) == INVALID_ARGUMENT
        assert fn(dec, out.ctypes.data, 64, 0, 0, 0, C.byref(report), None, 5) == INVALID_ARGUMENT
        assert fn(dec, out.ctypes.data, 64, 0, 0, 1, C.byref(report), None, 0) == 100  # invalid_operation: no header was read
    finally:
        L.charls_jpegls_decoder_destroy.argtypes = [C.c_void_p]
        L.charls_jpegls_decoder_destroy(dec)


@pytest.mark.parametrize("library", ["libcharls_amd.so", "libcharls.so.3"])
def test_both_library_names_export_the_calls(library):
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB_DIR, library)], capture_output=True, text=True).stdout.split("\n")
    exported = {line.split()[-1] for line in names if line.strip()}
    assert set(NAMES) <= exported


def test_the_header_declares_the_calls():
    with open(os.path.join(common.ROOT, "include", "charls_amd.h")) as f:
        text = f.read()
    for name in NAMES:
        assert f" {name}(" in text, name
    assert "#define CHARLS_AMD_SALVAGE_PREFIX 1u" in text and "Part 2h" in text


# ---- the model on cases worked by hand ---------------------------------------------------------------------------------------

def fake_index(K, width, height, bits, comps, ilv, scans):
    """An index in the layout of host/seek_index.h.  scans: (segment length, reader positions of its seek points)."""
    planes = 1 if ilv == 0 else comps
    point = 2992 + ((planes * (width + 2) * (2 if bits > 8 else 1) + 7) & ~7) + 24
    out = bytearray(b"JLSSEEK\0" + struct.pack("<IIIIiiii", 1, K, width, height, bits, comps, ilv, 0))
    out += struct.pack("<iiiii", 3, 7, 21, 64, 0) + struct.pack("<III", len(scans), point, 0)
    assert len(out) == 72
    for length, positions in scans:
        out += struct.pack("<QQII", length, 0x1234, len(positions), 0)
    for _, positions in scans:
        for p in positions:
            out += bytes(point - 24) + struct.pack("<QQQ", p, 0xABCD, 17)
    return bytes(out), point


def fake_sound(K=4, height=10, width=5, scans=1, positions=(100, 180), segment=300):
    """A 'stream' of numbered bytes with `scans` segments of `segment` bytes behind headers of 14 bytes."""
    index, _ = fake_index(K, width, height, 8, scans, 0, [(segment, list(positions))] * scans)
    view = sim.read_index(index)
    jls = bytes((7 * k + 1) % 251 for k in range(20 + scans * (14 + segment) + 2))
    headers = [20 + c * (14 + segment) for c in range(scans)]
    starts = [h + 14 for h in headers]
    pixels = bytes((r + 1) & 0xFF for c in range(scans) for r in range(height) for _ in range(width))
    return sim.Sound(jls, index, view, pixels, starts, headers, width)


def test_model_reads_the_index_layout():
    index, point = fake_index(7, 70, 40, 12, 1, 0, [(999, [10, 20, 30, 40, 50])])
    v = sim.read_index(index)
    assert (v.lines, v.width, v.height, v.bits, v.components, v.ilv) == (7, 70, 40, 12, 1, 0)
    assert point == 2992 + 144 + 24 and v.point_bytes == point
    assert v.segments == [999] and v.positions == [[10, 20, 30, 40, 50]]
    index, point = fake_index(4, 35, 24, 8, 3, 2, [(500, [1, 2, 3, 4, 5])])
    assert point == 2992 + 112 + 24 and sim.read_index(index).positions == [[1, 2, 3, 4, 5]]


def test_model_spans_and_rows():
    s = fake_sound()
    assert s.intervals == 3 and [s.rows_of(i) for i in range(3)] == [4, 4, 2]
    assert [s.span(0, i) for i in range(3)] == [(34, 134), (134, 214), (214, 334)]


def test_model_damage_in_the_middle_interval():
    s = fake_sound()
    d = sim.zero4(s, 1)
    changed = [k for k in range(len(s.jls)) if d.data[k] != s.jls[k]]
    assert len(d.data) == len(s.jls) and changed and min(changed) >= 134 + 16 and max(changed) < 214 - 16
    assert d.raw.tolist() == [[0, 2, 0]]
    e = sim.expected_index(s, d.raw, 0x5B)
    assert e.status.tolist() == [[0, 2, 4]] and e.report == (1, 3, 1, 4, 4, 0)
    rows = [e.pixels[r * 5:(r + 1) * 5] for r in range(10)]
    assert rows == [bytes([r + 1]) * 5 for r in range(4)] + [b"\x5b" * 5] * 4 + [bytes([9]) * 5, bytes([10]) * 5]


def test_model_noise_keeps_the_margin_for_every_seed():
    s = fake_sound()
    for seed in range(50):
        d = sim.overwrite16(s, 0, seed)
        changed = [k for k in range(len(s.jls)) if d.data[k] != s.jls[k]]
        assert changed and min(changed) >= 34 + 16 and max(changed) < 134 - 16 and d.raw.tolist() == [[2, 0, 0]]
    with pytest.raises(AssertionError):
        sim.overwrite16(fake_sound(positions=(40, 180)), 0, 1)  # 40 bytes: no room for 16 with a margin of 16 on both sides


def test_model_two_damages_and_the_first_and_last_interval():
    s = fake_sound()
    d = sim.merge(s, sim.zero4(s, 0), sim.zero4(s, 2))
    assert d.raw.tolist() == [[2, 0, 2]]
    e = sim.expected_index(s, d.raw, 0)
    assert e.status.tolist() == [[2, 4, 2]] and e.report == (1, 3, 2, 6, 0, 0)
    assert e.pixels[:20] == bytes(20) and e.pixels[20:40] == s.pixels[20:40] and e.pixels[40:] == bytes(10)


def test_model_cut_and_destroyed_header_on_three_scans():
    s = fake_sound(scans=3)
    d = sim.cut(s, 1, scan=1)
    a, b = s.span(1, 1)
    assert d.data.endswith(b"\xff\xd9") and a + 16 <= len(d.data) - 2 <= b - 16 and d.data[:-2] == s.jls[:len(d.data) - 2]
    assert d.raw.tolist() == [[0, 0, 0], [0, 2, 3], [3, 3, 3]]
    e = sim.expected_index(s, d.raw, 0x5B)
    assert e.status.tolist() == [[0, 0, 0], [0, 2, 3], [3, 3, 3]] and e.report == (1, 9, 5, 4 + 2 + 10, 0, 0)
    d = sim.destroy_sos(s, 1)
    assert d.data[s.headers[1]:s.starts[1]] == b"\xff\xd9" + bytes(12) and d.data[:s.headers[1]] == s.jls[:s.headers[1]]
    assert d.raw.tolist() == [[0, 0, 0], [3, 3, 3], [3, 3, 3]]
    e = sim.expected_index(s, d.raw, 0x5B)
    assert e.report == (1, 9, 6, 20, 0, 0) and e.pixels[:50] == s.pixels[:50] and set(e.pixels[50:]) == {0x5B}


def test_model_sixteen_bit_fill_is_little_endian():
    index, _ = fake_index(2, 3, 4, 12, 1, 0, [(200, [100])])
    s = sim.Sound(bytes(300), index, sim.read_index(index), bytes(range(24)), [20], [6], 6)
    e = sim.expected_index(s, np.array([[2, 0]], dtype=np.uint8), 0x1C7)
    assert e.pixels == b"\xc7\x01" * 6 + bytes(range(12, 24)) and e.status.tolist() == [[2, 4]]


def test_model_prefix_is_what_the_oracle_leaves():
    """The figures of the header: 70 x 40, 8 bit, kind mixed, seed 7, four bytes zeroed in the middle."""
    w, h = 70, 40
    img = synth.frame_numpy(w, h, seed=7, bits=8, kind="mixed")
    jls = ob.encode(img, width=w, height=h)
    assert len(jls) == 1275
    sound_pixels = ob.decode(jls)[1].tobytes()
    index, _ = fake_index(4, w, h, 8, 1, 0, [(1, [0] * 9)])
    s = sim.Sound(jls, index, sim.read_index(index), sound_pixels, [0], [0], w)
    damaged = bytearray(jls)
    at = len(jls) // 2
    damaged[at:at + 4] = bytes(4)
    rows, left = sim.oracle_rows(s, bytes(damaged))
    assert rows == [38]
    right = next(r for r in range(h + 1) if r == h or left[r * w:(r + 1) * w] != sound_pixels[r * w:(r + 1) * w])
    assert right == 19
    e = sim.expected_prefix(s, bytes(damaged), 0x5B)
    assert e.status.tolist() == [sim.PREFIX] and e.report == (3, 1, 1, 2, 38, 0) and len(e.alternatives) == 1
    assert e.pixels[:38 * w] == left[:38 * w] and set(e.pixels[38 * w:]) == {0x5B}
    cut = jls[:at] + b"\xff\xd9"
    rows, left = sim.oracle_rows(s, cut)
    assert rows == [19] and left[:19 * w] == sound_pixels[:19 * w]
