"""The salvage decode (charls_amd.h part 2g) on the GPU: damaged DRI streams built from the oracle's coding of every interval
(tests/salvage_model.py) must come back with the oracle's rows in the kept intervals and the fill value elsewhere, with the
status bytes and the report of the model; round 1 must be the ragged call exactly.  The frames are tiny: what is under test is
the planner, the judge and the fill, not the decoders.  GPU only."""
import ctypes as C

import numpy as np
import pytest

import oracle_bind as ob
import salvage_model as sm
import strided
from charls_amd import batch, capi, synth

pytestmark = pytest.mark.gpu

CANARY = 0xA5
INVALID_ARGUMENT, INVALID_ARGUMENT_SIZE = 101, 110

# name -> (width, height, bits, components, interleave mode, NEAR, restart interval)
FRAMES = {
    "gray8": (40, 80, 8, 1, 0, 0, 4),          # N = 20
    "ri1": (16, 150, 8, 1, 0, 0, 1),           # N = 150
    "gray16": (129, 70, 16, 1, 0, 0, 5),       # N = 14
    "rgb_planar": (64, 50, 8, 3, 0, 0, 8),     # three scans of N = 7
    "rgb_line": (64, 50, 8, 3, 1, 0, 8),
    "rgb_sample_near3": (64, 50, 8, 3, 2, 3, 8),
}
FILL = {"gray16": 0x1C7}  # (a 16-bit value whose bytes differ; 8-bit frames: 0x5B)

_built = {}


def built(name) -> sm.Built:
    if name not in _built:
        w, h, bits, comps, ilv, near, ri = FRAMES[name]
        planes = [synth.frame_numpy(w, h, seed=5 + c, bits=bits, kind="mixed") for c in range(comps)]
        img = planes[0] if comps == 1 else (np.stack(planes, axis=0) if ilv == 0 else np.stack(planes, axis=-1))
        _built[name] = sm.build(np.ascontiguousarray(img), ri, bits=bits, comps=comps, ilv=ilv, near=near)
    return _built[name]


def fill_of(name):
    return FILL.get(name, 0x5B)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def lib():
    L = capi.load_product()
    assert L.lib.charls_amd_device_status() == 0
    return L


def pack(torch, streams):
    sizes = np.array([len(s) for s in streams], dtype=np.uint64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    blob = np.frombuffer(b"".join(streams) + bytes(16), dtype=np.uint8).copy()
    return torch.from_numpy(blob).cuda(), offsets, sizes


def canary_out(torch, nbytes):
    return torch.full((nbytes,), CANARY, dtype=torch.uint8, device="cuda:0")


def oracle_raises(data):
    try:
        ob.decode(data)
    except ob.OracleError:
        return True
    return False


def check_preconditions(sound: sm.Built, damaged_bytes, exp: sm.Expected):
    """The oracle fails on the damaged stream as a whole, and on every claimed piece that is not the interval's own coding,
    wrapped as an image of its own."""
    assert oracle_raises(damaged_bytes)
    for c, j, piece in exp.claimed_damaged:
        rows = min(sound.interval, sound.height - j * sound.interval)
        assert oracle_raises(sm.wrapped(sound, piece, rows)), (c, j)


def salvage_one(torch, lib, name, damaged: sm.Built, fill=None, status_pitch=None):
    sound = built(name)
    fill = fill_of(name) if fill is None else fill
    data = damaged.assemble()
    exp = sm.expected(sound, damaged, fill)
    check_preconditions(sound, data, exp)
    blob, offsets, sizes = pack(torch, [data])
    out = canary_out(torch, len(sound.pixels))
    cells = exp.status.size
    got = batch.decode_batch_salvage(blob, offsets, sizes, [out], fill, status_pitch=cells if status_pitch is None else status_pitch, lib=lib)
    torch.cuda.synchronize()
    return exp, got, out.cpu().numpy().tobytes()


def check_one(exp, got, pixels):
    assert int(got.errcs[0]) != 0
    assert got.reports[0].astuple() == exp.report
    assert got.status[0, :exp.status.size].tolist() == exp.status.reshape(-1).tolist()
    assert (got.status[0, exp.status.size:] == 0xFF).all()
    bad = np.flatnonzero(np.frombuffer(pixels, dtype=np.uint8) != np.frombuffer(exp.pixels, dtype=np.uint8))
    assert bad.size == 0, f"{bad.size} wrong bytes, the first at {int(bad[0])}"


# name of the frame, what is done to it (a function of the sound stream)
DAMAGE = {
    "gray8-delete_marker_5": ("gray8", lambda b: sm.delete_marker(b, 5)),
    "gray8-renumber_marker_9": ("gray8", lambda b: sm.renumber_marker(b, 9, 4)),
    "gray8-spurious_d5_in_piece_2": ("gray8", lambda b: sm.insert_marker(b, 2, 5)),
    "gray8-spurious_expected_4_in_piece_4": ("gray8", lambda b: sm.insert_marker(b, 4, 4)),
    "gray8-zero_bytes_in_piece_3": ("gray8", lambda b: sm.zero_bytes(b, 3)),
    "gray8-zero_bytes_in_piece_11": ("gray8", lambda b: sm.zero_bytes(b, 11)),
    "gray8-cut_inside_piece_7": ("gray8", lambda b: sm.cut_inside(b, 7)),
    "gray8-cut_behind_marker_6": ("gray8", lambda b: sm.cut_behind_marker(b, 6)),
    "gray8-eight_markers_deleted": ("gray8", lambda b: sm.delete_markers(b, 3, 8)),
    "gray8-two_kinds_of_damage": ("gray8", lambda b: sm.zero_bytes(sm.delete_marker(b, 15), 2)),
    "ri1-delete_marker_63": ("ri1", lambda b: sm.delete_marker(b, 63)),
    "ri1-eight_markers_deleted_across_a_chunk": ("ri1", lambda b: sm.delete_markers(b, 60, 8)),
    "ri1-spurious_d1_in_piece_128": ("ri1", lambda b: sm.insert_marker(b, 128, 1)),
    "ri1-renumber_marker_64": ("ri1", lambda b: sm.renumber_marker(b, 64, 7)),
    "ri1-cut_inside_piece_100": ("ri1", lambda b: sm.cut_inside(b, 100)),
    "gray16-zero_bytes_in_piece_6": ("gray16", lambda b: sm.zero_bytes(b, 6)),
    "gray16-delete_marker_12": ("gray16", lambda b: sm.delete_marker(b, 12)),
    "gray16-renumber_marker_0": ("gray16", lambda b: sm.renumber_marker(b, 0, 3)),
    "rgb_line-delete_marker_2": ("rgb_line", lambda b: sm.delete_marker(b, 2)),
    "rgb_line-zero_bytes_in_piece_4": ("rgb_line", lambda b: sm.zero_bytes(b, 4)),
    "rgb_sample_near3-cut_inside_piece_3": ("rgb_sample_near3", lambda b: sm.cut_inside(b, 3)),
    "rgb_sample_near3-spurious_d0_in_piece_5": ("rgb_sample_near3", lambda b: sm.insert_marker(b, 5, 0)),
    "rgb_planar-delete_marker_3_of_plane_1": ("rgb_planar", lambda b: sm.delete_marker(b, 3, scan=1)),
    "rgb_planar-zero_bytes_in_planes_0_and_2": ("rgb_planar", lambda b: sm.zero_bytes(sm.zero_bytes(b, 1, scan=0), 5, scan=2)),
    "rgb_planar-sos_of_plane_1_destroyed": ("rgb_planar", lambda b: sm.destroy_sos(b, 1)),
    "rgb_planar-cut_inside_plane_1": ("rgb_planar", lambda b: sm.cut_inside(b, 2, scan=1)),
}


@pytest.mark.parametrize("case", list(DAMAGE))
def test_damaged_frames_keep_their_intact_intervals(torch, lib, case):
    name, damage = DAMAGE[case]
    exp, got, pixels = salvage_one(torch, lib, name, damage(built(name)))
    assert exp.report[2] > 0  # (something is lost in every case)
    check_one(exp, got, pixels)


def test_planar_frame_whose_second_sos_is_destroyed(torch, lib):
    """Plane 0 is salvaged whole; planes 1 and 2 are not reached: status 3, filled."""
    b = built("rgb_planar")
    exp, got, pixels = salvage_one(torch, lib, "rgb_planar", sm.destroy_sos(b, 1))
    N = b.intervals
    assert exp.status.tolist() == [[sm.KEPT] * N, [sm.NOT_REACHED] * N, [sm.NOT_REACHED] * N]
    assert exp.report == (1, 3 * N, 2 * N, 2 * b.height, 0, 0)
    check_one(exp, got, pixels)
    plane = b.height * b.row_bytes
    assert pixels[:plane] == b.pixels[:plane] and set(pixels[plane:]) == {0x5B}


def test_intact_batch_is_the_ragged_call_and_launches_nothing_new(torch, lib):
    names = list(FRAMES)
    streams = [built(n).assemble() for n in names]
    blob, offsets, sizes = pack(torch, streams)
    outs = [canary_out(torch, len(built(n).pixels)) for n in names]
    ragged_outs = [canary_out(torch, len(built(n).pixels)) for n in names]
    params, errcs, _ = batch.decode_batch_ragged(blob, offsets, sizes, ragged_outs, lib=lib)
    before = batch.salvage_counters(lib)
    got = batch.decode_batch_salvage(blob, offsets, sizes, outs, 0x5B, status_pitch=512, lib=lib)
    torch.cuda.synchronize()
    assert batch.salvage_counters(lib) == before
    assert (errcs == 0).all() and (got.errcs == 0).all()
    assert bytes(got.params) == bytes(params)
    for f, n in enumerate(names):
        assert got.reports[f].astuple() == (0, 0, 0, 0, sm.NONE, 0)
        assert outs[f].cpu().numpy().tobytes() == ragged_outs[f].cpu().numpy().tobytes() == built(n).pixels
    assert (got.status == 0xFF).all()


def test_mixed_batch_round_one_is_the_ragged_call(torch, lib):
    b = built("gray8")
    w, h = 40, 80
    plain_img = synth.frame_numpy(w, h, seed=9, bits=8, kind="mixed")
    plain = bytearray(ob.encode(plain_img, width=w, height=h))
    plain[len(plain) // 2:len(plain) // 2 + 4] = bytes(4)  # damaged, and no restart intervals to salvage
    assert oracle_raises(bytes(plain))
    broken_header = bytearray(b.assemble())
    broken_header[3] = 0xF6  # the SOF55 marker is gone
    damaged = sm.delete_marker(b, 5)
    streams = [b.assemble(), damaged.assemble(), bytes(plain), bytes(broken_header), b.assemble()]
    blob, offsets, sizes = pack(torch, streams)
    size = len(b.pixels)
    capacities = [size, size, size, size, size - 1]

    def run(call):
        outs = [canary_out(torch, size) for _ in streams]
        result = call(outs)
        torch.cuda.synchronize()
        return result, [o.cpu().numpy().tobytes() for o in outs]

    (params, errcs, _), ragged = run(lambda outs: batch.decode_batch_ragged(blob, offsets, sizes, outs, capacities=capacities, lib=lib))
    got, pixels = run(lambda outs: batch.decode_batch_salvage(blob, offsets, sizes, outs, 0x5B, capacities=capacities, status_pitch=20, lib=lib))
    assert got.errcs.tolist() == errcs.tolist() and bytes(got.params) == bytes(params)
    assert int(errcs[0]) == 0 and all(int(e) != 0 for e in errcs[1:]) and int(errcs[4]) == INVALID_ARGUMENT_SIZE
    assert [r.state for r in got.reports] == [0, 1, 2, 2, 2]
    assert pixels[0] == ragged[0] == b.pixels
    exp = sm.expected(b, damaged, 0x5B)
    assert pixels[1] == exp.pixels and got.reports[1].astuple() == exp.report
    assert got.status[1].tolist() == exp.status.reshape(-1).tolist()
    assert pixels[4] == bytes([CANARY]) * size  # nothing of a frame whose capacity is too small is written
    for f in (2, 3, 4):
        assert got.reports[f].astuple() == (2, 0, 0, 0, sm.NONE, 0) and (got.status[f] == 0xFF).all()


def test_fill_value_above_maxval(torch, lib):
    b = built("gray8")
    damaged = sm.delete_marker(b, 5)
    blob, offsets, sizes = pack(torch, [damaged.assemble(), b.assemble()])
    outs = [canary_out(torch, len(b.pixels)) for _ in range(2)]
    got = batch.decode_batch_salvage(blob, offsets, sizes, outs, 256, status_pitch=20, lib=lib)
    torch.cuda.synchronize()
    assert got.errcs.tolist() == [INVALID_ARGUMENT, 0]
    assert got.reports[0].astuple() == (2, 0, 0, 0, sm.NONE, 0) and got.reports[1].state == 0
    assert outs[1].cpu().numpy().tobytes() == b.pixels


def test_status_pitch_that_is_too_small(torch, lib):
    b = built("gray8")
    exp, got, pixels = salvage_one(torch, lib, "gray8", sm.delete_marker(b, 5), status_pitch=19)
    assert got.reports[0].astuple() == exp.report[:5] + (1,)
    assert (got.status == 0xFF).all()
    assert pixels == exp.pixels


@pytest.mark.parametrize("name,cls,base", [("gray8", "p13", 1), ("gray8", "r16p16", 8), ("rgb_planar", "p1", 1), ("gray16", "p2", 2)])
def test_padded_rows_in_a_canary_arena(torch, lib, name, cls, base):
    b = built(name)
    w, h, bits, comps, ilv, _, _ = FRAMES[name]
    g = strided.Geometry(w, h, bits, comps, ilv)
    lay = strided.layout(g, cls, base, 1, tight=True)
    damaged = sm.zero_bytes(sm.delete_marker(b, 4), 1)
    fill = fill_of(name)
    exp = sm.expected(b, damaged, fill)
    check_preconditions(b, damaged.assemble(), exp)
    blob, offsets, sizes = pack(torch, [damaged.assemble()])
    arena = torch.from_numpy(lay.blank().copy()).cuda()
    assert arena.data_ptr() % 16 == 0
    got = batch.decode_batch_salvage(blob, offsets, sizes, [arena[lay.first:]], fill, strides=[lay.stride], capacities=[lay.need],
                                     status_pitch=exp.status.size, lib=lib)
    torch.cuda.synchronize()
    assert got.reports[0].astuple() == exp.report
    lay.check(arena.cpu().numpy(), [exp.pixels], what="salvaged")


def test_part_one_call_equals_the_batch_call(torch, lib):
    for name, damaged in (("gray8", sm.zero_bytes(sm.delete_marker(built("gray8"), 5), 11)), ("rgb_planar", sm.destroy_sos(built("rgb_planar"), 1))):
        exp, got, pixels = salvage_one(torch, lib, name, damaged)
        data = damaged.assemble()
        with pytest.raises(capi.JpegLSError) as plain:
            lib.decode(data)
        _, out, report, status, rc = lib.decode_salvage(data, fill_of(name), status_capacity=exp.status.size)
        assert rc == plain.value.errc != 0
        assert report.astuple() == got.reports[0].astuple() == exp.report
        assert status.tolist() == got.status[0].tolist()
        assert out.tobytes() == pixels == exp.pixels
    # a sound stream: decode_to_buffer's result, state 0
    b = built("gray16")
    _, out, report, _, rc = lib.decode_salvage(b.assemble(), 0)
    assert rc == 0 and report.astuple() == (0, 0, 0, 0, sm.NONE, 0) and out.tobytes() == b.pixels


def test_work_areas_are_counted_and_released(torch, lib):
    batch.release_work_areas(lib)
    idle = batch.work_area_bytes(lib)
    launches = batch.salvage_counters(lib)[3]
    exp, got, pixels = salvage_one(torch, lib, "gray8", sm.delete_marker(built("gray8"), 5))
    check_one(exp, got, pixels)
    counters = batch.salvage_counters(lib)
    assert counters[3] == launches + 3  # one launch of each of the three kernels
    assert batch.work_area_bytes(lib) >= idle + 7 * 65536  # (the seven buffers of the salvage launch, 64 KiB at least each)
    batch.release_work_areas(lib)
    assert batch.work_area_bytes(lib) == idle


def test_counters_count_frames_and_intervals(torch, lib):
    before = batch.salvage_counters(lib)
    exp, got, pixels = salvage_one(torch, lib, "gray8", sm.delete_marker(built("gray8"), 5))
    after = batch.salvage_counters(lib)
    assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (1, 18, 2)
