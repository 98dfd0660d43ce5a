"""Salvage decode through the seek-point index (charls_amd.h part 2h) on the GPU.  Streams without restart markers are the
oracle's; their indexes are built by the existing decode_to_buffer_and_index while they are sound; the damage and what must
come back for it -- pixels, report, status bytes -- are tests/salvage_index_model.py's.  Every case asserts its
preconditions on the CPU (the oracle raises on the damaged stream, decodes the sound one, the damage keeps its margin from
the seek points) and skips none.  The frames are the smallest at which the kernels can go wrong: 70 x 40 (more than one
64-sample chunk, no multiple of 16) with K = 4 (ten intervals, the last on another path) and K = 7 (a short last interval),
35 x 24 for every components-per-pixel instantiation.  GPU only."""
import random

import numpy as np
import pytest

import oracle_bind as ob
import salvage_index_model as sim
import salvage_model as sm
import strided
from charls_amd import batch, capi, synth

pytestmark = pytest.mark.gpu

CANARY = 0xA5
INVALID_ARGUMENT = 101

# name -> (width, height, bits, components, interleave mode, NEAR)
FRAMES = {
    "gray8": (70, 40, 8, 1, 0, 0),
    "gray12": (70, 40, 12, 1, 0, 0),
    "gray8_near2": (70, 40, 8, 1, 0, 2),
    "rgb_planar": (35, 24, 8, 3, 0, 0),
    "rgb_line": (35, 24, 8, 3, 1, 0),
    "rgb_sample": (35, 24, 8, 3, 2, 0),
}
FILL = {"gray12": 0x1C7}  # (a 16-bit value whose bytes differ; 8-bit frames: 0x5B)


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


def image(name, seed=7):
    """The frame in the user's layout, with a run to the end of a line and one interrupted in a line's last samples."""
    w, h, bits, comps, ilv, _ = FRAMES[name]
    return strided.mixed(strided.Geometry(w, h, bits, comps, ilv), seed)


_sound = {}


def sound(lib, name, K, seed=7) -> sim.Sound:
    """The oracle's stream of the frame with the index part 1 builds for it while it is sound."""
    key = (name, K, seed)
    if key not in _sound:
        w, h, bits, comps, ilv, near = FRAMES[name]
        jls = ob.encode(image(name, seed), width=w, height=h, bits_per_sample=bits, component_count=comps, interleave_mode=ilv,
                        near_lossless=near)
        _, out, index = lib.decode_with_index(jls, lines_per_seek_point=K)
        s = sim.sound(jls, index)
        assert out.tobytes() == s.pixels and s.view.lines == K
        _sound[key] = s
    return _sound[key]


def pack(torch, streams):
    sizes = np.array([len(s) for s in streams], dtype=np.uint64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    blob = np.frombuffer(b"".join(streams) + bytes(16), dtype=np.uint8).copy()
    return torch.from_numpy(blob).cuda(), offsets, sizes


def oracle_raises(data):
    try:
        ob.decode(data)
    except ob.OracleError:
        return True
    return False


def run_in_arena(torch, lib, s: sim.Sound, name, data, index, fill, flags=0, cls="p13", base=1, status_pitch=None):
    """The frame into padded rows at an odd base of a canary arena (16-bit frames: an even one, the seek kernels' condition)."""
    w, h, bits, comps, ilv, _ = FRAMES[name]
    g = strided.Geometry(w, h, bits, comps, ilv)
    if bits > 8:
        cls, base = "p2", 2
    lay = strided.layout(g, cls, base, 1, tight=True)
    blob, offsets, sizes = pack(torch, [data])
    arena = torch.from_numpy(lay.blank().copy()).cuda()
    assert arena.data_ptr() % 16 == 0
    cells = s.scans * s.intervals if status_pitch is None else status_pitch
    got = batch.decode_batch_salvage_indexed(blob, offsets, sizes, [arena[lay.first:]], [index], fill, flags=flags, strides=[lay.stride],
                                             capacities=[lay.need], status_pitch=cells, lib=lib)
    torch.cuda.synchronize()
    return got, lay, arena.cpu().numpy()


def check_index_case(torch, lib, name, K, make):
    s = sound(lib, name, K)
    d = make(s)
    fill = fill_of(name)
    assert oracle_raises(d.data) and not oracle_raises(s.jls)
    exp = sim.expected_index(s, d.raw, fill)
    got, lay, arena = run_in_arena(torch, lib, s, name, d.data, s.index, fill)
    assert int(got.errcs[0]) != 0
    assert got.status[0].tolist() == exp.status.reshape(-1).tolist()
    assert got.reports[0].astuple() == exp.report
    lay.check(arena, [exp.pixels], what="salvaged through the index")
    return exp


# (frame, K, what is done to the sound stream)
CASES = {
    "gray8-K4-middle": ("gray8", 4, lambda s: sim.zero4(s, 5)),
    "gray8-K4-first": ("gray8", 4, lambda s: sim.zero4(s, 0)),
    "gray8-K4-last": ("gray8", 4, lambda s: sim.zero4(s, 9)),
    "gray8-K4-noise": ("gray8", 4, lambda s: sim.overwrite16(s, 3, 11)),
    "gray8-K4-two": ("gray8", 4, lambda s: sim.merge(s, sim.zero4(s, 2), sim.overwrite16(s, 7, 5))),
    "gray8-K4-cut": ("gray8", 4, lambda s: sim.cut(s, 4)),
    "gray8-K7-middle": ("gray8", 7, lambda s: sim.zero4(s, 2)),
    "gray8-K7-short-last": ("gray8", 7, lambda s: sim.zero4(s, 5)),
    "gray8-K7-cut": ("gray8", 7, lambda s: sim.cut(s, 3)),
    "gray12-K4-middle": ("gray12", 4, lambda s: sim.zero4(s, 5)),
    "gray12-K4-last": ("gray12", 4, lambda s: sim.overwrite16(s, 9, 3)),
    "gray12-K7-cut": ("gray12", 7, lambda s: sim.cut(s, 2)),
    "near2-K4-middle": ("gray8_near2", 4, lambda s: sim.zero4(s, 4)),
    "rgb_line-K4-middle": ("rgb_line", 4, lambda s: sim.zero4(s, 2)),
    "rgb_line-K4-last": ("rgb_line", 4, lambda s: sim.overwrite16(s, 5, 2)),
    "rgb_sample-K4-first": ("rgb_sample", 4, lambda s: sim.zero4(s, 0)),
    "rgb_sample-K4-cut": ("rgb_sample", 4, lambda s: sim.cut(s, 3)),
    "rgb_planar-K4-scan1": ("rgb_planar", 4, lambda s: sim.zero4(s, 2, scan=1)),
    "rgb_planar-K4-scans-0-and-2": ("rgb_planar", 4, lambda s: sim.merge(s, sim.zero4(s, 1, scan=0), sim.overwrite16(s, 4, 9, scan=2))),
    "rgb_planar-K4-cut-in-scan1": ("rgb_planar", 4, lambda s: sim.cut(s, 3, scan=1)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_damaged_intervals_are_lost_and_the_others_kept(torch, lib, case):
    name, K, make = CASES[case]
    exp = check_index_case(torch, lib, name, K, make)
    assert exp.report[2] > 0 and exp.report[2] < exp.report[1]


def test_planar_damage_in_scan_0_leaves_the_later_scans_whole(torch, lib):
    """Part 2g loses the scans behind a damaged one; the index names where they start."""
    exp = check_index_case(torch, lib, "rgb_planar", 4, lambda s: sim.zero4(s, 3, scan=0))
    N = 6
    assert exp.status.tolist() == [[0, 0, 0, 2, 4, 4], [0] * N, [0] * N]
    assert exp.report == (1, 3 * N, 1, 4, 12, 0)


def test_planar_frame_whose_second_sos_is_destroyed(torch, lib):
    exp = check_index_case(torch, lib, "rgb_planar", 4, lambda s: sim.destroy_sos(s, 1))
    N = 6
    assert exp.status.tolist() == [[0] * N, [3] * N, [3] * N]
    assert exp.report == (1, 3 * N, 2 * N, 48, 0, 0)


def test_prefix_mode_keeps_what_the_reference_leaves(torch, lib):
    for name, make in (("gray8", lambda s: sim.zero4(s, 5)), ("gray8", lambda s: sim.cut(s, 4)), ("gray12", lambda s: sim.zero4(s, 4)),
                       ("rgb_line", lambda s: sim.overwrite16(s, 2, 1)), ("rgb_sample", lambda s: sim.cut(s, 3)),
                       ("rgb_planar", lambda s: sim.zero4(s, 2, scan=1))):
        s = sound(lib, name, 4)
        d = make(s)
        fill = fill_of(name)
        exp = sim.expected_prefix(s, d.data, fill)
        got, lay, arena = run_in_arena(torch, lib, s, name, d.data, None, fill, flags=batch.SALVAGE_PREFIX, status_pitch=s.scans)
        assert len(exp.alternatives) == 1 and sim.prefix_matches(exp, got.status[0], got.reports[0].astuple()), name
        lay.check(arena, [exp.pixels], what="prefix")
        # without the flag: nothing is salvaged
        got, _, _ = run_in_arena(torch, lib, s, name, d.data, None, fill, status_pitch=s.scans)
        assert got.reports[0].astuple() == (2, 0, 0, 0, sim.NONE, 0) and (got.status == 0xFF).all()


def test_prefix_rows_equal_the_oracles_on_a_seeded_sweep(torch, lib):
    """240 damaged streams over every form and every operator in ONE call: the rows kept in front of the first error are
    the rows the oracle writes before it raises, on every one."""
    rng = random.Random(2024)
    names = list(FRAMES)
    streams, wants, sounds = [], [], []
    for k in range(240):
        name = names[k % len(names)]
        s = sound(lib, name, 4)
        op = k // len(names) % 3
        places = [(c, i) for c in range(s.scans) for i in range(s.intervals) if sim.has_room(s, c, i, (4, 16, 0)[op])]
        scan, j = places[rng.randrange(len(places))]
        d = sim.zero4(s, j, scan) if op == 0 else (sim.overwrite16(s, j, k, scan) if op == 1 else sim.cut(s, j, scan))
        if not oracle_raises(d.data):
            continue  # (damage the reference cannot see either: nothing to compare)
        streams.append(d.data)
        sounds.append((name, s))
        wants.append(sim.expected_prefix(s, d.data, 0x5B))
    assert len(streams) >= 200
    blob, offsets, sizes = pack(torch, streams)
    outs = [torch.full((len(s.pixels),), CANARY, dtype=torch.uint8, device="cuda:0") for _, s in sounds]
    got = batch.decode_batch_salvage_indexed(blob, offsets, sizes, outs, None, 0x5B, flags=batch.SALVAGE_PREFIX, status_pitch=3, lib=lib)
    torch.cuda.synchronize()
    wrong = []
    for f, ((name, s), exp) in enumerate(zip(sounds, wants)):
        if not sim.prefix_matches(exp, got.status[f, :s.scans], got.reports[f].astuple()) or outs[f].cpu().numpy().tobytes() != exp.pixels:
            wrong.append((f, name, got.reports[f].astuple(), exp.report))
    assert not wrong, wrong[:5]


def test_mixed_batch(torch, lib):
    """A sound frame, a DRI frame as in part 2g, an indexed frame, a frame without index -- with and without the prefix
    flag --, a broken header: states [0, 1, 1, 3 | 2, 2]; round 1's results are the ragged call's."""
    s = sound(lib, "gray8", 4)
    d = sim.zero4(s, 5)
    w, h = 70, 40
    dri_sound = sm.build(synth.frame_numpy(w, h, seed=5, bits=8, kind="mixed"), 4, bits=8, comps=1, ilv=0, near=0)
    dri = sm.delete_marker(dri_sound, 5)
    broken = bytearray(s.jls)
    broken[3] = 0xF6  # the SOF55 marker is gone
    streams = [s.jls, dri.assemble(), d.data, d.data, bytes(broken)]
    indexes = [s.index, None, s.index, None, s.index]
    blob, offsets, sizes = pack(torch, streams)
    size = w * h

    def run(call):
        outs = [torch.full((size,), CANARY, dtype=torch.uint8, device="cuda:0") for _ in streams]
        result = call(outs)
        torch.cuda.synchronize()
        return result, [o.cpu().numpy().tobytes() for o in outs]

    (params, errcs, _), ragged = run(lambda outs: batch.decode_batch_ragged(blob, offsets, sizes, outs, lib=lib))
    exp_dri = sm.expected(dri_sound, dri, 0x5B)
    exp_index = sim.expected_index(s, d.raw, 0x5B)
    exp_prefix = sim.expected_prefix(s, d.data, 0x5B)
    for flags, states in ((batch.SALVAGE_PREFIX, [0, 1, 1, 3, 2]), (0, [0, 1, 1, 2, 2])):
        got, pixels = run(lambda outs: batch.decode_batch_salvage_indexed(blob, offsets, sizes, outs, indexes, 0x5B, flags=flags,
                                                                          status_pitch=10, lib=lib))
        assert got.errcs.tolist() == errcs.tolist() and bytes(got.params) == bytes(params)
        assert int(errcs[0]) == 0 and all(int(e) != 0 for e in errcs[1:])
        assert [r.state for r in got.reports] == states
        assert pixels[0] == ragged[0] == s.pixels
        assert pixels[1] == exp_dri.pixels and got.reports[1].astuple() == exp_dri.report
        assert got.status[1].tolist() == exp_dri.status.reshape(-1).tolist()
        assert pixels[2] == exp_index.pixels and got.reports[2].astuple() == exp_index.report
        assert got.status[2].tolist() == exp_index.status.reshape(-1).tolist()
        if flags:
            assert pixels[3] == exp_prefix.pixels and sim.prefix_matches(exp_prefix, got.status[3, :1], got.reports[3].astuple())
        else:
            assert got.reports[3].astuple() == (2, 0, 0, 0, sim.NONE, 0) and (got.status[3] == 0xFF).all()
        assert got.reports[4].astuple() == (2, 0, 0, 0, sim.NONE, 0) and (got.status[4] == 0xFF).all()


def test_intact_batch_launches_nothing_new(torch, lib):
    s = sound(lib, "gray8", 4)
    blob, offsets, sizes = pack(torch, [s.jls, s.jls])
    outs = [torch.full((len(s.pixels),), CANARY, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    before = batch.salvage_index_counters(lib), batch.salvage_counters(lib)
    got = batch.decode_batch_salvage_indexed(blob, offsets, sizes, outs, [s.index, None], 0x5B, flags=batch.SALVAGE_PREFIX, status_pitch=10,
                                             lib=lib)
    torch.cuda.synchronize()
    assert (batch.salvage_index_counters(lib), batch.salvage_counters(lib)) == before
    assert (got.errcs == 0).all() and all(r.astuple() == (0, 0, 0, 0, sim.NONE, 0) for r in got.reports)
    assert all(o.cpu().numpy().tobytes() == s.pixels for o in outs) and (got.status == 0xFF).all()


def test_index_of_another_stream_keeps_nothing_wrong(torch, lib):
    """The index of another stream of the same geometry: the first interval starts from the true initial state and cannot
    end in the foreign point's state; the others start from foreign states.  Whatever is kept must be the sound rows --
    intervals that decode identically from either state (the model cannot name them: none are expected on these frames)."""
    s = sound(lib, "gray8", 4)
    other = sound(lib, "gray8", 4, seed=23)
    assert other.jls != s.jls and len(other.index) == len(s.index)
    d = sim.zero4(s, 5)
    got, lay, arena = run_in_arena(torch, lib, s, "gray8", d.data, other.index, 0x5B)
    status = got.status[0].tolist()
    assert got.reports[0].state == 1 and status[0] == sim.LOST and sim.KEPT not in status
    raw = np.array([[sim.KEPT if v == sim.ON_INDEX else v for v in status]], dtype=np.uint8)
    raw[raw == sim.NOT_REACHED] = sim.LOST
    exp = sim.expected_index(s, raw, 0x5B)  # kept intervals hold the sound rows, all others the fill
    lay.check(arena, [exp.pixels], what="foreign index")
    assert status.count(sim.ON_INDEX) == 0


def test_truncated_index_counts_as_absent(torch, lib):
    s = sound(lib, "gray8", 4)
    d = sim.zero4(s, 5)
    got, _, arena = run_in_arena(torch, lib, s, "gray8", d.data, s.index[:-5], 0x5B)
    assert got.reports[0].astuple() == (2, 0, 0, 0, sim.NONE, 2) and (got.status == 0xFF).all()
    exp = sim.expected_prefix(s, d.data, 0x5B)
    got, lay, arena = run_in_arena(torch, lib, s, "gray8", d.data, s.index[:-5], 0x5B, flags=batch.SALVAGE_PREFIX, status_pitch=1)
    assert sim.prefix_matches(exp, got.status[0], got.reports[0].astuple(), reserved=2)
    lay.check(arena, [exp.pixels], what="prefix behind a refused index")


def test_fill_value_above_maxval(torch, lib):
    s = sound(lib, "gray8", 4)
    d = sim.zero4(s, 5)
    got, lay, arena = run_in_arena(torch, lib, s, "gray8", d.data, s.index, 256)
    assert got.errcs.tolist() == [INVALID_ARGUMENT] and got.reports[0].astuple() == (2, 0, 0, 0, sim.NONE, 0)


def test_status_pitch_that_is_too_small(torch, lib):
    s = sound(lib, "gray8", 4)
    d = sim.zero4(s, 5)
    exp = sim.expected_index(s, d.raw, 0x5B)
    got, lay, arena = run_in_arena(torch, lib, s, "gray8", d.data, s.index, 0x5B, status_pitch=9)
    assert got.reports[0].astuple() == exp.report[:5] + (1,) and (got.status == 0xFF).all()
    lay.check(arena, [exp.pixels], what="salvaged")


def test_counters_launches_and_work_areas(torch, lib):
    """Two groups (two geometries) of indexed frames: one resume launch and one fill launch per group; the work areas are
    the thread's, counted and released."""
    a, b = sound(lib, "gray8", 4), sound(lib, "rgb_line", 4)
    da, db = sim.zero4(a, 5), sim.zero4(b, 2)
    streams = [da.data, db.data, da.data, db.data]
    indexes = [a.index, b.index, a.index, b.index]
    blob, offsets, sizes = pack(torch, streams)
    outs = [torch.full((len(x.pixels),), CANARY, dtype=torch.uint8, device="cuda:0") for x in (a, b, a, b)]
    batch.release_work_areas(lib)
    idle = batch.work_area_bytes(lib)
    before = batch.salvage_index_counters(lib)
    got = batch.decode_batch_salvage_indexed(blob, offsets, sizes, outs, indexes, 0x5B, status_pitch=10, lib=lib)
    torch.cuda.synchronize()
    after = batch.salvage_index_counters(lib)
    delta = tuple(y - x for x, y in zip(before, after))
    # gray8: 10 intervals, 5 proven, 1 lost, 4 on the index; rgb_line: 6 intervals, 2 proven, 1 lost, 3 on the index
    assert delta == (4, 2 * (5 + 2), 2 * (4 + 3), 2 * 2, 0, 4)
    assert [r.state for r in got.reports] == [1, 1, 1, 1]
    assert batch.work_area_bytes(lib) >= idle + 5 * 65536
    batch.release_work_areas(lib)
    assert batch.work_area_bytes(lib) == idle


def test_part_one_call_equals_the_batch_call(torch, lib):
    for name, make, flags, use_index in (("gray8", lambda s: sim.zero4(s, 5), 0, True), ("rgb_planar", lambda s: sim.zero4(s, 3, scan=0), 0, True),
                                         ("gray12", lambda s: sim.cut(s, 4), batch.SALVAGE_PREFIX, False)):
        s = sound(lib, name, 4)
        d = make(s)
        fill = fill_of(name)
        exp = sim.expected_index(s, d.raw, fill) if use_index else sim.expected_prefix(s, d.data, fill)
        with pytest.raises(capi.JpegLSError) as plain:
            lib.decode(d.data)
        cells = exp.status.size
        _, out, report, status, rc = lib.decode_salvage_indexed(d.data, s.index if use_index else None, fill, flags, status_capacity=cells)
        assert rc == plain.value.errc != 0
        if use_index:
            assert report.astuple() == exp.report and status.tolist() == exp.status.reshape(-1).tolist()
        else:
            assert sim.prefix_matches(exp, status, report.astuple())
        assert out.tobytes() == exp.pixels
    # a sound stream: decode_to_buffer's result, state 0
    s = sound(lib, "gray12", 4)
    _, out, report, _, rc = lib.decode_salvage_indexed(s.jls, s.index, 0)
    assert rc == 0 and report.astuple() == (0, 0, 0, 0, sim.NONE, 0) and out.tobytes() == s.pixels
