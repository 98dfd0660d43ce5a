"""The seek-point index on packed streams (charls_amd.h part 2l): charls_amd_index_batch_device_packed with and without
destinations, charls_amd_decode_batch_device_ragged_indexed, charls_amd_decode_rows_batch_device_ragged and
charls_amd_index_batch_host.

The corpus is the 24 parameter sets of test_gpu_batch_index.py, packed at alignment 1 so that streams abut at odd offsets.
Streams come from the oracle's encoder, pixels are compared with the oracle's decoder byte for byte, indexes with the bytes
part 1 builds for the same stream:
  * the index-only build gives, per K, part 1's index bytes inside every frame's slot, with no scratch frame taken: it runs
    under a workspace limit of one byte, under which a frame that needed a scratch frame would get not_enough_memory;
  * frames without seek points (restart intervals) and damaged frames ride along: part 1's index without points, the errcs of
    charls_amd_decode_batch_device_packed, and the 24 unchanged -- with the scratch frames one window or one frame at a time;
  * with destinations -- padded strides at bases off a 16-byte boundary in a canary arena -- the pixels are the ragged
    decoder's; a 16-bit frame at an odd base gets its pixels and an index without points; a stride or capacity that is too
    small fails that frame alone;
  * the ragged indexed decode goes through the seek points without a fallback; a tampered index costs that frame one;
  * ragged bands at the top, across a seek point and at the last row, with indexes, without, and mixed;
  * 16 equal frames are one launch of the seek kernels in each of the three device calls;
  * an index built here drives the salvage decode of part 2h to the report an index of part 2c gives, and decodes on part 1;
  * the host form, from pageable and from pinned memory, over several windows, gives the device call's bytes and errcs;
  * the scratch frames are a work area.
GPU only."""
import numpy as np
import pytest

import oracle_bind as ob
import salvage_index_model as sim
import strided
from charls_amd import batch, capi, synth
from test_gpu_batch_index import BAND_SETS, _band_of, _gray, _part1_index, _slots, mixed  # noqa: F401 (mixed: a fixture)
from test_gpu_budget import dri_stream
from test_gpu_seek_index import _band, _stream, _tamper

pytestmark = pytest.mark.gpu

SUCCESS, INVALID_ARGUMENT, INVALID_ARGUMENT_SIZE, INVALID_ARGUMENT_STRIDE, NOT_ENOUGH_MEMORY = 0, 101, 110, 111, 1
CANARY = 0xC3
HEAD, SCAN_RECORD = 72, 24  # an index: its header, one record per scan, then the points


@pytest.fixture(scope="module")
def lib():
    L = capi.load_product()
    assert L.lib.charls_amd_device_status() == 0
    return L


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def pack(torch, streams):
    """Streams back to back (alignment 1): (device blob with 16 readable bytes behind the last stream, offsets, sizes)."""
    sizes = np.array([len(s) for s in streams], dtype=np.uint64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)[:len(streams)]
    blob = np.frombuffer(b"".join(streams) + bytes(16), dtype=np.uint8).copy()
    return torch.from_numpy(blob).cuda(), offsets, sizes


def bound(p, K, lib):
    return batch.index_size_bound(p["width"], p["height"], p["bits"], p["comps"], p["ilv"], p["near"], K, lib=lib)


def geometry(p):
    return strided.Geometry(p["width"], p["height"], p["bits"], p["comps"], p["ilv"])


def scans_of(p):
    return p["comps"] if p["ilv"] == 0 else 1


def build_index_only(lib, blob, offsets, sizes, K, pitch):
    """The index-only build into a canary-filled table: (params, errcs, indexes) with the canaries behind every index checked."""
    table = np.full((len(sizes), pitch), CANARY, dtype=np.uint8)
    params, errcs, built = batch.index_batch_packed(blob, offsets, sizes, K, index_pitch=pitch, indexes_out=table, lib=lib)
    for f, ix in enumerate(built):
        assert (table[f, len(ix):] == CANARY).all(), f
    return params, errcs, built


class Arena:
    """One canary-filled device buffer with a destination per frame in it: padded rows, a base off a 16-byte boundary, the
    smallest legal capacity (strided.Layout per frame, each sub-arena starting 16-byte aligned)."""

    def __init__(self, torch, geometries, bases=None):
        self.layouts, self.at = [], []
        size = 0
        for f, g in enumerate(geometries):
            wide = g.bits > 8
            base = bases[f] if bases is not None else (2 if wide else 1)  # (16-bit rows at even addresses: the seek kernels' condition)
            lay = strided.layout(g, "p2" if wide else "p13", base, 1, tight=True)
            self.layouts.append(lay)
            self.at.append(size)
            size += (lay.size + 15) & ~15
        self.device = torch.full((size,), strided.CANARY, dtype=torch.uint8, device="cuda")
        assert self.device.data_ptr() % 16 == 0
        self.outs = [self.device[at + lay.first:] for at, lay in zip(self.at, self.layouts)]
        self.strides = [lay.stride for lay in self.layouts]
        self.capacities = [lay.need for lay in self.layouts]

    def check(self, wants):
        """wants[f]: the frame's packed bytes, or None for a frame of which nothing may have been written."""
        host = self.device.cpu().numpy()
        for f, (at, lay) in enumerate(zip(self.at, self.layouts)):
            part = host[at:at + lay.size]
            if wants[f] is None:
                assert (part == strided.CANARY).all(), f
            else:
                lay.check(part, [wants[f]], what=f"frame {f}")


# ---- index-only build ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 4, 16])
def test_index_only_build_gives_part_1s_indexes_without_a_frame(torch, lib, mixed, K):
    ps, streams, _ = mixed
    blob, offsets, sizes = pack(torch, streams)
    assert any(int(o) & 1 for o in offsets)
    bounds = [bound(p, K, lib) for p in ps]
    before = capi.index_counters(lib)
    batch.release_work_areas(lib)
    batch.set_workspace_limit(1, lib)  # (no scratch frame can be had: a frame on the ordinary path would get not_enough_memory)
    try:
        params, errcs, built = build_index_only(lib, blob, offsets, sizes, K, max(bounds) + 40)
    finally:
        batch.set_workspace_limit(0, lib)
    assert errcs.tolist() == [SUCCESS] * len(ps)
    for f, p in enumerate(ps):
        want = _part1_index(lib, streams[f], K)
        assert len(built[f]) == len(want) <= bounds[f], f
        assert built[f] == want, (f, p)
        if p["height"] > K:
            assert len(built[f]) > HEAD + SCAN_RECORD * scans_of(p), f  # (seek points, not the index without them)
        assert (params[f].frame_info.width, params[f].frame_info.height, params[f].interleave_mode) == (p["width"], p["height"], p["ilv"]), f
    assert capi.index_counters(lib)["fallback_scans"] == before["fallback_scans"]


def odd_frames(lib, mixed):
    """Three more frames: restart intervals; a truncated stream; four bytes zeroed in the middle of a scan."""
    ps, streams, _ = mixed
    w, h = 40, 24
    img = synth.frame_numpy(w, h, seed=901, bits=8)
    dri = dri_stream(img, w, h, dict(bits_per_sample=8), 8)
    assert ob.decode(dri)[1].tobytes() == img.tobytes()
    noise = _stream(dict(width=64, height=40, bits=8, comps=1, ilv=0, near=0, kind="noise", seed=902))
    cut = noise[:len(noise) * 2 // 3]
    zeroed = bytearray(noise)
    zeroed[len(noise) // 2:len(noise) // 2 + 4] = bytes(4)
    return [dri, cut, bytes(zeroed)], (w, h)


@pytest.mark.parametrize("window", [0, 1])
def test_frames_without_seek_points_ride_along(torch, lib, knobs, mixed, window):
    ps, streams, _ = mixed
    K = 4
    extra, (w, h) = odd_frames(lib, mixed)
    everything = streams + extra
    n = len(ps)
    blob, offsets, sizes = pack(torch, everything)
    pitch = max([bound(p, K, lib) for p in ps] + [batch.index_size_bound(64, 40, lines_per_seek_point=K, lib=lib)]) + 40
    out = torch.zeros((len(everything), 1 << 17), dtype=torch.uint8, device="cuda")
    _, plain, _ = batch.decode_batch_packed(blob, offsets, sizes, out, lib=lib)
    assert plain[:n + 1].tolist() == [SUCCESS] * (n + 1) and plain[n + 1] != SUCCESS and plain[n + 2] != SUCCESS
    if window:
        knobs.set("INDEX_WINDOW_FRAMES", window)
    batch.release_work_areas(lib)
    held = batch.work_area_bytes(lib)
    params, errcs, built = build_index_only(lib, blob, offsets, sizes, K, pitch)
    assert errcs.tolist() == plain.tolist()
    for f in range(n):
        assert built[f] == _part1_index(lib, streams[f], K), f
    assert built[n] == lib.decode_with_index(extra[0], lines_per_seek_point=K)[2]
    assert len(built[n]) == HEAD + SCAN_RECORD  # (no seek points)
    assert (params[n].frame_info.width, params[n].frame_info.height, params[n].restart_interval) == (w, h, 8)
    assert built[n + 1] == b"" and built[n + 2] == b""
    # the scratch frame is a work area: counted, and freed
    assert batch.work_area_bytes(lib) >= held + w * h
    batch.release_work_areas(lib)
    assert batch.work_area_bytes(lib) <= held
    # without room for one scratch frame the frame that needs one says so, and the others are what they were
    batch.set_workspace_limit(1, lib)
    try:
        _, errcs, again = build_index_only(lib, blob, offsets, sizes, K, pitch)
    finally:
        batch.set_workspace_limit(0, lib)
    assert errcs[:n].tolist() == [SUCCESS] * n and errcs[n] == NOT_ENOUGH_MEMORY
    assert again[:n] == built[:n] and again[n] == b""


# ---- build with destinations ---------------------------------------------------------------------------------------------

def test_build_with_destinations(torch, lib, mixed):
    ps, streams, wants = mixed
    K = 4
    blob, offsets, sizes = pack(torch, streams)
    gs = [geometry(p) for p in ps]
    pitch = max(bound(p, K, lib) for p in ps) + 40
    plain = Arena(torch, gs)
    _, errcs, _ = batch.decode_batch_ragged(blob, offsets, sizes, plain.outs, strides=plain.strides, capacities=plain.capacities, lib=lib)
    assert errcs.tolist() == [SUCCESS] * len(ps)
    arena = Arena(torch, gs)
    table = np.full((len(ps), pitch), CANARY, dtype=np.uint8)
    before = capi.index_counters(lib)
    params, errcs, built = batch.index_batch_packed(blob, offsets, sizes, K, outs=arena.outs, strides=arena.strides, capacities=arena.capacities,
                                                    index_pitch=pitch, indexes_out=table, lib=lib)
    torch.cuda.synchronize()
    assert errcs.tolist() == [SUCCESS] * len(ps)
    arena.check(wants)
    assert bytes(arena.device.cpu().numpy()) == bytes(plain.device.cpu().numpy())
    for f, p in enumerate(ps):
        assert built[f] == _part1_index(lib, streams[f], K), f
        assert (table[f, len(built[f]):] == CANARY).all(), f
        assert (params[f].frame_info.width, params[f].frame_info.height) == (p["width"], p["height"]), f
    assert capi.index_counters(lib)["fallback_scans"] == before["fallback_scans"]


def test_a_sixteen_bit_frame_at_an_odd_base(torch, lib):
    ps = [dict(width=33, height=20, bits=16, comps=1, ilv=0, near=0, kind="noise", seed=910 + i) for i in range(3)]
    streams = [_stream(p) for p in ps]
    wants = [ob.decode(s)[1].tobytes() for s in streams]
    K = 4
    blob, offsets, sizes = pack(torch, streams)
    arena = Arena(torch, [geometry(p) for p in ps], bases=[2, 1, 8])
    _, errcs, built = batch.index_batch_packed(blob, offsets, sizes, K, outs=arena.outs, strides=arena.strides, capacities=arena.capacities,
                                               index_pitch=bound(ps[0], K, lib), lib=lib)
    torch.cuda.synchronize()
    assert errcs.tolist() == [SUCCESS] * 3
    arena.check(wants)
    assert built[0] == _part1_index(lib, streams[0], K) and built[2] == _part1_index(lib, streams[2], K)
    assert len(built[1]) == HEAD + SCAN_RECORD  # an index without seek points ...
    assert lib.decode(streams[1], index=built[1])[1].tobytes() == wants[1]  # ... that part 1 accepts
    # without a destination no frame is at an odd address
    _, errcs, only = build_index_only(lib, blob, offsets, sizes, K, bound(ps[0], K, lib))
    assert errcs.tolist() == [SUCCESS] * 3
    assert only == [_part1_index(lib, s, K) for s in streams]


def test_a_stride_or_capacity_too_small_fails_that_frame_alone(torch, lib, mixed):
    ps, streams, wants = mixed
    K = 4
    blob, offsets, sizes = pack(torch, streams)
    gs = [geometry(p) for p in ps]
    wide = [f for f, g in enumerate(gs) if g.row > 2]
    short, small = wide[0], wide[1]
    arena = Arena(torch, gs)
    strides, capacities = list(arena.strides), list(arena.capacities)
    strides[short] = gs[short].row - 1
    capacities[small] -= 1
    _, errcs, built = batch.index_batch_packed(blob, offsets, sizes, K, outs=arena.outs, strides=strides, capacities=capacities,
                                               index_pitch=max(bound(p, K, lib) for p in ps), lib=lib)
    torch.cuda.synchronize()
    want_errcs = [SUCCESS] * len(ps)
    want_errcs[short], want_errcs[small] = INVALID_ARGUMENT_STRIDE, INVALID_ARGUMENT_SIZE
    assert errcs.tolist() == want_errcs
    arena.check([None if f in (short, small) else w for f, w in enumerate(wants)])
    for f in range(len(ps)):
        assert built[f] == (b"" if f in (short, small) else _part1_index(lib, streams[f], K)), f
    # the same two frames through their indexes, and as bands
    indexes = [_part1_index(lib, s, K) for s in streams]
    arena = Arena(torch, gs)
    _, errcs = batch.decode_batch_ragged_indexed(blob, offsets, sizes, indexes, arena.outs, strides=strides, capacities=capacities, lib=lib)
    torch.cuda.synchronize()
    assert errcs.tolist() == want_errcs
    arena.check([None if f in (short, small) else w for f, w in enumerate(wants)])
    # an index slot too small: nothing of that frame is decoded
    arena = Arena(torch, gs)
    bounds = [bound(p, K, lib) for p in ps]
    largest = max(range(len(ps)), key=lambda f: bounds[f])
    _, errcs, built = batch.index_batch_packed(blob, offsets, sizes, K, outs=arena.outs, strides=arena.strides, capacities=arena.capacities,
                                               index_pitch=bounds[largest] - 1, lib=lib)
    torch.cuda.synchronize()
    refused = [f for f in range(len(ps)) if bounds[f] > bounds[largest] - 1]
    assert largest in refused
    assert errcs.tolist() == [INVALID_ARGUMENT_SIZE if f in refused else SUCCESS for f in range(len(ps))]
    arena.check([None if f in refused else w for f, w in enumerate(wants)])
    assert all(built[f] == b"" for f in refused)
    _, errcs, built = build_index_only(lib, blob, offsets, sizes, K, bounds[largest] - 1)
    assert errcs.tolist() == [INVALID_ARGUMENT_SIZE if f in refused else SUCCESS for f in range(len(ps))]
    assert all(built[f] == b"" for f in refused)


# ---- ragged indexed decode -----------------------------------------------------------------------------------------------

def test_ragged_indexed_decode_goes_through_the_seek_points(torch, lib, mixed):
    ps, streams, wants = mixed
    K = 4
    blob, offsets, sizes = pack(torch, streams)
    _, errcs, built = build_index_only(lib, blob, offsets, sizes, K, max(bound(p, K, lib) for p in ps))
    assert errcs.tolist() == [SUCCESS] * len(ps)
    arena = Arena(torch, [geometry(p) for p in ps])
    before = capi.index_counters(lib)
    params, errcs = batch.decode_batch_ragged_indexed(blob, offsets, sizes, built, arena.outs, strides=arena.strides,
                                                      capacities=arena.capacities, lib=lib)
    torch.cuda.synchronize()
    after = capi.index_counters(lib)
    assert errcs.tolist() == [SUCCESS] * len(ps)
    arena.check(wants)
    assert after["fallback_scans"] == before["fallback_scans"]
    assert after["scans_from_points"] == before["scans_from_points"] + sum(scans_of(p) for p in ps if p["height"] > K)
    for f, p in enumerate(ps):
        assert (params[f].frame_info.width, params[f].frame_info.height) == (p["width"], p["height"]), f


def test_one_tampered_index_costs_that_frame_a_fallback(torch, lib):
    p, streams, wants = _gray(8, seed0=300)
    blob, offsets, sizes = pack(torch, streams)
    _, errcs, indexes = build_index_only(lib, blob, offsets, sizes, 8, bound(p, 8, lib))
    assert errcs.tolist() == [SUCCESS] * 8
    point_bytes = int.from_bytes(indexes[3][64:68], "little")
    bad = list(indexes)
    bad[3] = _tamper(indexes[3], "context", point_bytes)
    assert bad[3] != indexes[3]
    arena = Arena(torch, [geometry(p)] * 8)
    before = capi.index_counters(lib)
    _, errcs = batch.decode_batch_ragged_indexed(blob, offsets, sizes, bad, arena.outs, strides=arena.strides, capacities=arena.capacities, lib=lib)
    torch.cuda.synchronize()
    after = capi.index_counters(lib)
    assert errcs.tolist() == [SUCCESS] * 8
    arena.check(wants)
    assert after["fallback_scans"] == before["fallback_scans"] + 1
    assert after["scans_from_points"] == before["scans_from_points"] + 7


# ---- ragged bands --------------------------------------------------------------------------------------------------------

def band_arena(torch, ps, bands_rows):
    """A band per frame in one canary buffer: padded rows, the smallest capacity, 8-bit bands at odd and 16-bit at even bases."""
    wide = ps[0]["bits"] > 8
    row = ps[0]["width"] * (2 if wide else 1) * (1 if ps[0]["ilv"] == 0 else ps[0]["comps"])
    stride = row + (2 if wide else 3)
    scans = scans_of(ps[0])
    needs = [stride * count * scans - (stride - row) for _, count in bands_rows]
    pitch = (max(needs) + 2 + 31) & ~15
    base = 2 if wide else 1
    device = torch.full((len(ps), pitch), CANARY, dtype=torch.uint8, device="cuda")
    return device, [device[f, base:] for f in range(len(ps))], stride, row, scans, needs, base


@pytest.mark.parametrize("name", sorted(BAND_SETS))
@pytest.mark.parametrize("which", ["indexed", "from_the_top", "mixed"])
def test_ragged_bands(torch, lib, name, which):
    ps = BAND_SETS[name]
    streams = [_stream(p) for p in ps]
    wants = [ob.decode(s)[1] for s in streams]
    blob, offsets, sizes = pack(torch, streams)
    built = [_part1_index(lib, s, p["K"]) for s, p in zip(streams, ps)]
    indexes = {"indexed": built, "from_the_top": [None] * len(ps), "mixed": [ix if f % 2 == 0 else None for f, ix in enumerate(built)]}[which]
    for shift in (0, 2, 3):  # the top, across a seek point, the last row (and the others, frame by frame)
        bands_rows = [_band_of(p, f + shift) for f, p in enumerate(ps)]
        device, outs, stride, row, scans, needs, base = band_arena(torch, ps, bands_rows)
        errcs = batch.decode_rows_batch_ragged(blob, offsets, sizes, indexes, [b[0] for b in bands_rows], [b[1] for b in bands_rows], outs,
                                               strides=[stride] * len(ps), capacities=needs, lib=lib)
        torch.cuda.synchronize()
        assert errcs.tolist() == [SUCCESS] * len(ps), (shift, errcs)
        got = device.cpu().numpy()
        for f, (p, (first, count)) in enumerate(zip(ps, bands_rows)):
            rows = np.frombuffer(_band(wants[f], p, first, count), dtype=np.uint8).reshape(scans * count, row)
            want = np.full(got.shape[1], CANARY, dtype=np.uint8)
            for r in range(scans * count):
                want[base + r * stride:base + r * stride + row] = rows[r]
            assert got[f].tobytes() == want.tobytes(), (shift, f, first, count)


def test_bands_refuse_a_foreign_index_and_a_small_capacity_for_that_frame_only(torch, lib):
    p, streams, wants = _gray(8, seed0=300)
    blob, offsets, sizes = pack(torch, streams)
    indexes = [_part1_index(lib, s, 8) for s in streams]
    indexes[2] = indexes[6]
    device = torch.full((8, 96 * 8 + 16), CANARY, dtype=torch.uint8, device="cuda")
    outs = [device[f, 1:] for f in range(8)]
    capacities = [96 * 8] * 8
    capacities[5] -= 1
    errcs = batch.decode_rows_batch_ragged(blob, offsets, sizes, indexes, [40] * 8, [8] * 8, outs, strides=[0] * 8, capacities=capacities, lib=lib)
    torch.cuda.synchronize()
    assert errcs.tolist() == [0, 0, INVALID_ARGUMENT, 0, 0, INVALID_ARGUMENT_SIZE, 0, 0]
    got = device.cpu().numpy()
    for f in range(8):
        if f in (2, 5):
            assert (got[f] == CANARY).all(), f
        else:
            assert got[f, 1:1 + 96 * 8].tobytes() == wants[f][40 * 96:48 * 96], f
            assert got[f, 0] == CANARY and (got[f, 1 + 96 * 8:] == CANARY).all(), f


# ---- launches --------------------------------------------------------------------------------------------------------------

def test_sixteen_equal_frames_are_one_launch_in_each_call(torch, lib):
    ps = [dict(width=33, height=20, bits=8, comps=1, ilv=0, near=0, kind="mixed", seed=930 + i) for i in range(16)]
    streams = [_stream(p) for p in ps]
    wants = [ob.decode(s)[1].tobytes() for s in streams]
    K = 4
    blob, offsets, sizes = pack(torch, streams)
    launches = batch.seek_launches(lib)
    _, errcs, indexes = build_index_only(lib, blob, offsets, sizes, K, bound(ps[0], K, lib))
    assert errcs.tolist() == [SUCCESS] * 16
    assert batch.seek_launches(lib) == launches + 1
    assert indexes == [_part1_index(lib, s, K) for s in streams]
    arena = Arena(torch, [geometry(p) for p in ps])
    before, launches = capi.index_counters(lib), batch.seek_launches(lib)
    _, errcs = batch.decode_batch_ragged_indexed(blob, offsets, sizes, indexes, arena.outs, strides=arena.strides, capacities=arena.capacities, lib=lib)
    torch.cuda.synchronize()
    after = capi.index_counters(lib)
    assert errcs.tolist() == [SUCCESS] * 16
    assert batch.seek_launches(lib) == launches + 1
    assert after["intervals"] == before["intervals"] + 16 * 5
    assert after["scans_from_points"] == before["scans_from_points"] + 16
    arena.check(wants)
    device = torch.full((16, 33 * 3 + 15), CANARY, dtype=torch.uint8, device="cuda")
    launches = batch.seek_launches(lib)
    errcs = batch.decode_rows_batch_ragged(blob, offsets, sizes, indexes, [3] * 16, [3] * 16, [device[f, 1:] for f in range(16)],
                                           strides=[0] * 16, capacities=[33 * 3] * 16, lib=lib)
    torch.cuda.synchronize()
    assert errcs.tolist() == [SUCCESS] * 16
    assert batch.seek_launches(lib) == launches + 1
    got = device.cpu().numpy()
    for f in range(16):
        assert got[f, 1:1 + 99].tobytes() == wants[f][3 * 33:6 * 33], f


# ---- interchange -----------------------------------------------------------------------------------------------------------

def test_an_index_built_here_drives_the_salvage_decode_and_part_1(torch, lib):
    import test_gpu_salvage_index as tsi
    name, K = "gray8", 4
    s = tsi.sound(lib, name, K)
    w, h = tsi.FRAMES[name][:2]
    blob, offsets, sizes = pack(torch, [s.jls])
    _, errcs, mine = build_index_only(lib, blob, offsets, sizes, K, batch.index_size_bound(w, h, lines_per_seek_point=K, lib=lib))
    assert errcs.tolist() == [SUCCESS]
    d_streams, slot_sizes = _slots([s.jls])
    out = torch.zeros((1, h, w), dtype=torch.uint8, device="cuda")
    _, errcs, theirs = batch.decode_batch_and_index(d_streams, slot_sizes, out, K, lib=lib)
    assert errcs.tolist() == [SUCCESS]
    d = sim.zero4(s, 5)
    assert tsi.oracle_raises(d.data)
    exp = sim.expected_index(s, d.raw, 0x5B)
    results = []
    for index in (mine[0], theirs[0]):
        got, lay, arena = tsi.run_in_arena(torch, lib, s, name, d.data, index, 0x5B)
        lay.check(arena, [exp.pixels], what="salvaged through the index")
        results.append((int(got.errcs[0]), got.reports[0].astuple(), got.status[0].tolist(), arena.tobytes()))
    assert results[0] == results[1]
    assert results[0][1] == exp.report
    before = capi.index_counters(lib)
    assert lib.decode(s.jls, index=mine[0])[1].tobytes() == s.pixels
    after = capi.index_counters(lib)
    assert after["fallback_scans"] == before["fallback_scans"] and after["scans_from_points"] > before["scans_from_points"]


# ---- host form -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("memory", ["pageable", "pinned"])
@pytest.mark.parametrize("window", [0, 5])
def test_host_form_gives_the_device_calls_results(torch, lib, knobs, mixed, memory, window):
    ps, streams, _ = mixed
    K = 4
    extra, _ = odd_frames(lib, mixed)
    everything = streams + extra
    blob, offsets, sizes = pack(torch, everything)
    pitch = max([bound(p, K, lib) for p in ps] + [batch.index_size_bound(64, 40, lines_per_seek_point=K, lib=lib)]) + 40
    want_params, want_errcs, want = build_index_only(lib, blob, offsets, sizes, K, pitch)
    data = b"".join(everything)
    host = batch.host_alloc(len(data), lib=lib) if memory == "pinned" else np.empty(len(data), dtype=np.uint8)
    host[:] = np.frombuffer(data, dtype=np.uint8)
    if window:
        knobs.set("HOST_WINDOW_FRAMES", window)
    calls = batch.host_counters(lib)
    table = np.full((len(everything), pitch), CANARY, dtype=np.uint8)
    params, errcs, built = batch.index_batch_host(host, offsets, sizes, K, index_pitch=pitch, indexes_out=table, lib=lib)
    after = batch.host_counters(lib)
    assert errcs.tolist() == want_errcs.tolist()
    assert built == want
    for f, ix in enumerate(built):
        assert (table[f, len(ix):] == CANARY).all(), f
        assert bytes(params[f]) == bytes(want_params[f]), f
    assert after[1] - calls[1] == (-(-len(everything) // window) if window else 1)  # windows
    assert after[3] == calls[3]  # nothing comes down
