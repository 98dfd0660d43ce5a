"""The seek-point index in the batch API (charls_amd.h part 2c): charls_amd_decode_batch_device_and_index,
charls_amd_decode_batch_device_indexed and charls_amd_decode_rows_batch_device on device-resident streams.

Streams come from the oracle's encoder, pixels are compared with the oracle's decoder byte for byte, indexes with the
bytes part 1 builds for the same stream:
  * a batch of 24 frames that differ in everything builds, per K, the pixels and the very index bytes of part 1, inside
    every frame's own extent of the frame and index slots;
  * batch-built indexes decode on part 1 and part-1 indexes in the batch, without a fallback;
  * a batch is a batch: one launch of the seek kernels for 16 frames, and for planar frames a number of launches that does
    not grow with the frames;
  * bands at the top, in the middle, across a seek point and at the last row, with indexes, without, and mixed, at padded
    strides;
  * one tampered or foreign index in a batch costs that frame a fallback (or an errc) and the others nothing;
  * damaged streams give decode_batch's errcs; argument errors stay with their frame;
  * building 16 indexes in one call is much faster than 16 part-1 builds (slow).
16-bit frames lie at even addresses here (frame pitches are rounded up to 16): at odd ones they go the ordinary way and
get an index without seek points, which tests/test_gpu_strides.py's ordinary path covers.  GPU only."""
import ctypes as C
import random
import time

import numpy as np
import pytest

import oracle_bind as ob
from charls_amd import batch, capi, synth
from test_gpu_seek_index import _band, _fixture, _mutations, _params, _stream, _tamper

pytestmark = pytest.mark.gpu

SUCCESS, INVALID_ARGUMENT, INVALID_ARGUMENT_SIZE, INVALID_ARGUMENT_STRIDE = 0, 101, 110, 111
CANARY = 0xC3


@pytest.fixture(scope="module")
def lib():
    return capi.load_product()


def _torch():
    import torch
    return torch


def _slots(streams, odd=True):
    """(F, pitch) uint8 device tensor with stream f in slot f (zeros behind it), sizes; an odd pitch on request."""
    torch = _torch()
    pitch = max(len(s) for s in streams) + 16
    pitch += (pitch & 1) ^ (1 if odd else 0)
    host = np.zeros((len(streams), pitch), dtype=np.uint8)
    for f, s in enumerate(streams):
        host[f, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    return torch.from_numpy(host).cuda(), np.array([len(s) for s in streams], dtype=np.uint64)


def _frames(count, pitch):
    torch = _torch()
    return torch.full((count, pitch), CANARY, dtype=torch.uint8, device="cuda")


def _check_frames(out, wants):
    got = out.cpu().numpy()
    for f, want in enumerate(wants):
        n = len(want)
        assert got[f, :n].tobytes() == want, f
        assert (got[f, n:] == CANARY).all(), f


def _pitch(p, K, lib):
    return batch.index_size_bound(p["width"], p["height"], p["bits"], p["comps"], p["ilv"], p["near"], K, lib=lib)


def _part1_index(lib, jls, K, cache={}):
    key = (jls, K)
    if key not in cache:
        cache[key] = lib.decode_with_index(jls, lines_per_seek_point=K)[2]
    return cache[key]


@pytest.fixture(scope="module")
def mixed():
    """The first 24 parameter sets of test_gpu_seek_index.py: part 1 decodes them through its index without a fallback."""
    ps = [_params(random.Random(s)) for s in range(24)]
    streams = [_stream(p) for p in ps]
    wants = [ob.decode(s)[1].tobytes() for s in streams]
    return ps, streams, wants


@pytest.mark.parametrize("K", [1, 4, 16])
def test_mixed_batch_builds_the_pixels_and_indexes_of_part_1(lib, mixed, K):
    ps, streams, wants = mixed
    l = batch._bind(lib)
    d_streams, sizes = _slots(streams, odd=True)
    assert d_streams.shape[1] % 2 == 1
    frame_pitch = (max(len(w) for w in wants) + 15) & ~15
    out = _frames(len(ps), frame_pitch)
    bounds = [batch.index_size_bound(p["width"], p["height"], p["bits"], p["comps"], p["ilv"], p["near"], K, lib=lib) for p in ps]
    index_pitch = max(bounds) + 40
    indexes = np.full((len(ps), index_pitch), CANARY, dtype=np.uint8)
    index_sizes = np.full(len(ps), 77, dtype=np.uint64)
    errcs = np.full(len(ps), -1, dtype=np.int32)
    params = batch.CodecParams()
    before = capi.index_counters(lib)
    rc = l.charls_amd_decode_batch_device_and_index(len(ps), d_streams.data_ptr(), d_streams.shape[1],
                                                    sizes.ctypes.data_as(C.POINTER(C.c_uint64)), out.data_ptr(), frame_pitch, 0, K,
                                                    indexes.ctypes.data, index_pitch, index_sizes.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                    C.byref(params), errcs.ctypes.data_as(C.POINTER(C.c_int32)), None)
    assert rc == 0
    assert errcs.tolist() == [0] * len(ps)
    _check_frames(out, wants)
    assert (params.frame_info.width, params.frame_info.height) == (ps[0]["width"], ps[0]["height"])
    for f, p in enumerate(ps):
        want = _part1_index(lib, streams[f], K)
        n = int(index_sizes[f])
        assert n == len(want) <= bounds[f], f
        assert indexes[f, :n].tobytes() == want, (f, p)
        assert (indexes[f, n:] == CANARY).all(), f
    assert capi.index_counters(lib)["fallback_scans"] == before["fallback_scans"]


def test_indexes_cross_between_part_1_and_the_batch(lib, mixed):
    ps, streams, wants = mixed
    K = 4
    d_streams, sizes = _slots(streams)
    frame_pitch = (max(len(w) for w in wants) + 15) & ~15
    out = _frames(len(ps), frame_pitch)
    _, errcs, built = batch.decode_batch_and_index(d_streams, sizes, out, K, index_pitch=max(
        batch.index_size_bound(p["width"], p["height"], p["bits"], p["comps"], p["ilv"], p["near"], K, lib=lib) for p in ps), lib=lib)
    assert errcs.tolist() == [0] * len(ps)
    # batch-built -> part 1
    for f, p in enumerate(ps):
        before = capi.index_counters(lib)
        _, px = lib.decode(streams[f], index=built[f])
        after = capi.index_counters(lib)
        assert px.tobytes() == wants[f], f
        assert after["fallback_scans"] == before["fallback_scans"], f
        if p["height"] > K:
            assert after["scans_from_points"] > before["scans_from_points"], f
    # part 1 -> batch
    theirs = [_part1_index(lib, s, K) for s in streams]
    out = _frames(len(ps), frame_pitch)
    before = capi.index_counters(lib)
    _, errcs = batch.decode_batch_indexed(d_streams, sizes, theirs, out, lib=lib)
    after = capi.index_counters(lib)
    assert errcs.tolist() == [0] * len(ps)
    _check_frames(out, wants)
    assert after["fallback_scans"] == before["fallback_scans"]
    scans_with_points = sum((p["comps"] if p["ilv"] == 0 else 1) for p in ps if p["height"] > K)
    assert after["scans_from_points"] == before["scans_from_points"] + scans_with_points


def _gray(count, seed0=200):
    fx = [_fixture(width=96, height=80, K=8, seed=seed0 + i) for i in range(count)]
    streams = [jls for _, jls in fx]
    return fx[0][0], streams, [ob.decode(s)[1].tobytes() for s in streams]


def test_sixteen_frames_are_one_launch(lib):
    p, streams, wants = _gray(16)
    d_streams, sizes = _slots(streams)
    out = _frames(16, 96 * 80)
    launches = batch.seek_launches(lib)
    _, errcs, indexes = batch.decode_batch_and_index(d_streams, sizes, out, 8, index_pitch=_pitch(p, 8, lib), lib=lib)
    assert errcs.tolist() == [0] * 16
    assert batch.seek_launches(lib) == launches + 1
    _check_frames(out, wants)
    out = _frames(16, 96 * 80)
    before, launches = capi.index_counters(lib), batch.seek_launches(lib)
    _, errcs = batch.decode_batch_indexed(d_streams, sizes, indexes, out, lib=lib)
    after = capi.index_counters(lib)
    assert errcs.tolist() == [0] * 16
    assert batch.seek_launches(lib) == launches + 1
    assert after["intervals"] == before["intervals"] + 160
    assert after["scans_from_points"] == before["scans_from_points"] + 16
    assert after["fallback_scans"] == before["fallback_scans"]
    _check_frames(out, wants)


def _planar(count):
    ps = [dict(width=64, height=40, bits=8, comps=3, ilv=0, near=0, kind="mixed", seed=400 + i, K=8) for i in range(count)]
    streams = [_stream(p) for p in ps]
    return ps, streams, [ob.decode(s)[1].tobytes() for s in streams]


def test_planar_launches_do_not_grow_with_the_frames(lib):
    """Building runs one launch per scan ordinal (scan c + 1 starts where scan c ended): 3 for three-component planar frames;
    decoding through the indexes is one launch for all scans of all frames (the index names every segment's length)."""
    counted = {}
    for count in (4, 16):
        ps, streams, wants = _planar(count)
        p = ps[0]
        d_streams, sizes = _slots(streams)
        out = _frames(count, 3 * 64 * 40)
        launches = batch.seek_launches(lib)
        _, errcs, indexes = batch.decode_batch_and_index(d_streams, sizes, out, 8, index_pitch=_pitch(p, 8, lib), lib=lib)
        built = batch.seek_launches(lib) - launches
        assert errcs.tolist() == [0] * count
        _check_frames(out, wants)
        assert [bytes(ix) for ix in indexes] == [_part1_index(lib, s, 8) for s in streams]
        out = _frames(count, 3 * 64 * 40)
        before, launches = capi.index_counters(lib), batch.seek_launches(lib)
        _, errcs = batch.decode_batch_indexed(d_streams, sizes, indexes, out, lib=lib)
        used = batch.seek_launches(lib) - launches
        after = capi.index_counters(lib)
        assert errcs.tolist() == [0] * count
        _check_frames(out, wants)
        assert after["scans_from_points"] == before["scans_from_points"] + 3 * count
        assert after["intervals"] == before["intervals"] + 3 * 5 * count
        assert after["fallback_scans"] == before["fallback_scans"]
        counted[count] = (built, used)
    assert counted[4] == counted[16] == (3, 1)


BAND_SETS = {
    "gray8": [dict(width=96, height=h, bits=8, comps=1, ilv=0, near=0, kind="mixed", seed=500 + i, K=8) for i, h in enumerate([80, 57, 80, 33, 80, 80, 57, 33])],
    "gray12": [dict(width=64, height=40, bits=12, comps=1, ilv=0, near=n, kind="mixed", seed=520 + i, K=8) for i, n in enumerate([0, 0, 3, 0])],
    "planar8": [dict(width=33, height=40, bits=8, comps=3, ilv=0, near=0, kind="mixed", seed=540 + i, K=4) for i in range(4)],
    "sample8": [dict(width=33, height=40, bits=8, comps=3, ilv=2, near=0, kind="mixed", seed=560 + i, K=4) for i in range(4)],
    "line16": [dict(width=20, height=24, bits=16, comps=3, ilv=1, near=0, kind="noise", seed=580 + i, K=4) for i in range(4)],
}


def _band_of(p, kind):
    h, K = p["height"], p["K"]
    return [(0, 1), (h // 2 - h // 8, max(1, h // 4)), (K - 1, min(2, h - K + 1)), (h - 1, 1)][kind % 4]


@pytest.mark.parametrize("name", sorted(BAND_SETS))
@pytest.mark.parametrize("which", ["indexed", "from_the_top", "mixed"])
def test_bands_of_many_frames(lib, name, which):
    ps = BAND_SETS[name]
    streams = [_stream(p) for p in ps]
    wants = [ob.decode(s)[1] for s in streams]
    d_streams, sizes = _slots(streams)
    built = [_part1_index(lib, s, p["K"]) for s, p in zip(streams, ps)]
    indexes = {"indexed": built, "from_the_top": [None] * len(ps), "mixed": [ix if f % 2 == 0 else None for f, ix in enumerate(built)]}[which]
    wide = ps[0]["bits"] > 8
    row = ps[0]["width"] * (2 if wide else 1) * (1 if ps[0]["ilv"] == 0 else ps[0]["comps"])
    stride = row + (2 if wide else 3)
    scans = ps[0]["comps"] if ps[0]["ilv"] == 0 else 1
    for shift in range(4):
        bands_rows = [_band_of(p, f + shift) for f, p in enumerate(ps)]
        band_pitch = (max(stride * count * scans for _, count in bands_rows) + 15) & ~15
        bands = _frames(len(ps), band_pitch)
        errcs = batch.decode_rows_batch(d_streams, sizes, indexes, [b[0] for b in bands_rows], [b[1] for b in bands_rows], bands,
                                        stride=stride, lib=lib)
        assert errcs.tolist() == [0] * len(ps), (shift, errcs)
        got = bands.cpu().numpy()
        for f, (p, (first, count)) in enumerate(zip(ps, bands_rows)):
            rows = np.frombuffer(_band(wants[f], p, first, count), dtype=np.uint8).reshape(scans * count, row)
            want = np.full(band_pitch, CANARY, dtype=np.uint8)
            for r in range(scans * count):
                want[r * stride:r * stride + row] = rows[r]
            assert got[f].tobytes() == want.tobytes(), (shift, f, first, count)


def _out_of_range(index, point_bytes):
    """The reader position of point 3 pushed past any segment: set_index refuses it."""
    b = bytearray(index)
    at = 72 + 24 + 4 * point_bytes - 24
    b[at:at + 8] = (1 << 40).to_bytes(8, "little")
    return bytes(b)


@pytest.mark.parametrize("how", ["context", "sample", "swap", "foreign", "out_of_range"])
def test_one_tampered_index_in_a_batch(lib, how):
    p, streams, wants = _gray(8, seed0=300)
    d_streams, sizes = _slots(streams)
    out = _frames(8, 96 * 80)
    _, errcs, indexes = batch.decode_batch_and_index(d_streams, sizes, out, 8, index_pitch=_pitch(p, 8, lib), lib=lib)
    assert errcs.tolist() == [0] * 8
    point_bytes = int.from_bytes(indexes[3][64:68], "little")
    bad = list(indexes)
    bad[3] = _out_of_range(indexes[3], point_bytes) if how == "out_of_range" else _tamper(indexes[3], how, point_bytes, indexes[5])
    assert bad[3] != indexes[3]
    out = _frames(8, 96 * 80)
    before = capi.index_counters(lib)
    _, errcs = batch.decode_batch_indexed(d_streams, sizes, bad, out, lib=lib)
    after = capi.index_counters(lib)
    got = out.cpu().numpy()
    if how == "out_of_range":
        assert errcs.tolist() == [0, 0, 0, INVALID_ARGUMENT, 0, 0, 0, 0]
        assert (got[3] == CANARY).all()
        assert after["fallback_scans"] == before["fallback_scans"]
    else:
        assert errcs.tolist() == [0] * 8
        assert got[3].tobytes() == wants[3]
        assert after["fallback_scans"] == before["fallback_scans"] + 1
    for f in range(8):
        if f != 3:
            assert got[f].tobytes() == wants[f], f
    assert after["scans_from_points"] == before["scans_from_points"] + 7


def test_bands_refuse_a_foreign_index_for_that_frame_only(lib):
    p, streams, wants = _gray(8, seed0=300)
    d_streams, sizes = _slots(streams)
    indexes = [_part1_index(lib, s, 8) for s in streams]
    indexes[2] = indexes[6]
    bands = _frames(8, 96 * 8)
    errcs = batch.decode_rows_batch(d_streams, sizes, indexes, [40] * 8, [8] * 8, bands, lib=lib)
    assert errcs.tolist() == [0, 0, INVALID_ARGUMENT, 0, 0, 0, 0, 0]
    got = bands.cpu().numpy()
    for f in range(8):
        if f == 2:
            assert (got[f] == CANARY).all()
        else:
            assert got[f].tobytes() == wants[f][40 * 96:48 * 96], f


def test_damaged_streams_through_the_index_of_the_undamaged_stream(lib):
    p, jls = _fixture(kind="noise")
    index = _part1_index(lib, jls, p["K"])
    damaged = _mutations(jls, random.Random(3), 24)
    d_streams, sizes = _slots(damaged)
    plain_out = _frames(24, 96 * 80)
    _, plain, _ = batch.decode_batch(d_streams, sizes, plain_out, lib=lib)
    out = _frames(24, 96 * 80)
    _, errcs = batch.decode_batch_indexed(d_streams, sizes, [index] * 24, out, lib=lib)
    assert errcs.tolist() == plain.tolist()
    a, b = out.cpu().numpy(), plain_out.cpu().numpy()
    for f in range(24):
        if plain[f] == 0:
            assert a[f].tobytes() == b[f].tobytes(), f


def test_argument_errors_stay_with_their_frame(lib):
    ps = [dict(width=96, height=80, bits=8, comps=1, ilv=0, near=0, kind="mixed", seed=600, K=8),
          dict(width=64, height=40, bits=8, comps=1, ilv=0, near=0, kind="mixed", seed=601, K=8),
          dict(width=96, height=80, bits=8, comps=1, ilv=0, near=0, kind="mixed", seed=602, K=8)]
    streams = [_stream(p) for p in ps]
    wants = [ob.decode(s)[1].tobytes() for s in streams]
    d_streams, sizes = _slots(streams)
    big = batch.index_size_bound(96, 80, lines_per_seek_point=8, lib=lib)
    small = batch.index_size_bound(64, 40, lines_per_seek_point=8, lib=lib)
    assert small < big - 1
    # an index pitch one byte below what the large frames need: they are not decoded, the small one is
    out = _frames(3, 96 * 80)
    _, errcs, indexes = batch.decode_batch_and_index(d_streams, sizes, out, 8, index_pitch=big - 1, lib=lib)
    assert errcs.tolist() == [INVALID_ARGUMENT_SIZE, 0, INVALID_ARGUMENT_SIZE]
    got = out.cpu().numpy()
    assert (got[0] == CANARY).all() and (got[2] == CANARY).all()
    assert got[1, :64 * 40].tobytes() == wants[1]
    assert indexes[0] == b"" and indexes[2] == b"" and indexes[1] == _part1_index(lib, streams[1], 8)
    # a stride below the wide frames' row
    indexes = [_part1_index(lib, s, 8) for s in streams]
    out = _frames(3, 96 * 80)
    _, errcs, _ = batch.decode_batch_and_index(d_streams, sizes, out, 8, index_pitch=big, stride=80, lib=lib)
    assert errcs.tolist() == [INVALID_ARGUMENT_STRIDE, 0, INVALID_ARGUMENT_STRIDE]
    bands = _frames(3, 96 * 8)
    errcs = batch.decode_rows_batch(d_streams, sizes, indexes, [0, 0, 0], [4, 4, 4], bands, stride=80, lib=lib)
    assert errcs.tolist() == [INVALID_ARGUMENT_STRIDE, 0, INVALID_ARGUMENT_STRIDE]
    # no rows, a band past the height, a band slot too small
    bands = _frames(3, 96 * 8)
    errcs = batch.decode_rows_batch(d_streams, sizes, indexes, [10, 36, 79], [0, 5, 1], bands, lib=lib)
    assert errcs.tolist() == [INVALID_ARGUMENT, INVALID_ARGUMENT, 0]
    got = bands.cpu().numpy()
    assert (got[0] == CANARY).all() and (got[1] == CANARY).all()
    assert got[2, :96].tobytes() == wants[2][79 * 96:]
    errcs = batch.decode_rows_batch(d_streams, sizes, indexes, [0, 0, 0], [9, 9, 8], bands, lib=lib)
    assert errcs.tolist() == [INVALID_ARGUMENT_SIZE, 0, 0]
    l = batch._bind(lib)
    assert l.charls_amd_decode_batch_device_and_index(1, d_streams.data_ptr(), d_streams.shape[1], sizes.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                      out.data_ptr(), 96 * 80, 0, 0, got.ctypes.data, 64, sizes.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                      None, errcs.ctypes.data_as(C.POINTER(C.c_int32)), None) == INVALID_ARGUMENT


def test_seek_buffers_are_work_areas(lib):
    p, streams, wants = _gray(4)
    d_streams, sizes = _slots(streams)
    out = _frames(4, 96 * 80)
    batch.release_work_areas(lib)
    held = batch.work_area_bytes(lib)
    batch.decode_batch_and_index(d_streams, sizes, out, 8, index_pitch=_pitch(p, 8, lib), lib=lib)
    assert batch.work_area_bytes(lib) > held
    batch.release_work_areas(lib)
    assert batch.work_area_bytes(lib) <= held


@pytest.mark.slow
def test_building_sixteen_indexes_in_one_call(lib, capsys):
    """16 frames of 512 x 512: the part-1 loop is the only way to build them without the batch call, and is the reference.
    The 16 builds occupy 16 SIMDs side by side, so about 16 x is expected; 4 x leaves room for launch overheads and clocks."""
    imgs = [synth.frame_numpy(512, 512, seed=700 + i, bits=8) for i in range(16)]
    streams = [ob.encode(img, width=512, height=512, bits_per_sample=8) for img in imgs]
    d_streams, sizes = _slots(streams)
    out = _frames(16, 512 * 512)
    pitch = batch.index_size_bound(512, 512, lines_per_seek_point=64, lib=lib)
    batch.decode_batch_and_index(d_streams[:1], sizes[:1], out[:1], 64, index_pitch=pitch, lib=lib)  # (warm)
    lib.decode_with_index(streams[0], lines_per_seek_point=64)
    _torch().cuda.synchronize()
    a = time.perf_counter()
    _, errcs, indexes = batch.decode_batch_and_index(d_streams, sizes, out, 64, index_pitch=pitch, lib=lib)
    together = time.perf_counter() - a
    a = time.perf_counter()
    theirs = [lib.decode_with_index(s, lines_per_seek_point=64)[2] for s in streams]
    loop = time.perf_counter() - a
    with capsys.disabled():
        print(f"\n[seek index, batch] 16 x 512x512 K=64: one call {together:.3f}s, part-1 loop {loop:.3f}s ({loop / together:.1f} x)")
    assert errcs.tolist() == [0] * 16
    assert indexes == theirs
    _check_frames(out, [img.tobytes() for img in imgs])
    assert together < loop / 4
