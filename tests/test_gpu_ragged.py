"""Ragged frames in the batch API (charls_amd.h part 2e): one call over frames that differ in geometry and coding parameters and
sit in allocations of their own.  The contract of every call is stated against the packed calls of part 2d, so every test here
compares with them -- the ragged encoder with charls_amd_encode_batch_device_packed called on each frame alone (and with the
oracle's stream), the probe and the ragged decoder with charls_amd_decode_batch_device_packed and part 1's reader.  Every
destination is filled with a canary first: nothing outside what a call owns may change.  All frames are tiny.  GPU only."""
import ctypes as C

import numpy as np
import pytest

import oracle_bind as ob
import strided
from charls_amd import batch, capi, synth
from strided import Geometry

pytestmark = pytest.mark.gpu

CANARY = 0xA5
NOT_ENOUGH_MEMORY, DESTINATION_TOO_SMALL = 1, 3
INVALID_ARGUMENT_BITS, INVALID_ARGUMENT_COLOR_TRANSFORMATION, INVALID_ARGUMENT_SIZE, INVALID_ARGUMENT_STRIDE = 104, 109, 110, 111
u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)

# kind -> (geometry, NEAR, restart interval, frames of that kind)
KINDS = {
    "gray_4096x4": (Geometry(4096, 4), 0, 0, 4),
    "gray_150x7": (Geometry(150, 7), 0, 0, 3),
    "gray_8192x2": (Geometry(8192, 2), 0, 0, 3),
    "gray_1x1": (Geometry(1, 1), 0, 0, 3),
    "gray_64x64": (Geometry(64, 64), 0, 0, 4),
    "gray12_33x17": (Geometry(33, 17, bits=12), 0, 0, 3),
    "rgb_planar_40x9": (Geometry(40, 9, comps=3, ilv=0), 0, 0, 4),
    "rgb_line_31x6": (Geometry(31, 6, comps=3, ilv=1), 0, 0, 3),
    "rgb_sample_31x6": (Geometry(31, 6, comps=3, ilv=2), 0, 0, 3),
    "near2_70x5": (Geometry(70, 5), 2, 0, 3),
    "restart2_50x6": (Geometry(50, 6), 0, 2, 3),
}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def l():
    return batch._bind(capi.load_product())


def rule_offsets(sizes, alignment):
    """offsets[0] = 0, offsets[f + 1] = offsets[f] + sizes[f] rounded up to the alignment."""
    out = [0]
    for s in sizes:
        out.append(-(-(out[-1] + int(s)) // alignment) * alignment)
    return np.array(out, dtype=np.uint64)


def canary_buffer(torch, nbytes):
    return torch.full((nbytes,), CANARY, dtype=torch.uint8, device="cuda:0")


def to_device(torch, img):
    return torch.from_numpy(img.view(np.int16) if img.dtype == np.uint16 else img).cuda()


def packed_alone(torch, l, params, pointer, stride=0, max_stream_bytes=0):
    """charls_amd_encode_batch_device_packed on ONE frame: (return value, errc, the stream)."""
    dst = canary_buffer(torch, 1 << 17)
    offsets, sizes, errcs = np.zeros(2, dtype=np.uint64), np.zeros(1, dtype=np.uint64), np.full(1, -1, dtype=np.int32)
    rc = l.charls_amd_encode_batch_device_packed(C.byref(params), 1, pointer, 1 << 40, stride, dst.data_ptr(), dst.numel(), 1, max_stream_bytes,
                                                 offsets.ctypes.data_as(u64p), sizes.ctypes.data_as(u64p), errcs.ctypes.data_as(i32p), None)
    return rc, int(errcs[0]), dst[:int(sizes[0])].cpu().numpy().tobytes()


class Frame:
    def __init__(self, torch, l, kind, seed):
        self.kind = kind
        self.g, self.near, self.restart, _ = KINDS[kind]
        self.img = strided.mixed(self.g, seed)
        self.tensor = to_device(torch, self.img)  # an allocation of its own
        self.params = strided.codec_params(self.g, near=self.near, restart=self.restart)
        rc, errc, self.jls = packed_alone(torch, l, self.params, self.tensor.data_ptr())
        assert rc == 0 and errc == 0 and len(self.jls) > 0
        if not self.restart:  # (the reference's encoder writes no restart markers)
            assert self.jls == ob.encode(self.img, near_lossless=self.near, destination_size=8 * self.g.packed + 4096, **self.g.kw()), kind
        self.pixels = ob.decode(self.jls)[1].tobytes()
        assert self.near or self.pixels == self.img.tobytes()


_base = []


@pytest.fixture(scope="module")
def base(torch, l):
    """The batch of the issue: 3 to 4 frames of every kind, the kinds interleaved; every frame coded alone, once."""
    if not _base:
        order = [kind for kind, (_, _, _, count) in KINDS.items() for _ in range(count)]
        order = [order[i] for i in np.random.default_rng(5).permutation(len(order))]
        _base.extend(Frame(torch, l, kind, 300 + f) for f, kind in enumerate(order))
        where = {}
        for f, x in enumerate(_base):
            where.setdefault(x.kind, []).append(f)
        assert any(max(v) - min(v) >= len(v) for v in where.values())  # (a kind whose frames are not neighbours)
    return _base


def encode(torch, frames, *, alignment=1, capacity=None, room=None, strides=None, max_stream_bytes=None):
    """encode_batch_ragged of a list of Frame-likes (tensor, params) into a canary buffer: (PackedBatch, the buffer on the host)."""
    dst = canary_buffer(torch, room if room is not None else sum(len(x.jls) + alignment for x in frames) + 64)
    got = batch.encode_batch_ragged([x.tensor for x in frames], [x.params for x in frames], dst, alignment=alignment, capacity=capacity,
                                    strides=strides, max_stream_bytes=max_stream_bytes)
    return got, dst.cpu().numpy()


def check_blob(host, got, streams, alignment, end_canary=True):
    sizes = [len(s) for s in streams]
    want = rule_offsets(sizes, alignment)
    assert got.sizes.tolist() == sizes
    assert got.offsets.tolist() == want.tolist()
    for f, s in enumerate(streams):
        o = int(want[f])
        assert host[o:o + len(s)].tobytes() == s, f
        assert not host[o + len(s):int(want[f + 1])].any(), f  # the gaps are zero
    if end_canary:
        assert (host[int(want[-1]):] == CANARY).all()


# ---- 1, 2: the mixed batch equals the existing calls, whatever the windows -------------------------------------------------------

@pytest.mark.parametrize("alignment", [1, 2, 16])
def test_mixed_encode_equals_the_packed_call_on_each_frame(torch, base, alignment):
    got, host = encode(torch, base, alignment=alignment)
    assert (got.errcs == 0).all()
    check_blob(host, got, [x.jls for x in base], alignment)


def test_windows_do_not_change_the_result(torch, base, knobs):
    want, want_host = encode(torch, base, alignment=2)
    for window in (1, 2, 3, 5):
        knobs.set("PACK_PASS_FRAMES", window)
        got, host = encode(torch, base, alignment=2)
        assert got.offsets.tolist() == want.offsets.tolist() and got.sizes.tolist() == want.sizes.tolist(), window
        assert got.errcs.tolist() == want.errcs.tolist() and (host == want_host).all(), window
    knobs.clear("PACK_PASS_FRAMES")
    got, host = encode(torch, base, alignment=2)
    assert (host == want_host).all()


# ---- 3: failures stay local --------------------------------------------------------------------------------------------------------

class Plain:
    def __init__(self, tensor, params, jls=b""):
        self.tensor, self.params, self.jls = tensor, params, jls


def test_failures_stay_local(torch, l, base, knobs):
    noise = synth.frame_numpy(64, 64, seed=9, kind="noise")
    rgb = strided.mixed(Geometry(31, 6, comps=3, ilv=2), 77)
    g64, grgb = Geometry(64, 64), Geometry(31, 6, comps=3, ilv=2)
    bits1 = strided.codec_params(g64)
    bits1.frame_info.bits_per_sample = 1
    hp1_near = strided.codec_params(grgb, near=2, ct=1)
    bad = {  # position -> (frame, stride, max_stream_bytes, the code)
        3: (Plain(to_device(torch, noise), strided.codec_params(g64)), 0, 600, DESTINATION_TOO_SMALL),
        11: (Plain(to_device(torch, noise), bits1), 0, 0, INVALID_ARGUMENT_BITS),
        12: (Plain(to_device(torch, rgb), hp1_near), 0, 0, INVALID_ARGUMENT_COLOR_TRANSFORMATION),
        20: (Plain(to_device(torch, noise), strided.codec_params(g64)), 63, 0, INVALID_ARGUMENT_STRIDE),
    }
    frames, strides, limits = list(base), [0] * len(base), [0] * len(base)
    for at in sorted(bad):
        frames.insert(at, bad[at][0])
        strides.insert(at, bad[at][1])
        limits.insert(at, bad[at][2])
    for at, (x, stride, limit, code) in bad.items():  # what the packed call says about the frame alone: the same code
        rc, errc, jls = packed_alone(torch, l, x.params, x.tensor.data_ptr(), stride, limit)
        assert (rc or errc) == code and jls == b"", at
    for window in (None, 3):
        if window:
            knobs.set("PACK_PASS_FRAMES", window)
        got, host = encode(torch, frames, alignment=2, strides=strides, max_stream_bytes=limits)
        for at, (_, _, _, code) in bad.items():
            assert got.errcs[at] == code and got.sizes[at] == 0 and got.offsets[at + 1] == got.offsets[at], at
        assert (np.delete(got.errcs, sorted(bad)) == 0).all()
        check_blob(host, got, [x.jls for x in frames], 2)  # (the others' bytes are those of test 1; a failed frame takes no room)


# ---- 4: the capacity, in the caller's order ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("window", [None, 3, 7])
def test_the_capacity_rule_follows_the_callers_order(torch, base, knobs, window):
    kinds = [x.kind for x in base]
    k = next(f for f in range(8, len(base)) if kinds[f] in kinds[:f] and kinds[f] in kinds[f + 1:])
    if window:  # (a window that holds k with an earlier and a later frame of its group, and windows that do not)
        knobs.set("PACK_PASS_FRAMES", window)
    full = rule_offsets([len(x.jls) for x in base], 16)
    capacity = int(full[k]) + len(base[k].jls) - 1
    got, host = encode(torch, base, alignment=16, capacity=capacity, room=int(full[-1]) + 100)
    assert (got.errcs[:k] == 0).all() and got.sizes[:k].tolist() == [len(x.jls) for x in base[:k]]
    assert got.offsets[:k + 1].tolist() == full[:k + 1].tolist()
    assert (got.errcs[k:] == DESTINATION_TOO_SMALL).all() and (got.sizes[k:] == 0).all() and (got.offsets[k:] == full[k]).all()
    for f in range(k):
        o = int(full[f])
        assert host[o:o + len(base[f].jls)].tobytes() == base[f].jls, f
        assert not host[o + len(base[f].jls):int(full[f + 1])].any()
    assert (host[int(full[k]):] == CANARY).all()  # nothing of them is written, nothing at or beyond the capacity


# ---- 5: sources anywhere -------------------------------------------------------------------------------------------------------------

def test_sources_anywhere(torch, base):
    frames, strides, want = [], [], []
    # padded rows at odd bases, every frame in an allocation of its own
    cases = [(Geometry(150, 7), 1, "p1"), (Geometry(150, 7), 8, "r16p16"), (Geometry(33, 17, bits=12), 2, "p1"), (Geometry(33, 17, bits=12), 1, "r16p16"),
             (Geometry(40, 9, comps=3, ilv=0), 2, "r16p16"), (Geometry(40, 9, comps=3, ilv=0), 1, "p1"), (Geometry(31, 6, comps=3, ilv=2), 8, "p1")]
    for n, (g, at, cls) in enumerate(cases):
        img = strided.mixed(g, 500 + n)
        lay = strided.layout(g, cls, at, 1, pitch="tight", tight=True)
        arena = torch.from_numpy(lay.pad([img])).cuda()
        assert arena.data_ptr() % 16 == 0 and lay.first % 16 == at
        frames.append(Plain(arena[lay.first:], strided.codec_params(g)))
        strides.append(lay.stride)
        want.append(ob.encode(img, destination_size=8 * g.packed + 4096, **g.kw()))
    # one tensor named twice
    for _ in range(2):
        frames.append(Plain(base[0].tensor, base[0].params))
        strides.append(0)
        want.append(base[0].jls)
    # the tiles of a 64 x 64 grid over one 200 x 100 image, the image's row length as their stride
    image = strided.mixed(Geometry(200, 100), 900)
    d_image = torch.from_numpy(image).cuda()
    shapes = set()
    for y in range(0, 100, 64):
        for x in range(0, 200, 64):
            w, h = min(64, 200 - x), min(64, 100 - y)
            shapes.add((w, h))
            frames.append(Plain(d_image[y:y + h, x:x + w], strided.codec_params(Geometry(w, h))))
            strides.append(200)
            want.append(ob.encode(np.ascontiguousarray(image[y:y + h, x:x + w]), width=w, height=h))
    assert shapes == {(64, 64), (8, 64), (64, 36), (8, 36)}
    for x, s in zip(frames, want):
        x.jls = s
    got, host = encode(torch, frames, strides=strides)
    assert (got.errcs == 0).all()
    check_blob(host, got, want, 1)
    # the binding reads a view's row stride from the view itself
    tiles = frames[-8:]
    again, host = encode(torch, tiles)
    check_blob(host, again, want[-8:], 1)


# ---- 6: the probe --------------------------------------------------------------------------------------------------------------------

def part1_header(lib, jls):
    """(errc of set_source_buffer + read_header, get_destination_size(stride 0)) of a fresh part-1 decoder."""
    try:
        dec, keep = lib._open(jls)
    except capi.JpegLSError as e:
        return e.errc, 0
    try:
        n = C.c_size_t()
        assert lib.lib.charls_jpegls_decoder_get_destination_size(dec, 0, C.byref(n)) == 0
        return 0, n.value
    finally:
        lib.lib.charls_jpegls_decoder_destroy(dec)


def blob_of(torch, streams, lead=3):
    """The streams back to back behind `lead` bytes, with 16 bytes behind the last one: (device blob, offsets, sizes)."""
    offsets, at = [], lead
    for s in streams:
        offsets.append(at)
        at += len(s)
    host = np.full(at + 16, CANARY, dtype=np.uint8)
    for o, s in zip(offsets, streams):
        host[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return torch.from_numpy(host).cuda(), np.array(offsets, dtype=np.uint64), np.array([len(s) for s in streams], dtype=np.uint64)


def test_probe(torch, base):
    lib = capi.load_product()
    streams = [x.jls for x in base]
    streams[5:5] = [base[4].jls[:9], b"not a JPEG-LS stream, whatever else it is", b""]
    bad = (5, 6, 7)
    blob, offsets, sizes = blob_of(torch, streams)
    before = capi.engine_counters(lib)
    params, frame_bytes, errcs = batch.probe_packed(blob, offsets, sizes)
    assert batch.last_timings() == (0.0, 0.0) and capi.engine_counters(lib) == before  # no decoder ran
    for f, s in enumerate(streams):
        errc, nbytes = part1_header(lib, s)
        assert errcs[f] == errc and frame_bytes[f] == nbytes, f
        assert (errc != 0) == (f in bad)
        if errc:
            assert bytes(params[f]) == bytes(batch.CodecParams())
            continue
        out = canary_buffer(torch, nbytes)
        p, e, _ = batch.decode_batch_packed(blob, offsets[f:f + 1], sizes[f:f + 1], out, frame_pitch=nbytes)
        assert e[0] == 0 and bytes(params[f]) == bytes(p), f


# ---- 7: ragged decode ----------------------------------------------------------------------------------------------------------------

def decode_into_arenas(torch, l, blob, offsets, sizes, lays, capacities):
    """charls_amd_decode_batch_device_ragged, frame f into a canary arena of its own laid out by lays[f]: (params, errcs, arenas on the host)."""
    n = len(lays)
    arenas = [torch.full((lay.size,), CANARY, dtype=torch.uint8, device="cuda:0") for lay in lays]
    dests = (batch.FrameDest * n)(*[batch.FrameDest(a.data_ptr() + lay.first, int(c), 0 if lay.stride == lay.g.row else lay.stride, 0)
                                    for a, lay, c in zip(arenas, lays, capacities)])
    params = (batch.CodecParams * n)()
    errcs = np.full(n, -1, dtype=np.int32)
    rc = l.charls_amd_decode_batch_device_ragged(n, blob.data_ptr(), offsets.ctypes.data_as(u64p), sizes.ctypes.data_as(u64p), dests, params,
                                                 errcs.ctypes.data_as(i32p), None)
    assert rc == 0
    return params, errcs, [a.cpu().numpy() for a in arenas]


def slot_pixels(torch, blob, offsets, sizes, nbytes):
    """What charls_amd_decode_batch_device_packed makes of the streams, each frame in a canary-filled row of nbytes: (rows, params of frame 0, errcs)."""
    out = torch.full((len(sizes), nbytes), CANARY, dtype=torch.uint8, device="cuda:0")
    p, errcs, _ = batch.decode_batch_packed(blob, offsets, sizes, out)
    return out.cpu().numpy(), p, errcs


def test_ragged_decode_into_arenas_of_the_probed_size(torch, l, base):
    blob, offsets, sizes = blob_of(torch, [x.jls for x in base])
    _, frame_bytes, errcs = batch.probe_packed(blob, offsets, sizes)
    assert (errcs == 0).all() and frame_bytes.tolist() == [x.g.packed for x in base]
    lays = [strided.Layout(x.g, x.g.row, x.g.packed, 0, 1, tight=True) for x in base]
    params, errcs, arenas = decode_into_arenas(torch, l, blob, offsets, sizes, lays, frame_bytes)
    assert (errcs == 0).all()
    rows, _, _ = slot_pixels(torch, blob, offsets, sizes, max(x.g.packed for x in base))
    for f, x in enumerate(base):
        assert rows[f, :x.g.packed].tobytes() == x.pixels
        lays[f].check(arenas[f], [x.pixels])  # the slot decoder's pixels, and every other byte of the arena is the canary
        assert bytes(params[f]) == bytes(batch.decode_batch_packed(blob, offsets[f:f + 1], sizes[f:f + 1], canary_buffer(torch, x.g.packed),
                                                                   frame_pitch=x.g.packed)[0]), f


def test_ragged_decode_capacities_and_strides(torch, l, base):
    pick = [next(f for f, x in enumerate(base) if x.kind == kind) for kind in ("gray_150x7", "rgb_planar_40x9", "gray12_33x17", "rgb_sample_31x6", "gray_64x64")]
    chosen = [base[f] for f in pick]
    blob, offsets, sizes = blob_of(torch, [x.jls for x in chosen])
    # the smallest legal capacity with a padded stride (planar: the rows of all planes), at odd bases: accepted, gaps untouched
    lays = [strided.layout(x.g, "r16p16", at, 1, pitch="tight", tight=True) for x, at in zip(chosen, (1, 2, 8, 1, 0))]
    need = [lay.need for lay in lays]
    _, errcs, arenas = decode_into_arenas(torch, l, blob, offsets, sizes, lays, need)
    assert (errcs == 0).all()
    for lay, arena, x in zip(lays, arenas, chosen):
        lay.check(arena, [x.pixels])
    # one byte less for one frame at a time -- for the planar frame also room for two planes of three: that frame alone is
    # invalid_argument_size and nothing of it is written
    for bad, capacity in [(0, need[0] - 1), (1, need[1] - 1), (1, lays[1].stride * 2 * chosen[1].g.height), (3, need[3] - 1), (2, 0)]:
        capacities = list(need)
        capacities[bad] = capacity
        params, errcs, arenas = decode_into_arenas(torch, l, blob, offsets, sizes, lays, capacities)
        assert errcs.tolist() == [INVALID_ARGUMENT_SIZE if f == bad else 0 for f in range(len(chosen))], (bad, capacity, errcs)
        assert bytes(params[bad]) == bytes(batch.CodecParams())
        for f, (lay, arena, x) in enumerate(zip(lays, arenas, chosen)):
            if f == bad:
                assert (arena == CANARY).all()
            else:
                lay.check(arena, [x.pixels])
    # a stride one below the row
    short = strided.Layout.__new__(strided.Layout)
    short.__dict__.update(lays[3].__dict__)
    short.stride = chosen[3].g.row - 1
    _, errcs, arenas = decode_into_arenas(torch, l, blob, offsets, sizes, lays[:3] + [short] + lays[4:], need)
    assert errcs.tolist() == [0, 0, 0, INVALID_ARGUMENT_STRIDE, 0] and (arenas[3] == CANARY).all()
    lays[4].check(arenas[4], [chosen[4].pixels])


def entropy_start(jls):
    at = jls.rfind(b"\xff\xda")
    return at + 2 + int.from_bytes(jls[at + 2:at + 4], "big")


@pytest.mark.parametrize("damage", ["truncated", "flipped"])
def test_ragged_decode_of_damaged_streams(torch, l, base, damage):
    pick = [next(f for f, x in enumerate(base) if x.kind == kind) for kind in ("gray_64x64", "rgb_planar_40x9", "gray12_33x17", "gray_150x7")]
    chosen = [base[f] for f in pick]
    nbytes = max(x.g.packed for x in chosen)
    for bad in (0, 1, 2):
        streams, declared = [x.jls for x in chosen], [len(x.jls) for x in chosen]
        at = entropy_start(streams[bad]) + (len(streams[bad]) - entropy_start(streams[bad])) // 2
        if damage == "truncated":
            declared[bad] = at
        else:
            raw = bytearray(streams[bad])
            raw[at] ^= 0x5A
            streams[bad] = bytes(raw)
        blob, offsets, _ = blob_of(torch, streams)
        sizes = np.array(declared, dtype=np.uint64)
        rows, _, want = slot_pixels(torch, blob, offsets, sizes, nbytes)
        outs = [canary_buffer(torch, x.g.packed) for x in chosen]
        _, errcs, _ = batch.decode_batch_ragged(blob, offsets, sizes, outs)
        assert errcs.tolist() == want.tolist(), (bad, errcs, want)
        assert (np.delete(errcs, bad) == 0).all() and (damage == "flipped" or errcs[bad] != 0)
        for f, x in enumerate(chosen):  # (the damaged frame too: written where, and only where, the packed decoder writes it)
            assert outs[f].cpu().numpy().tobytes() == rows[f, :x.g.packed].tobytes(), (bad, f)


# ---- 8: round trips --------------------------------------------------------------------------------------------------------------------

def test_probe_allocate_decode_of_the_ragged_encoders_blob(torch, base):
    got, _ = encode(torch, base, alignment=16)
    params, frame_bytes, errcs = batch.probe_packed(got.packed, got.offsets, got.sizes)
    assert (errcs == 0).all()
    for f, x in enumerate(base):
        fi = params[f].frame_info
        assert (fi.width, fi.height, fi.bits_per_sample, fi.component_count) == (x.g.width, x.g.height, x.g.bits, x.g.comps)
        assert (params[f].near_lossless, params[f].interleave_mode, params[f].restart_interval) == (x.near, x.g.ilv, x.restart)
    outs = [torch.empty(int(n), dtype=torch.uint8, device="cuda:0") for n in frame_bytes]  # separate allocations of the probed sizes
    _, errcs, _ = batch.decode_batch_ragged(got.packed, got.offsets, got.sizes, outs)
    assert (errcs == 0).all()
    for f, x in enumerate(base):
        assert outs[f].cpu().numpy().tobytes() == x.pixels, f


def test_dicom_shaped_study_of_two_series(torch):
    """The even-size encoding option with offset_alignment = 2 over two series of different geometry: every offset and every size
    is even, and probe, allocate, decode gives the frames back."""
    series = [(Geometry(64, 20, bits=16), 3), (Geometry(33, 17), 4)]
    frames = []
    for g, count in series:
        for n in range(count):
            img = strided.mixed(g, 40 + len(frames))
            p = strided.codec_params(g)
            p.encoding_options = 1
            frames.append((img, Plain(to_device(torch, img), p)))
    dst = canary_buffer(torch, sum(2 * img.nbytes + 2048 for img, _ in frames))
    got = batch.encode_batch_ragged([x.tensor for _, x in frames], [x.params for _, x in frames], dst, alignment=2)
    assert (got.errcs == 0).all() and not (got.offsets % 2).any() and not (got.sizes % 2).any()
    assert got.offsets.tolist() == rule_offsets(got.sizes, 2).tolist()
    _, frame_bytes, errcs = batch.probe_packed(dst, got.offsets, got.sizes)
    assert (errcs == 0).all() and frame_bytes.tolist() == [img.nbytes for img, _ in frames]
    outs = [torch.empty_like(x.tensor) for _, x in frames]
    _, errcs, _ = batch.decode_batch_ragged(dst, got.offsets, got.sizes, outs)
    assert (errcs == 0).all() and all(torch.equal(o, x.tensor) for o, (_, x) in zip(outs, frames))


# ---- 9: work areas -----------------------------------------------------------------------------------------------------------------------

def test_the_staging_is_a_work_area(torch, base, knobs):
    """Near-lossless and interleaved frames (off the tile pipeline, whose arena would dwarf the staging): the staging is counted
    after the call, shrinks with the window, is gone after charls_amd_release_work_areas; a workspace limit below one slot is
    not_enough_memory."""
    frames = [x for x in base if x.kind in ("near2_70x5", "rgb_sample_31x6")]
    slots = [batch.estimated_destination_size(x.g.width, x.g.height, x.g.bits, x.g.comps) for x in frames]
    batch.release_work_areas()
    assert batch.work_area_bytes() == 0
    got, host = encode(torch, frames)
    check_blob(host, got, [x.jls for x in frames], 1)
    whole = batch.work_area_bytes()
    assert whole >= sum(slots)
    batch.release_work_areas()
    assert batch.work_area_bytes() == 0
    # windows of two frames: the staging holds two slots (each with up to 512 bytes for its stretch's alignment), whatever else
    # the coder keeps is what it kept before
    knobs.set("PACK_PASS_FRAMES", 2)
    got, host = encode(torch, frames)
    assert 2 * min(slots) <= batch.work_area_bytes() <= whole - (sum(slots) - 2 * max(slots) - 1024)
    batch.release_work_areas()
    try:
        batch.set_workspace_limit(min(slots) - 1)
        with pytest.raises(capi.JpegLSError) as e:
            encode(torch, frames)
        assert e.value.errc == NOT_ENOUGH_MEMORY
    finally:
        batch.set_workspace_limit(0)
        batch.release_work_areas()


# ---- 10: the slot encoder behind its new door ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["gray_64x64", "rgb_planar_40x9", "near2_70x5"])
def test_a_uniform_batch_is_what_it_was(torch, kind):
    """charls_amd_encode_batch_device -- whose body now takes a pointer per frame -- still gives the oracle's streams, slots too small
    for a planar frame's scans included (the frames that are coded again, on the pointer form); the ragged call over the same frames
    gives the same bytes."""
    g, near, _, _ = KINDS[kind]
    imgs = [strided.mixed(g, 700 + f) for f in range(6)]
    want = [ob.encode(img, near_lossless=near, destination_size=8 * g.packed + 4096, **g.kw()) for img in imgs]
    frames = to_device(torch, np.stack(imgs))
    kw = dict(bits_per_sample=g.bits, component_count=g.comps, interleave_mode=g.ilv, near_lossless=near)
    for pitch in (4096, (min(len(s) for s in want) + max(len(s) for s in want)) // 2):
        slots = torch.zeros((6, pitch), dtype=torch.uint8, device="cuda:0")
        enc = batch.encode_batch(frames, streams=slots, **kw)
        host = slots.cpu().numpy()
        for f, s in enumerate(want):
            if len(s) > pitch:
                assert enc.errcs[f] == DESTINATION_TOO_SMALL and enc.sizes[f] == 0, (pitch, f)
            elif enc.errcs[f] == 0 or len(s) + 8 <= pitch:  # (a scan that ends within a few bytes of its destination: part 1 may refuse it)
                assert enc.errcs[f] == 0 and host[f, :int(enc.sizes[f])].tobytes() == s, (pitch, f)
            else:
                assert enc.errcs[f] == DESTINATION_TOO_SMALL, (pitch, f)
    got, host = encode(torch, [Plain(frames[f], strided.codec_params(g, near=near), want[f]) for f in range(6)])
    assert (got.errcs == 0).all()
    check_blob(host, got, want, 1)
