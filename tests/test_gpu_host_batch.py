"""The batch API on host memory (charls_amd.h part 2i): one call takes host pointers and gives host bytes.  Its contract is
stated against the device calls of part 2e, so every test compares with them on device copies of the same data (and with the
oracle's streams and pixels): offsets, sizes, bytes, gaps, errcs, params and pixels, whatever the windows, the lanes and the
kind of host memory.  Every buffer a call writes is filled with a canary first.  All frames are tiny.  GPU only."""
import mmap
import threading

import numpy as np
import pytest

import corners
import oracle_bind as ob
import strided
from charls_amd import batch, capi
from strided import CANARY, GUARD, Geometry

pytestmark = pytest.mark.gpu

NOT_ENOUGH_MEMORY, DESTINATION_TOO_SMALL = 1, 3
INVALID_ARGUMENT_BITS, INVALID_ARGUMENT_SIZE, INVALID_ARGUMENT_STRIDE = 104, 110, 111
KINDS_OF_MEMORY = ("pageable", "torch_pinned", "host_alloc", "registered")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def lib():
    return capi.load_product()


def rule_offsets(sizes, alignment):
    out = [0]
    for s in sizes:
        out.append(-(-(out[-1] + int(s)) // alignment) * alignment)
    return out


class Frame:
    """A packed frame in the user's layout with its parameters; the oracle's pixels of its stream (the product's own part-1
    encoder writes the stream where the frame has restart markers, which the reference's encoder cannot write)."""

    def __init__(self, lib, name, g, img, *, near=0, ct=0, preset=None, restart=0, options=0):
        self.name, self.g, self.img, self.near, self.restart = name, g, np.ascontiguousarray(img), near, restart
        assert self.img.nbytes == g.packed
        self.params = strided.codec_params(g, near=near, ct=ct, preset=preset, restart=restart)
        self.params.encoding_options = options
        kw = dict(near_lossless=near, color_transformation=ct, preset=preset, destination_size=8 * g.packed + 4096, encoding_options=options, **g.kw())
        self.jls = lib.encode(self.img, restart_interval=restart, **kw) if restart else ob.encode(self.img, **kw)
        self.pixels = ob.decode(self.jls)[1].tobytes()
        assert near or self.pixels == self.img.tobytes()

    def device(self, torch):
        return torch.from_numpy(self.img.view(np.int16) if self.img.dtype == np.uint16 else self.img).cuda()


def corner_frame(lib, name):
    c = corners.CORPUS[name]
    return Frame(lib, name, Geometry(c.width, c.height, c.bits, c.comps, c.ilv), c.img, near=c.near, ct=c.ct, preset=c.preset)


_mixed = []


@pytest.fixture(scope="module")
def mixed(lib):
    """One frame of every kind of the issue, made once."""
    if not _mixed:
        def plain(name, g, seed, **kw):
            return Frame(lib, name, g, strided.mixed(g, seed), **kw)
        _mixed.extend([
            plain("gray8", Geometry(64, 33), 1), plain("gray12", Geometry(33, 17, bits=12), 2), plain("gray16", Geometry(40, 21, bits=16), 3),
            plain("rgb_planar", Geometry(40, 9, comps=3, ilv=0), 4), plain("rgb_line", Geometry(31, 6, comps=3, ilv=1), 5),
            plain("rgb_sample", Geometry(31, 6, comps=3, ilv=2), 6), plain("hp1", Geometry(31, 6, comps=3, ilv=2), 7, ct=1),
            plain("near2", Geometry(70, 5), 8, near=2), plain("thresholds", Geometry(37, 11), 9, preset=(255, 4, 8, 20, 32)),
            plain("restart2", Geometry(50, 6), 10, restart=2), plain("one", Geometry(1, 1), 11), plain("column", Geometry(1, 37), 12),
            corner_frame(lib, "noise_8_reset3"), corner_frame(lib, "line3_16_hp1"), corner_frame(lib, "escape_run_12"),
        ])
    return _mixed


def canary(nbytes):
    return np.full(nbytes, CANARY, dtype=np.uint8)


def device_encode(torch, frames, *, alignment=1, capacity=None, room=None, strides=None, max_stream_bytes=None, tensors=None, params=None):
    """charls_amd_encode_batch_device_ragged on device copies into a canary buffer: (PackedBatch, the buffer on the host)."""
    dst = torch.full((room,), CANARY, dtype=torch.uint8, device="cuda:0")
    got = batch.encode_batch_ragged(tensors or [x.device(torch) for x in frames], params or [x.params for x in frames], dst, alignment=alignment,
                                    capacity=capacity, strides=strides, max_stream_bytes=max_stream_bytes)
    return got, dst.cpu().numpy()


def host_encode(frames, *, alignment=1, capacity=None, room=None, strides=None, max_stream_bytes=None, arrays=None, params=None, dst=None):
    dst = canary(room) if dst is None else dst
    got = batch.encode_batch_host_ragged(arrays or [x.img for x in frames], params or [x.params for x in frames], dst, alignment=alignment,
                                         capacity=capacity, strides=strides, max_stream_bytes=max_stream_bytes)
    return got, dst


def same_batch(got, host, want, want_host):
    assert got.offsets.tolist() == want.offsets.tolist()
    assert got.sizes.tolist() == want.sizes.tolist()
    assert got.errcs.tolist() == want.errcs.tolist()
    assert host.tobytes() == want_host.tobytes()  # streams, zeroed gaps, and the canary everywhere else


def room_for(frames, alignment):
    return sum(len(x.jls) + alignment for x in frames) + 64


def blob_of(streams, lead=3):
    """The streams back to back behind `lead` bytes: (host blob, offsets, sizes)."""
    offsets, at = [], lead
    for s in streams:
        offsets.append(at)
        at += len(s)
    host = canary(at + 16)
    for o, s in zip(offsets, streams):
        host[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return host, np.array(offsets, dtype=np.uint64), np.array([len(s) for s in streams], dtype=np.uint64)


def device_decode(torch, blob, offsets, sizes, nbytes, **kw):
    outs = [torch.full((n,), CANARY, dtype=torch.uint8, device="cuda:0") for n in nbytes]
    params, errcs, _ = batch.decode_batch_ragged(torch.from_numpy(blob).cuda(), offsets, sizes, outs, **kw)
    return params, errcs, [o.cpu().numpy() for o in outs]


def host_decode(blob, offsets, sizes, nbytes, **kw):
    outs = [canary(n) for n in nbytes]
    params, errcs = batch.decode_batch_host_ragged(blob, offsets, sizes, outs, **kw)
    return params, errcs, outs


def same_decode(got, want, failed=()):
    (params, errcs, outs), (want_params, want_errcs, want_outs) = got, want
    assert errcs.tolist() == want_errcs.tolist()
    for f in range(len(outs)):
        assert bytes(params[f]) == bytes(want_params[f]), f
        if f in failed:  # (the host call writes nothing of a frame that fails)
            assert (outs[f] == CANARY).all(), f
        else:
            assert outs[f].tobytes() == want_outs[f].tobytes(), f


# ---- 1: parity with the device calls -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("alignment", [1, 16])
def test_mixed_batch_equals_the_device_calls_and_the_oracle(torch, mixed, alignment):
    room = room_for(mixed, alignment)
    want, want_host = device_encode(torch, mixed, alignment=alignment, room=room)
    got, host = host_encode(mixed, alignment=alignment, room=room)
    same_batch(got, host, want, want_host)
    assert (got.errcs == 0).all() and got.offsets.tolist() == rule_offsets(got.sizes, alignment)
    for f, x in enumerate(mixed):
        o, n = int(got.offsets[f]), int(got.sizes[f])
        assert host[o:o + n].tobytes() == x.jls, x.name  # the oracle's stream (the part-1 encoder's for the restart frame)
        assert not host[o + n:int(got.offsets[f + 1])].any()
    # ---- and back
    nbytes = [x.g.packed for x in mixed]
    want = device_decode(torch, host, got.offsets, got.sizes, nbytes)
    back = host_decode(host, got.offsets, got.sizes, nbytes)
    same_decode(back, want)
    assert (back[1] == 0).all()
    for f, x in enumerate(mixed):
        assert back[2][f].tobytes() == x.pixels, x.name
    params, frame_bytes, errcs = batch.probe_host(host, got.offsets, got.sizes)
    assert (errcs == 0).all() and frame_bytes.tolist() == nbytes and all(bytes(params[f]) == bytes(back[0][f]) for f in range(len(mixed)))


# ---- 2: windows and lanes ------------------------------------------------------------------------------------------------------

def test_windows_and_lanes_do_not_change_the_result(torch, mixed, knobs):
    frames = mixed[:7]
    room = room_for(frames, 16)
    want, want_host = device_encode(torch, frames, alignment=16, room=room)
    nbytes = [x.g.packed for x in frames]
    want_back = device_decode(torch, want_host, want.offsets, want.sizes, nbytes)
    # a capacity that ends inside the second window of two frames: frame 3, one byte short
    capacity = int(want.offsets[3] + want.sizes[3]) - 1
    short, short_host = device_encode(torch, frames, alignment=16, room=room, capacity=capacity)
    assert short.errcs.tolist() == [0] * 3 + [DESTINATION_TOO_SMALL] * 4 and (short.offsets[3:] == want.offsets[3]).all()
    for window in (1, 2, 3, 7):
        for lanes in (1, 2, 3):
            knobs.set("HOST_WINDOW_FRAMES", window)
            knobs.set("HOST_LANES", lanes)
            before = batch.host_counters()
            got, host = host_encode(frames, alignment=16, room=room)
            same_batch(got, host, want, want_host)
            after = batch.host_counters()
            assert after[0] - before[0] == 1 and after[1] - before[1] == -(-7 // window), (window, lanes)
            same_decode(host_decode(host, got.offsets, got.sizes, nbytes), want_back)
            assert batch.host_counters()[1] - after[1] == -(-7 // window), (window, lanes)
            got, host = host_encode(frames, alignment=16, room=room, capacity=capacity)
            same_batch(got, host, short, short_host)


# ---- 3: memory kinds and placement ---------------------------------------------------------------------------------------------

class Memory:
    """nbytes of host memory of one kind, its first byte 64-byte aligned."""

    def __init__(self, torch, kind, nbytes):
        self.kind, self.raw = kind, None
        if kind == "torch_pinned":
            self.keep = torch.empty(nbytes + 64, dtype=torch.uint8, pin_memory=True)
            raw = self.keep.numpy()
        elif kind == "host_alloc":
            raw = batch.host_alloc(nbytes + 64)
        elif kind == "registered":
            # A mapping of its own, whole pages: registering pins pages, and a page of the heap is shared with whatever else
            # lives on it -- arrays registered one by one would pin, and unpin, each other's pages.
            self.keep = mmap.mmap(-1, -(-(nbytes + 64) // mmap.PAGESIZE) * mmap.PAGESIZE)
            raw = np.frombuffer(self.keep, dtype=np.uint8)
            batch.host_register(raw)
            self.raw = raw
        else:
            raw = np.empty(nbytes + 64, dtype=np.uint8)
        skew = (-raw.ctypes.data) % 64
        self.bytes = raw[skew:skew + nbytes]

    def release(self):
        if self.raw is not None:
            batch.host_unregister(self.raw)
            self.raw = None


def placement_round_trip(torch, frames, kinds):
    """Encode from padded rows at odd bases in arenas of the given kinds into the smallest legal capacity at an odd address,
    decode back into such arenas: (pageable bytes that went up and down on encode, on decode)."""
    held = []
    try:
        lays, arenas, pristine = [], [], []
        for f, x in enumerate(frames):
            lay = strided.layout(x.g, ("p1", "r16p16", "p13")[f % 3], (1, 3)[f % 2], 1, pitch="tight", tight=True)
            padded = lay.pad([x.img])
            m = Memory(torch, kinds[f % len(kinds)], lay.size)
            held.append(m)
            m.bytes[:] = padded
            assert m.bytes.ctypes.data % 16 == 0 and (m.bytes.ctypes.data + lay.first) % 2 == 1  # (16-bit rows at odd addresses too)
            lays.append(lay)
            arenas.append(m.bytes)
            pristine.append(padded.copy())
        total = sum(len(x.jls) for x in frames)
        out = Memory(torch, kinds[0], total + 2 * GUARD)
        held.append(out)
        out.bytes[:] = CANARY
        before = batch.host_counters()
        got = batch.encode_batch_host_ragged([a[lay.first:] for a, lay in zip(arenas, lays)], [x.params for x in frames], out.bytes[GUARD + 1:],
                                             strides=[lay.stride for lay in lays], capacity=total)
        staged_encode = batch.host_counters()[4] - before[4]
        assert (got.errcs == 0).all() and int(got.offsets[-1]) == total
        assert out.bytes[GUARD + 1:GUARD + 1 + total].tobytes() == b"".join(x.jls for x in frames)
        assert (out.bytes[:GUARD + 1] == CANARY).all() and (out.bytes[GUARD + 1 + total:] == CANARY).all()
        for a, p in zip(arenas, pristine):
            assert a.tobytes() == p.tobytes()  # encode never writes to a source
        # ---- decode into fresh canary arenas of the same kinds and layouts, each of the smallest legal capacity
        for a in arenas:
            a[:] = CANARY
        before = batch.host_counters()
        _, errcs = batch.decode_batch_host_ragged(out.bytes[GUARD + 1:], got.offsets, got.sizes, [a[lay.first:] for a, lay in zip(arenas, lays)],
                                                  strides=[lay.stride for lay in lays], capacities=[lay.need for lay in lays])
        staged_decode = batch.host_counters()[4] - before[4]
        assert (errcs == 0).all()
        for a, lay, x in zip(arenas, lays, frames):
            lay.check(a, [x.pixels])  # the rows, and stride padding, guard bands and everything else still the canary
        return staged_encode, staged_decode
    finally:
        for m in held:
            m.release()


@pytest.mark.parametrize("kind", KINDS_OF_MEMORY)
def test_memory_kinds_padded_strides_odd_bases(torch, mixed, kind):
    frames = [x for x in mixed if x.name in ("gray8", "gray16", "rgb_planar", "rgb_sample", "near2", "column", "line3_16_hp1")]
    staged_encode, staged_decode = placement_round_trip(torch, frames, [kind])
    pixels, streams = sum(x.g.packed for x in frames), sum(len(x.jls) for x in frames)
    assert (staged_encode, staged_decode) == ((pixels + streams, pixels + streams) if kind == "pageable" else (0, 0))


def test_memory_kinds_mixed_within_one_call(torch, mixed, knobs):
    knobs.set("HOST_STAGE_BYTES", 1024)  # (pageable frames longer than a half of the staging buffer: they go in pieces)
    frames = mixed[:8]
    staged_encode, staged_decode = placement_round_trip(torch, frames, list(KINDS_OF_MEMORY))
    pageable = sum(x.g.packed for f, x in enumerate(frames) if KINDS_OF_MEMORY[f % 4] == "pageable")
    assert staged_encode == pageable + sum(len(x.jls) for x in frames)  # (the streams came down into pageable memory)
    assert staged_decode == pageable + sum(len(x.jls) for x in frames)


# ---- 4: local failures -----------------------------------------------------------------------------------------------------------

def test_encode_failures_stay_local(torch, mixed):
    frames = mixed[:6]
    params = [x.params for x in frames]
    bits1 = strided.codec_params(frames[2].g)
    bits1.frame_info.bits_per_sample = 1
    params[2] = bits1                                  # a parameter set the encoder refuses
    strides = [0, 0, 0, 0, frames[4].g.row - 1, 0]     # a stride below the row
    limits = [0, 40, 0, 0, 0, 0]                       # a slot too small for the stream
    room = room_for(frames, 2)
    want, want_host = device_encode(torch, frames, alignment=2, room=room, params=params, strides=strides, max_stream_bytes=limits)
    assert want.errcs.tolist() == [0, DESTINATION_TOO_SMALL, INVALID_ARGUMENT_BITS, 0, INVALID_ARGUMENT_STRIDE, 0]
    got, host = host_encode(frames, alignment=2, room=room, params=params, strides=strides, max_stream_bytes=limits)
    same_batch(got, host, want, want_host)
    for f in (0, 3, 5):
        assert host[int(got.offsets[f]):int(got.offsets[f] + got.sizes[f])].tobytes() == frames[f].jls


def test_decode_failures_stay_local(torch, mixed):
    frames = mixed[:7]
    streams = [x.jls for x in frames]
    raw = bytearray(streams[3])
    at = raw.rfind(b"\xff\xda")
    at += 2 + int.from_bytes(raw[at + 2:at + 4], "big")
    raw[at + (len(raw) - at) // 2] ^= 0x5A             # a damaged stream in the middle
    streams[3] = bytes(raw)
    blob, offsets, sizes = blob_of(streams)
    sizes[0] = len(streams[0]) // 2                    # and a truncated one
    nbytes = [x.g.packed for x in frames]
    capacities = list(nbytes)
    capacities[1] -= 1                                 # a destination one byte short
    strides = [0] * 7
    strides[5] = frames[5].g.row - 1                   # a stride below the row
    want = device_decode(torch, blob, offsets, sizes, nbytes, strides=strides, capacities=capacities)
    assert want[1][1] == INVALID_ARGUMENT_SIZE and want[1][5] == INVALID_ARGUMENT_STRIDE and want[1][0] != 0 and want[1][3] != 0
    assert [want[1][f] for f in (2, 4, 6)] == [0, 0, 0]
    got = host_decode(blob, offsets, sizes, nbytes, strides=strides, capacities=capacities)
    same_decode(got, want, failed=(0, 1, 3, 5))
    for f in (2, 4, 6):
        assert got[2][f].tobytes() == frames[f].pixels


# ---- 5: the uniform wrappers -----------------------------------------------------------------------------------------------------

def test_uniform_wrappers_equal_the_packed_device_calls(torch, lib):
    """The DICOM shape: 16-bit frames with the even-size encoding option and offset_alignment = 2."""
    g = Geometry(64, 20, bits=16)
    imgs = np.stack([strided.mixed(g, 40 + f) for f in range(5)])
    kw = dict(bits_per_sample=16, encoding_options=1, alignment=2)
    room = 5 * (2 * g.packed + 2048)
    d_packed = torch.full((room,), CANARY, dtype=torch.uint8, device="cuda:0")
    want = batch.encode_batch_packed(torch.from_numpy(imgs.view(np.int16)).cuda(), d_packed, **kw)
    packed = canary(room)
    got = batch.encode_batch_host(imgs, packed, **kw)
    same_batch(got, packed, want, d_packed.cpu().numpy())
    assert (got.errcs == 0).all() and not (got.offsets % 2).any() and not (got.sizes % 2).any()
    for f in range(5):
        assert packed[int(got.offsets[f]):int(got.offsets[f] + got.sizes[f])].tobytes() == ob.encode(imgs[f], encoding_options=1, **g.kw())
    d_out = torch.full((5, g.packed + 6), CANARY, dtype=torch.uint8, device="cuda:0")  # (a pitch with room behind every frame)
    want_p, want_errcs, _ = batch.decode_batch_packed(d_packed, got.offsets, got.sizes, d_out)
    out = np.full((5, g.packed + 6), CANARY, dtype=np.uint8)
    p, errcs = batch.decode_batch_host(packed, got.offsets, got.sizes, out)
    assert errcs.tolist() == want_errcs.tolist() == [0] * 5 and bytes(p) == bytes(want_p)
    assert out.tobytes() == d_out.cpu().numpy().tobytes()
    assert out[:, :g.packed].tobytes() == imgs.tobytes()
    # parameters the encoder refuses are the call's error, as the packed device call has it
    with pytest.raises(capi.JpegLSError) as e:
        batch.encode_batch_host(imgs, packed, bits_per_sample=1)
    assert e.value.errc == INVALID_ARGUMENT_BITS


# ---- 6: stream lengths at the end of a window -----------------------------------------------------------------------------------

def test_stream_lengths_that_are_no_multiple_of_16_end_a_window(torch, mixed, knobs):
    """With windows of one frame every stream is the last of its device window: the decoders' whole 16-byte loads behind it stay
    inside the allocation."""
    frames = sorted(mixed, key=lambda x: len(x.jls) % 16)
    assert sum(len(x.jls) % 16 != 0 for x in frames) >= 10 and len({len(x.jls) % 16 for x in frames}) >= 6
    blob, offsets, sizes = blob_of([x.jls for x in frames], lead=0)
    for window in (1, 2):
        knobs.set("HOST_WINDOW_FRAMES", window)
        _, errcs, outs = host_decode(blob, offsets, sizes, [x.g.packed for x in frames])
        assert (errcs == 0).all()
        for out, x in zip(outs, frames):
            assert out.tobytes() == x.pixels, x.name


# ---- 7: the budget -----------------------------------------------------------------------------------------------------------------

def test_the_lanes_stay_within_the_workspace_limit(torch, lib, knobs):
    g = Geometry(64, 40, bits=16)
    frames = [Frame(lib, f"f{f}", g, strided.mixed(g, 60 + f, kind="noise")) for f in range(48)]
    room = room_for(frames, 1)
    want, want_host = host_encode(frames, room=room)
    assert (want.errcs == 0).all() and all(want_host[int(o):int(o + n)].tobytes() == x.jls for o, n, x in zip(want.offsets, want.sizes, frames))
    nbytes = [g.packed] * 48
    limit = 1 << 20  # the frames and their slots alone are 48 * 11.5 KiB: more than half of the limit, which is all the lanes' own buffers get
    try:
        batch.release_work_areas()
        assert batch.host_counters()[5:] == (0, 0)
        batch.set_workspace_limit(limit)
        knobs.set("HOST_WINDOW_FRAMES", 1000)  # (nothing but the limit cuts the windows)
        before = batch.host_counters()
        got, host = host_encode(frames, room=room)
        after = batch.host_counters()
        same_batch(got, host, want, want_host)
        assert after[1] - before[1] >= 2
        assert 0 < after[5] <= limit and after[6] > 0
        _, errcs, outs = host_decode(host, got.offsets, got.sizes, nbytes)
        assert (errcs == 0).all() and all(o.tobytes() == x.pixels for o, x in zip(outs, frames))
        assert batch.host_counters()[1] - after[1] >= 2
        assert 0 < batch.host_counters()[5] <= limit
        batch.release_work_areas()
        assert batch.host_counters()[5:] == (0, 0)
        # a limit that cannot hold the largest single frame
        batch.set_workspace_limit(16 << 10)
        with pytest.raises(capi.JpegLSError) as e:
            host_encode(frames, room=room)
        assert e.value.errc == NOT_ENOUGH_MEMORY
        with pytest.raises(capi.JpegLSError) as e:
            host_decode(host, got.offsets, got.sizes, nbytes)
        assert e.value.errc == NOT_ENOUGH_MEMORY
    finally:
        batch.set_workspace_limit(0)
        batch.release_work_areas()


# ---- 8: threads ------------------------------------------------------------------------------------------------------------------------

def test_four_threads_call_at_once(torch, mixed):
    results, errors = {}, []

    def work(t):
        try:
            frames = mixed[t::4] + mixed[:t + 1]
            got, host = host_encode(frames, alignment=4, room=room_for(frames, 4))
            _, errcs, outs = host_decode(host, got.offsets, got.sizes, [x.g.packed for x in frames])
            results[t] = (frames, got, host, errcs, outs)
        except Exception as e:  # noqa: BLE001 (reported by the main thread)
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors and sorted(results) == [0, 1, 2, 3], errors
    for t, (frames, got, host, errcs, outs) in results.items():
        assert (got.errcs == 0).all() and (errcs == 0).all()
        assert got.offsets.tolist() == rule_offsets([len(x.jls) for x in frames], 4)
        for f, x in enumerate(frames):
            assert host[int(got.offsets[f]):int(got.offsets[f] + got.sizes[f])].tobytes() == x.jls, (t, x.name)
            assert outs[f].tobytes() == x.pixels, (t, x.name)
