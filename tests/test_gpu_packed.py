"""Packed streams in the batch API (charls_amd.h part 2d): the streams of a batch back to back in one device buffer with a
host table of offsets.  The contract of every call is stated against the slot calls of part 2, so every test here compares
with them: pack_streams against numpy slicing of the slots, encode_batch_device_packed against encode_batch_device with
stream_pitch_bytes = max_stream_bytes followed by slicing, decode_batch_device_packed against decode_batch_device on the same
bytes.  Every destination is filled with a canary first: nothing outside what a call owns may change.  GPU only."""
import ctypes as C

import numpy as np
import pytest

import oracle_bind as ob
from charls_amd import batch, capi, synth

pytestmark = pytest.mark.gpu

CANARY = 0xA5
INVALID_ARGUMENT, INVALID_ARGUMENT_SIZE, DESTINATION_TOO_SMALL = 101, 110, 3
FRAMES = 37  # PACK_PASS_FRAMES = 5 makes eight passes of it


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def rule_offsets(sizes, alignment):
    """offsets[0] = 0, offsets[f + 1] = offsets[f] + sizes[f] rounded up to the alignment."""
    out = [0]
    for s in sizes:
        out.append(-(-(out[-1] + int(s)) // alignment) * alignment)
    return np.array(out, dtype=np.uint64)


def canary_buffer(torch, nbytes):
    return torch.full((nbytes,), CANARY, dtype=torch.uint8, device="cuda:0")


def check_blob(host, offsets, sizes, streams, capacity=None):
    """`host` (the packed buffer, numpy): frame f's bytes at offsets[f], zero gaps, the canary from the total (or the capacity,
    where that comes first) on."""
    for f, want in enumerate(streams):
        o, n = int(offsets[f]), int(sizes[f])
        assert n == len(want), (f, n, len(want))
        assert host[o:o + n].tobytes() == want, f
        gap_end = int(offsets[f + 1]) if capacity is None else min(int(offsets[f + 1]), capacity)
        assert not host[o + n:gap_end].any(), f
    end = int(offsets[len(streams)]) if capacity is None else min(int(offsets[len(streams)]), capacity)
    assert (host[end:] == CANARY).all()


# ---- pack_streams on arbitrary bytes ----------------------------------------------------------------------------------------

PACK_SIZES = [0, 1, 3, 5, 2, 15, 16, 17, 4097, 200001, 0, 7]


@pytest.fixture(scope="module")
def random_slots(torch):
    pitch = 200003  # (odd: every slot at another misalignment)
    host = np.random.default_rng(31).integers(0, 256, (len(PACK_SIZES), pitch), dtype=np.uint8)
    return torch.from_numpy(host).cuda(), host


@pytest.mark.parametrize("alignment", [1, 2, 16, 4096])
def test_pack_streams_equals_numpy(torch, random_slots, alignment):
    slots, host = random_slots
    sizes = np.array(PACK_SIZES, dtype=np.uint64)
    want = rule_offsets(sizes, alignment)
    total = int(want[-1])
    dst = canary_buffer(torch, total + 333)
    got = batch.pack_streams(slots, sizes, alignment=alignment, packed=dst, capacity=total)  # a capacity equal to the total
    assert (got.offsets == want).all()
    check_blob(dst.cpu().numpy(), got.offsets, sizes, [host[f, :n].tobytes() for f, n in enumerate(PACK_SIZES)])
    # one byte less: invalid_argument_size, and the destination stays as it is
    dst = canary_buffer(torch, total + 333)
    with pytest.raises(capi.JpegLSError) as e:
        batch.pack_streams(slots, sizes, alignment=alignment, packed=dst, capacity=total - 1)
    assert e.value.errc == INVALID_ARGUMENT_SIZE
    assert (dst == CANARY).all().item()


def test_pack_streams_refuses_a_size_beyond_the_pitch(torch, random_slots):
    slots, _ = random_slots
    sizes = np.array(PACK_SIZES, dtype=np.uint64)
    sizes[3] = slots.shape[1] + 1
    dst = canary_buffer(torch, 1 << 20)
    with pytest.raises(capi.JpegLSError) as e:
        batch.pack_streams(slots, sizes, packed=dst)
    assert e.value.errc == INVALID_ARGUMENT_SIZE and (dst == CANARY).all().item()


# ---- encode_batch_device_packed against encode_batch_device + slicing -------------------------------------------------------

KINDS = ["mixed", "gradient", "noise", "zero", "hard"]  # (differing content: the sizes differ)
ENCODE_CASES = {
    "gray8_33x17": dict(w=33, h=17, bits=8, comps=1, ilv=0, near=0, restart=0),
    "gray16_64x64": dict(w=64, h=64, bits=16, comps=1, ilv=0, near=0, restart=0),
    "rgb_sample_31x9": dict(w=31, h=9, bits=8, comps=3, ilv=2, near=0, restart=0),
    "rgb_planar_20x12": dict(w=20, h=12, bits=8, comps=3, ilv=0, near=0, restart=0),  # (the scan-round path)
    "gray8_near2": dict(w=33, h=17, bits=8, comps=1, ilv=0, near=2, restart=0),
    "gray8_restart4": dict(w=33, h=17, bits=8, comps=1, ilv=0, near=0, restart=4),
}
_slot_reference = {}


def case_frames(torch, c, count=FRAMES):
    imgs = [synth.frame_numpy(c["w"], c["h"], seed=70 + f, bits=c["bits"], components=c["comps"], kind=KINDS[f % len(KINDS)],
                              interleaved=c["ilv"] != 0) for f in range(count)]
    host = np.stack(imgs)
    return torch.from_numpy(host.view(np.int16) if c["bits"] > 8 else host).cuda()


def encode_kw(c, options=0):
    return dict(bits_per_sample=c["bits"], component_count=c["comps"], interleave_mode=c["ilv"], near_lossless=c["near"],
                restart_interval=c["restart"], encoding_options=options)


def slot_reference(torch, name):
    """The case's frames, its slot pitch (part 1's estimated destination size) and what the slot encoder gives with it: computed once."""
    if name not in _slot_reference:
        c = ENCODE_CASES[name]
        frames = case_frames(torch, c)
        pitch = batch.estimated_destination_size(c["w"], c["h"], c["bits"], c["comps"])
        if c["restart"]:
            pitch += 6 + 2 * -(-c["h"] // c["restart"]) * c["comps"]
        slots = torch.zeros((FRAMES, pitch), dtype=torch.uint8, device="cuda:0")
        enc = batch.encode_batch(frames, streams=slots, **encode_kw(c))
        host = slots.cpu().numpy()
        streams = [host[f, :int(enc.sizes[f])].tobytes() for f in range(FRAMES)]
        assert (enc.errcs == 0).all() and len(set(len(s) for s in streams)) > 3
        _slot_reference[name] = (frames, pitch, enc, streams)
    return _slot_reference[name]


@pytest.mark.parametrize("alignment", [1, 2, 16])
@pytest.mark.parametrize("pass_frames", [None, 5])
@pytest.mark.parametrize("name", list(ENCODE_CASES))
def test_packed_encode_equals_slot_encode(torch, knobs, name, pass_frames, alignment):
    c = ENCODE_CASES[name]
    frames, pitch, ref, streams = slot_reference(torch, name)
    if pass_frames:
        knobs.set("PACK_PASS_FRAMES", pass_frames)  # eight passes: the running offset carries across them
    want = rule_offsets(ref.sizes, alignment)
    dst = canary_buffer(torch, int(want[-1]) + 100)
    # (0 = part 1's estimated destination size, which is the reference's pitch; the default passes state it, the short ones leave it to the call)
    got = batch.encode_batch_packed(frames, dst, alignment=alignment, max_stream_bytes=0 if pass_frames else pitch, **encode_kw(c))
    assert (got.errcs == ref.errcs).all() and (got.sizes == ref.sizes).all()
    assert (got.offsets == want).all()
    check_blob(dst.cpu().numpy(), got.offsets, got.sizes, streams)


def test_a_frame_that_fails_takes_no_room(torch, knobs):
    """Flat frames with one frame of full-range noise in the middle and a max_stream_bytes between their sizes: the noise frame
    is destination_too_small exactly as the slot encoder reports it with that pitch, takes no room, and its neighbours are exact."""
    w, h, n, bad = 64, 64, 7, 3
    imgs = [synth.frame_numpy(w, h, seed=5 + f, kind="noise") if f == bad else np.full((h, w), 10 * f, dtype=np.uint8) for f in range(n)]
    flat = max(len(ob.encode(imgs[f], width=w, height=h)) for f in range(n) if f != bad)
    noise = len(ob.encode(imgs[bad], width=w, height=h))
    limit = (flat + noise) // 2
    assert flat < limit < noise
    frames = torch.from_numpy(np.stack(imgs)).cuda()
    slots = torch.zeros((n, limit), dtype=torch.uint8, device="cuda:0")
    ref = batch.encode_batch(frames, streams=slots)
    assert ref.errcs[bad] == DESTINATION_TOO_SMALL and ref.sizes[bad] == 0 and (np.delete(ref.errcs, bad) == 0).all()
    host = slots.cpu().numpy()
    streams = [host[f, :int(ref.sizes[f])].tobytes() for f in range(n)]
    for pass_frames in (None, 2):
        if pass_frames:
            knobs.set("PACK_PASS_FRAMES", pass_frames)
        dst = canary_buffer(torch, n * limit)
        got = batch.encode_batch_packed(frames, dst, alignment=1, max_stream_bytes=limit)
        assert (got.errcs == ref.errcs).all() and (got.sizes == ref.sizes).all()
        assert (got.offsets == rule_offsets(ref.sizes, 1)).all() and got.offsets[bad + 1] == got.offsets[bad]
        check_blob(dst.cpu().numpy(), got.offsets, got.sizes, streams)


@pytest.mark.parametrize("alignment", [1, 16])
@pytest.mark.parametrize("pass_frames", [None, 5])
def test_the_capacity_rule(torch, knobs, pass_frames, alignment):
    """A capacity one byte short of frame k's end: frames before k are exact, frame k and every frame after it are
    destination_too_small with size 0, and every byte from offsets[k] on is still the canary."""
    name, k = "gray8_33x17", 18
    frames, pitch, ref, streams = slot_reference(torch, name)
    full = rule_offsets(ref.sizes, alignment)
    capacity = int(full[k]) + int(ref.sizes[k]) - 1
    if pass_frames:
        knobs.set("PACK_PASS_FRAMES", pass_frames)
    dst = canary_buffer(torch, int(full[-1]) + 100)
    got = batch.encode_batch_packed(frames, dst, alignment=alignment, max_stream_bytes=pitch, capacity=capacity,
                                    **encode_kw(ENCODE_CASES[name]))
    assert (got.errcs[:k] == 0).all() and (got.sizes[:k] == ref.sizes[:k]).all() and (got.offsets[:k + 1] == full[:k + 1]).all()
    assert (got.errcs[k:] == DESTINATION_TOO_SMALL).all() and (got.sizes[k:] == 0).all() and (got.offsets[k:] == full[k]).all()
    host = dst.cpu().numpy()
    for f in range(k):
        assert host[int(full[f]):int(full[f]) + len(streams[f])].tobytes() == streams[f], f
        assert not host[int(full[f]) + len(streams[f]):int(full[f + 1])].any()
    assert (host[int(full[k]):] == CANARY).all()


# ---- decode_batch_device_packed against decode_batch_device on the same streams ---------------------------------------------

def slots_of(torch, streams, sizes=None):
    """The streams in (F, pitch) slots -- what the slot decoder is given -- and their sizes."""
    pitch = (max(len(s) for s in streams) + 255) & ~255
    host = np.zeros((len(streams), pitch), dtype=np.uint8)
    for f, s in enumerate(streams):
        host[f, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    return torch.from_numpy(host).cuda(), np.array([len(s) for s in streams] if sizes is None else sizes, dtype=np.uint64)


def blob_of(torch, streams, lead=1):
    """The streams back to back at alignment 1 behind `lead` bytes (odd starts), with 16 bytes behind the last one."""
    offsets, at = [], lead
    for s in streams:
        offsets.append(at)
        at += len(s)
    host = np.full(at + 16, CANARY, dtype=np.uint8)
    for o, s in zip(offsets, streams):
        host[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return torch.from_numpy(host).cuda(), np.array(offsets, dtype=np.uint64)


def decode_both(torch, streams, sizes, out_shape, dtype, *, order=None, lead=1):
    """Slot decode and packed decode of the same bytes (frame f's declared size sizes[f]; order: the packed call names the
    streams in this order, possibly more than once).  Returns ((pixels, params bytes, errcs) of each) with the slot result
    re-ordered the same way."""
    slots, sz = slots_of(torch, streams, sizes)
    blob, offsets = blob_of(torch, streams, lead)
    order = [int(f) for f in (range(len(streams)) if order is None else order)]
    out_a = torch.zeros((len(streams),) + out_shape, dtype=dtype, device="cuda:0")
    p_a, errcs_a, _ = batch.decode_batch(slots, sz, out_a)
    out_b = torch.zeros((len(order),) + out_shape, dtype=dtype, device="cuda:0")
    p_b, errcs_b, _ = batch.decode_batch_packed(blob, offsets[order], sz[order], out_b)
    return (out_a[order], bytes(p_a), errcs_a[order]), (out_b, bytes(p_b), errcs_b)


def test_packed_decode_of_the_encoders_blob(torch):
    """The packed encoder's own output at alignment 1 (odd starts) decodes to the frames; the same streams in a shuffled order
    and with one stream named twice decode exactly as the slot decoder decodes them."""
    name = "gray8_33x17"
    c = ENCODE_CASES[name]
    frames, pitch, ref, streams = slot_reference(torch, name)
    dst = canary_buffer(torch, int(rule_offsets(ref.sizes, 1)[-1]) + 16)
    enc = batch.encode_batch_packed(frames, dst, alignment=1, **encode_kw(c))
    assert any(int(o) % 2 for o in enc.offsets[:-1])
    out = torch.zeros_like(frames)
    p, errcs, _ = batch.decode_batch_packed(dst, enc.offsets, enc.sizes, out)
    assert (errcs == 0).all() and torch.equal(out, frames)
    assert (p.frame_info.width, p.frame_info.height, p.frame_info.bits_per_sample) == (c["w"], c["h"], c["bits"])
    order = list(np.random.default_rng(41).permutation(FRAMES)) + [7, 7, 0]
    (pix_a, p_a, errcs_a), (pix_b, p_b, errcs_b) = decode_both(torch, streams, None, (c["h"], c["w"]), torch.uint8, order=order)
    assert (errcs_a == 0).all() and (errcs_b == 0).all() and torch.equal(pix_a, pix_b) and torch.equal(pix_b, frames[order])


def mixed_streams():
    """Gray 8-bit, 16-bit, RGB sample-interleaved and planar frames of different sizes, coded by the oracle."""
    made = []
    for i, (w, h, bits, comps, ilv) in enumerate([(33, 17, 8, 1, 0), (64, 20, 16, 1, 0), (31, 9, 8, 3, 2), (20, 12, 8, 3, 0), (50, 11, 8, 1, 0),
                                                  (16, 16, 12, 1, 0), (40, 8, 8, 3, 0), (9, 31, 8, 3, 2), (128, 5, 8, 1, 0)]):
        img = synth.frame_numpy(w, h, seed=90 + i, bits=bits, components=comps, kind="mixed", interleaved=ilv != 0)
        made.append(ob.encode(img, width=w, height=h, bits_per_sample=bits, component_count=comps, interleave_mode=ilv))
    return made


def entropy_start(jls):
    """The first byte behind the (last) start-of-scan segment."""
    at = jls.rfind(b"\xff\xda")
    return at + 2 + int.from_bytes(jls[at + 2:at + 4], "big")


@pytest.mark.parametrize("order", ["as_is", "shuffled"])
def test_packed_decode_of_a_mixed_batch(torch, order):
    streams = mixed_streams()
    order = None if order == "as_is" else list(np.random.default_rng(42).permutation(len(streams))) + [2]
    a, b = decode_both(torch, streams, None, (4096,), torch.uint8, order=order, lead=3)
    assert (a[2] == 0).all() and (b[2] == a[2]).all()
    assert torch.equal(a[0], b[0])
    if order is None:
        assert a[1] == b[1]  # params_out: the first frame's, byte for byte
        for f, s in enumerate(streams):
            want = ob.decode(s)[1].tobytes()
            assert b[0][f, :len(want)].cpu().numpy().tobytes() == want, f


@pytest.mark.parametrize("damage", ["truncated", "flipped"])
def test_damage_stays_in_its_frame(torch, damage):
    """One stream in the middle of the blob truncated inside its entropy-coded data (the rest of its bytes and the next
    stream follow directly) or with a byte flipped there: the error codes equal the slot call's for the same bytes, and the
    neighbours -- whose bytes abut the damaged stream -- decode exactly."""
    streams = mixed_streams()
    sizes = [len(s) for s in streams]
    for bad in (1, 3, 4):  # 16-bit gray, planar RGB (inside its last scan), 8-bit gray
        damaged, declared = list(streams), list(sizes)
        at = entropy_start(streams[bad]) + (len(streams[bad]) - entropy_start(streams[bad])) // 2
        if damage == "truncated":
            declared[bad] = at
        else:
            raw = bytearray(streams[bad])
            raw[at] ^= 0x5A
            damaged[bad] = bytes(raw)
        a, b = decode_both(torch, damaged, declared, (4096,), torch.uint8, lead=5)
        assert list(a[2]) == list(b[2]), (bad, a[2], b[2])
        assert torch.equal(a[0], b[0])  # (the damaged frame too: the same decoder ran on the same bytes)
        assert (np.delete(b[2], bad) == 0).all() and (damage == "flipped" or b[2][bad] != 0), (bad, b[2])
        for f, s in enumerate(streams):
            if f != bad:
                want = ob.decode(s)[1].tobytes()
                assert b[0][f, :len(want)].cpu().numpy().tobytes() == want, (bad, f)


def test_dicom_shaped_round_trip(torch):
    """The even-size encoding option with offset_alignment = 2: every offset and every size is even (fragments and a basic
    offset table as they stand), and decoding from (offsets, sizes) gives the frames back."""
    c = ENCODE_CASES["gray8_33x17"]
    frames = case_frames(torch, c)
    dst = canary_buffer(torch, FRAMES * batch.estimated_destination_size(c["w"], c["h"], c["bits"], c["comps"]))
    enc = batch.encode_batch_packed(frames, dst, alignment=2, **encode_kw(c, options=1))
    assert (enc.errcs == 0).all() and not (enc.offsets % 2).any() and not (enc.sizes % 2).any()
    plain = slot_reference(torch, "gray8_33x17")[2]
    assert (enc.sizes != plain.sizes).any()  # (some stream had an odd size: the option did something)
    out = torch.zeros_like(frames)
    _, errcs, _ = batch.decode_batch_packed(dst, enc.offsets[:-1], enc.sizes, out)
    assert (errcs == 0).all() and torch.equal(out, frames)


# ---- arguments, work areas -----------------------------------------------------------------------------------------------------

def test_arguments(torch):
    c = ENCODE_CASES["gray8_33x17"]
    frames, pitch, ref, streams = slot_reference(torch, "gray8_33x17")
    slots, sizes = slots_of(torch, streams)
    dst = canary_buffer(torch, 1 << 16)
    for alignment in (0, 3, 8192):
        with pytest.raises(capi.JpegLSError) as e:
            batch.pack_streams(slots, sizes, alignment=alignment, packed=dst)
        assert e.value.errc == INVALID_ARGUMENT
        with pytest.raises(capi.JpegLSError) as e:
            batch.encode_batch_packed(frames, dst, alignment=alignment, **encode_kw(c))
        assert e.value.errc == INVALID_ARGUMENT
    assert (dst == CANARY).all().item()
    l = batch._bind(capi.load_product())
    u64p = C.POINTER(C.c_uint64)
    # NULL offsets: what check_pointer raises
    assert l.charls_amd_pack_streams_device(len(streams), slots.data_ptr(), slots.shape[1], sizes.ctypes.data_as(u64p), dst.data_ptr(),
                                            dst.numel(), 1, None, None) == INVALID_ARGUMENT
    errcs = np.zeros(len(streams), dtype=np.int32)
    out = torch.zeros_like(frames)
    assert l.charls_amd_decode_batch_device_packed(len(streams), dst.data_ptr(), None, sizes.ctypes.data_as(u64p), out.data_ptr(),
                                                   frames[0].numel(), 0, None, errcs.ctypes.data_as(C.POINTER(C.c_int32)), None) == INVALID_ARGUMENT
    p = batch.CodecParams(capi.FrameInfo(c["w"], c["h"], 8, 1), 0, 0, 0, capi.PcParameters(0, 0, 0, 0, 0), 0, 0)
    assert l.charls_amd_encode_batch_device_packed(C.byref(p), len(streams), frames.data_ptr(), frames[0].numel(), 0, dst.data_ptr(), dst.numel(),
                                                   1, 0, None, sizes.ctypes.data_as(u64p), errcs.ctypes.data_as(C.POINTER(C.c_int32)), None) == INVALID_ARGUMENT
    # offset + size overflows
    with pytest.raises(capi.JpegLSError) as e:
        batch.decode_batch_packed(dst, np.array([0, 2**64 - 8], dtype=np.uint64), np.array([int(sizes[0]), 16], dtype=np.uint64), out[:2])
    assert e.value.errc == INVALID_ARGUMENT_SIZE
    # no frames: success
    none = np.zeros(0, dtype=np.uint64)
    assert batch.pack_streams(slots[:0], none, packed=dst).offsets.tolist() == [0]
    assert batch.encode_batch_packed(frames[:0], dst, **encode_kw(c)).offsets.tolist() == [0]
    _, got, _ = batch.decode_batch_packed(dst, none, none, out[:0])
    assert len(got) == 0 and (dst == CANARY).all().item()


def test_the_staging_slots_are_a_work_area(torch, knobs):
    """After a packed encode charls_amd_work_area_bytes includes the staging slots (near-lossless frames: the coder itself keeps
    no work area, so they are all of it); after charls_amd_release_work_areas it is 0."""
    name = "gray8_near2"
    frames, pitch, ref, streams = slot_reference(torch, name)
    batch.release_work_areas()
    assert batch.work_area_bytes() == 0
    knobs.set("PACK_PASS_FRAMES", 5)
    dst = canary_buffer(torch, FRAMES * pitch)
    enc = batch.encode_batch_packed(frames, dst, max_stream_bytes=pitch, **encode_kw(ENCODE_CASES[name]))
    assert (enc.errcs == 0).all()
    assert batch.work_area_bytes() >= 5 * pitch
    batch.release_work_areas()
    assert batch.work_area_bytes() == 0
