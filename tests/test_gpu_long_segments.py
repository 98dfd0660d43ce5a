"""Marker segments longer than the batch decoders' 2048-byte window, on every batch decode route.

The host parses every frame's marker segments from small windows of the device-resident streams; a parse that runs off
its window is retried on one 8 times as large, from a snapshot of the reader.  Four tiny frames (48 x 40: 8-bit gray, 8-bit
3-component planar, 16-bit 2-component planar, 8-bit 3-component sample-interleaved) get comment segments of bytes below
0x80 put into the oracle's streams:
  (a) 3000 bytes right behind SOI: the header pass grows its window once, 2048 -> 16384;
  (b) 40000 bytes right behind SOI: twice, -> 131072;
  (c) planar frames: (a), and 40000 bytes in front of the second SOS: the retry behind a scan, and on the probe copy of the
      one-launch planar plan;
  (d) (b) cut at byte 1502 and at byte 3016: the oracle's errc 15;
  (e) (c) cut one byte short of its end: the oracle's errc 4.
One batch holds them all, good and bad frames alternating.  Every stream is checked against the oracle on the CPU first;
then every route gives the oracle's pixels byte for byte, the oracle's errc for the cut streams and 0 for the others, and
writes nothing outside the frames it decodes.  GPU only."""
import ctypes as C

import numpy as np
import pytest

import oracle_bind as ob
from charls_amd import batch, capi, synth

pytestmark = pytest.mark.gpu

W, H = 48, 40
CANARY = 0xC3
K = 8
FIRST_ROW, ROWS = 10, 20
FRAMES = [  # bits, components, interleave mode
    (8, 1, 0),
    (8, 3, 0),
    (16, 2, 0),
    (8, 3, 2),
]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def lib():
    return capi.load_product()


def _com(n):
    """A COM segment with n payload bytes, all below 0x80."""
    assert n + 2 <= 0xFFFF
    return bytes([0xFF, 0xFE, (n + 2) >> 8, (n + 2) & 0xFF]) + bytes((7 * i + 3) % 0x80 for i in range(n))


def _oracle_errc(jls):
    try:
        ob.decode(jls)
    except ob.OracleError as e:
        return e.errc
    return 0


class Case:
    def __init__(self, name, jls, frame, pixels, errc):
        self.name, self.jls, self.frame, self.pixels, self.errc = name, jls, frame, pixels, errc

    def band(self):
        """Rows [FIRST_ROW, FIRST_ROW + ROWS) in decode_rows' layout: one band per component of a planar frame."""
        bits, comps, ilv = FRAMES[self.frame]
        row = W * (2 if bits > 8 else 1) * (comps if ilv else 1)
        planes = np.frombuffer(self.pixels, dtype=np.uint8).reshape(1 if ilv else comps, H, row)
        return planes[:, FIRST_ROW:FIRST_ROW + ROWS].tobytes()


@pytest.fixture(scope="module")
def cases():
    """The streams of the batch, each checked against the oracle: good ones decode to the frame, cut ones raise their errc."""
    good, bad = [], []
    for f, (bits, comps, ilv) in enumerate(FRAMES):
        img = synth.frame_numpy(W, H, seed=700 + f, bits=bits, components=comps, kind="mixed", interleaved=ilv != 0)
        pixels = img.tobytes()
        plain = ob.encode(img, width=W, height=H, bits_per_sample=bits, component_count=comps, interleave_mode=ilv)
        assert plain[:2] == b"\xff\xd8"
        a = plain[:2] + _com(3000) + plain[2:]
        b = plain[:2] + _com(40000) + plain[2:]
        good += [Case("plain", plain, f, pixels, 0), Case("a", a, f, pixels, 0), Case("b", b, f, pixels, 0)]
        bad += [Case("d1502", b[:1502], f, pixels, 15), Case("d3016", b[:3016], f, pixels, 15)]
        if comps > 1 and ilv == 0:
            first = a.index(b"\xff\xda", 2 + 3004)
            second = a.index(b"\xff\xda", first + 2)  # (no FF DA inside an entropy-coded segment)
            c = a[:second] + _com(40000) + a[second:]
            good.append(Case("c", c, f, pixels, 0))
            bad.append(Case("e", c[:-1], f, pixels, 4))
    for x in good:
        assert ob.decode(x.jls)[1].tobytes() == x.pixels, (x.name, x.frame)
    for x in bad:
        assert _oracle_errc(x.jls) == x.errc, (x.name, x.frame)
    order = []
    for k in range(max(len(good), len(bad))):  # good and bad frames alternate
        order += good[k:k + 1] + bad[k:k + 1]
    assert len(order) == 24
    return order


@pytest.fixture(scope="module")
def slots(torch, cases):
    """(F, pitch) device tensor with stream f in slot f, sizes."""
    pitch = max(len(x.jls) for x in cases) + 16
    host = np.zeros((len(cases), pitch), dtype=np.uint8)
    for f, x in enumerate(cases):
        host[f, :len(x.jls)] = np.frombuffer(x.jls, dtype=np.uint8)
    return torch.from_numpy(host).cuda(), np.array([len(x.jls) for x in cases], dtype=np.uint64)


FRAME_PITCH = 7680  # the largest frame (16-bit, 2 components); 16-bit frames lie at even addresses


def _canary_frames(torch, count, pitch=FRAME_PITCH):
    return torch.full((count, pitch), CANARY, dtype=torch.uint8, device="cuda:0")


def _check(cases, errcs, out, want=lambda x: x.pixels):
    """The oracle's errc for every frame; a good frame holds the oracle's bytes and nothing behind them was written."""
    assert list(errcs) == [x.errc for x in cases]
    got = out.cpu().numpy()
    for f, x in enumerate(cases):
        if x.errc == 0:
            n = len(want(x))
            assert got[f, :n].tobytes() == want(x), (f, x.name, x.frame)
            assert (got[f, n:] == CANARY).all(), (f, x.name, x.frame)


def test_slot_decoder_in_one_launch_and_in_rounds(torch, cases, slots, knobs):
    streams, sizes = slots
    out_a, out_b = _canary_frames(torch, len(cases)), _canary_frames(torch, len(cases))
    knobs.clear("BATCH_ROUNDS")
    _, errcs_a, _ = batch.decode_batch(streams, sizes, out_a)
    knobs.set("BATCH_ROUNDS", 1)
    _, errcs_b, _ = batch.decode_batch(streams, sizes, out_b)
    knobs.clear("BATCH_ROUNDS")
    _check(cases, errcs_a, out_a)
    _check(cases, errcs_b, out_b)


@pytest.fixture(scope="module")
def packed(torch, slots):
    streams, sizes = slots
    return batch.pack_streams(streams, sizes, alignment=1)


def test_packed_decoder(torch, cases, packed):
    out = _canary_frames(torch, len(cases))
    _, errcs, _ = batch.decode_batch_packed(packed.packed, packed.offsets, packed.sizes, out)
    _check(cases, errcs, out)


def _part1_header(lib, jls):
    """(errc, Header, get_destination_size(stride 0)) of a fresh part-1 decoder's header read."""
    try:
        dec, keep = lib._open(jls)
    except capi.JpegLSError as e:
        return e.errc, None, 0
    try:
        n = C.c_size_t()
        assert lib.lib.charls_jpegls_decoder_get_destination_size(dec, 0, C.byref(n)) == 0
        return 0, lib._header(dec), n.value
    finally:
        lib.lib.charls_jpegls_decoder_destroy(dec)


def test_probe_reads_the_headers_part_1_reads(lib, cases, packed):
    params, frame_bytes, errcs = batch.probe_packed(packed.packed, packed.offsets, packed.sizes)
    for f, x in enumerate(cases):
        errc, hdr, nbytes = _part1_header(lib, x.jls)
        assert errc == (15 if x.name.startswith("d") else 0), (f, x.name)  # (stream (e) is cut behind its headers)
        assert errcs[f] == errc and frame_bytes[f] == nbytes, (f, x.name, x.frame)
        if errc:
            assert bytes(params[f]) == bytes(batch.CodecParams())
            continue
        p = params[f]
        pc = p.preset_coding_parameters
        assert (p.frame_info.width, p.frame_info.height, p.frame_info.bits_per_sample, p.frame_info.component_count, p.near_lossless,
                p.interleave_mode, p.color_transformation,
                (pc.maximum_sample_value, pc.threshold1, pc.threshold2, pc.threshold3, pc.reset_value)) == \
               (hdr.width, hdr.height, hdr.bits_per_sample, hdr.component_count, hdr.near_lossless, hdr.interleave_mode,
                hdr.color_transformation, hdr.preset), (f, x.name, x.frame)
        assert nbytes == len(x.pixels)


def test_ragged_decoder_into_canary_buffers(torch, cases, packed):
    outs = [torch.full((len(x.pixels) + 32,), CANARY, dtype=torch.uint8, device="cuda:0") for x in cases]
    _, errcs, _ = batch.decode_batch_ragged(packed.packed, packed.offsets, packed.sizes, outs, capacities=[len(x.pixels) for x in cases])
    assert list(errcs) == [x.errc for x in cases]
    for f, x in enumerate(cases):
        got = outs[f].cpu().numpy()
        assert (got[len(x.pixels):] == CANARY).all(), (f, x.name, x.frame)
        if x.errc == 0:
            assert got[:len(x.pixels)].tobytes() == x.pixels, (f, x.name, x.frame)


@pytest.fixture(scope="module")
def built(torch, lib, cases, slots):
    """charls_amd_decode_batch_device_and_index with K = 8: (errcs, frames, index bytes)."""
    streams, sizes = slots
    out = _canary_frames(torch, len(cases))
    pitch = max(batch.index_size_bound(W, H, bits, comps, ilv, 0, K, lib=lib) for bits, comps, ilv in FRAMES)
    _, errcs, indexes = batch.decode_batch_and_index(streams, sizes, out, K, index_pitch=pitch, lib=lib)
    return errcs, out, indexes


def test_build_gives_the_pixels_and_the_indexes_of_part_1(lib, cases, built):
    errcs, out, indexes = built
    _check(cases, errcs, out)
    for f, x in enumerate(cases):
        want = lib.decode_with_index(x.jls, lines_per_seek_point=K)[2] if x.errc == 0 else b""
        assert indexes[f] == want, (f, x.name, x.frame)


def test_indexed_decoder(torch, lib, cases, slots, built):
    streams, sizes = slots
    out = _canary_frames(torch, len(cases))
    _, errcs = batch.decode_batch_indexed(streams, sizes, built[2], out, lib=lib)
    _check(cases, errcs, out)


def test_row_bands(torch, lib, cases, slots, built):
    streams, sizes = slots
    bands = _canary_frames(torch, len(cases), FRAME_PITCH // 2)
    errcs = batch.decode_rows_batch(streams, sizes, built[2], [FIRST_ROW] * len(cases), [ROWS] * len(cases), bands, lib=lib)
    _check(cases, errcs, bands, Case.band)
