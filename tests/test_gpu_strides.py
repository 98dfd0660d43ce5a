"""Padded rows on the MI355X: charls_amd_decode_batch_device / charls_amd_encode_batch_device called directly with `stride`,
`frame_pitch_bytes` and a base offset (charls_amd/batch.py always passes stride 0, and the part-1 decoder applies a stride
with a 2-D copy, so no other test hands a kernel a padded row), the part-1 entry points with `stride`, and the argument
checks of part 2.  Layout, canary check and geometry: tests/strided.py and the header of tests/test_emu_strides.py.

Every case says which kernel it is for and forces or confirms it: a knob (DECODE_GROUP, DECODE_WORKGROUP_WAVES,
EXACT_DECODER, SEQUENTIAL_INTERVALS, TILE_SAMPLES, PIXEL_MODE, set_encode_engine), a counter (exact_retry_scans must not
rise on a speed path; charls_amd_speculation_counters[0] rises when the tile pipeline coded the scan) or a geometry that
admits one route only (decode_launch.hip: wave_decode_eligible; encode_launch.hip: pipeline_eligible).  Everything is compared for equality.  GPU only."""
import ctypes as C

import numpy as np
import pytest

import jls_container
import oracle_bind as ob
import strided as S
from charls_amd import batch, capi
from strided import Geometry as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def lib():
    L = capi.load_product()
    assert L.lib.charls_amd_device_status() == 0
    L.lib.charls_amd_speculation_counters.argtypes = [C.POINTER(C.c_uint64), C.c_int32]
    L.lib.charls_amd_speculation_counters.restype = C.c_int32
    return L


def retries():
    return capi.engine_counters()["exact_retry_scans"]


def tile_jobs(lib):
    out = (C.c_uint64 * 4)()
    lib.lib.charls_amd_speculation_counters(out, 4)
    return int(out[0])


def decode(torch, lib, g, cls, base, *, count=3, pitch="pad", tight=False, near=0, ct=0, preset=None, restart=0, seed=1, kind="mixed"):
    """`count` frames of geometry g decoded as ONE batch into a canary-filled arena; returns the rise of exact_retry_scans."""
    lay = S.layout(g, cls, base, count, pitch, tight)
    frames = [S.Coded(g, seed + 31 * f, near=near, ct=ct, preset=preset, restart=restart, product=lib, kind=kind) for f in range(count)]
    before = retries()
    rc, errcs, arena = S.decode_batch(torch, lib, [f.jls for f in frames], lay)
    rise = retries() - before
    assert rc == 0 and not errcs.any(), (rc, errcs.tolist())
    lay.check(arena, [f.pixels for f in frames])
    return rise


# ---- scan_group_decode.hip through DECODE_GROUP x DECODE_WORKGROUP_WAVES ----------------------------------------------------

GROUP_CASES = [  # width, height, bits, near, stride class, base, count, pitch, tight
    (150, 5, 8, 0, "r16", 0, 44, "mod8", False),     # 9 uint4 + 6 samples per line; neighbouring scans differ in `aligned`
    (150, 2, 8, 2, "r16", 0, 9, "mod0", True),
    (257, 3, 8, 0, "r16p16", 8, 9, "pad", False),
    (16, 6, 8, 2, "r16p16", 0, 9, "mod8", True),
    (7, 9, 8, 0, "p1", 1, 9, "pad", False),
    (1, 7, 8, 0, "p2", 2, 9, "tight", True),
    (150, 3, 8, 0, "p13", 2, 9, "pad", False),
    (257, 1, 8, 2, "big", 0, 5, "pad", True),
    (150, 4, 12, 0, "r16", 0, 44, "mod8", False),    # 16-bit samples: 18 uint4 + 6 samples
    (150, 3, 16, 2, "r16", 0, 9, "mod0", True),
    (257, 2, 16, 0, "r16p16", 2, 9, "even", False),
    (16, 5, 12, 2, "r16p16", 0, 9, "mod8", False),
    (7, 3, 16, 0, "p2", 8, 9, "even", True),
    (1, 2, 12, 0, "p2", 0, 9, "even", False),
    (257, 3, 12, 2, "big", 2, 5, "even", False),
]


@pytest.mark.parametrize("group", [8, 16, 32])
@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("slot", range(5))
def test_group_decoder_rows(torch, lib, knobs, group, waves, slot):
    """Each (G, W) takes a third of the table, the table turned by the slot: over the 30 cases every row of the table meets
    two lanes-per-scan settings and both workgroup shapes."""
    knobs.set("DECODE_GROUP", group)
    knobs.set("DECODE_WORKGROUP_WAVES", waves)
    which = (slot * 3 + (group // 8 - 1 if group < 32 else 2) + (waves == 4) * 7) % len(GROUP_CASES)
    w, h, bits, near, cls, base, count, pitch, tight = GROUP_CASES[which]
    rise = decode(torch, lib, G(w, h, bits), cls, base, count=count, pitch=pitch, tight=tight, near=near, seed=w + h + group)
    assert rise == 0, "a scan left the group decoder"


def test_every_row_of_the_group_table_is_used():
    used = {(slot * 3 + g + (waves == 4) * 7) % len(GROUP_CASES) for slot in range(5) for g in range(3) for waves in (1, 4)}
    assert used == set(range(len(GROUP_CASES)))


@pytest.mark.parametrize("group,waves", [(16, 4), (32, 1)])
def test_group_decoder_unreached_tail_regression(torch, lib, knobs, group, waves):
    """width = 150, stride = 160, every frame 16-byte aligned: the tail loop runs behind the wide stores in every scan."""
    knobs.set("DECODE_GROUP", group)
    knobs.set("DECODE_WORKGROUP_WAVES", waves)
    assert decode(torch, lib, G(150, 6), 160, 0, count=12, pitch=160 * 6, tight=True) == 0


def test_group_decoder_wide_lines(torch, lib, knobs):
    """4096-wide lines, workgroups of four wavefronts."""
    knobs.set("DECODE_GROUP", 32)
    knobs.set("DECODE_WORKGROUP_WAVES", 4)
    assert decode(torch, lib, G(4096, 3), "r16p16", 0, count=9, pitch="mod8") == 0
    assert decode(torch, lib, G(4096, 2, 12), "p2", 2, count=5, pitch="even", tight=True) == 0


@pytest.mark.parametrize("group,w,h,bits,comps,near,ct,cls,base,tight", [
    (8, 150, 3, 8, 3, 0, 1, "r16", 0, False), (16, 150, 2, 8, 3, 0, 2, "p1", 1, True), (32, 257, 2, 8, 2, 0, 0, "p2", 2, False),
    (8, 16, 5, 8, 4, 0, 0, "r16p16", 8, False), (16, 7, 4, 8, 3, 2, 0, "p13", 0, True), (32, 1, 3, 8, 3, 0, 3, "big", 1, False),
    (8, 150, 2, 16, 3, 0, 3, "r16", 0, True), (16, 7, 1, 12, 2, 3, 0, "p2", 2, False), (32, 16, 3, 16, 4, 0, 0, "r16p16", 8, False),
    (16, 150, 4, 16, 3, 0, 1, "big", 0, False)])
def test_line_interleaved_rows(torch, lib, knobs, group, w, h, bits, comps, near, ct, cls, base, tight):
    """decode_scans_group<S, G, NL = 2..4>: the pixel row is interleaved (and inverse-transformed: HP1..3) behind its last line."""
    knobs.set("DECODE_GROUP", group)
    rise = decode(torch, lib, G(w, h, bits, comps, 1), cls, base, count=9, pitch="even", tight=tight, near=near, ct=ct, seed=w + comps)
    assert rise == 0


@pytest.mark.parametrize("group,w,h,bits,comps,near,ct,cls,base,count,pitch,tight", [
    (8, 150, 3, 8, 3, 0, 1, "r16", 0, 41, "mod8", False), (16, 150, 2, 8, 4, 0, 0, "r16p16", 0, 5, "mod0", True),
    (32, 257, 2, 8, 2, 3, 0, "r16", 8, 5, "pad", False), (8, 16, 4, 8, 3, 0, 2, "r16p16", 1, 9, "pad", False),
    (16, 7, 5, 8, 3, 3, 0, "p1", 2, 5, "tight", True), (32, 1, 3, 8, 4, 0, 0, "p2", 1, 5, "pad", False),
    (8, 257, 1, 8, 3, 0, 3, "p13", 0, 9, "pad", False), (16, 150, 2, 8, 2, 0, 0, "big", 2, 5, "pad", True),
    (32, 150, 3, 16, 3, 0, 1, "r16", 0, 41, "mod8", False), (8, 7, 2, 12, 4, 3, 0, "p2", 8, 9, "even", True),
    (16, 16, 3, 16, 2, 0, 0, "r16p16", 2, 5, "even", False), (32, 150, 2, 16, 3, 0, 2, "big", 0, 5, "even", False),
    (16, 257, 2, 16, 3, 3, 0, "r16p16", 0, 5, "mod0", True), (8, 150, 2, 16, 3, 0, 3, "p2", 2, 9, "even", False)])
def test_pixel_decoder_rows(torch, lib, knobs, group, w, h, bits, comps, near, ct, cls, base, count, pitch, tight):
    """scan_group_pixels.hip: sample-interleaved scans take it whenever pixel_group_lanes() != 0 (8-bit, or 16-bit at even addresses)."""
    knobs.set("DECODE_GROUP", group)
    rise = decode(torch, lib, G(w, h, bits, comps, 2), cls, base, count=count, pitch=pitch, tight=tight, near=near, ct=ct, seed=w + comps)
    assert rise == 0


@pytest.mark.parametrize("w,h,bits,cls,base,tight", [(150, 3, 8, "r16", 0, False), (257, 2, 8, "p1", 1, True), (16, 5, 8, "r16p16", 8, False),
                                                     (7, 1, 8, "p13", 2, True), (1, 4, 8, "p2", 0, False), (150, 2, 12, "big", 2, False),
                                                     (150, 3, 16, "r16", 0, True), (7, 2, 16, "p2", 8, False), (257, 2, 16, "r16p16", 0, False)])
def test_fast_decoder_rows(torch, lib, knobs, w, h, bits, cls, base, tight):
    """DECODE_GROUP = 0: decode_scans_fast, one scan per wavefront."""
    knobs.set("DECODE_GROUP", 0)
    assert decode(torch, lib, G(w, h, bits), cls, base, count=5, pitch="even", tight=tight, seed=w) == 0


@pytest.mark.parametrize("w,h,bits,comps,ilv,near,cls,base,tight", [
    (150, 3, 8, 1, 0, 0, "r16", 0, False), (257, 2, 8, 3, 0, 2, "p1", 1, True), (16, 3, 8, 3, 1, 0, "r16p16", 8, False),
    (7, 2, 8, 3, 2, 3, "p13", 2, True), (1, 4, 8, 4, 2, 0, "p2", 1, False), (150, 1, 8, 2, 1, 2, "big", 0, False),
    (150, 2, 16, 3, 2, 0, "r16", 0, True), (7, 3, 12, 1, 0, 0, "p2", 2, False), (16, 2, 16, 3, 1, 0, "r16p16", 8, False)])
def test_wave_decoder_rows(torch, lib, knobs, w, h, bits, comps, ilv, near, cls, base, tight):
    """EXACT_DECODER = 1: decode_scans_wave<S, NC> takes every scan that is wave_decode_eligible."""
    knobs.set("EXACT_DECODER", 1)
    decode(torch, lib, G(w, h, bits, comps, ilv), cls, base, count=5, pitch="even", tight=tight, near=near, seed=w + comps)


# ---- decode_scans_serial: each of the three reasons wave_decode_eligible() has to say no, on its own -------------------------

@pytest.mark.parametrize("w,h,bits,comps,ilv,cls,base,tight", [(150, 3, 12, 1, 0, "r16", 0, False), (7, 2, 16, 3, 2, "p2", 2, True),
                                                               (257, 2, 12, 3, 0, "r16p16", 8, False), (16, 3, 16, 3, 1, "big", 0, False)])
def test_serial_decoder_rows_reset_256(torch, lib, w, h, bits, comps, ilv, cls, base, tight):
    """RESET = 256 is stored as 0 by the reference: the scan's N never halves and only the serial kernel holds it.  Even
    addresses, narrow lines: nothing else keeps the scan off the other kernels."""
    decode(torch, lib, G(w, h, bits, comps, ilv), cls, base, count=3, pitch="even", tight=tight, preset=(0, 0, 0, 0, 256), seed=w)


@pytest.mark.parametrize("cls,base,h", [("p1", 1, 3), ("r16", 0, 2)])
def test_serial_decoder_rows_line_beyond_lds(torch, lib, cls, base, h):
    """A 65535-wide 8-bit line does not fit the 64 KiB of LDS the wave decoders keep it in."""
    decode(torch, lib, G(65535, h), cls, base, count=1, pitch="tight", tight=True, seed=5)


@pytest.mark.parametrize("w,h,bits,comps,cls,base,tight", [(150, 3, 16, 3, "p1", 0, False), (7, 2, 12, 1, "p13", 2, True), (16, 2, 16, 4, "p1", 8, False),
                                                           (257, 1, 16, 1, "p13", 0, True), (1, 5, 16, 3, "p1", 2, False)])
def test_serial_decoder_rows_wide_samples_at_odd_addresses(torch, lib, w, h, bits, comps, cls, base, tight):
    """16-bit planar scans with an odd stride: every second row starts at an odd address."""
    decode(torch, lib, G(w, h, bits, comps, 0), cls, base, count=3, pitch="pad", tight=tight, seed=w + comps)


@pytest.mark.parametrize("w,h,comps,ilv,cls,base", [(150, 3, 1, 0, "r16", 0), (33, 4, 3, 2, "p2", 0), (16, 3, 3, 1, "p2", 1), (257, 2, 3, 0, "r16p16", 0)])
def test_wide_frames_of_one_batch_decode_at_even_and_odd_addresses(torch, lib, knobs, w, h, comps, ilv, cls, base):
    """An odd frame_pitch with an even stride: every other 16-bit frame is off the wave kernels and goes to another launch
    than its neighbours (decode_launch.hip: decode_launch_key); the speed path keeps the others."""
    knobs.set("DECODE_GROUP", 16)
    assert decode(torch, lib, G(w, h, 16, comps, ilv), cls, base, count=9, pitch="pad", seed=w + comps) == 0


# ---- restart intervals: sub-scans at j * lines * stride --------------------------------------------------------------------

@pytest.mark.parametrize("sequential", [None, 1], ids=["interval_parallel", "sequential_intervals"])
@pytest.mark.parametrize("w,h,bits,comps,ilv,near,lines,cls,base,tight", [
    (150, 10, 8, 1, 0, 0, 4, "r16", 0, False), (7, 5, 8, 3, 1, 0, 2, "p13", 1, True), (16, 7, 16, 1, 0, 0, 3, "p2", 2, False),
    (257, 3, 8, 3, 2, 0, 1, "big", 8, False), (150, 9, 8, 1, 0, 2, 4, "p1", 1, True), (16, 6, 8, 3, 0, 0, 5, "r16p16", 0, False)])
def test_restart_interval_rows(torch, lib, knobs, sequential, w, h, bits, comps, ilv, near, lines, cls, base, tight):
    """DRI streams of the product's encoder.  Interval-parallel: restart_intervals_decode.hip builds a sub-scan per interval.  With
    SEQUENTIAL_INTERVALS = 1 a scan stays whole: the speed path meets the RSTm and hands exactly these scans to the exact
    decoder, which crosses the markers itself -- the retry count says so."""
    if sequential is not None:
        knobs.set("SEQUENTIAL_INTERVALS", sequential)
    knobs.set("DECODE_GROUP", 16)
    count = 5
    g = G(w, h, bits, comps, ilv)
    rise = decode(torch, lib, g, cls, base, count=count, pitch="even", tight=tight, near=near, restart=lines, seed=w + lines)
    scans = count * (comps if ilv == 0 else 1)
    assert rise == (scans if sequential else 0), rise


# ---- planar frames: plane c at c * stride * height (batch_api.cpp) ------------------------------------------------------------

@pytest.mark.parametrize("w,h,bits,comps,near,cls,base,count,pitch,tight", [
    (150, 3, 8, 3, 0, "r16", 0, 15, "mod8", False), (7, 2, 8, 4, 2, "p1", 1, 5, "tight", True), (257, 2, 8, 3, 0, "p13", 2, 5, "pad", False),
    (16, 5, 8, 4, 0, "r16p16", 8, 5, "pad", True), (1, 3, 8, 3, 0, "p2", 0, 5, "pad", False), (150, 2, 16, 3, 0, "big", 2, 5, "even", True),
    (150, 3, 12, 4, 2, "r16", 0, 15, "mod8", False)])
def test_planar_multi_scan_rows(torch, lib, w, h, bits, comps, near, cls, base, count, pitch, tight):
    rise = decode(torch, lib, G(w, h, bits, comps, 0), cls, base, count=count, pitch=pitch, tight=tight, near=near, seed=w + comps)
    assert rise == 0


# ---- encode through the batch API ---------------------------------------------------------------------------------------------

def encode(torch, lib, g, cls, base, *, count=3, pitch="pad", tight=False, near=0, ct=0, seed=1):
    """`count` padded frames coded as ONE batch: the oracle's bytes of the PACKED frames, the source arena unchanged.
    Returns the rise of the tile pipeline's job counter."""
    lay = S.layout(g, cls, base, count, pitch, tight)
    frames = [S.Coded(g, seed + 17 * f, near=near, ct=ct) for f in range(count)]
    arena = lay.pad([f.img for f in frames])
    before = tile_jobs(lib)
    rc, errcs, streams, after = S.encode_batch(torch, lib, arena, lay, S.codec_params(g, near, ct))
    rise = tile_jobs(lib) - before
    assert rc == 0 and not errcs.any(), (rc, errcs.tolist())
    for f, fr in enumerate(frames):
        assert streams[f] == fr.jls, (f, len(streams[f]), len(fr.jls))
    assert np.array_equal(after, arena), "the encoder wrote to its source"
    # and through part 1 (charls_jpegls_encoder_encode_from_buffer with `stride`): the smallest legal source buffer of frame 0
    src = arena[lay.first:lay.first + lay.need].copy()
    assert lib.encode(src, near_lossless=near, color_transformation=ct, stride=lay.stride, destination_size=8 * g.packed + 4096, **g.kw()) == frames[0].jls
    assert np.array_equal(src, arena[lay.first:lay.first + lay.need])
    return rise


@pytest.mark.parametrize("w,h,bits,comps,ilv,ct,cls,base,tile,pixel,tight", [
    (150, 5, 8, 1, 0, 0, "r16", 0, None, 0, False), (257, 3, 8, 1, 0, 0, "p1", 1, 64, 0, True),       # a line wider than a tile
    (150, 4, 8, 3, 0, 0, "p13", 2, 128, 0, False), (16, 5, 8, 1, 0, 0, "r16p16", 8, None, 0, False),
    (7, 2, 8, 1, 0, 0, "p2", 1, None, 0, True), (1, 3, 8, 1, 0, 0, "big", 0, None, 0, False),
    (150, 3, 16, 1, 0, 0, "r16", 0, 64, 0, False), (257, 2, 12, 1, 0, 0, "p2", 2, 192, 0, True),
    (150, 5, 8, 1, 0, 0, "p1", 0, None, 1, False), (150, 4, 8, 3, 2, 1, "p1", 1, 64, 0, True), (257, 3, 8, 3, 2, 0, "r16", 0, 128, 0, False),
    (16, 4, 8, 4, 2, 0, "p13", 2, None, 0, False), (7, 3, 8, 2, 2, 0, "p2", 8, None, 0, True), (150, 3, 8, 3, 1, 2, "p13", 1, 64, 0, False),
    (257, 2, 8, 3, 1, 0, "r16p16", 8, 512, 1, False), (150, 3, 16, 3, 2, 0, "p2", 2, 64, 0, True), (1, 2, 8, 3, 2, 0, "big", 1, None, 0, False),
    (257, 4, 8, 1, 0, 0, "p13", 2, 64, 1, False), (150, 2, 16, 3, 1, 3, "r16p16", 0, 128, 0, False)])
def test_tile_pipeline_reads_padded_rows(torch, lib, knobs, w, h, bits, comps, ilv, ct, cls, base, tile, pixel, tight):
    """Regular mode and pixel mode (interleaved scans, lines cut into segment tiles, PIXEL_MODE = 1): pixel mode reads rows as
    4-byte words from a per-row lead that changes from row to row with stride R + 1."""
    if tile:
        knobs.set("TILE_SAMPLES", tile)
    if pixel:
        knobs.set("PIXEL_MODE", 1)
    rise = encode(torch, lib, G(w, h, bits, comps, ilv), cls, base, count=4, pitch="even", tight=tight, ct=ct, seed=w + comps)
    assert rise > 0, "not coded by the tile pipeline"


@pytest.mark.parametrize("w,h,bits,comps,ilv,near,cls,base,tight", [
    (150, 3, 8, 1, 0, 2, "r16", 0, False), (257, 2, 8, 3, 2, 3, "p1", 1, True), (16, 3, 8, 3, 1, 2, "r16p16", 8, False),
    (7, 2, 8, 4, 2, 1, "p13", 2, True), (1, 4, 8, 2, 1, 2, "p2", 1, False), (150, 2, 8, 3, 0, 2, "big", 0, False),
    (150, 3, 16, 1, 0, 3, "r16", 0, True), (7, 2, 12, 3, 2, 2, "p2", 2, False), (16, 2, 16, 3, 1, 5, "r16p16", 8, False)])
def test_group_encoder_reads_padded_rows(torch, lib, w, h, bits, comps, ilv, near, cls, base, tight):
    """NEAR != 0: the tile pipeline is lossless only, scan_group_encode.hip codes these."""
    rise = encode(torch, lib, G(w, h, bits, comps, ilv), cls, base, count=5, pitch="even", tight=tight, near=near, seed=w + comps)
    assert rise == 0


@pytest.mark.parametrize("w,h,bits,comps,ilv,near,ct,cls,base,tight", [
    (150, 3, 8, 1, 0, 0, 0, "r16", 0, False), (257, 2, 8, 3, 0, 2, 0, "p1", 1, True), (16, 3, 8, 3, 1, 0, 1, "r16p16", 8, False),
    (7, 2, 8, 3, 2, 3, 0, "p13", 2, True), (1, 4, 8, 4, 2, 0, 0, "p2", 1, False), (150, 1, 8, 2, 1, 0, 0, "big", 0, False),
    (16, 2, 16, 3, 2, 0, 2, "p2", 2, False)])
def test_serial_encoder_reads_padded_rows(torch, lib, w, h, bits, comps, ilv, near, ct, cls, base, tight):
    batch.set_encode_engine(1, lib)
    try:
        rise = encode(torch, lib, G(w, h, bits, comps, ilv), cls, base, count=3, pitch="even", tight=tight, near=near, ct=ct, seed=w + comps)
    finally:
        batch.set_encode_engine(0, lib)
    assert rise == 0


@pytest.mark.parametrize("w,h,bits,comps,ilv,cls,base,tight", [(150, 3, 16, 1, 0, "p1", 0, False), (7, 2, 12, 3, 0, "p13", 2, True),
                                                               (16, 2, 16, 3, 2, "p1", 8, False), (257, 2, 16, 3, 1, "p13", 1, True),
                                                               (150, 3, 16, 1, 0, "p2", 1, False)])
def test_wide_samples_at_odd_addresses_stay_off_the_tile_pipeline(torch, lib, w, h, bits, comps, ilv, cls, base, tight):
    """16-bit rows with an odd stride or an odd base: pipeline_eligible() is false."""
    rise = encode(torch, lib, G(w, h, bits, comps, ilv), cls, base, count=3, pitch="even", tight=tight, seed=w + comps)
    assert rise == 0


@pytest.mark.parametrize("w,h,comps,ilv,cls,base", [(150, 3, 1, 0, "p2", 0), (33, 4, 3, 2, "r16p16", 0), (16, 3, 3, 1, "p2", 1), (257, 2, 3, 0, "p2", 0)])
def test_wide_frames_of_one_batch_at_even_and_odd_addresses(torch, lib, w, h, comps, ilv, cls, base):
    """An odd frame_pitch with an even stride: every other 16-bit frame of the batch starts at an odd address, and the launch
    chooses its kernel from ONE of them (batch_api.cpp: proto = descs[0])."""
    encode(torch, lib, G(w, h, 16, comps, ilv), cls, base, count=6, pitch="pad", seed=w + comps)


def _dri_scan(img, g, lines, near):
    """The entropy-coded segment a restart-interval encoder has to write: the oracle's coding of every interval of the packed
    image as an image of its own, RSTm between them."""
    want, n = b"", (g.height + lines - 1) // lines
    for j in range(n):
        sub = np.ascontiguousarray(img[j * lines:(j + 1) * lines])
        s = ob.encode(sub, width=g.width, height=sub.shape[0], bits_per_sample=g.bits, component_count=g.comps, interleave_mode=g.ilv,
                      near_lossless=near, destination_size=8 * sub.nbytes + 4096)
        sc = jls_container.parse(s).scans[0]
        want += s[sc.data_start:sc.data_end] + (bytes([0xFF, 0xD0 + (j & 7)]) if j + 1 < n else b"")
    return want


@pytest.mark.parametrize("w,h,bits,comps,ilv,near,lines,cls,base,tight", [
    (150, 8, 8, 1, 0, 0, 3, "r16", 0, False), (17, 4, 8, 1, 0, 0, 1, "p1", 1, True), (16, 5, 8, 3, 2, 0, 2, "p13", 2, False),
    (7, 6, 8, 3, 1, 0, 4, "r16p16", 8, True), (150, 5, 16, 1, 0, 0, 2, "p2", 2, False), (257, 3, 8, 1, 0, 2, 2, "big", 0, False)])
def test_restart_interval_encode_reads_padded_rows(torch, lib, w, h, bits, comps, ilv, near, lines, cls, base, tight):
    g = G(w, h, bits, comps, ilv)
    count = 3
    lay = S.layout(g, cls, base, count, "even", tight)
    imgs = [S.mixed(g, seed=w + lines + f) for f in range(count)]
    arena = lay.pad(imgs)
    rc, errcs, streams, after = S.encode_batch(torch, lib, arena, lay, S.codec_params(g, near, restart=lines))
    assert rc == 0 and not errcs.any(), (rc, errcs.tolist())
    for f, img in enumerate(imgs):
        cont = jls_container.parse(streams[f])
        assert cont.restart_interval == lines and len(cont.scans) == 1
        assert streams[f][cont.scans[0].data_start:cont.scans[0].data_end] == _dri_scan(img, g, lines, near), f
    assert np.array_equal(after, arena), "the encoder wrote to its source"


# ---- part 1: decode_to_buffer / decode_rows / indexed decode with `stride` (decoded packed, placed by a 2-D copy) --------------

@pytest.mark.parametrize("w,h,bits,comps,ilv,cls", [(150, 5, 16, 1, 0, "p1"), (257, 3, 8, 3, 0, "r16"), (16, 4, 8, 3, 1, "r16p16"), (7, 2, 16, 3, 2, "p13"),
                                                    (1, 3, 8, 3, 0, "p2"), (150, 2, 8, 3, 2, "big")])
def test_part1_decode_with_stride(lib, w, h, bits, comps, ilv, cls):
    g = G(w, h, bits, comps, ilv)
    fr = S.Coded(g, seed=w + comps)
    stride = S.stride_of(g.row, cls)
    full = lib.decode(fr.jls, stride=stride)[1].size  # what get_destination_size(stride) returns
    assert full >= S.need(g, stride)
    for size in (full, S.need(g, stride)):
        lay = S.Layout(g, stride, size, 0, 1, tight=False)
        arena = lay.blank()
        lib.decode(fr.jls, stride=stride, out=arena[lay.first:lay.first + size])
        lay.check(arena, [fr.pixels])


@pytest.mark.parametrize("w,h,bits,comps,ilv,K,cls", [(150, 20, 16, 1, 0, 4, "p2"), (33, 17, 8, 3, 0, 5, "r16"), (16, 13, 8, 3, 1, 3, "p13"),
                                                      (7, 9, 8, 3, 2, 2, "p1")])
def test_part1_decode_rows_and_indexed_decode_with_stride(lib, w, h, bits, comps, ilv, K, cls):
    """Buffers of zeros here (capi allocates them): the gaps must still hold zeros."""
    g = G(w, h, bits, comps, ilv)
    fr = S.Coded(g, seed=w + K)
    stride = S.stride_of(g.row, cls)

    def whole(buf):
        lay = S.Layout(g, stride, buf.size, 0, 1)
        arena = lay.blank(0)
        arena[lay.first:lay.first + buf.size] = buf
        lay.check(arena, [fr.pixels], canary=0)

    _, out, index = lib.decode_with_index(fr.jls, K, stride)
    whole(out)
    before = capi.index_counters()["scans_from_points"]
    whole(lib.decode_indexed(fr.jls, index, stride)[1])
    assert capi.index_counters()["scans_from_points"] > before
    packed = np.frombuffer(fr.pixels, dtype=np.uint8).reshape(g.rows, g.row)
    for index_arg in (None, index):
        for first, rows in ((0, h), (K + 1, 2), (h - 1, 1)):
            band = G(w, rows, bits, comps, ilv)
            want = np.concatenate([packed[c * h + first:c * h + first + rows] for c in range(g.rows // h)]).tobytes()
            got = lib.decode_rows(fr.jls, first, rows, index=index_arg, stride=stride)
            lay = S.Layout(band, stride, S.need(band, stride), 0, 1, tight=True)
            assert got.size == lay.need
            arena = lay.blank(0)
            arena[lay.first:lay.first + got.size] = got
            lay.check(arena, [want], canary=0, what=f"rows {first}..{first + rows}")


# ---- the argument checks of part 2 ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,bits,comps,ilv,cls", [(150, 3, 8, 1, 0, "p13"), (16, 4, 8, 3, 0, "r16p16"), (7, 2, 16, 3, 2, "p2"), (33, 3, 8, 3, 1, "r16")])
def test_part2_argument_checks(torch, lib, w, h, bits, comps, ilv, cls):
    """stride < row: invalid_argument_stride.  frame_pitch == need - 1: invalid_argument_size.  frame_pitch == need: success,
    and the byte behind the last row of the last frame is the guard band's."""
    g = G(w, h, bits, comps, ilv)
    stride = S.stride_of(g.row, cls)
    n = S.need(g, stride)
    count = 2
    frames = [S.Coded(g, seed=w + f) for f in range(count)]
    jls = [f.jls for f in frames]
    params = S.codec_params(g)

    def untouched(arena, lay):
        assert (arena == S.CANARY).all(), f"a refused call wrote to {lay.where(int(np.argmax(arena != S.CANARY)))}"

    # decode: the code is the frame's (errcs), the call itself succeeds
    lay = S.Layout(g, g.row, g.packed + 64, 0, count)
    lay.stride = g.row - 1
    rc, errcs, arena = S.decode_batch(torch, lib, jls, lay)
    assert rc == 0 and errcs.tolist() == [S.INVALID_ARGUMENT_STRIDE] * count
    untouched(arena, lay)
    lay = S.Layout(g, stride, n, 0, count, tight=True)
    lay.pitch = n - 1
    rc, errcs, arena = S.decode_batch(torch, lib, jls, lay)
    assert rc == 0 and errcs.tolist() == [S.INVALID_ARGUMENT_SIZE] * count
    if g.rows == g.height:  # (a planar frame's first planes fit and are decoded before the last one is refused)
        untouched(arena, lay)
    assert (arena[:lay.first] == S.CANARY).all() and (arena[-S.GUARD:] == S.CANARY).all()
    lay = S.Layout(g, stride, n, 0, count, tight=True)
    rc, errcs, arena = S.decode_batch(torch, lib, jls, lay)
    assert rc == 0 and not errcs.any()
    lay.check(arena, [f.pixels for f in frames])

    # encode: the call is refused
    lay = S.Layout(g, stride, n, 0, count, tight=True)
    src = lay.pad([f.img for f in frames])
    bad = S.Layout(g, stride, n, 0, count, tight=True)
    bad.stride = g.row - 1
    rc, errcs, streams, after = S.encode_batch(torch, lib, src, bad, params)
    assert rc == S.INVALID_ARGUMENT_STRIDE and all(len(s) == 0 for s in streams)
    bad.stride, bad.pitch = stride, n - 1
    rc, errcs, streams, after = S.encode_batch(torch, lib, src, bad, params)
    assert rc == S.INVALID_ARGUMENT_SIZE and all(len(s) == 0 for s in streams)
    rc, errcs, streams, after = S.encode_batch(torch, lib, src, lay, params)
    assert rc == 0 and not errcs.any() and streams == jls
    assert np.array_equal(after, src)
