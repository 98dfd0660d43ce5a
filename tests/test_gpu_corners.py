"""The corner corpus (tests/corners.py) on every coding route of the MI355X.

The other GPU tests draw their pixels from charls_amd.synth and the conformance images, which rarely or never drive the model
into its corner states (the census).  Here every frame is one that does -- C and B on their clamps, escape codes in
both modes, RUNindex 31, contexts halved at N = RESET (RESET = 3 too), the largest NEAR and k, N << k == A, samples wrapped by
RANGE -- and every route is forced or confirmed the way tests/test_gpu_strides.py does it: a knob, a counter or a geometry that
admits one route only.  Which frames a route gets is the table corners.ROUTES; the frames of one geometry go through as ONE
batch in the corpus' order, which puts different corners into the lane groups of one wavefront.

Everything is compared for equality with the oracle: encoded bytes, decoded pixels, errc 0.  GPU only."""
import ctypes as C

import numpy as np
import pytest

import corners
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
    """charls_amd_speculation_counters [0] + [2]: the jobs of the context chains and of the run chain that the tile pipeline has
    coded so far.  (A frame of zeros has no regular sample: only its run chain has jobs.)"""
    out = (C.c_uint64 * 4)()
    lib.lib.charls_amd_speculation_counters(out, 4)
    return int(out[0]) + int(out[2])


def geometry(c):
    return G(c.width, c.height, c.bits, c.comps, c.ilv)


def packed(g, count):
    """Packed frames one behind the other; the canary-filled guard bands in front and behind still catch a stray store."""
    return S.Layout(g, g.row, g.packed, 0, count, tight=True)


def cases(route, by="geometry", keep=None):
    """The batches of a route as pytest parameters."""
    names = [n for n in corners.route_frames(route) if keep is None or keep(corners.CORPUS[n])]
    return [pytest.param(v, id=corners.batch_id(k)) for k, v in corners.batches(names, by).items()]


def decode(torch, lib, names, streams=None):
    """The frames `names` (one geometry) decoded as ONE batch; returns the rise of exact_retry_scans."""
    coded = [corners.coded(n) for n in names]
    lay = packed(geometry(coded[0].corner), len(names))
    before = retries()
    rc, errcs, arena = S.decode_batch(torch, lib, streams or [c.jls for c in coded], lay)
    rise = retries() - before
    assert rc == 0 and not errcs.any(), (rc, dict(zip(names, errcs.tolist())))
    lay.check(arena, [c.pixels for c in coded])
    return rise


def encode(torch, lib, names):
    """The frames `names` (one geometry, one set of coding parameters) coded as ONE batch: the oracle's bytes.  Returns the
    rise of the tile pipeline's job counter."""
    coded = [corners.coded(n) for n in names]
    c = coded[0].corner
    g = geometry(c)
    lay = packed(g, len(names))
    arena = lay.pad([x.corner.img for x in coded])
    before = tile_jobs(lib)
    rc, errcs, streams, after = S.encode_batch(torch, lib, arena, lay, S.codec_params(g, c.near, c.ct, c.preset))
    rise = tile_jobs(lib) - before
    assert rc == 0 and not errcs.any(), (rc, dict(zip(names, errcs.tolist())))
    for n, got, want in zip(names, streams, coded):
        assert got == want.jls, (n, len(got), len(want.jls))
    assert np.array_equal(after, arena), "the encoder wrote to its source"
    return rise


# ---- decode ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", [8, 16, 32])
@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("names", cases("group_decode", by="thresholds"))
def test_group_decoder(torch, lib, knobs, group, waves, names):
    """scan_group_decode.hip, the assembly step loop: lossless and near-lossless, gray, planar and line-interleaved.  These are
    valid streams: escape codes, long prefixes and runs beyond the step loop's own service go to the kernel's general path
    (DESIGN 4.2), no scan to the exact decoder."""
    knobs.set("DECODE_GROUP", group)
    knobs.set("DECODE_WORKGROUP_WAVES", waves)
    assert decode(torch, lib, names) == 0, "a valid corner stream left the group decoder"


@pytest.mark.parametrize("names", cases("fast_decode"))
def test_fast_decoder(torch, lib, knobs, names):
    """DECODE_GROUP = 0: decode_scans_fast, whose context records are packed A:24 | N:8 and B:16 | C:16."""
    knobs.set("DECODE_GROUP", 0)
    assert decode(torch, lib, names) == 0


@pytest.mark.parametrize("names", cases("exact_decode"))
def test_exact_decoder(torch, lib, knobs, names):
    knobs.set("EXACT_DECODER", 1)
    decode(torch, lib, names)


@pytest.mark.parametrize("names", cases("serial_decode"))
def test_serial_decoder(torch, lib, names):
    """RESET = 256 (N never halves) and lines of 2^15 samples wider than 8 bits (beyond LDS): wave_decode_eligible() says no."""
    decode(torch, lib, names)


@pytest.mark.parametrize("names", cases("exact_decode", keep=lambda c: c.long and c.bits <= 8))
def test_long_lines_of_narrow_samples_decode(torch, lib, names):
    """The 2^15-sample lines of 8-bit samples fit LDS: whichever kernel the launch plan gives them."""
    decode(torch, lib, names)


@pytest.mark.parametrize("group", [8, 16, 32])
@pytest.mark.parametrize("names", cases("pixel_decode", by="thresholds", keep=lambda c: c.ilv == 2))
def test_pixel_decoder_sample_interleaved(torch, lib, knobs, group, names):
    """scan_group_pixels.hip: one pixel has one component in an escape code and another on a C clamp."""
    knobs.set("DECODE_GROUP", group)
    assert decode(torch, lib, names) == 0


@pytest.mark.parametrize("group", [8, 32])
@pytest.mark.parametrize("names", cases("pixel_decode", by="thresholds", keep=lambda c: c.ilv != 2))
def test_pixel_decoder_near_lossless(torch, lib, knobs, group, names):
    """NEAR_DECODE_PIXELS = 1 brings near-lossless gray and line-interleaved scans back to the pixel kernels."""
    knobs.set("NEAR_DECODE_PIXELS", 1)
    knobs.set("DECODE_GROUP", group)
    assert decode(torch, lib, names) == 0


# (planar frames are one gray scan per component: the gray frames stand for them)
RESTART = [n for n, c in corners.SMALL.items() if c.preset is None and c.bits in (8, 16) and c.ct == 0 and (c.comps == 1 or c.ilv != 0)]


def _restart_cases():
    # 5 lines: no multiple of the tiles' periods (2 and 3), so an interval boundary falls inside the pattern
    return [pytest.param(v, id=corners.batch_id(k)) for k, v in corners.batches(RESTART, by="parameters").items()]


def _dri_scan(c, lines):
    """The entropy-coded segment a restart-interval encoder has to write: the oracle's coding of every interval as an image of
    its own, RSTm between them."""
    want, n = b"", (c.height + lines - 1) // lines
    for j in range(n):
        rows = slice(j * lines, (j + 1) * lines)
        sub = np.ascontiguousarray(c.img[rows])
        s = ob.encode(sub, **dict(c.kw(), height=sub.shape[0]), destination_size=8 * sub.nbytes + 4096)
        sc = jls_container.parse(s).scans[0]
        want += s[sc.data_start:sc.data_end] + (bytes([0xFF, 0xD0 + (j & 7)]) if j + 1 < n else b"")
    return want


@pytest.mark.parametrize("names", _restart_cases())
def test_restart_intervals_both_ways(torch, lib, knobs, names):
    """Restart intervals of 5 lines: the encoder's intervals are the oracle's coding of each interval, the decoder gives the
    oracle's pixels interval-parallel (restart_intervals_decode.hip) and, SEQUENTIAL_INTERVALS = 1, with the scan left whole: the
    speed path meets the RSTm and hands exactly these scans to the exact decoder."""
    lines = 5
    cs = [corners.CORPUS[n] for n in names]
    c = cs[0]
    g = geometry(c)
    lay = packed(g, len(names))
    arena = lay.pad([x.img for x in cs])
    rc, errcs, streams, after = S.encode_batch(torch, lib, arena, lay, S.codec_params(g, c.near, c.ct, c.preset, restart=lines))
    assert rc == 0 and not errcs.any(), (rc, errcs.tolist())
    for n, x, s in zip(names, cs, streams):
        cont = jls_container.parse(s)
        assert cont.restart_interval == lines and len(cont.scans) == 1
        assert s[cont.scans[0].data_start:cont.scans[0].data_end] == _dri_scan(x, lines), n
    pixels = [ob.decode(s)[1].tobytes() for s in streams]
    knobs.set("DECODE_GROUP", 16)
    for sequential in (None, 1):
        if sequential:
            knobs.set("SEQUENTIAL_INTERVALS", 1)
        before = retries()
        rc, errcs, out = S.decode_batch(torch, lib, streams, lay)
        rise = retries() - before
        assert rc == 0 and not errcs.any(), (sequential, errcs.tolist())
        lay.check(out, pixels)
        speed_path = corners.ROUTES["group_decode"](c) or corners.ROUTES["pixel_decode"](c)
        assert rise == (len(names) if sequential and speed_path else 0), (sequential, rise)


@pytest.mark.parametrize("names", cases("seek_decode"))
def test_indexed_decode(lib, names):
    """A seek-point index of 7 lines a point (2 for the few long lines) built from the same stream: the resume states carry C,
    RUNindex and the run contexts at their extremes.  The indexed decode gives the oracle's pixels and starts from the points."""
    for n in names:
        c = corners.coded(n)
        _, out, index = lib.decode_with_index(c.jls, 7 if c.corner.height > 7 else 2, 0)
        assert out.tobytes() == c.pixels, n
        before = capi.index_counters()["scans_from_points"]
        assert lib.decode_indexed(c.jls, index, 0)[1].tobytes() == c.pixels, n
        assert capi.index_counters()["scans_from_points"] > before, n


# ---- encode ---------------------------------------------------------------------------------------------------------------------

FORCED = {"JOB_EVENTS": "32", "WARM_EVENTS": "0", "RUN_JOB_EVENTS": "32", "RUN_WARM_EVENTS": "0"}


@pytest.mark.parametrize("names", cases("tile_encode", by="parameters"))
def test_tile_pipeline_default_knobs(torch, lib, names):
    assert encode(torch, lib, names) > 0, "not coded by the tile pipeline"


@pytest.mark.parametrize("how", ["small_tiles", "pixel_mode", "forced_speculation"])
@pytest.mark.parametrize("names", cases("tile_encode", by="parameters"))
def test_tile_pipeline_forced(torch, lib, knobs, how, names):
    """TILE_SAMPLES = 64: a line is cut into tiles.  PIXEL_MODE = 1.  Jobs of 32 events without warm-up: a job boundary falls
    where C sits on its clamp and where the run chain's RUNindex is high, and every guess of a boundary state is checked."""
    if how == "small_tiles":
        knobs.set("TILE_SAMPLES", 64)
    elif how == "pixel_mode":
        knobs.set("PIXEL_MODE", 1)
    else:
        for k, v in FORCED.items():
            knobs.set(k, v)
    assert encode(torch, lib, names) > 0, "not coded by the tile pipeline"


@pytest.mark.parametrize("names", cases("group_encode", by="parameters"))
def test_group_encoder_and_its_measuring_form(torch, lib, names):
    """scan_group_encode.hip codes every near-lossless frame; charls_amd_measure_batch_device sizes it without writing it."""
    assert encode(torch, lib, names) == 0
    cs = [corners.CORPUS[n] for n in names]
    c = cs[0]
    frames = torch.from_numpy(np.stack([np.frombuffer(x.img.tobytes(), dtype=np.uint8) for x in cs])).cuda()
    sizes = batch.measure_batch(frames, [c.near], bits_per_sample=c.bits, component_count=c.comps, interleave_mode=c.ilv,
                                color_transformation=c.ct, preset=c.preset or (0, 0, 0, 0, 0), width=c.width, height=c.height, lib=lib)
    assert sizes[:, 0].tolist() == [len(corners.coded(n).jls) for n in names]


@pytest.mark.parametrize("names", cases("serial_encode", by="parameters"))
def test_serial_encoder(torch, lib, names):
    batch.set_encode_engine(1, lib)
    try:
        rise = encode(torch, lib, names)
    finally:
        batch.set_encode_engine(0, lib)
    assert rise == 0


# ---- mixed ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 12, 16])
def test_one_batch_of_corners_and_ordinary_frames(torch, lib, bits):
    """All 48 x 64 gray corner frames of one sample width and ordinary `mixed` frames in turn, in ONE call of
    charls_amd_decode_batch_device (every coding parameter occurs) and, the lossless ones with the default parameters, in ONE
    call of charls_amd_encode_batch_device."""
    g = G(corners.W, corners.H, bits)
    for lossless_defaults in (False, True):
        names = [n for n, c in corners.SMALL.items() if c.bits == bits and c.comps == 1 and
                 (not lossless_defaults or (c.near == 0 and c.preset is None))]
        frames = []
        for i, n in enumerate(names):
            frames.append(corners.coded(n))
            frames.append(S.Coded(g, 100 + i))
        lay = packed(g, len(frames))
        if lossless_defaults:
            arena = lay.pad([f.corner.img if isinstance(f, corners.CodedCorner) else f.img for f in frames])
            rc, errcs, streams, _ = S.encode_batch(torch, lib, arena, lay, S.codec_params(g))
            assert rc == 0 and not errcs.any() and streams == [f.jls for f in frames]
        else:
            rc, errcs, arena = S.decode_batch(torch, lib, [f.jls for f in frames], lay)
            assert rc == 0 and not errcs.any(), errcs.tolist()
            lay.check(arena, [f.pixels for f in frames])


PART1 = [n for i, n in enumerate(corners.CORPUS) if i % 5 == 0 or corners.CORPUS[n].long]


@pytest.mark.parametrize("name", PART1)
def test_part1_abi(lib, name):
    """charls_jpegls_encoder / charls_jpegls_decoder (capi.encode / capi.decode) on every fifth frame and the long lines."""
    c = corners.coded(name)
    assert lib.encode(c.corner.img, destination_size=8 * c.corner.img.nbytes + 4096, **c.corner.kw()) == c.jls
    assert lib.decode(c.jls)[1].tobytes() == c.pixels
