"""Re-coding a packed blob in one call (charls_amd.h part 2j) on the GPU.  The contract is a composition, so the first test holds
the call, byte for byte, to the explicit probe + charls_amd_decode_batch_device_ragged + charls_amd_encode_batch_device_ragged of
the same build; the others hold it to the oracle (identity on reference-written streams, the same pixels behind a new restart
interval, the NEAR bound), to its own windows, to the failure and capacity rules, to the work-area rules, to the host form, and
to what it is for: a stream that part 2g can salvage.  Every output buffer is filled with a canary first.  All frames are tiny.
GPU only."""
import os

import numpy as np
import pytest

import common
import oracle_bind as ob
import strided
from charls_amd import batch, capi
from strided import Geometry

pytestmark = pytest.mark.gpu

CANARY = 0xA5
NOT_ENOUGH_MEMORY, DESTINATION_TOO_SMALL, INVALID_OPERATION, INVALID_ARGUMENT_COLOR_TRANSFORMATION = 1, 3, 100, 109

# kind -> (geometry, NEAR, colour transformation, restart interval of the SOURCE stream)
KINDS = {
    "gray8_48x64": (Geometry(48, 64), 0, 0, 0),
    "gray12_150x40": (Geometry(150, 40, bits=12), 0, 0, 0),
    "gray16_48x64": (Geometry(48, 64, bits=16), 0, 0, 0),
    "rgb_planar_48x64": (Geometry(48, 64, comps=3, ilv=0), 0, 0, 0),
    "rgb_line_150x40": (Geometry(150, 40, comps=3, ilv=1), 0, 0, 0),
    "rgb_sample_48x64": (Geometry(48, 64, comps=3, ilv=2), 0, 0, 0),
    "hp1_sample_150x40": (Geometry(150, 40, comps=3, ilv=2), 0, 1, 0),
    "near2_150x40": (Geometry(150, 40), 2, 0, 0),
    "restart16_48x64": (Geometry(48, 64), 0, 0, 16),
    "gray_1x1": (Geometry(1, 1), 0, 0, 0),
    "gray_1x40": (Geometry(1, 40), 0, 0, 0),
    "gray_150x1": (Geometry(150, 1), 0, 0, 0),
    "gray8_150x40": (Geometry(150, 40), 0, 0, 0),
}
LOSSLESS_PLAIN = [k for k, (_, near, ct, _) in KINDS.items() if near == 0 and ct == 0]

# The specs of the issue.  The restart intervals are 8 and 16 lines against heights of 64, 40 and 1 -- 40 is no multiple of 16
# -- and 100, which is at least every height.
SPECS = {
    "nothing": lambda: capi.transcode_spec(),
    "restart8": lambda: capi.transcode_spec(restart_interval=8),
    "restart16": lambda: capi.transcode_spec(restart_interval=16),
    "restart100": lambda: capi.transcode_spec(restart_interval=100),
    "near2": lambda: capi.transcode_spec(near_lossless=2),
    "near2_restart16": lambda: capi.transcode_spec(near_lossless=2, restart_interval=16),
    "reset31": lambda: capi.transcode_spec(preset=(0, 0, 0, 0, 31)),
}


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


_base = []


@pytest.fixture(scope="module")
def base(lib):
    """One source stream of every kind, thirteen in all: the oracle's coding (the product's, for the one with restart
    intervals, which the reference cannot write) and the oracle's pixels of it."""
    if not _base:
        for f, (kind, (g, near, ct, restart)) in enumerate(KINDS.items()):
            x = strided.Coded(g, 900 + f, near=near, ct=ct, restart=restart, product=lib)
            x.kind = kind
            _base.append(x)
    return _base


def blob_of(torch, streams, lead=3):
    """The streams back to back behind `lead` bytes (odd offsets), on the device: (blob, offsets, sizes)."""
    offsets, raw = [], bytearray(b"\x00" * lead)
    for s in streams:
        offsets.append(len(raw))
        raw += s
    raw += bytes(32)
    return (torch.from_numpy(np.frombuffer(bytes(raw), dtype=np.uint8).copy()).cuda(), np.array(offsets, dtype=np.uint64),
            np.array([len(s) for s in streams], dtype=np.uint64))


def canary_buffer(torch, nbytes):
    return torch.full((nbytes,), CANARY, dtype=torch.uint8, device="cuda:0")


def room_for(streams, alignment):
    """Bytes that hold every stream re-coded with any of SPECS (markers of restart intervals, an LSE segment) at the alignment."""
    return sum(-(-(2 * len(s) + 1024) // alignment) * alignment for s in streams) + 64


def spec_list(specs, count):
    return [specs] * count if isinstance(specs, capi.TranscodeSpec) else list(specs)


def with_spec(params, spec):
    p = batch.CodecParams.from_buffer_copy(params)
    if spec.set & capi.TRANSCODE_NEAR:
        p.near_lossless = spec.near_lossless
    if spec.set & capi.TRANSCODE_RESTART_INTERVAL:
        p.restart_interval = spec.restart_interval
    if spec.set & capi.TRANSCODE_PRESET:
        p.preset_coding_parameters = spec.preset_coding_parameters
    if spec.set & capi.TRANSCODE_ENCODING_OPTIONS:
        p.encoding_options = spec.encoding_options
    return p


def transcode(torch, blob, offsets, sizes, specs, room, *, alignment=1, capacity=None):
    dst = canary_buffer(torch, room)
    got = batch.transcode_batch(blob, offsets, sizes, specs, dst, alignment=alignment, capacity=capacity)
    torch.cuda.synchronize()
    return got, dst.cpu().numpy()


def composed(torch, blob, offsets, sizes, specs, room, *, alignment=1, capacity=None, refused=()):
    """What the caller-side glue gives: probe, ragged decode into packed frames of the caller's own, ragged encode of the frames
    that decoded -- (offsets, sizes, errcs, params as bytes, the output buffer on the host).  `refused`: frames that name a
    mapping table, which the glue cannot see and the call refuses."""
    count = len(sizes)
    specs = spec_list(specs, count)
    _, frame_bytes, _ = batch.probe_packed(blob, offsets, sizes)
    outs = [canary_buffer(torch, max(int(n), 1)) for n in frame_bytes]
    params, errcs, _ = batch.decode_batch_ragged(blob, offsets, sizes, outs, capacities=[int(n) for n in frame_bytes])
    errcs = errcs.copy()
    for f in refused:
        assert errcs[f] == 0
        errcs[f] = INVALID_OPERATION
    sent = [f for f in range(count) if errcs[f] == 0]
    coded_with = {f: with_spec(params[f], specs[f]) for f in sent}
    dst = canary_buffer(torch, room)
    enc = batch.encode_batch_ragged([outs[f] for f in sent], [coded_with[f] for f in sent], dst, alignment=alignment, capacity=capacity,
                                    strides=[0] * len(sent))
    torch.cuda.synchronize()
    offsets_out, sizes_out = np.zeros(count + 1, dtype=np.uint64), np.zeros(count, dtype=np.uint64)
    params_out = [bytes(batch.CodecParams())] * count
    at = len(sent)
    offsets_out[count] = enc.offsets[at]
    for f in reversed(range(count)):  # (a frame that was not sent stands where the next one that was starts)
        if errcs[f] == 0:
            at -= 1
            sizes_out[f], errcs[f], params_out[f] = enc.sizes[at], enc.errcs[at], bytes(coded_with[f])
        offsets_out[f] = enc.offsets[at]
    return offsets_out, sizes_out, errcs, params_out, dst.cpu().numpy()


def same_as_composed(got, host, want):
    offsets, sizes, errcs, params, want_host = want
    assert got.offsets.tolist() == offsets.tolist()
    assert got.sizes.tolist() == sizes.tolist()
    assert got.errcs.tolist() == errcs.tolist()
    for f in range(len(sizes)):
        assert bytes(got.params[f]) == params[f], f
    bad = np.flatnonzero(host != want_host)
    assert bad.size == 0, f"{bad.size} bytes differ, the first at {int(bad[0])}"


def streams_of(got, host):
    return [host[int(o):int(o) + int(n)].tobytes() for o, n in zip(got.offsets[:-1], got.sizes)]


# ---- 1: the composition -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alignment", [1, 16, 4096])
def test_the_call_is_the_composition(torch, base, alignment):
    streams = [x.jls for x in base]
    blob, offsets, sizes = blob_of(torch, streams)
    room = room_for(streams, alignment)
    names = list(SPECS)
    runs = [SPECS[name]() for name in names]                                    # uniform: one spec for every frame
    runs.append([SPECS[names[(f + 1) % len(names)]]() for f in range(len(base))])  # one each, every spec in turn
    runs.append([SPECS[names[(3 * f) % len(names)]]() for f in range(len(base))])
    assert sum(1 for x in base if x.ct) == 1  # (the HP1 source: the frame the encoder refuses once NEAR is set)
    for specs in runs:
        got, host = transcode(torch, blob, offsets, sizes, specs, room, alignment=alignment)
        same_as_composed(got, host, composed(torch, blob, offsets, sizes, specs, room, alignment=alignment))
        each = spec_list(specs, len(base))
        for f, x in enumerate(base):  # (and the composition is not a batch of failures)
            refused = x.ct and (each[f].set & capi.TRANSCODE_NEAR)
            assert got.errcs[f] == (INVALID_ARGUMENT_COLOR_TRANSFORMATION if refused else 0), (f, x.kind)
            assert (got.sizes[f] == 0) == bool(refused)
            if each[f].set & capi.TRANSCODE_RESTART_INTERVAL and not refused:
                assert got.params[f].restart_interval == each[f].restart_interval
        assert (host[int(got.offsets[-1]):] == CANARY).all()


# ---- 2: against the oracle -------------------------------------------------------------------------------------------------------

# The reference-written goldens under tests/golden/small whose container is the plain one -- SOI, SOF55, an LSE exactly when the
# parameters are not the defaults, the scans, EOI: no SPIFF header, no comment, no application data (which leaves out the colour
# transformations, announced in an APP8 segment), no mapping table, no DNL -- as is_plain below
# finds them; tests/test_transcode_cpu.py holds this list to that rule without a GPU.
PLAIN_GOLDENS = [
    "c2_ilv1", "c2_ilv2", "c4_ilv1", "c4_ilv2", "c5_ilv0", "cfg2_crop256", "cfg3_crop256", "cfg3b_crop256_12bit", "cfg5b_crop128",
    "gray10_64x48", "gray10_near3_64x48", "gray12_64x48", "gray12_near3_64x48", "gray12_pc_jai", "gray15_64x48", "gray15_near3_64x48",
    "gray16_64x48", "gray16_near3_64x48", "gray16_noise_64", "gray2_64x48", "gray2_near1_64x48", "gray4_64x48", "gray4_near3_64x48",
    "gray7_64x48", "gray7_near3_64x48", "gray8_1x1", "gray8_64x48", "gray8_custom_pc", "gray8_h1", "gray8_hard_128", "gray8_maxval100",
    "gray8_near3_64x48", "gray8_noise_96", "gray8_runs_300x40", "gray8_w1", "gray8_zero_512", "rgb16_ilv0_40x30", "rgb16_ilv1_40x30",
    "rgb16_ilv2_40x30", "rgb8_ilv0_80x60", "rgb8_ilv0_near2_80x60", "rgb8_ilv1_80x60", "rgb8_ilv1_near2_80x60", "rgb8_ilv2_80x60",
    "rgb8_ilv2_near2_80x60", "tiny_c2_ilv1", "tiny_c4_ilv2_near1", "tiny_gray12", "tiny_gray16_noise", "tiny_gray2", "tiny_gray8_near3",
    "tiny_gray8_noise", "tiny_rgb8_ilv0", "tiny_rgb8_ilv1", "tiny_rgb8_ilv1_near1", "tiny_rgb8_ilv2", "tiny_rgb8_ilv2_near2",
]


def golden(name):
    with open(os.path.join(common.GOLDEN, "small", name + ".jls"), "rb") as f:
        return f.read()


def segments(data):
    """[(marker, payload)] of a stream, the entropy-coded segments skipped; raises on anything that is no marker segment."""
    assert data[:2] == b"\xff\xd8"
    out, i = [], 2
    while True:
        assert data[i] == 0xFF and data[i + 1] >= 0x80, i
        marker = data[i + 1]
        if marker == 0xD9:
            assert i + 2 == len(data)
            return out
        n = int.from_bytes(data[i + 2:i + 4], "big")
        out.append((marker, data[i + 4:i + 2 + n]))
        i += 2 + n
        if marker == 0xDA:
            while not (data[i] == 0xFF and data[i + 1] >= 0x80 and not 0xD0 <= data[i + 1] <= 0xD7):
                i += 1


def is_plain(data, case):
    try:
        found = segments(data)
    except (AssertionError, IndexError):
        return False
    markers = [m for m, _ in found]
    if any(m not in (0xF7, 0xF8, 0xDA) for m in markers):  # SOF55, LSE, SOS: no SPIFF / APPn, COM, DNL, DRI
        return False
    lse = [payload for m, payload in found if m == 0xF8]
    if any(payload[0] != 1 for payload in lse):  # (an LSE that is no preset-parameters segment: a mapping table, oversize)
        return False
    if any(payload[2 + 2 * k] != 0 for m, payload in found if m == 0xDA for k in range(payload[0])):  # a scan names a table
        return False
    return (len(lse) == 1) == (case["preset"] is not None)  # (an LSE exactly when the case asked for parameters of its own)


# Near-lossless coding is not idempotent where a reconstructed sample was clamped at 0 or MAXVAL: the error of the clamped value
# against its prediction quantises differently the second time.  For these ten goldens the ORACLE's own coding of its own decode
# differs from the golden (sizes: 9687 for 9332 bytes of cfg5b_crop128, 171 for 174 of tiny_gray8_near3, ...), so no re-coder can
# give the input back; the call must give what the oracle gives.  Every other plain golden, all lossless ones among them, comes
# back byte for byte.
NOT_IDEMPOTENT = ["cfg5b_crop128", "gray4_near3_64x48", "gray7_near3_64x48", "gray8_near3_64x48", "rgb8_ilv0_near2_80x60",
                  "rgb8_ilv1_near2_80x60", "rgb8_ilv2_near2_80x60", "tiny_gray8_near3", "tiny_rgb8_ilv1_near1", "tiny_rgb8_ilv2_near2"]


def oracle_recoded(data):
    """The oracle's coding of the oracle's decode of `data`, with the parameters it read from it."""
    p, pixels = ob.decode(data)
    preset = (p.maximum_sample_value, p.threshold1, p.threshold2, p.threshold3, p.reset_value)
    return ob.encode(pixels, width=p.width, height=p.height, bits_per_sample=p.bits_per_sample, component_count=p.component_count,
                     near_lossless=p.near_lossless, interleave_mode=p.interleave_mode, preset=preset if any(preset) else None,
                     destination_size=4 * pixels.nbytes + 4096)


def test_identity_on_reference_written_streams(torch):
    streams = [golden(name) for name in PLAIN_GOLDENS]
    blob, offsets, sizes = blob_of(torch, streams)
    got, host = transcode(torch, blob, offsets, sizes, capi.transcode_spec(), room_for(streams, 1))
    assert (got.errcs == 0).all()
    for f, (name, s, back) in enumerate(zip(PLAIN_GOLDENS, streams, streams_of(got, host))):
        if name in NOT_IDEMPOTENT:
            assert got.params[f].near_lossless > 0 and oracle_recoded(s) != s, name
            assert back == oracle_recoded(s), name
        else:
            assert back == s, name


def samples(x, raw):
    return np.frombuffer(raw, dtype=np.uint8 if x.g.bits <= 8 else np.uint16).astype(np.int32)


def test_a_new_restart_interval_keeps_the_pixels(torch, base):
    streams = [x.jls for x in base]
    blob, offsets, sizes = blob_of(torch, streams)
    got, host = transcode(torch, blob, offsets, sizes, capi.transcode_spec(restart_interval=8), room_for(streams, 2), alignment=2)
    assert (got.errcs == 0).all()
    out = streams_of(got, host)
    for x, s in zip(base, out):
        if x.near == 0:
            assert ob.decode(s)[1].tobytes() == x.pixels, x.kind
        else:  # a near-lossless source is coded near-lossless again, now from other contexts: within its NEAR, not equal
            error = np.abs(samples(x, ob.decode(s)[1].tobytes()) - samples(x, x.pixels))
            assert 0 < int(error.max()) <= x.near, x.kind
        assert (b"\xff\xd0" in s) == (x.g.height > 8), x.kind  # (the intervals are there)
    again, o, n = blob_of(torch, out, lead=1)
    params, _, errcs = batch.probe_packed(again, o, n)
    assert (errcs == 0).all() and all(params[f].restart_interval == 8 for f in range(len(base)))


@pytest.mark.parametrize("near", [1, 2, 5])
def test_the_near_lossless_bound(torch, base, near):
    frames = [x for x in base if x.kind in LOSSLESS_PLAIN]
    streams = [x.jls for x in frames]
    blob, offsets, sizes = blob_of(torch, streams)
    got, host = transcode(torch, blob, offsets, sizes, capi.transcode_spec(near_lossless=near, restart_interval=16), room_for(streams, 1))
    assert (got.errcs == 0).all()
    largest = 0
    for f, (x, s) in enumerate(zip(frames, streams_of(got, host))):
        assert got.params[f].near_lossless == near
        error = int(np.abs(samples(x, ob.decode(s)[1].tobytes()) - samples(x, x.pixels)).max())
        assert error <= near, x.kind
        largest = max(largest, error)
    assert largest > 0  # (the frames were coded near-lossless, not copied)


# ---- 3: windows -------------------------------------------------------------------------------------------------------------------

def test_windows_do_not_change_the_result(torch, base, knobs):
    assert len(base) == 13
    streams = [x.jls for x in base]
    blob, offsets, sizes = blob_of(torch, streams)
    specs = [SPECS[("restart8", "near2_restart16", "nothing")[f % 3]]() for f in range(13)]
    room = room_for(streams, 16)
    before = capi.transcode_counters()
    want, want_host = transcode(torch, blob, offsets, sizes, specs, room, alignment=16)
    assert capi.transcode_counters()[1] - before[1] == 1  # (tiny frames: one window holds them all)
    for window in (1, 2, 5):
        knobs.set("TRANSCODE_WINDOW_FRAMES", window)
        before = capi.transcode_counters()
        got, host = transcode(torch, blob, offsets, sizes, specs, room, alignment=16)
        after = capi.transcode_counters()
        assert after[1] - before[1] == -(-13 // window), window
        assert after[0] - before[0] == int((want.errcs == 0).sum())
        assert got.offsets.tolist() == want.offsets.tolist() and got.sizes.tolist() == want.sizes.tolist(), window
        assert got.errcs.tolist() == want.errcs.tolist() and (host == want_host).all(), window
        assert all(bytes(got.params[f]) == bytes(want.params[f]) for f in range(13)), window
    knobs.clear("TRANSCODE_WINDOW_FRAMES")
    got, host = transcode(torch, blob, offsets, sizes, specs, room, alignment=16)
    assert (host == want_host).all()


# ---- 4: failures stay local -------------------------------------------------------------------------------------------------------

def names_a_table(jls):
    """The stream with mapping table 1 named for the first component of its first scan (the table itself is not there: an
    abbreviated-format reference, which decodes like any other stream)."""
    at = jls.index(b"\xff\xda")
    out = bytearray(jls)
    assert out[at + 6] == 0
    out[at + 6] = 1  # FF DA, length (2), Ns, Cs_1, Tm_1
    return bytes(out)


def test_failures_stay_local(torch, base, knobs):
    gray = next(x for x in base if x.kind == "gray8_48x64")
    zeroed = bytearray(gray.jls)
    middle = len(zeroed) // 2
    assert any(zeroed[middle:middle + 4])
    zeroed[middle:middle + 4] = bytes(4)
    bad = {  # position -> the stream
        2: gray.jls[:len(gray.jls) // 2],                                                # truncated
        5: bytes(zeroed),                                                                 # four bytes zeroed
        6: bytes(np.random.default_rng(3).integers(0, 256, 300, dtype=np.uint8)),        # garbage
        9: b"",                                                                           # sizes_in[f] == 0
        12: names_a_table(gray.jls),
    }
    streams = [x.jls for x in base]
    for at in sorted(bad):
        streams.insert(at, bad[at])
    hp1 = next(f for f, s in enumerate(streams) if s == next(x.jls for x in base if x.ct))
    specs = [capi.transcode_spec(restart_interval=8) for _ in streams]
    specs[hp1] = capi.transcode_spec(near_lossless=1, restart_interval=8)  # an HP1 frame with NEAR set: the encoder refuses it
    failing = sorted(list(bad) + [hp1])
    blob, offsets, sizes = blob_of(torch, streams)
    room = room_for(streams, 4)
    sound = [s for f, s in enumerate(streams) if f not in failing]
    clean_blob, clean_offsets, clean_sizes = blob_of(torch, sound)
    clean, clean_host = transcode(torch, clean_blob, clean_offsets, clean_sizes, capi.transcode_spec(restart_interval=8), room, alignment=4)
    assert (clean.errcs == 0).all()
    before = capi.transcode_counters()
    for window in (None, 3):
        if window:
            knobs.set("TRANSCODE_WINDOW_FRAMES", window)
        got, host = transcode(torch, blob, offsets, sizes, specs, room, alignment=4)
        same_as_composed(got, host, composed(torch, blob, offsets, sizes, specs, room, alignment=4, refused=[12]))
        for at in bad:
            assert got.errcs[at] != 0 and got.sizes[at] == 0 and got.offsets[at + 1] == got.offsets[at], at
            assert bytes(got.params[at]) == bytes(batch.CodecParams()), at
        assert got.errcs[12] == INVALID_OPERATION and got.errcs[hp1] == INVALID_ARGUMENT_COLOR_TRANSFORMATION
        assert got.sizes[hp1] == 0 and got.params[hp1].near_lossless == 1  # (what the encoder was handed and refused)
        # every other frame's bytes are those of the batch without the failing frames
        assert np.delete(got.sizes, failing).tolist() == clean.sizes.tolist()
        assert np.delete(got.offsets[:-1], failing).tolist() == clean.offsets[:-1].tolist() and got.offsets[-1] == clean.offsets[-1]
        assert (host == clean_host).all()
    assert capi.transcode_counters()[2] - before[2] == 2  # (the frame that names a table, refused in either run)


# ---- 5: the capacity ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window", [None, 2, 4])
def test_the_capacity_rule(torch, base, knobs, window):
    streams = [x.jls for x in base]
    blob, offsets, sizes = blob_of(torch, streams)
    spec = capi.transcode_spec(restart_interval=16)
    room = room_for(streams, 16)
    full, full_host = transcode(torch, blob, offsets, sizes, spec, room, alignment=16)
    assert (full.errcs == 0).all()
    if window:  # (k = 7 is the last frame of a window of 2 ... and of 4: the frames behind it lie in later windows)
        knobs.set("TRANSCODE_WINDOW_FRAMES", window)
    for k in (7, 8):
        capacity = int(full.offsets[k]) + int(full.sizes[k]) - 1  # inside frame k
        before = capi.transcode_counters()
        got, host = transcode(torch, blob, offsets, sizes, spec, room, alignment=16, capacity=capacity)
        after = capi.transcode_counters()
        assert (got.errcs[:k] == 0).all() and got.sizes[:k].tolist() == full.sizes[:k].tolist()
        assert got.offsets[:k + 1].tolist() == full.offsets[:k + 1].tolist()
        assert (got.errcs[k:] == DESTINATION_TOO_SMALL).all() and (got.sizes[k:] == 0).all()
        assert (got.offsets[k:] == full.offsets[k]).all()
        assert after[3] - before[3] == len(base) - k - 1 and after[0] - before[0] == k
        for f in range(len(base)):  # (what a frame would have been coded with is reported all the same)
            assert bytes(got.params[f]) == bytes(full.params[f]), f
        end = int(full.offsets[k])
        assert (host[:end] == full_host[:end]).all()  # the frames that fit, and the zeroed gaps between them
        assert (host[end:] == CANARY).all()           # nothing of frame k or behind it; the canary from the capacity on survives
        same_as_composed(got, host, composed(torch, blob, offsets, sizes, spec, room, alignment=16, capacity=capacity))
    # a capacity that ends inside the zeroed gap behind frame k: the zeros stop there
    k = next(f for f in range(len(base) - 1) if int(full.offsets[f + 1]) - int(full.offsets[f]) - int(full.sizes[f]) >= 2)
    end = int(full.offsets[k]) + int(full.sizes[k])
    got, host = transcode(torch, blob, offsets, sizes, spec, room, alignment=16, capacity=end + 1)
    assert (got.errcs[:k + 1] == 0).all() and (got.errcs[k + 1:] == DESTINATION_TOO_SMALL).all()
    assert (host[:end] == full_host[:end]).all() and host[end] == 0 and (host[end + 1:] == CANARY).all()


# ---- 6: the work area -----------------------------------------------------------------------------------------------------------------

def test_the_frames_are_a_work_area(torch, base, knobs):
    streams = [x.jls for x in base]
    blob, offsets, sizes = blob_of(torch, streams)
    spec = capi.transcode_spec(restart_interval=8)
    room = room_for(streams, 1)
    frames = [x.g.packed for x in base]
    batch.release_work_areas()
    assert batch.work_area_bytes() == 0
    limit = 256 << 20
    try:
        batch.set_workspace_limit(limit)
        want, want_host = transcode(torch, blob, offsets, sizes, spec, room)
        whole = batch.work_area_bytes()
        assert sum(frames) <= whole <= limit  # (the decoded frames of the one window are part of it)
        batch.release_work_areas()
        assert batch.work_area_bytes() == 0
        knobs.set("TRANSCODE_WINDOW_FRAMES", 1)  # the area holds one frame at a time: smaller by the other twelve, at least
        got, host = transcode(torch, blob, offsets, sizes, spec, room)
        assert (host == want_host).all()
        assert 0 < batch.work_area_bytes() <= whole - (sum(frames) - max(frames) - 13 * 256)
        batch.release_work_areas()
        assert batch.work_area_bytes() == 0
        knobs.clear("TRANSCODE_WINDOW_FRAMES")
        batch.set_workspace_limit(max(frames) - 1)  # below the largest frame
        dst = canary_buffer(torch, room)
        with pytest.raises(capi.JpegLSError) as e:
            batch.transcode_batch(blob, offsets, sizes, spec, dst)
        assert e.value.errc == NOT_ENOUGH_MEMORY
        torch.cuda.synchronize()
        assert (dst.cpu().numpy() == CANARY).all()
    finally:
        batch.set_workspace_limit(0)
        batch.release_work_areas()


# ---- 7: the host form -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["pageable", "host_alloc"])
def test_the_host_form_equals_the_device_call(torch, base, knobs, kind):
    streams = [x.jls for x in base] + [b"\xff\xd8garbage"]
    blob, offsets, sizes = blob_of(torch, streams)
    specs = [SPECS[("restart8", "near2", "nothing", "restart16")[f % 4]]() for f in range(len(streams))]
    room = room_for(streams, 16)
    want, want_host = transcode(torch, blob, offsets, sizes, specs, room, alignment=16)
    cut = int(want.offsets[9]) + 5  # (inside frame 9)
    short, short_host = transcode(torch, blob, offsets, sizes, specs, room, alignment=16, capacity=cut)

    def arena(nbytes):
        raw = batch.host_alloc(nbytes + 64) if kind == "host_alloc" else np.empty(nbytes + 64, dtype=np.uint8)
        raw[:] = CANARY
        return raw

    source = arena(blob.numel() + 1)
    source[1:1 + blob.numel()] = blob.cpu().numpy()  # the blob at an odd base
    pristine = source.copy()
    for window in (None, 1, 4):
        if window:
            knobs.set("HOST_WINDOW_FRAMES", window)
        for expect, expect_host, capacity in ((want, want_host, None), (short, short_host, cut)):
            out = arena(room + 3)
            got = batch.transcode_batch_host(source[1:1 + blob.numel()], offsets, sizes, specs, out[3:3 + room], alignment=16, capacity=capacity)
            assert got.offsets.tolist() == expect.offsets.tolist() and got.sizes.tolist() == expect.sizes.tolist(), window
            assert got.errcs.tolist() == expect.errcs.tolist(), window
            assert all(bytes(got.params[f]) == bytes(expect.params[f]) for f in range(len(streams))), window
            assert (out[3:3 + room] == expect_host).all(), window
            assert (out[:3] == CANARY).all() and (out[3 + room:] == CANARY).all()
        assert (source == pristine).all()  # the input is only read


# ---- 8: the point of it -------------------------------------------------------------------------------------------------------------------

def test_a_recoded_stream_can_be_salvaged(torch, base, lib):
    x = next(x for x in base if x.kind == "gray8_48x64")
    blob, offsets, sizes = blob_of(torch, [x.jls])
    got, host = transcode(torch, blob, offsets, sizes, capi.transcode_spec(restart_interval=8), room_for([x.jls], 1))
    assert got.errcs[0] == 0
    recoded = streams_of(got, host)[0]
    marks = [i for i in range(len(recoded) - 1) if recoded[i] == 0xFF and 0xD0 <= recoded[i + 1] <= 0xD7]
    assert len(marks) == 64 // 8 - 1

    def damage(stream, at):
        out = bytearray(stream)
        assert all(out[at:at + 4])  # (four bytes that are not zero yet)
        out[at:at + 4] = bytes(4)
        return bytes(out)

    def first_without_zeros(stream, lo, hi):
        return next(i for i in range((lo + hi) // 2, hi - 4) if all(stream[i:i + 4]))

    # interval 3 of the re-coded stream: the piece between markers 2 and 3
    hurt = damage(recoded, first_without_zeros(recoded, marks[2] + 2, marks[3]))
    old = damage(x.jls, first_without_zeros(x.jls, len(x.jls) // 4, len(x.jls) - 8))
    fill = 0x5B
    for stream, state in ((hurt, 1), (old, 2)):
        packed, o, n = blob_of(torch, [stream], lead=0)
        out = canary_buffer(torch, x.g.packed)
        report = batch.decode_batch_salvage(packed, o, n, [out], fill, lib=lib)
        torch.cuda.synchronize()
        assert report.errcs[0] != 0 and report.reports[0].state == state
        if state == 1:  # only the damaged interval is lost
            r = report.reports[0]
            assert (r.intervals, r.intervals_lost, r.rows_lost, r.first_lost_row) == (8, 1, 8, 24)
            want = np.frombuffer(x.pixels, dtype=np.uint8).reshape(64, 48).copy()
            want[24:32] = fill
            assert out.cpu().numpy().tobytes() == want.tobytes()
