"""The stuffing corpus (tests/stuffing.py) on every coding route of the MI355X: streams with a 0xFF in every second to fourth
byte -- eight stuffed bits in a 16-byte lane, a 0xFF as the last byte of a lane and of a chunk, as the first coded byte and as the
last data byte -- where the other GPU tests' streams have one in 256.  tests/test_stuffing_census_cpu.py asserts from the
oracle's bytes that the corpus reaches these cases.

Routes are forced or confirmed as tests/test_gpu_corners.py does it: a knob, a counter, or a geometry that admits one route only.
The frames of one geometry are ONE batch in the corpus' order, which puts the dense frames between their partners (`synth` noise,
a gradient, a flat frame whose scan ends while its neighbours are in mid-stream) in the lane groups of one wavefront.

Everything is compared for equality with the oracle: encoded bytes, decoded pixels, errc 0.  GPU only."""
import numpy as np
import pytest

import oracle_bind as ob
import salvage_index_model as sim
import salvage_model as sm
import strided as S
import stuffing as st
from charls_amd import batch, capi
from test_gpu_corners import FORCED, geometry, lib, packed, retries, tile_jobs, torch  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CORPUS = st.CORPUS
TOO_SMALL = 3


def cases(route, by="geometry", keep=None, dense=False):
    names = [n for n in st.route_frames(route, dense=dense) if keep is None or keep(CORPUS[n])]
    return [pytest.param(v, id=st.batch_id(k)) for k, v in st.batches(names, by).items()]


def decode(torch, lib, names, streams=None, pixels=None):
    """The frames `names` (one geometry) decoded as ONE batch into a canary arena; returns the rise of exact_retry_scans."""
    coded = [st.coded(n) for n in names]
    lay = packed(geometry(coded[0].corner), len(names))
    before = retries()
    rc, errcs, arena = S.decode_batch(torch, lib, streams or [c.jls for c in coded], lay)
    rise = retries() - before
    assert rc == 0 and not errcs.any(), (rc, dict(zip(names, errcs.tolist())))
    lay.check(arena, pixels or [c.pixels for c in coded])
    return rise


def encode(torch, lib, names):
    """The frames `names` (one geometry, one set of coding parameters) coded as ONE batch: the oracle's bytes.  Returns the
    rise of the tile pipeline's job counter."""
    coded = [st.coded(n) for n in names]
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


def to_device(torch, streams, front=0):
    """The streams back to back in one device buffer, `front` bytes before the first: (blob, offsets, sizes)."""
    sizes = np.array([len(s) for s in streams], dtype=np.uint64)
    offsets = (front + np.concatenate([[0], np.cumsum(sizes)])).astype(np.uint64)
    blob = np.frombuffer(bytes(front) + b"".join(streams) + bytes(16), dtype=np.uint8).copy()
    return torch.from_numpy(blob).cuda(), offsets, sizes


# ---- decode ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", [8, 16, 32])
@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("names", cases("group_decode", by="thresholds"))
def test_group_decoder(torch, lib, knobs, group, waves, names):
    """scan_group_decode.hip: refill's delete loop makes eight trips in the lanes of a dense scan while the lanes of its partners
    make none, and a flat partner's scan ends while its neighbours are in mid-stream.  Valid streams: none leaves the group
    decoder for the exact one."""
    knobs.set("DECODE_GROUP", group)
    knobs.set("DECODE_WORKGROUP_WAVES", waves)
    assert decode(torch, lib, names) == 0, "a valid stream of the corpus left the group decoder"


@pytest.mark.parametrize("names", cases("fast_decode"))
def test_fast_decoder(torch, lib, knobs, names):
    """DECODE_GROUP = 0: DenseBits::refill of scan_fast_decode.hip, chunks of 1024 bytes."""
    knobs.set("DECODE_GROUP", 0)
    assert decode(torch, lib, names) == 0


@pytest.mark.parametrize("names", cases("exact_decode"))
def test_exact_decoder(torch, lib, knobs, names):
    knobs.set("EXACT_DECODER", 1)
    decode(torch, lib, names)


@pytest.mark.parametrize("names", cases("serial_decode"))
def test_serial_decoder(torch, lib, names):
    """RESET = 256: wave_decode_eligible() says no."""
    decode(torch, lib, names)


@pytest.mark.parametrize("group", [8, 16, 32])
@pytest.mark.parametrize("names", cases("pixel_decode", by="thresholds", keep=lambda c: c.ilv == 2))
def test_pixel_decoder_sample_interleaved(torch, lib, knobs, group, names):
    knobs.set("DECODE_GROUP", group)
    assert decode(torch, lib, names) == 0


@pytest.mark.parametrize("group", [8, 32])
@pytest.mark.parametrize("names", cases("pixel_decode", by="thresholds", keep=lambda c: c.ilv != 2))
def test_pixel_decoder_near_lossless(torch, lib, knobs, group, names):
    knobs.set("NEAR_DECODE_PIXELS", 1)
    knobs.set("DECODE_GROUP", group)
    assert decode(torch, lib, names) == 0


# ---- alignment ------------------------------------------------------------------------------------------------------------------

ALIGNED = [pytest.param(v, id=st.batch_id(k)) for k, v in st.batches(
    [n for n in st.DENSE if CORPUS[n].comps == 1 and CORPUS[n].near == 0 and CORPUS[n].preset is None and CORPUS[n].bits in (8, 16)]).items()]


@pytest.mark.parametrize("group", [0, 8, 32])
@pytest.mark.parametrize("names", ALIGNED)
def test_every_residue_of_the_first_coded_byte(torch, lib, knobs, group, names):
    """The packed decode call with an offset table that puts the first entropy-coded byte of every dense gray frame (8 and 16
    bit) on each of the 16 residues of a device address, (base + offset + data_start) % 16; into a canary arena."""
    knobs.set("DECODE_GROUP", group)
    coded = [st.coded(n) for n in names for _ in range(16)]
    pieces, offsets, at = [], [], 0
    for i, c in enumerate(coded):
        gap = (i % 16 - (at + c.scans[0].data_start)) % 16
        pieces.append(bytes(gap) + c.jls)
        offsets.append(at + gap)
        at += gap + len(c.jls)
    blob = torch.from_numpy(np.frombuffer(b"".join(pieces) + bytes(16), dtype=np.uint8).copy()).cuda()
    assert blob.data_ptr() % 16 == 0
    residues = {(n, (blob.data_ptr() + o + c.scans[0].data_start) % 16) for n, o, c in zip([x.corner.name for x in coded], offsets, coded)}
    assert residues == {(n, r) for n in names for r in range(16)}
    lay = packed(geometry(coded[0].corner), len(coded))
    arena = torch.from_numpy(lay.blank().copy()).cuda()
    before = retries()
    _, errcs, _ = batch.decode_batch_packed(blob, offsets, [len(c.jls) for c in coded], arena[lay.first:], stride=lay.stride,
                                            frame_pitch=lay.pitch, lib=lib)
    torch.cuda.synchronize()
    assert not errcs.any() and retries() == before
    lay.check(arena.cpu().numpy(), [c.pixels for c in coded])


# ---- restart intervals ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lines", st.RESTART_LINES)
@pytest.mark.parametrize("name", st.RESTART_FRAMES)
def test_restart_intervals_both_ways(torch, lib, knobs, name, lines):
    """Intervals that end in FF xx, then FF D0+m: the encoder's intervals are the oracle's coding of each interval, the decoder
    gives the oracle's pixels interval-parallel and (SEQUENTIAL_INTERVALS = 1) with the scan left whole."""
    c = CORPUS[name]
    g = geometry(c)
    lay = packed(g, 1)
    rc, errcs, streams, _ = S.encode_batch(torch, lib, lay.pad([c.img]), lay, S.codec_params(g, c.near, c.ct, c.preset, restart=lines))
    assert rc == 0 and not errcs.any()
    want = st.dri_stream(name, lines)
    cont = st.jls_container.parse(streams[0])
    assert cont.restart_interval == lines and len(cont.scans) == 1
    assert streams[0][cont.scans[0].data_start:cont.scans[0].data_end] == st.dri_scan(name, lines)[0]
    assert ob.decode(streams[0])[1].tobytes() == st.dri_pixels(name, lines)
    knobs.set("DECODE_GROUP", 16)
    for sequential in (None, 1):
        if sequential:
            knobs.set("SEQUENTIAL_INTERVALS", 1)
        rc, errcs, out = S.decode_batch(torch, lib, [want], lay)
        assert rc == 0 and not errcs.any(), (sequential, errcs.tolist())
        lay.check(out, [st.dri_pixels(name, lines)])


# ---- index ----------------------------------------------------------------------------------------------------------------------

INDEXED = [(n, K) for n in st.SEEK_FLAT for K in (1, 7)] + [("ramp_8", 16), ("ramp_16_specks30", 16)]


@pytest.mark.parametrize("name,K", INDEXED)
def test_index_indexed_decode_and_row_band(torch, lib, name, K):
    """A seek point every line of a frame that costs a bit a line: the points stand inside 7-bit bytes.  The indexed decode and
    a row band that starts at such a point give the oracle's rows; the batch call builds part 1's index bytes."""
    c = st.coded(name)
    x = c.corner
    _, out, index = lib.decode_with_index(c.jls, K, 0)
    assert out.tobytes() == c.pixels
    before = capi.index_counters()["scans_from_points"]
    assert lib.decode_indexed(c.jls, index, 0)[1].tobytes() == c.pixels
    assert capi.index_counters()["scans_from_points"] > before
    row = x.width * (2 if x.bits > 8 else 1)
    rows = np.frombuffer(c.pixels, dtype=np.uint8).reshape(x.height, row)
    # the precondition, from the oracle's bytes and the saved reader states: point p, the state in front of row (p + 1) K, stands
    # inside a byte that follows a 0xFF (ramp_16_specks30, here for the sample width, has no such point among its five)
    view = sim.read_index(index)
    points = np.frombuffer(index, dtype=np.uint8)[sim.INDEX_HEADER + sim.INDEX_SCAN:]
    where = [st.current_byte(c.segments[0], p, v) for p, _, v in st.reader_states(points, view.point_bytes)]
    inside = [p for p, (b, phase) in enumerate(where) if phase and b and c.segments[0][b - 1] == 0xFF]
    assert inside or name == "ramp_16_specks30"
    bands = [((p + 1) * K, min(K + 2, x.height - (p + 1) * K)) for p in inside[:1]]
    for first, count in bands + [(K * 3, K + 2), (K * ((x.height - 1) // K), x.height - K * ((x.height - 1) // K)), (K * 2 + K // 2, 5)]:
        assert lib.decode_rows(c.jls, first, count, index=index).tobytes() == rows[first:first + count].tobytes(), (first, count)
    blob, offsets, sizes = to_device(torch, [c.jls], front=3)
    _, errcs, indexes = batch.index_batch_packed(blob, offsets, sizes, K, lib=lib)
    assert not errcs.any() and indexes[0] == index


# ---- salvage --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ramp_8", "ramp_8_specks100", "line3_8", "ramp_16_specks30"])
def test_salvage_with_restart_markers(torch, lib, name):
    """Four zero bytes in the middle of an interval of FF 7F FF 7F: that interval is lost, its neighbours -- whose last bytes
    are FF xx in front of the RSTm -- are kept."""
    import test_gpu_salvage as gs
    c = CORPUS[name]
    sound = sm.build(c.img, 16, bits=c.bits, comps=c.comps, ilv=c.ilv, near=c.near)
    damaged = st.zero_in_stretch(sound, 3)   # (asserts that the interval has an FF 7F FF 7F and puts the zeros over it)
    fill = 0x1C7 if c.bits > 8 else 0x5B
    exp = sm.expected(sound, damaged, fill)
    gs.check_preconditions(sound, damaged.assemble(), exp)
    blob, offsets, sizes = gs.pack(torch, [damaged.assemble()])
    out = gs.canary_out(torch, len(sound.pixels))
    got = batch.decode_batch_salvage(blob, offsets, sizes, [out], fill, status_pitch=exp.status.size, lib=lib)
    torch.cuda.synchronize()
    assert exp.report[2] > 0
    gs.check_one(exp, got, out.cpu().numpy().tobytes())


@pytest.mark.parametrize("name,K", [("ramp_8", 16), ("ramp_8_specks100", 16), ("line3_8", 16)])
def test_salvage_with_an_index(torch, lib, name, K):
    """The same damage in a stream without restart markers, salvaged through its seek points."""
    c = st.coded(name)
    x = c.corner
    _, out, index = lib.decode_with_index(c.jls, lines_per_seek_point=K)
    s = sim.sound(c.jls, index)
    assert out.tobytes() == s.pixels == c.pixels
    # sim.zero4 with the place chosen: the FF 7F FF 7F nearest the middle of interval 1, inside zero4's margins
    lo, hi = sim._room(s, 0, 1, 4)
    at = st.stretch_near_middle(s.jls, lo, hi + 4)
    assert lo <= at <= hi and s.jls[at:at + 4] == st.STRETCH
    raw = sim._blank(s)
    raw[0, 1] = sim.LOST
    d = sim.Damaged(s.jls[:at] + bytes(4) + s.jls[at + 4:], raw)
    fill = 0x5B
    exp = sim.expected_index(s, d.raw, fill)
    lay = S.layout(geometry(x), "p13", 1, 1, tight=True)
    blob, offsets, sizes = to_device(torch, [d.data])
    arena = torch.from_numpy(lay.blank().copy()).cuda()
    got = batch.decode_batch_salvage_indexed(blob, offsets, sizes, [arena[lay.first:]], [index], fill, strides=[lay.stride],
                                             capacities=[lay.need], status_pitch=s.scans * s.intervals, lib=lib)
    torch.cuda.synchronize()
    assert int(got.errcs[0]) != 0
    assert got.status[0].tolist() == exp.status.reshape(-1).tolist()
    assert got.reports[0].astuple() == exp.report and exp.report[2] > 0
    lay.check(arena.cpu().numpy(), [exp.pixels], what="salvaged through the index")


# ---- encode ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("names", cases("tile_encode", by="parameters", dense=True))
def test_tile_pipeline_default_knobs(torch, lib, names):
    assert encode(torch, lib, names) > 0, "not coded by the tile pipeline"


@pytest.mark.parametrize("how", ["forced_small_jobs", "speculative_stage_e"])
@pytest.mark.parametrize("names", cases("tile_encode", by="parameters", dense=True))
def test_tile_pipeline_forced(torch, lib, knobs, how, names):
    """Jobs of 32 events without warm-up; stage E in its speculative form (passes of more than 8 scans: the batch is repeated to
    12 frames) with chunks of 64 bytes and no warm-up: the raw bits of a ramp are ones, a stuffed bit in every second byte, and
    every guess of a chunk's entry state is checked."""
    if how == "forced_small_jobs":
        for k, v in FORCED.items():
            knobs.set(k, v)
    else:
        knobs.set("SPEC_CHUNK", 64)
        knobs.set("SPEC_WARM", 0)
        names = (names * 12)[:12]
    assert encode(torch, lib, names) > 0, "not coded by the tile pipeline"


@pytest.mark.parametrize("names", cases("group_encode", by="parameters", dense=True))
def test_group_encoder_and_measured_sizes(torch, lib, names):
    """scan_group_encode.hip's RingWriter; the measuring form counts the stuffed bits: the oracle's sizes exactly."""
    assert encode(torch, lib, names) == 0
    cs = [CORPUS[n] for n in names]
    c = cs[0]
    frames = torch.from_numpy(np.stack([np.frombuffer(x.img.tobytes(), dtype=np.uint8) for x in cs])).cuda()
    sizes = batch.measure_batch(frames, [c.near], bits_per_sample=c.bits, component_count=c.comps, interleave_mode=c.ilv,
                                color_transformation=c.ct, preset=c.preset or (0, 0, 0, 0, 0), width=c.width, height=c.height, lib=lib)
    assert sizes[:, 0].tolist() == [len(st.coded(n).jls) for n in names]


@pytest.mark.parametrize("name", [n for n, c in CORPUS.items() if c.near and c.preset == st.RESET256])
def test_near_lossless_reset_256_is_the_serial_encoder_s(torch, lib, name):
    """RESET = 256 is stored as 0: N never halves and outgrows the 8 bits the group encoder's packed contexts keep it in
    (encode_launch.hip, group_encode_lanes).  Found by this corpus: a ramp puts thousands of samples into one context.  The
    default engine codes the oracle's bytes, and measures the oracle's size."""
    assert encode(torch, lib, [name]) == 0
    c = CORPUS[name]
    frames = torch.from_numpy(np.frombuffer(c.img.tobytes(), dtype=np.uint8).copy()[None]).cuda()
    sizes = batch.measure_batch(frames, [c.near], bits_per_sample=c.bits, preset=c.preset, width=c.width, height=c.height, lib=lib)
    assert sizes[:, 0].tolist() == [len(st.coded(name).jls)]


@pytest.mark.parametrize("names", cases("serial_encode", by="parameters", dense=True))
def test_serial_encoder(torch, lib, names):
    batch.set_encode_engine(1, lib)
    try:
        rise = encode(torch, lib, names)
    finally:
        batch.set_encode_engine(0, lib)
    assert rise == 0


@pytest.mark.parametrize("name", ["ramp_8", "ramp_8_specks100", "flat_1x600_zeros", "flat_2x597_255", "flat_16x595_near2", "ramp_8n_near3",
                                  "ramp_16_specks30", "sample3_8_specks10"])
def test_capacity_verdicts_are_the_oracle_s(lib, name):
    """A destination one byte shorter than the stream is destination_too_small.  From the exact length on the verdict is the
    reference's, which wants four free bytes at every flush of its writer (the oracle is pinned to it,
    tests/test_oracle_vs_reference.py): for most of these frames it refuses the exact length too.  Size by size the product
    says what the oracle says, and where both succeed the bytes are the oracle's."""
    c = st.coded(name)
    x = c.corner
    for size in range(len(c.jls) - 1, len(c.jls) + 6):
        verdicts = []
        for codec, error in ((ob, ob.OracleError), (lib, capi.JpegLSError)):
            try:
                verdicts.append((0, codec.encode(x.img, destination_size=size, **x.kw())))
            except error as e:
                verdicts.append((e.errc, None))
        assert verdicts[0] == verdicts[1], (name, size - len(c.jls), verdicts[0][0], verdicts[1][0])
        if size < len(c.jls):
            assert verdicts[1][0] == TOO_SMALL
    assert verdicts[1] == (0, c.jls)


# ---- mixed ----------------------------------------------------------------------------------------------------------------------

def test_one_ragged_call_each_way_over_all_geometries(torch, lib):
    """Every lossless frame of the corpus with the default parameters in ONE ragged encode, every frame in ONE ragged decode."""
    names = list(CORPUS)
    coded = [st.coded(n) for n in names]
    blob, offsets, sizes = to_device(torch, [c.jls for c in coded], front=5)
    outs = [torch.full((len(c.pixels),), 0xA5, dtype=torch.uint8, device="cuda:0") for c in coded]
    _, errcs, _ = batch.decode_batch_ragged(blob, offsets, sizes, outs, lib=lib)
    torch.cuda.synchronize()
    assert not errcs.any(), dict(zip(names, errcs.tolist()))
    for n, c, o in zip(names, coded, outs):
        assert o.cpu().numpy().tobytes() == c.pixels, n
    frames, params = [], []
    for c in coded:
        x = c.corner
        a = np.ascontiguousarray(x.img)
        frames.append(torch.from_numpy(a.view(np.int16) if x.bits > 8 else a).cuda())
        params.append(batch.codec_params(x.width, x.height, x.bits, x.comps, x.ilv, x.near, color_transformation=x.ct,
                                         preset=x.preset or (0, 0, 0, 0, 0)))
    room = torch.full((sum(8 * c.corner.img.nbytes + 4096 for c in coded),), 0xA5, dtype=torch.uint8, device="cuda:0")
    enc = batch.encode_batch_ragged(frames, params, room, lib=lib)
    torch.cuda.synchronize()
    assert not enc.errcs.any(), dict(zip(names, enc.errcs.tolist()))
    host = room.cpu().numpy()
    for f, (n, c) in enumerate(zip(names, coded)):
        assert host[int(enc.offsets[f]):int(enc.offsets[f]) + int(enc.sizes[f])].tobytes() == c.jls, n


def test_transcode_adds_restart_intervals_to_dense_streams(torch, lib):
    """One call re-codes the dense streams with a restart interval of 7 lines: the oracle's intervals, RSTm between them."""
    names = [n for n in st.RESTART_FRAMES if CORPUS[n].near == 0]   # (a near-lossless stream is re-coded from its own pixels)
    blob, offsets, sizes = to_device(torch, [st.coded(n).jls for n in names])
    room = torch.zeros(2 * int(offsets[-1]) + 65536, dtype=torch.uint8, device="cuda:0")
    got = batch.transcode_batch(blob, offsets[:-1], sizes, capi.transcode_spec(restart_interval=7), room, lib=lib)
    torch.cuda.synchronize()
    assert not got.errcs.any(), dict(zip(names, got.errcs.tolist()))
    host = room.cpu().numpy()
    for f, n in enumerate(names):
        assert host[int(got.offsets[f]):int(got.offsets[f]) + int(got.sizes[f])].tobytes() == st.dri_stream(n, 7), n


@pytest.mark.parametrize("name", list(CORPUS))
def test_part1_abi(lib, name):
    """charls_jpegls_encoder / charls_jpegls_decoder on every frame of the corpus."""
    c = st.coded(name)
    assert lib.encode(c.corner.img, destination_size=8 * c.corner.img.nbytes + 4096, **c.corner.kw()) == c.jls
    assert lib.decode(c.jls)[1].tobytes() == c.pixels
