"""Re-coding a packed blob to byte budgets (charls_amd.h part 2k) on the GPU.  The contract is a composition, so the call is held,
byte for byte and table for table, to charls_amd_decode_batch_device_ragged + charls_amd_encode_batch_device_ragged_budget of
the same build; and, independently, to the model: the oracle's decode of every source, the oracle's coding of those pixels at
every candidate, the selection rule (tests/budget_model.py).  Then its own windows, the capacity rule across a window boundary,
the host form and the counters.  Sources are oracle streams of the frame kinds of tests/budget_model.py plus a near-lossless
one, one with SPIFF and comment segments, one that names a mapping table, a truncated one and an abbreviated table-only one.
Every output buffer is filled with a canary first.  All frames are tiny.  GPU only."""
import numpy as np
import pytest

import budget_model as bm
import oracle_bind as ob
import test_gpu_markers as markers
import test_gpu_transcode as plain
from charls_amd import batch, capi

pytestmark = pytest.mark.gpu

CANARY = 0xA5
DESTINATION_TOO_SMALL, INVALID_OPERATION = 3, 100
CANDIDATES = bm.NARROW
ROOM = 1 << 17


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


class Source:
    """One input stream.  `kind` and `pixels`: what the model re-codes (None: the frame is not coded, or only the composition
    says how); `restart`: the restart interval the stream announces."""

    def __init__(self, name, jls, kind=None, pixels=None, restart=0):
        self.name, self.jls, self.kind, self.pixels, self.restart = name, jls, kind, pixels, restart


_sources = []


@pytest.fixture(scope="module")
def sources(lib):
    if not _sources:
        for kind in bm.KINDS:  # lossless: the stream decodes to the image
            _sources.append(Source(kind, bm.oracle_stream(kind, 0, 0), kind, bm.image(kind, 0), bm.KINDS[kind][7]))
        near2 = bm.oracle_stream("gray8_33x17", 1, 2)
        _sources.append(Source("near2", near2, "gray8_33x17", ob.decode(near2)[1].reshape(17, 33)))
        img = bm.image("gray8_33x17", 2)
        rc, spiff = markers._encode_session(lib, img, bits=8, comps=1, ilv=0, near=0, xform=0, options=0, table_id=0, spiff="standard")
        assert b"SPIFF" in spiff and b"\xff\xfe" in spiff
        _sources.append(Source("spiff_and_comments", spiff, "gray8_33x17", img))
        gray = bm.oracle_stream("gray8_33x17", 0, 0)
        _sources.append(Source("names_a_table", plain.names_a_table(gray)))
        _sources.append(Source("truncated", gray[:len(gray) // 2]))
        _sources.append(Source("table_only", b"\xff\xd8" + b"\xff\xf8\x00\x09\x02\x01\x01\x00\x01\x02\x03" + b"\xff\xd9"))
    return _sources


def recoded(source, near, restart=None):
    """The model's stream of a source re-coded at `near`: the oracle's coding of the pixels the source decodes to, with the
    parameters of the stream (encoding options are not part of a stream) and the restart interval it announces, or `restart`."""
    w, h, bits, comps, ilv, ct = bm.KINDS[source.kind][:6]
    interval = source.restart if restart is None else restart
    kw = dict(bits_per_sample=bits, component_count=comps, interleave_mode=ilv, color_transformation=ct, near_lossless=near)
    if interval == 0:
        return ob.encode(source.pixels, width=w, height=h, **kw)
    return bm.dri_stream(source.pixels, w, h, kw, interval)


def modelled(source, candidates, restart=None):
    """Whether the model says what the frame becomes: it is coded, no candidate is refused, and the builder of streams with
    restart intervals can put it together (single-scan frames)."""
    if source.kind is None or bm.refusal(source.kind, candidates):
        return False
    interval = source.restart if restart is None else restart
    return interval == 0 or bm.KINDS[source.kind][3] == 1 or bm.KINDS[source.kind][4] != 0


def budgets_for(sources, candidates, restart=None):
    """Budgets taken from the model's sizes, by position: the size at the first candidate, the size at candidate 1, that size
    less one byte, 0, 2^63; plenty where the model has no sizes."""
    out = []
    for at, s in enumerate(sources):
        if not modelled(s, candidates, restart):
            out.append(1 << 20)
            continue
        sizes = [len(recoded(s, near, restart)) for near in candidates]
        out.append((sizes[0], sizes[1], sizes[1] - 1, 0, 1 << 63)[at % 5])
    return np.array(out, dtype=np.uint64)


def canary_buffer(torch, nbytes=ROOM):
    return torch.full((nbytes,), CANARY, dtype=torch.uint8, device="cuda:0")


def transcode(torch, blob, offsets, sizes, specs, budgets, candidates, *, room=ROOM, alignment=1, capacity=None):
    dst = canary_buffer(torch, room)
    got, nears = batch.transcode_batch_budget(blob, offsets, sizes, specs, budgets, candidates, dst, alignment=alignment, capacity=capacity)
    torch.cuda.synchronize()
    return got, nears, dst.cpu().numpy()


def composed(torch, blob, offsets, sizes, specs, budgets, candidates, *, room=ROOM, alignment=1, capacity=None, refused=()):
    """What the caller-side glue gives: probe, ragged decode into packed frames of the caller's own, ragged budget encode of the
    frames that decoded -- (offsets, sizes, errcs, nears, params as bytes, the output buffer on the host).  `refused`: frames that
    name a mapping table, which the glue cannot see and the call refuses."""
    count = len(sizes)
    specs = plain.spec_list(specs, count)
    probed, frame_bytes, probe_errcs = batch.probe_packed(blob, offsets, sizes)
    outs = [canary_buffer(torch, max(int(n), 1)) for n in frame_bytes]
    params, errcs, _ = batch.decode_batch_ragged(blob, offsets, sizes, outs, capacities=[int(n) for n in frame_bytes])
    errcs = errcs.copy()
    for f in refused:
        assert errcs[f] == 0
        errcs[f] = INVALID_OPERATION
    sent = [f for f in range(count) if errcs[f] == 0]
    coded_with = {f: plain.with_spec(params[f], specs[f]) for f in sent}
    dst = canary_buffer(torch, room)
    enc, chosen = batch.encode_batch_ragged_budget([outs[f] for f in sent], [coded_with[f] for f in sent], budgets[sent], candidates, dst,
                                                   alignment=alignment, capacity=capacity, strides=[0] * len(sent))
    torch.cuda.synchronize()
    offsets_out, sizes_out = np.zeros(count + 1, dtype=np.uint64), np.zeros(count, dtype=np.uint64)
    nears = np.full(count, -1, dtype=np.int32)
    params_out = [bytes(batch.CodecParams())] * count
    at = len(sent)
    offsets_out[count] = enc.offsets[at]
    for f in reversed(range(count)):  # (a frame that was not sent stands where the next one that was starts)
        if errcs[f] == 0:
            at -= 1
            sizes_out[f], errcs[f], nears[f] = enc.sizes[at], enc.errcs[at], chosen[at]
            if chosen[at] >= 0:
                coded_with[f].near_lossless = int(chosen[at])
            params_out[f] = bytes(coded_with[f])
        offsets_out[f] = enc.offsets[at]
    if capacity is not None:  # the rule of part 2j: every frame behind the one that met the capacity, decoded or not
        assert (budgets[sent] == 1 << 63).all()  # (so that destination_too_small among the frames sent is the capacity's)
        beyond = next((f for f in sent if errcs[f] == DESTINATION_TOO_SMALL), count)
        for f in range(beyond + 1, count):
            errcs[f], sizes_out[f], nears[f] = DESTINATION_TOO_SMALL, 0, -1
            readable = probe_errcs[f] == 0 and frame_bytes[f] != 0
            params_out[f] = bytes(plain.with_spec(probed[f], specs[f])) if readable else bytes(batch.CodecParams())
    return offsets_out, sizes_out, errcs, nears, params_out, dst.cpu().numpy()


def same_as_composed(got, nears, host, want):
    offsets, sizes, errcs, want_nears, params, want_host = want
    assert got.offsets.tolist() == offsets.tolist()
    assert got.sizes.tolist() == sizes.tolist()
    assert got.errcs.tolist() == errcs.tolist()
    assert nears.tolist() == want_nears.tolist()
    for f in range(len(sizes)):
        assert bytes(got.params[f]) == params[f], f
    bad = np.flatnonzero(host != want_host)
    assert bad.size == 0, f"{bad.size} bytes differ, the first at {int(bad[0])}"


def table_frames(sources):
    return [f for f, s in enumerate(sources) if s.name == "names_a_table"]


# ---- 1: the composition ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alignment", [1, 16, 4096])
def test_the_call_is_the_composition(torch, sources, alignment):
    blob, offsets, sizes = plain.blob_of(torch, [s.jls for s in sources])
    room = ROOM if alignment < 4096 else 24 * 4096
    for specs in (capi.transcode_spec(), [capi.transcode_spec(restart_interval=(0, 4, 100)[f % 3]) for f in range(len(sources))]):
        budgets = budgets_for(sources, CANDIDATES)
        got, nears, host = transcode(torch, blob, offsets, sizes, specs, budgets, CANDIDATES, room=room, alignment=alignment)
        same_as_composed(got, nears, host, composed(torch, blob, offsets, sizes, specs, budgets, CANDIDATES, room=room, alignment=alignment,
                                                    refused=table_frames(sources)))
        assert (host[int(got.offsets[-1]):] == CANARY).all()
        for f, s in enumerate(sources):
            assert (got.errcs[f] == 0) == (nears[f] >= 0) == (got.sizes[f] != 0), (f, s.name)
            if nears[f] >= 0:  # params_out is what the frame was coded with
                assert got.params[f].near_lossless == nears[f], (f, s.name)
        by_name = {s.name: f for f, s in enumerate(sources)}
        assert got.errcs[by_name["names_a_table"]] == INVALID_OPERATION
        assert got.errcs[by_name["rgb_sample_hp1_16x8"]] == bm.INVALID_ARGUMENT_COLOR_TRANSFORMATION  # (with any NEAR above 0)
        assert got.params[by_name["rgb_sample_hp1_16x8"]].color_transformation == 1  # the source's parameters with the spec
        assert got.errcs[by_name["truncated"]] not in (0, DESTINATION_TOO_SMALL)
        assert bytes(got.params[by_name["truncated"]]) == bytes(batch.CodecParams())
        assert got.errcs[by_name["table_only"]] != 0 and got.sizes[by_name["table_only"]] == 0


# ---- 2: the model ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("restart", [None, 4])
def test_the_call_against_the_model(torch, sources, restart):
    """None: the restart interval of every source stays; 4: the specs add one, and the streams are the builder's."""
    blob, offsets, sizes = plain.blob_of(torch, [s.jls for s in sources])
    spec = capi.transcode_spec() if restart is None else capi.transcode_spec(restart_interval=restart)
    budgets = budgets_for(sources, CANDIDATES, restart)
    got, nears, host = transcode(torch, blob, offsets, sizes, spec, budgets, CANDIDATES, alignment=2)
    outcomes = set()
    for f, s in enumerate(sources):
        if not modelled(s, CANDIDATES, restart):
            continue
        streams = [recoded(s, near, restart) for near in CANDIDATES]
        k = bm.choose([len(x) for x in streams], budgets[f])
        outcomes.add(min(k, 1))
        at = int(got.offsets[f])
        if k < 0:
            assert (int(got.errcs[f]), int(nears[f]), int(got.sizes[f])) == (DESTINATION_TOO_SMALL, -1, 0), (f, s.name)
            assert int(got.offsets[f + 1]) == at
            continue
        assert (int(got.errcs[f]), int(nears[f]), int(got.sizes[f])) == (0, CANDIDATES[k], len(streams[k])), (f, s.name)
        assert host[at:at + len(streams[k])].tobytes() == streams[k], (f, s.name)
        assert got.params[f].restart_interval == (s.restart if restart is None else restart)
        if restart:
            assert (b"\xff\xd0" in streams[k]) == (bm.KINDS[s.kind][1] > restart)
    assert outcomes == {-1, 0, 1}
    assert sum(1 for s in sources if modelled(s, CANDIDATES, restart)) >= 9


def test_a_lossless_source_within_its_budget_comes_back(torch, sources):
    """Plain-container lossless sources, candidates (0, 1, 2), a budget at and above the source's size: byte for byte, NEAR 0."""
    kinds = ("gray8_33x17", "gray12_19x9", "gray16_65x5", "gray_1x1", "rgb_planar_16x8", "rgb_line_16x8", "rgb_sample_16x8")
    chosen = [s for s in sources if s.name in kinds]
    assert len(chosen) == len(kinds)
    blob, offsets, sizes = plain.blob_of(torch, [s.jls for s in chosen])
    budgets = np.array([len(s.jls) + (f % 2) * 100 for f, s in enumerate(chosen)], dtype=np.uint64)
    got, nears, host = transcode(torch, blob, offsets, sizes, capi.transcode_spec(), budgets, (0, 1, 2))
    assert (got.errcs == 0).all() and (nears == 0).all()
    assert plain.streams_of(got, host) == [s.jls for s in chosen]


# ---- 3: windows --------------------------------------------------------------------------------------------------------------

def test_windows_do_not_change_the_result(torch, sources, knobs):
    blob, offsets, sizes = plain.blob_of(torch, [s.jls for s in sources])
    budgets = budgets_for(sources, CANDIDATES)
    spec = capi.transcode_spec(restart_interval=4)
    count = len(sources)
    before = capi.transcode_counters()
    want, want_nears, want_host = transcode(torch, blob, offsets, sizes, spec, budgets, CANDIDATES, alignment=16)
    after = capi.transcode_counters()
    coded = int((want.errcs == 0).sum())
    assert [a - b for a, b in zip(after, before)] == [coded, 1, 1, 0]  # re-coded, one window, the table refusal, nothing behind
    for window in (1, 2, 5):
        knobs.set("TRANSCODE_WINDOW_FRAMES", window)
        before = capi.transcode_counters()
        got, nears, host = transcode(torch, blob, offsets, sizes, spec, budgets, CANDIDATES, alignment=16)
        after = capi.transcode_counters()
        assert [a - b for a, b in zip(after, before)] == [coded, -(-count // window), 1, 0], window
        assert got.offsets.tolist() == want.offsets.tolist() and got.sizes.tolist() == want.sizes.tolist(), window
        assert got.errcs.tolist() == want.errcs.tolist() and nears.tolist() == want_nears.tolist() and (host == want_host).all(), window
        assert all(bytes(got.params[f]) == bytes(want.params[f]) for f in range(count)), window
    knobs.clear("TRANSCODE_WINDOW_FRAMES")


def test_the_capacity_rule_across_a_window_boundary(torch, sources, knobs):
    blob, offsets, sizes = plain.blob_of(torch, [s.jls for s in sources])
    budgets = np.full(len(sources), 1 << 63, dtype=np.uint64)
    spec = capi.transcode_spec()
    full, full_nears, full_host = transcode(torch, blob, offsets, sizes, spec, budgets, CANDIDATES, alignment=16)
    count = len(sources)
    for window in (None, 4):  # (frame 3 is the last of a window of 4, frame 4 the first of the next)
        if window:
            knobs.set("TRANSCODE_WINDOW_FRAMES", window)
        for k in (3, 4):
            assert full.sizes[k] > 1
            capacity = int(full.offsets[k]) + int(full.sizes[k]) - 1
            before = capi.transcode_counters()
            got, nears, host = transcode(torch, blob, offsets, sizes, spec, budgets, CANDIDATES, alignment=16, capacity=capacity)
            after = capi.transcode_counters()
            assert got.errcs[:k].tolist() == full.errcs[:k].tolist() and got.sizes[:k].tolist() == full.sizes[:k].tolist()
            assert nears[:k].tolist() == full_nears[:k].tolist() and got.offsets[:k + 1].tolist() == full.offsets[:k + 1].tolist()
            assert (got.errcs[k:] == DESTINATION_TOO_SMALL).all() and (got.sizes[k:] == 0).all() and (nears[k:] == -1).all()
            assert (got.offsets[k:] == full.offsets[k]).all()
            assert after[3] - before[3] == count - k - 1 and after[0] - before[0] == int((full.errcs[:k] == 0).sum())
            end = int(full.offsets[k])
            assert (host[:end] == full_host[:end]).all() and (host[end:] == CANARY).all()
            same_as_composed(got, nears, host, composed(torch, blob, offsets, sizes, spec, budgets, CANDIDATES, alignment=16, capacity=capacity,
                                                        refused=table_frames(sources)))
    knobs.clear("TRANSCODE_WINDOW_FRAMES")


# ---- 4: the host form --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["pageable", "host_alloc"])
def test_the_host_form_equals_the_device_call(torch, sources, knobs, kind):
    blob, offsets, sizes = plain.blob_of(torch, [s.jls for s in sources])
    budgets = budgets_for(sources, CANDIDATES)
    specs = [capi.transcode_spec(restart_interval=(0, 4)[f % 2]) for f in range(len(sources))]
    room = 1 << 16
    want, want_nears, want_host = transcode(torch, blob, offsets, sizes, specs, budgets, CANDIDATES, room=room, alignment=16)
    cut = int(want.offsets[9]) + 5  # (inside frame 9)
    assert want.sizes[9] > 5
    short, short_nears, short_host = transcode(torch, blob, offsets, sizes, specs, budgets, CANDIDATES, room=room, alignment=16, capacity=cut)

    def arena(nbytes):
        raw = batch.host_alloc(nbytes + 64) if kind == "host_alloc" else np.empty(nbytes + 64, dtype=np.uint8)
        raw[:] = CANARY
        return raw

    source = arena(blob.numel() + 1)
    source[1:1 + blob.numel()] = blob.cpu().numpy()  # the blob at an odd base
    pristine = source.copy()
    for window in (None, 1, 3):
        if window:
            knobs.set("HOST_WINDOW_FRAMES", window)
        for expect, expect_nears, expect_host, capacity in ((want, want_nears, want_host, None), (short, short_nears, short_host, cut)):
            out = arena(room + 3)
            got, nears = batch.transcode_batch_host_budget(source[1:1 + blob.numel()], offsets, sizes, specs, budgets, CANDIDATES,
                                                           out[3:3 + room], alignment=16, capacity=capacity)
            assert got.offsets.tolist() == expect.offsets.tolist() and got.sizes.tolist() == expect.sizes.tolist(), window
            assert got.errcs.tolist() == expect.errcs.tolist() and nears.tolist() == expect_nears.tolist(), window
            assert all(bytes(got.params[f]) == bytes(expect.params[f]) for f in range(len(sources))), window
            assert (out[3:3 + room] == expect_host).all(), window
            assert (out[:3] == CANARY).all() and (out[3 + room:] == CANARY).all()
        assert (source == pristine).all()  # the input is only read
    knobs.clear("HOST_WINDOW_FRAMES")


def test_the_host_form_takes_streams_longer_than_the_estimated_size(torch, knobs):
    """Noise coded losslessly is longer than part 1's estimated destination size -- only at a size where 1/16 of the frame no
    longer covers it, hence 1536 x 1024 -- and the budget calls code it all the same: their slots follow the measured stream.
    The host form must give such frames the room too, several to a window and one alone (three frames in windows of two): it
    equals the device call.  Two re-codes of three chains of 1.5 MPix: 3 to 4 s."""
    from charls_amd import synth
    w, h, count = 1536, 1024, 3
    tensors = [torch.from_numpy(synth.frame_numpy(w, h, seed=500 + f, kind="noise")).cuda() for f in range(count)]
    budgets = np.full(count, 1 << 63, dtype=np.uint64)
    room = count * 2 * w * h
    archive = canary_buffer(torch, room)
    coded = batch.encode_batch_ragged(tensors, batch.codec_params(w, h), archive, max_stream_bytes=[2 * w * h] * count)
    assert (coded.errcs == 0).all()
    estimate = batch.estimated_destination_size(w, h, 8, 1)
    print(f"\n[noise] lossless sizes {coded.sizes.tolist()}, estimated destination size {estimate}")
    assert (coded.sizes > estimate).all()
    offsets, sizes = coded.offsets[:count].copy(), coded.sizes.copy()
    spec = capi.transcode_spec()
    want, want_nears, want_host = transcode(torch, archive, offsets, sizes, spec, budgets, (0,), room=room, alignment=16)
    assert (want.errcs == 0).all() and (want_nears == 0).all() and want.sizes.tolist() == sizes.tolist()
    source = archive.cpu().numpy()
    assert plain.streams_of(want, want_host) == [source[int(o):int(o) + int(n)].tobytes() for o, n in zip(offsets, sizes)]
    knobs.set("HOST_WINDOW_FRAMES", 2)  # a window of two frames, then one alone
    before = batch.host_counters()
    out = np.full(room, CANARY, dtype=np.uint8)
    got, nears = batch.transcode_batch_host_budget(source, offsets, sizes, spec, budgets, (0,), out, alignment=16)
    knobs.clear("HOST_WINDOW_FRAMES")
    assert got.errcs.tolist() == want.errcs.tolist() and nears.tolist() == want_nears.tolist()
    assert got.offsets.tolist() == want.offsets.tolist() and got.sizes.tolist() == want.sizes.tolist()
    assert (out == want_host).all()
    print(f"[noise] host counters moved by {[a - b for a, b in zip(batch.host_counters(), before)]}")


# ---- 5: timings --------------------------------------------------------------------------------------------------------------

def test_last_timings_have_the_four_stages(torch, sources):
    blob, offsets, sizes = plain.blob_of(torch, [s.jls for s in sources])
    transcode(torch, blob, offsets, sizes, capi.transcode_spec(), budgets_for(sources, CANDIDATES), CANDIDATES)
    t = batch.last_timings()
    assert len(t) == 4 and t[2] > 0 and t[3] > 0 and abs(t[0] - (t[2] + t[3])) < 1e-6 * max(t[0], 1)
