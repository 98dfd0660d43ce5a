"""Encoding to a byte budget (charls_amd.h part 2f) on the GPU: charls_amd_measure_batch_device must report, for every frame
and candidate NEAR, the length of the ORACLE's stream at that NEAR without writing one, and
charls_amd_encode_batch_device_budget must give every frame the first candidate whose oracle stream fits its budget and
exactly that stream's bytes, placed by the offset rule of part 2d.  Every expected value comes from the oracle
(tests/oracle_bind.py, ample destination), once per frame and candidate; all frames are tiny.  GPU only."""
import functools

import numpy as np
import pytest

import jls_container
import oracle_bind as ob
from charls_amd import batch, synth

pytestmark = pytest.mark.gpu

CANARY = 0xA5
DESTINATION_TOO_SMALL = 3
EVEN_DESTINATION_SIZE = 1
CANDIDATES = (0, 1, 2, 4, 8)
FRAMES = 8
KINDS = ("gradient", "noise", "zero")  # frame f: KINDS[f % 3] with seed 3 + f // 3 (frame 1 is `noise`, seed 3)

# name -> width, height, bits, components, interleave mode, encoding options, row stride (0 = minimal)
CASES = {
    "gray8_33x17": (33, 17, 8, 1, 0, 0, 0),
    "gray12_19x9": (19, 9, 12, 1, 0, 0, 0),
    "gray16_65x5": (65, 5, 16, 1, 0, 0, 0),
    "rgb_none_16x8": (16, 8, 8, 3, 0, 0, 0),
    "rgb_line_16x8": (16, 8, 8, 3, 1, 0, 0),
    "rgb_sample_16x8": (16, 8, 8, 3, 2, 0, 0),
    "gray8_33x17_padded_rows_odd_base": (33, 17, 8, 1, 0, 0, 48),
    "gray8_33x17_even_size": (33, 17, 8, 1, 0, EVEN_DESTINATION_SIZE, 0),
}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def coding(case, restart_interval=0):
    w, h, bits, comps, ilv, options, _ = CASES[case]
    return dict(bits_per_sample=bits, component_count=comps, interleave_mode=ilv, encoding_options=options, restart_interval=restart_interval)


def dri_stream(img, w, h, kw, interval):
    """The stream of a single-scan frame with restart intervals, put together from the oracle's coding of every interval as an
    image of its own with RSTm between them (the reference cannot write restart markers; tests/test_gpu_restart.py)."""
    full = ob.encode(img, width=w, height=h, **kw)
    scan = jls_container.parse(full).scans[0]
    sos = full.rfind(b"\xff\xda", 0, scan.data_start)
    body, n = b"", (h + interval - 1) // interval
    for j in range(n):
        sub = np.ascontiguousarray(img[j * interval:(j + 1) * interval])
        s = ob.encode(sub, width=w, height=sub.shape[0], **kw)
        sc = jls_container.parse(s).scans[0]
        body += s[sc.data_start:sc.data_end] + (bytes([0xFF, 0xD0 + (j & 7)]) if j + 1 < n else b"")
    out = full[:sos] + b"\xff\xdd\x00\x04" + interval.to_bytes(2, "big") + full[sos:scan.data_start] + body
    if kw.get("encoding_options", 0) & EVEN_DESTINATION_SIZE and len(out) & 1:
        out += b"\xff"
    return out + b"\xff\xd9"


@functools.lru_cache(maxsize=None)
def expected(case, restart_interval=0):
    """(images, streams): streams[f][c] is the oracle's .jls of frame f at CANDIDATES[c].  Computed once, shared, never changed."""
    w, h, bits, comps, ilv, options, _ = CASES[case]
    images, streams = [], []
    for f in range(FRAMES):
        img = synth.frame_numpy(w, h, seed=3 + f // 3, bits=bits, components=comps, kind=KINDS[f % 3], interleaved=ilv != 0)
        images.append(img)
        kw = dict(bits_per_sample=bits, component_count=comps, interleave_mode=ilv, encoding_options=options)
        if restart_interval == 0:
            streams.append(tuple(ob.encode(img, width=w, height=h, near_lossless=c, **kw) for c in CANDIDATES))
        else:
            assert comps == 1 or ilv != 0
            streams.append(tuple(dri_stream(img, w, h, dict(kw, near_lossless=c), restart_interval) for c in CANDIDATES))
    return tuple(images), tuple(streams)


def oracle_sizes(case, candidates=CANDIDATES, restart_interval=0):
    streams = expected(case, restart_interval)[1]
    return np.array([[len(streams[f][CANDIDATES.index(c)]) for c in candidates] for f in range(FRAMES)], dtype=np.uint64)


def device_frames(torch, case):
    """(tensor, keyword arguments that state the geometry): the frames of a case on the device, rows padded to the case's stride
    and the first frame at an odd address when it has one."""
    w, h, bits, comps, ilv, _, stride = CASES[case]
    images = expected(case)[0]
    if stride == 0:
        stacked = np.stack(images)
        return torch.from_numpy(stacked.view(np.int16) if stacked.dtype == np.uint16 else stacked).cuda(), {}
    assert bits <= 8 and comps == 1
    pitch = stride * h + 5
    host = np.full(1 + FRAMES * pitch, CANARY, dtype=np.uint8)
    for f, img in enumerate(images):
        rows = host[1 + f * pitch:1 + f * pitch + stride * h].reshape(h, stride)
        rows[:, :w] = img
    whole = torch.from_numpy(host).cuda()
    assert whole.data_ptr() % 2 == 0
    return whole[1:].view(FRAMES, pitch), dict(stride=stride, width=w, height=h, frame_pitch=pitch)


def choose(sizes, budget):
    """The rule of the call on the oracle's sizes: the index of the first candidate, in the order given, that fits."""
    for k, s in enumerate(sizes):
        if int(s) <= int(budget):
            return k
    return -1


def rule_offsets(sizes, alignment):
    out = [0]
    for s in sizes:
        out.append(-(-(out[-1] + int(s)) // alignment) * alignment)
    return np.array(out, dtype=np.uint64)


def budgets_with_every_outcome(sizes):
    """Per-frame budgets from the oracle's sizes (frames x candidates): the first candidate fits exactly, a middle candidate
    exactly, that size - 1, none, plenty, the last exactly, none (0), another - 1."""
    b = [sizes[0][0], sizes[1][2], sizes[2][2] - 1, min(sizes[3]) - 1, 1 << 30, sizes[5][4], 0, sizes[7][1] - 1]
    return np.array([int(x) for x in b], dtype=np.uint64)


def check_budget_result(torch, case, result, nears, candidates, budgets, alignment, streams, capacity=None):
    """The whole contract of one budget call against the oracle: choices, errcs, sizes, offsets, bytes, zeroed gaps, canary."""
    sizes = np.array([[len(streams[f][CANDIDATES.index(c)]) for c in candidates] for f in range(FRAMES)], dtype=np.uint64)
    want_index = [choose(sizes[f], budgets[f]) for f in range(FRAMES)]
    want_sizes = [int(sizes[f][k]) if k >= 0 else 0 for f, k in enumerate(want_index)]
    want_offsets = rule_offsets(want_sizes, alignment)
    if capacity is not None:  # the first frame whose end lies beyond the capacity, and every frame after it
        full = next((f for f in range(FRAMES) if want_sizes[f] and int(want_offsets[f]) + want_sizes[f] > capacity), FRAMES)
        for f in range(full, FRAMES):
            want_index[f], want_sizes[f] = -1, 0
        want_offsets = rule_offsets(want_sizes, alignment)
    blob = result.packed.cpu().numpy()
    limit = blob.size if capacity is None else capacity
    covered = np.zeros(blob.size, dtype=bool)
    for f in range(FRAMES):
        k = want_index[f]
        assert int(nears[f]) == (candidates[k] if k >= 0 else -1), (case, f, nears, want_index)
        assert int(result.errcs[f]) == (0 if k >= 0 else DESTINATION_TOO_SMALL), (case, f)
        assert int(result.sizes[f]) == want_sizes[f], (case, f)
        assert int(result.offsets[f]) == int(want_offsets[f]), (case, f)
        if k >= 0:
            at = int(result.offsets[f])
            assert blob[at:at + want_sizes[f]].tobytes() == streams[f][CANDIDATES.index(candidates[k])], (case, f)
            gap_end = min(int(want_offsets[f + 1]), limit)
            assert (blob[at + want_sizes[f]:gap_end] == 0).all(), (case, f)
            covered[at:gap_end] = True
    assert int(result.offsets[FRAMES]) == int(want_offsets[FRAMES])
    assert (blob[~covered] == CANARY).all(), case  # nothing outside the frames and their gaps, nothing beyond the capacity
    return want_index


def canary_buffer(torch, nbytes):
    return torch.full((nbytes,), CANARY, dtype=torch.uint8, device="cuda:0")


# ---- measure ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_measured_sizes_are_the_oracles(torch, case):
    w, h, bits, comps, ilv, _, _ = CASES[case]
    frames, geometry = device_frames(torch, case)
    before = batch.measure_counters()
    sizes = batch.measure_batch(frames, CANDIDATES, **coding(case), **geometry)
    after = batch.measure_counters()
    want = oracle_sizes(case)
    print(f"\n[measure] {case}: {sizes.tolist()}")
    assert np.array_equal(sizes, want), case
    scans = comps if ilv == 0 else 1
    assert after[0] - before[0] == FRAMES * scans * len(CANDIDATES)
    assert after[2] - before[2] == 0
    assert 1 <= after[1] - before[1] <= 2


def test_candidates_in_any_order_and_repeated(torch):
    frames, geometry = device_frames(torch, "gray12_19x9")
    candidates = (8, 0, 8, 2, 0)
    before = batch.measure_counters()
    sizes = batch.measure_batch(frames, candidates, **coding("gray12_19x9"), **geometry)
    assert np.array_equal(sizes, oracle_sizes("gray12_19x9", candidates))
    assert batch.measure_counters()[0] - before[0] == FRAMES * 3  # a NEAR that repeats is walked once


def test_the_stuffed_and_the_tied_frame_are_in_the_batches():
    """What the cases above rest on: frame 1 of the 16-bit case has 0xFF bytes in its segment at every candidate, and frame 1 of
    the 12-bit case has 339 bytes at NEAR 1 and at NEAR 2."""
    for stream in expected("gray16_65x5")[1][1]:
        scan = jls_container.parse(stream).scans[0]
        assert 0xFF in stream[scan.data_start:scan.data_end]
    sizes = oracle_sizes("gray12_19x9")[1]
    assert int(sizes[1]) == 339 and int(sizes[2]) == 339


# ---- budget ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_budget_picks_the_first_candidate_that_fits_and_writes_the_oracles_bytes(torch, case):
    w, h, bits, comps, ilv, options, _ = CASES[case]
    images, streams = expected(case)
    frames, geometry = device_frames(torch, case)
    budgets = budgets_with_every_outcome(oracle_sizes(case))
    alignment = 2 if options & EVEN_DESTINATION_SIZE else 1
    packed = canary_buffer(torch, 1 << 15)
    result, nears = batch.encode_batch_budget(frames, budgets, CANDIDATES, packed, alignment=alignment, **coding(case), **geometry)
    print(f"\n[budget] {case}: budgets {budgets.tolist()} nears {nears.tolist()} sizes {result.sizes.tolist()}")
    chosen = check_budget_result(torch, case, result, nears, CANDIDATES, budgets, alignment, streams)
    # every outcome occurs: the first candidate, a later one at exactly its size, a later one because the one before it is one
    # byte too long, none (with coded neighbours on either side)
    sizes = oracle_sizes(case)
    assert chosen[0] == 0 and chosen[4] == 0
    assert chosen[1] > 0 and int(sizes[1][chosen[1]]) == int(budgets[1])
    assert chosen[7] >= 2 and int(sizes[7][1]) == int(budgets[7]) + 1
    assert chosen[3] == -1 and chosen[6] == -1 and chosen[5] >= 0 and chosen[7] >= 0
    # the blob decodes, every frame within the NEAR it was coded with
    coded = [f for f in range(FRAMES) if chosen[f] >= 0]
    out = torch.zeros((len(coded),) + tuple(images[0].shape), dtype=torch.uint8 if bits <= 8 else torch.int16, device="cuda:0")
    _, errcs, _ = batch.decode_batch_packed(packed, result.offsets[coded], result.sizes[coded], out)
    assert (errcs == 0).all()
    decoded = out.cpu().numpy()
    for k, f in enumerate(coded):
        got = decoded[k].view(np.uint16) if bits > 8 else decoded[k]
        assert np.abs(got.astype(np.int64) - images[f].astype(np.int64)).max() <= int(nears[f]), (case, f)


def test_a_tie_goes_to_the_candidate_named_first(torch):
    """Frame 1 of the 12-bit case: 339 bytes at NEAR 1 and at NEAR 2, so a budget of 339 gives NEAR 1 -- and NEAR 2 when the
    list names it first."""
    case = "gray12_19x9"
    frames, geometry = device_frames(torch, case)
    budgets = np.full(FRAMES, 339, dtype=np.uint64)
    for candidates, want in ((CANDIDATES, 1), ((0, 2, 1, 4, 8), 2)):
        packed = canary_buffer(torch, 1 << 14)
        result, nears = batch.encode_batch_budget(frames, budgets, candidates, packed, **coding(case), **geometry)
        check_budget_result(torch, case, result, nears, candidates, budgets, 1, expected(case)[1])
        assert int(nears[1]) == want


def test_candidates_are_tried_in_the_order_given(torch):
    case = "gray8_33x17"
    frames, geometry = device_frames(torch, case)
    candidates = (4, 0, 2)
    sizes = oracle_sizes(case, candidates)
    # exactly the size at NEAR 4 (the first named); plenty; the size at NEAR 2; one byte short of NEAR 4; the lossless size; ...
    budgets = np.array([sizes[0][0], 1 << 20, sizes[2][2], sizes[3][0] - 1, sizes[4][1], sizes[5][0], sizes[6][2] - 1, 1 << 20], dtype=np.uint64)
    packed = canary_buffer(torch, 1 << 15)
    result, nears = batch.encode_batch_budget(frames, budgets, candidates, packed, alignment=16, **coding(case), **geometry)
    chosen = check_budget_result(torch, case, result, nears, candidates, budgets, 16, expected(case)[1])
    assert chosen[0] == 0 and chosen[1] == 0 and chosen[7] == 0
    assert int(nears[1]) == 4  # not the lossless stream, which would fit as well


def test_capacity_rule(torch):
    """A capacity that ends inside frame 3: frames 3 .. are destination_too_small and nothing is written from the capacity on."""
    case = "gray8_33x17"
    frames, geometry = device_frames(torch, case)
    sizes = oracle_sizes(case)
    budgets = np.full(FRAMES, 1 << 20, dtype=np.uint64)
    offsets = rule_offsets(sizes[:, 0], 4)
    capacity = int(offsets[3]) + int(sizes[3][0]) - 1
    packed = canary_buffer(torch, 1 << 15)
    result, nears = batch.encode_batch_budget(frames, budgets, CANDIDATES, packed, alignment=4, capacity=capacity, **coding(case), **geometry)
    chosen = check_budget_result(torch, case, result, nears, CANDIDATES, budgets, 4, expected(case)[1], capacity=capacity)
    assert chosen == [0, 0, 0, -1, -1, -1, -1, -1]
    assert (packed[capacity:].cpu().numpy() == CANARY).all()


@pytest.mark.parametrize("case", ["gray8_33x17", "gray12_19x9", "rgb_none_16x8", "rgb_sample_16x8"])
def test_fallback_engine_gives_the_same_choices_and_bytes(torch, case):
    """charls_amd_set_encode_engine(1): the group encoder takes no scan, so every candidate is sized by coding it for real."""
    images, streams = expected(case)
    frames, geometry = device_frames(torch, case)
    budgets = budgets_with_every_outcome(oracle_sizes(case))
    packed = canary_buffer(torch, 1 << 15)
    before = batch.measure_counters()
    batch.set_encode_engine(1)
    try:
        sizes = batch.measure_batch(frames, CANDIDATES, **coding(case), **geometry)
        middle = batch.measure_counters()
        result, nears = batch.encode_batch_budget(frames, budgets, CANDIDATES, packed, **coding(case), **geometry)
    finally:
        batch.set_encode_engine(0)
    after = batch.measure_counters()
    assert np.array_equal(sizes, oracle_sizes(case))
    check_budget_result(torch, case, result, nears, CANDIDATES, budgets, 1, streams)
    scans = CASES[case][3] if CASES[case][4] == 0 else 1
    assert after[0] == before[0] and after[1] == before[1]
    assert middle[2] - before[2] == FRAMES * scans * len(CANDIDATES)  # the measure call codes all candidates
    assert 0 < after[2] - middle[2] < FRAMES * scans * len(CANDIDATES)  # the budget call stops at the first that fits


@pytest.mark.parametrize("case", ["gray8_33x17", "rgb_sample_16x8"])
def test_fallback_restart_intervals(torch, case):
    """restart_interval = 4: frames with restart intervals are sized by coding them; expected streams are the oracle's coding of
    every interval, joined with RSTm markers."""
    images, streams = expected(case, 4)
    frames, geometry = device_frames(torch, case)
    sizes_want = oracle_sizes(case, restart_interval=4)
    budgets = budgets_with_every_outcome(sizes_want)
    packed = canary_buffer(torch, 1 << 15)
    before = batch.measure_counters()
    sizes = batch.measure_batch(frames, CANDIDATES, **coding(case, 4), **geometry)
    result, nears = batch.encode_batch_budget(frames, budgets, CANDIDATES, packed, **coding(case, 4), **geometry)
    after = batch.measure_counters()
    assert np.array_equal(sizes, sizes_want)
    check_budget_result(torch, case, result, nears, CANDIDATES, budgets, 1, streams)
    assert after[0] == before[0] and after[2] > before[2]


def test_work_areas_are_released(torch):
    case = "gray8_33x17"
    frames, geometry = device_frames(torch, case)
    batch.release_work_areas()
    held = batch.work_area_bytes()
    packed = canary_buffer(torch, 1 << 15)
    budgets = budgets_with_every_outcome(oracle_sizes(case))
    batch.measure_batch(frames, CANDIDATES, **coding(case), **geometry)
    batch.encode_batch_budget(frames, budgets, CANDIDATES, packed, **coding(case), **geometry)
    assert batch.work_area_bytes() >= held
    batch.release_work_areas()
    assert batch.work_area_bytes() == held
