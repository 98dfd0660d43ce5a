"""Byte budgets for ragged frames (charls_amd.h part 2k) on the GPU: charls_amd_measure_batch_device_ragged and
charls_amd_encode_batch_device_ragged_budget on ONE call that interleaves every frame kind of tests/budget_model.py -- a, b, c,
..., a, b, c, ... -- each in an allocation of its own.  The calls are held to the oracle (sizes, the selection rule on them,
bytes) and, frame by frame, to the uniform calls of part 2f on each frame alone.  tests/test_ragged_budget_cpu.py checks that
the corpus meets every outcome of the selection.  Every output buffer is filled with a canary first.  All frames are tiny.
GPU only."""
import numpy as np
import pytest

import budget_model as bm
from charls_amd import batch, capi

pytestmark = pytest.mark.gpu

CANARY = 0xA5
NOT_ENOUGH_MEMORY, DESTINATION_TOO_SMALL = 1, 3
ROOM = 1 << 17


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


_frames = {}


def device_frame(torch, kind, repeat):
    """The device tensor of frame (kind, repeat), an allocation of its own: rows padded to the kind's stride at an odd base where
    it has one.  The last repeat names the tensor of the first."""
    repeat = 0 if repeat == bm.REPEATS - 1 else repeat
    if (kind, repeat) not in _frames:
        w, h, stride = bm.KINDS[kind][0], bm.KINDS[kind][1], bm.KINDS[kind][8]
        img = bm.image(kind, repeat)
        if stride == 0:
            _frames[kind, repeat] = torch.from_numpy(img.view(np.int16).copy() if img.dtype == np.uint16 else img.copy()).cuda()
        else:
            host = np.full(1 + stride * h, CANARY, dtype=np.uint8)
            host[1:].reshape(h, stride)[:, :w] = img
            whole = torch.from_numpy(host).cuda()
            assert whole.data_ptr() % 2 == 0
            _frames[kind, repeat] = whole[1:]
    return _frames[kind, repeat]


def params_of(kind, near=0):
    w, h, bits, comps, ilv, ct, options, restart, _ = bm.KINDS[kind]
    return batch.codec_params(w, h, bits, comps, ilv, near, color_transformation=ct, encoding_options=options, restart_interval=restart)


def the_call(torch, frames):
    """(tensors, params, strides) of a list of (kind, repeat)."""
    return ([device_frame(torch, k, r) for k, r in frames], [params_of(k, near=7) for k, _ in frames],  # (NEAR is not looked at)
            [bm.KINDS[k][8] for k, _ in frames])


def uniform_kw(kind):
    w, h, bits, comps, ilv, ct, options, restart, stride = bm.KINDS[kind]
    return dict(bits_per_sample=bits, component_count=comps, interleave_mode=ilv, color_transformation=ct, encoding_options=options,
                restart_interval=restart, stride=stride, width=w, height=h, frame_pitch=device_frame_bytes(kind))


def device_frame_bytes(kind):
    w, h, bits, comps, _, _, _, _, stride = bm.KINDS[kind]
    return stride * h if stride else w * h * comps * ((bits + 7) // 8)


def alone(torch, kind, repeat):
    """Frame (kind, repeat) as a uniform batch of one frame."""
    t = device_frame(torch, kind, repeat)
    return t.view(1, -1) if bm.KINDS[kind][8] else t[None]


def canary_buffer(torch, nbytes=ROOM):
    return torch.full((nbytes,), CANARY, dtype=torch.uint8, device="cuda:0")


def budgets_of(frames, candidates):
    return np.array([bm.budget_of(k, r, candidates, at) for at, (k, r) in enumerate(frames)], dtype=np.uint64)


def check_against_the_oracle(result, nears, frames, candidates, budgets, alignment, capacity=None):
    """The whole contract of one budget call against the model: choices, errcs, sizes, offsets, bytes, zeroed gaps, canary."""
    want = bm.expected(frames, candidates, budgets)
    sizes = [len(s) for _, _, s in want]
    offsets = bm.rule_offsets(sizes, alignment)
    if capacity is not None:  # the first frame whose end lies beyond the capacity, and every frame behind it
        full = next((f for f in range(len(frames)) if sizes[f] and int(offsets[f]) + sizes[f] > capacity), len(frames))
        for f in range(full, len(frames)):
            want[f], sizes[f] = (DESTINATION_TOO_SMALL, -1, b""), 0
        offsets = bm.rule_offsets(sizes, alignment)
    blob = result.packed.cpu().numpy()
    limit = blob.size if capacity is None else capacity
    covered = np.zeros(blob.size, dtype=bool)
    for f, (errc, near, stream) in enumerate(want):
        assert (int(result.errcs[f]), int(nears[f]), int(result.sizes[f])) == (errc, near, len(stream)), (f, frames[f])
        assert int(result.offsets[f]) == int(offsets[f]), (f, frames[f])
        if stream:
            at = int(offsets[f])
            assert blob[at:at + len(stream)].tobytes() == stream, (f, frames[f])
            gap_end = min(int(offsets[f + 1]), limit)
            assert (blob[at + len(stream):gap_end] == 0).all(), (f, frames[f])
            covered[at:gap_end] = True
    assert int(result.offsets[len(frames)]) == int(offsets[len(frames)])
    assert (blob[~covered] == CANARY).all()  # nothing outside the streams and their gaps, nothing beyond the capacity
    return want


# ---- measure -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("candidates", [bm.WIDE, bm.NARROW])
def test_measured_sizes_are_the_oracles_and_the_uniform_calls(torch, candidates):
    frames = bm.call_frames()
    tensors, params, strides = the_call(torch, frames)
    sizes, errcs = batch.measure_batch_ragged(tensors, params, candidates, strides=strides)
    for f, (kind, repeat) in enumerate(frames):
        code = bm.refusal(kind, candidates)
        assert int(errcs[f]) == code, (f, kind)
        want = [0] * len(candidates) if code else bm.oracle_sizes(kind, repeat, candidates)
        assert sizes[f].tolist() == want, (f, kind)
        try:  # the uniform call on this frame alone
            uniform = batch.measure_batch(alone(torch, kind, repeat), candidates, **uniform_kw(kind))
            assert code == 0 and uniform[0].tolist() == sizes[f].tolist(), (f, kind)
        except capi.JpegLSError as e:
            assert e.errc == code != 0, (f, kind)


# ---- budget ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alignment", [1, 16, 4096])
@pytest.mark.parametrize("candidates", [bm.WIDE, bm.NARROW])
def test_budget_call_against_the_oracle(torch, candidates, alignment):
    frames = bm.call_frames()
    tensors, params, strides = the_call(torch, frames)
    budgets = budgets_of(frames, candidates)
    packed = canary_buffer(torch, ROOM if alignment < 4096 else 48 * 4096)
    result, nears = batch.encode_batch_ragged_budget(tensors, params, budgets, candidates, packed, alignment=alignment, strides=strides)
    torch.cuda.synchronize()
    want = check_against_the_oracle(result, nears, frames, candidates, budgets, alignment)
    # failures stay local: refused kinds and frames without a fitting candidate stand between coded ones
    codes = [errc for errc, _, _ in want]
    assert 0 in codes and DESTINATION_TOO_SMALL in codes
    assert (bm.INVALID_ARGUMENT_COLOR_TRANSFORMATION in codes) and ((bm.INVALID_ARGUMENT_NEAR_LOSSLESS in codes) == (candidates == bm.WIDE))


@pytest.mark.parametrize("candidates", [bm.WIDE, bm.NARROW])
def test_budget_call_equals_the_uniform_call_on_each_frame_alone(torch, candidates):
    frames = bm.call_frames()
    tensors, params, strides = the_call(torch, frames)
    budgets = budgets_of(frames, candidates)
    packed = canary_buffer(torch)
    result, nears = batch.encode_batch_ragged_budget(tensors, params, budgets, candidates, packed, strides=strides)
    torch.cuda.synchronize()
    blob = packed.cpu().numpy()
    for f, (kind, repeat) in enumerate(frames):
        single = canary_buffer(torch, 1 << 13)
        try:
            one, one_near = batch.encode_batch_budget(alone(torch, kind, repeat), budgets[f:f + 1], candidates, single, **uniform_kw(kind))
        except capi.JpegLSError as e:  # refused as a whole call: the frame's errc here
            assert (int(result.errcs[f]), int(nears[f]), int(result.sizes[f])) == (e.errc, -1, 0), (f, kind)
            continue
        assert (int(result.errcs[f]), int(nears[f]), int(result.sizes[f])) == (int(one.errcs[0]), int(one_near[0]), int(one.sizes[0])), (f, kind)
        at, n = int(result.offsets[f]), int(result.sizes[f])
        assert blob[at:at + n].tobytes() == single.cpu().numpy()[:n].tobytes(), (f, kind)


def test_the_capacity_rule_cuts_in_the_middle_of_a_group(torch):
    """The capacity ends inside a frame of the second repeat: its group has frames on both sides of the cut."""
    frames = bm.call_frames()
    tensors, params, strides = the_call(torch, frames)
    budgets = np.array([0 if bm.refusal(k, bm.NARROW) else 1 << 63 for k, _ in frames], dtype=np.uint64)
    sizes = [len(s) for _, _, s in bm.expected(frames, bm.NARROW, budgets)]
    offsets = bm.rule_offsets(sizes, 4)
    cut = len(bm.KINDS) + 4
    assert sizes[cut] > 1 and frames[cut][1] == 1
    capacity = int(offsets[cut]) + sizes[cut] - 1
    packed = canary_buffer(torch)
    result, nears = batch.encode_batch_ragged_budget(tensors, params, budgets, bm.NARROW, packed, alignment=4, strides=strides, capacity=capacity)
    torch.cuda.synchronize()
    want = check_against_the_oracle(result, nears, frames, bm.NARROW, budgets, 4, capacity=capacity)
    assert all(errc == DESTINATION_TOO_SMALL for errc, _, _ in want[cut:]) and (nears[cut:] == -1).all()
    assert (packed[capacity:].cpu().numpy() == CANARY).all()


def test_the_same_pixels_with_different_budgets(torch):
    kind = "gray8_33x17"
    sizes = bm.oracle_sizes(kind, 0, bm.NARROW)
    assert len(set(sizes)) >= 3
    frames = [(kind, 0)] * 4
    tensors, params, strides = the_call(torch, frames)
    assert len({t.data_ptr() for t in tensors}) == 1
    budgets = np.array([sizes[0], sizes[4], sizes[3], sizes[4] - 1], dtype=np.uint64)
    packed = canary_buffer(torch)
    result, nears = batch.encode_batch_ragged_budget(tensors, params, budgets, bm.NARROW, packed, alignment=16, strides=strides)
    torch.cuda.synchronize()
    check_against_the_oracle(result, nears, frames, bm.NARROW, budgets, 16)
    assert int(nears[0]) == 0 and int(nears[3]) == -1 and len(set(nears.tolist())) >= 3


# ---- how: groups, not frames -------------------------------------------------------------------------------------------------

def test_a_group_is_sized_by_one_uniform_call(torch):
    """12 frames of 3 groups, interleaved: the counters move by exactly the sum of what the uniform call on each group's frames
    moves them by -- one measuring launch per group, never one per frame."""
    kinds = ("gray8_33x17", "rgb_planar_16x8", "gray8_restart2_33x17")
    frames = [(kind, repeat) for repeat in range(4) for kind in kinds]
    tensors, params, strides = the_call(torch, frames)
    # the uniform calls: every group's frames gathered into one batch tensor
    want = [0, 0, 0]
    for kind in kinds:
        stacked = torch.stack([device_frame(torch, kind, r) for r in range(4)]).contiguous()
        before = batch.measure_counters()
        uniform = batch.measure_batch(stacked, bm.NARROW, **uniform_kw(kind))
        after = batch.measure_counters()
        assert uniform.tolist() == [bm.oracle_sizes(kind, r, bm.NARROW) for r in range(4)]
        want = [w + a - b for w, a, b in zip(want, after, before)]
    before = batch.measure_counters()
    sizes, errcs = batch.measure_batch_ragged(tensors, params, bm.NARROW, strides=strides)
    after = batch.measure_counters()
    assert (errcs == 0).all() and sizes.tolist() == [bm.oracle_sizes(k, r, bm.NARROW) for k, r in frames]
    print(f"\n[ragged measure] counters moved by {[a - b for a, b in zip(after, before)]}, the uniform calls by {want}")
    assert [a - b for a, b in zip(after, before)] == want
    assert want[1] == 2 and want[2] > 0  # (two groups take the measuring launch, the one with restart intervals is coded)
    # and the budget call: the same sizing launches
    budgets = np.full(len(frames), 1 << 63, dtype=np.uint64)
    want_launches = 0
    for kind in kinds:
        stacked = torch.stack([device_frame(torch, kind, r) for r in range(4)]).contiguous()
        before = batch.measure_counters()
        batch.encode_batch_budget(stacked, budgets[:4], bm.NARROW, canary_buffer(torch), **uniform_kw(kind))
        want_launches += batch.measure_counters()[1] - before[1]
    before = batch.measure_counters()
    batch.encode_batch_ragged_budget(tensors, params, budgets, bm.NARROW, canary_buffer(torch), strides=strides)
    assert batch.measure_counters()[1] - before[1] == want_launches == 2


# ---- the work areas ----------------------------------------------------------------------------------------------------------

def test_a_workspace_limit_that_does_not_hold_a_slot(torch):
    frames = bm.call_frames()
    tensors, params, strides = the_call(torch, frames)
    budgets = budgets_of(frames, bm.NARROW)
    packed = canary_buffer(torch)
    batch.release_work_areas()
    try:
        batch.set_workspace_limit(64)  # below every frame's staging slot
        with pytest.raises(capi.JpegLSError) as e:
            batch.encode_batch_ragged_budget(tensors, params, budgets, bm.NARROW, packed, strides=strides)
        assert e.value.errc == NOT_ENOUGH_MEMORY
        torch.cuda.synchronize()
        assert (packed.cpu().numpy() == CANARY).all()
    finally:
        batch.set_workspace_limit(0)
        batch.release_work_areas()
    result, nears = batch.encode_batch_ragged_budget(tensors, params, budgets, bm.NARROW, packed, strides=strides)
    torch.cuda.synchronize()
    check_against_the_oracle(result, nears, frames, bm.NARROW, budgets, 1)
