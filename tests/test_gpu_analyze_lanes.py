"""The frames of test_emu_analyze_lanes.py through the batch API on the GPU: the neighbours of a sample from the lane next to
it in P2 of sort_tiles (a DPP wave shift, lane 0 from the chunk in front), and in pass 2 of analyze_tiles the run state a
piece starts in by look-ahead over the chunks in front of it.  Two frames per call; every stream must be the oracle's and must
decode to its frame."""
import numpy as np
import pytest

import oracle_bind as ob
import test_emu_analyze_lanes as A
from charls_amd import batch, capi

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
    return L


@pytest.mark.parametrize("name", list(A.FRAMES))
def test_frame_equals_oracle_and_round_trips(torch, lib, knobs, name):
    """The frame and the frame upside down, so that a launch has more than one scan."""
    make, bits, cap = A.FRAMES[name]
    if cap is not None:
        knobs.set("TILE_SAMPLES", cap)
    img = make()
    imgs = [img, np.ascontiguousarray(img[::-1])]
    h, w = img.shape
    frames = torch.from_numpy(np.stack(imgs).view(np.int16) if bits > 8 else np.stack(imgs)).cuda()
    enc = batch.encode_batch(frames, bits_per_sample=bits, lib=lib)
    host = enc.streams.cpu().numpy()
    for f, one in enumerate(imgs):
        assert enc.errcs[f] == 0
        assert host[f, :int(enc.sizes[f])].tobytes() == ob.encode(one, width=w, height=h, bits_per_sample=bits), f
    out = torch.empty_like(frames)
    _, errcs, _ = batch.decode_batch(enc.streams, enc.sizes, out, lib=lib)
    assert (errcs == 0).all() and torch.equal(out, frames)
