"""Every instantiation of the group decoder with 8 lanes per scan or more (decode_launch.hip: group_decode_built), each forced
with DECODE_GROUP / DECODE_WORKGROUP_WAVES and launched once: 2 sample widths x {8, 16, 32} lanes x 1..4 lines per pixel row x
lossless / NEAR = 2 with one-wavefront workgroups (48), and the workgroups of 4 and 8 wavefronts -- near-lossless: 4 -- of
single-line scans with 16 or 32 lanes (12).

Frames of 70 x 3 samples: beyond one 64-sample chunk and no multiple of 16.  (64 / G) * W + 1 frames: one more than a
workgroup takes, so a second, partly empty workgroup runs -- the smallest shape at which a wrong G or W in the dispatch shows
(a block size that does not match the grid leaves scans undecoded or decodes them twice over).  GPU only."""
import numpy as np
import pytest

import oracle_bind as ob
from charls_amd import batch, capi, synth

pytestmark = pytest.mark.gpu

WIDTH, HEIGHT = 70, 3
MAX_FRAMES = (64 // 16) * 8 + 1  # the largest case: 16 lanes, 8 wavefronts

CASES = [(bits, lanes, nl, 1, near) for bits in (8, 12) for lanes in (8, 16, 32) for nl in (1, 2, 3, 4) for near in (0, 2)] + \
        [(bits, lanes, 1, waves, near) for bits in (8, 12) for lanes in (16, 32) for waves, near in ((4, 0), (8, 0), (4, 2))]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


_coded = {}


def coded(torch, bits, nl, near):
    """MAX_FRAMES frames of one coding mode, encoded once: (streams, sizes, expected pixels as a device tensor).  Expected: the
    source (lossless), the oracle's decode of every stream (near-lossless)."""
    key = (bits, nl, near)
    if key not in _coded:
        source = np.stack([synth.frame_numpy(WIDTH, HEIGHT, seed=40 + 3 * f + nl, bits=bits, components=nl, kind="mixed")
                           for f in range(MAX_FRAMES)])
        as_tensor = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to("cuda:0").contiguous()
        enc = batch.encode_batch(as_tensor(source), bits_per_sample=bits, component_count=nl, interleave_mode=1 if nl > 1 else 0,
                                 near_lossless=near)
        assert (enc.errcs == 0).all()
        expected = source
        if near != 0:
            host = enc.streams.cpu().numpy()
            expected = np.stack([np.asarray(ob.decode(host[f, :int(enc.sizes[f])].tobytes())[1]).view(source.dtype).reshape(source.shape[1:])
                                 for f in range(MAX_FRAMES)])
        _coded[key] = (enc.streams, enc.sizes, as_tensor(expected))
    return _coded[key]


def test_the_cases_are_the_sixty_instantiations():
    assert len(CASES) == 60 and len(set(CASES)) == 60


@pytest.mark.parametrize("bits,lanes,nl,waves,near", CASES)
def test_group_decoder_instantiation(torch, knobs, bits, lanes, nl, waves, near):
    streams, sizes, expected = coded(torch, bits, nl, near)
    count = (64 // lanes) * waves + 1
    knobs.set("DECODE_GROUP", lanes)
    knobs.set("DECODE_WORKGROUP_WAVES", waves)
    out = torch.zeros_like(expected[:count])
    before = capi.engine_counters()["exact_retry_scans"]
    _, errcs, _ = batch.decode_batch(streams[:count].contiguous(), sizes[:count], out)
    rise = capi.engine_counters()["exact_retry_scans"] - before
    assert (errcs == 0).all(), errcs.tolist()
    assert torch.equal(out, expected[:count])
    assert rise == 0, "a scan left the group decoder"
