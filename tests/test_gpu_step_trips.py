"""The step loop of scan_group_decode.hip as a loop of trips, on the MI355X: the assembly of scan_group_step.inc decodes the frames
of tests/step_trips_frames.py (the ones tests/test_emu_step_trips.py puts through the C++ rendering) to the oracle's pixels,
through the batch API, with 8, 16 and 32 lanes per scan and workgroups of one and of four wavefronts -- and on its fast path: no
scan of these valid streams goes to the exact decoder.  GPU only."""
import pytest

import step_trips_frames as F
import strided as S
from charls_amd import capi

pytestmark = pytest.mark.gpu

CASES = F.all_cases()


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


def retries():
    return capi.engine_counters()["exact_retry_scans"]


@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("group", F.GROUPS)
@pytest.mark.parametrize("name", list(CASES))
def test_frames_decode_on_the_fast_path(torch, lib, knobs, name, group, waves):
    frames = [f.code() for f in CASES[name]]
    h, w = frames[0].img.shape
    g = S.Geometry(w, h, frames[0].bits)
    assert all(f.img.shape == (h, w) and (f.bits > 8) == (g.bits > 8) for f in frames)
    lay = S.Layout(g, g.row, g.packed, 0, len(frames), tight=True)
    knobs.set("DECODE_GROUP", group)
    knobs.set("DECODE_WORKGROUP_WAVES", waves)
    before = retries()
    rc, errcs, arena = S.decode_batch(torch, lib, [f.jls for f in frames], lay)
    rise = retries() - before
    assert rc == 0 and not errcs.any(), (rc, errcs.tolist())
    lay.check(arena, [f.pixels for f in frames])
    assert rise == 0, "a valid stream left the group decoder's fast path"
