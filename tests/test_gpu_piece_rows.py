"""The frames of test_emu_piece_rows.py through the batch API on the GPU: the piece copies of sort_tiles, sort_pixel_tiles and
pack_tiles by flat rows (the row table read as 16 bytes, the piece of a lane from two v_mbcnt, the start bits ORed into LDS).
Two frames per call; every stream must be the oracle's and must decode to its frame."""
import ctypes as C

import numpy as np
import pytest

import oracle_bind as ob
import test_emu_piece_rows as R
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
    L.lib.charls_amd_speculation_counters.argtypes = [C.POINTER(C.c_uint64), C.c_int32]
    L.lib.charls_amd_speculation_counters.restype = C.c_int32
    return L


def _tile_jobs(lib):
    """Jobs of the context chains and of the run chain the tile pipeline has coded so far."""
    out = (C.c_uint64 * 4)()
    lib.lib.charls_amd_speculation_counters(out, 4)
    return int(out[0]) + int(out[2])


def _round_trip(torch, lib, imgs, bits, **kw):
    """imgs as ONE batch: the oracle's bytes, coded by the tile pipeline, and the decoder gives the frames back."""
    frames = torch.from_numpy(np.stack(imgs).view(np.int16) if bits > 8 else np.stack(imgs)).cuda()
    before = _tile_jobs(lib)
    enc = batch.encode_batch(frames, bits_per_sample=bits, lib=lib, **kw)
    assert _tile_jobs(lib) > before, "not coded by the tile pipeline"
    host = enc.streams.cpu().numpy()
    comps = kw.get("component_count", 1)
    h, w = imgs[0].shape[:2]
    for f, img in enumerate(imgs):
        want = ob.encode(img, width=w, height=h, bits_per_sample=bits, component_count=comps,
                         interleave_mode=kw.get("interleave_mode", 0))
        assert enc.errcs[f] == 0
        assert host[f, :int(enc.sizes[f])].tobytes() == want, f
    out = torch.empty_like(frames)
    _, errcs, _ = batch.decode_batch(enc.streams, enc.sizes, out, lib=lib)
    assert (errcs == 0).all() and torch.equal(out, frames)


@pytest.mark.parametrize("name", list(R.FRAMES))
def test_frame_equals_oracle_and_round_trips(torch, lib, knobs, name):
    """The frame and the frame upside down, so that a launch has more than one scan."""
    make, bits, cap, pixel = R.FRAMES[name]
    if cap is not None:
        knobs.set("TILE_SAMPLES", cap)
    if pixel:
        knobs.set("PIXEL_MODE", 1)
    img = make()
    _round_trip(torch, lib, [img, np.ascontiguousarray(img[::-1])], bits)


@pytest.mark.parametrize("name", list(R.RGB_FRAMES))
def test_sample_interleaved_frame_equals_oracle_and_round_trips(torch, lib, knobs, name):
    make, cap = R.RGB_FRAMES[name]
    if cap is not None:
        knobs.set("TILE_SAMPLES", cap)
    img = make()
    _round_trip(torch, lib, [img, np.ascontiguousarray(img[::-1])], 8, component_count=3, interleave_mode=2)
