"""The frames of test_emu_tile_tables.py through the batch API on the GPU: the table work of sort_tiles and pack_tiles (run
leads built by a wavefront per line, chain offsets behind the combined scan, the scan of two series, a tile's bits put together
from bit 0 and shifted on the way out).  Every stream must be the oracle's."""
import numpy as np
import pytest

import oracle_bind as ob
import test_emu_tile_tables as T
from charls_amd import batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _encode_and_compare(torch, imgs, bits):
    h, w = imgs[0].shape
    frames = torch.from_numpy(np.stack(imgs).view(np.int16) if bits > 8 else np.stack(imgs)).cuda()
    enc = batch.encode_batch(frames, bits_per_sample=bits)
    host = enc.streams.cpu().numpy()
    for f, img in enumerate(imgs):
        want = ob.encode(img, width=w, height=h, bits_per_sample=bits)
        assert enc.errcs[f] == 0
        assert host[f, :int(enc.sizes[f])].tobytes() == want, f


@pytest.mark.parametrize("name", list(T.FRAMES))
def test_frame_equals_oracle(torch, name):
    """Two frames per call (the frame and the frame upside down), so that a launch has more than one scan."""
    make, bits = T.FRAMES[name]
    img = make()
    _encode_and_compare(torch, [img, np.ascontiguousarray(img[::-1])], bits)


def test_destination_exactly_as_large_as_the_stream_and_around_it(torch):
    """The bound of the words a tile stores and the exact answer behind it: with a destination of the stream's size, a byte
    less and up to four more, the batch API gives the oracle's verdict (the reference's depends on its flush history within
    three bytes of the size) and, where that is success, its bytes."""
    make, bits = T.FRAMES["hard_4096x4"]
    img = make()
    full = ob.encode(img, width=4096, height=4)
    frames = torch.from_numpy(img[None]).cuda()
    for size in (len(full) + d for d in (-1, 0, 1, 2, 3, 4)):
        try:
            want, errc = ob.encode(img, width=4096, height=4, destination_size=size), 0
        except ob.OracleError as e:
            want, errc = None, e.errc
        enc = batch.encode_batch(frames, streams=torch.zeros((1, size), dtype=torch.uint8, device="cuda:0"))
        assert enc.errcs[0] == errc, (size - len(full), enc.errcs[0], errc)
        if want is not None:
            assert enc.streams.cpu().numpy()[0, :int(enc.sizes[0])].tobytes() == want, size - len(full)
    assert errc == 0  # (the largest of them fits)


def test_geometries_back_to_back(torch):
    """4096 x 4, 150 x 7 and 8192 x 2 frames through the same work areas, one after the other and back (a call of the batch
    API has one frame geometry: the mix is across calls), five frames each."""
    for w, h in ((4096, 4), (150, 7), (8192, 2), (150, 7), (4096, 4)):
        imgs = [T.synth.frame_numpy(w, h, seed=300 + w + f, kind="mixed") for f in range(5)]
        _encode_and_compare(torch, imgs, 8)
