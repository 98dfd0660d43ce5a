"""The frames of test_emu_sort_runs.py through the batch API on the GPU: P2 of sort_tiles with its keys in registers or
fetched in batches, the slots stored behind a batch, the run records worked out behind the chunk loop; the global pointers of
analyze_tiles, sort_tiles and pack_tiles.  Every stream must be the oracle's."""
import numpy as np
import pytest

import oracle_bind as ob
import strided as S
import test_emu_sort_runs as R
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


def _encode_and_compare(torch, imgs, bits):
    h, w = imgs[0].shape
    frames = torch.from_numpy(np.stack(imgs).view(np.int16) if bits > 8 else np.stack(imgs)).cuda()
    enc = batch.encode_batch(frames, bits_per_sample=bits)
    host = enc.streams.cpu().numpy()
    for f, img in enumerate(imgs):
        want = ob.encode(img, width=w, height=h, bits_per_sample=bits)
        assert enc.errcs[f] == 0
        assert host[f, :int(enc.sizes[f])].tobytes() == want, f


@pytest.mark.parametrize("name", list(R.FRAMES))
def test_frame_equals_oracle(torch, name):
    """Two frames per call (the frame and the frame upside down), so that a launch has more than one scan."""
    make, bits = R.FRAMES[name]
    img = make()
    _encode_and_compare(torch, [img, np.ascontiguousarray(img[::-1])], bits)


def test_frame_with_64_to_128_run_starts_in_a_segment(torch):
    img = R._every(4096, 4, 9)
    assert any(64 < n < 128 for n in R.starts_per_segment(img).values())
    _encode_and_compare(torch, [img, np.ascontiguousarray(img[::-1])], 8)


@pytest.mark.parametrize("w,h,bits,cls,base", [(150, 5, 8, "p1", 1), (150, 5, 16, "r16", 0)])
def test_padded_rows(torch, lib, w, h, bits, cls, base):
    """stage_lines sample by sample from an odd address (8 bits) and word by word over padded rows (16 bits)."""
    g = S.Geometry(w, h, bits)
    lay = S.layout(g, cls, base, 2, "even")
    frames = [S.Coded(g, 5 + 17 * f) for f in range(2)]
    arena = lay.pad([f.img for f in frames])
    rc, errcs, streams, after = S.encode_batch(torch, lib, arena, lay, S.codec_params(g))
    assert rc == 0 and not errcs.any(), (rc, errcs.tolist())
    for f, fr in enumerate(frames):
        assert streams[f] == fr.jls, f
    assert np.array_equal(after, arena), "the encoder wrote to its source"


def test_destination_exactly_as_large_as_the_stream(torch):
    """A many-runs frame into a destination of the stream's size, a byte less and four more: the oracle's verdict and, where
    that is success, its bytes (the words pack_tiles stores are bounded by the destination)."""
    img = R.FRAMES["every_3_4096x4"][0]()
    full = ob.encode(img, width=4096, height=4)
    frames = torch.from_numpy(img[None]).cuda()
    for size in (len(full) + d for d in (-1, 0, 4)):
        try:
            want, errc = ob.encode(img, width=4096, height=4, destination_size=size), 0
        except ob.OracleError as e:
            want, errc = None, e.errc
        enc = batch.encode_batch(frames, streams=torch.zeros((1, size), dtype=torch.uint8, device="cuda:0"))
        assert enc.errcs[0] == errc, (size - len(full), enc.errcs[0], errc)
        if want is not None:
            assert enc.streams.cpu().numpy()[0, :int(enc.sizes[0])].tobytes() == want, size - len(full)
    assert errc == 0  # (the largest of them fits)
