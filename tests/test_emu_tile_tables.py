"""The table work of sort_tiles and pack_tiles on the CPU (tile_pipeline.hip compiled for the host by tests/emu; the harness
of test_emu_tile_pipeline.py): the run-lead table built by a wavefront per line, the chain offsets behind the combined scan, the
scan of two series at once, and the pack stage that puts a tile's bits together from bit 0 and shifts them on the way out.
The scan bytes must be the oracle's.  The frames sit where that code can go wrong: runs across chunks and to the end of the
line, lines of 128 chunks (two per lane), partial last chunks, every segment geometry, tiles of a few bits."""
import ctypes as C
import os

import numpy as np
import pytest

import emu_bind
import jls_container
import oracle_bind as ob
import test_emu_tile_pipeline as P
from charls_amd import synth


def _flat(w, h, other_at=None, value=77):
    img = np.full((h, w), value, dtype=np.uint8)
    if other_at is not None:
        img[min(2, h - 1), other_at] = value + 9
    return img


def _mixed(w, h):
    return synth.frame_numpy(w, h, seed=w + h, kind="mixed")


# name -> (frame, bits per sample); test_gpu_tile_tables.py runs the same frames through the batch API
FRAMES = {}
# ---- leads across chunks: every chunk all ones (a run to the end of every line), and one sample that ends the run, at the
# edges of chunks; 128 chunks, two per lane, with a run that crosses from the first 64 chunks into the others; partial last
# chunks; width 1
for _x in (None, 0, 63, 64, 4031, 4095):
    FRAMES[f"flat_4096x4_other_at_{_x}"] = (lambda x=_x: _flat(4096, 4, x), 8)
for _x in (None, 4485, 8191):
    FRAMES[f"flat_8192x2_other_at_{_x}"] = (lambda x=_x: _flat(8192, 2, x), 8)
for _w, _h in ((65, 5), (150, 5), (4097, 3), (1, 20)):
    FRAMES[f"flat_{_w}x{_h}"] = (lambda w=_w, h=_h: _flat(w, h), 8)
    FRAMES[f"flat_{_w}x{_h}_other_at_end"] = (lambda w=_w, h=_h: _flat(w, h, w - 1), 8)
# ---- segment geometry: 16 lines per tile with one piece each; a short last tile; one line of eight pieces; run starts in
# many chunks
for _w, _h in ((512, 32), (4096, 3), (8192, 1), (2048, 16)):
    FRAMES[f"mixed_{_w}x{_h}"] = (lambda w=_w, h=_h: _mixed(w, h), 8)
# ---- pack words: all zeros (tiles of a few bits, chains of tiles with no word of their own, no tile but the first starts
# on a word boundary); codes longer than a word; a frame with many bits per tile
for _w, _h in ((64, 64), (4096, 8)):
    FRAMES[f"zeros_{_w}x{_h}"] = (lambda w=_w, h=_h: np.zeros((h, w), dtype=np.uint8), 8)
FRAMES["noise16_256x8"] = (lambda: synth.frame_numpy(256, 8, seed=21, bits=16, kind="noise"), 16)
FRAMES["hard_4096x4"] = (lambda: synth.frame_numpy(4096, 4, seed=17, kind="hard"), 8)


@pytest.mark.parametrize("name", list(FRAMES))
def test_frame_equals_oracle(name):
    make, bits = FRAMES[name]
    img = make()
    h, w = img.shape
    pc = jls_container.validated_pc((0,) * 5, bits, 0)
    want = P._scan_bytes(ob.encode(img, width=w, height=h, bits_per_sample=bits))
    (errc, flags, data), = P._encode_planes([img], w, h, bits, pc, len(want) + 1024, job=512, warm=256)
    assert errc == 0 and flags == 0
    assert data == want


@pytest.fixture(scope="module")
def hard_frame():
    img = synth.frame_numpy(4096, 4, seed=17, kind="hard")
    return img, P._scan_bytes(ob.encode(img, width=4096, height=4))


CANARY = 0xC7


def _encode_guarded(img, capacity):
    """One 8-bit frame into a destination of `capacity` bytes that lies inside a larger buffer of canary bytes: returns
    errc, flags, the bytes written and whether anything outside the destination changed."""
    h, w = img.shape
    guard = 4096
    arena = np.full(guard + capacity + guard, CANARY, dtype=np.uint8)
    out = arena[guard:guard + capacity]
    keep = []
    pix = np.ascontiguousarray(img).reshape(-1).copy()
    pc = jls_container.validated_pc((0,) * 5, 8, 0)
    desc = emu_bind.make_desc(w, h, 1, 0, 8, 0, 0, pc, 0, pix, w, out, keep)
    arr, res = (emu_bind.ScanDesc * 1)(desc), (emu_bind.ScanResult * 1)()
    emu_bind.tile_lib().emu_encode_tile_pipeline(arr, res, 1, 512, 256, *P.RUN_JOBS)
    clean = bool((arena[:guard] == CANARY).all() and (arena[guard + capacity:] == CANARY).all())
    return res[0].errc, res[0].flags, out[:res[0].bytes].tobytes(), clean


def test_destination_sizes_around_the_stream_and_far_below_it(hard_frame):
    """The bound of the words a tile stores (raw_words) and what stands behind it, on a frame of two tiles.  A destination
    of the stream's size + 4 takes the stream, byte for byte; the stream's size exactly is left to the exact kernel (flags 2,
    as in test_emu_tile_pipeline); one byte less, and a third of the stream (the tiles' words then end far beyond the raw
    buffer, which is sized by the destination), are destination_too_small.  Nothing outside the destination is written in
    any of them.  (The raw buffer itself belongs to the emulator's driver: a store beyond IT is not visible from here.)"""
    img, want = hard_frame
    errc, flags, data, clean = _encode_guarded(img, len(want) + 4)
    assert clean and errc == 0 and flags == 0 and data == want
    errc, flags, data, clean = _encode_guarded(img, len(want))
    assert clean and errc == 0 and flags == 2
    for capacity in (len(want) - 1, len(want) // 3):
        errc, flags, data, clean = _encode_guarded(img, capacity)
        assert clean and errc == 3, capacity


# ---- the scan of two series
@pytest.mark.parametrize("threads,count", [(256, 1), (256, 256), (256, 367), (256, 512), (512, 1), (512, 367), (512, 512),
                                           (512, 700), (512, 1024)])
def test_scan_of_two_series_against_numpy(threads, count):
    """One value per thread (the second half skipped) and two; 367 is the number of chains."""
    L = emu_bind._build_and_load("emu_scan_driver.cpp", os.path.join(emu_bind.ROOT, "tests", "_emu_build", "libjls_emu_scan.so"))
    rng = np.random.default_rng(count * 1000 + threads)
    a = rng.integers(0, 70, count).astype(np.uint32)
    b = rng.integers(0, 1 << 20, count).astype(np.uint32)
    out_a, out_b = np.full(count, 0xA5A5A5A5, np.uint32), np.full(count, 0xA5A5A5A5, np.uint32)
    ptr = lambda v: v.ctypes.data_as(C.POINTER(C.c_uint32))
    L.emu_scan_pair(ptr(a), ptr(b), C.c_uint32(count), C.c_uint32(threads), ptr(out_a), ptr(out_b))
    assert np.array_equal(out_a, np.cumsum(a) - a)
    assert np.array_equal(out_b, np.cumsum(b) - b)
