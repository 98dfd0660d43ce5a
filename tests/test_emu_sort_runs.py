"""P2 of sort_tiles on the CPU (tile_pipeline.hip compiled for the host by tests/emu; the harness of
test_emu_tile_pipeline.py): the keys of a segment held in registers from P1 or fetched in batches of 16 chunks, the tile-local
slots stored behind a batch, and the run records worked out behind the chunk loop, 64 run starts at a time, from the columns
the loop leaves in their slots.  The scan bytes must be the oracle's.

Every frame is chosen for a path, and says so: `analysis` restates pass 2 of analyze_tiles in numpy (which sample starts a
run, how long the run is, where it is interrupted) and `geometry` restates tile_geometry, and the tests assert with them that
the frame is where it was meant to be."""
import numpy as np
import pytest

import emu_bind
import jls_container
import oracle_bind as ob
import strided as S
import test_emu_tile_pipeline as P
import test_emu_tile_tables as T
from charls_amd import synth


# ---- what the kernels make of a frame, restated ------------------------------------------------------------------------------

def geometry(w, bits=8):
    """lines per tile, pieces per line, chunks per line, chunks per piece (plan_tiles / tile_geometry, planar whole lines)."""
    cap = 8192 if bits <= 8 else 4096
    lpt = min(16, cap // w)
    pieces = 1 if lpt >= 8 else 8 // lpt
    chunks = (w + 63) // 64
    return lpt, pieces, chunks, (chunks + pieces - 1) // pieces


def analysis(img):
    """Run starts of a frame by the rule of analyze_tiles pass 2: a list of (line, column, run length, column of the
    interruption sample or None where the run ends with the line)."""
    h, w = img.shape
    a = img.astype(np.int64)
    out = []
    for y in range(h):
        cur = a[y]
        prev = a[y - 1] if y >= 1 else np.zeros(w, dtype=np.int64)
        edge_a = prev[0] if y >= 1 else 0
        edge_c = a[y - 2][0] if y >= 2 else 0
        ra = np.concatenate(([edge_a], cur[:-1]))
        rb = prev
        rc = np.concatenate(([edge_c], prev[:-1])) if y >= 1 else np.concatenate(([edge_c], np.zeros(w - 1, dtype=np.int64)))
        rd = np.concatenate((prev[1:], prev[-1:]))
        eq = cur == ra
        q0 = (rd == rb) & (rb == rc) & (rc == ra)
        s, x = False, 0
        while x < w:
            if not s and q0[x]:  # a run starts here
                run = 0
                if eq[x]:
                    run = 1
                    while x + run < w and eq[x + run]:
                        run += 1
                out.append((y, x, run, x + run if x + run < w else None))
                x += run + 1  # (the interruption sample is coded by the run; the state behind it is `not in a run`)
                s = False
                continue
            x += 1
    return out


def starts_per_segment(img, bits=8):
    """(line, piece) -> run starts of that segment."""
    h, w = img.shape
    lpt, pieces, chunks, cpp = geometry(w, bits)
    counts = {}
    for y, x, run, xi in analysis(img):
        key = (y, (x // 64) // cpp)
        counts[key] = counts.get(key, 0) + 1
    return counts


def _mixed(w, h):
    return synth.frame_numpy(w, h, seed=w + h, kind="mixed")


def _every(w, h, nth, dtype=np.uint8, value=77, other=90):
    """A flat frame with one differing sample every `nth` column on every other line."""
    img = np.full((h, w), value, dtype=dtype)
    img[1::2, nth - 1::nth] = other
    return img


def _columns(w, h):
    """The same five columns on every line (a, a, a, a, b): a run start in every group of five samples of every line but the
    first, so in every chunk."""
    return np.tile(np.array([40, 40, 40, 40, 200], dtype=np.uint8), (h, (w + 4) // 5))[:, :w].copy()


def _geometry_frame():
    """4096 x 4 (two lines per tile, four pieces of 16 chunks per line): noise with flat stretches painted where the run
    geometry of the issue needs them; test_run_geometry_frame_is_where_it_should_be says what each one is for."""
    img = synth.frame_numpy(4096, 4, seed=41, kind="noise").copy()
    img[img == 0] = 1
    img[0:3, 0:30] = 50          # a run start at column 0 of line 2, the first line of the second tile: Rc is the sample two lines up
    img[0:2, 62:80] = 60         # a run start in lane 63 (line 1, column 63)
    img[0:2, 1000:1010] = 70     # a run start in the last chunk of a segment (line 1, column 1001)
    img[2:4, 1000:1100] = 80     # a run that starts in piece 0 of line 3 and is interrupted in piece 1
    img[0:2, 4000:4096] = 90     # a run to the end of line 1
    img[2, 2000:2010] = 100      # a run of length 0 on line 3: all gradients zero at column 2001, the sample differs from Ra
    img[3, 2000] = 100
    img[3, 2001] = 7
    img[2:4, 4050:4096] = 110    # a run on line 3 that is interrupted by the last sample of the line
    img[3, 4095] = 9
    img[0, 3000:3020] = 0        # a run start on line 0 (the line above it is zeros)
    return img


# name -> (frame, bits per sample); test_gpu_sort_runs.py runs the same frames through the batch API
FRAMES = {}
for _w, _h in ((2688, 6), (2112, 3),              # segments of more than 16 chunks (21 and 17): a second, partial batch
               (512, 32),                         # two segments per wavefront
               (4096, 4), (8192, 2), (1024, 16),  # exactly 16 chunks per segment
               (4097, 3), (150, 7), (65, 5), (1, 20)):  # partial last chunks, tiny widths
    FRAMES[f"mixed_{_w}x{_h}"] = (lambda w=_w, h=_h: _mixed(w, h), 8)
for _w, _h in ((4096, 4), (8192, 2)):
    for _n in (3, 5):
        FRAMES[f"every_{_n}_{_w}x{_h}"] = (lambda w=_w, h=_h, n=_n: _every(w, h, n), 8)
FRAMES["columns_4096x4"] = (lambda: _columns(4096, 4), 8)
FRAMES["noise_256x8"] = (lambda: np.maximum(synth.frame_numpy(256, 8, seed=23, kind="noise"), 1), 8)  # (no zeros: line 0 lies under zeros)
FRAMES["geometry_4096x4"] = (_geometry_frame, 8)
FRAMES["noise16_256x8"] = T.FRAMES["noise16_256x8"]
FRAMES["every_5_16bit_1024x4"] = (lambda: _every(1024, 4, 5, np.uint16, 30000, 31000), 16)
FRAMES["every_3_16bit_2048x2"] = (lambda: _every(2048, 2, 3, np.uint16, 1000, 65535), 16)


@pytest.fixture(scope="module")
def coded():
    """name -> (frame, the oracle's scan bytes), worked out once."""
    cache = {}

    def get(name):
        if name not in cache:
            make, bits = FRAMES[name]
            img = make()
            h, w = img.shape
            cache[name] = (img, P._scan_bytes(ob.encode(img, width=w, height=h, bits_per_sample=bits)))
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(FRAMES))
def test_frame_equals_oracle(coded, name):
    img, want = coded(name)
    bits = FRAMES[name][1]
    h, w = img.shape
    pc = jls_container.validated_pc((0,) * 5, bits, 0)
    (errc, flags, data), = P._encode_planes([img], w, h, bits, pc, len(want) + 1024, job=512, warm=256)
    assert errc == 0 and flags == 0
    assert data == want


# ---- the frames are where they were meant to be ---------------------------------------------------------------------------------

def test_segment_geometries():
    assert geometry(2688)[3] == 21 and geometry(2112)[3] == 17            # more than one batch of 16 chunks
    assert geometry(512)[0] == 16 and geometry(512)[1] == 1                 # 16 segments on eight wavefronts
    assert [geometry(w)[3] for w in (4096, 8192, 1024)] == [16, 16, 16]
    assert geometry(4096)[:2] == (2, 4) and geometry(8192)[:2] == (1, 8) and geometry(1024)[:2] == (8, 1)
    assert geometry(4097)[2] == 65 and 4097 % 64 == 1 and 150 % 64 != 0 and 65 % 64 == 1
    assert geometry(1024, 16)[:2] == (4, 2) and geometry(2048, 16)[:2] == (2, 4)


@pytest.mark.parametrize("name,most_over", [("every_3_4096x4", 128), ("every_3_8192x2", 128), ("every_5_4096x4", 128),
                                            ("every_5_8192x2", 128), ("columns_4096x4", 128), ("every_5_16bit_1024x4", 64),
                                            ("every_3_16bit_2048x2", 128)])
def test_many_run_starts_in_one_segment(name, most_over):
    """More than 64 / 128 run starts in a segment: the pass behind the chunk loop goes round two / three times and more, and
    its last round is partial."""
    make, bits = FRAMES[name]
    counts = starts_per_segment(make(), bits)
    most = max(counts.values())
    assert most > most_over, counts
    assert any(n > 64 and n % 64 != 0 for n in counts.values()), counts


def test_frames_with_64_to_128_run_starts_in_a_segment():
    """Between 64 and 128: exactly two rounds, the second one partial (the frames above have segments of three and more)."""
    img = _every(4096, 4, 9)
    counts = starts_per_segment(img)
    assert any(64 < n < 128 for n in counts.values()), counts
    want = P._scan_bytes(ob.encode(img, width=4096, height=4))
    pc = jls_container.validated_pc((0,) * 5, 8, 0)
    (errc, flags, data), = P._encode_planes([img], 4096, 4, 8, pc, len(want) + 1024, job=512, warm=256)
    assert errc == 0 and flags == 0 and data == want


def test_no_run_start_at_all_and_one_in_every_chunk():
    # (the first sample of a scan always finds all gradients zero: the run of length 0 there is the one run start no frame is without)
    assert analysis(FRAMES["noise_256x8"][0]()) == [(0, 0, 0, 0)]
    img = _columns(4096, 4)
    seen = {(y, x // 64) for y, x, run, xi in analysis(img)}
    assert all((y, k) in seen for y in range(1, 4) for k in range(64))


def test_run_geometry_frame_is_where_it_should_be():
    img = _geometry_frame()
    lpt, pieces, chunks, cpp = geometry(4096)
    assert (lpt, pieces, cpp) == (2, 4, 16)
    runs = {(y, x): (run, xi) for y, x, run, xi in analysis(img)}
    assert (2, 0) in runs                                               # first line of the second tile, column 0: needs Rc from two lines up
    assert (1, 63) in runs                                              # lane 63
    assert (1, 1001) in runs and (1001 // 64) % cpp == cpp - 1          # the last chunk of a segment
    run, xi = runs[(3, 1001)]                                           # starts in piece 0, interrupted in piece 1
    assert xi == 1100 and (1001 // 64) // cpp == 0 and (xi // 64) // cpp == 1
    assert runs[(1, 4001)] == (95, None)                                # to the end of the line
    assert runs[(3, 2001)] == (0, 2001)                                 # length 0
    assert runs[(3, 4051)][1] == 4095                                   # interrupted by the last sample of the line
    assert any(y == 0 for y, x in runs)                                 # on line 0


# ---- padded rows, an odd base address --------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,bits,cls,base", [(150, 5, 8, "p1", 1),      # stage_lines sample by sample, from an odd address
                                               (150, 5, 16, "r16", 0)])   # and word by word, over the padding of every row
def test_padded_rows(w, h, bits, cls, base):
    g = S.Geometry(w, h, bits)
    lay = S.layout(g, cls, base, 2, "even")
    frames = [S.Coded(g, 5 + 17 * f) for f in range(2)]
    assert any(analysis(fr.img) for fr in frames)  # (run starts among them)
    arena, keep = lay.pad([fr.img for fr in frames]), []
    before = arena.copy()
    descs, wants, outs = [], [], []
    for f, fr in enumerate(frames):
        cont = jls_container.parse(fr.jls)
        pc = jls_container.validated_pc(cont.pc, cont.bits, 0)
        scan = cont.scans[0]
        wants.append(fr.jls[scan.data_start:scan.data_end])
        outs.append(np.zeros(len(wants[-1]) + 64, dtype=np.uint8))
        descs.append(emu_bind.make_desc(w, h, 1, 0, bits, 0, 0, pc, 0, arena[lay.row_offset(f, 0):], lay.stride, outs[-1], keep))
    res = (emu_bind.ScanResult * 2)()
    emu_bind.tile_lib().emu_encode_tile_pipeline((emu_bind.ScanDesc * 2)(*descs), res, 2, 64, 32, 8, 8, 24)
    for k in range(2):
        assert res[k].errc == 0 and outs[k][:res[k].bytes].tobytes() == wants[k], k
    assert np.array_equal(arena, before), "the encoder wrote to its source"


# ---- a destination exactly as large as the stream ------------------------------------------------------------------------------

def test_destination_exactly_as_large_as_the_stream(coded):
    """A many-runs frame: with four bytes to spare the stream is the oracle's, with none the verdict is left to the exact kernel
    (flags 2, as in test_emu_tile_tables), a byte less is destination_too_small; nothing outside the destination is written."""
    img, want = coded("every_3_4096x4")
    errc, flags, data, clean = T._encode_guarded(img, len(want) + 4)
    assert clean and errc == 0 and flags == 0 and data == want
    errc, flags, data, clean = T._encode_guarded(img, len(want))
    assert clean and errc == 0 and flags == 2
    errc, flags, data, clean = T._encode_guarded(img, len(want) - 1)
    assert clean and errc == 3
