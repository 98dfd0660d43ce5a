"""analyze_tiles and P2 of sort_tiles on the CPU (tile_pipeline.hip compiled for the host by tests/emu; the harness of
test_emu_tile_pipeline.py): in P2 the neighbours of a sample taken from the lane next to it -- lane 0 from the chunk in front,
a piece that starts inside a line seeded from LDS, a lane behind the line's end on the line's last column -- and in pass 2 of
analyze_tiles the run state a piece starts in, resolved over the chunks in front of it by one addition over two ballots.  The
frames also hold what a version of pass 1 with all four neighbours from lanes needs (Rd of lane 63 from the chunk behind, Rd
of the line's last column its own Rb), so that the next attempt at it finds its tests.  The scan bytes must be the oracle's.

Every frame is there for a property and asserts in numpy that it has it: `neighbours` restates pass 1 (Ra, Rb, Rc, Rd with
the edge rules), `R.analysis` pass 2 and `geometry` tile_geometry with a lowered tile size."""
import numpy as np
import pytest

import jls_container
import oracle_bind as ob
import test_emu_sort_runs as R
import test_emu_tile_pipeline as P
from charls_amd import synth

T3 = {8: 21, 16: 276}  # default thresholds (ISO/IEC 14495-1 C.2.4.1.1.1): a difference of T3 and more quantises to +-4
WIDTHS = (1, 2, 63, 64, 65, 127, 128, 129, 150, 4095, 4096, 4097)


# ---- what the kernels make of a frame, restated ------------------------------------------------------------------------------

def geometry(w, bits=8, cap=None):
    """lines per tile, pieces per line, chunks per line, chunks per piece (plan_tiles / tile_geometry, planar whole lines);
    cap: CHARLS_AMD_TILE_SAMPLES."""
    limit = 8192 if bits <= 8 else 4096
    if cap is not None:
        limit = min(limit, max(64, cap))
    assert w <= limit, "lines wider than a tile are cut into segments and take the pixel-mode kernels"
    lpt = min(16, limit // w)
    pieces = 1 if lpt >= 8 else 8 // lpt
    chunks = (w + 63) // 64
    return lpt, pieces, chunks, (chunks + pieces - 1) // pieces


def neighbours(img, y):
    """Ra, Rb, Rc, Rd of every sample of line y (pass 1 of analyze_tiles; src/scan_codec.hpp:189-195)."""
    a = img.astype(np.int64)
    w = a.shape[1]
    cur = a[y]
    prev = a[y - 1] if y >= 1 else np.zeros(w, dtype=np.int64)
    edge_a = prev[0]
    edge_c = a[y - 2][0] if y >= 2 else 0
    ra = np.concatenate(([edge_a], cur[:-1]))
    rc = np.concatenate(([edge_c], prev[:-1]))
    rd = np.concatenate((prev[1:], prev[-1:]))
    return ra, prev, rc, rd


def masks(img, y):
    """eq and q0 of line y (lossless: a gradient quantises to 0 only where it is 0)."""
    ra, rb, rc, rd = neighbours(img, y)
    return img[y].astype(np.int64) == ra, (rd == rb) & (rb == rc) & (rc == ra)


def runs_of(img):
    return {(y, x): (run, xi) for y, x, run, xi in R.analysis(img)}


# ---- frames ------------------------------------------------------------------------------------------------------------------

def _mixed(w, h, bits=8):
    """Flat patches in noise-like texture (8 bits: synth's `mixed`); 16 bits: seeded noise over the whole range with flat
    stretches across chunk ends, so that both run mode and the wide quantiser see every lane."""
    if bits == 8:
        return synth.frame_numpy(w, h, seed=w + h, kind="mixed")
    rng = np.random.default_rng(1000 + w + h)
    img = rng.integers(1, 65536, size=(h, w), dtype=np.uint16)
    for x0 in range(40, w, 97):
        img[:, x0:x0 + 30] = 20000 + x0
    return img


def _noise(w, h, seed):
    return np.maximum(synth.frame_numpy(w, h, seed=seed, kind="noise"), 1)  # (no zeros: line 0 lies under zeros)


def _stepped(w, h, dtype=np.uint8, step=40):
    """A ripple that keeps every sample out of run mode, and a step of more than T3 between columns 64 k - 1 and 64 k on every
    line: the contexts at the two sides of every chunk (and so of every piece) need the neighbour from the other chunk."""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return (100 + (x * 7 + y * 3) % 5 + step * ((x // 64) % 2)).astype(dtype)


def _edge_column(w, h):
    """Noise whose column 0 changes by more than T3 from line to line: Rc at x = 0 is the sample two lines up."""
    img = _noise(w, h, 77).copy()
    img[:, 0] = [30 + 70 * (y % 3) for y in range(h)]
    return img


def _look_ahead_frame():
    """4096 x 6 (two lines per tile, four pieces of 16 chunks per line); test_look_ahead_frame_is_where_it_should_be says what
    each stretch is for."""
    img = _noise(4096, 6, 5).copy()
    img[0:2, 500:3500] = 60      # line 1: a run that starts in piece 0 and is interrupted in piece 3
    img[2:4, :] = 80             # line 2: equal samples under a line that keeps q0 false; line 3: a whole flat line
    img[4:6, 900:1024] = 90      # line 5: a run whose last sample is the last sample of piece 0
    img[4:6, 2047:2200] = 95     # a run that starts on the first sample of piece 2
    img[4:6, 3006:3100] = 70     # a run that starts in lane 63 of a chunk (generate in the chunk's last sample)
    return img


def _look_ahead_8192():
    """8192 x 2 (one line per tile, eight pieces of 16 chunks): a run across chunks 63 / 64 -- the end of the look-ahead's
    first round -- and one across pieces 5 to 7, which take two rounds."""
    img = _noise(8192, 2, 9).copy()
    img[0:2, 4000:4200] = 50
    img[0:2, 6000:7500] = 55
    return img


# name -> (frame, bits per sample, CHARLS_AMD_TILE_SAMPLES or None); test_gpu_analyze_lanes.py runs the same frames
FRAMES = {}
for _w in WIDTHS:
    FRAMES[f"mixed_{_w}x4"] = (lambda w=_w: _mixed(w, 4), 8, None)
    FRAMES[f"mixed16_{_w}x3"] = (lambda w=_w: _mixed(w, 3, 16), 16, None)
FRAMES["stepped_4096x4"] = (lambda: _stepped(4096, 4), 8, None)
FRAMES["stepped_4097x3"] = (lambda: _stepped(4097, 3), 8, None)
FRAMES["stepped16_2048x4"] = (lambda: _stepped(2048, 4, np.uint16, 5000), 16, None)
FRAMES["edge_column_4096x6"] = (lambda: _edge_column(4096, 6), 8, None)
FRAMES["edge_column_1100x9"] = (lambda: _edge_column(1100, 9), 8, None)
# one segment of at most 16 chunks per wavefront, or not: (width, height, tile samples)
SHAPES = ((4096, 4, None), (8192, 2, None), (2048, 8, None), (1024, 16, None), (512, 32, None), (4097, 2, None),
          (1100, 10, 5500), (1100, 4, 2200))
for _w, _h, _cap in SHAPES:
    FRAMES[f"shape_{_w}x{_h}" + (f"_cap{_cap}" if _cap else "")] = (lambda w=_w, h=_h: _mixed(w, h), 8, _cap)
FRAMES["look_ahead_4096x6"] = (_look_ahead_frame, 8, None)
FRAMES["look_ahead_8192x2"] = (_look_ahead_8192, 8, None)


@pytest.mark.parametrize("name", list(FRAMES))
def test_frame_equals_oracle(monkeypatch, name):
    make, bits, cap = FRAMES[name]
    if cap is not None:
        monkeypatch.setenv("CHARLS_AMD_TILE_SAMPLES", str(cap))
    img = make()
    h, w = img.shape
    want = P._scan_bytes(ob.encode(img, width=w, height=h, bits_per_sample=bits))
    pc = jls_container.validated_pc((0,) * 5, bits, 0)
    (errc, flags, data), = P._encode_planes([img], w, h, bits, pc, len(want) + 1024, job=512, warm=256)
    assert errc == 0 and flags == 0
    assert data == want


# ---- the frames are where they were meant to be ---------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 16])
def test_widths_have_partial_chunks_a_lone_lane_and_a_last_lane(bits):
    assert {w % 64 for w in WIDTHS} >= {0, 1, 63, 2, 22}  # full, a lone lane, lane 62 last, two lanes, a partial chunk
    for w in WIDTHS:
        if w < 2:
            continue
        make = FRAMES[f"mixed_{w}x4" if bits == 8 else f"mixed16_{w}x3"][0]
        img = make().astype(np.int64)
        # behind the last sample of the line above lies the first of the coded line: Rd of the last column must be its own Rb,
        # and the frame tells the two apart on some line
        assert any(img[y, 0] != img[y - 1, w - 1] for y in range(1, img.shape[0])), w


@pytest.mark.parametrize("name,bits", [("stepped_4096x4", 8), ("stepped_4097x3", 8), ("stepped16_2048x4", 16)])
def test_stepped_frame_needs_the_neighbour_from_the_other_chunk(name, bits):
    img = FRAMES[name][0]()
    h, w = img.shape
    lpt, pieces, chunks, cpp = geometry(w, bits)
    assert pieces > 1 and all((p * cpp * 64) % 64 == 0 for p in range(pieces))  # pieces start where chunks start
    assert set(runs_of(img)) <= {(0, 0)}  # every sample is coded in regular mode: its context counts
    for y in range(1, h):
        ra, rb, rc, rd = neighbours(img, y)
        cur = img[y].astype(np.int64)
        first = np.arange(64, w, 64)  # lane 0 of every chunk but the line's first
        last = first - 1              # lane 63 of the chunk in front
        assert (np.abs(cur[first] - ra[first]) >= T3[bits]).all() and (np.abs(rb[first] - rc[first]) >= T3[bits]).all()
        assert (np.abs(rd[last] - rb[last]) >= T3[bits]).all()
        inner = np.ones(w, dtype=bool)
        inner[first] = False
        assert (np.abs(cur - ra)[inner][1:] < 5).all()  # (elsewhere the lane's own sample would do for its neighbour's)


@pytest.mark.parametrize("name", ["edge_column_4096x6", "edge_column_1100x9"])
def test_edge_column_frame_tells_the_three_sources_of_rc_apart(name):
    make, bits, cap = FRAMES[name]
    img = make().astype(np.int64)
    h, w = img.shape
    lpt = geometry(w)[0]
    assert img[0, 0] >= T3[8]  # line 1: Rc at x = 0 is zero, not the sample above Ra
    later_first = [y for y in range(2, h) if y % lpt == 0]      # a tile's first line: the sample comes from global memory
    later_inner = [y for y in range(2, h) if y % lpt != 0]      # further down in a tile: from the staged lines
    assert later_first and later_inner
    for y in range(2, h):
        assert abs(img[y - 1, 0] - img[y - 2, 0]) >= T3[8]


def test_shapes_keep_or_do_not_keep():
    kept = {}
    for w, h, cap in SHAPES:
        lpt, pieces, chunks, cpp = geometry(w, 8, cap)
        kept[(w, cap)] = min(h, lpt) * pieces <= 8 and cpp <= 16
    assert kept == {(4096, None): True, (8192, None): True, (2048, None): True, (1024, None): True, (512, None): False,
                    (4097, None): True, (1100, 5500): False, (1100, 2200): True}
    assert geometry(512)[0] == 16                                    # two segments per wavefront
    assert geometry(4097)[3] == 9                                    # nine chunks per piece, the last piece short
    assert geometry(1100, 8, 5500)[1:] == (1, 18, 18)                # a piece of more than 16 chunks
    assert geometry(1100, 8, 2200)[1:] == (4, 18, 5)


def test_look_ahead_frame_is_where_it_should_be():
    img = _look_ahead_frame()
    lpt, pieces, chunks, cpp = geometry(4096)
    assert (lpt, pieces, cpp) == (2, 4, 16)
    piece = lambda x: (x // 64) // cpp
    runs = runs_of(img)
    run, xi = runs[(1, 501)]                                         # starts in piece 0, interrupted in piece 3
    assert xi == 3500 and piece(501) == 0 and piece(xi) == 3
    eq, q0 = masks(img, 2)                                           # propagate without generate across all pieces
    assert eq[1:].all() and not q0.any() and not any(y == 2 for y, x in runs)
    assert [(x, r) for (y, x), r in runs.items() if y == 3] in ([(0, (4096, None))], [(1, (4095, None))])  # a whole flat line
    run, xi = runs[(5, 901)]                                         # ends on the last sample of piece 0
    assert xi == 1024 and piece(xi - 1) == 0 and piece(xi) == 1
    assert (5, 2048) in runs and 2048 == 2 * cpp * 64                # starts on the first sample of piece 2
    eq, q0 = masks(img, 5)
    assert (5, 3007) in runs and 3007 % 64 == 63 and eq[3007] and q0[3007] and eq[3008]  # generate in lane 63


def test_look_ahead_8192_frame_is_where_it_should_be():
    img = _look_ahead_8192()
    lpt, pieces, chunks, cpp = geometry(8192)
    assert (lpt, pieces, chunks, cpp) == (1, 8, 128, 16)
    runs = runs_of(img)
    run, xi = runs[(1, 4001)]
    assert 4001 // 64 < 63 and xi == 4200 and xi // 64 > 64            # across chunks 63 / 64
    run, xi = runs[(1, 6001)]
    assert (6001 // 64) // cpp == 5 and (xi // 64) // cpp == 7 and 5 * cpp > 64  # pieces behind chunk 64: two rounds
