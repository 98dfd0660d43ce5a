"""The piece copies of the tile encoder on the CPU (tile_pipeline.hip compiled for the host by tests/emu; the harness of
test_emu_tile_pipeline.py): P3 of sort_tiles / sort_pixel_tiles and the code-word phase of pack_tiles move a tile between its
local order in LDS and the chain-ordered global arrays by FLAT rows of 64 local slots; a lane finds the piece of its slot from
the row's first piece and a mask of the piece starts inside the row.  The scan bytes must be the oracle's.

Every frame sits where that lookup can go wrong, and says so: `pieces` restates in numpy what analyze_tiles makes of a planar
frame (pass 2 decides what a sample is, the context its chain) and lays the tile's non-empty pieces out in local order the way
the offsets phase of sort_tiles does; the tests assert with it that the frame has the property it was built for.

Case h of the issue asks for a non-empty interruption piece with non-empty neighbours on both sides.  In local order only the
zero-context chain (366) lies behind the interruption chain (365); it has events in sample-interleaved scans only, and those
go through sort_pixel_tiles, which copies the interruption piece like any other.  So the planar frame of case h has the
interruption piece behind a non-empty piece inside one flat row and ending inside a row (lanes that store, lanes that are
left out and lanes behind the tile's last slot in one row), and a sample-interleaved frame has chains 365 and 366 both
non-empty, where nothing may be left out."""
import numpy as np
import pytest

import jls_container
import oracle_bind as ob
import test_emu_tile_pipeline as P
from charls_amd import synth

RUN, INTERRUPT, ZERO_CONTEXT = 0, 365, 366


# ---- what the kernels make of a planar frame, restated --------------------------------------------------------------------

def _thresholds(bits):
    """Default T1, T2, T3 of ISO 14495-1 C.2.4.1.1.1 for MAXVAL = 2^bits - 1, NEAR = 0."""
    maxval = (1 << bits) - 1
    if maxval < 128:
        f = 256 // (maxval + 1)
        t1 = max(2, 3 // f)
        t2 = max(t1, 7 // f)
        return t1, t2, max(t2, 21 // f)
    f = (min(maxval, 4095) + 128) // 256
    clamp = lambda v, low: v if low <= v <= maxval else low
    t1 = clamp(f * (3 - 2) + 2, 1)
    t2 = clamp(f * (7 - 3) + 3, t1)
    return t1, t2, clamp(f * (21 - 4) + 4, t2)


def _quantize(d, t):
    t1, t2, t3 = t
    q = np.zeros(d.shape, dtype=np.int64)
    q[d <= -t3] = -4
    q[(d > -t3) & (d <= -t2)] = -3
    q[(d > -t2) & (d <= -t1)] = -2
    q[(d > -t1) & (d < 0)] = -1
    q[(d > 0) & (d < t1)] = 1
    q[(d >= t1) & (d < t2)] = 2
    q[(d >= t2) & (d < t3)] = 3
    q[d >= t3] = 4
    return q


def chains(img, bits=8):
    """The chain of every sample of a planar frame, -1 where it has no event of its own (inside a run): the context
    (1..364) of a regular sample, RUN for a run start, INTERRUPT for the sample that ends a run started earlier (analyze_tiles,
    pass 1 and pass 2)."""
    h, w = img.shape
    a = img.astype(np.int64)
    t = _thresholds(bits)
    out = np.full((h, w), -1, dtype=np.int64)
    zeros = np.zeros(w, dtype=np.int64)
    for y in range(h):
        cur = a[y]
        prev = a[y - 1] if y >= 1 else zeros
        edge_a = prev[0] if y >= 1 else 0
        edge_c = a[y - 2][0] if y >= 2 else 0
        ra = np.concatenate(([edge_a], cur[:-1]))
        rb = prev
        rc = np.concatenate(([edge_c], prev[:-1]))
        rd = np.concatenate((prev[1:], prev[-1:]))
        q = (_quantize(rd - rb, t) * 9 + _quantize(rb - rc, t)) * 9 + _quantize(rc - ra, t)
        eq = cur == ra
        s = False
        for x in range(w):
            q0 = q[x] == 0
            if not (s or q0):
                out[y, x] = abs(q[x])
            elif s and eq[x]:
                pass
            elif s:
                out[y, x] = INTERRUPT
            else:
                out[y, x] = RUN
            s = bool(eq[x]) and (s or q0)
    return out


def tiles(w, h, bits=8, cap=None):
    """The tiles of a planar frame as lists of (line, first column, end column): plan_tiles / tile_span."""
    limit = 8192 if bits <= 8 else 4096
    if cap is not None:
        limit = min(limit, max(64, cap))
    if w <= limit:
        lpt = min(16, limit // w)
        return [[(y, 0, w) for y in range(y0, min(h, y0 + lpt))] for y0 in range(0, h, lpt)]
    max_px = max(64, limit // 64 * 64)
    segs = (w + max_px - 1) // max_px
    seg = ((w + segs - 1) // segs + 63) // 64 * 64
    return [[(y, x0, min(w, x0 + seg))] for y in range(h) for x0 in range(0, w, seg)]


def pieces(img, bits=8, cap=None):
    """Per tile, the non-empty pieces in local order as (chain, first local slot, slots): chains in order, an entry of the run
    chain takes two of the 2-byte slots of 8-bit samples (the offsets phase of sort_tiles)."""
    h, w = img.shape
    ch = chains(img, bits)
    out = []
    for spans in tiles(w, h, bits, cap):
        ids = np.concatenate([ch[y, x0:x1] for y, x0, x1 in spans])
        counts = np.bincount(ids[ids >= 0], minlength=367)
        if bits <= 8:
            counts[RUN] *= 2
        off, tile = 0, []
        for c in np.nonzero(counts)[0]:
            tile.append((int(c), off, int(counts[c])))
            off += int(counts[c])
        out.append(tile)
    return out


def total_slots(tile):
    return tile[-1][1] + tile[-1][2] if tile else 0


def most_starts_in_a_row(tile):
    """The largest number of pieces that start inside one flat row (local slots 64 r + 1 ... 64 r + 63)."""
    rows = {}
    for c, off, n in tile:
        if off % 64:
            rows[off // 64] = rows.get(off // 64, 0) + 1
    return max(rows.values()) if rows else 0


# ---- the frames -------------------------------------------------------------------------------------------------------------

def _mixed(w, h):
    return synth.frame_numpy(w, h, seed=w + h, kind="mixed")


def _aligned():
    """Case a: a flat frame with isolated samples that differ.  The run chain of the only tile has 32 entries: 64 slots, so the
    piece behind it starts on the second flat row's first slot."""
    img = np.full((6, 200), 77, dtype=np.uint8)
    xs = list(range(7, 197, 13))
    for i in range(26):
        img[1 + i % 4, xs[i % len(xs)] + (i // len(xs)) * 3] = 90 + i
    return img


def _run_then_piece():
    """Case g: an odd number of run entries, a regular piece directly behind the run piece."""
    img = np.full((5, 150), 30, dtype=np.uint8)
    img[2, 40] = 31
    img[3, 100] = 99
    return img


def _interrupted():
    """Case h: runs that are interrupted (the interruption chain has slots in the tile's local order and no records), regular
    samples around them."""
    img = synth.frame_numpy(150, 7, seed=9, kind="mixed").copy()
    img[2:5, 20:90] = 50
    img[3, 60] = 200
    img[4, 33] = 1
    return img


def _rgb_zero_context():
    """Case h / i, sample-interleaved: flat patches in ONE component (the zero-context chain) and in all of them (runs with
    interruptions)."""
    img = P._rgb(70, 9, seed=12, flat=1.5).copy()
    img[1:4, 5:40, 1] = 17
    return img


# name -> (frame, bits per sample, CHARLS_AMD_TILE_SAMPLES or None, CHARLS_AMD_PIXEL_MODE); planar frames of one component
FRAMES = {
    "a_aligned_200x6": (_aligned, 8, None, False),
    "b_hard_300x9": (lambda: synth.frame_numpy(300, 9, seed=3, kind="hard"), 8, None, False),
    "b_noise_256x8": (lambda: synth.frame_numpy(256, 8, seed=23, kind="noise"), 8, None, False),
    "c_flat_4096x4": (lambda: np.full((4, 4096), 77, dtype=np.uint8), 8, None, False),
    "c_zero_4096x4": (lambda: np.zeros((4, 4096), dtype=np.uint8), 8, None, False),
    "d_mixed_150x7": (lambda: _mixed(150, 7), 8, None, False),
    "d_mixed_65x5": (lambda: _mixed(65, 5), 8, None, False),
    "d_mixed_1x20": (lambda: _mixed(1, 20), 8, None, False),
    "e_mixed_8192x1": (lambda: _mixed(8192, 1), 8, None, False),
    "e_mixed_4096x2": (lambda: _mixed(4096, 2), 8, None, False),
    "f_noise16_256x8": (lambda: synth.frame_numpy(256, 8, seed=21, bits=16, kind="noise"), 16, None, False),
    "f_mixed16_256x8": (lambda: synth.frame_numpy(256, 8, seed=22, bits=16, kind="mixed"), 16, None, False),
    "g_run_then_piece_150x5": (_run_then_piece, 8, None, False),
    "h_interrupted_150x7": (_interrupted, 8, None, False),
    "i_planar_in_pixel_mode_130x11": (lambda: _mixed(130, 11), 8, None, True),
    "j_cut_700x5": (lambda: _mixed(700, 5), 8, 192, False),
    "j_cut16_300x4": (lambda: synth.frame_numpy(300, 4, seed=7, bits=16, kind="mixed"), 16, 64, False),
}
# sample-interleaved frames (sort_pixel_tiles): name -> (frame, CHARLS_AMD_TILE_SAMPLES or None)
RGB_FRAMES = {
    "i_rgb_70x9": (_rgb_zero_context, None),
    "i_rgb_cut_70x9": (_rgb_zero_context, 128),
}


def _set_knobs(monkeypatch, cap, pixel):
    if cap is not None:
        monkeypatch.setenv("CHARLS_AMD_TILE_SAMPLES", str(cap))
    if pixel:
        monkeypatch.setenv("CHARLS_AMD_PIXEL_MODE", "1")


@pytest.mark.parametrize("name", list(FRAMES))
def test_frame_equals_oracle(monkeypatch, name):
    make, bits, cap, pixel = FRAMES[name]
    _set_knobs(monkeypatch, cap, pixel)
    img = make()
    h, w = img.shape
    want = P._scan_bytes(ob.encode(img, width=w, height=h, bits_per_sample=bits))
    pc = jls_container.validated_pc((0,) * 5, bits, 0)
    (errc, flags, data), = P._encode_planes([img], w, h, bits, pc, len(want) + 1024, job=512, warm=256)
    assert errc == 0 and flags == 0
    assert data == want


@pytest.mark.parametrize("name", list(RGB_FRAMES))
def test_sample_interleaved_frame_equals_oracle(monkeypatch, name):
    make, cap = RGB_FRAMES[name]
    _set_knobs(monkeypatch, cap, False)
    img = make()
    h, w, comps = img.shape
    want = P._scan_bytes(ob.encode(img, width=w, height=h, component_count=comps, interleave_mode=2))
    errc, flags, data = P._encode_scan(img, w, h, comps, 2, 8)
    assert errc == 0 and data == want


# ---- the frames are where they were meant to be -----------------------------------------------------------------------------

def _tiles_of(name):
    make, bits, cap, pixel = FRAMES[name]
    return pieces(make(), bits, cap)


def test_model_thresholds():
    assert _thresholds(8) == (3, 7, 21) and _thresholds(16) == (18, 67, 276) and _thresholds(12) == (18, 67, 276)


def test_a_piece_starts_on_a_row_and_a_piece_fills_a_row():
    tile, = _tiles_of("a_aligned_200x6")
    assert tile[0] == (RUN, 0, 64)                          # exactly one flat row
    assert tile[1][1] == 64 and len(tile) > 2               # the piece behind it starts on the second row's first slot


def test_b_many_pieces_in_one_row():
    for name in ("b_hard_300x9", "b_noise_256x8"):
        assert max(most_starts_in_a_row(t) for t in _tiles_of(name)) >= 8, name
    # (and a row with a start bit in each half of its mask)
    assert any(off % 64 > 32 for t in _tiles_of("b_noise_256x8") for c, off, n in t)


def test_c_one_piece_and_no_regular_event():
    first, second = _tiles_of("c_flat_4096x4")              # two lines per tile
    assert len(first) > 1 and second == [(RUN, 0, 4)]       # the second tile: two runs to the end of their lines
    for tile in _tiles_of("c_zero_4096x4"):
        assert tile == [(RUN, 0, 4)]


def test_d_partial_last_row_and_less_than_a_row():
    for name in ("d_mixed_150x7", "d_mixed_65x5"):
        tile, = _tiles_of(name)
        assert total_slots(tile) > 64 and total_slots(tile) % 64 != 0, name
    for tile in _tiles_of("d_mixed_1x20"):                   # (16 lines per tile: two tiles)
        assert 0 < total_slots(tile) < 64


def test_e_full_tiles():
    for name, count in (("e_mixed_8192x1", 1), ("e_mixed_4096x2", 1)):
        make, bits, cap, pixel = FRAMES[name]
        h, w = make().shape
        spans = tiles(w, h)
        assert len(spans) == count and sum(x1 - x0 for y, x0, x1 in spans[0]) == 8192
    tile, = _tiles_of("e_mixed_8192x1")
    assert total_slots(tile) > 128 * 64                     # 129 flat rows: the eight wavefronts of pack_tiles take a second batch
    tile, = _tiles_of("e_mixed_4096x2")
    assert total_slots(tile) > 100 * 64 and len(tile) > 100 and most_starts_in_a_row(tile) >= 8


def test_f_wide_samples_take_one_slot_per_run_entry():
    for name in ("f_noise16_256x8", "f_mixed16_256x8"):
        make, bits, cap, pixel = FRAMES[name]
        img = make()
        starts = int((chains(img, 16) == RUN).sum())
        assert starts >= 1 and sum(n for t in pieces(img, 16) for c, off, n in t if c == RUN) == starts
    assert max(most_starts_in_a_row(t) for t in _tiles_of("f_noise16_256x8")) >= 8


def test_g_run_piece_ends_on_an_odd_slot_inside_a_row():
    tile, = _tiles_of("g_run_then_piece_150x5")
    c, off, n = tile[0]
    assert c == RUN and (n // 2) % 2 == 1 and (off + n - 1) % 2 == 1 and n % 64 != 0
    assert tile[1][1] == n and tile[1][0] != INTERRUPT      # a regular piece directly behind it, in the same flat row


def test_h_interruption_piece_inside_a_row():
    tile, = _tiles_of("h_interrupted_150x7")
    assert tile[-1][0] == INTERRUPT and tile[-1][2] >= 2
    c, off, n = tile[-1]
    assert off % 64 != 0 and tile[-2][2] > 0                # lanes of one row store the piece before it and leave this one out
    assert (off + n) % 64 != 0                              # and the row goes on behind the tile's last slot
    img = _rgb_zero_context()                               # sample-interleaved: component 1 is flat where component 0 is not,
    assert (img[1:4, 5:40, 1] == 17).all()                  # so its gradients are all zero outside run mode: the zero-context chain
    assert (img[2:4, 6:40, 0] != img[2:4, 5:39, 0]).any()


def test_i_pixel_mode_is_forced():
    make, bits, cap, pixel = FRAMES["i_planar_in_pixel_mode_130x11"]
    assert pixel and len(pieces(make(), bits)) == 1 and total_slots(pieces(make(), bits)[0]) % 64 != 0


def test_j_many_short_tiles_and_a_short_last_one():
    spans = tiles(700, 5, 8, 192)
    assert len(spans) == 20 and [x1 - x0 for (y, x0, x1), in spans[:4]] == [192, 192, 192, 124]
    got = _tiles_of("j_cut_700x5")
    assert len(got) == 20 and all(total_slots(t) > 0 for t in got)
    assert any(total_slots(t) < 64 for t in got) or any(total_slots(t) % 64 for t in got)
    spans = tiles(300, 4, 16, 64)
    assert len(spans) == 20 and [x1 - x0 for (y, x0, x1), in spans[:5]] == [64, 64, 64, 64, 44]
