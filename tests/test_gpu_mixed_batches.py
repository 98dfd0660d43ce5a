"""Batch decode of batches whose frames differ in their coding parameters (charls_amd.h part 2: every slot holds a complete
.jls file and decodes as the part-1 decoder would decode it).  The launch key (decode_launch.hip: decode_launch_key) puts scans of
one width, layout and sample type into one launch whose kernel is chosen from its first scan; a workgroup of the group
decoder builds its gradient table from its own first scan, and everything the scans of a wavefront do not share in the step
loop (RESET, the height) is per lane.  So each batch here is built frame by frame with the oracle (the product's encoder
for restart intervals, which the reference cannot write), and every frame must get:
  * the oracle's error code,
  * the oracle's bytes,
  * its slot untouched past its own extent (the slots are filled with a canary first: a kernel that took the height or the
    size of another frame of its launch writes over it),
and the count of scans the speed path handed to the exact decoder (engine counter exact_retry_scans) must move as the
batch's mix says: not at all where only per-lane parameters differ, by at least one where a workgroup's table does not fit
a scan.  GPU only."""
import ctypes as C
import random

import numpy as np
import pytest

import oracle_bind as ob
from charls_amd import batch, capi, synth

pytestmark = pytest.mark.gpu

CANARY = 0xA5


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def default_preset(bits, near):
    """(0, T1, T2, T3, RESET) with the default thresholds of the sample precision spelled out (src/jpegls_preset_coding_parameters.hpp)."""
    out = (C.c_int32 * 5)()
    ob.lib().jls_oracle_default_pc((1 << bits) - 1, near, out)
    return (0, out[1], out[2], out[3], out[4])


class Frame:
    """One slot of a batch: its stream, what the oracle decodes from it, and how many scans it has."""

    def __init__(self, width, height, *, bits=8, comps=1, ilv=0, near=0, preset=None, kind="mixed", seed=1, restart=0):
        self.what = dict(width=width, height=height, bits=bits, comps=comps, ilv=ilv, near=near, preset=preset, kind=kind, seed=seed,
                         restart=restart)
        img = synth.frame_numpy(width, height, seed=seed, bits=bits, components=comps, kind=kind, interleaved=ilv != 0)
        self.extent = width * height * comps * ((bits + 7) // 8)
        # (room for the worst case of few bits per sample: a limited-length code per sample)
        kw = dict(width=width, height=height, bits_per_sample=bits, component_count=comps, near_lossless=near, interleave_mode=ilv,
                  preset=preset, destination_size=8 * width * height * comps + 4096)
        if restart:
            self.jls = capi.load_product().encode(img, restart_interval=restart, **kw)
        else:
            self.jls = ob.encode(img, **kw)
        self.scans = comps if ilv == 0 and comps > 1 else 1
        self.expect()

    def expect(self):
        try:
            self.errc, self.pixels = 0, ob.decode(self.jls)[1].tobytes()
        except ob.OracleError as e:
            self.errc, self.pixels = e.errc, None

    def damaged(self, jls):
        self.jls = bytes(jls)
        self.expect()
        return self

    def __repr__(self):
        return f"Frame({self.what})"


def retries():
    return capi.engine_counters()["exact_retry_scans"]


def stage(torch, frames):
    """The streams of `frames` in (F, pitch) slots on the device, and their sizes."""
    pitch = (max(len(f.jls) for f in frames) + 255) & ~255
    host = np.zeros((len(frames), pitch), dtype=np.uint8)
    for i, f in enumerate(frames):
        host[i, :len(f.jls)] = np.frombuffer(f.jls, dtype=np.uint8)
    return torch.from_numpy(host).cuda(), np.array([len(f.jls) for f in frames], dtype=np.uint64)


def check_slots(frames, errcs, out):
    for i, f in enumerate(frames):
        assert errcs[i] == f.errc, (i, f, int(errcs[i]), f.errc)
        if f.pixels is not None:
            assert out[i, :len(f.pixels)].tobytes() == f.pixels, (i, f)
        tail = out[i, f.extent:]
        assert (tail == CANARY).all(), (i, f, "wrote past its own extent at", f.extent + int(np.argmax(tail != CANARY)))


def decode(torch, frames, *, odd_pitch=False):
    """Decodes `frames` as ONE batch into canary-filled uint8 slots, checks every slot, returns (the rise of the retry count,
    errcs, slots)."""
    streams, sizes = stage(torch, frames)
    pitch = max(f.extent for f in frames) + 64
    pitch += (pitch + 1) % 2 if odd_pitch else pitch % 2
    out = torch.full((len(frames), pitch), CANARY, dtype=torch.uint8, device="cuda")
    before = retries()
    _, errcs, _ = batch.decode_batch(streams, sizes, out)
    torch.cuda.synchronize()
    rise = retries() - before
    host = out.cpu().numpy()
    check_slots(frames, errcs, host)
    return rise, errcs, host


def scans(frames):
    return sum(f.scans for f in frames)


# ---- the step loop with lanes that differ in RESET and in height -------------------------------------------------------

@pytest.mark.parametrize("group", [8, 16, 32])
@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("bits,near", [(8, 0), (8, 2), (12, 0), (12, 2)])
def test_fast_path_mixes_reset_and_height_in_one_wavefront(torch, knobs, group, waves, bits, near):
    """One width, one sample precision, one set of T1..T3: only RESET (per lane in the loop's configuration word), the height
    (each scan ends its own lines) and the data differ, neighbour to neighbour.  No scan may leave the speed path."""
    knobs.set("DECODE_GROUP", group)
    knobs.set("DECODE_WORKGROUP_WAVES", waves)
    pc = default_preset(bits, near)
    resets = (64, 5, 255, 17, 100, 3, 32)
    heights = (17, 40, 5, 64, 1, 23, 33, 2)
    kinds = ("mixed", "hard", "zero", "gradient", "noise")
    frames = [Frame(150, heights[i % len(heights)], bits=bits, near=near, preset=pc[:4] + (resets[i % len(resets)],),
                    kind=kinds[i % len(kinds)], seed=100 + i) for i in range(44)]
    rise, _, _ = decode(torch, frames)
    assert rise == 0, "a scan that differs from its wavefront only in RESET or height was handed to the exact decoder"


# ---- scans the group kernel must hand over: its workgroup's table does not fit them -------------------------------------

def _with_odd(frames, odd, first):
    return [odd] + frames if first else frames[:5] + [odd] + frames[5:]


@pytest.mark.parametrize("first", [True, False], ids=["odd_first", "odd_later"])
@pytest.mark.parametrize("mix", ["thresholds", "near", "bits"])
def test_retry_path_takes_scans_the_table_does_not_fit(torch, knobs, mix, first):
    knobs.set("DECODE_GROUP", 16)
    w = 120
    if mix == "thresholds":
        frames = [Frame(w, 20 + i, kind="mixed", seed=200 + i) for i in range(10)]
        odd = Frame(w, 31, preset=(0, 5, 11, 40, 0), kind="hard", seed=299)
    elif mix == "near":
        # NEAR = 2 and NEAR = 3 share a launch (lossless frames of the width do not: the key holds near-lossless)
        frames = [Frame(w, 20 + i, near=2, kind="mixed", seed=200 + i) for i in range(8)] + \
                 [Frame(w, 12 + i, kind="hard", seed=250 + i) for i in range(3)]
        odd = Frame(w, 31, near=3, kind="hard", seed=299)
    else:
        frames = [Frame(w, 20 + i, bits=(7, 8)[i % 2], kind="mixed", seed=200 + i) for i in range(10)]
        odd = Frame(w, 31, bits=5, kind="hard", seed=299)
    batch_frames = _with_odd(frames, odd, first)
    rise, _, _ = decode(torch, batch_frames)
    assert 1 <= rise <= scans(batch_frames), rise


def t3_beyond_table_batch():
    """A 16-bit lossless frame whose T3 (2000) is beyond the group kernel's table (kMaxTableT3) ahead of 16-bit NEAR = 3
    frames of its width: the first scan of a launch chooses the kernel, and decode_scans_fast has no near-lossless code."""
    pc = default_preset(16, 0)
    return [Frame(160, 24, bits=16, preset=(0, pc[1], pc[2], 2000, 0), kind="hard", seed=300)] + \
           [Frame(160, 10 + 3 * i, bits=16, near=3, kind=("mixed", "hard")[i % 2], seed=301 + i) for i in range(6)]


def test_near_lossless_scans_stay_off_the_lossless_kernel(torch):
    frames = t3_beyond_table_batch()
    rise, _, _ = decode(torch, frames)
    assert rise == 0, "near-lossless scans went through a kernel without near-lossless code"


# ---- layouts and addresses ------------------------------------------------------------------------------------------------

def test_planar_line_and_sample_frames_beside_gray_frames(torch):
    """Gray frames and planar RGB frames of one width share a key (the component scans go through the one-launch planar
    path and find_scan_end); a line-interleaved and a sample-interleaved frame of the width sit among them."""
    w = 96
    frames = []
    for i in range(4):
        frames.append(Frame(w, 30 + i, kind="mixed", seed=400 + i))
        frames.append(Frame(w, 17 + 5 * i, comps=3, ilv=0, kind=("hard", "mixed")[i % 2], seed=410 + i))
    frames.insert(3, Frame(w, 21, comps=3, ilv=1, kind="mixed", seed=420))
    frames.insert(6, Frame(w, 13, comps=3, ilv=2, kind="hard", seed=421))
    frames.append(Frame(w, 9, comps=3, ilv=1, near=2, kind="hard", seed=422))
    rise, _, _ = decode(torch, frames)
    assert rise == 0


@pytest.mark.parametrize("bits", [12, 16])
def test_wide_frames_at_odd_addresses(torch, bits):
    """Slots of an odd size: every other 16-bit frame starts at an odd address, is not wave-decode eligible and goes to
    another launch than its neighbours."""
    frames = [Frame(70, 11 + 4 * i, bits=bits, kind=("mixed", "hard")[i % 2], seed=500 + i) for i in range(7)]
    frames.append(Frame(70, 15, bits=bits, comps=3, ilv=2, kind="mixed", seed=510))
    frames.append(Frame(70, 15, bits=bits, comps=3, ilv=0, kind="hard", seed=511))
    rise, _, _ = decode(torch, frames, odd_pitch=True)
    assert rise == 0


# ---- restart intervals ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sequential", [None, 1], ids=["interval_parallel", "sequential_intervals"])
def test_restart_intervals_mixed_with_plain_frames(torch, knobs, sequential):
    """Frames with a restart interval shorter than the height, one at least the height, and none, of one width.  With
    SEQUENTIAL_INTERVALS = 1 the ones with markers share the plain frames' launch: the group kernel meets an RSTm inside
    the scan and hands exactly those scans to the exact decoder."""
    if sequential is not None:
        knobs.set("SEQUENTIAL_INTERVALS", sequential)
    knobs.set("DECODE_GROUP", 16)
    w = 110
    spec = [(40, 7), (40, 0), (33, 40), (25, 5), (48, 0), (12, 12), (40, 7), (31, 64), (20, 0), (64, 9)]
    frames = [Frame(w, h, restart=r, kind=("mixed", "hard", "gradient")[i % 3], seed=600 + i) for i, (h, r) in enumerate(spec)]
    with_markers = sum(1 for h, r in spec if 0 < r < h)
    rise, _, _ = decode(torch, frames)
    assert rise == (with_markers if sequential else 0), rise


# ---- damage -----------------------------------------------------------------------------------------------------------------

def test_damaged_streams_among_healthy_frames(torch, knobs):
    knobs.set("DECODE_GROUP", 16)
    w = 128
    pc8 = default_preset(8, 0)
    frames = [Frame(w, 20 + 3 * i, near=(0, 0, 2)[i % 3], preset=pc8[:4] + ((64, 9, 200)[i % 3],) if i % 3 != 2 else None,
                    kind=("mixed", "hard")[i % 2], seed=700 + i) for i in range(9)]
    frames.append(Frame(w, 30, bits=12, kind="hard", seed=720))
    cut = Frame(w, 40, kind="hard", seed=730)
    cut.damaged(cut.jls[:len(cut.jls) * 3 // 5])
    smashed = Frame(w, 40, kind="mixed", seed=731)
    j = bytearray(smashed.jls)
    j[len(j) // 2:len(j) // 2 + 6] = b"\xff" * 6
    smashed.damaged(j)
    assert cut.errc != 0 and smashed.errc != 0
    frames.insert(2, cut)
    frames.insert(7, smashed)
    rise, errcs, _ = decode(torch, frames)
    assert rise <= 2, rise  # (only the damaged scans may be handed over)
    assert sum(1 for e in errcs if e != 0) == 2


# ---- several shards ---------------------------------------------------------------------------------------------------------

def test_mixed_batch_through_two_shards_on_one_device(torch, knobs):
    pc = default_preset(8, 0)
    frames = [Frame(140, (9, 30, 17, 44)[i % 4], preset=pc[:4] + ((64, 7, 130)[i % 3],), kind=("mixed", "hard", "zero")[i % 3],
                    seed=800 + i) for i in range(13)]
    frames += [Frame(140, 21, bits=12, kind="hard", seed=850), Frame(140, 19, comps=3, ilv=0, seed=851),
               Frame(140, 12, near=2, seed=852)]
    random.Random(3).shuffle(frames)
    rise, errcs_one, out_one = decode(torch, frames)
    assert rise == 0
    streams, sizes = stage(torch, frames)
    pitch = out_one.shape[1]
    k = 7
    outs = [torch.full((k, pitch), CANARY, dtype=torch.uint8, device="cuda"),
            torch.full((len(frames) - k, pitch), CANARY, dtype=torch.uint8, device="cuda")]
    before = retries()
    _, errcs = batch.decode_batch_devices([streams[:k].contiguous(), streams[k:].contiguous()], sizes, outs)
    torch.cuda.synchronize()
    assert retries() == before
    host = np.concatenate([o.cpu().numpy() for o in outs])
    assert list(errcs) == list(errcs_one)
    assert np.array_equal(host, out_one)
    check_slots(frames, errcs, host)


# ---- seeded sweep -------------------------------------------------------------------------------------------------------

def _random_frame(rng, width, seed):
    bits = rng.choice((2, 5, 7, 8, 8, 8, 10, 12, 12, 16, 16))
    maxval = (1 << bits) - 1
    near = min(rng.choice((0, 0, 0, 1, 2, 3)), maxval // 2)
    comps, ilv = rng.choice(((1, 0), (1, 0), (1, 0), (3, 0), (3, 1), (3, 2), (2, 1)))
    preset = None
    roll = rng.random()
    if roll < 0.3:  # RESET only
        preset = default_preset(bits, near)[:4] + (rng.choice((3, 9, 31, 64, 200, 255)),)
    elif roll < 0.5 and maxval >= 16:  # thresholds of its own (16-bit: now and then beyond the group kernel's table)
        d = default_preset(bits, near)
        t1 = min(maxval, d[1] + rng.randrange(0, 4))
        t2 = min(maxval, max(t1, d[2] + rng.randrange(-1, 6)))
        t3 = min(maxval, max(t2, d[3] + rng.randrange(0, 30)))
        if bits == 16 and rng.random() < 0.3:
            t3 = 1500
        preset = (0, t1, t2, t3, 0)
    height = rng.randrange(1, 65)
    kind = rng.choice(("mixed", "hard", "gradient", "zero", "noise"))
    try:
        return Frame(width, height, bits=bits, comps=comps, ilv=ilv, near=near, preset=preset, kind=kind, seed=seed)
    except ob.OracleError:  # (thresholds the standard does not allow for this precision and NEAR)
        return Frame(width, height, bits=bits, comps=comps, ilv=ilv, near=near, kind=kind, seed=seed)


@pytest.mark.parametrize("case", range(7))
def test_seeded_sweep_of_mixed_batches(torch, knobs, case):
    rng = random.Random(9000 + case)
    width = rng.randrange(1, 301)
    if case % 3 == 1:
        knobs.set("DECODE_GROUP", rng.choice((8, 16, 32)))
        knobs.set("DECODE_WORKGROUP_WAVES", rng.choice((1, 4)))
    frames = [_random_frame(rng, width, 9100 + 100 * case + i) for i in range(rng.randrange(24, 97))]
    rise, _, _ = decode(torch, frames, odd_pitch=case % 2 == 1)
    assert 0 <= rise <= scans(frames), rise
