"""Encoding to a byte budget (charls_amd.h part 2f) beside what a caller had before it, every figure from the same run (host
clock around calls that end in a synchronise; every time of --repeats (2) is printed after one warm-up):

 (a) charls_amd_measure_batch_device with 1, 2, 4 and 8 candidate NEARs over --frames (256) frames of --size (1024) squared
     8-bit gray, half `gradient` and half `noise` (charls_amd/synth.py): K candidates are K x frames chains in one launch;
 (b) charls_amd_encode_batch_device_budget with 8 candidates and budgets at 60 % of every frame's lossless size;
 (c) the same selection with the calls that were there before: one charls_amd_encode_batch_device per candidate into slots
     of the estimated size, the sizes compared on the host, the chosen (frame, NEAR) pairs coded by
     charls_amd_encode_batch_device_ragged.  Choices and bytes of (b) and (c) are compared;
 (d) the HBM each route holds: the library's work areas (charls_amd_work_area_bytes) plus what the caller had to allocate.
Run on the GPU box: python tools/budget_encode_probe.py [--frames 256] [--size 1024] [--out profiles/r13_budget_encode.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from charls_amd import batch, capi, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--repeats", type=int, default=2)
ap.add_argument("--share", type=float, default=0.6, help="budget as a share of the frame's lossless size")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_budget_encode.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("budget_encode_probe.py measures on the GPU: no device found")
lib = capi.load_product()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
log = open(args.out, "w")
CANDIDATES = [0, 1, 2, 3, 4, 6, 8, 12]


def say(text):
    print(text, flush=True)
    log.write(text + "\n")
    log.flush()


def wall(fn):
    torch.cuda.synchronize()
    a = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - a) * 1e3, out


def timed(what, fn):
    runs = [wall(fn) for _ in range(args.repeats)]
    times = [t for t, _ in runs]
    say(f"  {what:<70} {'  '.join(f'{t:10.2f}' for t in times)} ms   best {min(times):10.2f}")
    return min(times), runs[-1][1]


N, S = args.frames, args.size
say(f"{torch.cuda.get_device_name(0)}; {N} frames of {S} x {S} 8-bit gray, half gradient (seeds 100 + f), half noise (seeds 500 + f)")
frames = torch.cat([synth.frames_torch(N // 2, S, S, seed0=100, kind="gradient", device="cuda:0"),
                    synth.frames_torch(N - N // 2, S, S, seed0=500, kind="noise", device="cuda:0")])
pixels = N * S * S

# ---- (a) sizes without streams
say(f"(a) measure_batch: K candidates = K x {N} chains in one launch, {N} x K x 16 bytes of results")
batch.release_work_areas(lib)
idle = batch.work_area_bytes(lib)
batch.measure_batch(frames, CANDIDATES[:1], lib=lib)  # warm-up: module load
sizes = None
for k in (1, 2, 4, 8):
    before = batch.measure_counters(lib)
    best, sizes = timed(f"measure_batch, {k} candidate(s) {CANDIDATES[:k]}", lambda: batch.measure_batch(frames, CANDIDATES[:k], lib=lib))
    after = batch.measure_counters(lib)
    say(f"    {k * pixels / best / 1e3:9.1f} MPix/s of chains walked; scans by the measuring kernel {(after[0] - before[0]) // args.repeats}, "
        f"launches {(after[1] - before[1]) // args.repeats}, scans coded for real {after[2] - before[2]}")
measure_held = batch.work_area_bytes(lib) - idle
lossless = sizes[:, 0].astype(np.float64)
say(f"  lossless bytes per frame: gradient median {np.median(lossless[:N // 2]):.0f}, noise median {np.median(lossless[N // 2:]):.0f}")

# ---- (b) the budget call
budgets = np.floor(lossless * args.share).astype(np.uint64)
total_budget = int(budgets.sum())
packed = torch.empty(total_budget + 4096, dtype=torch.uint8, device="cuda:0")
say(f"(b) encode_batch_budget: 8 candidates {CANDIDATES}, budgets at {args.share:.0%} of the lossless size ({total_budget} bytes in all)")
batch.release_work_areas(lib)
best_b, (result, nears) = timed("encode_batch_budget (measure, select, code the chosen pairs, pack)",
                                lambda: batch.encode_batch_budget(frames, budgets, CANDIDATES, packed, lib=lib))
budget_held = batch.work_area_bytes(lib) - idle
chosen, counts = np.unique(nears, return_counts=True)
say(f"    NEAR chosen -> frames: {dict(zip(chosen.tolist(), counts.tolist()))}; {int(result.offsets[-1])} bytes packed; "
    f"{pixels / best_b / 1e3:.1f} MPix/s of frames delivered")
assert all(int(result.sizes[f]) <= int(budgets[f]) for f in range(N) if nears[f] >= 0)

# ---- (c) the same selection with the calls that were there before
say("(c) the same selection without part 2f: one encode_batch_device per candidate into slots, sizes compared on the host, then ragged")
# (twice the frame: the lossless stream of a noise frame is a little longer than part 1's estimated destination size, which the
# budget call does not depend on -- its staging slots are sized by the measured streams)
slot = (2 * S * S + 4096 + 255) & ~255
slots = torch.empty((N, slot), dtype=torch.uint8, device="cuda:0")
packed_c = torch.empty_like(packed)


def by_hand():
    table = np.zeros((N, len(CANDIDATES)), dtype=np.uint64)
    for k, near in enumerate(CANDIDATES):
        enc = batch.encode_batch(frames, near_lossless=near, streams=slots, lib=lib)
        assert not enc.errcs.any()
        table[:, k] = enc.sizes
    pick = [next((k for k in range(len(CANDIDATES)) if table[f, k] <= budgets[f]), -1) for f in range(N)]
    keep = [f for f in range(N) if pick[f] >= 0]
    params = [batch.codec_params(S, S, near_lossless=CANDIDATES[pick[f]]) for f in keep]
    r = batch.encode_batch_ragged([frames[f] for f in keep], params, packed_c, lib=lib)
    assert not r.errcs.any()
    return table, pick, r


batch.release_work_areas(lib)
best_c, (table, pick, ragged) = timed("8 x encode_batch_device + host selection + encode_batch_device_ragged", by_hand)
hand_held = batch.work_area_bytes(lib) - idle
assert np.array_equal(table, sizes), "the measured sizes are not the sizes of the streams"
assert [CANDIDATES[k] if k >= 0 else -1 for k in pick] == nears.tolist(), "the two routes chose differently"
total = int(result.offsets[-1])
assert int(ragged.offsets[-1]) == total and torch.equal(packed[:total], packed_c[:total]), "the two routes wrote different bytes"
say(f"  same sizes, same choices, same {total} bytes; budget call / by hand, best of each: {best_b / best_c:.3f}")

# ---- (d) memory
say("(d) HBM held beyond the frames and the packed result")
say(f"  measure_batch, 8 candidates: work areas {measure_held} bytes + {N * 8 * (16 + 88)} bytes of descriptors and results during the call")
say(f"  encode_batch_budget:         work areas {budget_held} bytes (staging slots sized by the largest chosen stream)")
say(f"  by hand:                     work areas {hand_held} bytes + {N * slot} bytes of slots the caller allocates")
log.close()
