"""What the salvage round (charls_amd.h part 2g) costs, beside the ordinary decode of the same frames intact, every figure from
the same run and by device events around calls that end in a synchronise: by default 256 frames of 1024 x 1024 8-bit gray
(charls_amd/synth.py, seeds 100 + f) coded with a restart interval of 32 rows; in the damaged copy four bytes in the middle of
one interval of every frame are zeroed (interval f mod N of frame f).  A warm-up of each side, then --repeats rounds (3) in
which the sides take turns; every time is printed.  The damaged batch pays round 1 (which fails every frame) and round 2.
Run on the GPU box: python tools/salvage_batch_bench.py [--frames 256] [--size 1024] [--interval 32] [--out profiles/r16_salvage_batch.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from charls_amd import batch, capi, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--interval", type=int, default=32)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_salvage_batch.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("salvage_batch_bench.py measures on the GPU: no device found")
lib = capi.load_product()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
log = open(args.out, "w")


def say(text):
    print(text, flush=True)
    log.write(text + "\n")
    log.flush()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


F, S, RI = args.frames, args.size, args.interval
N = -(-S // RI)
say(f"{torch.cuda.get_device_name(0)}; {F} frames of {S} x {S} 8-bit gray (synth seeds 100 + f), restart interval {RI} rows ({N} intervals)")
frames = synth.frames_torch(F, S, S, seed0=100, device="cuda:0")
enc = batch.encode_batch(frames, restart_interval=RI, lib=lib)
assert (enc.errcs == 0).all()
host = enc.streams.cpu().numpy()
sound = [host[f, :int(enc.sizes[f])].tobytes() for f in range(F)]
damaged, hit = [], []
for f, jls in enumerate(sound):
    data = bytearray(jls)
    a = np.frombuffer(jls, dtype=np.uint8)
    marks = np.flatnonzero((a[:-1] == 0xFF) & (a[1:] >= 0xD0) & (a[1:] <= 0xD7)).tolist()
    assert len(marks) == N - 1, (f, len(marks))
    j = f % N
    sos = jls.rfind(b"\xff\xda")
    start = sos + 2 + int.from_bytes(jls[sos + 2:sos + 4], "big") if j == 0 else marks[j - 1] + 2
    end = marks[j] if j < N - 1 else len(data) - 2
    at = (start + end) // 2 - 2
    data[at:at + 4] = bytes(4)
    damaged.append(bytes(data))
    hit.append(j)


def pack(streams):
    sizes = np.array([len(s) for s in streams], dtype=np.uint64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    blob = np.frombuffer(b"".join(streams) + bytes(16), dtype=np.uint8).copy()
    return torch.from_numpy(blob).cuda(), offsets, sizes


sound_blob, damaged_blob = pack(sound), pack(damaged)
out = torch.empty_like(frames)
outs = [out[f] for f in range(F)]
say(f"coded bytes: {sum(len(s) for s in sound)} ({sum(len(s) for s in sound) / F / 1024:.1f} KiB per frame)")

sides = {
    "decode_batch_ragged, intact streams": lambda: batch.decode_batch_ragged(*sound_blob, outs, lib=lib),
    "decode_batch_salvage, intact streams (round 1 only)": lambda: batch.decode_batch_salvage(*sound_blob, outs, 0, lib=lib),
    "decode_batch_salvage, one zeroed interval per frame": lambda: batch.decode_batch_salvage(*damaged_blob, outs, 0, status_pitch=N, lib=lib),
}
results = {}
for name, fn in sides.items():
    ms, results[name] = timed(fn)
    say(f"  warm-up  {name:<56} {ms:9.3f} ms")
times = {name: [] for name in sides}
for turn in range(args.repeats):
    for name, fn in sides.items():
        ms, results[name] = timed(fn)
        times[name].append(ms)
        round_two = getattr(results[name], "gpu_ms", ())[2:3]
        say(f"  round {turn}  {name:<56} {ms:9.3f} ms" + (f"   of which the salvage round {round_two[0]:9.3f} ms" if round_two else ""))
for name, t in times.items():
    say(f"  {name:<56} {'  '.join(f'{x:9.3f}' for x in t)} ms   median {statistics.median(t):9.3f}  spread {max(t) - min(t):7.3f}")

# what the damaged batch came back as (the last call wrote `out`)
got = results["decode_batch_salvage, one zeroed interval per frame"]
states = [r.state for r in got.reports]
lost = [r.intervals_lost for r in got.reports]
say(f"damaged batch: round-1 errors in {int((got.errcs != 0).sum())} of {F} frames; states {sorted(set(states))}; "
    f"intervals lost per frame: min {min(lost)} max {max(lost)}; frames whose lost interval is the damaged one: "
    f"{sum(1 for f in range(F) if got.status[f].tolist() == [2 if j == hit[f] else 0 for j in range(N)])}")
back = out.cpu()
orig = frames.cpu()
wrong = 0
for f in range(F):
    keep = torch.ones(S, dtype=torch.bool)
    for j in range(N):
        if got.status[f, j] != 0:
            keep[j * RI:(j + 1) * RI] = False
    wrong += int((back[f][keep] != orig[f][keep]).sum()) + int((back[f][~keep] != 0).sum())
say(f"wrong samples in kept rows or unfilled samples in lost rows: {wrong}")
say(f"salvage counters (frames, intervals kept, intervals lost, kernel launches): {batch.salvage_counters(lib)}")
