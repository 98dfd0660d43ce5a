"""What the salvage round through the seek-point index (charls_amd.h part 2h) costs, beside the indexed decode of the same
frames undamaged (charls_amd_decode_batch_device_indexed: the same kernel on the same number of intervals), by device events
around calls that end in a synchronise: by default 256 frames of 1024 x 1024 8-bit gray (charls_amd/synth.py, seeds 100 + f)
without restart markers, their indexes built with K = 32 while they are sound; in the damaged copy four bytes in the middle
of one interval of every frame are zeroed (interval f mod N of frame f, placed by the reader positions the index holds).  A
warm-up of each side, then --repeats rounds (3); every time is printed, and the ratio with the spread of the repeats.

  --side indexed   only the indexed decode of the undamaged frames; with --lib PATH on another build of the library (the
                   parent commit's, which has no part 2h), so that both builds are measured in one session
  --side salvage   only the salvage call on the damaged frames (round 1, which fails every frame, and round 2)
  --side both      (default)
Run on the GPU box: python tools/salvage_index_bench.py [--frames 256] [--size 1024] [--lines 32] [--out FILE] [--append]"""
import argparse
import os
import statistics
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from charls_amd import batch, capi, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--lines", type=int, default=32)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--side", choices=["both", "indexed", "salvage"], default="both")
ap.add_argument("--lib", default=None, help="another build of libcharls_amd.so (indexed side only)")
ap.add_argument("--append", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_salvage_indexed.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("salvage_index_bench.py measures on the GPU: no device found")
if args.lib and args.side != "indexed":
    sys.exit("--lib serves --side indexed")
if args.lib:
    capi.PRODUCT_LIB = os.path.abspath(args.lib)
lib = capi.load_product()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
log = open(args.out, "a" if args.append else "w")


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


F, S, K = args.frames, args.size, args.lines
N = -(-S // K)
say(f"--- {' '.join(sys.argv)}")
say(f"{torch.cuda.get_device_name(0)}; library {args.lib or 'of this tree'}; {F} frames of {S} x {S} 8-bit gray (synth seeds 100 + f), "
    f"no restart markers, K = {K} ({N} intervals per frame)")
frames = synth.frames_torch(F, S, S, seed0=100, device="cuda:0")
enc = batch.encode_batch(frames, lib=lib)
assert (enc.errcs == 0).all()
out = torch.empty_like(frames)
_, errcs, indexes = batch.decode_batch_and_index(enc.streams, enc.sizes, out, K, lib=lib)
assert (errcs == 0).all() and bool((out == frames).all())
host = enc.streams.cpu().numpy()
sound = [host[f, :int(enc.sizes[f])].tobytes() for f in range(F)]
say(f"coded bytes: {sum(len(s) for s in sound)} ({sum(len(s) for s in sound) / F / 1024:.1f} KiB per frame); "
    f"index bytes per frame: {len(indexes[0])}")


def positions(index):
    """Reader positions of the seek points of scan 0 (host/seek_index.h, device/seek_decode.h)."""
    point = struct.unpack_from("<I", index, 64)[0]
    length, _, points, _ = struct.unpack_from("<QQII", index, 72)
    return [0] + [struct.unpack_from("<Q", index, 72 + 24 + (i + 1) * point - 24)[0] for i in range(points)] + [length]


damaged, hit = [], []
for f, jls in enumerate(sound):
    sos = jls.rfind(b"\xff\xda")
    start = sos + 2 + int.from_bytes(jls[sos + 2:sos + 4], "big")
    pos = positions(indexes[f])
    assert len(pos) == N + 1
    j = f % N
    at = start + (pos[j] + pos[j + 1]) // 2 - 2
    assert start + pos[j] + 16 <= at and at + 4 <= start + pos[j + 1] - 16
    data = bytearray(jls)
    data[at:at + 4] = bytes(4)
    damaged.append(bytes(data))
    hit.append(j)


def pack(streams):
    sizes = np.array([len(s) for s in streams], dtype=np.uint64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    blob = np.frombuffer(b"".join(streams) + bytes(16), dtype=np.uint8).copy()
    return torch.from_numpy(blob).cuda(), offsets, sizes


outs = [out[f] for f in range(F)]
sides = {}
if args.side in ("both", "indexed"):
    sides["decode_batch_indexed, undamaged"] = lambda: (batch.decode_batch_indexed(enc.streams, enc.sizes, indexes, out, lib=lib),
                                                          batch.last_timings(lib))
if args.side in ("both", "salvage"):
    damaged_blob = pack(damaged)
    sides["decode_batch_salvage_indexed, one zeroed interval per frame"] = \
        lambda: batch.decode_batch_salvage_indexed(*damaged_blob, outs, indexes, 0, status_pitch=N, lib=lib)


def detail(name, result):
    if name.startswith("decode_batch_indexed"):
        (_, errcs), t = result
        assert (errcs == 0).all()
        return f"   seek launches {t[0]:9.3f} ms, hash launches {t[1]:9.3f} ms", t[0]
    t = result.gpu_ms
    return f"   round 2 {t[2]:9.3f} ms by the host's clock, its launches {t[3]:9.3f} ms by device events", t[2]


results, times, inner = {}, {name: [] for name in sides}, {name: [] for name in sides}
for name, fn in sides.items():
    ms, results[name] = timed(fn)
    say(f"  warm-up  {name:<62} {ms:11.3f} ms" + detail(name, results[name])[0])
for turn in range(args.repeats):
    for name, fn in sides.items():
        ms, results[name] = timed(fn)
        text, part = detail(name, results[name])
        times[name].append(ms)
        inner[name].append(part)
        say(f"  round {turn}  {name:<62} {ms:11.3f} ms" + text)
for name in sides:
    for what, t in (("whole call", times[name]), ("seek launches" if name.startswith("decode_batch_indexed") else "round 2", inner[name])):
        say(f"  {name:<62} {what:<14} {'  '.join(f'{x:11.3f}' for x in t)} ms   median {statistics.median(t):11.3f}  "
            f"spread {max(t) - min(t):9.3f}")
if len(sides) == 2:
    a, b = (inner[name] for name in sides)
    ratios = [y / x for x, y in zip(a, b)]
    say(f"round 2 over the whole indexed call's seek launches, repeat by repeat: {'  '.join(f'{r:7.3f}' for r in ratios)}   "
        f"median {statistics.median(ratios):7.3f}  spread {max(ratios) - min(ratios):7.3f}")
    whole = [y / x for x, y in zip(times[list(sides)[0]], b)]
    say(f"round 2 over the whole indexed call: {'  '.join(f'{r:7.3f}' for r in whole)}   median {statistics.median(whole):7.3f}  "
        f"spread {max(whole) - min(whole):7.3f}")

if args.side in ("both", "salvage"):
    got = results["decode_batch_salvage_indexed, one zeroed interval per frame"]
    states = [r.state for r in got.reports]
    status = got.status[:, :N]
    want = np.array([[2 if j == hit[f] else (0 if j < hit[f] else 4) for j in range(N)] for f in range(F)], dtype=np.uint8)
    say(f"damaged batch: round-1 errors in {int((got.errcs != 0).sum())} of {F} frames; states {sorted(set(states))}; intervals kept "
        f"proven (0) {int((status == 0).sum())}, kept on the index (4) {int((status == 4).sum())}, lost (2) {int((status == 2).sum())}, "
        f"not reached (3) {int((status == 3).sum())}; frames whose status bytes are 0 above, 2 at and 4 below the damaged interval: "
        f"{int((status == want).all(axis=1).sum())}")
    back, orig = out.cpu(), frames.cpu()
    wrong = unfilled = 0
    for f in range(F):
        keep = torch.ones(S, dtype=torch.bool)
        for j in range(N):
            if status[f, j] not in (0, 4):
                keep[j * K:(j + 1) * K] = False
        wrong += int((back[f][keep] != orig[f][keep]).sum())
        unfilled += int((back[f][~keep] != 0).sum())
    say(f"samples in kept rows that differ from the sound frame: {wrong}; samples in lost rows that are not the fill: {unfilled}")
    say(f"salvage index counters (frames by index, kept proven, kept on the index, lost, frames by prefix, launches): "
        f"{batch.salvage_index_counters(lib)}")
