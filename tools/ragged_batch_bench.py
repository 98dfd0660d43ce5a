"""Ragged frames (charls_amd.h part 2e) beside their rulers, every figure from the same run (host clock around calls that end
in a synchronise; the two sides alternate --repeats times (3) after a warm-up of each and every time is printed, so the
run-to-run spread stands beside the difference):

 (a) a UNIFORM batch -- by default 512 frames of 2048 x 2048 8-bit gray (charls_amd/synth.py, seeds 100 + f), the shape of
     tools/packed_streams_bench.py -- through charls_amd_encode_batch_device_ragged against charls_amd_encode_batch_device_packed
     of the same build: the same launches, so what the ragged call adds is host table work.  The C call on tables made
     beforehand and the Python binding (which makes them) are timed apart;
 (b) a MIXED batch -- four geometries, --mixed frames (128) of each, interleaved, every frame a tensor of its own -- through one
     ragged call against what a caller does without it: per geometry, the frames copied into a pitched tensor (torch.stack) and
     one charls_amd_encode_batch_device_packed (which leaves the streams grouped by geometry, not in the caller's order);
 (c) charls_amd_probe_batch_device_packed over --probe (4096) small streams;
 (d) charls_amd_decode_batch_device_ragged against charls_amd_decode_batch_device_packed on (a)'s streams.
Run on the GPU box: python tools/ragged_batch_bench.py [--frames 512] [--size 2048] [--out profiles/r11_ragged_batch.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from charls_amd import batch, capi, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=512)
ap.add_argument("--size", type=int, default=2048)
ap.add_argument("--mixed", type=int, default=128)
ap.add_argument("--probe", type=int, default=4096)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_ragged_batch.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("ragged_batch_bench.py measures on the GPU: no device found")
lib = capi.load_product()
l = batch._bind(lib)
u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
log = open(args.out, "w")


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


def report(what, times):
    best, med = min(times), statistics.median(times)
    say(f"  {what:<66} {'  '.join(f'{t:9.3f}' for t in times)} ms   median {med:9.3f}  spread {max(times) - min(times):7.3f}")
    return best, max(times) - min(times)


def alternate(sides):
    """{name: fn}: a warm-up of each, then --repeats rounds in which the sides take turns.  Returns {name: (best, spread)}."""
    for fn in sides.values():
        fn()
    times = {name: [] for name in sides}
    for _ in range(args.repeats):
        for name, fn in sides.items():
            times[name].append(wall(fn)[0])
    return {name: report(name, t) for name, t in times.items()}


N, S = args.frames, args.size
say(f"{torch.cuda.get_device_name(0)}; {N} frames of {S} x {S} 8-bit gray (synth seeds 100 + f)")
frames = synth.frames_torch(N, S, S, seed0=100, device="cuda:0")
slot = batch.estimated_destination_size(S, S, 8, 1)
packed = torch.empty(N * slot, dtype=torch.uint8, device="cuda:0")
packed2 = torch.empty_like(packed)

# ---- (a) a uniform batch: ragged against packed
say("(a) uniform batch, encode: charls_amd_encode_batch_device_ragged against charls_amd_encode_batch_device_packed")
views = [frames[f] for f in range(N)]
p = batch.codec_params(S, S)
sources = (batch.FrameSource * N)(*[batch.FrameSource(p, frames.data_ptr() + f * S * S, 0, 0, 0) for f in range(N)])
offsets, sizes, errcs = np.zeros(N + 1, dtype=np.uint64), np.zeros(N, dtype=np.uint64), np.zeros(N, dtype=np.int32)


def ragged_c():
    rc = l.charls_amd_encode_batch_device_ragged(N, sources, packed2.data_ptr(), packed2.numel(), 1, offsets.ctypes.data_as(u64p),
                                                 sizes.ctypes.data_as(u64p), errcs.ctypes.data_as(i32p), None)
    assert rc == 0 and not errcs.any()


want = batch.encode_batch_packed(frames, packed, lib=lib)
assert (want.errcs == 0).all()
total = int(want.offsets[-1])
ragged_c()
assert (offsets == want.offsets).all() and (sizes == want.sizes).all() and torch.equal(packed2[:total], packed[:total])
got = alternate({
    "encode_batch_device_packed (the ruler: the parent's code)": lambda: batch.encode_batch_packed(frames, packed, lib=lib),
    "encode_batch_device_ragged, C call on prepared tables": ragged_c,
    "encode_batch_ragged, the Python binding (makes the tables)": lambda: batch.encode_batch_ragged(views, p, packed2, lib=lib),
})
ruler, c_call, binding = (got[k] for k in got)
say(f"  ragged (C call) / packed, best of each: {c_call[0] / ruler[0]:.4f}; difference of the bests {c_call[0] - ruler[0]:+.3f} ms, "
    f"the ruler's own spread {ruler[1]:.3f} ms, the ragged call's {c_call[1]:.3f} ms")
say(f"  the binding's table making: {binding[0] - c_call[0]:+.3f} ms over the C call")

# ---- (d) ragged decode against packed decode on the same streams
say("(d) uniform batch, decode: charls_amd_decode_batch_device_ragged against charls_amd_decode_batch_device_packed")
out = torch.empty_like(frames)
outs = [out[f] for f in range(N)]


def decode_packed():
    _, e, _ = batch.decode_batch_packed(packed, want.offsets, want.sizes, out, lib=lib)
    assert not e.any()


def decode_ragged():
    _, e, _ = batch.decode_batch_ragged(packed, want.offsets, want.sizes, outs, lib=lib)
    assert not e.any()


out.zero_()
decode_ragged()
assert torch.equal(out, frames)
got = alternate({"decode_batch_device_packed": decode_packed, "decode_batch_device_ragged (Python binding, a table entry per frame)": decode_ragged})
a, b = (got[k] for k in got)
say(f"  ragged / packed, best of each: {b[0] / a[0]:.4f}")
del out, outs, views, frames, packed2
torch.cuda.empty_cache()

# ---- (b) a mixed batch
M = args.mixed
shapes = [(S, S), (S // 2, S // 2), (3 * S // 4, S // 2), (S // 4, S // 4)]  # (width, height)
say(f"(b) mixed batch, encode: {M} frames each of " + ", ".join(f"{w} x {h}" for w, h in shapes) + ", interleaved, a tensor each")
pools = [synth.frames_torch(M, w, h, seed0=100 + 1000 * k, device="cuda:0") for k, (w, h) in enumerate(shapes)]
mixed = [pools[k][f].clone() for f in range(M) for k in range(len(shapes))]  # A0 B0 C0 D0 A1 ...
params = [batch.codec_params(*shapes[k]) for _ in range(M) for k in range(len(shapes))]
del pools
room = sum(batch.estimated_destination_size(w, h, 8, 1) for w, h in shapes) * M
packed_m = torch.empty(room, dtype=torch.uint8, device="cuda:0")
regions = [torch.empty(batch.estimated_destination_size(w, h, 8, 1) * M, dtype=torch.uint8, device="cuda:0") for w, h in shapes]


def one_ragged_call():
    r = batch.encode_batch_ragged(mixed, params, packed_m, lib=lib)
    assert not r.errcs.any()
    return r


def regroup_and_call_per_geometry():
    done = []
    for k in range(len(shapes)):
        r = batch.encode_batch_packed(torch.stack(mixed[k::len(shapes)]), regions[k], lib=lib)
        assert not r.errcs.any()
        done.append(r)
    return done


r, per = one_ragged_call(), regroup_and_call_per_geometry()
for k in range(len(shapes)):  # the same streams, frame by frame
    assert (r.sizes[k::len(shapes)] == per[k].sizes).all()
f = 4 * (M // 2) + 1
assert torch.equal(packed_m[int(r.offsets[f]):int(r.offsets[f]) + int(r.sizes[f])],
                   regions[1][int(per[1].offsets[M // 2]):int(per[1].offsets[M // 2]) + int(per[1].sizes[M // 2])])
got = alternate({"torch.stack + encode_batch_device_packed per geometry (4 calls)": regroup_and_call_per_geometry,
                 "ONE encode_batch_device_ragged (Python binding)": one_ragged_call})
a, b = (got[k] for k in got)
say(f"  ragged / regrouped, best of each: {b[0] / a[0]:.4f}")
del mixed, regions, packed_m
torch.cuda.empty_cache()

# ---- (c) the probe
P = args.probe
say(f"(c) probe: charls_amd_probe_batch_device_packed over {P} streams of 64 x 64 8-bit gray")
small = synth.frames_torch(P, 64, 64, seed0=7, device="cuda:0")
blob = torch.empty(P * batch.estimated_destination_size(64, 64, 8, 1), dtype=torch.uint8, device="cuda:0")
enc = batch.encode_batch_packed(small, blob, lib=lib)
assert not enc.errcs.any()


def probe():
    _, nbytes, e = batch.probe_packed(blob, enc.offsets, enc.sizes, lib=lib)
    assert not e.any() and (nbytes == 64 * 64).all()


probe()
best, _ = report("probe_batch_device_packed", [wall(probe)[0] for _ in range(args.repeats)])
say(f"  {best * 1e3 / P:.2f} us per stream")
log.close()
