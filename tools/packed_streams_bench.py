"""Packed streams (charls_amd.h part 2d) on the bench's synthetic frames -- by default 512 frames of 2048 x 2048 8-bit gray
(charls_amd/synth.py, seeds 100 + f) -- every figure beside its ruler from the same run:

 (a) the pack kernel: GPU time of charls_amd_pack_streams_device's launch (hipEvents, charls_amd_last_timings [0]) at offset
     alignments 1 and 16, as GB/s of payload, beside ONE hipMemcpyAsync device-to-device of the same total bytes;
 (b) charls_amd_encode_batch_device_packed against the path a caller had before it: charls_amd_encode_batch_device into slots
     followed by one hipMemcpyAsync per frame into a packed buffer (host clock around calls that end in a synchronise);
 (c) charls_amd_decode_batch_device_packed against charls_amd_decode_batch_device on the same streams;
 (d) the HBM held for the streams in both forms.
(b) and (c) alternate the two sides --repeats times (3) after a warm-up of each and print every time, so the run-to-run noise
stands beside the difference.  Run on the GPU box: python tools/packed_streams_bench.py [--frames 512] [--size 2048]"""
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
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("packed_streams_bench.py measures on the GPU: no device found")
lib = capi.load_product()
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
hip.hipMemcpyAsync.restype = C.c_int
D2D = 3  # hipMemcpyDeviceToDevice

N, S = args.frames, args.size
stream = torch.cuda.current_stream().cuda_stream


def d2d(dst_ptr, src_ptr, nbytes):
    rc = hip.hipMemcpyAsync(dst_ptr, src_ptr, nbytes, D2D, C.c_void_p(stream))
    assert rc == 0, rc


def wall(fn):
    torch.cuda.synchronize()
    a = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - a) * 1e3, out


def report(what, times, payload_bytes=None):
    best, med = min(times), statistics.median(times)
    rate = f"  best = {payload_bytes / best / 1e6:8.1f} GB/s" if payload_bytes else ""
    print(f"  {what:<58} {'  '.join(f'{t:9.3f}' for t in times)} ms   median {med:9.3f}  spread {max(times) - min(times):7.3f}{rate}",
          flush=True)
    return best, med


print(f"{N} frames of {S} x {S} 8-bit gray (synth seeds 100 + f)", flush=True)
frames = synth.frames_torch(N, S, S, seed0=100, device="cuda:0")
pitch = (batch.estimated_destination_size(S, S, 8, 1) + 255) & ~255  # (batch.encode_batch's own slot size)
slots = torch.empty((N, pitch), dtype=torch.uint8, device="cuda:0")
enc = batch.encode_batch(frames, streams=slots, lib=lib)
assert (enc.errcs == 0).all()
sizes = enc.sizes
total = int(sizes.sum())
print(f"streams: {total} B in all, {total / N:.0f} B on average, {int(sizes.min())} .. {int(sizes.max())} B; slot pitch {pitch} B", flush=True)

# ---- (a) the pack kernel against one device-to-device copy of the same bytes
print("(a) pack kernel, GPU time of its launch; payload = the streams' bytes, counted once", flush=True)
packed = torch.empty(total + 16 * N + 4096, dtype=torch.uint8, device="cuda:0")
source = torch.empty(total, dtype=torch.uint8, device="cuda:0")
rates = {}
for alignment in (1, 16):
    times = []
    for _ in range(args.repeats + 1):  # (the first is the warm-up)
        got = batch.pack_streams(slots, sizes, alignment=alignment, packed=packed, lib=lib)
        times.append(batch.last_timings(lib)[0])
    rates[alignment] = report(f"pack_streams alignment {alignment}", times[1:], total)[0]
f = N // 2
assert torch.equal(packed[int(got.offsets[f]):int(got.offsets[f]) + int(sizes[f])], slots[f, :int(sizes[f])])
times = []
for _ in range(args.repeats + 1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    d2d(packed.data_ptr(), source.data_ptr(), total)
    b.record()
    b.synchronize()
    times.append(a.elapsed_time(b))
ruler = report("ONE hipMemcpyAsync device to device of the same bytes", times[1:], total)[0]
for alignment in (1, 16):
    print(f"  pack kernel at alignment {alignment}: {100 * ruler / rates[alignment]:.0f}% of the copy's rate", flush=True)

# ---- (b) packed encode against slot encode + one copy per frame
print("(b) encode to the packed form, host clock, calls alternate", flush=True)
offsets1 = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def slots_then_copies():
    e = batch.encode_batch(frames, streams=slots, lib=lib)
    at = 0
    for f in range(N):
        n = int(e.sizes[f])
        if n:
            d2d(packed.data_ptr() + at, slots.data_ptr() + f * pitch, n)
        at += n
    return e


def packed_call():
    return batch.encode_batch_packed(frames, packed, alignment=1, lib=lib)


slots_then_copies()
before = batch.work_area_bytes(lib)
got = packed_call()
staging = batch.work_area_bytes(lib) - before
assert (got.errcs == 0).all() and (got.sizes == sizes).all() and (got.offsets == offsets1).all()
old, new = [], []
for _ in range(args.repeats):
    old.append(wall(slots_then_copies)[0])
    new.append(wall(packed_call)[0])
old_best, _ = report("encode_batch_device + hipMemcpyAsync per frame", old)
new_best, _ = report("encode_batch_device_packed", new)
print(f"  packed / slots + copies, best of each: {new_best / old_best:.3f}", flush=True)
for f in (0, N // 2, N - 1):
    assert torch.equal(packed[int(got.offsets[f]):int(got.offsets[f]) + int(sizes[f])], slots[f, :int(sizes[f])])

# ---- (c) packed decode against slot decode
print("(c) decode, host clock, calls alternate", flush=True)
out = torch.empty_like(frames)
batch.decode_batch(slots, sizes, out, lib=lib)
batch.decode_batch_packed(packed, got.offsets, sizes, out, lib=lib)
old, new = [], []
for _ in range(args.repeats):
    out.zero_()
    t, (_, errcs, _) = wall(lambda: batch.decode_batch(slots, sizes, out, lib=lib))
    assert (errcs == 0).all() and torch.equal(out, frames)
    old.append(t)
    out.zero_()
    t, (_, errcs, _) = wall(lambda: batch.decode_batch_packed(packed, got.offsets, sizes, out, lib=lib))
    assert (errcs == 0).all() and torch.equal(out, frames)
    new.append(t)
old_best, _ = report("decode_batch_device (slots)", old)
new_best, _ = report("decode_batch_device_packed", new)
print(f"  packed / slots, best of each: {new_best / old_best:.3f}", flush=True)

# ---- (d) HBM held for the streams
print("(d) HBM held for the streams", flush=True)
print(f"  slots:  {N} x {pitch} B = {N * pitch / 1e9:.3f} GB", flush=True)
print(f"  packed: {total / 1e9:.3f} GB ({100 * total / (N * pitch):.0f}% of the slots); while encoding, staging slots of "
      f"{staging / 1e9:.3f} GB are held as a work area (released by charls_amd_release_work_areas)", flush=True)
