"""The seek-point index on ONE 4096 x 4096 8-bit frame through the host-pointer C ABI (PCIe inclusive), best and median of N
calls: plain decode, decode + index build, decode through an index for K = 32, 64, 128, a 64-row band from the middle
with and without an index, and the index's size as a share of the stream.  Streams: the tulips image tiled, and the
synthetic frame of tools/one_frame_latency.py.  Run on the GPU box: python tools/seek_index_latency.py [--calls 5]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from charls_amd import capi, synth  # noqa: E402
import common  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--size", type=int, default=4096)
args = ap.parse_args()
lib = capi.load_product()


def clock(fn, calls):
    times, out = [], None
    for _ in range(calls):
        a = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - a)
    return min(times) * 1e3, statistics.median(times) * 1e3, out


def line(what, best, median, extra=""):
    print(f"  {what:<34} best {best:9.1f} ms  median {median:9.1f} ms{extra}", flush=True)


n = args.size
frames = {"tulips_tiled": common.tulips_tiled(n, n, 0), "synthetic": synth.frame_numpy(n, n, seed=2, bits=8)}
for name, img in frames.items():
    jls = lib.encode(img, width=n, height=n, bits_per_sample=8)
    print(f"{name} {n} x {n} 8-bit: {len(jls)} B", flush=True)
    lib.decode(jls)  # (warm)
    best, med, (_, px) = clock(lambda: lib.decode(jls), args.calls)
    assert px.tobytes() == img.tobytes()
    line("plain decode", best, med)
    best, med, (_, px, index64) = clock(lambda: lib.decode_with_index(jls, 64), 1)
    assert px.tobytes() == img.tobytes()
    line("decode + index build (K=64)", best, med)
    indexes = {64: index64}
    for K in (32, 128, 16):
        indexes[K] = lib.decode_with_index(jls, K)[2]
    for K in (32, 64, 128):
        best, med, (_, px) = clock(lambda: lib.decode(jls, index=indexes[K]), args.calls)
        assert px.tobytes() == img.tobytes()
        line(f"indexed decode K={K}", best, med, f"  index {len(indexes[K])} B = {100 * len(indexes[K]) / len(jls):.1f}% of the stream")
    first = n // 2 - 32
    want = img[first:first + 64].tobytes()
    for K in (16, 64):
        best, med, band = clock(lambda: lib.decode_rows(jls, first, 64, index=indexes[K]), args.calls)
        assert band.tobytes() == want
        line(f"64-row band, index K={K}", best, med, f"  index {100 * len(indexes[K]) / len(jls):.1f}% of the stream")
    best, med, band = clock(lambda: lib.decode_rows(jls, first, 64), 1)
    assert band.tobytes() == want
    line("64-row band, no index", best, med)
