"""The seek-point index on ONE 4096 x 4096 8-bit frame through the host-pointer C ABI (PCIe inclusive), best and median of N
calls: plain decode, decode + index build, decode through an index for K = 32, 64, 128, a 64-row band from the middle
with and without an index, and the index's size as a share of the stream.  Streams: the tulips image tiled, and the
synthetic frame of tools/one_frame_latency.py.  Run on the GPU box: python tools/seek_index_latency.py [--calls 5]

--batch: the same index through the device-memory batch API (charls_amd.h part 2c), every figure beside the part-1 or
plain-batch figure of the same run: building N indexes in one call against N x one part-1 build, decoding N frames through
K = 64 indexes against charls_amd_decode_batch_device, 64-row bands at K = 16 from N frames, and the GPU time of the
segment-hash launches (charls_amd_last_timings [1]).  The N slots hold N copies of one stream: frames are independent, so
the times are those of N different streams of that size.  --frames / --build-frames choose the N.

--batch --packed: the calls of part 2l on a packed blob (N copies of one stream back to back, alignment 1) beside the slot
calls of part 2c on the same streams, the two sides alternating, --calls repeats after one warm-up each: (a) the index-only
build against charls_amd_decode_batch_device_and_index -- of the library at --parent-lib where one is given (a build of the
commit before part 2l), else of this build --, with the frame memory the index-only build does not allocate; (b) the ragged
indexed decode and the ragged bands against their slot calls.  --packed-frames is the N (256), K = 64 (bands: K = 16)."""
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
ap.add_argument("--batch", action="store_true")
ap.add_argument("--frames", type=int, nargs="*", default=[1, 4, 16, 64, 256, 1024])
ap.add_argument("--build-frames", type=int, nargs="*", default=[1, 16, 256, 1024])
ap.add_argument("--band-frames", type=int, nargs="*", default=[1, 64, 1024])
ap.add_argument("--images", nargs="*", default=["tulips_tiled", "synthetic"])
ap.add_argument("--packed", action="store_true")
ap.add_argument("--packed-frames", type=int, default=256)
ap.add_argument("--parent-lib", default=None)
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
frames = {name: img for name, img in frames.items() if name in args.images}


def batch_mode():
    import numpy as np
    import torch
    from charls_amd import batch

    def gpu_clock(fn, calls):
        times, hashes, out = [], [], None
        for _ in range(calls):
            torch.cuda.synchronize()
            a = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - a)
            hashes.append(batch.last_timings(lib)[1])
        return min(times), statistics.median(times), min(hashes), out

    most = max(args.frames + args.build_frames + args.band_frames)
    mpix = n * n / 1e6
    for name, img in frames.items():
        jls = lib.encode(img, width=n, height=n, bits_per_sample=8)
        pitch = (len(jls) + 255) & ~255
        print(f"{name} {n} x {n} 8-bit: {len(jls)} B, slots of {pitch} B", flush=True)
        one = torch.zeros(pitch, dtype=torch.uint8)
        one[:len(jls)] = torch.frombuffer(bytearray(jls), dtype=torch.uint8)
        d_streams = one.cuda().repeat(most, 1).contiguous()
        sizes = np.full(most, len(jls), dtype=np.uint64)
        out = torch.empty((most, n * n), dtype=torch.uint8, device="cuda")
        want = torch.from_numpy(img.reshape(-1)).cuda()
        # ---- build
        a = time.perf_counter()
        _, px, part1 = lib.decode_with_index(jls, 64)
        part1_build = time.perf_counter() - a
        assert px.tobytes() == img.tobytes()
        print(f"  part-1 decode + index build (K=64): {part1_build:.3f} s = {mpix / part1_build:.2f} MPix/s", flush=True)
        bound = batch.index_size_bound(n, n, lines_per_seek_point=64, lib=lib)
        for N in args.build_frames:
            best, _, hash_ms, (_, errcs, built) = gpu_clock(
                lambda: batch.decode_batch_and_index(d_streams[:N], sizes[:N], out[:N], 64, index_pitch=bound, lib=lib), 1)
            assert (errcs == 0).all() and built[0] == part1 and built[-1] == part1 and torch.equal(out[N - 1], want)
            print(f"  build N={N:<5} one call {best:8.3f} s = {N * mpix / best:9.1f} MPix/s   N x part 1 = {N * part1_build:9.1f} s"
                  f"   hash launches {hash_ms:.2f} ms", flush=True)
        # ---- indexed decode against the plain batch decoder
        index16 = lib.decode_with_index(jls, 16)[2]
        for N in args.frames:
            out[:N].zero_()
            best, med, hash_ms, (_, errcs) = gpu_clock(lambda: batch.decode_batch_indexed(d_streams[:N], sizes[:N], [part1] * N, out[:N], lib=lib),
                                                       args.calls)
            assert (errcs == 0).all() and torch.equal(out[N - 1], want)
            out[:N].zero_()
            pbest, pmed, _, (_, errcs, _) = gpu_clock(lambda: batch.decode_batch(d_streams[:N], sizes[:N], out[:N], lib=lib), args.calls)
            assert (errcs == 0).all() and torch.equal(out[N - 1], want)
            print(f"  decode N={N:<5} indexed K=64 best {best * 1e3:9.1f} ms median {med * 1e3:9.1f} ms = {N * mpix / best:9.1f} MPix/s"
                  f" (hash launch {hash_ms:.2f} ms)   plain batch best {pbest * 1e3:9.1f} ms median {pmed * 1e3:9.1f} ms = {N * mpix / pbest:9.1f} MPix/s",
                  flush=True)
        # ---- 64-row bands
        first = n // 2 - 32
        band_want = want[first * n:(first + 64) * n]
        bands = torch.empty((max(args.band_frames), 64 * n), dtype=torch.uint8, device="cuda")
        b1, m1, band = clock(lambda: lib.decode_rows(jls, first, 64, index=index16), args.calls)
        print(f"  part-1 64-row band, index K=16: best {b1:.1f} ms median {m1:.1f} ms", flush=True)
        for N in args.band_frames:
            bands[:N].zero_()
            best, med, hash_ms, errcs = gpu_clock(lambda: batch.decode_rows_batch(d_streams[:N], sizes[:N], [index16] * N, [first] * N, [64] * N,
                                                                                bands[:N], lib=lib), args.calls)
            assert (errcs == 0).all() and torch.equal(bands[N - 1], band_want)
            print(f"  bands N={N:<5} K=16 best {best * 1e3:9.1f} ms median {med * 1e3:9.1f} ms, of which the hash launch {hash_ms:.2f} ms"
                  f" = {100 * hash_ms / (best * 1e3):.0f}%   N x part 1 = {N * b1:9.1f} ms", flush=True)


def packed_mode():
    import numpy as np
    import torch
    from charls_amd import batch

    N, K, repeats = args.packed_frames, 64, args.calls
    parent = capi.CharLSLibrary(args.parent_lib) if args.parent_lib else lib
    mpix = N * n * n / 1e6

    def alternate(sides):
        """[(name, fn)] -> {name: [seconds per repeat]}: one warm-up each, then the sides in turn, repeat by repeat."""
        for _, fn in sides:
            fn()
        times = {name: [] for name, _ in sides}
        for _ in range(repeats):
            for name, fn in sides:
                torch.cuda.synchronize()
                a = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - a)
        return times

    def report(what, times):
        for name, ts in times.items():
            print(f"  {what:<16} {name:<34} " + " ".join(f"{t * 1e3:9.1f}" for t in ts) +
                  f" ms   median {statistics.median(ts) * 1e3:9.1f} ms = {mpix / statistics.median(ts):8.1f} MPix/s"
                  f"   spread {(max(ts) - min(ts)) / statistics.median(ts) * 100:4.1f}%", flush=True)

    for name, img in frames.items():
        jls = lib.encode(img, width=n, height=n, bits_per_sample=8)
        pitch = (len(jls) + 255) & ~255
        print(f"{name} {n} x {n} 8-bit, N = {N}, K = {K}: {len(jls)} B per stream; slots of {pitch} B, blob of {N * len(jls)} B", flush=True)
        one = torch.zeros(pitch, dtype=torch.uint8)
        one[:len(jls)] = torch.frombuffer(bytearray(jls), dtype=torch.uint8)
        d_streams = one.cuda().repeat(N, 1).contiguous()
        blob = torch.cat([one[:len(jls)].repeat(N), torch.zeros(16, dtype=torch.uint8)]).cuda()
        sizes = np.full(N, len(jls), dtype=np.uint64)
        offsets = np.arange(N, dtype=np.uint64) * len(jls)
        want = torch.from_numpy(img.reshape(-1)).cuda()
        part1 = lib.decode_with_index(jls, K)[2]
        bound = batch.index_size_bound(n, n, lines_per_seek_point=K, lib=lib)
        # ---- (a) the index-only build against the slot build with frames
        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info()[0]
        out = torch.empty((N, n * n), dtype=torch.uint8, device="cuda")
        got = {}

        def slot_build():
            got["slot"] = batch.decode_batch_and_index(d_streams, sizes, out, K, index_pitch=bound, lib=parent)

        def index_only():
            got["only"] = batch.index_batch_packed(blob, offsets, sizes, K, index_pitch=bound, lib=lib)

        slot_name = "slot build + frames" + (" (parent)" if args.parent_lib else " (this build)")
        times = alternate([(slot_name, slot_build), ("index-only, packed", index_only)])
        report("(a) build", times)
        for key in ("slot", "only"):
            _, errcs, built = got[key]
            assert (errcs == 0).all() and built[0] == part1 and built[-1] == part1, key
        assert torch.equal(out[N - 1], want)
        print(f"  (a) frame memory the index-only build does not take: {N * n * n / 2**20:.0f} MiB "
              f"(free device memory fell by {(free_before - torch.cuda.mem_get_info()[0]) / 2**20:.0f} MiB when the slot side's frames were allocated); "
              f"work areas held now: {batch.work_area_bytes(lib) / 2**20:.0f} MiB", flush=True)
        # ---- (b) the ragged indexed decode and the ragged bands against their slot calls
        outs = [out[f] for f in range(N)]
        indexes = [part1] * N

        def slot_indexed():
            got["e"] = batch.decode_batch_indexed(d_streams, sizes, indexes, out, lib=lib)[1]

        def ragged_indexed():
            got["e"] = batch.decode_batch_ragged_indexed(blob, offsets, sizes, indexes, outs, lib=lib)[1]

        for side in (slot_indexed, ragged_indexed):
            out.zero_()
            side()
            assert (got["e"] == 0).all() and torch.equal(out[N - 1], want) and torch.equal(out[0], want)
        report("(b) decode", alternate([("indexed, slots", slot_indexed), ("indexed, packed + ragged", ragged_indexed)]))
        index16 = [lib.decode_with_index(jls, 16)[2]] * N
        first = n // 2 - 32
        band_want = want[first * n:(first + 64) * n]
        bands = torch.empty((N, 64 * n), dtype=torch.uint8, device="cuda")
        band_list = [bands[f] for f in range(N)]

        def slot_bands():
            got["e"] = batch.decode_rows_batch(d_streams, sizes, index16, [first] * N, [64] * N, bands, lib=lib)

        def ragged_bands():
            got["e"] = batch.decode_rows_batch_ragged(blob, offsets, sizes, index16, [first] * N, [64] * N, band_list, lib=lib)

        for side in (slot_bands, ragged_bands):
            bands.zero_()
            side()
            assert (got["e"] == 0).all() and torch.equal(bands[N - 1], band_want) and torch.equal(bands[0], band_want)
        report("(b) 64-row bands", alternate([("bands K=16, slots", slot_bands), ("bands K=16, packed + ragged", ragged_bands)]))
        del out, bands


if args.batch and args.packed:
    packed_mode()
    sys.exit(0)
if args.batch:
    batch_mode()
    sys.exit(0)
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
