#!/usr/bin/env python3
"""Measures row bands through restart markers (charls_amd.h part 2m) on the GPU.

The blob is 256 frames of 2048 x 2048 8-bit gray, coded by this library's ragged encoder with a restart interval of 64 lines
and of 8 lines.  Two bands of 64 rows of every frame: at row 1000 (at 64 lines per interval: two edge intervals per frame) and
at row 1024 (none).

  (a) charls_amd_decode_rows_batch_device_ragged_markers against charls_amd_decode_rows_batch_device_ragged on the same blob,
      the four inputs one after the other, the sides alternating, a warm-up and --repeats (at least 3) timed calls each: device
      events around the call and the host clock.  The bands of the two calls are compared byte for byte first.
  (b) --walk-only: nothing but whole-frame decodes of --walk-frames of those streams (charls_amd_decode_batch_device_ragged), so
      that a run of this mode under `rocprofv3 --kernel-trace --stats`, in a run of its own, gives the time of the
      find_restart_markers launches: once with --lib pointing at a build of the parent commit, once at the new build.  The same
      library codes the streams it decodes; the streams of the two builds are the same bytes.

    python tools/band_markers_probe.py [--frames 256] [--repeats 3] [--out FILE]
    rocprofv3 --kernel-trace --stats ... -- python tools/band_markers_probe.py --walk-only [--lib PATH]

The table of (a) goes to FILE, by default profiles/r25_band_markers.txt.  Needs the GPU: without one it fails."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INTERVALS = (64, 8)
BANDS = ((1000, 64), (1024, 64))  # (at 64 lines per interval: two edge intervals per frame, and none)


def coded_blob(torch, batch, synth, lib, n, width, height, interval, dev):
    """(blob, offsets, sizes, frames): n `mixed` frames coded with the restart interval, packed at alignment 1."""
    frames = synth.frames_torch(n, width, height, seed0=100, bits=8, kind="mixed", device=dev)
    packed = torch.zeros(n * (width * height + width * height // 8 + 4096), dtype=torch.uint8, device=dev)
    p = batch.codec_params(width, height, 8, 1, 0, 0, restart_interval=interval)
    got = batch.encode_batch_ragged([frames[f] for f in range(n)], p, packed, lib=lib)
    torch.cuda.synchronize()
    assert (got.errcs == 0).all(), got.errcs
    return packed, got.offsets[:n].copy(), got.sizes.copy(), frames


def walk_only(args):
    import torch
    from charls_amd import batch, capi, synth
    assert torch.cuda.is_available(), "this tool measures on the GPU and does not fall back"
    lib = capi.CharLSLibrary(args.lib) if args.lib else capi.load_product()
    dev = torch.device("cuda:0")
    n, width, height = args.walk_frames, args.width, args.height
    for interval in INTERVALS:
        blob, offsets, sizes, frames = coded_blob(torch, batch, synth, lib, n, width, height, interval, dev)
        outs = [torch.empty((height, width), dtype=torch.uint8, device=dev) for _ in range(n)]
        for _ in range(1 + args.repeats):
            _, errcs, _ = batch.decode_batch_ragged(blob, offsets, sizes, outs, lib=lib)
            torch.cuda.synchronize()
            assert (errcs == 0).all(), errcs
        assert all(torch.equal(outs[f], frames[f]) for f in range(n))
        print(f"walk-only: {1 + args.repeats} decodes of {n} frames {width} x {height}, restart interval {interval}: "
              f"{int(sizes.sum())} bytes of streams per decode, {n} scans per find_restart_markers launch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--width", type=int, default=2048)  # (a rehearsal at a toy size; the rows to quote are 2048 x 2048)
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--walk-only", action="store_true")
    ap.add_argument("--walk-frames", type=int, default=16)
    ap.add_argument("--lib", default=None, help="the library to load (--walk-only): a build of another commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_band_markers.txt"))
    args = ap.parse_args()
    assert args.repeats >= 3, "at least three repeats: a difference means nothing without the spread"
    if args.walk_only:
        return walk_only(args)

    import torch
    from charls_amd import batch, capi, synth
    assert torch.cuda.is_available(), "this tool measures on the GPU and does not fall back"
    lib = capi.load_product()
    dev = torch.device("cuda:0")
    n, width, height = args.frames, args.width, args.height
    calls = (("markers", batch.decode_rows_batch_ragged_markers), ("existing", batch.decode_rows_batch_ragged))
    lines = [f"row bands through restart markers: {n} frames {width} x {height} 8-bit gray, bands of 64 rows of every frame",
             f"{torch.cuda.get_device_name(0)}; warm-up, then {args.repeats} timed calls a side, the sides alternating; ms, median (min .. max)",
             "",
             f"{'Ri':>3} {'band':>14} {'side':>9} {'device events':>28} {'host clock':>28}   route counters of one call"]
    slower = []
    for interval in INTERVALS:
        blob, offsets, sizes, frames = coded_blob(torch, batch, synth, lib, n, width, height, interval, dev)
        for first, rows in BANDS:
            if first + rows > height:  # (a rehearsal at a toy size)
                first, rows = height // 2, min(rows, height // 4)
            what = f"{(first % interval != 0) + ((first + rows) % interval != 0)} edges"
            bands = {name: torch.zeros((n, rows, width), dtype=torch.uint8, device=dev) for name, _ in calls}

            def once(name, call):
                begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                begin.record()
                errcs = call(blob, offsets, sizes, [None] * n, [first] * n, [rows] * n, [bands[name][f] for f in range(n)], lib=lib)
                end.record()
                torch.cuda.synchronize()
                assert (errcs == 0).all(), (name, errcs)
                return begin.elapsed_time(end), (time.perf_counter() - t0) * 1e3

            before = capi.band_marker_counters(lib)
            for name, call in calls:  # the warm-up, and the bands to compare
                once(name, call)
            after = capi.band_marker_counters(lib)
            assert torch.equal(bands["markers"], bands["existing"]) and torch.equal(bands["markers"], frames[:, first:first + rows])
            times = {name: ([], []) for name, _ in calls}
            for _ in range(args.repeats):
                for name, call in calls:
                    ev, host = once(name, call)
                    times[name][0].append(ev)
                    times[name][1].append(host)
            counted = {k: after[k] - before[k] for k in after}
            for name, _ in calls:
                ev, host = times[name]
                lines.append(f"{interval:>3} {first:>5}+{rows:<3} {what:>7} {name:>9} "
                             f"{statistics.median(ev):10.1f} ({min(ev):.1f} .. {max(ev):.1f}) "
                             f"{statistics.median(host):10.1f} ({min(host):.1f} .. {max(host):.1f})   {counted if name == 'markers' else ''}")
            if min(times["markers"][0]) > max(times["existing"][0]):  # (device events: the table's first column)
                slower.append((interval, first))
            print("\n".join(lines[-2:]), flush=True)
    lines += ["", "the new call is slower than the existing call beyond the spread on: " + (str(slower) if slower else "none of the four inputs")]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
