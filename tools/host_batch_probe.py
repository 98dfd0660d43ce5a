#!/usr/bin/env python3
"""Measures the batch API on host memory (charls_amd.h part 2i) on the GPU: 4096 x 4096 8-bit frames, encode and decode
through charls_amd_encode_batch_host / charls_amd_decode_batch_host from pinned and from pageable memory, and -- in the same
process, alternating with them -- the reference: bench.py's Python pipeline on torch streams from pinned tensors
(`batch_api_host_buffers`; this file carries its own copy of that loop).  Every row is warmed up once and repeated
(--repeats, at least 3); the table gives the median and the spread (min .. max) of each.  The clock is the host's, around
calls that return when the results are in host memory (the reference ends in a device synchronise): PCIe inclusive.  With
--sweep the lane count and the window length are swept on the first batch size, pinned memory.

    python tools/host_batch_probe.py [--frames 256,1024] [--repeats 3] [--sweep] [--out FILE]

The results go to FILE, by default profiles/rNN_host_batch.txt with the next free round number.  Needs the GPU: without one
it fails."""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

WIDTH = HEIGHT = 4096
BITS = 8
CHUNK = 64  # frames per chunk of the reference's encode pipeline (bench.py)


def next_profile_path():
    rounds = [int(m.group(1)) for name in os.listdir(os.path.join(ROOT, "profiles")) if (m := re.match(r"r(\d+)_", name))]
    return os.path.join(ROOT, "profiles", f"r{max(rounds, default=0) + 1:02d}_host_batch.txt")


def spread(values):
    return {"median": round(statistics.median(values), 1), "min": round(min(values), 1), "max": round(max(values), 1), "runs": len(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="256,1024")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--width", type=int, default=WIDTH)   # (a rehearsal at a toy size; the rows to quote are 4096 x 4096)
    ap.add_argument("--height", type=int, default=HEIGHT)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 3, "at least three repeats: a difference means nothing without the spread"
    out_path = args.out or next_profile_path()

    import torch
    from charls_amd import batch, capi, synth
    assert torch.cuda.is_available(), "this tool measures on the GPU and does not fall back"
    lib = capi.load_product()
    dev = torch.device("cuda:0")
    width, height = args.width, args.height
    mpix = width * height / 1e6
    pitch = (batch.estimated_destination_size(width, height, BITS, 1) + 255) & ~255
    counts = [int(x) for x in args.frames.split(",") if x]
    most = max(counts)

    frames = synth.frames_torch(most, width, height, seed0=2, bits=BITS, device=dev)
    streams = torch.empty((most, pitch), dtype=torch.uint8, device=dev)
    out = torch.empty_like(frames)
    host_frames = torch.empty((most, height, width), dtype=torch.uint8).pin_memory()
    host_frames.copy_(frames)
    host_streams = torch.empty((most, pitch), dtype=torch.uint8).pin_memory()
    up, down, main_stream = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev), torch.cuda.current_stream(dev)
    torch.cuda.synchronize()
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    # ---- the reference: bench.py's pipeline (host_buffers / pipelined), from pinned torch tensors
    def pipelined(upload, code, download, chunks):
        ready = []
        with torch.cuda.stream(up):
            upload(0)
            ready.append(up.record_event())
        for k in range(chunks):
            if k + 1 < chunks:
                with torch.cuda.stream(up):
                    upload(k + 1)
                    ready.append(up.record_event())
            main_stream.wait_event(ready[k])
            code(k)
            coded = main_stream.record_event()
            with torch.cuda.stream(down):
                down.wait_event(coded)
                download(k)
        torch.cuda.synchronize()

    def reference(n):
        sizes = np.zeros(n, dtype=np.uint64)

        def rng(k):
            return slice(k * CHUNK, min(n, (k + 1) * CHUNK))

        def encode_chunk(k):
            e = batch.encode_batch(out[rng(k)], bits_per_sample=BITS, streams=streams[rng(k)], lib=lib)
            sizes[rng(k)] = e.sizes

        def download_streams(k):
            for f in range(k * CHUNK, min(n, (k + 1) * CHUNK)):
                host_streams[f, :int(sizes[f])].copy_(streams[f, :int(sizes[f])], non_blocking=True)

        def upload_streams(k):
            for f in range(n):
                streams[f, :int(sizes[f])].copy_(host_streams[f, :int(sizes[f])], non_blocking=True)

        a = time.perf_counter()
        pipelined(lambda k: out[rng(k)].copy_(host_frames[rng(k)], non_blocking=True), encode_chunk, download_streams, -(-n // CHUNK))
        b = time.perf_counter()
        back = host_frames_back[:n]
        pipelined(upload_streams, lambda k: batch.decode_batch(streams[:n], sizes, out[:n], lib=lib),
                  lambda k: back.copy_(out[:n], non_blocking=True), 1)
        c = time.perf_counter()
        return n * mpix / (b - a), n * mpix / (c - b), sizes

    # ---- the C calls
    def c_calls(n, source, packed, back):
        a = time.perf_counter()
        got = batch.encode_batch_host(source[:n], packed, bits_per_sample=BITS, lib=lib)
        b = time.perf_counter()
        _, errcs = batch.decode_batch_host(packed, got.offsets, got.sizes, back[:n], lib=lib)
        c = time.perf_counter()
        assert (got.errcs == 0).all() and (errcs == 0).all()
        return n * mpix / (b - a), n * mpix / (c - b), got

    host_frames_back = torch.empty((most, height, width), dtype=torch.uint8).pin_memory()
    pinned_source, pinned_back = host_frames.numpy(), host_frames_back.numpy()
    say(f"# host_batch_probe: {width} x {height} x {BITS} bit, frames {counts}, {args.repeats} repeats after one warm-up, MPix/s, PCIe inclusive")
    say(f"# device {torch.cuda.get_device_name(0)}; lanes / window / staging: the library's defaults unless a row says otherwise")
    results = []
    for n in counts:
        _, _, sizes = reference(n)  # warm-up of the reference, and the sizes the packed buffers need
        total = int(sizes.sum())
        packed_pinned = torch.empty(total + (1 << 20), dtype=torch.uint8).pin_memory().numpy()
        pageable_source = np.empty((n, height, width), dtype=np.uint8)
        pageable_source[:] = pinned_source[:n]
        pageable_back = np.empty_like(pageable_source)
        packed_pageable = np.empty(total + (1 << 20), dtype=np.uint8)
        rows = {"python pipeline, pinned (reference)": lambda: reference(n)[:2],
                "C call, pinned": lambda: c_calls(n, pinned_source, packed_pinned, pinned_back)[:2],
                "C call, pageable": lambda: c_calls(n, pageable_source, packed_pageable, pageable_back)[:2]}
        # the same bytes on every path, once, outside the clock
        _, _, got = c_calls(n, pinned_source, packed_pinned, pinned_back)
        assert got.sizes.tolist() == sizes.tolist()
        for f in range(0, n, max(1, n // 8)):
            assert packed_pinned[int(got.offsets[f]):int(got.offsets[f] + got.sizes[f])].tobytes() == host_streams[f, :int(sizes[f])].numpy().tobytes()
        assert (pinned_back[:n] == pinned_source[:n]).all()
        c_calls(n, pageable_source, packed_pageable, pageable_back)  # (warm-up: the staging buffers)
        assert (pageable_back == pageable_source).all()
        taken = {name: ([], []) for name in rows}
        for _ in range(args.repeats):  # alternating: whatever else the box does hits every row alike
            for name, run in rows.items():
                e, d = run()
                taken[name][0].append(e)
                taken[name][1].append(d)
        say(f"\nframes {n}")
        for name, (e, d) in taken.items():
            r = {"frames": n, "path": name, "encode_mpix_s": spread(e), "decode_mpix_s": spread(d)}
            results.append(r)
            say(f"  {name:38s} encode {r['encode_mpix_s']['median']:9.1f} ({r['encode_mpix_s']['min']:.1f} .. {r['encode_mpix_s']['max']:.1f})"
                f"   decode {r['decode_mpix_s']['median']:8.1f} ({r['decode_mpix_s']['min']:.1f} .. {r['decode_mpix_s']['max']:.1f})")
        if args.sweep and n == counts[0]:
            # (encode only: a decode window shorter than the batch is a loss by the number of frames in flight, nothing to choose)
            say(f"\nsweep at {n} frames, pinned, encode: HOST_LANES x HOST_WINDOW_FRAMES (0 = the default rule), median of {args.repeats}")

            def c_encode():
                a = time.perf_counter()
                got = batch.encode_batch_host(pinned_source[:n], packed_pinned, bits_per_sample=BITS, lib=lib)
                assert (got.errcs == 0).all()
                return n * mpix / (time.perf_counter() - a)

            for lanes in (1, 2, 3, 4):
                for window in (0, 32, 64):
                    capi.set_knob("HOST_LANES", lanes, lib)
                    capi.set_knob("HOST_WINDOW_FRAMES", window if window else None, lib)
                    c_encode()
                    e = spread([c_encode() for _ in range(args.repeats)])
                    results.append({"frames": n, "path": "C call, pinned", "lanes": lanes, "window": window, "encode_mpix_s": e})
                    say(f"  lanes {lanes} window {window:3d}   encode {e['median']:9.1f} ({e['min']:.1f} .. {e['max']:.1f})")
            capi.set_knob("HOST_LANES", None, lib)
            capi.set_knob("HOST_WINDOW_FRAMES", None, lib)
        del packed_pinned, pageable_source, pageable_back, packed_pageable
    say("\n# counters (calls, windows, bytes up, bytes down, pageable bytes staged, device bytes held, pinned bytes held): " + str(batch.host_counters(lib)))
    for r in results:
        lines.append(json.dumps(r))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("written:", out_path)


if __name__ == "__main__":
    main()
