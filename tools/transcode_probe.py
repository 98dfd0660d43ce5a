#!/usr/bin/env python3
"""Measures charls_amd_transcode_batch_device (charls_amd.h part 2j) on the GPU: 256 frames of 2048 x 2048 8-bit gray, coded the
way the reference codes them (no restart intervals), re-coded with a restart interval of 64 lines.

  (a) the call against the caller-side composition -- probe, ragged decode into a buffer the caller owns (allocated once,
      outside the clock), ragged encode --, the sides alternating: host clock around each, and the device-event time of their
      launches (charls_amd_last_timings [0]);
  (b) the call with its window forced to a quarter of the batch (TRANSCODE_WINDOW_FRAMES);
  (c) what the calling thread's work areas hold after the call, beside the frames the composition's caller allocates;
  (d) the plain batch decode (charls_amd_decode_batch_device_packed) of the outputs against that of the inputs;
  (e) charls_amd_transcode_batch_host from pinned memory, beside the device call on the same bytes: what is left is copies.

Every row is warmed up once and repeated (--repeats, at least 3); the table gives the median and the spread (min .. max).

    python tools/transcode_probe.py [--frames 256] [--repeats 3] [--out FILE]

The results go to FILE, by default profiles/r20_transcode.txt.  Needs the GPU: without one it fails."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

BITS = 8
INTERVAL = 64


def spread(values, digits=1):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits), "max": round(max(values), digits),
            "runs": len(values)}


def show(s):
    return f"{s['median']:9.1f} ({s['min']:.1f} .. {s['max']:.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--width", type=int, default=2048)  # (a rehearsal at a toy size; the rows to quote are 2048 x 2048)
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_transcode.txt"))
    args = ap.parse_args()
    assert args.repeats >= 3, "at least three repeats: a difference means nothing without the spread"

    import torch
    from charls_amd import batch, capi, synth
    assert torch.cuda.is_available(), "this tool measures on the GPU and does not fall back"
    lib = capi.load_product()
    dev = torch.device("cuda:0")
    n, width, height = args.frames, args.width, args.height
    mpix = n * width * height / 1e6
    lines, results = [], []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    # ---- the inputs: the batch encoder without a restart interval writes the reference's streams; packed with alignment 1
    frames = synth.frames_torch(n, width, height, seed0=2, bits=BITS, device=dev)
    slot = batch.estimated_destination_size(width, height, BITS, 1)
    blob_in = torch.empty(n * slot + (1 << 20), dtype=torch.uint8, device=dev)
    first = batch.encode_batch_packed(frames, packed=blob_in, bits_per_sample=BITS, lib=lib)
    assert (first.errcs == 0).all()
    offsets_in, sizes_in = first.offsets[:n].copy(), first.sizes.copy()
    in_bytes = int(first.offsets[n])
    del frames
    blob_out = torch.empty(in_bytes + n * (4096 + 2 * (height // INTERVAL + 1)) + (1 << 20), dtype=torch.uint8, device=dev)
    blob_ref = torch.empty_like(blob_out)
    spec = capi.transcode_spec(restart_interval=INTERVAL)
    frame_bytes = width * height
    owned = torch.empty(n * frame_bytes, dtype=torch.uint8, device=dev)  # what the composition's caller allocates
    say(f"# transcode_probe: {n} frames of {width} x {height} x {BITS} bit, no restart intervals -> Ri = {INTERVAL}; {args.repeats} repeats after one warm-up")
    say(f"# device {torch.cuda.get_device_name(0)}; input blob {in_bytes / 1e6:.1f} MB; times in ms, rates in MPix/s of the batch")

    def the_call():
        a = time.perf_counter()
        got = batch.transcode_batch(blob_in, offsets_in, sizes_in, spec, blob_out, lib=lib)
        b = time.perf_counter()
        assert (got.errcs == 0).all()
        return (b - a) * 1e3, batch.last_timings(lib)[0], got

    def the_composition():
        a = time.perf_counter()
        _, sizes, errcs = batch.probe_packed(blob_in, offsets_in, sizes_in, lib=lib)
        assert (errcs == 0).all() and int(sizes.max()) == frame_bytes
        outs = [owned[f * frame_bytes:(f + 1) * frame_bytes] for f in range(n)]
        params, errcs, gpu = batch.decode_batch_ragged(blob_in, offsets_in, sizes_in, outs, lib=lib)
        assert (errcs == 0).all()
        device_ms = gpu[0]
        for f in range(n):
            params[f].restart_interval = INTERVAL
        got = batch.encode_batch_ragged(outs, [params[f] for f in range(n)], blob_ref, lib=lib)
        device_ms += batch.last_timings(lib)[0]
        b = time.perf_counter()
        assert (got.errcs == 0).all()
        return (b - a) * 1e3, device_ms, got

    # ---- (a), (b): warm-up and the same bytes, once, outside the clock
    batch.release_work_areas(lib)
    _, _, got = the_call()
    held = batch.work_area_bytes(lib)
    _, _, ref = the_composition()
    assert got.offsets.tolist() == ref.offsets.tolist() and got.sizes.tolist() == ref.sizes.tolist()
    out_bytes = int(got.offsets[n])
    assert torch.equal(blob_out[:out_bytes], blob_ref[:out_bytes])
    offsets_out, sizes_out = got.offsets[:n].copy(), got.sizes.copy()
    quarter = max(1, n // 4)
    taken = {"call": ([], []), "composition": ([], []), f"call, window {quarter}": ([], [])}
    for _ in range(args.repeats):  # alternating: whatever else the machine does hits every row alike
        host_ms, device_ms, _ = the_call()
        taken["call"][0].append(host_ms)
        taken["call"][1].append(device_ms)
        host_ms, device_ms, _ = the_composition()
        taken["composition"][0].append(host_ms)
        taken["composition"][1].append(device_ms)
        capi.set_knob("TRANSCODE_WINDOW_FRAMES", quarter, lib)
        host_ms, device_ms, _ = the_call()
        capi.set_knob("TRANSCODE_WINDOW_FRAMES", None, lib)
        taken[f"call, window {quarter}"][0].append(host_ms)
        taken[f"call, window {quarter}"][1].append(device_ms)
    say("\n(a), (b) re-coding the batch: host clock ms, device-event ms of the launches")
    for name, (host_ms, device_ms) in taken.items():
        r = {"row": name, "host_ms": spread(host_ms), "device_ms": spread(device_ms), "mpix_s": round(mpix / (statistics.median(host_ms) / 1e3), 1)}
        results.append(r)
        say(f"  {name:24s} host {show(r['host_ms'])}   device {show(r['device_ms'])}   {r['mpix_s']:8.1f} MPix/s")
    ratio = statistics.median(taken["call"][0]) / statistics.median(taken["composition"][0])
    small = statistics.median(taken[f"call, window {quarter}"][0]) / statistics.median(taken["call"][0])
    say(f"  call / composition (medians, host clock): {ratio:.3f};  window {quarter} / one window: {small:.3f}")
    results.append({"row": "ratios", "call_over_composition": round(ratio, 3), "quarter_window_over_whole": round(small, 3)})

    # ---- (c)
    say(f"\n(c) work areas of the calling thread after the call: {held / 1e9:.3f} GB (charls_amd_work_area_bytes, all roles: the frames of the")
    say(f"    window, the encoder's staging and pipeline areas, the decoder's buffers); the composition's caller allocates {n * frame_bytes / 1e9:.3f} GB")
    say("    of frames and the encoder's and decoder's areas besides")
    results.append({"row": "memory", "work_area_bytes": int(held), "caller_frames_bytes": n * frame_bytes})

    # ---- (d): what it is for
    back = torch.empty((n, height, width), dtype=torch.uint8, device=dev)

    def plain_decode(blob, offsets, sizes):
        a = time.perf_counter()
        _, errcs, gpu = batch.decode_batch_packed(blob, offsets, sizes, back, lib=lib)
        b = time.perf_counter()
        assert (errcs == 0).all()
        return (b - a) * 1e3, gpu[0]

    plain_decode(blob_in, offsets_in, sizes_in)
    plain_decode(blob_out, offsets_out, sizes_out)
    taken = {"inputs (no intervals)": ([], []), f"outputs (Ri = {INTERVAL})": ([], [])}
    for _ in range(args.repeats):
        for name, tables in zip(taken, ((blob_in, offsets_in, sizes_in), (blob_out, offsets_out, sizes_out))):
            host_ms, device_ms = plain_decode(*tables)
            taken[name][0].append(host_ms)
            taken[name][1].append(device_ms)
    say("\n(d) charls_amd_decode_batch_device_packed of the whole batch")
    for name, (host_ms, device_ms) in taken.items():
        r = {"row": "decode " + name, "host_ms": spread(host_ms), "device_ms": spread(device_ms), "mpix_s": round(mpix / (statistics.median(host_ms) / 1e3), 1)}
        results.append(r)
        say(f"  {name:24s} host {show(r['host_ms'])}   device {show(r['device_ms'])}   {r['mpix_s']:8.1f} MPix/s")
    gain = statistics.median(taken["inputs (no intervals)"][0]) / statistics.median(taken[f"outputs (Ri = {INTERVAL})"][0])
    say(f"  the outputs decode {gain:.2f} x as fast as the inputs; they are {out_bytes / in_bytes:.4f} x their size")
    results.append({"row": "gain", "decode_speedup": round(gain, 2), "size_ratio": round(out_bytes / in_bytes, 4)})
    del back

    # ---- (e): the host form, pinned memory
    host_in = torch.empty(in_bytes + 64, dtype=torch.uint8).pin_memory()
    host_in[:in_bytes + 32].copy_(blob_in[:in_bytes + 32])
    host_out = torch.empty(out_bytes + (1 << 20), dtype=torch.uint8).pin_memory()

    def host_form():
        a = time.perf_counter()
        got = batch.transcode_batch_host(host_in.numpy(), offsets_in, sizes_in, spec, host_out.numpy(), lib=lib)
        b = time.perf_counter()
        assert (got.errcs == 0).all() and int(got.offsets[n]) == out_bytes
        return (b - a) * 1e3

    host_form()
    assert torch.equal(host_out[:out_bytes], blob_out[:out_bytes].cpu())
    host_ms, device_call_ms = [], []
    for _ in range(args.repeats):
        host_ms.append(host_form())
        device_call_ms.append(the_call()[0])
    whole, inside = spread(host_ms), spread(device_call_ms)
    share = 1 - inside["median"] / whole["median"]
    say("\n(e) charls_amd_transcode_batch_host, pinned memory, beside the device call on the same bytes (host clock, ms)")
    say(f"  host form {show(whole)}   device call {show(inside)}   left for copies and the lane: {100 * share:.1f} % of the host form")
    say(f"  ({(in_bytes + out_bytes) / 1e6:.1f} MB cross PCIe: the streams up, the streams down)")
    results.append({"row": "host form", "host_ms": whole, "device_call_ms": inside, "copy_share": round(share, 4)})
    say("\n# transcode counters (frames re-coded, windows, refused for a table, behind the capacity): " + str(capi.transcode_counters(lib)))
    for r in results:
        lines.append(json.dumps(r))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("written:", args.out)


if __name__ == "__main__":
    main()
