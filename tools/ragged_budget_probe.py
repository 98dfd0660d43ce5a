#!/usr/bin/env python3
"""Measures the byte-budget calls of charls_amd.h part 2k on the GPU, each beside what a caller can do without it.  Two batches:
256 frames of 2048 x 2048 8-bit gray (the batch of tools/transcode_probe.py), and a mix of three geometries (2048 x 2048,
2048 x 1024, 1024 x 1024) interleaved in the caller's order.  Candidates (0, 1, 2, 4); every frame's budget is half its lossless
size.

  (a) charls_amd_encode_batch_device_ragged_budget beside the SUM of charls_amd_encode_batch_device_budget over its geometry
      groups -- what a caller has without part 2k, the re-pack into the caller's order it would still owe not included;
  (b) charls_amd_transcode_batch_device_budget beside its caller-side composition (probe, ragged decode into frames the caller
      owns, ragged budget encode) and beside the plain re-code of part 2j at one fixed NEAR: the difference is the candidates;
  (c) charls_amd_transcode_batch_host_budget from pinned memory beside the device call on the same bytes.

Everything is warmed up once; the alternatives alternate inside one process; every row is repeated (--repeats, at least 5) and
the table gives the median and the spread (min .. max) of the host clock, ms.

    python tools/ragged_budget_probe.py [--frames 256] [--repeats 5] [--out FILE]

The results go to FILE, by default profiles/r21_ragged_budget.txt (another name at any other --size or --frames).  Needs the GPU: without one it fails."""
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
CANDIDATES = (0, 1, 2, 4)
FIXED_NEAR = 2


def spread(values, digits=1):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits), "max": round(max(values), digits),
            "runs": len(values)}


def show(s):
    return f"{s['median']:9.1f} ({s['min']:.1f} .. {s['max']:.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--size", type=int, default=2048)  # (a rehearsal at a toy size; the rows to quote are 2048)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:  # (a rehearsal does not overwrite the profile)
        name = "r21_ragged_budget.txt" if (args.size, args.frames) == (2048, 256) else f"rehearsal_ragged_budget_{args.frames}x{args.size}.txt"
        args.out = os.path.join(ROOT, "profiles", name)
    assert args.repeats >= 5, "at least five repeats: a difference means nothing without the spread"

    import torch
    from charls_amd import batch, capi, synth
    assert torch.cuda.is_available(), "this tool measures on the GPU and does not fall back"
    lib = capi.load_product()
    dev = torch.device("cuda:0")
    n, size = args.frames, args.size
    lines, results = [], []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def clock(fn):
        a = time.perf_counter()
        out = fn()
        return (time.perf_counter() - a) * 1e3, out

    def alternate(rows):
        """rows: name -> callable.  One warm-up of each, then --repeats rounds with the rows in turn."""
        for fn in rows.values():
            fn()
        taken = {name: [] for name in rows}
        for _ in range(args.repeats):
            for name, fn in rows.items():
                taken[name].append(clock(fn)[0])
        return taken

    def report(title, taken, mpix, reference):
        say("\n" + title)
        for name, ms in taken.items():
            r = {"row": f"{title.split()[0]} {name}", "host_ms": spread(ms), "mpix_s": round(mpix / (statistics.median(ms) / 1e3), 1)}
            results.append(r)
            say(f"  {name:44s} {show(r['host_ms'])} ms   {r['mpix_s']:9.1f} MPix/s")
        ref = taken[reference]
        say(f"  spread of `{reference}` itself: {(max(ref) - min(ref)) / statistics.median(ref) * 100:.1f} % of its median")
        for name, ms in taken.items():
            if name != reference:
                ratio = statistics.median(ms) / statistics.median(ref)
                say(f"  {name} / {reference} (medians): {ratio:.3f}")
                results.append({"row": f"{title.split()[0]} ratio", "of": name, "over": reference, "ratio": round(ratio, 3)})

    say(f"# ragged_budget_probe: candidates {CANDIDATES}, budgets at half of every frame's lossless size; {args.repeats} repeats after one warm-up")
    say(f"# device {torch.cuda.get_device_name(0)}; host clock ms around each call, rates in MPix/s of the batch")

    geometries = {"uniform": [(size, size)], "mixed": [(size, size), (size, size // 2), (size // 2, size // 2)]}
    for label, shapes in geometries.items():
        # ---- the frames: one tensor per geometry group, named in the caller's order a, b, c, a, b, c, ...
        per = n // len(shapes)
        groups = [synth.frames_torch(per, w, h, seed0=2 + 100 * g, bits=BITS, device=dev) for g, (w, h) in enumerate(shapes)]
        order = [(g, k) for k in range(per) for g in range(len(shapes))]
        count = len(order)
        tensors = [groups[g][k] for g, k in order]
        params = [batch.codec_params(shapes[g][0], shapes[g][1], BITS) for g, _ in order]
        mpix = sum(w * h for w, h in shapes) * per / 1e6
        lossless, errcs = batch.measure_batch_ragged(tensors, params, (0,), lib=lib)
        assert (errcs == 0).all()
        budgets = (lossless[:, 0] // 2).astype(np.uint64)
        group_budgets = [np.array([budgets[at] for at, (g, _) in enumerate(order) if g == gi], dtype=np.uint64) for gi in range(len(shapes))]
        room = int(lossless.sum()) + count * 4096
        packed = torch.empty(room, dtype=torch.uint8, device=dev)
        packed_groups = [torch.empty(room, dtype=torch.uint8, device=dev) for _ in shapes]
        say(f"\n## {label}: {count} frames, " + ", ".join(f"{per} of {w} x {h}" for w, h in shapes) + f"; {mpix:.0f} MPix; lossless {int(lossless.sum()) / 1e6:.1f} MB")

        def ragged_call():
            got, nears = batch.encode_batch_ragged_budget(tensors, params, budgets, CANDIDATES, packed, lib=lib)
            return got, nears

        def uniform_calls():
            out = []
            for gi, (w, h) in enumerate(shapes):
                out.append(batch.encode_batch_budget(groups[gi], group_budgets[gi], CANDIDATES, packed_groups[gi], bits_per_sample=BITS, lib=lib))
            return out

        got, nears = ragged_call()
        per_group = uniform_calls()
        for gi in range(len(shapes)):  # the same choices and sizes, group by group
            mine = [at for at, (g, _) in enumerate(order) if g == gi]
            assert nears[mine].tolist() == per_group[gi][1].tolist() and got.sizes[mine].tolist() == per_group[gi][0].sizes.tolist()
        coded = int((nears >= 0).sum())
        say(f"  coded {coded} of {count}; NEAR chosen: " + ", ".join(f"{c}: {int((nears == c).sum())}" for c in CANDIDATES) +
            f", none: {count - coded}; output {int(got.offsets[count]) / 1e6:.1f} MB")
        results.append({"row": f"{label} choices", "coded": coded, "frames": count, "out_bytes": int(got.offsets[count])})
        report(f"(a) {label}: budgeted encode of raw frames", alternate({"ragged budget call": ragged_call, "sum of uniform budget calls": uniform_calls}),
               mpix, "sum of uniform budget calls")

        # ---- (b), (c): the archive -- the frames coded losslessly as the reference codes them -- re-coded to the budgets
        blob_in = torch.empty(room, dtype=torch.uint8, device=dev)
        archive = batch.encode_batch_ragged(tensors, params, blob_in, lib=lib)
        assert (archive.errcs == 0).all()
        offsets_in, sizes_in, in_bytes = archive.offsets[:count].copy(), archive.sizes.copy(), int(archive.offsets[count])
        budgets = (sizes_in // 2).astype(np.uint64)
        blob_out, blob_ref = torch.empty(room, dtype=torch.uint8, device=dev), torch.empty(room, dtype=torch.uint8, device=dev)
        frame_bytes = [w * h for g, _ in order for w, h in [shapes[g]]]
        owned = [torch.empty(b, dtype=torch.uint8, device=dev) for b in frame_bytes]  # what the composition's caller allocates
        spec = capi.transcode_spec()

        def budget_transcode():
            return batch.transcode_batch_budget(blob_in, offsets_in, sizes_in, spec, budgets, CANDIDATES, blob_out, lib=lib)

        def composition():
            _, sizes, errcs = batch.probe_packed(blob_in, offsets_in, sizes_in, lib=lib)
            assert (errcs == 0).all()
            decoded, errcs, _ = batch.decode_batch_ragged(blob_in, offsets_in, sizes_in, owned, lib=lib)
            assert (errcs == 0).all()
            return batch.encode_batch_ragged_budget(owned, [decoded[f] for f in range(count)], budgets, CANDIDATES, blob_ref, strides=[0] * count,
                                                    lib=lib)

        def plain_transcode():
            return batch.transcode_batch(blob_in, offsets_in, sizes_in, capi.transcode_spec(near_lossless=FIXED_NEAR), blob_ref, lib=lib)

        got, nears = budget_transcode()
        ref, ref_nears = composition()
        out_bytes = int(got.offsets[count])
        assert nears.tolist() == ref_nears.tolist() and got.offsets.tolist() == ref.offsets.tolist()
        assert torch.equal(blob_out[:out_bytes], blob_ref[:out_bytes])
        say(f"  archive {in_bytes / 1e6:.1f} MB -> {out_bytes / 1e6:.1f} MB; re-coded {int((nears >= 0).sum())} of {count}")
        taken = alternate({"budget transcode": budget_transcode, "composition (probe, decode, budget encode)": composition,
                           f"plain transcode at NEAR {FIXED_NEAR}": plain_transcode})
        report(f"(b) {label}: budgeted re-coding of the archive", taken, mpix, "composition (probe, decode, budget encode)")
        budget_transcode()
        t = batch.last_timings(lib)
        say(f"  device-event ms of one budget transcode: all {t[0]:.1f}, dominant kernels {t[1]:.1f}, decodes {t[2]:.1f}, sizing and encoding {t[3]:.1f}")

        host_in = torch.empty(in_bytes + 64, dtype=torch.uint8).pin_memory()
        host_in[:in_bytes + 32].copy_(blob_in[:in_bytes + 32])
        host_out = torch.empty(out_bytes + (1 << 20), dtype=torch.uint8).pin_memory()

        def host_form():
            return batch.transcode_batch_host_budget(host_in.numpy(), offsets_in, sizes_in, spec, budgets, CANDIDATES, host_out.numpy(), lib=lib)

        back, back_nears = host_form()
        assert back_nears.tolist() == nears.tolist() and torch.equal(host_out[:out_bytes], blob_out[:out_bytes].cpu())
        report(f"(c) {label}: the host form, pinned memory ({(in_bytes + out_bytes) / 1e6:.1f} MB cross PCIe)",
               alternate({"host form": host_form, "device call": budget_transcode}), mpix, "device call")
        del groups, tensors, packed, packed_groups, blob_in, blob_out, blob_ref, owned, host_in, host_out
        batch.release_work_areas(lib)
        torch.cuda.empty_cache()

    say("\n# measure counters (scans sized by the measuring kernels, launches of them, scans coded for real): " + str(batch.measure_counters(lib)))
    say("# transcode counters (frames re-coded, windows, refused for a table, behind the capacity): " + str(capi.transcode_counters(lib)))
    for r in results:
        lines.append(json.dumps(r))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("written:", args.out)


if __name__ == "__main__":
    main()
