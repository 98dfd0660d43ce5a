"""The step loop of scan_group_decode.hip as a loop of trips, on the CPU harness: the C++ rendering of the loop -- the
specification of the assembly in scan_group_step.inc -- decodes the frames of tests/step_trips_frames.py to the oracle's
pixels with 8, 16 and 32 lanes per scan: every width around the lengths of a call, run events in both copies of a trip and in the
last samples of a call and of a line (the run service rounds what is left of the count down to whole trips), contexts halved
in both copies, both texts of the 8-bit container, samples that wrap, near-lossless and wider samples.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import emu_bind
import jls_container
import step_trips_frames as F
from test_emu_serial_kernels import _stream_copy

SERVED_IN_LOOP = 16   # path counter of the kernel: run services inside the step loop

CASES = F.all_cases()


def _descs(frames, keep):
    outs, descs, ends = [], [], []
    for f in frames:
        f.code()
        h, w = f.img.shape
        cont = jls_container.parse(f.jls)
        pc = jls_container.validated_pc(cont.pc, cont.bits, f.near)
        bps = 1 if f.bits <= 8 else 2
        pix = np.zeros(w * h * bps, dtype=np.uint8)
        scan = cont.scans[0]
        descs.append(emu_bind.make_desc(w, h, 1, 0, f.bits, f.near, 0, pc, 0, pix, w * bps, _stream_copy(f.jls, scan.data_start), keep))
        outs.append(pix)
        ends.append(scan.data_end - scan.data_start)
    return outs, descs, ends


def _check(frames, res, outs, ends):
    for i, (f, r, o, e) in enumerate(zip(frames, res, outs, ends)):
        assert (r.errc, r.flags, r.bytes) == (0, 0, e), (i, r.errc, r.flags, r.bytes, e)
        assert o.tobytes() == f.pixels, i


@pytest.mark.parametrize("group", F.GROUPS)
@pytest.mark.parametrize("name", list(CASES))
def test_frames_decode_to_the_oracles_pixels(name, group):
    frames, keep = CASES[name], []
    outs, descs, ends = _descs(frames, keep)
    n = len(descs)
    arr, res = (emu_bind.ScanDesc * n)(*descs), (emu_bind.ScanResult * n)()
    if name in F.SERVED:
        counts = (C.c_ulonglong * 32)()
        assert emu_bind.profile_lib().emu_profile_decode_group(arr, res, n, group, counts) == 0
        print(name, group, "run services inside the step loop:", counts[SERVED_IN_LOOP])
        assert counts[SERVED_IN_LOOP] > 0, "no run event of these frames was served by the step loop"
    else:
        assert emu_bind.lib().emu_decode_scans_group(arr, res, n, group) == 0
    _check(frames, res, outs, ends)


@pytest.mark.parametrize("name", ["maxval_255_and_127", "runs_cols_1_8", "reset_3_4_64"])
def test_four_wavefronts_per_workgroup(name):
    """16 lanes per scan, four wavefronts: 16 scans per workgroup (the 7-bit and the 8-bit frames of one launch sit in separate
    workgroups)."""
    frames, keep = CASES[name], []
    outs, descs, ends = _descs(frames, keep)
    n = len(descs)
    arr, res = (emu_bind.ScanDesc * n)(*descs), (emu_bind.ScanResult * n)()
    assert emu_bind.lib().emu_decode_scans_group_waves(arr, res, n, 16, 4) == 0
    _check(frames, res, outs, ends)
