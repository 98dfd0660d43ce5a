"""The MEASURING form of the group encoder (scan_group_encode.hip, kMeasure) on the CPU harness, through a driver of its own
(tests/emu/emu_measure_driver.cpp): for every descriptor ScanResult.bytes must be what the encoding form reports with an
ample destination AND the length of the entropy-coded segment of the oracle's stream, errc 0, and nothing may be written
through ScanDesc.stream -- a canary buffer handed in with stream_capacity 0 and no line_scratch comes back untouched.
Test infrastructure only."""
import functools
import os

import numpy as np
import pytest

import emu_bind
import jls_container
import oracle_bind as ob
from charls_amd import synth

CANARY = 0xA5
GROUPS = (8, 16, 64)
KINDS = ("zero", "gradient", "noise")  # zero: every line is one run to its end
LAYOUTS = {"gray": (1, 0), "sample": (3, 2), "line": (3, 1)}  # components, interleave mode
_measure = None


def measure_lib():
    global _measure
    if _measure is None:
        _measure = emu_bind._build_and_load("emu_measure_driver.cpp", os.path.join(emu_bind.ROOT, "tests", "_emu_build", "libjls_emu_measure.so"))
    return _measure


def largest_near(bits):
    return min(255, ((1 << bits) - 1) // 2)


@functools.lru_cache(maxsize=None)
def oracle_segment(w, h, bits, comps, ilv, near, kind, seed):
    """(pixels as bytes, the entropy-coded segment of the oracle's stream, validated preset parameters)."""
    img = synth.frame_numpy(w, h, seed=seed, bits=bits, components=comps, kind=kind, interleaved=True)
    jls = ob.encode(img, width=w, height=h, bits_per_sample=bits, component_count=comps, interleave_mode=ilv, near_lossless=near)
    cont = jls_container.parse(jls)
    assert len(cont.scans) == 1
    scan = cont.scans[0]
    return np.ascontiguousarray(img).tobytes(), jls[scan.data_start:scan.data_end], jls_container.validated_pc(cont.pc, bits, near)


def check(scans, group):
    """scans: [(w, h, bits, comps, ilv, near, kind, seed)], one geometry, one launch of each form."""
    n = len(scans)
    keep, measure_descs, encode_descs, outs, canaries, wants = [], [], [], [], [], []
    for w, h, bits, comps, ilv, near, kind, seed in scans:
        pixels, segment, pc = oracle_segment(w, h, bits, comps, ilv, near, kind, seed)
        wants.append(segment)
        pix = np.frombuffer(pixels, dtype=np.uint8).copy()
        row = w * comps * (1 if bits <= 8 else 2)
        out = np.zeros(len(segment) + 64, dtype=np.uint8)
        outs.append(out)
        encode_descs.append(emu_bind.make_desc(w, h, comps, ilv, bits, near, 0, pc, 0, pix, row, out, keep))
        canary = np.full(len(segment) + 64, CANARY, dtype=np.uint8)
        canaries.append(canary)
        d = emu_bind.make_desc(w, h, comps, ilv, bits, near, 0, pc, 0, pix, row, canary, keep)
        d.stream_capacity = 0
        d.line_scratch = None
        measure_descs.append(d)
    measured = (emu_bind.ScanResult * n)()
    assert measure_lib().emu_measure_pixels_group((emu_bind.ScanDesc * n)(*measure_descs), measured, n, group) == 0
    encoded = (emu_bind.ScanResult * n)()
    assert emu_bind.lib().emu_encode_pixels_group((emu_bind.ScanDesc * n)(*encode_descs), encoded, n, group) == 0
    for k in range(n):
        assert encoded[k].errc == 0 and outs[k][:encoded[k].bytes].tobytes() == wants[k], (scans[k], group)
        assert (measured[k].errc, measured[k].bytes) == (0, encoded[k].bytes), (scans[k], group)
        assert measured[k].bytes == len(wants[k]), (scans[k], group)
        assert (canaries[k] == CANARY).all(), (scans[k], group)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("bits", [8, 12, 16])
def test_measured_bytes_equal_the_encoder_and_the_oracle(bits, layout):
    """Every G x widths around the lanes of a group (1, 2, G - 1, G, G + 1, 65) x NEAR 0, 1, 3 and the largest legal, the
    heights 1, 2, 5 taking turns so that every width and every NEAR meets each of them (the harness runs a thread per lane:
    the full product would take minutes); the three kinds of data are the scans of one launch (they share NEAR: the pixel
    loop where it applies)."""
    comps, ilv = LAYOUTS[layout]
    heights = (1, 2, 5)
    for group in GROUPS:
        for wi, w in enumerate(sorted({1, 2, group - 1, group, group + 1, 65})):
            for ni, near in enumerate((0, 1, 3, largest_near(bits))):
                check([(w, heights[(wi + ni) % 3], bits, comps, ilv, near, kind, 3) for kind in KINDS], group)


@pytest.mark.parametrize("near", [0, 1, 2, 4, 8])
def test_stuffed_bytes_are_counted(near):
    """The 65 x 5 16-bit noise frame (seed 3) has 0xFF bytes in its segment at these NEARs: every one makes the byte after it a
    7-bit byte, so a count that ignored the byte values would be short."""
    scan = (65, 5, 16, 1, 0, near, "noise", 3)
    segment = oracle_segment(*scan)[1]
    assert 0xFF in segment
    for group in GROUPS:
        check([scan], group)


def test_mixed_near_in_one_wavefront():
    """Four scans of one wavefront with NEAR 0, 1, 2 and 4 (they do not share a gradient table: the general step), 8- and
    16-bit, every kind of data."""
    for bits in (8, 16):
        for kind in KINDS:
            check([(33, 5, bits, 1, 0, near, kind, 5 + near) for near in (0, 1, 2, 4)], 16)
            check([(17, 4, bits, 3, 2, near, kind, 5 + near) for near in (4, 2, 1, 0)], 16)


@pytest.mark.parametrize("group,count", [(8, 19), (16, 9)])
def test_more_scans_than_a_wavefront_holds(group, count):
    """Several workgroups, the last one partly filled (a count that is no multiple of 64 / G), candidate-major as the host
    lays them out: the scans of one NEAR contiguous, the wavefronts at the seams mixed."""
    nears = (0, 2, 7)
    per = -(-count // len(nears))
    scans = [(37, 4, 8, 1, 0, nears[k // per], KINDS[k % 3], 11 + k) for k in range(count)]
    assert count % (64 // group) != 0 and count > 64 // group
    check(scans, group)
    scans = [(21, 3, 12, 3, 1, nears[k // per], KINDS[k % 3], 11 + k) for k in range(count)]
    check(scans, group)
