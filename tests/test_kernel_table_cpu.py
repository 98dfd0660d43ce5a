"""The library's kernels by name: what the device objects of a build hold equals tests/golden/kernel_names.txt (328 names, written
from the build before the launch code was split into units and moved to kernel_dispatch.h), and no kernel is compiled into two
objects.  A launch unit that loses an instantiation, gains one or includes a kernel source a second time fails here, on the
CPU.  (tools/compare_kernels.py compares registers and instruction text of two builds.)"""
import collections
import os

from charls_amd import build as b

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_names.txt")


def built_names():
    b.build()
    objs = [os.path.join(b.OUT_DIR, "obj", s.replace("/", "_") + ".o") for s in b.SOURCES if s.endswith(".hip")]
    missing = [o for o in objs if not os.path.exists(o)]
    assert not missing, f"device objects missing beside a current library (build(force=True) makes them): {missing}"
    return [k["name"] for o in objs for k in b.kernel_resources(o)]


def test_the_kernels_are_the_golden_ones_each_once():
    names = built_names()
    with open(GOLDEN) as f:
        golden = f.read().split()
    assert len(golden) == 328 and golden == sorted(set(golden))
    twice = [n for n, c in collections.Counter(names).items() if c > 1]
    assert not twice, twice
    assert sorted(names) == golden, (sorted(set(golden) - set(names)), sorted(set(names) - set(golden)))
    families = collections.Counter()
    for n in names:
        for family in ("decode_scans_groupI", "decode_pixels_groupI", "encode_pixels_groupI", "decode_scans_waveI",
                       "decode_scans_wave_emitI", "decode_scans_wave_resumeI", "decode_scans_fastI"):
            families[family] += family in n
    assert dict(families) == {"decode_scans_groupI": 68, "decode_pixels_groupI": 42, "encode_pixels_groupI": 112, "decode_scans_waveI": 8,
                              "decode_scans_wave_emitI": 8, "decode_scans_wave_resumeI": 8, "decode_scans_fastI": 2}
