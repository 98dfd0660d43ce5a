"""The calls of charls_amd.h part 2k (byte budgets for ragged frames and for re-coding) without a GPU: what they refuse for the
whole call is refused before a device is asked for -- the answer is the check's code here, where no device exists, not
device_unavailable -- and writes nothing, a call without frames succeeds, both library names export the calls, and the corpus
of the GPU tests (tests/budget_model.py) reaches every outcome of the selection rule."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import budget_model as bm
import common
from charls_amd import batch, capi

INVALID_ARGUMENT, INVALID_ARGUMENT_SIZE = 101, 110
LIB_DIR = os.path.join(common.ROOT, "charls_amd", "lib")
NAMES = ["charls_amd_measure_batch_device_ragged", "charls_amd_encode_batch_device_ragged_budget",
         "charls_amd_transcode_batch_device_budget", "charls_amd_transcode_batch_host_budget"]
SOMEWHERE = 0x1000  # a non-NULL "device pointer": no call below gets as far as touching it

u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def l():
    return batch._bind(capi.load_product())


class Call:
    """Valid arguments of all four calls over n frames, every output filled with a canary.  The blobs of the transcode calls are
    host memory: the device form only looks at the pointers for NULL before it asks for a device."""

    def __init__(self, n, nears=(0, 1, 2), spec_count=1, alignment=1):
        self.n = n
        self.alignment = alignment
        self.sources = (batch.FrameSource * max(n, 1))()
        for f in range(n):
            self.sources[f] = batch.FrameSource(batch.codec_params(16, 8), SOMEWHERE, 0, 0, 0)
        self.nears = np.asarray(nears, dtype=np.int32)
        self.count = len(nears)
        self.budgets = np.full(max(n, 1), 1000, dtype=np.uint64)
        self.offsets_in = np.arange(max(n, 1), dtype=np.uint64) * 100
        self.sizes_in = np.full(max(n, 1), 100, dtype=np.uint64)
        self.specs = (capi.TranscodeSpec * max(spec_count, 1))()
        for k in range(spec_count):
            self.specs[k] = capi.transcode_spec(restart_interval=8)
        self.spec_count = spec_count
        self.blob_in = np.full(4096, 0x3C, dtype=np.uint8)
        self.blob_out = np.full(4096, 0xA5, dtype=np.uint8)
        self.offsets = np.full(n + 1, 77, dtype=np.uint64)
        self.sizes = np.full(max(n, 1), 78, dtype=np.uint64)
        self.near_out = np.full(max(n, 1), 55, dtype=np.int32)
        self.errcs = np.full(max(n, 1), -1, dtype=np.int32)
        self.sizes_out = np.full(max(n, 1) * max(self.count, 1), 99, dtype=np.uint64)
        self.params = (batch.CodecParams * max(n, 1))()
        for f in range(max(n, 1)):
            self.params[f].near_lossless = 79

    def measure_args(self):
        return [self.n, self.sources, self.nears.ctypes.data_as(i32p), self.count, self.sizes_out.ctypes.data_as(u64p),
                self.errcs.ctypes.data_as(i32p), None]

    def budget_args(self):
        return [self.n, self.sources, self.budgets.ctypes.data_as(u64p), self.nears.ctypes.data_as(i32p), self.count, SOMEWHERE, 1 << 20,
                self.alignment, self.offsets.ctypes.data_as(u64p), self.sizes.ctypes.data_as(u64p), self.near_out.ctypes.data_as(i32p),
                self.errcs.ctypes.data_as(i32p), None]

    def transcode_args(self):
        return [self.n, self.blob_in.ctypes.data, self.offsets_in.ctypes.data_as(u64p), self.sizes_in.ctypes.data_as(u64p), self.specs,
                self.spec_count, self.budgets.ctypes.data_as(u64p), self.nears.ctypes.data_as(i32p), self.count, self.blob_out.ctypes.data,
                self.blob_out.nbytes, self.alignment, self.offsets.ctypes.data_as(u64p), self.sizes.ctypes.data_as(u64p),
                self.near_out.ctypes.data_as(i32p), self.params, self.errcs.ctypes.data_as(i32p)]

    def untouched(self):
        return bool((self.offsets == 77).all() and (self.sizes == 78).all() and (self.near_out == 55).all() and (self.errcs == -1).all() and
                    (self.sizes_out == 99).all() and (self.blob_out == 0xA5).all() and (self.blob_in == 0x3C).all() and
                    all(self.params[f].near_lossless == 79 for f in range(max(self.n, 1))))

    def ragged(self, l):
        """The codes of (measure, budget encode); a call that is refused must not have written anything."""
        got = (l.charls_amd_measure_batch_device_ragged(*self.measure_args()), l.charls_amd_encode_batch_device_ragged_budget(*self.budget_args()))
        assert self.untouched()
        return got

    def transcode(self, l):
        """The code of the device form and of the host form of the budget transcode, which agree."""
        args = self.transcode_args()
        device, host = l.charls_amd_transcode_batch_device_budget(*args, None), l.charls_amd_transcode_batch_host_budget(*args)
        assert device == host, (device, host)
        assert self.untouched()
        return device

    def all_four(self, l):
        return self.ragged(l) + (self.transcode(l),)


def test_null_tables_and_blobs(l):
    for n in (0, 2):
        c = Call(n)
        for at in (1, 2, 4, 5):  # sources, near_candidates, sizes_out, errcs
            args = c.measure_args()
            args[at] = None
            assert l.charls_amd_measure_batch_device_ragged(*args) == INVALID_ARGUMENT, (n, at)
        for at in (1, 2, 3, 8, 9, 10, 11):  # sources, budgets, near_candidates, offsets, sizes, near_out, errcs
            args = c.budget_args()
            args[at] = None
            assert l.charls_amd_encode_batch_device_ragged_budget(*args) == INVALID_ARGUMENT, (n, at)
        for at in (2, 3, 4, 6, 7, 12, 13, 14, 15, 16):  # the tables of part 2j, budgets, near_candidates, near_out
            args = c.transcode_args()
            args[at] = None
            assert l.charls_amd_transcode_batch_device_budget(*args, None) == INVALID_ARGUMENT, (n, at)
            assert l.charls_amd_transcode_batch_host_budget(*args) == INVALID_ARGUMENT, (n, at)
        assert c.untouched()
    c = Call(2)  # the blobs of a call that has frames
    args = c.budget_args()
    args[5] = None
    assert l.charls_amd_encode_batch_device_ragged_budget(*args) == INVALID_ARGUMENT
    for at in (1, 9):
        args = c.transcode_args()
        args[at] = None
        assert l.charls_amd_transcode_batch_device_budget(*args, None) == INVALID_ARGUMENT, at
        assert l.charls_amd_transcode_batch_host_budget(*args) == INVALID_ARGUMENT, at
    assert c.untouched()


@pytest.mark.parametrize("count", [0, 65])
def test_candidate_count(l, count):
    for n in (0, 2):
        c = Call(n, nears=[0] * 65)
        c.count = count
        assert c.all_four(l) == (INVALID_ARGUMENT,) * 3


def test_sixty_four_candidates_are_taken(l):
    c = Call(0, nears=list(range(64)))
    assert l.charls_amd_measure_batch_device_ragged(*c.measure_args()) == 0
    assert l.charls_amd_encode_batch_device_ragged_budget(*c.budget_args()) == 0
    args = c.transcode_args()
    assert l.charls_amd_transcode_batch_device_budget(*args, None) == 0 and l.charls_amd_transcode_batch_host_budget(*args) == 0


@pytest.mark.parametrize("alignment", [0, 3, 24, 8192])
def test_offset_alignment(l, alignment):
    for n in (0, 2):
        c = Call(n, alignment=alignment)
        assert l.charls_amd_encode_batch_device_ragged_budget(*c.budget_args()) == INVALID_ARGUMENT
        assert c.transcode(l) == INVALID_ARGUMENT


def test_the_frame_table(l):
    """`reserved` must be 0, d_pixels must be there, and max_stream_bytes must be 0: the budget is the limit."""
    for bad in (0, 2):
        for field, value in (("reserved", 1), ("d_pixels", None), ("max_stream_bytes", 4096)):
            c = Call(3)
            setattr(c.sources[bad], field, value)
            assert c.ragged(l) == (INVALID_ARGUMENT,) * 2, (bad, field)


@pytest.mark.parametrize("frames, spec_count", [(3, 0), (3, 2), (3, 4), (2, 3), (0, 2)])
def test_spec_count_is_one_or_the_frame_count(l, frames, spec_count):
    assert Call(frames, spec_count=max(spec_count, 0)).transcode(l) == INVALID_ARGUMENT


@pytest.mark.parametrize("bit", [16, 32, 1 << 31])
def test_an_undefined_set_bit(l, bit):
    for spec_count, bad in ((1, 0), (3, 0), (3, 2)):
        c = Call(3, spec_count=spec_count)
        c.specs[bad].set |= bit
        assert c.transcode(l) == INVALID_ARGUMENT


def test_a_spec_must_not_set_near(l):
    """The candidates decide NEAR: a spec that sets it is refused, wherever it stands; the plain call of part 2j takes it."""
    for spec_count, bad in ((1, 0), (3, 0), (3, 2)):
        c = Call(3, spec_count=spec_count)
        c.specs[bad] = capi.transcode_spec(near_lossless=0, restart_interval=8)
        assert c.transcode(l) == INVALID_ARGUMENT


def test_reserved_of_a_spec_must_be_zero(l):
    for spec_count, bad in ((1, 0), (3, 1), (3, 2)):
        c = Call(3, spec_count=spec_count)
        c.specs[bad].reserved = 1
        assert c.transcode(l) == INVALID_ARGUMENT


def test_an_offset_plus_size_that_overflows(l):
    for bad in (0, 2):
        c = Call(3)
        c.offsets_in[bad] = (1 << 64) - 50
        assert c.transcode(l) == INVALID_ARGUMENT_SIZE


def test_no_frames_is_success(l):
    c = Call(0, nears=[4, 0, 4, 2])
    assert l.charls_amd_measure_batch_device_ragged(*c.measure_args()) == 0
    assert c.untouched()
    args = c.budget_args()
    args[5], args[6] = None, 0  # no frames, no blob
    assert l.charls_amd_encode_batch_device_ragged_budget(*args) == 0
    assert c.offsets[0] == 0
    for spec_count in (0, 1):
        c = Call(0, spec_count=spec_count)
        args = c.transcode_args()
        args[1] = args[9] = None
        args[10] = 0
        assert l.charls_amd_transcode_batch_device_budget(*args, None) == 0
        assert c.offsets[0] == 0
        c.offsets[0] = 77
        assert l.charls_amd_transcode_batch_host_budget(*args) == 0
        assert c.offsets[0] == 0
        assert (c.errcs == -1).all() and (c.sizes == 78).all() and (c.near_out == 55).all()


@pytest.mark.parametrize("library", ["libcharls_amd.so", "libcharls.so.3"])
def test_both_library_names_export_the_calls(library):
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB_DIR, library)], capture_output=True, text=True).stdout.split("\n")
    exported = {line.split()[-1] for line in names if line.strip()}
    assert set(NAMES) <= exported


def test_the_python_calls_are_bound(l):
    for name in ("measure_batch_ragged", "encode_batch_ragged_budget", "transcode_batch_budget", "transcode_batch_host_budget"):
        assert callable(getattr(batch, name))
    assert all(getattr(l, name).restype is C.c_int32 for name in NAMES)


def test_the_corpus_reaches_every_outcome_of_the_selection():
    """Not a test of the library -- it passes without part 2k -- but the precondition of tests/test_gpu_ragged_budget.py, a
    condition on its INPUTS: the oracle's sizes of its frame kinds at its candidates, with
    the budgets it derives from them, meet every outcome -- so the GPU test cannot pass without meeting them."""
    frames = bm.call_frames()
    seen = set()
    for candidates in (bm.WIDE, bm.NARROW):
        for position, (kind, repeat) in enumerate(frames):
            if bm.refusal(kind, candidates):
                continue
            sizes = bm.oracle_sizes(kind, repeat, candidates)
            budget = bm.budget_of(kind, repeat, candidates, position)
            k = bm.choose(sizes, budget)
            seen.add("first" if k == 0 else "later" if k > 0 else "none")
            if k >= 0 and sizes[k] == budget:
                seen.add("exact")
            if k != 0 and any(s - 1 == budget for s in sizes[:k if k > 0 else None]):
                seen.add("misses by one")
            if candidates == bm.NARROW and k == 1:
                seen.add("the repeated candidate, where it stands first")
            if candidates == bm.NARROW and k > 2 and sizes[1] > budget:
                seen.add("behind the repeated candidate")
    assert seen == {"first", "later", "none", "exact", "misses by one", "the repeated candidate, where it stands first",
                    "behind the repeated candidate"}
    # 200 is legal for the 12- and 16-bit kinds only, and the HP1 kind is refused by every list that holds a NEAR above 0
    assert [kind for kind in bm.KINDS if bm.refusal(kind, bm.WIDE) == 0] == ["gray12_19x9", "gray16_65x5"]
    assert [kind for kind in bm.KINDS if bm.refusal(kind, bm.NARROW)] == ["rgb_sample_hp1_16x8"]
