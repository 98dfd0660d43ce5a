"""The calls of charls_amd.h part 2f without a GPU: what they refuse for the whole call is refused before a device is asked
for (the answer is the check's code here, where no device exists, not device_unavailable) and before anything is written, a
call without frames succeeds, and both library names export the three entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import common
from charls_amd import batch, capi

INVALID_ARGUMENT = 101
INVALID_ARGUMENT_NEAR_LOSSLESS = 107
INVALID_ARGUMENT_JPEGLS_PC_PARAMETERS = 108
INVALID_ARGUMENT_COLOR_TRANSFORMATION = 109
INVALID_ARGUMENT_SIZE = 110
INVALID_ARGUMENT_STRIDE = 111
LIB_DIR = os.path.join(common.ROOT, "charls_amd", "lib")
NAMES = ["charls_amd_measure_batch_device", "charls_amd_encode_batch_device_budget", "charls_amd_measure_counters"]
SOMEWHERE = 0x1000  # a non-NULL "device pointer": no call below gets as far as touching it
W, H = 16, 8

u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def l():
    return batch._bind(capi.load_product())


class Call:
    """Valid arguments of both calls over n 16 x 8 frames (8-bit gray unless params says otherwise)."""

    def __init__(self, n, nears=(0, 1, 2), params=None, pitch=None, stride=0, alignment=1):
        self.n = n
        self.params = params or batch.codec_params(W, H)
        self.pitch = W * H * self.params.frame_info.component_count * 2 if pitch is None else pitch
        self.stride = stride
        self.alignment = alignment
        self.nears = np.asarray(nears, dtype=np.int32)
        self.count = len(nears)
        self.budgets = np.full(max(n, 1), 1000, dtype=np.uint64)
        self.offsets = np.full(n + 1, 77, dtype=np.uint64)
        self.sizes = np.full(max(n, 1), 10, dtype=np.uint64)
        self.near_out = np.full(max(n, 1), 55, dtype=np.int32)
        self.errcs = np.full(max(n, 1), -1, dtype=np.int32)
        self.sizes_out = np.full(max(n, 1) * max(self.count, 1), 99, dtype=np.uint64)

    def measure_args(self):
        return [C.byref(self.params), self.n, SOMEWHERE, self.pitch, self.stride, self.nears.ctypes.data_as(i32p), self.count,
                self.sizes_out.ctypes.data_as(u64p), None]

    def budget_args(self):
        return [C.byref(self.params), self.n, SOMEWHERE, self.pitch, self.stride, self.budgets.ctypes.data_as(u64p),
                self.nears.ctypes.data_as(i32p), self.count, SOMEWHERE, 1 << 20, self.alignment, self.offsets.ctypes.data_as(u64p),
                self.sizes.ctypes.data_as(u64p), self.near_out.ctypes.data_as(i32p), self.errcs.ctypes.data_as(i32p), None]

    def untouched(self):
        return bool((self.offsets == 77).all() and (self.sizes == 10).all() and (self.near_out == 55).all() and (self.errcs == -1).all() and
                    (self.sizes_out == 99).all())

    def both(self, l, refused=True):
        """The codes of (measure, budget); a call that is refused must not have written anything."""
        got = (l.charls_amd_measure_batch_device(*self.measure_args()), l.charls_amd_encode_batch_device_budget(*self.budget_args()))
        assert not refused or self.untouched()
        return got


def test_null_tables_and_pointers(l):
    for n in (0, 2):
        c = Call(n)
        for at in (0, 5, 7):  # params, near_candidates, sizes_out
            args = c.measure_args()
            args[at] = None
            assert l.charls_amd_measure_batch_device(*args) == INVALID_ARGUMENT, (n, at)
        for at in (0, 5, 6, 11, 12, 13, 14):  # params, budgets, near_candidates, offsets, sizes, near_out, errcs
            args = c.budget_args()
            args[at] = None
            assert l.charls_amd_encode_batch_device_budget(*args) == INVALID_ARGUMENT, (n, at)
        assert c.untouched()
    c = Call(2)  # the device pointers of a call that has frames
    args = c.measure_args()
    args[2] = None
    assert l.charls_amd_measure_batch_device(*args) == INVALID_ARGUMENT
    for at in (2, 8):
        args = c.budget_args()
        args[at] = None
        assert l.charls_amd_encode_batch_device_budget(*args) == INVALID_ARGUMENT, at
    assert c.untouched()


@pytest.mark.parametrize("count", [0, 65])
def test_candidate_count(l, count):
    for n in (0, 2):
        c = Call(n, nears=[0] * 65)
        c.count = count
        assert c.both(l) == (INVALID_ARGUMENT, INVALID_ARGUMENT)


def test_sixty_four_candidates_are_taken(l):
    assert Call(0, nears=list(range(64))).both(l, refused=False) == (0, 0)


@pytest.mark.parametrize("alignment", [0, 3, 8192])
def test_offset_alignment(l, alignment):
    for n in (0, 2):
        c = Call(n, alignment=alignment)
        assert l.charls_amd_encode_batch_device_budget(*c.budget_args()) == INVALID_ARGUMENT
        assert c.untouched()


@pytest.mark.parametrize("n", [0, 2])
def test_parameters_the_encoder_refuses_with_any_candidate(l, n):
    # NEAR above max_near_for(255) = 127, wherever it stands in the list; a negative one
    assert Call(n, nears=[0, 1, 128]).both(l) == (INVALID_ARGUMENT_NEAR_LOSSLESS,) * 2
    assert Call(n, nears=[128, 0]).both(l) == (INVALID_ARGUMENT_NEAR_LOSSLESS,) * 2
    assert Call(n, nears=[0, -1]).both(l) == (INVALID_ARGUMENT_NEAR_LOSSLESS,) * 2
    assert Call(0, nears=[0, 127]).both(l, refused=False) == (0, 0)  # the largest legal one passes (no frames: nothing asks for a device)
    # 12-bit samples: 255 is legal, 256 is not
    assert Call(n, nears=[256], params=batch.codec_params(W, H, 12)).both(l) == (INVALID_ARGUMENT_NEAR_LOSSLESS,) * 2
    # a colour transformation goes with NEAR 0 only
    rgb = batch.codec_params(W, H, 8, 3, 2, color_transformation=1)
    assert Call(n, nears=[0, 1], params=rgb).both(l) == (INVALID_ARGUMENT_COLOR_TRANSFORMATION,) * 2
    # preset parameters that hold for NEAR 0 and not for NEAR 3: T1 = 3 < NEAR + 1
    preset = batch.codec_params(W, H, preset=(255, 3, 7, 21, 64))
    assert Call(0, nears=[0, 2], params=preset).both(l, refused=False) == (0, 0)
    assert Call(n, nears=[0, 3], params=preset).both(l) == (INVALID_ARGUMENT_JPEGLS_PC_PARAMETERS,) * 2
    # the first refused candidate decides the code
    assert Call(n, nears=[1, 128], params=rgb).both(l) == (INVALID_ARGUMENT_COLOR_TRANSFORMATION,) * 2
    # the checks that do not depend on NEAR: a stride below the row, frames that do not fit their pitch
    assert Call(n, stride=W - 1).both(l) == (INVALID_ARGUMENT_STRIDE,) * 2
    assert Call(2, pitch=W * H - 1).both(l) == (INVALID_ARGUMENT_SIZE,) * 2


def test_no_frames(l):
    c = Call(0, nears=[4, 0, 4, 2])
    assert l.charls_amd_measure_batch_device(C.byref(c.params), 0, None, 0, 0, c.nears.ctypes.data_as(i32p), c.count,
                                             c.sizes_out.ctypes.data_as(u64p), None) == 0
    args = c.budget_args()
    args[2] = args[8] = None  # no frames, no blob
    args[3] = args[9] = 0
    assert l.charls_amd_encode_batch_device_budget(*args) == 0
    assert c.offsets[0] == 0
    assert (c.errcs == -1).all() and (c.sizes_out == 99).all()


def test_measure_counters_capacity(l):
    out = np.full(4, 12345, dtype=np.uint64)
    assert l.charls_amd_measure_counters(out.ctypes.data_as(u64p), 2) == 2
    assert out[0] != 12345 and out[1] != 12345 and out[2] == 12345 and out[3] == 12345
    assert l.charls_amd_measure_counters(out.ctypes.data_as(u64p), 4) == 3
    assert out[3] == 12345
    assert l.charls_amd_measure_counters(None, 3) == 0
    assert len(batch.measure_counters()) == 3


@pytest.mark.parametrize("library", ["libcharls_amd.so", "libcharls.so.3"])
def test_both_library_names_export_the_calls(library):
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB_DIR, library)], capture_output=True, text=True).stdout.split("\n")
    exported = {line.split()[-1] for line in names if line.strip()}
    assert set(NAMES) <= exported
