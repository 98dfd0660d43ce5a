"""The corner corpus (tests/corners.py) through the emulated kernels: the unmodified kernel sources compiled for the host
(tests/emu), fed with frames that drive the model into its corner states -- C and B on their clamps, escape codes in both
modes, contexts halved at N = RESET (RESET = 3 too), the largest NEAR and k, N << k == A, RUNindex 31 -- instead of the
kinds of charls_amd.synth.  Which frames a kernel gets is corners.EMU_ROUTES; tests/test_corner_census_cpu.py asserts from
the census that a kernel's frames reach every corner that can occur on it.

The frames of a launch of the group kernels are the frames of one geometry and one set of thresholds in the corpus'
order: different corners sit side by side in the lane groups of ONE wavefront, each in another rare path in the same step.
Everything is compared for equality with the oracle: scan bytes, pixels and result records.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import corners
import emu_bind
import jls_container
import test_emu_group_measure as measure
import test_emu_seek_index as seek
from test_emu_group_decode import _encode_group, _launch, _launch_pixels
from test_emu_serial_kernels import _stream_copy


class Scan:
    """One scan of a corner frame: its pixels in the user's layout, the oracle's entropy-coded segment and what the oracle
    decodes from it."""

    def __init__(self, c, index, start, end, jls, pixels, misalignment=None):
        self.c, self.index = c, index
        self.nc = 1 if c.ilv == 0 else c.comps
        bps = 1 if c.bits <= 8 else 2
        self.stride = c.width * bps * self.nc
        size = self.stride * c.height
        self.source = np.frombuffer(c.img.tobytes(), dtype=np.uint8)[index * size:(index + 1) * size].copy()
        self.want = pixels[index * size:(index + 1) * size]
        self.segment = jls[start:end]
        self.stream = _stream_copy(jls, start, misalignment)
        self.pc = corners.coding_parameters(c)

    def decode_desc(self, keep):
        out = np.zeros(self.stride * self.c.height, dtype=np.uint8)
        c = self.c
        return out, emu_bind.make_desc(c.width, c.height, self.nc, c.ilv, c.bits, c.near, c.ct, self.pc, 0, out, self.stride, self.stream, keep)

    def encode_desc(self, keep):
        out = np.zeros(len(self.segment) + 64, dtype=np.uint8)
        c = self.c
        return out, emu_bind.make_desc(c.width, c.height, self.nc, c.ilv, c.bits, c.near, c.ct, self.pc, 0, self.source.copy(), self.stride, out, keep)


_scans = {}


def scans(name):
    if name not in _scans:
        cc = corners.coded(name)
        cont = jls_container.parse(cc.jls)
        assert len(cont.scans) == (cc.corner.comps if cc.corner.ilv == 0 else 1)
        _scans[name] = [Scan(cc.corner, i, s.data_start, s.data_end, cc.jls, cc.pixels) for i, s in enumerate(cont.scans)]
    return _scans[name]


def turn(names, k, n):
    """Every n-th frame from the k-th on.  Where several kernels take the same frames, each frame goes to them in turn (all of
    them get every frame on the GPU, tests/test_gpu_corners.py): the file stays at about three minutes."""
    return [x for i, x in enumerate(names) if i % n == k]


def each(route, keep=None):
    return [n for n in corners.route_frames(route, "emu") if keep is None or keep(corners.CORPUS[n])]


def cases(names, by="thresholds"):
    return [pytest.param(i, v, id=corners.batch_id(k)) for i, (k, v) in enumerate(corners.batches(names, by).items())]


# near-lossless gray and line-interleaved frames have two kernels, the group decoder and (NEAR_DECODE_PIXELS) the pixel decoder
_NEAR_BOTH = [n for n in each("pixel_decode") if corners.CORPUS[n].ilv != 2]
GROUP_DECODE = [n for n in each("group_decode") if n not in turn(_NEAR_BOTH, 1, 2)]
PIXEL_DECODE = [n for n in each("pixel_decode") if n not in turn(_NEAR_BOTH, 0, 2)]


def check_decoded(launch, names, flags=0):
    """`launch(descs)` -> results for all the scans of `names` at once: errc 0, no flag (the wave decoder: its own, 1), the
    segment's length, the oracle's pixels."""
    keep, outs, descs, all_scans = [], [], [], [s for n in names for s in scans(n)]
    for s in all_scans:
        out, d = s.decode_desc(keep)
        outs.append(out)
        descs.append(d)
    res = launch(descs)
    for s, r, out in zip(all_scans, res, outs):
        assert (r.errc, r.flags, r.bytes) == (0, flags, len(s.segment)), (s.c.name, s.index, r.errc, r.flags)
        assert out.tobytes() == s.want, (s.c.name, s.index)


def one_by_one(kernel):
    def launch(descs):
        res = (emu_bind.ScanResult * len(descs))()
        for k, d in enumerate(descs):
            getattr(emu_bind.lib(), kernel)((emu_bind.ScanDesc * 1)(d), C.byref(res[k]), 1)
        return res
    return launch


# ---- decoders -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i,names", cases(GROUP_DECODE))
def test_group_decoder(i, names):
    """The C++ rendering of the step loop of scan_group_decode.hip, lossless and kNear; G taken in turn over the batches, and
    four wavefronts per workgroup for every ninth one."""
    group = (8, 16, 32)[i % 3]
    L = emu_bind.lib()
    check_decoded(lambda descs: _launch(L, descs, group), names)
    if i % 9 == 1 and corners.CORPUS[names[0]].comps == 1:
        def waves(descs):
            n = len(descs)
            res = (emu_bind.ScanResult * n)()
            assert L.emu_decode_scans_group_waves((emu_bind.ScanDesc * n)(*descs), res, n, 32, 4) == 0
            return res
        check_decoded(waves, names)


@pytest.mark.parametrize("i,names", cases(PIXEL_DECODE))
def test_pixel_decoders(i, names):
    group = (8, 16, 32)[i % 3]
    check_decoded(lambda descs: _launch_pixels(emu_bind.lib(), descs, group), names)


@pytest.mark.parametrize("name", turn(each("fast_decode"), 0, 3))
def test_fast_decoder(name):
    check_decoded(one_by_one("emu_decode_scans_fast"), [name])


@pytest.mark.parametrize("name", turn(each("exact_decode"), 1, 3))
def test_wave_decoder(name):
    check_decoded(one_by_one("emu_decode_scans_wave"), [name], flags=1)


@pytest.mark.parametrize("name", each("serial_decode"))
def test_serial_decoder(name):
    check_decoded(one_by_one("emu_decode_scans_serial"), [name])


class SeekScan(seek.Scan):
    """tests/test_emu_seek_index.py's harness on scan 0 of a corner frame."""

    def __init__(self, name):
        s = scans(name)[0]
        c = s.c
        self.pc, self.width, self.height, self.bits, self.near, self.ilv = s.pc, c.width, c.height, c.bits, c.near, c.ilv
        self.comps, self.planes, self.row, self.stream = s.nc, s.nc, s.stride, s.stream
        self.point_bytes = seek.lib().emu_seek_point_bytes(c.width, self.planes, int(c.bits > 8))


@pytest.mark.parametrize("name", turn(each("seek_decode", keep=lambda c: c.ct == 0), 2, 3))
def test_seek_decoder(name):
    """Seek points every 7 lines: the resume states carry C, RUNindex and the run contexts at their extremes.  Emitting decodes as
    the plain decoder does, every interval resumed from its point ends in exactly the next point's state."""
    sc = scans(name)[0]
    s = SeekScan(name)
    px, r, points = s.emit(7)
    assert r == (0, 1, len(sc.segment)) and px.tobytes() == sc.want
    got, results = s.resume(7, points)
    assert got.tobytes() == sc.want
    for e, f, _ in results[:-1]:
        assert e == 0 and f & seek.CHECKED and not f & seek.MISMATCH
    assert results[-1] == r


# ---- encoders -----------------------------------------------------------------------------------------------------------------

def check_encoded(launch, names):
    keep, outs, descs, all_scans = [], [], [], [s for n in names for s in scans(n)]
    for s in all_scans:
        out, d = s.encode_desc(keep)
        outs.append(out)
        descs.append(d)
    res = launch(descs)
    for s, r, out in zip(all_scans, res, outs):
        assert r.errc == 0 and out[:r.bytes].tobytes() == s.segment, (s.c.name, s.index, r.errc, r.bytes, len(s.segment))
    return descs, res, keep   # (the descriptors point into `keep`)


@pytest.mark.parametrize("i,names", cases(each("group_encode")))
def test_group_encoder_and_its_measuring_form(i, names):
    """scan_group_encode.hip: k from the exponents of two float conversions, mad24 for e (2 NEAR + 1) and the B update,
    sign_extend for the modulo reduction, med3 for the clamps.  The measuring form gives the length without writing a byte."""
    group = (8, 16, 32, 64)[i % 4]
    descs, res, keep = check_encoded(lambda descs: _encode_group(emu_bind.lib(), descs, group), names)
    if i % 2:
        return   # the measuring form: every other batch
    group = 16 if group == 32 else group   # (the measuring form has the instantiations the product launches: 8, 16, 64)
    n = len(descs)
    canaries = []
    for d in descs:
        canary = np.full(64, measure.CANARY, dtype=np.uint8)
        canaries.append(canary)
        d.stream, d.stream_capacity, d.line_scratch = canary.ctypes.data, 0, None
    measured = (emu_bind.ScanResult * n)()
    assert measure.measure_lib().emu_measure_pixels_group((emu_bind.ScanDesc * n)(*descs), measured, n, group) == 0
    assert [(m.errc, m.bytes) for m in measured] == [(0, r.bytes) for r in res]
    assert all((c == measure.CANARY).all() for c in canaries)


@pytest.mark.parametrize("name", each("serial_encode"))
def test_serial_encoder(name):
    def launch(descs):
        res = (emu_bind.ScanResult * len(descs))()
        emu_bind.lib().emu_encode_scans_serial((emu_bind.ScanDesc * len(descs))(*descs), res, len(descs))
        return res
    check_encoded(launch, [name])


SPECULATION = [(64, 32, (8, 8, 24)), (16, 0, (32, 0, 0)), (1024, 1024, (2048, 2048, 32768))]


@pytest.mark.parametrize("i,names", cases(each("tile_encode"), by="parameters"))
def test_tile_pipeline(monkeypatch, i, names):
    """The tile pipeline in line mode and (PIXEL_MODE = 1; sample-interleaved scans always) in pixel mode, the modes and the job
    sizes and warm-ups of its speculation taken in turn: jobs of 16 events without warm-up put a job boundary where C sits on
    its clamp."""
    mode = ("line", "pixel")[i % 2]
    if mode == "pixel":
        monkeypatch.setenv("CHARLS_AMD_PIXEL_MODE", "1")
    job, warm, runs = SPECULATION[(i // 2) % 3]

    def launch(descs):
        n = len(descs)
        res = (emu_bind.ScanResult * n)()
        emu_bind.tile_lib().emu_encode_tile_pipeline((emu_bind.ScanDesc * n)(*descs), res, n, job, warm, runs[0], runs[1], runs[2])
        return res
    check_encoded(launch, names)
