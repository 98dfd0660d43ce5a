"""Padded rows on the CPU: every kernel that has an emulated entry (tests/emu) gets a ScanDesc whose pixel_stride differs
from the packed row length, a base address 0, 1, 2 or 8 bytes off a 16-byte boundary, and frames `pitch` bytes apart in ONE
canary-filled arena (tests/strided.py).  A decoder must put the oracle's pixels into the rows and leave every other byte of
the arena alone (the gaps behind the rows, the bytes up to the pitch, the guard bands; `tight`: no byte behind the last
row); an encoder must write the oracle's bytes and leave the source alone.  Every comparison is for equality.

Geometry (R = packed row bytes): strides R + 1, R + 2, R + 13, roundup(R, 16) with R % 16 != 0 -- the first input after
whose uint4 stores the per-sample tail loop of the group kernels has anything to do --, roundup(R, 16) + 16 and R + 4096;
widths 1, 7, 16, 150, 257 (below, at and above the lanes per scan; R % 16 zero and non-zero), heights that include 1 and 2.
Pairwise, not a full product: every stride class on every kernel, every base offset with the strides that allow uint4
stores and with the ones that do not.  Test infrastructure only."""
import ctypes as C

import numpy as np
import pytest

import emu_bind
import jls_container
import strided as S
from strided import Geometry as G
from test_emu_serial_kernels import _stream_copy


def _results(n):
    return (emu_bind.ScanResult * n)()


def _decode_descs(lay, frames, arena, keep, restart=0):
    """One descriptor per scan (a planar frame: one per component, `stride * height` apart) and the bytes of each scan."""
    g = lay.g
    descs, ends = [], []
    for f, fr in enumerate(frames):
        cont = jls_container.parse(fr.jls)
        pc = jls_container.validated_pc(cont.pc, cont.bits, fr.near)
        assert len(cont.scans) == (g.comps if g.ilv == 0 else 1)
        for c, scan in enumerate(cont.scans):
            view = arena[lay.row_offset(f, c * g.height):]
            descs.append(emu_bind.make_desc(g.width, g.height, scan.components, scan.ilv, g.bits, scan.near, cont.transform, pc,
                                            restart, view, lay.stride, _stream_copy(fr.jls, scan.data_start), keep))
            ends.append(scan.data_end - scan.data_start)
    return descs, ends


def _decode(launch, g, cls, base, *, count=3, pitch="pad", tight=False, near=0, ct=0, preset=None, seed=1, speed=True):
    lay = S.layout(g, cls, base, count, pitch, tight)
    frames = [S.Coded(g, seed + 31 * f, near=near, ct=ct, preset=preset) for f in range(count)]
    arena, keep = lay.blank(), []
    descs, ends = _decode_descs(lay, frames, arena, keep)
    n = len(descs)
    res = _results(n)
    launch((emu_bind.ScanDesc * n)(*descs), res, n)
    for k in range(n):
        assert res[k].errc == 0 and res[k].bytes == ends[k], (k, res[k].errc, res[k].bytes, ends[k])
        if speed:
            assert res[k].flags == 0, (k, "the speed path handed a valid scan to the exact decoder")
    lay.check(arena, [fr.pixels for fr in frames])
    return lay


def _group(group):
    return lambda arr, res, n: _zero(emu_bind.lib().emu_decode_scans_group(arr, res, n, group))


def _group_waves(group, waves):
    return lambda arr, res, n: _zero(emu_bind.lib().emu_decode_scans_group_waves(arr, res, n, group, waves))


def _pixels(group):
    return lambda arr, res, n: _zero(emu_bind.lib().emu_decode_pixels_group(arr, res, n, group))


def _zero(rc):
    assert rc == 0, "no such instantiation"


# ---- the helper itself ------------------------------------------------------------------------------------------------------

def test_the_check_names_frame_row_and_offset():
    g = G(10, 3, comps=3, ilv=0)
    lay = S.layout(g, "p13", 1, 2, "pad", tight=True)
    frames = [np.arange(g.packed, dtype=np.uint8) for _ in range(2)]
    arena = lay.pad(frames)
    lay.check(arena, frames)
    assert arena.size == S.GUARD + 1 + lay.pitch + lay.need + S.GUARD and lay.need == 23 * 9 - 13
    assert (arena[:lay.first] == S.CANARY).all() and (arena[-S.GUARD:] == S.CANARY).all()
    assert arena[lay.row_offset(1, 4):][:10].tobytes() == frames[1][40:50].tobytes()  # component 1, line 1: band of stride * height
    for at, words in [(lay.row_offset(1, 4) + 3, "frame 1 row 4 (component 1 line 1) byte 3"), (lay.row_offset(0, 2) + 10, "the gap behind frame 0 row 2"),
                      (lay.first - 1, "guard band in front"), (lay.row_offset(0, 8) + 10, "up to the pitch behind frame 0"),
                      (lay.row_offset(1, 8) + 10, "the guard band behind frame 1, 0 bytes behind its last row")]:
        hurt = arena.copy()
        hurt[at] ^= 0x40
        with pytest.raises(AssertionError) as e:
            lay.check(hurt, frames)
        assert words in str(e.value) and f"arena offset {at} " in str(e.value), str(e.value)


# ---- scan_group_decode.hip, NL = 1: uint4 stores, the tail loop behind them, the per-sample loop ---------------------------

GROUP_NL1 = [  # group, width, height, bits, near, stride class, base, count, pitch, tight
    (8, 150, 5, 8, 0, "r16", 0, 9, "mod8", False),      # the tail behind the wide stores; every other scan of a wavefront unaligned
    (16, 150, 2, 8, 0, "r16", 0, 5, "mod0", True),      # all aligned, the smallest legal buffer
    (32, 150, 4, 8, 2, "r16", 0, 3, "mod8", False),
    (8, 257, 3, 8, 0, "r16p16", 0, 9, "mod0", False),
    (16, 257, 1, 8, 0, "r16p16", 8, 5, "pad", True),    # a stride that allows uint4, a base that does not
    (32, 16, 6, 8, 0, "r16p16", 1, 3, "pad", False),
    (8, 16, 5, 8, 2, "r16p16", 2, 9, "tight", True),
    (16, 7, 9, 8, 0, "r16", 0, 5, "mod8", False),       # width below G, R below one uint4
    (32, 7, 2, 8, 0, "p1", 0, 3, "pad", False),
    (8, 1, 7, 8, 0, "p2", 1, 9, "tight", True),
    (16, 150, 3, 8, 0, "p13", 2, 5, "pad", False),
    (32, 257, 2, 8, 0, "big", 8, 3, "pad", True),
    (8, 150, 3, 8, 0, "big", 0, 3, "mod8", False),      # R + 4096 is a multiple of 16 for no width here: per sample
    (16, 150, 4, 12, 0, "r16", 0, 5, "mod8", False),    # 16-bit samples: R = 300, the tail starts at sample 144
    (32, 150, 3, 16, 3, "r16", 0, 3, "mod0", True),
    (8, 257, 2, 16, 0, "r16p16", 2, 9, "even", False),
    (16, 16, 5, 12, 0, "r16p16", 0, 5, "mod8", False),  # R = 32: wide stores only, stride 48
    (32, 7, 3, 16, 0, "p2", 8, 3, "even", True),
    (8, 1, 2, 16, 2, "p2", 0, 9, "even", False),
    (16, 257, 3, 12, 0, "big", 2, 3, "even", False),
]


@pytest.mark.parametrize("group,w,h,bits,near,cls,base,count,pitch,tight", GROUP_NL1)
def test_group_decoder_rows(group, w, h, bits, near, cls, base, count, pitch, tight):
    _decode(_group(group), G(w, h, bits), cls, base, count=count, pitch=pitch, tight=tight, near=near, seed=w + h)


def test_group_decoder_unreached_tail_regression():
    """width = 150, stride = 160: the named first input whose finished line is stored as 9 uint4 and then 6 samples."""
    lay = _decode(_group(16), G(150, 6), 160, 0, count=4, pitch=160 * 6, tight=True)
    assert lay.stride % 16 == 0 and lay.pitch % 16 == 0 and lay.g.row % 16 == 6


@pytest.mark.parametrize("group,waves,w,h,bits,near,cls,base,count", [(16, 4, 150, 3, 8, 0, "r16", 0, 21), (32, 4, 257, 2, 12, 2, "r16p16", 0, 9),
                                                                       (32, 8, 150, 2, 8, 0, "p13", 1, 19), (32, 4, 4096, 2, 8, 0, "r16p16", 0, 3)])
def test_group_decoder_rows_with_several_wavefronts_per_workgroup(group, waves, w, h, bits, near, cls, base, count):
    """decode_scans_group<S, G, 1, W>; the 4096-wide frames are the W = 4 shape of wide lines."""
    _decode(_group_waves(group, waves), G(w, h, bits), cls, base, count=count, pitch="mod8", near=near, seed=w)


def test_group_decoder_planar_planes_are_stride_times_height_apart():
    """The component scans of planar frames as the batch API places them: plane c at c * stride * height."""
    _decode(_group(16), G(150, 3, comps=3, ilv=0), "r16", 0, count=3, pitch="mod8")
    _decode(_group(8), G(7, 2, bits=12, comps=4, ilv=0), "p2", 2, count=2, pitch="tight", tight=True)


# ---- scan_group_decode.hip, NL = 2..4: line-interleaved rows, with and without colour transform ----------------------------

@pytest.mark.parametrize("group,w,h,bits,comps,near,ct,cls,base,tight", [
    (8, 150, 3, 8, 3, 0, 1, "r16", 0, False), (16, 150, 2, 8, 3, 0, 0, "p1", 1, True), (32, 257, 2, 8, 2, 0, 0, "p2", 2, False),
    (8, 16, 5, 8, 4, 0, 0, "r16p16", 8, False), (16, 7, 4, 8, 3, 2, 0, "p13", 0, True), (32, 1, 3, 8, 3, 0, 2, "big", 1, False),
    (8, 150, 2, 16, 3, 0, 3, "r16", 0, True), (16, 7, 1, 12, 2, 3, 0, "p2", 2, False), (32, 16, 3, 16, 4, 0, 0, "r16p16", 8, False)])
def test_group_decoder_line_interleaved_rows(group, w, h, bits, comps, near, ct, cls, base, tight):
    _decode(_group(group), G(w, h, bits, comps, 1), cls, base, count=3, pitch="even", tight=tight, near=near, ct=ct, seed=w + comps)


# ---- scan_group_pixels.hip: sample-interleaved pixels (NC = 2..4) and its near-lossless line form --------------------------

@pytest.mark.parametrize("group,w,h,bits,comps,ilv,near,ct,cls,base,count,pitch,tight", [
    (8, 150, 3, 8, 3, 2, 0, 1, "r16", 0, 5, "mod8", False),   # R = 450: uint4 stores and a tail of 2 bytes
    (16, 150, 2, 8, 4, 2, 0, 0, "r16p16", 0, 3, "mod0", True), (32, 257, 2, 8, 2, 2, 3, 0, "r16", 8, 3, "pad", False),
    (8, 16, 4, 8, 3, 2, 0, 2, "r16p16", 1, 5, "pad", False), (16, 7, 5, 8, 3, 2, 3, 0, "p1", 2, 3, "tight", True),
    (32, 1, 3, 8, 4, 2, 0, 0, "p2", 1, 3, "pad", False), (8, 257, 1, 8, 3, 2, 0, 3, "p13", 0, 5, "pad", False),
    (16, 150, 2, 8, 2, 2, 0, 0, "big", 2, 3, "pad", True), (32, 150, 3, 16, 3, 2, 0, 1, "r16", 0, 3, "mod8", False),
    (8, 7, 2, 12, 4, 2, 3, 0, "p2", 8, 5, "even", True), (16, 16, 3, 16, 2, 2, 0, 0, "r16p16", 2, 3, "even", False),
    (8, 150, 3, 8, 3, 1, 2, 0, "r16", 0, 5, "mod8", False),   # NLINES = 3, near-lossless
    (16, 7, 2, 8, 2, 1, 3, 0, "p13", 1, 3, "pad", True), (32, 16, 2, 12, 4, 1, 2, 0, "big", 2, 3, "even", False),
    (8, 150, 2, 8, 1, 0, 2, 0, "r16", 0, 5, "mod8", False),   # near-lossless single component on the pixel kernel
])
def test_pixel_decoder_rows(group, w, h, bits, comps, ilv, near, ct, cls, base, count, pitch, tight):
    _decode(_pixels(group), G(w, h, bits, comps, ilv), cls, base, count=count, pitch=pitch, tight=tight, near=near, ct=ct, seed=w + comps)


# ---- the one-scan-per-wavefront decoders: fast, wave (exact), serial -----------------------------------------------------------

def _fast(arr, res, n):
    emu_bind.lib().emu_decode_scans_fast(arr, res, n)


def _wave(arr, res, n):
    emu_bind.lib().emu_decode_scans_wave(arr, res, n)


def _serial(arr, res, n):
    emu_bind.lib().emu_decode_scans_serial(arr, res, n)


@pytest.mark.parametrize("w,h,bits,cls,base,tight", [(150, 3, 8, "r16", 0, False), (257, 2, 8, "p1", 1, True), (16, 5, 8, "r16p16", 8, False),
                                                     (7, 1, 8, "p13", 2, True), (1, 4, 8, "p2", 0, False), (150, 2, 12, "big", 2, False),
                                                     (150, 3, 16, "r16", 0, True), (7, 2, 16, "p2", 8, False)])
def test_fast_decoder_rows(w, h, bits, cls, base, tight):
    _decode(_fast, G(w, h, bits), cls, base, count=2, pitch="even", tight=tight, seed=w)


@pytest.mark.parametrize("w,h,bits,comps,ilv,near,cls,base,tight", [
    (150, 3, 8, 1, 0, 0, "r16", 0, False), (257, 2, 8, 3, 0, 2, "p1", 1, True), (16, 3, 8, 3, 1, 0, "r16p16", 8, False),
    (7, 2, 8, 3, 2, 3, "p13", 2, True), (1, 4, 8, 4, 2, 0, "p2", 1, False), (150, 1, 8, 2, 1, 2, "big", 0, False),
    (150, 2, 16, 3, 2, 0, "r16", 0, True), (7, 3, 12, 1, 0, 0, "p2", 2, False), (16, 2, 16, 3, 1, 0, "r16p16", 8, False)])
def test_wave_decoder_rows(w, h, bits, comps, ilv, near, cls, base, tight):
    _decode(_wave, G(w, h, bits, comps, ilv), cls, base, count=2, pitch="even", tight=tight, near=near, seed=w + comps, speed=False)


@pytest.mark.parametrize("w,h,bits,comps,ilv,near,cls,base,pitch,tight", [
    (150, 3, 8, 1, 0, 0, "r16", 0, "pad", False), (257, 2, 8, 3, 0, 0, "p2", 2, "pad", True), (16, 3, 8, 3, 1, 2, "r16p16", 8, "pad", False),
    (7, 2, 8, 3, 2, 0, "big", 1, "tight", True),
    (150, 3, 16, 1, 0, 0, "p1", 0, "pad", False),    # 16-bit rows at odd addresses: the route the product keeps for the serial kernel
    (7, 2, 12, 3, 0, 2, "p13", 1, "pad", True), (16, 2, 16, 1, 0, 0, "p2", 1, "pad", False), (1, 5, 16, 3, 0, 0, "p13", 8, "tight", True),
    (257, 1, 16, 3, 2, 0, "p1", 2, "pad", False)])
def test_serial_decoder_rows(w, h, bits, comps, ilv, near, cls, base, pitch, tight):
    _decode(_serial, G(w, h, bits, comps, ilv), cls, base, count=2, pitch=pitch, tight=tight, near=near, seed=w + comps, speed=False)


# ---- restart_intervals_decode.hip, restart_intervals_encode.hip: the interval builders offset their sub-scans by j * lines * pixel_stride -------------------------

@pytest.mark.parametrize("w,h,bits,comps,ilv,lines,cls,base", [(150, 10, 8, 1, 0, 4, "r16", 0), (7, 5, 8, 3, 1, 2, "p13", 1), (16, 7, 16, 1, 0, 3, "p2", 2),
                                                               (257, 3, 8, 3, 2, 1, "big", 8), (1, 4, 16, 1, 0, 2, "p1", 1), (16, 6, 8, 1, 0, 5, "r16p16", 0)])
def test_decode_interval_descriptors_follow_the_stride(w, h, bits, comps, ilv, lines, cls, base):
    L = emu_bind.lib()
    g = G(w, h, bits, comps, ilv)
    lay = S.layout(g, cls, base, 2)
    arena, keep = lay.blank(), []
    n = (h + lines - 1) // lines
    body = np.zeros(64 * n + 64, dtype=np.uint8)
    marks = np.array([64 * (j + 1) - 2 for j in range(n - 1)] * 2, dtype=np.uint32)
    parents = (emu_bind.ScanDesc * 2)(*[emu_bind.make_desc(w, h, comps, ilv, bits, 0, 0, (0, 3, 7, 21, 64), lines, arena[lay.row_offset(f, 0):], lay.stride,
                                                           body, keep) for f in range(2)])
    subs = (emu_bind.ScanDesc * (2 * n))()
    L.emu_build_decode_intervals(parents, marks.ctypes.data_as(C.c_void_p), C.c_uint32(n), subs, 2)
    for f in range(2):
        for j in range(n):
            s = subs[f * n + j]
            assert s.pixels - arena.ctypes.data == lay.row_offset(f, j * lines), (f, j)
            assert (s.pixel_stride, s.height, s.width, s.restart_interval) == (lay.stride, min(lines, h - j * lines), w, 0), (f, j)


@pytest.mark.parametrize("w,h,bits,comps,ilv,lines,cls,base,tight", [(150, 8, 8, 1, 0, 3, "r16", 0, False), (17, 4, 8, 1, 0, 1, "p1", 1, True),
                                                                     (16, 5, 8, 3, 2, 2, "p13", 2, False), (7, 6, 8, 3, 1, 4, "r16p16", 8, True),
                                                                     (150, 5, 16, 1, 0, 2, "p2", 2, False), (257, 3, 8, 1, 0, 2, "big", 0, False)])
def test_restart_interval_encode_reads_padded_rows(w, h, bits, comps, ilv, lines, cls, base, tight):
    """build_encode_intervals + the pipeline on the intervals + the join (encode_launch.hip: launch_encode_intervals): the joined
    scan is the oracle's coding of every interval of the PACKED image with FF D0+m between them."""
    import oracle_bind as ob
    L = emu_bind.lib()
    g = G(w, h, bits, comps, ilv)
    lay = S.layout(g, cls, base, 1, "even", tight)
    img = S.mixed(g, seed=w + h)
    want, n = b"", (h + lines - 1) // lines
    for j in range(n):
        sub = np.ascontiguousarray(img[j * lines:(j + 1) * lines])
        s = ob.encode(sub, width=w, height=sub.shape[0], bits_per_sample=bits, component_count=comps, interleave_mode=ilv)
        sc = jls_container.parse(s).scans[0]
        want += s[sc.data_start:sc.data_end] + (bytes([0xFF, 0xD0 + (j & 7)]) if j + 1 < n else b"")
    arena, keep = lay.pad([img]), []
    before = arena.copy()
    out = np.zeros(len(want) + 100, dtype=np.uint8)
    d = emu_bind.make_desc(w, h, comps, ilv, bits, 0, 0, jls_container.validated_pc((0,) * 5, bits, 0), lines, arena[lay.first:], lay.stride, out, keep)
    res = _results(1)
    L.emu_encode_with_restart_intervals(C.byref(d), res, 1, C.c_uint64(g.row * lines * 4 + 256))
    assert (res[0].errc, res[0].flags, res[0].bytes) == (0, 0, len(want))
    assert out[:len(want)].tobytes() == want
    assert np.array_equal(arena, before), "the encoder wrote to its source"


# ---- scan_seek_decode.hip: the emit and resume kernels index rows by y * pixel_stride ----------------------------------------

@pytest.mark.parametrize("w,h,bits,comps,ilv,near,K,cls,base,tight", [(150, 9, 8, 1, 0, 0, 4, "r16", 0, False), (7, 7, 8, 3, 2, 2, 3, "p1", 1, True),
                                                                      (16, 13, 8, 3, 1, 0, 6, "r16p16", 8, False), (257, 5, 8, 1, 0, 0, 1, "p13", 2, True),
                                                                      (33, 7, 16, 1, 0, 0, 3, "p2", 2, False), (1, 6, 12, 2, 2, 0, 4, "big", 0, False)])
def test_seek_emit_and_resume_rows(w, h, bits, comps, ilv, near, K, cls, base, tight):
    import test_emu_seek_index as seek
    L = seek.lib()
    g = G(w, h, bits, comps, ilv)
    lay = S.layout(g, cls, base, 1, "even", tight)
    fr = S.Coded(g, seed=w + K, near=near)
    cont = jls_container.parse(fr.jls)
    pc = jls_container.validated_pc(cont.pc, bits, near)
    planes = 1 if ilv == 0 else comps
    pb = L.emu_seek_point_bytes(w, planes, int(bits > 8))

    def desc(arena, keep):
        return (emu_bind.ScanDesc * 1)(emu_bind.make_desc(w, h, comps, ilv, bits, near, 0, pc, 0, arena[lay.first:], lay.stride,
                                                          _stream_copy(fr.jls, cont.scans[0].data_start), keep))

    arena, keep = lay.blank(), []
    points = np.zeros(max(1, (h - 1) // K) * pb, dtype=np.uint8)
    res = _results(1)
    L.emu_seek_emit(desc(arena, keep), res, points.ctypes.data_as(C.c_void_p), K)
    assert res[0].errc == 0 and res[0].bytes == cont.scans[0].data_end - cont.scans[0].data_start
    lay.check(arena, [fr.pixels], what="emit")
    n = (h - 1) // K + 1
    work = (seek.SeekWork * n)()
    for i in range(n):
        last = i + 1 == n
        work[i] = seek.SeekWork(0, i * K, min(h, (i + 1) * K), i * K, seek.END if last else seek.COMPARE, 0, (i - 1) * pb if i else 0,
                                0 if last else i * pb)
    arena, keep = lay.blank(), []
    res = _results(n)
    L.emu_seek_resume(desc(arena, keep), work, res, n, points.ctypes.data_as(C.c_void_p))
    for i in range(n - 1):
        assert res[i].errc == 0 and res[i].flags & seek.CHECKED and not res[i].flags & seek.MISMATCH, i
    assert res[n - 1].errc == 0
    lay.check(arena, [fr.pixels], what="resume")


# ---- the encoders: scan_serial.hip, scan_group_encode.hip, the tile pipeline ----------------------------------------------------

def _encode(launch, g, cls, base, *, count=2, pitch="pad", tight=False, near=0, ct=0, seed=1):
    """`count` frames of one arena per launch (planar frames: a scan per plane): every scan's bytes are the oracle's of the
    PACKED image, the arena is unchanged."""
    lay = S.layout(g, cls, base, count, pitch, tight)
    frames = [S.Coded(g, seed + 17 * f, near=near, ct=ct) for f in range(count)]
    arena, keep = lay.pad([fr.img for fr in frames]), []
    before = arena.copy()
    descs, wants, outs = [], [], []
    for f, fr in enumerate(frames):
        cont = jls_container.parse(fr.jls)
        pc = jls_container.validated_pc(cont.pc, cont.bits, near)
        for c, scan in enumerate(cont.scans):
            wants.append(fr.jls[scan.data_start:scan.data_end])
            outs.append(np.zeros(len(wants[-1]) + 64, dtype=np.uint8))
            descs.append(emu_bind.make_desc(g.width, g.height, scan.components, scan.ilv, g.bits, near, ct, pc, 0,
                                            arena[lay.row_offset(f, c * g.height):], lay.stride, outs[-1], keep))
    n = len(descs)
    res = _results(n)
    launch((emu_bind.ScanDesc * n)(*descs), res, n)
    for k in range(n):
        assert res[k].errc == 0 and outs[k][:res[k].bytes].tobytes() == wants[k], (k, res[k].errc, res[k].flags)
    assert np.array_equal(arena, before), "the encoder wrote to its source"


@pytest.mark.parametrize("w,h,bits,comps,ilv,near,ct,cls,base,tight", [
    (150, 3, 8, 1, 0, 0, 0, "r16", 0, False), (257, 2, 8, 3, 0, 2, 0, "p1", 1, True), (16, 3, 8, 3, 1, 0, 1, "r16p16", 8, False),
    (7, 2, 8, 3, 2, 3, 0, "p13", 2, True), (1, 4, 8, 4, 2, 0, 0, "p2", 1, False), (150, 1, 8, 2, 1, 0, 0, "big", 0, False),
    (150, 3, 16, 1, 0, 0, 0, "p1", 0, True), (7, 2, 12, 3, 0, 2, 0, "p13", 1, False), (16, 2, 16, 3, 2, 0, 2, "p2", 2, False)])
def test_serial_encoder_reads_padded_rows(w, h, bits, comps, ilv, near, ct, cls, base, tight):
    _encode(lambda arr, res, n: emu_bind.lib().emu_encode_scans_serial(arr, res, n), G(w, h, bits, comps, ilv), cls, base,
            pitch="pad" if bits <= 8 or cls in ("p1", "p13") else "even", tight=tight, near=near, ct=ct, seed=w + comps)


@pytest.mark.parametrize("group,w,h,bits,comps,ilv,near,ct,cls,base,tight", [
    (8, 150, 3, 8, 1, 0, 2, 0, "r16", 0, False), (16, 257, 2, 8, 3, 2, 3, 0, "p1", 1, True), (32, 16, 3, 8, 3, 1, 2, 0, "r16p16", 8, False),
    (64, 7, 2, 8, 4, 2, 1, 0, "p13", 2, True), (8, 1, 4, 8, 2, 1, 2, 0, "p2", 1, False), (16, 150, 2, 8, 3, 2, 0, 1, "big", 0, False),
    (32, 150, 3, 16, 1, 0, 3, 0, "r16", 0, True), (8, 7, 2, 12, 3, 2, 2, 0, "p2", 2, False), (16, 16, 2, 16, 3, 1, 5, 0, "r16p16", 8, False)])
def test_group_encoder_reads_padded_rows(group, w, h, bits, comps, ilv, near, ct, cls, base, tight):
    _encode(lambda arr, res, n: _zero(emu_bind.lib().emu_encode_pixels_group(arr, res, n, group)), G(w, h, bits, comps, ilv), cls, base,
            count=3, pitch="even", tight=tight, near=near, ct=ct, seed=w + comps)


def _tile(arr, res, n):
    emu_bind.tile_lib().emu_encode_tile_pipeline(arr, res, n, 64, 32, 8, 8, 24)


@pytest.mark.parametrize("w,h,bits,comps,ilv,ct,cls,base,tile,pixel,tight", [
    (150, 5, 8, 1, 0, 0, "r16", 0, None, 0, False), (257, 3, 8, 1, 0, 0, "p1", 1, 64, 0, True),       # lines cut into segments of 64 samples
    (150, 4, 8, 3, 0, 0, "p13", 2, 128, 0, False), (16, 5, 8, 1, 0, 0, "r16p16", 8, None, 0, False),
    (7, 2, 8, 1, 0, 0, "p2", 1, None, 0, True), (1, 3, 8, 1, 0, 0, "big", 0, None, 0, False),
    (150, 3, 16, 1, 0, 0, "r16", 0, 64, 0, False), (257, 2, 12, 1, 0, 0, "p2", 2, 192, 0, True),
    # pixel mode: source rows read as 4-byte words from a lead that changes from row to row with stride R + 1
    (150, 5, 8, 1, 0, 0, "p1", 0, None, 1, False), (150, 4, 8, 3, 2, 1, "p1", 1, 64, 0, True), (257, 3, 8, 3, 2, 0, "r16", 0, 128, 0, False),
    (16, 4, 8, 4, 2, 0, "p13", 2, None, 0, False), (7, 3, 8, 2, 2, 0, "p2", 8, None, 0, True), (150, 3, 8, 3, 1, 2, "p13", 1, 64, 0, False),
    (257, 2, 8, 3, 1, 0, "r16p16", 8, None, 1, False), (150, 3, 16, 3, 2, 0, "p2", 2, 64, 0, True), (1, 2, 8, 3, 2, 0, "big", 1, None, 0, False),
    (257, 4, 8, 1, 0, 0, "p13", 2, 64, 1, False), (150, 2, 16, 3, 1, 3, "r16p16", 0, 128, 0, False)])
def test_tile_pipeline_reads_padded_rows(monkeypatch, w, h, bits, comps, ilv, ct, cls, base, tile, pixel, tight):
    """The tile pipeline, regular (single-component lines that fit a tile) and pixel mode (sample- and line-interleaved scans,
    lines cut into segment tiles by TILE_SAMPLES, PIXEL_MODE = 1)."""
    if tile:
        monkeypatch.setenv("CHARLS_AMD_TILE_SAMPLES", str(tile))
    if pixel:
        monkeypatch.setenv("CHARLS_AMD_PIXEL_MODE", "1")
    _encode(_tile, G(w, h, bits, comps, ilv), cls, base, count=2, pitch="even", tight=tight, ct=ct, seed=w + comps)
