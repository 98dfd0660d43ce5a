"""Padded rows for the tests of ScanDesc::pixel_stride (tests/test_emu_strides.py, tests/test_gpu_strides.py).

A batch of frames is laid out in a canary-filled uint8 arena the way charls_amd.h part 2 describes it: frame f at
`base + f * pitch`, `stride` bytes from row to row, a planar frame as one band of `stride * height` bytes per component.
The arena starts 16-byte aligned, has a guard band of GUARD bytes in front of the first and behind the last frame, and
(`tight`) can end in the smallest legal buffer: the last row of the last frame has no padding behind it, the guard band
follows at once.

Nothing here comes from the code under test: streams are the oracle's coding of the PACKED image, pixels the oracle's
decode of that stream, and numpy places them."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

import oracle_bind as ob
from charls_amd import synth

CANARY = 0xA5
GUARD = 256  # a multiple of 16: `base` is the offset from a 16-byte aligned address

INVALID_ARGUMENT_SIZE, INVALID_ARGUMENT_STRIDE = 110, 111

STRIDE_CLASSES = ("p1", "p2", "p13", "r16", "r16p16", "big")
BASES = (0, 1, 2, 8)
WIDTHS = (1, 7, 16, 150, 257)


@dataclass(frozen=True)
class Geometry:
    width: int
    height: int
    bits: int = 8
    comps: int = 1
    ilv: int = 0

    @property
    def bps(self):
        return (self.bits + 7) // 8

    @property
    def row(self):
        """R: the packed row length in bytes."""
        return self.width * self.bps * (self.comps if self.ilv != 0 else 1)

    @property
    def rows(self):
        """Rows of a frame in the user's layout: a planar frame has `height` rows per component."""
        return self.height * (self.comps if self.ilv == 0 else 1)

    @property
    def packed(self):
        return self.row * self.rows

    def kw(self):
        return dict(width=self.width, height=self.height, bits_per_sample=self.bits, component_count=self.comps,
                    interleave_mode=self.ilv)


def stride_of(row, cls):
    """The stride classes of the issue for a packed row of `row` bytes."""
    up = (row + 15) & ~15
    if cls == "r16":
        assert row % 16 != 0, "roundup(R, 16) is a stride of its own only where R % 16 != 0"
    return {"p1": row + 1, "p2": row + 2, "p13": row + 13, "r16": up, "r16p16": up + 16, "big": row + 4096}[cls]


def need(g: Geometry, stride):
    """The smallest frame the API accepts: no padding behind the last row."""
    return stride * g.rows - (stride - g.row)


def pitch_of(g: Geometry, stride, how):
    """`tight` = need; `pad` = some bytes more; `mod8` / `mod0` = the next pitch that is 8 / 0 modulo 16 (with base 0 and a
    stride that is a multiple of 16, mod8 makes every other frame start 16-byte aligned)."""
    n = need(g, stride)
    if how == "tight":
        return n
    if how == "pad":
        return n + 37
    if how == "even":
        return n + 38 + n % 2
    target = 8 if how == "mod8" else 0
    p = n + 16
    return p + (target - p) % 16


class Layout:
    def __init__(self, g: Geometry, stride, pitch, base, count, tight=False):
        assert stride >= g.row and pitch >= need(g, stride) and count >= 1
        self.g, self.stride, self.pitch, self.base, self.count, self.tight = g, stride, pitch, base, count, tight
        self.first = GUARD + base
        self.need = need(g, stride)
        self.size = self.first + (count - 1) * pitch + (self.need if tight else pitch) + GUARD

    def row_offset(self, f, r):
        return self.first + f * self.pitch + r * self.stride

    def blank(self, canary=CANARY):
        """A canary-filled arena whose first byte is 16-byte aligned."""
        raw = np.full(self.size + 64, canary, dtype=np.uint8)
        skew = (-raw.ctypes.data) % 64
        arena = raw[skew:skew + self.size]
        assert arena.ctypes.data % 16 == 0
        return arena

    def pad(self, frames, canary=CANARY):
        g = self.g
        assert len(frames) == self.count
        arena = self.blank(canary)
        for f, img in enumerate(frames):
            raw = np.frombuffer(img.tobytes() if isinstance(img, np.ndarray) else bytes(img), dtype=np.uint8)
            assert raw.size == g.packed, (raw.size, g.packed)
            for r in range(g.rows):
                at = self.row_offset(f, r)
                arena[at:at + g.row] = raw[r * g.row:(r + 1) * g.row]
        return arena

    def where(self, index):
        """What byte `index` of the arena is, in words."""
        g = self.g
        if index < self.first:
            return f"the guard band in front of frame 0 ({self.first - index} bytes before it)"
        rel = index - self.first
        f = min(rel // self.pitch, self.count - 1)
        within = rel - f * self.pitch
        if within >= self.need:
            what = "the guard band" if f == self.count - 1 and (self.tight or within >= self.pitch) else "the bytes up to the pitch"
            return f"{what} behind frame {f}, {within - self.need} bytes behind its last row"
        r, col = divmod(within, self.stride)
        band = f"component {r // g.height} line {r % g.height}" if g.ilv == 0 and g.comps > 1 else f"line {r}"
        if col < g.row:
            return f"frame {f} row {r} ({band}) byte {col} of {g.row}"
        return f"the gap behind frame {f} row {r} ({band}), {col - g.row} bytes behind the row"

    def check(self, arena, frames, canary=CANARY, what="decoded"):
        """Every row holds exactly the bytes of `frames`, every other byte of the arena still holds the canary."""
        want = self.pad(frames, canary)
        got = np.asarray(arena, dtype=np.uint8).reshape(-1)
        assert got.size == want.size, (got.size, want.size)
        bad = np.flatnonzero(got != want)
        if bad.size:
            i = int(bad[0])
            raise AssertionError(f"{what}: {bad.size} wrong bytes, the first at arena offset {i} = {self.where(i)}: "
                                 f"got {int(got[i]):#04x}, want {int(want[i]):#04x} "
                                 f"(stride {self.stride}, pitch {self.pitch}, base {self.base}, row {self.g.row}, {self.g})")


def layout(g: Geometry, cls, base, count, pitch="pad", tight=False):
    stride = stride_of(g.row, cls) if isinstance(cls, str) else int(cls)
    return Layout(g, stride, pitch_of(g, stride, pitch) if isinstance(pitch, str) else int(pitch), base, count, tight)


def pad(frames, g, stride, pitch, base, canary=CANARY, tight=False):
    return Layout(g, stride, pitch, base, len(frames), tight).pad(frames, canary)


def check(arena, frames, g, stride, pitch, base, canary=CANARY, tight=False):
    Layout(g, stride, pitch, base, len(frames), tight).check(arena, frames, canary)


def mixed(g: Geometry, seed, kind="mixed"):
    """A frame in the user's layout with a run to the end of a line and one that is interrupted in the last samples of a line
    (tests/test_gpu_pixel_mode.py), in every component at once: row stores follow run service and regular steps."""
    w, h = g.width, g.height
    img = synth.frame_numpy(w, h, seed=seed, bits=g.bits, components=g.comps, kind=kind, interleaved=True)
    img = img.reshape(h, w, g.comps).copy()
    y = h // 2
    img[y, w // 3:, :] = img[y, w // 3, :]
    if w > 4:
        img[h - 1, 1:w - 2, :] = img[h - 1, 1, :]
    if g.comps == 1:
        return np.ascontiguousarray(img[:, :, 0])
    return np.ascontiguousarray(np.moveaxis(img, 2, 0)) if g.ilv == 0 else img


class Coded:
    """A packed frame, the oracle's stream of it and the oracle's pixels of that stream."""

    def __init__(self, g: Geometry, seed, *, near=0, ct=0, preset=None, kind="mixed", restart=0, product=None, img=None):
        """`img`: given pixels in the user's layout (tests/corners.py) instead of the frame `seed` and `kind` make."""
        self.g, self.img = g, mixed(g, seed, kind) if img is None else np.ascontiguousarray(img)
        assert self.img.nbytes == g.packed, (self.img.nbytes, g.packed)
        kw = dict(near_lossless=near, color_transformation=ct, preset=preset, destination_size=8 * g.packed + 4096, **g.kw())
        # a stream with restart markers is the product encoder's extension (the reference cannot write one): written from
        # the PACKED image, and what it holds is what the oracle decodes from it
        self.jls = product.encode(self.img, restart_interval=restart, **kw) if restart else ob.encode(self.img, **kw)
        self.pixels = ob.decode(self.jls)[1].tobytes()
        self.near, self.ct, self.preset = near, ct, preset


# ---- charls_amd.h part 2 on a device arena (GPU tests only) -------------------------------------------------------------

def bind(lib):
    from charls_amd import batch
    return batch._bind(lib)


def codec_params(g: Geometry, near=0, ct=0, preset=None, restart=0):
    from charls_amd import batch, capi
    return batch.CodecParams(capi.FrameInfo(g.width, g.height, g.bits, g.comps), near, g.ilv, ct,
                             capi.PcParameters(*(preset or (0, 0, 0, 0, 0))), 0, restart)


def decode_batch(torch, lib, jls_list, lay: Layout, canary=CANARY):
    """charls_amd_decode_batch_device into a canary-filled device arena: (rc, errcs, the arena back on the host)."""
    from charls_amd import batch
    l = bind(lib)
    n = len(jls_list)
    spitch = (max(len(j) for j in jls_list) + 255) & ~255
    host = np.zeros((n, spitch), dtype=np.uint8)
    for i, j in enumerate(jls_list):
        host[i, :len(j)] = np.frombuffer(j, dtype=np.uint8)
    streams = torch.from_numpy(host).cuda()
    sizes = np.array([len(j) for j in jls_list], dtype=np.uint64)
    arena = torch.full((lay.size,), canary, dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 16 == 0
    errcs = np.full(n, -1, dtype=np.int32)
    p = batch.CodecParams()
    rc = l.charls_amd_decode_batch_device(n, streams.data_ptr(), spitch, sizes.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          arena.data_ptr() + lay.first, lay.pitch, lay.stride, C.byref(p),
                                          errcs.ctypes.data_as(C.POINTER(C.c_int32)), None)
    torch.cuda.synchronize()
    return rc, errcs, arena.cpu().numpy()


def encode_batch(torch, lib, arena_host, lay: Layout, params, stream_pitch=None):
    """charls_amd_encode_batch_device from a device copy of `arena_host`: (rc, errcs, list of streams, the arena afterwards)."""
    l = bind(lib)
    g, n = lay.g, lay.count
    arena = torch.from_numpy(np.ascontiguousarray(arena_host)).cuda()
    assert arena.data_ptr() % 16 == 0
    spitch = stream_pitch or ((8 * g.packed + 4096 + 255) & ~255)
    streams = torch.zeros((n, spitch), dtype=torch.uint8, device="cuda")
    sizes = np.zeros(n, dtype=np.uint64)
    errcs = np.full(n, -1, dtype=np.int32)
    rc = l.charls_amd_encode_batch_device(C.byref(params), n, arena.data_ptr() + lay.first, lay.pitch, lay.stride,
                                          streams.data_ptr(), spitch, sizes.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          errcs.ctypes.data_as(C.POINTER(C.c_int32)), None)
    torch.cuda.synchronize()
    out = streams.cpu().numpy()
    return rc, errcs, [out[i, :int(sizes[i])].tobytes() for i in range(n)], arena.cpu().numpy()
