"""The corner corpus: small, deterministic frames that drive the JPEG-LS model into its rare states -- C and B on their
clamps, escape codes, RUNindex 31, contexts halved at N = RESET, the largest NEAR and k, samples wrapped by RANGE.

Which states a frame reaches is what the oracle's census says (oracle/jls_oracle.h, enum jls_census);
tests/test_corner_census_cpu.py holds the corpus to floors on it.  The generators use integer numpy and the integer hash
of charls_amd.synth only, so a frame is the same bytes wherever the suite runs.  Nothing here comes from the code under
test.

`h` = 2^(bits-1), `m` = MAXVAL = 2^bits - 1.  A "tile" is a small block repeated over the frame."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import oracle_bind as ob
from charls_amd import synth

W, H = 48, 64          # the small frames: 3072 samples
LONG = 32768           # a line of 2^15 samples: one run block at RUNindex 31


@dataclass(frozen=True)
class Corner:
    name: str
    img: np.ndarray = field(repr=False, compare=False)   # the user's layout: (H, W), (C, H, W) planar or (H, W, C)
    bits: int = 8
    near: int = 0
    preset: tuple | None = None
    comps: int = 1
    ilv: int = 0
    ct: int = 0

    @property
    def width(self):
        return self.img.shape[-1] if (self.comps == 1 or self.ilv == 0) else self.img.shape[1]

    @property
    def height(self):
        return self.img.shape[-2] if (self.comps == 1 or self.ilv == 0) else self.img.shape[0]

    @property
    def klass(self):
        """The sample-width class the census floors are kept for."""
        return "8" if self.bits <= 8 else ("9-12" if self.bits <= 12 else "13-16")

    @property
    def long(self):
        return self.width >= LONG // 2

    def kw(self):
        return dict(width=self.width, height=self.height, bits_per_sample=self.bits, component_count=self.comps,
                    near_lossless=self.near, interleave_mode=self.ilv, color_transformation=self.ct, preset=self.preset)

    def params(self):
        """What tests/golden/corners.json records of the coding parameters."""
        return dict(self.kw(), preset=list(self.preset) if self.preset else None)


def dtype(bits):
    return np.uint8 if bits <= 8 else np.uint16


def max_near(bits):
    """The largest legal NEAR: min(255, MAXVAL / 2)."""
    return min(255, ((1 << bits) - 1) // 2)


def tile(block, bits, w=W, h=H):
    b = np.asarray(block, dtype=np.int64)
    reps = (-(-h // b.shape[0]), -(-w // b.shape[1]))
    return np.tile(b, reps)[:h, :w].astype(dtype(bits))


def hash_noise(values, seed, bits, w=W, h=H):
    """Hash noise over the few given sample values."""
    y, x = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    v = np.asarray(values, dtype=np.int64)
    return v[synth._hash(np, x, y, seed) % len(v)].astype(dtype(bits))


def extremes(bits):
    m = (1 << bits) - 1
    return (0, 1, 2, m - 2, m - 1, m)


def long_zeros(bits, rows=4):
    return np.zeros((rows, LONG), dtype=dtype(bits))


def long_interrupted(bits):
    """Six lines of 2^15 zeros with the last column set: every line is one long run that a sample interrupts, so RUNindex
    climbs to 31 and stays near it.  From row 3 on a bright sample in mid-line interrupts at RUNindex 31, where the
    reduced limit LIMIT - J[RUNindex] - 1 is smallest: an escape code."""
    m = (1 << bits) - 1
    img = np.zeros((6, LONG), dtype=dtype(bits))
    img[:, LONG - 1] = m // 2
    img[3:, LONG // 2] = m
    return img


def half_long(bits):
    """Five lines of 2^14 zeros: the blocks of the first three raise RUNindex to 31 (RUNindex lives on from line to line);
    the last line ends in a set sample, a run interruption at RUNindex 31."""
    img = np.zeros((5, LONG // 2), dtype=dtype(bits))
    img[4, -1] = 1 << (bits - 1)
    return img


def sparse_escape_run(bits, small=1, w=W, h=H):
    """Zeros with a 1 in every fourth column: twelve run interruptions of error 0 or 1 a line keep the run contexts'
    A / N small.  Every sixth line one of them is 2^(bits-1) instead: an escape code under the reduced limit, at every
    sample width (the 3x3 tile of `escape_run` gets there at 8 bit only), and again on the line below."""
    img = np.zeros((h, w), dtype=dtype(bits))
    img[:, 2::4] = small   # (under NEAR: 2 NEAR + 1, the smallest step that still interrupts a run)
    img[5::6, 10] = 1 << (bits - 1)
    return img


def noise_tail(bits, w=W, h=H):
    """Eight columns of noise, then zeros: every line ends in a run that stops inside a block."""
    img = hash_noise(extremes(bits), 9, bits, w, h)
    img[:, 8:] = 0
    return img


def _plane(recipe, bits, seed=0):
    m, h = (1 << bits) - 1, 1 << (bits - 1)
    blocks = {
        "checker": [[0, m], [m, 0]],
        "c_low": [[h, 0], [0, h]],
        "c_high": [[m, h], [h, m]] if bits > 8 else [[m, h], [h, 0]],
        "escape_regular": [[m, 0, m], [h, m, 0], [0, m, h]],
        "escape_run": [[h, 0, m], [h, h, 0], [0, 0, 0]],
        "run_halved": [[0, 0], [0, h]],
    }
    if recipe == "noise":
        return hash_noise(extremes(bits), 1 + seed, bits)
    if recipe == "escape_run_sparse":
        return sparse_escape_run(bits)
    if recipe == "noise_tail":
        return noise_tail(bits)
    return tile(blocks[recipe], bits)


RECIPES = ("checker", "c_low", "c_high", "escape_regular", "escape_run", "run_halved", "escape_run_sparse", "noise_tail")


def _build():
    out = []

    def add(name, img, **kw):
        out.append(Corner(name, np.ascontiguousarray(img), **kw))

    for bits in (8, 12, 16):
        for r in RECIPES:
            add(f"{r}_{bits}", _plane(r, bits), bits=bits)
        add(f"checker_{bits}_near2", _plane("checker", bits), bits=bits, near=2)
        for near in (1, 3, max_near(bits)):
            add(f"noise_{bits}_near{near}", _plane("noise", bits), bits=bits, near=near)
        for reset in (3, 255):
            add(f"noise_{bits}_reset{reset}", _plane("noise", bits), bits=bits, preset=(0, 0, 0, 0, reset))
        # the escape and clamp tiles under NEAR: the clamps of Rx at 0 / MAXVAL after the RANGE * (2 NEAR + 1) wrap
        add(f"escape_regular_{bits}_near3", _plane("escape_regular", bits), bits=bits, near=3)
        add(f"c_low_{bits}_near1", _plane("c_low", bits), bits=bits, near=1)
    # NEAR = 100: T3 = 980 is the widest gradient table the group decoder holds for samples wider than 8 bits
    for bits in (12, 16):
        add(f"noise_{bits}_near100", _plane("noise", bits), bits=bits, near=100)
    # RESET = 256 is stored as 0 by the reference: N never halves, only the serial kernels hold such a scan
    add("noise_12_reset256", _plane("noise", 12), bits=12, preset=(0, 0, 0, 0, 256))
    add("escape_run_sparse_16_reset256", _plane("escape_run_sparse", 16), bits=16, preset=(0, 0, 0, 0, 256))
    # the quirk widths: RANGE, qbpp and LIMIT come from 2^bpp
    add("checker_2", _plane("checker", 2), bits=2)
    add("noise_2_near1", hash_noise((0, 1, 2, 3), 3, 2), bits=2, near=1)
    add("run_halved_2", _plane("run_halved", 2), bits=2)
    add("c_high_15", _plane("c_high", 15), bits=15)
    add("escape_run_15", _plane("escape_run", 15), bits=15)
    add("noise_15_near255", _plane("noise", 15), bits=15, near=255)
    add("noise_15_reset3", _plane("noise", 15), bits=15, preset=(0, 0, 0, 0, 3))
    # three DIFFERENT corner recipes as the planes of one frame
    for bits in (8, 12, 16):
        planes = [_plane("escape_regular", bits), _plane("c_low", bits), _plane("noise", bits, seed=5)]
        add(f"sample3_{bits}", np.stack(planes, axis=2), bits=bits, comps=3, ilv=2)
        add(f"line3_{bits}", np.stack(planes, axis=2), bits=bits, comps=3, ilv=1)
        add(f"planar3_{bits}", np.stack(planes, axis=0), bits=bits, comps=3, ilv=0)
        planes = [_plane("noise", bits, seed=2), _plane("escape_run", bits), _plane("c_high", bits)]
        add(f"sample3_{bits}_near3", np.stack(planes, axis=2), bits=bits, comps=3, ilv=2, near=3)
    for bits, cts in ((8, (1, 2, 3)), (16, (1, 2, 3))):
        planes = [_plane("checker", bits), _plane("noise", bits, seed=7), _plane("escape_regular", bits)]
        for ct in cts:
            add(f"line3_{bits}_hp{ct}", np.stack(planes, axis=2), bits=bits, comps=3, ilv=1, ct=ct)
        add(f"sample3_{bits}_hp1", np.stack(planes, axis=2), bits=bits, comps=3, ilv=2, ct=1)
    # runs in a sample-interleaved scan need every component flat at once: three planes with runs, lossless and NEAR = 1
    for bits in (8, 12, 16):
        planes = [_plane("run_halved", bits), _plane("escape_run_sparse", bits), _plane("noise_tail", bits)]
        for near in (0, 1):
            tag = f"_near{near}" if near else ""
            add(f"sample3_{bits}_runs{tag}", np.stack(planes, axis=2), bits=bits, comps=3, ilv=2, near=near)
            add(f"line3_{bits}_runs{tag}", np.stack(planes, axis=2), bits=bits, comps=3, ilv=1, near=near)
        # the run recipes and the C clamp from above under NEAR = 1: the near-lossless kernels' own run service
        for r in ("run_halved", "noise_tail", "c_high", "escape_run"):
            add(f"{r}_{bits}_near1", _plane(r, bits), bits=bits, near=1)
        add(f"escape_run_sparse_{bits}_near3", sparse_escape_run(bits, small=7), bits=bits, near=3)
    add("noise_8_near30", _plane("noise", 8), bits=8, near=30)   # C on both clamps in an 8-bit near-lossless scan
    # three equal planes of the run recipe: the run contexts of a sample-interleaved scan at the largest k
    for bits in (8, 12, 16):
        p = _plane("run_halved", bits)
        add(f"sample3_{bits}_run_k", np.stack([p, p, p], axis=2), bits=bits, comps=3, ilv=2)
    # lines of 2^14 samples wider than 8 bits: RUNindex reaches 31 on a line that still fits LDS, and is interrupted there
    for bits in (12, 16):
        add(f"half_long_{bits}", half_long(bits), bits=bits)
        add(f"half_long_{bits}_near1", half_long(bits), bits=bits, near=1)
    # lines of 2^15 samples
    for bits in (8, 12, 16):
        add(f"long_zeros_{bits}", long_zeros(bits), bits=bits)
    for bits in (8, 12, 16):
        add(f"long_zeros_{bits}_near1", long_zeros(bits), bits=bits, near=1)
    for bits in (8, 12, 16):
        add(f"long_interrupted_{bits}", long_interrupted(bits), bits=bits)
    return {c.name: c for c in out}


CORPUS = _build()
SMALL = {n: c for n, c in CORPUS.items() if not c.long}

_coded = {}


class CodedCorner:
    """A corner frame, the oracle's stream of it, the oracle's pixels of that stream and the census of both directions;
    computed once per frame and shared."""

    def __init__(self, c: Corner):
        self.corner, self.encode_census, self.decode_census = c, {}, {}
        size = 8 * c.img.nbytes + 4096
        self.jls = ob.encode(c.img, destination_size=size, census=self.encode_census, **c.kw())
        self.pixels = ob.decode(self.jls, census=self.decode_census)[1].tobytes()


def coded(name) -> CodedCorner:
    if name not in _coded:
        _coded[name] = CodedCorner(CORPUS[name])
    return _coded[name]


# ---- which frames go to which coding route -------------------------------------------------------------------------------
#
# What a route can take is what charls_amd/csrc/device/decode_launch.hip and encode_launch.hip say of it (wave_decode_eligible, fast_decode_eligible,
# pixel_group_lanes, pipeline_eligible); tests/test_gpu_corners.py sends every frame of ROUTES through its route,
# tests/test_emu_corners.py the frames of EMU_ROUTES (taken in turn where several kernels share them), and
# tests/test_corner_census_cpu.py asserts from the census that the frames of a route reach every corner that can occur on it.

def coding_parameters(c: Corner):
    """(MAXVAL, T1, T2, T3, RESET) as the scan is coded with."""
    import jls_container
    return jls_container.validated_pc(c.preset or (0, 0, 0, 0, 0), c.bits, c.near)


def _reset_byte(c):
    return coding_parameters(c)[4] & 0xFF   # the reference keeps RESET in a uint8: 256 becomes 0 and N never halves


def _line_in_lds(c):
    """wave_decode_lds() <= 64 KiB: 5008 bytes of contexts and bit ring, and (width + 2) samples per plane of the scan.  The
    2^15-sample lines of 8-bit samples and the 2^14-sample lines of wider ones fit, 2^15 wider samples do not."""
    planes = 1 if c.ilv == 0 else c.comps
    return 5008 + planes * (c.width + 2) * (2 if c.bits > 8 else 1) <= 64 * 1024


def _wave(c):
    return _reset_byte(c) != 0 and _line_in_lds(c)


def _table(c):
    """The group kernels' gradient table holds T3 <= 1023 for samples wider than 8 bits."""
    return c.bits <= 8 or coding_parameters(c)[3] <= 1023


ROUTES = {
    # decoders
    "group_decode": lambda c: _wave(c) and _table(c) and (c.comps == 1 or c.ilv in (0, 1)),
    "fast_decode": lambda c: _wave(c) and c.near == 0 and (c.comps == 1 or c.ilv == 0),
    "exact_decode": _wave,
    "serial_decode": lambda c: not _wave(c),
    "pixel_decode": lambda c: _wave(c) and _table(c) and (c.ilv == 2 or (c.near != 0 and c.ilv in (0, 1))),
    "seek_decode": _wave,
    # encoders
    "tile_encode": lambda c: c.near == 0,
    "group_encode": lambda c: c.near != 0 and _reset_byte(c) != 0,   # (its contexts keep N in 8 bits: RESET = 256 is the serial encoder's)
    "serial_encode": lambda c: True,
}


# The emulated kernels (tests/test_emu_corners.py) are called one by one, so a kernel also gets frames the product would send
# elsewhere: the serial kernels take every frame.  The lines of 2^14 and 2^15 samples go to the kernels whose emulation walks
# them in seconds.
EMU_ROUTES = {
    "group_decode": lambda c: ROUTES["group_decode"](c) and not c.long,
    "fast_decode": lambda c: ROUTES["fast_decode"](c) and not c.long,
    "exact_decode": lambda c: _wave(c) and not (c.long and c.near != 0),
    "serial_decode": lambda c: True,
    "pixel_decode": lambda c: ROUTES["pixel_decode"](c) and not c.long,
    "seek_decode": lambda c: _wave(c) and not c.long,
    "tile_encode": lambda c: c.near == 0 and not c.long,
    "group_encode": lambda c: ROUTES["group_encode"](c) and not c.long,
    "serial_encode": lambda c: True,
}


def route_frames(route, where="gpu", corpus=None):
    """The frames of a route on the MI355X ("gpu"), in the emulator ("emu") or in either ("any"); of `corpus` (another
    {name: Corner}, tests/stuffing.py) where one is given."""
    tables = {"gpu": (ROUTES,), "emu": (EMU_ROUTES,), "any": (ROUTES, EMU_ROUTES)}[where]
    return [n for n, c in (CORPUS if corpus is None else corpus).items() if any(t[route](c) for t in tables)]


def batches(names, by="geometry", corpus=None):
    """Frames that can share a launch, {key: [names]} in the corpus' order, which puts different recipes side by side:
    "geometry"   one geometry and sample width: a decode batch of the API;
    "thresholds" and NEAR, T1..T3 as well: the scans of a wavefront of the group kernels share the gradient table, a scan with
                 other thresholds is handed to the exact decoder (tests/test_emu_group_decode.py);
    "parameters" and every coding parameter: an encode batch of the API."""
    out = {}
    for n in names:
        c = (CORPUS if corpus is None else corpus)[n]
        key = (c.width, c.height, c.bits, c.comps, c.ilv)
        if by == "thresholds":
            key += (c.near,) + tuple(coding_parameters(c)[1:4])
        elif by == "parameters":
            key += (c.near, c.ct, c.preset)
        out.setdefault(key, []).append(n)
    return out


def batch_id(key):
    w, h, bits, comps, ilv = key[:5]
    s = f"{w}x{h}x{bits}b" + (f"-{comps}c-ilv{ilv}" if comps > 1 else "")
    if len(key) == 9:
        s += f"-near{key[5]}-t{key[6]}.{key[7]}.{key[8]}"
    elif len(key) == 8:
        near, ct, preset = key[5:]
        s += (f"-near{near}" if near else "") + (f"-hp{ct}" if ct else "") + (f"-reset{preset[4]}" if preset else "")
    return s
