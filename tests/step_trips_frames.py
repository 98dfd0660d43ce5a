"""Frames for the step loop of scan_group_decode.hip as a loop of TRIPS (tests/test_emu_step_trips.py on the CPU harness,
tests/test_gpu_step_trips.py on the MI355X): a call's count is a count of trips of two steps, lm and pp advance once per trip,
and in 8-bit containers the MED predictor is taken relative to Ra.  Every generator asserts in numpy that its frames have the
property they are made for.  A case is a list of `Frame`s of ONE geometry that decode in one launch.  Test infrastructure."""
from dataclasses import dataclass, field

import numpy as np

import oracle_bind as ob

GROUPS = (8, 16, 32)   # lanes per scan
RUN_LENGTHS = sorted({n for g in GROUPS for n in (0, 1, g - 1, g, g + 1)})


@dataclass
class Frame:
    img: np.ndarray
    bits: int = 8
    near: int = 0
    preset: tuple = None
    jls: bytes = field(default=None, repr=False)
    pixels: bytes = field(default=None, repr=False)

    def code(self):
        """The oracle's stream of the frame and the oracle's pixels of that stream."""
        if self.jls is None:
            h, w = self.img.shape
            self.jls = ob.encode(self.img, width=w, height=h, bits_per_sample=self.bits, near_lossless=self.near, preset=self.preset)
            self.pixels = ob.decode(self.jls)[1].tobytes()
        return self


def noise(w, h, seed, bits=8, low=None, span=None):
    """Independent samples: regular mode everywhere (four equal neighbours are an accident), codes of a few bits."""
    top = 1 << bits
    low = top * 3 // 8 if low is None else low
    span = top // 4 if span is None else span
    r = np.random.default_rng(seed)
    return (low + r.integers(0, span, size=(h, w))).astype(np.uint8 if bits <= 8 else np.uint16)


def is_run_start(img, y, c):
    """Ra = Rb = Rc = Rd at sample (y, c), y >= 1, 1 <= c: the lossless condition of run mode."""
    w = img.shape[1]
    ra, rb, rc, rd = img[y, c - 1], img[y - 1, c], img[y - 1, c - 1], img[y - 1, min(c + 1, w - 1)]
    return ra == rb == rc == rd


def has_run(img, y, c, length):
    v = img[y, c - 1]
    return bool(is_run_start(img, y, c) and (img[y, c:c + length] == v).all() and img[y, c + length] != v)


def put_run(img, y, c, length, step=50, bits=8):
    """A run event whose first sample is (y, c): `length` samples equal to Ra, then the interruption sample.  It changes three
    samples of the line above, so events go on every other line."""
    w = img.shape[1]
    assert y >= 1 and c >= 1 and c + length < w
    v = img[y, c - 1]
    img[y - 1, c - 1:min(c + 2, w)] = v
    img[y, c:c + length] = v
    img[y, c + length] = (int(v) + step) % (1 << bits)
    assert has_run(img, y, c, length)


def widths():
    """Widths 1 - 9, 62 - 66, 125 - 130 and 257, three lines each, four frames per width: a call's count meets every remainder
    at both copies of the trip, and the last sample of a line is met alone (a line of 64 = 63 + 1 samples, of 127 = 63 + 63 + 1)."""
    out = {}
    for w in [*range(1, 10), *range(62, 67), *range(125, 131), 257]:
        frames = [Frame(noise(w, 3, 1000 + 4 * w + f)) for f in range(4)]
        assert all(f.img.shape == (3, w) for f in frames)
        out[f"w{w}"] = frames
    return out


def runs_in_every_copy():
    """Run events of the lengths 0, 1, G - 1, G, G + 1 (G = 8, 16, 32) with their first sample in columns 1 - 8: eight frames, frame
    f has the event of line y in column 1 + (f + y) % 8, so that every length meets every column, hence both copies of a trip."""
    w, frames = 48, []
    for f in range(8):
        img = noise(w, 2 * len(RUN_LENGTHS) + 1, 2000 + f)
        for k, n in enumerate(RUN_LENGTHS):
            put_run(img, 2 * k + 2, 1 + (f + k) % 8, n)
        assert all(has_run(img, 2 * k + 2, 1 + (f + k) % 8, n) for k, n in enumerate(RUN_LENGTHS))
        frames.append(Frame(img))
    return {"runs_cols_1_8": frames}


def runs_near_the_end():
    """Run events (lengths 0, 1, 3) whose interruption sample leaves the served scan 0 - 5 samples of its CALL -- a call takes the
    samples 1 - 63 of an undisturbed line: the interruption sample is sample 63 - r -- and 0 - 5 samples of its LINE (a line
    of 40 samples: the interruption sample is sample 40 - r)."""
    out = {}
    for name, w, last in (("call_end", 100, 63), ("line_end", 40, 40)):
        frames = []
        for f, n in enumerate((0, 1, 3)):
            img = noise(w, 13, 3000 + 10 * w + f)
            for r in range(6):
                c = last - r - 1 - n   # 0-based column of the event's first sample: sample `last - r` is the interruption sample
                put_run(img, 2 * r + 2, c, n)
            for r in range(6):
                c = last - r - 1 - n
                assert has_run(img, 2 * r + 2, c, n) and c + n + 1 == last - r and (name != "line_end" or w - (c + n + 1) == r)
            frames.append(Frame(img))
        out[f"runs_{name}"] = frames
    return out


def halvings():
    """RESET = 3 and RESET = 4 beside the default RESET (64) in one wavefront: A.12's halving every third / fourth sample of a
    context lands in both copies of a trip.  Few contexts (a small gradient alphabet), so that each is met often."""
    frames = []
    for f, reset in enumerate((3, 0, 4, 0, 3, 4, 0, 3)):
        r = np.random.default_rng(4000 + f)
        img = (120 + r.integers(0, 4, size=(6, 70))).astype(np.uint8)
        assert img.size >= 400   # (a gradient alphabet of -3 .. 3 has few contexts: each is halved many times)
        frames.append(Frame(img, preset=(0, 0, 0, 0, reset) if reset else None))
    assert {f.preset[4] for f in frames if f.preset} == {3, 4} and any(f.preset is None for f in frames)
    return {"reset_3_4_64": frames}


def narrow_blocks():
    """8-bit containers: MAXVAL 255 (the step leaves its sample unmasked) and MAXVAL 127 (it keeps the mask), one launch each,
    and both in one launch -- 32 frames of the one behind 32 of the other: 32 scans are a whole number of workgroups for 8, 16
    and 32 lanes per scan and one or four wavefronts per workgroup, and a workgroup shares one sample precision."""
    w, h = 33, 3
    eight = [Frame(noise(w, h, 5000 + f, bits=8, low=0, span=256)) for f in range(32)]
    seven = [Frame(noise(w, h, 5100 + f, bits=7, low=0, span=128), bits=7) for f in range(32)]
    assert max(int(f.img.max()) for f in eight) > 127 and max(int(f.img.max()) for f in seven) <= 127
    return {"maxval_255": eight[:8], "maxval_127": seven[:8], "maxval_255_and_127": eight + seven}


def wraps(near=0, w=40, h=4):
    """Ramps of +200 and -200 per sample (mod 256): Px + Errval leaves 0 .. 255 on both sides, so the unmasked sample is really
    out of range."""
    frames = []
    for f, step in enumerate((200, -200, 200, -200)):
        c, y = np.meshgrid(np.arange(w), np.arange(h))
        img = ((c * step + y * 7 + 3 * f + noise(w, h, 6000 + f, low=0, span=3)) % 256).astype(np.uint8)
        d = np.diff(img.astype(np.int32), axis=1)
        assert ((d > 128).any(), (d < -128).any()) == (step > 0, step < 0)   # (steps of 200 up, wrapped: 56 down -- and the mirror)
        frames.append(Frame(img, near=near))
    return frames


def other_renderings():
    out = {}
    for near in (1, 3):
        frames = [Frame(noise(70, 7, 7000 + 10 * near + f, low=0, span=256), near=near) for f in range(3)]
        img = noise(70, 7, 7090 + near)
        for y, n in ((2, 0), (4, 5), (6, 1)):
            put_run(img, y, 3 + y, n)
        out[f"near{near}_8bit"] = frames + [Frame(img, near=near)] + wraps(near, 70, 7)[:2]
    for bits in (12, 16):
        for near in (0, 2):
            frames = [Frame(noise(70, 7, 8000 + bits + near + f, bits=bits), bits=bits, near=near) for f in range(3)]
            img = noise(70, 7, 8090 + bits + near, bits=bits)
            for y, n in ((2, 0), (4, 5), (6, 1)):
                put_run(img, y, 3 + y, n, step=500, bits=bits)
            out[f"{bits}bit_near{near}"] = frames + [Frame(img, bits=bits, near=near)]
    return out


def all_cases():
    out = {}
    out.update(widths())
    out.update(runs_in_every_copy())
    out.update(runs_near_the_end())
    out.update(halvings())
    out.update(narrow_blocks())
    out["wraps"] = wraps()
    out.update(other_renderings())
    return out


# cases whose run events the step loop itself must serve (the emulator's path counter SERVED_IN_LOOP)
SERVED = ("runs_cols_1_8", "runs_call_end", "runs_line_end")
