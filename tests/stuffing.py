"""The stuffing corpus: small, deterministic frames whose JPEG-LS streams are dense in 0xFF bytes, for every reader and writer
of the 0xFF stuffing.

A stream coded from `synth` frames or natural images has a 0xFF in every 256 bytes; the streams here have one in every two to
four.  Three recipes (all are plain integer numpy; nothing comes from the code under test):

* ramp         every row is x * step.  After the first row every sample is predicted exactly in regular mode with k = 0: a
               single 1 bit.  The stream is FF 7F FF 7F ... (near-lossless: step is a multiple of 2 NEAR + 1);
* specks       n samples of a ramp XORed with a constant: zeros at every bit phase, 0xFF bytes at every byte position;
* tall flat    width 1 .. 16: once RUNindex outgrows the line every line costs exactly one bit.

Beside them stand the partners of each gray geometry, for mixing in one wavefront: `synth` noise (a long stream, sparse in 0xFF),
a `synth` gradient and a flat frame (a stream of a few bytes: this scan ends while its neighbours are in mid-stream).

What the streams reach is what `ff_census` says of the ORACLE's bytes; tests/test_stuffing_census_cpu.py holds the corpus to
floors on it.  The records are corners.Corner, the route tables corners.ROUTES / EMU_ROUTES."""
from __future__ import annotations

import numpy as np

import corners
import jls_container
import oracle_bind as ob
from charls_amd import synth
from corners import Corner, batch_id, dtype  # noqa: F401  (batch_id: for the tests that parametrise over batches)

MISALIGNMENTS = range(16)
CHUNKS = (128, 256, 512, 1024)   # G x 16 bytes of the group kernels' refill (G = 8, 16, 32) and DenseBits' 1024
# the route classes whose kernels un-stuff, each met at every misalignment (tests/test_emu_stuffing.py, tests/test_gpu_stuffing.py)
DECODE_CLASSES = ("group_decode", "fast_decode", "exact_decode", "pixel_decode", "serial_decode")
RESET256 = (0, 0, 0, 0, 256)


def ramp(w, h, bits, step):
    assert (w - 1) * step < (1 << bits)
    return np.tile(np.arange(w, dtype=np.int64) * step, (h, 1)).astype(dtype(bits))


def specked(img, n, xor, seed):
    """`n` samples below the first row, at hashed places, XORed with `xor`."""
    out = img.copy()
    h, w = img.shape
    k = np.arange(n, dtype=np.int64)
    x = synth._hash(np, k, k * 0 + 1, seed) % w
    y = 1 + synth._hash(np, k, k * 0 + 2, seed) % (h - 1)
    out[y, x] ^= xor
    return out


def flat(w, h, bits, value):
    return np.full((h, w), value, dtype=dtype(bits))


# The ramp geometries: key -> (width, height, bits, step, NEAR, XOR constant, the speck counts; None first: the pure ramp).
# A context starts with A = (RANGE + 32) / 64, k = 10 at 16 bit: the first row, and the few hundred samples each of the three
# contexts of a ramp (first column, last column, the rest) takes to bring k down to 0, cost 700 bytes before the one-bit samples
# start.  No 16-bit ramp of 200 x 200 has a 0xFF in 45 % of its bytes; one of 16 x 2400 has ("16t", "16tn": two columns are
# edges, but the first row is short).
GRAY = {
    "8": (128, 96, 8, 1, 0, 1, (None, 30, 100)),
    "12": (128, 160, 12, 30, 0, 1, (None, 20, 80)),
    "16": (128, 96, 16, 300, 0, 1, (30, 100)),
    "16t": (16, 2400, 16, 300, 0, 1, (None,)),
    "8n": (36, 160, 8, 5, 2, 16, (None, 30, 90)),
    "16n": (96, 128, 16, 500, 2, 16, (20, 60)),
}


def _build():
    out = []

    def add(name, img, **kw):
        out.append(Corner(name, np.ascontiguousarray(img), **kw))

    for key, (w, h, bits, step, near, xor, counts) in GRAY.items():
        r = ramp(w, h, bits, step)
        dense = [(f"ramp_{key}" + (f"_specks{n}" if n else ""), specked(r, n, xor, 7) if n else r) for n in counts]
        partners = [(f"noise_{key}", synth.frame_numpy(w, h, seed=41, bits=bits, kind="noise")),
                    (f"gradient_{key}", synth.frame_numpy(w, h, seed=42, bits=bits, kind="gradient")),
                    (f"flat_{key}", flat(w, h, bits, 3))]
        # the partners stand between the dense frames: in a batch of this order a wavefront of the group kernels holds both
        for i in range(3):
            for name, img in dense[i:i + 1] + partners[i:i + 1]:
                add(name, img, bits=bits, near=near)
        # RESET = 256 is stored as 0: N never halves, only the serial kernels hold such a scan (corners._wave).  It is legal
        # for samples wider than 8 bits only (RESET <= max(255, MAXVAL)): the 8-bit geometries have no such frame.
        if bits > 8:
            add(f"ramp_{key}_reset256", specked(r, 3, xor, 9), bits=bits, near=near, preset=RESET256)
    # the other NEARs, on the near-lossless geometries: a step of 2 NEAR + 1 (times a constant at 16 bit)
    add("ramp_8n_near1_specks30", specked(ramp(36, 160, 8, 3), 30, 16, 11), bits=8, near=1)
    add("ramp_8n_near3", ramp(36, 160, 8, 7), bits=8, near=3)
    add("ramp_16tn", ramp(16, 2400, 16, 500), bits=16, near=2)   # (their partners: the near-lossless ones of "16n")
    add("ramp_16tn_near1", ramp(16, 2400, 16, 300), bits=16, near=1)
    add("ramp_16n_near3_specks20", specked(ramp(96, 128, 16, 630), 20, 16, 12), bits=16, near=3)
    # colour: the same ramp in every component, specks of their own
    planes = [specked(ramp(64, 64, 8, 3), 10, 1, 20 + p) for p in range(3)]
    add("sample3_8_specks10", np.stack(planes, axis=2), comps=3, ilv=2)
    add("line3_8", np.stack([ramp(64, 64, 8, 3)] * 3, axis=2), comps=3, ilv=1)
    add("planar3_8_specks10", np.stack(planes, axis=0), comps=3, ilv=0)
    add("line3_8_near2_specks10", np.stack([specked(ramp(48, 64, 8, 5), 10, 16, 30 + p) for p in range(3)], axis=2), comps=3, ilv=1, near=2)
    add("sample3_16_specks10", np.stack([specked(ramp(64, 64, 16, 300), 10, 1, 40 + p) for p in range(3)], axis=2), bits=16, comps=3, ilv=2)
    # tall flat frames: 4096 lines, and about 600 for the seek points (a point is about 3 KB).  A line is a bit: the heights are
    # chosen for the last bytes -- 600 lines of width 1 end in FF 7F (a 0xFF, then 7 data bits), 597 of width 2 in 7F FE (the last
    # byte full, no padding bit), 595 of width 16 in FF 00 (a 0xFF, then padding alone)
    for h1, h2, h5, h16 in ((4096, 4096, 4096, 4096), (600, 597, 600, 595)):
        add(f"flat_1x{h1}_zeros", flat(1, h1, 8, 0))
        add(f"flat_2x{h2}_255", flat(2, h2, 8, 255))
        add(f"flat_5x{h5}_specks", specked(flat(5, h5, 8, 0), 3 * h5 // 40, 1, 52))
        add(f"flat_16x{h16}_near2", flat(16, h16, 8, 0), near=2)
    add("flat_1x600_zeros_reset256", flat(1, 600, 12, 0), bits=12, preset=RESET256)
    return {c.name: c for c in out}


CORPUS = _build()

PARTNER = ("noise_", "gradient_")


def is_partner(name):
    return name.startswith(PARTNER) or name in {f"flat_{k}" for k in GRAY}


def is_flat(name):
    return name.startswith("flat_") and not is_partner(name)


def is_specked(name):
    return "specks" in name


def is_pure(name):
    """A pure ramp or a pure flat frame."""
    return not is_partner(name) and not is_specked(name) and "reset256" not in name or name == "flat_1x600_zeros_reset256"


DENSE = [n for n in CORPUS if not is_partner(n)]
SEEK_FLAT = [n for n in CORPUS if is_flat(n) and CORPUS[n].height <= 600 and CORPUS[n].preset is None]

_coded = {}


class CodedFrame:
    """A frame, the oracle's stream of it, its entropy-coded segments (one per scan) and the oracle's pixels of that stream;
    computed once per frame and shared."""

    def __init__(self, c: Corner):
        self.corner = c
        self.jls = ob.encode(c.img, destination_size=8 * c.img.nbytes + 4096, **c.kw())
        self.pixels = ob.decode(self.jls)[1].tobytes()
        self.scans = jls_container.parse(self.jls).scans
        self.segments = [self.jls[s.data_start:s.data_end] for s in self.scans]


def coded(name) -> CodedFrame:
    if name not in _coded:
        _coded[name] = CodedFrame(CORPUS[name])
    return _coded[name]


def route_frames(route, where="gpu", dense=False):
    names = corners.route_frames(route, where, corpus=CORPUS)
    return [n for n in names if not dense or not is_partner(n)]


def batches(names, by="geometry"):
    return corners.batches(names, by, corpus=CORPUS)


# ---- restart intervals ------------------------------------------------------------------------------------------------------

RESTART_LINES = (7, 16)
# (A pure gray ramp would not do: every interval of it is the same image.  An interval of a 16-bit frame is over before k reaches
# 0: ramp_16_specks30 is here for the sample width, the FF xx endings are the others'.)
RESTART_FRAMES = ["ramp_8_specks30", "ramp_8_specks100", "ramp_8n_specks30", "ramp_8n_near1_specks30", "ramp_8n_near3", "line3_8",
                  "sample3_8_specks10", "ramp_16_specks30"]
RESTART_ENDINGS = [n for n in RESTART_FRAMES if n != "ramp_16_specks30"]   # the frames that are to supply the FF xx endings

_intervals = {}


def intervals(name, lines):
    """The oracle's coding of every interval of `lines` lines as an image of its own: what a restart-interval encoder has to
    write between its RSTm."""
    if (name, lines) not in _intervals:
        c, out = CORPUS[name], []
        for j in range((c.height + lines - 1) // lines):
            sub = np.ascontiguousarray(c.img[j * lines:(j + 1) * lines])
            s = ob.encode(sub, **dict(c.kw(), height=sub.shape[0]), destination_size=8 * sub.nbytes + 4096)
            sc = jls_container.parse(s).scans[0]
            out.append(s[sc.data_start:sc.data_end])
        _intervals[name, lines] = out
    return _intervals[name, lines]


def dri_scan(name, lines):
    """The entropy-coded segment with RSTm between the intervals, and the offset of every marker in it."""
    seg, at = b"", []
    parts = intervals(name, lines)
    for j, p in enumerate(parts):
        seg += p
        if j + 1 < len(parts):
            at.append(len(seg))
            seg += bytes([0xFF, 0xD0 + (j & 7)])
    return seg, at


def dri_stream(name, lines):
    """A whole JPEG-LS stream with that segment: the oracle's headers, a DRI segment in front of SOS."""
    cc = coded(name)
    assert len(cc.scans) == 1
    sos = cc.jls.rindex(b"\xff\xda", 0, cc.scans[0].data_start)
    seg, _ = dri_scan(name, lines)
    return cc.jls[:sos] + b"\xff\xdd\x00\x04" + lines.to_bytes(2, "big") + cc.jls[sos:cc.scans[0].data_start] + seg + cc.jls[cc.scans[0].data_end:]


_dri_pixels = {}


def dri_pixels(name, lines):
    """The oracle's pixels of dri_stream (near-lossless: every interval is reconstructed on its own, not as the whole frame is)."""
    if (name, lines) not in _dri_pixels:
        _dri_pixels[name, lines] = ob.decode(dri_stream(name, lines))[1].tobytes()
    return _dri_pixels[name, lines]


STRETCH = b"\xff\x7f\xff\x7f"


def stretch_near_middle(data: bytes, lo=0, hi=None):
    """The offset in [lo, hi - 4] of the FF 7F FF 7F that stands nearest the middle of data[lo:hi]; there must be one."""
    hi = len(data) if hi is None else hi
    middle = (lo + hi - 4) // 2
    found, at = [], data.find(STRETCH, lo, hi)
    while at >= 0:
        found.append(at)
        at = data.find(STRETCH, at + 1, hi)
    assert found, "no FF 7F FF 7F here"
    return min(found, key=lambda a: abs(a - middle))


def zero_in_stretch(built, j, scan=0):
    """tests/salvage_model.py's zero_bytes with the place chosen: four zero bytes over an FF 7F FF 7F of piece j, the one
    nearest its middle.  `built` is a salvage_model.Built; returns a damaged copy."""
    b = built.copy()
    piece = bytearray(b.scans[scan].pieces[j])
    at = stretch_near_middle(bytes(piece))
    assert 0 < at < len(piece) - 4
    piece[at:at + 4] = bytes(4)
    b.scans[scan].pieces[j] = bytes(piece)
    return b


# ---- seek points ------------------------------------------------------------------------------------------------------------

def reader_states(points, point_bytes):
    """(position, cache, valid) of every seek point: the last 24 bytes of a point (seek_decode.h)."""
    tail = points.reshape(-1, point_bytes)[:, -24:]
    return [(int(t[:8].view(np.uint64)[0]), int(t[8:16].view(np.uint64)[0]), int(t[16:20].view(np.int32)[0])) for t in tail]


def current_byte(segment, position, valid):
    """(b, phase): the byte the reader's next bit lies in and how many of its data bits are read.  The reader has fetched
    `position` bytes and counts 7 bits for a 0xFF (its eighth bit shares a place with the next byte's stuffed bit), 8 for any
    other; `valid` of them are unread.  In the stream itself it is the byte BEHIND a 0xFF that holds seven data bits."""
    read = sum(7 if b == 0xFF else 8 for b in segment[:position]) - valid
    assert read >= 0
    first = 0
    for b in range(len(segment)):
        bits = 7 if b and segment[b - 1] == 0xFF else 8
        if read < first + bits:
            return b, read - first
        first += bits
    return len(segment), read - first


# ---- the census -------------------------------------------------------------------------------------------------------------

def ff_census(segment: bytes, misalignment: int = 0, interval_parts=None) -> dict:
    """Where the 0xFF bytes of an entropy-coded segment fall when its first byte stands at an address that is `misalignment`
    mod 16: byte i has the coded position u = misalignment + i, which is what the kernels' aligned loads see.  (In a
    valid segment every 0xFF is a data byte followed by a 7-bit byte, or the first byte of an RSTm.)"""
    b = np.frombuffer(segment, dtype=np.uint8)
    ff = np.flatnonzero(b == 0xFF)
    u = ff + misalignment
    lanes = np.bincount(u // 16, minlength=1)
    words = np.zeros((len(lanes), 4), dtype=np.int64)
    np.add.at(words, (u // 16, (u % 16) // 4), 1)
    out = {
        "bytes": len(b),
        "count": len(ff),
        "density": len(ff) / max(1, len(b)),
        "positions_mod_16": set((u % 16).tolist()),
        "max_per_lane": int(lanes.max()) if len(ff) else 0,
        "lane_with_ff_in_every_word": bool((words > 0).all(axis=1).any()),
        "lane_with_two_in_every_word": bool((words >= 2).all(axis=1).any()),
        "ff_xx_ff": int(np.count_nonzero((b[:-2] == 0xFF) & (b[2:] == 0xFF))) if len(b) > 2 else 0,
        "ff_at_15_mod_16": bool((u % 16 == 15).any()),
        "ff_at_7_mod_8": bool((u % 8 == 7).any()),
        "first_is_ff": bool(len(b) and b[0] == 0xFF),
        "ends_ff_padding": bool(len(b) >= 2 and b[-2] == 0xFF),
    }
    for c in CHUNKS:
        out[f"ff_last_of_{c}"] = bool((u % c == c - 1).any())
        out[f"ff_first_of_{c}"] = bool((u % c == 0).any())
    if interval_parts is not None:
        out["intervals"] = len(interval_parts)
        out["intervals_ending_ff_xx"] = sum(1 for p in interval_parts if len(p) >= 2 and p[-2] == 0xFF)
    return out


# the chunk-edge and carry cases every decode class has to meet, at some misalignment
EDGE_CASES = tuple(f"ff_{e}_of_{c}" for c in CHUNKS for e in ("last", "first")) + \
    ("ff_at_15_mod_16", "ff_at_7_mod_8", "first_is_ff", "ends_ff_padding")
