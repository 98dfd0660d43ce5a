"""What the tests of charls_amd.h part 2k (byte budgets for ragged frames and for re-coding) share: the selection rule, the
offset rule of part 2d, the builder of streams with restart intervals, and the corpus -- the frame kinds of the GPU tests with
the oracle's stream of every kind and candidate (tests/oracle_bind.py), computed once and never changed.  No tests here."""
import functools

import numpy as np

import jls_container
import oracle_bind as ob
from charls_amd import synth

DESTINATION_TOO_SMALL = 3
INVALID_ARGUMENT_NEAR_LOSSLESS, INVALID_ARGUMENT_COLOR_TRANSFORMATION = 107, 109
EVEN_DESTINATION_SIZE = 1

# kind -> width, height, bits, components, interleave mode, colour transformation, encoding options, restart interval, row stride
KINDS = {
    "gray8_33x17": (33, 17, 8, 1, 0, 0, 0, 0, 0),
    "gray12_19x9": (19, 9, 12, 1, 0, 0, 0, 0, 0),
    "gray16_65x5": (65, 5, 16, 1, 0, 0, 0, 0, 0),
    "gray_1x1": (1, 1, 8, 1, 0, 0, 0, 0, 0),
    "rgb_planar_16x8": (16, 8, 8, 3, 0, 0, 0, 0, 0),
    "rgb_line_16x8": (16, 8, 8, 3, 1, 0, 0, 0, 0),
    "rgb_sample_16x8": (16, 8, 8, 3, 2, 0, 0, 0, 0),
    "rgb_sample_hp1_16x8": (16, 8, 8, 3, 2, 1, 0, 0, 0),          # refused with any NEAR > 0
    "gray8_restart2_33x17": (33, 17, 8, 1, 0, 0, 0, 2, 0),         # sized by coding it for real
    "gray8_padded48_odd_base_33x17": (33, 17, 8, 1, 0, 0, 0, 0, 48),
    "gray8_even_size_33x17": (33, 17, 8, 1, 0, 0, EVEN_DESTINATION_SIZE, 0, 0),
}
# 200 is legal for the 12- and 16-bit kinds and above the largest NEAR of the 8-bit ones; NARROW names NEAR 1 twice.
WIDE = (0, 1, 2, 4, 200)
NARROW = (0, 1, 1, 2, 4)
REPEATS = 4  # the frames of a call: every kind REPEATS times, interleaved -- a, b, c, ..., a, b, c, ...


# ---- the rules ---------------------------------------------------------------------------------------------------------------

def choose(sizes, budget):
    """The selection rule: the index of the first candidate, in the order given, whose size is at most the budget; -1: none."""
    for k, s in enumerate(sizes):
        if int(s) <= int(budget):
            return k
    return -1


def rule_offsets(sizes, alignment):
    """The offset rule of part 2d: every stream starts at the end of the one before it, rounded up to the alignment."""
    out = [0]
    for s in sizes:
        out.append(-(-(out[-1] + int(s)) // alignment) * alignment)
    return np.array(out, dtype=np.uint64)


def dri_stream(img, w, h, kw, interval):
    """The stream of a single-scan frame with restart intervals, put together from the oracle's coding of every interval as an
    image of its own with RSTm between them (the reference cannot write restart markers)."""
    full = ob.encode(img, width=w, height=h, **kw)
    scan = jls_container.parse(full).scans[0]
    sos = full.rfind(b"\xff\xda", 0, scan.data_start)
    body, n = b"", (h + interval - 1) // interval
    for j in range(n):
        sub = np.ascontiguousarray(img[j * interval:(j + 1) * interval])
        s = ob.encode(sub, width=w, height=sub.shape[0], **kw)
        sc = jls_container.parse(s).scans[0]
        body += s[sc.data_start:sc.data_end] + (bytes([0xFF, 0xD0 + (j & 7)]) if j + 1 < n else b"")
    out = full[:sos] + b"\xff\xdd\x00\x04" + interval.to_bytes(2, "big") + full[sos:scan.data_start] + body
    if kw.get("encoding_options", 0) & EVEN_DESTINATION_SIZE and len(out) & 1:
        out += b"\xff"
    return out + b"\xff\xd9"


# ---- the corpus --------------------------------------------------------------------------------------------------------------

def refusal(kind, candidates):
    """The code the encoder refuses the kind's parameters with at the first candidate it refuses, 0 when it takes them all."""
    bits, ct = KINDS[kind][2], KINDS[kind][5]
    largest = min(255, ((1 << bits) - 1) // 2)
    for near in candidates:
        if near < 0 or near > largest:
            return INVALID_ARGUMENT_NEAR_LOSSLESS
        if near > 0 and ct != 0:
            return INVALID_ARGUMENT_COLOR_TRANSFORMATION
    return 0


@functools.lru_cache(maxsize=None)
def image(kind, repeat):
    """The pixels of frame (kind, repeat) in the user's layout.  The last repeat names the pixels of the first again."""
    w, h, bits, comps, ilv = KINDS[kind][:5]
    repeat = 0 if repeat == REPEATS - 1 else repeat
    img = synth.frame_numpy(w, h, seed=11 + 5 * repeat, bits=bits, components=comps, kind=("gradient", "noise", "noise")[repeat % 3],
                            interleaved=ilv != 0)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def oracle_stream(kind, repeat, near, restart=None):
    """The oracle's .jls of frame (kind, repeat) at `near`; `restart`: another restart interval than the kind's."""
    w, h, bits, comps, ilv, ct, options, interval, _ = KINDS[kind]
    interval = interval if restart is None else restart
    kw = dict(bits_per_sample=bits, component_count=comps, interleave_mode=ilv, color_transformation=ct, encoding_options=options,
              near_lossless=near)
    if interval == 0:
        return ob.encode(image(kind, repeat), width=w, height=h, **kw)
    assert comps == 1 or ilv != 0
    return dri_stream(image(kind, repeat), w, h, kw, interval)


def oracle_sizes(kind, repeat, candidates):
    return [len(oracle_stream(kind, repeat, near)) for near in candidates]


def call_frames():
    """[(kind, repeat)] of the GPU test's call, in the caller's order."""
    return [(kind, repeat) for repeat in range(REPEATS) for kind in KINDS]


def budget_of(kind, repeat, candidates, position):
    """The budget of frame (kind, repeat) -- taken from the oracle's sizes: repeat 0 the size at the first candidate exactly, repeat
    1 the size at candidate 1 exactly, repeat 2 that size less one byte, repeat 3 nothing (0) or 2^63 in turn."""
    if refusal(kind, candidates):
        return 1 << 20
    sizes = oracle_sizes(kind, repeat, candidates)
    return (sizes[0], sizes[1], sizes[1] - 1, (0, 1 << 63)[position % 2])[repeat]


def expected(frames, candidates, budgets):
    """[(errc, near, stream)] of the frames under the selection rule on the oracle's sizes; stream b"" for a frame not coded."""
    out = []
    for (kind, repeat), budget in zip(frames, budgets):
        code = refusal(kind, candidates)
        if code:
            out.append((code, -1, b""))
            continue
        k = choose(oracle_sizes(kind, repeat, candidates), budget)
        out.append((0, candidates[k], oracle_stream(kind, repeat, candidates[k])) if k >= 0 else (DESTINATION_TOO_SMALL, -1, b""))
    return out
