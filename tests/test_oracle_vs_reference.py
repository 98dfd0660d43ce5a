"""Cross-check oracle <-> reference, randomized parameters.  CPU only.
What the reference (oracle/_ref/libcharls_ref.so) gives for every case is stored in tests/golden/oracle_vs_reference.json
(tests/golden/make_oracle_vs_reference.py), so the oracle is held to the reference wherever the suite runs; where the reference
build is present it is run live as well and must still give what is stored."""
import json
import os

import numpy as np
import pytest

import common
import oracle_bind as ob
from charls_amd import synth
from charls_amd.capi import CharLSLibrary, JpegLSError

GOLDEN_FILE = os.path.join(common.GOLDEN, "oracle_vs_reference.json")
CHUNKS = 8


def _image(rng, w, h, bits, comps, ilv, kind, seed):
    dt = np.uint8 if bits <= 8 else np.uint16
    shape = (h, w) if comps == 1 else ((comps, h, w) if ilv == 0 else (h, w, comps))
    if kind == "rand":
        return rng.integers(0, 1 << bits, size=shape).astype(dt)
    if kind == "smooth":
        base = int(rng.integers(0, 1 << bits))
        axis = -1 if (comps == 1 or ilv == 0) else 1
        return np.clip(base + rng.integers(-2, 3, size=shape).cumsum(axis=axis) // 3, 0, (1 << bits) - 1).astype(dt)
    return synth.frame_numpy(w, h, seed=seed, bits=bits, components=comps, kind=kind, interleaved=(ilv != 0))


def random_cases(chunk):
    """The 150 seeded (encoder arguments, image) pairs of one chunk."""
    rng = np.random.default_rng(1000 + chunk)
    for it in range(150):
        bits = int(rng.integers(2, 17))
        comps = int(rng.choice([1, 1, 1, 2, 3, 3, 4]))
        ilv = 0 if comps == 1 else int(rng.integers(0, 3))
        w = int(rng.choice([1, 2, 3, 5, 17, 64, 100, 257]))
        h = int(rng.choice([1, 2, 3, 8, 33, 64]))
        maxval = (1 << bits) - 1
        near = 0 if rng.random() < 0.5 else int(rng.integers(0, min(255, maxval // 2) + 1))
        ct = 0
        if comps == 3 and bits in (8, 16) and near == 0 and ilv != 0 and rng.random() < 0.5:
            ct = int(rng.integers(1, 4))
        kind = str(rng.choice(["rand", "smooth", "gradient", "mixed", "zero", "hard"]))
        preset = None
        if rng.random() < 0.25:
            mv = int(rng.integers(max(1, 2 * near), maxval + 1)) if rng.random() < 0.5 else 0
            mvv = mv or maxval
            if near <= min(255, mvv // 2):
                t1 = int(rng.integers(near + 1, mvv + 1))
                t2 = int(rng.integers(t1, mvv + 1))
                t3 = int(rng.integers(t2, mvv + 1))
                preset = (mv, t1, t2, t3, int(rng.integers(3, max(255, mvv) + 1)))
        img = _image(rng, w, h, bits, comps, ilv, kind, it)
        kw = dict(width=w, height=h, bits_per_sample=bits, component_count=comps, near_lossless=near,
                  interleave_mode=ilv, color_transformation=ct, preset=preset)
        yield kw, img


def boundary_image():
    return synth.frame_numpy(64, 64, seed=3, kind="mixed")


def observe(encode, decode, error, img, kw):
    """What one codec makes of one case: [errc, SHA-256 of the .jls, SHA-256 of the samples it decodes that .jls to]
    (the hashes are None after an encoder error; the last one also when `decode` is None)."""
    try:
        data = encode(img, **kw)
    except error as e:
        return [e.errc, None, None]
    return [0, common.sha(data), common.sha(decode(data)[1].tobytes()) if decode is not None else None]


def _golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ref():
    """The live reference, where oracle/_ref was built; None elsewhere (the stored observations stand in for it)."""
    return CharLSLibrary(ob.REF_LIB) if os.path.exists(ob.REF_LIB) else None


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_random_parameters(chunk, ref):
    want = _golden()["random_parameters"][str(chunk)]
    cases = list(random_cases(chunk))
    assert len(want) == len(cases)
    for (kw, img), stored in zip(cases, want):
        assert observe(ob.encode, ob.decode, ob.OracleError, img, kw) == stored, kw
        if ref is not None:
            assert observe(ref.encode, ref.decode, JpegLSError, img, kw) == stored, kw


def test_destination_too_small_boundary(ref):
    """src/scan_encoder.hpp:119-120: the encoder needs >= 4 free bytes at every flush."""
    golden = _golden()["destination_too_small"]
    img, full = boundary_image(), golden["full_size"]
    if ref is not None:
        assert len(ref.encode(img, width=64, height=64)) == full
    caps = list(range(full - 8, full + 8))
    assert len(golden["observations"]) == len(caps)
    for cap, stored in zip(caps, golden["observations"]):
        kw = dict(width=64, height=64, destination_size=cap)
        assert observe(ob.encode, None, ob.OracleError, img, kw) == stored, cap
        if ref is not None:
            assert observe(ref.encode, None, JpegLSError, img, kw) == stored, cap
