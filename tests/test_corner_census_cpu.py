"""The census of the corner corpus (tests/corners.py): which corner states of the JPEG-LS model the frames reach, counted
by the oracle (oracle/jls_oracle.h, enum jls_census).

* floors: every counter is reached, in every sample-width class, by some frame of the corpus;
* the inputs the other tests use (the kinds of charls_amd.synth) reach fewer of them -- printed, so the table of DESIGN 2
  can be made again;
* the oracle decodes its own streams, with the same census in both directions, and is pinned on these frames to what the
  reference made of them (tests/golden/corners.json, tests/golden/make_corner_golden.py) and to the live reference where
  oracle/_ref was built;
* every coding route meets, between the emulator and the GPU, every counter that can occur on it (corners.ROUTES).

CPU only."""
import json
import os

import numpy as np
import pytest

import common
import corners
import oracle_bind as ob
from charls_amd import synth
from charls_amd.capi import CharLSLibrary

CLASSES = ("8", "9-12", "13-16")
FLOOR = 8   # events; a condition, not a measurement
# The "largest" counters have to equal the legal extreme.  k is the smallest k with N << k >= A, and A grows by |Errval| <=
# RANGE / 2 = 2^(bits-1) a sample while N grows by one (both halve together): A <= N * 2^(bits-1), so k <= bits - 1; the same
# holds for the run-interruption contexts.  RUNindex stops at 31.
EXTREME = {"max_regular_k": {"8": 7, "9-12": 11, "13-16": 15}, "max_run_k": {"8": 7, "9-12": 11, "13-16": 15},
           "max_run_index": {"8": 31, "9-12": 31, "13-16": 31}}
AT_LEAST_ONCE = ("block_at_run_index_31",)   # 32768 samples each

# (counter, class) pairs that cannot occur, each with its reason: the only permitted omissions
CANNOT_OCCUR = {
    ("prefix_over_31", "8"): "the longest prefix is LIMIT - qbpp = 32 - qbpp bits with its closing 1, and qbpp >= 1 (NEAR = 127: RANGE = 2)",
}

# counters that cannot occur on a route (whatever the class), each with its reason
ROUTE_CANNOT = {
    "group_encode": {
        "error_correction": "needs NEAR = 0; the group encoder codes the near-lossless scans",
        "max_regular_k": "k = bits - 1 needs errors of RANGE / 2 = 2^(bits-1): NEAR = 0",
        "max_run_k": "as max_regular_k",
    },
}
# ... and in a class: a completed block at RUNindex 31 is 2^15 samples of ONE line
for _route in ("group_decode", "fast_decode", "exact_decode", "pixel_decode", "seek_decode"):
    ROUTE_CANNOT.setdefault(_route, {})["block_at_run_index_31", "9-12"] = ROUTE_CANNOT[_route]["block_at_run_index_31", "13-16"] = \
        "a line of 2^15 samples wider than 8 bits is beyond the 64 KiB of LDS the wave kernels keep a line in"


def reached(censuses, klass):
    """The counters that a set of census dicts (of frames of one class) reaches."""
    out = set()
    for k in ob.CENSUS:
        top = max((c[k] for c in censuses), default=0)
        need = EXTREME[k][klass] if k in EXTREME else (1 if k in AT_LEAST_ONCE else FLOOR)
        if top >= need:
            out.add(k)
    return out


def corpus_census(names, klass):
    return [corners.coded(n).encode_census for n in names if corners.CORPUS[n].klass == klass]


def test_the_names_of_the_counters_are_the_header_s():
    with open(os.path.join(ob.ORACLE_DIR, "jls_oracle.h")) as f:
        text = f.read()
    body = text[text.index("enum jls_census"):text.index("JLS_CENSUS_COUNT")]
    names = [line.split("JLS_CENSUS_")[1].split(",")[0].split(" ")[0].lower() for line in body.splitlines() if "JLS_CENSUS_" in line]
    assert tuple(names) == ob.CENSUS
    assert set(ob.CENSUS_MAXIMA) == set(EXTREME)


@pytest.mark.parametrize("klass", CLASSES)
def test_census_floors(klass):
    got = reached(corpus_census(corners.CORPUS, klass), klass)
    missing = {k for k in ob.CENSUS if k not in got and (k, klass) not in CANNOT_OCCUR}
    assert not missing, (klass, sorted(missing))
    # what is listed as impossible does not occur: the list holds no counter the corpus could be held to
    for (k, cl) in CANNOT_OCCUR:
        if cl == klass:
            assert all(c[k] == 0 for c in corpus_census(corners.CORPUS, klass)), k


def _todays_inputs(bits):
    w, h = 256, 64
    kinds = ["gradient", "mixed", "zero", "noise", "hard"]
    frames = [(k, synth.frame_numpy(w, h, seed=3, bits=bits, kind=k)) for k in kinds]
    if bits == 8:  # the reference's natural image, as bench.py's `tulips` data tiles it: a window of it
        frames.append(("tulips_tiled", np.ascontiguousarray(common.read_pnm("tulips-gray-8bit-512-512.pgm")[0][:h, :w])))
    return w, h, frames


def test_census_of_todays_inputs(capsys):
    """Informational: the census of the kinds of charls_amd.synth at 256 x 64, NEAR 0 and 3 -- the table of DESIGN 2.  The
    corpus has to reach strictly more counters in every class."""
    lines = []
    for klass, bits in zip(CLASSES, (8, 12, 16)):
        w, h, frames = _todays_inputs(bits)
        seen = []
        for kind, img in frames:
            for near in (0, 3):
                c = {}
                ob.encode(img, width=w, height=h, bits_per_sample=bits, near_lossless=near, census=c,
                          destination_size=4 * img.nbytes + 4096)
                seen.append(c)
                lines.append(f"{bits:2d} bit {kind:12s} NEAR {near}: " + " ".join(f"{k}={v}" for k, v in c.items() if v))
        theirs, ours = reached(seen, klass), reached(corpus_census(corners.CORPUS, klass), klass)
        lines.append(f"{bits:2d} bit: synth reaches {len(theirs)} counters, the corpus {len(ours)}; synth misses {sorted(set(ob.CENSUS) - theirs)}")
        assert theirs < ours, (klass, sorted(theirs - ours))
    with capsys.disabled():
        print("\n" + "\n".join(lines))


@pytest.mark.parametrize("name", list(corners.CORPUS))
def test_oracle_round_trip_and_census_both_ways(name):
    cc = corners.coded(name)
    c = cc.corner
    got = np.frombuffer(cc.pixels, dtype=c.img.dtype).astype(np.int64)
    want = c.img.reshape(-1).astype(np.int64)
    if c.ct == 0:
        assert np.abs(got - want).max() <= c.near
    if c.near == 0:
        assert cc.pixels == c.img.tobytes()
    assert cc.encode_census == cc.decode_census   # every counter is shared by the two directions
    assert set(cc.encode_census) == set(ob.CENSUS)


def test_census_calls_change_nothing():
    """The counting entry points give the bytes and pixels of the plain ones."""
    for name in ("escape_run_8", "noise_16_near3", "sample3_12"):
        c = corners.CORPUS[name]
        cc = corners.coded(name)
        assert ob.encode(c.img, destination_size=8 * c.img.nbytes + 4096, **c.kw()) == cc.jls
        assert ob.decode(cc.jls)[1].tobytes() == cc.pixels


GOLDEN_FILE = os.path.join(common.GOLDEN, "corners.json")


def _golden():
    with open(GOLDEN_FILE) as f:
        return {row["name"]: row for row in json.load(f)}


def observe(codec, c):
    """What one codec (encode / decode as oracle_bind's or CharLSLibrary's) makes of one corner frame."""
    jls = codec.encode(c.img, destination_size=8 * c.img.nbytes + 4096, **c.kw())
    return dict(name=c.name, parameters=c.params(), jls_size=len(jls), jls_sha256=common.sha(jls),
                pixels_sha256=common.sha(codec.decode(jls)[1].tobytes()))


def test_golden_file_lists_the_corpus():
    assert list(_golden()) == list(corners.CORPUS)


@pytest.fixture(scope="module")
def ref():
    """The live reference, where oracle/_ref was built; None elsewhere (the stored observations stand in for it)."""
    return CharLSLibrary(ob.REF_LIB) if os.path.exists(ob.REF_LIB) else None


@pytest.mark.parametrize("name", list(corners.CORPUS))
def test_oracle_is_pinned_to_the_reference(name, ref):
    c = corners.CORPUS[name]
    stored = _golden()[name]
    assert observe(ob, c) == stored
    if ref is not None:
        assert observe(ref, c) == stored


# ---- the routes --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", list(corners.ROUTES))
def test_every_route_meets_every_corner_that_can_occur_on_it(route):
    """Between the emulator (tests/test_emu_corners.py) and the GPU (tests/test_gpu_corners.py), which both take their frames
    from corners.route_frames."""
    names = corners.route_frames(route, "any")
    cannot = ROUTE_CANNOT.get(route, {})
    for klass in CLASSES:
        got = reached(corpus_census(names, klass), klass)
        missing = {k for k in ob.CENSUS if k not in got and (k, klass) not in CANNOT_OCCUR and k not in cannot and (k, klass) not in cannot}
        assert not missing, (route, klass, sorted(missing))


def test_route_tables_name_the_same_routes_and_use_every_frame():
    assert set(corners.ROUTES) == set(corners.EMU_ROUTES)
    for where in ("gpu", "emu"):
        used = set()
        for route in corners.ROUTES:
            used |= set(corners.route_frames(route, where))
        assert used == set(corners.CORPUS), where
