"""The census of the stuffing corpus (tests/stuffing.py): that its streams reach what they are for, asserted from the ORACLE's
bytes alone -- nothing here runs the code under test.

* density: a 0xFF in 45 % of the bytes of a pure ramp or flat frame, in 20 % of a specked one (`synth` noise: 0.2 %);
* a specked frame has a 0xFF at every byte position of a 16-byte lane, a pure ramp a lane with 8 of them, two in each word;
* every decode class meets, at one of the 16 misalignments the other tests use, a 0xFF on each chunk edge of its kernels;
* a tall flat frame costs one bit a line; streams that start with 0xFF, that end in 0xFF and its padding byte, and that do not;
* a quarter of the restart intervals of 7 and of 16 lines end in FF xx, in all and in every frame that is there for them;
* the oracle's stream is the reference's wherever oracle/_ref was built.

CPU only."""
import os

import numpy as np
import pytest

import oracle_bind as ob
import stuffing as st
from charls_amd.capi import CharLSLibrary

CORPUS = st.CORPUS
PURE = [n for n in CORPUS if st.is_pure(n)]
SPECKED = [n for n in CORPUS if st.is_specked(n)]
PURE_RAMPS = [n for n in PURE if not st.is_flat(n)]
FLAT = [n for n in CORPUS if st.is_flat(n)]


def census(name, misalignment=0):
    return [st.ff_census(s, misalignment) for s in st.coded(name).segments]


def test_ff_census_on_a_hand_made_segment():
    """The census is test code too: a segment of 40 bytes with known 0xFF bytes, its first byte at address 13 mod 16."""
    seg = bytearray(40)
    for i in (0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 20, 38):   # u = 13, 15, 16 .. 23, 33, 51
        seg[i] = 0xFF
    c = st.ff_census(bytes(seg), 13)
    assert (c["bytes"], c["count"], c["density"]) == (40, 12, 0.3)
    assert c["positions_mod_16"] == {13, 15, 0, 1, 2, 3, 4, 5, 6, 7}
    assert c["max_per_lane"] == 8 and c["lane_with_ff_in_every_word"] is False   # lane 1 holds u = 16 .. 23: words 0 and 1
    assert c["ff_xx_ff"] == 8   # (0, 2), (2, 4), (3, 5) .. (8, 10)
    assert c["ff_at_15_mod_16"] and c["ff_at_7_mod_8"] and c["first_is_ff"] and c["ends_ff_padding"]
    assert not c["ff_last_of_128"] and not c["ff_first_of_128"]
    c = st.ff_census(bytes(seg), 0)
    assert not c["ff_at_15_mod_16"] and c["ff_at_7_mod_8"] and c["ff_first_of_1024"]
    assert st.ff_census(b"\xff" * 16, 0)["lane_with_ff_in_every_word"] and st.ff_census(b"\xff" * 16, 0)["lane_with_two_in_every_word"]
    assert st.ff_census(b"\x00" * 127 + b"\xff\x7f", 0)["ff_last_of_128"] and st.ff_census(b"\x00" * 127 + b"\xff\x7f", 1)["ff_first_of_128"]
    assert not st.ff_census(b"\x12\x34", 0)["ends_ff_padding"] and st.ff_census(b"\x12", 0)["count"] == 0


def test_the_corpus_holds_what_it_was_asked_to_hold():
    c = CORPUS
    assert 30 <= len(c) <= 60
    assert all((x.width <= 200 and x.height <= 200) or (x.width <= 16 and x.height <= 4096) for x in c.values())
    gray = [x for n, x in c.items() if x.comps == 1 and not st.is_partner(n)]
    for bits in (8, 12, 16):
        names = [n for n in PURE_RAMPS if c[n].bits == bits and c[n].comps == 1 and c[n].near == 0]
        assert names, bits
        assert len({n for n in SPECKED if c[n].bits == bits and c[n].comps == 1 and c[n].near == 0 and n.startswith("ramp")}) >= 2
    assert {(x.comps, x.ilv) for x in c.values() if x.comps == 3} == {(3, 0), (3, 1), (3, 2)}
    assert {(x.near, x.bits) for x in gray if x.near} >= {(n, b) for n in (1, 2, 3) for b in (8, 16)}
    assert {x.width for n, x in c.items() if st.is_flat(n)} == {1, 2, 5, 16}
    assert any(st.is_flat(n) and x.near for n, x in c.items()) and any(st.is_flat(n) and st.is_specked(n) for n in c)
    for key, (w, h, bits, *_rest) in st.GRAY.items():
        assert {f"noise_{key}", f"gradient_{key}", f"flat_{key}"} <= set(c)
        reset = [n for n, x in c.items() if (x.width, x.height, x.bits) == (w, h, bits) and x.preset == st.RESET256]
        assert len(reset) == (1 if bits > 8 else 0), key   # (RESET = 256 is not legal at 8 bit)


@pytest.mark.parametrize("name", PURE)
def test_pure_frames_have_a_ff_in_45_percent_of_their_bytes(name):
    for c in census(name):
        assert c["density"] >= 0.45, (name, c["density"])


@pytest.mark.parametrize("name", SPECKED)
def test_specked_frames_are_dense_and_reach_every_byte_position(name):
    for c in census(name):
        assert c["density"] >= 0.2, (name, c["density"])
        assert c["positions_mod_16"] == set(range(16)), (name, sorted(c["positions_mod_16"]))
        assert c["ff_xx_ff"] >= 8   # a condition, not a measurement (a lane's worth; the noise frames have none)


@pytest.mark.parametrize("name", PURE_RAMPS)
def test_pure_ramps_have_a_lane_with_two_ff_in_every_word(name):
    for m in (0, 1):   # FF 7F FF 7F ...: whichever parity the stream starts at
        for c in census(name, m):
            assert c["max_per_lane"] == 8 and c["lane_with_two_in_every_word"], (name, m)


def test_partners_are_not_dense():
    for key in st.GRAY:
        for kind in ("noise", "gradient"):
            assert census(f"{kind}_{key}")[0]["density"] < 0.01
        dense = next(n for n in st.DENSE if n.startswith(f"ramp_{key}"))
        assert census(f"noise_{key}")[0]["bytes"] > 2 * census(dense)[0]["bytes"]   # a long stream
        assert 8 * census(f"flat_{key}")[0]["bytes"] < census(dense)[0]["bytes"]   # this scan ends while its neighbours are in mid-stream


@pytest.mark.parametrize("route", st.DECODE_CLASSES)
def test_every_decode_class_meets_every_chunk_edge(route, capsys):
    """Over the frames of the class (emulator or GPU) and the 16 misalignments: a 0xFF as the last and as the first byte of a
    chunk of 128, 256, 512 and 1024 bytes, as byte 15 of a lane, as byte 7 of the exact reader's 8-byte fill, as the first coded
    byte and as the last data byte."""
    names = st.route_frames(route, "gpu", dense=True) if route == "serial_decode" else st.route_frames(route, "any", dense=True)
    found = {}
    for n in names:
        for m in st.MISALIGNMENTS:
            for i, c in enumerate(census(n, m)):
                for case in st.EDGE_CASES:
                    if c[case]:
                        found.setdefault(case, (n, i, m))
    with capsys.disabled():
        print(f"\n{route}: " + ", ".join(f"{k}: {v[0]}[{v[1]}]@{v[2]}" for k, v in found.items()))
    assert set(found) == set(st.EDGE_CASES), (route, sorted(set(st.EDGE_CASES) - set(found)))


def test_flat_frames_cost_one_bit_a_line_and_cover_both_ends():
    cs = {n: census(n)[0] for n in FLAT}
    for n, c in cs.items():
        if not st.is_specked(n):
            assert c["bytes"] <= CORPUS[n].height / 7.5 + 16, (n, c["bytes"])
    assert sum(c["first_is_ff"] for c in cs.values()) >= 1
    assert sum(c["ends_ff_padding"] for c in cs.values()) >= 2
    assert sum(not c["ends_ff_padding"] for c in cs.values()) >= 2


@pytest.mark.parametrize("lines", st.RESTART_LINES)
def test_a_quarter_of_the_restart_intervals_end_in_ff_xx(lines, capsys):
    ending, total = 0, 0
    for name in st.RESTART_FRAMES:
        seg, at = st.dri_scan(name, lines)
        c = st.ff_census(seg, 0, interval_parts=st.intervals(name, lines))
        assert c["intervals"] == len(at) + 1 == -(-CORPUS[name].height // lines)
        assert all(seg[a] == 0xFF and seg[a + 1] == 0xD0 + (j & 7) for j, a in enumerate(at))
        x = CORPUS[name]
        got = np.frombuffer(st.dri_pixels(name, lines), dtype=x.img.dtype).astype(np.int64)
        assert np.abs(got - x.img.reshape(-1).astype(np.int64)).max() <= x.near   # the oracle reads what was put together here
        ending, total = ending + c["intervals_ending_ff_xx"], total + c["intervals"]
        if name in st.RESTART_ENDINGS:   # each of them on its own, so that no frame carries the sum
            assert 4 * c["intervals_ending_ff_xx"] >= c["intervals"], (lines, name, c["intervals_ending_ff_xx"], c["intervals"])
        with capsys.disabled():
            print(f"\n{lines} lines, {name}: {c['intervals_ending_ff_xx']} of {c['intervals']} intervals end in FF xx", end="")
    assert 4 * ending >= total, (lines, ending, total)


def test_a_synth_noise_frame_in_place_of_a_recipe_fails_the_floors():
    """The floors are not met by the inputs the other tests use."""
    from charls_amd import synth
    img = synth.frame_numpy(128, 96, seed=41, bits=8, kind="noise")
    jls = ob.encode(img, width=128, height=96)
    c = st.ff_census(jls[st.jls_container.parse(jls).scans[0].data_start:-2], 0)
    assert c["density"] < 0.01 and c["max_per_lane"] <= 2 and not c["lane_with_ff_in_every_word"]


@pytest.fixture(scope="module")
def ref():
    """The live reference, where oracle/_ref was built; None elsewhere."""
    return CharLSLibrary(ob.REF_LIB) if os.path.exists(ob.REF_LIB) else None


@pytest.mark.parametrize("name", list(CORPUS))
def test_oracle_round_trip_and_the_reference_s_stream(name, ref):
    cc = st.coded(name)
    c = cc.corner
    got = np.frombuffer(cc.pixels, dtype=c.img.dtype).astype(np.int64)
    assert np.abs(got - c.img.reshape(-1).astype(np.int64)).max() <= c.near
    if ref is not None:
        assert ref.encode(c.img, destination_size=8 * c.img.nbytes + 4096, **c.kw()) == cc.jls
        assert ref.decode(cc.jls)[1].tobytes() == cc.pixels
