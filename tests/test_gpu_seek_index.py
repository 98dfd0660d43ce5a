"""Seek-point index of the part-1 decoder (charls_amd.h: charls_amd_jpegls_decoder_*index*, decode_rows).

Streams come from the oracle's encoder, pixels are compared with the oracle's decoder byte for byte:
  * decode_to_buffer_and_index gives the plain decoder's pixels, decode_to_buffer through the index the same, and
    decode_rows bands at the top, the middle, across a seek point and the last row;
  * a tampered index still decodes exactly (the chain check sends the scan to the ordinary path, and the fallback counter
    moves); decode_rows with a foreign index of the same geometry is invalid_argument;
  * damaged streams decoded through the index of the undamaged stream give the errc of a plain decode;
  * one 4096 x 4096 frame decodes much faster through an index (slow).
GPU only."""
import random
import threading
import time

import numpy as np
import pytest

import oracle_bind as ob
from charls_amd import capi, synth

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 101
POINT_HEAD = 2992  # seek_decode.h: where the line buffer of a seek point starts


@pytest.fixture(scope="module")
def lib():
    return capi.load_product()


def _params(rng):
    bits = rng.choice([2, 8, 8, 12, 16])
    comps = rng.choice([1, 1, 3, 4, 2])
    ilv = 0 if comps == 1 else rng.choice([0, 1, 2])
    near = min(rng.choice([0, 0, 1, 3]), ((1 << bits) - 1) // 2)
    return dict(width=rng.choice([1, 7, 33, 64, 129]), height=rng.choice([5, 17, 40, 71]), bits=bits, comps=comps, ilv=ilv,
                near=near, kind=rng.choice(["mixed", "noise", "zero"]), seed=rng.randrange(1000), K=rng.choice([1, 4, 16, 32]))


def _stream(p, preset=None):
    img = synth.frame_numpy(p["width"], p["height"], seed=p["seed"], bits=p["bits"], components=p["comps"], kind=p["kind"],
                            interleaved=p["ilv"] != 0)
    return ob.encode(img, width=p["width"], height=p["height"], bits_per_sample=p["bits"], component_count=p["comps"],
                     near_lossless=p["near"], interleave_mode=p["ilv"], preset=preset,
                     destination_size=8 * p["width"] * p["height"] * p["comps"] + 4096)


def _band(full, p, first, count):
    """Rows [first, first + count) of an oracle destination in decode_to_buffer's layout."""
    bps = (p["bits"] + 7) // 8
    scans = p["comps"] if p["ilv"] == 0 else 1
    row = p["width"] * bps * (1 if p["ilv"] == 0 else p["comps"])
    planes = full.reshape(scans, p["height"], row)
    return planes[:, first:first + count, :].tobytes()


CASES = [_params(random.Random(s)) for s in range(60)]


@pytest.mark.parametrize("p", CASES, ids=[f"c{i}" for i in range(len(CASES))])
def test_indexed_decodes_match_the_oracle(lib, p):
    jls = _stream(p)
    _, want = ob.decode(jls)
    before = capi.index_counters()
    _, px, index = lib.decode_with_index(jls, lines_per_seek_point=p["K"])
    assert px.tobytes() == want.tobytes()
    _, px2 = lib.decode(jls, index=index)
    assert px2.tobytes() == want.tobytes()
    after = capi.index_counters()
    assert after["fallback_scans"] == before["fallback_scans"]
    has_points = p["height"] > p["K"]
    if has_points:
        assert after["scans_from_points"] > before["scans_from_points"]
    h, K = p["height"], p["K"]
    bands = {(0, 1), (h // 2, max(1, h // 4)), (h - 1, 1)}
    if K < h:
        bands.add((K - 1, min(2, h - K + 1)))
    for first, count in sorted(bands):
        count = min(count, h - first)
        for idx in (index, None):
            got = lib.decode_rows(jls, first, count, index=idx)
            assert got.tobytes() == _band(want, p, first, count), (first, count, idx is None)


def _fixture(width=96, height=80, K=8, seed=5, kind="mixed"):
    p = dict(width=width, height=height, bits=8, comps=1, ilv=0, near=0, kind=kind, seed=seed, K=K)
    jls = _stream(p)
    return p, jls


def _tamper(index, how, point_bytes, foreign=None):
    b = bytearray(index)
    pts = 72 + 24  # header + one scan record
    if how == "context":
        b[pts + 3 * point_bytes + 100 * 8 + 1] ^= 0x01  # a byte of A of context 100 in point 3
    elif how == "sample":
        b[pts + 3 * point_bytes + POINT_HEAD + 10] ^= 0x01
    elif how == "position":
        at = pts + 4 * point_bytes - 24 + 16  # valid bits of point 3
        b[at] ^= 1  # (one bit more or fewer in the cache: the reader sits one bit away)
    elif how == "swap":
        a0, a1 = pts + 2 * point_bytes, pts + 5 * point_bytes
        b[a0:a0 + point_bytes], b[a1:a1 + point_bytes] = b[a1:a1 + point_bytes], b[a0:a0 + point_bytes]
    elif how == "foreign":
        b[pts:] = foreign[pts:]
    return bytes(b)


@pytest.mark.parametrize("how", ["context", "sample", "position", "swap", "foreign"])
def test_a_tampered_index_still_decodes_exactly(lib, how):
    p, jls = _fixture()
    _, want = ob.decode(jls)
    _, _, index = lib.decode_with_index(jls, lines_per_seek_point=p["K"])
    _, _, other = lib.decode_with_index(_fixture(seed=77)[1], lines_per_seek_point=p["K"])
    point_bytes = int.from_bytes(index[64:68], "little")
    bad = _tamper(index, how, point_bytes, other)
    assert bad != index
    before = capi.index_counters()
    try:
        _, px = lib.decode(jls, index=bad)
    except capi.JpegLSError as e:  # a field pushed out of range is refused by set_index
        assert e.errc == INVALID_ARGUMENT and how == "position"
        return
    assert px.tobytes() == want.tobytes()
    assert capi.index_counters()["fallback_scans"] == before["fallback_scans"] + 1


def test_decode_rows_refuses_a_foreign_index(lib):
    p, jls = _fixture()
    _, _, other = lib.decode_with_index(_fixture(seed=78)[1], lines_per_seek_point=p["K"])
    with pytest.raises(capi.JpegLSError) as e:
        lib.decode_rows(jls, 40, 8, index=other)
    assert e.value.errc == INVALID_ARGUMENT


def _mutations(jls, rng, n):
    out = []
    for _ in range(n):
        b = bytearray(jls)
        kind = rng.choice(["flip", "truncate", "ff"])
        at = rng.randrange(len(b) // 3, len(b) - 2)
        if kind == "flip":
            b[at] ^= 1 << rng.randrange(8)
        elif kind == "ff":
            b[at] = 0xFF
        else:
            b = b[:at]
        out.append(bytes(b))
    return out


def _errc(fn):
    try:
        fn()
        return 0
    except capi.JpegLSError as e:
        return e.errc


def test_damaged_streams_through_the_index_of_the_undamaged_stream(lib):
    p, jls = _fixture(kind="noise")
    _, _, index = lib.decode_with_index(jls, lines_per_seek_point=p["K"])
    for bad in _mutations(jls, random.Random(3), 24):
        plain = _errc(lambda: lib.decode(bad))
        indexed = _errc(lambda: lib.decode(bad, index=index))
        assert indexed == plain, (plain, indexed)
        if plain == 0:
            assert lib.decode(bad, index=index)[1].tobytes() == lib.decode(bad)[1].tobytes()


def test_threads_with_their_own_index_alongside_plain_callers(lib):
    streams = [_fixture(width=64 + 8 * i, height=48, K=8, seed=200 + i)[1] for i in range(8)]
    wants = [ob.decode(s)[1].tobytes() for s in streams]
    indexes = [lib.decode_with_index(s, lines_per_seek_point=8)[2] for s in streams]
    errors = []

    def work(t):
        try:
            i = t % len(streams)
            for _ in range(3):
                got = lib.decode(streams[i], index=indexes[i] if t % 2 == 0 else None)[1].tobytes()
                if got != wants[i]:
                    errors.append(t)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(64)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert errors == []


@pytest.mark.slow
def test_single_frame_latency_with_an_index(lib, capsys):
    """One 4096 x 4096 8-bit frame: K = 64 turns one chain into 64 without restart markers."""
    img = synth.frame_numpy(4096, 4096, seed=2, bits=8)
    jls = ob.encode(img, width=4096, height=4096, bits_per_sample=8)
    lib.decode(jls)  # (warm)
    a = time.perf_counter()
    px = lib.decode(jls)[1]
    plain = time.perf_counter() - a
    assert px.tobytes() == img.tobytes()
    a = time.perf_counter()
    _, px, index = lib.decode_with_index(jls, lines_per_seek_point=64)
    build = time.perf_counter() - a
    assert px.tobytes() == img.tobytes()
    a = time.perf_counter()
    px = lib.decode(jls, index=index)[1]
    indexed = time.perf_counter() - a
    assert px.tobytes() == img.tobytes()
    # (a band is decoded by one wavefront per interval it touches: with the exact decoder at ~1.3 MPix/s a band takes up to
    # K rows on one chain, so bands want a finer index than whole frames)
    _, _, index16 = lib.decode_with_index(jls, lines_per_seek_point=16)
    a = time.perf_counter()
    band = lib.decode_rows(jls, 2048 - 32, 64, index=index16)
    banded = time.perf_counter() - a
    assert band.tobytes() == img[2048 - 32:2048 + 32].tobytes()
    a = time.perf_counter()
    band = lib.decode_rows(jls, 2048 - 32, 64)
    top = time.perf_counter() - a
    assert band.tobytes() == img[2048 - 32:2048 + 32].tobytes()
    with capsys.disabled():
        print(f"\n[seek index] 4096x4096: plain {plain:.3f}s, decode + index build {build:.3f}s, indexed K=64 {indexed:.3f}s, "
              f"64-row band from the middle: K=16 index {banded:.3f}s, no index {top:.3f}s; index K=64 {len(index)} B = "
              f"{100 * len(index) / len(jls):.1f}% of {len(jls)} B, K=16 {len(index16)} B")
    assert indexed < plain / 4
    assert banded < plain / 20
