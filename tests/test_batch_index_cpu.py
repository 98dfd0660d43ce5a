"""charls_amd_index_size_bound (charls_amd.h part 2c) without a GPU: for every kind of frame it equals what
charls_amd_jpegls_decoder_get_index_size reports for an oracle-coded stream with those parameters, and its arguments are
checked.  The fourth index counter is there, and three values are still what a caller that asks for three gets."""
import ctypes as C
import itertools

import pytest

import oracle_bind as ob
from charls_amd import batch, capi, synth

INVALID_ARGUMENT = 101
W, H = 21, 13


@pytest.fixture(scope="module")
def lib():
    return capi.load_product()


def _cases():
    for bits, comps in itertools.product([2, 8, 12, 16], [1, 2, 3, 4]):
        for ilv in ([0] if comps == 1 else [0, 1, 2]):
            for near in (0, 3):
                if near > ((1 << bits) - 1) // 2:
                    continue
                yield bits, comps, ilv, near


CASES = list(_cases())


@pytest.mark.parametrize("bits,comps,ilv,near", CASES, ids=[f"b{b}c{c}i{i}n{n}" for b, c, i, n in CASES])
def test_bound_equals_get_index_size(lib, bits, comps, ilv, near):
    img = synth.frame_numpy(W, H, seed=bits + comps, bits=bits, components=comps, interleaved=ilv != 0)
    jls = ob.encode(img, width=W, height=H, bits_per_sample=bits, component_count=comps, near_lossless=near, interleave_mode=ilv,
                    destination_size=8 * W * H * comps + 4096)
    L = lib._index_fns()
    dec, keep = lib._open(jls)
    try:
        for K in (1, 4, 64, H + 5):
            n = C.c_size_t()
            assert L.charls_amd_jpegls_decoder_get_index_size(dec, K, C.byref(n)) == 0
            assert batch.index_size_bound(W, H, bits, comps, ilv, near, K, lib=lib) == n.value, K
    finally:
        L.charls_jpegls_decoder_destroy(dec)


def test_bound_grows_with_the_points(lib):
    few = batch.index_size_bound(W, H, lines_per_seek_point=H, lib=lib)
    assert few == 72 + 24  # no seek point: the header and one scan record
    assert batch.index_size_bound(W, H, lines_per_seek_point=1, lib=lib) == few + (H - 1) * (2992 + (W + 2 + 7) // 8 * 8 + 24)


def test_arguments_are_checked(lib):
    l = batch._bind(lib)
    p = batch.CodecParams(capi.FrameInfo(W, H, 8, 1), 0, 0, 0, capi.PcParameters(0, 0, 0, 0, 0), 0, 0)
    n = C.c_size_t(7)
    assert l.charls_amd_index_size_bound(C.byref(p), 0, C.byref(n)) == INVALID_ARGUMENT
    assert l.charls_amd_index_size_bound(None, 4, C.byref(n)) == INVALID_ARGUMENT
    assert l.charls_amd_index_size_bound(C.byref(p), 4, None) == INVALID_ARGUMENT
    assert n.value == 7
    with pytest.raises(capi.JpegLSError) as e:
        batch.index_size_bound(W, H, lines_per_seek_point=0, lib=lib)
    assert e.value.errc == INVALID_ARGUMENT


def test_the_fourth_counter(lib):
    l = batch._bind(lib)
    four = (C.c_uint64 * 5)(9, 9, 9, 9, 9)
    assert l.charls_amd_index_counters(four, 5) == 4 and four[4] == 9
    three = (C.c_uint64 * 4)(9, 9, 9, 9)
    assert l.charls_amd_index_counters(three, 3) == 3 and three[3] == 9
    assert list(three[:3]) == list(four[:3])
    assert set(capi.index_counters(lib)) == {"scans_from_points", "intervals", "fallback_scans"}
    assert batch.seek_launches(lib) == four[3]
