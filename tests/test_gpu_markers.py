"""Marker fidelity END TO END on the GPU box: the same C-ABI session -- SPIFF header and directory
entries, COM, APPn, a mapping table, every encoding option, then a real encode -- is run on libcharls_amd.so and on the
reference (oracle/_ref/libcharls_ref.so, the checker) and must give the same bytes; the result is decoded by both with
comment / application-data callbacks, SPIFF and mapping-table queries, and every observation must agree.  What the
reference observes is stored in tests/golden/marker_sessions.json, so the comparison holds where oracle/_ref did not
travel; where it did, the reference is run live as well and must still give what is stored.  Also replays
tests/abi_scripts.py on the GPU box, where the branches that code a scan really code it.

Reference: src/jpeg_stream_writer.cpp:38-227, src/jpeg_stream_reader.cpp:87-189, test/jpeg_stream_writer_test.cpp,
test/charls_jpegls_encoder_test.cpp, test/charls_jpegls_decoder_test.cpp."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import abi_scripts as S
import common
from charls_amd import capi, synth
from charls_amd.capi import FrameInfo, MappingTableInfo, PcParameters, SpiffHeader

pytestmark = pytest.mark.gpu

REF_PATH = os.path.join(common.ROOT, "oracle", "_ref", "libcharls_ref.so")
GOLDEN_FILE = os.path.join(common.GOLDEN, "marker_sessions.json")


@pytest.fixture(scope="module")
def lib():
    L = capi.load_product()
    assert L.lib.charls_amd_device_status() == 0, "GPU box without a usable device: the product must not fall back"
    return L


@pytest.fixture(scope="module")
def ref():
    """The live reference where oracle/_ref travelled, None elsewhere: what it makes of every session here is stored in
    tests/golden/marker_sessions.json (tests/golden/make_marker_sessions.py) and stands in for it."""
    return capi.CharLSLibrary(REF_PATH) if os.path.exists(REF_PATH) else None


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


def _buf(data: bytes):
    return (C.c_ubyte * max(1, len(data))).from_buffer_copy(data if data else b"\0")


def _encode_session(L, img, *, bits, comps, ilv, near, xform, options, table_id, spiff, destination_size=None):
    """One scripted encoder session; returns (list of return codes, bytes written)."""
    l, rc = L.lib, []
    h, w = (img.shape[1], img.shape[2]) if (comps > 1 and ilv == 0) else (img.shape[0], img.shape[1])
    e = l.charls_jpegls_encoder_create()
    fi = FrameInfo(w, h, bits, comps)
    rc.append(l.charls_jpegls_encoder_set_frame_info(e, C.byref(fi)))
    rc.append(l.charls_jpegls_encoder_set_near_lossless(e, near))
    rc.append(l.charls_jpegls_encoder_set_interleave_mode(e, ilv))
    rc.append(l.charls_jpegls_encoder_set_color_transformation(e, xform))
    rc.append(l.charls_jpegls_encoder_set_encoding_options(e, options))
    if table_id:
        rc.append(l.charls_jpegls_encoder_set_mapping_table_id(e, 0, table_id))
    n = C.c_size_t()
    rc.append(l.charls_jpegls_encoder_get_estimated_destination_size(e, C.byref(n)))
    size = destination_size if destination_size is not None else n.value + 4096
    dst = (C.c_ubyte * size)()
    rc.append(l.charls_jpegls_encoder_set_destination_buffer(e, dst, size))
    if spiff == "standard":
        rc.append(l.charls_jpegls_encoder_write_standard_spiff_header(e, 8 if comps == 1 else 10, 1, 96, 72))
    elif spiff == "custom":
        sh = SpiffHeader(0, comps, h, w, 8 if comps == 1 else 10, bits, 5, 2, 300, 600)
        rc.append(l.charls_jpegls_encoder_write_spiff_header(e, C.byref(sh)))
    if spiff:
        entry = bytes(range(1, 30))
        rc.append(l.charls_jpegls_encoder_write_spiff_entry(e, 5, _buf(entry), len(entry)))
        rc.append(l.charls_jpegls_encoder_write_spiff_entry(e, 0x10, _buf(b""), 0))
        rc.append(l.charls_jpegls_encoder_write_spiff_end_of_directory_entry(e))
    com = b"coded on the GPU\0"
    rc.append(l.charls_jpegls_encoder_write_comment(e, _buf(com), len(com)))
    rc.append(l.charls_jpegls_encoder_write_comment(e, None, 0))
    app = bytes([7, 0, 255, 255, 3])
    rc.append(l.charls_jpegls_encoder_write_application_data(e, 12, _buf(app), len(app)))
    rc.append(l.charls_jpegls_encoder_write_application_data(e, 0, None, 0))
    if table_id:
        table = bytes((7 * i + 3) & 0xFF for i in range(3 * (1 << min(bits, 8))))
        rc.append(l.charls_jpegls_encoder_write_mapping_table(e, table_id, 3, _buf(table), len(table)))
    raw = np.ascontiguousarray(img).tobytes()
    rc.append(l.charls_jpegls_encoder_encode_from_buffer(e, _buf(raw), len(raw), 0))
    rc.append(l.charls_jpegls_encoder_get_bytes_written(e, C.byref(n)))
    rc.append(l.charls_jpegls_encoder_write_comment(e, _buf(com), len(com)))  # after the image: invalid_operation
    data = bytes(dst[:n.value])
    l.charls_jpegls_encoder_destroy(e)
    return rc, data


def _decode_session(L, data):
    """One scripted decoder session over a complete file; returns the observations."""
    l, obs = L.lib, []
    seen = []
    CB1 = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p)
    CB2 = C.CFUNCTYPE(C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p)

    def on_comment(p, n, ctx):
        seen.append(["com", n, bytes((C.c_ubyte * n).from_address(p)).hex() if n else "", ctx])
        return 0

    def on_app(i, p, n, ctx):
        seen.append(["app", i, n, bytes((C.c_ubyte * n).from_address(p)).hex() if n else ""])
        return 0

    c1, c2 = CB1(on_comment), CB2(on_app)
    d = l.charls_jpegls_decoder_create()
    src = _buf(data)
    obs.append(l.charls_jpegls_decoder_set_source_buffer(d, src, len(data)))
    obs.append(l.charls_jpegls_decoder_at_comment(d, c1, 77))
    obs.append(l.charls_jpegls_decoder_at_application_data(d, c2, None))
    sh, found = SpiffHeader(), C.c_int32(-1)
    obs.append(l.charls_jpegls_decoder_read_spiff_header(d, C.byref(sh), C.byref(found)))
    obs.append(found.value)
    if found.value == 1:
        obs.append([getattr(sh, f[0]) for f in SpiffHeader._fields_])
    obs.append(l.charls_jpegls_decoder_read_header(d))
    fi, pc, i32, sz = FrameInfo(), PcParameters(), C.c_int32(), C.c_size_t()
    obs.append(l.charls_jpegls_decoder_get_frame_info(d, C.byref(fi)))
    obs.append([fi.width, fi.height, fi.bits_per_sample, fi.component_count])
    obs.append(l.charls_jpegls_decoder_get_preset_coding_parameters(d, 0, C.byref(pc)))
    obs.append([pc.maximum_sample_value, pc.threshold1, pc.threshold2, pc.threshold3, pc.reset_value])
    obs.append(l.charls_jpegls_decoder_get_color_transformation(d, C.byref(i32)))
    obs.append(i32.value)
    obs.append(l.charls_decoder_get_mapping_table_id(d, 0, C.byref(i32)))
    obs.append(i32.value)
    obs.append(l.charls_jpegls_decoder_get_destination_size(d, 0, C.byref(sz)))
    obs.append(sz.value)
    out = (C.c_ubyte * sz.value)()
    obs.append(l.charls_jpegls_decoder_decode_to_buffer(d, out, sz.value, 0))
    obs.append(hashlib.sha256(bytes(out)).hexdigest())
    obs.append(l.charls_decoder_get_compressed_data_format(d, C.byref(i32)))
    obs.append(i32.value)
    obs.append(l.charls_decoder_get_mapping_table_count(d, C.byref(i32)))
    count = i32.value
    obs.append(count)
    mt = MappingTableInfo()
    for idx in range(count):
        obs.append(l.charls_decoder_get_mapping_table_info(d, idx, C.byref(mt)))
        obs.append([mt.table_id, mt.entry_size, mt.data_size])
        buf = (C.c_ubyte * max(1, mt.data_size))()
        obs.append(l.charls_decoder_get_mapping_table_data(d, idx, buf, mt.data_size))
        obs.append(hashlib.sha256(bytes(buf)).hexdigest())
    obs.append(l.charls_jpegls_decoder_decode_to_buffer(d, out, sz.value, 0))  # twice: invalid_operation
    obs.append(seen)
    l.charls_jpegls_decoder_destroy(d)
    return json.loads(json.dumps(obs)), bytes(out)


SESSIONS = [
    # name, bits, comps, ilv, near, xform, options, table id, spiff
    ("gray8_everything", 8, 1, 0, 0, 0, 1 | 2, 3, "standard"),
    ("gray16_jai_pc", 16, 1, 0, 0, 0, 1 | 2 | 4, 0, "custom"),
    ("gray12_jai_pc_near", 12, 1, 0, 2, 0, 4, 0, None),
    ("rgb8_sample_hp1", 8, 3, 2, 0, 1, 1, 0, "standard"),
    ("rgb8_planar_tables", 8, 3, 0, 0, 0, 1 | 2, 9, "standard"),
    ("rgb8_line_near3", 8, 3, 1, 3, 0, 2, 0, None),
]


def session_cases(name, bits, comps, ilv, near, xform, options, table_id, spiff):
    """(key, image, session arguments) of one row of SESSIONS; odd sizes: the even-size option pads some of them."""
    for w, h in ((37, 23), (64, 40)):
        img = synth.frame_numpy(w, h, seed=len(name) + w, bits=bits, components=comps, kind="mixed", interleaved=(ilv != 0))
        yield f"{w}x{h}", img, dict(bits=bits, comps=comps, ilv=ilv, near=near, xform=xform, options=options, table_id=table_id,
                                    spiff=spiff)


def observe_session(L, img, **kw):
    """The encoder session and the decoder session over what it wrote, as stored: (observations, bytes written, samples)."""
    rc, data = _encode_session(L, img, **kw)
    obs, px = _decode_session(L, data)
    return {"rc": rc, "jls_size": len(data), "jls_sha256": common.sha(data), "obs": obs, "px_sha256": common.sha(px)}, data, px


TOO_SMALL_IMAGE = dict(width=48, height=31, seed=5, bits=8, kind="mixed")
TOO_SMALL_SESSION = dict(bits=8, comps=1, ilv=0, near=0, xform=0, options=1 | 2, table_id=2, spiff="standard")


def too_small_sizes(full):
    return (full, full - 1, full - 2, full // 2, 60)


def observe_too_small(L, img, size):
    rc, data = _encode_session(L, img, destination_size=size, **TOO_SMALL_SESSION)
    return {"rc": rc, "jls_sha256": common.sha(data) if rc[-3] == 0 else None}


@pytest.mark.parametrize("name,bits,comps,ilv,near,xform,options,table_id,spiff", SESSIONS, ids=[s[0] for s in SESSIONS])
def test_full_marker_session_matches_the_reference(lib, ref, golden, name, bits, comps, ilv, near, xform, options, table_id, spiff):
    for key, img, kw in session_cases(name, bits, comps, ilv, near, xform, options, table_id, spiff):
        want = golden["sessions"][name][key]
        if ref is not None:
            assert observe_session(ref, img, **kw)[0] == want, (name, key)  # the stored observations are still the reference's
        got, data_gpu, px_gpu = observe_session(lib, img, **kw)
        for k in ("rc", "jls_size", "jls_sha256", "obs", "px_sha256"):
            assert got[k] == want[k], (name, key, k)
        if options & 1:
            assert len(data_gpu) % 2 == 0
        if near == 0:
            assert px_gpu == np.ascontiguousarray(img).tobytes()


def test_marker_session_with_a_destination_that_is_too_small(lib, ref, golden):
    """The exact boundary through the whole container: one byte less than the file fails with the reference's code."""
    img = synth.frame_numpy(**TOO_SMALL_IMAGE)
    full = golden["too_small"]["full_size"]
    if ref is not None:
        assert len(_encode_session(ref, img, **TOO_SMALL_SESSION)[1]) == full
    sizes = too_small_sizes(full)
    assert len(golden["too_small"]["observations"]) == len(sizes)
    for size, want in zip(sizes, golden["too_small"]["observations"]):
        if ref is not None:
            assert observe_too_small(ref, img, size) == want, size
        assert observe_too_small(lib, img, size) == want, size


@pytest.mark.parametrize("script", [f.__name__ for f in S.SCRIPTS])
def test_abi_script_replay_on_the_gpu_box(lib, script):
    """tests/test_host_facade.py's replay with a GPU behind the library: the observations recorded from the reference
    hold in full, including the steps whose return code is that of a scan actually coded."""
    with open(os.path.join(common.GOLDEN, "abi_observations.json")) as f:
        want = json.load(f)[script]
    got = json.loads(json.dumps(getattr(S, script)(lib)))
    if isinstance(want, dict):
        for k in want:
            assert got[k] == want[k], k
    else:
        assert got == want
