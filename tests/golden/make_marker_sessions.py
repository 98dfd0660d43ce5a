"""Writes tests/golden/marker_sessions.json: what THE REFERENCE (oracle/_ref/libcharls_ref.so, built by `make -C oracle ref`)
makes of every marker session of tests/test_gpu_markers.py -- return codes, size and SHA-256 of the file written, the decoder
session's observations over it and SHA-256 of its samples.  The test holds the GPU library to these where the reference build
did not travel.  Runs on the CPU.
Usage: python tests/golden/make_marker_sessions.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gpu_markers as t  # noqa: E402
from charls_amd import capi, synth  # noqa: E402


def main():
    ref = capi.CharLSLibrary(t.REF_PATH)
    sessions = {}
    for row in t.SESSIONS:
        sessions[row[0]] = {key: t.observe_session(ref, img, **kw)[0] for key, img, kw in t.session_cases(*row)}
    img = synth.frame_numpy(**t.TOO_SMALL_IMAGE)
    full = len(t._encode_session(ref, img, **t.TOO_SMALL_SESSION)[1])
    too_small = {"full_size": full, "observations": [t.observe_too_small(ref, img, size) for size in t.too_small_sizes(full)]}
    with open(t.GOLDEN_FILE, "w") as f:
        json.dump({"sessions": sessions, "too_small": too_small}, f, indent=1)
        f.write("\n")
    print(t.GOLDEN_FILE, sum(len(v) for v in sessions.values()), "sessions")


if __name__ == "__main__":
    main()
