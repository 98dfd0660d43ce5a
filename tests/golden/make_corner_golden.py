"""Writes tests/golden/corners.json: what THE REFERENCE (oracle/_ref/libcharls_ref.so, built by `make -C oracle ref`) makes
of every frame of the corner corpus (tests/corners.py) -- name, coding parameters, size and SHA-256 of the .jls, SHA-256 of
the samples it decodes that .jls to.  tests/test_corner_census_cpu.py holds the oracle to these where the reference build is
absent.  Usage: python tests/golden/make_corner_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import common  # noqa: E402
import corners  # noqa: E402
from charls_amd.capi import CharLSLibrary  # noqa: E402

REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libcharls_ref.so")
GOLDEN_FILE = os.path.join(common.GOLDEN, "corners.json")


def observe(codec, c):
    """What one codec (an object with encode / decode, as CharLSLibrary) makes of one corner frame."""
    jls = codec.encode(c.img, destination_size=8 * c.img.nbytes + 4096, **c.kw())
    return dict(name=c.name, parameters=c.params(), jls_size=len(jls), jls_sha256=common.sha(jls),
                pixels_sha256=common.sha(codec.decode(jls)[1].tobytes()))


def main():
    ref = CharLSLibrary(REF_LIB)
    rows = [observe(ref, c) for c in corners.CORPUS.values()]
    with open(GOLDEN_FILE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(GOLDEN_FILE, len(rows), "frames")


if __name__ == "__main__":
    main()
