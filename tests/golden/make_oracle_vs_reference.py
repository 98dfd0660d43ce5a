"""Writes tests/golden/oracle_vs_reference.json: what THE REFERENCE (oracle/_ref/libcharls_ref.so, built by
`make -C oracle ref`) makes of every case of tests/test_oracle_vs_reference.py -- error code, SHA-256 of the .jls and of
the samples it decodes that .jls to.  The test holds the oracle to these where the reference build is absent.
Usage: python tests/golden/make_oracle_vs_reference.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_oracle_vs_reference as t  # noqa: E402
from charls_amd.capi import CharLSLibrary, JpegLSError  # noqa: E402

REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libcharls_ref.so")


def main():
    ref = CharLSLibrary(REF_LIB)
    random_parameters = {str(chunk): [t.observe(ref.encode, ref.decode, JpegLSError, img, kw) for kw, img in t.random_cases(chunk)]
                         for chunk in range(t.CHUNKS)}
    img = t.boundary_image()
    full = len(ref.encode(img, width=64, height=64))
    boundary = [t.observe(ref.encode, None, JpegLSError, img, dict(width=64, height=64, destination_size=cap))
                for cap in range(full - 8, full + 8)]
    with open(t.GOLDEN_FILE, "w") as f:
        json.dump({"random_parameters": random_parameters, "destination_too_small": {"full_size": full, "observations": boundary}}, f)
        f.write("\n")
    print(t.GOLDEN_FILE, sum(len(v) for v in random_parameters.values()) + len(boundary), "observations")


if __name__ == "__main__":
    main()
