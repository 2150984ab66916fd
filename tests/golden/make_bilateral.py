#!/usr/bin/env python3
"""Generate tests/golden/bilateral.json: zlib.crc32 of the FIRST decoded picture of every golden clip (the .h4m files of manifest.json)
through the five shared parameter sets of tests/bilateral_cases.py (FIVE: a Gaussian 1.5 / 12, a sigma filter, a box, a disc, a
luma-only set), unguided, as tests/bilateral_ref.py, the plain-Python restatement of include/hvqm4_amd.h, computes them on the oracle's
picture: the builders of hvqm4_amd.bilateral supply the tables, no other module takes part in the arithmetic.  The pictures' SHA-256
are checked against manifest.json on the way.  Recorded results only; manifest.json is read, never written.
tests/test_bilateral_cpu.py checks every entry against hvqm4_amd.bilateral (numpy) and, for the small clips, the reference again.
Takes a few minutes.
"""
import hashlib
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from hvqm4_amd.container import parse_header  # noqa: E402
from oracle import bridge  # noqa: E402
from tests import bilateral_cases as cases  # noqa: E402
from tests import bilateral_ref as ref  # noqa: E402

SETS = [label for label, _b in cases.FIVE]


def main():
    manifest = json.load(open(os.path.join(HERE, "manifest.json")))
    out = {"generator": "tests/golden/make_bilateral.py",
           "what": "per clip: geometry, and per parameter set [label, crc32 of the first picture through it]", "clips": {}}
    for name, entry in manifest["clips"].items():
        if "file" not in entry:
            continue
        data = open(os.path.join(HERE, entry["file"]), "rb").read()
        hdr = parse_header(data)
        pic = bridge.oracle_decode(data, 1)[0]
        assert hashlib.sha256(pic.tobytes()).hexdigest() == entry["picture_sha256"][0], name
        geom = (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)
        rows = [[label, zlib.crc32(ref.bilateral_picture(pic.tobytes(), geom, ref.as_ref(b.luma), ref.as_ref(b.chroma)))] for label, b in cases.FIVE]
        out["clips"][name] = {"geometry": list(geom), "sets": rows}
        print(name, geom, flush=True)
    with open(os.path.join(HERE, "bilateral.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote bilateral.json")


if __name__ == "__main__":
    main()
