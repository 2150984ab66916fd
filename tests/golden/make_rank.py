#!/usr/bin/env python3
"""Generate tests/golden/rank.json: zlib.crc32 of the FIRST decoded picture of every golden clip (the .h4m files of manifest.json)
through five rank parameter sets -- erode 1, dilate (3, 1), range 2, median 3 x 3, median 5 x 5, each on all three planes -- as
tests/rank_ref.py, the plain-Python restatement of include/hvqm4_amd.h, computes them on the oracle's picture: no other module takes
part in the values.  The pictures' SHA-256 are checked against manifest.json on the way.  Recorded results only; manifest.json is read,
never written.  tests/test_rank_cpu.py checks every entry against hvqm4_amd.rank (numpy) and, for the small clips, the reference again.
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
from tests import rank_ref as ref  # noqa: E402

# (label, (op, rx, ry)): the plane operation of Y, U and V alike
SETS = [("erode1", (ref.MIN, 1, 1)), ("dilate3x1", (ref.MAX, 3, 1)), ("range2", (ref.RANGE, 2, 2)), ("median3", (ref.MEDIAN, 1, 1)),
        ("median5", (ref.MEDIAN, 2, 2))]


def main():
    manifest = json.load(open(os.path.join(HERE, "manifest.json")))
    out = {"generator": "tests/golden/make_rank.py",
           "what": "per clip: geometry, and per parameter set [label, crc32 of the first picture through it]", "clips": {}}
    for name, entry in manifest["clips"].items():
        if "file" not in entry:
            continue
        data = open(os.path.join(HERE, entry["file"]), "rb").read()
        hdr = parse_header(data)
        pic = bridge.oracle_decode(data, 1)[0]
        assert hashlib.sha256(pic.tobytes()).hexdigest() == entry["picture_sha256"][0], name
        geom = (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)
        rows = [[label, zlib.crc32(ref.rank_picture(pic.tobytes(), geom, p, p))] for label, p in SETS]
        out["clips"][name] = {"geometry": list(geom), "sets": rows}
        print(name, geom, flush=True)
    with open(os.path.join(HERE, "rank.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote rank.json")


if __name__ == "__main__":
    main()
