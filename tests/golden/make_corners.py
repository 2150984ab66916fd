#!/usr/bin/env python3
"""Generate tests/golden/corners.json: for picture 1 of the three golden clips of the three samplings (64 x 48 4:2:0, 48 x 64 4:4:4,
296 x 160 4:2:2), on every plane, under both measures, r in {1, 2, 3} and nms in {0, 1, 3, 7} (threshold 1, k 10 under Harris): K,
rows[Ny] and the CRC-32 of the list, of the mask picture and of the row index, as hvqm4_amd.corners computes them on the oracle's
picture.  (The plain-Python restatement tests/corner_ref.py takes hours on these planes; tests/test_corner_cpu.py holds the module to
it on small planes.)  Records and checksums only; manifest.json is read, never written.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from hvqm4_amd.container import parse_header  # noqa: E402
from oracle import bridge  # noqa: E402

CLIPS = ["crossplane420_64x48", "crossplane444_48x64", "yuv422_296x160"]
PICTURE = 1


def main():
    from tests.corner_cases import fixture_record, fixture_rules as _fixture_rules
    manifest = json.load(open(os.path.join(HERE, "manifest.json")))
    out = {"generator": "tests/golden/make_corners.py", "picture": PICTURE, "fields": ["K", "rows[Ny]", "crc32 points", "crc32 mask", "crc32 rows"],
           "rules": "plane 0 .. 2 x (Harris k 10, min-eigenvalue) x r 1 .. 3 x nms 0, 1, 3, 7; threshold 1", "clips": {}}
    for name in CLIPS:
        data = open(os.path.join(HERE, manifest["clips"][name]["file"]), "rb").read()
        hdr = parse_header(data)
        pic = bridge.oracle_decode(data, PICTURE + 1)[PICTURE].reshape(-1)
        geom = (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)
        out["clips"][name] = [fixture_record(pic, geom, r) for r in _fixture_rules()]
        print(name, geom, flush=True)
    with open(os.path.join(HERE, "corners.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote corners.json")


if __name__ == "__main__":
    main()
