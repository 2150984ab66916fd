#!/usr/bin/env python3
"""Generate tests/golden/warp.json: zlib.crc32 of the warped LAST decoded picture of every golden clip (the .h4m files of manifest.json)
under three warps each -- rotate(7) about the centre with the constant border, rotate90(1) into the turned geometry, and zoom(3/4) about
the centre with the replicate border -- as hvqm4_amd.warp.of_picture computes them on the oracle's picture.  The pictures' SHA-256 are
checked against manifest.json on the way.  Recorded results only; manifest.json is read, never written.  tests/test_warp_cpu.py checks
every entry against tests/warp_ref.py (plain Python) as well.
"""
import hashlib
import json
import os
import sys
import zlib
from fractions import Fraction

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from hvqm4_amd import warp  # noqa: E402
from hvqm4_amd.container import parse_header  # noqa: E402
from oracle import bridge  # noqa: E402


def fixture_warps(geom):
    """the fixture's warps of a clip of geometry geom: [(label, Warp, target geometry)]"""
    w, h, hs, vs = geom
    turn, (tw, th) = warp.rotate90(1, w, h)
    return [("rotate7_constant", warp.with_border(warp.rotate(7, w, h), warp.CONSTANT), geom),
            ("rotate90", turn, (tw, th, hs, vs)),
            ("zoom3/4_replicate", warp.zoom(Fraction(3, 4), centre=(Fraction(w, 2), Fraction(h, 2))), geom)]


def main():
    manifest = json.load(open(os.path.join(HERE, "manifest.json")))
    out = {"generator": "tests/golden/make_warp.py",
           "what": "per clip: geometry, and per warp [label, target geometry, crc32 of the warped last picture]", "clips": {}}
    for name, entry in manifest["clips"].items():
        if "file" not in entry:
            continue
        data = open(os.path.join(HERE, entry["file"]), "rb").read()
        hdr = parse_header(data)
        n = len(entry["frame_types"])
        pic = bridge.oracle_decode(data, n)[n - 1]
        assert hashlib.sha256(pic.tobytes()).hexdigest() == entry["picture_sha256"][n - 1], name
        geom = (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)
        rows = [[label, list(tg), zlib.crc32(warp.of_picture(pic, geom, w, tg).tobytes())] for label, w, tg in fixture_warps(geom)]
        out["clips"][name] = {"geometry": list(geom), "warps": rows}
        print(name, geom)
    with open(os.path.join(HERE, "warp.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote warp.json")


if __name__ == "__main__":
    main()
