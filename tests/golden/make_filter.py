#!/usr/bin/env python3
"""Generate tests/golden/filter.json: zlib.crc32 of the filtered LAST decoded picture of every golden clip (the .h4m files of
manifest.json) under three filters each -- a Gaussian of sigma 1.5 with chroma_for the clip's sampling, unsharp(1.0, 1/2) on luma only
and the Sobel gradient magnitude on luma only -- as hvqm4_amd.filters.of_picture computes them on the oracle's picture.  The pictures'
SHA-256 are checked against manifest.json on the way.  Recorded results only; manifest.json is read, never written.
tests/test_filters_cpu.py checks every entry against tests/filter_ref.py (plain Python) as well.
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

from hvqm4_amd import filters  # noqa: E402
from hvqm4_amd.container import parse_header  # noqa: E402
from oracle import bridge  # noqa: E402


def fixture_filters(hs, vs):
    """the fixture's filters of a clip of sampling (hs, vs): [(label, Filter)]"""
    return [("gauss1.5", filters.chroma_for(filters.gaussian(1.5), hs, vs)),
            ("unsharp1.0_1/2", filters.luma_only(filters.unsharp(1.0, Fraction(1, 2)))),
            ("sobelmag", filters.luma_only(filters.gradient_magnitude("sobel")))]


def main():
    manifest = json.load(open(os.path.join(HERE, "manifest.json")))
    out = {"generator": "tests/golden/make_filter.py",
           "what": "per clip: geometry, and per filter [label, crc32 of the filtered last picture]", "clips": {}}
    for name, entry in manifest["clips"].items():
        if "file" not in entry:
            continue
        data = open(os.path.join(HERE, entry["file"]), "rb").read()
        hdr = parse_header(data)
        n = len(entry["frame_types"])
        pic = bridge.oracle_decode(data, n)[n - 1]
        assert hashlib.sha256(pic.tobytes()).hexdigest() == entry["picture_sha256"][n - 1], name
        geom = (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)
        rows = [[label, zlib.crc32(filters.of_picture(pic, geom, f).tobytes())] for label, f in fixture_filters(*geom[2:])]
        out["clips"][name] = {"geometry": list(geom), "filters": rows}
        print(name, geom)
    with open(os.path.join(HERE, "filter.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote filter.json")


if __name__ == "__main__":
    main()
