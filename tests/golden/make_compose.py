#!/usr/bin/env python3
"""Generate tests/golden/compose.json: zlib.crc32 of pictures composed of the FIRST and the LAST decoded picture of every golden clip (the
.h4m files of manifest.json) under the recipes of tests/compose_cases.fixture_recipes -- a difference, a cross-fade, a translucent
overlay at an odd chroma offset, an inset and a side-by-side -- as tests/compose_ref.py (plain Python, the restatement of
include/hvqm4_amd.h) computes them on the oracle's pictures.  The pictures' SHA-256 are checked against manifest.json on the way.
Recorded results only; manifest.json is read, never written.  tests/test_compose_cpu.py checks every entry against
hvqm4_amd.compose.of_pictures as well.
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
from tests import compose_ref as ref  # noqa: E402
from tests.compose_cases import fixture_recipes  # noqa: E402


def main():
    manifest = json.load(open(os.path.join(HERE, "manifest.json")))
    out = {"generator": "tests/golden/make_compose.py",
           "what": "per clip: geometry, and per recipe [label, target geometry, crc32 of the picture composed of the clip's first and last]", "clips": {}}
    for name, entry in manifest["clips"].items():
        if "file" not in entry:
            continue
        data = open(os.path.join(HERE, entry["file"]), "rb").read()
        hdr = parse_header(data)
        n = len(entry["frame_types"])
        pics = bridge.oracle_decode(data, n)
        for k in (0, n - 1):
            assert hashlib.sha256(pics[k].tobytes()).hexdigest() == entry["picture_sha256"][k], name
        geom = (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)
        pair = [pics[0].tobytes(), pics[n - 1].tobytes()]
        rows = [[label, list(t.geometry()), zlib.crc32(ref.compose_picture(pair, [geom, geom], ref.as_ref(t)))] for label, t in fixture_recipes(geom)]
        out["clips"][name] = {"geometry": list(geom), "recipes": rows}
        print(name, geom)
    with open(os.path.join(HERE, "compose.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote compose.json")


if __name__ == "__main__":
    main()
