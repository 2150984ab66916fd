#!/usr/bin/env python3
"""Generate tests/golden/map.json: zlib.crc32 of the FIRST decoded picture of every golden clip (the .h4m files of manifest.json)
through five fixed tables -- the identity, inversion, the constant 77, two records of random permutations -- and through the tables of
three rules made of the picture's own histograms -- equalize, stretch 10 / 20 per mille, otsu, each on all three planes -- as
tests/map_ref.py, the plain-Python restatement of include/hvqm4_amd.h, computes them on the oracle's picture: no other module takes part
in the values (the permutations are numpy's, which is data, not arithmetic).  The pictures' SHA-256 are checked against manifest.json on
the way.  Recorded results only; manifest.json is read, never written.  tests/test_map_cpu.py checks every entry against hvqm4_amd.maps.
"""
import hashlib
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from hvqm4_amd.container import parse_header  # noqa: E402
from oracle import bridge  # noqa: E402
from tests import map_ref as ref  # noqa: E402


def _perm(seed):
    rng = np.random.default_rng(1000 + seed)                   # tests/map_cases.perm_table
    return [rng.permutation(256).tolist() for _ in range(3)]


# (label, the three tables)
SETS = [("identity", [list(range(256))] * 3), ("invert", [[255 - v for v in range(256)]] * 3), ("flat77", [[77] * 256] * 3), ("perm0", _perm(0)), ("perm1", _perm(1))]
# (label, (kind, a, b)): the rule of Y, U and V alike
RULES = [("equalize", (ref.EQUALIZE, 0, 0)), ("stretch10_20", (ref.STRETCH, 10, 20)), ("otsu", (ref.OTSU, 0, 0))]


def record(yuv: bytes, geom):
    rec, at = [], 0
    for pw, ph in ref.plane_sizes(geom):
        h = [0] * 256
        for a in yuv[at:at + pw * ph]:
            h[a] += 1
        rec.append(h)
        at += pw * ph
    return rec


def main():
    manifest = json.load(open(os.path.join(HERE, "manifest.json")))
    out = {"generator": "tests/golden/make_map.py",
           "what": "per clip: geometry, per table [label, crc32 of the first picture through it], per rule [label, crc32 of its three tables, crc32 of the picture through them]",
           "clips": {}}
    for name, entry in manifest["clips"].items():
        if "file" not in entry:
            continue
        data = open(os.path.join(HERE, entry["file"]), "rb").read()
        hdr = parse_header(data)
        pic = bridge.oracle_decode(data, 1)[0].tobytes()
        assert hashlib.sha256(pic).hexdigest() == entry["picture_sha256"][0], name
        geom = (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)
        rows = [[label, zlib.crc32(ref.map_picture(pic, geom, t))] for label, t in SETS]
        rec, rules = record(pic, geom), []
        for label, r in RULES:
            t = ref.record_tables(rec, r, r)
            rules.append([label, zlib.crc32(bytes(t[0] + t[1] + t[2])), zlib.crc32(ref.map_picture(pic, geom, t))])
        out["clips"][name] = {"geometry": list(geom), "sets": rows, "rules": rules}
        print(name, geom, flush=True)
    with open(os.path.join(HERE, "map.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote map.json")


if __name__ == "__main__":
    main()
