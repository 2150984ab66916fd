#!/usr/bin/env python3
"""Generate tests/golden/distance.json: for the FIRST decoded picture of every golden clip (the .h4m files of manifest.json), binarised by
Otsu's threshold as tests/map_ref.py computes it, the zlib.crc32 of the distance map of its Y plane (uint32, little endian) under
EUCLID2 without the border and under CHESS with it, and of the picture that an opening by the disc of radius 3 leaves, as
tests/distance_ref.py, the plain-Python restatement of include/hvqm4_amd.h, computes them (distance_by_rows, which
tests/test_distance_cpu.py holds equal to the brute force; the discs by their definition): no other module takes part in the values.
The pictures' SHA-256 are checked against manifest.json on the way.  Recorded results only; manifest.json is read, never written.
tests/test_distance_cpu.py checks every entry against hvqm4_amd.distance.
"""
import hashlib
import json
import os
import struct
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from hvqm4_amd.container import parse_header  # noqa: E402
from oracle import bridge  # noqa: E402
from tests import distance_ref  # noqa: E402
from tests import map_ref  # noqa: E402
from tests.golden.make_map import record  # noqa: E402


def main():
    manifest = json.load(open(os.path.join(HERE, "manifest.json")))
    out = {"generator": "tests/golden/make_distance.py",
           "what": "per clip: geometry, the crc32 of the Y distance map of the first picture's Otsu mask (euclid2; chess with the border) and of its opening by the disc of radius 3",
           "clips": {}}
    otsu = (map_ref.OTSU, 0, 0)
    for name, entry in manifest["clips"].items():
        if "file" not in entry:
            continue
        data = open(os.path.join(HERE, entry["file"]), "rb").read()
        hdr = parse_header(data)
        pic = bridge.oracle_decode(data, 1)[0].tobytes()
        assert hashlib.sha256(pic).hexdigest() == entry["picture_sha256"][0], name
        geom = (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)
        mask = map_ref.map_picture(pic, geom, map_ref.record_tables(record(pic, geom), otsu, otsu))
        w, h = geom[:2]
        plane = [list(mask[y * w:(y + 1) * w]) for y in range(h)]

        def crc(rows):
            return zlib.crc32(b"".join(struct.pack(f"<{w}I", *r) for r in rows))
        opened = distance_ref.dilate_disc(distance_ref.erode_disc(plane, 3), 3)
        row = {"geometry": list(geom),
               "euclid2": crc(distance_ref.distance_by_rows(plane, 255, 255, distance_ref.EUCLID2, 0)),
               "chess_border": crc(distance_ref.distance_by_rows(plane, 255, 255, distance_ref.CHESS, 1)),
               "opening3": zlib.crc32(b"".join(bytes(r) for r in opened) + bytes([128]) * (len(mask) - w * h))}
        out["clips"][name] = row
        print(name, geom, row, flush=True)
    with open(os.path.join(HERE, "distance.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote distance.json")


if __name__ == "__main__":
    main()
