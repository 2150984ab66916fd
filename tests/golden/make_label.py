#!/usr/bin/env python3
"""Generate tests/golden/label.json: for the FIRST decoded picture of every golden clip (the .h4m files of manifest.json), binarised by
Otsu's threshold as tests/map_ref.py computes it, the zlib.crc32 of the label map of its Y plane (uint32, little endian) and of its
records (uint64, little endian, every component stored) under the 4- and the 8-neighbourhood, as tests/label_ref.py, the plain-Python
restatement of include/hvqm4_amd.h, computes them: no other module takes part in the values.  The pictures' SHA-256 are checked against
manifest.json on the way.  Recorded results only; manifest.json is read, never written.  tests/test_label_cpu.py checks every entry
against hvqm4_amd.labels.
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
from tests import label_ref  # noqa: E402
from tests import map_ref  # noqa: E402
from tests.golden.make_map import record  # noqa: E402


def main():
    manifest = json.load(open(os.path.join(HERE, "manifest.json")))
    out = {"generator": "tests/golden/make_label.py",
           "what": "per clip: geometry, per connectivity the crc32 of the Y label map and of the records of the first picture's Otsu mask, and K",
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
        row = {"geometry": list(geom)}
        for conn in (4, 8):
            lab, rec = label_ref.label(plane, 255, 255, conn)
            row[str(conn)] = {"labels": zlib.crc32(b"".join(struct.pack(f"<{w}I", *r) for r in lab)),
                              "records": zlib.crc32(b"".join(struct.pack("<8Q", *r) for r in rec)), "K": rec[0][0]}
        out["clips"][name] = row
        print(name, geom, row["4"]["K"], row["8"]["K"], flush=True)
    with open(os.path.join(HERE, "label.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote label.json")


if __name__ == "__main__":
    main()
