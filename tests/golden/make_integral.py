#!/usr/bin/env python3
"""Generate tests/golden/integral.json: for the FIRST decoded picture of every golden clip (the .h4m files of manifest.json), the
zlib.crc32 of the summed-area tables of its Y plane (S uint32, Q uint64, little endian) and of the pictures that three window rules
leave -- the mean over radii (7, 3), the deviation over radius 2, and the threshold over radius 5 with c = 7 and k = 51 --, as
tests/integral_ref.py, the plain-Python restatement of include/hvqm4_amd.h, computes them (the tables by the recurrence, which
tests/test_integral_cpu.py holds equal to the slow way; the windows by visiting every sample): no other module takes part in the values.
The pictures' SHA-256 are checked against manifest.json on the way.  Recorded results only; manifest.json is read, never written.
tests/test_integral_cpu.py checks every entry against hvqm4_amd.integral.
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
from tests import integral_ref  # noqa: E402

# name -> (mode, rx, ry, k, c, invert)
WINDOWS = {"mean_7_3": (0, 7, 3, 0, 0, 0), "deviation_2": (1, 2, 2, 0, 0, 0), "adaptive_5_c7_k51": (2, 5, 5, 51, 7, 0)}


def main():
    manifest = json.load(open(os.path.join(HERE, "manifest.json")))
    out = {"generator": "tests/golden/make_integral.py",
           "what": "per clip: geometry, the crc32 of the tables S and Q of the first picture's Y plane and of the pictures three window rules leave",
           "windows": {k: list(v) for k, v in WINDOWS.items()}, "clips": {}}
    for name, entry in manifest["clips"].items():
        if "file" not in entry:
            continue
        data = open(os.path.join(HERE, entry["file"]), "rb").read()
        hdr = parse_header(data)
        pic = bridge.oracle_decode(data, 1)[0].tobytes()
        assert hashlib.sha256(pic).hexdigest() == entry["picture_sha256"][0], name
        geom = (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)
        w, h = geom[:2]
        plane = [list(pic[y * w:(y + 1) * w]) for y in range(h)]
        S, Q = integral_ref.tables_by_rows(plane)
        row = {"geometry": list(geom), "sums": zlib.crc32(b"".join(struct.pack(f"<{w}I", *r) for r in S)), "squares": zlib.crc32(b"".join(struct.pack(f"<{w}Q", *r) for r in Q))}
        for key, (mode, rx, ry, k, c, inv) in WINDOWS.items():
            y = integral_ref.window(plane, mode, rx, ry, k, c, inv)
            row[key] = zlib.crc32(b"".join(bytes(r) for r in y) + bytes([128]) * (len(pic) - w * h))
        out["clips"][name] = row
        print(name, geom, row, flush=True)
    with open(os.path.join(HERE, "integral.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote integral.json")


if __name__ == "__main__":
    main()
