#!/usr/bin/env python3
"""Generate tests/golden/scale.json: zlib.crc32 of the scaled LAST decoded picture of every golden clip (the .h4m files of
manifest.json) at three targets each -- half size (hvqm4_amd.scale.pyramid), fit(w, h, 56, 56), and the same size at 4:2:0 where the
clip is not 4:2:0 already -- as hvqm4_amd.scale.of_picture computes them on the oracle's picture.  The pictures' SHA-256 are checked
against manifest.json on the way.  Recorded results only; manifest.json is read, never written.  tests/test_scale_cpu.py checks every
entry against tests/scale_ref.py (plain Python) as well.
"""
import hashlib
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from hvqm4_amd import scale  # noqa: E402
from hvqm4_amd.container import parse_header  # noqa: E402
from oracle import bridge  # noqa: E402


def targets(w, h, hs, vs):
    """the fixture's targets of a clip: [(label, (w, h, h_samp, v_samp))]"""
    out = [("half", scale.pyramid(w, h, 2)[1] + (hs, vs)), ("fit56", scale.fit(w, h, 56, 56) + (hs, vs))]
    if (hs, vs) != (2, 2):
        out.append(("to420", (w, h, 2, 2)))
    return out


def main():
    manifest = json.load(open(os.path.join(HERE, "manifest.json")))
    out = {"generator": "tests/golden/make_scale.py",
           "what": "per clip: geometry, and per target [label, [w, h, h_samp, v_samp], crc32 of the scaled last picture]", "clips": {}}
    for name, entry in manifest["clips"].items():
        if "file" not in entry:
            continue
        data = open(os.path.join(HERE, entry["file"]), "rb").read()
        hdr = parse_header(data)
        n = len(entry["frame_types"])
        pic = bridge.oracle_decode(data, n)[n - 1]
        assert hashlib.sha256(pic.tobytes()).hexdigest() == entry["picture_sha256"][n - 1], name
        geom = (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)
        rows = []
        for label, dst in targets(*geom):
            scale.plane_sizes(geom, dst)                       # every entry respects the 32x limit
            rows.append([label, list(dst), zlib.crc32(scale.of_picture(pic, geom, dst).tobytes())])
        out["clips"][name] = {"geometry": list(geom), "targets": rows}
        print(name, geom, [r[1] for r in rows])
    with open(os.path.join(HERE, "scale.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote scale.json")


if __name__ == "__main__":
    main()
