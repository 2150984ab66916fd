#!/usr/bin/env python3
"""Generate tests/golden/checksums.json from the UNMODIFIED reference decoder.

Runs only in the build container (needs oracle/_ref/libh4mref.so, as make_golden.py does).  For every clip of manifest.json it stores,
per picture in decode order, the eight values of hvq_picture_checksums as zlib computes them on the reference's picture: crc32 of Y, U,
V and of the picture, adler32 of Y, U, V and of the picture.  The pictures' SHA-256 are checked against manifest.json on the way, so the
two fixtures describe the same pictures.  Recorded results only; manifest.json is read, never written.
"""
import hashlib
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import bridge  # noqa: E402
from tests import clips  # noqa: E402


def eight(pic, sizes):
    data = pic.tobytes()
    assert len(data) == sum(sizes), (len(data), sizes)
    at, planes = 0, []
    for n in sizes:
        planes.append(data[at:at + n])
        at += n
    return [zlib.crc32(p) for p in planes] + [zlib.crc32(data)] + [zlib.adler32(p) for p in planes] + [zlib.adler32(data)]


def main():
    if not bridge.have_ref():
        raise SystemExit("oracle/_ref/libh4mref.so missing: run `make -C oracle ref` where the reference exists")
    manifest = json.load(open(os.path.join(HERE, "manifest.json")))
    out = {"generator": "tests/golden/make_checksums.py",
           "what": "per clip and picture (decode order): crc32 of Y, U, V, picture, adler32 of Y, U, V, picture (zlib) of the reference's picture",
           "clips": {}}
    catalogue = {name: (name, cfg) for name, cfg in clips.SMALL + clips.MEDIUM + clips.C4_SHARE + clips.SHAPES}
    for name, entry in manifest["clips"].items():
        clip = clips.get(catalogue[name])
        assert hashlib.sha256(clip.data).hexdigest() == entry["clip_sha256"], name
        pics, _probe = bridge.ref_decode(clip.data, clip.n_pictures)
        assert [hashlib.sha256(p.tobytes()).hexdigest() for p in pics] == entry["picture_sha256"], name
        c = (clip.width >> int(clip.samp == 2)) * (clip.height >> int(clip.samp_v == 2))
        out["clips"][name] = [eight(p, (clip.width * clip.height, c, c)) for p in pics]
        print(name, clip.n_pictures, "pictures")
    with open(os.path.join(HERE, "checksums.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote checksums.json")


if __name__ == "__main__":
    main()
