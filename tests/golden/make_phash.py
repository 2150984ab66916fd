#!/usr/bin/env python3
"""Generate tests/golden/phash.json from the UNMODIFIED reference decoder.

Runs only in the build container (needs oracle/_ref/libh4mref.so, as make_golden.py and make_checksums.py do).  For every clip of
manifest.json it stores, per picture in decode order, the record of hvq_picture_hashes -- ahash, dhash, phash, sum_y, unsigned, the
hashes as 16 hex digits -- as tests/phash_ref.py (plain loops over Python integers) computes it on the reference's picture.  The
pictures' SHA-256 are checked against manifest.json on the way, so the fixtures describe the same pictures.  Recorded results only;
manifest.json is read, never written.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import bridge  # noqa: E402
from tests import clips  # noqa: E402
from tests.phash_ref import picture_reference  # noqa: E402


def main():
    if not bridge.have_ref():
        raise SystemExit("oracle/_ref/libh4mref.so missing: run `make -C oracle ref` where the reference exists")
    manifest = json.load(open(os.path.join(HERE, "manifest.json")))
    out = {"generator": "tests/golden/make_phash.py",
           "what": "per clip and picture (decode order): ahash, dhash, phash (16 hex digits each) and sum_y of the reference's picture, by tests/phash_ref.py",
           "clips": {}}
    catalogue = {name: (name, cfg) for name, cfg in clips.SMALL + clips.MEDIUM + clips.C4_SHARE + clips.SHAPES}
    for name, entry in manifest["clips"].items():
        clip = clips.get(catalogue[name])
        assert hashlib.sha256(clip.data).hexdigest() == entry["clip_sha256"], name
        pics, _probe = bridge.ref_decode(clip.data, clip.n_pictures)
        assert [hashlib.sha256(p.tobytes()).hexdigest() for p in pics] == entry["picture_sha256"], name
        rows = []
        for p in pics:
            a, d, ph, s = picture_reference(p.tobytes(), clip.width, clip.height)
            rows.append([f"{a:016x}", f"{d:016x}", f"{ph:016x}", s])
        out["clips"][name] = rows
        print(name, clip.n_pictures, "pictures")
    with open(os.path.join(HERE, "phash.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote phash.json")


if __name__ == "__main__":
    main()
