"""GPU: blocks stored from the registers of their owner lanes (hvq_recon_inline_kernel, phase C) and the items' block column in LDS.

Small clips through the batched path against the CPU oracle, once per forced workgroup shape, each shape in a child process of its own
(HVQM4_AMD_TILES_PER_WG is read once per process).  The clips are the ones whose geometry or content reaches the places the store path
and the item column can go wrong:

  ragged24x40        rows of 6 and 3 blocks: a wave's lanes wrap several rows, the last wave is mostly invalid
  ip8                one block row; chroma planes of a single block
  portrait152x280    luma 38 blocks wide; planes with an odd number of tiles: a two-tile workgroup with one live tile
  literals96x96      owners filled from the staged pool behind barrier 1
  bigscalars64x64, gop64x48_13   MC-residual items (the MC block passes through the item's column), both half-sample rules, B pictures
                     (non-temporal stores)
  yuv444_64x48, yuv422_64x48     chroma geometry
  pselfref64x48_15   the destination is the side buffer
  qvga_13            320x240, rows of 80 and 40 blocks, 56-75 items in the fullest tile of every picture: with two tiles forced its P and B
                     pictures run the instantiations of the dense levels (accumulators for 128 and 160 items, seven workgroups per CU),
                     which store four rows from registers on rows that are multiples of four blocks; the small clips run the
                     instantiations of the sparse levels, which regroup such rows into 16-byte pieces first

The children print every launch's shape (HVQM4_AMD_FLUSH_TIMING); the two-tile run must have seen both kinds of instantiation.
"""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIPS = ["ragged24x40", "ip8", "portrait152x280", "literals96x96", "bigscalars64x64", "gop64x48_13", "yuv444_64x48", "yuv422_64x48",
         "pselfref64x48_15", "qvga_13"]


def child(tiles, args):
    env = dict(os.environ, HVQM4_AMD_TILES_PER_WG=tiles, HVQM4_AMD_FLUSH_TIMING="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "register_stores_child.py")] + args, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    shapes = {(int(t), int(c)) for t, c in re.findall(r"-> (\d) tile\(s\) per workgroup, items (\d+),", r.stderr)}
    return r.stdout.split("\n"), shapes


@pytest.mark.parametrize("tiles", ["1", "2"])
def test_clips_of_the_store_path_equal_the_oracle(tiles):
    out, shapes = child(tiles, CLIPS)
    assert [l for l in out if l] == [f"{name} ok" for name in CLIPS]
    assert shapes and {t for t, _c in shapes} == {int(tiles)}
    if tiles == "2":
        assert any(c >= 128 for _t, c in shapes) and any(c < 128 for _t, c in shapes), shapes


@pytest.mark.parametrize("tiles", ["1", "2"])
def test_no_store_strays_into_a_neighbouring_picture(tiles):
    out, _shapes = child(tiles, ["neighbours", "gop64x48_15"])
    assert len([l for l in out if l.endswith(" ok")]) == 2
