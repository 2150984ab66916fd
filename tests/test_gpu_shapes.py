"""GPU: the witness of tests/test_launch_coverage.py.  That file predicts, from blob headers and hvq_recon_inline_plan, which instantiation
of hvq_recon_inline_kernel every picture of clips.SHAPES and manybases320x240 is launched in; here the runtime says which it launched.

A child process per forced shape (HVQM4_AMD_TILES_PER_WG is read once per process; torch imported first, see tests/gpu_child.py)
decodes the clips with HVQM4_AMD_FLUSH_TIMING=1, one picture a flush, and writes a marker line to stderr before each flush: the runtime's
`[flush] launch` line behind it belongs to that picture.  Every picture must equal the oracle (and the compiled reference where it is
built), and the (tiles per workgroup, items cap, picture kind) seen must be the 15 cells of the one-tile run and the 27 of the two-tile
run.  A third child decodes all shape clips and a sparse clip in ONE flush: sparse pictures in launches sized by another stream's fullest
tile.  The child stops at the first HVQ_E_HIP or HIP error: nothing more is started on a GPU that has reported a fault."""
import os
import re
import subprocess
import sys
import traceback

import numpy as np
import pytest

from tests import clips
from tests.gpu_child import gpu_error
from tests.gpu_kit import launch_lines
from tests.test_launch_coverage import survey
from tests.test_recon_plan import L  # noqa: F401 -- the fixture: it asserts that the two environment caps are unset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 120                                 # a run takes seconds; a hung child is ended, not waited for
WITNESS = clips.SHAPES + [c for c in clips.MEDIUM if c[0] == "manybases320x240"]
ONE_BATCH = clips.SHAPES + [c for c in clips.SMALL if c[0] == "realistic128x96"]
KIND = {0x10: "I", 0x20: "P", 0x30: "B"}

MARKER_LINE = re.compile(r"^\[witness\] (?P<clip>\S+) (?P<ordinal>\d+) (?P<kind>[IPB])$")


# ------------------------------------------------------------------------------------------------------------- child side
def _child(out_path, one_batch):
    import torch                                   # FIRST: the library then binds torch's HIP runtime
    torch.cuda.init()
    from hvqm4_amd import batch
    from hvqm4_amd.container import parse_header, video_pictures
    ctx = batch.Context(0)
    got = {}
    try:
        opened = []
        for case in (ONE_BATCH if one_batch else WITNESS):
            clip = clips.get(case)
            hdr = parse_header(clip.data)
            sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, clip.n_pictures + 3)
            opened.append((case[0], sid, clip.n_pictures))
            for i, (ft, _d, pic) in enumerate(video_pictures(clip.data)):
                ctx.submit(sid, ft, pic)
                if not one_batch:
                    print(f"[witness] {case[0]} {i} {KIND[ft]}", file=sys.stderr, flush=True)
                    ctx.flush()
        if one_batch:
            ctx.flush()
        for name, sid, n in opened:
            got[name] = np.stack([ctx.read_picture(sid, i) for i in range(n)])
            ctx.close_stream(sid)
    except Exception as e:
        traceback.print_exc()
        if gpu_error(e):
            print("stopped: the GPU reported an error", file=sys.stderr, flush=True)
            os._exit(3)                            # no further GPU call, not even the context's teardown
        raise
    np.savez(out_path, **got)
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ parent side
def _run(tmp_path, tiles, one_batch):
    out = str(tmp_path / "pictures.npz")
    env = dict(os.environ, HVQM4_AMD_FLUSH_TIMING="1")
    env.pop("HVQM4_AMD_TILES_PER_WG", None)
    if tiles:
        env["HVQM4_AMD_TILES_PER_WG"] = str(tiles)
    r = subprocess.run([sys.executable, "-c", f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_gpu_shapes import _child; "
                        f"_child({out!r}, {one_batch!r})"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0 and os.path.exists(out), f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return r.stderr, np.load(out)


def _compare(cases, got):
    from oracle import bridge
    for case in cases:
        clip = clips.get(case)
        want = bridge.oracle_decode(clip.data, clip.n_pictures)
        assert got[case[0]].shape == want.shape
        for i in range(clip.n_pictures):
            assert np.array_equal(got[case[0]][i], want[i]), f"{case[0]}: picture {i} ({KIND[clip.kinds[i]]}) differs from the oracle"
        if bridge.have_ref():
            assert np.array_equal(got[case[0]], bridge.ref_decode(clip.data, clip.n_pictures)[0]), f"{case[0]} differs from the compiled reference"


@pytest.mark.gpu
@pytest.mark.parametrize("tiles,ncells", [(1, 15), (2, 27)])
def test_every_instantiation_runs_every_picture_kind_and_equals_the_oracle(L, tiles, ncells, tmp_path):
    stderr, got = _run(tmp_path, tiles, False)
    seen, per_picture, current = set(), {}, None
    for line in stderr.splitlines():
        m = MARKER_LINE.match(line)
        if m:
            current = (m["clip"], int(m["ordinal"]), m["kind"])
            per_picture[current] = []
        elif line.startswith("[flush] launch"):
            assert current is not None, line
            per_picture[current] += launch_lines(line)
    for (name, ordinal, kind), lines in per_picture.items():
        assert len(lines) == 1, f"{name}, picture {ordinal}: a flush of one picture is one launch, the runtime reports {len(lines)}"
        assert lines[0]["tpw"] == tiles
        seen.add((lines[0]["tpw"], lines[0]["items"], kind))
    print(f"{tiles} tile(s) per workgroup: {len(seen)} cells seen: {sorted(seen)}")
    assert len(per_picture) == sum(clips.get(c).n_pictures for c in WITNESS)
    predicted = set(survey(L, WITNESS, forces=(tiles,))[0])
    assert seen == predicted, f"launched but not predicted {sorted(seen - predicted)}, predicted but not launched {sorted(predicted - seen)}"
    assert len(seen) == ncells
    _compare(WITNESS, got)


@pytest.mark.gpu
def test_sparse_pictures_in_launches_sized_by_another_stream(tmp_path):
    stderr, got = _run(tmp_path, 0, True)
    lines = launch_lines(stderr)
    assert len(lines) >= 3 and max(l["max_items"] for l in lines) > 192      # the launches of the levels are sized by the fullest shape clip
    _compare(ONE_BATCH, got)
