"""CPU: which instantiations of hvq_recon_inline_kernel<ITEMS_CAP, TPW> the clips of the parity suites launch, and with which kind of
picture.  The kernel is compiled fourteen times (test_recon_plan.STEPS); hvq_recon_inline_plan picks one per launch from the fullest tile
of the launch's pictures (HvqPicHeader.max_items, max_pairs), and the parity suites run every clip with one and with two tiles per
workgroup forced (tests/test_gpu_modes.py).  A cell is (tiles per workgroup, items cap, picture kind): inside one instantiation I and
P/B pictures take very different paths.  An empty cell fails: an instantiation no clip launches is a kernel nobody compares with the
oracle.  tests/test_gpu_shapes.py observes on the GPU what this file predicts.

A launch reconstructs one dependency level of a flush (coverage.levels) and is sized by the fullest picture of the level, so a level
counts for a kind only when all its pictures are of that kind: the clips of clips.SHAPES have a picture per level (gop "IPB"), the two
B pictures between two anchors of the older clips share theirs."""
import pytest

from tests import clips, coverage
from tests.test_recon_plan import STEPS, L, plan  # noqa: F401 -- L is the fixture: it asserts that the two environment caps are unset

KINDS = "IPB"
FORCES = (1, 2)
# No cell is waived: every (instantiation, kind) can be reached by a stream the parsers accept, and clips.SHAPES reaches them.
WAIVED = ()


def launches(clip):
    """the launches of `clip` decoded as one stream in one flush: (kind or None for a level of mixed kinds, max_items, max_pairs, whether
    some plane has an odd number of tiles -- its last two-tile workgroup then has one tile)"""
    pics = coverage.launch_inputs(clip)
    lv = coverage.levels(clip.kinds)
    out = []
    for level in sorted(set(lv)):
        group = [p for p, l in zip(pics, lv) if l == level]
        kinds = {p[0] for p in group}
        out.append((kinds.pop() if len(kinds) == 1 else None, max(p[1] for p in group), max(p[2] for p in group),
                    any(t & 1 for p in group for t in p[3])))
    return out


def instantiations(L):
    """{tiles per workgroup: items caps} as hvq_recon_inline_plan hands them out: max_items swept under both forces, with no pairs and
    with four bases an item"""
    seen = {t: set() for t in FORCES}
    for force in FORCES:
        for mi in range(0, 257):
            for mp in (0, 4 * mi):
                p = plan(L, mi, mp, force)
                assert p["tpw"] == force
                seen[force].add(p["items"])
    return {t: tuple(sorted(v)) for t, v in seen.items()}


def survey(L, cases, forces=FORCES):
    """-> ({(tpw, items cap, kind): [clip names]}, {items cap: [clip names]} of the two-tile launches with a single-tile workgroup)"""
    cells, single = {}, {}
    for case in cases:
        for kind, mi, mp, odd in launches(clips.get(case)):
            for force in forces:
                p = plan(L, mi, mp, force)
                if kind is not None:
                    cells.setdefault((p["tpw"], p["items"], kind), []).append(case[0])
                if p["tpw"] == 2 and odd:
                    single.setdefault(p["items"], []).append(case[0])
    return cells, single


def required(L):
    return [(t, cap, k) for t, caps in sorted(instantiations(L).items()) for cap in caps for k in KINDS if (t, cap, k) not in WAIVED]


@pytest.fixture(scope="module")
def surveyed(L):
    return survey(L, clips.PARITY)


def test_the_plan_hands_out_the_fourteen_instantiations(L):
    assert instantiations(L) == STEPS
    assert len(required(L)) == 3 * 14 - len(WAIVED)


def test_every_instantiation_is_launched_with_every_picture_kind(L, surveyed):
    cells, _single = surveyed
    empty = [c for c in required(L) if c not in cells]
    assert not empty, (f"{len(empty)} of {len(required(L))} cells (tiles per workgroup, items cap, picture kind) are launched by no parity clip -- "
                       f"an instantiation no clip launches is a kernel nobody compares with the oracle: {empty}")
    assert set(cells) <= set(required(L)), "a launch outside the instantiations the plan hands out"


def test_the_large_two_tile_instantiations_meet_a_workgroup_with_one_tile(L, surveyed):
    """a plane with an odd number of tiles ends in a workgroup that has one tile (ntl == 1) in a kernel sized for two"""
    _cells, single = surveyed
    missing = [cap for cap in STEPS[2] if cap >= 224 and cap not in single]
    assert not missing, f"no two-tile launch with items cap {missing} has a plane with an odd number of tiles"


def test_shape_clips_have_one_picture_per_launch_and_all_samplings():
    """what lets tests/test_gpu_shapes.py tell which picture a launch belongs to, and full chroma tiles in the large instantiations"""
    for name, cfg in clips.SHAPES:
        assert cfg.gop == "IPB" and cfg.n_gops == 1, name
        assert coverage.levels(clips.get((name, cfg)).kinds) == [0, 1, 2], name
    assert {cfg.sampling for _n, cfg in clips.SHAPES} == {"420", "422", "444"}
