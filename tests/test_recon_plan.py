"""CPU: the LDS shape the host gives a launch of hvq_recon_inline_kernel (hvq_recon_inline_plan, hvq_runtime.cpp).

The function is pure apart from the two environment caps it reads once (HVQM4_AMD_PAIR_CAP, HVQM4_AMD_POOL_CAP: unset here): the fullest tile's items and pairs in, tiles per workgroup, accumulator cap, pair list, staged pool and the LDS
bytes of the launch out.  A CU has 160 KB of LDS; one tile per workgroup is resident eight times by waves, the two-tile kernels with
accumulators for 128 items and more seven times (they are allocated for seven waves per SIMD)."""
import ctypes as C
import os

import pytest

CU_LDS = 163840
NEST_LDS = 1360                      # the packed nest, padded to 16 bytes
ITEM_LDS = 64 + 16 + 12              # 16 accumulators, the block column, three record dwords
STEPS = {1: (64, 96, 128, 192, 256), 2: (64, 96, 128, 160, 192, 224, 256, 384, 512)}


@pytest.fixture(scope="module")
def L():
    for k in ("HVQM4_AMD_PAIR_CAP", "HVQM4_AMD_POOL_CAP"):       # read once per process by the function under test
        assert k not in os.environ
    from hvqm4_amd._lib import lib
    l = lib()
    u32, p32 = C.c_uint32, C.POINTER(C.c_uint32)
    l.hvq_recon_inline_plan.restype = None
    l.hvq_recon_inline_plan.argtypes = [u32, u32, C.c_int, p32, p32, p32, p32, p32]
    for n in ("hvq_recon_inline_static_lds", "hvq_recon_inline_dyn_lds"):
        getattr(l, n).restype = u32
        getattr(l, n).argtypes = [u32, u32]
    l.hvq_recon_inline_residency.restype = u32
    l.hvq_recon_inline_residency.argtypes = [u32, u32, u32]
    return l


def plan(L, mi, mp, force=0):
    out = [C.c_uint32() for _ in range(5)]
    L.hvq_recon_inline_plan(mi, mp, force, *[C.byref(o) for o in out])
    return dict(zip(("tpw", "items", "pairs", "pool", "lds"), (o.value for o in out)))


def workgroups(L, p):
    return L.hvq_recon_inline_residency(p["tpw"], p["items"], p["lds"])


def untrimmed_pool(t, mi, mp):
    return (min(1536, t * (mp + 2 * mi + 128)) + 4 + 3) & ~3


def test_dense_pb_level_runs_two_tiles_at_seven_workgroups(L):
    p = plan(L, 75, 250)
    assert (p["tpw"], p["items"]) == (2, 160)
    assert p["lds"] <= 23040
    assert p["pairs"] >= 500 and p["pool"] == untrimmed_pool(2, 75, 250)
    assert workgroups(L, p) == 7


def test_fullest_tile_beyond_80_items_takes_the_next_accumulator_step(L):
    p = plan(L, 83, 281, 2)
    assert (p["tpw"], p["items"]) == (2, 192)
    assert workgroups(L, p) == 6
    # the host's own decision is the same launch: two tiles at six workgroups per CU (12 tiles) against one tile at eight
    assert plan(L, 83, 281) == p


def test_sparse_stream_keeps_two_tiles_at_eight_workgroups(L):
    p = plan(L, 20, 60)
    assert p["tpw"] == 2 and p["items"] == 64
    assert workgroups(L, p) == 8 and 8 * p["lds"] <= CU_LDS


@pytest.mark.parametrize("mi,mp", [(20, 60), (75, 250), (83, 281), (120, 400), (1, 1), (0, 0)])
def test_forced_shapes_are_honoured(L, mi, mp):
    for t in (1, 2):
        p = plan(L, mi, mp, t)
        assert p["tpw"] == t
        assert p["items"] >= min(256 * t, t * mi) and p["items"] in STEPS[t]
        assert p["pairs"] >= max(1, t * mp)


def test_only_the_staged_pool_is_trimmed_and_only_by_the_literal_reserve(L):
    """Every (items, pairs) of a grid: the pair list and the accumulator cap never go below what the fullest tile needs, the pool gives up
    at most the literal reserve (128 dwords per tile), and only where that reaches the next residency step."""
    trimmed = 0
    for t in (1, 2):
        for mi in range(0, 260, 3):
            for mp in range(0, 1100, 7):
                p = plan(L, mi, mp, t)
                assert p["items"] >= min(256 * t, t * mi) and p["pairs"] >= max(1, t * mp)
                full = untrimmed_pool(t, mi, mp)
                reserve = max(0, min(1536, t * (mp + 2 * mi + 128)) - t * (mp + 2 * mi))      # what the 1536-dword limit left of it
                assert reserve <= 128 * t and full - reserve <= p["pool"] <= full
                if p["pool"] < full:
                    trimmed += 1
                    lds_full = (L.hvq_recon_inline_static_lds(t, p["items"]) + L.hvq_recon_inline_dyn_lds(p["pairs"], full) + 511) & ~511
                    assert workgroups(L, p) == L.hvq_recon_inline_residency(t, p["items"], lds_full) + 1
    assert trimmed > 0


def test_a_launch_that_misses_seven_workgroups_by_less_than_the_reserve_reaches_it(L):
    # two tiles of 78 items and 300 pairs: 16 096 B static + 4 * (600 + 1172) = 23 184 B, 144 B above a seventh of the CU's LDS
    p = plan(L, 78, 300, 2)
    assert (p["items"], p["pairs"]) == (160, 600)
    assert 0 < untrimmed_pool(2, 78, 300) - p["pool"] <= 256
    assert workgroups(L, p) == 7


def test_a_pool_clipped_by_its_limit_gives_up_no_bases(L):
    # two tiles of 200 items and 700 pairs want 2 * (700 + 400 + 128) dwords, the limit of 1536 leaves no reserve: nothing to give up
    p = plan(L, 200, 700, 2)
    assert p["pool"] == untrimmed_pool(2, 200, 700) == 1540


def test_lds_bytes_is_static_plus_dynamic_for_every_instantiation(L):
    for t in (1, 2):
        for cap in STEPS[t]:
            assert L.hvq_recon_inline_static_lds(t, cap) == NEST_LDS + ITEM_LDS * cap + 16
        seen = set()
        for mi in range(0, 300, 5):
            for mp in (0, 60, 250, 281, 700, 1500):
                p = plan(L, mi, mp, t)
                seen.add(p["items"])
                dyn = L.hvq_recon_inline_dyn_lds(p["pairs"], p["pool"])
                assert dyn == 4 * (((max(p["pairs"], 1) + 3) & ~3) + ((p["pool"] + 3) & ~3))
                assert p["lds"] == (L.hvq_recon_inline_static_lds(t, p["items"]) + dyn + 511) & ~511
        assert seen == set(STEPS[t])
