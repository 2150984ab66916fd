"""CPU: the rule that splits a large batch into launch groups (hvq_launch_group_plan, hvq_runtime.cpp), through ctypes.

The function is pure.  It sees per stream the picture size and the kinds and dependency levels of the pending pictures -- what build_tiles
knows at hvq_flush_begin -- and answers with G and the group of every stream:

  window(stream) = the largest sum, over two consecutive levels, of its pictures' algorithmic bytes (1 x pic_bytes for I, 2 x for P/B)
  G = ceil(sum of the windows / budget), at most streams // (8 x launch queues), at least 1; budget 0: 1
  streams to groups by work, heaviest first to the lightest group that is not full (floor(n / G) streams, n % G groups one more)

The levels of a stream come from `ring_levels`, a restatement of the runtime's slot ring and level assignment (enqueue_common) for a
stream submitted whole: it is pinned below by the two level counts the project records for its benchmark shapes (7 for one 16-picture GOP
in 6 slots, 25 for four of them)."""
import ctypes as C
import math

import pytest

GOP16 = "IPBBPBBPBBPBBPBB"
VGA, QVGA = 640 * 480 * 3 // 2, 320 * 240 * 3 // 2
KIND = {"I": 0, "P": 1, "B": 2}
MIN_PER_QUEUE = 8


@pytest.fixture(scope="module")
def L():
    from hvqm4_amd._lib import lib
    return lib()


def ring_levels(kinds, nslots):
    """dependency level of every picture of one stream, submitted whole into a fresh ring of `nslots` slots (hvq_runtime.cpp: alloc_slot,
    enqueue_common)"""
    w = [-1] * nslots
    r = [-1] * nslots
    occupant = [-1] * nslots
    pic_slot = []
    ring, a_old, a_new = 0, -1, -1
    rp_past = rp_future = rp_present = -1
    out = []
    for n, k in enumerate(kinds):
        if k != "B":
            a_old, a_new = a_new, a_old
            rp_past, rp_future = rp_future, rp_past
        old_ord = rp_present
        old_slot = -1 if old_ord < 0 else (pic_slot[old_ord] if pic_slot[old_ord] >= 0 else -2)
        rp_present = n
        if k != "B":
            rp_present, rp_future = rp_future, rp_present
        dst = next(c for c in ((ring + i) % nslots for i in range(nslots)) if c not in (a_old, a_new))
        ring = (dst + 1) % nslots
        ref0, ref1 = (-1, -1) if k == "I" else (a_old, dst) if k == "P" else (a_old, a_new)
        lvl = 0
        for ref in (ref0, ref1):
            if ref >= 0 and ref != dst:
                lvl = max(lvl, w[ref] + 1)
        lvl = max(lvl, max(w[dst], r[dst]) + 1)
        if k == "P" and old_slot >= 0 and old_slot != dst:
            lvl = max(lvl, w[old_slot])
            r[old_slot] = max(r[old_slot], lvl)
        if ref0 >= 0:
            r[ref0] = max(r[ref0], lvl)
        if ref1 >= 0 and ref1 != dst:
            r[ref1] = max(r[ref1], lvl)
        if occupant[dst] >= 0:
            pic_slot[occupant[dst]] = -1
        w[dst], r[dst], occupant[dst] = lvl, -1, n
        pic_slot.append(dst)
        if k != "B":
            a_new = dst
        out.append(lvl)
    return out


def stream(pic_bytes, kinds, nslots=6):
    return pic_bytes, list(kinds), ring_levels(kinds, nslots)


def window(st):
    pic_bytes, kinds, levels = st
    per = [0] * (max(levels, default=0) + 2)
    for k, l in zip(kinds, levels):
        per[l] += pic_bytes * (1 if k == "I" else 2)
    return max((per[l] + per[l + 1] for l in range(len(per) - 1)), default=0)


def work(st):
    return sum(st[0] * (1 if k == "I" else 2) for k in st[1])


def plan(L, streams, budget, queues=2):
    """-> (G, group of every stream, the batch's window as the library sums it)"""
    n = len(streams)
    first = [0]
    for _pb, kinds, _lv in streams:
        first.append(first[-1] + len(kinds))
    total = first[-1]
    a_pb = (C.c_uint32 * max(n, 1))(*[s[0] for s in streams])
    a_first = (C.c_uint32 * (n + 1))(*first)
    a_kinds = (C.c_uint8 * max(total, 1))(*[KIND[k] for s in streams for k in s[1]])
    a_levels = (C.c_int32 * max(total, 1))(*[l for s in streams for l in s[2]])
    gof = (C.c_uint16 * max(n, 1))()
    win = C.c_uint64()
    g = L.hvq_launch_group_plan(n, a_pb, a_first, a_kinds, a_levels, budget, queues, gof, C.byref(win))
    assert g == L.hvq_launch_group_plan(n, a_pb, a_first, a_kinds, a_levels, budget, queues, None, None)
    return g, list(gof)[:n], win.value


def default_budget(L):
    """the budget a new context carries"""
    return L.hvq_launch_group_default_bytes()


def test_the_restated_levels_are_the_recorded_ones():
    assert max(ring_levels(GOP16, 6)) + 1 == 7                 # the benchmark's dense step: 7 levels (DESIGN "Launch queues")
    assert max(ring_levels(GOP16 * 4, 6)) + 1 == 25            # config 4: 25 levels (build_tiles)
    assert ring_levels("IPBBPBB", 10) == [0, 1, 2, 2, 2, 3, 3]  # a slot per picture: only the references count (tests/coverage.py levels)


def test_budget_zero_never_splits(L):
    dense = [stream(VGA, GOP16)] * 128
    g, gof, win = plan(L, dense, 0)
    assert g == 1 and set(gof) == {0}
    assert win == sum(window(s) for s in dense)


def test_the_benchs_shape_gets_the_groups_the_arithmetic_predicts(L):
    dense = [stream(VGA, GOP16)] * 128
    one = window(dense[0])
    assert one == 12 * VGA                                     # two consecutive levels of P B B: six P/B pictures, written and read
    total = 128 * one                                          # 707.8 MB
    for budget in (1 << 40, total, total - 1, 400 * 10**6, 250 * 10**6, 180 * 10**6, 120 * 10**6, 100 * 10**6, 1):
        g, gof, win = plan(L, dense, budget)
        assert win == total
        assert g == min(math.ceil(total / budget), 128 // (2 * MIN_PER_QUEUE)), budget
        assert sorted(set(gof)) == list(range(g))
    assert [plan(L, dense, b)[0] for b in (400 * 10**6, 250 * 10**6, 180 * 10**6, 120 * 10**6)] == [2, 3, 4, 6]
    assert plan(L, dense, 1)[0] == 8                           # capped: 16 streams per group with two queues
    assert plan(L, dense, 1, queues=1)[0] == 16                # ... 8 with one


@pytest.mark.parametrize("n", [0, 1, 15, 16, 31, 32, 33, 40, 47, 48, 50, 128, 129])
@pytest.mark.parametrize("queues", [1, 2])
def test_no_group_falls_below_the_minimum_per_queue(L, n, queues):
    sizes = [VGA, QVGA, 72 * 56 * 3 // 2]
    streams = [stream(sizes[i % 3] if i % 5 else VGA, GOP16 if i % 2 else "IPBBPBB") for i in range(n)]
    g, gof, _win = plan(L, streams, 1, queues)                 # the smallest budget: as many groups as the cap allows
    assert g == max(1, n // (MIN_PER_QUEUE * queues))
    counts = [gof.count(k) for k in range(g)]
    assert sum(counts) == n
    if g > 1:
        assert min(counts) >= MIN_PER_QUEUE * queues
        assert max(counts) - min(counts) <= 1


def test_groups_are_balanced_by_work_within_one_streams_work(L):
    # uniform: equal work; the bench's shape with a few lighter clips among it; 40 streams with one small clip (the GPU test's case 2)
    cases = [([stream(VGA, GOP16)] * 128, 180 * 10**6),
             ([stream(VGA, GOP16)] * 100 + [stream(QVGA, GOP16)] * 28, 180 * 10**6),
             ([stream(64 * 48 * 3 // 2, "IPBBPBB", 10)] * 39 + [stream(72 * 56 * 3 // 2, "IPBBPBB", 10)], 1)]
    for streams, budget in cases:
        g, gof, _win = plan(L, streams, budget)
        assert g >= 2
        loads = [sum(work(s) for s, k in zip(streams, gof) if k == grp) for grp in range(g)]
        assert max(loads) - min(loads) <= max(work(s) for s in streams)
    # heaviest first to the lightest group: two heavy streams never share a group while another has none
    streams = [stream(VGA, GOP16)] * 2 + [stream(QVGA, GOP16)] * 30
    g, gof, _win = plan(L, streams, 1)
    assert g == 2 and gof[0] != gof[1]


def test_config_4_stays_one_group_at_the_default(L):
    """64 clips, 320x240 and 640x480 in alternating runs of eight, four 16-picture GOPs each in 6 slots: 25 levels, one launch queue (mixed
    sizes).  The rule is in bytes, so a batch of 64 streams is not split for its count.  By the rule's own arithmetic its window is
    221.2 MB: the fullest pair of levels holds six P/B pictures per stream, each written once and reading as much (a count of the
    writes alone gives the 110 MB quoted when the rule was proposed).  A default other than 0 must therefore be at least 221.2 MB,
    which leaves the dense benchmark batch (707.8 MB) at most four groups."""
    c4 = [stream(QVGA if (i // 8) % 2 == 0 else VGA, GOP16 * 4) for i in range(64)]
    total = sum(window(s) for s in c4)
    assert total == 32 * 12 * (VGA + QVGA) == 221184000
    budget = default_budget(L)
    assert budget == 0 or budget >= total
    g, gof, win = plan(L, c4, budget, queues=1)
    assert win == total and g == 1 and set(gof) == {0}
    # ... while a budget below its window would split it, uniform or not
    assert plan(L, c4, total // 2, queues=1)[0] == 2 and plan(L, c4, total // 2 - 1, queues=1)[0] == 3


def test_one_stream_no_stream_and_one_level(L):
    assert plan(L, [], 1) == (1, [], 0)
    assert plan(L, [], 0) == (1, [], 0)
    g, gof, win = plan(L, [stream(VGA, GOP16)], 1)
    assert (g, gof, win) == (1, [0], 12 * VGA)
    flat = [stream(VGA, "IIII", 8)] * 64                        # every picture on level 0: the window is that level alone
    assert set(flat[0][2]) == {0}
    g, gof, win = plan(L, flat, 4 * VGA * 16, queues=2)
    assert win == 64 * 4 * VGA
    assert g == 4 and [gof.count(k) for k in range(4)] == [16] * 4
