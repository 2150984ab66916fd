"""CPU: a batch split into launch groups (hvq_context_set_group_bytes) on the fake device -- the runtime linked unchanged against
tests/native/fake_device.cpp and fake_kernels.cpp, driven by tests/native/fake_groups_driver.cpp, under the schedules `eager` and `late`
(`late` runs nothing until the host observes it: a picture that runs behind the wrong launch, or a missing ordering edge, shows there).

The batch: 32 streams of 64 x 48, 4:2:0, GOP IPBBPBB, two launch queues, one flush; stream 11 is a clip whose P pictures carry
future-referencing macroblocks, so its raster-order walks (SelfRef, run_launches) must follow the launch of their own group.  With a budget
of one byte the rule splits as far as it may: 32 streams / (8 per queue x 2 queues) = 2 groups.

Passing: exit status 0, no sanitizer report, no fake_span abort; every picture byte-identical to the oracle's and to the same batch in one
group (budget 0); the launches of each queue, as the runtime lists them under HVQM4_AMD_FLUSH_TIMING in the order it issues them, are
group-major with levels ascending inside a group, and both queues walk the groups in the same order."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_fake_device import BUILDS, CXX_SOURCES, GOLDEN, NATIVE, build_driver, oracle_pictures

SOURCES = [s for s in CXX_SOURCES if not s.endswith("fake_driver.cpp")] + [os.path.join(NATIVE, "fake_groups_driver.cpp")]
GROUP_LINE = re.compile(r"^\[flush\] group (?P<group>\d+) of (?P<groups>\d+): launch (?P<launch>\d+) \(level (?P<level>\d+), queue (?P<queue>\d+)\), "
                        r"(?P<slots>\d+) picture slots$")
LEVELS = 4                                                   # IPBBPBB with a slot per picture: levels 0 1 2 2 2 3 3 (stream 11, in four slots: more)


@pytest.fixture(scope="module")
def drivers():
    return {kind: build_driver(kind, "groups", "fake_groups_driver", SOURCES, __file__) for kind in BUILDS}


def run(exe, budget, schedule, out):
    out.mkdir()
    env = dict(os.environ, FAKEHIP_SCHEDULE=schedule, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1", HVQM4_AMD_FLUSH_TIMING="1")
    env.pop("HVQM4_AMD_GROUP_BYTES", None)
    env.pop("HVQM4_AMD_QUEUES", None)
    r = subprocess.run([exe, "groups", str(out), GOLDEN, str(budget)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "fake_span" not in r.stderr and "fakehip:" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    pictures = np.fromfile(out / "pictures.bin", dtype=np.uint8)
    P, G = [], {}
    for line in open(out / "results.txt").read().splitlines():
        f = line.split()
        if f[0] == "P":
            P.append((f[6], int(f[5]), f[1], int(f[2]), pictures[int(f[3]):int(f[3]) + int(f[4])]))
        elif f[0] == "G":
            G[f[1]] = (int(f[2]), int(f[3]), int(f[4]))
    flushes, lines = [], []                                  # the group lines of every flush, in the order of the flushes (host, device)
    for line in r.stderr.splitlines():
        if line.startswith("[flush] group"):
            m = GROUP_LINE.match(line)
            assert m, line
            lines.append({k: int(v) for k, v in m.groupdict().items()})
        elif line.startswith("flush_end "):
            flushes.append(lines)
            lines = []
    return P, G, flushes


@pytest.mark.parametrize("schedule", ["eager", "late"])
@pytest.mark.parametrize("build", list(BUILDS))
def test_two_groups_decode_what_one_group_and_the_oracle_decode(drivers, build, schedule, tmp_path):
    P2, G2, F2 = run(drivers[build], 1, schedule, tmp_path / "two")
    P1, G1, F1 = run(drivers[build], 0, schedule, tmp_path / "one")
    # what was flushed: 32 streams on two queues, in one group and in two
    for label in ("groups/host", "groups/device"):
        assert G1[label][0] == 1 and G2[label][0] == 2 and G1[label][2] == G2[label][2] == 2, (G1, G2)
    assert [G1[label][1] for label in ("groups/host", "groups/device")] == [len(lines) for lines in F1]      # HvqStats.launches counts them all
    assert [G2[label][1] for label in ("groups/host", "groups/device")] == [len(lines) for lines in F2]
    # the pictures: all of the 31 clips, and what the four slots of stream 11 still hold -- its last pictures, two self-referencing P among them
    assert len(P2) == len(P1) and len(P2) >= 2 * (31 * 7 + 3)
    for label in ("groups/host", "groups/device"):
        assert {6, 7} <= {k for lb, sid, name, k, _b in P2 if lb == label and sid == 11 and name == "pselfref64x48_15"}
    for (label, sid, name, k, got), (label1, sid1, name1, k1, one) in zip(P2, P1):
        assert (label, sid, name, k) == (label1, sid1, name1, k1)
        want = oracle_pictures(name)[k]
        assert got.size == want.size and np.array_equal(got, want), f"{label}: picture {k} of stream {sid} ({name}) differs from the oracle with two groups"
        assert np.array_equal(one, want), f"{label}: picture {k} of stream {sid} ({name}) differs from the oracle with one group"
        assert np.array_equal(got, one)
    # the order of the launches
    assert len(F2) == len(F1) == 2
    for lines in F1:
        assert [l["groups"] for l in lines] == [1] * len(lines) and {l["group"] for l in lines} == {0}
    for lines in F2:
        assert [l["launch"] for l in lines] == list(range(len(lines)))
        assert {l["groups"] for l in lines} == {2}
        # every level that all streams have is a launch of its own per group and queue
        assert {(g, lv, q) for g in (0, 1) for lv in range(LEVELS) for q in (0, 1)} <= {(l["group"], l["level"], l["queue"]) for l in lines}
        for q in (0, 1):
            seq = [(l["group"], l["level"]) for l in lines if l["queue"] == q]
            assert seq == sorted(seq) and len(set(seq)) == len(seq), f"queue {q} does not run group-major, levels ascending: {seq}"
        # both queues walk the groups in the same order: in the order of issue no launch of group 1 comes before a launch of group 0
        assert [l["group"] for l in lines] == sorted(l["group"] for l in lines)
        # every group keeps 8 streams per queue: 8 picture slots at level 0 (one I picture per stream)
        assert [l["slots"] for l in lines if l["level"] == 0] == [8] * 4
