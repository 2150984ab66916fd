"""The case loop of tests/gpu_child.py without a GPU: fake cases in a fresh Python process.  A case whose exception reads like a HIP
error ends the process with status 3 at once: the results written so far stay, no later case starts.  Nothing here touches a device."""
import json
import os
import subprocess
import sys

import pytest

from tests import gpu_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAKES = """
import sys
sys.path.insert(0, {root!r})
from tests import gpu_child

def case_passes(marker):
    pass

def case_asserts(marker):
    assert 1 + 1 == 3, "arithmetic"

def case_faults(marker):
    raise RuntimeError("HIP error: an illegal memory access was encountered")

def case_marks(marker):
    open(marker, "w").write("ran")

gpu_child.run_cases(globals(), {names!r}, {out!r}, ({marker!r},))
print("complete after the last case:", sorted(__import__("json").load(open({out!r}))), flush=True)
"""


def _run(tmp_path, names):
    out, marker = str(tmp_path / "results.json"), str(tmp_path / "marker")
    r = subprocess.run([sys.executable, "-c", FAKES.format(root=ROOT, names=names, out=out, marker=marker)], cwd=ROOT, capture_output=True, text=True,
                       timeout=60)
    res = json.load(open(out))
    res["_log"] = f"exit {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    return r, res, marker


def test_the_loop_stops_at_the_first_gpu_error(tmp_path):
    r, res, marker = _run(tmp_path, ["passes", "asserts", "faults", "marks"])
    assert r.returncode == 3, res["_log"]
    assert res["passes"] == "ok"
    assert "Traceback" in res["asserts"] and "AssertionError" in res["asserts"] and "arithmetic" in res["asserts"]
    assert "Traceback" in res["faults"] and "illegal memory access" in res["faults"]
    assert "marks" not in res and not os.path.exists(marker)
    lines = r.stdout.splitlines()
    assert [l.split(":")[0] for l in lines[:3]] == ["passes", "asserts", "faults"] and all(l.endswith(" s") for l in lines[:3]), lines
    assert lines[3:] == ["stopped after faults: the GPU reported an error"], lines          # nothing ran behind the stop
    gpu_child.report("passes", res)
    with pytest.raises(AssertionError, match="arithmetic"):
        gpu_child.report("asserts", res)
    with pytest.raises(AssertionError) as e:
        gpu_child.report("marks", res)
    assert "the case did not run" in str(e.value) and "exit 3" in str(e.value) and "stopped after faults" in str(e.value)


def test_without_a_gpu_error_every_case_runs(tmp_path):
    r, res, marker = _run(tmp_path, ["asserts", "passes", "marks"])
    assert r.returncode == 0, res["_log"]
    assert res["passes"] == res["marks"] == "ok" and "AssertionError" in res["asserts"]
    assert open(marker).read() == "ran"
    lines = r.stdout.splitlines()
    assert [l.split(":")[0] for l in lines[:3]] == ["asserts", "passes", "marks"]
    assert lines[3] == "complete after the last case: ['asserts', 'marks', 'passes']"    # read back before the process ended
    assert "stopped after" not in r.stdout


def test_gpu_error_tells_a_fault_from_a_refusal():
    from hvqm4_amd._lib import HVQ_E_ARG, HVQ_E_HIP, HvqError
    assert gpu_child.gpu_error(HvqError(HVQ_E_HIP, "hipMemcpyAsync: an illegal memory access was encountered")) is True
    assert gpu_child.gpu_error(HvqError(HVQ_E_ARG, "a HIP error in the text of a refusal is not one")) is False
    assert gpu_child.gpu_error(RuntimeError("the destination is too small")) is False
    assert gpu_child.gpu_error(AssertionError("HIP error")) is False
