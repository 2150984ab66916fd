"""The runner of the GPU tests whose cases need torch: one child process per test module, one case loop, one stop rule.

Torch brings its own HIP runtime, and a stream handle of torch's means something to the library only when both share one runtime:
torch must be imported before the library is loaded (hvqm4_amd.export.check_one_hip_runtime).  The main suite loads the library long
before these files run, so a module's cases run in ONE child process that imports torch first; each test reports its case.

A test module holds `CASES`, its `case_<name>(torch, ctx)` functions and

    child_results = gpu_child.results_fixture(__name__, "rank", CHILD_TIMEOUT)

    @pytest.mark.parametrize("case", CASES)
    def test_rank(case, child_results):
        gpu_child.report(case, child_results)

The child stops at the first HVQ_E_HIP or HIP error: nothing more is started on a GPU that has reported a fault, not even the
context's teardown.  This module imports neither torch nor the library at module level; tests/test_gpu_child_runner.py drives the
loop without a GPU."""
import importlib
import json
import os
import subprocess
import sys
import time
import traceback

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu_error(exc) -> bool:
    """HVQ_E_HIP from the library, or a HIP error torch reports: the GPU may have faulted, nothing more is started on it"""
    from hvqm4_amd._lib import HVQ_E_HIP, HvqError
    if isinstance(exc, HvqError):
        return exc.code == HVQ_E_HIP
    text = str(exc)
    return isinstance(exc, RuntimeError) and ("HIP error" in text or "hipError" in text or "CUDA error" in text)


# ------------------------------------------------------------------------------------------------------------- child side
def run_cases(namespace, names, out_path, args):
    """namespace["case_" + name](*args) for every name; "ok" or the traceback of each into the JSON file `out_path`"""
    res = {}
    stopped = False
    for name in names:
        t0 = time.time()
        try:
            namespace["case_" + name](*args)
            res[name] = "ok"
        except Exception as e:
            res[name] = traceback.format_exc()
            stopped = gpu_error(e)
        print(f"{name}: {time.time() - t0:.1f} s", flush=True)
        with open(out_path, "w") as f:             # after every case: what a crash leaves is readable
            json.dump(res, f)
        if stopped:
            print(f"stopped after {name}: the GPU reported an error", flush=True)
            os._exit(3)                            # no further GPU call, not even the context's teardown


def child(module, out_path):
    """the child's entry: the CASES of the test module `module` (a dotted path) on one context of device 0"""
    import torch                                   # FIRST: the library then binds torch's HIP runtime
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    mod = importlib.import_module(module)
    run_cases(vars(mod), mod.CASES, out_path, (torch, ctx))
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ parent side
def run_child(module, out_path, timeout):
    """the cases of `module` in a fresh process -> {case: "ok" or a traceback, "_log": exit status and the ends of its output}"""
    r = subprocess.run([sys.executable, "-c", f"import sys; sys.path.insert(0, {ROOT!r}); from tests.gpu_child import child; "
                        f"child({module!r}, {out_path!r})"], cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    res["_log"] = f"exit {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    print(res["_log"])
    return res


def results_fixture(module, label, timeout):
    """a module-scoped fixture: the results of `module`'s child, run once for all its tests"""
    @pytest.fixture(scope="module")
    def child_results(tmp_path_factory):
        return run_child(module, str(tmp_path_factory.mktemp(label) / "results.json"), timeout)
    return child_results


def report(case, results):
    got = results.get(case)
    assert got == "ok", got or f"the case did not run: {results['_log']}"
