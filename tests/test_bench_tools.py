"""tools/benchlib.py and the trace summaries of the feature benchmarks (tools/*_bench.py), without a GPU and without rocprofv3: the summaries
against tests/golden/bench_tools.json (recorded from the tools before they shared a reader, see tests/golden/make_bench_tools.py), the
refusals of a trace that is not the planned one, and the driver of the steps on children that are plain Python."""
import argparse
import importlib
import importlib.util
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from tools import benchlib  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_bench_tools", os.path.join(HERE, "golden", "make_bench_tools.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

CASES = gen.cases()
GOLDEN = json.load(open(os.path.join(HERE, "golden", "bench_tools.json")))
PLANNED = [c for c in CASES if c != "export_float"]                   # export_float's trace step has no plan: it takes the launches it finds
ORDERED = ["metrics", "ssim", "histogram", "scale", "filter", "warp", "compose"]      # cut by a plan of more than one kernel


@pytest.fixture(autouse=True)
def in_tree_library(monkeypatch):
    monkeypatch.delenv("HVQM4_AMD_LIB", raising=False)


def summary(name, trace_dir):
    tool, function, _blocks, printed, earlier, _how = CASES[name]
    res = getattr(importlib.import_module("tools." + tool), function)(str(trace_dir), json.loads(json.dumps(printed)), earlier)
    return json.loads(json.dumps(res))


def test_golden_covers_every_tool_with_a_trace():
    tools = {f[:-3] for f in os.listdir(os.path.join(ROOT, "tools")) if f.endswith("_bench.py")} - {"export_bench"}
    assert {c[0] for c in CASES.values()} == tools and set(GOLDEN["summaries"]) == set(CASES)
    assert GOLDEN["recorded_from_commit"] == gen.PARENT


@pytest.mark.parametrize("name", sorted(CASES))
def test_summary_equals_the_recorded_one(name, tmp_path):
    gen.write_trace(str(tmp_path), CASES[name][2])
    got, want = summary(name, tmp_path), GOLDEN["summaries"][name]
    if name == "export_float":
        assert got["calls"] == CASES[name][3]
        got = got["kernels"]
    assert got == want


def test_the_recorded_summaries_leave_the_warm_up_launch_out():
    m = GOLDEN["summaries"]["metrics"]["metrics_all"]
    assert m["launches"] == gen.REPS and m["min_us"] < m["median_us"] < m["max_us"] < 140.0       # the warm-up launch of block 0 takes 140 us


@pytest.mark.parametrize("name", PLANNED)
def test_one_launch_too_few_is_refused(name, tmp_path):
    blocks = [list(b) for b in CASES[name][2]]
    blocks[-1].pop()
    gen.write_trace(str(tmp_path), blocks)
    res = summary(name, tmp_path)
    assert list(res) == ["error"] and "in the trace" in res["error"] and "planned" in res["error"]


@pytest.mark.parametrize("name", ORDERED)
def test_blocks_out_of_the_planned_order_are_refused(name, tmp_path):
    blocks = list(CASES[name][2])
    i = next(i for i in range(len(blocks) - 1) if set(blocks[i]) != set(blocks[i + 1]))
    blocks[i], blocks[i + 1] = blocks[i + 1], blocks[i]
    gen.write_trace(str(tmp_path), blocks)
    res = summary(name, tmp_path)
    assert list(res) == ["error"] and "not in the planned order" in res["error"]


def test_a_call_of_jpeg_out_of_order_is_refused(tmp_path):
    gen.write_trace(str(tmp_path), [b[1:] + b[:1] for b in CASES["jpeg"][2]])
    assert "launch 0 of a call is hvq_jpeg_layout_kernel" in summary("jpeg", tmp_path)["error"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_no_trace_and_two_traces_are_refused(name, tmp_path):
    assert summary(name, tmp_path) == {"error": f"no kernel trace under {tmp_path}"}
    gen.write_trace(str(tmp_path), CASES[name][2])
    gen.write_trace(str(tmp_path), CASES[name][2], name="8_kernel_trace.csv")
    res = summary(name, tmp_path)
    assert list(res) == ["error"] and res["error"].startswith("2 kernel traces under") and "fresh --out-dir" in res["error"]
    assert sorted(os.listdir(tmp_path / "host")) == ["7_kernel_trace.csv", "8_kernel_trace.csv"], "the tools delete nothing"


def test_names_are_read_in_every_spelling(tmp_path):
    gen.write_trace(str(tmp_path), [["hvq_jpeg_code_kernel<true>"], ["hvq_jpeg_code_kernel<false>"], ["hvq_metrics_kernel"], ["hvq_yuv_tensor_kernel<_Float16>"],
                                    ["hvq_metrics_kernel_of_another_name"]])
    got = benchlib.read_kernel_trace(str(tmp_path), ("hvq_jpeg_code_kernel", "hvq_metrics_kernel", "hvq_yuv_tensor_kernel"))
    assert [(l.kernel, l.shown) for l in got] == [("hvq_jpeg_code_kernel", "void hvq_jpeg_code_kernel<true>"), ("hvq_jpeg_code_kernel", "hvq_jpeg_code_kernel<false>.kd"),
                                                  ("hvq_metrics_kernel", "hvq_metrics_kernel"), ("hvq_yuv_tensor_kernel", "_Z21hvq_yuv_tensor_kernelIDF16_EvPK6HvqJobj")]
    assert [l.start for l in got] == sorted(l.start for l in got) and (got[0].vgprs, got[0].lds, got[0].scratch) == ("72", "3072", "0")


def test_launch_stats():
    assert benchlib.launch_stats([3049, 1000, 2051, 1950]) == {"launches": 4, "median_us": 2.0, "min_us": 1.0, "max_us": 3.0}


def child(code):
    return [sys.executable, "-c", code]


def test_run_step_returns_the_last_json_line(tmp_path):
    log = str(tmp_path / "s.log")
    assert benchlib.run_step(child("print('{\"a\": 1}'); print('between'); print('{\"a\": 2}')"), 20, log) == '{"a": 2}'
    assert "between" in open(log).read()


def test_run_step_ends_the_run_on_a_status(tmp_path):
    log = str(tmp_path / "s.log")
    with pytest.raises(SystemExit) as e:
        benchlib.run_step(child("import sys; print('{}'); sys.stderr.write('why'); sys.exit(3)"), 20, log)
    assert "ended with status 3" in str(e.value) and log in str(e.value) and "why" in open(log).read()


def test_run_step_ends_the_run_at_the_time_limit(tmp_path):
    log = str(tmp_path / "s.log")
    with pytest.raises(SystemExit) as e:
        benchlib.run_step(child("import time; print('{}', flush=True); time.sleep(30)"), 1, log)
    assert "ended with status 124" in str(e.value) and os.path.exists(log)


def test_run_step_names_the_log_of_a_child_without_a_json_line(tmp_path):
    log = str(tmp_path / "s.log")
    with pytest.raises(SystemExit) as e:
        benchlib.run_step(child("print('nothing of use')"), 20, log)
    assert "printed no JSON line" in str(e.value) and log in str(e.value)


def test_optional_route(monkeypatch):
    monkeypatch.setattr(benchlib, "timed", lambda torch, fn, reps: fn())

    def fault():
        raise RuntimeError("HIP error: an illegal memory access was encountered")

    def missing():
        raise RuntimeError('"replication_pad2d_cuda" not implemented for \'Byte\'' + " and more" * 40)

    fine = lambda: None
    with pytest.raises(RuntimeError, match="illegal memory access"):
        benchlib.optional_route(None, fault)
    route, why = benchlib.optional_route(None, missing)
    assert route is None and len(why) == 200 and why.startswith('"replication_pad2d_cuda" not implemented')
    assert benchlib.optional_route(None, fine) == (fine, None)


FAKE_TOOL = """import json, sys
a = sys.argv
print("# not the result")
print(json.dumps({"child": a[a.index("--child") + 1], "arguments": a[3:]}))
"""


def driven(tmp_path, monkeypatch, steps, table):
    monkeypatch.setattr(benchlib, "traced", lambda cmd, trace_dir: cmd)
    tool = tmp_path / "fake_bench.py"
    tool.write_text(FAKE_TOOL)
    args = argparse.Namespace(child=None, streams=8, per=4, valu_per_pair=9.6, steps=steps, step_timeout=20, out_dir=str(tmp_path / "out"), out=str(tmp_path / "all.json"))
    benchlib.drive(args, table, [sys.executable, str(tool)])


def test_traced():
    assert benchlib.traced(["python", "x"], "d") == ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", "d", "--", "python", "x"]


def test_drive_writes_what_the_tools_wrote(tmp_path, monkeypatch, capsys):
    seen = []

    def summarise(trace_dir, printed, earlier):
        seen.append((trace_dir, printed, dict(earlier)))
        return {"median_us": 1.5, "of": printed["child"]}

    driven(tmp_path, monkeypatch, "calls,trace", {"calls": ("calls", None), "trace": ("identity", summarise)})
    arguments = ["--streams", "8", "--per", "4", "--valu-per-pair", "9.6"]
    calls = {"child": "calls", "arguments": arguments}
    everything = {"calls": calls, "trace": {"median_us": 1.5, "of": "identity"}}
    out = tmp_path / "out"
    assert seen == [(str(out / "trace"), {"child": "identity", "arguments": arguments}, {"calls": calls})]
    for step, res in everything.items():
        assert (out / (step + ".json")).read_text() == json.dumps({step: res}) + "\n" and (out / (step + ".log")).exists()
    assert (tmp_path / "all.json").read_text() == json.dumps(everything, indent=1) + "\n"
    assert capsys.readouterr().out.splitlines() == ["# step calls", json.dumps({"calls": calls}), "# step trace", json.dumps({"trace": everything["trace"]})]


def test_drive_ends_at_an_unknown_step(tmp_path, monkeypatch):
    with pytest.raises(SystemExit, match="unknown step zzz"):
        driven(tmp_path, monkeypatch, "calls,zzz,trace", {"calls": ("calls", None), "trace": ("trace", None)})
    assert sorted(os.listdir(tmp_path / "out")) == ["calls.json", "calls.log"]


def test_drive_ends_at_a_summary_with_an_error(tmp_path, monkeypatch):
    with pytest.raises(SystemExit, match="trace: 3 launches in the trace, 4 planned"):
        driven(tmp_path, monkeypatch, "trace,calls", {"calls": ("calls", None), "trace": ("trace", lambda d, p, e: {"error": "3 launches in the trace, 4 planned"})})
    assert os.listdir(tmp_path / "out") == ["trace.log"] and not (tmp_path / "all.json").exists()


def test_export_float_says_which_child_its_trace_step_runs():
    from tools import export_float_bench
    assert export_float_bench.STEPS["trace"] == ("identity", export_float_bench.trace_summary)


def test_importing_the_tools_does_not_import_torch():
    tools = sorted({c[0] for c in CASES.values()})
    code = "import sys\n" + "".join(f"import tools.{t}\n" for t in tools) + "import tools.benchlib\nassert 'torch' not in sys.modules, 'torch'\nprint('fine')"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "fine", r.stderr
