"""What the feature benchmarks (tools/*_bench.py) share: the resident workload, HIP-event timing, a GPU step as a child process under its own
time limit, the reader of a rocprofv3 kernel trace, and the driver of a tool's steps.  A tool is its workload, its `child_*` functions and
a step table on `drive`.  A step guarantees: its own `timeout`; a step that fails, or whose summary has an "error", ends the run, so that
nothing more is started on a device that faulted; one kernel trace per trace directory.  One JSON line per step on stdout and in
--out-dir.  torch and hvqm4_amd are imported inside the functions that need them (torch before the library, so both share one HIP
runtime): this module and the tools import without a GPU."""
import collections
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8.0e12
SAMPLINGS = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}
DEVICE_FAULT = ("HIP", "illegal")                    # in the text of a RuntimeError: a fault of the device, not a missing operator
DRIVER_ONLY = ("child", "steps", "step_timeout", "out_dir", "out")

# kernel: the exact name; shown: the name with its template arguments, as a tool reports it
Launch = collections.namedtuple("Launch", "start ns shown vgprs lds scratch kernel")


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def resident(ctx, *, preset, sampling="420", streams, per, distinct, w=640, h=480):
    """`streams` open streams with `per` decoded pictures each, of `distinct` synthetic clips dealt over them -> the stream ids"""
    from hvqm4_amd.container import video_pictures
    from hvqm4_amd.synth import SynthConfig, make_clip
    hs, vs = SAMPLINGS[sampling]
    clips = [make_clip(SynthConfig(width=w, height=h, version="1.5", gop="IPBBPBBPBBPBBPBB", seed=1000 + i, preset=preset, sampling=sampling))
             for i in range(distinct)]
    pics = [[(ft, bytes(p)) for ft, _d, p in video_pictures(c.data)][:per] for c in clips]
    sids = [ctx.open_stream(w, h, hs, vs, True, per + 2) for _ in range(streams)]
    a_s, a_t, a_p = [], [], []
    for k in range(per):                                   # decode order, streams interleaved
        for i, sid in enumerate(sids):
            ft, p = pics[i % distinct][k]
            a_s.append(sid); a_t.append(ft); a_p.append(p)
    ctx.submit_many(a_s, a_t, a_p, threads=16)
    ctx.flush()
    ctx.sync()
    return sids


def picture_lists(sids, per):
    """(stream ids, ordinals) of every resident picture, stream by stream"""
    return [s for s in sids for _ in range(per)], [k for _ in sids for k in range(per)]


def optional_route(torch, route):
    """one run of a torch route that a torch build may lack an operator for -> (route, None), or (None, the first 200 characters of the
    error): the route is reported as missing.  After a fault of the device the error is raised again: nothing more is started"""
    try:
        timed(torch, route, 1)
    except RuntimeError as e:
        if any(p in str(e) for p in DEVICE_FAULT):
            raise
        return None, str(e)[:200]
    return route, None


def run_step(cmd, limit, log):
    """one GPU step under its own time limit -> the last JSON line it printed; a failed step ends the run"""
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, capture_output=True, text=True)
    with open(log, "w") as f:
        f.write(r.stdout + "\n--- stderr ---\n" + r.stderr[-20000:])
    if r.returncode:
        sys.exit(f"{' '.join(cmd[:6])} ... ended with status {r.returncode}: see {log}")
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if not lines:
        sys.exit(f"{' '.join(cmd[:6])} ... printed no JSON line: see {log}")
    return lines[-1]


def traced(cmd, trace_dir):
    return ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "--"] + cmd


def read_kernel_trace(trace_dir, kernels):
    """the launches of the named kernels in the one kernel trace under trace_dir, sorted by start; {"error": ...} without exactly one trace"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return {"error": f"no kernel trace under {trace_dir}"}
    if len(files) > 1:
        return {"error": f"{len(files)} kernel traces under {trace_dir}: which run they are of cannot be told, give a fresh --out-dir"}
    rows = []
    with open(files[0], newline="") as f:
        for row in csv.DictReader(f):
            shown = (row.get("Kernel_Name") or row.get("Name") or "").split("(")[0]
            name = shown.strip()
            name = (name[:-3] if name.endswith(".kd") else name).split("<")[0].split(" ")[-1]
            mangled = re.match(r"_Z(\d+)", name)                # rocprofv3 leaves some instantiations (_Float16) mangled: _Z<length><name>...
            if mangled:
                name = name[mangled.end():mangled.end() + int(mangled.group(1))]
            if name in kernels:
                rows.append(Launch(int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"]), shown,
                                   row.get("VGPR_Count"), row.get("LDS_Block_Size"), row.get("Scratch_Size"), name))
    return sorted(rows)


def cut_by_plan(launches, plan):
    """plan: (label, kernel or None for any, count) in launch order -> {label: its launches}; {"error": ...} for another total or order"""
    total = sum(count for _l, _k, count in plan)
    if len(launches) != total:
        return {"error": f"{len(launches)} launches of the kernels in the trace, {total} planned"}
    cut, at = {}, 0
    for label, kernel, count in plan:
        cut[label] = launches[at:at + count]
        at += count
        if kernel and any(l.kernel != kernel for l in cut[label]):
            return {"error": f"{label}: the launches in the trace are not in the planned order"}
    return cut


def read_planned(trace_dir, plan, kernels=None):
    """read_kernel_trace of the plan's kernels, cut by the plan"""
    launches = read_kernel_trace(trace_dir, kernels or {kernel for _l, kernel, _c in plan})
    return launches if isinstance(launches, dict) else cut_by_plan(launches, plan)


def read_per_kernel(trace_dir, kernels, count):
    """for a tool whose calls launch several kernels in turn, so that a kernel's launches are no block of the trace: {kernel: its `count`
    launches}; {"error": ...} for another number.  The order between the kernels goes unchecked"""
    launches = read_kernel_trace(trace_dir, kernels)
    if isinstance(launches, dict):
        return launches
    cut = {k: [l for l in launches if l.kernel == k] for k in kernels}
    for k, r in cut.items():
        if len(r) != count:
            return {"error": f"{len(r)} launches of {k} in the trace, {count} planned"}
    return cut


def launch_stats(durations_ns):
    d = sorted(durations_ns)
    return {"launches": len(d), "median_us": round(statistics.median(d) / 1e3, 1), "min_us": round(d[0] / 1e3, 1), "max_us": round(d[-1] / 1e3, 1)}


def resources(launch):
    return {"vgprs": launch.vgprs, "lds": launch.lds, "scratch": launch.scratch}


def add_common_arguments(ap, *, children, reps, warmup, rounds, steps, out_dir, step_timeout=300, distinct=2, out=None):
    """the arguments every tool has, with the tool's defaults; out: the name of the option for the file of all steps, where the tool has one"""
    ap.add_argument("--child", choices=children, default=None)
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--per", type=int, default=8, help="resident pictures per stream")
    ap.add_argument("--distinct", type=int, default=distinct, help="distinct clips dealt over the streams")
    ap.add_argument("--reps", type=int, default=reps)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--rounds", type=int, default=rounds)
    ap.add_argument("--steps", default=steps)
    ap.add_argument("--step-timeout", type=int, default=step_timeout)
    ap.add_argument("--out-dir", default=out_dir)
    if out:
        ap.add_argument(out, dest="out", default=None, help="all measurements as one JSON file")


def drive(args, steps, me):
    """steps: step -> (child, summary or None).  Per step of --steps: `me --child child` with the tool's arguments under the step's time
    limit; with a summary, under rocprofv3 into <out-dir>/<step>, and the result is summary(trace directory, what the child printed, the
    results so far).  The result goes to stdout and <out-dir>/<step>.json, and all of them so far into --out"""
    os.makedirs(args.out_dir, exist_ok=True)
    common = [x for k, v in vars(args).items() if k not in DRIVER_ONLY for x in ("--" + k.replace("_", "-"), str(v))]
    everything = {}
    for step in args.steps.split(","):
        print(f"# step {step}", flush=True)
        if step not in steps:
            sys.exit(f"unknown step {step}")
        child, summary = steps[step]
        cmd = me + ["--child", child] + common
        tdir = os.path.join(args.out_dir, step)
        res = json.loads(run_step(traced(cmd, tdir) if summary else cmd, args.step_timeout, os.path.join(args.out_dir, step + ".log")))
        if summary:
            res = summary(tdir, res, everything)
            if "error" in res:
                sys.exit(f"{step}: {res['error']}")
        everything[step] = res
        line = json.dumps({step: res})
        print(line, flush=True)
        with open(os.path.join(args.out_dir, step + ".json"), "w") as f:
            f.write(line + "\n")
        if getattr(args, "out", None):
            with open(args.out, "w") as f:
                json.dump(everything, f, indent=1)
                f.write("\n")
