"""Warped pictures in slot layout (hvq_warp_pictures) on the GPU: the measurement that sets the rule of hvq_wp_choose (hvq_warp.h).

Two measurements, each a child process of this driver under its own `timeout`; a step that fails ends the run:
  calls   128 640x480 4:2:0 streams, 8 resident pictures each, 1024 pictures per call, on natural content, through the identity, a
          half-sample translation, rotations by 5 and 45 degrees, the quarter turn into 480x640, zoom 1/2 into 320x240 and zoom 2, each
          under the chosen body, the forced direct body and the tiled body wherever LDS holds the box: (a) warp_pictures, (b)
          scale_pictures to the pictures' own geometry on the same pictures -- it reads and writes the same bytes: the memory floor of
          the identity --, (c) a torch route on a device copy of the same pictures: per plane a float view, affine_grid + grid_sample,
          rounding, cast, concatenation.  HIP-event timed per call on one stream in alternating rounds after a warm-up; medians over
          the rounds.  (a) must equal hvqm4_amd.warp on pictures read back under every body.
  trace   rocprofv3 --kernel-trace --stats around a child that launches warp_pictures per map and body and scale_pictures (identity) in a
          fixed order, one warm-up and `reps` launches each; one configuration (the identity under the direct body) is repeated at the
          start, in the middle and at the end: the largest distance between the medians of its three blocks is the run-to-run spread.
          Kernel times are read from the trace: median with min-max per map and body, and per map whether the body the rule chose is
          no slower than the direct one plus the spread.
One JSON line per measurement on stdout and in --out-dir.  torch is imported before the library, so both share one HIP runtime."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

W, H = 640, 480
SRC = (W, H, 2, 2)
BODIES = (("chosen", 0), ("direct", 1), ("tiled", 2))


def the_maps():
    """(label, Warp, target geometry)"""
    from hvqm4_amd import warp as wp
    c = (Fraction(W, 2), Fraction(H, 2))
    turn, size = wp.rotate90(1, W, H)
    return [("identity", wp.identity(), SRC), ("translate_half", wp.translate(Fraction(-1, 2), Fraction(-1, 2)), SRC), ("rotate5", wp.rotate(5, W, H), SRC),
            ("rotate45", wp.rotate(45, W, H), SRC), ("quarter_turn", turn, size + (2, 2)), ("zoom_half_to_320x240", wp.zoom(Fraction(1, 2)), (320, 240, 2, 2)),
            ("zoom2", wp.zoom(2, centre=c), SRC)]


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def torch_route(torch, copy, w, tg, chunk=128):
    """the warped pictures the way a pipeline without the call gets them: per plane a float view, affine_grid + grid_sample (bilinear,
    align_corners=False: sample centres at integer + 1/2, as here), rounding, cast, concatenation"""
    from hvqm4_amd import warp as wp
    tf = torch.nn.functional
    outs = []
    for at0 in range(0, copy.shape[0], chunk):
        part = copy[at0:at0 + chunk]
        n = part.shape[0]
        out, at = [], 0
        for p in range(3):
            (hd, vd), (hs, vs) = wp._samplings(SRC, tg, p)
            nx, ny = wp.plane_dims(SRC, p)
            mx, my = wp.plane_dims(tg, p)
            a, b, cc = w.m00 / 65536 * hd / hs, w.m01 / 65536 * vd / hs, w.t0 / 65536 / hs
            d, e, ff = w.m10 / 65536 * hd / vs, w.m11 / 65536 * vd / vs, w.t1 / 65536 / vs
            theta = torch.tensor([[a * mx / nx, b * my / nx, (a * mx + b * my + 2 * cc) / nx - 1], [d * mx / ny, e * my / ny, (d * mx + e * my + 2 * ff) / ny - 1]],
                                 dtype=torch.float32, device="cuda")
            plane = part[:, at:at + nx * ny].to(torch.float32).view(n, 1, ny, nx)
            at += nx * ny
            grid = tf.affine_grid(theta.expand(n, 2, 3), (n, 1, my, mx), align_corners=False)
            s = tf.grid_sample(plane, grid, mode="bilinear", padding_mode="border", align_corners=False)
            out.append(torch.floor(s + 0.5).clamp_(0, 255).to(torch.uint8).view(n, -1))
        outs.append(torch.cat(out, dim=1))
    return torch.cat(outs, dim=0)


def setup(args):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    from scale_bench import resident
    ctx = batch.Context(0)
    sids = resident(ctx, args.contents.split(",")[0], args.streams, args.per, args.distinct)
    a_s = [s for s in sids for _ in range(args.per)]
    a_o = [k for _ in sids for k in range(args.per)]
    return torch, ctx, a_s, a_o


def child_calls(args):
    import numpy as np
    from hvqm4_amd import scale
    from hvqm4_amd import warp as wp
    torch, ctx, a_s, a_o = setup(args)
    n = len(a_s)
    pb = scale.nbytes(*SRC)
    res = {"size": f"{W}x{H}", "pictures": n, "reps": args.reps, "rounds": args.rounds, "content": args.contents.split(",")[0], "maps": {}}
    copy = torch.empty((n, pb), dtype=torch.uint8, device="cuda")
    sout = torch.empty((n, pb), dtype=torch.uint8, device="cuda")
    probe = list(range(0, n, max(1, n // 8)))
    host = {i: ctx.read_picture(a_s[i], a_o[i]) for i in probe}
    for at in range(0, n, 64):                                  # the device copy the torch route works on
        copy[at:at + 64] = torch.from_numpy(np.stack([ctx.read_picture(a_s[i], a_o[i]) for i in range(at, min(n, at + 64))])).cuda()
    ident = lambda: ctx.scale_pictures(a_s, a_o, (W, H), out=sout)
    timed(torch, ident, args.warmup)
    for label, w, tg in the_maps():
        out = torch.empty((n, scale.nbytes(*tg)), dtype=torch.uint8, device="cuda")
        call = lambda: ctx.warp_pictures(a_s, a_o, w, tg[:2], tg[2:], out=out)
        route = lambda: torch_route(torch, copy, w, tg)
        want = {i: wp.of_picture(host[i], SRC, w, tg) for i in probe}
        r = {"bodies_of_planes": [wp.body(w, SRC, tg, p) for p in (0, 1)], "target": list(tg), "scale_identity_ms": [], "torch_ms": []}
        agree = True
        for name, force in BODIES:
            ctx.warp_force_direct(force)
            timed(torch, call, args.warmup)
            got = out.cpu().numpy()
            agree = agree and all(np.array_equal(got[i], want[i]) for i in probe)
            r[name + "_ms"] = []
        try:                                                    # a torch build without this sampler: the route is reported as missing
            timed(torch, route, 1)
            off = int((route().to(torch.int16) - out.to(torch.int16)).abs().max())
        except RuntimeError as e:
            if "HIP" in str(e) or "illegal" in str(e):              # a fault of the device, not a missing operator: nothing more is started
                raise
            off, route = str(e)[:200], None
        for _ in range(args.rounds):
            for name, force in BODIES:
                ctx.warp_force_direct(force)
                r[name + "_ms"].append(round(timed(torch, call, args.reps), 4))
            r["scale_identity_ms"].append(round(timed(torch, ident, args.reps), 4))
            if route:
                r["torch_ms"].append(round(timed(torch, route, max(1, args.reps // 10)), 4))
        ctx.warp_force_direct(0)
        for k in ("chosen", "direct", "tiled", "scale_identity", "torch"):
            r[k + "_median_ms"] = statistics.median(r[k + "_ms"]) if r[k + "_ms"] else None
        r["torch_over_chosen"] = round(r["torch_median_ms"] / r["chosen_median_ms"], 1) if route else None
        r["equal_host_module_under_every_body"] = bool(agree)
        r["torch_route_largest_difference"] = off
        res["maps"][label] = r
    ctx.close()
    print(json.dumps(res))


def child_trace(args):
    """the launches the trace is taken of, in this order: the spread block, per map and body 1 + reps of the warp kernel, the spread block
    again after the fourth map and at the end, then the scale kernel (identity)"""
    from hvqm4_amd import scale
    from hvqm4_amd import warp as wp
    torch, ctx, a_s, a_o = setup(args)
    n = len(a_s)
    out = torch.empty((n, scale.nbytes(W, H, 2, 2)), dtype=torch.uint8, device="cuda")

    def block(w, tg, force):
        ctx.warp_force_direct(force)
        o = out if tg == SRC else torch.empty((n, scale.nbytes(*tg)), dtype=torch.uint8, device="cuda")
        for _ in range(1 + args.reps):
            ctx.warp_pictures(a_s, a_o, w, tg[:2], tg[2:], out=o)
        torch.cuda.synchronize()
    block(wp.identity(), SRC, 1)
    for i, (_label, w, tg) in enumerate(the_maps()):
        for _name, force in BODIES:
            block(w, tg, force)
        if i == 3:
            block(wp.identity(), SRC, 1)
    block(wp.identity(), SRC, 1)
    ctx.warp_force_direct(0)
    for _ in range(1 + args.reps):
        ctx.scale_pictures(a_s, a_o, (W, H), out=out)
    torch.cuda.synchronize()
    ctx.close()
    print(json.dumps({"launches": 1 + args.reps, "pictures": n, "content": args.contents.split(",")[0]}))


def trace_summary(trace_dir, plan):
    from hvqm4_amd import warp as wp
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return {"error": f"no kernel trace under {trace_dir}"}
    rows = {"hvq_warp_kernel": [], "hvq_scale_kernel": []}
    with open(files[0], newline="") as f:
        for row in csv.DictReader(f):
            name = (row.get("Kernel_Name") or row.get("Name") or "").split("(")[0].strip()
            name = name[:-3] if name.endswith(".kd") else name
            k = name.split(" ")[-1]
            if k in rows:
                rows[k].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"]), row.get("VGPR_Count"), row.get("LDS_Block_Size"),
                                row.get("Scratch_Size")))
    per = plan["launches"]
    maps = the_maps()
    wk, sc = sorted(rows["hvq_warp_kernel"]), sorted(rows["hvq_scale_kernel"])
    blocks = 3 + 3 * len(maps)
    if len(wk) != per * blocks or len(sc) != per:
        return {"error": f"{len(wk)} warp and {len(sc)} scale launches in the trace, {per * blocks} and {per} planned"}

    def stats(r):
        d = sorted(x[1] for x in r[1:])                                               # without the warm-up launch
        return {"launches": len(d), "median_us": round(statistics.median(d) / 1e3, 1), "min_us": round(d[0] / 1e3, 1), "max_us": round(d[-1] / 1e3, 1)}

    res = {"pictures": plan["pictures"], "content": plan["content"], "vgprs": wk[0][2], "lds": wk[0][3], "scratch": wk[0][4], "maps": {}}
    cut = [wk[i * per:(i + 1) * per] for i in range(blocks)]
    spread_blocks = [stats(cut[0]), stats(cut[1 + 3 * 4]), stats(cut[-1])]
    rest = cut[1:1 + 3 * 4] + cut[2 + 3 * 4:-1]
    med = [b["median_us"] for b in spread_blocks]
    res["spread"] = {"configuration": "identity, direct body", "blocks": spread_blocks, "spread_us": round(max(med) - min(med), 1)}
    res["hvq_scale_kernel_identity"] = stats(sc)
    ok = True
    for i, (label, w, tg) in enumerate(maps):
        m = {name: stats(rest[3 * i + j]) for j, (name, _f) in enumerate(BODIES)}
        m["bodies_of_planes"] = [wp.body(w, SRC, tg, p) for p in (0, 1)]
        m["chosen_no_slower_than_direct_plus_spread"] = m["chosen"]["median_us"] <= m["direct"]["median_us"] + res["spread"]["spread_us"]
        m["tiled_minus_direct_us"] = round(m["tiled"]["median_us"] - m["direct"]["median_us"], 1)
        ok = ok and m["chosen_no_slower_than_direct_plus_spread"]
        res["maps"][label] = m
    res["rule_agrees"] = ok
    return res


def run(cmd, limit, log):
    """one GPU step under its own time limit; a failed step ends the run"""
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, capture_output=True, text=True)
    with open(log, "w") as f:
        f.write(r.stdout + "\n--- stderr ---\n" + r.stderr[-20000:])
    if r.returncode:
        sys.exit(f"{' '.join(cmd[:6])} ... ended with status {r.returncode}: see {log}")
    return [l for l in r.stdout.splitlines() if l.startswith("{")][-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("calls", "trace"), default=None)
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--per", type=int, default=8, help="resident pictures per stream")
    ap.add_argument("--distinct", type=int, default=2, help="distinct clips dealt over the streams")
    ap.add_argument("--contents", default="natural")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", default="calls,trace")
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out-dir", default="warp_bench_out")
    ap.add_argument("--out", default=None, help="all measurements as one JSON file (profiles/warp_bench.json)")
    args = ap.parse_args()
    if args.child:
        return {"calls": child_calls, "trace": child_trace}[args.child](args)
    os.makedirs(args.out_dir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    common = ["--streams", str(args.streams), "--per", str(args.per), "--distinct", str(args.distinct), "--reps", str(args.reps), "--warmup", str(args.warmup),
              "--rounds", str(args.rounds), "--contents", args.contents]
    everything = {}
    for step in args.steps.split(","):
        print(f"# step {step}", flush=True)
        if step == "calls":
            res = json.loads(run(me + ["--child", step] + common, args.step_timeout, os.path.join(args.out_dir, step + ".log")))
        elif step == "trace":
            tdir = os.path.join(args.out_dir, "trace")
            line = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--"] + me + ["--child", "trace"] + common,
                       args.step_timeout, os.path.join(args.out_dir, "trace.log"))
            res = trace_summary(tdir, json.loads(line))
            if "error" in res:
                sys.exit(f"trace: {res['error']}")
        else:
            sys.exit(f"unknown step {step}")
        everything[step] = res
        line = json.dumps({step: res})
        print(line, flush=True)
        with open(os.path.join(args.out_dir, step + ".json"), "w") as f:
            f.write(line + "\n")
        if args.out:
            with open(args.out, "w") as f:
                json.dump(everything, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
