"""Float export (hvq_export_tensors, Context.export_float) on the GPU: 128 dense 640x480 4:2:0 streams, 8 resident pictures each.

Four measurements (steps of tools/benchlib.py; --steps defaults to the first two):
  trace   the kernel trace of a child (`identity`) that exports all 1024 pictures at their own size (the identity body) as
          float32 / float16 / bfloat16, and -- in the same process, on the same box -- as uint8 planar RGB and RGB24 through
          hvq_export_pictures.  Kernel times are read from the trace; bytes = source planes read + destination written; share of
          8 TB/s.
  route   the fused call against the route a user of the uint8 export takes: export(..., "rgbp"), .to(dtype), crop,
          F.interpolate(bilinear), normalise in torch (in place).  Both event-timed on one stream, alternating rounds, 640x480 ->
          same size and -> 224x224, float32 and float16.
  aa      the antialiased call (export_float(antialias=True), hvq_export_resampled) for 128 pictures (16 streams of 8) 640x480 ->
          224x224 and -> 320x240, float32 and float16, four legs: (a) the call as the library runs it (the tiled body at these shapes),
          (b) the same forced to the direct body (HVQ_FILTER_TRIANGLE_DIRECT: an argument for this tool and the tests, not a switch
          of the product), (c) the plain two-tap call at the same shapes, (d) the torch route export("rgbp") -> .float() ->
          F.interpolate(antialias=True) -> normalise.  Event-timed on one stream in alternating rounds.
  aa_trace  the kernel trace of legs (a), (b), (c) in a fixed order: the kernel times of the legs.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.benchlib import PEAK, add_common_arguments, drive, launch_stats, picture_lists, read_kernel_trace, read_planned, resident, timed  # noqa: E402

W, H = 640, 480
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ES = {"float32": 4, "float16": 2, "bfloat16": 2}
KERNELS = ("hvq_yuv_tensor_kernel", "hvq_yuv_resample_kernel", "hvq_yuv_rgb_kernel")


def setup(args):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    all_s, all_o = picture_lists(resident(ctx, preset="dense", streams=args.streams, per=args.per, distinct=args.distinct), args.per)
    return torch, ctx, all_s, all_o


def child_identity(args):
    """the launches the trace is taken of; the event-timed call rate (host-bound at 1024 destinations per call) goes to stdout"""
    torch, ctx, all_s, all_o = setup(args)
    n = len(all_s)
    res = {"pictures": n, "size": f"{W}x{H}", "reps": args.reps}
    for dt in ES:
        out = torch.empty((n, 3, H, W), dtype=getattr(torch, dt), device="cuda")
        fn = lambda: ctx.export_float(all_s, all_o, out, mean=MEAN, std=STD)
        timed(torch, fn, args.warmup)
        res[f"export_float_{dt}_call_ms"] = round(timed(torch, fn, args.reps), 4)
        del out
        torch.cuda.empty_cache()
    for fmt in ("rgbp", "rgb"):
        out = torch.empty((n, 3, H, W) if fmt == "rgbp" else (n, H, W, 3), dtype=torch.uint8, device="cuda")
        fn = lambda: ctx.export(all_s, all_o, out, fmt)
        timed(torch, fn, args.warmup)
        res[f"export_{fmt}_call_ms"] = round(timed(torch, fn, args.reps), 4)
        del out
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(res))


def child_route(args):
    torch, ctx, all_s, all_o = setup(args)
    import torch.nn.functional as F
    from hvqm4_amd.export import normalisation
    n = len(all_s)
    mul, add = normalisation(MEAN, STD)
    res = {"pictures": n, "source": f"{W}x{H}", "reps": args.reps, "rounds": args.rounds}
    u8 = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
    for hw in ((H, W), (224, 224)):
        for dt in ("float32", "float16"):
            td = getattr(torch, dt)
            m = torch.tensor(mul, dtype=td, device="cuda").view(1, 3, 1, 1)
            a = torch.tensor(add, dtype=td, device="cuda").view(1, 3, 1, 1)
            out = torch.empty((n, 3) + hw, dtype=td, device="cuda")
            keep = {}

            def fused():
                ctx.export_float(all_s, all_o, out, mean=MEAN, std=STD)

            def route():
                ctx.export(all_s, all_o, u8, "rgbp")
                x = u8.to(td)
                if hw != (H, W):
                    x = F.interpolate(x, size=hw, mode="bilinear", align_corners=False)
                keep["x"] = x.mul_(m).add_(a)

            timed(torch, fused, args.warmup)
            timed(torch, route, args.warmup)
            worst = float((out.float() - keep["x"].float()).abs().max())        # the two routes agree up to rounding
            rows = {"fused_ms": [], "route_ms": []}
            for _ in range(args.rounds):
                rows["fused_ms"].append(round(timed(torch, fused, args.reps), 4))
                rows["route_ms"].append(round(timed(torch, route, args.reps), 4))
            src = W * H * 3 // 2
            rows["fused_bytes"] = n * (src + 3 * hw[0] * hw[1] * ES[dt])
            rows["speedup"] = round(statistics.median(rows["route_ms"]) / statistics.median(rows["fused_ms"]), 2)
            rows["max_abs_difference"] = worst
            res[f"{hw[1]}x{hw[0]}_{dt}"] = rows
            del out, m, a
            keep.clear()
            torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(res))


AA_SHAPES = ((224, 224), (240, 320))
AA_DTYPES = ("float32", "float16")


def aa_setup(args):
    args.streams, args.per = args.aa_streams, 8
    return setup(args)


def aa_legs(torch, ctx, all_s, all_o, hw, dt):
    """the four legs of one shape and dtype as closures: {leg: (fn, result tensor getter)}"""
    import torch.nn.functional as F
    from hvqm4_amd.export import FILTER_TRIANGLE, FILTER_TRIANGLE_DIRECT, normalisation
    n = len(all_s)
    td = getattr(torch, dt)
    mul, add = normalisation(MEAN, STD)
    m = torch.tensor(mul, dtype=td, device="cuda").view(1, 3, 1, 1)
    a = torch.tensor(add, dtype=td, device="cuda").view(1, 3, 1, 1)
    outs = {k: torch.empty((n, 3) + hw, dtype=td, device="cuda") for k in "abc"}
    u8 = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
    keep = {}

    def leg_d():
        ctx.export(all_s, all_o, u8, "rgbp")
        keep["d"] = F.interpolate(u8.to(td), size=hw, mode="bilinear", align_corners=False, antialias=True).mul_(m).add_(a)

    legs = {"a_tiled": lambda: ctx._export_float(all_s, all_o, outs["a"], None, MEAN, STD, 1 / 255, FILTER_TRIANGLE),
            "b_direct": lambda: ctx._export_float(all_s, all_o, outs["b"], None, MEAN, STD, 1 / 255, FILTER_TRIANGLE_DIRECT),
            "c_plain": lambda: ctx.export_float(all_s, all_o, outs["c"], mean=MEAN, std=STD),
            "d_torch": leg_d}
    return legs, outs, keep


def child_aa(args):
    torch, ctx, all_s, all_o = aa_setup(args)
    from hvqm4_amd._lib import lib
    res = {"pictures": len(all_s), "source": f"{W}x{H}", "reps": args.reps, "rounds": args.rounds}
    for hw in AA_SHAPES:
        for dt in AA_DTYPES:
            legs, outs, keep = aa_legs(torch, ctx, all_s, all_o, hw, dt)
            for fn in legs.values():
                timed(torch, fn, args.warmup)
            rows = {k: [] for k in legs}
            for _ in range(args.rounds):
                for k, fn in legs.items():
                    rows[k].append(round(timed(torch, fn, args.reps), 4))
            out = {k + "_ms": v for k, v in rows.items()}
            out.update({k + "_median_ms": statistics.median(v) for k, v in rows.items()})
            out["tile_rows"] = lib().hvq_resample_tile_rows(W, H, hw[1], hw[0])
            out["bodies_equal_bits"] = bool(torch.equal(outs["a"], outs["b"]))
            out["max_abs_difference_to_torch"] = float((outs["a"].float() - keep["d"].float()).abs().max())
            res[f"{hw[1]}x{hw[0]}_{dt}"] = out
            del legs, outs, keep
            torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(res))


def child_aa_trace(args):
    """legs (a), (b), (c) in a fixed order, `reps` launches each after one warm-up launch: aa_trace_summary reads them by order"""
    torch, ctx, all_s, all_o = aa_setup(args)
    plan = []
    for hw in AA_SHAPES:
        for dt in AA_DTYPES:
            legs, outs, keep = aa_legs(torch, ctx, all_s, all_o, hw, dt)
            for k in ("a_tiled", "b_direct", "c_plain"):
                for _ in range(1 + args.reps):
                    legs[k]()
                torch.cuda.synchronize()
                plan.append([f"{hw[1]}x{hw[0]}_{dt}_{k}", 1 + args.reps])
            del legs, outs, keep
            torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps({"plan": plan}))


def aa_trace_summary(trace_dir, printed, _earlier=None):
    cut = read_planned(trace_dir, [(label, None, count) for label, count in printed["plan"]], KERNELS[:2])
    if "error" in cut:
        return cut
    res = {}
    for label, part in cut.items():
        part = part[1:]                                                           # without the warm-up launch
        res[label] = {"kernel": part[0].shown, **launch_stats(l.ns for l in part), "lds": part[0].lds}
    return res


def trace_summary(trace_dir, calls, _earlier=None):
    """what the child printed, and median / min of every export kernel in the kernel trace -> share of 8 TB/s"""
    launches = read_kernel_trace(trace_dir, KERNELS)
    if isinstance(launches, dict):
        return launches
    dur = {}
    for l in launches:
        dur.setdefault(l.shown, []).append(l.ns)
    src = W * H * 3 // 2
    per_px = {"<float>": 12, "<_Float16>": 6, "<hvq_bf16>": 6, "hvq_yuv_rgb_kernel": 3}
    res = {}
    for name, d in sorted(dur.items()):
        d = sorted(d)
        big = [x for x in d if x > 0.5 * d[-1]]                                   # the 1024-picture launches, not the warm-up of setup
        b = next((v for k, v in per_px.items() if k in name), None)
        if b is None:
            continue
        by = calls["pictures"] * (src + b * W * H)
        med = statistics.median(big)
        res[name] = {"launches": len(big), "median_us": round(med / 1e3, 1), "min_us": round(big[0] / 1e3, 1), "bytes": by,
                     "of_peak_median": round(by / (med * 1e-9) / PEAK, 3), "of_peak_best": round(by / (big[0] * 1e-9) / PEAK, 3)}
    return {"calls": calls, "kernels": res}


STEPS = {"trace": ("identity", trace_summary), "route": ("route", None), "aa": ("aa", None), "aa_trace": ("aa_trace", aa_trace_summary)}


def main():
    ap = argparse.ArgumentParser()
    add_common_arguments(ap, children=("identity", "route", "aa", "aa_trace"), reps=30, warmup=3, rounds=5, steps="trace,route", step_timeout=400,
                         out_dir="export_float_bench_out")
    ap.add_argument("--aa-streams", type=int, default=16, help="streams of 8 resident pictures for the aa steps (16: 128 pictures)")
    args = ap.parse_args()
    if args.child:
        return {"identity": child_identity, "route": child_route, "aa": child_aa, "aa_trace": child_aa_trace}[args.child](args)
    drive(args, STEPS, [sys.executable, os.path.abspath(__file__)])


if __name__ == "__main__":
    main()
