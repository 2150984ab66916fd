"""Lookup tables on pictures in slot layout (hvq_map_pictures, hvq_histogram_tables, Context.equalize_pictures) on the GPU.

Two measurements (steps of tools/benchlib.py), both on 128 640x480 4:2:0 streams with 8 resident pictures each, 1024 pictures a call:
  calls   time per call, HIP-event timed on one stream in alternating rounds after a warm-up, medians over the rounds, of: inversion with
          one shared table; 1024 distinct tables; planes = 1 (luma only); in place (from a device copy of the pictures into itself);
          histogram_tables for 1024 records under each kind; the whole equalize_pictures chain; and in the same session rank_pictures
          with the identity (the rank kernel's copy body) and scale_pictures to the pictures' own geometry, which move the same bytes.
          The torch route: per plane lut[plane.long()] on a device copy of the pictures, and for the chain export() of the luma planes,
          torch.bincount + cumsum for the equalisation tables, and a gather.  The results of the calls must equal hvqm4_amd.maps on
          pictures read back, and so must the torch route.
  trace   the kernel trace of a child that launches the same calls in a fixed order, one warm-up and `reps` launches each; the chain's
          three kernels are launched as three blocks.  Kernel times are read from the trace: median with min-max per row, the aim (map
          kernel <= 1.5 x the rank copy-body kernel of the same session) and the sum of the chain's kernels.
The one condition -- equalize_pictures per call is faster than the torch route of the same session -- is in the calls step.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.benchlib import (PEAK, add_common_arguments, drive, launch_stats, picture_lists, read_planned, resident, resources, timed)  # noqa: E402

W, H = 640, 480
SRC = (W, H, 2, 2)
PIC_BYTES = W * H * 3 // 2
KINDS = ("identity", "flat", "equalize", "stretch", "otsu")


def the_rules():
    from hvqm4_amd import maps as M
    return dict(zip(KINDS, (M.keep(), M.flat(7), M.equalize(), M.stretch(10, 10), M.otsu())))


def trace_plan():
    """(label, kernel) of the trace step's blocks in launch order.  The first and the third fill what later rows work on: the device copy of
    the pictures (the in-place row) and the histogram records"""
    return [("scale_identity", "hvq_scale_kernel"), ("rank_identity", "hvq_rank_kernel"), ("chain_histograms", "hvq_histogram_kernel")] + \
           [(label, "hvq_map_kernel") for label in ("invert_shared", "distinct_tables", "luma_only", "inplace")] + \
           [("tables_" + k, "hvq_tables_kernel") for k in KINDS] + [("chain_tables", "hvq_tables_kernel"), ("chain_map", "hvq_map_kernel")]


def setup(args, fill=True):
    import numpy as np
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    from hvqm4_amd import maps as M
    ctx = batch.Context(0)
    a_s, a_o = picture_lists(resident(ctx, preset=args.contents.split(",")[0], streams=args.streams, per=args.per, distinct=args.distinct), args.per)
    n = len(a_s)
    rng = np.random.default_rng(5)
    distinct = np.stack([np.stack([rng.permutation(256).astype(np.uint8) for _ in range(3)]) for _ in range(n)])
    S = {"torch": torch, "ctx": ctx, "a_s": a_s, "a_o": a_o, "n": n,
         "shared": torch.from_numpy(M.pack([M.invert()])).cuda(), "distinct": torch.from_numpy(distinct).cuda(), "distinct_host": distinct,
         "out": torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda"), "copy": torch.empty((n, PIC_BYTES), dtype=torch.uint8, device="cuda")}
    S["hist"] = torch.empty((n, 3, 256), dtype=torch.int32, device="cuda")
    if fill:                                                               # the trace child leaves both to the first rows of its plan
        ctx.scale_pictures(a_s, a_o, (W, H), out=S["copy"])               # a device copy of the pictures: the in-place row and the torch route work on it
        ctx.picture_histograms(a_s, a_o, out=S["hist"])
    S["tables"] = torch.empty((n, 3, 256), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return S


def the_calls(S):
    """label -> the call, in the trace plan's order (the chain as one call under `chain`, and as its three launches)"""
    ctx, a_s, a_o, n, out = S["ctx"], S["a_s"], S["a_o"], S["n"], S["out"]
    rows = [S["copy"][i] for i in range(n)]
    rules = the_rules()
    calls = {"invert_shared": lambda: ctx.map_pictures(a_s, a_o, S["shared"], out=out),
             "distinct_tables": lambda: ctx.map_pictures(a_s, a_o, S["distinct"], out=out),
             "luma_only": lambda: ctx.map_pictures(a_s, a_o, S["shared"], planes=1, out=out),
             "inplace": lambda: ctx.map_pictures(a_s, [-1] * n, S["shared"], src=rows, out=S["copy"])}
    for k in KINDS:
        calls["tables_" + k] = lambda k=k: ctx.histogram_tables(S["hist"], rules[k], out=S["tables"])
    calls["chain_histograms"] = lambda: ctx.picture_histograms(a_s, a_o, out=S["hist"])
    calls["chain_tables"] = lambda: ctx.histogram_tables(S["hist"], rules["equalize"].luma_only(), out=S["tables"])
    calls["chain_map"] = lambda: ctx.map_pictures(a_s, a_o, S["tables"], out=out)
    from hvqm4_amd import rank as R
    calls["rank_identity"] = lambda: ctx.rank_pictures(a_s, a_o, R.identity(), out=out)
    calls["scale_identity"] = lambda: ctx.scale_pictures(a_s, a_o, (W, H), out=S["copy"])
    return calls


def torch_map(torch, copy, lut):
    """per plane lut[plane.long()]; lut: uint8 [3, 256] on the device"""
    ny, nc = W * H, (W // 2) * (H // 2)
    return torch.cat([lut[p][copy[:, at:at + m].long()] for p, (at, m) in enumerate(((0, ny), (ny, nc), (ny + nc, nc)))], dim=1)


def torch_chain(torch, ctx, a_s, a_o, planar):
    """the equalisation of the luma planes the way a pipeline without the calls gets it: export (yuv444p), bincount per picture, cumsum,
    the table in integers, a gather.  -> uint8 [n, H, W]"""
    n = len(a_s)
    ctx.export(a_s, a_o, planar, "yuv444p")
    y = planar[:, 0].reshape(n, -1).long()
    h = torch.bincount((y + 256 * torch.arange(n, device=y.device)[:, None]).reshape(-1), minlength=256 * n).view(n, 256)
    c = h.cumsum(1)
    cmin = torch.where(h > 0, c, torch.full_like(c, 1 << 40)).min(1, keepdim=True).values
    d = (c[:, -1:] - cmin)
    lut = torch.where(d > 0, (2 * 255 * (c - cmin).clamp(min=0) + d) // (2 * d.clamp(min=1)), torch.arange(256, device=y.device)[None]).to(torch.uint8)
    return torch.gather(lut, 1, y).view(n, H, W)


def child_calls(args):
    import numpy as np
    from hvqm4_amd import histograms as Hs
    from hvqm4_amd import maps as M
    S = setup(args)
    torch, ctx, a_s, a_o, n = S["torch"], S["ctx"], S["a_s"], S["a_o"], S["n"]
    calls = the_calls(S)
    calls["chain"] = lambda: ctx.equalize_pictures(a_s, a_o, out=S["out"])
    res = {"size": f"{W}x{H}", "pictures": n, "reps": args.reps, "rounds": args.rounds, "content": args.contents.split(",")[0], "rows": {}}
    probe = list(range(0, n, max(1, n // 4)))
    host = {i: ctx.read_picture(a_s[i], a_o[i]) for i in probe}
    # what the calls compute, against the host module
    checks = {}
    calls["invert_shared"](); got = S["out"].cpu().numpy()
    checks["invert_shared"] = all(np.array_equal(got[i], 255 - host[i].reshape(-1)) for i in probe)
    calls["distinct_tables"](); got = S["out"].cpu().numpy()
    checks["distinct_tables"] = all(np.array_equal(got[i], M.of_picture(host[i].reshape(-1), SRC, M.from_lut(*S["distinct_host"][i]))) for i in probe)
    calls["luma_only"](); got = S["out"].cpu().numpy()
    checks["luma_only"] = all(np.array_equal(got[i], M.of_picture(host[i].reshape(-1), SRC, M.invert(), 1)) for i in probe)
    calls["chain"](); got = S["out"].cpu().numpy()
    want = {i: M.of_picture(host[i].reshape(-1), SRC, M.from_lut(*M.tables_of_records(Hs.of_picture(host[i].reshape(-1), *SRC), M.equalize().luma_only()))) for i in probe}
    checks["chain"] = all(np.array_equal(got[i], want[i]) for i in probe)
    calls["inplace"](); calls["inplace"]()                                  # twice inverted: the pictures again
    checks["inplace"] = all(np.array_equal(S["copy"][i].cpu().numpy(), host[i].reshape(-1)) for i in probe)
    # the torch routes
    lut = S["shared"][0]
    route_map = lambda: torch_map(torch, S["copy"], lut)
    planar = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
    route_chain = lambda: torch_chain(torch, ctx, a_s, a_o, planar)
    checks["torch_map"] = bool((route_map() == 255 - S["copy"]).all())
    y = route_chain().cpu().numpy()
    checks["torch_chain"] = all(np.array_equal(y[i].reshape(-1), want[i][:W * H]) for i in probe)
    labels = list(calls)
    for label in labels:
        timed(torch, calls[label], args.warmup)
    timed(torch, route_map, 1); timed(torch, route_chain, 1)
    ms = {label: [] for label in labels + ["torch_map", "torch_chain"]}
    for _ in range(args.rounds):
        for label in labels:
            ms[label].append(round(timed(torch, calls[label], args.reps), 4))
        ms["torch_map"].append(round(timed(torch, route_map, 2), 4))
        ms["torch_chain"].append(round(timed(torch, route_chain, 2), 4))
    for label, v in ms.items():
        res["rows"][label] = {"ms": v, "median_ms": statistics.median(v)}
    med = lambda label: res["rows"][label]["median_ms"]
    for label in ("invert_shared", "distinct_tables", "luma_only", "inplace", "rank_identity", "scale_identity"):
        res["rows"][label]["gb_per_s"] = round(2 * n * PIC_BYTES / (med(label) * 1e-3) / 1e9, 1)
    res["equal_host_module"] = checks
    res["torch_map_over_map"] = round(med("torch_map") / med("invert_shared"), 1)
    # the one condition, no tolerance
    res["condition"] = {"what": "equalize_pictures per call faster than export + bincount + cumsum + gather in torch, same session", "chain_ms": med("chain"),
                        "torch_chain_ms": med("torch_chain"), "torch_over_chain": round(med("torch_chain") / med("chain"), 1), "holds": med("chain") < med("torch_chain")}
    ctx.close()
    print(json.dumps(res))


def child_trace(args):
    """the launches the trace is taken of: per row of the plan 1 + reps launches"""
    S = setup(args, fill=False)
    calls = the_calls(S)
    for label, _kernel in trace_plan():
        for _ in range(1 + args.reps):
            calls[label]()
        S["torch"].cuda.synchronize()
    S["ctx"].close()
    print(json.dumps({"launches": 1 + args.reps, "pictures": S["n"]}))


def trace_summary(trace_dir, plan, _earlier=None):
    per = plan["launches"]
    cut = read_planned(trace_dir, [(label, kernel, per) for label, kernel in trace_plan()])
    if "error" in cut:
        return cut
    stats = lambda r: launch_stats(l.ns for l in r[1:])                               # without the warm-up launch
    res = {"pictures": plan["pictures"], "map_kernel": resources(cut["invert_shared"][0]), "tables_kernel": resources(cut["tables_otsu"][0])}
    moved = {"luma_only": 2 * plan["pictures"] * PIC_BYTES}
    for label, kernel in trace_plan():
        t = stats(cut[label])
        if kernel in ("hvq_map_kernel", "hvq_rank_kernel", "hvq_scale_kernel"):
            t["bytes"] = moved.get(label, 2 * plan["pictures"] * PIC_BYTES)
            t["of_peak_median"] = round(t["bytes"] / (t["median_us"] * 1e-6) / PEAK, 3)
        res[label] = t
    med = lambda label: res[label]["median_us"]
    res["aim"] = {"what": "map kernel (inversion, one shared table) <= 1.5 x the rank copy-body kernel, same session",
                  "map_over_rank_copy": round(med("invert_shared") / med("rank_identity"), 2), "met": med("invert_shared") <= 1.5 * med("rank_identity")}
    res["ratios"] = {"map_over_scale_identity": round(med("invert_shared") / med("scale_identity"), 2),
                     "distinct_over_shared": round(med("distinct_tables") / med("invert_shared"), 2),
                     "luma_only_over_shared": round(med("luma_only") / med("invert_shared"), 2),
                     "inplace_over_shared": round(med("inplace") / med("invert_shared"), 2)}
    res["chain_kernels_us"] = round(med("chain_histograms") + med("chain_tables") + med("chain_map"), 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    add_common_arguments(ap, children=("calls", "trace"), reps=20, warmup=3, rounds=5, steps="calls,trace", out_dir="map_bench_out", out="--out")
    ap.add_argument("--contents", default="natural")
    args = ap.parse_args()
    if args.child:
        return {"calls": child_calls, "trace": child_trace}[args.child](args)
    drive(args, {"calls": ("calls", None), "trace": ("trace", trace_summary)}, [sys.executable, os.path.abspath(__file__)])


if __name__ == "__main__":
    main()
