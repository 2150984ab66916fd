"""Perceptual hashes and nearest-hash search (hvq_picture_hashes / hvq_hash_nearest) on the GPU.

Three measurements (steps of tools/benchlib.py):
  hashes   128 640x480 4:2:0 streams, 8 resident pictures each, 1024 pictures per call, on dense, natural and flat content:
           (a) picture_hashes, (b) picture_metrics against zeros on the same pictures -- existing code that reads Y, U and V once, 1.5
           times the bytes (a) needs -- and (c) the torch route on the same pictures: export to YUV 4:4:4, area pooling of Y to 32 x 32,
           two matmuls with the DCT matrix, a median, bit packing.  HIP-event timed per call on one stream in alternating rounds after a
           warm-up; medians over the rounds; the factors (a)/(b) and (c)/(a).  (a) must equal hvqm4_amd.phash on pictures read back.
  nearest  16 384 x 16 384 and 65 536 x 65 536 random hashes: (a) hash_nearest, (b) a torch route (xor, a byte-table popcount, min over
           chunks of queries); pairs per second, the factor (b)/(a), and the share of the v_bcnt_u32_b32 issue bound reached (two per pair;
           --valu-per-pair is the inner loop's vector instructions per pair from profiles/phash_isa.txt).  (a) and (b) must agree.
  trace    the kernel trace of a child that launches picture_hashes, picture_metrics and hash_nearest in a fixed
           order, one warm-up and `reps` launches each.  Kernel times are read from the trace: median with min-max per kernel.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.benchlib import PEAK, add_common_arguments, drive, launch_stats, picture_lists, read_per_kernel, resident, resources, timed  # noqa: E402

CLOCK, SIMDS = 2.4e9, 1024                       # a wave64 vector instruction issues over 2 cycles on a SIMD
W, H = 640, 480
PIC_BYTES = W * H * 3 // 2
KERNELS = ("hvq_phash_cells_kernel", "hvq_phash_finish_kernel", "hvq_metrics_kernel", "hvq_hash_nearest_kernel")


def torch_route(torch, ctx, a_s, a_o, yuv, dct):
    """the hashes the way a pipeline without the call gets them: float arithmetic, so the bits are close to, not equal to, the call's"""
    ctx.export(a_s, a_o, yuv, "yuv444p")
    y = yuv[:, 0].float()
    m = torch.nn.functional.adaptive_avg_pool2d(y, (32, 32))
    f = (dct @ m @ dct.T).reshape(-1, 64)
    med = f.median(dim=1, keepdim=True).values
    weights = torch.arange(63, -1, -1, device=f.device, dtype=torch.int64)
    return ((f > med).to(torch.int64) << weights).sum(dim=1)


def child_hashes(args):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch, phash
    res = {"size": f"{W}x{H}", "pictures": args.streams * args.per, "reps": args.reps, "rounds": args.rounds, "contents": {}}
    dct = torch.from_numpy(phash.TABLE.astype("float32") / 4096).cuda()
    for preset in args.contents.split(","):
        ctx = batch.Context(0)
        a_s, a_o = picture_lists(resident(ctx, preset=preset, streams=args.streams, per=args.per, distinct=args.distinct), args.per)
        n = len(a_s)
        out = torch.empty((n, 4), dtype=torch.int64, device="cuda")
        met = torch.empty((n, 3, 4), dtype=torch.int64, device="cuda")
        yuv = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
        call = lambda: ctx.picture_hashes(a_s, a_o, out=out)
        metrics = lambda: ctx.picture_metrics(a_s, a_o, None, out=met)
        route = lambda: torch_route(torch, ctx, a_s, a_o, yuv, dct)
        for fn in (call, metrics, route):
            timed(torch, fn, args.warmup)
        got = phash.as_uint64(out.cpu().numpy()).tolist()
        probe = list(range(0, n, max(1, n // 16)))
        agree = all(got[i] == phash.of_picture(ctx.read_picture(a_s[i], a_o[i]), W, H) for i in probe)
        close = phash.hamming(route().cpu().numpy(), out[:, phash.PHASH].cpu().numpy())
        r = {"hashes_ms": [], "metrics_ms": [], "torch_ms": []}
        for _ in range(args.rounds):
            r["hashes_ms"].append(round(timed(torch, call, args.reps), 4))
            r["metrics_ms"].append(round(timed(torch, metrics, args.reps), 4))
            r["torch_ms"].append(round(timed(torch, route, max(1, args.reps // 5)), 4))
        for k in ("hashes", "metrics", "torch"):
            r[k + "_median_ms"] = statistics.median(r[k + "_ms"])
        r["hashes_over_metrics"] = round(r["hashes_median_ms"] / r["metrics_median_ms"], 2)
        r["torch_over_hashes"] = round(r["torch_median_ms"] / r["hashes_median_ms"], 1)
        r["hashes_luma_gb_per_s"] = round(n * W * H / (r["hashes_median_ms"] * 1e-3) / 1e9, 1)
        r["records_equal_host_module"] = bool(agree)
        r["torch_route_phash_bits_off_mean"] = round(float(close.mean()), 2)
        res["contents"][preset] = r
        ctx.close()
    print(json.dumps(res))


def torch_nearest(torch, q, db, table, chunk):
    best_d, best_j = [], []
    for at in range(0, q.numel(), chunk):
        x = (q[at:at + chunk, None] ^ db[None, :]).view(torch.uint8).view(-1, db.numel(), 8)
        d = table[x.long()].sum(dim=2, dtype=torch.int32)
        m = d.min(dim=1)
        best_d.append(m.values); best_j.append(m.indices)
    return torch.cat(best_d), torch.cat(best_j)


def child_nearest(args):
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    table = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.uint8, device="cuda")
    res = {"reps": args.reps, "rounds": args.rounds, "valu_per_pair": args.valu_per_pair, "sizes": {}}
    bcnt_bound = SIMDS * CLOCK / 2 * 64 / 2                     # pairs per second if nothing but the two v_bcnt per pair issued
    for n in (int(v) for v in args.nearest_sizes.split(",")):
        g = torch.Generator(device="cuda").manual_seed(n)
        h = torch.randint(-(1 << 62), 1 << 62, (n,), generator=g, device="cuda", dtype=torch.int64)
        q = h[torch.randperm(n, device="cuda", generator=g)] ^ 5
        out = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        call = lambda: ctx.hash_nearest(q, h, -1, 10, out=out)
        route = lambda: torch_nearest(torch, q, h, table, args.chunk)
        timed(torch, call, args.warmup)
        d, _j = route()
        agree = bool(torch.equal(out[:, 1], d))                 # distances: torch's min does not promise the first of equal ones
        r = {"nearest_ms": [], "torch_ms": []}
        for _ in range(args.rounds):
            r["nearest_ms"].append(round(timed(torch, call, args.reps), 4))
            r["torch_ms"].append(round(timed(torch, route, 1), 3))
        r["nearest_median_ms"] = statistics.median(r["nearest_ms"])
        r["torch_median_ms"] = statistics.median(r["torch_ms"])
        pairs = n * n
        r["pairs_per_s"] = round(pairs / (r["nearest_median_ms"] * 1e-3), -6)
        r["share_of_bcnt_issue_bound"] = round(r["pairs_per_s"] / bcnt_bound, 3)
        r["share_of_valu_issue_bound"] = round(r["pairs_per_s"] * args.valu_per_pair / (SIMDS * CLOCK / 2 * 64), 3)
        r["torch_over_nearest"] = round(r["torch_median_ms"] / r["nearest_median_ms"], 1)
        r["distances_agree_with_torch"] = agree
        res["sizes"][str(n)] = r
    ctx.close()
    print(json.dumps(res))


def child_trace(args):
    """the launches the trace is taken of: a picture_hashes call launches hvq_phash_cells_kernel and hvq_phash_finish_kernel in turn"""
    import torch
    torch.cuda.init()
    from hvqm4_amd import batch
    ctx = batch.Context(0)
    a_s, a_o = picture_lists(resident(ctx, preset="dense", streams=args.streams, per=args.per, distinct=args.distinct), args.per)
    n = len(a_s)
    out = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    met = torch.empty((n, 3, 4), dtype=torch.int64, device="cuda")
    for _ in range(1 + args.reps):
        ctx.picture_hashes(a_s, a_o, out=out)
    torch.cuda.synchronize()
    for _ in range(1 + args.reps):
        ctx.picture_metrics(a_s, a_o, None, out=met)
    torch.cuda.synchronize()
    nn = int(args.nearest_sizes.split(",")[0])
    h = torch.randint(-(1 << 62), 1 << 62, (nn,), device="cuda", dtype=torch.int64)
    near = torch.empty((nn, 4), dtype=torch.int32, device="cuda")
    for _ in range(1 + args.reps):
        ctx.hash_nearest(h, h, -1, 10, out=near)
    torch.cuda.synchronize()
    ctx.close()
    print(json.dumps({"launches": 1 + args.reps, "pictures": n, "nearest": nn}))


def trace_summary(trace_dir, plan, _earlier=None):
    cut = read_per_kernel(trace_dir, KERNELS, plan["launches"])
    if "error" in cut:
        return cut
    res = {"pictures": plan["pictures"], "nearest": plan["nearest"]}
    for k, r in cut.items():
        res[k] = {**launch_stats(l.ns for l in r[1:]), **resources(r[0])}         # without the warm-up launch
    luma, pic = plan["pictures"] * W * H, plan["pictures"] * PIC_BYTES
    res[KERNELS[0]].update({"bytes": luma, "of_peak_median": round(luma / (res[KERNELS[0]]["median_us"] * 1e-6) / PEAK, 3)})
    res[KERNELS[2]].update({"bytes": pic, "of_peak_median": round(pic / (res[KERNELS[2]]["median_us"] * 1e-6) / PEAK, 3)})
    res["hash_over_metrics_kernels"] = round((res[KERNELS[0]]["median_us"] + res[KERNELS[1]]["median_us"]) / res[KERNELS[2]]["median_us"], 2)
    res[KERNELS[3]]["pairs_per_s"] = round(plan["nearest"] ** 2 / (res[KERNELS[3]]["median_us"] * 1e-6), -6)
    return res


def main():
    ap = argparse.ArgumentParser()
    add_common_arguments(ap, children=("hashes", "nearest", "trace"), reps=20, warmup=3, rounds=5, steps="hashes,nearest,trace", out_dir="phash_bench_out",
                         out="--out")
    ap.add_argument("--contents", default="dense,natural,flat")
    ap.add_argument("--nearest-sizes", default="16384,65536")
    ap.add_argument("--chunk", type=int, default=512, help="queries per chunk of the torch route")
    ap.add_argument("--valu-per-pair", type=float, default=9.6, help="vector instructions per pair of the inner loop (profiles/phash_isa.txt)")
    args = ap.parse_args()
    if args.child:
        return {"hashes": child_hashes, "nearest": child_nearest, "trace": child_trace}[args.child](args)
    drive(args, {"hashes": ("hashes", None), "nearest": ("nearest", None), "trace": ("trace", trace_summary)}, [sys.executable, os.path.abspath(__file__)])


if __name__ == "__main__":
    main()
