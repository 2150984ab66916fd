#!/usr/bin/env python3
"""bench.py -- HVQM4 picture-reconstruction throughput on MI355X.

Metric (BASELINE.json): decoded Mpixels/s (bit-exact YUV) and % of the HBM roofline.

Workloads, weak scaling, one rank per GPU, no collective on the data path:
  c5 (default)  the per-GPU share of config C5: 128 concurrent 640x480 HVQM4 1.5 streams, GOP I P B B P B B ...
                (16 pictures), descriptors pre-parsed and resident in HBM.  One step = every stream decodes one GOP
                (128 * 16 = 2048 pictures) through the batched path (hvq_replay_stage, what = 1): EVERYTHING a batch of
                new pictures costs behind its parse -- the launches of the dependency levels on the launch queues, forked
                and joined per step exactly as a flush forks and joins them (round 6; rounds 1-5 let the queues run free
                over all timed steps, which is reported beside the headline as `free_running`).
  c4            config C4: 64 clips = 32 x 320x240 + 32 x 640x480, HVQM4 1.3 and 1.5 alternating, seeds 0..63,
                four 16-picture GOPs each, clip i -> rank i mod N.  One step = every clip of the rank decoded once.
`value` = luma pixels decoded by all ranks / max-over-ranks time.

`python bench.py --gpus N` without a launcher (no WORLD_SIZE in the environment) starts the N ranks itself, before
anything touches a GPU, and forwards rank 0's line; under torchrun it runs as one of the ranks.

A plain run does only what the headline needs: it generates the clips, parses them once into resident descriptors, warms up,
times `--steps` steps and prints the line (`roofline` is derived from the timed steps and the committed profiles).
`--dump-outputs DIR` then also writes what the last timed step left for its caller (rank 0's resident pictures) as float32 .npy
files.  `--full` adds everything else below: the oracle parity check, the free-running replay, the CPU baseline and the side legs.

Extra objects on the JSON line (`--full` only, except `roofline`):
  roofline      algorithmic bytes (1.5 B/px written + 1.5 B/px read for P/B) of a step / HIP-event
                time of the step on the launch stream (= bytes per launch / average launch duration: the step is its 7
                launches), vs 8 TB/s; `traffic` = HBM bytes per launch from the committed rocprofv3 PMC passes
                (profiles/*_pmc_traffic.json), calibrated as MI355X_MICROARCH.md prescribes
  cpu_baseline  the reference decoder (oracle/_ref, kind "reference") or this repo's scalar restatement (kind "port")
                on the host cores: one core on C1, C2, C3 and one process per clip over all cores on a C4 sample
Side legs (rank 0 at N=1; never `value`): end_to_end_gpu_parse (bitstreams in host memory -> pictures, streaming; h2d_GBs, h2d_probe_GBs and
pcie_bound_Mpixels say what PCIe allows at this stream density), end_to_end (host parse), sdk_path (the seven SDK calls, PCIe both ways),
c4_share (one GPU's share of config 4 against the reference's SHA-256), single_clip (configs 2 and 3: one clip alone), c5_staggered,
rgb_epilogue.  `--gpus N --dry-run` runs everything a multi-rank run does around the GPU work, on the CPU.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec
GOP16 = "IPBBPBBPBBPBBPBB"


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="c5", choices=["c5", "c4"])
    ap.add_argument("--streams", type=int, default=128, help="c5: concurrent streams per GPU")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--gop", default=GOP16)
    ap.add_argument("--distinct", type=int, default=8, help="c5: distinct synthetic clips per GPU (replicated over the streams)")
    ap.add_argument("--preset", default="dense", choices=["dense", "realistic", "flat", "natural"])
    ap.add_argument("--nslots", type=int, default=6)
    ap.add_argument("--no-gpu-parse", action="store_true", help="skip the GPU-entropy-parse end-to-end leg")
    ap.add_argument("--no-sdk", action="store_true", help="skip the SDK-boundary (PCIe-inclusive) leg")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="CPU baseline budget in seconds (rank 0, N=1 only; 0 = skip)")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--parse-threads", type=int, default=0, help="host parse threads for the end-to-end pass (0 = all cores, max 64)")
    ap.add_argument("--mv-bits", default="0,1,2", help="vector residual-bit choices of the synthetic P/B pictures (reach = 16 << bits samples)")
    ap.add_argument("--gen-workers", type=int, default=0, help="processes that generate the synthetic clips (0 = cores / ranks)")
    ap.add_argument("--clip-cache", default="", help="directory that keeps generated clips between runs (profiling passes of one workload)")
    ap.add_argument("--full", action="store_true",
                    help="also run the parity check against the CPU oracle, the free-running replay, the CPU baseline and the side legs")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write rank 0's resident pictures (what the last step computed) to DIR/*.npy as float32")
    ap.add_argument("--dry-run", action="store_true",
                    help="plumbing rehearsal, no GPU: start the ranks, rendezvous, bind cores (sysfs tree from HVQM4_AMD_SYSFS), deal the "
                         "clips / streams to the ranks, reduce -- and print what every rank would decode")
    return ap.parse_args(argv)


# ---------------------------------------------------------------------------------------------- rank launcher
def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_ranks(n: int, argv, child=None) -> int:
    """Parent of a self-started multi-rank run.  Imports neither torch nor the HIP library and makes no GPU call: it
    starts one child per GPU with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, waits, forwards rank 0's stdout (the
    JSON line) and returns non-zero when any child failed (the others are then terminated)."""
    import tempfile
    port = free_port()
    cmd = child or [sys.executable, os.path.abspath(__file__)]
    out0 = tempfile.TemporaryFile()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen(cmd + list(argv), env=env, stdout=out0 if r == 0 else sys.stderr))
    rc = 0
    try:
        while rc == 0 and any(p.poll() is None for p in procs):
            time.sleep(0.1)
            for r, p in enumerate(procs):
                if p.poll() not in (None, 0):
                    rc = p.returncode
                    print(f"bench.py: rank {r} exited with code {rc}", file=sys.stderr)
                    break
        for r, p in enumerate(procs):
            if rc == 0 and p.poll() not in (None, 0):
                rc = p.returncode
                print(f"bench.py: rank {r} exited with code {rc}", file=sys.stderr)
    finally:
        for p in procs:                               # a failed rank leaves the others at a barrier: end exactly those
            if p.poll() is None:
                p.terminate()
        for p in procs:
            try:
                p.wait(timeout=20)
            except subprocess.TimeoutExpired:
                p.kill()
    if rc == 0:
        out0.seek(0)
        sys.stdout.write(out0.read().decode(errors="replace"))
        sys.stdout.flush()
    return rc


# ---------------------------------------------------------------------------------------------- workloads
def c4_clip_config(i: int, preset: str = "dense", gops: int = 4, mv_bits=(0, 1, 2)):
    """Clip i of config C4 (seed i).  Sizes alternate per group of 8 and versions per clip and group of 16, so that every
    rank of an i mod N sharding (N = 1, 2, 4, 8) decodes the same mix of both sizes and both versions."""
    from hvqm4_amd.synth import SynthConfig
    small = (i // 8) % 2 == 0
    v13 = ((i // 16) + i) % 2 == 0
    return SynthConfig(width=320 if small else 640, height=240 if small else 480, version="1.3" if v13 else "1.5",
                       gop=GOP16, n_gops=1, repeat_gops=gops, seed=i, preset=preset, mv_res_bits=tuple(mv_bits))


def _make(cfg):
    from hvqm4_amd.synth import make_clip
    return make_clip(cfg)


def gen_clips(cfgs, workers: int, cache: str = ""):
    """synthetic clips, generated by a process pool (pure Python + numpy; no GPU or HIP call happens in the children);
    `cache`: directory of pickled clips keyed by their configuration"""
    import hashlib
    import pickle
    paths = [os.path.join(cache, hashlib.sha256(repr(c).encode()).hexdigest()[:24] + ".clip") if cache else None for c in cfgs]
    out = [pickle.load(open(p, "rb")) if p and os.path.exists(p) else None for p in paths]
    todo = [i for i, o in enumerate(out) if o is None]
    if todo:
        assert not (_GPU_OPEN and workers > 1 and len(todo) > 1), "no process pool once this process has opened the GPU"
        if workers <= 1 or len(todo) <= 1:
            made = [_make(cfgs[i]) for i in todo]
        else:
            import multiprocessing as mp
            with mp.get_context("spawn").Pool(min(workers, len(todo))) as pool:
                made = pool.map(_make, [cfgs[i] for i in todo], chunksize=1)
        for i, m in zip(todo, made):
            out[i] = m
            if paths[i]:
                os.makedirs(cache, exist_ok=True)
                pickle.dump(m, open(paths[i], "wb"))
    return out


_GPU_OPEN = False       # set by main() right before the first batch.Context: no process pool may start afterwards


def host_cores() -> int:
    return len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)


def usable_cores() -> int:
    """cores this process can actually keep busy: its affinity mask, capped by the cgroup's CPU quota (a 1-GPU box shows all of the host's
    logical CPUs but grants a share of them: 64 busy threads on a 16-core quota spend three quarters of every period throttled)"""
    q = cpu_quota()
    n = host_cores()
    if not q:
        return n
    ranks = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1"))))     # the quota is the whole job's: the ranks share it
    return max(1, min(n, int(q / ranks + 0.5)))


def cpu_quota():
    """CPU limit of this container's cgroup in cores (cgroup v2 cpu.max), None when unlimited or unknown"""
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else round(int(q) / int(p), 2)
    except Exception:
        return None


def pin_rank(local_rank: int, local_world: int):
    """One rank per GPU on a shared host (the scaling risk is host-side): every rank binds itself to cores of the NUMA
    node ITS GPU hangs off (hvqm4_amd/topology.py: KFD topology -> PCI address -> numa_node -> cpulist; ranks that share a node split
    its cores) -- its copy threads inherit the mask, and the pinned arenas, allocated after this call, are first touched from those
    cores, so the bitstreams a rank copies and its GPU's DMA reads stay on one socket.  Where sysfs does not tell (a container without
    /sys/class/kfd) the ranks take even linear slices of the allowed cores, as before round 5.  Reads sysfs only: no GPU call.
    Returns (copy threads, cores of the slice, numa node or None, "numa" | "linear")."""
    from hvqm4_amd import topology
    sysfs = os.environ.get("HVQM4_AMD_SYSFS", "/sys")                   # tests: a fake tree (tests/test_topology.py)
    cores = sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else list(range(os.cpu_count() or 1))
    shared = bool(os.environ.get("HVQM4_BENCH_SHARE_GPU"))             # rehearsal: every rank drives device 0
    devices = [0] * local_world if shared else None
    if shared:                                                        # ... so the node of device 0 is everybody's: split linearly
        mine, node, how = topology.rank_cores(local_rank, local_world, cores, sysfs=os.devnull)
        node = topology.gpu_numa_node(0, sysfs)
    else:
        mine, node, how = topology.rank_cores(local_rank, local_world, cores, sysfs=sysfs, devices=devices)
    if local_world > 1 and hasattr(os, "sched_setaffinity"):
        os.sched_setaffinity(0, mine)
    threads = int(os.environ.get("HVQM4_AMD_COPY_THREADS", "0")) or max(1, min(8, len(mine)))
    os.environ["HVQM4_AMD_COPY_THREADS"] = str(threads)
    return threads, mine, node, how


# ---------------------------------------------------------------------------------------------- one rank
def main():
    global _GPU_OPEN
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))

    from hvqm4_amd.distrib import Group, shard
    grp = Group()                       # torch.distributed (nccl = RCCL) only when WORLD_SIZE > 1
    rank, local_rank, world = grp.rank, grp.local_rank, grp.world
    if world != args.gpus:
        print(f"warning: WORLD_SIZE={world} but --gpus {args.gpus}; running {world} rank(s)", file=sys.stderr)

    if args.dry_run:
        return dry_run(args, grp)

    import numpy as np
    from hvqm4_amd import batch
    from hvqm4_amd._lib import HVQ_E_STATE, HvqError
    from hvqm4_amd.container import video_pictures
    from hvqm4_amd.synth import SynthConfig

    mv_bits = tuple(int(x) for x in args.mv_bits.split(","))
    full = args.full                    # everything beside the headline (module docstring)
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    copy_threads, my_cores, my_node, pin_how = pin_rank(local_rank % max(1, local_world), local_world)
    workers = args.gen_workers or usable_cores()                # after pin_rank: the cores of this rank's slice, capped by the cgroup quota

    # ---- synthetic inputs (fixed seeds) ----
    t0 = time.time()
    if args.workload == "c5":
        # clip i of rank r has seed 1000 + r*distinct + i; stream s replays clip s mod distinct
        cfgs = [SynthConfig(width=args.width, height=args.height, version="1.5", gop=args.gop,
                            seed=1000 + rank * args.distinct + i, preset=args.preset, mv_res_bits=mv_bits)
                for i in range(args.distinct)]
        stream_clip = [s % args.distinct for s in range(args.streams)]
        what = (f"C5 share: {args.streams} concurrent {args.width}x{args.height} HVQM4 1.5 streams per GPU, GOP {args.gop}, "
                f"{args.preset} synthetic streams, descriptors resident in HBM")
    else:
        mine = shard(64, rank, world)
        cfgs = [c4_clip_config(i, args.preset, 4, mv_bits) for i in mine]
        stream_clip = list(range(len(cfgs)))
        what = (f"C4: 64 clips (32 x 320x240 + 32 x 640x480, HVQM4 1.3/1.5 alternating, seeds 0..63, 4 x 16-picture GOPs), "
                f"clip i -> rank i mod {world}, {args.preset} synthetic streams, descriptors resident in HBM")
    clips = gen_clips(cfgs, workers, args.clip_cache)
    # every synthetic clip of the run is made HERE, before this process opens the GPU: a process pool started later would fork
    # (spawn) from a GPU-initialised parent -- under rocprofv3 every child gets the tool injected (round 4's evidence logs ended
    # in eight "Aborted" blocks from exactly that) -- and this pool is touchy about it
    c4_share_clips = single_clips = None
    if full and rank == 0 and world == 1 and not args.no_sdk:
        c4_share_clips = gen_clips(c4_share_configs(), workers, args.clip_cache)
        single_clips = gen_clips([SynthConfig(width=320, height=240, version="1.5", gop="I", n_gops=64, seed=2, preset=args.preset),
                                  SynthConfig(width=640, height=480, version="1.5", gop=GOP16, seed=1000, preset=args.preset)],
                                 workers, args.clip_cache)
    gen_s = time.time() - t0
    pics = [list(video_pictures(c.data)) for c in clips]

    # CPU baseline first: the host is otherwise idle, and its worker processes start before this process touches the GPU
    cpu_base = None
    if full and rank == 0 and world == 1 and args.cpu_seconds > 0:
        c3 = clips[0] if (args.workload == "c5" and (args.width, args.height, args.gop) == (640, 480, GOP16)) else None
        cpu_base = cpu_baseline(args.cpu_seconds, c3, args.preset)
    _GPU_OPEN = True                    # from here on gen_clips refuses to start a process pool

    # one rank per GPU; HVQM4_BENCH_SHARE_GPU=1 lets several ranks share device 0 (rehearsal on a 1-GPU box only)
    device = 0 if os.environ.get("HVQM4_BENCH_SHARE_GPU") else local_rank
    ctx = batch.Context(device)
    sids = [ctx.open_stream(clips[ci].width, clips[ci].height, 2, 2, clips[ci].version == "1.5", args.nslots)
            for ci in stream_clip]
    # decode-order interleave: picture k of every stream, then k+1 ... (the order a player would submit).
    # This first pass is also the END-TO-END measurement with the host parser: entropy parse (thread pool) +
    # descriptor upload + all launches, from bitstreams in host memory to pictures in HBM.
    threads = max(1, min(args.parse_threads or usable_cores(), 64))
    a_sid, a_ft, a_pic, a_stream = [], [], [], []
    for k in range(max(len(p) for p in pics)):
        for s, sid in enumerate(sids):
            seq = pics[stream_clip[s]]
            if k < len(seq):
                ft, _d, pic = seq[k]
                a_sid.append(sid); a_ft.append(ft); a_pic.append(pic); a_stream.append(s)
    ctx.sync()
    t0 = time.perf_counter()
    ctx.submit_many(a_sid, a_ft, a_pic, threads)
    t_parse = time.perf_counter() - t0
    ctx.flush()
    ctx.sync()
    t_e2e = time.perf_counter() - t0
    st = ctx.stats()
    # ... and once more in steady state (a context of its own, second pass: the pinned arenas and the workers' buffers are sized by then --
    # the first pass above pays for a few hundred MB of pinned allocation)
    e2e_steady = None
    if full and rank == 0 and world == 1 and not args.no_sdk:
        ctxh = batch.Context(device)
        sidh = [ctxh.open_stream(clips[ci].width, clips[ci].height, 2, 2, clips[ci].version == "1.5", args.nslots) for ci in stream_clip]
        a_sidh = [sidh[s] for s in a_stream]
        best = None
        for rep in range(3):
            ctxh.sync()
            th0 = time.perf_counter()
            ctxh.submit_many(a_sidh, a_ft, a_pic, threads)
            th1 = time.perf_counter()
            ctxh.flush(); ctxh.sync()
            th2 = time.perf_counter()
            if rep and (best is None or th2 - th0 < best[0]):
                best = (th2 - th0, th1 - th0)
        ctxh.close()
        e2e_steady = best

    # ---- parity check against the CPU oracle on what is still resident ----
    # every stream keeps its last min(nslots, pictures) pictures; the first `distinct` streams (c4: every 4th clip) are checked
    verified = expected = None
    if full and not args.no_verify:
        from oracle import bridge
        verified = expected = 0
        check = list(range(min(args.distinct, len(sids)))) if args.workload == "c5" else list(range(0, len(sids), 4))
        for s in check:
            clip, seq = clips[stream_clip[s]], pics[stream_clip[s]]
            want = bridge.oracle_decode(clip.data, len(seq))
            expected += min(args.nslots, len(seq))
            for k in range(len(seq)):
                try:
                    got = ctx.read_picture(sids[s], k)
                except HvqError as e:
                    if e.code != HVQ_E_STATE:
                        raise
                    continue        # slot already reused by a later picture
                if not np.array_equal(got, want[k]):
                    raise SystemExit(f"PARITY FAILURE: stream {s} picture {k} differs from the oracle")
                verified += 1
        if verified != expected:
            raise SystemExit(f"PARITY CHECK INCOMPLETE: {verified} pictures compared, {expected} expected to be resident")

    def barrier():
        ctx.sync()
        grp.barrier()

    # One step = what a batch of NEW pictures costs behind its parse: the reconstruction launches of all dependency levels, the
    # launch queues forked and joined around every step as hvq_flush_end does (hvq_replay_stage what = 1).
    # untimed pre-roll: the measurement that runs first otherwise reads ~3 % low (the same launches measured a second time come out
    # faster: clocks still ramping after the host-bound parity check), then the W warm-up steps the contract asks for
    PREROLL = int(os.environ.get("HVQM4_BENCH_PREROLL", "20"))
    ctx.replay_stage(PREROLL, 1)
    for _ in range(args.warmup):
        ctx.replay_stage(1, 1)
    barrier()
    t0 = time.perf_counter()
    gpu_ms = ctx.replay_stage(args.steps, 1)  # K steps, timed by HIP events on the launch stream
    barrier()
    wall = grp.max(time.perf_counter() - t0)
    if args.dump_outputs and rank == 0:
        dump_outputs(ctx, sids, [len(pics[ci]) for ci in stream_clip], args.dump_outputs)
    # beside the headline: the same launches with the launch queues running free over all steps (forked once, joined once: rounds
    # 1-5's timed region -- a queue that is ahead runs into the next step)
    recon_ms = ctx.replay(args.steps) if full else None
    st = ctx.stats()

    # ---- end to end with the entropy parse ON THE GPU, on EVERY rank at once: raw bitstreams in
    # host memory -> H2D -> parse kernel -> reconstruction launches; host copy threads, pinned arenas and PCIe of all
    # ranks contend as they would in production.  Second pass of a fresh context = steady state (buffers sized).
    gpu_e2e = None
    if full and not args.no_gpu_parse:
        ctx2 = batch.Context(device)
        sids2 = [ctx2.open_stream(clips[ci].width, clips[ci].height, 2, 2, clips[ci].version == "1.5", args.nslots)
                 for ci in stream_clip]
        a_sid2 = [sids2[s] for s in a_stream]
        a_raw = [bytes(p) for p in a_pic]
        t_pass, parse_ms = [], []
        t_split = []
        for _ in range(3):
            barrier(); ctx2.sync()
            t0 = time.perf_counter()
            ctx2.submit_many_device(a_sid2, a_ft, a_raw)
            t1 = time.perf_counter()
            ctx2.flush()
            t2 = time.perf_counter()
            ctx2.sync()
            t_pass.append(time.perf_counter() - t0)
            t_split = [round((t1 - t0) * 1e3, 2), round((t2 - t1) * 1e3, 2), round((time.perf_counter() - t2) * 1e3, 2)]
            parse_ms.append(ctx2.stats().gpu_parse_ms)
        # streaming: batch n+1 is submitted (copied into the second pinned arena, uploaded on the copy stream) while
        # batch n is parsed.  Steady-state period = time between the completions of consecutive hvq_flush_end calls,
        # after two warm-up batches (the second arena and its staging are allocated on first use).
        # 24 batches: on a shared host one batch in four or five waits 1-2 ms for its bitstreams (the host's copy of 160 MB into the
        # pinned arena), so a window of 8 says 4.7 or 5.2 ms by luck; the mean over the window is the number, the median beside it
        nwarm, nbatch = 2, int(os.environ.get("HVQM4_BENCH_STREAM_BATCHES", "24"))
        def stream_loop(submit, plain_pair=False):
            """steady-state period of submit next / hvq_flush_next (= flush_end of the batch in flight + flush_begin of the queued one,
            the queued batch's parse kernel launched first; plain_pair: the two calls in their plain order); returns (mean period,
            median period, mean ms of the calls [submit, end or next, begin], parse kernel ms of the last batch)"""
            barrier(); ctx2.sync()
            submit()
            ctx2.flush_begin()
            calls = [0.0, 0.0, 0.0]
            ends = []
            for k in range(nwarm + nbatch - 1):
                ta = time.perf_counter()
                submit()
                tb = time.perf_counter()
                if plain_pair:
                    ctx2.flush_end()
                    tc = time.perf_counter()
                    ctx2.flush_begin()
                else:
                    ctx2.flush_next()
                    tc = time.perf_counter()
                td = time.perf_counter()
                ends.append(tc)
                if k >= nwarm:
                    calls[0] += tb - ta; calls[1] += tc - tb; calls[2] += td - tc
            ctx2.flush_end()
            ends.append(time.perf_counter())
            ctx2.sync()
            pipe = (ends[-1] - ends[nwarm]) / (len(ends) - 1 - nwarm)
            periods = sorted(b - a for a, b in zip(ends[nwarm:], ends[nwarm + 1:]))
            return pipe, periods[len(periods) // 2], [round(x / (nbatch - 1) * 1e3, 2) for x in calls], ctx2.stats().gpu_parse_ms

        # (a) the caller's buffers are copied into the pinned arena by the library's worker threads (hvq_submit_many_device_async)
        st_c0 = ctx2.stats()
        t_pipe, t_pipe_median, t_calls, parse_ms_streaming = stream_loop(lambda: ctx2.submit_many_device(a_sid2, a_ft, a_raw, defer=True))
        st_c1 = ctx2.stats()
        copy_gbs = (st_c1.copy_bytes - st_c0.copy_bytes) / max(st_c1.copy_seconds - st_c0.copy_seconds, 1e-9) / 1e9
        # (b) zero copy: the bitstreams ARE in the pinned arena when the batch is submitted (hvq_arena_reserve: a reader's read()
        # target).  Both arenas are filled once during the warm-up batches; afterwards a batch costs the host its bookkeeping only.
        z_len = [len(p) for p in a_raw]
        z_off, z_at = [], 0
        for ln in z_len:
            z_off.append(z_at); z_at += ctx2.arena_stride(ln)
        z_fills = [0]

        def submit_zero():
            view = ctx2.arena_reserve(z_at)
            if z_fills[0] < 2:                          # first use of each of the two arenas
                for p, o in zip(a_raw, z_off):
                    view[o:o + len(p)] = np.frombuffer(p, np.uint8)
                z_fills[0] += 1
            ctx2.submit_many_arena(a_sid2, a_ft, z_off, z_len)
        z_pipe, z_median, z_calls, z_parse = stream_loop(submit_zero)
        # (c) the plain pair hvq_flush_end / hvq_flush_begin (rounds 2-4's loop): the GPU idles between a batch's parse kernel and its
        # first reconstruction launch while the host reads the results and builds the tables
        pp_pipe, pp_median, pp_calls, _pp = stream_loop(lambda: ctx2.submit_many_device(a_sid2, a_ft, a_raw, defer=True), plain_pair=True)
        # (d) the same 128 streams over TWO contexts of this process (even / odd streams), each fed by its own thread: their parse kernels
        # are half the size and out of phase -- one context's pictures sit in the scalar chains while the other's are in the all-thread
        # passes or being reconstructed -- which is what a single launch of 2048 pictures cannot arrange (profiles/r05_flush_next.txt)
        two_ctx = None
        nctx = int(os.environ.get("HVQM4_BENCH_STREAM_CONTEXTS", "2"))
        if len(sids) >= nctx >= 2:
            import threading
            halves = []
            for hh in range(nctx):
                cx = batch.Context(device)
                cx.set_launch_queues(1)                         # the contexts are each other's second launch queue
                sid_of = {s: cx.open_stream(clips[stream_clip[s]].width, clips[stream_clip[s]].height, 2, 2, clips[stream_clip[s]].version == "1.5", args.nslots)
                          for s in range(len(sids)) if s % nctx == hh}
                idx = [i for i, s in enumerate(a_stream) if s % nctx == hh]
                halves.append((cx, sid_of, [sid_of[a_stream[i]] for i in idx], [a_ft[i] for i in idx], [a_raw[i] for i in idx]))

            def half_loop(cx, _sid_of, hs, ht, hp, n, marks):
                cx.submit_many_device(hs, ht, hp, defer=True)
                cx.flush_begin()
                for _ in range(n):
                    cx.submit_many_device(hs, ht, hp, defer=True)
                    cx.flush_next()
                    marks.append(time.perf_counter())
                cx.flush_end()
                cx.sync()

            for hv in halves:                                   # buffers sized, both arenas and parse-buffer sets in use
                half_loop(*hv, 3, [])
            barrier()
            marks = [[] for _ in halves]
            th = [threading.Thread(target=half_loop, args=(*halves[i], nwarm + nbatch, marks[i])) for i in range(nctx)]
            for t in th: t.start()
            for t in th: t.join()
            n_batches_half = 4 + 1 + nwarm + nbatch               # batches each context has seen
            per = [(m[-1] - m[nwarm]) / (len(m) - 1 - nwarm) for m in marks]
            px_half = [sum(clips[stream_clip[s]].width * clips[stream_clip[s]].height * len(pics[stream_clip[s]]) for s in hv[1]) for hv in halves]
            rate2 = sum(p_ / t_ for p_, t_ in zip(px_half, per)) / 1e6
            ok2 = 0
            n_seq = [len(pics[stream_clip[s]]) for s in range(len(sids))]
            for hv in halves:                                    # the last batch of either context against the host-parsed pictures
                for s in sorted(hv[1])[:2]:
                    for k in range(n_seq[s]):
                        try:
                            a = ctx.read_picture(sids[s], k); b = hv[0].read_picture(hv[1][s], k + (n_batches_half - 1) * n_seq[s])
                        except HvqError as e:
                            if e.code != HVQ_E_STATE:
                                raise
                            continue
                        if not np.array_equal(a, b):
                            raise SystemExit(f"PARITY FAILURE: two-context streaming, stream {s} picture {k} differs from the host-parsed one")
                        ok2 += 1
            if ok2 < 1:
                raise SystemExit("PARITY CHECK INCOMPLETE on the two-context streaming leg")
            two_ctx = {"value": round(grp.sum(rate2), 1), "unit": "Mpixels/s", "contexts": nctx,
                       "ms_per_batch_of_each_context": [round(t_ * 1e3, 2) for t_ in per], "pictures_checked_against_host_parsed": ok2,
                       "what": "the same streams dealt to %d contexts of the process (stream s to context s mod %d, one thread each, hvq_flush_next): "
                               "smaller parse kernels out of phase with each other and with the other contexts' reconstruction" % (nctx, nctx)}
            for hv in halves:
                hv[0].close()
        n_done = 3 + 3 * (nwarm + nbatch)
        ok = 0
        ok_per_stream = []
        n_seq = [len(pics[stream_clip[s]]) for s in range(len(sids))]
        for s in range(min(4, len(sids))):
            ok_per_stream.append(0)
            for k in range(n_seq[s]):
                try:
                    a = ctx.read_picture(sids[s], k); b = ctx2.read_picture(sids2[s], k + (n_done - 1) * n_seq[s])
                except HvqError as e:
                    if e.code != HVQ_E_STATE:
                        raise
                    continue
                if not np.array_equal(a, b):
                    raise SystemExit(f"PARITY FAILURE: GPU-parsed stream {s} picture {k} differs from the host-parsed one")
                ok += 1; ok_per_stream[-1] += 1
        # which ordinals are still resident depends on the ring phase of either context (13 passes here, one there): every
        # picture resident in BOTH was compared; at least one of EVERY checked stream must have been
        if not ok_per_stream or min(ok_per_stream) < 1:
            raise SystemExit(f"PARITY CHECK INCOMPLETE on the GPU-parsed streams: pictures compared per stream {ok_per_stream}")
        px = int(st.luma_pixels)
        one = px / min(t_pass[1:]) / 1e6
        stream_v = px / t_pipe / 1e6
        # what PCIe allows: the batch's bitstreams cross it once per batch -- the rate the streaming loop moves them at, the rate a
        # plain pinned-host -> device copy of the same size reaches on this box, and the Mpixel/s that rate is worth at this stream density
        batch_bytes = int(sum(z_len))
        try:
            h2d_peak = ctx2.h2d_probe(batch_bytes, 8)
        except HvqError:
            h2d_peak = None
        # the same streaming loop with EVERY picture brought back to (pinned) host memory: hvq_read_pictures of batch k runs
        # beside the parse of batch k + 1 (one synchronisation per batch).  PCIe-bound; never `value`.
        rb = None
        try:
            n_seq0 = len(pics[stream_clip[0]])
            if all(len(pics[stream_clip[s]]) == n_seq0 for s in range(len(sids))) and len({clips[ci].picsize for ci in stream_clip}) == 1:
                ctx3 = batch.Context(device)
                sids3 = [ctx3.open_stream(clips[ci].width, clips[ci].height, 2, 2, clips[ci].version == "1.5", 2 * n_seq0 + 4)
                         for ci in stream_clip]
                a_sid3 = [sids3[s] for s in a_stream]
                host = ctx3.pinned_array((len(a_sid3), ctx3.pic_bytes(sids3[0])))
                k_of = []                                   # ordinal of entry i inside its stream's batch
                seen = {}
                for s in a_stream:
                    k_of.append(seen.get(s, 0)); seen[s] = k_of[-1] + 1
                nb3, nwarm3 = 6, 2
                barrier(); ctx3.sync()
                ctx3.submit_many_device(a_sid3, a_ft, a_raw, defer=True)
                ctx3.flush_begin()
                t_done = []
                for b in range(nb3 + nwarm3):
                    last = b == nb3 + nwarm3 - 1
                    if not last:
                        ctx3.submit_many_device(a_sid3, a_ft, a_raw, defer=True)
                    ctx3.flush_end()
                    if not last:
                        ctx3.flush_begin()
                    ctx3.read_pictures(a_sid3, [b * n_seq0 + k for k in k_of], out=host)
                    t_done.append(time.perf_counter())
                t_rb = (t_done[-1] - t_done[nwarm3 - 1]) / nb3
                # what came back is what the CPU oracle decodes: 17 entries spread over the batch (every kind of picture, several streams)
                chk = 0
                if not args.no_verify:
                    from oracle import bridge as _br
                    want_of = {}
                    for i in range(0, len(a_sid3), max(1, len(a_sid3) // 16)):
                        ci = stream_clip[a_stream[i]]
                        if ci not in want_of:
                            want_of[ci] = _br.oracle_decode(clips[ci].data, len(pics[ci]))
                        if not np.array_equal(host[i], want_of[ci][k_of[i]]):
                            raise SystemExit(f"PARITY FAILURE: bulk readback entry {i} (stream {a_stream[i]} picture {k_of[i]}) differs from the oracle")
                        chk += 1
                    if chk == 0:
                        raise SystemExit("PARITY CHECK INCOMPLETE: no bulk readback entry was compared")
                rb_v = px / t_rb / 1e6
                rb = {"value": round(grp.sum(rb_v), 1), "unit": "Mpixels/s", "ms_per_batch": round(t_rb * 1e3, 2),
                      "d2h_GBs": round(host.nbytes / t_rb / 1e9, 2), "pictures_checked": chk,
                      "what": "streaming as above with every picture copied to pinned host memory (hvq_read_pictures of batch k beside "
                              "the parse of batch k + 1); bounded by PCIe, 1.5 B per pixel"}
                ctx3.close()
        except (MemoryError, HvqError) as e:
            rb = {"error": str(e)}
        gpu_e2e = {"value": round(grp.sum(one), 1), "unit": "Mpixels/s",
                   "streaming_value": round(grp.sum(stream_v), 1),
                   "streaming_value_min_rank": round(-grp.max(-stream_v), 1),
                   "streaming_value_max_rank": round(grp.max(stream_v), 1),
                   "ranks": world,
                   "streaming_ms_per_batch": round(t_pipe * 1e3, 2), "streaming_ms_per_batch_median": round(t_pipe_median * 1e3, 2),
                   "streaming_batches": nbatch, "streaming_submit_end_begin_ms": t_calls,
                   "streaming_parse_kernel_ms": round(parse_ms_streaming, 3),
                   "parse_kernel_ms": round(min(parse_ms[1:]), 3), "pass_ms": [round(t * 1e3, 2) for t in t_pass],
                   "submit_flush_sync_ms": t_split,
                   "host_copy_threads": copy_threads,
                   "host_copy_GBs": round(copy_gbs, 2), "host_copy_GBs_all_ranks": round(grp.sum(copy_gbs), 2),
                   "host_copy_bytes_per_batch": int(sum(z_len)),
                   "h2d_GBs": round(batch_bytes / t_pipe / 1e9, 2),
                   "h2d_GBs_what": "bitstream bytes of a batch / streaming period: what the streaming loop moves over PCIe per GPU",
                   "h2d_probe_GBs": round(h2d_peak, 2) if h2d_peak else None,
                   "pcie_bound_Mpixels": round(px / (batch_bytes / (h2d_peak * 1e9)) / 1e6, 1) if h2d_peak else None,
                   "pcie_bound_what": "pixels of a batch / (its bitstream bytes / h2d_probe_GBs): the streaming rate at which the upload alone "
                                      "fills the period at this stream density (%.1f bitstream bytes per kilopixel), whatever the kernels do"
                                      % (batch_bytes / (px / 1e3)),
                   "streaming_zero_copy": {"value": round(grp.sum(px / z_pipe / 1e6), 1), "unit": "Mpixels/s",
                                           "ms_per_batch": round(z_pipe * 1e3, 2), "ms_per_batch_median": round(z_median * 1e3, 2),
                                           "submit_end_begin_ms": z_calls, "parse_kernel_ms": round(z_parse, 3),
                                           "what": "the same streaming loop with the bitstreams already in the library's pinned arena "
                                                   "(hvq_arena_reserve / hvq_submit_many_arena: what a container reader that read()s into the "
                                                   "reservation leaves): no host memcpy, the batch costs the host its bookkeeping and the DMA"},
                   "streaming_plain_pair": {"value": round(grp.sum(px / pp_pipe / 1e6), 1), "unit": "Mpixels/s",
                                            "ms_per_batch": round(pp_pipe * 1e3, 2), "ms_per_batch_median": round(pp_median * 1e3, 2),
                                            "submit_end_begin_ms": pp_calls,
                                            "what": "the same loop with hvq_flush_end + hvq_flush_begin in place of hvq_flush_next (the loop of "
                                                    "rounds 2-4): the host's part of a batch is not hidden behind the next batch's parse kernel"},
                   "streaming_two_contexts": two_ctx,
                   "affinity": {"cores_of_rank0": len(my_cores), "first": my_cores[0], "last": my_cores[-1], "ranks_on_host": local_world,
                                "pinned": local_world > 1, "numa_node_of_gpu": my_node, "core_choice": pin_how},
                   "pictures_checked_against_host_parsed": ok,
                   "streaming_with_readback": rb,
                   "what": "raw bitstreams in host memory -> H2D -> entropy parse kernel (one workgroup per picture) -> "
                           "reconstruction launches -> pictures in HBM; no host entropy parse; all ranks at once (sum over ranks, "
                           "per-rank min and max of the streaming rate; the per-rank detail fields are rank 0's).  value: one "
                           "batch start to finish; streaming_value: steady-state period of submit next / hvq_flush_next "
                           "(next batch copied and uploaded while this one is parsed; its parse kernel queued before the host takes this "
                           "batch's results; everything on the one launch stream, the reconstruction's two launch queues forked from it), mean over `streaming_batches` "
                           "batches after 2 warm-up batches"}
        ctx2.close()

    px_step = int(st.luma_pixels)
    total_px = grp.sum(float(px_step))
    value = total_px * args.steps / wall / 1e6
    launches = int(st.launches)
    queues = max(1, int(st.launch_queues))          # launch queues whose launches run side by side (2 for a batch of 16 streams or more)
    # average duration of ONE launch, derived: a queue runs its launches back to back, so a step lasts as long as a queue's
    # launches / queues launches; the queues run side by side, hence `queues x`.  `avg_launch_us_measured` beside it is rocprofv3's
    # per-kernel average from the committed kernel trace of this same command (profiles/*_kernel_stats.csv).
    stage_s = gpu_ms * 1e-3 / args.steps
    avg_launch_s = stage_s / (launches / queues)
    achieved = st.algorithmic_bytes / stage_s / 1e9
    traffic = pmc_traffic(args)
    trace = kernel_trace_avg(args)

    out = {
        "metric": "decoded Mpixels/s (bit-exact YUV)",
        "value": round(value, 1),
        "unit": "Mpixels/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(wall * 1e3 / args.steps, 4),
        "higher_is_better": True,
        "scaling": "weak" if args.workload == "c5" else "strong",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic",
        "config": {
            "workload": what,
            "step": ("reconstruction launches of all dependency levels, the launch queues forked and joined per step as in a flush; the "
                     "workgroups derive block records, item queues and pair lists from the parser's descriptors themselves "
                     "(hvq_recon_inline_kernel): no per-picture pass outside the step"),
            "streams_per_gpu": len(sids), "pictures_per_step": int(st.pictures),
            "distinct_clips_per_gpu": len(clips), "launches_per_step": launches,
            "reconstruction_launches_per_step": launches, "launch_queues": queues,
            "workgroups_per_step": int(st.workgroups), "nslots": args.nslots,
            "sharding": "one clip per stream, streams split across GPUs, no collective",
            "clip_generation_s": round(gen_s, 1), "untimed_preroll_steps": PREROLL,
        },
        "roofline": {
            "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4),
            "what": ("algorithmic bytes of one step / HIP-event time of one step (everything a new batch costs behind its parse), the launch "
                     "queues forked and joined around EVERY step exactly as hvq_flush_end does (stage_us_per_step_joined)"),
            "stage_us_per_step": round(stage_s * 1e6, 2),
            "stage_us_per_step_joined": round(stage_s * 1e6, 2),
            "algorithmic_bytes_per_step": int(st.algorithmic_bytes),
            "traffic": traffic["hbm_bytes_per_launch"] if traffic else None,
            "traffic_over_algorithmic": traffic["over_algorithmic"] if traffic else None,
            "traffic_source": traffic["source"] if traffic else None,
            "traffic_what": "HBM bytes per launch of the dominant kernel (hvq_recon_inline_kernel), PMC passes",
            "valu": pmc_valu(args),
            "kernel": "hvq_recon_inline_kernel", "algorithmic_bytes_per_launch": int(st.algorithmic_bytes // launches),
            "avg_launch_us": round(avg_launch_s * 1e6, 2),
            "avg_launch_us_what": "derived: joined step time / (launches / queues) -- a queue's launches run back to back",
            "avg_launch_us_measured": trace["avg_us"] if trace else None,
            "avg_launch_us_measured_source": trace["source"] if trace else None,
            "launch_queues": queues,
            "launch_queues_what": ("a batch's streams are dealt -- by work -- to two chains of launches on two HIP streams "
                                   "(a hardware queue each); a step = launches / queues launches per queue, back to back, the queues side by "
                                   "side: achieved = queues x algorithmic_bytes_per_launch / avg_launch_us = algorithmic bytes of a step / its time"
                                   if queues > 1 else "one launch queue"),
            "descriptor_bytes_per_launch": int(st.descriptor_bytes // launches),
            "descriptor_bytes_what": "blobs (maps, vectors, payload pools, nests) per reconstruction launch; not credited",
        },
        "gpu_event_ms_per_step": round(gpu_ms / args.steps, 4),
        "full": full,
        "end_to_end_gpu_parse": gpu_e2e,
        "end_to_end": {"value": round(px_step / t_e2e / 1e6, 1), "unit": "Mpixels/s", "parse_threads": threads,
                       "parse_only_mpix_s": round(px_step / t_parse / 1e6, 1),
                       "steady_value": round(px_step / e2e_steady[0] / 1e6, 1) if e2e_steady else None,
                       "steady_parse_only_mpix_s": round(px_step / e2e_steady[1] / 1e6, 1) if e2e_steady else None,
                       "what": "rank 0: host entropy parse (pictures side by side on `parse_threads` threads) + descriptor H2D + kernels, bitstreams in "
                               "host memory -> pictures in HBM.  value: the first pass of a fresh context (pays for the pinned arenas); "
                               "steady_value: best of the second and third pass of a context of its own"},
        "verified_pictures": verified, "verified_pictures_expected": expected,
        "flags_or": int(st.flags_or),
    }
    if recon_ms is not None:
        free_s = recon_ms * 1e-3 / args.steps
        free_achieved = st.algorithmic_bytes / free_s / 1e9
        out["roofline"]["free_running"] = {
            "achieved": round(free_achieved, 1), "frac": round(free_achieved / HBM_PEAK_GBS, 4), "us_per_step": round(free_s * 1e6, 2),
            "what": "the same launches with the launch queues forked once and joined once around all timed steps (hvq_replay; "
                    "the timed region of rounds 1-5): a queue that is ahead runs into the next step.  Never the headline"}
        out["gpu_event_ms_per_step_free_running"] = round(recon_ms / args.steps, 4)

    # display epilogue: YUV420 -> RGB24 of the newest picture of every stream, one launch
    if full:
        try:
            ctx.rgb_bench(2)
            rms, rbytes, rpics = ctx.rgb_bench(50)
            out["rgb_epilogue"] = {"kernel": "hvq_yuv420_rgb_kernel", "pictures_per_launch": rpics,
                                   "bytes_per_launch": rbytes, "avg_launch_us": round(rms * 1e3 / 50, 2),
                                   "achieved_GBs": round(rbytes * 50 / (rms * 1e-3) / 1e9, 1),
                                   "frac_of_8TBs": round(rbytes * 50 / (rms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        except Exception as e:      # never let the optional epilogue measurement break the headline number
            out["rgb_epilogue"] = {"error": str(e)}

    # the SDK boundary itself (PCIe-inclusive, never `value`): one stream, one synchronous call per picture -- upload
    # of the caller's reference pictures, host parse, launch, download of the decoded picture
    if full and rank == 0 and world == 1 and not args.no_sdk:
        out["sdk_path"] = sdk_leg(clips[0], pics[0])

    if cpu_base is not None:
        out["cpu_baseline"] = cpu_base
    ctx.close()
    # the same 2048 pictures per step with the GOP phase of the streams STAGGERED (stream s is s mod 16 pictures into its GOP when
    # the batch starts): every launch then holds I, P and B pictures in the stream's own proportion instead of one kind per
    # dependency level.  An extra line; the headline stays lock-step (every stream at the same picture, as a batch of players is).
    if full and rank == 0 and world == 1 and not args.no_sdk and args.workload == "c5" and all(len(p) == 16 for p in pics):
        try:
            from oracle import bridge as _bridge
            ctxs = batch.Context(device)
            sidss = [ctxs.open_stream(clips[ci].width, clips[ci].height, 2, 2, clips[ci].version == "1.5", args.nslots) for ci in stream_clip]
            phase = [s % 16 for s in range(len(sidss))]
            w_sid, w_ft, w_pic = [], [], []
            for k in range(16):                                          # warm-up: every stream up to its phase
                for s, sid in enumerate(sidss):
                    if k < phase[s]:
                        ft, _d, pic = pics[stream_clip[s]][k]
                        w_sid.append(sid); w_ft.append(ft); w_pic.append(pic)
            ctxs.submit_many(w_sid, w_ft, w_pic, threads); ctxs.flush(); ctxs.sync()
            b_sid, b_ft, b_pic = [], [], []
            for j in range(16):                                          # the batch: 16 pictures of every stream from its phase on (the GOP repeats)
                for s, sid in enumerate(sidss):
                    ft, _d, pic = pics[stream_clip[s]][(phase[s] + j) % 16]
                    b_sid.append(sid); b_ft.append(ft); b_pic.append(pic)
            ctxs.submit_many(b_sid, b_ft, b_pic, threads); ctxs.flush(); ctxs.sync()
            sts = ctxs.stats()
            chk = 0
            for s in (1, 5, 11):                                         # first pass checked against the oracle (ordinal o = GOP position o mod 16)
                if s >= len(sidss):
                    continue
                want = _bridge.oracle_decode(clips[stream_clip[s]].data, 16)
                for o in range(phase[s] + 16):
                    try:
                        got = ctxs.read_picture(sidss[s], o)
                    except HvqError as e:
                        if e.code != HVQ_E_STATE:
                            raise
                        continue
                    if not np.array_equal(got, want[o % 16]):
                        raise SystemExit(f"PARITY FAILURE (staggered): stream {s} ordinal {o} differs from the oracle")
                    chk += 1
            if chk == 0:
                raise SystemExit("PARITY CHECK INCOMPLETE (staggered): no picture was compared")
            # replays repeat the launches over whatever the slots hold by then (the references of the first pictures have been
            # overwritten by the batch's last ones): the same descriptors, addresses and work -- timing only
            ctxs.replay_stage(args.warmup or 1, 1)
            mss_stage = ctxs.replay_stage(args.steps, 1)
            mss = ctxs.replay(args.steps)
            ctxs.close()
            out["c5_staggered"] = {"value": round(int(sts.luma_pixels) * args.steps / (mss_stage * 1e-3) / 1e6, 1), "unit": "Mpixels/s",
                                   "frac_of_roofline": round(sts.algorithmic_bytes * args.steps / (mss_stage * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                   "recon_only_value": round(int(sts.luma_pixels) * args.steps / (mss * 1e-3) / 1e6, 1),
                                   "recon_only_frac": round(sts.algorithmic_bytes * args.steps / (mss * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                   "launches_per_step": int(sts.launches), "pictures_per_step": int(sts.pictures), "pictures_checked": chk,
                                   "what": "stream s starts its batch s mod 16 pictures into its GOP: mixed picture kinds in every launch"}
        except Exception as e:
            out["c5_staggered"] = {"error": str(e)}

    # BASELINE config 4 at the shape one GPU of eight sees it: clips 0, 8, ..., 56 of the 64 (4 x 320x240 + 4 x 640x480, HVQM4 1.3
    # and 1.5 alternating), every picture checked against the SHA-256 the REFERENCE decoder produced (tests/golden/manifest.json)
    if full and rank == 0 and world == 1 and not args.no_sdk:
        out["c4_share"] = c4_share_leg(device, args.steps, args.warmup or 1, threads, c4_share_clips)
        # BASELINE configs 2 and 3: ONE clip on one GPU (latency-bound by construction: a 16-picture GOP is seven dependent launches)
        out["single_clip"] = {"C2": single_clip_leg(device, single_clips[0], args.steps, args.warmup or 1, not args.no_verify),
                              "C3": single_clip_leg(device, single_clips[1], args.steps, args.warmup or 1, not args.no_verify)}

    if rank == 0:
        grp.emit(json.dumps(out))
    grp.close()


DUMP_BYTES = 64 << 20           # --dump-outputs: at most this much in all
DUMP_SEED = 20240611


def dump_outputs(ctx, sids, n_pics, out_dir):
    """--dump-outputs: what the last timed step left in the streams' slots, i.e. what a caller reads back (Y|U|V, uint8), as float32:
      picture_sNNN.npy    the newest picture of each of the first (up to 8) streams, whole
      resident_sample.npy one row per resident picture of every stream (stream-major, ordinals ascending), the same seeded positions
                          (fractions of the picture size) in every row
    The inputs are seeded, so two builds run with the same arguments can be compared file for file."""
    import numpy as np
    from hvqm4_amd._lib import HVQ_E_STATE, HvqError
    os.makedirs(out_dir, exist_ok=True)
    used = 0
    for s in range(min(8, len(sids))):
        pic = ctx.read_picture(sids[s], n_pics[s] - 1).astype(np.float32)
        if used + pic.nbytes > DUMP_BYTES // 2:
            break
        np.save(os.path.join(out_dir, f"picture_s{s:03d}.npy"), pic)
        used += pic.nbytes
    # positions per row sized for every ordinal (the resident ones are fewer), so that the sample fits whatever the ring keeps
    k = max(1, min(8192, (DUMP_BYTES - used) // (4 * max(1, sum(n_pics)))))
    frac = np.sort(np.random.default_rng(DUMP_SEED).random(k))
    rows = []
    for s, sid in enumerate(sids):
        for o in range(n_pics[s]):
            try:
                p = ctx.read_picture(sid, o)
            except HvqError as e:
                if e.code != HVQ_E_STATE:
                    raise
                continue                    # slot reused by a later picture
            rows.append(p[(frac * p.size).astype(np.int64)])
    np.save(os.path.join(out_dir, "resident_sample.npy"), np.stack(rows).astype(np.float32))


def dry_run(args, grp):
    """`bench.py --gpus N --dry-run`: everything a multi-GPU run does around the GPU work and nothing of the GPU work -- the ranks
    are started (launch_ranks or torchrun), meet (gloo), bind themselves to the cores of their GPU's NUMA node (pin_rank; sysfs tree
    from HVQM4_AMD_SYSFS), deal the workload (c4: clip i -> rank i mod N; c5: `--streams` streams per rank, their clips' seeds), pass the
    barriers of the timed region and reduce.  No clip is generated, neither the HIP library nor a GPU is touched.  Rank 0 prints one
    JSON line with every rank's share, so that the first real 8-GPU run cannot die in plumbing (tests/test_bench_launcher.py)."""
    from hvqm4_amd.distrib import shard
    rank, world = grp.rank, grp.world
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    copy_threads, my_cores, my_node, pin_how = pin_rank(grp.local_rank % max(1, local_world), local_world)
    if args.workload == "c4":
        ids = shard(64, rank, world)
        cfgs = [c4_clip_config(i, args.preset, 4) for i in ids]
        units = [{"clip": i, "w": c.width, "h": c.height, "version": c.version, "seed": c.seed} for i, c in zip(ids, cfgs)]
        pictures = sum(16 * c.repeat_gops for c in cfgs)
        pixels = sum(16 * c.repeat_gops * c.width * c.height for c in cfgs)
    else:
        seeds = [1000 + rank * args.distinct + i for i in range(args.distinct)]
        units = {"streams": args.streams, "first_global_stream": rank * args.streams, "clip_seeds": seeds, "w": args.width, "h": args.height}
        pictures = args.streams * len(args.gop)
        pixels = pictures * args.width * args.height
    mine = {"rank": rank, "local_rank": grp.local_rank, "device": 0 if os.environ.get("HVQM4_BENCH_SHARE_GPU") else grp.local_rank,
            "cores": my_cores, "numa_node": my_node, "core_choice": pin_how, "copy_threads": copy_threads,
            "units": units, "pictures_per_step": pictures, "pixels_per_step": pixels}
    grp.barrier()
    t0 = time.perf_counter()
    grp.barrier()
    wall = grp.max(time.perf_counter() - t0)
    total_px = grp.sum(float(pixels))
    total_pics = grp.sum(float(pictures))
    if grp.dist is not None:
        everyone = [None] * world
        grp.dist.all_gather_object(everyone, mine)
    else:
        everyone = [mine]
    if rank == 0:
        grp.emit(json.dumps({"dry_run": True, "workload": args.workload, "n_gpus": world, "scaling": "weak" if args.workload == "c5" else "strong",
                             "pictures_per_step": int(total_pics), "pixels_per_step": int(total_px), "barrier_s": round(wall, 4),
                             "ranks": everyone}))
    grp.close()


C4_SHARE_IDS = list(range(0, 64, 8))


def c4_share_configs():
    """the golden clips' configuration (tests/clips.py _c4) of the eight clips one GPU of eight gets"""
    from hvqm4_amd.synth import SynthConfig
    cfgs = []
    for i in C4_SHARE_IDS:
        small, v13 = (i // 8) % 2 == 0, ((i // 16) + i) % 2 == 0
        cfgs.append(SynthConfig(width=320 if small else 640, height=240 if small else 480, version="1.3" if v13 else "1.5", gop=GOP16, seed=i))
    return cfgs


def c4_share_leg(device, steps, warmup, threads, cl):
    try:
        import hashlib
        import numpy as np
        from hvqm4_amd import batch
        from hvqm4_amd.container import video_pictures
        manifest = json.load(open(os.path.join(ROOT, "tests", "golden", "manifest.json")))["clips"]
        ids = C4_SHARE_IDS
        for i, c in zip(ids, cl):
            if hashlib.sha256(c.data).hexdigest() != manifest[f"c4_clip{i:02d}"]["clip_sha256"]:
                return {"error": f"clip {i} differs from the golden clip (generator drift)"}
        ctx = batch.Context(device)
        seqs = [[(ft, bytes(p)) for ft, _d, p in video_pictures(c.data)] for c in cl]
        sids = [ctx.open_stream(c.width, c.height, 2, 2, c.version == "1.5", 16 + 3) for c in cl]
        s_, f_, d_ = [], [], []
        for k in range(16):
            for j, sid in enumerate(sids):
                s_.append(sid); f_.append(seqs[j][k][0]); d_.append(seqs[j][k][1])
        ctx.submit_many(s_, f_, d_, min(threads, 8))
        ctx.flush(); ctx.sync()
        st = ctx.stats()
        checked = 0
        for j, (i, sid) in enumerate(zip(ids, sids)):
            want = manifest[f"c4_clip{i:02d}"]["picture_sha256"]
            for k in range(16):
                if hashlib.sha256(ctx.read_picture(sid, k).tobytes()).hexdigest() != want[k]:
                    raise SystemExit(f"PARITY FAILURE (c4 share): clip {i} picture {k} differs from the reference decoder's SHA-256")
                checked += 1
        ctx.replay_stage(warmup, 1)
        ms = ctx.replay_stage(steps, 1)
        ctx.close()
        return {"value": round(int(st.luma_pixels) * steps / (ms * 1e-3) / 1e6, 1), "unit": "Mpixels/s",
                "frac_of_roofline": round(st.algorithmic_bytes * steps / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "us_per_step": round(ms * 1e3 / steps, 2), "pictures_per_step": int(st.pictures), "launches_per_step": int(st.launches),
                "pictures_checked_against_reference_sha256": checked,
                "what": "per-GPU share of BASELINE config 4 at 8 GPUs: clips 0, 8, ..., 56 (4 x 320x240 + 4 x 640x480, HVQM4 1.3 / 1.5), "
                        f"one 16-picture GOP each per step, descriptors resident; 128 pictures in {int(st.launches)} launches"}
    except Exception as e:
        return {"error": str(e)}


def single_clip_leg(device, clip, steps, warmup, verify):
    """ONE clip through the batched API on one GPU (BASELINE configs 2 and 3): the reconstruction stage over resident descriptors
    (roofline fraction), and bitstreams in host memory -> pictures in HBM with the host parser and with the GPU parser; every picture
    against the CPU oracle."""
    try:
        import numpy as np
        from hvqm4_amd import batch
        from hvqm4_amd.container import video_pictures
        seq = [(ft, bytes(p)) for ft, _d, p in video_pictures(clip.data)]
        n = len(seq)
        px = clip.width * clip.height * n
        ctx = batch.Context(device)
        res = {}
        for name in ("host_parse", "gpu_parse"):
            best = None
            for rep in range(3):                                   # first pass sizes the buffers
                sid = ctx.open_stream(clip.width, clip.height, 2, 2, clip.version == "1.5", n + 3)
                ctx.sync()
                t0 = time.perf_counter()
                if name == "host_parse":
                    ctx.set_parse_threads(sid, 4)                  # a lone stream: the sections of a picture side by side
                    for ft, p in seq:                              # ... its pictures one after the other
                        ctx.submit(sid, ft, p)
                else:
                    ctx.submit_many_device([sid] * n, [ft for ft, _p in seq], [p for _ft, p in seq])
                ctx.flush(); ctx.sync()
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
                if rep < 2:
                    ctx.close_stream(sid)
            res[name] = (best, sid)
        sid = res["gpu_parse"][1]
        checked = 0
        if verify:
            from oracle import bridge
            want = bridge.oracle_decode(clip.data, n)
            for k in range(n):
                if not np.array_equal(ctx.read_picture(sid, k), want[k]):
                    raise SystemExit(f"PARITY FAILURE (single clip {clip.width}x{clip.height}): picture {k} differs from the oracle")
                checked += 1
        st = ctx.stats()
        ctx.replay_stage(warmup, 1)
        ms = ctx.replay_stage(steps, 1)
        ctx.close()
        return {"value": round(px * steps / (ms * 1e-3) / 1e6, 1), "unit": "Mpixels/s",
                "frac_of_roofline": round(st.algorithmic_bytes * steps / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "us_per_step": round(ms * 1e3 / steps, 2), "pictures_per_step": int(st.pictures), "launches_per_step": int(st.launches),
                "end_to_end_host_parse": round(px / res["host_parse"][0] / 1e6, 1), "end_to_end_gpu_parse": round(px / res["gpu_parse"][0] / 1e6, 1),
                "pictures_checked": checked,
                "what": f"one {clip.width}x{clip.height} HVQM4 {clip.version} clip, {n} pictures ({''.join(sorted(set('IPB'[(ft >> 4) - 1] for ft, _p in seq)))}), one flush: "
                        "value = reconstruction stage over resident descriptors; end_to_end_* = bitstreams in host memory -> pictures in HBM "
                        "(submit + flush + sync, best of 3; host parse: hvq_stream_submit per picture, four threads sharing a picture's sections)"}
    except Exception as e:
        return {"error": str(e)}


def sdk_leg(clip, seq):
    try:
        from hvqm4_amd import sdk
        res = {}
        for name, env in (("default", None), ("trusted_pictures", "1")):
            if env is None:
                os.environ.pop("HVQM4_AMD_TRUST_PICTURES", None)
            else:
                os.environ["HVQM4_AMD_TRUST_PICTURES"] = env
            pl = sdk.Player(clip.width, clip.height, 2, 2, clip.version == "1.5")
            for ft, _d, pic in seq:                                  # warm-up pass
                pl.decode(ft, bytes(pic))
            t0 = time.perf_counter()
            reps = 3
            for _ in range(reps):
                for ft, _d, pic in seq:
                    pl.decode(ft, bytes(pic))
            dt = (time.perf_counter() - t0) / (reps * len(seq))
            pl.close()
            res[name] = {"value": round(clip.width * clip.height / dt / 1e6, 1), "ms_per_picture": round(dt * 1e3, 3)}
        os.environ.pop("HVQM4_AMD_TRUST_PICTURES", None)
        return {"value": res["default"]["value"], "unit": "Mpixels/s", "ms_per_picture": res["default"]["ms_per_picture"],
                "trusted_pictures": res["trusted_pictures"],
                "what": "HVQM4DecodeIpic/Ppic/Bpic through the C ABI with host picture buffers, one synchronous picture at a "
                        "time (PCIe both ways inside the call); trusted_pictures: HVQM4_AMD_TRUST_PICTURES=1 skips the upload "
                        "of `past`/`future` when they are the buffers this library last wrote for the same SeqObj"}
    except Exception as e:
        return {"error": str(e)}


def pmc_traffic(args):
    """HBM bytes per launch of the reconstruction kernel (hvq_recon_inline_kernel; the PMC scripts match `hvq_recon`) from the committed rocprofv3 --pmc passes of this same default workload
    (tools/pmc_passes.sh -> tools/pmc_traffic.py -> profiles/*_pmc_traffic.json, read side calibrated by
    tools/ubench/pmc_calib.hip as MI355X_MICROARCH.md prescribes); None for any other workload.  PMC counters cannot be
    collected from inside the timed process, so this is evidence from a separate run of the same command."""
    default = (args.workload, args.streams, args.width, args.height, args.gop, args.preset, args.distinct, args.mv_bits) == \
              ("c5", 128, 640, 480, GOP16, "dense", 8, "0,1,2")
    if not default:
        return None
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_traffic.json")))
    if not files:
        return None
    j = json.load(open(files[-1]))
    hbm = j.get("hbm_bytes_per_launch_calibrated", j.get("hbm_bytes_per_launch"))
    return {"hbm_bytes_per_launch": int(hbm), "over_algorithmic": j.get("over_algorithmic"),
            "source": "profiles/" + os.path.basename(files[-1]) + (" (calibrated)" if "hbm_bytes_per_launch_calibrated" in j else " (raw counters)")}


def kernel_trace_avg(args):
    """rocprofv3's average duration of hvq_recon_inline_kernel over the committed kernel trace of this default workload
    (profiles/r*_kernel_stats.csv, newest round); None for any other workload"""
    if pmc_traffic(args) is None:
        return None
    import csv
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_kernel_stats.csv")))
    for f in reversed(files):
        try:
            tot_ns = calls = 0
            for row in csv.DictReader(open(f)):
                if "hvq_recon_inline_kernel" in row.get("Name", ""):
                    tot_ns += float(row["TotalDurationNs"]); calls += int(row["Calls"])
            if calls:
                return {"avg_us": round(tot_ns / calls / 1e3, 2), "source": "profiles/" + os.path.basename(f) + f" ({calls} launches)"}
        except Exception:
            continue
    return None


def pmc_valu(args):
    """vector-instruction bound of the reconstruction kernel (hvq_recon_inline_kernel) beside the HBM fraction (which stays the contract number): instructions per
    wave and VALU busy fraction from the committed PMC passes of this default workload (tools/pmc_valu.py); None otherwise"""
    if pmc_traffic(args) is None:
        return None
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_valu.json")))
    if not files:
        return None
    j = json.load(open(files[-1]))
    return {"insts_per_wave": j["insts_per_wave"], "busy_frac": j["busy_frac"], "note": j.get("note"),
            "source": "profiles/" + os.path.basename(files[-1])}


def _time_clip_worker(job):
    data, reps = job
    from oracle import bridge
    timer = bridge.ref_time if bridge.have_ref() else bridge.oracle_time
    return timer(data, reps)


def cpu_baseline(budget_s: float, c3_clip, preset: str):
    """The reference decoder on the host cores (decode calls only): one core on C1 (one 320x240 1.3 I picture),
    C2 (320x240 1.5, I pictures only) and C3 (640x480 1.5, I P B B ...), plus one process per clip over all cores on a
    sample of the C4 clip set.  `value` is the C3 figure (the configuration `metric` is quoted on)."""
    from hvqm4_amd.synth import SynthConfig, make_clip
    from oracle import bridge
    have_ref = bridge.have_ref()
    kind, timer = ("reference", bridge.ref_time) if have_ref else ("port", bridge.oracle_time)
    per = max(0.5, budget_s / 5.0)

    def one_core(clip):
        t, px = timer(clip.data, 1)
        reps = max(1, int(per / max(t, 1e-6)))
        t, px = timer(clip.data, reps)
        return {"value": round(px / t / 1e6, 1), "unit": "Mpixels/s", "cores": 1,
                "sample": f"{reps} passes over one {clip.width}x{clip.height} HVQM4 {clip.version} clip of {len(clip.kinds)} "
                          f"picture(s) (decode calls only, {t:.1f} s)"}

    c1 = make_clip(SynthConfig(width=320, height=240, version="1.3", gop="I", seed=1, preset=preset))
    c2 = make_clip(SynthConfig(width=320, height=240, version="1.5", gop="I", n_gops=16, seed=2, preset=preset))
    c3 = c3_clip or make_clip(SynthConfig(width=640, height=480, version="1.5", gop=GOP16, seed=1000, preset=preset))
    res = {"C1": one_core(c1), "C2": one_core(c2), "C3": one_core(c3)}
    # all cores (SURVEY.md 8d ii): ALL 64 clips of C4 (32 x 320x240 + 32 x 640x480, both versions), one GOP each, one process
    # per clip over min(nproc, 64) processes.  nproc = cores this process may run on; the container's CPU quota (cgroup cpu.max)
    # is reported beside it -- the box gives a 1-GPU job a share of the host, so "all cores" is that share, not the host's 256.
    cores = host_cores()
    nproc = min(usable_cores(), 64)
    cfgs = [c4_clip_config(i, preset, 1) for i in range(64)]
    sample = gen_clips(cfgs, usable_cores())
    t1, _ = timer(sample[-1].data, 1)                    # a 640x480 clip, the slow kind
    waves = (64 + nproc - 1) // nproc
    reps = max(1, int(2.0 * per / max(t1 * waves, 1e-6)))
    import multiprocessing as mp
    t0 = time.perf_counter()
    with mp.get_context("spawn").Pool(nproc) as pool:
        t_start = time.perf_counter()
        r = pool.map(_time_clip_worker, [(c.data, reps) for c in sample], chunksize=1)
        t_all = time.perf_counter() - t_start
    px_all = sum(px for _t, px in r)
    res["all_cores_C4"] = {"value": round(px_all / t_all / 1e6, 1), "unit": "Mpixels/s", "cores": nproc, "nproc": cores,
                           "processes": nproc, "cgroup_cpu_quota_cores": cpu_quota(), "host_logical_cpus": os.cpu_count(),
                           "sample": f"all 64 C4 clips (32 x 320x240 + 32 x 640x480, HVQM4 1.3/1.5 alternating, one 16-picture GOP each), "
                                     f"{reps} passes per clip, one process per clip over {nproc} processes "
                                     f"(wall time of the pool map {t_all:.1f} s, process start-up {t_start - t0:.1f} s excluded)"}
    info = {}
    try:
        info = json.load(open(os.path.join(ROOT, "oracle", "_ref" if have_ref else ".", "build_info.json")))
    except Exception:
        pass
    fast = bridge.ref_fast_flags() if have_ref else None
    return {"value": res["C3"]["value"], "unit": "Mpixels/s", "cores": 1, "kind": kind, "sample": "C3: " + res["C3"]["sample"],
            "configs": res, "compiler": info.get("compiler"), "flags": info.get("flags_v3" if fast else "flags"),
            "note": info.get("note", "CPU restatement built by oracle/Makefile")}


if __name__ == "__main__":
    main()
