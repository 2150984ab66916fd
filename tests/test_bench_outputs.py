"""bench.py's plain run and `--dump-outputs DIR`.  CPU: the dump stays under its size cap, takes the same positions every time
and passes over slots a later picture reused.  GPU: a plain run (no `--full`) times exactly `--steps` steps, prints the headline
fields without the side legs, and the pictures it dumps are the CPU oracle's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class _FakeContext:
    """read_picture of a context whose streams keep their last `keep` pictures (Y|U|V of `nbytes` bytes)"""

    def __init__(self, nbytes, n_pics, keep):
        self.nbytes, self.n_pics, self.keep = nbytes, n_pics, keep

    def read_picture(self, sid, ordinal):
        from hvqm4_amd._lib import HVQ_E_STATE, HvqError
        if ordinal < self.n_pics - self.keep:
            raise HvqError(HVQ_E_STATE, "slot reused")
        return ((np.arange(self.nbytes, dtype=np.int64) * (sid + 1) + ordinal * 7) % 251).astype(np.uint8)


def _dump(tmp, ctx, streams):
    import bench
    bench.dump_outputs(ctx, list(range(streams)), [ctx.n_pics] * streams, str(tmp))
    return {f: np.load(os.path.join(tmp, f)) for f in sorted(os.listdir(tmp))}


def test_dump_of_the_default_workload_fits_the_cap_and_is_repeatable(tmp_path):
    import bench
    ctx = _FakeContext(640 * 480 * 3 // 2, 16, 6)                   # the default c5 share: 128 streams of 16 pictures, 6 slots
    a = _dump(tmp_path / "a", ctx, 128)
    b = _dump(tmp_path / "b", ctx, 128)
    assert sorted(a) == [f"picture_s{s:03d}.npy" for s in range(8)] + ["resident_sample.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in a) <= bench.DUMP_BYTES
    for f in a:
        assert a[f].dtype == np.float32 and np.array_equal(a[f], b[f]), f
    assert np.array_equal(a["picture_s003.npy"], ctx.read_picture(3, 15).astype(np.float32))
    rows = a["resident_sample.npy"]
    assert rows.shape[0] == 128 * 6 and rows.shape[1] >= 1024
    full = ctx.read_picture(0, 10)                                  # first resident picture of stream 0
    assert set(rows[0].astype(np.uint8).tolist()) <= set(full.tolist())


def test_dump_stays_under_the_cap_with_many_streams(tmp_path):
    import bench
    ctx = _FakeContext(640 * 480 * 3 // 2, 16, 6)
    a = _dump(tmp_path, ctx, 1024)
    assert sum(os.path.getsize(tmp_path / f) for f in a) <= bench.DUMP_BYTES
    assert a["resident_sample.npy"].shape[0] == 1024 * 6


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_decoded_pictures(tmp_path):
    import bench
    from hvqm4_amd.synth import SynthConfig
    from oracle import bridge
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--streams", "8", "--distinct", "2", "--width", "320",
           "--height", "240", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK")}
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads(p.stdout.strip().splitlines()[-1])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["metric"] == "decoded Mpixels/s (bit-exact YUV)" and d["unit"] == "Mpixels/s" and d["higher_is_better"] is True
    assert d["dtype"] == "u8" and d["ms_per_step"] > 0
    assert abs(d["value"] - 8 * 16 * 320 * 240 / (d["ms_per_step"] * 1e-3) / 1e6) < 0.01 * d["value"]
    for side in ("cpu_baseline", "sdk_path", "c4_share", "single_clip", "rgb_epilogue", "c5_staggered"):
        assert side not in d, side
    assert d["end_to_end_gpu_parse"] is None and d["verified_pictures"] is None
    # stream s replays clip s mod 2 (seed 1000 + s mod 2); every dumped picture is one the oracle decodes from it
    cfgs = [SynthConfig(width=320, height=240, version="1.5", gop=bench.GOP16, seed=1000 + i, preset="dense", mv_res_bits=(0, 1, 2))
            for i in range(2)]
    want = [bridge.oracle_decode(c.data, 16) for c in bench.gen_clips(cfgs, 1)]
    for s in range(8):
        got = np.load(out / f"picture_s{s:03d}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, want[s % 2][15].astype(np.float32)), s
    rows = np.load(out / "resident_sample.npy")
    assert rows.shape[0] == 8 * 6 and rows.dtype == np.float32
    frac = np.sort(np.random.default_rng(bench.DUMP_SEED).random(rows.shape[1]))
    idx = (frac * want[0].shape[1]).astype(np.int64)
    for r, row in enumerate(rows):
        assert any(np.array_equal(row, w[idx].astype(np.float32)) for w in want[(r // 6) % 2]), r
