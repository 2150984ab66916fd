"""GPU: malformed P/B pictures (tests/test_malformed_pb.py has the CPU side) through every entry point.

* Crafted clips (synth.py pb_big_kinds, mb_type3): host-parsed submits, GPU-parsed batches, submit_many on four threads and the
  SDK calls.  Accepted pictures are bit-exact against the oracle, a refused picture is refused by both parse paths
  (HVQ_E_UNSUPPORTED, the HVQ_F_MALFORMED reason), the stream resumes at its next I picture and a neighbour stream of the same
  batches decodes unaffected.
* Mutated pictures through the host-parsed and the GPU-parsed path of one context: same verdicts, identical pictures."""
import numpy as np
import pytest

from tests import clips
from tests.test_malformed_pb import I_FRAME, REFUSE, _Host, _mutate

pytestmark = pytest.mark.gpu


def _clips():
    from hvqm4_amd.synth import SynthConfig, make_clip
    return [make_clip(SynthConfig(width=64, height=48, version="1.5", sampling="420", gop="IPBB", n_gops=3, seed=64,
                                  pb_big_kinds=0.006, p_zero=0.2)),
            make_clip(SynthConfig(width=48, height=32, version="1.3", sampling="422", gop="IPBB", n_gops=3, seed=65, mb_type3=0.5)),
            make_clip(SynthConfig(width=64, height=48, version="1.3", sampling="444", gop="IPBB", n_gops=3, seed=68,
                                  pb_big_kinds=0.006, p_zero=0.2))]


def _refused(clip):
    """the host parser's verdict per picture (the CPU suite checks that the device parse core agrees)"""
    h = _Host(clip, 1)
    try:
        out = []
        for ft, pic in zip(clip.kinds, clip.pictures):
            rc, fl, _b = h.parse(ft, pic)
            assert rc == 0
            out.append(bool(fl & REFUSE))
    finally:
        h.close()
    assert any(out) and not all(out)
    return out


def _gops(clip):
    starts = [k for k, ft in enumerate(clip.kinds) if ft == I_FRAME] + [clip.n_pictures]
    return [list(range(a, b)) for a, b in zip(starts[:-1], starts[1:])]


def _expect(clip, refused):
    """per picture: 'ok' (decoded), 'refused' (HVQ_E_UNSUPPORTED) or 'state' (behind a refusal, before the next I picture)"""
    out, need_i = [], False
    for k, ft in enumerate(clip.kinds):
        if ft == I_FRAME:
            need_i = False
        if need_i:
            out.append("state")
        elif refused[k]:
            out.append("refused"); need_i = True
        else:
            out.append("ok")
    return out


@pytest.mark.parametrize("which", [0, 1, 2])
def test_crafted_malformed_pictures_through_every_entry_point(gpu_ctx, which):
    from hvqm4_amd import sdk
    from hvqm4_amd._lib import HVQ_E_STATE, HVQ_E_UNSUPPORTED, HvqError
    from oracle import bridge
    clip = _clips()[which]
    want = bridge.oracle_decode(clip.data, clip.n_pictures)
    refused = _refused(clip)
    expect = _expect(clip, refused)
    pics = list(zip(clip.kinds, clip.pictures))
    samp = (clip.samp_h, clip.samp_v)
    is15 = clip.version == "1.5"
    good = clips.get(clips.SMALL[3])
    gp = [(ft, bytes(p)) for ft, p in zip(good.kinds, good.pictures)]
    want_g = bridge.oracle_decode(good.data, good.n_pictures)

    # 1. host-parsed submits, picture by picture
    sid = gpu_ctx.open_stream(clip.width, clip.height, *samp, is15, clip.n_pictures + 3)
    ords = {}
    for k, (ft, pic) in enumerate(pics):
        if expect[k] == "ok":
            ords[k] = gpu_ctx.submit(sid, ft, pic)
            continue
        with pytest.raises(HvqError) as e:
            gpu_ctx.submit(sid, ft, pic)
        if expect[k] == "refused":
            assert e.value.code == HVQ_E_UNSUPPORTED and "malformed" in str(e.value), k
        else:
            assert e.value.code == HVQ_E_STATE, k
    gpu_ctx.flush()
    for k, o in ords.items():
        assert np.array_equal(gpu_ctx.read_picture(sid, o), want[k]), ("host-parsed", k)
    gpu_ctx.close_stream(sid)

    # 2. GPU-parsed batches, one GOP each, beside a legal neighbour stream; 3. the same GOPs through submit_many on four threads
    for path in ("device", "many"):
        sid = gpu_ctx.open_stream(clip.width, clip.height, *samp, is15, clip.n_pictures + 3)
        sg = gpu_ctx.open_stream(good.width, good.height, 2, 2, True, 4 * len(gp) + 3)
        for gop in _gops(clip):
            bad_at = next((k for k in gop if refused[k]), None)
            if path == "device":
                o = gpu_ctx.submit_many_device([sid] * len(gop), [pics[k][0] for k in gop], [pics[k][1] for k in gop])
                og = gpu_ctx.submit_many_device([sg] * len(gp), [p[0] for p in gp], [p[1] for p in gp])
                if bad_at is None:
                    gpu_ctx.flush()
                else:
                    with pytest.raises(HvqError) as e:
                        gpu_ctx.flush()
                    assert e.value.code == HVQ_E_UNSUPPORTED and f"stream {sid} picture" in str(e.value), bad_at
                    gpu_ctx.sync()
            else:
                og = gpu_ctx.submit_many([sg] * len(gp), [p[0] for p in gp], [p[1] for p in gp], threads=4)
                if bad_at is None:
                    o = gpu_ctx.submit_many([sid] * len(gop), [pics[k][0] for k in gop], [pics[k][1] for k in gop], threads=4)
                else:
                    with pytest.raises(HvqError) as e:
                        gpu_ctx.submit_many([sid] * len(gop), [pics[k][0] for k in gop], [pics[k][1] for k in gop], threads=4)
                    assert e.value.code == HVQ_E_UNSUPPORTED and "malformed" in str(e.value), bad_at
                    o = None                                   # nothing of the call was queued
                gpu_ctx.flush()
            for k, ok in enumerate(og):                        # the neighbour: unaffected
                assert np.array_equal(gpu_ctx.read_picture(sg, ok), want_g[k]), (path, "neighbour", k)
            if o is None:
                continue
            for j, k in enumerate(gop):
                if bad_at is None or k < bad_at:
                    assert np.array_equal(gpu_ctx.read_picture(sid, o[j]), want[k]), (path, k)
                else:                                          # the refused picture and what followed it: not resident
                    with pytest.raises(HvqError) as e2:
                        gpu_ctx.read_picture(sid, o[j])
                    assert e2.value.code == HVQ_E_STATE
        gpu_ctx.close_stream(sid); gpu_ctx.close_stream(sg)

    # 4. the SDK calls: a fresh player per GOP, up to the GOP's first refusal
    for gop in _gops(clip):
        pl = sdk.Player(clip.width, clip.height, *samp, is15)
        try:
            for k in gop:
                if refused[k]:
                    with pytest.raises(HvqError) as e:
                        pl.decode(*pics[k])
                    assert e.value.code == HVQ_E_UNSUPPORTED, k
                    break
                assert np.array_equal(pl.decode(*pics[k]), want[k]), ("sdk", k)
        finally:
            pl.close()


def test_mutated_pictures_reach_the_same_verdict_on_both_parse_paths(gpu_ctx):
    """byte overwrites, bit flips and truncations of P and B pictures: host-parsed and GPU-parsed streams of one context take or refuse
    the same pictures, and what they take reads back identical.  One mutated picture per batch (a capped one is parsed again on the
    host: far below the bound of tests/test_gpu_reject.py test_host_reparses_of_capped_pictures_are_bounded_per_batch)."""
    from hvqm4_amd._lib import HvqError
    from hvqm4_amd.synth import SynthConfig, make_clip
    rng = np.random.default_rng(41)
    taken = refused = 0
    for seed, (w, h, samp, preset) in enumerate([(64, 48, "420", "dense"), (96, 64, "422", "natural"), (48, 80, "444", "realistic"),
                                                 (160, 96, "420", "flat")]):
        clip = make_clip(SynthConfig(width=w, height=h, gop="IPB", seed=seed + 51, preset=preset, sampling=samp))
        pics = list(zip(clip.kinds, clip.pictures))
        hs, vs = clip.samp_h, clip.samp_v
        for v in range(10):
            k = 1 + v % 2                                        # the P picture, then the B picture
            q = _mutate(rng, pics[k][1], v)
            if v % 4 == 3:                                       # and garbage in the head of the sections: trees, kinds, type runs
                q = bytearray(q)
                for _ in range(16):
                    q[int(rng.integers(8 + 0x44, min(len(q), 8 + 0x44 + 96)))] = int(rng.integers(0, 256))
                q = bytes(q)
            seq = pics[:k] + [(pics[k][0], q)]
            s_host = gpu_ctx.open_stream(w, h, hs, vs, True, 6)
            s_dev = gpu_ctx.open_stream(w, h, hs, vs, True, 6)
            host_ok = True
            for j, (ft, p) in enumerate(seq):
                try:
                    gpu_ctx.submit(s_host, ft, p)
                except HvqError:
                    assert j == k
                    host_ok = False
            gpu_ctx.submit_many_device([s_dev] * len(seq), [p[0] for p in seq], [p[1] for p in seq])
            dev_ok = True
            try:
                gpu_ctx.flush()
            except HvqError as e:
                assert f"stream {s_dev} picture {k}" in str(e), str(e)
                dev_ok = False
                gpu_ctx.sync()
            assert host_ok == dev_ok, (seed, v)
            if host_ok:
                assert np.array_equal(gpu_ctx.read_picture(s_host, k), gpu_ctx.read_picture(s_dev, k)), (seed, v)
                taken += 1
            else:
                refused += 1
            gpu_ctx.close_stream(s_host); gpu_ctx.close_stream(s_dev)
    assert taken > 0 and refused > 0
