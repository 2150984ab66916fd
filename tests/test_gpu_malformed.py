"""GPU: malformed P/B pictures (tests/test_malformed_pb.py has the CPU side) through every entry point.

* Crafted clips (synth.py pb_big_kinds, mb_type3): host-parsed submits, GPU-parsed batches, submit_many on four threads and the
  SDK calls.  Accepted pictures are bit-exact against the oracle, a refused picture is refused by both parse paths
  (HVQ_E_UNSUPPORTED, the HVQ_F_MALFORMED reason), the stream resumes at its next I picture and a neighbour stream of the same
  batches decodes unaffected.
* Mutated pictures through the host-parsed and the GPU-parsed path of one context: same verdicts, identical pictures.
* A fixed slice of the corpus of tests/test_mutants_vs_oracle.py (288 mutants of I, P and B pictures, 4:2:0 / 4:2:2 / 4:4:4, a
  p_future_refs clip for hvq_selfref_kernel) and the cross-plane clips of tests/clips.py against the CHECKED oracle: what it
  classes `defined` decodes bit-exact on every path (and equals the compiled reference where that is built), everything else is
  refused with HVQ_E_UNSUPPORTED; the stream resumes at its next I picture, a neighbour stream of the same batches is unaffected.
  Under HVQM4_AMD_ALLOW_CLAMPED=1 the `mem` mutants decode to completion (the kernels pin every address into the slot)."""
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


# ---- against the checked oracle (tests/test_mutants_vs_oracle.py has the CPU side and the corpus)
SLICE = (0, 1, 2, 4)            # dense420_15, natural422_13, portrait444_15, pselfref420_15
SLICE_PB, SLICE_I = 16, 8      # mutants per picture: 3 * (3 * 16 + 8) + (7 * 16 + 8) = 288


def _sdk_length(ft, q, clean):
    """the length the SDK calls take a picture to have -- they are given none, and read it off the picture's own section table
    (hvq_picture_length) -- or None where that walk would leave the buffer: a changed offset table, a truncated picture, a section
    that ends behind the bytes we hold (the SDK contract wants HVQM4SetMaxFrameSize for such input)"""
    nsec = 16 if ft == I_FRAME else 17
    base = 8 + 4 * nsec
    if len(q) != len(clean) or q[8:base] != clean[8:base]:
        return None
    end = base
    for i in range(nsec):
        at = base + int.from_bytes(q[8 + 4 * i:12 + 4 * i], "big")
        if at + 4 > len(q):
            return None
        end = max(end, at + 4 + int.from_bytes(q[at:at + 4], "big"))
    return end if end <= len(q) else None


def _slice(n):
    """[(k, frame type, mutant, class mask, oracle picture or None, host parser's return code, the same three for the picture as
    the SDK calls see it or None)] of corpus clip n, and the clip"""
    from hvqm4_amd.synth import make_clip
    from tests import test_mutants_vs_oracle as tm
    name, cfg = tm.CONFIGS[n]
    clip = make_clip(cfg)
    pl = tm.player_for(clip)
    host = _Host(clip, 1)
    out, clean = [], []
    try:
        for k, ft, muts in tm.mutants_of(clip, 500 + n):
            for q in muts[:SLICE_I if ft == I_FRAME else SLICE_PB]:
                cls, _rep, want = pl.check(ft, q)
                sdk_len = _sdk_length(ft, q, clip.pictures[k])
                as_sdk = None
                if sdk_len is not None:
                    cls_s, _rep, want_s = pl.check(ft, q[:sdk_len])
                    as_sdk = (q[:sdk_len], cls_s, want_s, host.parse(ft, q[:sdk_len])[0])
                out.append((k, ft, q, cls, want, host.parse(ft, q)[0], as_sdk))
            clean.append(pl.advance(ft, clip.pictures[k]))
            host.parse(ft, clip.pictures[k])
    finally:
        pl.close(); host.close()
    return name, clip, out, clean


@pytest.mark.parametrize("n", SLICE)
def test_mutants_against_the_checked_oracle_on_every_path(gpu_ctx, n, monkeypatch):
    from hvqm4_amd import sdk
    from hvqm4_amd._lib import HVQ_E_STATE, HVQ_E_UNSUPPORTED, HvqError
    from oracle import bridge
    from tests import test_mutants_vs_oracle as tm
    monkeypatch.delenv("HVQM4_AMD_ALLOW_CLAMPED", raising=False)
    name, clip, muts, clean = _slice(n)
    pics = list(zip(clip.kinds, clip.pictures))
    samp = (clip.samp_h, clip.samp_v)
    is15 = clip.version == "1.5"
    good = clips.get(clips.SMALL[3])
    gp = [(ft, bytes(p)) for ft, p in zip(good.kinds, good.pictures)]
    want_g = bridge.oracle_decode(good.data, good.n_pictures)
    accepted = refused = limits = through_sdk = 0
    ref_jobs = []
    for v, (k, ft, q, cls, want, host_rc, as_sdk) in enumerate(muts):
        where = (name, k, hex(ft), v, bridge.class_name(cls))
        if host_rc != 0:                                     # more payload than a blob holds (HVQ_E_OVERFLOW): a limit, the CPU suite counts them
            limits += 1
            continue
        seq = pics[:k] + [(ft, q)]
        # 1. host-parsed submits
        sid = gpu_ctx.open_stream(clip.width, clip.height, *samp, is15, k + 6)
        for ft2, p in seq[:-1]:
            gpu_ctx.submit(sid, ft2, p)
        if cls == 0:
            o = gpu_ctx.submit(sid, ft, q)
            gpu_ctx.flush()
            assert np.array_equal(gpu_ctx.read_picture(sid, o), want), (where, "host-parsed")
        else:
            with pytest.raises(HvqError) as e:
                gpu_ctx.submit(sid, ft, q)
            assert e.value.code == HVQ_E_UNSUPPORTED, where
            if k + 1 < len(pics) and pics[k + 1][0] != I_FRAME:
                with pytest.raises(HvqError) as e:           # what follows a refusal waits for an I picture
                    gpu_ctx.submit(sid, *pics[k + 1])
                assert e.value.code == HVQ_E_STATE, where
        o = gpu_ctx.submit(sid, *pics[0])                    # the stream resumes at its next I picture
        gpu_ctx.flush()
        assert np.array_equal(gpu_ctx.read_picture(sid, o), clean[0]), (where, "host-parsed, resumed")
        gpu_ctx.close_stream(sid)
        # 2. GPU-parsed batch beside a legal neighbour stream
        sid = gpu_ctx.open_stream(clip.width, clip.height, *samp, is15, k + 6)
        sg = gpu_ctx.open_stream(good.width, good.height, 2, 2, True, len(gp) + 3)
        o = gpu_ctx.submit_many_device([sid] * len(seq), [p[0] for p in seq], [p[1] for p in seq])
        og = gpu_ctx.submit_many_device([sg] * len(gp), [p[0] for p in gp], [p[1] for p in gp])
        if cls == 0:
            gpu_ctx.flush()
            assert np.array_equal(gpu_ctx.read_picture(sid, o[k]), want), (where, "GPU-parsed")
        else:
            with pytest.raises(HvqError) as e:
                gpu_ctx.flush()
            assert e.value.code == HVQ_E_UNSUPPORTED and f"stream {sid} picture" in str(e.value), where
            gpu_ctx.sync()
            with pytest.raises(HvqError) as e2:
                gpu_ctx.read_picture(sid, o[k])
            assert e2.value.code == HVQ_E_STATE, where
        for j in range(k):                                   # the clean pictures in front of it
            assert np.array_equal(gpu_ctx.read_picture(sid, o[j]), clean[j]), (where, "GPU-parsed", j)
        for j, oj in enumerate(og):
            assert np.array_equal(gpu_ctx.read_picture(sg, oj), want_g[j]), (where, "neighbour", j)
        o = gpu_ctx.submit_many_device([sid], [pics[0][0]], [pics[0][1]])
        gpu_ctx.flush()
        assert np.array_equal(gpu_ctx.read_picture(sid, o[0]), clean[0]), (where, "GPU-parsed, resumed")
        gpu_ctx.close_stream(sid); gpu_ctx.close_stream(sg)
        # 3. the SDK calls, on the picture as they see it (_sdk_length)
        if as_sdk is not None and as_sdk[3] == 0:
            q_s, cls_s, want_s, _rc = as_sdk
            pl = sdk.Player(clip.width, clip.height, *samp, is15)
            try:
                for ft2, p in seq[:-1]:
                    pl.decode(ft2, p)
                if cls_s == 0:
                    assert np.array_equal(pl.decode(ft, q_s), want_s), (where, "sdk")
                else:
                    with pytest.raises(HvqError) as e:
                        pl.decode(ft, q_s)
                    assert e.value.code == HVQ_E_UNSUPPORTED, where
                assert np.array_equal(pl.decode(*pics[0]), clean[0]), (where, "sdk, resumed")
            finally:
                pl.close()
            through_sdk += 1
        if cls == 0:
            accepted += 1
            ref_jobs.append((k, q, want))
        else:
            refused += 1
    assert accepted >= len(muts) // 5 and refused >= len(muts) // 5 and limits <= 3, (accepted, refused, limits)
    assert through_sdk >= len(muts) // 3, through_sdk
    if bridge.have_ref():
        tm._through_reference(name, clip, ref_jobs)


def test_mem_mutants_decode_to_completion_when_clamping_is_allowed(gpu_ctx, monkeypatch):
    """HVQM4_AMD_ALLOW_CLAMPED=1 over the `mem` mutants only: the kernels pin every address into the slot (each stage by its own
    rule), so the pictures are invented but complete -- asserted: completion and picture size, on both parse paths"""
    from oracle import bridge
    monkeypatch.setenv("HVQM4_AMD_ALLOW_CLAMPED", "1")
    done = 0
    for n in SLICE:
        name, clip, muts, _clean = _slice(n)
        pics = list(zip(clip.kinds, clip.pictures))
        samp = (clip.samp_h, clip.samp_v)
        for k, ft, q, cls, _want, host_rc, _as_sdk in muts:
            if host_rc != 0 or cls != bridge.C_MEM:          # out-of-picture reads and nothing else
                continue
            seq = pics[:k] + [(ft, q)]
            s_host = gpu_ctx.open_stream(clip.width, clip.height, *samp, clip.version == "1.5", k + 4)
            s_dev = gpu_ctx.open_stream(clip.width, clip.height, *samp, clip.version == "1.5", k + 4)
            for ft2, p in seq:
                oh = gpu_ctx.submit(s_host, ft2, p)
            od = gpu_ctx.submit_many_device([s_dev] * len(seq), [p[0] for p in seq], [p[1] for p in seq])
            gpu_ctx.flush()
            assert gpu_ctx.read_picture(s_host, oh).size == clip.picsize
            assert gpu_ctx.read_picture(s_dev, od[k]).size == clip.picsize
            gpu_ctx.close_stream(s_host); gpu_ctx.close_stream(s_dev)
            done += 1
    assert done >= 40, done


@pytest.mark.parametrize("case", [c for c in clips.SMALL if c[0].startswith("crossplane")], ids=lambda c: c[0])
def test_cross_plane_clips_on_every_path(gpu_ctx, case):
    """MC reads that leave their plane inside the picture buffer: accepted, and bit-exact against the checked oracle (the golden
    manifest pins the same pictures to the reference)"""
    from hvqm4_amd import sdk
    from tests import test_mutants_vs_oracle as tm
    clip = clips.get(case)
    pl = tm.player_for(clip)
    want = [pl.advance(ft, pic) for ft, pic in zip(clip.kinds, clip.pictures)]
    pl.close()
    pics = list(zip(clip.kinds, clip.pictures))
    samp = (clip.samp_h, clip.samp_v)
    is15 = clip.version == "1.5"
    s_host = gpu_ctx.open_stream(clip.width, clip.height, *samp, is15, len(pics) + 3)
    s_dev = gpu_ctx.open_stream(clip.width, clip.height, *samp, is15, len(pics) + 3)
    oh = [gpu_ctx.submit(s_host, ft, p) for ft, p in pics]
    od = gpu_ctx.submit_many_device([s_dev] * len(pics), [p[0] for p in pics], [p[1] for p in pics])
    gpu_ctx.flush()
    player = sdk.Player(clip.width, clip.height, *samp, is15)
    try:
        for k, (ft, p) in enumerate(pics):
            assert np.array_equal(gpu_ctx.read_picture(s_host, oh[k]), want[k]), ("host-parsed", k)
            assert np.array_equal(gpu_ctx.read_picture(s_dev, od[k]), want[k]), ("GPU-parsed", k)
            assert np.array_equal(player.decode(ft, p), want[k]), ("sdk", k)
    finally:
        player.close()
    gpu_ctx.close_stream(s_host); gpu_ctx.close_stream(s_dev)
