"""GPU: batches split into launch groups (hvq_context_set_group_bytes) decode the oracle's pictures.

A batch whose reuse window exceeds the context's budget runs group by group: each launch queue walks all dependency levels of group 0's
streams, then group 1's (build_tiles, hvq_runtime.cpp).  The shapes are the smallest at which each part can go wrong: 32 streams on two
queues (two groups of 16), 40 streams with a larger clip among them (uneven work, dealt 20 and 20), 16 streams on one queue (groups of
8, the minimum), and a stream whose P pictures reference themselves, whose raster-order walks must follow their own group's launch.
The budget is forced through the setter to half the batch's window, which the rule turns into G = 2.

After every case the resident batch is run again (replay_stage(2, 1): forked and joined per pass as a flush; replay(2): the queues run
free) and the pictures are read once more.  The batch with the self-referencing stream cannot be replayed -- the library refuses, because
the previous content those pictures read is gone after the first pass -- so there the refusal is what is checked."""
import numpy as np
import pytest

from hvqm4_amd.synth import SynthConfig, make_clip
from tests import clips
from tests.test_launch_groups_cpu import stream, window

pytestmark = pytest.mark.gpu

GOP = "IPBBPBB"
_clips, _want = {}, {}


def small(seed, w=64, h=48):
    """a 4:2:0 clip of HVQM4 1.5, GOP IPBBPBB, and the oracle's pictures of it (decoded once)"""
    key = (seed, w, h)
    if key not in _clips:
        from oracle import bridge
        _clips[key] = make_clip(SynthConfig(width=w, height=h, gop=GOP, seed=seed, version="1.5"))
        _want[key] = bridge.oracle_decode(_clips[key].data, _clips[key].n_pictures)
    return _clips[key], _want[key]


def selfref():
    if "selfref" not in _clips:
        from oracle import bridge
        _clips["selfref"] = clips.get(next(c for c in clips.SMALL if c[0] == "pselfref64x48_15"))
        _want["selfref"] = bridge.oracle_decode(_clips["selfref"].data, _clips["selfref"].n_pictures)
    return _clips["selfref"], _want["selfref"]


def half_window(batch_clips):
    """the budget that makes two groups of the batch: half its reuse window, rounded up (a slot per picture: only the references count)"""
    total = sum(window(stream(cl.width * cl.height * 3 // 2, "".join("IPB"[(ft >> 4) - 1] for ft in cl.kinds), len(cl.kinds) + 3)) for cl, _w in batch_clips)
    return (total + 1) // 2


def decode(batch_clips, budget, queues=2):
    """the clips as one batch of a context of its own, submitted in turns, one flush -> (context, stream ids)"""
    from hvqm4_amd import batch
    from hvqm4_amd.container import parse_header, video_pictures
    ctx = batch.Context(0)
    ctx.set_launch_queues(queues)
    ctx.set_group_bytes(budget)
    sids, pics = [], []
    for cl, _want_pics in batch_clips:
        hdr = parse_header(cl.data)
        seq = list(video_pictures(cl.data))
        sids.append(ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, len(seq) + 3))
        pics.append(seq)
    for k in range(max(len(p) for p in pics)):
        for sid, seq in zip(sids, pics):
            if k < len(seq):
                ctx.submit(sid, seq[k][0], seq[k][2])
    ctx.flush()
    return ctx, sids


def check_pictures(ctx, sids, batch_clips, what):
    for s, (sid, (cl, want)) in enumerate(zip(sids, batch_clips)):
        for k in range(cl.n_pictures):
            assert np.array_equal(ctx.read_picture(sid, k), want[k]), f"{what}: picture {k} of stream {s} ({cl.width}x{cl.height})"


def check_replays(ctx, sids, batch_clips):
    assert ctx.replay_stage(2, 1) > 0
    check_pictures(ctx, sids, batch_clips, "after replay_stage(2, 1)")
    assert ctx.replay(2) > 0
    check_pictures(ctx, sids, batch_clips, "after replay(2)")


def test_32_streams_on_two_queues_in_two_groups():
    batch_clips = [small(100 + s % 4) for s in range(32)]
    ctx, sids = decode(batch_clips, half_window(batch_clips))
    one, sids1 = decode(batch_clips, 0)
    try:
        assert ctx.launch_groups() == 2 and one.launch_groups() == 1
        st, st1 = ctx.stats(), one.stats()
        assert st.launch_queues == st1.launch_queues == 2
        assert st1.launches == 2 * 4                           # four levels on two queues
        assert st.launches == 2 * st1.launches
        assert st.pictures == st1.pictures == 32 * 7 and st.workgroups == st1.workgroups
        check_pictures(ctx, sids, batch_clips, "two groups")
        for sid, sid1, (cl, _w) in zip(sids, sids1, batch_clips):
            for k in range(cl.n_pictures):
                assert np.array_equal(ctx.read_picture(sid, k), one.read_picture(sid1, k))
        check_replays(ctx, sids, batch_clips)
    finally:
        ctx.close()
        one.close()


def test_40_streams_with_a_larger_clip_among_them():
    batch_clips = [small(100 + s % 4) for s in range(40)]
    batch_clips[13] = small(104, 72, 56)
    ctx, sids = decode(batch_clips, half_window(batch_clips))
    try:
        assert ctx.launch_groups() == 2
        assert ctx.stats().pictures == 40 * 7
        check_pictures(ctx, sids, batch_clips, "two groups of 20")
        check_replays(ctx, sids, batch_clips)
    finally:
        ctx.close()


def test_16_streams_on_one_queue_in_groups_of_eight():
    batch_clips = [small(100 + s % 4) for s in range(16)]
    ctx, sids = decode(batch_clips, half_window(batch_clips), queues=1)
    try:
        st = ctx.stats()
        assert ctx.launch_groups() == 2 and st.launch_queues == 1
        assert st.launches == 2 * 4                            # four levels, twice
        check_pictures(ctx, sids, batch_clips, "two groups of 8")
        check_replays(ctx, sids, batch_clips)
    finally:
        ctx.close()


def test_a_self_referencing_stream_follows_its_own_groups_launch():
    from hvqm4_amd._lib import HVQ_E_STATE, HvqError
    batch_clips = [small(100 + s % 4) for s in range(32)]
    batch_clips[11] = selfref()
    ctx, sids = decode(batch_clips, half_window(batch_clips))
    try:
        assert ctx.launch_groups() == 2 and ctx.stats().launch_queues == 2
        check_pictures(ctx, sids, batch_clips, "two groups, stream 11 self-referencing")
        for again in (lambda: ctx.replay_stage(2, 1), lambda: ctx.replay(2)):
            with pytest.raises(HvqError) as e:              # refused: the walks' previous content is gone after the first pass
                again()
            assert e.value.code == HVQ_E_STATE
            check_pictures(ctx, sids, batch_clips, "after the refused replay")
    finally:
        ctx.close()
