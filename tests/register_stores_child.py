"""Child process of tests/test_gpu_register_stores.py: decodes the named clips through the batched path with whatever workgroup shape the
environment forces (HVQM4_AMD_TILES_PER_WG is read once per process) and compares every picture with the CPU oracle.  Prints one line
per clip; the exit status is the number of clips that differ."""
import sys

import numpy as np

from hvqm4_amd import batch
from hvqm4_amd.container import parse_header, video_pictures
from oracle import bridge
from tests import clips


def by_name(name):
    for group in (clips.SMALL, clips.MEDIUM):
        for c in group:
            if c[0] == name:
                return clips.get(c)
    raise KeyError(name)


def decode_each(ctx, names):
    bad = 0
    for name in names:
        cl = by_name(name)
        want = bridge.oracle_decode(cl.data, cl.n_pictures)
        got = batch.decode_clip(ctx, cl.data)
        same = [bool(np.array_equal(got[i], want[i])) for i in range(cl.n_pictures)]
        print(name, "ok" if all(same) else "DIFFERS at pictures %s" % [i for i, s in enumerate(same) if not s], flush=True)
        bad += not all(same)
    return bad


def neighbours(ctx, name):
    """two streams of one clip, opened one after the other with the fewest slots the clip needs, submitted in turns and flushed once: their
    pictures lie slot by slot, so a store that strays past a picture's end lands in a neighbour that is checked too"""
    cl = by_name(name)
    want = bridge.oracle_decode(cl.data, cl.n_pictures)
    hdr = parse_header(cl.data)
    pics = list(video_pictures(cl.data))
    sids = [ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, len(pics)) for _ in range(2)]
    for ft, _d, p in pics:
        for sid in sids:
            ctx.submit(sid, ft, bytes(p))
    ctx.flush()
    bad = 0
    for sid in sids:
        same = all(np.array_equal(ctx.read_picture(sid, i), want[i]) for i in range(len(pics)))
        print("neighbours", name, sid, "ok" if same else "DIFFERS", flush=True)
        bad += not same
    for sid in sids:
        ctx.close_stream(sid)
    return bad


if __name__ == "__main__":
    ctx = batch.Context(0)
    if sys.argv[1] == "neighbours":
        rc = neighbours(ctx, sys.argv[2])
    else:
        rc = decode_each(ctx, sys.argv[1:])
    ctx.close()
    sys.exit(rc)
