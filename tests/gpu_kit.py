"""What the cases of the tests/test_gpu_*.py files share on the child's side (tests/gpu_child.py): the clips and their decoding, the
oracle's pictures, outputs between guards of sentinel bytes and their byte-for-byte check, pictures uploaded for src=.  Torch is the
child's and is passed in; nothing here imports it or the library at module level."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5
GUARD = 256
# the clips of tests/test_gpu_checksums.py and tests/test_gpu_phash.py: all three samplings, a 240-byte chroma plane, a 24-wide plane
SEVEN_CLIPS = ["ragged24x40", "gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "wide296x160", "natural128x96", "pselfref64x48_15"]
LONG = dict(width=640, height=480, gop="IPBBPBBPBBPB", seed=61)        # the clip of tests/test_gpu_export.py's slot-safety case

_cache = {}


# ------------------------------------------------------------------------------------------------------------------ clips
def clip(name):
    return open(os.path.join(ROOT, "tests", "golden", name + ".h4m"), "rb").read()


def geom(hdr):
    return (hdr.width, hdr.height, hdr.h_samp, hdr.v_samp)


def decode(ctx, data, nslots=None):
    """a clip through the batched path: (sid, header, number of pictures)"""
    from hvqm4_amd.container import parse_header, video_pictures
    hdr = parse_header(data)
    pics = list(video_pictures(data))
    sid = ctx.open_stream(hdr.width, hdr.height, hdr.h_samp, hdr.v_samp, hdr.is15, nslots or len(pics) + 3)
    for ft, _d, p in pics:
        ctx.submit(sid, ft, p)
    ctx.flush()
    return sid, hdr, len(pics)


def golden():
    """the golden clips: [(name, data, header, number of pictures)]"""
    from tests.test_export_cpu import golden_clips
    return list(golden_clips())


def golden_by_name():
    """the golden clips, read once: name -> (data, header, number of pictures)"""
    if "golden" not in _cache:
        _cache["golden"] = {name: (data, hdr, n) for name, data, hdr, n in golden()}
    return _cache["golden"]


def oracle(name, data, n):
    """the oracle's pictures of a clip, decoded once for all cases"""
    if ("yuv", name) not in _cache:
        from oracle import bridge
        _cache["yuv", name] = bridge.oracle_decode(data, n)
    return _cache["yuv", name]


def synth(width, height, gop, seed):
    """the bytes of a synthesised clip, made once"""
    key = ("synth", width, height, gop, seed)
    if key not in _cache:
        from hvqm4_amd.synth import SynthConfig, make_clip
        _cache[key] = make_clip(SynthConfig(width=width, height=height, gop=gop, seed=seed)).data
    return _cache[key]


def long_clip():
    from hvqm4_amd.synth import SynthConfig, make_clip
    return make_clip(SynthConfig(**LONG))


def long_clip_data():
    return synth(**LONG)


def pics(cl):
    """[(frame type, picture bytes)] of a clip, or of a patched one"""
    from hvqm4_amd.container import video_pictures
    if hasattr(cl, "pics"):
        return list(cl.pics)
    return [(ft, bytes(p)) for ft, _d, p in video_pictures(cl.data)]


class Patched:
    """a clip with one picture replaced (what the container iterator would hand out)"""
    def __init__(self, clip, pics):
        self.width, self.height, self.version, self.data, self.n_pictures, self.pics = clip.width, clip.height, clip.version, clip.data, clip.n_pictures, pics


def self_ref_clip(seed=5, w=64, h=48, gop="IPBBPB"):
    """a clip whose SECOND picture (the first P) can never be decoded like the reference: its luma DC tree is a single leaf 0x7F
    with dc_shift 0, outside the overflow window (-128, 127) -- every overflow read of the section spins for ever"""
    import struct
    from hvqm4_amd.synth import SynthConfig, make_clip
    clip = make_clip(SynthConfig(width=w, height=h, gop=gop, seed=seed))
    ps = pics(clip)
    b = bytearray(ps[1][1])
    off = 8 + 0x44 + struct.unpack_from(">I", b, 8 + 4 * 4)[0] + 4           # section 4 = DC buffer of the luma plane
    b[0] = 0
    b[off:off + 2] = b"\x3f\x80"
    ps[1] = (ps[1][0], bytes(b))
    return Patched(clip, ps)


# ------------------------------------------------------------------------------------------------ outputs between guards
def rooms(torch, nb, uniform):
    """out for a call that writes pictures of nb[i] bytes, with GUARD sentinel bytes before and behind every allocation -> (out,
    guards): one tensor [n, bytes] when `uniform` (the byte counts are one), a list otherwise"""
    n = len(nb)
    if uniform:
        room = torch.full((n * nb[0] + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        return room[GUARD:GUARD + n * nb[0]].view(n, nb[0]), [room[:GUARD], room[GUARD + n * nb[0]:]]
    rs = [torch.full((b + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for b in nb]
    return [r[GUARD:GUARD + b] for r, b in zip(rs, nb)], [r[:GUARD] for r in rs] + [r[GUARD + b:] for r, b in zip(rs, nb)]


def geometry_rooms(torch, geoms):
    """rooms for pictures of the geometries `geoms` in slot layout: one tensor when they are one geometry, a list otherwise"""
    from hvqm4_amd import scale
    geoms = [tuple(g) for g in geoms]
    return rooms(torch, [scale.nbytes(*g) for g in geoms], bool(geoms) and all(g == geoms[0] for g in geoms))


def check_bytes(torch, got, guards, wants, what):
    """the guards untouched, then got[i] == wants[i] (bytes or arrays) byte for byte"""
    for g in guards:
        assert g.numel() == GUARD and bool(g.eq(SENTINEL).all()), f"{what}: the bytes around an output were written"
    assert len(got) == len(wants), what
    for i, (g, w) in enumerate(zip(got, wants)):
        g = g.cpu().numpy()
        w = np.frombuffer(w, dtype=np.uint8) if isinstance(w, bytes) else np.asarray(w, dtype=np.uint8).reshape(-1)
        assert g.shape == w.shape, (what, i, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError(f"{what}: picture {i}: {bad.size} of {g.size} bytes differ, first at {bad[0]}: got {g[bad[0]]}, want {w[bad[0]]}")


class Uploaded:
    """pictures in the caller's memory (src=), on streams that nothing was decoded into: one stream of three slots per geometry"""

    def __init__(self, torch, ctx, pics, geoms):
        self.ctx, self.pics, self.geoms, self.by_geom = ctx, pics, list(geoms), {}
        for g in geoms:
            if g not in self.by_geom:
                self.by_geom[g] = ctx.open_stream(g[0], g[1], g[2], g[3], True, 3)
        self.sids = [self.by_geom[g] for g in geoms]
        self.bufs = [torch.from_numpy(np.array(p, dtype=np.uint8)).cuda() for p in pics]

    def close(self):
        for s in self.by_geom.values():
            self.ctx.close_stream(s)


# --------------------------------------------------------------------------------------------------- the runtime's lines
# the runtime's line per launch under HVQM4_AMD_FLUSH_TIMING (hvq_runtime.cpp, flush_end); tests/test_fake_device.py pins it without a GPU
LAUNCH_LINE = re.compile(r"^\[flush\] launch (?P<launch>\d+) \(level (?P<level>\d+), queue (?P<queue>\d+)\): fullest tile (?P<max_items>\d+) items, "
                         r"(?P<max_pairs>\d+) pairs -> (?P<tpw>\d+) tile\(s\) per workgroup, items (?P<items>\d+), pairs (?P<pairs>\d+), pool (?P<pool>\d+), "
                         r"(?P<lds>\d+) B of LDS = (?P<workgroups>\d+) workgroups per CU$")


def launch_lines(stderr):
    """the `[flush] launch` lines of a run as dicts of integers; a line that starts like one and does not match the expression fails"""
    out = []
    for line in stderr.splitlines():
        if line.startswith("[flush] launch"):
            m = LAUNCH_LINE.match(line)
            assert m, f"the runtime's launch line has changed: {line!r}"
            out.append({k: int(v) for k, v in m.groupdict().items()})
    return out
