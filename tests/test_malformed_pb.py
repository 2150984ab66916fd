"""CPU: malformed P/B pictures against the contract of DESIGN.md 8 f4 -- refuse, never decode differently.

* Crafted clips (synth.py pb_big_kinds, mb_type3): luma kind symbols above 15 -- the reference ORs them into the type byte and
  takes the macroblock's type and proc from the first luma block's (h4m:1701, 1927) -- and type runs that open at value 3 (a
  residual-bit count the stream does not set, a transition that indexes past its table, h4m:1591, 1606, 1950-1951).  The host
  parser (1 and 4 threads) and the GPU parse core (tests/native/gparse_emul.c, chains and flat path) must give the same verdict,
  refuse exactly those pictures with HVQ_F_MALFORMED, give the same blob for the others, and the accepted pictures must
  reconstruct (oracle/hvq_desc_recon.c) to the oracle's pictures -- which equal the compiled reference's where it is built.
* Mutated pictures: host parser against GPU parse core, verdict and whole blob.
* Sanitizer fuzz: the host parser and the parse core built with AddressSanitizer and UBSan, fed mutated pictures
  (tests/native/parse_fuzz_asan.c)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.test_gparse_emul import CHAINS, FLAT, NESTP, Result, emul, header  # noqa: F401  (emul: the fixture)

I_FRAME, P_FRAME, B_FRAME = 0x10, 0x20, 0x30
CLAMPED, CAPPED, MALFORMED = 0x20, 0x40, 0x80
REFUSE = CLAMPED | CAPPED | MALFORMED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def crafted_configs():
    """both knobs, for 4:2:0, 4:2:2 and 4:4:4, in 1.3 and 1.5; several GOPs, so that refused pictures are followed by I pictures"""
    from hvqm4_amd.synth import SynthConfig
    out = []
    for k, samp in enumerate(("420", "422", "444")):
        for ver in ("1.3", "1.5"):
            s = 60 + 4 * k + 2 * (ver == "1.5")
            out.append((f"bigkinds_{samp}_{ver}", SynthConfig(width=64, height=48, version=ver, sampling=samp, gop="IPBB", n_gops=3,
                                                              seed=s, pb_big_kinds=0.006, p_zero=0.2)))
            out.append((f"type3_{samp}_{ver}", SynthConfig(width=48, height=32, version=ver, sampling=samp, gop="IPBB", n_gops=3,
                                                           seed=s + 1, mb_type3=0.5)))
            out.append((f"type3exit0_{samp}_{ver}", SynthConfig(width=48, height=32, version=ver, sampling=samp, gop="IPBB", n_gops=3,
                                                                seed=s + 1, mb_type3=0.5, mb_type3_exits=(0,))))
    return out


CRAFTED = crafted_configs()


def _verdict(ok, flags):
    """what a back end does with the picture: the refusal flags in the order the runtime reports them"""
    if not ok:
        return "error"
    for f, name in ((MALFORMED, "malformed"), (CAPPED, "capped"), (CLAMPED, "clamped")):
        if flags & f:
            return name
    return "ok"


class _Host:
    def __init__(self, clip, threads):
        from hvqm4_amd._lib import lib
        self.l = lib()
        self.p = self.l.hvq_parser_create(clip.width, clip.height, clip.samp_h, clip.samp_v, 1 if clip.version == "1.5" else 0)
        assert self.p
        assert self.l.hvq_parser_set_threads(self.p, threads) == threads
        self.bound = self.l.hvq_parser_blob_bound(self.p)
        self.blob = np.zeros(self.bound, dtype=np.uint8)

    def parse(self, ft, pic):
        n = C.c_size_t(0)
        rc = self.l.hvq_parse_picture(self.p, ft, pic + b"\0" * 8, len(pic), self.blob.ctypes.data, self.bound, C.byref(n))
        fl = (struct.unpack_from("<I", self.blob, 20)[0] | self.l.hvq_parser_last_flags(self.p)) if rc == 0 else 0
        return rc, fl, self.blob[:n.value].copy() if rc == 0 else None

    def close(self):
        self.l.hvq_parser_destroy(self.p)


def _device(emul, clip, ft, pic, mode, cap):
    b = np.zeros(cap, dtype=np.uint8)
    nest = np.zeros(NESTP, dtype=np.uint8)
    res = Result()
    assert emul.gparse_emul2(pic, len(pic), ft, clip.width, clip.height, clip.samp_h, clip.samp_v, 1 if clip.version == "1.5" else 0,
                             b.ctypes.data, cap, nest.ctypes.data, C.byref(res), mode) == 0
    return res, b


def _same_blob(a, b, where):
    """host blob `a` against device blob `b`: header (the nest travels aside on the device), maps, vectors, run bases, pool"""
    ha, hb = header(a.tobytes()), header(b.tobytes())
    for k in ha:
        if k not in ("total", "nest_off"):
            assert ha[k] == hb[k], (where, k, ha[k], hb[k])
    for i in range(3):
        o, n = ha["map_off"][i], 2 * (ha["hb"][i] + 2) * (ha["vb"][i] + 2)
        assert np.array_equal(a[o:o + n], b[o:o + n]), (where, "map", i)
    if ha["kind"] != 0:
        o, n = ha["mv_off"], 4 * ha["mcb_w"] * ha["mcb_h"]
        assert np.array_equal(a[o:o + n], b[o:o + n]), (where, "mv")
    o, n = ha["wave_off"], 16 * ha["tile_first"][3]
    assert np.array_equal(a[o:o + n], b[o:o + n]), (where, "wave_base")
    o, n = ha["pool_off"], 4 * ha["pool_dwords"]
    assert np.array_equal(a[o:o + n], b[o:o + n]), (where, "pool")


def _recon(clip, blobs, want):
    """accepted pictures through the descriptor spec, in the player's rotation; a refused picture leaves the oracle's content in its
    buffer, so that every accepted picture is compared whatever it references"""
    from oracle import bridge
    o = bridge.oracle()
    o.hvqd_recon.restype = C.c_int
    o.hvqd_recon.argtypes = [C.c_void_p] * 4 + [C.c_uint32]
    ps = clip.picsize
    slot = ps + 64
    bufs = [np.zeros(slot, dtype=np.uint8) for _ in range(3)]        # past, present, future
    for k, (ft, blob) in enumerate(zip(clip.kinds, blobs)):
        if ft != B_FRAME:
            bufs[0], bufs[2] = bufs[2], bufs[0]
        if blob is None:
            bufs[1][:ps] = want[k]
        else:
            ref1 = bufs[1] if ft == P_FRAME else bufs[2]
            assert o.hvqd_recon(blob.ctypes.data, bufs[1].ctypes.data, bufs[0].ctypes.data, ref1.ctypes.data, slot) == 0
            assert np.array_equal(bufs[1][:ps], want[k]), (k, hex(ft))
        if ft != B_FRAME:
            bufs[1], bufs[2] = bufs[2], bufs[1]


@pytest.mark.parametrize("case", CRAFTED, ids=lambda c: c[0])
def test_crafted_malformed_pictures_three_ways(emul, case):
    from hvqm4_amd.synth import make_clip
    from oracle import bridge
    name, cfg = case
    clip = make_clip(cfg)
    want = bridge.oracle_decode(clip.data, clip.n_pictures)
    h1, h4 = _Host(clip, 1), _Host(clip, 4)
    cap = h1.bound
    blobs, refused, taint = [], [], False
    try:
        for k, (ft, pic) in enumerate(zip(clip.kinds, clip.pictures)):
            where = f"{name} picture {k} type {ft:#x}"
            rc1, f1, b1 = h1.parse(ft, pic)
            rc4, f4, b4 = h4.parse(ft, pic)
            verdict = _verdict(rc1 == 0, f1)
            assert verdict == _verdict(rc4 == 0, f4), where
            for mode in (CHAINS, FLAT):
                res, bd = _device(emul, clip, ft, pic, mode, cap)
                assert _verdict(res.status == 0, res.flags) == verdict, (where, mode, hex(res.flags), hex(f1))
                if verdict == "ok":
                    assert res.flags == f1, where
                    _same_blob(b1, bd, where)
            assert verdict in ("ok", "malformed"), where
            if verdict == "ok":
                assert np.array_equal(b1, b4), where
            refused.append(verdict != "ok")
            blobs.append(b1 if verdict == "ok" else None)
    finally:
        h1.close(); h4.close()
    assert any(refused) and not all(refused), refused
    assert not any(r for r, ft in zip(refused, clip.kinds) if ft == I_FRAME)
    _recon(clip, blobs, want)
    if bridge.have_ref() and not (cfg.mb_type3 and 1 in cfg.mb_type3_exits):
        # the oracle against the live reference on the accepted pictures that reference no refused one (a refused P picture decodes
        # differently in the two: what the reference reads there is not in the stream).  A type-3 run left through bit 1 puts the
        # reference out of step with the stream (mcbtypetrans[1][3] lies past its table): those clips are not run through it
        got = bridge.ref_decode(clip.data, clip.n_pictures)[0]
        for k, ft in enumerate(clip.kinds):
            if ft == I_FRAME:
                taint = False
            if refused[k]:
                taint = taint or ft != B_FRAME
                continue
            if not taint:
                assert np.array_equal(got[k], want[k]), (name, k)


def _mutate(rng, pic, v):
    q = bytearray(pic)
    if v % 3 == 0:
        for _ in range(int(rng.integers(1, 25))):
            q[int(rng.integers(0x50, len(q)))] = int(rng.integers(0, 256))
    elif v % 3 == 1:
        for _ in range(int(rng.integers(1, 12))):
            q[int(rng.integers(8, len(q)))] ^= 1 << int(rng.integers(0, 8))
    else:
        q = q[:int(rng.integers(0x60, len(q)))]
    return bytes(q)


def test_host_and_device_parsers_agree_on_mutated_pictures(emul):
    """byte overwrites, bit flips and truncations of P/B pictures of four geometries and presets: the host parser and the GPU parse
    core must agree on the verdict and, where neither raised a flag, on the whole blob.  By design the device parser stops long
    overflow runs at its cap (HVQ_F_CAPPED) where the host parser follows them; hvq_flush_end then parses the picture again on the
    host, so a picture capped on the device side alone takes the host's verdict."""
    from hvqm4_amd.synth import SynthConfig, make_clip
    rng = np.random.default_rng(23)
    total = compared = malformed = 0
    for seed, (w, h, samp, preset) in enumerate([(64, 48, "420", "dense"), (96, 64, "422", "natural"), (48, 80, "444", "realistic"),
                                                 (160, 96, "420", "flat")]):
        clip = make_clip(SynthConfig(width=w, height=h, gop="IPBB", seed=seed + 31, preset=preset, sampling=samp))
        host = _Host(clip, 1)
        try:
            for ft, pic in zip(clip.kinds, clip.pictures):
                if ft == I_FRAME:
                    continue
                for v in range(36):
                    q = _mutate(rng, pic, v)
                    rc, fl, blob = host.parse(ft, q)
                    hv = _verdict(rc == 0, fl)
                    res, bd = _device(emul, clip, ft, q, FLAT, host.bound)
                    dv = _verdict(res.status == 0, res.flags)
                    total += 1
                    malformed += hv == "malformed"
                    where = (seed, hex(ft), v, hex(fl), hex(res.flags), rc, int(res.status))
                    if dv == "capped" and hv != "capped":
                        continue
                    if res.status & 2:                      # GP_ST_BADTREE: the host parser refuses such a tree as malformed
                        assert hv == "malformed", where
                        continue
                    assert hv == dv, where
                    if hv == "ok":
                        assert res.flags == fl
                        _same_blob(blob, bd, (seed, hex(ft), v))
                        compared += 1
        finally:
            host.close()
    assert total == 4 * 3 * 36 and compared > total // 4 and malformed > 0


def _records(clip, path):
    with open(path, "wb") as f:
        for ft, pic in zip(clip.kinds, clip.pictures):
            f.write(struct.pack("<II", ft, len(pic)) + pic)


def test_parsers_stay_in_bounds_on_mutated_pictures_under_sanitizers(tmp_path):
    """The host parser with 1 and 4 threads, and the GPU parse core (chains and flat path), built with AddressSanitizer and UBSan, on
    mutated P/B pictures of three geometries and samplings: 1..24 byte overwrites behind offset 0x50, bit flips, truncations, fixed
    seeds.  Any read outside an allocation or undefined behaviour ends the run; the thread counts must agree on every verdict."""
    from hvqm4_amd.synth import SynthConfig, make_clip
    exe = tmp_path / "parse_fuzz_asan"
    subprocess.check_call(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-sanitize=shift",
                           "-fno-omit-frame-pointer", "-Wall",
                           os.path.join(ROOT, "tests", "native", "parse_fuzz_asan.c"), os.path.join(ROOT, "tests", "native", "gparse_emul.c"),
                           os.path.join(ROOT, "hvqm4_amd", "csrc", "hvq_parse.c"), "-lpthread", "-o", str(exe)])
    runs = [(SynthConfig(width=64, height=48, gop="IPBP", seed=3), 12000),
            (SynthConfig(width=64, height=48, gop="IPBP", seed=3, version="1.3", sampling="422"), 5000),
            (SynthConfig(width=48, height=40, gop="IPBB", seed=7, sampling="444", preset="natural"), 5000),
            (SynthConfig(width=96, height=32, gop="IPPB", seed=9, preset="realistic"), 4000)]
    for k, (cfg, rounds) in enumerate(runs):
        clip = make_clip(cfg)
        rec = tmp_path / f"pics{k}.bin"
        _records(clip, rec)
        r = subprocess.run([str(exe), str(clip.width), str(clip.height), str(clip.samp_h), str(clip.samp_v),
                            "1" if clip.version == "1.5" else "0", str(rounds), str(k + 1), str(rec)],
                           capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
        assert r.returncode == 0, (k, (r.stdout + r.stderr)[-4000:])
        assert "fuzz ok" in r.stdout
