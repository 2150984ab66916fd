"""CPU: mutated pictures against a CHECKED oracle -- the contract of DESIGN.md 8 f4 (refuse, never decode differently) measured
against the reference's behaviour instead of product against product.

The checked oracle (oracle/hvq_oracle_chk.c: the oracle's own code with every input-controlled access behind a guard) gives every
picture a class: `defined`, or why the reference would leave its own memory or never return (mem, map, empty, tree, hang, rules).
Per mutant the host parser (1 and 4 threads) and the GPU parse core (tests/native/gparse_emul.c, chains and flat path) give their
verdicts, and:
* all four agree (a picture capped on the device side alone takes the host's verdict: hvq_flush_end parses it again on the host;
  a picture whose payload exceeds the blob bound is an error, HVQ_E_OVERFLOW, in all four -- a limit, not a different decode);
* accepted => the class is `defined`, and the blob through the descriptor spec (oracle/hvq_desc_recon.c) with the clean clip's
  references equals the checked oracle's picture byte for byte; where oracle/_ref is built, the picture also goes through the
  compiled reference (a child process per clip, stopping at its first failure; only `defined` pictures are ever run) and equals it;
* refused => the class is not `defined` and the flag says why: mem, map, empty -> HVQ_F_CLAMPED; hang -> HVQ_F_CAPPED;
  tree, rules -> HVQ_F_MALFORMED.  The rule is exact in both parsers (hvq_refuse.h: used bases only), so nothing is over-refused.

Corpus (fixed seeds): seven clips -- 4:2:0, 4:2:2, 4:4:4, versions 1.3 and 1.5, a portrait clip, a p_future_refs clip; 112 mutants
per P/B picture and 48 per I picture: byte overwrites, bit flips (three parts in eight each), truncations and one section size
zeroed in the offset table (one part each).  Counts of the frozen corpus, from the checked oracle on the CPU (the
test asserts the bounds): 3024 mutants; 1106 `defined`, of which 1100 accepted and compared (36 %; bound: more than a quarter) and
6 beyond the blob bound; 766 `mem` (25 %; bound: more than a tenth), 708 `empty`, 77 `hang`, 339 `rules`, 28 `tree`; 32 `defined`
pictures read bits past their end and 503 contain a cross-plane read (bounds: 20 each); 1099 went through the compiled reference.
On the parent commit the `mem` and `empty` pictures were accepted and decoded with invented content."""
import ctypes as C
import multiprocessing
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.test_gparse_emul import CHAINS, FLAT, emul  # noqa: F401  (emul: the fixture)
from tests.test_malformed_pb import B_FRAME, I_FRAME, P_FRAME, REFUSE, ROOT, _Host, _device, _mutate, _same_blob, _verdict

PER_PB, PER_I = 112, 48
FLAG_OF_CLASS = {"mem": "clamped", "map": "clamped", "empty": "clamped", "hang": "capped", "tree": "malformed", "rules": "malformed"}


def corpus_configs():
    from hvqm4_amd.synth import SynthConfig
    return [("dense420_15", SynthConfig(width=64, height=48, gop="IPBB", seed=31, preset="dense", sampling="420", version="1.5")),
            ("natural422_13", SynthConfig(width=96, height=64, gop="IPBB", seed=32, preset="natural", sampling="422", version="1.3")),
            ("portrait444_15", SynthConfig(width=48, height=80, gop="IPBB", seed=33, preset="realistic", sampling="444", version="1.5")),
            ("flat420_13", SynthConfig(width=160, height=96, gop="IPBB", seed=34, preset="flat", sampling="420", version="1.3")),
            ("pselfref420_15", SynthConfig(width=64, height=48, gop="IPBBPBPP", seed=36, p_future_refs=True)),
            ("natural444_13", SynthConfig(width=80, height=64, gop="IPBP", seed=37, sampling="444", version="1.3", preset="natural")),
            ("plain422_15", SynthConfig(width=64, height=64, gop="IPB", seed=38, sampling="422", version="1.5"))]


CONFIGS = corpus_configs()


def mutate(rng, pic, v, ft):
    """v % 8: 0-2 byte overwrites, 3-5 bit flips, 6 truncation (tests/test_malformed_pb.py _mutate), 7 one section size zeroed --
    or, every fourth time, the head of the DC section overwritten with a one-leaf tree of the escape value"""
    m = v % 8
    if m == 7:
        q = bytearray(pic)
        data = 8 + (0x40 if ft == I_FRAME else 0x44)
        if v % 32 == 31:                                     # the DC tree replaced by ONE leaf, the escape value 0x7F: a run without end
            off = data + int.from_bytes(q[8 + 4 * 4:12 + 4 * 4], "big") + 4
            q[off:off + 2] = b"\x3f\x80"
            return bytes(q)
        i = int(rng.integers(0, 16 if ft == I_FRAME else 17))
        off = data + int.from_bytes(q[8 + 4 * i:12 + 4 * i], "big")
        if off + 4 <= len(q):
            q[off:off + 4] = b"\0\0\0\0"
        return bytes(q)
    return _mutate(rng, pic, 0 if m < 3 else (1 if m < 6 else 2))


def mutants_of(clip, seed):
    """[(k, frame type, [mutants])] for every picture of the clip, fixed by `seed`"""
    rng = np.random.default_rng(seed)
    return [(k, ft, [mutate(rng, pic, v, ft) for v in range(PER_I if ft == I_FRAME else PER_PB)])
            for k, (ft, pic) in enumerate(zip(clip.kinds, clip.pictures))]


def player_for(clip):
    from oracle import bridge
    return bridge.CheckedPlayer(clip.width, clip.height, clip.samp_h, clip.samp_v, clip.version == "1.5")


def _recon_one(clip, ft, blob, refs):
    """the blob through the descriptor spec with the clean clip's references -> picture"""
    from oracle import bridge
    o = bridge.oracle()
    o.hvqd_recon.restype = C.c_int
    o.hvqd_recon.argtypes = [C.c_void_p] * 4 + [C.c_uint32]
    ps = clip.picsize
    slot = ps + 64
    past, present, future = (np.concatenate([b, np.zeros(64, dtype=np.uint8)]) for b in refs)
    ref1 = present if ft == P_FRAME else future
    assert o.hvqd_recon(blob.ctypes.data, present.ctypes.data, past.ctypes.data, ref1.ctypes.data, slot) == 0
    return present[:ps]


def container(clip, kinds, pics, pad):
    """an .h4m of one block with these pictures; `pad` zero bytes behind the last one (bits past a picture's end read as zero)"""
    frames = bytearray()
    biggest = 0
    for n, (ft, pic) in enumerate(zip(kinds, pics)):
        payload = struct.pack(">I", n) + pic + (b"\0" * pad if n == len(pics) - 1 else b"")
        frames += struct.pack(">HHI", 1, ft, len(payload)) + payload
        biggest = max(biggest, len(payload))
    body = struct.pack(">IIIII", 0, len(frames), len(pics), 0, 0x01000000) + bytes(frames)
    hdr = clip.data[:16] + struct.pack(">IIIIIIIII", 0x44, len(body), 1, len(pics), 0, 33366, biggest, 0, 0) + clip.data[0x34:0x44]
    assert len(hdr) == 0x44
    return hdr + body


REF_PAD = 4096


def _ref_child(conn, clip, jobs):
    """in a child process: every job (k, mutant, want) through the compiled reference, behind the clean pictures 0..k-1"""
    from oracle import bridge
    try:
        for n, (k, q, want) in enumerate(jobs):
            conn.send(("at", n, k))
            data = container(clip, clip.kinds[:k + 1], clip.pictures[:k] + [q], REF_PAD)
            got = bridge.ref_decode(data, k + 1)[0][k]
            if not np.array_equal(got, want):
                conn.send(("differs", n, k))
                return
        conn.send(("ok", len(jobs), -1))
    except Exception as e:                                   # noqa: BLE001
        conn.send(("error", repr(e), -1))


def _through_reference(name, clip, jobs):
    ctx = multiprocessing.get_context("spawn")               # a fresh process: the GPU suite calls this with a device open
    a, b = ctx.Pipe()
    p = ctx.Process(target=_ref_child, args=(b, clip, jobs))
    p.start()
    b.close()
    msg = ("started", -1, -1)
    try:
        while msg[0] in ("started", "at"):                   # the last "at" names the job a crashed child died in
            msg = a.recv() if a.poll(600) else ("timeout",) + msg[1:]
    except EOFError:
        msg = ("died in job",) + msg[1:] + (jobs[msg[1]][0] if msg[1] >= 0 else None,)
    p.join(10)
    if p.is_alive():
        p.kill()
    assert p.exitcode == 0 and msg[0] == "ok", (name, msg, p.exitcode)


class Tally:
    def __init__(self):
        self.total = self.accepted = self.errors = self.dev_capped_only = self.past = self.cross = self.ref_run = 0
        self.classes = {}


def check_clip(emul, name, clip, seed, tally):
    """the three assertions of the module docstring over every mutant of one clip"""
    from oracle import bridge
    h1, h4 = _Host(clip, 1), _Host(clip, 4)
    pl = player_for(clip)
    ref_jobs = []
    try:
        for k, ft, muts in mutants_of(clip, seed):
            for v, q in enumerate(muts):
                where = (name, k, hex(ft), v)
                cls, rep, want = pl.check(ft, q)
                cname = bridge.class_name(cls)
                rc1, f1, b1 = h1.parse(ft, q)
                rc4, f4, b4 = h4.parse(ft, q)
                hv = _verdict(rc1 == 0, f1)
                assert hv == _verdict(rc4 == 0, f4), (where, hex(f1), hex(f4))
                if hv == "ok":
                    assert np.array_equal(b1, b4), where
                for mode in (CHAINS, FLAT):
                    res, bd = _device(emul, clip, ft, q, mode, h1.bound)
                    dv = _verdict(res.status == 0, res.flags)
                    if res.status & 2:                      # GP_ST_BADTREE: the host parser refuses such a tree as malformed
                        assert hv == "malformed", (where, mode)
                        continue
                    if dv == "capped" and hv != "capped":   # the device's cap: the runtime parses the picture again on the host
                        tally.dev_capped_only += 1
                        continue
                    assert dv == hv, (where, mode, cname, hex(res.flags), hex(f1), int(res.status), rc1)
                    if hv == "ok":
                        assert res.flags == f1, (where, mode)
                        _same_blob(b1, bd, (where, mode))
                tally.total += 1
                tally.classes[cname] = tally.classes.get(cname, 0) + 1
                if hv == "error":
                    tally.errors += 1
                elif hv == "ok":
                    assert cls == 0, (where, "accepted, but the reference", cname)
                    got = _recon_one(clip, ft, b1, pl.refs(ft))
                    assert np.array_equal(got, want), (where, "differs from the checked oracle")
                    tally.accepted += 1
                    tally.past += rep.past_bits > 0
                    tally.cross += rep.cross > 0
                    if rep.past_bits <= 8 * (REF_PAD - 64):
                        ref_jobs.append((k, q, want))
                else:
                    assert cls != 0, (where, "refused as", hv, "but the reference decodes it inside its own buffers")
                    assert FLAG_OF_CLASS[cname] == hv, (where, cname, hv)
            pl.advance(ft, clip.pictures[k])
            for h in (h1, h4):                              # the stream's own picture last: its nest is what later P/B pictures use
                rc, fl, _ = h.parse(ft, clip.pictures[k])
                assert rc == 0 and not fl & REFUSE, (name, k)
    finally:
        h1.close(); h4.close(); pl.close()
    if bridge.have_ref() and ref_jobs:
        _through_reference(name, clip, ref_jobs)
        tally.ref_run += len(ref_jobs)


def test_mutants_agree_and_match_the_checked_oracle(emul):
    from hvqm4_amd.synth import make_clip
    t = Tally()
    for n, (name, cfg) in enumerate(CONFIGS):
        check_clip(emul, name, make_clip(cfg), 500 + n, t)
    print("corpus:", t.total, "accepted", t.accepted, "classes", t.classes, "errors", t.errors, "device-only capped", t.dev_capped_only,
          "past-the-end", t.past, "cross-plane", t.cross, "through the reference", t.ref_run)
    # the conditions that keep this test from hiding failures
    assert t.total == 3024
    assert t.accepted > t.total // 4
    assert t.classes.get("mem", 0) > t.total // 10
    for c in ("empty", "hang", "rules"):
        assert t.classes.get(c, 0) >= 1, c
    assert t.past >= 20 and t.cross >= 20
    assert t.errors <= t.total // 100


def test_checked_oracle_equals_the_oracle_on_every_catalogue_clip():
    """legal streams are `defined` and decode to the same pictures: tests/clips.py SMALL, REGRESSION and the nest_border clips"""
    from oracle import bridge
    from tests import clips
    for nc in clips.SMALL + clips.REGRESSION + [c for c in clips.MEDIUM if c[0].startswith("nest_border")]:
        clip = clips.get(nc)
        want = bridge.oracle_decode(clip.data, clip.n_pictures)
        pl = player_for(clip)
        try:
            for k, (ft, pic) in enumerate(zip(clip.kinds, clip.pictures)):
                assert np.array_equal(pl.advance(ft, pic), want[k]), (nc[0], k)
        finally:
            pl.close()


def test_legal_random_clips_are_defined_and_never_refused(emul):
    """no over-refusal: 150 clips drawn like tools/parity_sweep.py (geometry, version, sampling, preset, GOP, run-off) -- every
    picture is `defined` and neither parser raises a refusal flag (500 clips of the same draw, 3444 pictures: none either)"""
    from hvqm4_amd.synth import make_clip
    from tools.parity_sweep import draw
    rng = np.random.default_rng(12345)
    pictures = 0
    for i in range(150):
        clip = make_clip(draw(rng))
        pl, h = player_for(clip), _Host(clip, 1)
        try:
            for k, (ft, pic) in enumerate(zip(clip.kinds, clip.pictures)):
                cls, _rep, _out = pl.check(ft, pic)
                rc, fl, _b = h.parse(ft, pic)
                res, _bd = _device(emul, clip, ft, pic, FLAT, h.bound)
                assert cls == 0 and rc == 0 and not fl & REFUSE and res.status == 0 and not res.flags & REFUSE, (i, k, cls, rc, hex(fl), hex(res.flags))
                pl.advance(ft, pic)
                pictures += 1
        finally:
            pl.close(); h.close()
    assert pictures > 800


def test_checked_oracle_under_sanitizers(tmp_path):
    """the guard list is complete: the checked oracle built with AddressSanitizer and UBSan, picture and picture buffers exactly
    sized heap allocations, over the whole corpus -- no report, and a class for every picture, the same the library gives"""
    from hvqm4_amd.synth import make_clip
    exe = tmp_path / "oracle_chk_asan"
    subprocess.check_call(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-sanitize=shift",
                           "-fno-omit-frame-pointer", "-Wall", os.path.join(ROOT, "tests", "native", "oracle_chk_asan.c"),
                           os.path.join(ROOT, "oracle", "hvq_oracle_chk.c"), "-o", str(exe)])
    for n, (name, cfg) in enumerate(CONFIGS):
        clip = make_clip(cfg)
        rec = tmp_path / f"corpus{n}.bin"
        want = []
        pl = player_for(clip)
        with open(rec, "wb") as f:
            for k, ft, muts in mutants_of(clip, 500 + n):
                for q in muts:
                    f.write(struct.pack("<III", ft, len(q), 1) + q)
                    cls, rep, _ = pl.check(ft, q)
                    want.append((cls, rep.past_bits, rep.cross))
                f.write(struct.pack("<III", ft, len(clip.pictures[k]), 0) + clip.pictures[k])
                pl.advance(ft, clip.pictures[k])
        pl.close()
        r = subprocess.run([str(exe), str(clip.width), str(clip.height), str(clip.samp_h), str(clip.samp_v),
                            "1" if clip.version == "1.5" else "0", str(rec)], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
        assert r.returncode == 0, (name, (r.stdout + r.stderr)[-4000:])
        lines = r.stdout.strip().split("\n")
        assert lines[-1] == f"oracle ok: {len(want)} mutants", lines[-1]
        got = [tuple(int(x) for x in ln.split()[1:]) for ln in lines[:-1]]
        assert got == want, name
