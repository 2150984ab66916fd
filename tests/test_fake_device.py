"""The runtime (hvqm4_amd/csrc/hvq_runtime.cpp: every pointer, table, launch shape, buffer lifetime and stream or event edge the kernels
depend on) linked UNCHANGED against a CPU fake device and driven through include/hvqm4_amd.h -- no GPU.

  tests/native/fakehip/hip/hip_runtime.h, fake_device.cpp   the HIP calls the runtime uses: memory is the host heap (one malloc per
      allocation, a registry behind fake_span), streams are FIFOs under one of two schedules (FAKEHIP_SCHEDULE): `eager` runs every
      operation at the call, `late` runs nothing until the host observes it -- a GPU as far behind as HIP allows, under which a
      dependency that holds only because the GPU is usually fast fails;
  tests/native/fake_kernels.cpp    the hvq_launch_* entry points: reconstruction through the scalar descriptor interpreter
      (oracle/hvq_desc_recon.c) walking the launch's grid, the parse through the GPU parse core (tests/native/gparse_emul.c), the small
      kernels restated, the colour / filter kernels as footprint checks plus a log of what their sources held when they ran;
  tests/native/fake_driver.cpp     the scenarios; it writes what it read back and judges nothing.

Every scenario runs under both schedules in two builds (plain, and AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone
program).  Passing: exit status 0, no sanitizer report, no fake_span abort, every picture byte-identical to the oracle's, every export
launch saw the oracle's pictures in its sources, nothing asked for is missing.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests.test_recon_plan import L, plan  # noqa: F401 -- L is the fixture: the library with hvq_recon_inline_plan declared

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NATIVE = os.path.join(HERE, "native")
BUILD = os.path.join(NATIVE, "_build")
GOLDEN = os.path.join(HERE, "golden")
CSRC = os.path.join(ROOT, "hvqm4_amd", "csrc")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))
CLIPS = {name: c for name, c in MANIFEST["clips"].items() if "file" in c}

C_SOURCES = [os.path.join(CSRC, "hvq_parse.c"), os.path.join(CSRC, "hvq_container.c"), os.path.join(NATIVE, "gparse_emul.c"),
             os.path.join(ROOT, "oracle", "hvq_desc_recon.c")]
CXX_SOURCES = [os.path.join(CSRC, "hvq_runtime.cpp"), os.path.join(NATIVE, "fake_device.cpp"), os.path.join(NATIVE, "fake_kernels.cpp"),
               os.path.join(NATIVE, "fake_helpers.cpp"), os.path.join(NATIVE, "fake_driver.cpp")]
# -ffp-contract=off: the runtime's `#pragma clang fp contract(off)` (resample tables) is unknown to g++
COMMON = ["-O1", "-g", "-march=x86-64-v3", "-ffp-contract=off", "-pthread", "-I" + os.path.join(NATIVE, "fakehip"), "-I" + NATIVE, "-I" + CSRC]
# the sanitizers' runtimes linked statically: the program starts whatever else the environment loads in front of it
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"]
BUILDS = {"plain": [], "sanitizer": SANITIZE}

SEVEN = ["gop64x48_15", "yuv422_296x160", "yuv444_13_portrait48x64", "ragged24x40", "wide296x160", "yuv444_64x48", "ip8"]
INTERLEAVED = ["wide296x160", "ip8", "literals96x96", "yuv444_13_portrait48x64", "pselfref422_64x48"]
STREAMING = ["gop64x48_15", "yuv422_64x48", "ragged24x40", "weird64x64", "yuv444_64x48", "ipb32", "portrait48x64", "gop64x48_13",
             "literals96x96", "ip8", "bigshift64x48", "yuv422_13_portrait48x64"]

# (id, driver scenario, environment)
SCENARIOS = [
    ("clips0", "clips0", {}), ("clips1", "clips1", {}),
    ("seven", "seven", {}), ("seven_history", "seven_history", {}),
    ("interleaved_tpw1", "interleaved", {"HVQM4_AMD_TILES_PER_WG": "1"}),
    ("interleaved_tpw2", "interleaved", {"HVQM4_AMD_TILES_PER_WG": "2"}),
    ("interleaved_queues2", "interleaved", {"HVQM4_AMD_QUEUES": "2"}),
    ("lifecycle", "lifecycle", {}), ("streaming", "streaming", {}), ("dropped", "dropped", {}),
]


def build_driver(kind, tag, exe_name, cxx_sources, test_file):
    """The stand-alone driver `exe_name` of build `kind` (a key of BUILDS) from C_SOURCES and `cxx_sources`, in BUILD/<tag>_<kind>; built
    again when a source, a header or one of the two test files (this one, and `test_file` of the test that asks) is newer"""
    out = os.path.join(BUILD, tag + "_" + kind)
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, exe_name)
    flags = COMMON + BUILDS[kind]
    dirs = (CSRC, NATIVE, os.path.join(NATIVE, "fakehip", "hip"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "include"))
    deps = C_SOURCES + cxx_sources + [os.path.join(d, f) for d in dirs for f in os.listdir(d) if f.endswith(".h")]
    if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps + [test_file, __file__]):
        return exe
    jobs, objs = [], []
    for src in C_SOURCES + cxx_sources:
        obj = os.path.join(out, os.path.basename(src) + ".o")
        objs.append(obj)
        cc = ["g++", "-std=c++17"] if src.endswith(".cpp") else ["gcc"]
        jobs.append((src, subprocess.Popen(cc + flags + ["-c", src, "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for src, p in jobs:
        log = p.communicate()[0]
        assert p.returncode == 0, f"{src} ({kind}):\n{log}"
    subprocess.run(["g++"] + flags + objs + ["-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def drivers():
    return {kind: build_driver(kind, "fake", "fake_driver", CXX_SOURCES, __file__) for kind in BUILDS}


_oracle, _hash = {}, {}


def oracle_pictures(name):
    if name not in _oracle:
        from oracle import bridge
        data = open(os.path.join(GOLDEN, CLIPS[name]["file"]), "rb").read()
        _oracle[name] = bridge.oracle_decode(data, len(CLIPS[name]["frame_types"]))
    return _oracle[name]


def fnv1a64(data):
    h = 0xcbf29ce484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def oracle_hash(name, k):
    if (name, k) not in _hash:
        _hash[name, k] = fnv1a64(oracle_pictures(name)[k].tobytes())
    return _hash[name, k]


def corrupted_p_picture():
    """the P picture of ipb32, cut short by the recipe of tests/corrupt_hashes.py (its variant 1: truncation at a random length)"""
    from hvqm4_amd.container import video_pictures
    data = open(os.path.join(GOLDEN, CLIPS["ipb32"]["file"]), "rb").read()
    pics = [(ft, bytes(p)) for ft, _d, p in video_pictures(data)]
    assert pics[1][0] == 0x20
    rng = np.random.default_rng(17)
    q = bytearray(pics[1][1])
    return bytes(q[:int(rng.integers(0x60, len(q)))])


def run_driver(exe, scenario, env_extra, schedule, tmp_path):
    out = tmp_path / "out"
    out.mkdir()
    args = [exe, scenario, str(out), GOLDEN]
    if scenario == "dropped":
        bad = tmp_path / "corrupt.bin"
        bad.write_bytes(corrupted_p_picture())
        args.append(str(bad))
    env = dict(os.environ, FAKEHIP_SCHEDULE=schedule, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1", **env_extra)
    r = subprocess.run(args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    return r, out


def run_checked(exe, scenario, schedule, tmp_path, extra=(), inputs=None, timeout=600):
    """One scenario of a stand-alone driver under `schedule`: `inputs` (name -> text or bytes) are written into the out directory first,
    `extra` follows the golden directory on the command line.  Passing: no sanitizer report, no fake_span abort, exit status 0.
    -> (the out directory, the lines of results.txt)"""
    out = tmp_path / "out"
    out.mkdir()
    for name, data in (inputs or {}).items():
        (out / name).write_bytes(data) if isinstance(data, bytes) else (out / name).write_text(data)
    env = dict(os.environ, FAKEHIP_SCHEDULE=schedule, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, scenario, str(out), GOLDEN] + [str(x) for x in extra], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=timeout)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "fake_span" not in r.stderr and "fakehip:" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    return out, open(out / "results.txt").read().splitlines()


def refusal_texts(lines):
    """the E lines of a `refused` scenario: label -> the library's words, which run to the end of the line"""
    return {f[1]: (f[2] if len(f) > 2 else "") for f in (line.split(" ", 2) for line in lines) if f[0] == "E"}


def n_pics(name):
    return len(CLIPS[name]["frame_types"])


def expected(scenario, seen_clips):
    """(pictures read back, pictures not resident, export sources) the driver must report: multisets of (clip, ordinal, label)"""
    P, N, E = [], [], []

    def whole(names, label, into):
        for nm in names:
            into.extend((nm, k, label) for k in range(n_pics(nm)))

    if scenario.startswith("clips"):
        whole(seen_clips, "clips/host", P); whole(seen_clips, "clips/device", P)
    elif scenario == "seven":
        whole(SEVEN, "seven", P); whole(SEVEN, "seven", E)
    elif scenario == "seven_history":
        whole(SEVEN, "seven/history", P); whole(SEVEN, "seven/history", E)
        for _ in range(3):
            whole(CLIPS, "seven/history", E)
    elif scenario == "interleaved":
        whole(INTERLEAVED, "interleaved/host", P); whole(INTERLEAVED, "interleaved/device", P)
    elif scenario == "lifecycle":
        whole(["ragged24x40"], "lifecycle/close", P); whole(["yuv422_64x48", "yuv444_64x48"], "lifecycle/second", P)
        whole(["gop64x48_15"], "lifecycle/reuse", P)
        whole(["ragged24x40", "gop64x48_15"], "lifecycle/close", E); whole(["gop64x48_15"], "lifecycle/reuse", E)
        whole(["yuv444_64x48"], "lifecycle/destroy", E)
    elif scenario == "streaming":
        whole(STREAMING, "streaming", P)
    elif scenario == "dropped":
        whole(["gop64x48_15", "yuv444_64x48"], "dropped", P)
        P.append(("ipb32", 0, "dropped"))
        N.extend(("ipb32", k, "dropped") for k in range(1, n_pics("ipb32")))
    return sorted(P), sorted(N), sorted(E)


def check_run(r, out, scenario):
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "fake_span" not in r.stderr and "fakehip:" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    pictures = np.fromfile(out / "pictures.bin", dtype=np.uint8)
    P, N, E, R, X = [], [], [], {}, None
    for line in open(out / "results.txt").read().splitlines():
        f = line.split()
        if f[0] == "P":
            name, k, off, n, h, label = f[1], int(f[2]), int(f[3]), int(f[4]), int(f[5], 16), f[6]
            want = oracle_pictures(name)[k]
            got = pictures[off:off + n]
            assert got.size == want.size and np.array_equal(got, want), \
                f"{label}: picture {k} of {name} differs from the oracle in {int((got != want).sum()) if got.size == want.size else -1} bytes"
            if n <= 4096:
                assert h == fnv1a64(got), "the driver's hash is not FNV-1a-64"
            P.append((name, k, label))
        elif f[0] == "N":
            N.append((f[1], int(f[2]), f[3]))
        elif f[0] == "E":
            name, k, h, label = f[1], int(f[2]), int(f[3], 16), f[4]
            assert name in CLIPS, line
            assert h == oracle_hash(name, k), f"{label}: the export read picture {k} of {name} while it did not hold the oracle's picture"
            E.append((name, k, label))
        elif f[0] == "R":
            R[f[1]] = int(f[2])
        elif f[0] == "X":
            X = (int(f[1]), int(f[2]))
    seen = sorted({name for name, _k, _l in P})
    wantP, wantN, wantE = expected(scenario, seen)
    assert sorted(P) == wantP and sorted(N) == wantN and sorted(E) == wantE
    assert X is not None and X[0] == X[1] == len(wantE)
    if scenario == "dropped":
        assert R["dropped/flush"] < 0, "the flush must report the corrupted picture"
    return seen


_clips_seen = {}


@pytest.mark.parametrize("schedule", ["eager", "late"])
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("case", SCENARIOS, ids=[s[0] for s in SCENARIOS])
def test_scenario(drivers, case, build, schedule, tmp_path):
    _id, scenario, env = case
    r, out = run_driver(drivers[build], scenario, env, schedule, tmp_path)
    seen = check_run(r, out, scenario)
    if scenario.startswith("clips"):
        _clips_seen[scenario] = seen


def test_the_clips_scenarios_cover_every_clip_of_the_manifest(drivers, tmp_path):
    for i, scenario in enumerate(("clips0", "clips1")):
        if scenario not in _clips_seen:
            d = tmp_path / str(i)
            d.mkdir()
            r, out = run_driver(drivers["plain"], scenario, {}, "late", d)
            _clips_seen[scenario] = check_run(r, out, scenario)
    assert sorted(_clips_seen["clips0"] + _clips_seen["clips1"]) == sorted(CLIPS)


def test_flush_timing_lines_say_what_the_plan_says(drivers, L, tmp_path):
    """tests/test_gpu_shapes.py reads which instantiation a launch took off the runtime's HVQM4_AMD_FLUSH_TIMING lines.  Pinned here without
    a GPU: the `seven` scenario flushes seven golden clips one after the other, so flush k holds one launch per dependency level of clip k
    (coverage.levels) -- every line must match the expression that test imports and say what hvq_recon_inline_plan says for the fullest
    tile of the level's blob headers."""
    from tests import clips, coverage
    from tests.gpu_kit import launch_lines
    r, out = run_driver(drivers["plain"], "seven", {"HVQM4_AMD_FLUSH_TIMING": "1"}, "eager", tmp_path)
    check_run(r, out, "seven")
    flushes, lines = [], []
    for line in r.stderr.splitlines():
        lines.append(line)
        if line.startswith("flush_end "):
            flushes.append(launch_lines("\n".join(lines)))
            lines = []
    assert len(flushes) == len(SEVEN)
    small = dict(clips.SMALL)
    for name, got in zip(SEVEN, flushes):
        clip = clips.get((name, small[name]))
        pics, lv = coverage.launch_inputs(clip), coverage.levels(clip.kinds)
        want = []
        for level in sorted(set(lv)):
            mi = max(p[1] for p, l in zip(pics, lv) if l == level)
            mp = max(p[2] for p, l in zip(pics, lv) if l == level)
            p = plan(L, mi, mp)
            want.append(dict(launch=len(want), level=level, queue=0, max_items=mi, max_pairs=mp, tpw=p["tpw"], items=p["items"], pairs=p["pairs"],
                             pool=p["pool"], lds=p["lds"], workgroups=L.hvq_recon_inline_residency(p["tpw"], p["items"], p["lds"])))
        assert got == want, name


def test_fake_helpers_equal_the_librarys():
    """The LDS and scratch sizing helpers the runtime imports from the HIP units, restated in tests/native/fake_helpers.cpp, against the real
    library (it loads without a GPU) over the whole grid of shapes: the two cannot drift.  Not compared: hvq_gparse_scratch_bytes, which
    the library does not export -- there and in the fake it is one call of gp_scratch_bytes of the shared header hvq_gparse_core.h, so
    there is nothing to drift; hvq_parse_occupancy, which asks the HIP runtime about a device and feeds a diagnostic line only."""
    from hvqm4_amd._lib import lib
    real = lib()
    so = os.path.join(BUILD, "libfake_helpers.so")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-shared", "-fPIC"] + COMMON + [os.path.join(NATIVE, "fake_helpers.cpp"), "-o", so], check=True)
    fake = C.CDLL(so)
    for l in (real, fake):
        for fn, nargs in (("hvq_recon_inline_static_lds", 2), ("hvq_recon_inline_dyn_lds", 2), ("hvq_recon_inline_max_wgs", 2)):
            getattr(l, fn).restype = C.c_uint32
            getattr(l, fn).argtypes = [C.c_uint32] * nargs
    caps = sorted({64, 96, 128, 160, 192, 224, 256, 384, 512} | set(range(0, 1025, 32)) | {1, 63, 65, 127, 129, 511, 513, 4096})
    for tpw in (1, 2, 3):
        for cap in caps:
            assert fake.hvq_recon_inline_static_lds(tpw, cap) == real.hvq_recon_inline_static_lds(tpw, cap), (tpw, cap)
            assert fake.hvq_recon_inline_max_wgs(tpw, cap) == real.hvq_recon_inline_max_wgs(tpw, cap), (tpw, cap)
    for pairs in list(range(0, 40)) + [255, 256, 1023, 1024, 4095, 4096, 8192, 100000]:
        for pool in list(range(0, 40)) + [1535, 1536, 1540, 3080, 100001]:
            assert fake.hvq_recon_inline_dyn_lds(pairs, pool) == real.hvq_recon_inline_dyn_lds(pairs, pool), (pairs, pool)
