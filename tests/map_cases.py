"""What the map tests share: the tables, the rules, the histogram records and the made pictures (tests/test_map_cpu.py,
tests/test_gpu_map.py, tests/golden/make_map.py).  Every table that is not a known answer is a random PERMUTATION, distinct per plane and
per table: a swapped byte, plane or `which` entry changes the output."""
import numpy as np

from hvqm4_amd import maps as M

MAX_N = 1 << 26                                     # the samples of the largest plane the library opens


def perm_table(seed: int) -> M.Table:
    rng = np.random.default_rng(1000 + seed)
    return M.from_lut(*[rng.permutation(256).astype(np.uint8) for _ in range(3)])


# the fixture's five, by label (tests/golden/make_map.py spells the same tables without the module)
FIVE = [("identity", M.identity()), ("invert", M.invert()), ("flat77", M.flat_table(77)), ("perm0", perm_table(0)), ("perm1", perm_table(1))]


def tables(n: int):
    """n distinct tables: the known answers, then permutations"""
    known = [t for _l, t in FIVE[:3]]
    return (known + [perm_table(i) for i in range(max(0, n - len(known)))])[:n]


RULES = {                                           # the first is well formed in both planes (the driver's malformed ones derive from it)
    "equalize": M.equalize(), "identity": M.keep(), "flat9": M.flat(9), "stretch0": M.stretch(0, 0), "stretch499": M.stretch(499, 499),
    "stretch10_20": M.stretch(10, 20), "otsu": M.otsu(), "mixed": M.Rule(M.otsu().luma, M.equalize().chroma), "eq_luma": M.equalize().luma_only(),
    "flat255_stretch": M.Rule(M.flat(255).luma, M.stretch(5, 0).chroma),
}


def _bins(**at):
    h = np.zeros(256, dtype=np.int64)
    for k, v in at.items():
        h[int(k[1:])] = v
    return h


def special_records():
    """(label, int64 [3, 256]): the records the header's text has a sentence for"""
    uniform = np.full(256, 1200, dtype=np.int64)
    ramp = np.arange(256, dtype=np.int64)
    out = [
        ("single value", np.stack([_bins(v77=4096), _bins(v0=1024), _bins(v255=1024)])),
        ("two values", np.stack([_bins(v3=10, v200=30), _bins(v0=1, v255=1), _bins(v127=500, v128=501)])),
        ("uniform", np.stack([uniform, uniform // 4, ramp])),
        ("otsu tie", np.stack([_bins(v10=5, v20=5), _bins(v0=7, v255=7), _bins(v100=3, v101=3)])),        # symmetric peaks: every t between them ties
        ("empty", np.zeros((3, 256), dtype=np.int64)),
        ("empty luma only", np.stack([np.zeros(256, dtype=np.int64), uniform, _bins(v9=2)])),
        ("2^26 between 0 and 255", np.stack([_bins(v0=MAX_N // 2, v255=MAX_N // 2), _bins(v0=1, v255=MAX_N - 1), _bins(v0=MAX_N - 1, v255=1)])),
        ("2^26 between 0 and 1", np.stack([_bins(v0=MAX_N // 2, v1=MAX_N // 2), _bins(v0=MAX_N // 3, v1=MAX_N - MAX_N // 3), _bins(v254=MAX_N // 2, v255=MAX_N // 2)])),
        ("2^26 in three peaks", np.stack([_bins(v0=MAX_N // 4, v128=MAX_N // 2, v255=MAX_N // 4), _bins(v1=MAX_N // 2, v127=MAX_N // 4, v254=MAX_N // 4), uniform * 0 + MAX_N // 256])),
        ("hi <= lo", np.stack([_bins(v50=1000, v60=1), _bins(v1=1, v2=1000, v3=1), _bins(v0=999, v255=1)])),   # the clipped ranks meet in the heavy bin
        ("one sample", np.stack([_bins(v200=1), _bins(v0=1), _bins(v255=1)])),
    ]
    for _l, r in out:
        assert r.shape == (3, 256) and r.sum(-1).max() <= MAX_N
    return out


def random_records(n: int = 300, seed: int = 11):
    """int64 [n, 3, 256]: sparse and dense histograms of 1 .. 2^26 samples, every third one of exactly 2^26"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 3, 256), dtype=np.int64)
    for i in range(n):
        for p in range(3):
            total = MAX_N if (i + p) % 3 == 0 else int(rng.integers(1, MAX_N + 1)) if i % 2 else int(rng.integers(1, 5000))
            k = int(rng.choice([1, 2, 3, 8, 64, 256]))
            where = rng.choice(256, size=k, replace=False)
            w = rng.random(k) ** 3 + 1e-9
            c = np.floor(w / w.sum() * total).astype(np.int64)
            c[0] += total - int(c.sum())
            out[i, p, where] = c
            assert int(out[i, p].sum()) == total
    return out


def all_records():
    """int64 [r, 3, 256]: the special ones, then the random ones"""
    return np.concatenate([np.stack([r for _l, r in special_records()]), random_records()])


def nbytes(geom):
    w, h, hs, vs = geom
    return w * h + 2 * (w >> (hs == 2)) * (h >> (vs == 2))


def made(geom, seed: int) -> np.ndarray:
    """a picture of random bytes in which every value occurs"""
    a = np.random.default_rng(seed).integers(0, 256, nbytes(geom), dtype=np.uint8)
    if a.size >= 256:
        a[:256] = np.arange(256, dtype=np.uint8)
    return a


def synth(geom, k: int) -> np.ndarray:
    """the fake-device driver's made picture: byte i = ((i + k) * 2654435761 mod 2^32) >> 13 & 255"""
    n = nbytes(geom)
    return ((((np.arange(n, dtype=np.uint64) + np.uint64(k)) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(13)).astype(np.uint8)


# GPU shapes: the smallest geometry in the three samplings, planes of 72 x 24 and 136 x 40, a luma plane of a tile and 512 bytes (136 x 64),
# a chroma plane of a tile and four dwords (the 108 x 76 of 216 x 152), and rows of 8192
SMALL = [(8, 8, 2, 2), (8, 8, 2, 1), (8, 8, 1, 1), (72, 24, 2, 2), (72, 24, 1, 1), (136, 40, 2, 2), (136, 40, 2, 1)]
SEAMS = [(128, 64, 2, 2), (136, 64, 2, 2), (216, 152, 2, 2), (128, 72, 1, 1)]
WIDE = (8192, 16, 2, 2)
