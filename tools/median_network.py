"""The selection network of the 5 x 5 median in hvqm4_amd/csrc/hvq_rank.h (hvq_rk_med_select5), derived and checked by machine.

Wire 5 c + l holds level l of column c; every column arrives sorted (the kernel sorts the columns once for all the targets that share
them).  A sorting network of 25 -- the levels sorted across the columns, then Batcher's odd-even merge sort, over the wires in several
orders -- loses (1) every exchange that never swaps on any admissible input and (2) every exchange, or half of one, that the median's
wire does not depend on.  Checking on the 6^5 0 / 1 patterns of sorted columns suffices: a threshold of sorted columns is sorted
columns, so the 0 / 1 principle holds for the restricted inputs, and an exchange that never swaps on them never swaps at all.

    python tools/median_network.py

prints the cheapest candidate as the X / LO / HI lines of hvq_rank.h: X(a,b) leaves the minimum on a and the maximum on b, LO(a,b) only
the minimum on a, HI(a,b) only the maximum on b.  check(ops, out) verifies a list of such operations; tests/test_rank_cpu.py runs it
on the lines the header holds."""
import itertools
import re

SORT5 = [(0, 1), (3, 4), (2, 4), (2, 3), (0, 3), (0, 2), (1, 4), (1, 3), (1, 2)]       # the column sort of hvq_rk_med_sort5


def admissible():
    """the 0 / 1 inputs with sorted columns: column c has k[c] ones at its top levels"""
    out = []
    for ks in itertools.product(range(6), repeat=5):
        v = [0] * 25
        for c, k in enumerate(ks):
            for l in range(5 - k, 5):
                v[c * 5 + l] = 1
        out.append(v)
    return out


def batcher(n):
    """the exchanges of the odd-even merge sort of n wires, n a power of two"""
    out = []

    def merge(lo, n, r):
        m = r * 2
        if m < n:
            merge(lo, n, m)
            merge(lo + r, n, m)
            out.extend((i, i + r) for i in range(lo + r, lo + n - r, m))
        else:
            out.append((lo, lo + r))

    def sort(lo, n):
        if n > 1:
            sort(lo, n // 2)
            sort(lo + n // 2, n // 2)
            merge(lo, n, 1)
    sort(0, n)
    return out


def check(ops, outw, inputs=None):
    """AssertionError unless the operations (kind, a, b) leave the median of every admissible 0 / 1 input on wire outw"""
    for v in inputs or admissible():
        w = list(v)
        for k, a, b in ops:
            lo, hi = min(w[a], w[b]), max(w[a], w[b])
            if k in ("X", "LO"):
                w[a] = lo
            if k in ("X", "HI"):
                w[b] = hi
        assert w[outw] == sorted(v)[12], v


def prune(net, outw, inputs):
    """the exchanges (a, b) of a sorting network -> the operations the median on wire outw needs"""
    while True:
        swaps = [0] * len(net)
        for v in inputs:
            v = list(v)
            for i, (a, b) in enumerate(net):
                if v[a] > v[b]:
                    v[a], v[b] = v[b], v[a]
                    swaps[i] += 1
        kept = [c for c, s in zip(net, swaps) if s]
        if len(kept) == len(net):
            break
        net = kept
    live, ops = {outw}, []
    for a, b in reversed(net):
        if a in live or b in live:
            ops.append(("X" if a in live and b in live else "LO" if a in live else "HI", a, b))
            live |= {a, b}
    return ops[::-1]


def candidates():
    rows = [(l + 5 * a, l + 5 * b) for l in range(5) for a, b in SORT5]                # every level sorted across the columns
    full = [(a, b) for a, b in batcher(32) if b < 25]                                 # wires 25 .. 31 hold infinity
    order = sorted(range(25), key=lambda w: ((w % 5) + (w // 5), w))                  # by anti-diagonal: close to sorted after the row sorts
    yield "batcher", full, 12
    yield "rows + batcher", rows + full, 12
    yield "rows + batcher over the anti-diagonals", rows + [(order[a], order[b]) for a, b in full], order[12]


def derive():
    """-> (min / max operations, name, operations, output wire) of the cheapest candidate"""
    inputs = admissible()
    best = None
    for name, net, outw in candidates():
        ops = prune(net, outw, inputs)
        check(ops, outw, inputs)
        cost = sum(2 if k == "X" else 1 for k, _a, _b in ops)
        if best is None or cost < best[0]:
            best = (cost, name, ops, outw)
    return best


def parse(text):
    """the operations in a piece of C that spells them X(a,b) LO(a,b) HI(a,b)"""
    return [(k, int(a), int(b)) for k, a, b in re.findall(r"\b(X|LO|HI)\((\d+),\s*(\d+)\)", text)]


def main():
    cost, name, ops, outw = derive()
    print(f"/* {name}: {len(ops)} exchanges, {cost} min / max; the median leaves on wire {outw} */")
    line = ""
    for k, a, b in ops:
        t = f"{k}({a},{b}) "
        if len(line) + len(t) > 130:
            print(line.rstrip())
            line = ""
        line += t
    print(line.rstrip())


if __name__ == "__main__":
    main()
