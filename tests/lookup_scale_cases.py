"""Inputs for the lookup kernels beyond one workgroup, shared by tests/test_gpu_lookup.py (the device against oracle/lookup.py, row by
row) and tests/test_lookup_scale_host.py (the generator against the oracle alone: that every case reaches what it is named for).

What the sizes reach (k_lk_rank takes 1024 rows per workgroup and keeps a 64-slot table keyed by rank & 63, the counter scans of
scan.cuh split into segments of 8192, the multiplicative scans into tiles of 1024, the grand product flags rows only from 4096 usable
rows on and takes its sparse form when at most a quarter of them are flagged):
    k = 11, u = 2042    two k_lk_rank workgroups, two tiles
    k = 13, u = 8186    past the 4096 threshold, still one scan segment
    k = 14, u = 16378   two scan segments, 16 tiles
Everything is seeded from the case's name; the values are Python integers below the scalar field's modulus."""
import random
import types
import zlib

import numpy as np

from oracle import bn254 as o
from oracle.plonk import BLINDING_FACTORS

R = o.R
RANK_BLOCK, RANK_SLOTS, COLLIDING_SLOT = 1024, 64, 5


def usable(k: int) -> int:
    return (1 << k) - (BLINDING_FACTORS + 1)


def _rng(*key) -> random.Random:
    return random.Random(zlib.crc32(repr(key).encode()))


def mont_limbs(values) -> np.ndarray:
    """integers -> (count, 4) uint64 Montgomery limbs, the columns' memory format"""
    return np.frombuffer(b"".join(((v << 256) % R).to_bytes(32, "little") for v in values), dtype=np.uint64).reshape(-1, 4)


def from_mont_limbs(arr) -> list:
    raw, rinv = np.ascontiguousarray(arr).tobytes(), pow(1 << 256, -1, R)
    return [int.from_bytes(raw[i : i + 32], "little") * rinv % R for i in range(0, len(raw), 32)]


def distinct_sorted(table, u: int) -> list:
    return sorted(set(table[:u]))


# ---- 1. permuted columns -----------------------------------------------------------------------------------------------------------
KS = (11, 13, 14)
TABLES = ("uniform", "repeats", "low word", "range")
INPUTS = ("uniform", "skewed", "rank 5 mod 64", "ends", "permutation")
DISTINCT_TABLES = ("uniform", "low word")  # a permutation of the table as the input needs a table without a repeated value
PERMUTE_CASES = [(k, t, i) for k in KS for t in TABLES for i in INPUTS if i != "permutation" or t in DISTINCT_TABLES]
LOW_WORD_PERIOD = 37


def _distinct(rng, count: int, draw) -> list:
    seen = set()
    while len(seen) < count:
        seen.add(draw())
    out = sorted(seen)
    rng.shuffle(out)
    return out


def make_table(kind: str, k: int, u: int, rng, n_unique: int = None) -> list:
    """the table column's first u rows"""
    if kind == "uniform":
        return _distinct(rng, u, lambda: rng.randrange(R))
    if kind == "repeats":  # about half the rows distinct, the other half repeating five of them
        values = _distinct(rng, u // 2 if n_unique is None else n_unique, lambda: rng.randrange(R))
        often = values[:5]
        rows = values + [often[min(rng.randrange(8), 4)] for _ in range(u - len(values))]
        rng.shuffle(rows)
        return rows
    if kind == "low word":  # the low 32-bit word is a valid index into the sorted table and (mostly) not the value's rank
        high = _distinct(rng, u, lambda: rng.randrange(1, (R >> 64) - 1))
        return [(i % LOW_WORD_PERIOD) + (h << 64) for i, h in enumerate(high)]
    assert kind == "range"  # 0 .. 2^(k-2) - 1 and zeros: where a value is its own rank
    return list(range(1 << (k - 2))) + [0] * (u - (1 << (k - 2)))


def make_input(kind: str, table, u: int, rng) -> list:
    """u input values, every one a table value; 'uniform' is uniform over the table's distinct values"""
    values = distinct_sorted(table, u)
    if kind == "uniform":
        return [rng.choice(values) for _ in range(u)]
    if kind == "skewed":
        often = rng.choice(values)
        return [often if rng.random() < 0.9 else rng.choice(values) for _ in range(u)]
    if kind == "rank 5 mod 64":
        picks = [values[r] for r in range(COLLIDING_SLOT, len(values), RANK_SLOTS)]
        rows = [rng.choice(picks) for _ in range(u)]
        for i in range(u):  # the first eight rows of every workgroup: eight different ranks for certain
            if i % RANK_BLOCK < 8:
                rows[i] = picks[(i % RANK_BLOCK + i // RANK_BLOCK) % len(picks)]
        return rows
    if kind == "ends":
        return [values[0] if rng.random() < 0.5 else values[-1] for _ in range(u)]
    assert kind == "permutation"
    rows = list(table[:u])
    rng.shuffle(rows)
    return rows


def absent_values(table, u: int) -> dict:
    """three values that are in no usable table row: below the smallest, above the largest, strictly between two neighbours.  A range
    table starts at zero and has no gap, so there all three lie above the largest."""
    ordered = distinct_sorted(table, u)
    lo, hi = ordered[0], ordered[-1]
    gap = next((a + 1 for a, b in zip(ordered[len(ordered) // 2 :], ordered[len(ordered) // 2 + 1 :]) if b - a > 1), None)
    if lo == 0 or gap is None:
        return {"above": hi + 1, "above 2": hi + 2, "top of the field": R - 1}
    return {"below": lo - 1, "above": hi + 1, "between": gap}


def _finish(k: int, u: int, table, inputs, rng):
    n = 1 << k
    rest = lambda: [rng.randrange(R) for _ in range(n - u)]
    # the rows beyond the usable ones: the table's and the input's are not read; the permuted columns' are the caller's and stay
    return types.SimpleNamespace(k=k, n=n, u=u, table=list(table) + rest(), inputs=list(inputs) + rest(), keep_a=rest(), keep_s=rest())


def permute_case(k: int, table_kind: str, input_kind: str):
    rng = _rng("permute", k, table_kind, input_kind)
    u = usable(k)
    table = make_table(table_kind, k, u, rng)
    case = _finish(k, u, table, make_input(input_kind, table, u, rng), rng)
    case.absent = absent_values(table, u)
    case.absent_rows = (0, RANK_BLOCK, u - 1)
    bad = list(case.inputs)
    for row, v in zip(case.absent_rows, case.absent.values()):
        bad[row] = v
    case.bad_inputs = bad
    return case


# usable_rows as a free argument: every residue modulo 4 (the scans' zero pads), one row either side of a k_lk_rank workgroup and of a
# scan segment; the table's distinct count takes every residue too
USABLE_ROWS = [(11, usable(11) - d) for d in range(4)] + [(11, 1023), (11, 1024), (11, 1025), (14, 8191), (14, 8192), (14, 8193), (14, usable(14))]


def usable_case_distinct(index: int) -> int:
    u = USABLE_ROWS[index][1]
    base = u // 2 + 8
    return base + (index - base) % 4  # n_unique % 4 == index % 4


def usable_case(index: int):
    k, u = USABLE_ROWS[index]
    rng = _rng("usable", k, u)
    table = make_table("repeats", k, u, rng, n_unique=usable_case_distinct(index))
    return _finish(k, u, table, make_input("uniform", table, u, rng), rng)


# ---- 2. grand product ----------------------------------------------------------------------------------------------------------------
# name -> (k, usable_rows, m = rows whose ratio differs from one, the form the library must take)
PRODUCT_CASES = {
    "dense, two tiles (k = 11)": (11, usable(11), 700, "dense"),
    "dense, below the flag threshold, partial last tile (k = 12)": (12, usable(12), 1500, "dense"),
    "dense, every row (k = 13)": (13, usable(13), usable(13), "dense"),
    "threshold: a quarter of the rows": (13, usable(13), usable(13) // 4, "sparse"),
    "threshold: a quarter of the rows plus one": (13, usable(13), usable(13) // 4 + 1, "dense"),
    "usable_rows = 4095": (13, 4095, 10, "dense"),
    "usable_rows = 4096": (13, 4096, 10, "sparse"),
    "sparse, m = 0": (13, usable(13), 0, "sparse"),
    "sparse, m = 1": (13, usable(13), 1, "sparse"),
    "sparse, m = 1023": (13, usable(13), 1023, "sparse"),
    "sparse, m = 1024": (13, usable(13), 1024, "sparse"),
    "sparse, m = 1025": (13, usable(13), 1025, "sparse"),
    "sparse, two scan segments (k = 14)": (14, usable(14), 3000, "sparse"),
}
SEGMENT = 8192
SENTINEL = 0xDEAD


def product_case(name: str):
    """four columns of which exactly m usable rows have (input, table) != (permuted input, permuted table): the kernel multiplies any
    four columns, they need not be a permutation of one another"""
    k, u, m, form = PRODUCT_CASES[name]
    rng = _rng("product", name)
    n = 1 << k
    column = lambda: [rng.randrange(R) for _ in range(n)]
    inputs, table = column(), column()
    pin, ptab = list(inputs), list(table)
    if m == u:
        rows = list(range(u))
    elif k == 14:  # the first and the last usable row, more than a tile of rows in the compaction's second scan segment
        rows = sorted([0, u - 1] + rng.sample(range(1, SEGMENT), m - 1402) + rng.sample(range(SEGMENT + 1, u - 1), 1400))
    else:
        rows = sorted(rng.sample(range(u), m))
    for j, row in enumerate(rows):  # a third each: the permuted input alone, the permuted table alone, both
        if j % 3 != 1:
            pin[row] = rng.randrange(R)
        if j % 3 != 0:
            ptab[row] = rng.randrange(R)
    for col in (pin, ptab):  # beyond the usable rows nothing is read: every column differs there
        col[u:] = [rng.randrange(R) for _ in range(n - u)]
    return types.SimpleNamespace(k=k, n=n, u=u, m=m, form=form, rows=rows, inputs=inputs, table=table, pin=pin, ptab=ptab, beta=rng.randrange(R),
                                 gamma=rng.randrange(R))
