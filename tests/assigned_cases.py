"""Assigned cells (H2MI_CELLS_RATIONAL, h2mi_fr_batch_invert_dev, h2mi_fr_assigned_evaluate_dev), shared by tests/test_assigned_host.py
and tests/test_gpu_assigned.py: the sizes and data of the vector kernels with their references in Python integers
(`n * pow(d, -1, r) if d else 0` — Assigned::evaluate and ff's BatchInvert restated), and the circuits whose columns are handed over as
rationals next to the same circuits with the resolved values.  Every comparison made with these is exact."""
import functools
import random

import extreme_cases as X
from oracle import bn254 as o

R = o.R
TILE = 1024  # ASG_TILE of csrc/h2mi_plonk.hip: the elements one workgroup of passes (a) and (c) owns
PASS_B_THREADS = 1024  # k_assigned_tile_inverses: one workgroup; beyond this many tiles every thread owns a run of them
SIZES = [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 3 * TILE + 5]
BIG_N = (PASS_B_THREADS + 1) * TILE + 3  # 1025 tiles and three elements: runs of two tiles per thread, a ragged last tile
EXTREMES = list(dict.fromkeys(X.EXTREME_VALUES + [X.word_value(w) for w in X.EXTREME_WORDS]))  # values, and the values of the extreme words
PATTERNS = ("uniform", "no zero", "all zero", "zero at the ends", "zero at tile edges", "a tile of zeros", "one nonzero", "one and r - 1", "extremes")


def evaluate(n: int, d: int) -> int:
    """Assigned::evaluate of Rational(n, d)"""
    return n * pow(d, -1, R) % R if d else 0


def denominators(pattern: str, n: int) -> list:
    rng = random.Random(f"den {pattern} {n}")
    nz = lambda: rng.randrange(1, R)
    if pattern == "uniform":  # zero has probability 2^-254: a few are planted so that the pattern meets the rule at every size
        d = [rng.randrange(R) for _ in range(n)]
        for i in rng.sample(range(n), min(n, 3)) if n > 2 else []:
            d[i] = 0
        return d
    if pattern == "no zero":
        return [nz() for _ in range(n)]
    if pattern == "all zero":
        return [0] * n
    if pattern == "zero at the ends":
        d = [nz() for _ in range(n)]
        d[0] = d[-1] = 0
        return d
    if pattern == "zero at tile edges":  # the first and the last slot of every tile (the last tile: its last element too)
        d = [nz() for _ in range(n)]
        for i in range(n):
            if i % TILE in (0, TILE - 1) or i == n - 1:
                d[i] = 0
        return d
    if pattern == "a tile of zeros":  # the second tile whole, between live tiles (a shorter vector: its middle third)
        lo, hi = (TILE, 2 * TILE) if n > 2 * TILE else (n // 3, max(n // 3 + 1, 2 * n // 3))
        return [0 if lo <= i < hi else nz() for i in range(n)]
    if pattern == "one nonzero":
        d = [0] * n
        d[rng.randrange(n)] = nz()
        return d
    if pattern == "one and r - 1":
        return [(1, R - 1)[(i + i // 3) % 2] for i in range(n)]
    if pattern == "extremes":  # every extreme value at every size from len(EXTREMES) on, rotated so that tile edges see different ones
        return [EXTREMES[(i + i // TILE) % len(EXTREMES)] for i in range(n)]
    raise KeyError(pattern)


def numerators(pattern: str, n: int) -> list:
    """random, with zeros and extremes mixed in: over a zero denominator both a zero and a nonzero numerator occur (cells i % 2)"""
    rng = random.Random(f"num {pattern} {n}")
    out = []
    for i in range(n):
        t = rng.randrange(8)
        out.append(0 if t == 0 else EXTREMES[rng.randrange(len(EXTREMES))] if t == 1 else rng.randrange(1, R))
    d = denominators(pattern, n)
    zeros = [i for i in range(n) if d[i] == 0]
    for j, i in enumerate(zeros):
        out[i] = 0 if j % 2 == 0 else rng.randrange(1, R)
    return out


@functools.lru_cache(maxsize=None)
def vector_case(pattern: str, n: int):
    """-> (numerators, denominators, the inverses with 0 for 0, the evaluated cells); computed once, shared, never changed"""
    d, num = denominators(pattern, n), numerators(pattern, n)
    inv = tuple(pow(x, -1, R) if x else 0 for x in d)
    return tuple(num), tuple(d), inv, tuple(a * b % R for a, b in zip(num, inv))


# ---- circuits ---------------------------------------------------------------------------------------------------------------------
def _value(v, resolved: bool):
    return v.evaluate() if resolved and not isinstance(v, int) else v


def is_zero_circuit(custom, x: int, resolved: bool = False, flip_out: bool = False):
    """src/circuits/is_zero.rs with value_inv assigned as the reference assigns it: `value.invert()` left to the prover, Rational(1, x) —
    which evaluates to 0 for x = 0 and satisfies the gate there too (x y + out - 1 = 0 + 1 - 1).  resolved: the same circuit with the
    evaluated integer in that cell.  -> (cs, assignment)"""
    meta = custom.ConstraintSystem()
    cx, cy, cout = (meta.advice_column() for _ in range(3))
    selector = meta.selector()
    for column in (cx, cout):
        meta.enable_equality(column)

    def gate(meta):
        x_, y_, out_ = (meta.query_advice(col, custom.Rotation.cur()) for col in (cx, cy, cout))
        s = meta.query_selector(selector)
        return [s * (x_ * y_ + out_ - custom.Expression.constant(1)), s * x_ * out_]

    meta.create_gate("ISZERO gate", gate)
    region = custom.Assignment(meta)
    x %= R
    region.assign_advice(cx, 0, x)
    region.assign_advice(cy, 0, _value(custom.Rational(1, x), resolved))
    out_val = 1 if x == 0 else 0
    out = region.assign_advice(cout, 0, out_val ^ 1 if flip_out else out_val)
    region.enable_selector(selector, 0)
    region.copy_advice(out, cx, 1)
    return meta, region


def mixed_values(custom, count: int, seed) -> list:
    """what a column of Assigned<F> holds: Trivial(x) as integers, true fractions, zero denominators under zero and nonzero numerators,
    zero numerators, the field's extremes in both halves"""
    rng = random.Random(f"mixed {seed}")
    out = []
    for i in range(count):
        t = i % 8
        if t in (0, 1):
            out.append(rng.randrange(R))
        elif t == 2:
            out.append(custom.Rational(rng.randrange(1, R), 0))
        elif t == 3:
            out.append(custom.Rational(0, 0) if i % 16 == 3 else custom.Rational(0, rng.randrange(1, R)))
        elif t == 4:
            out.append(custom.Rational(EXTREMES[i // 8 % len(EXTREMES)], EXTREMES[i // 64 % len(EXTREMES)]))
        else:
            out.append(custom.Rational(rng.randrange(R), rng.randrange(1, R)))
    return out


def columns_circuit(custom, advice, fixed=(), resolved: bool = False, phases=None):
    """a circuit that exists for its columns: advice / fixed are [{row: integer or Rational}] per column; the first advice column and every
    fixed column take part in the permutation argument (which queries them), one gate s (first advice * last advice - first advice)
    whose selector is never enabled, so any cells satisfy it.  phases: the phase per advice column.  -> (cs, assignment)"""
    meta = custom.ConstraintSystem()
    acols = [meta.advice_column_in(phases[j]) if phases else meta.advice_column() for j in range(len(advice))]
    fcols = [meta.fixed_column() for _ in fixed]
    s = meta.selector()
    for column in [acols[0]] + fcols:
        meta.enable_equality(column)
    cur = custom.Rotation.cur()

    def gate(meta):
        first, last = meta.query_advice(acols[0], cur), meta.query_advice(acols[-1], cur)
        return [meta.query_selector(s) * (first * last - first)]

    meta.create_gate("columns", gate)
    region = custom.Assignment(meta)
    for col, cells in zip(acols, advice):
        for row, v in cells.items():
            region.assign_advice(col, row, _value(v, resolved))
    for col, cells in zip(fcols, fixed):
        for row, v in cells.items():
            region.assign_fixed(col, row, _value(v, resolved))
    return meta, region


def dense(values) -> dict:
    return dict(enumerate(values))


def scattered(values, usable: int, seed) -> dict:
    """the values on shuffled rows of 0 .. usable - 1 (never rows 0 .. count - 1 exactly)"""
    rows = random.Random(f"rows {seed}").sample(range(1, usable), len(values))
    return dict(zip(rows, values))


BIG_K = 13  # 8192 rows: room for scattered columns beyond 4096 cells
