"""Shared inputs of the device-cells tests (H2MI_CELLS_I64 / H2MI_CELLS_DEVICE, h2mi_fr_scatter_cells_dev) and what they must become, in
Python integers: mont(v) = v 2^256 mod r as four little-endian 64-bit limbs.  Computed once per (format, count), shared, never changed.
tests/test_device_cells_host.py checks this file against pow / %; tests/test_gpu_device_cells.py checks the library against it."""
import functools
import random

import numpy as np

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
MASK64 = (1 << 64) - 1
FORMATS = {"montgomery": 0, "canonical": 1, "i64": 4}  # h2mi_cells_source.format: 0, H2MI_CELLS_CANONICAL, H2MI_CELLS_I64

I64_EDGES = [0, 1, -1, 2**32 - 1, -(2**32 - 1), 2**32, -(2**32), 2**62, 2**63 - 1, -(2**63)]
# canonical integers below r: the ends, 2^256 mod r (whose Montgomery form is R^2), and one saturated limb alone (the top limb of r is
# 0x30644E72E131A029, so a saturated top limb is not below r)
CANONICAL_EDGES = [0, 1, R - 1, (1 << 256) % R, MASK64, MASK64 << 64, MASK64 << 128]
# Montgomery words are carried verbatim, reduced or not: r itself, 2^256 - 1, r + 1, a saturated top limb
MONTGOMERY_EDGES = [0, 1, R - 1, R, R + 1, (1 << 256) - 1, MASK64 << 192, (1 << 256) % R]
COUNTS = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 4097, 2**13 - 6]
ROW_LISTS = ["ascending", "reversed", "stride3", "random", "ends"]
SENTINEL = np.array([0xF111F111F111F111, 0x5E5E5E5E5E5E5E5E, 0x0123456789ABCDEF, 0xFEDCBA9876543210], dtype=np.uint64)


def limbs(v: int) -> list:
    return [(v >> (64 * j)) & MASK64 for j in range(4)]


def mont(v: int) -> list:
    """the Montgomery word of v mod r"""
    return limbs((v % R) * (1 << 256) % R)


def values(fmt: str, count: int) -> list:
    """`count` cells as Python integers: the format's edge values first (as many as fit), then seeded random ones"""
    rng = random.Random(f"device cells {fmt} {count}")
    if fmt == "i64":
        edges, draw = I64_EDGES, lambda: rng.randrange(-(2**63), 2**63)
    elif fmt == "canonical":
        edges, draw = CANONICAL_EDGES, lambda: rng.randrange(R)
    else:
        edges, draw = MONTGOMERY_EDGES, lambda: rng.randrange(1 << 256)
    return (edges + [draw() for _ in range(max(0, count - len(edges)))])[:count]


@functools.lru_cache(maxsize=None)
def case(fmt: str, count: int):
    """-> (the values as the caller's array: int64 of shape (count,) or uint64 of shape (count, 4); the expected words, uint64 (count, 4))"""
    vals = values(fmt, count)
    if fmt == "i64":
        src = np.array(vals, dtype=np.int64)
        want = np.array([mont(v) for v in vals], dtype=np.uint64).reshape(count, 4)
    else:
        src = np.array([limbs(v) for v in vals], dtype=np.uint64).reshape(count, 4)
        want = src.copy() if fmt == "montgomery" else np.array([mont(v) for v in vals], dtype=np.uint64).reshape(count, 4)
    src.setflags(write=False)
    want.setflags(write=False)
    return src, want


def rows(kind: str, count: int, row_limit: int):
    """the row list of a column of `count` cells below row_limit: distinct rows, uint32; None for "dense" (rows 0 .. count - 1)"""
    if kind == "dense":
        assert count <= row_limit
        return None
    if kind == "ascending":
        out = list(range(row_limit - count, row_limit))  # not rows 0 .. count - 1 unless the column is full
    elif kind == "reversed":
        out = list(range(count))[::-1]
    elif kind == "stride3":
        assert 3 * (count - 1) < row_limit
        out = [3 * i for i in range(count)]
    elif kind == "random":
        out = random.Random(f"rows {count} {row_limit}").sample(range(row_limit), count)
    elif kind == "ends":  # the first and the last usable row, at the list's far ends in the wrong order, the rest between them
        inner = random.Random(f"ends {count} {row_limit}").sample(range(1, row_limit - 1), max(0, count - 2))
        out = ([row_limit - 1] + inner + [0])[:count] if count > 1 else [row_limit - 1]
    else:
        raise ValueError(kind)
    assert len(out) == count == len(set(out)) and all(0 <= r < row_limit for r in out)
    return np.array(out, dtype=np.uint32)


def expected_column(n_rows: int, row_list, want: np.ndarray) -> np.ndarray:
    """a destination of n_rows sentinel words after the cells have landed"""
    out = np.tile(SENTINEL, (n_rows, 1))
    out[np.arange(len(want)) if row_list is None else row_list.astype(np.int64)] = want
    return out


# the 64 columns of the one-call test: empty columns, one cell, lengths around a wave, a workgroup and the host thresholds
MANY_LENGTHS = [0, 1, 65, 4097, 2, 63, 0, 64, 255, 256, 257, 1023, 1024, 1025, 4096, 300] * 4


def many_columns():
    """-> [(fmt, row kind, count, n_rows)] for MANY_LENGTHS: formats and row lists cycle at different periods"""
    fmts, kinds = list(FORMATS), ["dense"] + ROW_LISTS
    return [(fmts[i % 3], kinds[(i // 3 + i) % 6], count, 3 * count + 2) for i, count in enumerate(MANY_LENGTHS)]
