"""Sizes, inputs and references for the one-workgroup TILE-OFFSET passes in their upper regimes, shared by tests/test_tile_regimes_host.py
(the generator and its references against the existing small references: every named size reaches what its name says) and
tests/test_gpu_tile_regimes.py (the device against the references here).

Five vector pipelines share one shape: a `local` kernel works tile by tile (TILE elements), ONE workgroup of THREADS threads turns the
tile totals into tile offsets, an `apply` / `finish` kernel folds the offsets back in.  Only the middle pass has control flow that
depends on the tile count T:
  A   T <= LANES           every owning thread sits in wavefront 0, nothing crosses a wavefront
  B   LANES < T <= THREADS one tile per thread, the scan crosses wavefronts through LDS
  C   T > THREADS          per = ceil(T / THREADS) >= 2: a thread owns a RUN of per tiles, used = ceil(T / per) threads own one, the last
                           run holds T - (used - 1) per tiles
(k_addscan_offsets in csrc/h2mi_plonk.hip, k_kate_offsets_multi in csrc/h2mi_poly.hip, k_assigned_tile_inverses in csrc/h2mi_plonk.hip).
k_cells_prefix (csrc/h2mi_cells.hip) walks a column's tile words in ROUNDS of CELL_ROUND words with a carry between the rounds.

The vectors have up to two million rows, so nothing here does per-element Python big-integer work: the data are Montgomery limb arrays
made with numpy, the arithmetic is oracle/vec.py's (the C oracle).  The running sums are not compared with a prefix sum: the statement
that determines the column — phi[0] = 0 and (phi[i + 1] - phi[i]) D_i = N_i on every usable row, with N / D the fraction of
tests/logup_sets_cases.py — is checked elementwise; with no D_i zero it fixes every row, so it is equality and not a weaker statement
(tests/perm_scale_cases.py does the same for z beyond 2^20).  Everything is seeded from the case's parameters."""
import random
import types
import zlib

import numpy as np

import extreme_cases
import key_file_cases as K
import logup_sets_cases
import perm_scale_cases
from oracle import bn254 as o
from oracle.plonk import BLINDING_FACTORS
from oracle.vec import FV

R = o.R
TILE, THREADS, LANES, CELL_ROUND = 1024, 1024, 64, 256
# element counts: usable rows of a running sum, coefficients of a division
SIZES = {
    "B-min": LANES * TILE + 1,      # 65 tiles, the last of one element
    "B-full": (1 << 20) - 6,        # 1024 tiles: every thread owns one
    "C-short": THREADS * TILE + 1,  # 1025 tiles: runs of two, the last run one tile of one element
    "C-even": 1026 * TILE - 3,      # 1026 tiles: runs of two, all full, the last tile ragged
}
CELL_TILES = (257, 512, 513)  # a second round of one word; two full rounds; a third
TABLE_VALUES = 4099  # five tiles of distinct table values, no multiple of 4


def tiles_of(count: int) -> int:
    return -(-count // TILE)


def middle_pass(tiles: int):
    """-> (per, used, tiles of the last run): the rule of the three one-workgroup passes"""
    per = -(-tiles // THREADS)
    used = -(-tiles // per)
    return per, used, tiles - (used - 1) * per


def regime(tiles: int) -> str:
    return "A" if tiles <= LANES else "B" if tiles <= THREADS else "C"


def cell_rounds(tiles: int):
    """-> (rounds of k_cells_prefix over a column of `tiles` tile words, words of the last round)"""
    rounds = -(-tiles // CELL_ROUND)
    return rounds, tiles - (rounds - 1) * CELL_ROUND


def smallest_k(u: int) -> int:
    """the smallest k whose usable rows 2^k - (BLINDING_FACTORS + 1) hold u"""
    k = 1
    while (1 << k) - (BLINDING_FACTORS + 1) < u:
        k += 1
    return k


# ---- limb vectors ---------------------------------------------------------------------------------------------------------------------
def _seed(*key) -> int:
    return zlib.crc32(repr(key).encode()) & 0x3FFFFFFF


def _fv(a) -> FV:
    return FV(np.ascontiguousarray(a, dtype=np.uint64))


def small_raw(ints) -> np.ndarray:
    """non-negative integers below 2^64 -> (count, 4) words, not Montgomery"""
    out = np.zeros((len(ints), 4), dtype=np.uint64)
    out[:, 0] = np.asarray(ints, dtype=np.uint64)
    return out


def to_mont(raw) -> np.ndarray:
    """canonical words -> the columns' Montgomery words: a Montgomery product with 2^512"""
    return (_fv(raw) * (1 << 256)).a


def from_mont(limbs) -> np.ndarray:
    """Montgomery words -> canonical words: a Montgomery product with the integer one"""
    return (_fv(limbs) * pow(1 << 256, -1, R)).a


def limbs_of(v: int) -> np.ndarray:
    return np.array(o.int_to_limbs(v), dtype=np.uint64)


def mont_of(v: int) -> np.ndarray:
    return limbs_of((v % R << 256) % R)


def _indices(count: int, seed: int, below: int) -> np.ndarray:
    return (o.splitmix64_np(np.arange(count, dtype=np.uint64), seed) % np.uint64(below)).astype(np.int64)


def filler(rows: int, seed: int) -> np.ndarray:
    """`rows` nonzero words that belong to no table: a block of uniform elements, repeated (sentinels, and rows nothing may read)"""
    block = o.random_field_limbs(1021, seed)
    assert nonzero_rows(block)
    return np.ascontiguousarray(np.resize(block, (rows, 4)))


def nonzero_rows(limbs) -> bool:
    return bool(np.asarray(limbs).any(axis=1).all())


canonical = perm_scale_cases.canonical


# ---- the running sums -----------------------------------------------------------------------------------------------------------------
def sum_case(size: str, K_sets: int, n_unique: int = TABLE_VALUES, absent: bool = False, u: int = None):
    """K_sets input columns over one table of n_unique distinct uniform values.  Table row r < n_unique holds distinct value r (so the
    first row of value r is row r), the rows behind repeat the values in turn; every input is a table value (absent: but the last usable
    row of the last column).  The rows beyond u of every column hold values that would change the result if they were read.
    -> k, n, u, K, values (n_unique Montgomery words), s_idx / a_idx (the value index per row), table / cols / m_col (n rows of
    Montgomery words), counts (per value index), m (per usable row, integers), beta, absent (the (row, column) pairs)"""
    u = SIZES[size] if u is None else u
    k = smallest_k(u)
    n = 1 << k
    nu = u if n_unique == "u" else n_unique
    seed = _seed("sum", size, u, K_sets, nu, absent)
    c = types.SimpleNamespace(name=f"{size}, K = {K_sets}, n_unique = {nu}" + (", one absent input" if absent else ""), k=k, n=n, u=u, K=K_sets, nu=nu)
    c.values = o.random_field_limbs(nu, seed)
    assert len(np.unique(c.values, axis=0)) == nu
    c.s_idx = np.arange(n, dtype=np.int64) % nu
    c.a_idx = [_indices(n, seed + 10 + j, nu) for j in range(K_sets)]
    c.table = np.ascontiguousarray(c.values[c.s_idx])
    c.cols = [np.ascontiguousarray(c.values[a]) for a in c.a_idx]
    present = [np.ones(u, dtype=bool) for _ in range(K_sets)]
    c.absent = []
    if absent:
        stranger = o.random_field_limbs(1, seed + 99)[0]
        assert not (c.values == stranger).all(axis=1).any()
        c.cols[K_sets - 1][u - 1] = stranger
        present[K_sets - 1][u - 1] = False
        c.absent = [(u - 1, K_sets - 1)]
    c.present = present
    c.counts = np.bincount(np.concatenate([a[:u][p] for a, p in zip(c.a_idx, present)]), minlength=nu)
    c.m = np.zeros(u, dtype=np.int64)
    c.m[:nu] = c.counts
    c.m_col = np.concatenate([to_mont(small_raw(c.m)), filler(n - u, seed + 2)])
    rng = random.Random(seed)
    c.beta = rng.randrange(R)
    return c


def fraction_limbs(cols, table, m_col, beta: int, u: int, absent=()):
    """logup_sets_cases.fraction on every usable row at once: a_j = A_j + beta, s = S + beta, D = s prod_j a_j, N = s sum_j prod_{m != j}
    a_m - M prod_j a_j.  An absent input (row, column) adds nothing: its row's fraction is the one of the other columns.  Asserts that
    no a_j and no s is zero.  -> (N, D) as Montgomery words"""
    a = [_fv(col[:u]) + beta for col in cols]
    s = _fv(table[:u]) + beta
    assert all(nonzero_rows(v.a) for v in a + [s]), "A + beta or S + beta is zero on a usable row"
    m = _fv(m_col[:u])

    def product(factors):
        out = None
        for v in factors:
            out = v if out is None else out * v
        return FV.full(u, 1) if out is None else out

    prod, total = product(a), None
    for j in range(len(a)):
        others = product(v for i, v in enumerate(a) if i != j)
        total = others if total is None else total + others
    num, den = s * total - m * prod, s * prod
    for row in sorted({row for row, _ in absent}):
        num.a[row], den.a[row] = fraction_row(cols, table, m_col, beta, row, absent)
    return num.a, den.a


def fraction_row(cols, table, m_col, beta: int, row: int, absent=()):
    """logup_sets_cases.fraction of one row in Python integers, over the columns whose input on that row is present -> (N, D) as
    Montgomery words"""
    ints = lambda limbs: o.unpack(limbs[row:row + 1], R)[0]
    nr, dr = logup_sets_cases.fraction([ints(c) for j, c in enumerate(cols) if (row, j) not in absent], ints(table), ints(m_col), beta)
    return mont_of(nr), mont_of(dr)


def sum_violation(phi, num, den, u: int):
    """phi: at least u + 1 rows of Montgomery words.  -> None when every word is canonical, phi[0] = 0 and (phi[i + 1] - phi[i]) D_i =
    N_i on every usable row; else the first violation in words.  With no D_i zero (fraction_limbs asserts it) that fixes every row"""
    phi = np.asarray(phi, dtype=np.uint64).reshape(-1, 4)
    if not canonical(phi[: u + 1]):
        return "a value at or above the modulus"
    if phi[0].any():
        return "row 0 is not zero"
    assert nonzero_rows(den)
    step = _fv(phi[1 : u + 1]) - _fv(phi[:u])
    bad = np.nonzero(((step * _fv(den)).a != num).any(axis=1))[0]
    if len(bad):
        return f"{len(bad)} rows do not follow from the row before, the first is row {int(bad[0]) + 1}"
    return None


def bumped(c, num, row: int = 0):
    """-> (the M column with one multiplicity raised by one, so that it no longer belongs to the inputs; the numerators for it: only
    that row's fraction changes)"""
    m_col, num = c.m_col.copy(), num.copy()
    m_col[row] = to_mont(small_raw([int(c.m[row]) + 1]))[0]
    num[row] = fraction_row(c.cols, c.table, m_col, c.beta, row, c.absent)[0]
    return m_col, num


def ranked(c):
    """the key's view of the case's table and the ranking in it -> sorted (canonical words ascending), first (the lowest row of each),
    counts (by rank), ranks (per column, u entries; an absent input's is -1)"""
    canon = from_mont(c.values)
    order = np.lexsort((canon[:, 0], canon[:, 1], canon[:, 2], canon[:, 3]))
    rank_of = np.empty(c.nu, dtype=np.int64)
    rank_of[order] = np.arange(c.nu)
    ranks = [np.where(p, rank_of[a[: c.u]], -1) for a, p in zip(c.a_idx, c.present)]
    return types.SimpleNamespace(sorted=np.ascontiguousarray(canon[order]), first=order.astype(np.uint32), counts=c.counts[order].astype(np.uint32), ranks=ranks)


# ---- Kate division ----------------------------------------------------------------------------------------------------------------------
def kate_roots(size: str, m: int):
    rng = random.Random(_seed("kate roots", size, m))
    if m == 1:
        return [1] if size == "C-short" else [R - 1]
    rest = [rng.randrange(2, R - 1) for _ in range(m - 2)]
    return rest[:1] + [1, R - 1] + rest[1:]


def kate_case(size: str, m: int, n: int = None, roots=None):
    """a numerator Q prod_i (X - r_i) of n coefficients, Q uniform of n - m: the quotient by all m roots is Q and the remaining m - 1
    coefficients of the n - 1 the division writes are zero.  -> n, m, roots, weights (the partial fractions'), num, want (n - 1 words)"""
    n = SIZES[size] if n is None else n
    roots = kate_roots(size, m) if roots is None else roots
    q = o.random_field_limbs(n - m, _seed("kate", size, n, m))
    num = _fv(q).padded(n)
    for r in roots:  # times (X - r): the top coefficient is zero before every step, so the rotation shifts
        num = num.roll(-1) - num * r
    want = _fv(q).padded(n - 1).a
    return types.SimpleNamespace(name=f"{size}, m = {m}", n=n, m=m, roots=roots, weights=extreme_cases.partial_fraction_weights(roots), num=num.a, want=want)


def extreme_words(pattern: str, n: int) -> np.ndarray:
    """extreme_cases.vector("words", pattern, n) as a limb array made with numpy: raw memory words, as the kernels take them"""
    words = o.pack(extreme_cases.EXTREME_WORDS)
    if pattern == "all r - 1":
        return np.ascontiguousarray(np.broadcast_to(words[0], (n, 4)))
    assert pattern == "random choice"
    return np.ascontiguousarray(words[_indices(n, _seed("extreme words", n), len(words))])


def kate_multi_reference(num, roots) -> np.ndarray:
    """the kernel's stated definition on memory words: sum_i c_i N / (X - r_i), every division the C oracle's (remainder dropped)
    -> n - 1 words"""
    acc = FV.zeros(len(num))
    for c, r in zip(extreme_cases.partial_fraction_weights(roots), roots):
        acc = acc + _fv(num).kate_division(r) * c
    return acc.a[: len(num) - 1]


# ---- the GWC witness polynomials -------------------------------------------------------------------------------------------------------
GWC_CAP = 72  # GWC_TERMS (csrc/h2mi_poly.hip)
GWC_CASES = {
    "B-min": dict(terms=[3, 1, GWC_CAP, 2, GWC_CAP + 1], roots=["r", 1, "r", R - 1, "r"], shared=[0, 2, 4], n_pool=12),
    "C-short": dict(terms=[2, 2], roots=["r", R - 1], shared=[0, 1], n_pool=3),
}


def gwc_case(size: str, n: int = None):
    """groups of terms over a pool of shared polynomials, indexed as tests/test_gpu_gwc.py's KERNEL_CASES are: a group's terms cycle
    through the pool from its own offset, term 0 of a `shared` group is pool polynomial 0.  -> n, terms, roots, pool (limb arrays), index,
    scalars (per group)"""
    spec = GWC_CASES[size]
    n = SIZES[size] if n is None else n
    seed = _seed("gwc", size, n)
    rng = random.Random(seed)
    terms, n_pool = spec["terms"], spec["n_pool"]
    c = types.SimpleNamespace(name=size, n=n, terms=terms, roots=[rng.randrange(2, R - 1) if r == "r" else r for r in spec["roots"]])
    c.pool = [o.random_field_limbs(n, seed + 1 + i) for i in range(n_pool)]
    c.index = [[(0 if j == 0 and g in spec["shared"] else (3 * g + j) % n_pool) for j in range(t)] for g, t in enumerate(terms)]
    c.scalars = [[rng.randrange(R) for _ in range(t)] for t in terms]
    return c


def gwc_reference(c):
    """per group the linear combination, then the C oracle's division by (X - root): n words, coefficient n - 1 zero"""
    out = []
    for g in range(len(c.terms)):
        acc = FV.zeros(c.n)
        for i, s in zip(c.index[g], c.scalars[g]):
            acc = acc + _fv(c.pool[i]) * s
        out.append(acc.kate_division(c.roots[g]).a)
    return out


# ---- key-file compaction ---------------------------------------------------------------------------------------------------------------
class DenseSmall:
    """a column given as an array of small non-negative integers on rows 0 .. len - 1 (zeros allowed), for columns of half a million
    cells: its device words and what the compaction must make of it come from numpy, not from a dict"""

    def __init__(self, ints):
        self.ints = np.asarray(ints, dtype=np.uint64)
        assert int(self.ints.max()) <= K.I64_MAX

    def limbs(self, n_rows: int) -> np.ndarray:
        out = np.zeros((n_rows, 4), dtype=np.uint64)
        out[: len(self.ints)] = to_mont(small_raw(self.ints))
        return out

    def cells(self) -> dict:
        return {r: int(v) for r, v in enumerate(self.ints) if v}

    def expect(self, limit: int, flags: int = 0):
        """key_file_cases.expect of self.cells(), for the layouts a column of small integers can take without a forced flag"""
        assert flags == 0
        v = self.ints[:limit]
        rows = np.nonzero(v)[0]
        count, last = len(rows), int(rows[-1]) + 1
        layout = K.layout_of(count, last, 8)
        if layout == K.DENSE:
            return (count, last, 1, layout, 8, None, v[:last].astype("<u8").tobytes())
        return (count, last, 1, layout, 8, rows.tolist(), v[rows].astype("<u8").tobytes())


def cells_limit(tiles: int) -> int:
    return tiles * TILE - 6


def tile_end_rows(tiles: int):
    """the first and the last row of tiles 0, 255, 256, 257 and the last tile, as far as the column has them and below its limit"""
    limit = cells_limit(tiles)
    rows = {r for t in (0, 255, 256, 257, tiles - 1) if t < tiles for r in (t * TILE, t * TILE + TILE - 1)}
    return sorted(r for r in rows | {limit - 1} if r < limit)


def cell_patterns(tiles: int):
    """name -> column ({row: value} or DenseSmall) over tiles * TILE rows of which cells_limit(tiles) are read"""
    limit = cells_limit(tiles)
    rng = random.Random(_seed("cells", tiles))
    ends = tile_end_rows(tiles)
    sparse37 = {t * TILE + (131 * t) % TILE: rng.randrange(1, 1 << 40) for t in range(0, tiles, 37)}
    run = (np.arange(limit, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 20)
    run[::5] = 0  # zeros inside the run travel as zeros
    run[limit - 1] = 7
    return {
        "tile_ends": {r: rng.randrange(1, 1 << 62) for r in ends},
        "tile_ends_wide": {r: rng.randrange(1 << 64, R - (1 << 64)) for r in ends},
        "every_37th_tile": sparse37,
        "dense_small": DenseSmall(run),
        "wide_in_the_last_tile": {**sparse37, limit - 3: R - (1 << 63) - 1},
    }
