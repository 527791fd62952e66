"""Inputs and references for the permutation argument's grand products in every regime of perm_products() (csrc/h2mi_plonk.hip),
shared by tests/test_gpu_permutation.py (the device against the references here) and tests/test_perm_scale_host.py (the generator and
the references against each other: that every case reaches what it is named for).

What the sizes reach.  With a position list (plonk.ActiveRows) of n_active <= 256 entries one workgroup does everything
(k_perm_sparse_small); above that the numerators / denominators, three multiplicative scans in tiles of 1024 and one inversion run over
the list ("general" form), and without a list — or with one that holds more than an eighth of the sets * usable_rows positions — over
every position ("dense" form).  A scan of more than one tile launches k_mulscan_offsets, whose 1024 threads each own a run of
per = ceil(tiles / 1024) tiles: per >= 2 needs more than 2^20 scanned elements.

Two references.  `formula_products`: plonk/permutation/prover.rs row by row in Python integers, for k <= 13.  `recurrence_violation`:
for the case beyond 2^20 elements, the statement z_0[0] = 1, z_s[i + 1] den_s[i] = z_s[i] num_s[i], z_(s+1)[0] = z_s[u] checked with the
C oracle's vector field operations on Montgomery limbs — with no denominator zero it determines every row, so it is equality with the
row-by-row construction and not a weaker statement.
Everything is seeded from the case's name."""
import functools
import random
import types
import zlib

import numpy as np

from oracle import bn254 as o
from oracle import cref
from oracle.plonk import BLINDING_FACTORS, FR_DELTA

R = o.R
SENTINEL = 0xDEAD
MS_TILE, OFFSET_THREADS, SMALL_MAX = 1024, 1024, 256  # the scans' tile, k_mulscan_offsets' workgroup, PERM_SMALL_MAX


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


@functools.lru_cache(maxsize=None)
def identity(k: int, m: int):
    """the identity permutation's columns: delta^j omega^i (cached: read, never written)"""
    w = o.omega_for(k)
    wp = [1] * (1 << k)
    for i in range(1, 1 << k):
        wp[i] = wp[i - 1] * w % R
    return [[pow(FR_DELTA, j, R) * x % R for x in wp] for j in range(m)]


# ---- reference 1: row by row -----------------------------------------------------------------------------------------------------------
def formula_products(k: int, u: int, chunk: int, vals, sig, beta: int, gamma: int, ident=None, sentinel: int = SENTINEL):
    """plonk/permutation/prover.rs in Python integers: per set of `chunk` columns z[0] = the previous set's z[u] (one for the first),
    z[i + 1] = z[i] prod_j (v_j[i] + beta delta^j omega^i + gamma) / prod_j (v_j[i] + beta sigma_j[i] + gamma) for i < u; the rows
    beyond u hold `sentinel`.  -> one column of 2^k integers per set"""
    n, m = 1 << k, len(vals)
    ident = identity(k, m) if ident is None else ident
    want, start = [], 1
    for s in range(-(-m // chunk)):
        z = [sentinel] * n
        z[0] = start
        for i in range(u):
            num = den = 1
            for j in range(s * chunk, min(m, (s + 1) * chunk)):
                num = num * ((vals[j][i] + beta * ident[j][i] + gamma) % R) % R
                den = den * ((vals[j][i] + beta * sig[j][i] + gamma) % R) % R
            z[i + 1] = z[i] if num == den else z[i] * num % R * pow(den, -1, R) % R  # raises on a zero denominator
        start = z[u]
        want.append(z)
    return want


# ---- reference 2: the recurrence, on Montgomery limbs ---------------------------------------------------------------------------------
def _mul(a, b):
    return cref.field_op(1, 0, a, b)


def _add(a, b):
    return cref.field_op(1, 1, a, b)


def _const(v: int, count: int) -> np.ndarray:
    return np.tile(mont_limbs([v]), (count, 1))


def identity_limbs(k: int, m: int):
    """`identity` as limb vectors: omega^i by doubling, pows[2^j : 2^(j+1)] = pows[: 2^j] * omega^(2^j)"""
    n, w = 1 << k, o.omega_for(k)
    pows = np.zeros((n, 4), dtype=np.uint64)
    pows[0] = mont_limbs([1])[0]
    for j in range(k):
        h = 1 << j
        pows[h : 2 * h] = _mul(pows[:h], _const(pow(w, h, R), h))
    return [pows if j == 0 else _mul(pows, _const(pow(FR_DELTA, j, R), n)) for j in range(m)]


def _limbs(col) -> np.ndarray:
    return col if isinstance(col, np.ndarray) else mont_limbs(col)


def factors(case):
    """per set (num, den): u-element limb vectors of prod_j (v_j + beta delta^j omega^i + gamma) and prod_j (v_j + beta sigma_j + gamma)"""
    u = case.u
    ident = identity_limbs(case.k, case.m)
    beta, gamma = _const(case.beta, u), _const(case.gamma, u)
    out = []
    for s in range(case.sets):
        num = den = None
        for j in range(s * case.chunk, min(case.m, (s + 1) * case.chunk)):
            vg = _add(_limbs(case.vals[j])[:u], gamma)
            nf, df = _add(vg, _mul(ident[j][:u], beta)), _add(vg, _mul(_limbs(case.sig[j])[:u], beta))
            num, den = (nf, df) if num is None else (_mul(num, nf), _mul(den, df))
        out.append((num, den))
    return out


def zero_denominators(case, fac=None) -> int:
    return sum(int((~den.any(axis=1)).sum()) for _, den in (factors(case) if fac is None else fac))


def canonical(arr) -> bool:
    """every element's limbs, read as an integer, are below the modulus"""
    arr = np.asarray(arr, dtype=np.uint64).reshape(-1, 4)
    lt, eq = np.zeros(len(arr), dtype=bool), np.ones(len(arr), dtype=bool)
    for w in (3, 2, 1, 0):
        word = np.uint64((R >> (64 * w)) & 0xFFFFFFFFFFFFFFFF)
        lt |= eq & (arr[:, w] < word)
        eq &= arr[:, w] == word
    return bool(lt.all())


def recurrence_violation(case, zs, fac=None):
    """zs: per set a limb array of at least u + 1 rows.  -> None when z_0[0] = 1, every row follows from the one before and every set
    starts from the value the one before ends with; else the first violation in words.  Asserts that no denominator is zero: with
    that, the three statements fix every row."""
    u = case.u
    fac = factors(case) if fac is None else fac
    assert zero_denominators(case, fac) == 0
    one = mont_limbs([1])[0]
    for s, (num, den) in enumerate(fac):
        z = np.asarray(zs[s], dtype=np.uint64).reshape(-1, 4)
        if not canonical(z[: u + 1]):
            return f"set {s}: a value at or above the modulus"
        start = one if s == 0 else np.asarray(zs[s - 1], dtype=np.uint64).reshape(-1, 4)[u]
        if not np.array_equal(z[0], start):
            return f"set {s}: row 0 is not " + ("one" if s == 0 else f"row {u} of set {s - 1}")
        bad = np.nonzero((_mul(z[1 : u + 1], den) != _mul(z[:u], num)).any(axis=1))[0]
        if len(bad):
            return f"set {s}: {len(bad)} rows do not follow from the row before, the first is row {int(bad[0]) + 1}"
    return None


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
SPARSE = dict(k=13, m=4, chunk=2, u=usable(13))  # n_active * 8 <= 2 * 8186 holds up to 2046
SMALL_COUNTS = (1, 2, 63, 64, 65, 255, 256)
GENERAL_COUNTS = (257, 1023, 1024, 1025, 2046)
FALLBACK_COUNT = 2047  # a list the plonk.permutation_products wrapper must not hand on
REAL_COUNTS = (256, 2046, 2047)  # one per regime: cycles of cells with equal values, the last z[u] is one
ADJACENT_ROW = 100
BIG_U = 261939  # 5 * 261939 = 1309695 elements: 1279 tiles (the last of 1023 elements), per = 2, 640 owning threads, the last with one tile


def _sparse_name(count: int) -> str:
    return f"sparse, n_active = {count}"


def _cases():
    form = lambda c: "small" if c <= SMALL_MAX else "general" if c != FALLBACK_COUNT else "dense"
    out = {_sparse_name(c): dict(SPARSE, n_active=c, form=form(c), real=c in REAL_COUNTS) for c in SMALL_COUNTS + GENERAL_COUNTS + (FALLBACK_COUNT,)}
    dense = {
        "dense, more than 1024 tiles (k = 18)": dict(k=18, m=5, chunk=1, u=BIG_U, big=True),
        "dense, 64 columns (k = 6)": dict(k=6, m=64, chunk=7, u=usable(6)),  # ten sets, the last with one column
        "dense, one set (k = 11)": dict(k=11, m=3, chunk=5, u=usable(11), real=True),
        "dense, usable_rows = 1 (k = 1)": dict(k=1, m=2, chunk=1, u=1),
        "dense, usable_rows = 1 (k = 6)": dict(k=6, m=3, chunk=2, u=1),
        "dense, usable_rows = 2^k - 1 (k = 10)": dict(k=10, m=3, chunk=2, u=1023),
    }
    for name, c in dense.items():
        out[name] = dict(dict(n_active=None, form="dense", real=False, big=False), **c)
    return out


PRODUCT_CASES = _cases()
SINGLE_SET_CASE = dict(k=11, m=3, chunk=2, u=1025, n_active=None, form="dense", real=False)  # h2mi_plonk_permutation_product_dev, set by set


def pattern_positions(u: int, sets: int):
    """what every non-trivial list holds: row 0 and row u - 1 of set 0 and of the last set, two adjacent rows, one row in two sets"""
    last = (sets - 1) * u
    return [0, u - 1, last, last + u - 1, ADJACENT_ROW, ADJACENT_ROW + 1, last + ADJACENT_ROW]


def _positions(count: int, u: int, sets: int, rng):
    if count == 1:
        return [u - 1]  # the row whose ratio the next set starts from
    if count == 2:
        return [u - 1, u]
    fixed = pattern_positions(u, sets)
    assert count >= len(fixed) == len(set(fixed))
    rest = [p for p in rng.sample(range(sets * u), count + len(fixed)) if p not in fixed][: count - len(fixed)]
    return sorted(fixed + rest)


def scan_shape(case):
    """-> (elements the scans run over, tiles, k_mulscan_offsets' run length, its threads that own a run)"""
    total = case.sets * case.u if case.form == "dense" else len(case.active)
    tiles = -(-total // MS_TILE)
    per = -(-tiles // OFFSET_THREADS)
    return total, tiles, per, -(-tiles // per)


def expected_launches(case) -> dict:
    """kernel -> launches of one permutation_products call in the case's form"""
    _, tiles, _, _ = scan_shape(case)
    if case.form == "small":
        return {"k_perm_sparse_small": 1, "k_mulscan_local": 0}
    if case.form == "general":
        return {"k_perm_sparse_small": 0, "k_perm_to_mont256": 1, "k_mulscan_offsets": 3 if len(case.active) > MS_TILE else 0}
    return {"k_perm_to_mont256": 0, "k_mulscan_offsets": 3 if tiles > 1 else 0, "k_perm_numden_sets": 1}


def _cycles(cells, rng):
    """the cells in cycles of two, one of three when their count is odd"""
    cells = list(cells)
    rng.shuffle(cells)
    head = [cells[:3]] if len(cells) % 2 else []
    rest = cells[3:] if head else cells
    return head + [rest[i : i + 2] for i in range(0, len(rest), 2)]


def _big_case(case):
    """columns as limb vectors: uniform values; sigma_j = c_j * value_(j+1) on three rows of four, the identity on the others"""
    k, n, m, seed = case.k, case.n, case.m, zlib.crc32(case.name.encode())
    case.vals = [o.random_field_limbs(n, seed + j) for j in range(m)]
    ident = identity_limbs(k, m)
    rng = _rng("big", case.name)
    case.sig = []
    for j in range(m):
        moved = o.splitmix64_np(np.arange(n, dtype=np.uint64), seed + 100 + j) % np.uint64(4) != 0
        case.sig.append(np.where(moved[:, None], _mul(case.vals[(j + 1) % m], _const(rng.randrange(1, R), n)), ident[j]))
    case.beta, case.gamma = rng.randrange(R), rng.randrange(R)
    return case


def product_case(name: str, spec: dict = None):
    """-> k, n, u, m, chunk, sets, vals / sig (m columns of 2^k integers; limb vectors when `big`), beta, gamma, active (the sorted
    positions set * u + row, or None), form ("small" | "general" | "dense"), real.
    At a position of the list at least one column of its set gets a sigma other than the identity — a random value: the kernels
    compute a formula and do not care that sigma is a permutation; `real` cases move the cells in cycles of equal values instead.
    Off the list every column of the set keeps the identity.  Without a list ("dense" data) three cells of four are moved."""
    spec = PRODUCT_CASES[name] if spec is None else spec
    case = types.SimpleNamespace(name=name, n=1 << spec["k"], sets=-(-spec["m"] // spec["chunk"]), active=None, big=spec.get("big", False),
                                 **{key: spec[key] for key in ("k", "m", "chunk", "u", "form", "real")})
    if case.big:
        return _big_case(case)
    rng = _rng("perm product", name)
    k, n, u, m, chunk = case.k, case.n, case.u, case.m, case.chunk
    ident = identity(k, m)
    case.vals = [[rng.randrange(R) for _ in range(n)] for _ in range(m)]
    case.sig = [col[:u] + [rng.randrange(R) for _ in range(n - u)] for col in ident]  # beyond the usable rows nothing is read
    columns = lambda pos: range((pos // u) * chunk, min(m, (pos // u + 1) * chunk))
    if spec["n_active"] is not None:
        case.active = _positions(spec["n_active"], u, case.sets, rng)
    positions = case.active if case.active is not None else list(range(case.sets * u))
    if case.real:
        cells = [(columns(pos)[idx % len(columns(pos))], pos % u) for idx, pos in enumerate(positions)]  # one moved cell per position
        for cycle in _cycles(cells, rng):
            v = rng.randrange(R)
            for (j, i), (jn, i_n) in zip(cycle, cycle[1:] + cycle[:1]):
                case.vals[j][i], case.sig[j][i] = v, ident[jn][i_n]
    else:
        for idx, pos in enumerate(positions):
            cols, i = columns(pos), pos % u
            pick = [cols[0]] if idx % 3 == 0 else [cols[-1]] if idx % 3 == 1 else list(cols)  # the first column, the last, all of them
            for j in pick:
                if case.active is not None or rng.randrange(4):
                    case.sig[j][i] = rng.randrange(R)
    case.beta, case.gamma = rng.randrange(R), rng.randrange(R)
    return case


def single_set_case():
    return product_case("single-set entry, usable_rows = 1025 (k = 11)", SINGLE_SET_CASE)


def moved_positions(case):
    """the positions at which some column of the set differs from the identity, read off sigma (integer cases)"""
    ident = identity(case.k, case.m)
    return sorted({(j // case.chunk) * case.u + i for j in range(case.m) for i in range(case.u) if case.sig[j][i] != ident[j][i]})


# ---- proofs: check_cases.copies_circuit(custom, k, cycles) — four equality columns, chunks of one, four sets --------------------------
# (k, cycles) -> (n_active as keygen computes it, the form the prover's rule n_active * 8 <= n_sets * u then takes)
PROOF_CASES = {
    (11, 60): (203, "small"),
    (11, 82): (275, "general"),     # one tile
    (11, 311): (1019, "general"),   # the last cycle count under the rule
    (11, 312): (1022, "dense"),     # the first over it
    (13, 700): (2283, "general"),   # three tiles
}


def proof_positions(cs, asg, k: int):
    """plonk.ActiveRows' rule on an assignment's copy constraints: every cell of a cycle of two or more cells is moved by the
    permutation; its position is (column's index in the argument // chunk) * usable_rows + row.  -> (sorted positions, u, sets, chunk)"""
    chunk = cs.degree() - 2
    u = (1 << k) - (cs.blinding_factors() + 1)
    index = {col: j for j, col in enumerate(cs.perm_columns)}
    parent = {}

    def find(c):
        parent.setdefault(c, c)
        while parent[c] != c:
            parent[c] = parent[parent[c]]
            c = parent[c]
        return c

    for left, right in asg.copies:
        parent[find(left)] = find(right)
    size = {}
    for c in parent:
        size[find(c)] = size.get(find(c), 0) + 1
    moved = [c for c in parent if size[find(c)] >= 2]
    pos = sorted({(index[(kind, col)] // chunk) * u + row for kind, col, row in moved if row < u})
    return pos, u, -(-len(cs.perm_columns) // chunk), chunk
