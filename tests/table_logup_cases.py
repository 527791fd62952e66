"""LogUp against a table sorted at keygen, shared by tests/test_table_logup_host.py and tests/test_gpu_table_logup.py: the ranks, the
joint histogram, the multiplicity column and the running sum BY RANK in Python integers (h2mi_plonk_logup_rank_cols_dev /
h2mi_plonk_logup_sum_ranked_dev), and the named inputs of the kernel tests, each with a function that states what it is
named for.  The argument itself is tests/logup_sets_cases.py's: the host test checks these numbers against that file's."""
import random

from oracle import bn254 as o

R = o.R
LK_SLOTS = 64  # csrc/h2mi_lookup.hip: the workgroup's LDS table of ranks
RANK_WORKGROUP = 1024
MAX_LOGUP_INPUTS = 6
# (k, usable rows): one workgroup of the ranking kernel; two, the last wavefront ragged; eight
SIZES = [(10, (1 << 10) - 6), (11, (1 << 11) - 6), (13, (1 << 13) - 6)]
KINDS = ["zeros", "distinct", "collide", "arbitrary", "repeats", "padzero", "absent"]


# ---- the two calls in Python integers -------------------------------------------------------------------------------------------------
def table_data(s_rows, u: int):
    """the key's view of a fixed table -> (the distinct values of its usable rows ascending, first[r]: the lowest usable row holding
    distinct value r)"""
    first = {}
    for r in range(u):
        first.setdefault(s_rows[r], r)
    values = sorted(first)
    return values, [first[v] for v in values]


def rank_columns(cols, values, u: int):
    """-> (ranks[j][i] for i < u, None for an input that is no table value; the joint histogram; the absent (row, column) pairs)"""
    rank_of = {v: r for r, v in enumerate(values)}
    ranks, counts, absent = [], [0] * len(values), []
    for j, col in enumerate(cols):
        rk = [rank_of.get(col[i]) for i in range(u)]
        for i, r in enumerate(rk):
            if r is None:
                absent.append((i, j))
            else:
                counts[r] += 1
        ranks.append(rk)
    return ranks, counts, absent


def m_column(counts, first, u: int):
    m = [0] * u
    for c, row in zip(counts, first):
        m[row] = c
    return m


def ranked_sum(ranks, values, counts, first, beta: int, u: int):
    """-> phi[0 .. u] the way the device forms it: T[r] = 1 / (values[r] + beta), row i adds sum_j T[rank_j[i]], row first[r] subtracts
    counts[r] T[r]; an absent input (None) adds nothing"""
    T = [pow((v + beta) % R, -1, R) for v in values]
    term = [0] * u
    for rk in ranks:
        for i in range(u):
            if rk[i] is not None:
                term[i] += T[rk[i]]
    for r, row in enumerate(first):
        term[row] -= counts[r] * T[r]
    phi = [0]
    for t in term:
        phi.append((phi[-1] + t) % R)
    return phi


# ---- named inputs ---------------------------------------------------------------------------------------------------------------------
def kernel_input(kind: str, K: int, u: int, rng: random.Random):
    """-> (K input columns of u rows, u table rows).  The table rows beyond what a kind declares are its padding zeros, as a fixed table
    column's are."""
    pad = lambda rows: rows + [0] * (u - len(rows))
    if kind == "zeros":  # every usable row of every column zero, a range table: one rank across wavefronts, workgroups and columns
        return [[0] * u for _ in range(K)], pad(list(range(256)))
    if kind == "distinct":  # a range table as long as the rows and every row of a column another rank; the guess hits
        return [[(i + 17 * (j + 1)) % u for i in range(u)] for j in range(K)], list(range(u))
    if kind == "collide":  # a range table; ranks equal modulo LK_SLOTS, so all but the first comer miss their LDS slot
        ranks = list(range(5, 960, LK_SLOTS))
        return [[rng.choice(ranks) for _ in range(u)] for _ in range(K)], pad(list(range(960)))
    if kind == "arbitrary":  # uniform 254-bit table values in no order: the guess misses and the binary search runs
        table = [rng.randrange(1 << 64, R) for _ in range(u)]
        return [[rng.choice(table) for _ in range(u)] for _ in range(K)], table
    if kind == "repeats":  # a table with repeated values: first[r] != r; and values no input takes
        pool = [rng.randrange(R) for _ in range(max(3, u // 3))]
        table = [rng.choice(pool) for _ in range(u)]
        used = [v for v in table if v != pool[0]] or table
        return [[rng.choice(used) for _ in range(u)] for _ in range(K)], table
    if kind == "padzero":  # the declared table is 1 .. 300; its zero exists through the padding rows alone, and most inputs are zero
        return [[rng.randrange(1, 301) if rng.randrange(8) == 0 else 0 for _ in range(u)] for _ in range(K)], pad(list(range(1, 301)))
    assert kind == "absent"  # ONE input that is no table value: the last usable row (the last wavefront of the last workgroup), last column
    cols, table = kernel_input("repeats", K, u, rng)
    cols[K - 1][u - 1] = next(v for v in iter(lambda: rng.randrange(R), None) if v not in set(table))
    return cols, table


def guess_hits(v: int, values) -> bool:
    """lk_rank_body's first try: is the table value at index min(low 32 bits of v, n_unique - 1) the input itself?"""
    return values[min(v & 0xFFFFFFFF, len(values) - 1)] == v


def reaches(kind: str, cols, table, u: int) -> bool:
    """does the input exercise what it is named for?"""
    values, first = table_data(table, u)
    ranks, counts, absent = rank_columns(cols, values, u)
    flat = [r for rk in ranks for r in rk]
    everywhere = all(guess_hits(col[i], values) for j, col in enumerate(cols) for i in range(u) if ranks[j][i] is not None)
    if kind == "zeros":
        return set(flat) == {0} and counts[0] == len(cols) * u and everywhere
    if kind == "distinct":
        return all(sorted(rk) == list(range(u)) for rk in ranks) and len(values) == u and everywhere
    if kind == "collide":
        group = ranks[0][:RANK_WORKGROUP]
        return len({r % LK_SLOTS for r in flat}) == 1 and len(set(group)) > 1 and everywhere
    if kind == "arbitrary":
        return not any(guess_hits(col[i], values) for col in cols for i in range(u) if col[i] != values[-1]) and table != sorted(table)
    if kind == "repeats":
        return any(f != r for r, f in enumerate(first)) and 0 in counts and len(values) < u
    if kind == "padzero":
        return values[0] == 0 and first[0] == 300 and table[:300] == list(range(1, 301)) and counts[0] > u // 2 and everywhere
    assert kind == "absent"
    K = len(cols)
    return absent == [(u - 1, K - 1)] and u % 64 != 0 and sum(counts) == K * u - 1
