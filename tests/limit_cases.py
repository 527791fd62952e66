"""Satisfiable circuits AT the limits of the prover ABI, shared by tests/test_limits_host.py and tests/test_gpu_limits.py: every
count the headers allow a constraint system to hold (include/h2mi.h, include/h2mi_prover.h: 64 advice / fixed / permutation columns, 8
lookups of up to 6 logUp input sets, 8 shuffles, 16 challenges in 3 phases, 8 circuits per proof, 4096 ops / 256 constants / stack
depth 8) is reached by one shape here, and so are the sizes at which the prover's host code takes another path without any header
saying so: a rotation set of 5 or more points (kate_chain's chained division), of more than 16 (the head of a remainder goes to the
device in slices), more than 16 and more than 32 opening points (no power-table prefetch; the 64-entry table cache evicts inside one
proof), and a signed range table (sort_unique's full re-sort).  The limits are READ from the headers; every shape asserts that the
count it reaches equals the constant.  Witnesses are satisfiable by construction: a cell a gate constrains is computed from the cells
it reads, selectors are on only where every rotation stays inside the usable rows.

build(custom, name) -> (cs, witness, k, logup): witness an Assignment, a callable synthesize(challenges) -> Assignment, or (batch8) a
list of them, one per circuit; logup: the key to make.  reached(name): what the shape counted, by limit.  plants(name): per argument
kind one advice cell whose change breaks that argument and nothing mock tests before it."""
import os
import random
import re

from oracle import bn254 as o

R = o.R
_INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def header_limits():
    """every `#define H2MI_<NAME> <number or other name>` of the two headers, resolved to integers"""
    text = "".join(open(os.path.join(_INCLUDE, f)).read() for f in ("h2mi.h", "h2mi_prover.h"))
    raw = dict(re.findall(r"#define (H2MI_\w+) (\w+)", text))
    out = {}
    for name, val in raw.items():
        while val in raw:
            val = raw[val]
        if val.isdigit():
            out[name] = int(val)
    return out


_H = header_limits()
LIMITS = {short: _H["H2MI_" + short] for short in (
    "MAX_ADVICE", "MAX_FIXED", "MAX_PERM", "MAX_LOOKUPS", "MAX_LOGUP_INPUTS", "MAX_SHUFFLES", "MAX_CHALLENGES", "MAX_ADVICE_PHASES", "MAX_QUERIES",
    "MAX_CIRCUITS", "MAX_EXPR_OPS", "MAX_EXPR_CONSTANTS", "MAX_EXPR_STACK")}
PUBLIC_INPUTS = 16  # the instance column's values travel as kernel arguments (h2mi_plonk_instance_coset_dev): 16 at most
HEAD_SLICE = 16     # and so do the coefficients h2mi_fr_add_head_dev adds
_REACHED, _PLANTS = {}, {}


def _total(terms):
    e = terms[0]
    for t in terms[1:]:
        e = e + t
    return e


def usable_rows(cs, k: int) -> int:
    return (1 << k) - (cs.blinding_factors() + 1)


# ---- wide: every column table full ---------------------------------------------------------------------------------------------------
def wide_circuit(custom):
    """k = 6, degree 3 (one permutation column per set): 64 advice columns, all in the permutation argument; 61 fixed columns and 3
    selectors (fixed column 63 is the last selector); one instance column with 16 public inputs.  Gates: q0 (a63 a62 - a0), q1 (sum_j
    f_j a_j - a63) over every user fixed column, q2 (a0 - instance) on the public rows.  Copies chain a_j -> a_(j+1) through all 64
    columns and close from a63 back to a0."""
    A, F = LIMITS["MAX_ADVICE"], LIMITS["MAX_FIXED"]
    meta = custom.ConstraintSystem()
    adv = [meta.advice_column() for _ in range(A)]
    fix = [meta.fixed_column() for _ in range(F - 3)]
    inst = meta.instance_column()
    q_prod, q_dot, q_pub = meta.selector(), meta.selector(), meta.selector()
    for c in adv:
        meta.enable_equality(c)
    cur = custom.Rotation.cur()
    qa = lambda m, j: m.query_advice(adv[j], cur)
    meta.create_gate("product", lambda m: [m.query_selector(q_prod) * (qa(m, A - 1) * qa(m, A - 2) - qa(m, 0))])
    meta.create_gate("dot", lambda m: [m.query_selector(q_dot) * (_total([m.query_fixed(f, cur) * qa(m, j) for j, f in enumerate(fix)]) - qa(m, A - 1))])
    meta.create_gate("public", lambda m: [m.query_selector(q_pub) * (qa(m, 0) - m.query_instance(inst, cur))])
    rng = random.Random(6401)
    public = [rng.randrange(R) for _ in range(PUBLIC_INPUTS)]
    region = custom.Assignment(meta, instance=public)
    val = lambda: rng.choice([0, 1, R - 1]) if rng.random() < 0.2 else rng.randrange(R)
    rows = {"public": range(0, 16), "product": range(16, 26), "dot": range(26, 36)}
    a = [[val() for _ in range(40)] for _ in range(A)]
    f = [[val() for _ in range(40)] for _ in range(F - 3)]
    for r in rows["public"]:
        a[0][r] = public[r]
        region.enable_selector(q_pub, r)
    for r in rows["product"]:
        a[0][r] = a[A - 1][r] * a[A - 2][r] % R
        region.enable_selector(q_prod, r)
    for r in rows["dot"]:
        a[A - 1][r] = sum(f[j][r] * a[j][r] for j in range(F - 3)) % R
        region.enable_selector(q_dot, r)
    cells = {}
    for j in range(A):
        for r in range(40):
            cells[(j, r)] = region.assign_advice(adv[j], r, a[j][r])
    for j in range(F - 3):
        for r in range(40):
            region.assign_fixed(fix[j], r, f[j][r])
    cell = cells[(0, 20)]
    for j in range(1, A):  # a chain through every permutation column, 63 included
        cell = region.copy_advice(cell, adv[j], 41 + (j & 1))
    region.copy_advice(cells[(A - 1, 30)], adv[0], 43)
    region.copy_advice(cells[(A - 1, 5)], adv[A - 1], 44)
    assert meta.degree() == 3 and len(public) == PUBLIC_INPUTS and meta.selector_column(q_pub) == F - 1
    assert (A - 1, 0) in meta.advice_queries and (F - 1, 0) in meta.fixed_queries and meta.instance_queries == [(0, 0)]
    n_sets = -(-len(meta.perm_columns) // (meta.degree() - 2))
    reached = {"MAX_ADVICE": meta.n_advice, "MAX_FIXED": meta.n_fixed, "MAX_PERM": len(meta.perm_columns), "permutation sets": (n_sets, LIMITS["MAX_PERM"])}
    assert meta.perm_columns[-1] == ("advice", A - 1)
    plants = {"gate": (0, 20, "gate 'product' not satisfied at row 20"), "copy": (5, 42, "copy constraint")}
    return meta, region, reached, plants


# ---- rotations: columns queried at many points ---------------------------------------------------------------------------------------
def rotation_circuit(custom, k: int, runs, fixed_run=None):
    """one advice column per (first rotation, count) of `runs`, each queried at `count` consecutive rotations, and one gate q (sum over
    every such query c_r a_j(w^r X) - b(X)); fixed_run: a fixed column queried at that run too, q (sum d_r f(w^r X) - b2(X)).  b is in
    the permutation argument (degree 3: one set).  Every other column is queried at one rotation.  The selector is on where every
    rotation stays inside the usable rows."""
    meta = custom.ConstraintSystem()
    cols = [meta.advice_column() for _ in runs]
    b = meta.advice_column()
    b2 = meta.advice_column() if fixed_run else None
    f = meta.fixed_column() if fixed_run else None
    q = meta.selector()
    meta.enable_equality(b)
    cur = custom.Rotation.cur()
    rng = random.Random(1700 + 31 * len(runs) + sum(c for _, c in runs))
    coef = [[rng.randrange(1, R) for _ in range(count)] for _, count in runs]
    fcoef = [rng.randrange(1, R) for _ in range(fixed_run[1])] if fixed_run else []
    terms = lambda m: [m.query_advice(cols[j], custom.Rotation(first + i)) * coef[j][i] for j, (first, count) in enumerate(runs) for i in range(count)]
    meta.create_gate("advice window", lambda m: [m.query_selector(q) * (_total(terms(m)) - m.query_advice(b, cur))])
    if fixed_run:
        meta.create_gate("fixed window", lambda m: [m.query_selector(q) * (_total([m.query_fixed(f, custom.Rotation(fixed_run[0] + i)) * fcoef[i]
                                                                                    for i in range(fixed_run[1])]) - m.query_advice(b2, cur))])
    u = usable_rows(meta, k)
    every = list(runs) + ([fixed_run] if fixed_run else [])
    lo, hi = min(first for first, _ in every), max(first + count - 1 for first, count in every)
    on = range(max(0, -lo), u - max(0, hi))
    assert len(on) >= 8
    region = custom.Assignment(meta)
    a = [[rng.randrange(R) for _ in range(u)] for _ in runs]
    fv = [rng.randrange(R) for _ in range(u)]
    for j, col in enumerate(cols):
        for r in range(u):
            region.assign_advice(col, r, a[j][r])
    if fixed_run:
        for r in range(u):
            region.assign_fixed(f, r, fv[r])
    first_b = None
    for r in on:
        cell = region.assign_advice(b, r, sum(coef[j][i] * a[j][r + first + i] for j, (first, count) in enumerate(runs) for i in range(count)) % R)
        first_b = first_b or cell
        if fixed_run:
            region.assign_advice(b2, r, sum(fcoef[i] * fv[r + fixed_run[0] + i] for i in range(fixed_run[1])) % R)
        region.enable_selector(q, r)
    region.copy_advice(first_b, b, u - 1)  # the selector is off there
    plants = {"gate": (len(runs), on[3], "gate 'advice window' not satisfied at row %d" % on[3]), "copy": (len(runs), u - 1, "copy constraint")}
    return meta, region, plants


def rot_circuit(custom, count: int):
    """k = 6: one advice and one fixed column at rotations 0 .. count - 1: ONE rotation set of `count` points with two members (the
    blinding factors grow to count + 2)"""
    meta, region, plants = rotation_circuit(custom, 6, [(0, count)], fixed_run=(0, count))
    per_column = lambda queries, c: sum(1 for col, _ in queries if col == c)
    assert meta.blinding_factors() == count + 2 and meta.degree() == 3
    reached = {"rotations of advice 0": (per_column(meta.advice_queries, 0), count), "rotations of fixed 0": (per_column(meta.fixed_queries, 0), count)}
    return meta, region, reached, plants


ROT_MANY_RUNS = [(0, 12), (12, 12), (-12, 12)]


def rot_many_circuit(custom):
    """k = 7: three advice columns at the disjoint runs 0 .. 11, 12 .. 23 and -12 .. -1: 36 opening points — with their inverses 72
    power tables, more than the prefetch takes (32) and more than the table cache holds (64)"""
    meta, region, plants = rotation_circuit(custom, 7, ROT_MANY_RUNS)
    points = {r for _, r in meta.advice_queries} | {0, 1}
    assert len(points) > 32 and 2 * len(points) > 64
    return meta, region, {"opening points": (len(points), sum(c for _, c in ROT_MANY_RUNS))}, plants


def opening_sets(cs, logup: bool):
    """the rotation sets of a proof of one circuit, as sets of rotations (-(blinding factors + 1) stands for x_last), in the words of
    the verifiers' query list: per advice / fixed column its queries; Z_s at {0, 1} and, but for the last set, x_last; per lookup phi
    {0, 1} and M {0} (logUp) or Z {0, 1}, A' {0, -1} and S' {0}; per shuffle Z {0, 1}; sigmas, h and the random polynomial at {0}"""
    per = []
    for queries, count in ((cs.advice_queries, cs.n_advice), (cs.fixed_queries, cs.n_fixed)):
        per += [frozenset(r for c, r in queries if c == j) for j in range(count)]
    n_sets = -(-len(cs.perm_columns) // (cs.degree() - 2))
    last = -(cs.blinding_factors() + 1)
    per += [frozenset({0, 1, last}) if s + 1 < n_sets else frozenset({0, 1}) for s in range(n_sets)]
    for _ in cs.lookup_arguments:
        per += [frozenset({0, 1}), frozenset({0})] if logup else [frozenset({0, 1}), frozenset({0, -1}), frozenset({0})]
    per += [frozenset({0, 1})] * len(cs.shuffles) + [frozenset({0})]
    return {s for s in per if s}


def expected_divisions(cs, logup: bool) -> int:
    """launches of the division kernel in one proof: a rotation set of 2 .. 4 points is ONE round of independent divisions, every other
    set one division per point (the chain), and the final opening divides once"""
    return sum(1 if 2 <= len(s) <= 4 else len(s) for s in opening_sets(cs, logup)) + 1


# ---- eight lookups, eight shuffles -----------------------------------------------------------------------------------------------------
def _fill_xor_table(region, cols):
    for i in range(16):
        for tab, v in zip(cols, (i >> 2, i & 3, (i >> 2) ^ (i & 3))):
            region.assign_fixed(tab, i, v)


def _declare_shuffles(meta, custom):
    """MAX_SHUFFLES shuffles over five columns s0 .. s4 (each a permutation of s0 over the usable rows) and p0, p1: seven of one pair
    and, last, the tuple shuffle (s0, p0) against (s1, p1).  -> (columns, fill(region, u, rng))"""
    S = LIMITS["MAX_SHUFFLES"]
    s = [meta.advice_column() for _ in range(5)]
    p0, p1 = meta.advice_column(), meta.advice_column()
    cur = custom.Rotation.cur()
    pairs = [(0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (1, 3), (2, 4), (3, 4), (1, 4), (2, 3)][: S - 1]
    for x, y in pairs:
        meta.shuffle("s%d is s%d permuted" % (x, y), lambda m, x=x, y=y: [(m.query_advice(s[x], cur), m.query_advice(s[y], cur))])
    meta.shuffle("tuples", lambda m: [(m.query_advice(s[0], cur), m.query_advice(s[1], cur)), (m.query_advice(p0, cur), m.query_advice(p1, cur))])

    def fill(region, u, rng):
        vals = [rng.choice([2, 2, 6, R - 2, rng.randrange(R)]) for _ in range(u)]
        tags = [rng.randrange(R) for _ in range(u)]
        for j, col in enumerate(s):
            order = list(range(u))
            if j:
                rng.shuffle(order)
            for row, src in enumerate(order):
                region.assign_advice(col, row, vals[src])
                if j < 2:
                    region.assign_advice((p0, p1)[j], row, tags[src])

    return s + [p0, p1], fill


def args_plain_circuit(custom):
    """k = 6, a plain key: 8 lookups of two- or three-expression tuples — seven in the fixed 2-bit XOR table, the LAST in a table held
    in two advice columns (sorted on the device in every proof) — and 8 shuffles of which the last is a tuple shuffle; a degree-3 gate
    q (a0 a1 - m) and a copy"""
    Lk = LIMITS["MAX_LOOKUPS"]
    meta = custom.ConstraintSystem()
    a = [meta.advice_column() for _ in range(6)]
    t0, t1, m = meta.advice_column(), meta.advice_column(), meta.advice_column()
    ta, tb, tc = (meta.fixed_column() for _ in range(3))
    q = meta.selector()
    meta.enable_equality(m)
    cur = custom.Rotation.cur()
    meta.create_gate("product", lambda mt: [mt.query_selector(q) * (mt.query_advice(a[0], cur) * mt.query_advice(a[1], cur) - mt.query_advice(m, cur))])
    triples = [(0, 1, 2), (3, 4, 5), (1, 0, 2), (0, 1), (3, 4), (4, 3, 5), (2, 0, 1), (5, 4, 3), (2, 1, 0)][: Lk - 1]
    for l, cols in enumerate(triples):
        meta.lookup("xor %d" % l, lambda mt, cols=cols: [(mt.query_advice(a[c], cur), mt.query_fixed(tab, cur)) for c, tab in zip(cols, (ta, tb, tc))])
    meta.lookup_any("advice table", lambda mt: [(mt.query_advice(a[0], cur), mt.query_advice(t0, cur)), (mt.query_advice(a[2], cur), mt.query_advice(t1, cur))])
    _, fill = _declare_shuffles(meta, custom)
    region = custom.Assignment(meta)
    _fill_xor_table(region, (ta, tb, tc))
    rng = random.Random(8008)
    u = usable_rows(meta, 6)
    first = None
    for row in range(40):
        x, y, x2, y2 = (rng.randrange(4) for _ in range(4))
        for col, v in zip(a, (x, y, x ^ y, x2, y2, x2 ^ y2)):
            region.assign_advice(col, row, v)
        cell = region.assign_advice(m, row, x * y)
        first = first or cell
        if row < 30:
            region.enable_selector(q, row)
    for i in range(16):  # the advice table: every (x, z) pair, from row 3 on
        region.assign_advice(t0, 3 + i, i >> 2)
        region.assign_advice(t1, 3 + i, i & 3)
    region.copy_advice(first, m, 45)
    fill(region, u, rng)
    assert all(2 <= len(pairs) <= 3 for pairs in meta.lookups) and meta.degree() == 4
    assert any(len(pairs) > 1 for pairs in meta.shuffles)
    reached = {"MAX_LOOKUPS": len(meta.lookup_arguments), "MAX_SHUFFLES": len(meta.shuffles)}
    plants = {"gate": (8, 4, "gate 'product' not satisfied at row 4"), "copy": (8, 45, "copy constraint"),
              "lookup": (5, 3, "lookup 'xor 1' not satisfied at row 3"), "shuffle": (9 + 4, 2, "shuffle 's0 is s4 permuted' not satisfied")}
    return meta, region, reached, plants


def args_logup_circuit(custom):
    """k = 6, a logUp key, degree 9: 14 lookups over 8 tables merged into 8 arguments — argument 0 with two input sets, argument 2 the
    XOR tuple lookup, argument 7 with SIX input sets (the top nibble of the quotient kernel's packed counts) — and 8 shuffles; a gate
    and a copy"""
    Lk, K = LIMITS["MAX_LOOKUPS"], LIMITS["MAX_LOGUP_INPUTS"]
    meta = custom.ConstraintSystem()
    r = [meta.advice_column() for _ in range(K)]
    a = [meta.advice_column() for _ in range(3)]
    m = meta.advice_column()
    tabs = [meta.fixed_column() for _ in range(Lk - 1)]  # argument 2 reads the XOR table instead
    ta, tb, tc = (meta.fixed_column() for _ in range(3))
    q = meta.selector()
    meta.enable_equality(m)
    cur = custom.Rotation.cur()
    meta.create_gate("product", lambda mt: [mt.query_selector(q) * (mt.query_advice(a[0], cur) * mt.query_advice(a[1], cur) - mt.query_advice(m, cur))])
    one = lambda name, col, tab: meta.lookup(name, lambda mt: [(mt.query_advice(col, cur), mt.query_fixed(tab, cur))])
    one("pair 0", r[0], tabs[0])
    one("pair 1", r[1], tabs[0])
    one("single 1", r[2], tabs[1])
    meta.lookup("xor", lambda mt: [(mt.query_advice(c, cur), mt.query_fixed(t, cur)) for c, t in zip(a, (ta, tb, tc))])
    for l in range(3, Lk - 1):
        one("single %d" % l, r[l % K], tabs[l - 1])
    for j in range(K):
        one("six %d" % j, r[j], tabs[Lk - 2])
    merged = meta.merge_lookups(9)
    _, fill = _declare_shuffles(meta, custom)
    region = custom.Assignment(meta)
    _fill_xor_table(region, (ta, tb, tc))
    rng = random.Random(9009)
    for tab in tabs:  # every table holds 0 .. 7, each in another order; 0 stands on the rows beyond
        order = list(range(8))
        rng.shuffle(order)
        for row, v in enumerate(order):
            region.assign_fixed(tab, row, v)
    first = None
    for row in range(40):
        for col in r:
            region.assign_advice(col, row, rng.choice([0, 3, 3, 7, rng.randrange(8)]))
        x, y = rng.randrange(4), rng.randrange(4)
        for col, v in zip(a, (x, y, x ^ y)):
            region.assign_advice(col, row, v)
        cell = region.assign_advice(m, row, x * y)
        first = first or cell
        if row < 30:
            region.enable_selector(q, row)
    region.copy_advice(first, m, 45)
    fill(region, usable_rows(meta, 6), rng)
    sets = [len(arg) for arg in merged]
    assert sets[0] == 2 and sets[2] == 1 and len(meta.lookups[merged[2][0]]) == 3 and meta.degree() == 9
    reached = {"MAX_LOOKUPS": len(meta.lookup_arguments), "MAX_LOGUP_INPUTS": sets[-1], "MAX_SHUFFLES": len(meta.shuffles)}
    plants = {"gate": (K + 3, 4, "gate 'product' not satisfied at row 4"), "copy": (K + 3, 45, "copy constraint"),
              "lookup": (K - 1, 3, "lookup 'single %d' not satisfied at row 3" % (K - 1)), "shuffle": (K + 4 + 4, 2, "shuffle 's0 is s4 permuted' not satisfied")}
    region.assign_advice(r[K - 1], 3, 7)  # the cell to plant in: 7 + 1 is outside the tables
    return meta, region, reached, plants


# ---- signed: the table the sort has to sort completely --------------------------------------------------------------------------------
SIGNED_BITS = 9


def signed_circuit(custom):
    """k = 11, a logUp key: the signed range -2^9 .. 2^9 - 1 in one fixed column (field elements at BOTH ends of the field: the keys
    differ in more than eight bytes and their 8-byte prefixes tie, so the per-proof sort of the table runs its full re-sort), looked
    up from two advice columns on every assigned row, merged into one argument of two sets.  The inputs are skewed: seven values near
    zero take half of the rows, 300 values the rest, the others are never hit.  A gate q (x + y - s) and a copy."""
    k = 11
    meta = custom.ConstraintSystem()
    x, y, s = meta.advice_column(), meta.advice_column(), meta.advice_column()
    t = meta.fixed_column()
    q = meta.selector()
    meta.enable_equality(s)
    cur = custom.Rotation.cur()
    meta.create_gate("sum", lambda m: [m.query_selector(q) * (m.query_advice(x, cur) + m.query_advice(y, cur) - m.query_advice(s, cur))])
    for name, col in (("x in range", x), ("y in range", y)):
        meta.lookup(name, lambda m, col=col: [(m.query_advice(col, cur), m.query_fixed(t, cur))])
    merged = meta.merge_lookups()
    assert merged == [[0, 1]]
    u = usable_rows(meta, k)
    half = 1 << SIGNED_BITS
    region = custom.Assignment(meta)
    for row, v in enumerate(range(-half, half)):
        region.assign_fixed(t, row, v % R)
    rng = random.Random(1109)
    some = rng.sample(range(-half, half), 300)
    draw = lambda: rng.randrange(-3, 4) if rng.random() < 0.5 else rng.choice(some)
    first = None
    for row in range(u - 2):
        xv, yv = draw(), draw()
        region.assign_advice(x, row, xv % R)
        region.assign_advice(y, row, yv % R)
        cell = region.assign_advice(s, row, (xv + yv) % R)
        first = first or cell
        region.enable_selector(q, row)
    region.copy_advice(first, s, u - 1)
    assert u > 2 * half
    region.assign_advice(x, u - 2, half - 1)  # the cell to plant in: the largest table value, + 1 is outside (no gate on this row)
    values = set(region.fixed[t.index].values())
    assert min(values) == 0 and max(values) == R - 1  # both ends of the field
    reached = {"distinct table values": (len(values), 2 * half)}
    plants = {"gate": (2, 7, "gate 'sum' not satisfied at row 7"), "copy": (2, u - 1, "copy constraint"),
              "lookup": (0, u - 2, "lookup 'x in range' not satisfied at row %d" % (u - 2))}
    return meta, region, reached, plants


# ---- phases: challenges, constants, ops and the stack ---------------------------------------------------------------------------------
PHASE_TABLE = [(0, 0), (1, 2), (2, 3), (3, 5), (4, 7), (5, 11), (6, 13), (7, 17)]  # (t_a, t_b), the zero tuple first
PHASE_ROWS = (3, 1, 7, 7, 0, 5, 2, 6, 4, 1, 5)  # the table row every selected witness row holds; the gates are off on the last


def phases_circuit(custom):
    """k = 6, a plain key: three advice phases and 16 challenges (6 usable after phase 0, 5 after phase 1, 5 after phase 2).  Challenge
    j < 11 defines the column w_j = a + c_j b of the NEXT phase; about 280 small polynomials q (const w_j - const (a + c_j b)), every
    sixteenth-to-eleventh of them multiplied by a phase-2 challenge, fill the gate program to within 16 ops of its limit and use every
    one of 256 constants; the first polynomial has stack depth 8.  The lookup q (a + C b) in t_a + C t_b and the shuffle of a + C b
    against d + C e read C = c_0 + .. + c_10 (a phase-2 challenge appears in gates only)."""
    n_ch, n_ph = LIMITS["MAX_CHALLENGES"], LIMITS["MAX_ADVICE_PHASES"]
    max_ops, n_const = LIMITS["MAX_EXPR_OPS"], LIMITS["MAX_EXPR_CONSTANTS"]
    meta = custom.ConstraintSystem()
    a, b, d, e = (meta.advice_column() for _ in range(4))
    per_phase = [n_ch - 2 * (n_ch // n_ph)] + [n_ch // n_ph] * (n_ph - 1)  # 6, 5, 5
    ch, w = [], []
    for phase, count in enumerate(per_phase):
        ch += [meta.challenge_usable_after(phase) for _ in range(count)]
        if phase + 1 < n_ph:
            w += [meta.advice_column_in(phase + 1) for _ in range(count)]
    n_w = len(w)
    ta, tb = meta.fixed_column(), meta.fixed_column()
    q, q_look = meta.selector(), meta.selector()
    meta.enable_equality(w[0])
    cur = custom.Rotation.cur()
    rng = random.Random(1603)
    pool = [R - 1, R - 2, 1, 2] + [rng.randrange(R) for _ in range(n_const - 4)]
    assert len(set(pool)) == n_const
    const = custom.Expression.constant
    qa = lambda m, col: m.query_advice(col, cur)
    rlc = lambda m, j: qa(m, a) + m.query_challenge(ch[j]) * qa(m, b)

    def deep(m):  # x1 - (x2 - (x3 - .. - x8)): SUB keeps its order, eight operands deep; pairwise equal, so it is zero
        xs = [qa(m, a), qa(m, a), qa(m, b), qa(m, b), qa(m, w[0]), qa(m, w[0]), const(pool[0]), const(pool[0])]
        expr = xs[-1]
        for x in reversed(xs[:-1]):
            expr = x - expr
        return [m.query_selector(q) * expr]

    meta.create_gate("deep", deep)
    assert meta.polynomials[0].stack_depth() == LIMITS["MAX_EXPR_STACK"]

    def small(m, i):
        j, c = i % n_ch, const(pool[i % n_const])
        body = c * qa(m, w[j % n_w]) - c * rlc(m, j % n_w)
        return m.query_selector(q) * body if j < n_w else m.query_selector(q) * m.query_challenge(ch[j]) * body

    total = len(meta.program()[0])
    i = 0
    while True:
        size = len(small(meta, i).resolve(0).program()[0])
        if total + size > max_ops:
            break
        meta.create_gate("rlc %d" % i, lambda m: [small(m, i)])
        total += size
        i += 1
    big_c = lambda m: _total([m.query_challenge(c) for c in ch[:n_w]])
    meta.lookup_any("rlc in the table", lambda m: [(m.query_selector(q_look) * (qa(m, a) + big_c(m) * qa(m, b)),
                                                    m.query_fixed(ta, cur) + big_c(m) * m.query_fixed(tb, cur))])
    meta.shuffle("rlc rows", lambda m: [(qa(m, a) + big_c(m) * qa(m, b), qa(m, d) + big_c(m) * qa(m, e))])
    ops, constants = meta.program()
    assert len(ops) == total and max_ops - 16 < total <= max_ops
    used = {index for op, index, _ in ops if op == 9}  # H2MI_EXPR_CHALLENGE
    assert used == set(range(n_ch)) and [c.phase for c in ch[n_w:]] == [n_ph - 1] * (n_ch - n_w)
    rows = [PHASE_TABLE[s] for s in PHASE_ROWS]
    perm = list(rows)
    rng.shuffle(perm)

    def synthesize(challenges):
        region = custom.Assignment(meta, challenges=challenges)
        for row, (x, y) in enumerate(PHASE_TABLE):
            region.assign_fixed(ta, row, x)
            region.assign_fixed(tb, row, y)
        cell = None
        for row, ((x, y), (x2, y2)) in enumerate(zip(rows, perm)):
            region.assign_advice(a, row, x)
            region.assign_advice(b, row, y)
            region.assign_advice(d, row + 7, x2)  # other rows than the inputs'
            region.assign_advice(e, row + 7, y2)
            region.enable_selector(q_look, row)
            if row + 1 == len(rows):  # a row only the lookup and the shuffle read
                continue
            region.enable_selector(q, row)
            for j, col in enumerate(w):
                cv = region.get_challenge(ch[j])
                c0 = region.assign_advice(col, row, (x + cv * y) % R if cv is not None else 0)
                cell = cell if j else c0
        region.copy_advice(cell, w[0], len(rows) + 2)
        return region

    reached = {"MAX_ADVICE_PHASES": meta.n_phases, "MAX_CHALLENGES": len(meta.challenge_phase), "MAX_EXPR_CONSTANTS": len(constants),
               "MAX_EXPR_STACK": max(p.stack_depth() for p in meta.polynomials), "ops short of MAX_EXPR_OPS, in sixteens": ((max_ops - total) // 16, 0)}
    plants = {"gate": (4 + n_w - 1, 2, "gate 'rlc %d' not satisfied at row 2" % (n_w - 1)), "copy": (4, len(rows) + 2, "copy constraint"),
              "lookup": (1, len(rows) - 1, "lookup 'rlc in the table' not satisfied at row %d" % (len(rows) - 1)), "shuffle": (3, 9, "shuffle 'rlc rows' not satisfied")}
    return meta, synthesize, reached, plants


# ---- batch8: the most circuits one proof takes -------------------------------------------------------------------------------------------
def batch_circuit(custom):
    """k = 6, a plain key, MAX_CIRCUITS witnesses of one system: columns a, b, d, m (phase 0) and w (phase 1), a challenge c; gates q (a
    b - m), q (w - a - c b) and q_pub (a - instance); a in the fixed range 0 .. 15; d a permutation of a (a shuffle); copies of m and w"""
    N = LIMITS["MAX_CIRCUITS"]
    meta = custom.ConstraintSystem()
    a, b, d, m = (meta.advice_column() for _ in range(4))
    inst = meta.instance_column()
    t = meta.fixed_column()
    ch = meta.challenge_usable_after(0)
    w = meta.advice_column_in(1)
    q, q_pub = meta.selector(), meta.selector()
    meta.enable_equality(m)
    meta.enable_equality(w)
    cur = custom.Rotation.cur()
    qa = lambda mt, col: mt.query_advice(col, cur)
    meta.create_gate("product", lambda mt: [mt.query_selector(q) * (qa(mt, a) * qa(mt, b) - qa(mt, m))])
    meta.create_gate("rlc", lambda mt: [mt.query_selector(q) * (qa(mt, w) - qa(mt, a) - mt.query_challenge(ch) * qa(mt, b))])
    meta.create_gate("public", lambda mt: [mt.query_selector(q_pub) * (qa(mt, a) - mt.query_instance(inst, cur))])
    meta.lookup("a in range", lambda mt: [(qa(mt, a), mt.query_fixed(t, cur))])
    meta.shuffle("d is a permuted", lambda mt: [(qa(mt, a), qa(mt, d))])
    u = usable_rows(meta, 6)

    def circuit(variant):
        rng = random.Random(800 + variant)
        av = [rng.randrange(16) for _ in range(u)]
        av[40] = 15  # the cell to plant in: 15 + 1 is outside the range
        bv = [rng.randrange(R) for _ in range(24)]
        dv = list(av)
        rng.shuffle(dv)

        def synthesize(challenges):
            region = custom.Assignment(meta, instance=av[:4], challenges=challenges)
            cv = region.get_challenge(ch)
            for v in range(16):
                region.assign_fixed(t, v, v)
            cm = cw = None
            for row in range(u):
                region.assign_advice(a, row, av[row])
                region.assign_advice(d, row, dv[row])
                if row < 24:
                    region.assign_advice(b, row, bv[row])
                    cm = region.assign_advice(m, row, av[row] * bv[row] % R)
                    cw = region.assign_advice(w, row, (av[row] + cv * bv[row]) % R if cv is not None else 0)
                    region.enable_selector(q, row)
                if row < 4:
                    region.enable_selector(q_pub, row)
            region.copy_advice(cm, m, 30)
            region.copy_advice(cw, w, 31)
            return region

        return synthesize

    witnesses = [circuit(v) for v in range(N)]
    reached = {"MAX_CIRCUITS": len(witnesses)}
    plants = {"gate": (3, 5, "gate 'product' not satisfied at row 5"), "copy": (3, 30, "copy constraint"),
              "lookup": (0, 40, "lookup 'a in range' not satisfied at row 40"), "shuffle": (2, 6, "shuffle 'd is a permuted' not satisfied")}
    return meta, witnesses, reached, plants


# name -> (k, logup key, maker)
SHAPES = {
    "wide": (6, False, wide_circuit),
    "rot5": (6, False, lambda custom: rot_circuit(custom, 5)),
    "rot8": (6, False, lambda custom: rot_circuit(custom, 8)),
    "rot16": (6, False, lambda custom: rot_circuit(custom, HEAD_SLICE)),
    "rot17": (6, False, lambda custom: rot_circuit(custom, HEAD_SLICE + 1)),
    "rot_many": (7, False, rot_many_circuit),
    "args_plain": (6, False, args_plain_circuit),
    "args_logup": (6, True, args_logup_circuit),
    "signed": (11, True, signed_circuit),
    "phases": (6, False, phases_circuit),
    "batch8": (6, False, batch_circuit),
}


def build(custom, name: str):
    """-> (cs, witness, k, logup); asserts that every count the shape reached equals its limit"""
    k, logup, maker = SHAPES[name]
    cs, witness, reached, plants = maker(custom)
    for what, got in reached.items():
        got, want = got if isinstance(got, tuple) else (got, LIMITS[what])
        assert got == want, f"{name}: {what} is {got}, the limit is {want}"
    _REACHED[name], _PLANTS[name] = reached, plants
    return cs, witness, k, logup


def reached(name: str) -> dict:
    return _REACHED[name]


def plants(name: str) -> dict:
    """argument kind -> (advice column, row, the words mock refuses the changed witness with)"""
    return _PLANTS[name]


def planted(witness, column: int, row: int):
    """the witness with one advice cell one larger"""
    def alter(region):
        region.advice[column][row] = (region.advice[column].get(row, 0) + 1) % R
        return region

    return (lambda challenges: alter(witness(challenges))) if callable(witness) else alter(witness)


def first_assignment(cs, witness):
    """the assignment keygen reads the fixed cells and the copies from"""
    one = witness[0] if isinstance(witness, list) else witness
    return one([None] * len(cs.challenge_phase)) if callable(one) else one


def proof_layout(cs, n_circuits: int, logup: bool, length: int) -> dict:
    """byte offsets into a proof of n_circuits circuits, in the order the verifiers read it: the LAST advice commitment, the last
    lookup's [M] (logUp) or its permuted pair, the last permutation product, the last lookup product / [phi], the last shuffle product,
    the last evaluation and the two SHPLONK points.  Points and scalars take 32 bytes each."""
    N, L, S = n_circuits, len(cs.lookup_arguments), len(cs.shuffles)
    n_sets = -(-len(cs.perm_columns) // (cs.degree() - 2))
    per_lookup = 1 if logup else 2
    at = {"advice": N * cs.n_advice - 1}
    pos = N * cs.n_advice
    if L:
        at["lookup M" if logup else "lookup permuted input"] = pos + N * L * per_lookup - per_lookup
        if not logup:
            at["lookup permuted table"] = pos + N * L * per_lookup - 1
    pos += N * L * per_lookup
    if n_sets:
        at["permutation product"] = pos + N * n_sets - 1
    pos += N * n_sets
    if L:
        at["lookup phi" if logup else "lookup product"] = pos + N * L - 1
    pos += N * L
    if S:
        at["shuffle product"] = pos + N * S - 1
    out = {name: 32 * p for name, p in at.items()}
    out.update({"last evaluation": length - 96, "SHPLONK h1": length - 64, "SHPLONK h2": length - 32})
    return out


def proof_length(cs, n_circuits: int, logup: bool) -> int:
    N, L, S, m = n_circuits, len(cs.lookup_arguments), len(cs.shuffles), len(cs.perm_columns)
    n_sets = -(-m // (cs.degree() - 2))
    points = N * (cs.n_advice + (1 if logup else 2) * L + n_sets + L + S) + 1 + (cs.degree() - 1) + 2
    evals = N * len(cs.advice_queries) + len(cs.fixed_queries) + 1 + m + N * ((3 * n_sets - 1 if n_sets else 0) + (3 if logup else 5) * L + 2 * S)
    return 32 * (points + evals)
