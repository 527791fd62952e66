"""LogUp lookups with SEVERAL INPUT SETS over one table, shared by tests/test_logup_sets_host.py and tests/test_gpu_logup_sets.py: the
functions of tests/logup_cases.py generalised to a list of input columns [the merging of lookups that share a table in the `mv-lookup`
line of halo2_proofs — RESTATED FROM MEMORY like the argument itself and pinned to DESIGN.md 4.5 and to this file, not to a crate].
With a_j = A_j + beta and s = S + beta a row's fraction is sum_j 1 / a_j - M / s = N / D, D = s prod_j a_j, N = s sum_j prod_{m != j}
a_m - M prod_j a_j.  One input set gives the numbers of tests/logup_cases.py (tests/test_logup_sets_host.py checks that).  Then `verify`
with the per-lookup input count, and the circuits of the tests through custom.py."""
import random

import logup_cases
import shuffle_cases
from batch_cases import KINDS, MAX_CIRCUITS, keys_delta, lookup_terms, permutation_terms
from lookup_expr_cases import compress
from oracle import bn254 as o
from oracle.flex import ADVICE, FIXED, INSTANCE, ProofReader, construct_intermediate_sets
from oracle.prover import evaluate_vanishing_polynomial, lagrange_interpolate, rotate_omega
from phase_cases import run_postfix
from shuffle_cases import shuffle_terms

R = o.R
MAX_LOGUP_INPUTS = 6  # include/h2mi.h H2MI_MAX_LOGUP_INPUTS


# ---- the argument in Python integers -------------------------------------------------------------------------------------------------
def multiplicities(a_sets, s_rows, u: int):
    """a_sets: K input columns.  -> (M[0 .. u - 1], the (row, set) pairs whose input is no table value).  M[r] = sum_j #{i < u: A_j[i] =
    S[r]} on the lowest usable row r that holds its table value, 0 on every other usable row"""
    first = {}
    for r in range(u):
        first.setdefault(s_rows[r], r)
    m, missing = [0] * u, []
    for j, a_rows in enumerate(a_sets):
        for i in range(u):
            r = first.get(a_rows[i])
            if r is None:
                missing.append((i, j))
            else:
                m[r] += 1
    return m, missing


def running_sum(a_sets, s_rows, m_rows, beta: int, u: int):
    """-> phi[0 .. u]: phi[0] = 0, phi[i+1] = phi[i] + sum_j 1 / (A_j,i + beta) - M_i / (S_i + beta)"""
    phi = [0]
    for i in range(u):
        step = sum(pow((a_rows[i] + beta) % R, -1, R) for a_rows in a_sets) - m_rows[i] * pow((s_rows[i] + beta) % R, -1, R)
        phi.append((phi[-1] + step) % R)
    return phi


def fraction(a_vals, s_val, m, beta):
    """-> (N, D) of one row, written out: D = s prod_j a_j, N = s sum_j prod_{m != j} a_m - M prod_j a_j"""
    a = [(v + beta) % R for v in a_vals]
    s = (s_val + beta) % R
    prod = 1
    for v in a:
        prod = prod * v % R
    total = 0
    for j in range(len(a)):
        others = 1
        for i, v in enumerate(a):
            if i != j:
                others = others * v % R
        total = (total + others) % R
    return (s * total - m * prod) % R, s * prod % R


def logup_terms(v, y, beta, a_vals, s_in, m, phi, phi_next, l0, l_last, l_active):
    """one logUp lookup's three terms folded into v with y: l_0 phi, l_last phi, l_active ((phi(wX) - phi(X)) D - N)"""
    v = (v * y + phi * l0) % R
    v = (v * y + phi * l_last) % R
    num, den = fraction(a_vals, s_in, m, beta)
    v = (v * y + ((phi_next - phi) * den - num) * l_active) % R
    return v


def batched_quotient(k, extended_k, zeta, extended_omega, delta, blinding_factors, ops, constants, challenges, circuits, shared, beta, gamma, y,
                     logup: bool = False):
    """logup_cases.batched_quotient with a circuit's "lookups" entries (LIST of compressed inputs, None, compressed table, M, None, phi)
    on the extended coset; without logup the list holds one input"""
    size, rot = 1 << extended_k, 1 << (extended_k - k)
    t_inv = [pow((pow(zeta * pow(extended_omega, i, R) % R, 1 << k, R) - 1) % R, -1, R) for i in range(rot)]
    sig, chunk = shared["perm_sigmas"], shared["chunk"]
    out = []
    x = zeta
    for idx in range(size):
        at = lambda r: (idx + r * rot) % size
        nxt, prv, lst = at(1), at(-1), at(-(blinding_factors + 1))
        l0, ll, la = shared["l0"][idx], shared["l_last"][idx], shared["l_active"][idx]
        v = 0
        for c in circuits:
            cols = {"advice": c["advice"], "fixed": c["fixed"], "instance": [c.get("instance")]}
            for poly in run_postfix(ops, constants, lambda op, col, r: cols[KINDS[op]][col][at(r)], challenges):
                v = (v * y + poly) % R
            zs = c["perm_zs"]
            v = permutation_terms(v, y, beta, gamma, delta, chunk, [p[idx] for p in c["perm_values"]], [s[idx] for s in sig], [z[idx] for z in zs],
                                  [z[nxt] for z in zs], [z[lst] for z in zs], l0, ll, la, x)
            for a_ins, _, table, pin, ptab, lz in c["lookups"]:
                if logup:
                    v = logup_terms(v, y, beta, [a[idx] for a in a_ins], table[idx], pin[idx], lz[idx], lz[nxt], l0, ll, la)
                else:
                    v = lookup_terms(v, y, beta, gamma, a_ins[0][idx], table[idx], pin[idx], pin[prv], ptab[idx], lz[idx], lz[nxt], l0, ll, la)
            for a_in, s_in, sz in c.get("shuffles", ()):
                v = shuffle_terms(v, y, gamma, a_in[idx], s_in[idx], sz[idx], sz[nxt], l0, ll, la)
        out.append(v * t_inv[idx % rot] % R)
        x = x * extended_omega % R
    return out


# ---- the verifier ---------------------------------------------------------------------------------------------------------------------
def verify(keys, proof: bytes, instances, gates, lookups, shuffles=(), advice_phase=None, challenge_phase=(), challenges_out=None,
           logup: bool = False) -> bool:
    """logup_cases.verify, line for line, with the per-lookup input count: `lookups` holds per lookup ARGUMENT ([input set], table) with
    every input set and the table a list of g(q, challenges) — a merged argument is still one [M], one [phi], three evaluations and
    three openings; only its third quotient term reads every set (the lines marked `sets`).  Without logup every argument has one set."""
    cs, n, dom = keys.cs, keys.n, keys.dom
    bf = cs.blinding_factors
    N = len(instances)
    if not 1 <= N <= MAX_CIRCUITS:
        return False
    m = len(cs.perm_columns)
    n_sets = -(-m // cs.chunk)
    advice_phase = [0] * cs.n_advice if advice_phase is None else list(advice_phase)
    challenges = [None] * len(challenge_phase)
    C = range(N)
    try:
        rd = ProofReader(proof)
        rd.tr.common_scalar(keys.transcript_repr)
        for circuit in instances:
            for vals in circuit:
                for v in vals:
                    rd.tr.common_scalar(v)
        advice_c = [[None] * cs.n_advice for _ in C]
        for phase in range(1 + max(advice_phase, default=0)):
            for i in C:
                for j in range(cs.n_advice):
                    if advice_phase[j] == phase:
                        advice_c[i][j] = rd.read_point()
            for ci, p in enumerate(challenge_phase):
                if p == phase:
                    challenges[ci] = rd.squeeze()
        theta = rd.squeeze()
        if logup:  # one point per lookup: [M]
            lk_perm_c = [[(rd.read_point(), None) for _ in lookups] for _ in C]
        else:
            lk_perm_c = [[(rd.read_point(), rd.read_point()) for _ in lookups] for _ in C]
        beta, gamma = rd.squeeze(), rd.squeeze()
        z_c = [[rd.read_point() for _ in range(n_sets)] for _ in C]
        lz_c = [[rd.read_point() for _ in lookups] for _ in C]  # logup: [phi], in the lookup product's slot
        sz_c = [[rd.read_point() for _ in shuffles] for _ in C]
        random_c = rd.read_point()
        y = rd.squeeze()
        h_c = [rd.read_point() for _ in range(dom.quotient_poly_degree)]
        x = rd.squeeze()
        advice_evals = [[rd.read_scalar() for _ in cs.advice_queries] for _ in C]
        fixed_evals = [rd.read_scalar() for _ in cs.fixed_queries]
        random_eval = rd.read_scalar()
        sigma_evals = [rd.read_scalar() for _ in cs.perm_columns]
        z_evals = []
        for _ in C:
            mine = []
            for s in range(n_sets):
                e, en = rd.read_scalar(), rd.read_scalar()
                mine.append((e, en, rd.read_scalar() if s + 1 < n_sets else None))
            z_evals.append(mine)
        lk_evals = [[tuple(rd.read_scalar() for _ in range(3 if logup else 5)) for _ in lookups] for _ in C]  # logup: phi(x), phi(wx), M(x)
        sf_evals = [[(rd.read_scalar(), rd.read_scalar()) for _ in shuffles] for _ in C]
    except ValueError:
        return False
    if challenges_out is not None:
        challenges_out[:] = challenges
    xn = pow(x, n, R)
    w = dom.omega
    l_at = lambda rot: (xn - 1) * pow(n, -1, R) % R * pow(w, rot % n, R) % R * pow((x - pow(w, rot % n, R)) % R, -1, R) % R
    l_evals = [l_at(rot) for rot in range(-(bf + 1), 1)]
    l_last, l_blind, l_0 = l_evals[0], sum(l_evals[1 : 1 + bf]) % R, l_evals[1 + bf]
    lact = (1 - (l_last + l_blind)) % R
    v = 0
    for i in C:
        evals = {}
        for qi, (c, r) in enumerate(cs.advice_queries):
            evals[(ADVICE, c, r)] = advice_evals[i][qi]
        for qi, (c, r) in enumerate(cs.fixed_queries):
            evals[(FIXED, c, r)] = fixed_evals[qi]
        for c, r in cs.instance_queries:
            pt = rotate_omega(dom, x, r)
            ptn = pow(pt, n, R)
            evals[(INSTANCE, c, r)] = sum(val * ((ptn - 1) * pow(n, -1, R) % R * pow(w, row, R) % R * pow((pt - pow(w, row, R)) % R, -1, R) % R)
                                          for row, val in enumerate(instances[i][c])) % R
        q = lambda kind, col, r: evals[(kind, col, r)]
        for gate in gates:
            v = (v * y + gate(q, challenges)) % R
        ze = z_evals[i]
        v = permutation_terms(v, y, beta, gamma, keys_delta(), cs.chunk, [evals[(kc[0], kc[1], 0)] for kc in cs.perm_columns], sigma_evals,
                              [e[0] for e in ze], [e[1] for e in ze], [e[2] for e in ze], l_0, l_last, lact, x)
        for (in_sets, tabs), ev in zip(lookups, lk_evals[i]):
            a_vals = [compress([g(q, challenges) for g in ins], theta) for ins in in_sets]  # sets
            t_val = compress([g(q, challenges) for g in tabs], theta)
            if logup:
                phi, phi_next, m_eval = ev
                v = logup_terms(v, y, beta, a_vals, t_val, m_eval, phi, phi_next, l_0, l_last, lact)
            else:
                if len(a_vals) != 1:
                    return False
                lz, lz_next, ap, ap_inv, sp = ev
                v = lookup_terms(v, y, beta, gamma, a_vals[0], t_val, ap, ap_inv, sp, lz, lz_next, l_0, l_last, lact)
        for (ins, shs), (sz, sz_next) in zip(shuffles, sf_evals[i]):
            a_val, s_val = compress([g(q, challenges) for g in ins], theta), compress([g(q, challenges) for g in shs], theta)
            v = shuffle_terms(v, y, gamma, a_val, s_val, sz, sz_next, l_0, l_last, lact)
    expected_h = v * pow((xn - 1) % R, -1, R) % R
    h_commitment = None
    for cmt in reversed(h_c):
        h_commitment = o.g1_add(o.g1_mul(xn, h_commitment) if h_commitment else None, cmt)
    rx = lambda r: rotate_omega(dom, x, r)
    x_next, x_last, x_inv = rx(1), rx(-(bf + 1)), rx(-1)
    points, queries = {}, []

    def qq(key, cmt, pt, evl):
        points[key] = cmt
        queries.append((key, pt, evl))

    for i in C:
        for qi, (c, r) in enumerate(cs.advice_queries):
            qq(("advice", i, c), advice_c[i][c], rx(r), advice_evals[i][qi])
        for s in range(n_sets):
            qq(("z", i, s), z_c[i][s], x, z_evals[i][s][0])
            qq(("z", i, s), z_c[i][s], x_next, z_evals[i][s][1])
        for s in reversed(range(n_sets - 1)):
            qq(("z", i, s), z_c[i][s], x_last, z_evals[i][s][2])
        for li, ev in enumerate(lk_evals[i]):
            if logup:  # lookups.open: phi at x, phi at omega x, M at x
                phi, phi_next, m_eval = ev
                qq(("lz", i, li), lz_c[i][li], x, phi)
                qq(("lz", i, li), lz_c[i][li], x_next, phi_next)
                qq(("la", i, li), lk_perm_c[i][li][0], x, m_eval)
                continue
            lz, lz_next, ap, ap_inv, sp = ev
            qq(("lz", i, li), lz_c[i][li], x, lz)
            qq(("la", i, li), lk_perm_c[i][li][0], x, ap)
            qq(("ls", i, li), lk_perm_c[i][li][1], x, sp)
            qq(("la", i, li), lk_perm_c[i][li][0], x_inv, ap_inv)
            qq(("lz", i, li), lz_c[i][li], x_next, lz_next)
        for si, (sz, sz_next) in enumerate(sf_evals[i]):
            qq(("sz", i, si), sz_c[i][si], x, sz)
            qq(("sz", i, si), sz_c[i][si], x_next, sz_next)
    for qi, (c, r) in enumerate(cs.fixed_queries):
        qq(("fixed", c), keys.fixed_commitments[c], rx(r), fixed_evals[qi])
    for j in range(m):
        qq(("sigma", j), keys.permutation_commitments[j], x, sigma_evals[j])
    qq(("h",), h_commitment, x, expected_h)
    qq(("random",), random_c, x, random_eval)
    rotation_sets, super_points = construct_intermediate_sets(queries)
    y_sh, vv = rd.squeeze(), rd.squeeze()
    try:
        h1 = rd.read_point()
        uu = rd.squeeze()
        h2 = rd.read_point()
    except ValueError:
        return False
    if rd.pos != len(proof):
        return False
    outer, r_outer, z_0, z_0_diff_inv, vp = None, 0, 0, 0, 1
    for si, (pts, comms) in enumerate(rotation_sets):
        z_diff = evaluate_vanishing_polynomial([p for p in super_points if p not in pts], uu)
        if si == 0:
            z_0 = evaluate_vanishing_polynomial(pts, uu)
            z_0_diff_inv = pow(z_diff, -1, R)
            z_diff = 1
        else:
            z_diff = z_diff * z_0_diff_inv % R
        inner, r_inner, yp = None, 0, 1
        for key, evs in comms:
            r_inner = (r_inner + yp * o.eval_polynomial(lagrange_interpolate(pts, evs), uu)) % R
            inner = o.g1_add(inner, o.g1_mul(yp, points[key]))
            yp = yp * y_sh % R
        r_outer = (r_outer + vp * r_inner % R * z_diff) % R
        outer = o.g1_add(outer, o.g1_mul(vp * z_diff % R, inner))
        vp = vp * vv % R
    outer = o.g1_add(outer, o.g1_mul((-r_outer) % R, o.G1_GEN))
    outer = o.g1_add(outer, o.g1_mul((-z_0) % R, h1))
    outer = o.g1_add(outer, o.g1_mul(uu, h2))
    return o.g1_mul(keys.s, h2) == outer



def lookup_sets(lookups, n_inputs=None):
    """logup_cases' per-lookup (inputs, table) lists -> this verifier's form, consecutive lookups merged by n_inputs (None: one each)"""
    n_inputs = [1] * len(lookups) if n_inputs is None else list(n_inputs)
    assert sum(n_inputs) == len(lookups)
    out, at = [], 0
    for count in n_inputs:
        out.append(([ins for ins, _ in lookups[at:at + count]], lookups[at][1]))
        at += count
    return out


def expr_lookup_sets(cs):
    """a custom.ConstraintSystem's lookup ARGUMENTS (after merge_lookups, or one per lookup) in the verifier's form"""
    from phase_cases import expr_lookups

    declared = expr_lookups(cs)
    return [([declared[l][0] for l in arg], declared[arg[0]][1]) for arg in cs.lookup_arguments]


def verify_circuits(vk, cs, proof: bytes, instances, logup: bool, challenges_out=None) -> bool:
    """`verify` for N circuits of one custom.ConstraintSystem; instances[i]: circuit i's public inputs (one instance column at most)"""
    from phase_cases import expr_gates

    per_circuit = [[list(v)] if cs.n_instance else [] for v in instances]
    return verify(vk, proof, per_circuit, expr_gates(cs), expr_lookup_sets(cs), shuffle_cases.expr_shuffles(cs), cs.advice_phase, cs.challenge_phase,
                  challenges_out=challenges_out, logup=logup)


def proof_offsets(cs, n_circuits: int = 1):
    """logup_cases.proof_offsets with the ARGUMENTS of a (merged) constraint system: -> (byte offset of the first [M], of the first [phi],
    of the first lookup evaluation phi(x))"""
    m, chunk = len(cs.perm_columns), cs.degree() - 2
    n_sets = -(-m // chunk)
    L, S, N = len(cs.lookup_arguments), len(cs.shuffles), n_circuits
    m_at = N * cs.n_advice
    phi_at = m_at + N * L + N * n_sets
    points = phi_at + N * L + N * S + 1 + (cs.degree() - 1)
    evals_before = N * len(cs.advice_queries) + len(cs.fixed_queries) + 1 + m + N * (3 * n_sets - 1 if n_sets else 0)
    return 32 * m_at, 32 * phi_at, 32 * (points + evals_before)


def argument_rows(cs, asg, k: int, challenges=()):
    """per lookup ARGUMENT ([input tuples of set j on all 2^k rows], table tuples)"""
    rows = logup_cases.lookup_rows(cs, asg, k, challenges)
    return [([rows[l][0] for l in arg], rows[arg[0]][1]) for arg in cs.lookup_arguments]


# ---- the circuits ----------------------------------------------------------------------------------------------------------------------
RANGE_BITS = 3


def range_circuit(custom, columns: int = 3, variant: int = 0, bad=None, merge=True, max_degree=6):
    """k = 5: `columns` lookup-advice columns, each looked up in ONE fixed table 0 .. 2^RANGE_BITS - 1 (the shape the Range builder makes
    with several lookup-advice columns), a gate q (c_0 - 5) on four rows and a permutation over the first two.  bad = (column, row): that cell holds a value outside
    the table.  max_degree: the budget of merge_lookups (6 holds three sets of degree-1 inputs; None is the default budget, which
    at this system's degree 4 merges pairs).  -> (cs, assignment)"""
    meta = custom.ConstraintSystem()
    cols = [meta.advice_column() for _ in range(columns)]
    table = meta.fixed_column()
    q = meta.selector()
    for c in cols[:2]:
        meta.enable_equality(c)
    cur = custom.Rotation.cur()
    meta.create_gate("five", lambda meta: [meta.query_selector(q) * (meta.query_advice(cols[0], cur) - 5)])
    for j, c in enumerate(cols):
        meta.lookup("range %d" % j, lambda meta, c=c: [(meta.query_advice(c, cur), meta.query_fixed(table, cur))])
    if merge:
        meta.merge_lookups(max_degree)
    region = custom.Assignment(meta)
    for v in range(1 << RANGE_BITS):
        region.assign_fixed(table, v, v)
    rng = random.Random(700 + variant)
    cells = {}
    for j, c in enumerate(cols):
        for row in range(20):
            v = 7 if j == columns - 1 and row == 0 else rng.randrange(1 << RANGE_BITS)  # 7 at least once, in the last set
            if j == 0 and row < 4:
                v = 5  # the gate's rows
                region.enable_selector(q, row)
            cells[(j, row)] = region.assign_advice(c, row, v)
    if bad is not None:
        region.assign_advice(cols[bad[0]], bad[1], 1 << RANGE_BITS)
    region.copy_advice(cells[(0, 3)], cols[1], 22)
    return meta, region


def xor_pair_circuit(custom, variant: int = 0):
    """k = 6: the 2-bit XOR tuple table looked up by TWO tuples, (q a, q b, q c) on the row and (q a(wX), q b(wX), q c(wX)) one row down
    (a rotation inside the second set), merged into one argument of degree 2 + 2 + 2 + 1 = 7; a degree-5 gate on c.  -> (cs, assignment)"""
    meta = custom.ConstraintSystem()
    a, b, c = (meta.advice_column() for _ in range(3))
    t_a, t_b, t_c = (meta.fixed_column() for _ in range(3))
    q = meta.selector()
    meta.enable_equality(a)
    cur, nxt = custom.Rotation.cur(), custom.Rotation.next()

    def two_bits(meta):
        c_ = meta.query_advice(c, cur)
        return [meta.query_selector(q) * c_ * (c_ - 1) * (c_ - 2) * (c_ - 3)]

    meta.create_gate("c has two bits", two_bits)
    for name, rot in (("xor", cur), ("xor below", nxt)):
        meta.lookup(name, lambda meta, rot=rot: [(meta.query_selector(q) * meta.query_advice(col, rot), meta.query_fixed(tab, cur))
                                                  for col, tab in ((a, t_a), (b, t_b), (c, t_c))])
    meta.merge_lookups(9)
    region = custom.Assignment(meta)
    for i in range(16):
        for tab, v in ((t_a, i >> 2), (t_b, i & 3), (t_c, (i >> 2) ^ (i & 3))):
            region.assign_fixed(tab, i, v)
    rng = random.Random(900 + variant)
    first = None
    for row in range(30):
        x, y = rng.randrange(4), rng.randrange(4)
        cell = region.assign_advice(a, row, x)
        first = first or cell
        region.assign_advice(b, row, y)
        region.assign_advice(c, row, x ^ y)
        if row < 29:
            region.enable_selector(q, row)
    region.copy_advice(first, a, 40)
    return meta, region


def beside_circuit(custom, variant: int = 0, extra=((0, 2),), max_degree=None):
    """k = 6: logup_cases.mixed_circuit (two gates, a permutation over three columns, the XOR tuple lookup, a shuffle) with more lookups
    behind it: per (table column, count) of `extra` that many fresh advice columns looked up in that fixed column of the XOR table.  The
    default — two columns in t_a at the default budget — is one merged argument beside the unmerged XOR lookup; ((0, 3), (1, 2)) at
    budget 6 gives arguments of 1, 3 and 2 input sets.  -> (cs, assignment)"""
    meta, region = logup_cases.mixed_circuit(custom, variant)
    cur = custom.Rotation.cur()
    added = []
    for tab, count in extra:
        for _ in range(count):
            col = meta.advice_column()
            added.append(col)
            meta.lookup("r%d in t%d" % (len(added) - 1, tab),
                        lambda meta, col=col, tab=tab: [(meta.query_advice(col, cur), meta.query_fixed(custom.Column(custom.FIXED, tab), cur))])
    meta.merge_lookups(max_degree)
    grown = custom.Assignment(meta)
    grown.advice[: len(region.advice)] = [dict(c) for c in region.advice]
    grown.fixed, grown.copies, grown.instance = [dict(c) for c in region.fixed], list(region.copies), list(region.instance)
    rng = random.Random(40 + variant)
    for col in added:
        for row in range(25):
            grown.assign_advice(col, row, rng.randrange(4))
    return meta, grown


def three_arguments_circuit(custom, variant: int = 0):
    """beside_circuit with arguments of 1, 3 and 2 input sets (degree 6)"""
    return beside_circuit(custom, variant, extra=((0, 3), (1, 2)), max_degree=6)


def phased_pair_circuit(custom):
    """k = 6, two advice phases: logup_cases.phased_circuit's lookup (the challenge inside its input and its table) and a second lookup
    of the phase-0 combination q (a + c b) in the same table, merged.  -> (cs, synthesize)"""
    meta = custom.ConstraintSystem()
    a, b = meta.advice_column(), meta.advice_column()
    t_a, t_b = meta.fixed_column(), meta.fixed_column()
    ch = meta.challenge_usable_after(0)
    w = meta.advice_column_in(1)
    q = meta.selector()
    meta.enable_equality(w)
    cur = custom.Rotation.cur()
    meta.create_gate("w = a + c b", lambda meta: [meta.query_selector(q) * (meta.query_advice(w, cur) - meta.query_advice(a, cur)
                                                                           - meta.query_challenge(ch) * meta.query_advice(b, cur))])
    table = lambda meta: meta.query_fixed(t_a, cur) + meta.query_challenge(ch) * meta.query_fixed(t_b, cur)
    meta.lookup_any("w in the table", lambda meta: [(meta.query_selector(q) * meta.query_advice(w, cur), table(meta))])
    meta.lookup_any("a + c b in the table", lambda meta: [(meta.query_selector(q) * (meta.query_advice(a, cur) + meta.query_challenge(ch)
                                                                                    * meta.query_advice(b, cur)), table(meta))])
    meta.merge_lookups(9)

    def synthesize(challenges):
        region = custom.Assignment(meta, challenges=challenges)
        cv = region.get_challenge(ch)
        for row, (x, y) in enumerate(logup_cases.PHASED_TABLE):
            region.assign_fixed(t_a, row, x)
            region.assign_fixed(t_b, row, y)
        cell = None
        for row, s in enumerate(logup_cases.PHASED_ROWS):
            x, y = logup_cases.PHASED_TABLE[s]
            region.assign_advice(a, row, x)
            region.assign_advice(b, row, y)
            region.enable_selector(q, row)
            cell = region.assign_advice(w, row, (x + cv * y) % R if cv is not None else 0)
        region.copy_advice(cell, w, len(logup_cases.PHASED_ROWS) + 2)
        return region

    return meta, synthesize


CASES = {"range3": 5, "xor_pair": 6, "beside": 6, "phased_pair": 6}  # name -> k: the circuits whose proofs the tests verify


def build(custom, name: str):
    """-> (cs, assignment or synthesize(challenges), k)"""
    maker = {"range3": range_circuit, "xor_pair": xor_pair_circuit, "beside": beside_circuit, "phased_pair": phased_pair_circuit}[name]
    return (*maker(custom), CASES[name])


first_assignment = shuffle_cases.first_assignment
