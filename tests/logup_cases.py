"""The logUp lookup argument, shared by tests/test_logup_host.py and tests/test_gpu_logup.py.  oracle/ knows no logUp, so this module
carries the Python-integer restatement [Haboeck, "Multivariate lookups based on logarithmic derivatives"; the `mv-lookup` feature of the
Scroll and ezkl lines of halo2_proofs — RESTATED FROM MEMORY like the shuffle and pinned to DESIGN.md 4.5 and to this file, not to a
crate; one input tuple per lookup, the crate's merging of several input sets over one table is not modelled]: the multiplicity column
by the first-occurrence rule (`multiplicities`), the running sum (`running_sum`), the three quotient terms (`logup_terms`), the
batched quotient of tests/shuffle_cases.py with a circuit's lookups in either form, and `verify` — tests/shuffle_cases.verify with the
lookup lines generalised: with logup = False it reads and checks exactly what that verifier does (tests/test_logup_host.py pins it on
the committed goldens and against that verifier), with logup = True every circuit's lookups commit ONE point [M] behind theta, [phi]
sits in the lookup product's slot, and a lookup has the evaluations phi(x), phi(omega x), M(x) and the openings phi at x, phi at
omega x, M at x.  Then the circuits of the tests through custom.py."""
import random

import shuffle_cases
from batch_cases import KINDS, MAX_CIRCUITS, keys_delta, lookup_terms, permutation_terms
from lookup_expr_cases import compress
from oracle import bn254 as o
from oracle.flex import ADVICE, FIXED, INSTANCE, ProofReader, construct_intermediate_sets
from oracle.prover import evaluate_vanishing_polynomial, lagrange_interpolate, rotate_omega
from phase_cases import run_postfix
from shuffle_cases import shuffle_terms

R = o.R
KEYGEN_LOGUP = 2  # include/h2mi_prover.h H2MI_KEYGEN_LOGUP


# ---- the argument in Python integers -------------------------------------------------------------------------------------------------
def multiplicities(a_rows, s_rows, u: int):
    """-> (M[0 .. u - 1], the usable rows whose input is no table value).  M[r] = #{i < u: A[i] = S[r]} on the lowest usable row r that
    holds its table value, 0 on every other usable row"""
    first = {}
    for r in range(u):
        first.setdefault(s_rows[r], r)
    m, missing = [0] * u, []
    for i in range(u):
        r = first.get(a_rows[i])
        if r is None:
            missing.append(i)
        else:
            m[r] += 1
    return m, missing


def running_sum(a_rows, s_rows, m_rows, beta: int, u: int):
    """-> phi[0 .. u]: phi[0] = 0, phi[i+1] = phi[i] + 1 / (A_i + beta) - M_i / (S_i + beta)"""
    phi = [0]
    for i in range(u):
        phi.append((phi[-1] + pow((a_rows[i] + beta) % R, -1, R) - m_rows[i] * pow((s_rows[i] + beta) % R, -1, R)) % R)
    return phi


def logup_terms(v, y, beta, a_in, s_in, m, phi, phi_next, l0, l_last, l_active):
    """one logUp lookup's three terms folded into v with y: l_0 phi, l_last phi,
    l_active ((phi(wX) - phi(X)) (A + beta)(S + beta) - ((S + beta) - M (A + beta)))"""
    v = (v * y + phi * l0) % R
    v = (v * y + phi * l_last) % R
    ab, sb = (a_in + beta) % R, (s_in + beta) % R
    v = (v * y + ((phi_next - phi) * ab % R * sb - (sb - m * ab)) * l_active) % R
    return v


def num_evaluations(n_circuits, n_advice_queries, n_fixed_queries, n_perm, n_sets, n_lookups, n_shuffles, logup: bool) -> int:
    """the count formula of include/h2mi_prover.h: three per lookup of a logUp key, five otherwise"""
    return (n_circuits * n_advice_queries + n_fixed_queries + 1 + n_perm
            + n_circuits * ((3 * n_sets - 1 if n_sets else 0) + (3 if logup else 5) * n_lookups + 2 * n_shuffles))


def batched_quotient(k, extended_k, zeta, extended_omega, delta, blinding_factors, ops, constants, challenges, circuits, shared, beta, gamma, y,
                     logup: bool = False):
    """shuffle_cases.batched_quotient with the lookups in either form.  logup: a circuit's "lookups" entries are (compressed input,
    None, compressed table, M, None, phi) on the extended coset — M in the permuted input's place, phi in the product's"""
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
            for a_in, b_in, table, pin, ptab, lz in c["lookups"]:
                a_val = a_in[idx] * b_in[idx] % R if b_in is not None else a_in[idx]
                if logup:
                    v = logup_terms(v, y, beta, a_val, table[idx], pin[idx], lz[idx], lz[nxt], l0, ll, la)
                else:
                    v = lookup_terms(v, y, beta, gamma, a_val, table[idx], pin[idx], pin[prv], ptab[idx], lz[idx], lz[nxt], l0, ll, la)
            for a_in, s_in, sz in c.get("shuffles", ()):
                v = shuffle_terms(v, y, gamma, a_in[idx], s_in[idx], sz[idx], sz[nxt], l0, ll, la)
        out.append(v * t_inv[idx % rot] % R)
        x = x * extended_omega % R
    return out


# ---- the verifier ---------------------------------------------------------------------------------------------------------------------
def verify(keys, proof: bytes, instances, gates, lookups, shuffles=(), advice_phase=None, challenge_phase=(), challenges_out=None,
           logup: bool = False) -> bool:
    """shuffle_cases.verify, line for line, with the lookup lines in either form (marked `logup`)"""
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
        for (ins, tabs), ev in zip(lookups, lk_evals[i]):
            a_val, t_val = compress([g(q, challenges) for g in ins], theta), compress([g(q, challenges) for g in tabs], theta)
            if logup:
                phi, phi_next, m_eval = ev
                v = logup_terms(v, y, beta, a_val, t_val, m_eval, phi, phi_next, l_0, l_last, lact)
            else:
                lz, lz_next, ap, ap_inv, sp = ev
                v = lookup_terms(v, y, beta, gamma, a_val, t_val, ap, ap_inv, sp, lz, lz_next, l_0, l_last, lact)
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


def verify_circuits(vk, cs, proof: bytes, instances, logup: bool, challenges_out=None) -> bool:
    """`verify` for N circuits of one custom.ConstraintSystem; instances[i]: circuit i's public inputs (one instance column at most)"""
    from phase_cases import expr_gates, expr_lookups

    per_circuit = [[list(v)] if cs.n_instance else [] for v in instances]
    return verify(vk, proof, per_circuit, expr_gates(cs), expr_lookups(cs), shuffle_cases.expr_shuffles(cs), cs.advice_phase, cs.challenge_phase,
                  challenges_out=challenges_out, logup=logup)


def proof_offsets(cs, n_circuits: int = 1):
    """-> (byte offset of the first [M], of the first [phi], of the first lookup evaluation phi(x)) in a logUp proof of n_circuits
    circuits of a custom.ConstraintSystem: points and scalars are 32 bytes each, in the order `verify` reads them"""
    m, chunk = len(cs.perm_columns), cs.degree() - 2
    n_sets = -(-m // chunk)
    L, S, N = len(cs.lookups), len(cs.shuffles), n_circuits
    m_at = N * cs.n_advice
    phi_at = m_at + N * L + N * n_sets
    points = phi_at + N * L + N * S + 1 + (cs.degree() - 1)
    evals_before = N * len(cs.advice_queries) + len(cs.fixed_queries) + 1 + m + N * (3 * n_sets - 1 if n_sets else 0)
    return 32 * m_at, 32 * phi_at, 32 * (points + evals_before)


# ---- a lookup's rows in Python integers -------------------------------------------------------------------------------------------------
def lookup_rows(cs, asg, k: int, challenges=()):
    """per lookup (input tuples, table tuples) on all 2^k rows of an assignment"""
    n = 1 << k
    value = {ADVICE: lambda c, r: asg.advice[c].get(r, 0), FIXED: lambda c, r: asg.fixed[c].get(r, 0),
             INSTANCE: lambda c, r: asg.instance[r] if r < len(asg.instance) else 0}
    at = lambda e, row: e.evaluate(lambda kind, c, rot: value[kind](c, (row + rot) % n), challenges)
    return [([tuple(at(a, row) for a, _ in pairs) for row in range(n)], [tuple(at(t, row) for _, t in pairs) for row in range(n)]) for pairs in cs.lookups]


# ---- the circuits ----------------------------------------------------------------------------------------------------------------------
PHASED_TABLE = [(0, 0), (1, 2), (2, 3), (3, 5), (4, 7), (5, 11), (1, 2), (6, 13)]  # (t_a, t_b); row 6 repeats row 1: the first-occurrence rule
PHASED_ROWS = (3, 1, 7, 7, 0, 5, 1)  # the table row each selected witness row holds


def phased_circuit(custom):
    """k = 6, two advice phases: phase-0 columns a, b; a challenge c usable after phase 0; a second-phase column w with the gate
    q (w - a - c b); the lookup of q w in t_a + c t_b — the challenge inside both sides of the lookup.  -> (cs, synthesize)"""
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
    meta.lookup_any("rlc in the table", lambda meta: [(meta.query_selector(q) * meta.query_advice(w, cur),
                                                       meta.query_fixed(t_a, cur) + meta.query_challenge(ch) * meta.query_fixed(t_b, cur))])

    def synthesize(challenges):
        region = custom.Assignment(meta, challenges=challenges)
        cv = region.get_challenge(ch)
        for row, (x, y) in enumerate(PHASED_TABLE):
            region.assign_fixed(t_a, row, x)
            region.assign_fixed(t_b, row, y)
        cell = None
        for row, s in enumerate(PHASED_ROWS):
            x, y = PHASED_TABLE[s]
            region.assign_advice(a, row, x)
            region.assign_advice(b, row, y)
            region.enable_selector(q, row)
            cell = region.assign_advice(w, row, (x + cv * y) % R if cv is not None else 0)
        region.copy_advice(cell, w, len(PHASED_ROWS) + 2)
        return region

    return meta, synthesize


MIXED_SA_ROWS = 24


def mixed_circuit(custom, variant: int = 0, bad: bool = False):
    """k = 6: the degree-3 gate q (a b - m), the packing gate of the XOR circuit, a permutation argument over three columns (p, m, a),
    the 2-bit XOR lookup (q a, q b, q c) in (t_a, t_b, t_c) and ONE shuffle, sa against sb (a seeded permutation with repeats) —
    shuffle_cases.mixed_circuit with its first shuffle only.  variant: the witness (the circuits of a batch differ in it); bad: the
    last triple is no row of the table."""
    meta = custom.ConstraintSystem()
    a, b, c, p, m, sa, sb = (meta.advice_column() for _ in range(7))
    t_a, t_b, t_c = (meta.fixed_column() for _ in range(3))
    q = meta.selector()
    for column in (p, m, a):
        meta.enable_equality(column)
    cur = custom.Rotation.cur()
    meta.create_gate("product", lambda meta: [meta.query_selector(q) * (meta.query_advice(a, cur) * meta.query_advice(b, cur) - meta.query_advice(m, cur))])

    def pack(meta):
        a_, b_, c_, p_ = (meta.query_advice(col, cur) for col in (a, b, c, p))
        return [meta.query_selector(q) * (a_ + b_ * 4 + c_ * 16 - p_)]

    meta.create_gate("pack", pack)
    meta.lookup("xor", lambda meta: [(meta.query_selector(q) * meta.query_advice(col, cur), meta.query_fixed(tab, cur))
                                     for col, tab in ((a, t_a), (b, t_b), (c, t_c))])
    meta.shuffle("sa is sb permuted", lambda meta: [(meta.query_advice(sa, cur), meta.query_advice(sb, cur))])
    region = custom.Assignment(meta)
    for i in range(16):
        for tab, v in ((t_a, i >> 2), (t_b, i & 3), (t_c, (i >> 2) ^ (i & 3))):
            region.assign_fixed(tab, i, v)
    triples = list(shuffle_cases.MIXED_TRIPLES[variant])
    if bad:
        triples[-1] = (1, 2, 0)  # each value occurs in its column, never together
    packed, products = [], []
    for row, (x, y, z) in enumerate(triples):
        for col, v in ((a, x), (b, y), (c, z)):
            region.assign_advice(col, row, v)
        packed.append(region.assign_advice(p, row, x + 4 * y + 16 * z))
        products.append(region.assign_advice(m, row, x * y))
        region.enable_selector(q, row)
    free = len(triples) + 1  # the selector is off there
    region.copy_advice(packed[0], p, free)
    region.copy_advice(products[1], p, free + 1)
    region.copy_advice(region.assign_advice(a, free + 2, 13 + variant), m, free + 2)
    rng = random.Random(300 + variant)
    vals = [rng.choice([2, 2, 6, R - 2, rng.randrange(R)]) for _ in range(MIXED_SA_ROWS)]
    perm = list(vals)
    rng.shuffle(perm)
    for row in range(MIXED_SA_ROWS):
        region.assign_advice(sa, row, vals[row])
        region.assign_advice(sb, row, perm[row])
    return meta, region


CASES = {"xor": 5, "any": 5, "two": 6, "phased": 6, "mixed": 6}  # name -> k


def build(custom, name: str):
    """-> (cs, assignment or synthesize(challenges), k): the 2-bit XOR tuple table, lookup_any with advice in the table and rotations,
    two lookups of degree 6 beside a gate and an instance column (tests/lookup_expr_cases.py), the two-phase circuit and the mixed one"""
    import lookup_expr_cases

    k = CASES[name]
    if name in lookup_expr_cases.CIRCUITS:
        return (*lookup_expr_cases.CIRCUITS[name][0](custom), k)
    if name == "phased":
        return (*phased_circuit(custom), k)
    return (*mixed_circuit(custom), k)


first_assignment = shuffle_cases.first_assignment
