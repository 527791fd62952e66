"""The shuffle argument, shared by tests/test_shuffle_host.py and tests/test_gpu_shuffle.py.  oracle/ knows no shuffles, so this module
carries the Python-integer restatement of what is new [RECALL halo2_proofs, PSE line, plonk/shuffle.rs, plonk/shuffle/prover.rs,
plonk/shuffle/verifier.rs — restated from memory like everything else here and pinned to DESIGN.md 4.5, not to the crate]: the three
quotient terms of one shuffle (`shuffle_terms`), the product column (`shuffle_product`), the batched quotient of tests/batch_cases.py
with the shuffle terms behind each circuit's lookup terms, and `verify` — tests/batch_cases.verify generalised: every circuit's
shuffle products are read behind every circuit's lookup products and in front of the random polynomial, every circuit's shuffle
evaluations (z(x), z(omega x) per shuffle) behind every circuit's lookup evaluations, and per circuit the shuffle openings follow the
lookups'.  Then the circuits of the tests through custom.py, their unsatisfied variants, and what the device check must report."""
import random
from collections import Counter

import batch_cases
from batch_cases import KINDS, MAX_CIRCUITS, keys_delta, lookup_terms, permutation_terms
from lookup_expr_cases import compress
from oracle import bn254 as o
from oracle.flex import ADVICE, FIXED, INSTANCE, ProofReader, construct_intermediate_sets
from oracle.prover import evaluate_vanishing_polynomial, lagrange_interpolate, rotate_omega
from phase_cases import run_postfix

R = o.R
MAX_SHUFFLES = 8  # include/h2mi.h H2MI_MAX_SHUFFLES


# ---- the argument in Python integers -------------------------------------------------------------------------------------------------
def shuffle_terms(v, y, gamma, a_in, s_in, z, z_next, l0, l_last, l_active):
    """one shuffle's three terms folded into v with y: l_0 (1 - z), l_last (z^2 - z), l_active (z(wX) (S + gamma) - z(X) (A + gamma))"""
    v = (v * y + (1 - z) * l0) % R
    v = (v * y + (z * z - z) * l_last) % R
    v = (v * y + (z_next * (s_in + gamma) - z * (a_in + gamma)) * l_active) % R
    return v


def shuffle_product(a_rows, s_rows, gamma: int, u: int):
    """-> z[0 .. u]: z[0] = 1, z[i+1] = z[i] (A_i + gamma) / (S_i + gamma)"""
    z = [1]
    for i in range(u):
        z.append(z[-1] * (a_rows[i] + gamma) % R * pow((s_rows[i] + gamma) % R, -1, R) % R)
    return z


def num_evaluations(n_circuits, n_advice_queries, n_fixed_queries, n_perm, n_sets, n_lookups, n_shuffles) -> int:
    """the count formula of include/h2mi_prover.h"""
    return (n_circuits * n_advice_queries + n_fixed_queries + 1 + n_perm
            + n_circuits * ((3 * n_sets - 1 if n_sets else 0) + 5 * n_lookups + 2 * n_shuffles))


def batched_quotient(k, extended_k, zeta, extended_omega, delta, blinding_factors, ops, constants, challenges, circuits, shared, beta, gamma, y):
    """batch_cases.batched_quotient with shuffles: a circuit may hold "shuffles": [(compressed input, compressed shuffle side, product)],
    columns on the extended coset, whose terms follow that circuit's lookup terms"""
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
                v = lookup_terms(v, y, beta, gamma, a_val, table[idx], pin[idx], pin[prv], ptab[idx], lz[idx], lz[nxt], l0, ll, la)
            for a_in, s_in, sz in c.get("shuffles", ()):
                v = shuffle_terms(v, y, gamma, a_in[idx], s_in[idx], sz[idx], sz[nxt], l0, ll, la)
        out.append(v * t_inv[idx % rot] % R)
        x = x * extended_omega % R
    return out


# ---- the verifier ---------------------------------------------------------------------------------------------------------------------
def verify(keys, proof: bytes, instances, gates, lookups, shuffles=(), advice_phase=None, challenge_phase=(), challenges_out=None) -> bool:
    """batch_cases.verify with shuffles: [([input g(q, challenges)], [shuffle-side g(q, challenges)])] — the key's, the same for every
    circuit.  With none it reads and checks exactly what batch_cases.verify does."""
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
        lk_perm_c = [[(rd.read_point(), rd.read_point()) for _ in lookups] for _ in C]
        beta, gamma = rd.squeeze(), rd.squeeze()
        z_c = [[rd.read_point() for _ in range(n_sets)] for _ in C]
        lz_c = [[rd.read_point() for _ in lookups] for _ in C]
        sz_c = [[rd.read_point() for _ in shuffles] for _ in C]  # the shuffle products: behind the lookups', in front of the random polynomial
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
        lk_evals = [[tuple(rd.read_scalar() for _ in range(5)) for _ in lookups] for _ in C]
        sf_evals = [[(rd.read_scalar(), rd.read_scalar()) for _ in shuffles] for _ in C]  # every circuit's shuffles behind every circuit's lookups
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
        for (ins, tabs), (lz, lz_next, ap, ap_inv, sp) in zip(lookups, lk_evals[i]):
            a_val, t_val = compress([g(q, challenges) for g in ins], theta), compress([g(q, challenges) for g in tabs], theta)
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
        for li, (lz, lz_next, ap, ap_inv, sp) in enumerate(lk_evals[i]):
            qq(("lz", i, li), lz_c[i][li], x, lz)
            qq(("la", i, li), lk_perm_c[i][li][0], x, ap)
            qq(("ls", i, li), lk_perm_c[i][li][1], x, sp)
            qq(("la", i, li), lk_perm_c[i][li][0], x_inv, ap_inv)
            qq(("lz", i, li), lz_c[i][li], x_next, lz_next)
        for si, (sz, sz_next) in enumerate(sf_evals[i]):  # shuffles.open follows lookups.open
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


def expr_shuffles(cs):
    """a custom.ConstraintSystem's shuffles as the verifier takes them: per shuffle ([input g(q, challenges)], [shuffle-side g])"""
    call = lambda e: (lambda q, ch, e=e: e.evaluate(q, ch))
    return [([call(a) for a, _ in pairs], [call(s) for _, s in pairs]) for pairs in cs.shuffles]


def verify_circuits(vk, cs, proof: bytes, instances, challenges_out=None) -> bool:
    """`verify` for N circuits of one custom.ConstraintSystem; instances[i]: circuit i's public inputs (one instance column at most)"""
    from phase_cases import expr_gates, expr_lookups

    per_circuit = [[list(v)] if cs.n_instance else [] for v in instances]
    return verify(vk, proof, per_circuit, expr_gates(cs), expr_lookups(cs), expr_shuffles(cs), cs.advice_phase, cs.challenge_phase,
                  challenges_out=challenges_out)


def proof_offsets(cs, n_circuits: int = 1):
    """-> (byte offset of the first shuffle product commitment, byte offset of the first shuffle evaluation) in a proof of n_circuits
    circuits of a custom.ConstraintSystem: points and scalars are 32 bytes each, in the order `verify` reads them"""
    m, chunk = len(cs.perm_columns), cs.degree() - 2
    n_sets = -(-m // chunk)
    L, S, N = len(cs.lookups), len(cs.shuffles), n_circuits
    points_before = N * cs.n_advice + N * 2 * L + N * n_sets + N * L
    after_products = points_before + N * S + 1 + (cs.degree() - 1)
    evals_before = N * len(cs.advice_queries) + len(cs.fixed_queries) + 1 + m + N * ((3 * n_sets - 1 if n_sets else 0) + 5 * L)
    return 32 * points_before, 32 * (after_products + evals_before)


# ---- what the device check must report ------------------------------------------------------------------------------------------------
def shuffle_rows(cs, asg, k: int, challenges=()):
    """per shuffle (input tuples, shuffle-side tuples) on all 2^k rows of an assignment, in Python integers"""
    n = 1 << k
    value = {ADVICE: lambda c, r: asg.advice[c].get(r, 0), FIXED: lambda c, r: asg.fixed[c].get(r, 0),
             INSTANCE: lambda c, r: asg.instance[r] if r < len(asg.instance) else 0}
    at = lambda e, row: e.evaluate(lambda kind, c, rot: value[kind](c, (row + rot) % n), challenges)
    return [([tuple(at(a, row) for a, _ in pairs) for row in range(n)], [tuple(at(s, row) for _, s in pairs) for row in range(n)]) for pairs in cs.shuffles]


def expected_failures(cs, asg, k: int, challenges=()):
    """-> [(shuffle index, smallest failing row, failing rows)]: the usable rows whose input tuple occurs more often among the inputs
    than on the shuffle side"""
    u = (1 << k) - (cs.blinding_factors() + 1)
    out = []
    for index, (ins, shs) in enumerate(shuffle_rows(cs, asg, k, challenges)):
        have, want = Counter(ins[:u]), Counter(shs[:u])
        bad = [row for row in range(u) if have[ins[row]] > want[ins[row]]]
        if bad:
            out.append((index, bad[0], len(bad)))
    return out


# ---- the circuits ----------------------------------------------------------------------------------------------------------------------
PERM_ROWS = 20


def perm_circuit(custom, seed: int = 1, bad: str = None):
    """k = 5: one shuffle of one pair, advice a against advice b, b a seeded permutation of a with repeated values; a trivial gate, no
    lookups, no permutation argument: the shuffle terms are the only argument terms.  bad: "cell" alters one cell of b; "multiplicity"
    makes a = [1, 1, 2, ..] against b = [1, 2, 2, ..] (the sets are equal, the multiplicities are not).  -> (cs, assignment)"""
    meta = custom.ConstraintSystem()
    a, b = meta.advice_column(), meta.advice_column()
    q = meta.selector()
    cur = custom.Rotation.cur()
    meta.create_gate("trivial", lambda meta: [meta.query_selector(q) * (meta.query_advice(a, cur) - meta.query_advice(a, cur))])
    meta.shuffle("a is b permuted", lambda meta: [(meta.query_advice(a, cur), meta.query_advice(b, cur))])
    rng = random.Random(100 + seed)
    vals = [rng.choice([3, 3, 7, 11, R - 1, rng.randrange(R)]) for _ in range(PERM_ROWS)]
    perm = list(vals)
    rng.shuffle(perm)
    if bad == "multiplicity":  # the rows behind the first three stay a permutation of each other
        perm = vals[3:]
        rng.shuffle(perm)
        vals, perm = [1, 1, 2] + vals[3:], [1, 2, 2] + perm
    if bad == "cell":
        perm[3] = (perm[3] + 1) % R
    region = custom.Assignment(meta)
    for row in range(PERM_ROWS):
        region.assign_advice(a, row, vals[row])
        region.assign_advice(b, row, perm[row])
    region.enable_selector(q, 0)
    return meta, region


TUPLE_IN_ROWS, TUPLE_SH_ROWS = range(0, 10), range(3, 13)


def tuple_circuit(custom, seed: int = 2, bad: bool = False):
    """k = 6: one shuffle of three pairs, inputs (q a, q a(wX), q c) against (q' d(w^-1 X), q' e, q' f + instance): degree 2 on both
    sides, required degree 4.  q is on on rows 0 .. 9, q' on rows 3 .. 12: the two sides' row sets differ, the rows outside hold the
    zero tuple on both sides, and the rotations wrap around 2^k inside the compression."""
    meta = custom.ConstraintSystem()
    a, c, d, e, f = (meta.advice_column() for _ in range(5))
    inst = meta.instance_column()
    q, q2 = meta.selector(), meta.selector()
    cur, nxt, prv = custom.Rotation.cur(), custom.Rotation.next(), custom.Rotation.prev()
    meta.create_gate("trivial", lambda meta: [meta.query_selector(q) * (meta.query_advice(a, cur) - meta.query_advice(a, cur))])
    meta.shuffle("tuples", lambda meta: [
        (meta.query_selector(q) * meta.query_advice(a, cur), meta.query_selector(q2) * meta.query_advice(d, prv)),
        (meta.query_selector(q) * meta.query_advice(a, nxt), meta.query_selector(q2) * meta.query_advice(e, cur)),
        (meta.query_selector(q) * meta.query_advice(c, cur), meta.query_selector(q2) * meta.query_advice(f, cur) + meta.query_instance(inst, cur))])
    rng = random.Random(200 + seed)
    a_vals = [rng.choice([0, 5, 5, rng.randrange(R)]) for _ in range(len(TUPLE_IN_ROWS) + 1)]
    c_vals = [rng.choice([0, 9, rng.randrange(R)]) for _ in TUPLE_IN_ROWS]
    tuples = [(a_vals[i], a_vals[i + 1], c_vals[i]) for i in range(len(TUPLE_IN_ROWS))]
    order = list(range(len(tuples)))
    rng.shuffle(order)
    public = [0] * TUPLE_SH_ROWS[0] + [rng.choice([0, 1, rng.randrange(R)]) for _ in TUPLE_SH_ROWS]  # zero wherever q' is off
    region = custom.Assignment(meta, instance=public)
    for i, row in enumerate(TUPLE_IN_ROWS):
        region.assign_advice(a, row, a_vals[i])
        region.assign_advice(c, row, c_vals[i])
        region.enable_selector(q, row)
    region.assign_advice(a, TUPLE_IN_ROWS[-1] + 1, a_vals[-1])
    for j, row in enumerate(TUPLE_SH_ROWS):
        t0, t1, t2 = tuples[order[j]]
        region.assign_advice(d, row - 1, t0)
        region.assign_advice(e, row, (t1 + 1) % R if bad and j == 4 else t1)
        region.assign_advice(f, row, (t2 - public[row]) % R)
        region.enable_selector(q2, row)
    return meta, region


MIXED_TRIPLES = [((1, 2, 3), (3, 3, 0), (0, 2, 2), (2, 1, 3), (1, 2, 3)), ((0, 0, 0), (1, 1, 0), (3, 0, 3), (2, 3, 1), (3, 0, 3))]
MIXED_SA_ROWS = 24


def mixed_circuit(custom, variant: int = 0, bad: int = None, shuffles: bool = True):
    """k = 6: a degree-3 gate q (a b - m), the packing gate of the XOR circuit, a permutation argument over three columns (p, m, a),
    the 2-bit XOR lookup (q a, q b, q c) in (t_a, t_b, t_c), and two shuffles: sa against sb (one pair, a seeded permutation with
    repeats) and (q a, q b) against (u1, u2) (two pairs).  variant: the witness (the circuits of a batch differ in it); bad: the
    index of a shuffle to break in one cell; shuffles = False: the same circuit and witness without the two shuffle arguments."""
    meta = custom.ConstraintSystem()
    a, b, c, p, m, sa, sb, u1, u2 = (meta.advice_column() for _ in range(9))
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
    if shuffles:
        meta.shuffle("sa is sb permuted", lambda meta: [(meta.query_advice(sa, cur), meta.query_advice(sb, cur))])
        meta.shuffle("pairs", lambda meta: [(meta.query_selector(q) * meta.query_advice(a, cur), meta.query_advice(u1, cur)),
                                            (meta.query_selector(q) * meta.query_advice(b, cur), meta.query_advice(u2, cur))])
    region = custom.Assignment(meta)
    for i in range(16):
        for tab, v in ((t_a, i >> 2), (t_b, i & 3), (t_c, (i >> 2) ^ (i & 3))):
            region.assign_fixed(tab, i, v)
    triples = MIXED_TRIPLES[variant]
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
    if bad == 0:
        perm[5] = (perm[5] + 1) % R
    for row in range(MIXED_SA_ROWS):
        region.assign_advice(sa, row, vals[row])
        region.assign_advice(sb, row, perm[row])
    order = list(range(len(triples)))
    rng.shuffle(order)
    for j, i in enumerate(order):  # the selected (a, b) pairs, permuted, on rows 30 ..: every other row holds the zero pair on both sides
        x, y, _ = triples[i]
        region.assign_advice(u1, 30 + j, x)
        region.assign_advice(u2, 30 + j, (y + 1) % R if bad == 1 and j == 2 else y)
    return meta, region


PHASED_ROWS = 12


def phased_circuit(custom, seed: int = 4):
    """k = 6: phase-0 columns a, b, d, e with (d, e) a seeded permutation of the (a, b) rows; a challenge c usable after phase 0; a
    second-phase column w with q (w - a - c b); the shuffle of a + c b against d + c e (one pair, a challenge on both sides).
    -> (cs, synthesize)"""
    meta = custom.ConstraintSystem()
    a, b, d, e = (meta.advice_column() for _ in range(4))
    ch = meta.challenge_usable_after(0)
    w = meta.advice_column_in(1)
    q = meta.selector()
    meta.enable_equality(w)
    cur = custom.Rotation.cur()
    meta.create_gate("w = a + c b", lambda meta: [meta.query_selector(q) * (meta.query_advice(w, cur) - meta.query_advice(a, cur)
                                                                           - meta.query_challenge(ch) * meta.query_advice(b, cur))])
    meta.shuffle("rlc rows", lambda meta: [(meta.query_advice(a, cur) + meta.query_challenge(ch) * meta.query_advice(b, cur),
                                            meta.query_advice(d, cur) + meta.query_challenge(ch) * meta.query_advice(e, cur))])
    rng = random.Random(400 + seed)
    rows = [(rng.choice([1, 4, rng.randrange(R)]), rng.choice([0, 8, rng.randrange(R)])) for _ in range(PHASED_ROWS)]
    perm = list(rows)
    rng.shuffle(perm)

    def synthesize(challenges):
        region = custom.Assignment(meta, challenges=challenges)
        cv = region.get_challenge(ch)
        cell = None
        for row, ((x, y), (x2, y2)) in enumerate(zip(rows, perm)):
            region.assign_advice(a, row, x)
            region.assign_advice(b, row, y)
            region.assign_advice(d, row + 7, x2)  # other rows than the inputs'
            region.assign_advice(e, row + 7, y2)
            region.enable_selector(q, row)
            cell = region.assign_advice(w, row, (x + cv * y) % R if cv is not None else 0)
        region.copy_advice(cell, w, PHASED_ROWS + 2)
        return region

    return meta, synthesize


CASES = {"perm": 5, "tuple": 6, "mixed": 6, "phased": 6}  # name -> k


def build(custom, name: str):
    """-> (cs, assignment or synthesize(challenges), k)"""
    k = CASES[name]
    if name == "perm":
        return (*perm_circuit(custom), k)
    if name == "tuple":
        return (*tuple_circuit(custom), k)
    if name == "mixed":
        return (*mixed_circuit(custom), k)
    return (*phased_circuit(custom), k)


def first_assignment(cs, asg):
    """the assignment keygen reads the fixed cells and copies from (a phased circuit: the run of synthesize() without challenges)"""
    return asg([None] * len(cs.challenge_phase)) if callable(asg) else asg


__all__ = ["batch_cases"]
