"""Advice phases and challenges, shared by tests/test_phases_host.py and tests/test_gpu_phases.py.  oracle/ knows no phases, so this
module carries the Python-integer restatement of what is new [RECALL halo2_proofs v2023_02_02 plonk/prover.rs, plonk/verifier.rs]: a
verifier — tests/lookup_expr_cases.py's `verify` with two changes: the advice commitments are read phase by phase with the squeezes
of that phase's challenges (in index order) behind each phase, and the gate and lookup callables are given the challenges.  Then the
circuits of the tests through custom.py, and a postfix stack machine that knows the CHALLENGE op."""
from custom_gate_cases import OP_ADD, OP_ADVICE, OP_CONSTANT, OP_END, OP_FIXED, OP_INSTANCE, OP_MUL, OP_NEG, OP_SUB  # noqa: F401
from lookup_expr_cases import compress
from oracle import bn254 as o
from oracle.flex import ADVICE, FIXED, INSTANCE, ProofReader, _lookup_terms, _permutation_terms, construct_intermediate_sets
from oracle.prover import evaluate_vanishing_polynomial, lagrange_interpolate, rotate_omega

R = o.R
OP_CHALLENGE = 9  # include/h2mi.h H2MI_EXPR_CHALLENGE: appended behind END


def run_postfix(ops, constants, q, challenges=()):
    """the stack machine of include/h2mi.h on Python integers, CHALLENGE included: -> one value per polynomial"""
    stack, out = [], []
    for op, index, rotation in ops:
        if op <= OP_INSTANCE:
            stack.append(q(op, index, rotation) % R)
        elif op == OP_CONSTANT:
            stack.append(constants[index] % R)
        elif op == OP_CHALLENGE:
            stack.append(challenges[index] % R)
        elif op == OP_NEG:
            stack.append(-stack.pop() % R)
        elif op == OP_END:
            assert len(stack) == 1
            out.append(stack.pop())
        else:
            b, a = stack.pop(), stack.pop()
            stack.append((a + b if op == OP_ADD else a - b if op == OP_SUB else a * b) % R)
    assert not stack
    return out


def compress_rows(exprs, value, n: int, theta: int, challenges=()):
    """custom.Expression list -> the theta-compressed column on all n rows; value(kind, column, row) reads a cell"""
    return [compress([e.evaluate(lambda kind, c, rot, row=row: value(kind, c, (row + rot) % n), challenges) for e in exprs], theta) for row in range(n)]


def expr_gates(cs):
    """a custom.ConstraintSystem's gate polynomials as the verifier takes them: g(q, challenges)"""
    return [(lambda q, ch, p=p: p.evaluate(q, ch)) for p in cs.polynomials]


def expr_lookups(cs):
    """its lookups: per lookup ([input g(q, challenges)], [table g(q, challenges)])"""
    call = lambda e: (lambda q, ch, e=e: e.evaluate(q, ch))
    return [([call(a) for a, _ in pairs], [call(t) for _, t in pairs]) for pairs in cs.lookups]


def without_challenges(gates):
    """callables g(q) of a circuit that has no challenge, in the verifier's form"""
    return [(lambda q, ch, g=g: g(q)) for g in gates]


def without_challenges_lookups(lookups):
    return [(without_challenges(ins), without_challenges(tabs)) for ins, tabs in lookups]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def verify(keys, proof: bytes, instances, gates, lookups, advice_phase=None, challenge_phase=(), g2=None, s_g2=None, challenges_out=None) -> bool:
    """lookup_expr_cases.verify with advice phases: advice_phase[j] is the phase of advice column j (None: all in phase 0),
    challenge_phase[i] the phase after which challenge i is squeezed.  gates: [g(q, challenges)]; lookups: [([input g(q, challenges)],
    [table g(q, challenges)])].  challenges_out: a list that receives the challenge values."""
    cs, n, dom = keys.cs, keys.n, keys.dom
    bf = cs.blinding_factors
    n_sets = -(-len(cs.perm_columns) // cs.chunk)
    advice_phase = [0] * cs.n_advice if advice_phase is None else list(advice_phase)
    challenges = [None] * len(challenge_phase)
    try:
        rd = ProofReader(proof)
        rd.tr.common_scalar(keys.transcript_repr)
        for vals in instances:
            for v in vals:
                rd.tr.common_scalar(v)
        advice_c = [None] * cs.n_advice
        for phase in range(1 + max(advice_phase, default=0)):
            for j in range(cs.n_advice):  # this phase's commitments, in column order
                if advice_phase[j] == phase:
                    advice_c[j] = rd.read_point()
            for i, p in enumerate(challenge_phase):  # then its challenges, in index order
                if p == phase:
                    challenges[i] = rd.squeeze()
        theta = rd.squeeze()
        lk_perm_c = [(rd.read_point(), rd.read_point()) for _ in lookups]
        beta, gamma = rd.squeeze(), rd.squeeze()
        z_c = [rd.read_point() for _ in range(n_sets)]
        lz_c = [rd.read_point() for _ in lookups]
        random_c = rd.read_point()
        y = rd.squeeze()
        h_c = [rd.read_point() for _ in range(dom.quotient_poly_degree)]
        x = rd.squeeze()
        advice_evals = [rd.read_scalar() for _ in cs.advice_queries]
        fixed_evals = [rd.read_scalar() for _ in cs.fixed_queries]
        random_eval = rd.read_scalar()
        sigma_evals = [rd.read_scalar() for _ in cs.perm_columns]
        z_evals = []
        for i in range(n_sets):
            e, en = rd.read_scalar(), rd.read_scalar()
            z_evals.append((e, en, rd.read_scalar() if i + 1 < n_sets else None))
        lk_evals = [tuple(rd.read_scalar() for _ in range(5)) for _ in lookups]
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
    instance_evals = []
    for c, r in cs.instance_queries:
        pt = rotate_omega(dom, x, r)
        ptn = pow(pt, n, R)
        instance_evals.append(sum(v * ((ptn - 1) * pow(n, -1, R) % R * pow(w, i, R) % R * pow((pt - pow(w, i, R)) % R, -1, R) % R)
                                  for i, v in enumerate(instances[c])) % R)
    evals = {}
    for qi, (c, r) in enumerate(cs.advice_queries):
        evals[(ADVICE, c, r)] = advice_evals[qi]
    for qi, (c, r) in enumerate(cs.fixed_queries):
        evals[(FIXED, c, r)] = fixed_evals[qi]
    for qi, (c, r) in enumerate(cs.instance_queries):
        evals[(INSTANCE, c, r)] = instance_evals[qi]
    q = lambda kind, col, r: evals[(kind, col, r)]
    v = 0
    for gate in gates:
        v = (v * y + gate(q, challenges)) % R
    v = _permutation_terms(cs, v, y, beta, gamma, lambda kc: evals[(kc[0], kc[1], 0)], sigma_evals, [e[0] for e in z_evals], [e[1] for e in z_evals],
                           [e[2] for e in z_evals], l_0, l_last, lact, x)
    for (ins, tabs), (lz, lz_next, ap, ap_inv, sp) in zip(lookups, lk_evals):
        a_val, t_val = compress([g(q, challenges) for g in ins], theta), compress([g(q, challenges) for g in tabs], theta)
        v = _lookup_terms(v, y, beta, gamma, a_val, t_val, ap, ap_inv, sp, lz, lz_next, l_0, l_last, lact)
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

    for qi, (c, r) in enumerate(cs.advice_queries):
        qq(("advice", c), advice_c[c], rx(r), advice_evals[qi])
    for i in range(n_sets):
        qq(("z", i), z_c[i], x, z_evals[i][0])
        qq(("z", i), z_c[i], x_next, z_evals[i][1])
    for i in reversed(range(n_sets - 1)):
        qq(("z", i), z_c[i], x_last, z_evals[i][2])
    for li, (lz, lz_next, ap, ap_inv, sp) in enumerate(lk_evals):
        qq(("lz", li), lz_c[li], x, lz)
        qq(("la", li), lk_perm_c[li][0], x, ap)
        qq(("ls", li), lk_perm_c[li][1], x, sp)
        qq(("la", li), lk_perm_c[li][0], x_inv, ap_inv)
        qq(("lz", li), lz_c[li], x_next, lz_next)
    for qi, (c, r) in enumerate(cs.fixed_queries):
        qq(("fixed", c), keys.fixed_commitments[c], rx(r), fixed_evals[qi])
    for i in range(len(cs.perm_columns)):
        qq(("sigma", i), keys.permutation_commitments[i], x, sigma_evals[i])
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
    for i, (pts, comms) in enumerate(rotation_sets):
        z_diff = evaluate_vanishing_polynomial([p for p in super_points if p not in pts], uu)
        if i == 0:
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
    if g2 is not None and s_g2 is not None:
        from oracle import pairing

        return pairing.pairing_product_is_one([(h2, s_g2), (o.g1_neg(outer), g2)]) if outer is not None else h2 is None
    return o.g1_mul(keys.s, h2) == outer


def verify_circuit(vk, cs, proof: bytes, instances, challenges_out=None) -> bool:
    """`verify` for a custom.ConstraintSystem"""
    return verify(vk, proof, instances, expr_gates(cs), expr_lookups(cs), cs.advice_phase, cs.challenge_phase, challenges_out=challenges_out)


# ---- the circuits --------------------------------------------------------------------------------------------------------------------
RLC_VALUES = (3, 1, 4, 1, 5, 9, 2, R - 6)


def rlc_circuit(custom, gamma_offset: int = 0, values=RLC_VALUES):
    """Two phases: a running linear combination.  Phase-0 column `a`, challenge gamma usable after phase 0, phase-1 column `acc` with
    q_first (acc - a) and q (acc(wX) - gamma acc - a(wX)): acc_0 = a_0, acc_(i+1) = gamma acc_i + a_(i+1).  The last acc cell is copied
    to a free cell of its column.  gamma_offset: the phase-1 witness is made with gamma + gamma_offset (a wrong witness).
    -> (cs, synthesize), synthesize(challenges) -> Assignment; with gamma unknown the phase-1 column stays unassigned."""
    meta = custom.ConstraintSystem()
    a = meta.advice_column()
    gamma = meta.challenge_usable_after(0)
    acc = meta.advice_column_in(1)
    q_first, q = meta.selector(), meta.selector()
    meta.enable_equality(acc)
    cur, nxt = custom.Rotation.cur(), custom.Rotation.next()
    meta.create_gate("rlc first", lambda meta: [meta.query_selector(q_first) * (meta.query_advice(acc, cur) - meta.query_advice(a, cur))])
    meta.create_gate("rlc step", lambda meta: [meta.query_selector(q) * (meta.query_advice(acc, nxt) - meta.query_challenge(gamma) * meta.query_advice(acc, cur)
                                                                         - meta.query_advice(a, nxt))])

    def synthesize(challenges):
        region = custom.Assignment(meta, challenges=challenges)
        for row, v in enumerate(values):
            region.assign_advice(a, row, v)
        region.enable_selector(q_first, 0)
        for row in range(len(values) - 1):
            region.enable_selector(q, row)
        g = region.get_challenge(gamma)
        run = values[0] % R
        cell = None
        for row, v in enumerate(values):
            if row:
                run = (((g or 0) + gamma_offset) * run + v) % R
            cell = region.assign_advice(acc, row, run if g is not None else 0)
        region.copy_advice(cell, acc, len(values) + 1)  # the selectors are off there
        return region

    return meta, synthesize


THREE_TABLE = [(0, 0), (1, 2), (2, 3), (3, 5), (4, 7), (5, 11), (6, 13), (7, 17)]  # (t_a, t_b): 8 rows, the zero tuple first
THREE_ROWS = (3, 1, 7, 7, 0, 5)  # the table row each selected witness row holds


def three_phase_circuit(custom, c0_offset: int = 0):
    """Three phases and a challenge inside a lookup.  Phase-0 columns a, b; challenge c0 after phase 0; phase-1 column r with
    q (r - a - c0 b); the lookup of q r in t_a + c0 t_b (a fixed 8-row table that holds the zero tuple; every selected (a, b) is one
    of its rows) — an RLC'd tuple lookup in one pair; challenge c1 after phase 1; phase-2 column w with q (w - c1 r - a); an instance
    column tied to the first a.  c0_offset: the phase-1 witness is made with c0 + c0_offset.  -> (cs, synthesize)"""
    meta = custom.ConstraintSystem()
    a, b = meta.advice_column(), meta.advice_column()
    c0 = meta.challenge_usable_after(0)
    r = meta.advice_column_in(1)
    c1 = meta.challenge_usable_after(1)
    w = meta.advice_column_in(2)
    t_a, t_b = meta.fixed_column(), meta.fixed_column()
    inst = meta.instance_column()
    q = meta.selector()
    meta.enable_equality(a)
    meta.enable_equality(inst)
    cur = custom.Rotation.cur()
    meta.create_gate("r = a + c0 b", lambda meta: [meta.query_selector(q) * (meta.query_advice(r, cur) - meta.query_advice(a, cur)
                                                                            - meta.query_challenge(c0) * meta.query_advice(b, cur))])
    meta.lookup_any("rlc in table", lambda meta: [(meta.query_selector(q) * meta.query_advice(r, cur),
                                                   meta.query_fixed(t_a, cur) + meta.query_challenge(c0) * meta.query_fixed(t_b, cur))])
    meta.create_gate("w = c1 r + a", lambda meta: [meta.query_selector(q) * (meta.query_advice(w, cur) - meta.query_challenge(c1) * meta.query_advice(r, cur)
                                                                            - meta.query_advice(a, cur))])

    def synthesize(challenges):
        region = custom.Assignment(meta, instance=[THREE_TABLE[THREE_ROWS[0]][0]], challenges=challenges)
        for row, (x, y) in enumerate(THREE_TABLE):
            region.assign_fixed(t_a, row, x)
            region.assign_fixed(t_b, row, y)
        v0, v1 = region.get_challenge(c0), region.get_challenge(c1)
        for row, t in enumerate(THREE_ROWS):
            x, y = THREE_TABLE[t]
            cell = region.assign_advice(a, row, x)
            region.assign_advice(b, row, y)
            region.enable_selector(q, row)
            if row == 0:
                region.constrain_instance(cell, inst, 0)
            rv = (x + ((v0 or 0) + c0_offset) * y) % R
            region.assign_advice(r, row, rv if v0 is not None else 0)
            region.assign_advice(w, row, ((v1 or 0) * rv + x) % R if v1 is not None else 0)
        return region

    return meta, synthesize


CIRCUITS = {"rlc": (rlc_circuit, 5), "three": (three_phase_circuit, 6)}
