"""Lookups given as data, shared by tests/test_lookup_exprs_host.py and tests/test_gpu_lookup_exprs.py.  oracle/ states the lookup
argument for single-expression lookups only, so this module carries the Python-integer restatement of what is new [RECALL
halo2_proofs v2023_02_02 plonk/lookup/prover.rs, plonk/lookup/verifier.rs]: the theta compression of expression lists over rows (the
fold acc theta + expr on all 2^k rows, rotations modulo 2^k; oracle.lookup.permute_expression_pair / lookup_product then apply to
the compressed columns as they are), and a verifier — oracle.flex.verify's transcript walk, quotient identity and SHPLONK check
with the two lookup lines generalised to compressed expression lists.  Then the circuits of the tests through custom.py."""
from custom_gate_cases import OP_ADVICE, OP_END, OP_FIXED, OP_MUL
from oracle import bn254 as o
from oracle import flex as FX
from oracle.flex import ADVICE, FIXED, INSTANCE, ProofReader, _lookup_terms, _permutation_terms, construct_intermediate_sets
from oracle.prover import evaluate_vanishing_polynomial, lagrange_interpolate, rotate_omega

R = o.R


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def compress(values, theta: int) -> int:
    """theta^(m-1) v_0 + ... + v_(m-1)"""
    acc = 0
    for v in values:
        acc = (acc * theta + v) % R
    return acc


def compress_rows(exprs, value, n: int, theta: int):
    """custom.Expression list -> the compressed column on all n rows; value(kind, column, row) reads a cell"""
    return [compress([e.evaluate(lambda kind, c, rot, row=row: value(kind, c, (row + rot) % n)) for e in exprs], theta) for row in range(n)]


def expr_lookups(cs):
    """a custom.ConstraintSystem's lookups as the verifier takes them: per lookup ([input g(q)], [table g(q)])"""
    call = lambda e: (lambda q, e=e: e.evaluate(q))
    return [([call(a) for a, _ in pairs], [call(t) for _, t in pairs]) for pairs in cs.lookups]


def one_pair_lookups(ocs):
    """the single-expression lookups of an oracle.flex.ConstraintSystem re-described as one-pair expression lookups"""

    def product(factors):
        def g(q):
            v = 1
            for kind, col in factors:
                v = v * q(kind, col, 0) % R
            return v

        return g

    return [([product(inp)], [product([tab])]) for inp, tab in ocs.lookups]


def one_pair_ops(abi):
    """the same re-description as a program, from an engine.ConstraintSystem's lookups[]: -> (n_pairs, ops)"""
    ops = []
    for l in range(abi.n_lookups):
        lk = abi.lookups[l]
        ops += [(OP_ADVICE, lk.input.index, 0)]
        if lk.selector_fixed >= 0:
            ops += [(OP_FIXED, lk.selector_fixed, 0), (OP_MUL, 0, 0)]
        ops += [(OP_END, 0, 0), (OP_FIXED, lk.table_fixed, 0), (OP_END, 0, 0)]
    return [1] * abi.n_lookups, ops


def verify(keys, proof: bytes, instances, lookups, g2=None, s_g2=None) -> bool:
    """oracle.flex.verify with `lookups` = [([input g(q)], [table g(q)])] in place of keys.cs.lookups: each side's expressions are
    evaluated from the opened evaluations and compressed with theta"""
    cs, n, dom = keys.cs, keys.n, keys.dom
    bf = cs.blinding_factors
    n_sets = -(-len(cs.perm_columns) // cs.chunk)
    try:
        rd = ProofReader(proof)
        rd.tr.common_scalar(keys.transcript_repr)
        for vals in instances:
            for v in vals:
                rd.tr.common_scalar(v)
        advice_c = [rd.read_point() for _ in range(cs.n_advice)]
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
    for gate in cs.gates:
        v = (v * y + gate(q)) % R
    v = _permutation_terms(cs, v, y, beta, gamma, lambda kc: evals[(kc[0], kc[1], 0)], sigma_evals, [e[0] for e in z_evals], [e[1] for e in z_evals],
                           [e[2] for e in z_evals], l_0, l_last, lact, x)
    for (ins, tabs), (lz, lz_next, ap, ap_inv, sp) in zip(lookups, lk_evals):
        a_val, t_val = compress([g(q) for g in ins], theta), compress([g(q) for g in tabs], theta)
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


def first_lookup_evaluation_offset(cs, n_lookups: int, pieces: int) -> int:
    """byte offset in a proof of the first lookup's first evaluation (z(x)): the commitments, then the evaluations before it"""
    n_sets = -(-len(cs.perm_columns) // cs.chunk)
    points = cs.n_advice + 2 * n_lookups + n_sets + n_lookups + 1 + pieces
    scalars = len(cs.advice_queries) + len(cs.fixed_queries) + 1 + len(cs.perm_columns) + (3 * n_sets - 1 if n_sets else 0)
    return 32 * (points + scalars)


def golden_range_case(g, case):
    """a committed range golden as the oracle describes it -> (oracle cs, oracle assignment)"""
    x, bits, k = int(case["x"], 16), case["lookup_bits"], case["k"]
    if "num_advice" in case:
        ocs = FX.flex_multi_cs(True, case["num_advice"], case["num_lookup_advice"])
        return ocs, FX.range_assignment_multi(ocs, x, bits, k)
    ocs = FX.flex_gate_cs(True)
    return ocs, FX.range_assignment(ocs, x, bits, 1 << k)


def golden_product_case(flex, engine, case):
    """the same golden as the product's host lays it out -> (flex cs, assignment, its ABI struct with gates = EXPRESSIONS)"""
    x, bits, k = int(case["x"], 16), case["lookup_bits"], case["k"]
    closure = lambda cs: flex.range_closure(cs, x, bits)
    cs = flex.configure(True, k, closure) if "num_advice" in case else flex.FlexGateCS(lookup=True)
    abi = cs.abi(k)
    abi.gates = engine.GATES_EXPRESSIONS
    return cs, closure(cs), abi


# ---- the circuits --------------------------------------------------------------------------------------------------------------------
XOR_BAD = {"absent": (5, 2, 7), "different rows": (1, 2, 0)}  # 5 is in no row of t_a; 1, 2 and 0 each occur in their column, never together


def xor_circuit(custom, triples=((1, 2, 3), (3, 3, 0), (0, 2, 2), (2, 1, 3)), bad=None):
    """(a) 2-bit XOR: the table (t_a, t_b, t_a ^ t_b) in three fixed columns (16 rows, the zero tuple among them), the inputs
    (q a, q b, q c) on the rows where the selector is on; a gate packs the three values into a fourth column that is copied on.
    bad: a key of XOR_BAD replaces the last triple.  -> (cs, assignment)"""
    meta = custom.ConstraintSystem()
    a, b, c, p = (meta.advice_column() for _ in range(4))
    t_a, t_b, t_c = (meta.fixed_column() for _ in range(3))
    q = meta.selector()
    meta.enable_equality(p)
    cur = custom.Rotation.cur()

    def pack(meta):
        a_, b_, c_, p_ = (meta.query_advice(col, cur) for col in (a, b, c, p))
        return [meta.query_selector(q) * (a_ + b_ * 4 + c_ * 16 - p_)]

    meta.create_gate("pack", pack)
    meta.lookup("xor", lambda meta: [(meta.query_selector(q) * meta.query_advice(col, cur), meta.query_fixed(tab, cur))
                                     for col, tab in ((a, t_a), (b, t_b), (c, t_c))])
    region = custom.Assignment(meta)
    for i in range(16):
        for tab, v in ((t_a, i >> 2), (t_b, i & 3), (t_c, (i >> 2) ^ (i & 3))):
            region.assign_fixed(tab, i, v)
    triples = list(triples)
    if bad:
        triples[-1] = XOR_BAD[bad]
    cells = []
    for row, (x, y, z) in enumerate(triples):
        for col, v in ((a, x), (b, y), (c, z)):
            region.assign_advice(col, row, v)
        cells.append(region.assign_advice(p, row, x + 4 * y + 16 * z))
        region.enable_selector(q, row)
    region.copy_advice(cells[0], p, len(triples) + 1)  # selector off there: a free cell tied to the first packed value
    return meta, region


XOR4_MARGIN = 8  # usable rows left free at the end (the copied cell sits among them)
XOR4_OFTEN = (9, 12, 5)
XOR4_ABSENT = (3, 5, 7)  # 3 ^ 5 = 6: in no table row


def xor4_rows(k: int, blinding_factors: int = 5) -> int:
    return (1 << k) - (blinding_factors + 1) - XOR4_MARGIN


def xor4_triples(k: int, seed: int = 4):
    """row -> (a, b, a ^ b), or None where the selector stays off (the zero tuple): about 60 % one triple, the rest uniform over the
    table's 256 rows, a selector off on every 97th row"""
    import random

    rng = random.Random(seed * 1000 + k)
    triples = []
    for row in range(xor4_rows(k)):
        if row % 97 == 41:
            triples.append(None)
        elif rng.random() < 0.6:
            triples.append(XOR4_OFTEN)
        else:
            x, y = rng.randrange(16), rng.randrange(16)
            triples.append((x, y, x ^ y))
    return triples


def xor4_circuit(custom, k: int, bad_row: int = None):
    """xor_circuit at any size: the 4-bit XOR table (256 rows) in three fixed columns, the inputs (q a, q b, q c) on every usable row
    but a margin at the end, the same packing gate and one copy constraint.  bad_row: that row's triple becomes XOR4_ABSENT.
    -> (cs, assignment)"""
    meta = custom.ConstraintSystem()
    a, b, c, p = (meta.advice_column() for _ in range(4))
    t_a, t_b, t_c = (meta.fixed_column() for _ in range(3))
    q = meta.selector()
    meta.enable_equality(p)
    cur = custom.Rotation.cur()

    def pack(meta):
        a_, b_, c_, p_ = (meta.query_advice(col, cur) for col in (a, b, c, p))
        return [meta.query_selector(q) * (a_ + b_ * 16 + c_ * 256 - p_)]

    meta.create_gate("pack", pack)
    meta.lookup("xor4", lambda meta: [(meta.query_selector(q) * meta.query_advice(col, cur), meta.query_fixed(tab, cur))
                                      for col, tab in ((a, t_a), (b, t_b), (c, t_c))])
    region = custom.Assignment(meta)
    for i in range(256):
        for tab, v in ((t_a, i >> 4), (t_b, i & 15), (t_c, (i >> 4) ^ (i & 15))):
            region.assign_fixed(tab, i, v)
    triples = xor4_triples(k)
    assert meta.blinding_factors() == 5 and triples[0] is not None
    if bad_row is not None:
        assert triples[bad_row] is not None
        triples[bad_row] = XOR4_ABSENT
    first = None
    for row, t in enumerate(triples):
        x, y, z = t if t is not None else (0, 0, 0)
        for col, v in ((a, x), (b, y), (c, z)):
            region.assign_advice(col, row, v)
        cell = region.assign_advice(p, row, x + 16 * y + 256 * z)
        first = first or cell
        if t is not None:
            region.enable_selector(q, row)
    region.copy_advice(first, p, len(triples) + 1)  # selector off there: a free cell tied to the first packed value
    return meta, region


def any_circuit(custom):
    """(b) lookup_any, advice in the table, rotations on both sides: (q a, q b(w^-1 X)) in (q_t x, q_t y(w X)), where a gate makes
    y(w X) = x^2 + 1 on the table's rows.  The selectors are off on the rows whose rotated query reaches a blinding row.
    Degree 2 + 2 + 2 = 6."""
    meta = custom.ConstraintSystem()
    a, b, x, y = (meta.advice_column() for _ in range(4))
    q, q_t = meta.selector(), meta.selector()
    meta.enable_equality(a)
    meta.enable_equality(x)
    cur, nxt, prv = custom.Rotation.cur(), custom.Rotation.next(), custom.Rotation.prev()

    def table_rows(meta):
        x_ = meta.query_advice(x, cur)
        return [meta.query_selector(q_t) * (meta.query_advice(y, nxt) - x_ * x_ - custom.Expression.constant(1))]

    meta.create_gate("square plus one", table_rows)
    meta.lookup_any("in the computed table", lambda meta: [
        (meta.query_selector(q) * meta.query_advice(a, cur), meta.query_selector(q_t) * meta.query_advice(x, cur)),
        (meta.query_selector(q) * meta.query_advice(b, prv), meta.query_selector(q_t) * meta.query_advice(y, nxt))])
    region = custom.Assignment(meta)
    xs = [3, 0, 7, R - 2, 11, 7, 250]
    cells = []
    for s, v in enumerate(xs):
        cells.append(region.assign_advice(x, s, v))
        region.assign_advice(y, s + 1, v * v + 1)
        region.enable_selector(q_t, s)
    for r, s in ((1, 2), (2, 0), (3, 3), (4, 6), (5, 2)):  # row r looks up table row s: a on row r, b on the row above
        cell = region.assign_advice(a, r, xs[s])
        region.assign_advice(b, r - 1, xs[s] * xs[s] + 1)
        region.enable_selector(q, r)
        if r == 1:
            region.constrain_equal(cell, cells[2])
    return meta, region


def two_lookups_circuit(custom):
    """(c) two lookups, a gate and an instance column: `la` in the fixed table t0 (one pair), and (q a, q b) in (q_t x, t1) (two
    pairs; the first has a degree-2 input and a degree-2 table side: the argument's degree 2 + 2 + 2 = 6 sets the constraint
    system's); the gate ties la to the public inputs."""
    meta = custom.ConstraintSystem()
    la, a, b, x = (meta.advice_column() for _ in range(4))
    t0, t1 = meta.fixed_column(), meta.fixed_column()
    inst = meta.instance_column()
    q, q_t, s_g = meta.selector(), meta.selector(), meta.selector()
    for column in (la, a, inst):
        meta.enable_equality(column)
    cur = custom.Rotation.cur()
    meta.create_gate("public", lambda meta: [meta.query_selector(s_g) * (meta.query_advice(la, cur) - meta.query_instance(inst, cur))])
    meta.lookup("range", lambda meta: [(meta.query_advice(la, cur), meta.query_fixed(t0, cur))])
    meta.lookup_any("pairs", lambda meta: [
        (meta.query_selector(q) * meta.query_advice(a, cur), meta.query_selector(q_t) * meta.query_advice(x, cur)),
        (meta.query_selector(q) * meta.query_advice(b, cur), meta.query_fixed(t1, cur))])
    public = [5, 2, 7]
    region = custom.Assignment(meta, instance=public)
    for i in range(8):
        region.assign_fixed(t0, i, i)
    for s in range(10):
        region.assign_advice(x, s, 3 * s + 1)
        region.assign_fixed(t1, s, s * s)
        region.enable_selector(q_t, s)
    la_cells = []
    for r, v in enumerate(public + [7, 0, 3, 3, 6]):
        la_cells.append(region.assign_advice(la, r, v))
        if r < len(public):
            region.enable_selector(s_g, r)
    region.constrain_instance(la_cells[1], inst, 1)
    for r, s in enumerate((9, 0, 4, 4, 7, 1)):
        cell = region.assign_advice(a, r + 2, 3 * s + 1)
        region.assign_advice(b, r + 2, s * s)
        region.enable_selector(q, r + 2)
        if r == 1:
            region.copy_advice(cell, a, 20)  # the selector is off on row 20: a free cell tied to this one
    return meta, region


CIRCUITS = {"xor": (xor_circuit, 5), "any": (any_circuit, 5), "two": (two_lookups_circuit, 6)}
