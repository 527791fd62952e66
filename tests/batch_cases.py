"""Several circuits per proof, shared by tests/test_batch_host.py and tests/test_gpu_batch.py.  oracle/ knows one circuit per proof, so
this module carries the Python-integer restatement of what is new [RECALL halo2_proofs v2023_02_02 plonk/prover.rs, plonk/verifier.rs,
plonk/evaluation.rs]: the verifier of tests/phase_cases.py generalised to N circuits against one key — per advice phase every
circuit's commitments in circuit order, then that phase's challenges; theta; every circuit's permuted pairs; beta, gamma; every
circuit's permutation products; every circuit's lookup products; ONE random polynomial; y; the h pieces; x; the evaluations (every
circuit's advice, fixed, random, sigma, every circuit's permutation sets, every circuit's lookups); the multiopen queries per circuit
(advice, permutation, lookups), then fixed, sigma, h, random — and the batched quotient on the extended coset: per point ONE value
folded with y over every circuit's gate polynomials, permutation terms and lookup terms in circuit order, divided by X^n - 1 once,
written out from the formulas of DESIGN.md 4.2 / 4.5 and not obtained by calling the library."""
import random

from custom_gate_cases import OP_ADVICE, OP_FIXED, OP_INSTANCE  # noqa: F401
from lookup_expr_cases import compress
from oracle import bn254 as o
from oracle.flex import ADVICE, FIXED, INSTANCE, ProofReader, construct_intermediate_sets
from oracle.prover import evaluate_vanishing_polynomial, lagrange_interpolate, rotate_omega
from phase_cases import run_postfix

R = o.R
MAX_CIRCUITS = 8  # include/h2mi.h H2MI_MAX_CIRCUITS


# ---- one circuit's permutation and lookup terms, folded into v with y (evaluate_h's order) -----------------------------
def permutation_terms(v, y, beta, gamma, delta, chunk, values, sigmas, z, z_next, z_last, l0, l_last, l_active, x):
    """values / sigmas: the m permuted columns and their sigma at the point; z / z_next: every set's product at the point and at omega
    times it; z_last[s]: set s at omega^-(blinding_factors + 1) times it (read for all but the last set); x: the point itself"""
    m = len(values)
    if not m:
        return v
    sets = -(-m // chunk)
    v = (v * y + (1 - z[0]) * l0) % R
    v = (v * y + (z[sets - 1] * z[sets - 1] - z[sets - 1]) * l_last) % R
    for s in range(1, sets):
        v = (v * y + (z[s] - z_last[s - 1]) * l0) % R
    cur = beta * x % R
    for s in range(sets):
        left, right = z_next[s], z[s]
        for j in range(chunk * s, min(m, chunk * (s + 1))):
            left = left * (values[j] + beta * sigmas[j] + gamma) % R
            right = right * (values[j] + cur + gamma) % R
            cur = cur * delta % R
        v = (v * y + (left - right) * l_active) % R
    return v


def lookup_terms(v, y, beta, gamma, a_in, t_in, ap, ap_prev, sp, lz, lz_next, l0, l_last, l_active):
    v = (v * y + (1 - lz) * l0) % R
    v = (v * y + (lz * lz - lz) * l_last) % R
    v = (v * y + (lz_next * (ap + beta) % R * (sp + gamma) - lz * (a_in + beta) % R * (t_in + gamma)) * l_active) % R
    v = (v * y + (ap - sp) * l0) % R
    v = (v * y + (ap - sp) * (ap - ap_prev) % R * l_active) % R
    return v


def horner_terms(n_polys: int, n_perm: int, chunk: int, n_lookups: int) -> int:
    """how many times one circuit multiplies the accumulator by y"""
    sets = -(-n_perm // chunk) if n_perm else 0
    return n_polys + (2 + (sets - 1) + sets if n_perm else 0) + 5 * n_lookups


# ---- the batched quotient on the extended coset -------------------------------------------------------------------------------------
KINDS = {0: "advice", 1: "fixed", 2: "instance"}


def batched_quotient(k, extended_k, zeta, extended_omega, delta, blinding_factors, ops, constants, challenges, circuits, shared, beta, gamma, y):
    """-> h on the 2^extended_k points.  circuits: per circuit {"advice": [column], "fixed": [column], "instance": column or None,
    "perm_values": [column], "perm_zs": [column], "lookups": [(input, second input factor or None, table, permuted input, permuted
    table, product)]}, every column a list of 2^extended_k integers; shared: {"perm_sigmas", "chunk", "l0", "l_last", "l_active"}.
    A rotation r reads point idx + r 2^(extended_k - k)."""
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
        for c in circuits:  # ONE value walks the circuits
            cols = {"advice": c["advice"], "fixed": c["fixed"], "instance": [c.get("instance")]}
            for poly in run_postfix(ops, constants, lambda op, col, r: cols[KINDS[op]][col][at(r)], challenges):
                v = (v * y + poly) % R
            zs = c["perm_zs"]
            v = permutation_terms(v, y, beta, gamma, delta, chunk, [p[idx] for p in c["perm_values"]], [s[idx] for s in sig], [z[idx] for z in zs],
                                  [z[nxt] for z in zs], [z[lst] for z in zs], l0, ll, la, x)
            for a_in, b_in, table, pin, ptab, lz in c["lookups"]:
                a_val = a_in[idx] * b_in[idx] % R if b_in is not None else a_in[idx]
                v = lookup_terms(v, y, beta, gamma, a_val, table[idx], pin[idx], pin[prv], ptab[idx], lz[idx], lz[nxt], l0, ll, la)
        out.append(v * t_inv[idx % rot] % R)  # the division comes behind the last circuit
        x = x * extended_omega % R
    return out


# ---- the verifier for N circuits ------------------------------------------------------------------------------------------------------
def verify(keys, proof: bytes, instances, gates, lookups, advice_phase=None, challenge_phase=(), challenges_out=None) -> bool:
    """phase_cases.verify for N = len(instances) circuits against one key.  instances[i]: circuit i's public inputs, one list per
    instance column.  gates: [g(q, challenges)]; lookups: [([input g], [table g])] — the key's, the same for every circuit."""
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
            for i in C:  # every circuit's commitments of this phase, in circuit then column order
                for j in range(cs.n_advice):
                    if advice_phase[j] == phase:
                        advice_c[i][j] = rd.read_point()
            for ci, p in enumerate(challenge_phase):  # then the phase's challenges, once for the proof
                if p == phase:
                    challenges[ci] = rd.squeeze()
        theta = rd.squeeze()
        lk_perm_c = [[(rd.read_point(), rd.read_point()) for _ in lookups] for _ in C]
        beta, gamma = rd.squeeze(), rd.squeeze()
        z_c = [[rd.read_point() for _ in range(n_sets)] for _ in C]
        lz_c = [[rd.read_point() for _ in lookups] for _ in C]
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
    for i in C:  # ONE value walks the circuits, as the prover's evaluate_h does
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


def keys_delta() -> int:
    """the permutation argument's DELTA: a generator of the multiplicative group's odd-order part (oracle/plonk.py FR_DELTA)"""
    from oracle import plonk as P

    return P.FR_DELTA


def verify_circuits(vk, cs, proof: bytes, instances, challenges_out=None) -> bool:
    """`verify` for N circuits of one custom.ConstraintSystem; instances[i]: circuit i's public inputs (one instance column at most)"""
    from phase_cases import expr_gates, expr_lookups

    per_circuit = [[list(v)] if cs.n_instance else [] for v in instances]
    return verify(vk, proof, per_circuit, expr_gates(cs), expr_lookups(cs), cs.advice_phase, cs.challenge_phase, challenges_out=challenges_out)


# ---- kernel cases: random columns on the extended coset (the kernel works point by point: they need not be polynomials) --------------
N_ADV, N_FIX, N_CH = 3, 2, 4
# (k, cs degree -> extended_k = k + 1 .. k + 3, circuits, stack depth of the program, challenges?, n_perm, chunk, lookups, share)
# 32, 256 and 512 points: less than one workgroup, exactly one, two.  n_perm = 0, or two chunk sets; lookups 0 or 2, one of them with
# a second input factor.  share: circuits i and i - 1 get the same advice pointers (all of them the same in "all")
KERNEL_CASES = [
    (4, 3, 1, 1, False, 0, 1, 0, None),
    (4, 3, 8, 1, True, 2, 1, 0, None),
    (5, 9, 2, 8, True, 9, 7, 2, "all"),
    (5, 5, 3, 8, False, 3, 2, 2, "pairs"),
    (6, 6, 3, 8, True, 5, 4, 0, None),
    (6, 9, 8, 1, True, 0, 1, 2, "pairs"),
    (6, 7, 1, 8, False, 6, 5, 2, None),
    (5, 4, 2, 1, False, 4, 2, 0, "all"),
]


def kernel_case(custom, case: int):
    """-> dict: k, degree, trees (custom.Expression), challenges, and the columns in Python integers: `shared` and `circuits` as
    batched_quotient takes them, plus beta, gamma, y"""
    k, degree, n_circuits, depth, with_ch, n_perm, chunk, n_lookups, share = KERNEL_CASES[case]
    rng = random.Random(8800 + case)
    ext_k = k + (degree - 2).bit_length()
    size = 1 << ext_k
    rots = list(range(-3, 4))
    columns = [("advice", j, rots) for j in range(N_ADV)] + [("fixed", j, rots) for j in range(N_FIX)] + [("instance", 0, rots)]
    Q = lambda: custom.Expression("query", *((lambda c: (c[0], c[1], rng.choice(c[2])))(rng.choice(columns))))
    CH = lambda: custom.Expression("challenge", rng.randrange(N_CH))
    leaf = lambda: CH() if with_ch and rng.random() < 0.4 else Q()
    if depth == 1:  # single operands and negations only: no LDS level
        trees = [Q(), -leaf(), custom.Expression.constant(R - 1)]
        if with_ch:
            trees.append(custom.Expression("challenge", 0))
    else:  # x0 - (x1 - (.. - x7)): SUB keeps its operand order, eight leaves need a stack of eight; a product and a sum beside it
        leaves = [leaf() for _ in range(8)]
        chain = leaves[-1]
        for e in reversed(leaves[:-1]):
            chain = e - chain
        trees = [chain, Q() * leaf() * Q() - custom.Expression.constant(rng.randrange(R)), Q() + leaf()]
    assert max(t.stack_depth() for t in trees) == depth
    special = [0, 1, R - 1]
    column = lambda: [rng.choice(special) if rng.random() < 0.2 else rng.randrange(R) for _ in range(size)]
    fixed = [column() for _ in range(N_FIX)]
    shared = {"perm_sigmas": [column() for _ in range(n_perm)], "chunk": chunk, "l0": column(), "l_last": column(), "l_active": column()}
    sets = -(-n_perm // chunk) if n_perm else 0
    assert n_perm == 0 or sets == 2
    circuits = []
    for i in range(n_circuits):
        reuse = i > 0 and (share == "all" or (share == "pairs" and i % 2 == 1))
        c = {"advice": circuits[i - 1]["advice"] if reuse else [column() for _ in range(N_ADV)], "fixed": fixed,
             "instance": circuits[i - 1]["instance"] if reuse else column()}
        # the permuted columns: an advice column of this circuit, a fixed one, then columns of their own
        own = [c["advice"][0], fixed[0]]
        c["perm_values"] = (own + [column() for _ in range(n_perm)])[:n_perm]
        c["perm_zs"] = [column() for _ in range(sets)]
        c["lookups"] = [(c["advice"][l % N_ADV], fixed[1] if l == 1 else None, fixed[0], column(), column(), column()) for l in range(n_lookups)]
        if share == "all" and i > 0:  # the very same circuit again: every pointer shared, the fold doubled
            c = circuits[0]
        circuits.append(c)
    return {"k": k, "degree": degree, "extended_k": ext_k, "trees": trees, "challenges": [rng.choice(special + [rng.randrange(R)]) for _ in range(N_CH)] if with_ch else [],
            "shared": shared, "circuits": circuits, "beta": rng.randrange(R), "gamma": rng.randrange(R), "y": rng.randrange(R), "bf": 5}
