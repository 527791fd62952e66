"""ProverGWC's multi-opening (poly/kzg/multiopen/gwc), shared by tests/test_gwc_host.py and tests/test_gpu_gwc.py — RESTATED FROM MEMORY of
halo2_proofs v2023_02_02 like the shuffle and logUp arguments, and pinned to DESIGN.md 4.5 and to this file, not to the crate.

Prover, after the evaluations are written: squeeze v; group the queries by point in order of first appearance (queries inside a group keep
the list's order, nothing is deduplicated); per group i with point z_i and queries (p_ij, e_ij): W_i(X) = (sum_j v^j p_ij(X) - sum_j v^j
e_ij) / (X - z_i), committed without blinding and written in group order, nothing squeezed between the points.
Verifier: squeeze v, read the P points, squeeze u, accept iff
    e(sum_i u^i [W_i], [s]_2) = e(sum_i u^i (z_i [W_i] + sum_j v^j C_ij - (sum_j v^j e_ij) G), [1]_2).

Shared with tests/logup_sets_cases.py: `verify` below IS that file's `verify` from its signature down to and including the query list
(`qq(("random",), random_c, x, random_eval)`), copied line for line — everything create_proof writes before the opening argument; only the
tail behind the query list is GWC's.  `verify_circuits` is that file's, over this `verify`."""
import logup_sets_cases
import shuffle_cases
from batch_cases import MAX_CIRCUITS, keys_delta, lookup_terms, permutation_terms
from logup_sets_cases import expr_lookup_sets, logup_terms
from lookup_expr_cases import compress
from oracle import bn254 as o
from oracle.flex import ADVICE, FIXED, INSTANCE, ProofReader
from oracle.prover import rotate_omega
from shuffle_cases import shuffle_terms

R = o.R


# ---- the argument in Python integers -------------------------------------------------------------------------------------------------
def gwc_groups(queries):
    """queries: [(key, point, evaluation)] in create_proof's order -> [(point, [(key, evaluation), ..])] by first appearance of the point"""
    groups, index = [], {}
    for key, pt, ev in queries:
        if pt not in index:
            index[pt] = len(groups)
            groups.append((pt, []))
        groups[index[pt]][1].append((key, ev))
    return groups


def gwc_witnesses(polys, queries, v: int):
    """the prover's tail: polys[key] = coefficients (low to high, all of one length n) -> [W_i], n - 1 coefficients each"""
    out = []
    for z, members in gwc_groups(queries):
        n = len(polys[members[0][0]])
        acc, vp = [0] * n, 1
        for key, ev in members:
            poly = polys[key]
            for t in range(n):
                acc[t] = (acc[t] + vp * poly[t]) % R
            acc[0] = (acc[0] - vp * ev) % R
            vp = vp * v % R
        out.append(o.kate_division(acc, z))
    return out


def gwc_check(points, queries, v: int, Ws, u: int, keys) -> bool:
    """the verifier's tail with the known test secret keys.s in place of the pairing, as the existing verifiers' last line:
    s sum_i u^i W_i == sum_i u^i (z_i W_i + C_i - e_i G), C_i = sum_j v^j points[key_ij], e_i = sum_j v^j e_ij"""
    groups = gwc_groups(queries)
    if len(Ws) != len(groups):
        return False
    left, right, up = None, None, 1
    for (z, members), W in zip(groups, Ws):
        c, e, vp = None, 0, 1
        for key, ev in members:
            c = o.g1_add(c, o.g1_mul(vp, points[key]))
            e = (e + vp * ev) % R
            vp = vp * v % R
        term = o.g1_add(o.g1_add(o.g1_mul(z, W), c), o.g1_mul((-e) % R, o.G1_GEN))
        left = o.g1_add(left, o.g1_mul(up, W))
        right = o.g1_add(right, o.g1_mul(up, term))
        up = up * u % R
    return o.g1_mul(keys.s, left) == right


# ---- the verifier ---------------------------------------------------------------------------------------------------------------------
def verify(keys, proof: bytes, instances, gates, lookups, shuffles=(), advice_phase=None, challenge_phase=(), challenges_out=None,
           logup: bool = False, tail_out=None) -> bool:
    """logup_sets_cases.verify line for line up to and including its query list (gates, lookups permuted and logUp, shuffles, advice
    phases, N circuits — the lines between `def verify` and `qq(("random",), ..)` there); then ProverGWC's tail instead of SHPLONK's:
    squeeze v, read one [W] per opening point, squeeze u, gwc_check.  tail_out: see verify_circuits."""
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
    vv = rd.squeeze()
    try:
        Ws = [rd.read_point() for _ in gwc_groups(queries)]
    except ValueError:
        return False
    uu = rd.squeeze()
    if rd.pos != len(proof):
        return False
    if tail_out is not None:  # what the tests compare the prover's own vectors with
        tail_out.update(queries=queries, points=points, v=vv, u=uu, Ws=Ws)
    return gwc_check(points, queries, vv, Ws, uu, keys)


def verify_circuits(vk, cs, proof: bytes, instances, logup: bool, challenges_out=None, tail_out=None) -> bool:
    """logup_sets_cases.verify_circuits over the GWC `verify`; tail_out (a dict) receives the verifier's query list [(key, point,
    evaluation)], the commitments by key, v, u and the [W_i] it read"""
    from phase_cases import expr_gates

    per_circuit = [[list(v)] if cs.n_instance else [] for v in instances]
    return verify(vk, proof, per_circuit, expr_gates(cs), expr_lookup_sets(cs), shuffle_cases.expr_shuffles(cs), cs.advice_phase, cs.challenge_phase,
                  challenges_out=challenges_out, logup=logup, tail_out=tail_out)

