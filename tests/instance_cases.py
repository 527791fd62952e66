"""Circuits with SEVERAL instance columns (h2mi_prover_instances, H2MI_MAX_INSTANCE = 8), shared by tests/test_instances_host.py and
tests/test_gpu_instances.py: the circuits, the bridge to oracle.flex (which proves and verifies any number of instance columns and is the
byte-for-byte reference here), the Python-integer references of the kernels, and the proof verifier over lists of columns.

Circuits:
  two_cols      k = 5: instance columns 0 and 1, both equality-enabled; the gate s (a - i0 - i1(wX)) reads column 1 one row down; one
                advice cell is copied to column 0 row 0 and another to column 1 row 2.
  eight_cols    k = 5: eight instance columns holding 0, 1, 2, 3, 15, 16, 17 and usable-rows values — the empty column, both sides of the
                16-value switch between the l_0 route and the transforms, the longest column there can be; one degree-3 gate reads all
                eight at rotations -1, 0, +1; copies into columns 0 (a zero beyond nothing), 5 and 7 (its last usable row).
  in_arguments  k = 6: column 0 inside the input expression of a lookup_any, column 1 inside a shuffle's input, column 2 read by a gate
                over a second-phase advice column together with a challenge; the same key with logup = True.

The verifier: `verify` is tests/gwc_cases.py's `verify` from its signature down to and including the query list, copied line for line
— that text already reads `instances[i][c]` and `cs.instance_queries`, i.e. any number of instance columns — with BOTH tails behind
it: ProverSHPLONK's (tests/logup_sets_cases.py's last lines) and ProverGWC's (gwc_cases.gwc_check).  What is new here is only
`verify_circuits`, which hands every circuit's LIST OF COLUMNS through where the other files wrap one column.

`coset_circuit` / `check_quotient` (GPU tests): a proof's vectors recomputed in Python integers from the prover's row buffers and
H2MI_BUF_H against `batched_quotient` on every extended-coset point — gates, the permutation argument, lookups (permuted or logUp,
merged sets), shuffles, challenges, any number of instance columns and circuits; shared by tests/test_gpu_instances.py and
tests/test_gpu_random_circuits.py."""
import random

import shuffle_cases
from batch_cases import KINDS, MAX_CIRCUITS, keys_delta, lookup_terms, permutation_terms
from gwc_cases import gwc_check, gwc_groups
from logup_sets_cases import expr_lookup_sets, logup_terms
from lookup_expr_cases import compress
from oracle import bn254 as o
from oracle import flex as FX
from oracle.flex import ADVICE, FIXED, INSTANCE, ProofReader, construct_intermediate_sets
from oracle.prover import evaluate_vanishing_polynomial, lagrange_interpolate, rotate_omega
from phase_cases import run_postfix
from shuffle_cases import shuffle_terms

R = o.R
MAX_INSTANCE = 8  # H2MI_MAX_INSTANCE (include/h2mi.h)
ALL_ONES = ((1 << 256) - 1) % R  # every limb all ones, reduced
EXTREMES = [0, 1, R - 1, ALL_ONES]


# ---- the circuits --------------------------------------------------------------------------------------------------------------------
def two_cols_circuit(custom, variant: int = 0, bad: str = None):
    """-> (cs, assignment).  variant: the public inputs (the circuits of a batch differ in it); bad = "copy1": the advice cell copied
    into instance column 1 is off by one"""
    meta = custom.ConstraintSystem()
    a = meta.advice_column()
    i0, i1 = meta.instance_column(), meta.instance_column()
    s = meta.selector()
    for column in (a, i0, i1):
        meta.enable_equality(column)
    meta.create_gate("a = i0 + i1 one row down", lambda meta: [meta.query_selector(s) * (
        meta.query_advice(a, custom.Rotation.cur()) - meta.query_instance(i0, custom.Rotation.cur()) - meta.query_instance(i1, custom.Rotation.next()))])
    rng = random.Random(8100 + variant)
    col0 = [rng.choice(EXTREMES + [rng.randrange(R)]) for _ in range(3)]
    col1 = [rng.randrange(R) for _ in range(4)] + [R - 1]
    region = custom.Assignment(meta, instance=[col0, col1])
    at = lambda col, r: col[r] if r < len(col) else 0
    for row in range(4):
        region.assign_advice(a, row, (at(col0, row) + at(col1, row + 1)) % R)
        region.enable_selector(s, row)
    region.constrain_instance(region.assign_advice(a, 6, col0[0]), i0, 0)
    region.constrain_instance(region.assign_advice(a, 7, (col1[2] + (1 if bad == "copy1" else 0)) % R), i1, 2)
    return meta, region


def eight_cols_counts(usable_rows: int):
    return [0, 1, 2, 3, 15, 16, 17, usable_rows]


# the gate of eight_cols: s (a - sum_c i_c(rotation_c) - i5 i6(wX) - i7(wX)); every column at least once, every rotation of -1, 0, +1
EIGHT_ROTATIONS = [-1, 0, 1, -1, 0, 0, 1, -1]


def eight_cols_circuit(custom, k: int = 5, variant: int = 0, bad: str = None):
    """-> (cs, assignment).  bad: "copy5" breaks the copy into instance column 5 by one, "gate5" changes a value of column 5 that only
    the gate reads (the witness was made for the unchanged value)."""
    meta = custom.ConstraintSystem()
    a, b = meta.advice_column(), meta.advice_column()
    inst = [meta.instance_column() for _ in range(MAX_INSTANCE)]
    s = meta.selector()
    for column in (b, inst[0], inst[5], inst[7]):
        meta.enable_equality(column)

    def gate(meta):
        q = [meta.query_instance(inst[c], custom.Rotation(EIGHT_ROTATIONS[c])) for c in range(MAX_INSTANCE)]
        linear = q[0] + q[1] + q[2] + q[3] + q[4] + q[7]
        return [meta.query_selector(s) * (meta.query_advice(a, custom.Rotation.cur()) - linear - q[5] * q[6]
                                          - meta.query_instance(inst[7], custom.Rotation.next()))]

    meta.create_gate("all eight", gate)
    n = 1 << k
    u = n - (meta.blinding_factors() + 1)
    rng = random.Random(8200 + variant)
    cols = [[rng.choice(EXTREMES) if rng.random() < 0.3 else rng.randrange(R) for _ in range(count)] for count in eight_cols_counts(u)]
    witness = [list(c) for c in cols]
    if bad == "gate5":
        cols[5][9] = (cols[5][9] + 1) % R
    region = custom.Assignment(meta, instance=cols)
    at = lambda c, r: witness[c][r % n] if r % n < len(witness[c]) else 0
    for row in range(u):
        v = sum(at(c, row + EIGHT_ROTATIONS[c]) for c in (0, 1, 2, 3, 4, 7)) + at(5, row) * at(6, row + 1) + at(7, row + 1)
        region.assign_advice(a, row, v % R)
        region.enable_selector(s, row)
    region.constrain_instance(region.assign_advice(b, 0, 0), inst[0], 3)  # the empty column: a zero, wherever
    region.constrain_instance(region.assign_advice(b, 1, (cols[5][4] + (1 if bad == "copy5" else 0)) % R), inst[5], 4)
    region.constrain_instance(region.assign_advice(b, 2, cols[7][u - 1]), inst[7], u - 1)
    return meta, region


IN_ARGUMENTS_ROWS = 10


def in_arguments_circuit(custom, seed: int = 0):
    """-> (cs, synthesize(challenges)): the witness of the second phase reads the challenge"""
    meta = custom.ConstraintSystem()
    a, t, sa, sb = (meta.advice_column() for _ in range(4))
    i0, i1, i2 = (meta.instance_column() for _ in range(3))
    ch = meta.challenge_usable_after(0)
    w = meta.advice_column_in(1)
    q, ql = meta.selector(), meta.selector()
    for column in (w, a, i0):
        meta.enable_equality(column)
    cur = custom.Rotation.cur()
    meta.create_gate("w = a + c i2", lambda meta: [meta.query_selector(q) * (meta.query_advice(w, cur) - meta.query_advice(a, cur)
                                                                            - meta.query_challenge(ch) * meta.query_instance(i2, cur))])
    meta.lookup_any("a + i0 in t", lambda meta: [(meta.query_selector(ql) * (meta.query_advice(a, cur) + meta.query_instance(i0, cur)),
                                                  meta.query_advice(t, cur))])
    meta.shuffle("sa + i1 is sb permuted", lambda meta: [(meta.query_advice(sa, cur) + meta.query_instance(i1, cur), meta.query_advice(sb, cur))])
    rng = random.Random(8300 + seed)
    rows = IN_ARGUMENTS_ROWS
    col0 = [rng.randrange(R) for _ in range(6)]
    col1 = [rng.choice([1, R - 1, rng.randrange(R)]) for _ in range(5)]
    col2 = [rng.randrange(R) for _ in range(4)]
    a_vals = [rng.choice([0, 3, rng.randrange(R)]) for _ in range(rows)]
    sa_vals = [rng.choice([2, 2, rng.randrange(R)]) for _ in range(rows)]
    at = lambda col, r: col[r] if r < len(col) else 0
    table = [(a_vals[r] + at(col0, r)) % R for r in range(rows)]
    rng.shuffle(table)
    perm = [(sa_vals[r] + at(col1, r)) % R for r in range(rows)]
    rng.shuffle(perm)

    def synthesize(challenges):
        region = custom.Assignment(meta, instance=[col0, col1, col2], challenges=challenges)
        cv = region.get_challenge(ch)
        cell = None
        for row in range(rows):
            region.assign_advice(a, row, a_vals[row])
            region.assign_advice(t, row + 20, table[row])  # the table on other rows than its inputs; every other row holds zero
            region.assign_advice(sa, row, sa_vals[row])
            region.assign_advice(sb, row + 3, perm[row])
            region.enable_selector(q, row)
            region.enable_selector(ql, row)
            cell = region.assign_advice(w, row, (a_vals[row] + cv * at(col2, row)) % R if cv is not None else 0)
        region.copy_advice(cell, w, rows + 2)
        region.constrain_instance(region.assign_advice(a, rows + 4, col0[1]), i0, 1)
        return region

    return meta, synthesize


CASES = {"two_cols": 5, "eight_cols": 5, "in_arguments": 6}  # name -> k


def build(custom, name: str):
    """-> (cs, assignment or synthesize(challenges), k)"""
    k = CASES[name]
    if name == "two_cols":
        return (*two_cols_circuit(custom), k)
    if name == "eight_cols":
        return (*eight_cols_circuit(custom, k), k)
    return (*in_arguments_circuit(custom), k)


first_assignment = shuffle_cases.first_assignment


def columns_of(cs, asg):
    """an assignment's public inputs as one list per instance column, whichever form custom.Assignment keeps them in"""
    if cs.n_instance > 1:
        return [list(c) for c in asg.instance]
    return [list(asg.instance)] if cs.n_instance else []


def tampered(columns, c: int):
    """the columns with one value of column c changed (an empty column: a value where there was none)"""
    out = [list(col) for col in columns]
    if out[c]:
        out[c][len(out[c]) // 2] = (out[c][len(out[c]) // 2] + 1) % R
    else:
        out[c] = [1]
    return out


# ---- the oracle's view ----------------------------------------------------------------------------------------------------------------
def oracle_cs(cs, name="instances"):
    """a custom.ConstraintSystem as oracle.flex.ConstraintSystem (custom_gate_cases.oracle_cs: nothing there depends on n_instance)"""
    return FX.ConstraintSystem(name, cs.n_advice, cs.n_fixed, cs.n_instance, cs.gates, list(cs.perm_columns), [], list(cs.advice_queries),
                               list(cs.fixed_queries), list(cs.instance_queries), cs.degree(), cs.blinding_factors())


def oracle_assignment(ocs, cs, asg):
    """custom_gate_cases.oracle_assignment with oasg.instance the list of columns"""
    oasg = FX.Assignment(ocs)
    oasg.advice = [dict(c) for c in asg.advice]
    oasg.fixed = [dict(c) for c in asg.fixed]
    oasg.instance = columns_of(cs, asg)
    oasg.copies = list(asg.copies)
    return oasg


# ---- the kernels in Python integers ------------------------------------------------------------------------------------------------------
def instance_coset(dom, values):
    """the extended-coset form of sum_r v_r L_r(X) through the oracle's transforms: what both routes of the prover must produce"""
    n = 1 << dom.k
    assert len(values) <= n
    return dom.coeff_to_extended(dom.lagrange_to_coeff(list(values) + [0] * (n - len(values))))


def extreme_columns(counts, seed: int):
    """one column of public inputs per count, made of the extreme values and uniform ones, every extreme in every non-empty column"""
    rng = random.Random(seed)
    cols = []
    for count in counts:
        col = [EXTREMES[i % len(EXTREMES)] if i < len(EXTREMES) or rng.random() < 0.25 else rng.randrange(R) for i in range(count)]
        rng.shuffle(col)
        cols.append(col)
    return cols


def batched_quotient(k, extended_k, zeta, extended_omega, delta, blinding_factors, ops, constants, challenges, circuits, shared, beta, gamma, y,
                     logup: bool = False):
    """shuffle_cases.batched_quotient with a circuit's "instance" a LIST of columns on the extended coset (an INSTANCE op's index picks one).
    logup: a circuit's "lookups" entries are logup_sets_cases.batched_quotient's (LIST of compressed inputs, None, compressed table, M,
    None, phi) and their terms logup_terms"""
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
            cols = {"advice": c["advice"], "fixed": c["fixed"], "instance": c["instance"]}
            for poly in run_postfix(ops, constants, lambda op, col, r: cols[KINDS[op]][col][at(r)], challenges):
                v = (v * y + poly) % R
            zs = c["perm_zs"]
            v = permutation_terms(v, y, beta, gamma, delta, chunk, [p[idx] for p in c["perm_values"]], [s[idx] for s in sig], [z[idx] for z in zs],
                                  [z[nxt] for z in zs], [z[lst] for z in zs], l0, ll, la, x)
            for a_in, b_in, table, pin, ptab, lz in c.get("lookups", ()):
                if logup:
                    v = logup_terms(v, y, beta, [a[idx] for a in a_in], table[idx], pin[idx], lz[idx], lz[nxt], l0, ll, la)
                    continue
                a_val = a_in[idx] * b_in[idx] % R if b_in is not None else a_in[idx]
                v = lookup_terms(v, y, beta, gamma, a_val, table[idx], pin[idx], pin[prv], ptab[idx], lz[idx], lz[nxt], l0, ll, la)
            for a_in, s_in, sz in c.get("shuffles", ()):
                v = shuffle_terms(v, y, gamma, a_in[idx], s_in[idx], sz[idx], sz[nxt], l0, ll, la)
        out.append(v * t_inv[idx % rot] % R)
        x = x * extended_omega % R
    return out


# ---- a proof's vectors in Python integers (GPU tests: the buffers are the device's) -----------------------------------------------------
def device_values(buf, count):
    return o.unpack(buf.to_numpy(shape=(count, 4), nbytes=count * 32), R)


def _compress_coset(exprs, cols, size, rot, theta, challenges):
    """custom.Expression list -> the theta-compressed column on the extended coset, point by point: a rotation r reads idx + r rot"""
    out = []
    for idx in range(size):
        q = lambda kind, c, r: cols[kind][c][(idx + r * rot) % size]
        out.append(compress([e.evaluate(q, challenges) for e in exprs], theta))
    return out


def coset_circuit(cs, keys, prover, k, theta=0, challenges=(), logup: bool = False):
    """every vector the quotient reads for one circuit, recomputed in Python integers on the extended coset from the ROW buffers of the
    prover (advice, instance columns, products; per lookup argument the permuted columns and the product, or M and phi of a logUp key;
    shuffle products) and of the key; nothing is read from a device coset buffer.  -> (circuit, shared, oracle domain, the instance
    columns' rows) as batched_quotient takes them"""
    from halo2_scaffold_amd import engine

    n = 1 << k
    dom = o.Domain(k, cs.degree())
    size, rot = 1 << dom.extended_k, 1 << (dom.extended_k - k)
    ext = lambda rows: dom.coeff_to_extended(dom.lagrange_to_coeff(rows))
    rows_of = lambda views: [device_values(v, n) for v in views]
    advice = [ext(r) for r in rows_of(prover.views(engine.BUF_ADVICE, cs.n_advice))]
    fixed = [ext(r) for r in rows_of(keys.fixed_values)]
    sigma = [ext(r) for r in rows_of(keys.sigma_values)]
    instance_rows = rows_of(prover.views(engine.BUF_INSTANCE, cs.n_instance))
    instance = [ext(r) for r in instance_rows]
    m, chunk = len(cs.perm_columns), cs.degree() - 2
    n_sets = -(-m // chunk)
    perm_zs = [ext(r) for r in rows_of(prover.views(engine.BUF_PERM_Z, n_sets))]
    by_kind = {"advice": advice, "fixed": fixed, "instance": instance}
    perm_values = [by_kind[kind][c] for kind, c in cs.perm_columns]
    circuit = {"advice": advice, "fixed": fixed, "instance": instance, "perm_values": perm_values, "perm_zs": perm_zs}
    L, S = len(cs.lookup_arguments), len(cs.shuffles)
    declared = cs.lookups
    view = lambda kind, count, i: ext(device_values(prover.views(kind, count)[i], n))
    lookups = []
    for l, arg in enumerate(cs.lookup_arguments):
        a_ins = [_compress_coset([a for a, _ in declared[j]], by_kind, size, rot, theta, challenges) for j in arg]
        t_in = _compress_coset([t for _, t in declared[arg[0]]], by_kind, size, rot, theta, challenges)
        if logup:
            lookups.append((a_ins, None, t_in, view(engine.BUF_LOGUP_M, L, l), None, view(engine.BUF_LOGUP_PHI, L, l)))
        else:
            assert len(a_ins) == 1
            lookups.append((a_ins[0], None, t_in, view(engine.BUF_LOOKUP_PERMUTED_INPUT, L, l), view(engine.BUF_LOOKUP_PERMUTED_TABLE, L, l),
                            view(engine.BUF_LOOKUP_Z, L, l)))
    shuffles = []
    for i, pairs in enumerate(cs.shuffles):
        a_in = _compress_coset([a for a, _ in pairs], by_kind, size, rot, theta, challenges)
        s_in = _compress_coset([s for _, s in pairs], by_kind, size, rot, theta, challenges)
        shuffles.append((a_in, s_in, view(engine.BUF_SHUFFLE_Z, S, i)))
    if lookups:
        circuit["lookups"] = lookups
    if shuffles:
        circuit["shuffles"] = shuffles
    u = n - (cs.blinding_factors() + 1)
    unit = lambda row: [1 if i == row else 0 for i in range(n)]
    shared = {"perm_sigmas": sigma, "chunk": chunk, "l0": ext(unit(0)), "l_last": ext(unit(u)), "l_active": ext([1] * u + [0] * (n - u))}
    return circuit, shared, dom, instance_rows


def check_quotient(cs, keys, provers, asgs, k, trace, logup: bool = False):
    """H2MI_BUF_H of a proof just made (the quotient kernel's values through the inverse transform, a bijection) against
    batched_quotient on every extended-coset point; the instance buffers against the assignments' public inputs.  provers / asgs: one
    per circuit of the proof; trace: create_proof's or prove_many's.  -> (the circuits' vectors, the arguments of batched_quotient
    before `circuits`, the expected vector), for further questions about the same proof"""
    from halo2_scaffold_amd import engine

    ops, consts = cs.program()
    challenges = list(trace.get("challenges") or [])
    built = [coset_circuit(cs, keys, p, k, trace["theta"], challenges, logup) for p in provers]
    n = 1 << k
    for (_, _, _, rows), asg in zip(built, asgs):  # H2MI_BUF_INSTANCE, index < n_instance: that column's values, zero below them
        assert rows == [list(col) + [0] * (n - len(col)) for col in columns_of(cs, asg)]
    shared, dom = built[0][1], built[0][2]
    args = (k, dom.extended_k, dom.g_coset, dom.extended_omega, keys_delta(), cs.blinding_factors(), ops, consts, challenges)
    tail = (shared, trace["beta"], trace["gamma"], trace["y"], logup)
    want = batched_quotient(*args, [b[0] for b in built], *tail)
    size = 1 << dom.extended_k
    got = dom.coeff_to_extended(device_values(provers[0].view(engine.BUF_H), size))
    assert len(want) == size and got == want
    return built, args, tail, want


# ---- the verifier ---------------------------------------------------------------------------------------------------------------------
def verify(keys, proof: bytes, instances, gates, lookups, shuffles=(), advice_phase=None, challenge_phase=(), challenges_out=None,
           logup: bool = False, multiopen: str = "shplonk") -> bool:
    """gwc_cases.verify line for line up to and including its query list (gates, lookups permuted and logUp, shuffles, advice phases, N
    circuits; instances[i][c]: the values of instance column c of circuit i), then the tail of the multi-opening the proof ends with:
    logup_sets_cases.verify's for "shplonk", gwc_cases.verify's for "gwc"."""
    assert multiopen in ("shplonk", "gwc")
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
        if len(instances[i]) != cs.n_instance:
            return False
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
    if multiopen == "gwc":  # gwc_cases.verify's tail
        vv = rd.squeeze()
        try:
            Ws = [rd.read_point() for _ in gwc_groups(queries)]
        except ValueError:
            return False
        uu = rd.squeeze()
        if rd.pos != len(proof):
            return False
        return gwc_check(points, queries, vv, Ws, uu, keys)
    # logup_sets_cases.verify's tail: ProverSHPLONK
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


def verify_circuits(vk, cs, proof: bytes, instances, logup: bool = False, multiopen: str = "shplonk", challenges_out=None) -> bool:
    """`verify` for N circuits of one custom.ConstraintSystem; instances[i]: circuit i's public inputs as a LIST OF COLUMNS, one list per
    instance column of the constraint system (columns_of gives it for an assignment)"""
    from phase_cases import expr_gates

    return verify(vk, proof, [[list(col) for col in circuit] for circuit in instances], expr_gates(cs), expr_lookup_sets(cs),
                  shuffle_cases.expr_shuffles(cs), cs.advice_phase, cs.challenge_phase, challenges_out=challenges_out, logup=logup, multiopen=multiopen)
