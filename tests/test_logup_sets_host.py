"""CPU tests of logUp lookups with several input sets over one table (tests/logup_sets_cases.py): the generalised functions equal those
of tests/logup_cases.py on one input set; the generalised verifier accepts and rejects exactly as logup_cases.verify does on
tests/golden/logup_proofs.json; for every merged circuit the restatement's sum ends at zero and the three terms vanish on every row;
h2mi_logup_inputs_check (the polynomial count, the degree rule, the counts, the challenges) and the keygen refusals that need no
device; ConstraintSystem.merge_lookups (grouping by table, declaration order, chunk sizes at budgets 5 and 9)."""
import json
import os
import random

import numpy as np
import pytest

import custom_gate_cases as gate_cases
import keygen_call
import logup_cases
import logup_sets_cases as cases
from lookup_expr_cases import compress
from oracle import flex as FX

R = cases.R
EINVAL = -1
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- one input set: the numbers of tests/logup_cases.py ---------------------------------------------------------------------------------
def test_one_set_is_the_existing_restatement():
    rng = random.Random(77)
    u, n = 40, 64
    table = [rng.randrange(R) for _ in range(12)] * 4
    a = [rng.choice(table[:u]) for _ in range(n)]
    a[17] = R - 1  # absent
    m, missing = cases.multiplicities([a], table, u)
    m1, missing1 = logup_cases.multiplicities(a, table, u)
    assert m == m1 and missing == [(i, 0) for i in missing1] == [(17, 0)]
    beta = rng.randrange(R)
    assert cases.running_sum([a], table, m, beta, u) == logup_cases.running_sum(a, table, m, beta, u)
    for _ in range(8):
        vals = [rng.randrange(R) for _ in range(10)]
        v, y, av, sv, mv, phi, phin, l0, ll, la = vals
        assert cases.logup_terms(v, y, beta, [av], sv, mv, phi, phin, l0, ll, la) == logup_cases.logup_terms(v, y, beta, av, sv, mv, phi, phin, l0, ll, la)
        num, den = cases.fraction([av], sv, mv, beta)
        assert num == ((sv + beta) - mv * (av + beta)) % R and den == (av + beta) * (sv + beta) % R


def test_the_fraction_is_the_recurrence_and_the_sum_of_fractions():
    """(N, D) = (-M, s), then N <- N a_j + D, D <- D a_j gives the written-out pair, and N / D is sum_j 1 / a_j - M / s"""
    rng = random.Random(5)
    for K in range(1, cases.MAX_LOGUP_INPUTS + 1):
        a_vals, s_val, m, beta = [rng.randrange(R) for _ in range(K)], rng.randrange(R), rng.randrange(50), rng.randrange(R)
        num, den = (-m) % R, (s_val + beta) % R
        for v in a_vals:
            num = (num * (v + beta) + den) % R
            den = den * (v + beta) % R
        assert (num, den) == cases.fraction(a_vals, s_val, m, beta)
        want = (sum(pow((v + beta) % R, -1, R) for v in a_vals) - m * pow((s_val + beta) % R, -1, R)) % R
        assert num * pow(den, -1, R) % R == want


def test_multiplicities_over_several_sets():
    s = [7, 3, 7, 9, 3, 0, 0, 5]
    sets = [[3, 3, 7, 0, 0, 0, 7, 3], [9, 9, 9, 9, 9, 9, 9, 9], [5, 0, 5, 0, 5, 0, 5, 4]]
    m, missing = cases.multiplicities(sets, s, 8)
    assert m == [2, 3, 0, 8, 0, 6, 0, 4] and missing == [(7, 2)] and sum(m) == 3 * 8 - 1
    single = [logup_cases.multiplicities(a, s, 8)[0] for a in sets]
    assert m == [sum(col) for col in zip(*single)]


# ---- the verifier on the committed logUp goldens ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(2))
def test_verifier_agrees_with_logup_cases_on_the_goldens(h2, index):
    from halo2_scaffold_amd import custom

    g = json.load(open(os.path.join(GOLD, "logup_proofs.json")))
    entry = g["cases"][index]
    cs, asg, k = logup_cases.build(custom, entry["circuit"])
    first = logup_cases.first_assignment(cs, asg)
    ocs = gate_cases.oracle_cs(cs, entry["circuit"])
    oasg = gate_cases.oracle_assignment(ocs, first)
    vk = FX.VerifierKeys(ocs, k, int(g["srs_secret"], 16), oasg.fixed, oasg.copies)
    proof = bytes.fromhex(entry["proof"])
    instances = [list(first.instance)]
    assert cases.verify_circuits(vk, cs, proof, instances, logup=True) and logup_cases.verify_circuits(vk, cs, proof, instances, logup=True)
    assert not cases.verify_circuits(vk, cs, proof, instances, logup=False) and not logup_cases.verify_circuits(vk, cs, proof, instances, logup=False)
    m_at, phi_at, ev_at = logup_cases.proof_offsets(cs)
    assert cases.proof_offsets(cs) == (m_at, phi_at, ev_at)
    for at in (3, m_at + 5, phi_at + 3, ev_at + 1, ev_at + 33, ev_at + 66, len(proof) - 1):
        flipped = bytearray(proof)
        flipped[at] ^= 1
        assert not cases.verify_circuits(vk, cs, bytes(flipped), instances, logup=True), at
        assert not logup_cases.verify_circuits(vk, cs, bytes(flipped), instances, logup=True), at
    assert not cases.verify_circuits(vk, cs, proof[:-1], instances, logup=True)


# ---- the restatement on the merged circuits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_running_sum_ends_at_zero_and_the_terms_vanish_on_every_row(h2, name):
    from halo2_scaffold_amd import custom

    rng = random.Random(sum(map(ord, name)))
    cs, asg, k = cases.build(custom, name)
    n = 1 << k
    u = n - (cs.blinding_factors() + 1)
    challenges = [rng.randrange(R) for _ in cs.challenge_phase]
    region = asg(challenges) if callable(asg) else asg
    custom.mock(region, k, challenges)
    for column in region.advice:  # what the prover puts there
        for row in range(u, n):
            column[row] = rng.randrange(R)
    theta, beta = rng.randrange(R), rng.randrange(R)
    arguments = cases.argument_rows(cs, region, k, challenges)
    assert len(arguments) == len(cs.lookup_arguments) and max(len(a[0]) for a in arguments) >= 2
    for in_sets, tabs in arguments:
        a_sets, s_rows = [[compress(t, theta) for t in ins] for ins in in_sets], [compress(t, theta) for t in tabs]
        m, missing = cases.multiplicities(a_sets, s_rows, u)
        assert missing == [] and sum(m) == len(a_sets) * u
        phi = cases.running_sum(a_sets, s_rows, m, beta, u)
        assert phi[0] == 0 and phi[u] == 0 and any(phi[1:u])
        m, phi = m + [rng.randrange(R) for _ in range(n - u)], phi + [rng.randrange(R) for _ in range(n - u - 1)]
        term = lambda mm, r, y: cases.logup_terms(0, y, beta, [a[r] for a in a_sets], s_rows[r], mm[r], phi[r], phi[(r + 1) % n], int(r == 0), int(r == u), int(r < u))
        for row in range(n):
            assert term(m, row, 1) == 0 and term(m, row, 12345) == 0, row
        bad = list(m)
        bad[0] = (bad[0] + 1) % R
        assert any(term(bad, r, 1) for r in range(n))


def test_an_absent_cell_of_one_set_is_reported(h2):
    from halo2_scaffold_amd import custom

    cs, asg = cases.range_circuit(custom, bad=(1, 6))
    u = 32 - (cs.blinding_factors() + 1)
    (in_sets, tabs), = cases.argument_rows(cs, asg, 5)
    m, missing = cases.multiplicities([[t[0] for t in ins] for ins in in_sets], [t[0] for t in tabs], u)
    assert missing == [(6, 1)] and sum(m) == 3 * u - 1
    with pytest.raises(ValueError, match="lookup 'range 1' not satisfied at row 6"):
        custom.mock(asg, 5)


# ---- h2mi_logup_inputs_check ----------------------------------------------------------------------------------------------------------------
def _range_system(custom, columns, input_degree=1, k=5):
    """`columns` lookups of degree-`input_degree` inputs over one fixed table, declared at a cs whose degree is forced to 9 by a gate"""
    meta = custom.ConstraintSystem()
    cols = [meta.advice_column() for _ in range(columns)]
    table = meta.fixed_column()
    cur = custom.Rotation.cur()

    def power(meta, c, d):
        e = meta.query_advice(c, cur)
        for _ in range(d - 1):
            e = e * meta.query_advice(c, cur)
        return e

    meta.create_gate("degree 9", lambda meta: [power(meta, cols[0], 9)])
    for j, c in enumerate(cols):
        meta.lookup("l%d" % j, lambda meta, c=c: [(power(meta, c, input_degree), meta.query_fixed(table, cur))])
    return meta


def test_inputs_check_counts_polynomials_and_degrees(h2):
    from halo2_scaffold_amd import custom, engine

    assert engine.MAX_LOGUP_INPUTS == cases.MAX_LOGUP_INPUTS == 6
    # K = 6 at degree 9 is accepted and needs exactly 9; K = 7 is refused by the count and cannot fit the degree either
    cs = _range_system(custom, 6)
    assert cs.merge_lookups(9) == [[0, 1, 2, 3, 4, 5]] and cs.degree() == 9
    abi, lp, li = cs.abi(5), cs.lookup_program(), cs.logup_inputs()
    assert abi.n_lookups == 1 and list(li.n_inputs)[:2] == [6, 1]
    assert li.check(abi, lp) == 9
    # the polynomial count: the program holds (6 + 1) polynomials — any other count is refused
    for wrong in (5, 7, 1, 0):
        with pytest.raises(Exception):
            engine.LogupInputs.build([wrong]).check(abi, lp)
    with pytest.raises(Exception):  # without the struct the program is one lookup of one pair: seven polynomials are five too many
        lp.check(abi)
    cs7 = _range_system(custom, 7)
    cs7._merged = [[0, 1, 2, 3, 4, 5, 6]]
    abi7 = cs7._abi(5)
    abi7.n_lookups = 1
    with pytest.raises(Exception):
        engine.LogupInputs.build([7]).check(abi7, cs7.lookup_program())
    # degree-2 inputs shrink K: 2 + 2 K + 1 <= 9 allows three sets, the fourth is refused by the degree rule
    cs3 = _range_system(custom, 4, input_degree=2)
    assert cs3.merge_lookups(9) == [[0, 1, 2], [3]]
    assert cs3.logup_inputs().check(cs3.abi(5), cs3.lookup_program()) == 9
    cs3._merged = [[0, 1, 2, 3]]
    assert cs3.degree() == 11
    abi3 = cs3.abi(5)
    abi3.degree = 9
    with pytest.raises(Exception):
        cs3.logup_inputs().check(abi3, cs3.lookup_program())
    # all ones is h2mi_lookup_program_check
    cs1 = _range_system(custom, 3)
    assert engine.LogupInputs.build([1, 1, 1]).check(cs1.abi(5), cs1.lookup_program()) == cs1.lookup_program().check(cs1.abi(5)) == 4


def test_inputs_check_and_challenges(h2):
    """CHALLENGE ops as h2mi_advice_phases_check allows them: an index below phases->n_challenges, refused without phases and beyond"""
    from halo2_scaffold_amd import custom, engine

    cs, _ = cases.phased_pair_circuit(custom)
    abi, lp, li = cs.abi(6), cs.lookup_program(), cs.logup_inputs()
    assert list(li.n_inputs)[:1] == [2] and cs.degree() == 7
    assert li.check(abi, lp, cs.phases()) == 7
    with pytest.raises(Exception):
        li.check(abi, lp)  # no phases: no challenges
    none = engine.AdvicePhases.build(cs.advice_phase, [])  # the key has no challenge: index 0 is beyond it
    with pytest.raises(Exception):
        li.check(abi, lp, none)


def test_a_count_without_the_flag_is_refused(h2):
    """h2mi_prover_keygen with `inputs`: a count above 1 without H2MI_KEYGEN_LOGUP is H2MI_EINVAL, decided in front of any device work; custom.Keys
    refuses merged lookups with logup=False in words"""
    from halo2_scaffold_amd import custom, engine

    cs, asg = cases.range_circuit(custom)
    assert cs.lookup_arguments == [[0, 1, 2]]
    abi, gates, lp, li = cs.abi(5), cs.gate_program(), cs.lookup_program(), cs.logup_inputs()
    cells, keep = engine.pack_cells(list(asg.fixed))
    copies = np.zeros((1, 4), dtype=np.uint32)
    for flags in (0, engine.KEYGEN_VK_ONLY, 4 | engine.KEYGEN_LOGUP):
        assert keygen_call.keygen(abi, gates=gates, lookups=lp, inputs=li, fixed=cells, copies=copies.ctypes.data, flags=flags, pk=0)[0] == EINVAL
    assert keygen_call.keygen(abi, gates=gates, inputs=li, fixed=cells, copies=copies.ctypes.data, pk=0)[0] == EINVAL
    del keep

    class NoParams:
        k = 5

    with pytest.raises(ValueError, match="only a logUp key proves them"):
        custom.Keys(NoParams(), cs, asg, logup=False)


# ---- merge_lookups ---------------------------------------------------------------------------------------------------------------------------
def test_merge_lookups_groups_by_table_in_declaration_order(h2):
    from halo2_scaffold_amd import custom

    meta = custom.ConstraintSystem()
    cols = [meta.advice_column() for _ in range(8)]
    t0, t1 = meta.fixed_column(), meta.fixed_column()
    cur = custom.Rotation.cur()
    order = [t0, t1, t0, t0, t1, t0, t0, t0]  # interleaved declarations over two tables
    for j, (c, t) in enumerate(zip(cols, order)):
        meta.lookup("l%d" % j, lambda meta, c=c, t=t: [(meta.query_advice(c, cur), meta.query_fixed(t, cur))])
    assert meta.degree() == 4 and meta.lookup_arguments == [[j] for j in range(8)] and meta.logup_inputs() is None
    before = meta.lookup_program()
    # default budget: the unmerged degree 4 has the extended domain of degree 5, so pairs merge for free
    assert meta.merge_lookups() == [[0, 2], [1, 4], [3, 5], [6, 7]] and meta.degree() == 5
    assert meta.merge_lookups(5) == [[0, 2], [1, 4], [3, 5], [6, 7]]
    assert meta.merge_lookups(9) == [[0, 2, 3, 5, 6, 7], [1, 4]] and meta.degree() == 9  # different tables never merge
    assert meta.merge_lookups(4) == [[j] for j in range(8)] and meta.degree() == 4
    assert meta.merge_lookups(7) == [[0, 2, 3, 5], [1, 4], [6, 7]] and meta.degree() == 7
    lp, li = meta.lookup_program(), meta.logup_inputs()
    assert lp.n_lookups == 3 and list(li.n_inputs)[:3] == [4, 2, 2] and meta.abi(5).n_lookups == 3
    assert lp.exprs.n_ops == before.exprs.n_ops - 2 * 5  # the same input polynomials, five table polynomials (a query and an END) fewer
    assert meta.argument_names == ["l0 + l2 + l3 + l5", "l1 + l4", "l6 + l7"]
    assert li.check(meta.abi(5), lp) == 7
    # a table that differs in structure only (a rotation) is another table
    other = custom.ConstraintSystem()
    a, b, t = other.advice_column(), other.advice_column(), other.fixed_column()
    other.lookup("cur", lambda meta: [(meta.query_advice(a, cur), meta.query_fixed(t, cur))])
    other.lookup("next", lambda meta: [(meta.query_advice(b, cur), meta.query_fixed(t, custom.Rotation.next()))])
    assert other.merge_lookups(9) == [[0], [1]]
    # a lookup declared after the merge undoes it: nothing is silently left out of the program
    c = other.advice_column()
    other.lookup("late", lambda meta: [(meta.query_advice(c, cur), meta.query_fixed(t, cur))])
    assert other.logup_inputs() is None and other.lookup_arguments == [[0], [1], [2]] and other.lookup_program().n_lookups == 3
    assert other.merge_lookups(9) == [[0, 2], [1]]


def test_merge_lookups_default_budget_keeps_the_extended_domain(h2):
    from halo2_scaffold_amd import custom
    from halo2_scaffold_amd.domain import EvaluationDomain

    for name in sorted(cases.CASES):
        cs, _, k = cases.build(custom, name)
        merged_degree, merged = cs.degree(), cs._merged
        cs._merged = None
        unmerged_degree = cs.degree()
        default = cs.merge_lookups()
        assert EvaluationDomain(cs.degree(), k).extended_k == EvaluationDomain(unmerged_degree, k).extended_k
        cs._merged = merged
        assert cs.degree() == merged_degree >= unmerged_degree and default
