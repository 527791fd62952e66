"""CPU tests of the logUp lookup argument (tests/logup_cases.py): the generalised verifier with logUp off pinned on the committed goldens
and against tests/shuffle_cases.verify; for every case the restatement's multiplicities sum to the usable rows, its running sum ends
at zero and the three quotient terms vanish on every row of the domain for random theta, beta; an altered input is reported missing;
the keygen flag's refusals that need no device; the lookup program check is what it was."""
import json
import os
import random

import numpy as np
import pytest

import custom_gate_cases as gate_cases
import keygen_call
import logup_cases as cases
import lookup_expr_cases as lookup_cases
import phase_cases
import shuffle_cases
from lookup_expr_cases import compress
from oracle import flex as FX

R = cases.R
EINVAL = -1
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _flipped(proof: bytes, at: int) -> bytes:
    out = bytearray(proof)
    out[at] ^= 1
    return bytes(out)


# ---- the verifier with logUp off is the existing one ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [7])
def test_verifier_without_logup_on_the_range_goldens(k):
    g = json.load(open(os.path.join(GOLD, "flex_proofs.json")))
    case = next(c for c in g["cases"] if c["shape"] == "range" and c["k"] == k)
    ocs, oasg = lookup_cases.golden_range_case(g, case)
    vk = FX.VerifierKeys(ocs, k, int(g["srs_secret"], 16), oasg.fixed, oasg.copies)
    lookups = lookup_cases.one_pair_lookups(ocs)
    gates, lks = phase_cases.without_challenges(ocs.gates), phase_cases.without_challenges_lookups(lookups)
    proof = bytes.fromhex(case["proof"])
    assert cases.verify(vk, proof, [oasg.instance], gates, lks) and shuffle_cases.verify(vk, proof, [oasg.instance], gates, lks)
    a_eval = lookup_cases.first_lookup_evaluation_offset(ocs, 1, ocs.degree - 1) + 64
    for at in (3, 32 * ocs.n_advice + 5, a_eval, len(proof) - 1):
        assert not cases.verify(vk, _flipped(proof, at), [oasg.instance], gates, lks)
    assert not cases.verify(vk, proof[:-1], [oasg.instance], gates, lks)
    # the same bytes read as a logUp proof are another proof
    assert not cases.verify(vk, proof, [oasg.instance], gates, lks, logup=True)


@pytest.mark.parametrize("index", range(3))
def test_verifier_without_logup_on_the_shuffle_goldens(h2, index):
    from halo2_scaffold_amd import custom

    g = json.load(open(os.path.join(GOLD, "shuffle_proofs.json")))
    entry = g["cases"][index]
    cs, asg, k = shuffle_cases.build(custom, entry["circuit"])
    first = shuffle_cases.first_assignment(cs, asg)
    ocs = gate_cases.oracle_cs(cs, entry["circuit"])
    oasg = gate_cases.oracle_assignment(ocs, first)
    vk = FX.VerifierKeys(ocs, k, int(g["srs_secret"], 16), oasg.fixed, oasg.copies)
    proof = bytes.fromhex(entry["proof"])
    instances = [list(first.instance)]
    assert cases.verify_circuits(vk, cs, proof, instances, logup=False) and shuffle_cases.verify_circuits(vk, cs, proof, instances)
    for at in (3, 32 * cs.n_advice + 7, len(proof) // 2, len(proof) - 1):
        assert not cases.verify_circuits(vk, cs, _flipped(proof, at), instances, logup=False), at
    if cs.lookups:
        assert not cases.verify_circuits(vk, cs, proof, instances, logup=True)


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def _columns(custom, name, rng):
    """per lookup of a case, with random theta, beta (and challenge): (A, S, M, phi) on all 2^k rows as a logUp prover lays them out —
    blinding scalars in the advice columns' last rows, in M from row u and in phi from row u + 1 — and (u, n, beta)"""
    cs, asg, k = cases.build(custom, name)
    n = 1 << k
    u = n - (cs.blinding_factors() + 1)
    challenges = [rng.randrange(R) for _ in cs.challenge_phase]
    region = asg(challenges) if callable(asg) else asg
    for column in region.advice:  # what the prover puts there
        for row in range(u, n):
            column[row] = rng.randrange(R)
    theta, beta = rng.randrange(R), rng.randrange(R)
    out = []
    for ins, tabs in cases.lookup_rows(cs, region, k, challenges):
        a_rows, s_rows = [compress(t, theta) for t in ins], [compress(t, theta) for t in tabs]
        m, missing = cases.multiplicities(a_rows, s_rows, u)
        assert missing == []
        phi = cases.running_sum(a_rows, s_rows, m, beta, u)
        out.append((a_rows, s_rows, m + [rng.randrange(R) for _ in range(n - u)], phi + [rng.randrange(R) for _ in range(n - u - 1)]))
    return out, u, n, beta


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_running_sum_ends_at_zero_and_the_terms_vanish_on_every_row(h2, name):
    from halo2_scaffold_amd import custom

    rng = random.Random(sum(map(ord, name)))
    columns, u, n, beta = _columns(custom, name, rng)
    assert columns
    for a_rows, s_rows, m, phi in columns:
        assert len(m) == n and len(phi) == n
        assert sum(m[:u]) == u and phi[0] == 0 and phi[u] == 0 and any(phi[1:u])
        for row in range(n):
            l0, ll, la = int(row == 0), int(row == u), int(row < u)
            for y in (1, rng.randrange(R)):  # each of the three terms by itself (y = 1 adds them) and folded
                v = cases.logup_terms(0, y, beta, a_rows[row], s_rows[row], m[row], phi[row], phi[(row + 1) % n], l0, ll, la)
                assert v == 0, (row, y)
        # a wrong multiplicity or a wrong sum is caught on some row
        bad = list(m)
        bad[0] = (bad[0] + 1) % R
        assert any(cases.logup_terms(0, 1, beta, a_rows[r], s_rows[r], bad[r], phi[r], phi[(r + 1) % n], int(r == 0), int(r == u), int(r < u)) for r in range(n))


def test_multiplicities_follow_the_first_occurrence_rule():
    s = [7, 3, 7, 9, 3, 0, 0, 5]
    a = [3, 3, 7, 0, 0, 0, 7, 3]
    m, missing = cases.multiplicities(a, s, 8)
    assert m == [2, 3, 0, 0, 0, 3, 0, 0] and missing == []  # 9 and 5 are taken by no input; the second 7, 3 and 0 stay zero
    m, missing = cases.multiplicities(a[:5] + [4] + a[6:], s, 8)
    assert missing == [5] and sum(m) == 7
    m, missing = cases.multiplicities(a, s, 4)  # only the usable rows count, on both sides
    assert m == [1, 2, 0, 0] and missing == [3]


@pytest.mark.parametrize("name", ["xor", "mixed"])
def test_an_altered_input_is_reported_missing(h2, name):
    from halo2_scaffold_amd import custom

    k = cases.CASES[name]
    cs, asg = lookup_cases.xor_circuit(custom, bad="different rows") if name == "xor" else cases.mixed_circuit(custom, bad=True)
    u = (1 << k) - (cs.blinding_factors() + 1)
    theta = 0x1234567
    ins, tabs = cases.lookup_rows(cs, asg, k)[0]
    m, missing = cases.multiplicities([compress(t, theta) for t in ins], [compress(t, theta) for t in tabs], u)
    last = 3 if name == "xor" else 4
    assert missing == [last] and sum(m) == u - 1
    with pytest.raises(ValueError, match="lookup 'xor' not satisfied at row %d" % last):
        custom.mock(asg, k)


def test_evaluation_counts_and_offsets(h2):
    from halo2_scaffold_amd import custom

    cs, _, _ = cases.build(custom, "mixed")
    m, chunk = len(cs.perm_columns), cs.degree() - 2
    args = (1, len(cs.advice_queries), len(cs.fixed_queries), m, -(-m // chunk), 1, 1)
    assert cases.num_evaluations(*args, logup=False) == shuffle_cases.num_evaluations(*args)
    assert cases.num_evaluations(*args, logup=True) == shuffle_cases.num_evaluations(*args) - 2
    m_at, phi_at, ev_at = cases.proof_offsets(cs)
    assert m_at == 32 * cs.n_advice and phi_at == m_at + 32 * (1 + -(-m // chunk)) and ev_at > phi_at


# ---- the flag ---------------------------------------------------------------------------------------------------------------------------
def test_lookup_program_check_is_what_it_was(h2):
    """the required degree does not depend on the argument: 2 + max(1, deg inputs) + max(1, deg tables) is what the check computes"""
    from halo2_scaffold_amd import custom

    for name, want in (("xor", 5), ("any", 6), ("two", 6), ("mixed", 5)):
        cs, _, k = cases.build(custom, name)
        assert cs.lookup_program().check(cs.abi(k)) == want
    cs, _, k = cases.build(custom, "phased")
    assert cs.degree() == 5 and cs.phases() is not None


def test_the_flag_is_refused_without_a_lookup_program(h2):
    """H2MI_KEYGEN_LOGUP: H2MI_EINVAL from h2mi_prover_keygen with lookups == NULL, whatever else the record holds; an unknown flag bit
    always.  All of it is decided on the host, in front of any device work."""
    from halo2_scaffold_amd import custom, engine

    assert engine.KEYGEN_LOGUP == cases.KEYGEN_LOGUP == 2 and engine.KEYGEN_VK_ONLY == 1
    assert isinstance(engine.BUF_LOGUP_M, int) and engine.BUF_LOGUP_PHI == engine.BUF_LOGUP_M + 1 == engine.BUF_SHUFFLE_TABLE + 2
    cs, asg = gate_cases.is_zero_circuit(custom, 5)
    abi, gates = cs.abi(5), cs.gate_program()
    cells, keep = engine.pack_cells(list(asg.fixed))
    copies = np.zeros((1, 4), dtype=np.uint32)
    ph = engine.AdvicePhases.build([0] * cs.n_advice, [])
    common = dict(fixed=cells, copies=copies.ctypes.data, pk=0)
    for flags in (2, 3, 4):
        assert keygen_call.keygen(abi, flags=flags, **common)[0] == EINVAL
        assert keygen_call.keygen(abi, gates=gates, flags=flags, **common)[0] == EINVAL
        assert keygen_call.keygen(abi, gates=gates, phases=ph, flags=flags, **common)[0] == EINVAL
    # an unknown bit beside a lookup program
    cs2, asg2, k2 = cases.build(custom, "xor")
    abi2, gates2, lks2 = cs2.abi(k2), cs2.gate_program(), cs2.lookup_program()
    cells2, keep2 = engine.pack_cells(list(asg2.fixed))
    assert keygen_call.keygen(abi2, gates=gates2, lookups=lks2, fixed=cells2, copies=copies.ctypes.data, flags=4 | 2, pk=0)[0] == EINVAL
    del keep, keep2
