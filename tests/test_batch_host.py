"""CPU tests of several circuits per proof: the N-circuit verifier of tests/batch_cases.py pinned with N = 1 on the committed range
goldens, the StandardPlonk golden and committed proofs of the phase circuits of tests/phase_cases.py (the same verdict as that file's
verifier, on the proofs and on each with a byte flipped), and on committed two-circuit proofs; the Python-integer batched quotient
with one circuit against the single-circuit restatement on the random programs of tests/custom_gate_cases.py."""
import json
import os
import random

import pytest

import batch_cases as cases
import custom_gate_cases as gate_cases
import lookup_expr_cases as lookup_cases
import phase_cases
from oracle import flex as FX

R = cases.R
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDENS = [("flex_proofs.json", 7), ("flex_multi_proofs.json", 5), ("flex_multi_proofs.json", 6)]  # those of tests/test_phases_host.py


def _flipped(proof: bytes, at: int) -> bytes:
    out = bytearray(proof)
    out[at] ^= 1
    return bytes(out)


@pytest.mark.parametrize("name,k", GOLDENS)
def test_batch_verifier_with_one_circuit_on_the_range_goldens(name, k):
    g = json.load(open(os.path.join(GOLD, name)))
    case = next(c for c in g["cases"] if c["shape"] == "range" and c["k"] == k)
    ocs, oasg = lookup_cases.golden_range_case(g, case)
    vk = FX.VerifierKeys(ocs, k, int(g["srs_secret"], 16), oasg.fixed, oasg.copies)
    lookups = lookup_cases.one_pair_lookups(ocs)
    gates, lks = phase_cases.without_challenges(ocs.gates), phase_cases.without_challenges_lookups(lookups)
    proof = bytes.fromhex(case["proof"])
    assert phase_cases.verify(vk, proof, oasg.instance, gates, lks) and cases.verify(vk, proof, [oasg.instance], gates, lks)
    a_eval = lookup_cases.first_lookup_evaluation_offset(ocs, 1, ocs.degree - 1) + 64
    for at in (3, a_eval, len(proof) - 1):
        assert not phase_cases.verify(vk, _flipped(proof, at), oasg.instance, gates, lks)
        assert not cases.verify(vk, _flipped(proof, at), [oasg.instance], gates, lks)
    other = [[(oasg.instance[0][0] + 1) % R]]
    assert not cases.verify(vk, proof, [other], gates, lks) and not cases.verify(vk, proof[:-1], [oasg.instance], gates, lks)
    assert not cases.verify(vk, proof, [oasg.instance, oasg.instance], gates, lks) and not cases.verify(vk, proof, [], gates, lks)


def test_batch_verifier_with_one_circuit_on_the_standard_plonk_golden():
    g = json.load(open(os.path.join(GOLD, "standard_plonk_proofs.json")))
    case = next(c for c in g["cases"] if c["k"] == 5)
    ocs = FX.standard_plonk_cs()
    oasg = FX.standard_plonk_assignment(ocs, int(case["witness_x"], 16) if isinstance(case["witness_x"], str) else case["witness_x"])
    vk = FX.VerifierKeys(ocs, 5, int(g["srs_secret"], 16), oasg.fixed, oasg.copies)
    gates = phase_cases.without_challenges(ocs.gates)
    proof = bytes.fromhex(case["proof"])
    assert FX.verify(vk, proof, []) and phase_cases.verify(vk, proof, [], gates, []) and cases.verify(vk, proof, [[]], gates, [])
    for at in (3, 32 * 9 + 5, len(proof) - 1):
        assert not phase_cases.verify(vk, _flipped(proof, at), [], gates, []) and not cases.verify(vk, _flipped(proof, at), [[]], gates, [])
    assert not cases.verify(vk, proof, [[], []], gates, [])


def _golden_batch_cases():
    return json.load(open(os.path.join(GOLD, "batch_proofs.json")))


def _phase_circuit(custom, entry):
    """a case of tests/golden/batch_proofs.json -> (cs, first assignment, k): the circuits of tests/phase_cases.py, as the GPU tests
    build them"""
    build, k = phase_cases.CIRCUITS[entry["circuit"]]
    cs, synthesize = build(custom)
    return cs, synthesize([None] * len(cs.challenge_phase)), k


@pytest.mark.parametrize("index", range(4))
def test_batch_verifier_on_committed_phase_proofs(h2, index):
    """proofs the device made of the two circuits phase_cases builds (tests/golden/batch_proofs.json: one circuit and two per proof).
    One circuit: the verdict of phase_cases' verifier, accepted and with a byte flipped.  Two circuits: accepted; rejected with a byte
    flipped, with the circuits' public inputs exchanged for others, and read as one circuit."""
    from halo2_scaffold_amd import custom

    g = _golden_batch_cases()
    entry = g["cases"][index]
    cs, first, k = _phase_circuit(custom, entry)
    ocs = gate_cases.oracle_cs(cs, entry["circuit"])
    oasg = gate_cases.oracle_assignment(ocs, first)
    vk = FX.VerifierKeys(ocs, k, int(g["srs_secret"], 16), oasg.fixed, oasg.copies)
    proof, n = bytes.fromhex(entry["proof"]), entry["circuits"]
    instances = [list(first.instance)] * n
    assert cases.verify_circuits(vk, cs, proof, instances)
    flips = (3, 32 * cs.n_advice * n + 7, len(proof) // 2, len(proof) - 1)
    for at in flips:
        assert not cases.verify_circuits(vk, cs, _flipped(proof, at), instances), at
    if n == 1:
        assert phase_cases.verify_circuit(vk, cs, proof, oasg.instance)
        for at in flips:
            assert not phase_cases.verify_circuit(vk, cs, _flipped(proof, at), oasg.instance)
    else:
        assert not phase_cases.verify_circuit(vk, cs, proof, oasg.instance) and not cases.verify_circuits(vk, cs, proof, instances[:1])
        if cs.n_instance:
            assert not cases.verify_circuits(vk, cs, proof, [instances[0], [(instances[1][0] + 1) % R]])


def test_committed_phase_proofs_cover_both_circuits():
    g = _golden_batch_cases()
    assert sorted((c["circuit"], c["circuits"]) for c in g["cases"]) == [("rlc", 1), ("rlc", 2), ("three", 1), ("three", 2)]


@pytest.mark.parametrize("case", range(4, 12))
def test_batched_quotient_with_one_circuit_is_the_single_restatement(h2, case):
    """without permutation and lookups and with N = 1 the fold is h[i] = (Horner in y over the polynomials) t_inv[i mod 2^(ek - k)]: the
    restatement tests/test_gpu_custom_gates.py compares the single-circuit kernel with, on its random programs"""
    import test_gpu_custom_gates as single
    from halo2_scaffold_amd import custom
    from halo2_scaffold_amd.domain import EvaluationDomain

    k, degree, trees = single._kernel_case(custom, case)
    dom = EvaluationDomain(degree, k)
    size, rot = 1 << dom.extended_k, 1 << (dom.extended_k - k)
    rng = random.Random(5 + case)
    column = lambda: [rng.randrange(R) for _ in range(size)]
    data = {("advice", j): column() for j in range(single.N_ADV)}
    data.update({("fixed", j): column() for j in range(single.N_FIX)})
    data[("instance", 0)] = column()
    constants, ops = {}, []
    for t in trees:
        ops += t.program(constants)[0]
    consts = sorted(constants, key=constants.get)
    y = rng.randrange(R)
    tinv = [pow((pow(dom.g_coset * pow(dom.extended_omega, i, R) % R, 1 << k, R) - 1) % R, -1, R) for i in range(rot)]
    want = []
    for idx in range(size):
        q = lambda op, c, r: data[(single.KINDS[op], c)][(idx + r * rot) % size]
        polys, _ = gate_cases.run_postfix(ops, consts, q)
        v = 0
        for p in polys:
            v = (v * y + p) % R
        want.append(v * tinv[idx % rot] % R)
    circuit = {"advice": [data[("advice", j)] for j in range(single.N_ADV)], "fixed": [data[("fixed", j)] for j in range(single.N_FIX)],
               "instance": data[("instance", 0)], "perm_values": [], "perm_zs": [], "lookups": []}
    unused = column()
    shared = {"perm_sigmas": [], "chunk": 1, "l0": unused, "l_last": unused, "l_active": unused}
    got = cases.batched_quotient(k, dom.extended_k, dom.g_coset, dom.extended_omega, cases.keys_delta(), 5, ops, consts, [], [circuit], shared,
                                 rng.randrange(R), rng.randrange(R), y)
    assert got == want
    # two circuits: the second fold continues the first (y^T H_0 + H_1 with T polynomials per circuit)
    two = cases.batched_quotient(k, dom.extended_k, dom.g_coset, dom.extended_omega, cases.keys_delta(), 5, ops, consts, [], [circuit, circuit], shared, 1, 2, y)
    assert two == [(pow(y, len(trees), R) + 1) * h % R for h in want]
