"""CPU tests of advice phases and challenges: the helper verifier of tests/phase_cases.py pinned on the committed range goldens that pin
the one of tests/lookup_expr_cases.py (no phases, no challenges); h2mi_advice_phases_check (host only) on the circuits of the GPU
tests and on what it must refuse; the older check functions on a program that holds a CHALLENGE op; custom.py's bookkeeping and mock."""
import json
import os

import pytest

import lookup_expr_cases as lookup_cases
import phase_cases as cases
from phase_cases import OP_ADVICE, OP_CHALLENGE, OP_END, OP_FIXED, OP_MUL
from oracle import flex as FX

R = cases.R
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDENS = [("flex_proofs.json", 7), ("flex_multi_proofs.json", 5), ("flex_multi_proofs.json", 6)]  # those of tests/test_lookup_exprs_host.py


@pytest.mark.parametrize("name,k", GOLDENS)
def test_phase_verifier_agrees_on_the_range_goldens(h2, name, k):
    """it accepts what lookup_expr_cases.verify accepts and rejects each golden proof with one byte flipped (a byte of the first
    advice commitment, of the lookup's A'(x) and the last byte)"""
    g = json.load(open(os.path.join(GOLD, name)))
    case = next(c for c in g["cases"] if c["shape"] == "range" and c["k"] == k)
    ocs, oasg = lookup_cases.golden_range_case(g, case)
    vk = FX.VerifierKeys(ocs, k, int(g["srs_secret"], 16), oasg.fixed, oasg.copies)
    lookups = lookup_cases.one_pair_lookups(ocs)
    gates, lks = cases.without_challenges(ocs.gates), cases.without_challenges_lookups(lookups)
    proof = bytes.fromhex(case["proof"])
    assert lookup_cases.verify(vk, proof, oasg.instance, lookups) and cases.verify(vk, proof, oasg.instance, gates, lks)
    a_eval = lookup_cases.first_lookup_evaluation_offset(ocs, 1, ocs.degree - 1) + 64
    for at in (3, a_eval, len(proof) - 1):
        flipped = bytearray(proof)
        flipped[at] ^= 1
        assert not lookup_cases.verify(vk, bytes(flipped), oasg.instance, lookups)
        assert not cases.verify(vk, bytes(flipped), oasg.instance, gates, lks)
    other = [[(oasg.instance[0][0] + 1) % R]]
    assert not cases.verify(vk, proof, other, gates, lks) and not cases.verify(vk, proof[:-1], oasg.instance, gates, lks)


@pytest.mark.parametrize("name", sorted(cases.CIRCUITS))
def test_phases_check_accepts_the_circuits(h2, name):
    from halo2_scaffold_amd import custom

    build, k = cases.CIRCUITS[name]
    cs, synthesize = build(custom)
    abi, gates, lp, ph = cs.abi(k), cs.gate_program(), cs.lookup_program(), cs.phases()
    ph.check(abi, gates, lp)
    want = {"rlc": ([0, 1], [0], 3), "three": ([0, 0, 1, 2], [0, 1], 5)}[name]
    assert (cs.advice_phase, cs.challenge_phase, cs.degree()) == want
    assert ph.n_phases == cs.n_phases == 1 + max(want[0]) and ph.n_challenges == len(want[1])
    assert list(ph.advice_phase[: cs.n_advice]) == want[0] and list(ph.challenge_phase[: ph.n_challenges]) == want[1]


def _refused(fn, *args):
    from halo2_scaffold_amd._lib import H2miError

    with pytest.raises(H2miError) as e:
        fn(*args)
    return e.value.code == -1  # H2MI_EINVAL


def test_phases_check_refusals(h2):
    from halo2_scaffold_amd import custom, engine

    cs, _ = cases.rlc_circuit(custom)
    abi, gates = cs.abi(5), cs.gate_program()
    build = engine.AdvicePhases.build
    build([0, 1], [0]).check(abi, gates)
    build([0, 1], [0, 1, 1]).check(abi, gates)                      # challenges no gate reads are allowed
    assert _refused(build([1, 1], [1]).check, abi, gates)           # a phase-1 column without a phase-0 column
    assert _refused(build([0, 2], [0], n_phases=3).check, abi, gates)  # phase 2 without phase 1
    assert _refused(build([0, 0], [1], n_phases=2).check, abi, gates)  # a challenge after a phase that has no column
    assert _refused(build([0, 0], [1]).check, abi, gates)           # the same with n_phases = 1: the challenge's phase is beyond it
    assert _refused(build([0, 1], []).check, abi, gates)            # the gate's CHALLENGE 0 with n_challenges = 0
    assert _refused(build([0, 1], [0] * 17).check, abi, gates)      # 17 challenges
    assert _refused(build([0, 3], [0], n_phases=4).check, abi, gates)  # phase 3
    assert _refused(build([0, 1], [0], n_phases=0).check, abi, gates)
    ops = [(OP_ADVICE, 0, 0), (OP_CHALLENGE, 1, 0), (OP_MUL, 0, 0), (OP_END, 0, 0)]
    beyond = engine.GateProgram.build(ops, [])
    assert _refused(build([0, 1], [0]).check, abi, beyond)          # a CHALLENGE index >= n_challenges
    build([0, 1], [0, 1]).check(abi, beyond)
    sixteen = engine.GateProgram.build([(OP_ADVICE, 0, 0), (OP_CHALLENGE, 15, 0), (OP_MUL, 0, 0), (OP_END, 0, 0)], [])
    build([0, 1], [0] * 16).check(abi, sixteen)                     # the limit itself
    vertical = cs.abi(5)
    vertical.gates = engine.GATES_FLEX_VERTICAL
    assert _refused(build([0, 1], [0]).check, vertical, gates)      # cs->gates other than H2MI_GATES_EXPRESSIONS
    # the lookup program's challenges are counted the same way
    cs3, _ = cases.three_phase_circuit(custom)
    abi3, gates3, lp3 = cs3.abi(6), cs3.gate_program(), cs3.lookup_program()
    build([0, 0, 1, 2], [0, 1]).check(abi3, gates3, lp3)
    one_challenge_gates = engine.GateProgram.build([(OP_ADVICE, 0, 0), (OP_END, 0, 0)], [])
    build([0, 0, 1, 2], [0]).check(abi3, one_challenge_gates, lp3)
    assert _refused(build([0, 0, 1, 2], []).check, abi3, one_challenge_gates, lp3)


def test_older_checks_refuse_the_challenge_op(h2):
    """h2mi_gate_program_check and h2mi_lookup_program_check know of no challenges"""
    from halo2_scaffold_amd import custom, engine

    cs, _ = cases.rlc_circuit(custom)
    assert _refused(cs.gate_program().check, cs.abi(5))
    plain = [(OP_ADVICE, 0, 0), (OP_ADVICE, 1, 0), (OP_MUL, 0, 0), (OP_END, 0, 0)]
    assert engine.GateProgram.build(plain, []).check(cs.abi(5)) == (2, 2)  # the same program without the op passes
    cs3, _ = cases.three_phase_circuit(custom)
    abi3 = cs3.abi(6)
    assert _refused(cs3.lookup_program().check, abi3)
    no_challenge = [(OP_ADVICE, 2, 0), (OP_FIXED, 2, 0), (OP_MUL, 0, 0), (OP_END, 0, 0), (OP_FIXED, 0, 0), (OP_END, 0, 0)]
    assert engine.LookupProgram.build([1], no_challenge, []).check(abi3) == 5


def test_custom_bookkeeping_for_phases_and_challenges(h2):
    from halo2_scaffold_amd import custom, engine

    meta = custom.ConstraintSystem()
    with pytest.raises(AssertionError):
        meta.advice_column_in(1)             # no phase-0 column yet
    a = meta.advice_column()
    with pytest.raises(AssertionError):
        meta.advice_column_in(2)             # no phase-1 column yet
    with pytest.raises(AssertionError):
        meta.challenge_usable_after(1)       # no column in phase 1
    with pytest.raises(AssertionError):
        meta.advice_column_in(3)
    assert meta.phases() is None and meta.n_phases == 1
    ch = meta.challenge_usable_after(0)
    assert (ch.index, ch.phase) == (0, 0) and meta.phases().n_challenges == 1 and meta.phases().n_phases == 1
    b = meta.advice_column_in(1)
    ch1 = meta.challenge_usable_after(1)
    assert (b.index, ch1.index, meta.n_phases) == (1, 1, 2)
    e = meta.query_challenge(ch1)
    assert e.degree() == 0 and e.stack_depth() == 1 and e.resolve(3) is e
    assert e.program() == ([(engine.EXPR_CHALLENGE, 1, 0), (engine.EXPR_END, 0, 0)], [])
    prod = meta.query_advice(a, 0) * e * meta.query_challenge(ch) - e
    assert prod.degree() == 1
    ops, consts = prod.program()
    assert [op for op, _, _ in ops].count(engine.EXPR_CHALLENGE) == 3 and consts == []
    q = lambda kind, c, r: 7
    assert prod.evaluate(q, [5, 11]) == (7 * 11 * 5 - 11) % R
    assert cases.run_postfix(ops, consts, lambda op, c, r: 7, [5, 11]) == [(7 * 11 * 5 - 11) % R]
    region = custom.Assignment(meta, challenges=[9, None])
    assert region.get_challenge(ch) == 9 and region.get_challenge(ch1) is None
    assert custom.Assignment(meta).get_challenge(ch) is None
    # a circuit without phases keeps its ABI: no phases struct, nothing new in its program
    plain, _ = lookup_cases.xor_circuit(custom)
    assert plain.phases() is None and plain.advice_phase == [0] * 4


@pytest.mark.parametrize("name", sorted(cases.CIRCUITS))
def test_mock_with_challenges(h2, name):
    """mock accepts the circuits with the challenge values their witness was made with, and names the failing gate when the phase-1
    witness was made with another value"""
    from halo2_scaffold_amd import custom

    build, k = cases.CIRCUITS[name]
    cs, synthesize = build(custom)
    challenges = [0x1234567 + 3 * i for i in range(len(cs.challenge_phase))]
    custom.mock(synthesize(challenges), k, challenges)
    custom.mock(synthesize([R - 1] * len(challenges)), k, [R - 1] * len(challenges))
    _, wrong = build(custom, 1)  # the phase-1 witness made with challenge 0 plus one
    gate = {"rlc": "rlc step", "three": "r = a \\+ c0 b"}[name]
    with pytest.raises(ValueError, match=f"gate '{gate}' not satisfied at row 0"):
        custom.mock(wrong(challenges), k, challenges)
    with pytest.raises(ValueError, match="not satisfied"):
        custom.mock(synthesize(challenges), k, [c + 1 for c in challenges])  # the right witness checked against other values
