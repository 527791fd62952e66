"""CPU tests of lookups given as data: the helper verifier of tests/lookup_expr_cases.py pinned against oracle.flex.verify on the
committed range goldens; h2mi_lookup_program_check (host only) on the circuits of the GPU tests and on programs it must refuse;
custom.mock on satisfying and unsatisfied witnesses; custom.py's bookkeeping for lookups."""
import json
import os

import pytest

import custom_gate_cases as gate_cases
import lookup_expr_cases as cases
from custom_gate_cases import OP_ADVICE, OP_END, OP_FIXED, OP_MUL
from oracle import flex as FX

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDENS = [("flex_proofs.json", 7), ("flex_multi_proofs.json", 5), ("flex_multi_proofs.json", 6)]  # q_lookup * a; lookup-advice columns


@pytest.mark.parametrize("name,k", GOLDENS)
def test_helper_verifier_agrees_with_the_oracle_on_the_range_goldens(h2, name, k):
    from halo2_scaffold_amd import engine, flex

    g = json.load(open(os.path.join(GOLD, name)))
    case = next(c for c in g["cases"] if c["shape"] == "range" and c["k"] == k)
    cs, _, abi = cases.golden_product_case(flex, engine, case)
    assert engine.LookupProgram.build(*cases.one_pair_ops(abi), []).check(abi) == cs.degree  # the program the GPU test proves with
    ocs, oasg = cases.golden_range_case(g, case)
    vk = FX.VerifierKeys(ocs, k, int(g["srs_secret"], 16), oasg.fixed, oasg.copies)
    lookups = cases.one_pair_lookups(ocs)
    assert len(lookups) == 1
    proof = bytes.fromhex(case["proof"])
    flipped = bytearray(proof)
    flipped[cases.first_lookup_evaluation_offset(ocs, 1, ocs.degree - 1) + 64] ^= 1  # A'(x) of the lookup
    other = [[(oasg.instance[0][0] + 1) % FX.R]]
    for p, inst, want in ((proof, oasg.instance, True), (bytes(flipped), oasg.instance, False), (proof, other, False), (proof[:-1], oasg.instance, False)):
        assert FX.verify(vk, p, inst) is want
        assert cases.verify(vk, p, inst, lookups) is want


@pytest.mark.parametrize("name", sorted(cases.CIRCUITS))
def test_program_check_accepts_the_circuits(h2, name):
    from halo2_scaffold_amd import custom

    build, k = cases.CIRCUITS[name]
    cs, asg = build(custom)
    abi, lp = cs.abi(k), cs.lookup_program()
    want = {"xor": 5, "any": 6, "two": 6}[name]
    assert lp.check(abi) == want == cs.degree() and abi.degree == want
    assert abi.n_lookups == len(cs.lookups) == lp.n_lookups
    custom.mock(asg, k)


def test_program_check_refusals(h2):
    from halo2_scaffold_amd import custom, engine
    from halo2_scaffold_amd._lib import H2miError

    cs, _ = cases.xor_circuit(custom)
    abi, lp = cs.abi(5), cs.lookup_program()
    assert lp.check(abi) == 5
    ops = [(op.op, op.index, op.rotation) for op in lp._exprs._ops[: lp.exprs.n_ops]]

    def refused(n_pairs, ops, abi_=abi):
        with pytest.raises(H2miError) as e:
            engine.LookupProgram.build(n_pairs, ops, []).check(abi_)
        return e.value.code == -1

    assert engine.LookupProgram.build([3], ops, []).check(abi) == 5  # the same ops rebuilt by hand
    unqueried = [(OP_ADVICE, 0, 1) if o == (OP_ADVICE, 0, 0) else o for o in ops]  # a(wX) is in no query list
    assert unqueried != ops and refused([3], unqueried)
    assert refused([2], ops) and refused([4], ops)                                  # 2 * sum n_pairs != the polynomial count
    assert refused([3, 0], ops) and refused([0], ops)                               # n_lookups != cs.n_lookups; n_pairs = 0
    two = cs.abi(5)
    two.n_lookups = 2
    assert refused([3, 0], ops, two) and refused([0, 3], ops, two)
    low = cs.abi(5)
    low.degree = 4                                                                  # the argument needs 2 + 2 + 1 = 5
    assert refused([3], ops, low)
    three = cs.abi(5)
    three.degree = 3                                                                # no lookup fits a degree-3 constraint system
    plain = [(OP_ADVICE, 0, 0), (OP_END, 0, 0), (OP_FIXED, 0, 0), (OP_END, 0, 0)]
    assert refused([1], plain, three)
    three.degree = 4
    assert engine.LookupProgram.build([1], plain, []).check(three) == 4
    deg3_in = [(OP_ADVICE, 0, 0)] * 3 + [(OP_MUL, 0, 0)] * 2 + [(OP_END, 0, 0), (OP_FIXED, 0, 0), (OP_END, 0, 0)]
    assert refused([1], deg3_in, abi)                                               # 2 + 3 + 1 = 6 > 5
    six = cs.abi(5)
    six.degree = 6
    assert engine.LookupProgram.build([1], deg3_in, []).check(six) == 6
    assert refused([1], [(OP_ADVICE, 0, 0), (OP_MUL, 0, 0), (OP_END, 0, 0), (OP_FIXED, 0, 0), (OP_END, 0, 0)], abi)  # stack underflow


@pytest.mark.parametrize("bad", sorted(cases.XOR_BAD))
def test_mock_refuses_unsatisfied_lookups(h2, bad):
    """a tuple absent from the table, and one whose components each occur in their table column but never on one row"""
    from halo2_scaffold_amd import custom

    cs, asg = cases.xor_circuit(custom, bad=bad)
    x, y, z = cases.XOR_BAD[bad]
    columns = [{asg.fixed[c].get(r, 0) for r in range(16)} for c in range(3)]
    assert all(v in col for v, col in zip((x, y, z), columns)) == (bad == "different rows")
    with pytest.raises(ValueError, match="lookup 'xor' not satisfied at row 3"):
        custom.mock(asg, 5)


def test_lookup_queries_enter_the_bookkeeping(h2):
    from halo2_scaffold_amd import custom

    cs, _ = cases.any_circuit(custom)
    assert cs.advice_queries == [(0, 0), (2, 0), (3, 1), (1, -1)]  # enable_equality a, x; the gate's y(wX); the lookup's b(w^-1 X)
    assert cs.blinding_factors() == 5 and cs.degree() == 6
    assert [len(p) for p in cs.lookups] == [2]
    plain, _ = gate_cases.is_zero_circuit(custom, 3)
    assert plain.lookup_program() is None and plain.abi(5).n_lookups == 0


def test_xor4_circuit_scales_and_stays_satisfied(h2):
    """the scalable XOR circuit of the GPU tests at k = 11: same degree and program shape as xor_circuit, inputs on every usable row
    but the margin, about 60 % of them one triple, some rows with the selector off; the broken row sits in the second 1024 rows"""
    from halo2_scaffold_amd import custom

    k = 11
    cs, asg = cases.xor4_circuit(custom, k)
    abi, lp = cs.abi(k), cs.lookup_program()
    assert lp.check(abi) == 5 == cs.degree() and abi.n_lookups == 1 and [len(p) for p in cs.lookups] == [3]
    custom.mock(asg, k)
    triples = cases.xor4_triples(k)
    rows = cases.xor4_rows(k)
    assert len(triples) == rows == (1 << k) - 6 - cases.XOR4_MARGIN and max(asg.advice[0]) == rows - 1 and max(asg.advice[3]) == rows + 1
    assert 0.55 * rows < triples.count(cases.XOR4_OFTEN) < 0.65 * rows and 10 < triples.count(None) < 40
    assert len({t for t in triples if t}) > 200 and all(t is None or t[0] ^ t[1] == t[2] for t in triples)
    x, y, z = cases.XOR4_ABSENT
    assert x ^ y != z and triples[1500] is not None
    _, broken = cases.xor4_circuit(custom, k, bad_row=1500)
    with pytest.raises(ValueError, match="lookup 'xor4' not satisfied at row 1500"):
        custom.mock(broken, k)
