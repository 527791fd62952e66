"""Several instance columns, the host side (no GPU): the verifier of tests/instance_cases.py — with one column it is the existing one, on
the committed goldens; with two it agrees with oracle.flex.verify on an oracle-made proof — h2mi_gate_program_check at the new column
limit (H2MI_MAX_INSTANCE = 8), custom.ConstraintSystem / Assignment / mock with lists of columns, and the column forms engine.py takes."""
import json
import os

import pytest

import custom_gate_cases as gate_cases
import instance_cases as cases
import lookup_expr_cases as lookup_cases
import phase_cases
from custom_gate_cases import OP_ADD, OP_ADVICE, OP_END, OP_INSTANCE
from oracle import flex as FX

R = cases.R
EINVAL = -1
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def custom(h2):
    from halo2_scaffold_amd import custom

    return custom


@pytest.fixture(scope="module")
def engine(h2):
    from halo2_scaffold_amd import engine

    return engine


def _flipped(proof: bytes, at: int) -> bytes:
    out = bytearray(proof)
    out[at] ^= 1
    return bytes(out)


# ---- the verifier --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,k", [("halo2_lib", None), ("range", 7)])
def test_verifier_with_one_column_on_the_committed_goldens(shape, k):
    """tests/golden/flex_proofs.json: accepted with the circuit's one column, rejected with a public input changed or a byte flipped"""
    g = json.load(open(os.path.join(GOLD, "flex_proofs.json")))
    case = next(c for c in g["cases"] if c["shape"] == shape and (k is None or c["k"] == k))
    if shape == "range":
        ocs, oasg = lookup_cases.golden_range_case(g, case)
        lookups = phase_cases.without_challenges_lookups(lookup_cases.one_pair_lookups(ocs))
        lookups = [([ins], tabs) for ins, tabs in lookups]  # one input set per lookup
    else:
        ocs = FX.flex_gate_cs(False)
        oasg = FX.halo2_lib_assignment(ocs, int(case["x"], 16))
        lookups = []
    vk = FX.VerifierKeys(ocs, case["k"], int(g["srs_secret"], 16), oasg.fixed, oasg.copies)
    gates = phase_cases.without_challenges(ocs.gates)
    proof = bytes.fromhex(case["proof"])
    assert len(oasg.instance) == 1 and oasg.instance[0] == [int(v, 16) for v in case["instance"]]
    assert cases.verify(vk, proof, [oasg.instance], gates, lookups) and FX.verify(vk, proof, oasg.instance)
    assert not cases.verify(vk, proof, [cases.tampered(oasg.instance, 0)], gates, lookups)
    assert not cases.verify(vk, proof, [oasg.instance + [[]]], gates, lookups)  # a column the circuit does not have
    for at in (3, len(proof) // 2, len(proof) - 1):
        assert not cases.verify(vk, _flipped(proof, at), [oasg.instance], gates, lookups)
    assert not cases.verify(vk, proof, [oasg.instance], gates, lookups, multiopen="gwc")  # the same bytes read with the other tail


def test_verifier_agrees_with_the_oracle_on_two_columns(custom):
    """an oracle-made proof of two_cols at k = 4: both verifiers accept it, and both reject it with one value of either column changed,
    with the columns swapped, or with a byte flipped"""
    cs, asg = cases.two_cols_circuit(custom)
    k = 4
    custom.mock(asg, k)
    ocs = cases.oracle_cs(cs, "two_cols")
    oasg = cases.oracle_assignment(ocs, cs, asg)
    assert len(oasg.instance) == 2 and oasg.instance == [list(c) for c in asg.instance]
    okeys = FX.Keys(ocs, k, 0x5EC2E7, oasg.fixed, oasg.copies)
    proof = FX.prove(okeys, oasg, 5)["proof"]
    both = lambda pf, inst: (FX.verify(okeys, pf, inst), cases.verify_circuits(okeys, cs, pf, [inst]))
    assert both(proof, oasg.instance) == (True, True)
    for c in range(2):
        assert both(proof, cases.tampered(oasg.instance, c)) == (False, False)
    assert both(proof, oasg.instance[::-1]) == (False, False)
    for at in (1, len(proof) // 3, len(proof) - 2):
        assert both(_flipped(proof, at), oasg.instance) == (False, False)
    assert not cases.verify_circuits(okeys, cs, proof, [oasg.instance[:1]])


# ---- the ABI's checks ------------------------------------------------------------------------------------------------------------------
def _code(engine, cs, ops):
    try:
        return engine.GateProgram.build(ops, []).check(cs)
    except engine.H2miError as e:
        return e.code


def test_program_check_takes_up_to_eight_instance_columns(engine):
    """h2mi_gate_program_check: a query of instance column 2 of 3 is accepted (the parent commit refused n_instance > 1); nine columns
    or a query of column 3 of 3 are H2MI_EINVAL"""
    build = lambda n_instance: engine.ConstraintSystem.build(5, 1, 0, n_instance, 3, 5, engine.GATES_EXPRESSIONS, [], [], [], [(0, 0)], [])
    ops = lambda column: [(OP_ADVICE, 0, 0), (OP_INSTANCE, column, 1), (OP_ADD, 0, 0), (OP_END, 0, 0)]
    assert engine.MAX_INSTANCE == cases.MAX_INSTANCE == 8
    assert _code(engine, build(3), ops(2)) == (1, 2)
    assert _code(engine, build(8), ops(7)) == (1, 2)
    assert _code(engine, build(1), ops(0)) == (1, 2)
    assert _code(engine, build(9), ops(2)) == EINVAL
    assert _code(engine, build(3), ops(3)) == EINVAL
    assert _code(engine, build(8), ops(8)) == EINVAL
    assert _code(engine, build(0), ops(0)) == EINVAL


def test_constraint_system_with_two_instance_columns_builds_its_abi(custom, engine):
    """custom.ConstraintSystem.abi (the parent commit asserted n_instance <= 1), the program's INSTANCE ops carry the column, the
    permutation columns name both"""
    cs, asg = cases.two_cols_circuit(custom)
    abi = cs.abi(5)
    assert abi.n_instance == 2 and cs.instance_queries == [(0, 0), (1, 0), (1, 1)]
    assert [(abi.perm_columns[j].kind, abi.perm_columns[j].index) for j in range(abi.n_perm)] == [(engine.ADVICE, 0), (engine.INSTANCE, 0), (engine.INSTANCE, 1)]
    ops, _ = cs.program()
    assert [(index, rot) for op, index, rot in ops if op == OP_INSTANCE] == [(0, 0), (1, 1)]
    assert cs.gate_program().check(abi)[0] == 2
    cs8, asg8 = cases.eight_cols_circuit(custom)
    abi8 = cs8.abi(5)
    assert abi8.n_instance == 8 and cs8.gate_program().check(abi8)[0] == 3 == cs8.degree()
    u = 32 - (cs8.blinding_factors() + 1)
    assert [len(c) for c in asg8.instance] == cases.eight_cols_counts(u) and u > 17
    nine = custom.ConstraintSystem()
    nine.advice_column()
    for _ in range(9):
        nine.instance_column()
    with pytest.raises(AssertionError):
        nine.abi(5)


def test_mock_follows_the_column(custom):
    for name in ("two_cols", "eight_cols", "in_arguments"):
        cs, asg, k = cases.build(custom, name)
        first = cases.first_assignment(cs, asg)
        if callable(asg):
            challenges = [7]
            custom.mock(asg(challenges), k, challenges)
        else:
            custom.mock(asg, k)
        assert len(cases.columns_of(cs, first)) == cs.n_instance
    cs, bad = cases.eight_cols_circuit(custom, bad="copy5")
    with pytest.raises(ValueError, match=r"copy constraint .*'instance', 5, 4"):
        custom.mock(bad, 5)
    cs, bad = cases.eight_cols_circuit(custom, bad="gate5")
    with pytest.raises(ValueError, match="gate 'all eight' not satisfied at row 9"):  # the only row that reads i5 on row 9
        custom.mock(bad, 5)
    cs, asg = cases.two_cols_circuit(custom)
    asg.instance[1] = asg.instance[1] + [0] * 40
    with pytest.raises(ValueError, match="NotEnoughRowsAvailable: instance column 1"):
        custom.mock(asg, 5)
    # one column: the flat form and every message stay what they were
    cs1, asg1 = gate_cases.degree6_circuit(custom, 3, 7)
    assert asg1.instance and all(isinstance(v, int) for v in asg1.instance)
    custom.mock(asg1, 5)


def test_engine_column_forms(engine):
    """a flat list is one column and travels as before; a list of lists is the columns; the transcript order is column by column"""
    assert engine.instance_columns([1, 2, 3]) is None and engine.instance_columns([]) is None
    assert engine.instance_columns([[1], [], [2, 3]]) == [[1], [], [2, 3]]
    assert engine.instance_values([4, 5]) == [4, 5]
    assert engine.instance_values([[1], [], [2, 3]]) == [1, 2, 3]
    with pytest.raises(ValueError):
        engine.instance_columns([1, [2]])
