"""The witness check, the host side (no GPU): the cases of tests/check_cases.py checked against themselves — every satisfied case
passes the host mock, every broken case's expected first violation is the one the host mock names, the planted level-A programs
give the planted report when the program is run row by row — and h2mi_shape_gate_program (include/h2mi_prover.h), the gate program
equivalent to a hard-wired shape, against vertical_gate_ops and the StandardPlonk polynomial of tests/custom_gate_cases.py."""
import ctypes as C
import random

import pytest

import check_cases as cases
import custom_gate_cases as gate_cases
import phase_cases

R = cases.R
EINVAL, ERANGE = -1, -6


@pytest.fixture(scope="module")
def custom(h2):
    from halo2_scaffold_amd import custom

    return custom


@pytest.fixture(scope="module")
def flex(h2):
    from halo2_scaffold_amd import flex

    return flex


@pytest.fixture(scope="module")
def engine(h2):
    from halo2_scaffold_amd import engine

    return engine


# ---- level A ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 6])
def test_planted_programs_report_what_was_planted(custom, k):
    n = 1 << k
    for n_rows in (n, n - 6):
        case = cases.planted_case(custom, k, 0, n_rows=n_rows)
        assert cases.report_by_evaluation(case) == case["want"]
        assert case["want"][0] == (0, cases.NONE) and case["want"][1] == (1, 0) and case["want"][5] == (n_rows, 0)
        assert case["want"][6] == ((2, 5) if n_rows == n else (1, 5))  # the rows at or beyond n_rows are not counted
        assert {1 + 1, 8} <= set(case["depths"])
        used = {op for op, _, _ in case["ops"]}
        assert used == set(range(10)) - {2} or used == set(range(10))  # every operator, a constant, a challenge
        assert {r for op, _, r in case["ops"] if op <= 2} == set(range(-3, 4))


def test_many_polynomials_and_redundant_zeros(custom):
    case = cases.many_polynomials_case(custom, k=6)
    assert len(case["want"]) >= 40 and case["want"][0][0] and case["want"][-1][0] and (0, cases.NONE) in case["want"]
    assert cases.report_by_evaluation(case) == case["want"]
    zero = cases.redundant_zero_case(4)
    assert len(zero["consts"]) == 256 and cases.report_by_evaluation(zero) == zero["want"] == [(0, cases.NONE)] * 8


# ---- level B ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.DATA_CIRCUITS))
def test_data_circuits(custom, name):
    k, build, broken = cases.DATA_CIRCUITS[name]
    cs, good = build(custom)
    custom.mock(good, k)
    assert cases.host_report(good, k) == []
    bad = broken(custom)
    report = cases.host_report(bad, k)
    assert report
    with pytest.raises(ValueError) as e:
        custom.mock(bad, k)
    assert str(e.value) == cases.first_violation(report, cs)


@pytest.mark.parametrize("name", ["rlc", "three"])
def test_phase_circuits(custom, name):
    build, k = phase_cases.CIRCUITS[name]
    cs, synthesize = build(custom)
    ch = [0x1234567, 0x89ABCDE][: len(cs.challenge_phase)]
    custom.mock(synthesize(ch), k, ch)
    assert cases.host_report(synthesize(ch), k, ch) == []
    _, wrong = build(custom, 1)
    report = cases.host_report(wrong(ch), k, ch)
    with pytest.raises(ValueError) as e:
        custom.mock(wrong(ch), k, ch)
    assert str(e.value) == cases.first_violation(report, cs)
    if name == "three":  # a wrong c0: the gate that defines r, and the lookup of r
        assert [entry[0] for entry in report] == [cases.GATE, cases.LOOKUP]


def test_boolean_and_copy_circuits(custom):
    cs, asg = cases.boolean_circuit(custom)
    custom.mock(asg, 5)
    assert not any(name for name in cs.gate_names if name != "boolean") and cs.n_selectors == 0
    for k, cycles in ((9, 120), (11, 500)):
        cs, good, _ = cases.copies_circuit(custom, k, cycles)
        custom.mock(good, k)
        moved = {cell for pair in good.copies for cell in pair}
        assert len(moved) > (256 if k == 9 else 1024) and {kind for kind, _, _ in moved} == {"advice", "fixed", "instance"}
        for change in ((cycles - 3, 1), (1, 2), (5, 0)):
            _, bad, members = cases.copies_circuit(custom, k, cycles, change)
            assert len(members) >= 3
            report = cases.host_report(bad, k)
            assert len(report) == 1 and report[0][0] == cases.COPY and report[0][1] <= set(members)
            with pytest.raises(ValueError, match="copy constraint"):
                custom.mock(bad, k)


def test_flex_cases(flex):
    for name, (k, cs, good, bad) in cases.flex_cases(flex).items():
        flex.mock(good, k)
        assert cases.flex_host_report(good, k) == [], name
        report = cases.flex_host_report(bad, k)
        with pytest.raises(ValueError) as e:
            flex.mock(bad, k)
        assert str(e.value) == cases.first_violation(report, cs, flex_shape=True), name
        kind, index, row, _ = report[0]
        if name.startswith("limbs"):
            assert kind == cases.LOOKUP and len(report) == 1
            if name == "limbs_k11":
                assert row >= 3 * 256 and len(good.table_values) == 1024
        else:
            assert kind == cases.GATE and (index > 0) == (name == "range_multi")


# ---- the shape programs ------------------------------------------------------------------------------------------------------------------
def test_shape_gate_program(custom, flex, engine):
    """h2mi_shape_gate_program: evaluated on random queries it equals vertical_gate_ops for 1, 2, 7 and 32 gate columns and the
    StandardPlonk polynomial; H2MI_ERANGE (and the needed counts) when the buffers are short; H2MI_EINVAL for EXPRESSIONS"""
    rng = random.Random(8)
    q = lambda: (lambda table: (lambda op, c, r: table.setdefault((op, c, r), rng.randrange(R))))({})
    for n_gates in (1, 2, 7, 32):
        pairs = [(rng.randrange(64), rng.randrange(64)) for _ in range(n_gates)]
        abi = engine.ConstraintSystem.build(5, 64, 64, 0, 3, 5, engine.GATES_FLEX_VERTICAL, pairs, [], [], [], [])
        ops, consts = engine.shape_gate_program(abi)
        want_ops = gate_cases.vertical_gate_ops(pairs)
        query = q()
        assert gate_cases.run_postfix(ops, consts, query)[0] == gate_cases.run_postfix(want_ops, [], query)[0]
        assert len(gate_cases.run_postfix(ops, consts, query)[0]) == n_gates
        with pytest.raises(engine.H2miError) as e:
            engine.shape_gate_program(abi, ops_cap=len(ops) - 1)
        assert e.value.code == ERANGE
        assert engine.shape_gate_program(abi, ops_cap=len(ops))[0] == ops
    abi = gate_cases.standard_plonk_cs(custom).abi(5)
    abi.gates = engine.GATES_STANDARD_PLONK
    ops, consts = engine.shape_gate_program(abi)
    (poly,) = gate_cases.standard_plonk_cs(custom).polynomials
    for _ in range(4):
        query = q()
        kinds = {0: "advice", 1: "fixed", 2: "instance"}
        assert gate_cases.run_postfix(ops, consts, query)[0] == [poly.evaluate(lambda kind, c, r: query({v: key for key, v in kinds.items()}[kind], c, r))]
    n_ops, n_consts = C.c_uint32(), C.c_uint32()
    lib = engine.lib
    assert lib.h2mi_shape_gate_program(C.byref(abi), None, 0, C.byref(n_ops), None, 0, C.byref(n_consts)) == ERANGE and n_ops.value == len(ops)
    abi.gates = engine.GATES_EXPRESSIONS
    assert lib.h2mi_shape_gate_program(C.byref(abi), None, 0, C.byref(n_ops), None, 0, C.byref(n_consts)) == EINVAL
    assert lib.h2mi_shape_gate_program(None, None, 0, C.byref(n_ops), None, 0, C.byref(n_consts)) == EINVAL
    abi = flex.FlexGateCS(lookup=True).abi(7)
    assert engine.shape_gate_program(abi)[0] == gate_cases.vertical_gate_ops([(0, 3)])
