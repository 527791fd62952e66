"""Gates given as data, the host side (no GPU): h2mi_gate_program_check (include/h2mi_prover.h) on the programs of the reference's
circuits and on every malformed program it must refuse, custom.Expression.program() — the postfix compiler — against direct
evaluation of random trees, and custom.ConstraintSystem's bookkeeping (query order, permutation columns, degree, blinding factors)
on the reference's configure() functions transcribed call for call."""
import random

import pytest

import custom_gate_cases as cases
from custom_gate_cases import OP_ADD, OP_ADVICE, OP_CONSTANT, OP_END, OP_FIXED, OP_INSTANCE, OP_MUL, OP_SUB
from oracle import flex as FX

R = cases.R
EINVAL = -1


@pytest.fixture(scope="module")
def custom(h2):
    from halo2_scaffold_amd import custom

    return custom


@pytest.fixture(scope="module")
def engine(h2):
    from halo2_scaffold_amd import engine

    return engine


def _code(engine, cs, ops, constants=()):
    try:
        return engine.GateProgram.build(ops, list(constants)).check(cs)
    except engine.H2miError as e:
        return e.code


def test_program_check_accepts_the_reference_circuits(custom, engine):
    """StandardPlonk, the vertical gate, is_zero and or: accepted, degree 3, with the stack the compiler promises"""
    k = 5
    for cs in (cases.standard_plonk_cs(custom), cases.is_zero_circuit(custom, 5)[0], cases.or_circuit(custom, 1, 1)[0]):
        abi = cs.abi(k)
        assert abi.gates == engine.GATES_EXPRESSIONS == 3
        degree, depth = cs.gate_program().check(abi)
        assert degree == 3 == cs.degree()
        assert depth == max(p.stack_depth() for p in cs.polynomials) <= 3
    from halo2_scaffold_amd import flex

    for fcs in (flex.FlexGateCS(lookup=False), flex.FlexGateCS(lookup=True), flex.FlexGateCS(True, 3, 1, k=5)):
        abi = fcs.abi(k)
        abi.gates = engine.GATES_EXPRESSIONS
        assert _code(engine, abi, cases.vertical_gate_ops(list(enumerate(fcs.col_qs)))) == (3, 2)


def test_program_check_refuses_malformed_programs(custom, engine):
    cs = cases.is_zero_circuit(custom, 0)[0].abi(5)  # advice x, y, out queried at 0; fixed 0 (the selector) at 0; degree 3; no instance
    A = lambda c, r=0: (OP_ADVICE, c, r)
    ADD, MUL, END = (OP_ADD, 0, 0), (OP_MUL, 0, 0), (OP_END, 0, 0)
    assert _code(engine, cs, [A(0), A(1), MUL, END]) == (2, 2)
    bad = {
        "stack underflow": [A(0), ADD, END],
        "depth 9": [A(0)] * 9 + [ADD] * 8 + [END],
        "two values at END": [A(0), A(1), END],
        "nothing at END": [A(0), END, END],
        "no final END": [A(0), END, A(1)],
        "advice column out of range": [A(3), END],
        "fixed column out of range": [(OP_FIXED, 1, 0), END],
        "instance column out of range": [(OP_INSTANCE, 0, 0), END],
        "constant out of range": [(OP_CONSTANT, 1, 0), END],
        "query not in the query list": [A(0, 1), END],
        "rotation of 2^k": [A(0, 32), END],
        "degree cs.degree + 1": [A(0), A(1), MUL, A(2), MUL, (OP_FIXED, 0, 0), MUL, END],
        "unknown op": [A(0), (9, 0, 0), END],
        "empty": [],
    }
    for what, ops in bad.items():
        assert _code(engine, cs, ops, constants=[7]) == EINVAL, what
    assert _code(engine, cs, [A(0)] * 8 + [ADD] * 7 + [END]) == (1, 8)  # depth 8 is the limit, not beyond it
    assert _code(engine, cs, [A(0), A(1), MUL, (OP_FIXED, 0, 0), MUL, END]) == (3, 2)  # degree cs.degree itself
    assert _code(engine, cs, [(OP_CONSTANT, 0, 0), A(2), (OP_SUB, 0, 0), END], constants=[7]) == (1, 2)
    too_long = [A(0), END] * 2049  # H2MI_MAX_EXPR_OPS + 2
    assert _code(engine, cs, too_long) == EINVAL
    assert engine.lib.h2mi_gate_program_check(None, None, None, None) == EINVAL


@pytest.mark.parametrize("seed", range(12))
def test_compiler_matches_direct_evaluation(custom, engine, seed):
    """random trees over advice / fixed / instance queries at rotations -3 .. 3 and constants: the emitted postfix, run by the stack
    machine of cases.run_postfix on random field values, gives the tree's value; degree and stack depth as the tree has them, and
    as h2mi_gate_program_check reports them"""
    rng = random.Random(1000 + seed)
    rots = list(range(-3, 4))
    columns = [(custom.ADVICE, 0, rots), (custom.ADVICE, 1, rots), (custom.FIXED, 0, rots), (custom.INSTANCE, 0, rots)]
    kinds = {OP_ADVICE: custom.ADVICE, OP_FIXED: custom.FIXED, OP_INSTANCE: custom.INSTANCE}
    tree = cases.random_tree(custom, rng, depth=2 + seed % 5, columns=columns, leaf_bias=0.15)
    values = {}
    q = lambda kind, c, r: values.setdefault((kind, c, r), rng.randrange(R))
    ops, constants = tree.program()
    got, deepest = cases.run_postfix(ops, constants, lambda op, c, r: q(kinds[op], c, r))
    assert got == [tree.evaluate(q)]
    assert deepest == tree.stack_depth() == cases.tree_stack_depth(tree)
    assert ops[-1][0] == OP_END and sum(1 for o in ops if o[0] == OP_END) == 1
    if deepest <= engine.MAX_EXPR_STACK and tree.degree() <= 9:
        queries = [(c, r) for c in range(2) for r in rots]
        cs = engine.ConstraintSystem.build(6, 2, 1, 1, 9, 9, engine.GATES_EXPRESSIONS, [], [], [], queries, [(0, r) for r in rots])
        assert engine.GateProgram.build(ops, constants).check(cs) == (tree.degree(), deepest)


def test_compiler_orders_operands_deeper_first(custom):
    """a right-leaning sum a + (b + (c + d * e)) needs five slots in source order and two with the deeper operand first"""
    qs = [custom.Expression("query", custom.ADVICE, i, 0) for i in range(5)]
    e = qs[0] + (qs[1] + (qs[2] + qs[3] * qs[4]))
    assert e.stack_depth() == 2
    ops, _ = e.program()
    assert cases.run_postfix(ops, [], lambda op, c, r: c + 2) == ([2 + 3 + 4 + 5 * 6], 2)


def test_transcriptions_have_halo2s_bookkeeping(custom):
    sp, osp = cases.standard_plonk_cs(custom), FX.standard_plonk_cs()
    assert (sp.n_advice, sp.n_fixed, sp.n_instance) == (osp.n_advice, osp.n_fixed, osp.n_instance) == (3, 5, 0)
    assert sp.perm_columns == osp.perm_columns
    assert sp.advice_queries == osp.advice_queries and sp.fixed_queries == osp.fixed_queries
    assert (sp.degree(), sp.blinding_factors()) == (osp.degree, osp.blinding_factors) == (3, 5)
    rng = random.Random(7)
    vals = {}
    q = lambda kind, c, r: vals.setdefault((kind, c, r), rng.randrange(R))
    assert [g(q) for g in sp.gates] == [g(q) for g in osp.gates]
    iz, asg = cases.is_zero_circuit(custom, 0)
    X, Y, OUT = 0, 1, 2
    assert iz.advice_queries == [(X, 0), (OUT, 0), (Y, 0)]  # enable_equality(x), (out) query first; the gate adds y
    assert iz.n_fixed == 1 and iz.fixed_queries == [(0, 0)]
    assert iz.perm_columns == [(custom.ADVICE, X), (custom.ADVICE, OUT)]
    assert (iz.degree(), iz.blinding_factors()) == (3, 5)
    assert len(iz.polynomials) == 2
    assert asg.advice == [{0: 0, 1: 1}, {0: 1}, {0: 1}] and asg.fixed == [{0: 1}]
    assert asg.copies == [((custom.ADVICE, OUT, 0), (custom.ADVICE, X, 1))]
    orc, oasg = cases.or_circuit(custom, 0, 1)
    assert orc.advice_queries == [(0, 0), (0, 1), (0, 2)] and orc.blinding_factors() == 5 and orc.degree() == 3
    assert oasg.advice == [{0: 0, 1: 1, 2: 1}]
    d6, _ = cases.degree6_circuit(custom, 3, 11)
    assert d6.degree() == 6 and d6.blinding_factors() == 5 and d6.n_fixed == 3
    assert d6.advice_queries == [(0, 0), (0, -1)] and d6.fixed_queries == [(0, 0), (1, 0), (2, 0)] and d6.instance_queries == [(0, 0)]


def test_mock_accepts_good_witnesses_and_names_broken_ones(custom):
    for x in (0, 5, R - 1):
        custom.mock(cases.is_zero_circuit(custom, x)[1], 5)
    for a, b in ((1, 1), (0, 1), (0, 0)):
        custom.mock(cases.or_circuit(custom, a, b)[1], 5)
    custom.mock(cases.degree6_circuit(custom, 3, 11)[1], 4)
    with pytest.raises(ValueError, match="ISZERO gate"):
        custom.mock(cases.is_zero_circuit(custom, 5, flip_out=True)[1], 5)
    with pytest.raises(ValueError, match="OR gate"):
        custom.mock(cases.or_circuit(custom, 0, 1, flip_out=True)[1], 5)
    _, asg = cases.degree6_circuit(custom, 3, 11)
    asg.instance[-1] += 1
    with pytest.raises(ValueError, match="public output"):
        custom.mock(asg, 4)
    _, asg = cases.is_zero_circuit(custom, 0)
    asg.advice[0][1] = 0  # the copy of `out`
    with pytest.raises(ValueError, match="copy constraint"):
        custom.mock(asg, 5)
    with pytest.raises(ValueError, match="NotEnoughRowsAvailable"):
        custom.mock(cases.degree6_circuit(custom, 3, 11, steps=12)[1], 4)
