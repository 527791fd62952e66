"""The MSB / POW2 hints, the builders that go with them and the chip's exp, log and sin family on the host (no GPU): flex.hint and the
interpreter against the cases' restatement; h2mi_witness_check on kinds 13 and 14; num_to_bits, idx_to_indicator and select_from_idx
under flex.mock on one column and on several, every hint cell moved by one refused; every new chip method exactly against the integer
model of tests/transcendental_cases.py — an operand the model calls unsatisfiable refused —, and against floats within the bounds
derived there; the logistic closures recorded and replayed cell for cell."""
import ctypes as C
import math

import pytest

import fixed_point_cases as FC
import transcendental_cases as TC
import witness_cases as W

R = TC.R
EINVAL = -1
LOOKUP_BITS = 8


# ---- the hint function and the interpreter ---------------------------------------------------------------------------------------------------
def test_msb_and_pow2_hints_against_bit_length(h2):
    from halo2_scaffold_amd import flex

    assert (flex.MSB, flex.POW2, flex.HINT_OF_MSB) == (TC.MSB, TC.POW2, TC.POW2_OF_MSB) == (13, 14, 1)
    for x in TC.MSB_OPERANDS:
        assert flex.hint(flex.MSB, x) == TC.ref_msb(x) and flex.hint(flex.POW2, x, 0, flex.HINT_OF_MSB) == TC.ref_pow2(x, True) == 1 << TC.ref_msb(x), x
    for x in TC.POW2_OPERANDS:
        assert flex.hint(flex.POW2, x) == TC.ref_pow2(x) == (1 << x if x <= 253 else 0), x
    assert (flex.hint(flex.MSB, 0), flex.hint(flex.MSB, 1), flex.hint(flex.MSB, R - 1)) == (1, 0, 253)
    assert flex.hint(flex.POW2, 253) == 1 << 253 < R and flex.hint(flex.POW2, 254) == 0


def _rc(program):
    from halo2_scaffold_amd._lib import lib

    d = program.descriptor()
    return lib.h2mi_witness_check(C.byref(d))


def test_hand_built_tapes_are_what_they_are_named_for(h2):
    """the GPU tests' inputs: the interpreter agrees with the cases' own evaluation, every operand is reached from INPUT, CONST and GATE
    cells, and the launch shapes are those the GPU tests name"""
    from halo2_scaffold_amd import witness

    t, inputs, listed = TC.ops_tape()
    program = t.program(witness)
    want = t.evaluate(inputs)
    assert program.cells(inputs) == want and _rc(program) == 0
    assert all(want[cell] == value for cell, value in listed) and len(listed) == 2 * len(TC.MSB_OPERANDS) + len(TC.POW2_OPERANDS)
    by_op = {}
    for cell, _ in listed:
        kind, a, flags = t.cells[cell][:3]
        by_op.setdefault((kind, flags), set()).add(t.cells[a][0])
    assert by_op == {(TC.MSB, 0): {W.INPUT, W.CONST, W.GATE}, (TC.POW2, 1): {W.INPUT, W.CONST, W.GATE}, (TC.POW2, 0): {W.INPUT, W.CONST, W.GATE}}
    sizes = [40, 1025, 1024, 1]
    t, inputs = TC.layered_ops_tape(sizes)
    program = t.program(witness)
    assert program.level_sizes == sizes and W.segmentation(sizes) == (1, 2) and program.cells(inputs) == t.evaluate(inputs) and _rc(program) == 0
    assert program.cells(inputs) == t.program(witness, reverse=True).cells(inputs)
    t, inputs, cell, value = TC.msb_pow2_div_chain_tape(40, (1 << 100) + 5)
    program = t.program(witness)
    assert len(program.level_sizes) >= 41 and max(program.level_sizes) == 3 and W.segmentation(program.level_sizes) == (0, 1)
    got = program.cells(inputs)
    assert got[cell] == value == t.evaluate(inputs)[cell] and _rc(program) == 0
    assert len({got[i] for i, op in enumerate(t.cells) if op[0] == TC.DIVQ}) >= 4  # the quotients differ from round to round, zero among them
    kinds = [t.cells[i][0] for i in range(3, len(t.cells))]
    assert kinds[:6] == [TC.MSB, TC.POW2, TC.DIVQ] * 2


# ---- h2mi_witness_check ----------------------------------------------------------------------------------------------------------------------
def _good(witness):
    """cells: 0 an input; 1 a copy of it; 2 MSB of cell 1; 3 POW2 of cell 2; 4 flagged POW2 of cell 1; 5 ISZERO of cell 3"""
    t = TC.Tape()
    a = t.input(0)
    c = t.copy(a)
    m = t.msb(c)
    p = t.pow2(m)
    t.pow2(c, of_msb=True)
    t.hint(FC.ISZERO, p)
    return t.program(witness, placement=[[0, 1, 2], [3, 4, 5]])


def _with_op(witness, dst, **change):
    p = _good(witness)
    ops = p.ops.copy()
    (at,) = [i for i, row in enumerate(ops.tolist()) if row[0] == dst]
    row = dict(zip(("dst", "code", "a", "b"), ops[at].tolist()))
    row.update(change)
    ops[at] = [row["dst"], row["code"], row["a"], row["b"]]
    return witness.Program(ops, p.level_ends, p.constants, p.n_inputs, p.checks, p.placement, [])


def test_validator_takes_msb_and_pow2_and_refuses_what_they_must_not_hold(h2):
    from halo2_scaffold_amd import witness

    good = _good(witness)
    assert _rc(good) == 0 and good.level_sizes == [1, 1, 2, 1, 1]
    assert good.cells([1000]) == [1000, 1000, 9, 512, 512, 0]
    code = lambda kind, flags=0, shift=0: kind | flags << 8 | shift << 16
    assert _rc(_with_op(witness, 3, code=code(TC.POW2, 1))) == 0 and _rc(_with_op(witness, 4, code=code(TC.POW2, 0))) == 0  # with and without the flag
    assert _rc(_with_op(witness, 4, code=code(TC.MSB))) == 0 and _rc(_with_op(witness, 2, code=code(TC.POW2, 1))) == 0
    bad = {
        "a flag on MSB": _with_op(witness, 2, code=code(TC.MSB, 1)),
        "an unknown flag on POW2": _with_op(witness, 3, code=code(TC.POW2, 2)),
        "an unknown flag beside the known": _with_op(witness, 4, code=code(TC.POW2, 1 | 128)),
        "a shift on MSB": _with_op(witness, 2, code=code(TC.MSB, 0, 1)),
        "a shift on POW2": _with_op(witness, 3, code=code(TC.POW2, 0, 7)),
        "a shift on the flagged POW2": _with_op(witness, 4, code=code(TC.POW2, 1, 1)),
        "b on MSB": _with_op(witness, 2, b=1),
        "b on POW2": _with_op(witness, 3, b=1),
        "MSB of its own cell": _with_op(witness, 2, a=2),
        "MSB of a cell of its own level": _with_op(witness, 2, a=4),
        "POW2 of a higher level": _with_op(witness, 3, a=5),
        "POW2 of a cell of its own level": _with_op(witness, 4, a=2),
        "a outside the cells": _with_op(witness, 3, a=6),
        "kind 12": _with_op(witness, 2, code=12),
        "kind 12 with the flag": _with_op(witness, 4, code=code(12, 1)),
        "kind 15": _with_op(witness, 2, code=15),
        "kind 5": _with_op(witness, 2, code=5),
        "kind 255": _with_op(witness, 2, code=255),
        "the top byte": _with_op(witness, 3, code=code(TC.POW2) | 1 << 24),
    }
    for what, p in bad.items():
        assert _rc(p) == EINVAL, what


# ---- builders ------------------------------------------------------------------------------------------------------------------------------------
def _noting(flex):
    class Noting(flex.Context):
        """flex.Context that notes its hint cells: (cell, (kind, a, b, flags))"""

        def __init__(self, asg):
            super().__init__(asg)
            self.hint_rows = []

        def assign_region_last(self, items, gate_offsets):
            base = len(self.cells)
            self.hint_rows += [(base + i, v) for i, (kind, v) in enumerate(items) if kind == "hint"]
            return super().assign_region_last(items, gate_offsets)

    return Noting


def _synth(flex, body, cases, cs, lookup_bits):
    """load every operand of every case as a witness, run body(ctx, cells) per case -> (assignment, context, [results])"""
    asg = flex.Assignment(cs)
    ctx = _noting(flex)(asg)
    ctx.lookup_bits = lookup_bits
    out = [body(ctx, [ctx.load_witness(FC.to_field(v)) for v in case]) for case in cases]
    ctx.finish([])
    return flex.load_lookup_table(asg, lookup_bits), ctx, out


def _several_columns(flex, body, cases):
    """the smallest 2^k rows at which the cases fit the prover's columns and need at least two gate columns -> (constraint system, LOOKUP_BITS)"""
    for k in range(5, 16):
        lookup_bits = min(k - 1, 8)
        try:
            cs = flex.configure(True, k, lambda cs: _synth(flex, body, cases, cs, lookup_bits)[0])
            if cs.num_advice > 1:
                flex.mock(_synth(flex, body, cases, cs, lookup_bits)[0], k)
                return cs, lookup_bits
        except (AssertionError, ValueError):
            continue
    raise AssertionError("no 2^k rows lay these cases over several columns")


def _moved_hints_are_refused(flex, asg, ctx):
    moved = 0
    for row, (kind, a, _, _) in ctx.hint_rows:
        if kind == flex.INV and ctx.cells[a] == 0:
            continue  # 1 + 0 * inv = 1 for every inv: the inverse of zero is the one hint cell no constraint fixes
        asg.advice[0][row] = (asg.advice[0][row] + 1) % R
        with pytest.raises(ValueError):
            flex.mock(asg, 14)
        asg.advice[0][row] = ctx.cells[row]
        moved += 1
    flex.mock(asg, 14)
    return moved


def test_num_to_bits(h2):
    from halo2_scaffold_amd import flex

    cases = [(0, 1), (1, 1), (0b1011, 4), (0b1011, 7), ((1 << 64) - 1, 64), (1 << 63, 64), (0x123456789ABCDEF, 64), (R - 1, 254), (1 << 253, 254)]
    body = lambda bits: lambda c, v: c.num_to_bits(v[0], bits)
    for x, bits in cases:
        asg, ctx, (out,) = _synth(flex, body(bits), [(x,)], flex.FlexGateCS(True), LOOKUP_BITS)
        flex.mock(asg, 14)
        assert [ctx.cells[b] for b in out] == [(x >> i) & 1 for i in range(bits)] and len(ctx.cells) == 1 + 1 + 3 * (bits - 1) + 4 * bits
        assert len(set(out)) == bits and not ctx.lookup_cells
    for x, bits in ((2, 1), (16, 4), (1 << 64, 64), ((1 << 65) - 1, 64)):  # range_bits + 1 bits: the sum of the bits is not the value
        asg, _, _ = _synth(flex, body(bits), [(x,)], flex.FlexGateCS(True), LOOKUP_BITS)
        with pytest.raises(ValueError, match="copy constraint"):
            flex.mock(asg, 14)
    whole = lambda c, v: c.num_to_bits(v[0], 64)
    spread = [(x,) for x, bits in cases if bits == 64] * 3
    cs, lookup_bits = _several_columns(flex, whole, spread)
    asg, ctx, out = _synth(flex, whole, spread, cs, lookup_bits)
    assert cs.num_advice >= 2
    flex.mock(asg, cs.k)
    assert all([ctx.cells[b] for b in bits] == [(x >> i) & 1 for i in range(64)] for (x,), bits in zip(spread, out))


INDEX_CASES = [(0, 5), (4, 5), (5, 5), (77, 5), (0, 1), (1, 1), (2, 3), (R - 1, 4)]  # index 0, len - 1, out of range


def test_idx_to_indicator_and_select_from_idx(h2):
    from halo2_scaffold_amd import flex

    values = [11, R - 2, 0, 1 << 200, 7]
    for idx, length in INDEX_CASES:
        asg, ctx, (out,) = _synth(flex, lambda c, v: c.idx_to_indicator(v[0], length), [(idx,)], flex.FlexGateCS(True), LOOKUP_BITS)
        flex.mock(asg, 14)
        assert [ctx.cells[i] for i in out] == [int(idx == i) for i in range(length)], (idx, length)
        assert len(ctx.hint_rows) == 2 * length and _moved_hints_are_refused(flex, asg, ctx) == 2 * length - (1 if idx < length else 0)
        for operands in ("cells", "constants"):
            def select(c, v):
                pool = v[1:] if operands == "cells" else [flex.Constant(x) for x in values[:length]]
                return c.select_from_idx(pool, v[0])

            asg, ctx, (out,) = _synth(flex, select, [(idx,) + tuple(values[:length])], flex.FlexGateCS(True), LOOKUP_BITS)
            flex.mock(asg, 14)
            assert ctx.cells[out] == (values[idx] if idx < length else 0), (idx, length, operands)
            assert _moved_hints_are_refused(flex, asg, ctx) == 2 * length - (1 if idx < length else 0)
    select5 = lambda c, v: c.select_from_idx(v[1:], v[0])
    spread = [(idx,) + tuple(values) for idx, length in INDEX_CASES if length == 5] * 2
    cs, lookup_bits = _several_columns(flex, select5, spread)
    asg, ctx, out = _synth(flex, select5, spread, cs, lookup_bits)
    assert cs.num_advice >= 2
    flex.mock(asg, cs.k)
    assert [ctx.cells[c] for c in out] == [values[case[0]] if case[0] < 5 else 0 for case in spread]


def test_inner_product_and_pow_of_two(h2):
    from halo2_scaffold_amd import flex

    assert [int(c) for c in flex.Context.pow_of_two()] == [1 << i for i in range(254)]
    a, b = [3, R - 1, 1 << 100], [5, 7, R - 2]

    def both(c, v):
        plain = c.inner_product(v[:3], v[3:])
        first = len(c.cells)
        led = c.inner_product(v[:3], [flex.Constant(1), v[4], flex.Constant(b[2])])  # starts with the constant one: a0 is the first sum
        return plain, led, first

    asg, ctx, ((plain, led, first),) = _synth(flex, both, [tuple(a + b)], flex.FlexGateCS(True), LOOKUP_BITS)
    flex.mock(asg, 12)
    assert ctx.cells[plain] == sum(x * y for x, y in zip(a, b)) % R and plain == 6 + 9
    assert ctx.cells[led] == (a[0] + a[1] * b[1] + a[2] * b[2]) % R and led == first + 6


# ---- chip methods, exactly ----------------------------------------------------------------------------------------------------------------------
def _method(flex, P, name, operands, lookup_bits=LOOKUP_BITS):
    """the method on signed integers on one column -> (assignment, context, result cell); whatever synthesis raises"""
    from halo2_scaffold_amd.fixed_point import FixedPointChip

    chip = FixedPointChip(P)
    return _synth(flex, lambda c, v: getattr(chip, name)(c, *v), [operands], flex.FlexGateCS(True), lookup_bits)


def _expect(flex, P, name, operands, k=18):
    """the model's value, exactly, on a satisfied circuit — or, for an operand the model calls unsatisfiable, a refusal at synthesis"""
    model = TC.Model(P)
    try:
        want = getattr(model, name)(*operands)
    except TC.Unsat:
        with pytest.raises((ValueError, AssertionError)) as e:
            asg, _, _ = _method(flex, P, name, operands)
            flex.mock(asg, k)
        assert isinstance(e.value, ValueError) or "witness out of range" in str(e.value), (name, operands)
        return None
    asg, ctx, (out,) = _method(flex, P, name, operands)
    assert ctx.cells[out] == FC.to_field(want), (name, P, operands, FC.to_signed(ctx.cells[out]), want)
    return asg


@pytest.mark.parametrize("name", ["qexp2", "qlog2", "qsin", "qcos", "qtan", "qexp", "qsinh", "qcosh", "qtanh", "qlog", "qpow", "qsqrt"])
def test_methods_on_edge_operands_are_the_integer_model_exactly(h2, name):
    """P = 32.  Every case alone on one column; the circuit of the first and the last satisfiable case is put to flex.mock (the whole
    list's cells are those two's, with other values)"""
    from halo2_scaffold_amd import flex

    cases = TC.edge_operands(32)[name]
    satisfied = [asg for asg in (_expect(flex, 32, name, case) for case in cases) if asg is not None]
    assert len(satisfied) >= 3 and len(satisfied) <= len(cases)
    if name in ("qexp2", "qlog2", "qexp", "qlog", "qpow"):
        assert len(satisfied) < len(cases)  # the list holds operands that must be refused
    for asg in (satisfied[0], satisfied[-1]):
        flex.mock(asg, 18)


def test_qexp2_is_refused_from_the_first_integer_part_without_a_reciprocal(h2):
    """2^|a| is divided into one for either sign, so it must stay below is_neg's threshold 2^(2P+1): integer part P is the last that does"""
    model = TC.Model(32)
    assert model.qexp2(32 << 32) == 1 << 64 and model.qexp2(-(32 << 32)) == 1
    for a in (33 << 32, -(33 << 32), 62 << 32, 254 << 32):
        with pytest.raises(TC.Unsat):
            model.qexp2(a)


@pytest.mark.parametrize("name", ["qexp", "qlog"])
def test_qexp_and_qlog_at_63_bits_are_the_integer_model_exactly(h2, name):
    from halo2_scaffold_amd import flex

    model = TC.Model(63)
    asgs = [_expect(flex, 63, name, (model.q(x),)) for x in TC.P63_OPERANDS[name]]
    assert all(asg is not None for asg in asgs)
    flex.mock(asgs[-1], 18)
    for name32, case in (("qexp2", (1 << 63,)), ("qlog2", ((1 << 125) - 1,)), ("qlog2", (1 << 125,)), ("qlog2", (0,)), ("qexp2", (-(64 << 63),))):
        _expect(flex, 63, name32, case)


def test_coefficients_are_the_model_s_roundings(h2):
    from halo2_scaffold_amd.fixed_point import FixedPointChip

    for P in (32, 48, 63):
        chip, model = FixedPointChip(P), TC.Model(P)
        for generate, coef in ((chip.generate_exp2_poly, TC.EXP2_COEF), (chip.generate_log_poly, TC.LOG_COEF), (chip.generate_sin_poly, TC.SIN_COEF)):
            got = generate()
            assert [int(c) for c in got] == [FC.to_field(model.q(c)) for c in coef] and len(got) == len(coef)


# ---- chip methods against floats ---------------------------------------------------------------------------------------------------------------
def _against_floats(flex, P, cases, capsys):
    from halo2_scaffold_amd.fixed_point import FixedPointChip

    chip, model = FixedPointChip(P), TC.Model(P)
    worst = {}
    for name, (bound, reals) in cases.items():
        for x in reals:
            a = model.q(x)
            _, ctx, (out,) = _method(flex, P, name, (a,))
            got = model.real(FC.to_signed(ctx.cells[out]))
            want, err = bound(P, model.real(a))  # at the quantised operand: what the circuit was given
            figure = (name, x, got, want, abs(got - want), err)
            assert abs(got - want) <= err, figure
            if abs(got - want) / err >= worst.get(name, (0.0,))[0]:
                worst[name] = (abs(got - want) / err, x, abs(got - want), err)
    with capsys.disabled():
        print(f"\nP = {P}: largest error as a share of its bound, (share, x, error, bound):", {k: tuple(float(f"{v:.3g}") for v in w) for k, w in worst.items()})


def test_accuracy_against_floats_at_32_bits(h2, capsys):
    from halo2_scaffold_amd import flex

    _against_floats(flex, 32, TC.FLOAT_CASES, capsys)


def test_accuracy_of_qexp_and_qlog_against_floats_at_63_bits(h2, capsys):
    from halo2_scaffold_amd import flex

    _against_floats(flex, 63, TC.FLOAT_CASES_63, capsys)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_unsatisfiable_operands_are_refused_at_synthesis_and_by_the_program(h2):
    from halo2_scaffold_amd import flex, witness
    from halo2_scaffold_amd.fixed_point import FixedPointChip

    chip = FixedPointChip(32)
    one = 1 << 32
    for name, bad, good in (("qlog2", [0, -one], one), ("qlog", [0, -1], one), ("qexp2", [254 * one, -254 * one, 33 * one], 0)):
        def f(ctx, inputs, make_public):
            make_public.append(getattr(chip, name)(ctx, ctx.load_witness(inputs[0])))

        for a in bad:
            with pytest.raises((ValueError, AssertionError)) as e:
                _method(flex, 32, name, (a,))
            assert isinstance(e.value, ValueError) or "witness out of range" in str(e.value), (name, a)
        program, _ = witness.Program.record(f, [good], flex.FlexGateCS(True), LOOKUP_BITS)
        assert program.cells([good])[program.public[0]] == FC.to_field(getattr(TC.Model(32), name)(good))
        for a in bad:
            with pytest.raises(ValueError, match="witness out of range"):
                program.cells([FC.to_field(a)])
    # a shift beyond the table: an operand whose highest bit leaves check_power_of_two's 2P bits
    with pytest.raises(ValueError, match="witness out of range"):
        program_log = witness.Program.record(lambda c, v, p: p.append(chip.qlog2(c, c.load_witness(v[0]))), [one], flex.FlexGateCS(True), LOOKUP_BITS)[0]
        program_log.cells([1 << 63])


# ---- recording -----------------------------------------------------------------------------------------------------------------------------------
def _host(f, inputs, cs, lookup_bits):
    from halo2_scaffold_amd import flex

    asg = flex.Assignment(cs)
    ctx = flex.Context(asg)
    ctx.lookup_bits = lookup_bits
    public = []
    f(ctx, inputs, public)
    ctx.finish(public)
    return flex.load_lookup_table(asg, lookup_bits), ctx.cells, public


def _circuits():
    """(closure, dummy, input sets, reference, DEGREE, LOOKUP_BITS) of the proofs of tests/test_gpu_transcendental.py"""
    from halo2_scaffold_amd import logistic_regression as LG
    from halo2_scaffold_amd.fixed_point import FixedPointChip

    return [(LG.inference, TC.INFERENCE_DUMMY, TC.INFERENCE_INPUTS, TC.ref_inference, 9, 8), (LG.train, TC.TRAIN_DUMMY, TC.TRAIN_INPUTS, TC.ref_train, 10, 9),
            (mixed_closure(FixedPointChip(32)), TC.MIXED_DUMMY, TC.MIXED_INPUTS, TC.ref_mixed, 11, 10)]


def mixed_closure(chip):
    def mixed(ctx, inputs, make_public):
        a, b, c = (ctx.load_witness(v) for v in inputs)
        make_public.append(chip.qlog(ctx, a))
        make_public.append(chip.qsin(ctx, b))
        make_public.append(chip.qpow(ctx, a, c))

    return mixed


def test_the_closures_record_and_replay_cell_for_cell(h2):
    from halo2_scaffold_amd import flex, witness

    for f, dummy, input_sets, reference, k, lookup_bits in _circuits():
        cs = flex.configure(True, k, lambda cs: _host(f, TC.field_inputs(dummy), cs, lookup_bits)[0])
        assert cs.num_advice >= 2 and cs.num_lookup_advice >= 2
        program, recorded = witness.Program.record(f, TC.field_inputs(dummy), cs, lookup_bits)
        plain, cells, public = _host(f, TC.field_inputs(dummy), cs, lookup_bits)
        assert recorded.advice == plain.advice and recorded.fixed == plain.fixed and recorded.copies == plain.copies and recorded.instance == plain.instance
        assert program.cells(TC.field_inputs(dummy)) == cells and program.public == public
        program.descriptor().check()
        kinds = {int(code) & 0xFF for code in program.ops[:, 1]}
        assert ({TC.MSB, TC.POW2} <= kinds) == (reference is TC.ref_mixed) and not ({TC.MSB, TC.POW2} & kinds) == (reference is not TC.ref_mixed)
        for inputs in input_sets:  # other inputs than the dummies
            fresh, cells, _ = _host(f, TC.field_inputs(inputs), cs, lookup_bits)
            got = program.cells(TC.field_inputs(inputs))
            assert got == cells
            assert program.break_points == list(fresh.break_points) == list(recorded.break_points)
            for j, column in enumerate(program.columns(got)):
                assert dict(enumerate(column)) == fresh.advice[j]
            assert [got[c] for c in program.public] == fresh.instance == [TC.to_field(v) for v in reference(*inputs)]
        flex.mock(fresh, k)


def test_msb_and_pow2_ops_appear_only_where_qlog2_is_used(h2):
    from halo2_scaffold_amd import flex, witness
    from halo2_scaffold_amd.fixed_point import FixedPointChip

    chip = FixedPointChip(32)
    count = lambda program, kind, flags=None: sum(1 for code in program.ops[:, 1].tolist() if code & 0xFF == kind and (flags is None or (code >> 8) & 0xFF == flags))
    closures = {"qlog": lambda c, v, p: p.append(chip.qlog(c, c.load_witness(v[0]))), "qexp": lambda c, v, p: p.append(chip.qexp(c, c.load_witness(v[0]))),
                "qsin": lambda c, v, p: p.append(chip.qsin(c, c.load_witness(v[0])))}
    for name, f in closures.items():
        program, _ = witness.Program.record(f, [1 << 32], flex.FlexGateCS(True), LOOKUP_BITS)
        want = (1, 1, 1) if name == "qlog" else (0, 0, 0)  # exp1, pow1 (flagged) and shift_pow2
        assert (count(program, TC.MSB), count(program, TC.POW2, 1), count(program, TC.POW2, 0)) == want, name
        assert all(len(row) == 4 for row in program.ops.tolist())
    # a hint of constants only is a CONST op with no fixed cell beside it: qsin's is_neg(Constant(2 pi)) adds no constant cell
    ctx = flex.Context(flex.Assignment(flex.FlexGateCS(True)))
    ctx.lookup_bits = LOOKUP_BITS
    before = len(ctx.const_cells)
    base = len(ctx.cells)
    ctx.div_mod(flex.Constant(12345), 100, 64)
    assert ctx.cells[base:base + 4] == [45, 100, 123, 12345] and [c for c in ctx.const_cells[before:] if c[0] in (base, base + 2)] == []
