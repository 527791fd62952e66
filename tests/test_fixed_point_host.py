"""The fixed-point chip, the builders' new instructions and the hint ops on the host (no GPU): flex.hint against divmod references; every
new instruction and chip method on edge operands — flex.mock satisfied on one column and on several, the value against signed-integer
references, mock raising for every hint cell moved by one —; the recorder on the regression closures; h2mi_witness_check on the new
kinds; and the chip's accuracy against float arithmetic within a bound derived from the roundings it makes."""
import ctypes as C

import pytest

import fixed_point_cases as FC
import witness_cases as W

R = FC.R
P, ONE = FC.P, FC.ONE
EINVAL = -1
LOOKUP_BITS = 8  # of the one-column runs, at 2^12 rows


# ---- the hint function ----------------------------------------------------------------------------------------------------------------------
def test_division_hints_against_divmod(h2):
    from halo2_scaffold_amd import flex

    assert (flex.DIVQ, flex.DIVR, flex.ISZERO, flex.INV, flex.HINT_CONST, flex.HINT_SIGNED) == (8, 9, 10, 11, 1, 2)
    pairs = FC.div_pairs()
    assert len(pairs) >= len(FC.DIVIDENDS) * (len(FC.DIVISORS) + 1)
    for x, y in pairs:
        q, rem = divmod(x, y) if y else (0, 0)
        for const in (0, flex.HINT_CONST):  # both divisor forms: the flag says where y comes from, not what is computed
            assert (flex.hint(flex.DIVQ, x, y, const), flex.hint(flex.DIVR, x, y, const)) == (q, rem), (x, y)
            sq, srem = flex.hint(flex.DIVQ, x, y, const | flex.HINT_SIGNED), flex.hint(flex.DIVR, x, y, const | flex.HINT_SIGNED)
            assert (sq, srem) == FC.ref_div(x, y, True), (x, y)
            if y:  # x~ = y q + rem with 0 <= rem < y, q rounded toward minus infinity
                assert 0 <= srem < y and (y * FC.to_signed(sq) + srem) == (x - R if x > FC.HALF else x)
    # on both sides of 2^252
    assert flex.hint(flex.DIVQ, FC.HALF, 2, flex.HINT_SIGNED) == FC.HALF // 2 and flex.hint(flex.DIVQ, FC.HALF + 1, 2, flex.HINT_SIGNED) == R - (R - FC.HALF - 1 + 1) // 2
    # exact negative multiples: no rounding step, remainder 0
    for x, y in FC.EXACT_NEGATIVE:
        assert (R - x) % y == 0
        assert flex.hint(flex.DIVR, x, y, flex.HINT_SIGNED) == 0 and flex.hint(flex.DIVQ, x, y, flex.HINT_SIGNED) == R - (R - x) // y
        assert flex.hint(flex.DIVQ, x - 1, y, flex.HINT_SIGNED) == R - (R - x) // y - 1 and flex.hint(flex.DIVR, x - 1, y, flex.HINT_SIGNED) == y - 1


def test_iszero_and_inverse_hints(h2):
    from halo2_scaffold_amd import flex

    for x in FC.UNARY:
        assert flex.hint(flex.ISZERO, x) == FC.ref_hint(FC.ISZERO, x) == int(x == 0)
        inv = flex.hint(flex.INV, x)
        assert inv == FC.ref_hint(FC.INV, x) and (inv * x % R == 1 if x else inv == 1)


# ---- instructions and methods on edge operands ---------------------------------------------------------------------------------------------
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
    """load every operand of every case as a witness, run body(ctx, cells) per case -> (assignment, context, [result cells])"""
    asg = flex.Assignment(cs)
    ctx = _noting(flex)(asg)
    ctx.lookup_bits = lookup_bits
    out = []
    for case in cases:
        out.append(body(ctx, [ctx.load_witness(FC.to_field(v)) for v in case]))
    ctx.finish([c for c in out if c is not None])
    return flex.load_lookup_table(asg, lookup_bits), ctx, out


def _several_columns(flex, body, cases):
    """the smallest 2^k rows (LOOKUP_BITS k - 1, at most 8) at which all the cases together fit the prover's 32 gate and 8 lookup-advice
    columns -> (constraint system, LOOKUP_BITS)"""
    for k in range(5, 16):
        lookup_bits = min(k - 1, 8)
        try:
            cs = flex.configure(True, k, lambda cs: _synth(flex, body, cases, cs, lookup_bits)[0])
            if cs.num_advice > 1:
                flex.mock(_synth(flex, body, cases, cs, lookup_bits)[0], k)
                return cs, lookup_bits
        except (AssertionError, ValueError):  # more columns than the prover's ABI takes or than configure counted (the break duplicates),
            continue                          # or constants and copies beyond the usable rows
    return None, None


def _exercise(h2, body, cases, reference):
    """every case alone on one column: mock satisfied, the value, mock raising for every hint cell moved by one; all cases together on
    several columns: mock satisfied, the values"""
    from halo2_scaffold_amd import flex

    for case in cases:
        asg, ctx, (out,) = _synth(flex, body, [case], flex.FlexGateCS(True), LOOKUP_BITS)
        flex.mock(asg, 12)
        want = reference(*case)
        if want is not None:
            assert ctx.cells[out] == FC.to_field(want), case
        for row, (kind, a, _, _) in ctx.hint_rows:
            if kind == flex.INV and ctx.cells[a] == 0:
                continue  # 1 + 0 * inv = 1 for every inv: the inverse of zero is the one hint cell no constraint fixes
            asg.advice[0][row] = (asg.advice[0][row] + 1) % R
            with pytest.raises(ValueError):
                flex.mock(asg, 12)
            asg.advice[0][row] = ctx.cells[row]
        flex.mock(asg, 12)
    cs, lookup_bits = _several_columns(flex, body, cases)
    while cs is None and len(cases) < 256:  # too few cells for a second column: the cases over again
        cases = cases * 2
        cs, lookup_bits = _several_columns(flex, body, cases)
    asg, ctx, out = _synth(flex, body, cases, cs, lookup_bits)
    assert cs.num_advice >= 2 and len(asg.break_points) == cs.num_advice - 1
    flex.mock(asg, cs.k)
    for case, cell in zip(cases, out):
        want = reference(*case)
        if want is not None:
            assert ctx.cells[cell] == FC.to_field(want), case


FIELD_EDGE = [0, 1, 2, R - 1, R - 2, ONE, R - ONE, (1 << 253) + 5]
FIELD_PAIRS = [(a, b) for i, a in enumerate(FIELD_EDGE) for j, b in enumerate(FIELD_EDGE) if i == j or (a + b) % R == 0 or (i + j) % 3 == 0]
BITS = [(0, 0), (0, 1), (1, 0), (1, 1)]


def _gate_instructions(flex):
    Const = flex.Constant
    return {
        "sub": (lambda c, v: c.sub(v[0], v[1]), FIELD_PAIRS, lambda a, b: a - b),
        "sub of a constant": (lambda c, v: c.sub(v[0], Const(7)), [(a,) for a in FIELD_EDGE], lambda a: a - 7),
        "neg": (lambda c, v: c.neg(v[0]), [(a,) for a in FIELD_EDGE], lambda a: -a),
        "mul_add": (lambda c, v: c.mul_add(v[0], v[1], v[2]), [(a, b, a ^ 5) for a, b in FIELD_PAIRS], lambda a, b, d: a * b + d),
        "mul_add with constants": (lambda c, v: c.mul_add(v[0], Const(R - 1), Const(3)), [(a,) for a in FIELD_EDGE], lambda a: 3 - a),
        "select": (lambda c, v: c.select(v[0], v[1], v[2]), [(a, b, s) for a, b in FIELD_PAIRS for s in (0, 1)], lambda a, b, s: a if s else b),
        "select of constants": (lambda c, v: c.select(Const(R - 1), Const(1), v[0]), [(0,), (1,)], lambda s: R - 1 if s else 1),
        "not_": (lambda c, v: c.not_(v[0]), [(0,), (1,)], lambda a: 1 - a),
        "and_": (lambda c, v: c.and_(v[0], v[1]), BITS, lambda a, b: a & b),
        "or_": (lambda c, v: c.or_(v[0], v[1]), BITS, lambda a, b: a | b),
        "is_zero": (lambda c, v: c.is_zero(v[0]), [(a,) for a in FIELD_EDGE], lambda a: int(a == 0)),
        "is_equal": (lambda c, v: c.is_equal(v[0], v[1]), FIELD_PAIRS, lambda a, b: int(a == b)),
        "assert_bit": (lambda c, v: c.assert_bit(v[0]), [(0,), (1,)], lambda a: None),
        "assert_is_const": (lambda c, v: c.assert_is_const(v[0], R - 3), [(R - 3,)], lambda a: None),
        "sum": (lambda c, v: c.sum(v), [(5,), (R - 1, 1), (R - 1, R - 1, 2, ONE), tuple(FIELD_EDGE)], lambda *a: sum(a)),
        # the three that take no operand, each added to one so that the cases fill columns (load_zero is one cell however often it is called)
        "sum of nothing": (lambda c, v: c.add(c.sum([]), v[0]), [(5,), (R - 1,)], lambda a: a),
        "load_constant": (lambda c, v: c.add(c.load_constant(R - 9), v[0]), [(5,), (9,)], lambda a: a - 9),
        "load_zero": (lambda c, v: c.add((c.load_zero(), c.load_zero())[1], v[0]), [(5,), (R - 1,)], lambda a: a),
    }


def _range_instructions(flex):
    top = (1 << 64) - 1
    less = [(0, 1), (0, top), (top - 1, top), (ONE - 1, ONE), (5, 6)]
    order = less + [(b, a) for a, b in less] + [(0, 0), (top, top), (ONE, ONE)]
    dividends = [0, 1, ONE - 1, ONE, (1 << 64) - 1, 1 << 64, (1 << 100) - 1]
    return {
        "check_less_than": (lambda c, v: c.check_less_than(v[0], v[1], 64), less, lambda a, b: None),
        "check_big_less_than_safe": (lambda c, v: c.check_big_less_than_safe(v[0], (1 << 96) + 1), [(0,), (1 << 96,), (ONE,)], lambda a: None),
        "is_less_than": (lambda c, v: c.is_less_than(v[0], v[1], 64), order, lambda a, b: int(a < b)),
        "div_mod quotient": (lambda c, v: c.div_mod(v[0], 1 << 33, 100)[0], [(a,) for a in dividends], lambda a: a >> 33),
        "div_mod remainder": (lambda c, v: c.div_mod(v[0], 7, 100)[1], [(a,) for a in dividends], lambda a: a % 7),
        "div_mod_var quotient": (lambda c, v: c.div_mod_var(v[0], v[1], 100, 64)[0], [(a, b) for a in dividends for b in (1, 3, ONE, top)], lambda a, b: a // b),
        "div_mod_var remainder": (lambda c, v: c.div_mod_var(v[0], v[1], 100, 64)[1], [(a, a + 1) for a in dividends[:6]] + [(a, a) for a in dividends[1:6]], lambda a, b: a % b),
    }


def _chip_methods(flex):
    from halo2_scaffold_amd.fixed_point import FixedPointChip

    chip = FixedPointChip(P)
    unary = [(a,) for a in FC.EDGE]
    nonzero = lambda pairs: [(a, b) for a, b in pairs if b != 0]
    m = lambda name: (lambda c, v: getattr(chip, name)(c, *v))
    coef = [FC.q(0.5), -FC.q(1.5), FC.q(2.25), -1]
    return {
        "qadd": (m("qadd"), FC.PAIRS, FC.REF["qadd"]),
        "qsub": (m("qsub"), FC.PAIRS, FC.REF["qsub"]),
        "neg": (m("neg"), unary, FC.REF["neg"]),
        "qsum": (lambda c, v: chip.qsum(c, v), [tuple(FC.EDGE), (FC.BIG, -FC.BIG), (-1,)], lambda *a: sum(a)),
        "qabs": (m("qabs"), unary, FC.REF["qabs"]),
        "is_neg": (m("is_neg"), unary, FC.REF["is_neg"]),
        "sign": (m("sign"), unary, FC.REF["sign"]),
        "cond_neg": (m("cond_neg"), [(a, s) for a in FC.EDGE for s in (0, 1)], lambda a, s: -a if s else a),
        "clip": (m("clip"), unary + [((1 << 64) + 5,), (-(1 << 64) - 5,), (-(1 << 100),)], FC.REF["clip"]),
        "signed_div_scale quotient": (lambda c, v: chip.signed_div_scale(c, v[0])[0], unary + [(-ONE - 1,), (-(1 << 127),), ((1 << 96) - 1,)], lambda a: a >> P),
        "signed_div_scale remainder": (lambda c, v: chip.signed_div_scale(c, v[0])[1], unary + [(-ONE - 1,), (-3 * ONE,)], lambda a: a % ONE),
        "qmul": (m("qmul"), FC.PAIRS + FC.QMUL_EXTREME, FC.REF["qmul"]),
        "qdiv": (m("qdiv"), nonzero(FC.PAIRS) + FC.QDIV_EXTREME, FC.REF["qdiv"]),
        "qmod": (m("qmod"), [(a, b) for a, b in FC.PAIRS if b > 0] + FC.QMOD_EXTREME, FC.REF["qmod"]),
        "bit_xor": (m("bit_xor"), BITS, lambda a, b: a ^ b),
        "qmax": (m("qmax"), FC.PAIRS, FC.REF["qmax"]),
        "qmin": (m("qmin"), FC.PAIRS, FC.REF["qmin"]),
        "polynomial": (lambda c, v: chip.polynomial(c, v[0], [flex.Constant(k) for k in coef]), unary[:7] + [(1 << 40,), (-(1 << 40),)], lambda x: FC.ref_polynomial(x, coef)),
        "polynomial of cells": (lambda c, v: chip.polynomial(c, v[0], v[1:]), [(ONE // 3, 5, -7, ONE), (-ONE - 1, -ONE, ONE - 1, 0)], lambda x, *k: FC.ref_polynomial(x, k)),
        "inner_product": (lambda c, v: chip.inner_product(c, v[:3], v[3:]), [tuple(FC.EDGE[:6]), tuple(FC.EDGE[3:]), (FC.BIG, -FC.BIG, 1, FC.BIG, FC.BIG, -1)],
                          lambda *v: FC.ref_inner_product(v[:3], v[3:])),
    }


GROUPS = {"gate": _gate_instructions, "range": _range_instructions, "chip": _chip_methods}
NAMES = [("gate", n) for n in ("sub", "sub of a constant", "neg", "mul_add", "mul_add with constants", "select", "select of constants", "not_", "and_", "or_",
                               "is_zero", "is_equal", "assert_bit", "assert_is_const", "sum", "sum of nothing", "load_constant", "load_zero")] + \
        [("range", n) for n in ("check_less_than", "check_big_less_than_safe", "is_less_than", "div_mod quotient", "div_mod remainder", "div_mod_var quotient",
                                "div_mod_var remainder")] + \
        [("chip", n) for n in ("qadd", "qsub", "neg", "qsum", "qabs", "is_neg", "sign", "cond_neg", "clip", "signed_div_scale quotient",
                               "signed_div_scale remainder", "qmul", "qdiv", "qmod", "bit_xor", "qmax", "qmin", "polynomial", "polynomial of cells", "inner_product")]


@pytest.mark.parametrize("group,name", NAMES, ids=[f"{g}-{n.replace(' ', '_')}" for g, n in NAMES])
def test_instruction_on_edge_operands(h2, group, name):
    from halo2_scaffold_amd import flex

    table = GROUPS[group](flex)
    assert sorted(n for g, n in NAMES if g == group) == sorted(table)  # every entry of the table is a test
    body, cases, reference = table[name]
    _exercise(h2, body, cases, reference)


def test_load_zero_is_one_cell(h2):
    from halo2_scaffold_amd import flex

    ctx = flex.Context(flex.Assignment(flex.FlexGateCS(False)))
    z = ctx.load_zero()
    assert ctx.load_zero() == z == ctx.sum([]) and ctx.cells == [0] and ctx.const_cells == [(0, 0)]
    assert ctx.load_constant(0) == 1 and ctx.sum([z]) == 2 and ctx.eqs == [(2, 0)]  # a constant cell of its own; one operand: its cell again


def test_unsatisfiable_operands_are_refused_on_the_host(h2):
    """a < b that does not hold, a bit that is none, a constant that is another, a zero divisor, a quotient beyond signed_div_scale's bound:
    synthesis stops at a range check (the builders' assertion) or mock names the violation"""
    from halo2_scaffold_amd import flex
    from halo2_scaffold_amd.fixed_point import FixedPointChip

    chip = FixedPointChip(P)
    bad = [(lambda c, v: c.check_less_than(v[0], v[1], 64), (5, 5)), (lambda c, v: c.check_less_than(v[0], v[1], 64), (6, 5)),
           (lambda c, v: c.assert_bit(v[0]), (2,)), (lambda c, v: c.assert_is_const(v[0], 4), (5,)),
           (lambda c, v: c.div_mod_var(v[0], v[1], 100, 64)[0], (9, 0)), (lambda c, v: c.div_mod_var(v[0], v[1], 100, 64)[0], (0, 0)),
           (lambda c, v: chip.qdiv(c, v[0], v[1]), (ONE, 0)), (lambda c, v: chip.qmul(c, v[0], v[1]), ((1 << 64) - 1, (1 << 33) + 1)),
           (lambda c, v: chip.qmul(c, v[0], v[1]), (-(1 << 64), 1 << 64)), (lambda c, v: chip.qmod(c, v[0], v[1]), (5, -3))]
    for body, case in bad:
        with pytest.raises((ValueError, AssertionError)) as e:
            asg, _, _ = _synth(flex, body, [case], flex.FlexGateCS(True), LOOKUP_BITS)
            flex.mock(asg, 12)
        assert isinstance(e.value, ValueError) or "witness out of range" in str(e.value), case


def test_is_neg_at_its_threshold(h2):
    from halo2_scaffold_amd import flex
    from halo2_scaffold_amd.fixed_point import FixedPointChip

    chip = FixedPointChip(P)
    assert chip.negative_point == R - (1 << 65)
    for v, want in (((1 << 65) - 1, 0), (1 << 65, 1), (R - 1, 1), (0, 0)):
        asg, ctx, (out,) = _synth(flex, lambda c, cells: chip.is_neg(c, cells[0]), [(v,)], flex.FlexGateCS(True), LOOKUP_BITS)
        flex.mock(asg, 12)
        assert ctx.cells[out] == want, v
    for bad in (31, 64):
        with pytest.raises(AssertionError):
            FixedPointChip(bad)
    FixedPointChip(63)


# ---- recording ----------------------------------------------------------------------------------------------------------------------------
def _host(f, inputs, cs, lookup_bits):
    from halo2_scaffold_amd import flex

    asg = flex.Assignment(cs)
    ctx = flex.Context(asg)
    ctx.lookup_bits = lookup_bits
    public = []
    f(ctx, inputs, public)
    ctx.finish(public)
    return flex.load_lookup_table(asg, lookup_bits), ctx.cells, public


def _regression_circuits(flex):
    """(closure, dummy, input sets, reference, k, LOOKUP_BITS) of the proofs of tests/test_gpu_fixed_point.py"""
    from halo2_scaffold_amd import linear_regression as LR

    flat_train = lambda w, b, x, y, rate: (lambda nw, nb: nw + [nb])(*FC.ref_train(w, b, x, y, rate))
    return [(LR.inference, FC.INFERENCE_DUMMY, FC.INFERENCE_INPUTS, lambda x, w, b: list(x) + [FC.ref_inference(x, w, b)], 8, 7),
            (LR.train, FC.TRAIN_DUMMY, FC.TRAIN_INPUTS, flat_train, 9, 8)]


def test_the_regression_closures_record_and_replay(h2):
    from halo2_scaffold_amd import flex, witness

    for f, dummy, input_sets, reference, k, lookup_bits in _regression_circuits(flex):
        cs = flex.configure(True, k, lambda cs: _host(f, FC.field_inputs(dummy), cs, lookup_bits)[0])
        assert cs.num_advice >= 2
        program, recorded = witness.Program.record(f, FC.field_inputs(dummy), cs, lookup_bits)
        plain, cells, public = _host(f, FC.field_inputs(dummy), cs, lookup_bits)
        assert recorded.advice == plain.advice and recorded.fixed == plain.fixed and recorded.copies == plain.copies and recorded.instance == plain.instance
        assert program.cells(FC.field_inputs(dummy)) == cells and program.public == public
        assert program.n_aux > 0 and program.n_cells == len(cells) + program.n_aux
        assert all(int(s) < len(cells) for p in program.placement for s in p)  # no column places an auxiliary cell
        kinds = {int(code) & 0xFF for code in program.ops[:, 1]}
        assert {flex.DIVQ, flex.DIVR, flex.ISZERO, flex.INV} <= kinds
        program.descriptor().check()
        for inputs in input_sets:
            fresh, cells, _ = _host(f, FC.field_inputs(inputs), cs, lookup_bits)
            flex.mock(fresh, k)
            got = program.cells(FC.field_inputs(inputs))
            assert got == cells
            assert program.break_points == list(fresh.break_points) == list(recorded.break_points)
            for j, column in enumerate(program.columns(got)):
                assert dict(enumerate(column)) == fresh.advice[j]
            assert [got[c] for c in program.public] == fresh.instance == [FC.to_field(v) for v in reference(*inputs)]


def test_a_closure_written_before_records_the_tape_it_recorded(h2):
    """no auxiliary cell, no new check: the instructions that were there, range_check's one-bit top limb among them"""
    from halo2_scaffold_amd import flex, witness

    for f, dummy, cs, lookup_bits, checks in ((W.gate_closure, 3, flex.FlexGateCS(False), None, 0), (W.range_closure, W.range_inputs(0, 2), flex.FlexGateCS(True), 7, 2),
                                              (W.range_closure, W.range_inputs(0, 2), flex.FlexGateCS(True), 12, 2)):
        program, _ = witness.Program.record(f, dummy, cs, lookup_bits)
        assert program.n_aux == 0 and len(program.checks) == checks and int(program.ops[:, 3].max()) == 0
        assert {int(code) & 0xFF for code in program.ops[:, 1]} <= {W.INPUT, W.CONST, W.COPY, W.GATE, W.LIMB}


def test_zero_divisor_and_overflowing_product_are_witnesses_out_of_range(h2):
    from halo2_scaffold_amd import flex, witness
    from halo2_scaffold_amd import linear_regression as LR
    from halo2_scaffold_amd.fixed_point import FixedPointChip

    chip = FixedPointChip(P)

    def quotient(ctx, inputs, make_public):
        a, b = (ctx.load_witness(v) for v in inputs)
        make_public.append(chip.qdiv(ctx, a, b))

    def quotient_var(ctx, inputs, make_public):
        a, b = (ctx.load_witness(v) for v in inputs)
        make_public.append(ctx.div_mod_var(a, b, 100, 64)[0])

    cs = flex.FlexGateCS(True)
    for f in (quotient, quotient_var):
        program, _ = witness.Program.record(f, [7, 2], cs, LOOKUP_BITS)
        assert program.cells([7 * ONE, 2 * ONE])[program.public[0]] in (7 * ONE // 2, 3)
        for bad in ([7, 0], [0, 0]):
            with pytest.raises(ValueError, match="witness out of range"):
                program.cells(bad)
    program, _ = witness.Program.record(LR.inference, FC.field_inputs(FC.INFERENCE_DUMMY), cs, LOOKUP_BITS)
    top = (1 << 64) - 1
    assert program.cells(([top, 0, 0], [(1 << 33) - 1, 0, 0], 0))[program.public[-1]] == FC.ref_inference([top, 0, 0], [(1 << 33) - 1, 0, 0], 0)
    for bad in (([top, 0, 0], [(1 << 33) + 1, 0, 0], 0), ([R - (1 << 64), 0, 0], [1 << 64, 0, 0], 0)):  # a quotient of 2^65 and more, of -2^96
        with pytest.raises(ValueError, match="witness out of range"):
            program.cells(bad)

    def constant(ctx, inputs, make_public):  # assert_is_const and a gate that closes on an existing cell are checks too
        a, b = (ctx.load_witness(v) for v in inputs)
        ctx.assert_is_const(a, 5)
        ctx.assert_bit(b)

    program, _ = witness.Program.record(constant, [5, 1], flex.FlexGateCS(False), None)
    assert len(program.checks) == 2 and program.cells([5, 0]) == program.cells([5, 0])
    for bad in ([4, 1], [5, 2]):
        with pytest.raises(ValueError, match="witness out of range"):
            program.cells(bad)


# ---- h2mi_witness_check ----------------------------------------------------------------------------------------------------------------------
def _good(witness):
    """cells: 0, 1 inputs; 2 a copy of 0; 3 = cell 2 div cell 1; 4 = cell 0 mod the constant 9, signed; 5, 6 ISZERO and INV of cell 3; 7 a constant"""
    t = FC.Tape()
    a, b = t.input(0), t.input(1)
    c = t.copy(a)
    d = t.div(FC.DIVQ, c, y_cell=b)
    t.div(FC.DIVR, a, y_const=9, signed=True)
    t.hint(FC.ISZERO, d)
    t.hint(FC.INV, d)
    t.const(11)
    return t.program(witness, checks=[(0, 2)], placement=[[0, 1, 2, 3], [4, 5, 6, 7]])


def _rc(program):
    from halo2_scaffold_amd._lib import lib

    d = program.descriptor()
    return lib.h2mi_witness_check(C.byref(d))


def _with_op(witness, dst, **change):
    p = _good(witness)
    ops = p.ops.copy()
    (at,) = [i for i, row in enumerate(ops.tolist()) if row[0] == dst]
    row = dict(zip(("dst", "code", "a", "b"), ops[at].tolist()))
    row.update(change)
    ops[at] = [row["dst"], row["code"], row["a"], row["b"]]
    return witness.Program(ops, p.level_ends, p.constants, p.n_inputs, p.checks, p.placement, [])


def test_validator_takes_the_new_kinds_and_refuses_what_they_must_not_hold(h2):
    from halo2_scaffold_amd import witness

    good = _good(witness)
    assert _rc(good) == 0 and good.level_sizes == [3, 2, 1, 2] and good.constants == [9, 11]
    assert good.cells([100, 7]) == [100, 7, 100, 14, 1, 0, pow(14, -1, R), 11]
    code = lambda kind, flags=0, shift=0: kind | flags << 8 | shift << 16
    bad = {
        "an unknown flag bit": _with_op(witness, 3, code=code(FC.DIVQ, 4)),
        "an unknown flag bit beside the known": _with_op(witness, 4, code=code(FC.DIVR, 3 | 128)),
        "a shift": _with_op(witness, 3, code=code(FC.DIVQ, 0, 1)),
        "a shift on ISZERO": _with_op(witness, 5, code=code(FC.ISZERO, 0, 5)),
        "b at its reader's level": _with_op(witness, 3, b=3),
        "b above its reader's level": _with_op(witness, 3, b=5),
        "b outside the cells": _with_op(witness, 3, b=8),
        "a at its reader's level": _with_op(witness, 3, a=3),
        "a outside the cells": _with_op(witness, 5, a=8),
        "a constant index out of range": _with_op(witness, 4, b=2),
        "flags on ISZERO": _with_op(witness, 5, code=code(FC.ISZERO, 1)),
        "flags on INV": _with_op(witness, 6, code=code(FC.INV, 2)),
        "b on ISZERO": _with_op(witness, 5, b=1),
        "b on INV": _with_op(witness, 6, b=1),
        "INV of a higher level": _with_op(witness, 6, a=5),
        "kind 6": _with_op(witness, 5, code=6),
        "kind 7": _with_op(witness, 5, code=7),
        "kind 12": _with_op(witness, 5, code=12),
        "the top byte": _with_op(witness, 3, code=code(FC.DIVQ) | 1 << 24),
    }
    for what, p in bad.items():
        assert _rc(p) == EINVAL, what
    # what is allowed: every flag combination, a constant where the cell was, a cell of a lower level where the constant was
    for flags in range(4):
        assert _rc(_with_op(witness, 4, code=code(FC.DIVR, flags | 1))) == 0 and _rc(_with_op(witness, 3, code=code(FC.DIVQ, flags & 2))) == 0
    assert _rc(_with_op(witness, 3, code=code(FC.DIVQ, 1), b=1)) == 0 and _rc(_with_op(witness, 4, code=code(FC.DIVR, 2), b=1)) == 0
    assert _rc(_with_op(witness, 4, code=code(FC.DIVR, 2), b=2)) == EINVAL  # cell 2 is at DIVR's own level


def test_hand_built_tapes_are_what_they_are_named_for(h2):
    """the GPU tests' inputs: the interpreter agrees with the cases' own evaluation, every form and every launch shape is reached"""
    from halo2_scaffold_amd import witness

    t, inputs, listed = FC.ops_tape()
    program = t.program(witness)
    want = t.evaluate(inputs)
    assert program.cells(inputs) == want and _rc(program) == 0
    assert all(want[cell] == FC.ref_hint(kind, x, y, flags) for cell, kind, x, y, flags in listed)
    forms = {(kind, flags) for _, kind, _, _, flags in listed}
    assert forms == {(k, f) for k in (FC.DIVQ, FC.DIVR) for f in range(4)} | {(FC.ISZERO, 0), (FC.INV, 0)}
    assert {(x, y) for _, kind, x, y, _ in listed if kind == FC.DIVQ} == set(FC.div_pairs())
    sources = {t.cells[t.cells[cell][1]][0] for cell, *_ in listed}  # the dividends' cells
    assert sources == {W.INPUT, W.CONST, W.GATE}
    assert W.segmentation(program.level_sizes) == (1, 2)  # a grid launch between two workgroup launches
    sizes = [40, 1025, 1024, 1]
    t, inputs = FC.layered_ops_tape(sizes)
    program = t.program(witness)
    assert program.level_sizes == sizes and W.segmentation(sizes) == (1, 2) and program.cells(inputs) == t.evaluate(inputs) and _rc(program) == 0
    t, inputs, cell, value = FC.quotient_chain_tape(40, R - 12345)
    program = t.program(witness)
    assert program.level_sizes == [2] * 41 and W.segmentation(program.level_sizes) == (0, 1) and value > 1 << 100
    assert program.cells(inputs)[cell] == value and _rc(program) == 0


# ---- accuracy ---------------------------------------------------------------------------------------------------------------------------------
ULP = 2.0 ** -P


class Approx:
    """a real value and a bound on how far the chip's dequantised value may lie from it, counted rounding by rounding: half an ulp per
    quantisation, less than one ulp per signed_div_scale or division (both round toward minus infinity, or toward zero), the operands'
    own errors carried through products and quotients to first and second order; 2^-50 relative per float operation of this class"""

    def __init__(self, value, err):
        self.value, self.err = value, err + abs(value) * 2.0 ** -50

    @classmethod
    def quantised(cls, x):
        return cls(x, ULP / 2)

    def __add__(self, o):
        return Approx(self.value + o.value, self.err + o.err)

    def __sub__(self, o):
        return Approx(self.value - o.value, self.err + o.err)

    def __mul__(self, o):  # qmul
        return Approx(self.value * o.value, abs(self.value) * o.err + abs(o.value) * self.err + self.err * o.err + ULP)

    def __truediv__(self, o):  # qdiv: |a^ / b^ - a / b| <= (ea + |a / b| eb) / (|b| - eb)
        assert abs(o.value) > o.err
        return Approx(self.value / o.value, (self.err + abs(self.value / o.value) * o.err) / (abs(o.value) - o.err) + ULP)


def _evaluate(flex, body, reals):
    from halo2_scaffold_amd.fixed_point import FixedPointChip

    chip = FixedPointChip(P)
    asg = flex.Assignment(flex.FlexGateCS(True))
    ctx = flex.Context(asg)
    ctx.lookup_bits = LOOKUP_BITS
    out = body(chip, ctx, [ctx.load_witness(chip.quantization(x)) for x in reals])
    return [chip.dequantization(ctx.cells[c]) for c in out]


def test_accuracy_against_float_arithmetic(h2, capsys):
    from halo2_scaffold_amd import flex
    from halo2_scaffold_amd.linear_regression import LinearRegressionChip

    worst = {}

    def compare(name, got, want):
        for g, w in zip(got, want):
            assert abs(g - w.value) <= w.err, (name, g, w.value, w.err)
            worst[name] = max(worst.get(name, 0.0), abs(g - w.value) / ULP)

    pairs = [(0.1, 0.2), (-3.75, 2.5), (1e-3, -1e3), (123.456, -0.001), (-7.0, -1.0 / 3.0), (2.0 ** -32, 1.0), (1000.0, 999.999)]
    for a, b in pairs:
        A, B = Approx.quantised(a), Approx.quantised(b)
        compare("qmul", _evaluate(flex, lambda chip, c, v: [chip.qmul(c, v[0], v[1])], [a, b]), [A * B])
        compare("qdiv", _evaluate(flex, lambda chip, c, v: [chip.qdiv(c, v[0], v[1])], [a, b]), [A / B])
    xs, ws = [0.5, -1.25, 3.0, 0.038, -0.0446], [-0.3, 0.7, 0.1, 152.1, -9.0]
    want = Approx(0.0, 0.0)
    for x, w in zip(xs, ws):
        want = want + Approx.quantised(x) * Approx.quantised(w)
    compare("inner_product", _evaluate(flex, lambda chip, c, v: [chip.inner_product(c, v[:5], v[5:])], xs + ws), [want])
    # one training step of 3 samples x 2 features, learning rate 0.01
    w, b, x, y, rate = [0.25, -0.5], 0.1, [[1.5, -2.0], [-0.75, 0.5], [0.038, 0.0507]], [3.0, -1.0, 151.0], 0.01 / 3
    lr = LinearRegressionChip(None, P)

    def step(chip, c, v):
        ctx_w, ctx_b, flat = v[:2], v[2], v[3:]
        new_w, new_b = lr.train_one_batch(c, ctx_w, ctx_b, [flat[0:2], flat[2:4], flat[4:6]], flat[6:9], chip.quantization(rate))
        return new_w + [new_b]

    got = _evaluate(flex, step, w + [b] + [v for xi in x for v in xi] + y)
    q = Approx.quantised
    W_, B_, X_, Y_, RATE = [q(v) for v in w], q(b), [[q(v) for v in xi] for xi in x], [q(v) for v in y], q(rate)
    diff = []
    for xi, ti in zip(X_, Y_):
        yi = Approx(0.0, 0.0)
        for xij, wj in zip(xi, W_):
            yi = yi + xij * wj
        diff.append(yi + B_ - ti)
    want = []
    for j in range(2):
        partial = Approx(0.0, 0.0)
        for d, xi in zip(diff, X_):
            partial = partial + d * xi[j]
        want.append(W_[j] - RATE * partial)
    total = Approx(0.0, 0.0)
    for d in diff:
        total = total + d
    want.append(B_ - RATE * total)
    compare("training step", got, want)
    with capsys.disabled():
        print("\nlargest error in ulps of 2^-32:", {k: round(v, 3) for k, v in worst.items()})
