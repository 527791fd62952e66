"""Witness programs: a builder closure recorded once as a tape and replayed on the device for every later proof.

`scaffold.prove_private` refuses a closure whose shape depends on its inputs (the break-point check), so under that rule a closure
`f(ctx, inputs, make_public)` is a fixed straight-line program over field elements in which only the private inputs change from proof
to proof.  `Program.record` runs the closure once in a `RecordingContext` — `flex.Context` with an op noted per cell — and keeps the
tape: one op per cell of `Context.cells` (INPUT, CONST, COPY, GATE, LIMB and the hints DIVQ, DIVR, ISZERO, INV, MSB, POW2: include/h2mi.h), sorted
into levels; behind them the auxiliary cells no column places — a value derived outside the gates (the a - b of `sub`) is the GATE of three
such cells, and an enabled gate whose fourth cell is not a GATE op is computed once more among them; the equalities no COPY makes true
(the checks), the auxiliary gates against their fourth cells among them; per advice column the flat cell index of every row (the placement, exactly what `finish` / `_finish_multi`
do with the cells); the public cells.  `Program.cells` interprets the tape on Python integers (the tests' reference);
`Program.on_device` hands it to libh2mi.so (engine.WitnessProgram: csrc/h2mi_witness.hip), whose run leaves dense Montgomery columns
in HBM that the advice call takes as engine.DeviceCells.  What a tape cannot express — a value computed in Python from the inputs
outside the context — is refused while recording, with the cell named."""
import types

import numpy as np

from . import engine, flex
from . import field as F

R = F.FR_MODULUS
INPUT, CONST, COPY, GATE, LIMB = range(5)  # H2MI_WITNESS_*
HINTS = (flex.DIVQ, flex.DIVR, flex.ISZERO, flex.INV, flex.MSB, flex.POW2)
WG_OPS, WG_LEVELS = 1024, 4096  # H2MI_WITNESS_WG_OPS, H2MI_WITNESS_WG_LEVELS


class Input(int):
    """a private input: an int that also carries its index in the program's inputs.  Arithmetic on it gives a plain int."""

    def __new__(cls, value, index: int):
        self = int.__new__(cls, value)
        self.index = index
        return self


def wrap_inputs(inputs):
    """an integer or a (nested) list / tuple of integers -> (the same shape with every integer an Input, numbered in order; how many)"""
    count = [0]

    def wrap(v):
        if isinstance(v, (list, tuple)):
            return type(v)(wrap(x) for x in v)
        if not isinstance(v, (int, np.integer)):
            raise ValueError(f"a witness program's inputs are integers or lists of integers, not {type(v).__name__}")
        count[0] += 1
        return Input(int(v), count[0] - 1)

    return wrap(inputs), count[0]


def flatten_inputs(inputs) -> list:
    """the canonical values of the inputs in the order wrap_inputs numbers them"""
    if isinstance(inputs, (list, tuple)):
        return [v for x in inputs for v in flatten_inputs(x)]
    return [int(inputs) % R]


class RecordingContext(flex.Context):
    """flex.Context that also notes, per cell, the op that computes it.  cells, gates, eqs, const_cells and lookup_cells — and so the
    Assignment and the key — are those of an unrecorded run."""

    def __init__(self, asg):
        super().__init__(asg)
        self.ops = []  # per cell: (kind, a, bits, shift), a hint (kind, a, flags, 0, b)
        self.constants, self._constant_index = [], {}
        # the cells no column places, numbered -1, -2, ... until the cells are counted (from_context), and their checks
        self.aux_ops, self.aux_checks = [], []

    def _aux(self, op) -> int:
        self.aux_ops.append(op)
        return -len(self.aux_ops)

    def _aux_gate(self, operands) -> int:
        """x + y * z of three operands ((COPY, cell) or (CONST, index)) as four consecutive auxiliary cells -> the gate's"""
        for kind, a in operands:
            self._aux((kind, a, 0, 0))
        return self._aux((GATE, 0, 0, 0))

    def derive(self, x, y, z) -> flex.Aux:
        operand = lambda q: (COPY, q.ref) if isinstance(q, flex.Aux) else (CONST, self._constant(int(q) % R)) if isinstance(q, flex.Constant) else (COPY, q)
        return flex.Aux(super().derive(x, y, z).value, self._aux_gate([operand(q) for q in (x, y, z)]))

    def assert_is_const(self, a, c: int):
        super().assert_is_const(a, c)
        self.aux_checks.append((a, self._aux((CONST, self._constant(c % R), 0, 0))))

    def _constant(self, v: int) -> int:
        if v not in self._constant_index:
            self._constant_index[v] = len(self.constants)
            self.constants.append(v)
        return self._constant_index[v]

    def load_witness(self, v: int) -> int:
        if not isinstance(v, Input):
            raise ValueError(f"cell {len(self.cells)}: load_witness of a plain integer — a hint computed in Python from the inputs, whose "
                             "dependence on them a witness program cannot see")
        self.ops.append((INPUT, v.index, 0, 0))
        return super().load_witness(v)

    def assign_region_last(self, items, gate_offsets, gates_hold: bool = False) -> int:
        """gates_hold: the caller knows the region's gates to hold for every input (range_check's one-bit top limb), so a gate that
        closes on a cell that is no GATE op needs no check"""
        base = len(self.cells)
        fourth = {off + 3 for off in gate_offsets}
        value = lambda row: vals[row - base] if row >= base else self.cells[row]
        ops, vals = [], []
        for i, (kind, v) in enumerate(items):
            row = base + i
            if kind == "existing":
                ops.append((COPY, v, 0, 0))
                vals.append(self.cells[v])
            elif kind == "constant":
                ops.append((CONST, self._constant(v % R), 0, 0))
                vals.append(v % R)
            elif kind == "hint":
                hint_kind, a, b, flags = v
                unary = hint_kind not in (flex.DIVQ, flex.DIVR)
                if isinstance(a, flex.Constant):  # known with the circuit: a CONST op, and no fixed cell beside it
                    if not unary and not flags & flex.HINT_CONST:
                        raise ValueError(f"cell {row}: a hint that divides a constant by a cell is not an op of the tape: load_constant the dividend")
                    ops.append((CONST, self._constant(self.hint_value(*v)), 0, 0))
                else:
                    ops.append((hint_kind, a, flags, 0, 0 if unary else self._constant(b % R) if flags & flex.HINT_CONST else b))
                vals.append(self.hint_value(*v))
            elif kind == "limb":
                ops.append((LIMB, v[0], v[1], v[2]))
                vals.append((self.cells[v[0]] >> v[2]) & ((1 << v[1]) - 1))
            elif kind == "aux":
                ops.append((COPY, v.ref, 0, 0))
                vals.append(v.value)
            elif kind == "copy":
                ops.append((COPY, v, 0, 0))
                vals.append(value(v))
            elif isinstance(v, Input):
                ops.append((INPUT, v.index, 0, 0))
                vals.append(v % R)
            elif i in fourth and row >= 3:
                want = (value(row - 3) + value(row - 2) * value(row - 1)) % R
                if v % R != want:
                    raise ValueError(f"cell {row}: the fourth cell of a gate is assigned a value that is not the gate's (an unsatisfying witness)")
                ops.append((GATE, 0, 0, 0))
                vals.append(want)
            else:
                raise ValueError(f"cell {row}: a witness value that is neither an Input nor the fourth cell of a gate enabled in this call")
        self.ops += ops
        for off in gate_offsets:  # a gate that closes on an existing cell, a constant or an input: computed once more, and compared
            if ops[off + 3][0] != GATE and not gates_hold:
                self.aux_checks.append((base + off + 3, self._aux_gate([(COPY, base + off + i) for i in range(3)])))
        return super().assign_region_last(items, gate_offsets)

    def range_check(self, a, range_bits: int, lookup_bits: int):
        """flex.Context.range_check cell for cell; the limbs are LIMB ops of cell a, the running sums and the shifted top limb GATEs.  The
        top limb takes the bits below range_bits only, so a value beyond them fails the check of a against its recomposition."""
        x = self.cells[a]
        assert x < 1 << range_bits, "witness out of range"
        if range_bits > 254 or not 1 <= lookup_bits <= 64:
            raise ValueError(f"cell {len(self.cells)}: range_check over {range_bits} bits in limbs of {lookup_bits} is beyond a LIMB op (shift + bits <= 254, bits <= 64)")
        num_limbs = -(-range_bits // lookup_bits)
        limbs = [(x >> (lookup_bits * i)) & ((1 << lookup_bits) - 1) for i in range(num_limbs)]
        limb_op = lambda i: (LIMB, a, min(lookup_bits, range_bits - lookup_bits * i), lookup_bits * i)
        rows = [len(self.cells)]
        self.cells.append(limbs[0] % R)
        self.ops.append(limb_op(0))
        acc, acc_row = limbs[0], rows[0]
        for i in range(1, num_limbs):
            base = len(self.cells) - 1
            acc += limbs[i] << (lookup_bits * i)
            self.cells.append(limbs[i])
            self.ops.append(limb_op(i))
            rows.append(len(self.cells) - 1)
            self.cells.append((1 << (lookup_bits * i)) % R)
            self.ops.append((CONST, self._constant((1 << (lookup_bits * i)) % R), 0, 0))
            self.const_cells.append((len(self.cells) - 1, (1 << (lookup_bits * i)) % R))
            self.cells.append(acc % R)
            self.ops.append((GATE, 0, 0, 0))
            self.gates.append(base)
            acc_row = len(self.cells) - 1
        self.eqs.append((a, acc_row))
        self.lookup_cells += rows
        rem = range_bits % lookup_bits
        if rem == 1:
            self.assign_region_last([("constant", 0), ("existing", rows[-1]), ("existing", rows[-1]), ("existing", rows[-1])], [0], gates_hold=True)
        elif rem:
            self.lookup_cells.append(self.assign_region_last([("constant", 0), ("existing", rows[-1]), ("constant", 1 << (lookup_bits - rem)),
                                                              ("witness", limbs[-1] << (lookup_bits - rem))], [0]))


def place(n_cells: int, gates, lookup_cells, cs):
    """where finish / _finish_multi put the cells, as indices instead of values -> (per advice column the flat cell index of every row
    0 .. count - 1, the break points).  The walk is flex.Context._finish_multi's: a cell on a column's last row, or one that starts a
    gate which no longer fits, is assigned a second time at row 0 of the next column; the cells to look up are copied into the
    lookup-advice columns."""
    if cs.num_advice == 1:
        return [list(range(n_cells))], []
    A, Lc = cs.num_advice, cs.num_lookup_advice
    max_rows = (1 << cs.k) - cs.minimum_rows
    gate_at = set(gates)
    columns, breaks = [[] for _ in range(A + Lc)], []
    col = 0
    for i in range(n_cells):
        row = len(columns[col])
        columns[col].append(i)
        if (i in gate_at and row + 4 > max_rows) or row >= max_rows - 1:
            if col + 1 >= A:
                raise ValueError(f"NOT ENOUGH ADVICE COLUMNS: more than {A} gate columns needed at 2^{cs.k} rows")
            breaks.append(row)
            col += 1
            columns[col].append(i)
    lcol = 0
    for i in lookup_cells:
        if lcol < Lc and len(columns[A + lcol]) >= max_rows:
            lcol += 1
        if lcol >= Lc:
            raise ValueError("NOT ENOUGH LOOKUP ADVICE COLUMNS")
        columns[A + lcol].append(i)
    return columns, breaks


def segmentation(level_sizes):
    """the launches of one run, by the rule of include/h2mi.h -> [("grid", level) | ("wg", first level, end level)]: a level of more
    than WG_OPS ops is a grid launch of its own; every maximal run of consecutive levels of at most WG_OPS ops is a sequence of
    single-workgroup launches of at most WG_LEVELS levels each"""
    plan, run0 = [], 0

    def close(end):
        for l in range(run0, end, WG_LEVELS):
            plan.append(("wg", l, min(end, l + WG_LEVELS)))

    for l, size in enumerate(level_sizes):
        if size > WG_OPS:
            close(l)
            plan.append(("grid", l))
            run0 = l + 1
    close(len(level_sizes))
    return plan


class Program:
    """a recorded closure.  ops: (n_cells, 4) uint32 rows (dst, kind | bits << 8 | shift << 16, a, b) sorted by level; level_ends;
    constants (integers below r); n_inputs; checks [(a, b)]; placement (one uint32 array of cell indices per advice column); public
    (the cells of make_public); break_points (of the gate columns, as gen_key returns them); n_aux: the last n_aux cells are auxiliary
    (no column places them, and `cells` does not return them)."""

    def __init__(self, ops, level_ends, constants, n_inputs, checks, placement, public, break_points=(), n_aux: int = 0):
        self.ops = np.ascontiguousarray(np.asarray(ops, dtype=np.uint32).reshape(-1, 4))
        self.level_ends = np.ascontiguousarray(level_ends, dtype=np.uint32)
        self.constants, self.n_inputs = [int(c) for c in constants], int(n_inputs)
        self.checks = [(int(a), int(b)) for a, b in checks]
        self.placement = [np.ascontiguousarray(p, dtype=np.uint32) for p in placement]
        self.public, self.break_points = [int(c) for c in public], list(break_points)
        self.n_aux = int(n_aux)
        self._device = None

    @property
    def n_cells(self) -> int:
        return len(self.ops)

    @property
    def level_sizes(self) -> list:
        ends = [0] + [int(e) for e in self.level_ends]
        return [b - a for a, b in zip(ends, ends[1:])]

    @classmethod
    def from_context(cls, ctx: RecordingContext, n_inputs: int, public) -> "Program":
        n = len(ctx.cells)
        assert len(ctx.ops) == n, "every cell has its op"
        cell = lambda s: s if s >= 0 else n - 1 - s  # auxiliary cell -1 - j is cell n + j
        ops = [tuple(op) + (0,) * (5 - len(op)) for op in list(ctx.ops) + ctx.aux_ops]
        ops = [(kind, cell(a) if kind in (COPY, LIMB) + HINTS else a, bits, shift, cell(b) if kind in (flex.DIVQ, flex.DIVR) and not bits & flex.HINT_CONST else b)
               for kind, a, bits, shift, b in ops]
        total = len(ops)

        def operands(i):
            kind, a, bits, _, b = ops[i]
            if kind == GATE:
                return (i - 3, i - 2, i - 1)
            if kind in (flex.DIVQ, flex.DIVR) and not bits & flex.HINT_CONST:
                return (a, b)
            return (a,) if kind in (COPY, LIMB) + HINTS else ()

        level = [None] * total  # one above the highest operand; an auxiliary cell may be read by a cell of a lower index
        for root in range(total):
            stack = [root]
            while stack:
                i = stack[-1]
                if level[i] is None:
                    waiting = [s for s in operands(i) if level[s] is None]
                    if waiting:
                        stack += waiting
                        continue
                    level[i] = 1 + max((level[s] for s in operands(i)), default=-1)
                stack.pop()
        order = sorted(range(total), key=lambda i: (level[i], i))
        rows = [(i, ops[i][0] | ops[i][2] << 8 | ops[i][3] << 16, ops[i][1], ops[i][4]) for i in order]
        sizes = np.bincount(np.array(level, dtype=np.int64), minlength=1) if total else np.zeros(0, dtype=np.int64)
        made = {(i, op[1]) for i, op in enumerate(ops) if op[0] == COPY}  # the equalities a COPY makes true
        checks = [(a, b) for a, b in ctx.eqs if (a, b) not in made and (b, a) not in made] + [(cell(a), cell(b)) for a, b in ctx.aux_checks]
        placement, breaks = place(n, ctx.gates, ctx.lookup_cells, ctx.asg.cs)
        return cls(rows, np.cumsum(sizes), ctx.constants, n_inputs, checks, placement, public, breaks, n_aux=total - n)

    @classmethod
    def record(cls, f, dummy_inputs, cs, lookup_bits):
        """run the closure once with its inputs wrapped as Inputs (what scaffold._synthesize does, in a RecordingContext)
        -> (program, assignment)"""
        asg = flex.Assignment(cs)
        ctx = RecordingContext(asg)
        ctx.lookup_bits = lookup_bits
        wrapped, n_inputs = wrap_inputs(dummy_inputs)
        make_public = []
        f(ctx, wrapped, make_public)
        ctx.finish(make_public)
        if cs.lookup:
            flex.load_lookup_table(asg, lookup_bits)
        program = cls.from_context(ctx, n_inputs, make_public)
        # the placement against what finish did with the values, and the tape against the run it was recorded from
        cells = program.cells(dummy_inputs)
        assert cells == ctx.cells and list(asg.break_points) == program.break_points
        for j, src in enumerate(program.placement):
            assert [cells[s] for s in src] == [asg.advice[j][r] for r in range(len(asg.advice[j]))], f"placement of column {j}"
        return program, asg

    def cells(self, inputs) -> list:
        """the tape on Python integers -> Context.cells of a run on these inputs; ValueError("witness out of range ...") naming the
        first check that fails"""
        values = flatten_inputs(inputs)
        if len(values) != self.n_inputs:
            raise ValueError(f"the program takes {self.n_inputs} inputs, not {len(values)}")
        cells = [None] * self.n_cells
        for dst, code, a, b in self.ops.tolist():
            kind, bits, shift = code & 0xFF, (code >> 8) & 0xFF, (code >> 16) & 0xFF
            if kind == INPUT:
                cells[dst] = values[a]
            elif kind == CONST:
                cells[dst] = self.constants[a]
            elif kind == COPY:
                cells[dst] = cells[a]
            elif kind == GATE:
                cells[dst] = (cells[dst - 3] + cells[dst - 2] * cells[dst - 1]) % R
            elif kind == LIMB:
                cells[dst] = (cells[a] >> shift) & ((1 << bits) - 1)
            else:  # a hint; bits holds its flags
                cells[dst] = flex.hint(kind, cells[a], (self.constants[b] if bits & flex.HINT_CONST else cells[b]) if kind in (flex.DIVQ, flex.DIVR) else 0, bits)
        for i, (a, b) in enumerate(self.checks):
            if cells[a] != cells[b]:
                raise ValueError(f"witness out of range: check {i} fails, cells {a} and {b} differ")
        return cells[:self.n_cells - self.n_aux]

    def columns(self, cells) -> list:
        """the dense advice columns of a cell list, by the placement"""
        return [[cells[s] for s in src] for src in self.placement]

    def descriptor(self) -> "engine.WitnessDesc":
        return engine.WitnessDesc.build(self.ops, self.level_ends, self.constants, self.n_inputs, self.checks, self.placement)

    def on_device(self) -> "engine.WitnessProgram":
        """the program in HBM (uploaded once, kept with this object until release())"""
        if self._device is None:
            self._device = engine.WitnessProgram(self.descriptor())
        return self._device

    def release(self):
        if self._device is not None:
            self._device.release()
            self._device = None


def advice(program: Program, inputs):
    """run the program on the device -> (advice, instance): what flex.create_proof reads off an Assignment as asg.advice (one
    engine.DeviceCells per column, valid until the program's next run) and asg.instance (the public cells, read back)"""
    values = flatten_inputs(inputs)
    if len(values) != program.n_inputs:
        raise ValueError(f"the program takes {program.n_inputs} inputs, not {len(values)}")
    dev = program.on_device()
    columns = dev.run(values)
    return columns, dev.read(program.public)


def assignment(program: Program, inputs) -> types.SimpleNamespace:
    """advice() as the small namespace that stands in for the Assignment in flex.create_proof / flex.check"""
    columns, instance = advice(program, inputs)
    return types.SimpleNamespace(advice=columns, instance=instance)
