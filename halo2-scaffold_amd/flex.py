"""keygen + create_proof for the halo2-lib constraint systems the reference proves through `scaffold::prove`
(src/scaffold.rs:246-366), with every vector resident in HBM — BASELINE configs[2] (halo2_lib.rs: x^2 + 72) and
configs[3] (range.rs: range_check(x, 64) with a LOOKUP_BITS table).  This module holds what the CALLER of the library's prover
holds: the constraint system as data (FlexGateCS.abi), the builders' cell layout (Context: witness generation on the CPU, as in the
reference), the transcript.  FlexKeys and create_proof are thin calls into libh2mi.so (engine.Keys / engine.Prover over
include/h2mi_prover.h); the device pipeline described below lives in csrc/h2mi_prover.cpp.

The reference builds these circuits with halo2-base (GateWithInstanceCircuitBuilder / RangeWithInstanceCircuitBuilder,
src/scaffold.rs:379-485: FlexGate's vertical gate q (a + a(wX) a(w^2 X) - a(w^3 X)) on the advice column, a constants
column, RangeConfig's table and — these circuits fit one advice column, so — its complex selector q_lookup on the
looked-up cells' own rows (`range.q_lookup`, :464-469) instead of a lookup-advice column, and one instance column added —
and equality-enabled — last, :394-395, :449-450).  halo2-base is an un-vendored dependency; its cell layout (load_witness, mul, add, mul_add,
range_check's limb decomposition) is restated from memory in `halo2_lib_closure` / `range_closure` below — the witness
generation a prover runs on the CPU.  Everything after it is the same device pipeline as prover.py, generalised:
an instance column (public inputs are hashed into the transcript and take part in the permutation argument), advice
queries at rotations 0..3, permutation sets of `degree - 2` columns, and for the Range builder one lookup argument with
the input expression q_lookup * a (row values by one element-wise product, permuted columns by counting sort against the
keygen-sorted table, lookup grand product, five more terms in evaluate_h; degree 5: extended domain 4n, four h pieces).  Checked against oracle/flex.py: byte-identical proofs at
small k, accepted by its verifier at k = 16 and above (tests/test_gpu_flex.py).
rng stand-in as in prover.py, plus streams seed+4 (blinding rows of the permuted lookup columns) and seed+5 (of the
lookup product).
"""
import json

from . import engine
from . import field as F
from .domain import EvaluationDomain
from .keygen import _m, transcript_repr
from .params import ParamsKZG
from .transcript import Blake2bWrite

R = F.FR_MODULUS
ADVICE, FIXED, INSTANCE = "advice", "fixed", "instance"
_KIND = {ADVICE: engine.ADVICE, FIXED: engine.FIXED, INSTANCE: engine.INSTANCE}

# the hints: values halo2-base computes outside the gates and assigns as witnesses (H2MI_WITNESS_DIVQ .. INV of include/h2mi.h)
DIVQ, DIVR, ISZERO, INV = 8, 9, 10, 11
MSB, POW2 = 13, 14  # H2MI_WITNESS_MSB, H2MI_WITNESS_POW2; 12 is reserved
HINT_CONST, HINT_SIGNED = 1, 2  # DIVQ / DIVR: the divisor is a constant, not a cell; the dividend is signed (above 2^252: x - r)
HINT_OF_MSB = 1  # POW2: of the index of the operand's highest set bit (H2MI_WITNESS_POW2_OF_MSB)
NUM_BITS = 254  # F::NUM_BITS: the length of pow_of_two


def hint(kind: int, x: int, y: int = 0, flags: int = 0) -> int:
    """THE definition of the hints, on canonical integers below r: what flex.Context assigns, what witness.Program.cells replays
    and what the device kernels are tested against.  DIVQ / DIVR: quotient and remainder of x by y, 0 for y = 0; signed, a dividend
    above 2^252 is x - r, the quotient rounds toward minus infinity and is stored mod r, the remainder is in [0, y) (the reference's
    signed_div_scale: src/gadget/fixed_point.rs:991-1001).  ISZERO: 1 for 0, else 0.  INV: x^-1 mod r, and 1 for 0 (halo2-base's
    is_zero assigns Assigned::Trivial(1) there [RECALL]).  MSB: the index of the highest set bit, and 1 for 0 (the fold over the bits in the
    reference's qlog2: src/gadget/fixed_point.rs:725-737).  POW2: 2^x for x <= 253 and 0 beyond (the reference indexes pow_of_two and
    would panic there: 0 satisfies no check_power_of_two); HINT_OF_MSB: 2^MSB(x)."""
    if kind == ISZERO:
        return int(x == 0)
    if kind == INV:
        return pow(x, -1, R) if x else 1
    if kind == MSB:
        assert not flags
        return x.bit_length() - 1 if x else 1
    if kind == POW2:
        assert not flags & ~HINT_OF_MSB
        e = hint(MSB, x) if flags & HINT_OF_MSB else x
        return 1 << e if e < NUM_BITS else 0
    assert kind in (DIVQ, DIVR) and not flags & ~(HINT_CONST | HINT_SIGNED)
    if y == 0:
        return 0
    if flags & HINT_SIGNED and x > 1 << 252:
        x -= R
    q, rem = divmod(x, y)  # Python's floor division: toward minus infinity, 0 <= rem < y
    return q % R if kind == DIVQ else rem


class Constant(int):
    """an operand that is a constant of the circuit instead of a cell (QuantumCell::Constant); a plain integer operand is a cell"""


class Aux:
    """a value derived from cells and constants as x + y * z outside the columns (Context.derive): what halo2-base computes in Rust and
    assigns as a Witness where it is not the fourth cell of a gate — the a - b of `sub`, the shifted value of `check_less_than`.  `ref`
    is the recorder's (witness.RecordingContext): the unplaced cell of the tape that holds it."""

    def __init__(self, value: int, ref=None):
        self.value, self.ref = value, ref


class FlexGateCS:
    """the constraint system of the Gate builder (lookup = False) or the Range builder (lookup = True) when the circuit
    fits ONE advice column (every example of the reference at its DEGREE).  Columns in configure()'s allocation order
    [RECALL halo2-base]: RangeConfig takes the lookup table column first; FlexGateConfig the constants column
    (enable_equality at once: it leads the permutation argument), then the gate advice column and its simple selector;
    the scaffold adds the instance column last.  With a single advice column RangeConfig looks up q_lookup * a (complex
    selector) instead of adding a lookup-advice column.  keygen appends the selector columns: complex ones first.
      Gate:  fixed 0 constants, 1 q_enable                          degree 3: permutation sets of one, 2 h pieces
      Range: fixed 0 table, 1 constants, 2 q_lookup, 3 q_enable     degree 2 + 2 + 1 = 5: sets of three, 4 h pieces
    Queries in creation order (enable_equality queries its column at Rotation::cur)."""

    def __init__(self, lookup: bool, num_advice: int = 1, num_lookup_advice: int = 0, k: int = None, minimum_rows: int = 9, num_fixed: int = 1):
        self.lookup = lookup
        self.num_advice, self.num_lookup_advice, self.num_fixed = num_advice, num_lookup_advice, num_fixed
        self.k, self.minimum_rows = k, minimum_rows  # the multi-column layout needs the row budget 2^k - minimum_rows
        if num_advice > 1:
            self._init_multi()
            return
        assert num_lookup_advice == 0 and num_fixed == 1  # at most 2^k - minimum_rows cells: their constants fit one column
        self.n_advice = 1
        if lookup:
            self.col_table, self.col_const, self.col_qlookup, self.col_q = 0, 1, 2, 3
            self.n_fixed = 4
            self.fixed_queries = [(1, 0), (0, 0), (2, 0), (3, 0)]
        else:
            self.col_table = self.col_qlookup = None
            self.col_const, self.col_q = 0, 1
            self.n_fixed = 2
            self.fixed_queries = [(0, 0), (1, 0)]
        self.col_qs = [self.col_q]
        self.perm_columns = [(FIXED, self.col_const), (ADVICE, 0), (INSTANCE, 0)]
        self.advice_queries = [(0, 0), (0, 1), (0, 2), (0, 3)]
        self.degree = 5 if lookup else 3          # the lookup of a degree-2 input is what raises it
        self.blinding_factors = 6                 # max(3, four queries on the gate column) + 2
        self.chunk = self.degree - 2

    def _init_multi(self):
        """more than one gate column (round 4): what `builder.config(k, Some(minimum_rows))` (src/scaffold.rs:268) configures when
        the cells overflow 2^k - minimum_rows rows [RECALL halo2-base 0.3]: FlexGateConfig allocates the constants column, then
        per gate column an advice column (equality-enabled) with its own simple selector and vertical gate; RangeConfig takes the
        table column first and — there being more than one gate column — no q_lookup but num_lookup_advice lookup-advice columns
        (advice, equality-enabled, after the gate columns), one lookup argument each with the column itself as input: degree
        2 + 1 + 1 = 4, permutation sets of two, three h pieces; keygen appends one fixed column per selector (gates of different
        columns share rows: compress_selectors cannot merge them); the scaffold adds the instance column last.  num_fixed constants
        columns (config: ceil(distinct constants / 2^k)), allocated where the single one was; assign_constants deals the distinct
        constants out round-robin (constant i: column i mod num_fixed, row i div num_fixed)."""
        A, Lc, Fc = self.num_advice, self.num_lookup_advice, self.num_fixed
        assert 2 <= A <= engine.MAX_GATES and Lc <= engine.MAX_LOOKUPS, "the prover ABI takes up to 32 gate columns and 8 lookup-advice columns"
        assert Lc == 0 or self.lookup, "the Gate builder has no lookup-advice column"  # Range builder, nothing looked up: Lc = 0, no lookup argument
        assert self.k is not None, "the multi-column layout needs k (rows per column = 2^k - minimum_rows)"
        self.n_advice = A + Lc
        self.col_table, self.col_const = (0, 1) if self.lookup else (None, 0)
        self.col_qlookup = None
        self.col_consts = [self.col_const + i for i in range(Fc)]
        self.col_qs = [self.col_const + Fc + j for j in range(A)]
        self.col_q = None
        self.n_fixed = self.col_const + Fc + A
        self.fixed_queries = [(c, 0) for c in self.col_consts] + ([(self.col_table, 0)] if Lc else []) + [(c, 0) for c in self.col_qs]
        self.perm_columns = [(FIXED, c) for c in self.col_consts] + [(ADVICE, j) for j in range(A + Lc)] + [(INSTANCE, 0)]
        self.advice_queries = [(j, r) for j in range(A) for r in range(4)] + [(A + l, 0) for l in range(Lc)]
        self.degree = 4 if Lc else 3  # the lookup arguments are what raises it
        self.blinding_factors = 6
        self.chunk = self.degree - 2

    def use_logup(self, lookup_sets=None):
        """Opt in to logUp over the fixed table (H2MI_KEYGEN_LOGUP on this shape; FlexKeys(..., logup=True) calls this): the lookup-advice
        columns — or the one q_lookup * a input — become logUp arguments, in column order.  lookup_sets None: one argument per column;
        an integer K: runs of at most K columns per argument; a list: the runs themselves.  The degree follows 2 + sum of the inputs'
        degrees + 1 per argument: q_lookup * a keeps 5, K lookup-advice columns give 3 + K — which moves the
        permutation sets and the number of h pieces with it.  -> the runs"""
        n = (1 if self.lookup else 0) if self.num_advice == 1 else self.num_lookup_advice
        if n == 0:
            raise ValueError("logup=True: the constraint system has no lookup")
        if lookup_sets is None:
            runs = [1] * n
        elif isinstance(lookup_sets, int):
            if not 1 <= lookup_sets <= engine.MAX_LOGUP_INPUTS:
                raise ValueError(f"lookup_sets must be 1 .. {engine.MAX_LOGUP_INPUTS}")
            runs = [lookup_sets] * (n // lookup_sets) + ([n % lookup_sets] if n % lookup_sets else [])
        else:
            runs = [int(r) for r in lookup_sets]
            if sum(runs) != n or any(not 1 <= r <= engine.MAX_LOGUP_INPUTS for r in runs):
                raise ValueError(f"lookup_sets {runs}: runs of 1 .. {engine.MAX_LOGUP_INPUTS} columns that sum to the {n} lookup columns")
        self.logup_runs = runs
        input_degree = 2 if self.num_advice == 1 else 1
        self.degree = max(3, 2 + max(runs) * input_degree + 1)
        self.chunk = self.degree - 2
        return runs

    def abi(self, k: int) -> engine.ConstraintSystem:
        """this constraint system as the data h2mi_prover_keygen takes: one vertical gate per gate column with its selector, the
        permutation argument's columns, the lookups (single column: q_lookup * a; several: one per lookup-advice column)"""
        A = self.num_advice
        if A == 1:
            lookups = [(0, self.col_qlookup, self.col_table)] if self.lookup else []
        else:
            lookups = [(A + l, None, self.col_table) for l in range(self.num_lookup_advice)]
        return engine.ConstraintSystem.build(
            k, self.n_advice, self.n_fixed, 1, self.degree, self.blinding_factors, engine.GATES_FLEX_VERTICAL, [(j, q) for j, q in enumerate(self.col_qs)],
            [(_KIND[kind], c) for kind, c in self.perm_columns], lookups, self.advice_queries, self.fixed_queries)


def configure(lookup: bool, k: int, closure, minimum_rows: int = 9) -> FlexGateCS:
    """GateThreadBuilder::config (src/scaffold.rs:268 `builder.config(k, Some(minimum_rows))`): run the closure once to count its
    cells and cells to look up, and take ceil(count / (2^k - minimum_rows)) columns of each kind.  `closure(cs) -> Assignment`."""
    probe = FlexGateCS(lookup)
    asg = closure(probe)
    max_rows = (1 << k) - minimum_rows
    cells = len(asg.advice[0])
    num_advice = max(1, -(-cells // max_rows))
    if num_advice == 1:
        return FlexGateCS(lookup, k=k, minimum_rows=minimum_rows)
    looked_up = len(asg.fixed[probe.col_qlookup]) if lookup else 0
    num_fixed = max(1, -(-len(asg.fixed[probe.col_const]) // (1 << k)))  # `(total_fixed + (1 << k) - 1) >> k` over the distinct constants
    return FlexGateCS(lookup, num_advice, -(-looked_up // max_rows) if lookup else 0, k=k, minimum_rows=minimum_rows, num_fixed=num_fixed)


class Assignment:
    def __init__(self, cs: FlexGateCS):
        self.cs = cs
        self.advice = [dict() for _ in range(cs.n_advice)]
        self.fixed = [dict() for _ in range(cs.n_fixed)]
        self.instance = []   # public inputs (column 0)
        self.copies = []     # ((kind, column, row), (kind, column, row)) in constrain_equal order
        self.break_points = []  # rows at which a gate column ended (several gate columns only)


class Context:
    """halo2-base `Context` on one advice column [layout restated from memory]: cells are appended in program order;
    Existing(cell) re-assigns the value and constrains it equal to the original; Constant(v) cells are tied to one fixed
    cell per distinct value afterwards; `cells_to_lookup` get q_lookup enabled on their own rows (single-column form)."""

    def __init__(self, asg: Assignment):
        self.asg = asg
        self.cells, self.const_cells, self.lookup_cells = [], [], []
        self.gates, self.eqs = [], []  # rows (flat cell indices) with the gate enabled; (new cell, source cell) equalities in call order

    def load_witness(self, v: int) -> int:
        self.cells.append(v % R)
        return len(self.cells) - 1

    def assign_region_last(self, items, gate_offsets) -> int:
        """items: ("existing", cell) | ("constant", value) | ("witness", value), and for the values halo2-base computes outside the
        gates: ("hint", (kind, a, b, flags)) — hint() of cell a (or of a Constant a, with no cell beside it: a value known with the
        circuit) and of cell b or, HINT_CONST, the constant b —, ("limb", (cell, bits, shift)) — bits of a cell's canonical value —,
        ("aux", Aux) — a derived value — and ("copy", cell) — a cell's value again, the equality left to assign_region_smart"""
        base = len(self.cells)
        for kind, v in items:
            row = len(self.cells)
            if kind == "existing":
                self.cells.append(self.cells[v])
                self.eqs.append((row, v))
            elif kind == "hint":
                assert not isinstance(v[1], Aux), "a hint reads a cell or a Constant"
                self.cells.append(self.hint_value(*v))
            elif kind == "limb":
                self.cells.append((self.cells[v[0]] >> v[2]) & ((1 << v[1]) - 1))
            elif kind == "aux":
                self.cells.append(v.value)
            elif kind == "copy":
                self.cells.append(self.cells[v])
            else:
                self.cells.append(v % R)
                if kind == "constant":
                    self.const_cells.append((row, v % R))
        for off in gate_offsets:
            self.gates.append(base + off)
        return len(self.cells) - 1

    def assign_region_smart(self, items, gate_offsets, equalities) -> int:
        """assign_region_last, then constrain_equal of the listed (offset, offset) pairs of the region"""
        last = self.assign_region_last(items, gate_offsets)
        base = last + 1 - len(items)
        self.eqs += [(base + i, base + j) for i, j in equalities]
        return last

    def hint_value(self, kind, a, b, flags) -> int:
        unary = kind not in (DIVQ, DIVR)
        return hint(kind, int(a) % R if isinstance(a, Constant) else self.cells[a], 0 if unary else b % R if flags & HINT_CONST else self.cells[b], flags)

    # operands: a cell (a plain integer: its index), a Constant or an Aux
    def _v(self, q) -> int:
        return q.value if isinstance(q, Aux) else int(q) % R if isinstance(q, Constant) else self.cells[q]

    def _i(self, q):
        return ("aux", q) if isinstance(q, Aux) else ("constant", int(q)) if isinstance(q, Constant) else ("existing", q)

    def derive(self, x, y, z) -> Aux:
        """x + y * z of operands, outside the columns"""
        return Aux((self._v(x) + self._v(y) * self._v(z)) % R)

    # GateInstructions [RECALL halo2-base 0.3 gates/flex_gate.rs; the layouts are tabled in DESIGN.md 4.5]
    def mul(self, a, b):
        return self.assign_region_last([("constant", 0), self._i(a), self._i(b), ("witness", self._v(a) * self._v(b))], [0])

    def add(self, a, b):
        return self.assign_region_last([self._i(a), self._i(b), ("constant", 1), ("witness", self._v(a) + self._v(b))], [0])

    def sub(self, a, b):
        """| a - b | b | 1 | a | -> the first cell"""
        out = self.derive(a, b, Constant(-1))
        return self.assign_region_last([("aux", out), self._i(b), ("constant", 1), self._i(a)], [0]) - 3

    def neg(self, a):
        """| a | -a | 1 | 0 | -> the second cell"""
        out = self.derive(Constant(0), a, Constant(-1))
        return self.assign_region_last([self._i(a), ("aux", out), ("constant", 1), ("constant", 0)], [0]) - 2

    def mul_add(self, a, b, c):
        """| c | a | b | a * b + c |"""
        return self.assign_region_last([self._i(c), self._i(a), self._i(b), ("witness", self._v(a) * self._v(b) + self._v(c))], [0])

    def select(self, a, b, sel):
        """sel ? a : b as | a - b | 1 | b | a | b | sel | a - b | out |, gates at 0 and 4, cells 0 = 6 and 2 = 4"""
        diff = self.derive(a, b, Constant(-1))
        base = len(self.cells)
        return self.assign_region_smart([("aux", diff), ("constant", 1), self._i(b), self._i(a), self._i(b), self._i(sel), ("copy", base),
                                         ("witness", diff.value * self._v(sel) + self._v(b))], [0, 4], [(0, 6), (2, 4)])

    def not_(self, a):
        return self.sub(Constant(1), a)

    def and_(self, a, b):
        return self.mul(a, b)

    def or_(self, a, b):
        """| 1 - b | 1 | b | 1 | b | a | 1 - b | a + b - a * b |, gates at 0 and 4, cells 0 = 6 and 2 = 4"""
        not_b = self.derive(Constant(1), b, Constant(-1))
        base = len(self.cells)
        return self.assign_region_smart([("aux", not_b), ("constant", 1), self._i(b), ("constant", 1), self._i(b), self._i(a), ("copy", base),
                                         ("witness", self._v(b) + self._v(a) * not_b.value)], [0, 4], [(0, 6), (2, 4)])

    def is_zero(self, a):
        """| is_zero | a | inv | 1 | 0 | a | is_zero | 0 |: is_zero + a * inv = 1 and a * is_zero = 0, cells 0 = 6 -> cell 6.  inv is
        a^-1, or 1 for a = 0; a is a cell"""
        base = len(self.cells)
        return self.assign_region_smart([("hint", (ISZERO, a, 0, 0)), ("existing", a), ("hint", (INV, a, 0, 0)), ("constant", 1), ("constant", 0),
                                         ("existing", a), ("copy", base), ("constant", 0)], [0, 4], [(0, 6)]) - 1

    def is_equal(self, a, b):
        return self.is_zero(self.sub(a, b))

    def assert_bit(self, x):
        """| 0 | x | x | x |"""
        self.assign_region_last([("constant", 0), self._i(x), self._i(x), self._i(x)], [0])

    def assert_is_const(self, a, c: int):
        """no cell: cell a joins the constant's fixed cell"""
        self.const_cells.append((a, c % R))

    def load_constant(self, c: int) -> int:
        return self.assign_region_last([("constant", c)], [])

    def load_zero(self) -> int:
        """one cell, the first time; the same cell afterwards"""
        if getattr(self, "_zero", None) is None:
            self._zero = self.load_constant(0)
        return self._zero

    def constrain_equal(self, a, b):
        """no cell: cells a and b join one another"""
        self.eqs.append((a, b))

    def load_copy(self, cell) -> int:
        """| cell's value |, constrained equal to the cell: load_witness(*cell.value()) and constrain_equal(new, cell), for a value read
        back from a cell — which is no input, so a recorder would not know where a plain load_witness of it came from"""
        new = self.assign_region_last([("copy", cell)], [])
        self.constrain_equal(new, cell)
        return new

    def sum(self, a):
        """| a0 | a1 | 1 | a0 + a1 | a2 | 1 | a0 + a1 + a2 | ...: a gate every third cell; one operand: its cell again; none: load_zero"""
        a = list(a)
        if not a:
            return self.load_zero()
        if len(a) == 1:
            return self.assign_region_last([self._i(a[0])], [])
        acc, items = self._v(a[0]), [self._i(a[0])]
        for q in a[1:]:
            acc += self._v(q)
            items += [self._i(q), ("constant", 1), ("witness", acc)]
        return self.assign_region_last(items, [3 * i for i in range(len(a) - 1)])

    def add_constant(self, a, c):
        return self.assign_region_last([("existing", a), ("constant", c), ("constant", 1), ("witness", self.cells[a] + c)], [0])

    def mul_add_constant(self, a, b, c):
        return self.assign_region_last([("constant", c), ("existing", a), ("existing", b), ("witness", self.cells[a] * self.cells[b] + c)], [0])

    @staticmethod
    def pow_of_two() -> list:
        """the constants 2^0 .. 2^253"""
        return [Constant(1 << i) for i in range(NUM_BITS)]

    def inner_product(self, a, b):
        """| 0 | a0 | b0 | s0 | a1 | b1 | s1 | ...: a gate every third cell -> the last sum.  A b that starts with Constant(1) gives
        | a0 | a1 | b1 | s1 | ... instead: a0 is the first accumulator"""
        a, b = list(a), list(b)
        assert len(a) == len(b) and a
        if isinstance(b[0], Constant) and int(b[0]) % R == 1:
            acc, items = self._v(a[0]), [self._i(a[0])]
            a, b = a[1:], b[1:]
        else:
            acc, items = 0, [("constant", 0)]
        for x, y in zip(a, b):
            acc += self._v(x) * self._v(y)
            items += [self._i(x), self._i(y), ("witness", acc)]
        return self.assign_region_last(items, [3 * i for i in range(len(a))])

    def num_to_bits(self, a, range_bits: int) -> list:
        """the low range_bits bits of cell a, lowest first, as inner_product of the bits with pow_of_two lays them out:
        | bit0 | bit1 | 2 | acc1 | bit2 | 4 | acc2 | ..., the last sum constrained equal to a — a value beyond range_bits bits satisfies
        no such sum —, then assert_bit of every bit in order"""
        assert 1 <= range_bits <= NUM_BITS
        x, base = self.cells[a], len(self.cells)
        items = [("limb", (a, 1, 0))]
        for i in range(1, range_bits):
            items += [("limb", (a, 1, i)), ("constant", 1 << i), ("witness", x & ((2 << i) - 1))]
        acc = self.assign_region_last(items, [3 * i for i in range(range_bits - 1)])
        self.eqs.append((a, acc))
        bits = [base] + [base + 1 + 3 * (i - 1) for i in range(1, range_bits)]
        for bit in bits:
            self.assert_bit(bit)
        return bits

    def idx_to_indicator(self, idx, length: int) -> list:
        """[idx == 0, idx == 1, ..]: the first entry is is_zero unrolled — | is_zero | idx | inv | 1 | 0 | idx | is_zero | 0 |, cells
        0 = 6 and 1 = 5 —, the others is_equal(the sixth cell of that region, Constant(i)).  An index of `length` or more gives zeros only"""
        base = len(self.cells)
        self.assign_region_smart([("hint", (ISZERO, idx, 0, 0)), ("existing", idx), ("hint", (INV, idx, 0, 0)), ("constant", 1), ("constant", 0),
                                  ("existing", idx), ("copy", base), ("constant", 0)], [0, 4], [(0, 6), (1, 5)])
        return [base + 6] + [self.is_equal(base + 5, Constant(i)) for i in range(1, length)]

    def select_by_indicator(self, a, indicator):
        """| 0 | a0 | ind0 | s0 | a1 | ind1 | s1 | ...: a gate every third cell -> the last sum, the a whose indicator is 1"""
        a, indicator = list(a), list(indicator)
        assert len(a) == len(indicator) and a
        acc, items = 0, [("constant", 0)]
        for x, ind in zip(a, indicator):
            acc += self._v(x) * self.cells[ind]
            items += [self._i(x), ("existing", ind), ("witness", acc)]
        return self.assign_region_last(items, [3 * i for i in range(len(a))])

    def select_from_idx(self, cells, idx):
        """cells[idx] of operands `cells` by a cell idx; 0 for an index beyond them"""
        cells = list(cells)
        return self.select_by_indicator(cells, self.idx_to_indicator(idx, len(cells)))

    # RangeInstructions::range_check(a, range_bits)
    def range_check(self, a, range_bits: int, lookup_bits: int):
        x = self.cells[a]
        assert x < 1 << range_bits, "witness out of range"
        num_limbs = -(-range_bits // lookup_bits)
        limbs = [(x >> (lookup_bits * i)) & ((1 << lookup_bits) - 1) for i in range(num_limbs)]
        rows = [self.load_witness(limbs[0])]  # inner_product_left_last with bases[0] = 1: the first limb is the first accumulator
        acc, acc_row = limbs[0], rows[0]
        for i in range(1, num_limbs):  # [acc, limb_i, 2^(b i), acc'] sharing the accumulator cell: a gate every third row
            base = len(self.cells) - 1
            acc += limbs[i] << (lookup_bits * i)
            self.cells.append(limbs[i])
            rows.append(len(self.cells) - 1)
            self.cells.append((1 << (lookup_bits * i)) % R)
            self.const_cells.append((len(self.cells) - 1, (1 << (lookup_bits * i)) % R))
            self.cells.append(acc % R)
            self.gates.append(base)
            acc_row = len(self.cells) - 1
        self.eqs.append((a, acc_row))  # ctx.constrain_equal(&a, &acc)
        self.lookup_cells += rows
        rem = range_bits % lookup_bits
        if rem == 1:  # the top limb is one bit: assert_bit, 0 + x * x - x = 0 on [0, x, x, x]
            self.assign_region_last([("constant", 0), ("existing", rows[-1]), ("existing", rows[-1]), ("existing", rows[-1])], [0])
        elif rem:  # the top limb times 2^(lookup_bits - rem) must be in the table too
            self.lookup_cells.append(self.assign_region_last([("constant", 0), ("existing", rows[-1]), ("constant", 1 << (lookup_bits - rem)),
                                                              ("witness", limbs[-1] << (lookup_bits - rem))], [0]))

    # RangeInstructions [RECALL halo2-base 0.3 gates/range.rs]; the limbs are of self.lookup_bits bits (the scaffold sets it)
    def _shifted(self, a, b, bits: int) -> int:
        """| a + 2^bits - b | b | 1 | a + 2^bits | -2^bits | 1 | a |, gates at 0 and 3 -> the first cell"""
        shift_a = self.derive(a, Constant(1 << bits), Constant(1))
        shifted = self.derive(shift_a, b, Constant(-1))
        return self.assign_region_last([("aux", shifted), self._i(b), ("constant", 1), ("witness", shift_a.value), ("constant", -(1 << bits)),
                                        ("constant", 1), self._i(a)], [0, 3]) - 6

    def check_less_than(self, a, b, num_bits: int):
        """a < b for a, b below 2^num_bits: a + 2^num_bits - b is range-checked to num_bits bits"""
        self.range_check(self._shifted(a, b, num_bits), num_bits, self.lookup_bits)

    def check_big_less_than_safe(self, a, b: int):
        """a < b for a cell a and an integer b: range_check to b's bit length rounded up to whole limbs, then check_less_than"""
        range_bits = -(-b.bit_length() // self.lookup_bits) * self.lookup_bits
        self.range_check(a, range_bits, self.lookup_bits)
        self.check_less_than(a, Constant(b), range_bits)

    def is_less_than(self, a, b, num_bits: int) -> int:
        """the bit a < b for a, b below 2^num_bits: a + 2^padded - b is range-checked to one limb more than padded bits, and that top limb
        (the last cell to look up) is zero exactly when a < b"""
        padded = -(-num_bits // self.lookup_bits) * self.lookup_bits
        self.range_check(self._shifted(a, b, padded), padded + self.lookup_bits, self.lookup_bits)
        return self.is_zero(self.lookup_cells[-1])

    def is_less_than_safe(self, a, b: int) -> int:
        """the bit a < b for a cell a and an integer b: range_check to b's bit length rounded up to whole limbs, then is_less_than
        against the constant"""
        range_bits = -(-b.bit_length() // self.lookup_bits) * self.lookup_bits
        self.range_check(a, range_bits, self.lookup_bits)
        return self.is_less_than(a, Constant(b), range_bits)

    def div_mod(self, a, b: int, a_num_bits: int):
        """(a div b, a mod b) for a cell a below 2^a_num_bits and an integer b: | rem | b | div | a |, then div < 2^a_num_bits / b + 1 and
        rem < b"""
        last = self.assign_region_last([("hint", (DIVR, a, b, HINT_CONST)), ("constant", b), ("hint", (DIVQ, a, b, HINT_CONST)), self._i(a)], [0])
        rem, div = last - 3, last - 1
        self.check_big_less_than_safe(div, (1 << a_num_bits) // b + 1)
        self.check_big_less_than_safe(rem, b)
        return div, rem

    def div_mod_var(self, a, b, a_num_bits: int, b_num_bits: int):
        """the same by a cell b below 2^b_num_bits (or a Constant b: the hints then take it as their constant divisor): div is
        range-checked to a_num_bits bits, rem < b.  b = 0 satisfies nothing"""
        by = (int(b) % R, HINT_CONST) if isinstance(b, Constant) else (b, 0)
        last = self.assign_region_last([("hint", (DIVR, a) + by), self._i(b), ("hint", (DIVQ, a) + by), self._i(a)], [0])
        rem, div = last - 3, last - 1
        self.range_check(div, a_num_bits, self.lookup_bits)
        self.check_less_than(rem, b, b_num_bits)
        return div, rem

    def finish(self, public_rows):
        asg = self.asg
        cs = asg.cs
        if cs.num_advice > 1:
            return self._finish_multi(public_rows)
        asg.advice[0] = dict(enumerate(self.cells))
        for g in self.gates:
            asg.fixed[cs.col_q][g] = 1
        asg.copies += [((ADVICE, 0, new), (ADVICE, 0, src)) for new, src in self.eqs]
        consts = {}
        for row, v in self.const_cells:  # assign_constants: one fixed cell per distinct value, in order of first use
            if v not in consts:
                consts[v] = len(consts)
                asg.fixed[cs.col_const][consts[v]] = v
            asg.copies.append(((ADVICE, 0, row), (FIXED, cs.col_const, consts[v])))
        for row in self.lookup_cells:
            asg.fixed[cs.col_qlookup][row] = 1
        for i, row in enumerate(public_rows):  # layouter.constrain_instance(cell, instance, i): src/scaffold.rs:411, 480
            asg.instance.append(self.cells[row])
            asg.copies.append(((ADVICE, 0, row), (INSTANCE, 0, i)))

    def _finish_multi(self, public_rows):
        """assign_all over several gate columns [RECALL halo2-base 0.3 gates/builder.rs]: the cells run down the current column; a
        cell that lands on the column's last row (row >= max_rows - 1), or that starts a gate which no longer fits (row + 4 >
        max_rows), is assigned a second time at row 0 of the next column and tied to its first copy — two gates may overlap at it —
        and a gate starting there is enabled on the new column.  The cells to look up are copied into the lookup-advice columns.
        constrain_equal order: break copies as they occur, lookup copies, the closure's equalities, constants, public cells."""
        asg = self.asg
        cs = asg.cs
        A, Lc = cs.num_advice, cs.num_lookup_advice
        max_rows = (1 << cs.k) - cs.minimum_rows
        gate_at = set(self.gates)
        where = []  # flat cell index -> (column, row) of its first copy
        col, row = 0, 0
        for i, v in enumerate(self.cells):
            asg.advice[col][row] = v
            where.append((col, row))
            q = i in gate_at
            if (q and row + 4 > max_rows) or row >= max_rows - 1:
                if col + 1 >= A:
                    raise ValueError(f"NOT ENOUGH ADVICE COLUMNS: more than {A} gate columns needed at 2^{cs.k} rows")
                asg.copies.append(((ADVICE, col + 1, 0), (ADVICE, col, row)))
                asg.break_points.append(row)  # what scaffold::gen_key returns next to the proving key (phase 0)
                col, row = col + 1, 0
                asg.advice[col][0] = v
            if q:
                asg.fixed[cs.col_qs[col]][row] = 1
            row += 1
        cell = lambda i: (ADVICE,) + where[i]
        lcol, lrow = 0, 0
        for i in self.lookup_cells:
            if lrow >= max_rows:
                lcol, lrow = lcol + 1, 0
            if lcol >= Lc:
                raise ValueError("NOT ENOUGH LOOKUP ADVICE COLUMNS")
            asg.advice[A + lcol][lrow] = self.cells[i]
            asg.copies.append((cell(i), (ADVICE, A + lcol, lrow)))
            lrow += 1
        asg.copies += [(cell(new), cell(src)) for new, src in self.eqs]
        consts, Fc = {}, cs.num_fixed
        for r, v in self.const_cells:
            if v not in consts:
                consts[v] = len(consts)
                asg.fixed[cs.col_consts[consts[v] % Fc]][consts[v] // Fc] = v
            asg.copies.append((cell(r), (FIXED, cs.col_consts[consts[v] % Fc], consts[v] // Fc)))
        for i, r in enumerate(public_rows):
            asg.instance.append(self.cells[r])
            asg.copies.append((cell(r), (INSTANCE, 0, i)))


def halo2_lib_closure(cs: FlexGateCS, x: int) -> Assignment:
    """reference examples/halo2_lib.rs:14-60 `some_algorithm_in_zk`: x^2 + 72 three ways; make_public = [x, out]"""
    asg = Assignment(cs)
    ctx = Context(asg)
    xc = ctx.load_witness(x)
    x_sq = ctx.mul(xc, xc)
    out = ctx.add_constant(x_sq, 72)
    ctx.assign_region_last([("constant", 72), ("existing", xc), ("existing", xc), ("witness", x * x + 72)], [0])
    ctx.mul_add_constant(xc, xc, 72)
    ctx.finish([xc, out])
    return asg


RANGE_MANY_STEP = 0x9E3779B97F4A7C15


def range_closure(cs: FlexGateCS, x: int, lookup_bits: int, count: int = 1) -> Assignment:
    """reference examples/range.rs:10-34: make_public = [x]; range_check(x, 64); x + x.  The table column is what
    RangeConfig::load_lookup_table assigns: 0 .. 2^LOOKUP_BITS - 1 (src/scaffold.rs:462).  count > 1: the same body for
    x, x + step, x + 2 step, ... (mod 2^64) in ONE context, every value public — a circuit that fills several gate and
    lookup-advice columns while the limb bases, shared by all the checks, still fit the one constants column."""
    asg = Assignment(cs)
    ctx = Context(asg)
    public = []
    for i in range(count):
        xc = ctx.load_witness((x + i * RANGE_MANY_STEP) & ((1 << 64) - 1))
        ctx.range_check(xc, 64, lookup_bits)
        ctx.add(xc, xc)
        public.append(xc)
    ctx.finish(public)
    return load_lookup_table(asg, lookup_bits)


def load_lookup_table(asg: Assignment, lookup_bits: int) -> Assignment:
    """RangeConfig::load_lookup_table (src/scaffold.rs:462): the Range builder's synthesize assigns 0 .. 2^LOOKUP_BITS - 1 to the table
    column whatever the closure does — also for a closure that looks nothing up (the reference picks the Range builder whenever
    LOOKUP_BITS is set: src/scaffold.rs:44-48)."""
    assert asg.cs.lookup, "the Gate builder has no table column"
    asg.fixed[asg.cs.col_table] = None  # dense: filled by keygen from `table_values`
    asg.table_values = list(range(1 << lookup_bits))
    return asg


def mock(asg: Assignment, k: int = None) -> None:
    """scaffold::mock (src/scaffold.rs:205-243: MockProver::run(..).assert_satisfied()) for these constraint systems, on the
    host: every enabled row satisfies the vertical gate, every copy constraint joins equal cells, every looked-up cell is
    a table value.  Raises ValueError naming the first violation — what the reference's users run before `prove`.  With the
    DEGREE known (k, or the constraint system's own for the multi-column layouts) cells beyond the usable rows are refused as
    MockProver::run refuses them (NotEnoughRowsAvailable) — the same rule h2mi_prover_keygen applies."""
    cs = asg.cs
    k = k if k is not None else cs.k
    if k is not None:
        u = (1 << k) - (cs.blinding_factors + 1)
        rows = [(f"fixed column {c}", max(cells)) for c, cells in enumerate(asg.fixed) if cells]
        rows += [(f"advice column {c}", max(cells)) for c, cells in enumerate(asg.advice) if cells]
        rows += [("a copy constraint", max(left[2], right[2])) for left, right in asg.copies]
        if cs.lookup:
            rows.append(("the lookup table", len(asg.table_values) - 1))
        for what, row in rows:
            if row >= u:
                raise ValueError(f"NotEnoughRowsAvailable: {what} reaches row {row}, the usable rows end at {u}")
    for j, cq in enumerate(cs.col_qs):  # gate column j with its own selector
        a = asg.advice[j]
        for r in sorted(asg.fixed[cq]):
            if (a.get(r, 0) + a.get(r + 1, 0) * a.get(r + 2, 0) - a.get(r + 3, 0)) % R:
                raise ValueError(f"gate not satisfied at row {r}" + (f" of column {j}" if len(cs.col_qs) > 1 else ""))
    value = {ADVICE: lambda c, r: asg.advice[c].get(r, 0), FIXED: lambda c, r: asg.fixed[c].get(r, 0),
             INSTANCE: lambda c, r: asg.instance[r] if r < len(asg.instance) else 0}
    for left, right in asg.copies:
        if value[left[0]](left[1], left[2]) % R != value[right[0]](right[1], right[2]) % R:
            raise ValueError(f"copy constraint {left} == {right} not satisfied")
    if cs.lookup:
        table = set(v % R for v in asg.table_values) | {0}
        if cs.num_advice == 1:
            looked_up = [(r, asg.advice[0].get(r, 0)) for r in sorted(asg.fixed[cs.col_qlookup])]
        else:
            looked_up = [(r, v) for l in range(cs.num_lookup_advice) for r, v in sorted(asg.advice[cs.num_advice + l].items())]
        for r, v in looked_up:
            if v % R not in table:
                raise ValueError(f"lookup not satisfied at row {r}")


# ---- keys ------------------------------------------------------------------------------------------------------------
class FlexKeys:
    """keygen_vk + keygen_pk (src/scaffold.rs:284,287) through h2mi_prover_keygen: the fixed cells of a run of the closure (the
    lookup table dense), the copy constraints with their columns renumbered into the permutation argument's order; the library
    builds the sigma polynomials (Assembly::copy over advice, constants and instance cells alike), l_0 / l_last / l_active, the
    lookup table's sorted form and the verifying key's commitments.  by_coset=True (H2MI_KEYGEN_BY_COSET): no extended-coset column
    on the device, the quotient one coset at a time — the same proof bytes; `fixed_cosets` / `sigma_cosets` are then refused."""

    def __init__(self, params: ParamsKZG, cs: FlexGateCS, asg: Assignment, by_coset: bool = False, logup: bool = False, lookup_sets=None):
        self.cs = cs
        self.by_coset = bool(by_coset)
        # logup=True (H2MI_KEYGEN_LOGUP on a hard-wired shape): the lookups are proven with multiplicities and a running sum against the key's sorted
        # table, lookup_sets columns per argument (FlexGateCS.use_logup, which also moves cs.degree); no by-coset form, no key file
        self.logup = bool(logup)
        if lookup_sets is not None and not logup:
            raise ValueError("lookup_sets groups the columns of a logUp key: FlexKeys(..., logup=True)")
        self.logup_inputs = engine.LogupInputs.build(cs.use_logup(lookup_sets)) if logup else None
        k = params.k
        self.domain = d = EvaluationDomain(cs.degree, k)
        self.u = u = d.n - (cs.blinding_factors + 1)
        fixed_cells = list(asg.fixed)
        if cs.lookup:
            tv = asg.table_values
            if len(tv) > u:
                raise ValueError(f"lookup table of {len(tv)} rows does not fit the {u} usable rows of a 2^{k} circuit (LOOKUP_BITS must be below DEGREE)")
            fixed_cells[cs.col_table] = [v % R for v in tv]  # dense: rows 0 .. len - 1
        index = {col: j for j, col in enumerate(cs.perm_columns)}
        copies = [(index[(left[0], left[1])], left[2], index[(right[0], right[1])], right[2]) for left, right in asg.copies]
        self.keys = engine.Keys(cs.abi(k), params, fixed_cells, copies, by_coset=by_coset, logup=logup, logup_inputs=self.logup_inputs)
        self._finish(k)

    def _finish(self, k: int):
        """what the key shows of its engine.Keys, however that was made"""
        cs = self.cs
        self.fixed_commitments, self.permutation_commitments = self.keys.fixed_commitments, self.keys.permutation_commitments
        # read-only views of the key's library-owned vectors (Lagrange / coefficient / extended-coset forms), for callers that check them
        nf, m = cs.n_fixed, len(cs.perm_columns)
        self.fixed_values, self.fixed_polys, self.fixed_cosets = (self.keys.views(kd, nf) for kd in (engine.PKBUF_FIXED, engine.PKBUF_FIXED_POLY, engine.PKBUF_FIXED_COSET))
        self.sigma_values, self.sigma_polys, self.sigma_cosets = (self.keys.views(kd, m) for kd in (engine.PKBUF_SIGMA, engine.PKBUF_SIGMA_POLY, engine.PKBUF_SIGMA_COSET))
        self._vk_bytes, self.transcript_repr = transcript_repr(k, cs.degree, self.fixed_commitments, self.permutation_commitments)

    def vk_bytes(self) -> bytes:
        return self._vk_bytes

    def release(self):
        self.keys.release()

    def save(self, path_or_file, user: bytes = b"") -> int:
        """the key as a file (engine.Keys.save: h2mi_prover_pk_export) -> the bytes written.  The builder's parameters — lookup, the
        column counts, k, minimum_rows, num_fixed — travel in the file's user section, in front of the caller's `user` bytes (the
        scaffold's break points): a 32-bit length, that many bytes of JSON, then `user`."""
        cs = self.cs
        head = json.dumps({"lookup": bool(cs.lookup), "num_advice": cs.num_advice, "num_lookup_advice": cs.num_lookup_advice, "k": self.domain.k,
                           "minimum_rows": cs.minimum_rows, "num_fixed": cs.num_fixed}, sort_keys=True).encode()
        return self.keys.save(path_or_file, len(head).to_bytes(4, "little") + head + bytes(user))

    @classmethod
    def load(cls, params: ParamsKZG, path_or_file, by_coset: bool = False) -> "FlexKeys":
        """the key of a file written by save(), without the closure: the builder's constraint system is rebuilt from the parameters in
        the user section and must be the file's own (ValueError otherwise).  `user` holds the caller's bytes."""
        blob = path_or_file.read() if hasattr(path_or_file, "read") else open(path_or_file, "rb").read()
        _, user = engine.blob_check(blob)
        n = int.from_bytes(user[:4], "little")
        if len(user) < 4 or len(user) < 4 + n:
            raise ValueError("key file: no builder parameters in its user section (not written by FlexKeys.save)")
        p = json.loads(user[4:4 + n].decode())
        if p["k"] != params.k:
            raise ValueError(f"key file: made for 2^{p['k']} rows, the SRS has 2^{params.k}")
        cs = FlexGateCS(p["lookup"], p["num_advice"], p["num_lookup_advice"], k=p["k"], minimum_rows=p["minimum_rows"], num_fixed=p["num_fixed"])
        if engine.blob_sections(blob, 1) != engine.key_blob_head(cs.abi(params.k))[:1]:
            raise ValueError("key file: its constraint system is not the one its builder parameters give")
        self = cls.__new__(cls)
        self.cs, self.by_coset = cs, bool(by_coset)
        self.domain = d = EvaluationDomain(cs.degree, params.k)
        self.u = d.n - (cs.blinding_factors + 1)
        self.keys = engine.Keys.from_blob(params, blob, by_coset)
        self.user = user[4 + n:]
        self._finish(params.k)
        return self


# ---- create_proof --------------------------------------------------------------------------------------------------------
class FlexWorkspace:
    """one library prover (device buffers, streams) kept for the next proof against the same proving key (the reference's drivers
    prove repeatedly against one pk / SRS, e.g. examples/linear_regression.rs:126-195).
    combiner: a dist.PhaseCombiner with >= 8 slots when `params` is one rank's slice of the SRS (one process per GPU): every
    commitment is then this rank's partial point, combined across ranks at every transcript write."""

    def __init__(self, params: ParamsKZG, pk: "FlexKeys", combiner=None):
        self.combiner = combiner
        self.prover = engine.Prover(pk.keys, params, combiner=combiner)

    def release(self):
        self.prover.release()


def create_proof(params: ParamsKZG, pk: FlexKeys, asg: Assignment, seed: int, transcript: Blake2bWrite = None, trace: dict = None,
                 ws: FlexWorkspace = None, multiopen: str = "shplonk") -> bytes:
    """create_proof for one circuit with one instance column: scaffold::prove's call (src/scaffold.rs:322-331,
    `&[&[&public_io]]`).  `params` is the whole SRS, or one rank's slice of it together with ws.combiner.  Without `ws` the
    device buffers live for this call only (released on every exit path).  multiopen: "shplonk" or "gwc" (engine.Prover.drive)."""
    engine.check_multiopen(multiopen)
    own = ws is None
    ws = ws or FlexWorkspace(params, pk)
    try:
        transcript = transcript or Blake2bWrite.init()
        transcript.common_scalar(_m(pk.transcript_repr))
        for v in engine.instance_values(asg.instance):  # KZG: the public inputs are hashed as scalars, not committed; column by column
            transcript.common_scalar(_m(v))
        ws.prover.drive(asg.advice, asg.instance, seed, transcript, trace, multiopen=multiopen)
        return transcript.finalize()
    finally:
        if own:
            ws.release()


def device_check(params: ParamsKZG, pk, asg, seed: int = 1, ws: FlexWorkspace = None, trace: dict = None) -> list:
    """the witness check of include/h2mi_prover.h (h2mi_prover_check) on a proof that is started exactly as create_proof starts it
    — the transcript, the advice phase(s), theta — and dropped behind the check: -> [engine.CheckFailure], empty for a witness that
    satisfies the circuit.  What `mock` answers on the host, at the sizes the prover runs at; the advice commitments are paid."""
    own = ws is None
    ws = ws or FlexWorkspace(params, pk)
    try:
        transcript = Blake2bWrite.init()
        transcript.common_scalar(_m(pk.transcript_repr))
        for v in engine.instance_values(asg.instance):
            transcript.common_scalar(_m(v))
        return ws.prover.drive(asg.advice, asg.instance, seed, transcript, trace, witness_check="only")
    finally:
        if own:
            ws.release()


def check(params: ParamsKZG, pk: FlexKeys, asg: Assignment, seed: int = 1, ws: FlexWorkspace = None, trace: dict = None) -> None:
    """`mock` on the device: raises ValueError in mock's words for the first violation (gates by gate column, then copy constraints,
    then lookups), with the number of rows or cells that fail; the whole report is the exception's `failures`"""
    failures = device_check(params, pk, asg, seed, ws, trace)
    cs = pk.cs
    for f in failures:
        if f.kind == engine.CHECK_GATE:
            msg = f"gate not satisfied at row {f.row}" + (f" of column {f.index}" if len(cs.col_qs) > 1 else "") + f" ({f.count} rows)"
        elif f.kind == engine.CHECK_COPY:
            kind, column = cs.perm_columns[f.index]
            msg = f"copy constraint at cell {(kind, column, f.row)} not satisfied ({f.count} cells differ from their copy)"
        else:
            msg = f"lookup not satisfied at row {f.row}" + (f" of lookup column {f.index}" if cs.num_lookup_advice > 1 else "") + f" ({f.count} rows)"
        e = ValueError(msg)
        e.failures = failures
        raise e
