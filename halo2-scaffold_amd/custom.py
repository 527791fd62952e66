"""Circuits with hand-written gates: halo2's `ConstraintSystem` API, name for name, in front of the library's prover.

The reference's src/circuits/is_zero.rs and or.rs configure their circuits with `meta.create_gate("...", |meta| vec![...])` over
`meta.query_advice(column, Rotation)` expressions.  This module is that API — `ConstraintSystem.advice_column / fixed_column /
instance_column / selector / enable_equality / create_gate / lookup / lookup_any`, `Expression` with + - * and `Expression.constant` — so that such a
configure() can be transcribed line by line, and the region API of synthesize() (`Assignment.assign_advice / assign_fixed /
enable_selector / constrain_equal / constrain_instance`).  `ConstraintSystem.program()` compiles the gate polynomials to the postfix
program of include/h2mi.h (h2mi_gate_program), `abi(k)` gives the constraint system as data with gates = H2MI_GATES_EXPRESSIONS;
`Keys` and `create_proof` are thin calls into libh2mi.so exactly as flex.FlexKeys / flex.create_proof are: one kernel interprets the
program on the extended coset (csrc/h2mi_plonk.hip k_evaluate_h_expr), everything else is the prover every other shape uses.

halo2's bookkeeping, restated from memory [RECALL halo2_proofs plonk/circuit.rs]:
  * enable_equality queries its column at Rotation::cur when it is called; query lists are in first-use order;
  * blinding_factors = max(3, most queries on one advice column) + 2;  degree = max(3, gate degrees, per lookup
    max(4, 2 + max(1, input degrees) + max(1, table degrees)));
  * every selector becomes ONE fixed column, appended after the user's fixed columns in selector order and queried last.  The crate's
    compress_selectors, which merges disjoint simple selectors into one column, is NOT modelled: a circuit whose selectors the crate
    would merge gets one column more here than there (and other proof bytes).  The C ABI sees expressions after the substitution
    and does not care.
Lookups: `meta.lookup(name, |meta| vec![(input, table), ..])` and `lookup_any` take any expressions on both sides (the crate's `lookup`
wants its table side to be TableColumn queries; here both spell the same argument).  `lookup_program()` compiles them to an
h2mi_lookup_program and `Keys` hands it to keygen beside the gates: each side is compressed with theta and the table sorted inside
every proof (csrc/h2mi_lookup.hip h2mi_fr_sort_unique_dev).  The single-expression lookups against a fixed table, sorted once at
keygen, stay the fast path of range checks and are reached through flex.py.
Phases and challenges [RECALL halo2_proofs v2023_02_02 plonk/circuit.rs, plonk/prover.rs]: `advice_column_in(phase)` (phases 0 .. 2; a
later phase needs a column in the one before), `challenge_usable_after(phase)` (needs a column in that phase; numbered in creation
order), `query_challenge` -> an Expression of degree 0 that any gate and either side of any lookup may hold.  `Keys` then passes an
h2mi_advice_phases, and `create_proof` takes synthesize(challenges) -> Assignment in place of an Assignment: it is called once
per advice phase with the challenges squeezed so far, and only that phase's columns are taken from what it returns.
Shuffles [RECALL halo2_proofs, PSE line, plonk/shuffle.rs — restated from memory and pinned to DESIGN.md 4.5, not to the crate]:
`meta.shuffle(name, |meta| vec![(input, shuffle), ..])` states that the two tuples take the same multiset of values over the usable
rows; required degree 2 + max(1, input degrees, shuffle degrees).  `shuffle_program()` compiles them to an h2mi_shuffle_program and
`Keys` passes it to keygen — only a circuit that has shuffles passes one.
Merged lookups [RECALL the `mv-lookup` line's merging of lookups over one table — restated from memory and pinned to DESIGN.md 4.5 and
tests/logup_sets_cases.py]: `merge_lookups(max_degree=None)` is an explicit opt-in that turns the lookups sharing a table into ONE logUp
argument of several input sets (h2mi_logup_inputs); `Keys(..., logup=True)` then passes the counts to keygen.
Assigned cells [RECALL halo2_proofs v2023_02_02 plonk/assigned.rs]: `assign_advice` / `assign_fixed` take `Rational(numerator,
denominator)` beside integers — `value.invert()` deferred to the prover, as the reference's is_zero.rs computes value_inv.  Such a
column crosses to the library unresolved (engine.pack_cells, H2MI_CELLS_RATIONAL) and is inverted there; `mock` evaluates it.
`mock` is MockProver::run(..).assert_satisfied() on the host, row by row in Python integers; `check` asks the same question of the
device, at the sizes the prover runs at (h2mi_prover_check: gates, copy constraints and lookups on the columns of a proof in flight).
"""
from . import engine, flex
from . import field as F
from .domain import EvaluationDomain
from .keygen import transcript_repr
from .params import ParamsKZG

R = F.FR_MODULUS
ADVICE, FIXED, INSTANCE = flex.ADVICE, flex.FIXED, flex.INSTANCE
_KIND = {ADVICE: engine.ADVICE, FIXED: engine.FIXED, INSTANCE: engine.INSTANCE}
_OP = {"add": engine.EXPR_ADD, "sub": engine.EXPR_SUB, "mul": engine.EXPR_MUL}


class Rotation(int):
    """poly::Rotation: a row offset"""

    @classmethod
    def cur(cls):
        return cls(0)

    @classmethod
    def next(cls):
        return cls(1)

    @classmethod
    def prev(cls):
        return cls(-1)


class Column:
    def __init__(self, kind: str, index: int):
        self.kind, self.index = kind, index

    def __repr__(self):
        return f"Column({self.kind}, {self.index})"


class Selector:
    def __init__(self, index: int):
        self.index = index


class Challenge:
    """plonk::Challenge: its index (creation order) and the phase after which the transcript yields it"""

    def __init__(self, index: int, phase: int):
        self.index, self.phase = index, phase


Rational = engine.Rational  # Assigned::Rational(numerator, denominator): a cell whose inversion is left to the prover


def _assigned(value):
    """a value as a column keeps it: an integer reduced modulo r, or the Rational as it is (Assigned<F>)"""
    return value if isinstance(value, Rational) else value % R


def _evaluated(value) -> int:
    """Assigned::evaluate"""
    return value.evaluate() if isinstance(value, Rational) else value


class Cell:
    """AssignedCell: `value` is what was assigned — an integer, or a Rational (copy_advice copies a rational as a rational)"""

    def __init__(self, kind: str, column: int, row: int, value):
        self.kind, self.column, self.row, self.value = kind, column, row, value


class Expression:
    """plonk::Expression<F>: a polynomial over column queries.  node: ("constant", v) | ("query", kind, column, rotation) |
    ("selector", index) | ("challenge", index) | ("neg", e) | ("add" | "sub" | "mul", a, b).  A selector stays symbolic until the constraint system knows how
    many fixed columns the user took (`resolve`)."""

    def __init__(self, *node):
        self.node = node
        self._depth = None  # stack_depth(), computed once: a node never changes, and a long sum would otherwise cost 2^terms

    @staticmethod
    def constant(v: int) -> "Expression":
        return Expression("constant", v % R)

    @staticmethod
    def _wrap(v) -> "Expression":
        return v if isinstance(v, Expression) else Expression.constant(v)

    def __add__(self, o):
        return Expression("add", self, Expression._wrap(o))

    def __radd__(self, o):
        return Expression("add", Expression._wrap(o), self)

    def __sub__(self, o):
        return Expression("sub", self, Expression._wrap(o))

    def __rsub__(self, o):
        return Expression("sub", Expression._wrap(o), self)

    def __mul__(self, o):
        return Expression("mul", self, Expression._wrap(o))

    def __rmul__(self, o):
        return Expression("mul", Expression._wrap(o), self)

    def __neg__(self):
        return Expression("neg", self)

    def clone(self):
        return self

    def key(self):
        """the expression's structure as nested tuples: two expressions are structurally equal when their keys are"""
        return tuple(e.key() if isinstance(e, Expression) else e for e in self.node)

    def resolve(self, first_selector_column: int) -> "Expression":
        """the expression keygen sees: every selector replaced by the query of its fixed column"""
        t = self.node[0]
        if t == "selector":
            return Expression("query", FIXED, first_selector_column + self.node[1], 0)
        if t in ("constant", "query", "challenge"):
            return self
        return Expression(t, *[e.resolve(first_selector_column) for e in self.node[1:]])

    def degree(self) -> int:
        t = self.node[0]
        if t in ("constant", "challenge"):
            return 0
        if t in ("query", "selector"):
            return 1
        if t == "neg":
            return self.node[1].degree()
        a, b = self.node[1].degree(), self.node[2].degree()
        return a + b if t == "mul" else max(a, b)

    def stack_depth(self) -> int:
        """operand-stack depth of the postfix `program()` emits"""
        if self._depth is None:
            t = self.node[0]
            if t in ("constant", "query", "selector", "challenge"):
                self._depth = 1
            elif t == "neg":
                self._depth = self.node[1].stack_depth()
            else:
                first, second = self._order()
                self._depth = max(first.stack_depth(), 1 + second.stack_depth())
        return self._depth

    def _order(self):
        """operands in emission order: ADD and MUL commute, so the deeper operand goes first (it runs on an empty stack, the
        shallower one on top of its result); SUB keeps its order"""
        a, b = self.node[1], self.node[2]
        if self.node[0] != "sub" and b.stack_depth() > a.stack_depth():
            return b, a
        return a, b

    def evaluate(self, q, challenges=()) -> int:
        """the value with q(kind, column, rotation) for the queries (selectors resolved) and challenges[i] for challenge i"""
        t = self.node[0]
        if t == "constant":
            return self.node[1]
        if t == "query":
            return q(*self.node[1:]) % R
        if t == "challenge":
            return challenges[self.node[1]] % R
        if t == "neg":
            return -self.node[1].evaluate(q, challenges) % R
        a, b = self.node[1].evaluate(q, challenges), self.node[2].evaluate(q, challenges)
        return (a + b if t == "add" else a - b if t == "sub" else a * b) % R

    def _emit(self, ops, constants):
        t = self.node[0]
        if t == "constant":
            if self.node[1] not in constants:
                constants[self.node[1]] = len(constants)
            ops.append((engine.EXPR_CONSTANT, constants[self.node[1]], 0))
        elif t == "query":
            ops.append((_KIND[self.node[1]], self.node[2], int(self.node[3])))
        elif t == "challenge":
            ops.append((engine.EXPR_CHALLENGE, self.node[1], 0))
        elif t == "neg":
            self.node[1]._emit(ops, constants)
            ops.append((engine.EXPR_NEG, 0, 0))
        elif t == "selector":
            raise ValueError("resolve() the selectors before compiling")
        else:
            first, second = self._order()
            first._emit(ops, constants)
            second._emit(ops, constants)
            ops.append((_OP[t], 0, 0))

    def program(self, constants: dict = None):
        """the postfix compiler: -> (ops [(op, index, rotation)] closed by END, constants [int]).  `constants`: a {value: index} table
        shared by the polynomials of one constraint system."""
        constants = {} if constants is None else constants
        ops = []
        self._emit(ops, constants)
        ops.append((engine.EXPR_END, 0, 0))
        return ops, sorted(constants, key=constants.get)


class ConstraintSystem:
    """plonk::ConstraintSystem<F> as configure() fills it"""

    def __init__(self):
        self.n_advice = self.n_user_fixed = self.n_instance = self.n_selectors = 0
        self.perm_columns = []                      # [(kind, column)] in enable_equality order
        self.advice_queries, self._fixed_queries, self.instance_queries = [], [], []
        self.gate_names, self._polys = [], []       # one entry per polynomial, selectors unresolved
        self.lookup_names, self._lookups = [], []   # per lookup [(input, table)] expressions, selectors unresolved
        self.shuffle_names, self._shuffles = [], []  # per shuffle [(input, shuffle)] expressions, selectors unresolved
        self.advice_phase, self.challenge_phase = [], []  # per advice column its phase; per challenge the phase it is usable after
        self._merged = None  # merge_lookups(): per lookup ARGUMENT the indices of the declared lookups it proves; None: one each

    # ---- columns -----------------------------------------------------------------------------------------------------
    def advice_column(self) -> Column:
        return self.advice_column_in(0)

    def advice_column_in(self, phase: int) -> Column:
        """meta.advice_column_in(FirstPhase | SecondPhase | ThirdPhase) with the crate's assertion [RECALL plonk/circuit.rs]: a later
        phase needs an advice column in the phase before it"""
        assert 0 <= phase < engine.MAX_ADVICE_PHASES, "phases are 0, 1, 2"
        assert phase == 0 or phase - 1 in self.advice_phase, f"no advice column in phase {phase - 1} yet"
        self.n_advice += 1
        self.advice_phase.append(phase)
        return Column(ADVICE, self.n_advice - 1)

    def challenge_usable_after(self, phase: int) -> Challenge:
        """meta.challenge_usable_after(phase), with the crate's assertion: the phase holds an advice column"""
        assert phase in self.advice_phase, f"no advice column in phase {phase}: nothing the challenge could depend on"
        self.challenge_phase.append(phase)
        return Challenge(len(self.challenge_phase) - 1, phase)

    def fixed_column(self) -> Column:
        self.n_user_fixed += 1
        return Column(FIXED, self.n_user_fixed - 1)

    def instance_column(self) -> Column:
        self.n_instance += 1
        return Column(INSTANCE, self.n_instance - 1)

    def selector(self) -> Selector:
        self.n_selectors += 1
        return Selector(self.n_selectors - 1)

    def enable_equality(self, column: Column) -> None:
        self._query(column, 0)
        if (column.kind, column.index) not in self.perm_columns:
            self.perm_columns.append((column.kind, column.index))

    # ---- gates (the closure receives this object as `meta`: VirtualCells) ---------------------------------------------
    def _query(self, column: Column, rotation: int) -> Expression:
        lst = {ADVICE: self.advice_queries, FIXED: self._fixed_queries, INSTANCE: self.instance_queries}[column.kind]
        if (column.index, int(rotation)) not in lst:
            lst.append((column.index, int(rotation)))
        return Expression("query", column.kind, column.index, int(rotation))

    def query_advice(self, column: Column, rotation: int) -> Expression:
        assert column.kind == ADVICE
        return self._query(column, rotation)

    def query_fixed(self, column: Column, rotation: int = 0) -> Expression:
        assert column.kind == FIXED
        return self._query(column, rotation)

    def query_instance(self, column: Column, rotation: int) -> Expression:
        assert column.kind == INSTANCE
        return self._query(column, rotation)

    def query_selector(self, selector: Selector) -> Expression:
        return Expression("selector", selector.index)

    def query_challenge(self, challenge: Challenge) -> Expression:
        return Expression("challenge", challenge.index)

    def create_gate(self, name: str, constraints) -> None:
        polys = list(constraints(self))
        assert polys, "a gate needs at least one polynomial"
        for p in polys:
            self.gate_names.append(name)
            self._polys.append(Expression._wrap(p))

    def lookup(self, name: str, table_map) -> int:
        """meta.lookup: table_map(meta) -> [(input Expression, table Expression)]; the queries it makes enter the query lists in
        first-use order.  -> the lookup's index"""
        pairs = [(Expression._wrap(a), Expression._wrap(t)) for a, t in table_map(self)]
        assert pairs, "a lookup needs at least one (input, table) pair"
        self.lookup_names.append(name)
        self._lookups.append(pairs)
        self._merged = None  # a merge made before this lookup does not know of it: merge_lookups() is called again
        return len(self._lookups) - 1

    lookup_any = lookup  # any expression on the table side: advice columns, rotations

    def merge_lookups(self, max_degree: int = None):
        """Opt in to ONE logUp argument per group of lookups over the same table (several input sets, h2mi_logup_inputs; a key of it
        needs Keys(..., logup=True)).  Lookups whose TABLE expression lists are structurally equal are grouped in declaration order; a
        group's inputs are then chunked greedily, in that order, so that every argument's required degree 2 + sum_j max(1, deg A_j) +
        max(1, deg S) stays within the budget [RECALL the chunking of lookups by degree in the mv-lookup line of halo2_proofs; restated
        from memory like the argument].  max_degree None: the largest degree that keeps the unmerged system's extended domain, 2^ceil(
        log2(degree() - 1)) + 1, at most 9 — the extended domain is what a degree costs, so a degree-4 system merges pairs for
        free.  Declaring another lookup afterwards undoes the merge (call it again); degree(), lookup_program(), logup_inputs() and abi() follow the merged
        system, mock and the declared lookups do not change.  -> the arguments as lists of lookup indices"""
        self._merged = None
        if max_degree is None:
            max_degree = min(9, (1 << (self.degree() - 2).bit_length()) + 1)
        assert max_degree <= 9, "the prover takes degrees up to 9"
        groups = {}  # table key -> the lookups over it; dicts keep declaration order
        for l, pairs in enumerate(self._lookups):
            groups.setdefault(tuple(t.key() for _, t in pairs), []).append(l)
        deg_in = lambda l: max([1] + [a.degree() for a, _ in self._lookups[l]])
        chunks = []
        for members in groups.values():
            tab = max([1] + [t.degree() for _, t in self._lookups[members[0]]])
            cur = []
            for l in members:
                if cur and (len(cur) == engine.MAX_LOGUP_INPUTS or 2 + tab + sum(deg_in(m) for m in cur) + deg_in(l) > max_degree):
                    chunks.append(cur)
                    cur = []
                cur.append(l)
            chunks.append(cur)
        self._merged = sorted(chunks)  # arguments in the order of their first lookup
        return self._merged

    @property
    def lookup_arguments(self):
        """per lookup argument the indices of the declared lookups it proves"""
        return self._merged if self._merged is not None else [[l] for l in range(len(self._lookups))]

    @property
    def argument_names(self):
        return [" + ".join(self.lookup_names[l] for l in arg) for arg in self.lookup_arguments]

    def shuffle(self, name: str, shuffle_map) -> int:
        """meta.shuffle: shuffle_map(meta) -> [(input Expression, shuffle Expression)]; the queries it makes enter the query lists in
        first-use order.  -> the shuffle's index"""
        pairs = [(Expression._wrap(a), Expression._wrap(s)) for a, s in shuffle_map(self)]
        assert pairs, "a shuffle needs at least one (input, shuffle) pair"
        self.shuffle_names.append(name)
        self._shuffles.append(pairs)
        return len(self._shuffles) - 1

    # ---- what keygen and create_proof read off it ------------------------------------------------------------------------
    @property
    def n_fixed(self) -> int:
        return self.n_user_fixed + self.n_selectors

    @property
    def fixed_queries(self):
        return self._fixed_queries + [(self.n_user_fixed + s, 0) for s in range(self.n_selectors)]

    def selector_column(self, selector: Selector) -> int:
        return self.n_user_fixed + selector.index

    @property
    def polynomials(self):
        return [p.resolve(self.n_user_fixed) for p in self._polys]

    @property
    def gates(self):
        """the polynomials as callables g(q, challenges=()), q(kind, column, rotation) -> value: the form oracle.flex.ConstraintSystem
        takes"""
        return [(lambda q, challenges=(), p=p: p.evaluate(q, challenges)) for p in self.polynomials]

    @property
    def lookups(self):
        return [[(a.resolve(self.n_user_fixed), t.resolve(self.n_user_fixed)) for a, t in pairs] for pairs in self._lookups]

    @property
    def shuffles(self):
        return [[(a.resolve(self.n_user_fixed), s.resolve(self.n_user_fixed)) for a, s in pairs] for pairs in self._shuffles]

    def degree(self) -> int:
        # per argument; merged: 2 + sum over its input sets + the table, which with one set is the lookup's own rule
        lookups = [max(4, 2 + sum(max([1] + [a.degree() for a, _ in self._lookups[l]]) for l in arg) +
                       max([1] + [t.degree() for _, t in self._lookups[arg[0]]])) for arg in self.lookup_arguments]
        shuffles = [2 + max([1] + [a.degree() for a, _ in pairs] + [s.degree() for _, s in pairs]) for pairs in self._shuffles]
        return max([3] + [p.degree() for p in self._polys] + lookups + shuffles)

    def blinding_factors(self) -> int:
        per_column = [sum(1 for c, _ in self.advice_queries if c == j) for j in range(self.n_advice)]
        return max([3] + per_column) + 2

    def program(self):
        """every gate polynomial in create_gate order -> (ops, constants) of one h2mi_gate_program"""
        constants, ops = {}, []
        for p in self.polynomials:
            ops += p.program(constants)[0]
        return ops, sorted(constants, key=constants.get)

    def gate_program(self) -> engine.GateProgram:
        return engine.GateProgram.build(*self.program())

    def lookup_program(self):
        """the lookups -> engine.LookupProgram (per lookup argument its input polynomials, set by set, then its table polynomials), None
        without lookups"""
        if not self._lookups:
            return None
        constants, ops = {}, []
        resolved = self.lookups
        for arg in self.lookup_arguments:
            for e in [a for l in arg for a, _ in resolved[l]] + [t for _, t in resolved[arg[0]]]:
                ops += e.program(constants)[0]
        return engine.LookupProgram.build([len(self._lookups[arg[0]]) for arg in self.lookup_arguments], ops, sorted(constants, key=constants.get))

    def logup_inputs(self):
        """-> engine.LogupInputs after merge_lookups(), None before (the keygen calls without it)"""
        if self._merged is None:
            return None
        return engine.LogupInputs.build([len(arg) for arg in self._merged])

    def shuffle_program(self):
        """the shuffles -> engine.ShuffleProgram (per shuffle its input polynomials, then its shuffle-side polynomials), None without"""
        if not self._shuffles:
            return None
        constants, ops = {}, []
        for pairs in self.shuffles:
            for e in [a for a, _ in pairs] + [s for _, s in pairs]:
                ops += e.program(constants)[0]
        return engine.ShuffleProgram.build([len(pairs) for pairs in self._shuffles], ops, sorted(constants, key=constants.get))

    @property
    def n_phases(self) -> int:
        return 1 + max(self.advice_phase, default=0)

    def phases(self):
        """-> engine.AdvicePhases, or None for a circuit with one advice phase and no challenge (the keygen calls without phases)"""
        if self.n_phases == 1 and not self.challenge_phase:
            return None
        return engine.AdvicePhases.build(self.advice_phase, self.challenge_phase)

    def abi(self, k: int) -> engine.ConstraintSystem:
        abi = self._abi(k)
        abi.n_lookups = len(self.lookup_arguments)  # described by lookup_program(), not by the struct's single-expression entries
        return abi

    def _abi(self, k: int) -> engine.ConstraintSystem:
        assert self.n_instance <= engine.MAX_INSTANCE, "the prover ABI takes up to eight instance columns"
        return engine.ConstraintSystem.build(k, self.n_advice, self.n_fixed, self.n_instance, self.degree(), self.blinding_factors(),
                                             engine.GATES_EXPRESSIONS, [], [(_KIND[kind], c) for kind, c in self.perm_columns], [],
                                             self.advice_queries, self.fixed_queries)


class Assignment:
    """what synthesize() leaves, through the calls of halo2's Region: sparse cells per column, the copy constraints in call order, the
    public inputs — `instance` is the list of values of the one instance column, or, for a constraint system with several instance
    columns, one list per column (missing columns are empty)"""

    def __init__(self, cs: ConstraintSystem, instance=(), challenges=()):
        self.cs = cs
        self.challenges = list(challenges)  # the values known to this run of synthesize(): integers, None for those not yet squeezed
        self.advice = [dict() for _ in range(cs.n_advice)]
        self.fixed = [dict() for _ in range(cs.n_fixed)]
        if cs.n_instance > 1:
            assert engine.instance_columns(instance) is not None or not len(instance), "several instance columns: one list of values per column"
            assert len(instance) <= cs.n_instance, "more lists of public inputs than instance columns"
            self.instance = [[v % R for v in col] for col in instance] + [[] for _ in range(cs.n_instance - len(instance))]
        else:
            self.instance = [v % R for v in instance]
        self.copies = []  # ((kind, column, row), (kind, column, row))

    def assign_advice(self, column: Column, row: int, value) -> Cell:
        """value: an integer, or a Rational — the column then reaches the prover unresolved and the library inverts"""
        assert column.kind == ADVICE
        self.advice[column.index][row] = _assigned(value)
        return Cell(ADVICE, column.index, row, _assigned(value))

    def assign_fixed(self, column: Column, row: int, value) -> Cell:
        assert column.kind == FIXED
        self.fixed[column.index][row] = _assigned(value)
        return Cell(FIXED, column.index, row, _assigned(value))

    def enable_selector(self, selector: Selector, row: int) -> None:
        self.fixed[self.cs.selector_column(selector)][row] = 1

    def get_challenge(self, challenge: Challenge):
        """Assignment::get_challenge: the value, or None while the transcript has not yielded it (Value::unknown)"""
        return self.challenges[challenge.index] if challenge.index < len(self.challenges) else None

    def constrain_equal(self, left: Cell, right: Cell) -> None:
        self.copies.append(((left.kind, left.column, left.row), (right.kind, right.column, right.row)))

    def constrain_instance(self, cell: Cell, column: Column, row: int) -> None:
        assert column.kind == INSTANCE
        self.copies.append(((cell.kind, cell.column, cell.row), (INSTANCE, column.index, row)))

    def copy_advice(self, cell: Cell, column: Column, row: int) -> Cell:
        """AssignedCell::copy_advice: assign the value again and constrain the two cells equal"""
        new = self.assign_advice(column, row, cell.value)
        self.constrain_equal(cell, new)
        return new


def instance_columns(asg: Assignment) -> list:
    """the public inputs of an assignment as one list per instance column, whichever form asg.instance has"""
    if asg.cs.n_instance > 1:
        return asg.instance
    return [asg.instance] if asg.cs.n_instance else []


def mock(asg: Assignment, k: int, challenges=()) -> None:
    """MockProver::run(k, ..).assert_satisfied() on the host: no cell or copy constraint beyond the usable rows, every gate polynomial
    zero on every usable row (unassigned cells are zero; rotations wrap around 2^k), every copy constraint between equal cells, every
    lookup's input tuple on a usable row equal to its table tuple on some usable row, every shuffle's input tuples over the usable rows
    the same multiset as its shuffle-side tuples.  challenges: the values the gates and lookups
    read (MockProver derives its own; here the caller states the ones the witness was made with).
    Raises ValueError naming the first violation."""
    cs = asg.cs
    n = 1 << k
    u = n - (cs.blinding_factors() + 1)
    rows = [(f"fixed column {c}", max(cells)) for c, cells in enumerate(asg.fixed) if cells]
    rows += [(f"advice column {c}", max(cells)) for c, cells in enumerate(asg.advice) if cells]
    rows += [("a copy constraint", max(left[2], right[2])) for left, right in asg.copies]
    inst = instance_columns(asg)
    rows += [("the instance column" if len(inst) == 1 else f"instance column {c}", len(col) - 1) for c, col in enumerate(inst)]
    for what, row in rows:
        if row >= u:
            raise ValueError(f"NotEnoughRowsAvailable: {what} reaches row {row}, the usable rows end at {u}")
    value = {ADVICE: lambda c, r: _evaluated(asg.advice[c].get(r, 0)), FIXED: lambda c, r: _evaluated(asg.fixed[c].get(r, 0)),
             INSTANCE: lambda c, r: inst[c][r] if r < len(inst[c]) else 0}
    for name, poly in zip(cs.gate_names, cs.polynomials):
        for row in range(u):
            if poly.evaluate(lambda kind, c, rot: value[kind](c, (row + rot) % n), challenges):
                raise ValueError(f"gate {name!r} not satisfied at row {row}")
    for left, right in asg.copies:
        if value[left[0]](left[1], left[2]) % R != value[right[0]](right[1], right[2]) % R:
            raise ValueError(f"copy constraint {left} == {right} not satisfied")
    for name, pairs in zip(cs.lookup_names, cs.lookups):
        at = lambda e, row: e.evaluate(lambda kind, c, rot: value[kind](c, (row + rot) % n), challenges)
        table = {tuple(at(t, row) for _, t in pairs) for row in range(u)}
        for row in range(u):
            if tuple(at(a, row) for a, _ in pairs) not in table:
                raise ValueError(f"lookup {name!r} not satisfied at row {row}")
    for name, pairs in zip(cs.shuffle_names, cs.shuffles):
        at = lambda e, row: e.evaluate(lambda kind, c, rot: value[kind](c, (row + rot) % n), challenges)
        if sorted(tuple(at(a, row) for a, _ in pairs) for row in range(u)) != sorted(tuple(at(s, row) for _, s in pairs) for row in range(u)):
            raise ValueError(f"shuffle {name!r} not satisfied: the two sides are not the same multiset over the usable rows")


class Keys:
    """keygen_vk + keygen_pk through h2mi_prover_keygen, with the lookup and shuffle programs, the logUp input sets and the advice phases
    the circuit has: the fixed cells of a run of synthesize() (selector columns included), the
    copy constraints with their columns renumbered into the permutation argument's order, the gates as a program the key copies.
    Same attributes as flex.FlexKeys.
    logup=True [the `mv-lookup` feature of the Scroll and ezkl lines of halo2_proofs, after Haboeck — restated from memory and pinned to
    DESIGN.md 4.5 and tests/logup_cases.py, not to a crate]: every lookup of the key is proven with a multiplicity column and a running
    sum (H2MI_KEYGEN_LOGUP) in place of the permuted columns and the grand product; needs a circuit with lookups.  `create_proof` and
    `prove_many` follow the key; `mock` and `check` test membership and do not depend on it.  A constraint system after
    merge_lookups() passes its input-set counts and needs logup=True.
    by_coset=True (H2MI_KEYGEN_BY_COSET): the key and its provers keep no column in extended-coset form and the quotient is evaluated
    one coset at a time — the same proof bytes from a fraction of the device memory, at the price of transforms redone
    in every proof; `fixed_cosets` / `sigma_cosets` are then refused by the library."""

    def __init__(self, params: ParamsKZG, cs: ConstraintSystem, asg: Assignment, logup: bool = False, by_coset: bool = False):
        self.cs = cs
        self.logup = bool(logup)
        self.by_coset = bool(by_coset)
        if not logup and any(len(arg) > 1 for arg in cs.lookup_arguments):
            raise ValueError("merge_lookups() merged lookups over one table: only a logUp key proves them, Keys(..., logup=True)")
        self.params = params  # prove_many's default SRS
        k = params.k
        self.domain = d = EvaluationDomain(cs.degree(), k)
        self.u = d.n - (cs.blinding_factors() + 1)
        index = {col: j for j, col in enumerate(cs.perm_columns)}
        copies = [(index[(left[0], left[1])], left[2], index[(right[0], right[1])], right[2]) for left, right in asg.copies]
        self.keys = engine.Keys(cs.abi(k), params, list(asg.fixed), copies, gates=cs.gate_program(), lookups=cs.lookup_program(),
                                phases=cs.phases(), shuffles=cs.shuffle_program(), logup=logup, logup_inputs=cs.logup_inputs() if logup else None,
                                by_coset=by_coset)
        self._finish()

    def _finish(self):
        """what the key shows of its engine.Keys, however that was made"""
        cs, k = self.cs, self.params.k
        self.fixed_commitments, self.permutation_commitments = self.keys.fixed_commitments, self.keys.permutation_commitments
        nf, m = cs.n_fixed, len(cs.perm_columns)
        self.fixed_values, self.fixed_polys, self.fixed_cosets = (self.keys.views(kd, nf) for kd in (engine.PKBUF_FIXED, engine.PKBUF_FIXED_POLY, engine.PKBUF_FIXED_COSET))
        self.sigma_values, self.sigma_polys, self.sigma_cosets = (self.keys.views(kd, m) for kd in (engine.PKBUF_SIGMA, engine.PKBUF_SIGMA_POLY, engine.PKBUF_SIGMA_COSET))
        self._vk_bytes, self.transcript_repr = transcript_repr(k, cs.degree(), self.fixed_commitments, self.permutation_commitments)

    def vk_bytes(self) -> bytes:
        return self._vk_bytes

    def release(self):
        self.keys.release()

    def save(self, path_or_file, user: bytes = b"") -> int:
        """the key as a file (engine.Keys.save: h2mi_prover_pk_export) -> the bytes written"""
        return self.keys.save(path_or_file, user)

    @classmethod
    def load(cls, params: ParamsKZG, cs: ConstraintSystem, path_or_file, by_coset: bool = False) -> "Keys":
        """the key of a file against the constraint system of the caller's own configure() — the crate's `ProvingKey::read::<_, C>`
        re-runs configure as well — without the circuit's synthesis.  ValueError when the file's constraint system, one of its
        programs or its advice phases is not what `cs` gives at params.k: such a key would prove another circuit.  logup is the file's."""
        blob = path_or_file.read() if hasattr(path_or_file, "read") else open(path_or_file, "rb").read()
        engine.blob_check(blob)
        logup = bool(blob[12] & 1)
        want = engine.key_blob_head(cs.abi(params.k), cs.gate_program(), cs.lookup_program(), cs.logup_inputs(), cs.shuffle_program(), cs.phases())
        for name, got, exp in zip(("constraint system", "gate program", "lookup program", "shuffle program", "advice phases"),
                                  engine.blob_sections(blob, 5), want):
            if got != exp:
                raise ValueError(f"key file: its {name} is not the one this constraint system gives")
        self = cls.__new__(cls)
        self.cs, self.logup, self.by_coset, self.params = cs, logup, bool(by_coset), params
        self.domain = d = EvaluationDomain(cs.degree(), params.k)
        self.u = d.n - (cs.blinding_factors() + 1)
        self.keys = engine.Keys.from_blob(params, blob, by_coset)
        self.user = self.keys.user
        self._finish()
        return self


Workspace = flex.FlexWorkspace  # one library prover kept from proof to proof: nothing in it depends on the gate shape


class _PhasedWitness:
    """what flex.create_proof reads off an assignment, for a witness made phase by phase: the public inputs of the first run of
    synthesize() and, as `advice`, the callable engine.Prover.drive calls once per advice phase"""

    def __init__(self, synthesize, n_challenges: int):
        first = [synthesize([None] * n_challenges)]  # the first phase's run, made here for its public inputs and used for phase 0
        self.instance = first[0].instance
        self.advice = lambda challenges: (first.pop() if first else synthesize(challenges)).advice


def create_proof(params: ParamsKZG, keys: Keys, asg, seed: int, transcript=None, trace: dict = None, ws: Workspace = None,
                 multiopen: str = "shplonk") -> bytes:
    """create_proof for one circuit: the transcript on this side, the phase calls into the library (flex.create_proof's body: the
    phases do not depend on how the gates were given; theta reaches the lookups phase through engine.Prover.drive).
    asg: an Assignment, or — a circuit whose witness reads challenges — a callable synthesize(challenges) -> Assignment, called once
    per advice phase with the challenges squeezed so far (None for the others); only that phase's advice columns are taken from
    what it returns, as the crate does.  multiopen: "shplonk" (ProverSHPLONK) or "gwc" (ProverGWC) — the crate's type parameter."""
    engine.check_multiopen(multiopen)
    if callable(asg):
        asg = _PhasedWitness(asg, len(keys.cs.challenge_phase))
    return flex.create_proof(params, keys, asg, seed, transcript=transcript, trace=trace, ws=ws, multiopen=multiopen)


class BatchWorkspace:
    """n library provers against one key bound into one engine.Batch, kept from proof to proof"""

    def __init__(self, params: ParamsKZG, keys, n: int):
        self.provers = [engine.Prover(keys.keys, params) for _ in range(n)]
        try:
            self.batch = engine.Batch(self.provers)
        except Exception:
            for p in self.provers:
                p.release()
            raise

    def release(self):
        self.batch.release()
        for p in self.provers:
            p.release()


def prove_many(pk, assignments, instances=None, seeds=None, params: ParamsKZG = None, transcript=None, trace: dict = None, ws: BatchWorkspace = None,
               hooks: dict = None, multiopen: str = "shplonk") -> bytes:
    """create_proof(&params, &pk, &[circuit_0, .., circuit_(N-1)], &[instances_0, ..], rng, &mut transcript): ONE proof of N <= 8 circuits
    against one key — the fixed and sigma columns, the random polynomial and h(X) opened once, one quotient, one SHPLONK round.
    assignments: per circuit an Assignment or a callable synthesize(challenges) -> Assignment as create_proof takes them (a phase's
    commitments of every circuit precede that phase's challenges).  instances: per circuit its public inputs (default: each
    assignment's own).  seeds: per circuit the seed of its blinding streams, at least 8 apart (the library refuses closer ones: two
    columns of one proof would share their blinding); default 1, 9, 17, ...  params: the SRS (default: the one the key was made with).
    `prove` / `create_proof` stay the single-circuit route; a batch of one gives the same bytes.  multiopen: as create_proof takes it."""
    engine.check_multiopen(multiopen)
    params = params if params is not None else pk.params
    n_challenges = len(getattr(getattr(pk, "cs", None), "challenge_phase", ()))
    wits = [_PhasedWitness(a, n_challenges) if callable(a) else a for a in assignments]
    instances = [list(w.instance) for w in wits] if instances is None else [list(v) for v in instances]  # per circuit: flat, or a list of columns
    seeds = [1 + 8 * i for i in range(len(wits))] if seeds is None else list(seeds)
    own = ws is None
    ws = ws or BatchWorkspace(params, pk, len(wits))
    try:
        transcript = transcript or flex.Blake2bWrite.init()
        transcript.common_scalar(flex._m(pk.transcript_repr))
        for inst in instances:  # KZG: every circuit's public inputs are hashed as scalars, in circuit order
            for v in engine.instance_values(inst):  # a circuit with several instance columns: column by column
                transcript.common_scalar(flex._m(v))
        ws.batch.drive([w.advice for w in wits], instances, seeds, transcript, trace, hooks, multiopen=multiopen)
        return transcript.finalize()
    finally:
        if own:
            ws.release()


def check(params: ParamsKZG, keys: Keys, asg, seed: int = 1, ws: Workspace = None, trace: dict = None) -> None:
    """`mock` on the device, at the sizes the prover runs at (h2mi_prover_check, include/h2mi_prover.h): the advice phase(s) with the
    transcript exactly as create_proof starts — asg an Assignment or synthesize(challenges) — then the check, and the proof is dropped.
    Raises ValueError in mock's words for the first violation (gates in create_gate order, then copy constraints, then lookups, then shuffles) with
    the number of rows or cells that fail; the whole report is the exception's `failures`.  Unlike mock it tests the gates on the
    blinding rows too: a gate that no selector switches off there fails at a row at or beyond the usable rows — the verifier looks
    there as well."""
    if callable(asg):
        asg = _PhasedWitness(asg, len(keys.cs.challenge_phase))
    failures = flex.device_check(params, keys, asg, seed, ws, trace)
    cs = keys.cs
    for f in failures:
        if f.kind == engine.CHECK_GATE:
            msg = f"gate {cs.gate_names[f.index]!r} not satisfied at row {f.row} ({f.count} rows)"
        elif f.kind == engine.CHECK_COPY:
            kind, column = cs.perm_columns[f.index]
            msg = f"copy constraint at cell {(kind, column, f.row)} not satisfied ({f.count} cells differ from their copy)"
        elif f.kind == engine.CHECK_SHUFFLE:
            msg = f"shuffle {cs.shuffle_names[f.index]!r} not satisfied at row {f.row} ({f.count} rows whose input is rarer on the shuffle side)"
        else:
            msg = f"lookup {cs.argument_names[f.index]!r} not satisfied at row {f.row} ({f.count} rows)"
        e = ValueError(msg)
        e.failures = failures
        raise e
