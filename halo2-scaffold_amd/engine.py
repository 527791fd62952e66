"""ctypes binding of include/h2mi_prover.h: the device-resident prover of libh2mi.so behind its phase-level C ABI.

`Keys` is keygen_vk + keygen_pk (reference examples/standard_plonk.rs:33-34, src/scaffold.rs:284,287); `Prover` owns one
h2mi_prover_t and `drive()` is the body of create_proof (examples/standard_plonk.rs:41-49, src/scaffold.rs:322-331) as a
caller sees it: seven phase calls with the Blake2b transcript in between.  The transcript, the witness cells and
vk.transcript_repr stay on this side; every pass over a vector is inside the library (csrc/h2mi_prover.cpp).  The circuit
modules (keygen.py / prover.py: StandardPlonk; flex.py: the halo2-lib builders) describe their constraint system as data and
call these two classes — there is no other prover orchestration in Python.
"""
import ctypes as C
import itertools
import weakref

import numpy as np

from . import field as F
from ._lib import H2miError, check, lib
from .transcript import Blake2bWrite

ADVICE, FIXED, INSTANCE = 0, 1, 2  # H2MI_COL_*
GATES_STANDARD_PLONK, GATES_FLEX_VERTICAL, GATES_EXPRESSIONS = 1, 2, 3
CELLS_CANONICAL = 1
CELLS_RATIONAL = 2  # H2MI_CELLS_RATIONAL: (numerator, denominator) pairs, resolved by the library
CELLS_I64 = 4  # H2MI_CELLS_I64: signed 64-bit integers, 8 bytes per cell (IntCells)
CELLS_DEVICE = 8  # H2MI_CELLS_DEVICE: values and rows are device addresses (DeviceCells)
KEYGEN_VK_ONLY = 1
KEYGEN_BY_COSET = 8  # H2MI_KEYGEN_BY_COSET: no extended-coset columns, the quotient one coset at a time (include/h2mi_prover.h)
KEYGEN_LOGUP = 2  # H2MI_KEYGEN_LOGUP: the key's program lookups are logUp arguments (include/h2mi_prover.h)
EUNSAT = -7
MAX_GATES, MAX_PERM, MAX_LOOKUPS, MAX_QUERIES = 32, 64, 8, 192  # H2MI_MAX_* (include/h2mi_prover.h)
MAX_SHUFFLES = 8  # H2MI_MAX_SHUFFLES (include/h2mi.h)
MAX_LOGUP_INPUTS = 6  # H2MI_MAX_LOGUP_INPUTS (include/h2mi.h)
MAX_ADVICE, MAX_CHALLENGES, MAX_ADVICE_PHASES = 64, 16, 3
MAX_INSTANCE = 8  # H2MI_MAX_INSTANCE (include/h2mi.h)

# h2mi_prover_buffer kinds
(BUF_ADVICE, BUF_ADVICE_POLY, BUF_ADVICE_COSET, BUF_INSTANCE, BUF_PERM_Z, BUF_PERM_Z_POLY, BUF_PERM_Z_COSET, BUF_LOOKUP_PERMUTED_INPUT,
 BUF_LOOKUP_PERMUTED_TABLE, BUF_LOOKUP_Z, BUF_RANDOM_POLY, BUF_H, BUF_H_POLY, BUF_SHPLONK_H, BUF_SHPLONK_H2, BUF_SHUFFLE_Z, BUF_SHUFFLE_Z_POLY,
 BUF_SHUFFLE_INPUT, BUF_SHUFFLE_TABLE, BUF_LOGUP_M, BUF_LOGUP_PHI, BUF_GWC_W) = range(22)
(PKBUF_FIXED, PKBUF_FIXED_POLY, PKBUF_FIXED_COSET, PKBUF_SIGMA, PKBUF_SIGMA_POLY, PKBUF_SIGMA_COSET, PKBUF_L0_COSET, PKBUF_L_LAST_COSET,
 PKBUF_L_ACTIVE_COSET) = range(64, 73)


class Column(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("index", C.c_uint32)]


class Query(C.Structure):
    _fields_ = [("column", C.c_uint32), ("rotation", C.c_int32)]


class Lookup(C.Structure):
    _fields_ = [("input", Column), ("selector_fixed", C.c_int32), ("table_fixed", C.c_uint32)]


class ConstraintSystem(C.Structure):
    """h2mi_constraint_system: ConstraintSystem<Fr> after configure(), as the numbers create_proof reads off it"""
    _fields_ = [("k", C.c_uint32), ("n_advice", C.c_uint32), ("n_fixed", C.c_uint32), ("n_instance", C.c_uint32), ("degree", C.c_uint32),
                ("blinding_factors", C.c_uint32), ("gates", C.c_uint32), ("n_gates", C.c_uint32), ("gate_advice", C.c_uint32 * MAX_GATES),
                ("gate_selector", C.c_uint32 * MAX_GATES), ("n_perm", C.c_uint32), ("perm_columns", Column * MAX_PERM), ("n_lookups", C.c_uint32),
                ("lookups", Lookup * MAX_LOOKUPS), ("n_advice_queries", C.c_uint32), ("n_fixed_queries", C.c_uint32),
                ("advice_queries", Query * MAX_QUERIES), ("fixed_queries", Query * MAX_QUERIES)]

    @classmethod
    def build(cls, k, n_advice, n_fixed, n_instance, degree, blinding_factors, gates, gate_columns, perm_columns, lookups, advice_queries,
              fixed_queries) -> "ConstraintSystem":
        """gate_columns: [(advice column, selector fixed column)]; perm_columns: [(kind, index)]; lookups: [(input advice column,
        selector fixed column or None, table fixed column)]; queries: [(column, rotation)] in creation order"""
        cs = cls()
        cs.k, cs.n_advice, cs.n_fixed, cs.n_instance, cs.degree, cs.blinding_factors, cs.gates = k, n_advice, n_fixed, n_instance, degree, blinding_factors, gates
        assert len(gate_columns) <= MAX_GATES and len(perm_columns) <= MAX_PERM and len(lookups) <= MAX_LOOKUPS
        assert len(advice_queries) <= MAX_QUERIES and len(fixed_queries) <= MAX_QUERIES
        cs.n_gates = len(gate_columns)
        for g, (a, q) in enumerate(gate_columns):
            cs.gate_advice[g], cs.gate_selector[g] = a, q
        cs.n_perm = len(perm_columns)
        for j, (kind, index) in enumerate(perm_columns):
            cs.perm_columns[j] = Column(kind, index)
        cs.n_lookups = len(lookups)
        for l, (inp, sel, table) in enumerate(lookups):
            cs.lookups[l] = Lookup(Column(ADVICE, inp), -1 if sel is None else sel, table)
        cs.n_advice_queries, cs.n_fixed_queries = len(advice_queries), len(fixed_queries)
        for i, (c, r) in enumerate(advice_queries):
            cs.advice_queries[i] = Query(c, r)
        for i, (c, r) in enumerate(fixed_queries):
            cs.fixed_queries[i] = Query(c, r)
        return cs


# h2mi_expr_op.op (include/h2mi.h): the first three are the column kinds above
EXPR_ADVICE, EXPR_FIXED, EXPR_INSTANCE, EXPR_CONSTANT, EXPR_ADD, EXPR_SUB, EXPR_MUL, EXPR_NEG, EXPR_END, EXPR_CHALLENGE = range(10)
MAX_EXPR_OPS, MAX_EXPR_CONSTANTS, MAX_EXPR_STACK = 4096, 256, 8


class ExprOp(C.Structure):
    _fields_ = [("op", C.c_uint32), ("index", C.c_uint32), ("rotation", C.c_int32)]


class GateProgram(C.Structure):
    """h2mi_gate_program: the gate polynomials in postfix, each closed by END, with the constants they push (Montgomery limbs)"""
    _fields_ = [("ops", C.POINTER(ExprOp)), ("n_ops", C.c_uint32), ("constants", C.c_void_p), ("n_constants", C.c_uint32)]

    @classmethod
    def build(cls, ops, constants) -> "GateProgram":
        """ops: [(op, index, rotation)]; constants: integers below r.  The arrays stay alive with the object."""
        g = cls()
        g._ops = (ExprOp * max(len(ops), 1))(*[ExprOp(*o) for o in ops])
        g._constants = np.ascontiguousarray(np.stack([F.fr_to_mont_limbs(v) for v in constants])) if len(constants) else np.zeros((1, 4), dtype=np.uint64)
        g.ops, g.n_ops = g._ops, len(ops)
        g.constants, g.n_constants = g._constants.ctypes.data, len(constants)
        return g

    def check(self, cs: "ConstraintSystem"):
        """h2mi_gate_program_check -> (largest polynomial degree, deepest stack); H2miError(-1) for a program keygen would refuse"""
        degree, depth = C.c_uint32(), C.c_uint32()
        check(lib.h2mi_gate_program_check(C.byref(cs), C.byref(self), C.byref(degree), C.byref(depth)), "gate_program_check")
        return degree.value, depth.value


class LookupProgram(C.Structure):
    """h2mi_lookup_program: the lookups of a constraint system as expressions — per lookup its n_pairs input polynomials, then its
    n_pairs table polynomials, in one postfix program"""
    _fields_ = [("n_lookups", C.c_uint32), ("n_pairs", C.c_uint32 * MAX_LOOKUPS), ("exprs", GateProgram)]

    @classmethod
    def build(cls, n_pairs, ops, constants) -> "LookupProgram":
        """n_pairs: pairs per lookup; ops / constants as GateProgram.build takes them"""
        assert len(n_pairs) <= MAX_LOOKUPS
        lp = cls()
        lp.n_lookups = len(n_pairs)
        for l, m in enumerate(n_pairs):
            lp.n_pairs[l] = m
        lp._exprs = GateProgram.build(ops, constants)  # keeps the arrays alive
        lp.exprs = lp._exprs
        return lp

    def check(self, cs: "ConstraintSystem") -> int:
        """h2mi_lookup_program_check -> the largest required degree; H2miError(-1) for a program keygen would refuse"""
        degree = C.c_uint32()
        check(lib.h2mi_lookup_program_check(C.byref(cs), C.byref(self), C.byref(degree)), "lookup_program_check")
        return degree.value


class LogupInputs(C.Structure):
    """h2mi_logup_inputs: per lookup of a logUp key the number of input tuples over its one table; the LookupProgram then holds per
    lookup its n_inputs x n_pairs input polynomials (set by set), then its n_pairs table polynomials"""
    _fields_ = [("n_inputs", C.c_uint32 * MAX_LOOKUPS)]

    @classmethod
    def build(cls, n_inputs) -> "LogupInputs":
        assert len(n_inputs) <= MAX_LOOKUPS
        li = cls()
        for l in range(MAX_LOOKUPS):
            li.n_inputs[l] = n_inputs[l] if l < len(n_inputs) else 1
        return li

    def check(self, cs: "ConstraintSystem", lookups: LookupProgram, phases: "AdvicePhases" = None) -> int:
        """h2mi_logup_inputs_check -> the largest required degree; H2miError(-1) for what keygen would refuse"""
        degree = C.c_uint32()
        check(lib.h2mi_logup_inputs_check(C.byref(cs), C.byref(lookups), C.byref(self), C.byref(phases) if phases is not None else None,
                                          C.byref(degree)), "logup_inputs_check")
        return degree.value

    def check_table(self, cs: "ConstraintSystem") -> int:
        """h2mi_table_logup_check: these counts as the grouping of a hard-wired shape's cs.lookups[] into logUp arguments over their fixed
        tables -> the largest required degree; H2miError(-1) for what keygen with H2MI_KEYGEN_LOGUP would refuse"""
        return table_logup_check(cs, self)


def table_logup_check(cs: "ConstraintSystem", logup_inputs: "LogupInputs" = None) -> int:
    """h2mi_table_logup_check (host only, works without a GPU); logup_inputs None: one argument per entry of cs.lookups[]"""
    degree = C.c_uint32()
    check(lib.h2mi_table_logup_check(C.byref(cs), C.byref(logup_inputs) if logup_inputs is not None else None, C.byref(degree)), "table_logup_check")
    return degree.value


class ShuffleProgram(C.Structure):
    """h2mi_shuffle_program: the shuffle arguments of a constraint system — per shuffle its n_pairs input polynomials, then its n_pairs
    shuffle-side polynomials, in one postfix program"""
    _fields_ = [("n_shuffles", C.c_uint32), ("n_pairs", C.c_uint32 * MAX_SHUFFLES), ("exprs", GateProgram)]

    @classmethod
    def build(cls, n_pairs, ops, constants) -> "ShuffleProgram":
        """n_pairs: pairs per shuffle (more than H2MI_MAX_SHUFFLES entries are counted, not stored: the check refuses them); ops /
        constants as GateProgram.build takes them"""
        sp = cls()
        sp.n_shuffles = len(n_pairs)
        for i, m in enumerate(n_pairs[:MAX_SHUFFLES]):
            sp.n_pairs[i] = m
        sp._exprs = GateProgram.build(ops, constants)  # keeps the arrays alive
        sp.exprs = sp._exprs
        return sp

    def check(self, cs: "ConstraintSystem", phases: "AdvicePhases" = None) -> int:
        """h2mi_shuffle_program_check (h2mi_shuffle_phases_check when `phases` is given: CHALLENGE ops allowed) -> the largest required
        degree; H2miError(-1) for a program keygen would refuse"""
        degree = C.c_uint32()
        if phases is None:
            check(lib.h2mi_shuffle_program_check(C.byref(cs), C.byref(self), C.byref(degree)), "shuffle_program_check")
        else:
            check(lib.h2mi_shuffle_phases_check(C.byref(cs), C.byref(self), C.byref(phases), C.byref(degree)), "shuffle_phases_check")
        return degree.value


class AdvicePhases(C.Structure):
    """h2mi_advice_phases: the phase of every advice column and of every challenge (meta.advice_column_in, meta.challenge_usable_after)"""
    _fields_ = [("n_phases", C.c_uint32), ("advice_phase", C.c_uint32 * MAX_ADVICE), ("n_challenges", C.c_uint32),
                ("challenge_phase", C.c_uint32 * MAX_CHALLENGES)]

    @classmethod
    def build(cls, advice_phase, challenge_phase=(), n_phases: int = None) -> "AdvicePhases":
        """advice_phase: the phase per advice column; challenge_phase: per challenge the phase it is usable after.  More challenges
        than H2MI_MAX_CHALLENGES are counted, not stored: the check refuses them."""
        assert len(advice_phase) <= MAX_ADVICE
        ph = cls()
        ph.n_phases = 1 + max(advice_phase, default=0) if n_phases is None else n_phases
        for j, p in enumerate(advice_phase):
            ph.advice_phase[j] = p
        ph.n_challenges = len(challenge_phase)
        for i, p in enumerate(challenge_phase[:MAX_CHALLENGES]):
            ph.challenge_phase[i] = p
        return ph

    def check(self, cs: "ConstraintSystem", gates: GateProgram, lookups: LookupProgram = None) -> None:
        """h2mi_advice_phases_check; H2miError(-1) for what keygen would refuse"""
        check(lib.h2mi_advice_phases_check(C.byref(cs), C.byref(gates), C.byref(lookups) if lookups is not None else None, C.byref(self)),
              "advice_phases_check")


def shape_gate_program(cs: "ConstraintSystem", ops_cap: int = None, constants_cap: int = 0):
    """h2mi_shape_gate_program (host only): the gate program equivalent to a hard-wired shape -> (ops [(op, index, rotation)], constants
    [int]).  ops_cap / constants_cap: the buffers to offer (default: enough); H2miError(-6) when they are too small"""
    cap = MAX_GATES * 10 if ops_cap is None else ops_cap
    ops = (ExprOp * max(cap, 1))()
    consts = np.zeros((max(constants_cap, 1), 4), dtype=np.uint64)
    n_ops, n_constants = C.c_uint32(), C.c_uint32()
    check(lib.h2mi_shape_gate_program(C.byref(cs), ops, cap, C.byref(n_ops), consts.ctypes.data, constants_cap, C.byref(n_constants)), "shape_gate_program")
    return ([(o.op, o.index, o.rotation) for o in ops[:n_ops.value]], [F.fr_from_mont_limbs(consts[i]) for i in range(n_constants.value)])


CHECK_GATE, CHECK_COPY, CHECK_LOOKUP, CHECK_SHUFFLE = 0, 1, 2, 3  # h2mi_check_failure.kind


class CheckFailure(C.Structure):
    """h2mi_check_failure: one entry of h2mi_prover_check's report"""
    _fields_ = [("kind", C.c_uint32), ("index", C.c_uint32), ("row", C.c_uint32), ("count", C.c_uint32)]

    def __repr__(self):
        return f"CheckFailure({('GATE', 'COPY', 'LOOKUP', 'SHUFFLE')[self.kind]}, index={self.index}, row={self.row}, count={self.count})"

    def astuple(self):
        return self.kind, self.index, self.row, self.count


class ColumnCells(C.Structure):
    _fields_ = [("rows", C.c_void_p), ("values", C.c_void_p), ("count", C.c_size_t), ("flags", C.c_uint32)]


class CellsSource(C.Structure):
    """h2mi_cells_source (include/h2mi.h): one column of h2mi_fr_scatter_cells_dev — device pointers, format 0 / CELLS_CANONICAL / CELLS_I64"""
    _fields_ = [("d_column", C.c_void_p), ("rows", C.c_void_p), ("values", C.c_void_p), ("count", C.c_size_t), ("row_limit", C.c_uint32),
                ("format", C.c_uint32)]


class Rational:
    """Assigned::Rational(numerator, denominator) [RECALL halo2_proofs v2023_02_02 plonk/assigned.rs, restated from memory]: a cell whose
    inversion is deferred to the prover.  evaluate() is Assigned::evaluate: numerator / denominator, and 0 where the denominator is 0.
    Both halves are kept reduced modulo r; two rationals are equal when their halves are (not when their values are)."""
    __slots__ = ("numerator", "denominator")

    def __init__(self, numerator: int, denominator: int):
        self.numerator, self.denominator = numerator % F.FR_MODULUS, denominator % F.FR_MODULUS

    def evaluate(self) -> int:
        return self.numerator * pow(self.denominator, -1, F.FR_MODULUS) % F.FR_MODULUS if self.denominator else 0

    def __eq__(self, other):
        return isinstance(other, Rational) and (self.numerator, self.denominator) == (other.numerator, other.denominator)

    def __hash__(self):
        return hash((self.numerator, self.denominator))

    def __repr__(self):
        return f"Rational({self.numerator}, {self.denominator})"


class IntCells:
    """a column whose cells are 64-bit integers (H2MI_CELLS_I64): range-check limbs, lookup advice, multiplicities, selectors,
    fixed-point values, lookup tables.  array: a host numpy int64 array, cell i the value array[i] mod r (negative values wrap to
    r - |v|); rows: the uint32 row of each cell, or None for rows 0 .. len - 1.  The array crosses as it is, 8 bytes per cell: no
    Python integer is made.  Accepted wherever pack_cells takes a column: advice, fixed columns (lookup tables included), instances."""

    def __init__(self, array, rows=None):
        a = np.asarray(array)
        if a.dtype != np.int64 or a.ndim != 1:
            raise ValueError(f"IntCells takes a one-dimensional int64 array, not {a.dtype} of shape {a.shape}")
        self.values = np.ascontiguousarray(a)
        self.rows = None
        if rows is not None:
            r = np.asarray(rows)
            if r.dtype != np.uint32 or r.shape != a.shape:
                raise ValueError(f"rows: one uint32 per cell, not {r.dtype} of shape {r.shape}")
            self.rows = np.ascontiguousarray(r)

    def __len__(self):
        return len(self.values)

    def _pack(self, out: ColumnCells, keep: list) -> None:
        out.count, out.flags = len(self.values), CELLS_I64
        if len(self.values):
            out.values = self.values.ctypes.data
            if self.rows is not None:
                out.rows = self.rows.ctypes.data
        keep.append(self)


def _is_tensor(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr")


class DeviceCells:
    """a column whose cells are in device memory already (H2MI_CELLS_DEVICE): advice only.  fmt: "montgomery" — 32-byte Montgomery
    words, carried verbatim; "canonical" — 32-byte integers below r; "i64" — signed 64-bit integers, the cell is v mod r.
    values / rows: a contiguous torch tensor on the library's device (values: int64 of shape (n,) for "i64", int64 or uint64 of shape
    (n, 4) for the 32-byte formats, limbs little-endian; rows: int32 or int64 of shape (n,) — int64 is converted once, on the device),
    an engine.DevView or device.DevBuf, or an integer device address with `count`.  rows None: rows 0 .. count - 1.
    The library reads the memory on its own stream during the advice call and not afterwards: a tensor's current stream is
    synchronised when the column is packed (pack_cells — every drive / create_proof does that right in front of the call); whoever
    hands over a bare address has ordered its producer already.  Bad rows and unreduced canonical values are found on the device and
    raise from the advice call (H2miError -6 / -1) like their host counterparts.  Rows of one column must be distinct."""

    FORMATS = {"montgomery": 0, "canonical": CELLS_CANONICAL, "i64": CELLS_I64}

    def __init__(self, values, rows=None, fmt: str = "montgomery", count: int = None):
        if fmt not in self.FORMATS:
            raise ValueError(f"fmt must be one of {tuple(self.FORMATS)}, not {fmt!r}")
        self.fmt, self.flags = fmt, CELLS_DEVICE | self.FORMATS[fmt]
        self._tensors = []  # kept alive, and their streams synchronised at packing
        width = 8 if fmt == "i64" else 32
        if _is_tensor(values):
            import torch

            self._require_device_tensor(values, "values")
            if fmt == "i64":
                ok = values.dtype == torch.int64 and values.dim() == 1
            else:
                ok = values.dtype in (torch.int64, getattr(torch, "uint64", torch.int64)) and values.dim() == 2 and values.shape[1] == 4
            if not ok:
                raise ValueError(f"values for fmt={fmt!r}: int64 of shape (n,) for 'i64', int64 / uint64 of shape (n, 4) otherwise; not "
                                 f"{values.dtype} of shape {tuple(values.shape)}")
            if count is not None and count != values.shape[0]:
                raise ValueError("count does not match the tensor")
            self.count, self.values_ptr = int(values.shape[0]), int(values.data_ptr())
            self._tensors.append(values)
        elif hasattr(values, "ptr") and hasattr(values, "nbytes"):  # DevView / DevBuf
            self.count = values.nbytes // width if count is None else int(count)
            if self.count * width > values.nbytes:
                raise ValueError("count exceeds the buffer")
            self.values_ptr = int(values.ptr)
            self._tensors.append(values)
        elif isinstance(values, (int, np.integer)):
            if count is None:
                raise ValueError("a device address needs count")
            self.count, self.values_ptr = int(count), int(values)
        else:
            raise ValueError(f"values: a torch tensor on the device, a DevView or an address with count, not {type(values).__name__}")
        self.rows_ptr = None
        if rows is None:
            return
        if _is_tensor(rows):
            import torch

            self._require_device_tensor(rows, "rows")
            if rows.dtype not in (torch.int32, torch.int64) or rows.dim() != 1 or rows.shape[0] != self.count:
                raise ValueError(f"rows: int32 or int64 of shape ({self.count},), not {rows.dtype} of shape {tuple(rows.shape)}")
            if rows.dtype == torch.int64:  # once, on the device; what does not fit stays out of range, where the library refuses it
                rows = rows.clamp(min=-1, max=0x7FFFFFFF).to(torch.int32)
            self.rows_ptr = int(rows.data_ptr())
            self._tensors.append(rows)
        elif hasattr(rows, "ptr") and hasattr(rows, "nbytes"):
            if self.count * 4 > rows.nbytes:
                raise ValueError("fewer rows than cells")
            self.rows_ptr = int(rows.ptr)
            self._tensors.append(rows)
        elif isinstance(rows, (int, np.integer)):
            self.rows_ptr = int(rows)
        else:
            raise ValueError(f"rows: a torch tensor on the device, a DevView or an address, not {type(rows).__name__}")

    @staticmethod
    def _require_device_tensor(t, what: str) -> None:
        if not t.is_cuda:
            raise ValueError(f"{what}: a CPU tensor (DeviceCells takes device memory; a host array goes as IntCells or as a list)")
        if not t.is_contiguous():
            raise ValueError(f"{what}: the tensor is not contiguous")
        primary = lib.h2mi_primary_device()
        if primary >= 0 and t.device.index != primary:
            raise ValueError(f"{what}: the tensor is on device {t.device.index}, the library on device {primary}")

    def __len__(self):
        return self.count

    def _pack(self, out: ColumnCells, keep: list) -> None:
        for t in self._tensors:
            if _is_tensor(t):
                import torch

                torch.cuda.current_stream(t.device).synchronize()  # the producer is done before the library's stream reads
        out.count, out.flags = self.count, self.flags
        if self.count:
            out.values = self.values_ptr
            if self.rows_ptr is not None:
                out.rows = self.rows_ptr
        keep.append(self)


class WitnessDesc(C.Structure):
    """h2mi_witness_desc (include/h2mi.h): a witness program as data — ops sorted by level, constants, checks, the placement"""
    _fields_ = [("ops", C.c_void_p), ("level_ends", C.c_void_p), ("constants", C.c_void_p), ("checks", C.c_void_p), ("placement", C.c_void_p),
                ("counts", C.c_void_p), ("n_ops", C.c_uint32), ("n_levels", C.c_uint32), ("n_constants", C.c_uint32), ("n_inputs", C.c_uint32),
                ("n_checks", C.c_uint32), ("n_columns", C.c_uint32)]

    @classmethod
    def build(cls, ops, level_ends, constants, n_inputs, checks, placement) -> "WitnessDesc":
        """ops: (n, 4) uint32 rows (dst, kind | bits << 8 | shift << 16, a, b); constants: integers (canonical limbs cross as they are:
        the check refuses one not below r); checks: [(a, b)]; placement: one sequence of cell indices per column.  The arrays stay alive
        with the object."""
        d = cls()
        limbs = lambda v: [(int(v) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
        d._keep = [np.ascontiguousarray(np.asarray(ops, dtype=np.uint32).reshape(-1, 4)), np.ascontiguousarray(level_ends, dtype=np.uint32),
                   np.array([limbs(c) for c in constants], dtype=np.uint64).reshape(-1, 4), np.array(checks, dtype=np.uint32).reshape(-1, 2),
                   np.concatenate([np.asarray(p, dtype=np.uint32) for p in placement] + [np.zeros(0, dtype=np.uint32)]),
                   np.array([len(p) for p in placement], dtype=np.uint32)]
        d.ops, d.level_ends, d.constants, d.checks, d.placement, d.counts = (a.ctypes.data if a.size else None for a in d._keep)
        d.n_ops, d.n_levels, d.n_constants, d.n_inputs = len(d._keep[0]), len(d._keep[1]), len(d._keep[2]), n_inputs
        d.n_checks, d.n_columns = len(d._keep[3]), len(d._keep[5])
        return d

    def check(self) -> None:
        """h2mi_witness_check (host only, works without a GPU); H2miError(-1 / -6) for a program h2mi_witness_create would refuse"""
        check(lib.h2mi_witness_check(C.byref(self)), "witness_check")


class WitnessInfo(C.Structure):
    """h2mi_witness_info_t"""
    _fields_ = [("n_cells", C.c_uint32), ("n_levels", C.c_uint32), ("n_grid_launches", C.c_uint32), ("n_wg_launches", C.c_uint32),
                ("device_bytes", C.c_uint64)]


class WitnessProgram:
    """one h2mi_witness_t: a witness program in HBM.  run(inputs) evaluates it and returns its dense Montgomery columns as DeviceCells
    (they belong to the program: valid until its next run or its release — the advice call that follows has consumed them when it
    returns); read(cells) the canonical values of cells after a run (the public inputs).  A failed check raises ValueError("witness
    out of range ...") naming the lowest failing check; the program and every prover stay usable."""

    def __init__(self, desc: WitnessDesc):
        h = C.c_void_p()
        check(lib.h2mi_witness_create(C.byref(desc), C.byref(h)), "witness_create")
        self.handle = h.value
        self.n_inputs, self.counts = desc.n_inputs, [int(c) for c in desc._keep[5]]
        self.checks = desc._keep[3].copy()
        self._columns = (C.c_void_p * max(len(self.counts), 1))()

    @property
    def info(self) -> WitnessInfo:
        out = WitnessInfo()
        check(lib.h2mi_witness_info(self.handle, C.byref(out)), "witness_info")
        return out

    def run(self, inputs) -> list:
        """inputs: n_inputs integers below r -> [DeviceCells(address, count=count_j)]"""
        if len(inputs) != self.n_inputs:
            raise ValueError(f"the program takes {self.n_inputs} inputs, not {len(inputs)}")
        try:
            raw = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in inputs), dtype=np.uint64)
        except OverflowError:
            raise ValueError("an input is not reduced modulo r")
        failed = C.c_uint32()
        rc = lib.h2mi_witness_run(self.handle, raw.ctypes.data if len(inputs) else None, self._columns, C.byref(failed))
        if rc == EUNSAT:
            a, b = self.checks[failed.value]
            raise ValueError(f"witness out of range: check {failed.value} fails, cells {a} and {b} differ")
        check(rc, "witness_run")
        return [DeviceCells(self._columns[j] or 0, count=n) for j, n in enumerate(self.counts)]

    def read(self, cells) -> list:
        """the canonical values of the listed cells of the last run"""
        idx = np.ascontiguousarray(cells, dtype=np.uint32)
        out = np.zeros((max(len(idx), 1), 4), dtype=np.uint64)
        check(lib.h2mi_witness_read(self.handle, idx.ctypes.data if len(idx) else None, len(idx), out.ctypes.data), "witness_read")
        return [int.from_bytes(out[i].tobytes(), "little") for i in range(len(idx))]

    def release(self):
        if self.handle:
            check(lib.h2mi_witness_release(self.handle), "witness_release")
            self.handle = None


CELLS_FOR_ADVICE, CELLS_FOR_INSTANCE, CELLS_FOR_FIXED = 0, 1, 2  # h2mi_column_cells_check's `where`


def cells_check(cells, n_columns: int, where: int) -> None:
    """h2mi_column_cells_check (host only, reads no cell memory): H2miError for what the entry point named by `where` would refuse
    at first sight — flag combinations, null and misaligned pointers, counts"""
    check(lib.h2mi_column_cells_check(cells, n_columns, where), "column_cells_check")


def pack_cells(columns):
    """[{row: value} or [value at row 0, 1, ..]] (integers below r, or Rational) -> (h2mi_column_cells array, objects to keep alive).
    The values cross as canonical 32-byte integers (H2MI_CELLS_CANONICAL): one C-level conversion per value and one join here, the
    Montgomery conversion where they land (long runs: on the device).  A column with at least one Rational crosses as (numerator,
    denominator) pairs (H2MI_CELLS_CANONICAL | H2MI_CELLS_RATIONAL), its integers as (x, 1), and the library resolves it; a column
    with none crosses exactly as it always has.  A column may also be an IntCells (a host int64 array, H2MI_CELLS_I64) or a
    DeviceCells (device memory, H2MI_CELLS_DEVICE): neither is touched cell by cell here."""
    arr = (ColumnCells * max(len(columns), 1))()
    keep = []
    for i, cells in enumerate(columns):
        if isinstance(cells, (IntCells, DeviceCells)):
            cells._pack(arr[i], keep)
            continue
        if isinstance(cells, dict):
            rows = sorted(cells)
            dense = bool(rows) and rows[0] == 0 and rows[-1] == len(rows) - 1
            vals = map(cells.__getitem__, rows)
        else:
            rows, dense, vals = range(len(cells)), True, cells
        count = len(rows)
        if not count:
            continue
        flags = CELLS_CANONICAL
        try:
            try:
                raw = b"".join(map(int.to_bytes, vals, itertools.repeat(32), itertools.repeat("little")))
            except TypeError:  # a Rational among the values: the plain route above pays nothing for the question
                vals = cells.values() if isinstance(cells, dict) else cells
                if not any(isinstance(v, Rational) for v in vals):
                    raise
                flags |= CELLS_RATIONAL
                vals = map(cells.__getitem__, rows) if isinstance(cells, dict) else cells
                halves = [h for v in vals for h in ((v.numerator, v.denominator) if isinstance(v, Rational) else (v, 1))]
                raw = b"".join(map(int.to_bytes, halves, itertools.repeat(32), itertools.repeat("little")))
        except OverflowError:
            raise ValueError("a cell value is not reduced modulo r")
        v = np.frombuffer(raw, dtype=np.uint8)
        keep.append(v)
        arr[i].values, arr[i].count, arr[i].flags = v.ctypes.data, count, flags
        if not dense:
            r = np.array(rows, dtype=np.uint32)
            keep.append(r)
            arr[i].rows = r.ctypes.data
    return arr, keep


def instance_columns(instance):
    """the public inputs of one circuit as callers give them -> None for a flat list of integers (one instance column: the form
    every caller has used so far), or the list of columns for a list of lists (`&[&[col_0], &[col_1], ..]`)"""
    instance = list(instance)
    if all(isinstance(v, (int, np.integer)) for v in instance):
        return None
    if any(isinstance(v, (int, np.integer)) for v in instance):
        raise ValueError("public inputs are a flat list of integers (one instance column) or a list of columns, not a mixture")
    return [list(col) for col in instance]


def instance_values(instance):
    """the public inputs of one circuit in the order the transcript hashes them (KZG: as scalars, before the advice): column by
    column, each column's values in row order"""
    columns = instance_columns(instance)
    return list(instance) if columns is None else [v for col in columns for v in col]


class DevView:
    """a device vector owned by the library (h2mi_prover_buffer / h2mi_prover_pk_buffer): the DevBuf read interface, no ownership"""

    def __init__(self, ptr: int, count: int):
        self.ptr, self.nbytes = ptr, count * 32

    def to_numpy(self, dtype=np.uint64, shape=None, nbytes=None, offset=0) -> np.ndarray:
        nbytes = self.nbytes - offset if nbytes is None else nbytes
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        check(lib.h2mi_memcpy_d2h(out.ctypes.data, self.ptr + offset, nbytes), "d2h")
        return out.reshape(shape) if shape is not None else out

    def free(self):
        pass


class _Views:
    """list-like access to one kind of library-owned buffers"""

    def __init__(self, getter, handle, kind: int, count: int):
        self._get, self._h, self._kind, self._count = getter, handle, kind, count

    def __len__(self):
        return self._count

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self._count))]
        if i < 0:
            i += self._count
        if not 0 <= i < self._count:
            raise IndexError(i)
        p, n = C.c_void_p(), C.c_size_t()
        check(self._get(self._h, self._kind, i, C.byref(p), C.byref(n)), "buffer")
        return DevView(p.value, n.value)

    def __iter__(self):
        return (self[i] for i in range(self._count))


class KeygenArgs(C.Structure):
    """h2mi_keygen_args: the one record h2mi_prover_keygen takes; a pointer left NULL means what include/h2mi_prover.h says beside the field"""
    _fields_ = [("cs", C.POINTER(ConstraintSystem)), ("gates", C.POINTER(GateProgram)), ("lookups", C.POINTER(LookupProgram)),
                ("inputs", C.POINTER(LogupInputs)), ("phases", C.POINTER(AdvicePhases)), ("shuffles", C.POINTER(ShuffleProgram)),
                ("g_lagrange_handle", C.c_uint64), ("fixed", C.c_void_p), ("copies", C.c_void_p), ("n_copies", C.c_size_t), ("flags", C.c_uint)]


class Keys:
    """h2mi_prover_keygen: keygen_vk + keygen_pk for a constraint system given as data, with what the circuit has beside it (gates, lookups,
    phases, shuffles, logUp input sets) as optional programs.  fixed: one {row: value} dict (or dense list, or an IntCells for a column of
    small integers such as a selector or a lookup table) per fixed column as synthesize() assigns them; copies: [(left column, left row,
    right column, right row)] per constrain_equal in call order, columns as indices into the permutation argument.  `params` is the WHOLE SRS."""

    def __init__(self, cs: ConstraintSystem, params, fixed, copies, vk_only: bool = False, gates: GateProgram = None,
                 lookups: LookupProgram = None, phases: AdvicePhases = None, shuffles: ShuffleProgram = None, logup: bool = False,
                 logup_inputs: "LogupInputs" = None, by_coset: bool = False):
        self.cs = cs
        self.by_coset = bool(by_coset)  # H2MI_KEYGEN_BY_COSET: same proofs, a device footprint without 2^extended_k columns, slower
        self.logup = bool(logup)  # H2MI_KEYGEN_LOGUP: a lookup program's lookups, or a hard-wired shape's over their keygen-sorted tables
        self.n_shuffles = shuffles.n_shuffles if shuffles is not None else 0
        cells, keep = pack_cells(fixed)
        cp = np.ascontiguousarray(np.array(copies, dtype=np.uint32).reshape(-1, 4))
        h = C.c_void_p()
        flags = (KEYGEN_VK_ONLY if vk_only else 0) | (KEYGEN_LOGUP if logup else 0) | (KEYGEN_BY_COSET if by_coset else 0)
        opt = lambda s: C.pointer(s) if s is not None else None
        args = KeygenArgs(C.pointer(cs), opt(gates), opt(lookups), opt(logup_inputs), opt(phases), opt(shuffles), params.g_lagrange_handle,
                          C.cast(cells, C.c_void_p), cp.ctypes.data, len(cp), flags)
        check(lib.h2mi_prover_keygen(C.byref(args), C.byref(h)), "keygen")
        del keep
        self.handle = h.value
        self.phases = phases
        self._provers = weakref.WeakSet()  # the library refuses to release a key while a prover created against it is alive
        self.fixed_commitments = np.zeros((cs.n_fixed, 8), dtype=np.uint64)
        self.permutation_commitments = np.zeros((cs.n_perm, 8), dtype=np.uint64)
        check(lib.h2mi_prover_vk_commitments(self.handle, self.fixed_commitments.ctypes.data, self.permutation_commitments.ctypes.data), "vk commitments")

    def views(self, kind: int, count: int) -> _Views:
        return _Views(lib.h2mi_prover_pk_buffer, self.handle, kind, count)

    def view(self, kind: int) -> DevView:
        return self.views(kind, 1)[0]

    def release(self):
        if self.handle:
            for p in list(self._provers):
                p.release()
            check(lib.h2mi_prover_pk_release(self.handle), "pk_release")
            self.handle = None

    # ---- key files: h2mi_prover_pk_export / _import (include/h2mi_prover.h; the format is DESIGN.md 3) ----
    def export(self, user: bytes = b"") -> bytes:
        """the key as one blob: the fixed columns' cells compacted on the device, the moved cells, the programs, the commitments and
        `user` (an opaque section of up to 1 MiB: break points, builder parameters).  The same key gives the same bytes every time."""
        user = bytes(user)
        n = C.c_size_t()
        check(lib.h2mi_prover_pk_export(self.handle, user, len(user), None, 0, C.byref(n)), "pk_export")
        buf = np.zeros(n.value // 8, dtype=np.uint64)
        check(lib.h2mi_prover_pk_export(self.handle, user, len(user), buf.ctypes.data, buf.nbytes, C.byref(n)), "pk_export")
        return buf.tobytes()

    def save(self, path_or_file, user: bytes = b"") -> int:
        """write export(user) to a path or to a binary file object -> the bytes written"""
        blob = self.export(user)
        if hasattr(path_or_file, "write"):
            path_or_file.write(blob)
        else:
            with open(path_or_file, "wb") as f:
                f.write(blob)
        return len(blob)

    @classmethod
    def from_blob(cls, params, blob: bytes, by_coset: bool = False) -> "Keys":
        """h2mi_prover_pk_import: the key a blob describes, against `params` (the WHOLE SRS the key was made against: the library
        recomputes the commitments and refuses, H2miError(-1), a blob whose stored ones differ).  The layout in HBM is the importer's:
        by_coset does not depend on how the exporting key was made.  cs, commitments, logup, n_shuffles and phases come from the blob;
        `user` holds its user section."""
        cs, user = blob_check(blob)
        buf = np.frombuffer(bytes(blob), dtype=np.uint8)
        h = C.c_void_p()
        check(lib.h2mi_prover_pk_import(buf.ctypes.data, buf.nbytes, params.g_lagrange_handle, KEYGEN_BY_COSET if by_coset else 0, C.byref(h)), "pk_import")
        self = cls.__new__(cls)
        self.cs, self.user, self.by_coset, self.handle = cs, user, bool(by_coset), h.value
        self.logup, self.n_shuffles, self.phases = _blob_programs(blob, cs)
        self._provers = weakref.WeakSet()
        self.fixed_commitments = np.zeros((cs.n_fixed, 8), dtype=np.uint64)
        self.permutation_commitments = np.zeros((cs.n_perm, 8), dtype=np.uint64)
        check(lib.h2mi_prover_vk_commitments(self.handle, self.fixed_commitments.ctypes.data, self.permutation_commitments.ctypes.data), "vk commitments")
        return self

    @classmethod
    def load(cls, params, path_or_file, by_coset: bool = False) -> "Keys":
        """from_blob over the contents of a path or of a binary file object"""
        if hasattr(path_or_file, "read"):
            return cls.from_blob(params, path_or_file.read(), by_coset)
        with open(path_or_file, "rb") as f:
            return cls.from_blob(params, f.read(), by_coset)


def blob_check(blob: bytes):
    """h2mi_prover_pk_blob_check (host only, works without a GPU): every validation import applies before its first device call ->
    (the blob's ConstraintSystem, its user section); H2miError(-1) for a blob import would refuse"""
    buf = np.frombuffer(bytes(blob), dtype=np.uint8)
    cs = ConstraintSystem()
    user, user_len = C.c_void_p(), C.c_size_t()
    check(lib.h2mi_prover_pk_blob_check(buf.ctypes.data, buf.nbytes, C.byref(cs), C.byref(user), C.byref(user_len)), "pk_blob_check")
    at = (user.value or 0) - buf.ctypes.data
    return cs, bytes(buf[at:at + user_len.value]) if user_len.value else b""


def blob_sections(blob: bytes, count: int) -> list:
    """the payloads of the first `count` sections of a CHECKED blob behind its 32-byte header (a 64-bit length, the payload, zeros to 8)"""
    at, out = 32, []
    for _ in range(count):
        n = int.from_bytes(blob[at:at + 8], "little")
        out.append(bytes(blob[at + 8:at + 8 + n]))
        at += 8 + (n + 7) // 8 * 8
    return out


def key_blob_head(cs: ConstraintSystem, gates: GateProgram = None, lookups: LookupProgram = None, logup_inputs: LogupInputs = None,
                  shuffles: ShuffleProgram = None, phases: AdvicePhases = None) -> list:
    """the five sections a key of this constraint system and these programs exports in front of its cells: the constraint
    system field by field, the gate, lookup and shuffle programs, the advice phases — what a host that re-runs its cheap configure()
    holds a key file against before it loads it (custom.Keys.load)"""
    u32s = lambda *v: b"".join(int(x & 0xFFFFFFFF).to_bytes(4, "little") for x in v)
    program = lambda g: u32s(g.n_ops, g.n_constants) + b"".join(u32s(o.op, o.index, o.rotation) for o in g._ops[:g.n_ops]) + \
        g._constants[:g.n_constants].tobytes()
    n_gates = cs.n_gates if cs.gates == GATES_FLEX_VERTICAL else 0
    head = u32s(cs.k, cs.n_advice, cs.n_fixed, cs.n_instance, cs.degree, cs.blinding_factors, cs.gates, n_gates, cs.n_perm, cs.n_lookups,
                cs.n_advice_queries, cs.n_fixed_queries)
    head += u32s(*cs.gate_advice[:n_gates]) + u32s(*cs.gate_selector[:n_gates])
    head += b"".join(u32s(c.kind, c.index) for c in cs.perm_columns[:cs.n_perm])
    head += b"".join(u32s(0, 0, 0, 0) if lookups is not None else u32s(l.input.kind, l.input.index, l.selector_fixed, l.table_fixed)
                     for l in cs.lookups[:cs.n_lookups])
    head += b"".join(u32s(q.column, q.rotation) for q in list(cs.advice_queries[:cs.n_advice_queries]) + list(cs.fixed_queries[:cs.n_fixed_queries]))
    out = [head, program(gates) if gates is not None else b"", b"", b"", b""]
    if lookups is not None:
        sets = [logup_inputs.n_inputs[l] if logup_inputs is not None else 1 for l in range(lookups.n_lookups)]
        out[2] = u32s(lookups.n_lookups, *lookups.n_pairs[:lookups.n_lookups], *sets) + program(lookups._exprs)
    if shuffles is not None:
        out[3] = u32s(shuffles.n_shuffles, *shuffles.n_pairs[:shuffles.n_shuffles]) + program(shuffles._exprs)
    if phases is not None and (phases.n_phases > 1 or phases.n_challenges):
        out[4] = u32s(phases.n_phases, phases.n_challenges, *phases.advice_phase[:cs.n_advice], *phases.challenge_phase[:phases.n_challenges])
    return out


def _blob_programs(blob: bytes, cs: ConstraintSystem):
    """what a prover's host needs of a CHECKED blob beside cs -> (logup, n_shuffles, AdvicePhases or None): the header's flag word, and
    the shuffle and phase sections — the fourth and fifth behind the 32-byte header, each a 64-bit length and a payload padded to 8"""
    u32 = lambda at: int.from_bytes(blob[at:at + 4], "little")
    at, payloads = 32, []
    for _ in range(5):
        n = int.from_bytes(blob[at:at + 8], "little")
        payloads.append((at + 8, n))
        at += 8 + (n + 7) // 8 * 8
    (sh_at, sh_len), (ph_at, ph_len) = payloads[3], payloads[4]
    phases = None
    if ph_len:
        n_phases, n_challenges = u32(ph_at), u32(ph_at + 4)
        phases = AdvicePhases.build([u32(ph_at + 8 + 4 * j) for j in range(cs.n_advice)],
                                    [u32(ph_at + 8 + 4 * cs.n_advice + 4 * i) for i in range(n_challenges)], n_phases=n_phases)
    return bool(u32(12) & 1), (u32(sh_at) if sh_len else 0), phases


class _Counts(C.Structure):
    _fields_ = [("advice", C.c_uint32), ("lookups", C.c_uint32), ("products", C.c_uint32), ("quotient", C.c_uint32), ("evaluations", C.c_uint32)]


class _PhaseCounts(C.Structure):
    _fields_ = [("n_phases", C.c_uint32), ("n_challenges", C.c_uint32), ("advice", C.c_uint32 * MAX_ADVICE_PHASES),
                ("challenges", C.c_uint32 * MAX_ADVICE_PHASES)]


_COMBINE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t)


MULTIOPEN = ("shplonk", "gwc")  # the multi-opening schemes create_proof ends with (the crate's type parameter P: ProverSHPLONK / ProverGWC)


def check_multiopen(multiopen: str) -> None:
    if multiopen not in MULTIOPEN:
        raise ValueError(f"multiopen must be one of {MULTIOPEN}, not {multiopen!r}")


class Prover:
    """one h2mi_prover_t: the device buffers, streams and phase state of one create_proof at a time, reused from proof to proof
    (the reference's drivers prove repeatedly against one pk / SRS, e.g. examples/linear_regression.rs:126-195).
    params: the whole SRS, or one rank's slice of it (ParamsKZG.register_slice) together with `combiner`, a dist.PhaseCombiner
    with a slot per commitment of the largest phase (8 covers the reference's shapes): every commitment is then this rank's partial point, combined across ranks whenever a phase reads its
    points back (the library calls back into combiner.combine)."""

    def __init__(self, keys: Keys, params, combiner=None):
        self.keys, self.combiner = keys, combiner
        h = C.c_void_p()
        check(lib.h2mi_prover_create(keys.handle, params.g_handle, params.g_lagrange_handle, params.lo, params.n, C.byref(h)), "prover_create")
        self.handle = h.value
        keys._provers.add(self)
        self.counts = _Counts()
        check(lib.h2mi_prover_get_counts(self.handle, C.byref(self.counts)), "prover counts")
        self.phase_counts = _PhaseCounts()
        check(lib.h2mi_prover_get_phase_counts(self.handle, C.byref(self.phase_counts)), "prover phase counts")
        self._points = np.zeros((max(self.counts.advice, self.counts.lookups, self.counts.products, self.counts.quotient, 8), 8), dtype=np.uint64)
        self._evals = np.zeros((self.counts.evaluations, 4), dtype=np.uint64)
        self._cb = None
        self._cb_error = None
        if combiner is not None:
            c = self.counts
            assert combiner.slots >= max(c.advice, c.lookups, c.products, c.quotient), "the combiner needs a slot per commitment of the largest phase"

            def _combine(_ctx, count):
                try:
                    combiner.combine(0, count)
                    return 0
                except BaseException as e:  # an exception must not unwind through the C frames
                    self._cb_error = e
                    return 1

            self._cb = _COMBINE_FN(_combine)
            check(lib.h2mi_prover_set_combiner(self.handle, combiner.partial_ptr, combiner.combined.ptr, self._cb, None), "set_combiner")

    def set_rng_key(self, key: bytes = None) -> None:
        """h2mi_prover_set_rng_key: blinding from ChaCha20 under a 256-bit key (the `seed` of later proofs is then the per-proof
        nonce, below 2^61) instead of the reproducible 32-bit seeded streams; None returns to those"""
        if key is not None and len(key) != 32:
            raise ValueError("the key is 32 bytes")
        check(lib.h2mi_prover_set_rng_key(self.handle, key), "set_rng_key")

    def device_bytes(self) -> tuple:
        """h2mi_prover_device_bytes: (key bytes, prover bytes) of the device vectors the key and this prover own; the library-wide
        caches (window tables, twiddles, scratch) are not in it"""
        kb, pb = C.c_size_t(), C.c_size_t()
        check(lib.h2mi_prover_device_bytes(self.handle, C.byref(kb), C.byref(pb)), "device_bytes")
        return kb.value, pb.value

    def views(self, kind: int, count: int) -> _Views:
        return _Views(lib.h2mi_prover_buffer, self.handle, kind, count)

    def view(self, kind: int) -> DevView:
        return self.views(kind, 1)[0]

    def _phase(self, rc: int, what: str):
        if rc and self._cb_error is not None:
            e, self._cb_error = self._cb_error, None
            raise e
        if rc == EUNSAT:
            raise ValueError("shuffle sides are not the same multiset (ConstraintSystemFailure)" if what == "products" else
                             "lookup input not in the table (ConstraintSystemFailure)")
        check(rc, what)

    def check(self, theta=None, cap: int = 64) -> list:
        """h2mi_prover_check on the proof in flight (after the last advice phase and set_challenges, before the products): -> the
        failures [CheckFailure], empty for a witness that satisfies the circuit.  theta: 4 Montgomery limbs (an array) or an integer;
        needed by a key whose lookups are a program.  Read-only: the proof goes on as if it had not been called."""
        if theta is not None and not isinstance(theta, np.ndarray):
            theta = F.fr_to_mont_limbs(theta)
        theta = None if theta is None else np.ascontiguousarray(theta, dtype=np.uint64)
        out, n = (CheckFailure * max(cap, 1))(), C.c_size_t()
        rc = lib.h2mi_prover_check(self.handle, None if theta is None else theta.ctypes.data, out, cap, C.byref(n))
        if rc != EUNSAT:
            check(rc, "check")
        if n.value > cap:
            return self.check(theta, n.value)
        return list(out[:n.value])

    def gwc_num_points(self) -> int:
        """h2mi_prover_gwc_num_points: the commitments of a GWC tail — the distinct rotations of the key's queries"""
        n = C.c_size_t()
        check(lib.h2mi_prover_gwc_num_points(self.handle, C.byref(n)), "gwc_num_points")
        return n.value

    def set_instances(self, columns) -> None:
        """h2mi_prover_instances: the public inputs of the NEXT proof, one list of integers per instance column (it holds for that
        proof only)"""
        cells, keep = pack_cells(columns)
        check(lib.h2mi_prover_instances(self.handle, cells), "instances")
        del keep

    def _public_inputs(self, instance):
        """what the advice call takes for `instance` -> (limbs, count): a flat list travels in its arguments as ever; a list of
        columns goes through h2mi_prover_instances first and leaves the arguments empty"""
        columns = instance_columns(instance)
        if columns is not None:
            self.set_instances(columns)
            instance = []
        inst = np.ascontiguousarray(np.stack([F.fr_to_mont_limbs(v) for v in instance])) if len(instance) else np.zeros((1, 4), dtype=np.uint64)
        return inst, len(instance)

    def drive(self, advice, instance, seed: int, transcript: Blake2bWrite, trace: dict = None, witness_check: str = None,
              multiopen: str = "shplonk"):
        """create_proof between the transcript's challenges.  advice: one {row: value} dict or dense list per advice column, or an
        IntCells (a host int64 array) or a DeviceCells (device memory: a torch tensor, a DevView, an address) in its place;
        instance: the public inputs — a flat list of integers (one instance column), or a list of columns, each a list of integers (any
        number of instance columns; engine.instance_values gives the order in which the caller hashes them).  The caller has hashed
        vk.transcript_repr and the public inputs already.
        A key with several advice phases or with challenges: `advice` may be a callable, synthesize(challenges) -> such a list,
        called once per advice phase with the challenges known so far (integers; None for those not yet squeezed), of whose result
        only that phase's columns are taken [RECALL halo2_proofs v2023_02_02 plonk/prover.rs]; a plain list serves every phase.
        witness_check: "only" — run the witness check (self.check with the transcript's theta) once the advice is committed and return its
        failures without going on (the next proof starts at the advice as usual); "also" — run it and prove on: the bytes are those
        of a proof without it.  Either way trace["check"] holds the failures.
        multiopen: "shplonk" (ProverSHPLONK: two points) or "gwc" (ProverGWC: one point per distinct opening point); the bytes before
        the opening argument do not depend on it."""
        check_multiopen(multiopen)
        c, h, pts = self.counts, self.handle, self._points
        pp = pts.ctypes.data
        sq = transcript.squeeze_challenge  # 4 Montgomery limbs

        def write_points(k):
            for i in range(k):
                transcript.write_point(pts[i])  # raises on the identity, as the crate's transcript does

        import time

        marks = [("start", time.perf_counter())]
        mark = (lambda name: marks.append((name, time.perf_counter()))) if trace is not None else (lambda name: None)
        inst, n_inst = self._public_inputs(instance)
        pc = self.phase_counts
        if pc.n_phases == 1 and pc.n_challenges == 0 and not callable(advice):
            cells, keep = pack_cells(advice)
            self._phase(lib.h2mi_prover_advice(h, cells, inst.ctypes.data, n_inst, seed, pp), "advice")
            del keep
            write_points(c.advice)
        else:
            column_phase = self.keys.phases.advice_phase if self.keys.phases is not None else [0] * c.advice
            challenge_phase = self.keys.phases.challenge_phase if pc.n_challenges else []
            limbs, known = [None] * pc.n_challenges, [None] * pc.n_challenges
            for phase in range(pc.n_phases):
                columns = advice(list(known)) if callable(advice) else advice
                cells, keep = pack_cells([cells_ if column_phase[j] == phase else {} for j, cells_ in enumerate(columns)])
                self._phase(lib.h2mi_prover_advice_phase(h, phase, cells, inst.ctypes.data, n_inst, seed, pp), f"advice phase {phase}")
                del keep
                write_points(pc.advice[phase])
                for i in range(pc.n_challenges):  # in index order, the challenges usable after this phase
                    if challenge_phase[i] == phase:
                        limbs[i] = sq()
                        known[i] = F.fr_from_mont_limbs(limbs[i])
                mark(f"advice phase {phase} committed")
            if pc.n_challenges:
                ch = np.ascontiguousarray(np.stack(limbs))
                self._phase(lib.h2mi_prover_set_challenges(h, ch.ctypes.data), "set_challenges")
            if trace is not None:
                trace["challenges"] = list(known)
        mark("advice committed")
        theta = sq()  # drawn even without lookups
        if witness_check is not None:
            failures = self.check(theta)
            mark("witness check")
            if trace is not None:
                trace["check"], trace["theta"] = failures, F.fr_from_mont_limbs(theta)
            if witness_check == "only":
                return failures
        if c.lookups or self.keys.n_shuffles:  # a key with shuffles takes theta through this call even without lookups (no points then)
            self._phase(lib.h2mi_prover_lookups(h, theta.ctypes.data, pp), "lookups")
            write_points(c.lookups)
            mark("permuted lookup columns committed")
        beta, gamma = sq(), sq()
        self._phase(lib.h2mi_prover_products(h, beta.ctypes.data, gamma.ctypes.data, pp), "products")
        write_points(c.products)
        mark("z, random committed")
        y = sq()
        self._phase(lib.h2mi_prover_quotient(h, y.ctypes.data, pp), "quotient")
        write_points(c.quotient)
        mark("h pieces committed")
        x = sq()
        self._phase(lib.h2mi_prover_evaluations(h, x.ctypes.data, self._evals.ctypes.data), "evaluations")
        for e in self._evals:
            transcript.write_scalar(e)
        mark("evaluations written")
        if multiopen == "gwc":  # ProverGWC: v, then every [W_i]
            gv, w = sq(), np.zeros((self.gwc_num_points(), 8), dtype=np.uint64)
            self._phase(lib.h2mi_prover_gwc_open(h, gv.ctypes.data, w.ctypes.data), "gwc open")
            for pt in w:
                transcript.write_point(pt)
            mark("gwc done")
        else:
            sy, sv = sq(), sq()  # ProverSHPLONK: y, v
            self._phase(lib.h2mi_prover_shplonk_quotient(h, sy.ctypes.data, sv.ctypes.data, pp), "shplonk quotient")
            write_points(1)
            su = sq()
            self._phase(lib.h2mi_prover_shplonk_open(h, su.ctypes.data, pp), "shplonk open")
            write_points(1)
            mark("shplonk done")
        if trace is not None:
            m = F.fr_from_mont_limbs
            trace.update(theta=m(theta), beta=m(beta), gamma=m(gamma), y=m(y), x=m(x),
                         phase_ms=[(b[0], round((b[1] - a[1]) * 1e3, 3)) for a, b in zip(marks, marks[1:])])

    def release(self):
        if self.handle:
            check(lib.h2mi_prover_destroy(self.handle), "prover_destroy")
            self.handle = None


class Batch:
    """one h2mi_batch_t: N provers over one key whose circuits go into ONE proof — create_proof(&params, &pk, &[c_0, .., c_(N-1)], ..).
    The per-circuit phases run on the members, `drive()` orders their points in the transcript as the crate does [RECALL halo2_proofs
    v2023_02_02 plonk/prover.rs] and calls the joint phases on the batch.  While the batch lives its members cannot be released;
    release() makes them ordinary provers again."""

    def __init__(self, provers):
        self.members = list(provers)
        arr = (C.c_void_p * max(len(self.members), 1))(*[p.handle for p in self.members])
        h = C.c_void_p()
        check(lib.h2mi_batch_create(arr, len(self.members), C.byref(h)), "batch_create")
        self.handle = h.value
        for p in self.members:  # a member behind the first commits no random polynomial: its products count has changed
            check(lib.h2mi_prover_get_counts(p.handle, C.byref(p.counts)), "prover counts")
        n = C.c_size_t()
        check(lib.h2mi_batch_num_evaluations(self.handle, C.byref(n)), "batch num_evaluations")
        self.n_evaluations = n.value
        self._evals = np.zeros((max(n.value, 1), 4), dtype=np.uint64)

    def gwc_num_points(self) -> int:
        n = C.c_size_t()
        check(lib.h2mi_batch_gwc_num_points(self.handle, C.byref(n)), "batch gwc_num_points")
        return n.value

    def drive(self, advices, instances, seeds, transcript: Blake2bWrite, trace: dict = None, hooks: dict = None, multiopen: str = "shplonk"):
        """create_proof for the batch between the transcript's challenges.  advices[i] / instances[i] / seeds[i]: what Prover.drive
        takes, for circuit i — instances[i] flat or a list of columns, every member with its own — (a callable synthesize(challenges) per circuit when the witness reads challenges: every circuit's
        commitments of a phase precede that phase's challenges, which all circuits then read).  The caller has hashed
        vk.transcript_repr and every circuit's public inputs, in circuit order.  hooks (tests): "products_done"(batch) is called when
        every member has run its products, "y"(limbs) -> the y handed to the library instead of the transcript's.
        multiopen: as Prover.drive takes it."""
        check_multiopen(multiopen)
        ms, hooks = self.members, hooks or {}
        lead = ms[0]
        c, pc = lead.counts, lead.phase_counts
        assert len(advices) == len(instances) == len(seeds) == len(ms)
        sq = transcript.squeeze_challenge
        m = F.fr_from_mont_limbs

        def points(p, k):
            return [p._points[i].copy() for i in range(k)]

        def write(pts):
            for pt in pts:
                transcript.write_point(pt)

        pubs = [p._public_inputs(inst) for p, inst in zip(ms, instances)]  # every member's own columns, read by its phase-0 call
        column_phase = lead.keys.phases.advice_phase if lead.keys.phases is not None else [0] * c.advice
        challenge_phase = lead.keys.phases.challenge_phase if pc.n_challenges else []
        limbs, known = [None] * pc.n_challenges, [None] * pc.n_challenges
        single = pc.n_phases == 1 and pc.n_challenges == 0
        for phase in range(pc.n_phases):
            for i, p in enumerate(ms):  # this phase's commitments of every circuit, in circuit order
                columns = advices[i](list(known)) if callable(advices[i]) else advices[i]
                pp = p._points.ctypes.data
                inst, n_inst = pubs[i]
                if single:
                    cells, keep = pack_cells(columns)
                    p._phase(lib.h2mi_prover_advice(p.handle, cells, inst.ctypes.data, n_inst, seeds[i], pp), "advice")
                else:
                    cells, keep = pack_cells([cells_ if column_phase[j] == phase else {} for j, cells_ in enumerate(columns)])
                    p._phase(lib.h2mi_prover_advice_phase(p.handle, phase, cells, inst.ctypes.data, n_inst, seeds[i], pp), f"advice phase {phase}")
                del keep
                write(points(p, pc.advice[phase]))
            for i in range(pc.n_challenges):  # then its challenges, once for the proof
                if challenge_phase[i] == phase:
                    limbs[i] = sq()
                    known[i] = m(limbs[i])
        if pc.n_challenges:
            ch = np.ascontiguousarray(np.stack(limbs))
            for p in ms:
                p._phase(lib.h2mi_prover_set_challenges(p.handle, ch.ctypes.data), "set_challenges")
        theta = sq()
        n_sh = lead.keys.n_shuffles
        if c.lookups or n_sh:
            for p in ms:
                p._phase(lib.h2mi_prover_lookups(p.handle, theta.ctypes.data, p._points.ctypes.data), "lookups")
                write(points(p, c.lookups))
        beta, gamma = sq(), sq()
        n_lk = c.lookups if lead.keys.logup else c.lookups // 2  # lookup products; a logUp key: one running sum per multiplicity column
        n_sets = c.products - 1 - n_lk - n_sh
        products = []
        for p in ms:
            p._phase(lib.h2mi_prover_products(p.handle, beta.ctypes.data, gamma.ctypes.data, p._points.ctypes.data), "products")
            products.append(points(p, p.counts.products))
        for pts in products:  # every circuit's permutation products, then every circuit's lookup products, then the random polynomial
            write(pts[:n_sets])
        for pts in products:
            write(pts[n_sets:n_sets + n_lk])
        for pts in products:  # every circuit's shuffle products behind every circuit's lookup products
            write(pts[n_sets + n_lk:n_sets + n_lk + n_sh])
        write(products[0][n_sets + n_lk + n_sh:])
        if "products_done" in hooks:
            hooks["products_done"](self)
        y = sq()
        y_lib = hooks["y"](y) if "y" in hooks else y
        pp = lead._points.ctypes.data
        lead._phase(lib.h2mi_batch_quotient(self.handle, y_lib.ctypes.data, pp), "batch quotient")
        write(points(lead, c.quotient))
        x = sq()
        lead._phase(lib.h2mi_batch_evaluations(self.handle, x.ctypes.data, self._evals.ctypes.data), "batch evaluations")
        for e in self._evals[:self.n_evaluations]:
            transcript.write_scalar(e)
        if multiopen == "gwc":
            gv, w = sq(), np.zeros((self.gwc_num_points(), 8), dtype=np.uint64)
            lead._phase(lib.h2mi_batch_gwc_open(self.handle, gv.ctypes.data, w.ctypes.data), "batch gwc open")
            write(w)
        else:
            sy, sv = sq(), sq()
            lead._phase(lib.h2mi_batch_shplonk_quotient(self.handle, sy.ctypes.data, sv.ctypes.data, pp), "batch shplonk quotient")
            write(points(lead, 1))
            su = sq()
            lead._phase(lib.h2mi_batch_shplonk_open(self.handle, su.ctypes.data, pp), "batch shplonk open")
            write(points(lead, 1))
        if trace is not None:
            trace.update(theta=m(theta), beta=m(beta), gamma=m(gamma), y=m(y), x=m(x), challenges=list(known))

    def release(self):
        if self.handle:
            check(lib.h2mi_batch_destroy(self.handle), "batch_destroy")
            self.handle = None
            for p in self.members:
                if p.handle:
                    check(lib.h2mi_prover_get_counts(p.handle, C.byref(p.counts)), "prover counts")


__all__ = ["ConstraintSystem", "Keys", "Prover", "Batch", "DevView", "H2miError", "ShuffleProgram", "IntCells", "DeviceCells", "WitnessProgram"]
