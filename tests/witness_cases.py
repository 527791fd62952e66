"""Witness programs: the closures the recorder is run on, hand-built tapes for the kernel tests, and their Python-integer references.
A hand-built tape is a list of cells in program order, each (kind, a, bits, shift); `levelled` sorts it into levels by the rule of
include/h2mi.h (INPUT and CONST at level 0, any other op one above its highest operand) without the recorder's code, `evaluate` computes
every cell on Python integers without the interpreter of witness.Program."""
import random

R = 0x30644E72E131A029B85045B68181585D2833E84879B97091_43E1F593F0000001
INPUT, CONST, COPY, GATE, LIMB = range(5)
WG_OPS, WG_LEVELS = 1024, 4096
STEP = 0x9E3779B97F4A7C15  # flex.RANGE_MANY_STEP
MASK64 = (1 << 64) - 1
R_INV = pow(1 << 256, -1, R)


# ---- closures f(ctx, inputs, make_public), as the scaffold takes them ------------------------------------------------------------------
def gate_closure(ctx, x, make_public):
    """x^2 + 72 three ways, written with instructions only (examples/halo2_lib.rs without its hand-assigned region)"""
    xc = ctx.load_witness(x)
    make_public.append(xc)
    x_sq = ctx.mul(xc, xc)
    make_public.append(ctx.add_constant(x_sq, 72))
    ctx.mul_add_constant(xc, xc, 72)
    c = ctx.add(x_sq, xc)
    ctx.mul(c, x_sq)


def range_closure(ctx, xs, make_public):
    """flex.range_closure's body for every value of the list xs: range_check(x, 64), x + x, every value public"""
    for x in xs:
        xc = ctx.load_witness(x)
        make_public.append(xc)
        ctx.range_check(xc, 64, ctx.lookup_bits)
        ctx.add(xc, xc)


def range_inputs(x: int, count: int) -> list:
    """the values flex.range_closure(cs, x, lookup_bits, count) checks"""
    return [(x + i * STEP) & MASK64 for i in range(count)]


# ---- hand-built tapes ---------------------------------------------------------------------------------------------------------------------
class Tape:
    def __init__(self, n_inputs: int = 0):
        self.cells, self.constants, self.n_inputs = [], [], n_inputs  # cells: (kind, a, bits, shift) in program order
        self.position = {}  # cell -> the position asked for inside its level (cells without one follow, in cell order)

    def _add(self, op, at=None) -> int:
        self.cells.append(op)
        if at is not None:
            self.position[len(self.cells) - 1] = at
        return len(self.cells) - 1

    def input(self, j: int, at=None) -> int:
        self.n_inputs = max(self.n_inputs, j + 1)
        return self._add((INPUT, j, 0, 0), at)

    def const(self, v: int, at=None) -> int:
        if v not in self.constants:
            self.constants.append(v)
        return self._add((CONST, self.constants.index(v), 0, 0), at)

    def copy(self, s: int, at=None) -> int:
        return self._add((COPY, s, 0, 0), at)

    def gate(self, at=None) -> int:
        return self._add((GATE, 0, 0, 0), at)

    def limb(self, s: int, shift: int, bits: int, at=None) -> int:
        return self._add((LIMB, s, bits, shift), at)

    def levels(self) -> list:
        level = []
        for i, (kind, a, _, _) in enumerate(self.cells):
            operands = (i - 3, i - 2, i - 1) if kind == GATE else (a,) if kind in (COPY, LIMB) else ()
            level.append(1 + max((level[s] for s in operands), default=-1))
        return level

    def levelled(self, reverse: bool = False):
        """-> (ops rows (dst, code, a, 0) sorted by level, level_ends).  Inside a level: the cells with a position at it (the gaps are
        the tape's to fill), the others in cell order — or, reverse, everything in descending cell order"""
        level = self.levels()
        n_levels = max(level, default=-1) + 1
        by_level = [[] for _ in range(n_levels)]
        for i, l in enumerate(level):
            by_level[l].append(i)
        rows, ends = [], []
        for members in by_level:
            if reverse:
                order = sorted(members, reverse=True)
            else:
                fixed = {self.position[i]: i for i in members if i in self.position}
                rest = iter(i for i in members if i not in self.position)
                order = [fixed[p] if p in fixed else next(rest) for p in range(len(members))]
            for i in order:
                kind, a, bits, shift = self.cells[i]
                rows.append((i, kind | bits << 8 | shift << 16, a, 0))
            ends.append(len(rows))
        return rows, ends

    def evaluate(self, inputs) -> list:
        out = []
        for i, (kind, a, bits, shift) in enumerate(self.cells):
            if kind == INPUT:
                out.append(inputs[a] % R)
            elif kind == CONST:
                out.append(self.constants[a] % R)
            elif kind == COPY:
                out.append(out[a])
            elif kind == GATE:
                out.append((out[i - 3] + out[i - 2] * out[i - 1]) % R)
            else:
                out.append((out[a] >> shift) & ((1 << bits) - 1))
        return out

    def program(self, witness, checks=(), placement=None, reverse: bool = False):
        """the tape as a witness.Program; placement None: one column holding every cell in order"""
        rows, ends = self.levelled(reverse)
        placement = [list(range(len(self.cells)))] if placement is None else placement
        return witness.Program(rows, ends, self.constants, self.n_inputs, checks, placement, [])


def segmentation(sizes) -> tuple:
    """(grid launches, single-workgroup launches) of levels of these sizes, counted as the rule of include/h2mi.h reads: a level of more
    than 1024 ops is one grid launch; a maximal run of narrower levels is ceil(length / 4096) workgroup launches"""
    grid = sum(1 for s in sizes if s > WG_OPS)
    wg, run = 0, 0
    for s in list(sizes) + [WG_OPS + 1]:
        if s > WG_OPS:
            wg += -(-run // WG_LEVELS)
            run = 0
        else:
            run += 1
    return grid, wg


# field values at the limb extremes: canonical and Montgomery words of all ones, the ends of the field, powers of two
EDGES = [0, 1, R - 1, MASK64, 1 << 253, (1 << 253) - 1, (1 << 192) - 1, ((1 << 253) - 1) * R_INV % R, MASK64 * R_INV % R, R_INV,
         0x2AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA]


def values_tape() -> tuple:
    """every triple (a, b, c) of EDGES as a + b * c: the operands as INPUT, CONST or COPY cells by turns, the result copied once more.
    Level 0 is wide (a grid launch), the gates and copies narrow or wide with the number of edges -> (tape, inputs)"""
    t, inputs = Tape(), list(EDGES)
    first = [t.input(j) for j in range(len(EDGES))]
    n = 0
    for ia, a in enumerate(EDGES):
        for ib, b in enumerate(EDGES):
            for ic, c in enumerate(EDGES):
                for pick, (j, v) in enumerate(((ia, a), (ib, b), (ic, c))):
                    how = (n + pick) % 3
                    if how == 0:
                        t.input(j)
                    elif how == 1:
                        t.const(v)
                    else:
                        t.copy(first[j])
                g = t.gate()
                if n % 5 == 0:
                    t.copy(g)
                n += 1
    return t, inputs


LIMB_SHIFTS = [0, 31, 32, 33, 63, 64, 65, 127, 128, 191, 192, 250]
LIMB_BITS = [1, 4, 12, 13, 31, 32, 33, 64]
LIMB_SOURCES = [R - 1, (1 << 253) - 1, 1 << 253, MASK64, 0x2AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA,
                random.Random("limb source").randrange(R), 1, 0]


def limb_tape() -> tuple:
    """LIMB at every shift x bits with shift + bits <= 254, of every source -> (tape, inputs, [(cell, source value, shift, bits)])"""
    t, listed = Tape(), []
    src = [t.input(j) for j in range(len(LIMB_SOURCES))]
    for j, v in enumerate(LIMB_SOURCES):
        for shift in LIMB_SHIFTS:
            for bits in LIMB_BITS:
                if shift + bits <= 254:
                    listed.append((t.limb(src[j], shift, bits), v, shift, bits))
    return t, list(LIMB_SOURCES), listed


def layered_tape(sizes, seed="layers") -> tuple:
    """levels of exactly these sizes: level 0 inputs, every later op a COPY or a LIMB of a cell of the level below -> (tape, inputs)"""
    rng = random.Random(seed)
    t = Tape()
    inputs = [rng.randrange(R) for _ in range(sizes[0])]
    below = [t.input(j) for j in range(sizes[0])]
    for size in sizes[1:]:
        level = []
        for i in range(size):
            s = below[rng.randrange(len(below))]
            if i % 3 == 2:
                bits = rng.choice(LIMB_BITS)
                level.append(t.limb(s, rng.randrange(0, 70), bits))
            else:
                level.append(t.copy(s))
        below = level
    assert [t.levels().count(l) for l in range(len(sizes))] == list(sizes)
    return t, inputs


def square_chain_tape(steps: int, x: int, c: int) -> tuple:
    """x <- c + x * x, `steps` times: two levels per step (the two copies of x, then the gate).  Inside its level every op of the chain
    sits at another lane, in another wavefront, than the ops that wrote its operands: the copies at lanes 64 + .., the gates at lanes
    0 .. 10, both moving from step to step; the lanes in front of them are copies of cells of the level below
    -> (tape, inputs, the cell of the last x, its value)"""
    t = Tape()
    x_cell = t.input(0)
    value = x % R
    at = lambda level: (level % 2) * 64 + (level * 5) % 11
    for step in range(steps):
        lc, lg = 2 * step + 1, 2 * step + 2  # the levels of the copies and of the gate
        prev = x_cell
        t.const(c)
        first = t.copy(prev, at=at(lc))
        t.copy(prev, at=at(lc) + 1)
        x_cell = t.gate(at=at(lg))
        value = (c + value * value) % R
        for _ in range(at(lc)):
            t.copy(prev)
        for _ in range(at(lg)):
            t.copy(first)
    return t, [x], x_cell, value


def one_op_chain_tape(levels: int, x: int) -> tuple:
    """`levels` levels of one op above the input: copies and 64-bit limbs of a value below 2^64 by turns -> (tape, inputs, last cell)"""
    t = Tape()
    cell = t.input(0)
    for l in range(levels):
        cell = t.copy(cell) if l % 2 else t.limb(cell, 0, 64)
    return t, [x & MASK64], cell
