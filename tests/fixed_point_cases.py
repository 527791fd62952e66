"""The fixed-point chip and the hint ops of witness programs: inputs, plain-integer references and hand-built tapes.  Nothing here comes
from the product: the hints are restated on Python's divmod (the signed forms by the route the reference takes, through the magnitude
and a ceiling), the chip's methods on signed integers, the tapes extend witness_cases.Tape."""
import random

import witness_cases as W

R = W.R
DIVQ, DIVR, ISZERO, INV = 8, 9, 10, 11
DIV_CONST, DIV_SIGNED = 1, 2
HALF = 1 << 252  # above it a signed dividend is negative
P = 32           # PRECISION_BITS of every test
ONE = 1 << P


# ---- the four ops ---------------------------------------------------------------------------------------------------------------------------
def ref_div(x: int, y: int, signed: bool) -> tuple:
    """(quotient mod r, remainder) of a canonical x by y"""
    if y == 0:
        return 0, 0
    if signed and x > HALF:
        m = R - x  # the magnitude
        ceil = -(-m // y)
        q = R - ceil
        return q, (x - y * q) % R  # = y * ceil - m, in [0, y)
    return divmod(x, y)


def ref_hint(kind: int, x: int, y: int = 0, flags: int = 0) -> int:
    if kind == ISZERO:
        return 1 if x == 0 else 0
    if kind == INV:
        return pow(x, R - 2, R) if x else 1
    return ref_div(x, y, bool(flags & DIV_SIGNED))[0 if kind == DIVQ else 1]


DIVIDENDS = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1, (1 << 65) - 1, 1 << 65, 1 << 128, HALF, HALF + 1, 1 << 253, R - (1 << 96), R - 2, R - 1]
DIVISORS = [0, 1, 2, 3, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 64, 1 << 65, (1 << 127) + 1, 1 << 253, R - 1]
EXACT_NEGATIVE = [(R - 6, 2), (R - 6, 3), (R - 6, 6), (R - (1 << 96), 1 << 64), (R - 3 * ONE, ONE), (R - 3 * ONE, 3)]  # -y * q exactly
UNARY = [0, 1, 2, R - 1, 1 << 253] + W.EDGES  # ISZERO and INV


def div_pairs() -> list:
    """every dividend with every listed divisor, with itself and with itself +- 1; the exact negative multiples"""
    pairs = []
    for x in DIVIDENDS:
        for y in DIVISORS + [x, x - 1, x + 1]:
            if 0 <= y < R and (x, y) not in pairs:
                pairs.append((x, y))
    return pairs + [p for p in EXACT_NEGATIVE if p not in pairs]


DIV_FORMS = [(kind, flags) for kind in (DIVQ, DIVR) for flags in (0, DIV_SIGNED)]  # each with a cell and with a constant as divisor


# ---- hand-built tapes ---------------------------------------------------------------------------------------------------------------------
class Tape(W.Tape):
    """witness_cases.Tape with hint cells: (kind, a, flags, 0, b)"""

    def hint(self, kind: int, a: int, b: int = 0, flags: int = 0, at=None) -> int:
        return self._add((kind, a, flags, 0, b), at)

    def div(self, kind: int, a: int, y_cell: int = None, y_const: int = None, signed: bool = False, at=None) -> int:
        """by the cell y_cell, or by the constant y_const"""
        flags = DIV_SIGNED if signed else 0
        if y_cell is not None:
            return self.hint(kind, a, y_cell, flags, at)
        if y_const not in self.constants:
            self.constants.append(y_const)
        return self.hint(kind, a, self.constants.index(y_const), flags | DIV_CONST, at)

    def value(self, v: int, how: int, inputs: list) -> int:
        """a cell holding v: an INPUT, a CONST or a GATE (v - 7 + 7 * 1 of three constants) by `how` mod 3"""
        if how % 3 == 0:
            inputs.append(v)
            return self.input(len(inputs) - 1)
        if how % 3 == 1:
            return self.const(v)
        self.const((v - 7) % R)
        self.const(7)
        self.const(1)
        return self.gate()

    @staticmethod
    def _operands(i, op) -> tuple:
        kind, a, flags = op[0], op[1], op[2]
        if kind == W.GATE:
            return (i - 3, i - 2, i - 1)
        if kind in (DIVQ, DIVR):
            return (a,) if flags & DIV_CONST else (a, op[4])
        return (a,) if kind in (W.COPY, W.LIMB, ISZERO, INV) else ()

    def levels(self) -> list:
        level = []
        for i, op in enumerate(self.cells):
            level.append(1 + max((level[s] for s in self._operands(i, op)), default=-1))
        return level

    def levelled(self, reverse: bool = False):
        """witness_cases.Tape.levelled with the second operand in the row's fourth word"""
        level = self.levels()
        by_level = [[] for _ in range(max(level, default=-1) + 1)]
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
                op = self.cells[i]
                rows.append((i, op[0] | op[2] << 8 | op[3] << 16, op[1], op[4] if len(op) == 5 else 0))
            ends.append(len(rows))
        return rows, ends

    def evaluate(self, inputs) -> list:
        out = []
        for i, op in enumerate(self.cells):
            kind, a, bits, shift = op[:4]
            if kind == W.INPUT:
                out.append(inputs[a] % R)
            elif kind == W.CONST:
                out.append(self.constants[a] % R)
            elif kind == W.COPY:
                out.append(out[a])
            elif kind == W.GATE:
                out.append((out[i - 3] + out[i - 2] * out[i - 1]) % R)
            elif kind == W.LIMB:
                out.append((out[a] >> shift) & ((1 << bits) - 1))
            elif kind in (DIVQ, DIVR):
                out.append(ref_hint(kind, out[a], self.constants[op[4]] if bits & DIV_CONST else out[op[4]], bits))
            else:
                out.append(ref_hint(kind, out[a]))
        return out


def ops_tape() -> tuple:
    """every pair of div_pairs in the four forms, by a cell and by a constant, and ISZERO / INV of UNARY; dividend and divisor cells are
    INPUT, CONST and GATE cells by turns -> (tape, inputs, [(cell, kind, x, y, flags)])"""
    t, inputs, listed = Tape(), [], []
    n = 0
    for x, y in div_pairs():
        xc, yc = t.value(x, n, inputs), t.value(y, n // 3 + 1, inputs)
        n += 1
        for kind, flags in DIV_FORMS:
            listed.append((t.div(kind, xc, y_cell=yc, signed=bool(flags)), kind, x, y, flags))
            listed.append((t.div(kind, xc, y_const=y, signed=bool(flags)), kind, x, y, flags | DIV_CONST))
    for i, x in enumerate(UNARY):
        xc = t.value(x, i, inputs)
        listed.append((t.hint(ISZERO, xc), ISZERO, x, 0, 0))
        listed.append((t.hint(INV, xc), INV, x, 0, 0))
    return t, inputs, listed


def layered_ops_tape(sizes, seed="hint layers") -> tuple:
    """levels of exactly these sizes: level 0 inputs, every later op a hint (or, one in five, a copy) of cells of the level below
    -> (tape, inputs)"""
    rng = random.Random(seed)
    t = Tape()
    pool = DIVIDENDS + DIVISORS + [rng.randrange(R) for _ in range(8)] + [rng.randrange(1 << 64) for _ in range(4)]
    inputs = [pool[j % len(pool)] for j in range(sizes[0])]
    below = [t.input(j) for j in range(sizes[0])]
    for size in sizes[1:]:
        level = []
        for i in range(size):
            a, b = below[rng.randrange(len(below))], below[rng.randrange(len(below))]
            pick = i % 5
            if pick == 0:
                level.append(t.copy(a))
            elif pick == 1:
                level.append(t.hint(rng.choice((ISZERO, INV)), a))
            elif pick == 2:
                level.append(t.div(rng.choice((DIVQ, DIVR)), a, y_const=rng.choice(DIVISORS), signed=bool(i & 8)))
            else:
                level.append(t.div(DIVQ if pick == 3 else DIVR, a, y_cell=b, signed=bool(i & 8)))
        below = level
    assert [t.levels().count(l) for l in range(len(sizes))] == list(sizes)
    return t, inputs


def quotient_chain_tape(levels: int, x: int) -> tuple:
    """x <- x div 7 (by a constant, odd levels) or x div y (by a cell) level after level, each beside the remainder that goes with it
    -> (tape, inputs, the last quotient's cell, its value)"""
    t = Tape()
    cell, y = t.input(0), t.input(1)
    value = x
    for l in range(levels):
        by = dict(y_const=7) if l % 2 else dict(y_cell=y)
        t.div(DIVR, cell, **by)
        cell = t.div(DIVQ, cell, **by)
        value //= 7 if l % 2 else 5
    return t, [x, 5], cell, value


# ---- the chip on signed integers -----------------------------------------------------------------------------------------------------------
def to_field(s: int) -> int:
    return s % R


def to_signed(v: int) -> int:
    return v - R if v > HALF else v


def sgn(s: int) -> int:
    return -1 if s < 0 else 1


REF = {
    "qadd": lambda a, b: a + b,
    "qsub": lambda a, b: a - b,
    "neg": lambda a: -a,
    "qabs": abs,
    "sign": sgn,
    "is_neg": lambda a: int(a < 0),
    "clip": lambda a: sgn(a) * (abs(a) % (1 << (2 * P))),
    "qmul": lambda a, b: (a * b) >> P,  # toward minus infinity
    "qdiv": lambda a, b: sgn(a) * sgn(b) * ((abs(a) << P) // abs(b)),
    "qmod": lambda a, b: a % b if a >= 0 else b - (-a) % b,
    "qmax": max,
    "qmin": min,
}


def ref_polynomial(x: int, coef) -> int:
    acc = 0
    for i, c in enumerate(coef):
        acc += c
        if i < len(coef) - 1:
            acc = (x * acc) >> P
    return acc


def ref_inner_product(a, b) -> int:
    return sum((x * y) >> P for x, y in zip(a, b))


def ref_inference(x, w, b) -> int:
    return ref_inner_product(w, x) + b


def ref_train(w, b, x, y, rate) -> tuple:
    """one step of src/gadget/linear_regression.rs on signed integers -> (w, b)"""
    diff = [ref_inner_product(xi, w) + b - ti for xi, ti in zip(x, y)]
    new_w = [wj - ((rate * sum((d * xi[j]) >> P for d, xi in zip(diff, x))) >> P) for j, wj in enumerate(w)]
    return new_w, b - ((rate * sum(diff)) >> P)


BIG = 1 << 48  # BIG * BIG / 2^P = 2^64: below the 2^(2P+1) from which a positive value reads as negative
EDGE = [0, 1, -1, ONE - 1, -(ONE - 1), ONE, -ONE, BIG, -BIG]
PAIRS = [(a, b) for i, a in enumerate(EDGE) for j, b in enumerate(EDGE) if i == j or a == -b or (i + j) % 3 == 0]
# the largest magnitudes the bounds allow.  qmul: a positive quotient stays below 2^(2P+1) (qabs reads it by is_neg), a negative one's
# magnitude below 2^(3P); qdiv: |a| 2^P < 2^(4P) with a positive a below 2^(2P+1), 0 < |b| < 2^(2P); qmod: |a| < 2^(4P) likewise, 0 < b < 2^(2P)
QMUL_EXTREME = [((1 << 64) - 1, (1 << 33) - 1), (-((1 << 64) - 1), (1 << 64) - 1), ((1 << 64) - 1, -((1 << 64) - 1)), (-((1 << 64) - 1), -((1 << 33) - 1))]
QDIV_EXTREME = [((1 << 65) - 1, 1), (-((1 << 96) - 1), 1), ((1 << 65) - 1, -((1 << 64) - 1)), (-((1 << 96) - 1), (1 << 64) - 1), (1, (1 << 64) - 1)]
QMOD_EXTREME = [((1 << 65) - 1, (1 << 64) - 1), (-((1 << 96) - 1), (1 << 64) - 1), ((1 << 65) - 1, 1), (-((1 << 96) - 1), 1)]

# proofs: (x, w, b) for inference with 3 features, (w, b, x, y, rate) for one step on 2 samples x 2 features; signed integers at scale 2^32.
# Negative values, and an exact zero difference: the second training set predicts its first target exactly
q = lambda x: int(round(x * ONE))
INFERENCE_DUMMY = ([0, 0, 0], [0, 0, 0], 0)
INFERENCE_INPUTS = [([q(0.5), q(-1.25), q(3.0)], [q(-0.3), q(0.7), q(0.1)], q(0.2)),
                    ([q(-0.5), q(1.25), 0], [q(-0.3), q(-0.7), q(0.1)], q(-0.2)),
                    ([-1, 1, -(ONE - 1)], [ONE, -ONE, ONE - 1], -1)]
TRAIN_DUMMY = ([0, 0], 0, [[0, 0], [0, 0]], [0, 0], 0)
TRAIN_INPUTS = [([q(0.25), q(-0.5)], q(0.1), [[q(1.5), q(-2.0)], [q(-0.75), q(0.5)]], [q(3.0), q(-1.0)], q(0.01 / 2)),
                ([ONE, -ONE], q(0.5), [[q(2.0), q(1.0)], [q(-1.0), q(-3.0)]], [q(1.5), q(-2.5)], q(0.05)),
                ([-3, 5], -q(0.125), [[-ONE, ONE - 1], [1, -1]], [q(-0.001), q(7.0)], q(0.25))]


def field_inputs(inputs):
    """nested signed integers -> the same shape in the field"""
    return type(inputs)(field_inputs(v) for v in inputs) if isinstance(inputs, (list, tuple)) else to_field(inputs)
