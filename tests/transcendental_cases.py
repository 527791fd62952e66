"""The MSB / POW2 hint ops and the fixed-point chip's exp, log and sin family: operands, plain-integer references, error bounds against
floats and hand-built tapes.  Nothing here comes from the product.  The two ops are restated on int.bit_length; the chip's methods on
signed Python integers with the floors, coefficient roundings and range bounds of the circuit, an operand no witness can satisfy being
an Unsat; the float bounds are derived rounding by rounding below; the tapes extend fixed_point_cases.Tape."""
import math

import fixed_point_cases as FC
import witness_cases as W

R = W.R
MSB, POW2 = 13, 14
POW2_OF_MSB = 1
DIVQ = FC.DIVQ
NUM_BITS = 254


# ---- the two ops ----------------------------------------------------------------------------------------------------------------------------
def ref_msb(x: int) -> int:
    """the index of the highest set bit; 1 for zero, as a fold over the bits that starts at 1 leaves it"""
    return x.bit_length() - 1 if x else 1


def ref_pow2(x: int, of_msb: bool = False) -> int:
    e = ref_msb(x) if of_msb else x
    return 1 << e if e <= 253 else 0


MSB_OPERANDS = [0, 1, 2, 3] + [v for k in (31, 32, 33, 63, 64, 65, 127, 128, 224, 252, 253) for v in ((1 << k) - 1, 1 << k, (1 << k) + 1)] + [R - 1]
POW2_OPERANDS = list(range(256)) + [256, (1 << 32) - 1, 1 << 32, 1 << 64, R - 1]
assert all(0 <= v < R for v in MSB_OPERANDS + POW2_OPERANDS)


class Tape(FC.Tape):
    """fixed_point_cases.Tape with MSB and POW2 cells: (kind, a, flags, 0, 0)"""

    def msb(self, a: int, at=None) -> int:
        return self._add((MSB, a, 0, 0, 0), at)

    def pow2(self, a: int, of_msb: bool = False, at=None) -> int:
        return self._add((POW2, a, POW2_OF_MSB if of_msb else 0, 0, 0), at)

    @staticmethod
    def _operands(i, op) -> tuple:
        return (op[1],) if op[0] in (MSB, POW2) else FC.Tape._operands(i, op)

    def evaluate(self, inputs) -> list:
        """fixed_point_cases.Tape.evaluate, the two ops beside the others"""
        out = []
        for i, op in enumerate(self.cells):
            kind, a, bits, shift = op[:4]
            if kind == MSB:
                out.append(ref_msb(out[a]))
            elif kind == POW2:
                out.append(ref_pow2(out[a], bool(bits & POW2_OF_MSB)))
            elif kind == W.INPUT:
                out.append(inputs[a] % R)
            elif kind == W.CONST:
                out.append(self.constants[a] % R)
            elif kind == W.COPY:
                out.append(out[a])
            elif kind == W.GATE:
                out.append((out[i - 3] + out[i - 2] * out[i - 1]) % R)
            elif kind == W.LIMB:
                out.append((out[a] >> shift) & ((1 << bits) - 1))
            elif kind in (FC.DIVQ, FC.DIVR):
                out.append(FC.ref_hint(kind, out[a], self.constants[op[4]] if bits & FC.DIV_CONST else out[op[4]], bits))
            else:
                out.append(FC.ref_hint(kind, out[a]))
        return out


def ops_tape() -> tuple:
    """MSB and flagged POW2 of every MSB operand, POW2 of every POW2 operand; the operand cells are INPUT, CONST and GATE cells by turns
    -> (tape, inputs, [(cell, the value it must hold)])"""
    t, inputs, listed = Tape(), [], []
    for n, x in enumerate(MSB_OPERANDS):
        xc = t.value(x, n, inputs)
        listed.append((t.msb(xc), ref_msb(x)))
        listed.append((t.pow2(xc, of_msb=True), ref_pow2(x, True)))
    for n, x in enumerate(POW2_OPERANDS):
        listed.append((t.pow2(t.value(x, n + 1, inputs)), ref_pow2(x)))
    return t, inputs, listed


def layered_ops_tape(sizes) -> tuple:
    """levels of exactly these sizes: level 0 inputs (the operands of both lists by turns), every later op an MSB, a POW2, a flagged POW2
    or — one in four — one of the old hints, of a cell of the level below -> (tape, inputs)"""
    t = Tape()
    pool = MSB_OPERANDS + POW2_OPERANDS
    inputs = [pool[(7 * j) % len(pool)] for j in range(sizes[0])]
    below = [t.input(j) for j in range(sizes[0])]
    for depth, size in enumerate(sizes[1:]):
        level = []
        for i in range(size):
            a = below[(i * 13 + depth) % len(below)]
            pick = (i + depth) % 4
            level.append(t.msb(a) if pick == 0 else t.pow2(a) if pick == 1 else t.pow2(a, of_msb=True) if pick == 2 else
                         t.hint(FC.ISZERO if i & 4 else FC.INV, a))
        below = level
    assert [t.levels().count(l) for l in range(len(sizes))] == list(sizes)
    return t, inputs


CHAIN_DIVIDENDS = [R - 12345, (1 << 190) + 987654321]


def msb_pow2_div_chain_tape(levels: int, x: int) -> tuple:
    """x -> MSB(x) -> 2^MSB(x) -> y div 2^MSB(x) -> MSB of that -> ..., y the two dividends by turns: one op per level, at least `levels`
    levels above the inputs -> (tape, inputs, last cell, its value)"""
    t = Tape()
    cell, value = t.input(0), x % R
    ys = [t.input(1), t.input(2)]
    n = 0
    while len(set(t.levels())) <= levels:
        p = t.pow2(t.msb(cell))
        cell = t.div(DIVQ, ys[n % 2], y_cell=p)
        value = CHAIN_DIVIDENDS[n % 2] >> ref_msb(value)
        n += 1
    return t, [x] + CHAIN_DIVIDENDS, cell, value


# ---- the chip on signed integers ---------------------------------------------------------------------------------------------------------------
class Unsat(Exception):
    """no witness satisfies the circuit on this operand"""


EXP2_COEF = (3.6240421303547230336183979205877e-11, 4.1284327467833130245549169910389e-10, 0.0000000071086385644026346316624185550542,
             0.00000010172297085296590958930245291448, 0.0000013215904023658396206789543841996, 0.000015252713316417140696221389106544,
             0.00015403531076657894204857389177279, 0.0013333558131297097698435464957392, 0.0096181291078409107025643582456283,
             0.055504108664804181586140094858174, 0.24022650695910142332414229540187, 0.69314718055994529934452147700678, 1.0)
LOG_COEF = (-3.319586265362338e-08, 1.4957235315170112e-06, -3.1350053389526744e-05, 0.00040554177582512901, -0.0036218342998850703,
            0.023663846121538389, -0.11691877183255484, 0.44524062371564499, -1.3195777548208449, 3.0518128028712077, -5.4904626000399528,
            7.6298580090181591, -8.1653313719804235, 7.1389971101896279, -3.1937385492842112)
SIN_COEF = (-1.1008071636607462e-11, 2.4208013888629323e-10, -3.8584805817996712e-10, -2.3786993104309845e-08, -2.9795813710683115e-09,
            2.7608543130047009e-06, -6.4467066994122565e-09, -0.00019840680551418068, -3.839555844512214e-09, 0.0083333350601673614,
            -5.0943769725466814e-10, -0.16666666657583049, -8.5029878414113731e-12, 1.0000000000003146, -1.9323057584419828e-15)
# the Remez errors the reference states beside the lists: "precision bits: 64.28" on values in [1, 2], and two estimated maxima
REMEZ = {"exp2": 2.0 * 2.0 ** -64.28, "log": 6.4897885416380772e-13, "sin": 1.9323057584419826e-15}


class Model:
    """the chip's methods on signed integers at scale 2^P.  A negative number is a negative integer; is_neg reads a value of 2^(2P+1) or
    more as negative, which no method survives: such a value is an Unsat wherever a sign is taken."""

    def __init__(self, P: int):
        self.P, self.one = P, 1 << P
        self.top = 1 << (2 * P + 1)  # is_neg's threshold

    def q(self, x: float) -> int:
        """round(|x| 2^P), halves away from zero, with the sign of x: a double of 2^52 or more is an integer already"""
        v = abs(x) * float(self.one)
        n = int(v) if v >= 2.0 ** 52 else int(math.floor(v + 0.5))
        return -n if x < 0 else n

    def real(self, v: int) -> float:
        return v / float(self.one)

    def signed(self, v: int) -> int:
        """a value whose sign a method takes"""
        if not -(R >> 1) < v < self.top:
            raise Unsat("read as negative")
        return v

    def qmul(self, a: int, b: int) -> int:
        div = (a * b) >> self.P  # toward minus infinity
        if not -(1 << (3 * self.P)) < div < self.top:
            raise Unsat("signed_div_scale's bound")
        return div

    def div_mod_var(self, a: int, b: int, a_bits: int, b_bits: int) -> tuple:
        """of non-negative integers: the quotient below 2^a_bits, rem < b <= rem + 2^b_bits"""
        if b <= 0:
            raise Unsat("no remainder below a zero divisor")
        div, rem = divmod(a, b)
        if div >> a_bits or b - rem > 1 << b_bits:
            raise Unsat("div_mod_var's bounds")
        return div, rem

    def qdiv(self, a: int, b: int) -> int:
        a, b = self.signed(a), self.signed(b)
        div, _ = self.div_mod_var(abs(a) << self.P, abs(b), 4 * self.P, 2 * self.P)
        return -div if (a < 0) != (b < 0) else div

    def qmod(self, a: int, b: int) -> int:
        a = self.signed(a)
        _, rem = self.div_mod_var(abs(a), b, 4 * self.P, 2 * self.P)
        return b - rem if a < 0 else rem

    def polynomial(self, x: int, coef) -> int:
        acc = 0
        for i, c in enumerate(coef):
            acc += self.q(c)
            if i < len(coef) - 1:
                acc = self.qmul(x, acc)
        return acc

    def qexp2(self, a: int) -> int:
        a = self.signed(a)
        int_part, frac = divmod(abs(a), self.one)
        if int_part > self.one:
            raise Unsat("div_mod's bound on the integer part")
        pow2 = 1 << int_part if int_part < NUM_BITS else 0  # select_from_idx beyond the table: no indicator is set
        res_pos = pow2 * self.polynomial(frac, EXP2_COEF)
        if res_pos >= R:
            raise Unsat("2^int wraps the field")
        res_neg = self.qdiv(self.one, res_pos)  # computed for either sign
        return res_neg if a < 0 else res_pos

    def qlog2(self, a: int) -> int:
        P = self.P
        if self.signed(a) <= 0:
            raise Unsat("qlog2 of zero or of a negative number")
        exp1 = a.bit_length() - 1
        if exp1 + 1 > 2 * P - 1:
            raise Unsat("2^(exp1 + 1) has no bit among check_power_of_two's 2P")
        shift = P + 1 - exp1
        a_norm = a << shift if shift >= 0 else a >> -shift
        return self.polynomial(a_norm, LOG_COEF) - shift * self.one

    def qsin(self, a: int) -> int:
        a = self.signed(a)
        a_mod = self.qmod(abs(a), self.q(math.pi * 2.0))
        a_mpi = a_mod - self.q(math.pi)
        sin_a_mod, sin_a_mpi = self.polynomial(a_mod, SIN_COEF), -self.polynomial(a_mpi, SIN_COEF)  # both are computed
        sin_abs = sin_a_mod if a_mpi < 0 else sin_a_mpi
        return -sin_abs if a < 0 else sin_abs

    def qcos(self, a: int) -> int:
        return self.qsin(a + self.q(math.pi / 2.0))

    def qtan(self, a: int) -> int:
        return self.qdiv(self.qsin(a), self.qcos(a))

    def qexp(self, a: int) -> int:
        return self.qexp2(self.qdiv(a, self.q(math.log(2.0))))

    def qsinh(self, a: int) -> int:
        return self.qdiv(self.qexp(a) - self.qexp(-a), self.q(2.0))

    def qcosh(self, a: int) -> int:
        return self.qdiv(self.qexp(a) + self.qexp(-a), self.q(2.0))

    def qtanh(self, a: int) -> int:
        return self.qdiv(self.qsinh(a), self.qcosh(a))

    def qlog(self, a: int) -> int:
        return self.qdiv(self.qlog2(a), self.q(math.log2(math.e)))

    def qpow(self, x: int, e: int) -> int:
        return self.qexp(self.qmul(e, self.qlog(x)))

    def qsqrt(self, x: int) -> int:
        return self.qpow(x, self.q(0.5))

    def sigmoid(self, logit: int) -> int:
        return self.qdiv(self.one, self.qexp(-logit) + self.one)

    def inner_product(self, a, b) -> int:
        return sum(self.qmul(x, y) for x, y in zip(a, b))

    def logistic_inference(self, x, w, b) -> int:
        return self.sigmoid(self.inner_product(w, x) + b)

    def logistic_train(self, w, b, x, y, rate) -> tuple:
        """src/gadget/logistic_regression.rs's train_multi_batch on signed integers: x[batch][sample][feature] -> (w, b)"""
        w = list(w)
        for bx, by in zip(x, y):
            diff = [self.sigmoid(self.inner_product(w, xi) + b) - ti for xi, ti in zip(bx, by)]
            w = [wj - self.qmul(rate, sum(self.qmul(d, xi[j]) for d, xi in zip(diff, bx))) for j, wj in enumerate(w)]
            b = b - self.qmul(rate, sum(diff))
        return w, b


def edge_operands(P: int) -> dict:
    """method -> the operands (tuples of signed integers) of its edge cases at this precision"""
    m = Model(P)
    one, ulp = m.one, 1
    pi, two_pi = m.q(math.pi), m.q(math.pi * 2.0)
    exp2 = [0] + [s * v for v in (ulp, one - ulp, one) for s in (1, -1)]
    # integer parts 0 (above), 1, P - 1, P (the last with a reciprocal to divide by), P + 1 (the first without), 2P - 2, and the ends of the table
    exp2 += [s * (i * one + f) for i in (1, P - 1, P, P + 1, 2 * P - 2, 253, 254) for f in (0, one // 3) for s in (1, -1) if i * one + f < m.top]
    log2 = [ulp, one - ulp, one, 2 * one - ulp, 2 * one, 1 << (P - 1),
            (1 << (2 * P - 1)) - 1,                       # the largest value check_power_of_two's 2P bits admit
            1 << (2 * P - 1), 0, -one,                    # and what they do not
            1 << (P + 1), (1 << (P + 1)) - 1,             # shift = 0, and the last positive shift
            1 << (P + 2), 3 << (P + 5), (1 << (P + 2)) + 1]  # negative shifts
    sin = [0, pi - 1, pi, pi + 1, -(pi - 1), -pi, -(pi + 1), two_pi - 1, -(two_pi - 1), two_pi, two_pi + 1, -(two_pi + 1), 5 * two_pi, -3 * two_pi,
           m.q(1.0), m.q(4.0), m.q(-2.5), m.q(100.0)]  # both branches of is_neg_a_mpi among them
    few = [m.q(v) for v in (0.0, 0.5, -0.5, 1.25, -3.0)]
    return {"qexp2": [(v,) for v in exp2], "qlog2": [(v,) for v in log2], "qsin": [(v,) for v in sin],
            "qcos": [(v,) for v in (0, pi, -pi, m.q(1.0), m.q(-2.0))], "qtan": [(v,) for v in (0, m.q(1.0), m.q(-0.7))],
            "qexp": [(v,) for v in few + [m.q(20.0), m.q(-20.0), m.q(30.0)]], "qsinh": [(v,) for v in few[:3]], "qcosh": [(v,) for v in few[:3]],
            "qtanh": [(v,) for v in few[:3]], "qlog": [(v,) for v in (ulp, one, m.q(0.3), m.q(math.e), m.q(1000.0), 0)],
            "qpow": [(m.q(2.0), m.q(3.0)), (m.q(9.0), m.q(0.5)), (m.q(0.5), m.q(-2.0)), (0, one)], "qsqrt": [(m.q(2.0),), (m.q(0.25),), (one,)]}


P63_OPERANDS = {"qexp": [0.0, 0.5, -0.5, 1.25, -3.0, 20.0, -20.0], "qlog": [2.0 ** -63, 1.0, 0.3, math.e, 1000.0]}  # reals, quantised by the model


# ---- against floats ---------------------------------------------------------------------------------------------------------------------------
# With u = 2^-P.  Horner over n + 1 coefficients (leading first) at a quantised x: acc_0 is the quantised c_0, within u/2 of it; step i
# multiplies the accumulator's error by |x|, floors the product (less than u) and adds a quantised c_i (u/2): e_i <= |x| e_(i-1) + 3u/2.  So
# the polynomial is within  horner(|x|, n) = u/2 |x|^n + 3u/2 (|x|^(n-1) + .. + 1)  of its real value, and within that plus the Remez error
# of the function.  At P = 32 and x near 4 the leading terms of the log polynomial make this a bound of a few percent: the coefficients of a
# degree-14 polynomial on [2, 4] do not fit 32 fractional bits, which is the reference's property and the reason it runs the chip at P = 63.
# The comparisons are made in doubles: every bound adds DOUBLE = 2^-50 times the magnitude for the doubles' own rounding.
DOUBLE = 2.0 ** -50


def horner(P: int, x: float, n: int) -> float:
    u = 2.0 ** -P
    return u / 2 * abs(x) ** n + 1.5 * u * sum(abs(x) ** j for j in range(n))


def quotient_error(v: float, ev: float, c: float, ec: float, u: float) -> float:
    """|floor(v^ / c^) - v / c| for |v^ - v| <= ev, |c^ - c| <= ec < |c|, the quotient floored to a multiple of u"""
    return ev / (abs(c) - ec) + abs(v) * ec / (abs(c) * (abs(c) - ec)) + u


def exp2_bound(P: int, x: float, dx: float = 0.0) -> tuple:
    """-> (2^x, the bound on the chip's error) for an operand within dx of x: 2^int scales the polynomial's error on the fraction; a
    negative operand takes the reciprocal, floored"""
    u = 2.0 ** -P
    v = 2.0 ** abs(x)
    e = 2.0 ** math.floor(abs(x) + dx) * (horner(P, 1.0, 12) + REMEZ["exp2"]) + v * (2.0 ** dx - 1.0)
    if x < 0:
        e = quotient_error(1.0, 0.0, v, e, u)
        v = 1.0 / v
    return v, e + DOUBLE * v


def exp_bound(P: int, x: float, dx: float = 0.0) -> tuple:
    """e^x = 2^(x / ln 2): the quotient by the quantised ln 2 (u/2) is floored (u)"""
    u = 2.0 ** -P
    v, e = exp2_bound(P, x / math.log(2.0), quotient_error(x, dx, math.log(2.0), u / 2, u))
    return math.exp(x), e + DOUBLE * v


def log2_bound(P: int, x: float) -> tuple:
    """the operand is shifted into [2, 4) — a right shift floors it, u on a value of 2 or more —, the polynomial runs there"""
    u = 2.0 ** -P
    norm = x / 2.0 ** (math.floor(math.log2(x)) - 1)
    e = horner(P, norm, 14) + REMEZ["log"] + (u / (2.0 * math.log(2.0)) if x >= 4.0 else 0.0)
    return math.log2(x), e + DOUBLE * (abs(math.log2(x)) + 1.0)


def log_bound(P: int, x: float) -> tuple:
    u = 2.0 ** -P
    v, e = log2_bound(P, x)
    return math.log(x), quotient_error(v, e, math.log2(math.e), u / 2, u) + DOUBLE


def sin_bound(P: int, x: float, dx: float = 0.0) -> tuple:
    """|x| is reduced by k times the quantised 2 pi (k u/2), the quantised pi is taken off on the upper half (u/2), the polynomial runs on
    a value of at most pi + u (one more u for the end of the Remez interval)"""
    u = 2.0 ** -P
    k = math.floor(abs(x) / (2.0 * math.pi))
    reduced = abs(x) - k * 2.0 * math.pi
    at = reduced if reduced < math.pi else reduced - math.pi
    e = horner(P, min(at + 2 * u + dx, math.pi + u), 14) + REMEZ["sin"] + k * u / 2 + u / 2 + u + dx
    return math.sin(x), e + DOUBLE * (1.0 + abs(x))


def cos_bound(P: int, x: float) -> tuple:
    u = 2.0 ** -P
    _, e = sin_bound(P, x + math.pi / 2.0, u / 2)  # the quantised pi / 2
    return math.cos(x), e


FLOAT_CASES = {  # method -> (bound, the reals it is compared at); P = 32, and qexp / qlog at P = 63 too
    "qexp2": (exp2_bound, [0.0, 0.5, -0.5, 1.999, -1.999, 7.25, -7.25, 20.0, -20.0, 31.75, -31.75]),
    "qexp": (exp_bound, [0.0, 0.7, -0.3, 1.0, -1.0, 5.0, -5.0, 20.0, -20.0]),
    "qlog2": (log2_bound, [2.0 ** -20, 0.001, 0.75, 1.0, 1.5, 2.0, 3.999, 4.0, 10.0, 1000.0, 2.0 ** 20]),
    "qlog": (log_bound, [0.001, 0.3, 1.0, math.e, 10.0, 12345.678]),
    "qsin": (sin_bound, [0.0, 0.5, -0.5, 1.5707963, 3.0, 3.2, -3.2, 6.0, 6.5, -7.0, 100.0, -1000.0]),
    "qcos": (cos_bound, [0.0, 0.5, -0.5, 1.5707963, 3.0, -4.0, 10.0]),
}
FLOAT_CASES_63 = {"qexp": FLOAT_CASES["qexp"], "qlog": FLOAT_CASES["qlog"]}


# ---- proofs ------------------------------------------------------------------------------------------------------------------------------------
def q63(x: float) -> int:
    return Model(63).q(x)


def q32(x: float) -> int:
    return Model(32).q(x)


# logistic inference with 2 features, (x, w, b), and one training step of 2 samples x 2 features, (w, b, x, y, rate) with x one batch; P = 63
INFERENCE_DUMMY = ([0, 0], [0, 0], 0)
INFERENCE_INPUTS = [([q63(0.5), q63(-1.25)], [q63(-0.3), q63(0.7)], q63(0.2)),
                    ([q63(-2.0), q63(3.0)], [q63(1.5), q63(-0.25)], q63(-0.125)),
                    ([-1, 1], [(1 << 63) - 1, -(1 << 63)], 0)]
TRAIN_RATE = q63(0.1 / 2)
TRAIN_DUMMY = ([0, 0], 0, [[[0, 0], [0, 0]]], [[0, 0]], TRAIN_RATE)
TRAIN_INPUTS = [([q63(0.25), q63(-0.5)], q63(0.1), [[[q63(1.5), q63(-2.0)], [q63(-0.75), q63(0.5)]]], [[q63(1.0), 0]], TRAIN_RATE),
                ([0, 0], 0, [[[q63(2.0), q63(1.0)], [q63(-1.0), q63(-3.0)]]], [[0, q63(1.0)]], TRAIN_RATE),
                ([q63(-1.0), 3], -q63(0.5), [[[-(1 << 63), (1 << 63) - 1], [1, -1]]], [[q63(1.0), q63(1.0)]], TRAIN_RATE)]


def ref_inference(x, w, b) -> list:
    return list(x) + [Model(63).logistic_inference(x, w, b)]


def ref_train(w, b, x, y, rate) -> list:
    new_w, new_b = Model(63).logistic_train(w, b, x, y, rate)
    return new_w + [new_b]


# ln a, sin b and a^c of three inputs at P = 32
MIXED_DUMMY = [q32(1.0), 0, 0]
MIXED_INPUTS = [[q32(0.3), q32(-4.0), q32(2.0)], [q32(100.0), q32(7.0), q32(-0.5)], [q32(2.0), q32(3.0), q32(3.0)]]


def ref_mixed(a, b, c) -> list:
    m = Model(32)
    return [m.qlog(a), m.qsin(b), m.qpow(a, c)]


field_inputs = FC.field_inputs
to_field = FC.to_field
