"""FixedPointChip: signed fixed-point arithmetic over the builders of flex.py, after the reference's src/gadget/fixed_point.rs, name for
name.  A real x is the integer round(x * 2^P) (P = precision_bits), a negative one its negation modulo r; every method takes the context
first and operands that are cells (plain integers: cell indices) or flex.Constant values, and returns a cell.  The values halo2-base
computes outside the gates — quotients, remainders, is-zero flags — are hint items (flex.hint), so every method runs unchanged under
flex.Context (host synthesis) and under witness.RecordingContext (a witness program: the hints are evaluated on the device).

Written from the algorithm; what is restated is the sequence of builder calls, which fixes the circuit.  The three values qlog2 takes
from outside the gates — the index of the operand's highest set bit, that power of two and the power of two of the shift — are the MSB
and POW2 hints.  An operand a function cannot take — qlog2 of zero or a negative number, a qexp2 whose result leaves the number format —
is refused: a ValueError or a failed range-check assertion at synthesis, a failed check of the witness program.  Quantisation is the
host's: a closure's inputs stay integers, callers quantise before `prove`."""
import math

from . import flex
from .flex import Constant

R = flex.R

# the reference's coefficient lists, leading coefficient first (src/gadget/fixed_point.rs:104-151)
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


class FixedPointChip:
    def __init__(self, precision_bits: int = 32, lookup_bits: int = None):
        assert 32 <= precision_bits <= 63, "support only 32 <= precision bits <= 63"
        self.precision_bits, self.lookup_bits = precision_bits, lookup_bits
        self.quantization_scale = 1 << precision_bits
        self.max_value = 1 << (2 * precision_bits)  # |x| < max_value is what `clip` reduces to
        # x > negative_point reads as negative: -2^(2P+1) modulo r
        self.negative_point = R - (1 << (2 * precision_bits + 1))

    # ---- the host's side --------------------------------------------------------------------------------------------------------------
    def quantization(self, x: float) -> int:
        """round(|x| * 2^P), halves away from zero, negated modulo r for a negative x"""
        q = math.floor(abs(x) * float(self.quantization_scale) + 0.5)
        return (R - q) % R if x < 0 else q

    def dequantization(self, v: int) -> float:
        """the real a field element stands for.  (The reference takes bn254_max - x - 1 as the magnitude of a negative x, one more than
        r - x; this is r - x, so that dequantization(quantization(x)) is x to half an ulp on both sides of zero.)"""
        v %= R
        sign, mag = (-1.0, R - v) if v > self.negative_point else (1.0, v)
        return sign * (float(mag // self.quantization_scale) + float(mag % self.quantization_scale) / float(self.quantization_scale))

    def signed(self, v: int) -> int:
        """the signed integer a field element stands for, by the threshold of signed_div_scale (above 2^252: negative)"""
        v %= R
        return v - R if v > 1 << 252 else v

    def _range(self, ctx):
        assert self.lookup_bits is None or ctx.lookup_bits == self.lookup_bits, "the chip's LOOKUP_BITS are not the context's"
        return ctx

    # ---- without a range check --------------------------------------------------------------------------------------------------------
    def qadd(self, ctx, a, b):
        return ctx.add(a, b)

    def qsub(self, ctx, a, b):
        return ctx.sub(a, b)

    def neg(self, ctx, a):
        return ctx.neg(a)

    def qsum(self, ctx, a):
        return ctx.sum(a)

    def cond_neg(self, ctx, a, is_neg):
        return ctx.select(ctx.neg(a), a, is_neg)

    def bit_xor(self, ctx, a, b):
        a = ctx.add(Constant(0), a)
        b = ctx.add(Constant(0), b)
        ctx.assert_bit(a)
        ctx.assert_bit(b)
        ab = ctx.add(a, b)
        one = ctx.add(Constant(1), Constant(0))
        return ctx.is_equal(ab, one)

    # ---- signs ------------------------------------------------------------------------------------------------------------------------
    def is_neg(self, ctx, a):
        """1 when a, a cell, is 2^(2P+1) or above as an integer below r: its quotient by 2^(2P+1) is not zero"""
        a_shift, _ = self._range(ctx).div_mod(a, 1 << (2 * self.precision_bits + 1), 254)
        return ctx.not_(ctx.is_zero(a_shift))

    def qabs(self, ctx, a):
        a_reverse = ctx.neg(a)
        return ctx.select(a_reverse, a, self.is_neg(ctx, a))

    def sign(self, ctx, a):
        """-1 or 1, as field elements"""
        neg_one = ctx.neg(Constant(1))
        return ctx.select(neg_one, Constant(1), self.is_neg(ctx, a))

    def clip(self, ctx, a):
        """a with its magnitude reduced modulo 2^(2P)"""
        sign = self.is_neg(ctx, a)
        a_abs = self.qabs(ctx, a)
        _, unsigned_clipped = ctx.div_mod(a_abs, self.max_value, 254)
        return self.cond_neg(ctx, unsigned_clipped, sign)

    def qmax(self, ctx, a, b):
        return ctx.select(b, a, self.is_neg(ctx, self.qsub(ctx, a, b)))

    def qmin(self, ctx, a, b):
        return ctx.select(a, b, self.is_neg(ctx, self.qsub(ctx, a, b)))

    # ---- products and quotients ----------------------------------------------------------------------------------------------------------
    def signed_div_scale(self, ctx, a):
        """(div, rem) with a = 2^P * div + rem, 0 <= rem < 2^P, |div| < 2^(3P), for a signed cell a: | rem | 2^P | div | a |, the
        quotient rounded toward minus infinity"""
        ctx = self._range(ctx)
        b = self.quantization_scale
        flags = flex.HINT_CONST | flex.HINT_SIGNED
        last = ctx.assign_region_last([("hint", (flex.DIVR, a, b, flags)), ("constant", b), ("hint", (flex.DIVQ, a, b, flags)), ("existing", a)], [0])
        rem, div = last - 3, last - 1
        ctx.check_big_less_than_safe(rem, b)
        div_abs = self.qabs(ctx, div)
        ctx.check_big_less_than_safe(div_abs, 1 << (3 * self.precision_bits))
        return div, rem

    def qmul(self, ctx, a, b):
        return self.signed_div_scale(ctx, ctx.mul(a, b))[0]

    def qdiv(self, ctx, a, b):
        """sign(a) sign(b) floor(|a| 2^P / |b|); b = 0 satisfies nothing"""
        P = self.precision_bits
        a_sign, b_sign = self.is_neg(ctx, a), self.is_neg(ctx, b)
        a_abs, b_abs = self.qabs(ctx, a), self.qabs(ctx, b)
        a_rescale = ctx.mul(a_abs, Constant(self.quantization_scale))
        res_abs, _ = ctx.div_mod_var(a_rescale, b_abs, 4 * P, 2 * P)
        return self.cond_neg(ctx, res_abs, self.bit_xor(ctx, a_sign, b_sign))

    def qmod(self, ctx, a, b):
        """|a| mod b for a >= 0, b - |a| mod b for a < 0; b must be positive"""
        P = self.precision_bits
        a_sign, b_sign = self.is_neg(ctx, a), self.is_neg(ctx, b)
        ctx.assert_is_const(b_sign, 0)
        a_abs = self.qabs(ctx, a)
        _, res_abs = ctx.div_mod_var(a_abs, b, 4 * P, 2 * P)
        res_abs_comp = ctx.sub(b, res_abs)
        return ctx.select(res_abs_comp, res_abs, a_sign)

    def polynomial(self, ctx, x, coef):
        """Horner's rule from the leading coefficient: (..(c0 x + c1) x + ..) x + c_last, a qmul a step"""
        coef = list(coef)
        last = Constant(0)
        result = self.qadd(ctx, x, Constant(0))
        for idx, c in enumerate(coef):
            y_add = self.qadd(ctx, last, c)
            if idx < len(coef) - 1:
                last = self.qmul(ctx, x, y_add)
            else:
                result = y_add
        return result

    def inner_product(self, ctx, a, b):
        a, b = list(a), list(b)
        assert len(a) == len(b)
        res = self.qadd(ctx, Constant(0), Constant(0))
        for ai, bi in zip(a, b):
            res = self.qadd(ctx, res, self.qmul(ctx, ai, bi))
        return res

    # ---- exp2, log2, sin and what is built on them ----------------------------------------------------------------------------------------
    def generate_exp2_poly(self) -> list:
        """2^x on [0, 1): Remez, degree 12"""
        return [Constant(self.quantization(c)) for c in EXP2_COEF]

    def generate_log_poly(self) -> list:
        """log2(x) on [2, 4]: Remez, degree 14"""
        return [Constant(self.quantization(c)) for c in LOG_COEF]

    def generate_sin_poly(self) -> list:
        """sin(x) on [0, pi]: Remez, degree 14"""
        return [Constant(self.quantization(c)) for c in SIN_COEF]

    @staticmethod
    def _assert_const(ctx, cell, c: int, what: str):
        """assert_is_const, refusing a witness that cannot satisfy it where it is synthesised"""
        if ctx.cells[cell] != c % R:
            raise ValueError(f"witness out of range: {what}")
        ctx.assert_is_const(cell, c)

    @staticmethod
    def _add_hint(ctx, hint):
        """gate().add(Witness(hint), Constant(0)): | hint | 0 | 1 | hint | -> the last cell"""
        return ctx.assign_region_last([("hint", hint), ("constant", 0), ("constant", 1), ("witness", ctx.hint_value(*hint))], [0])

    def check_power_of_two(self, ctx, pow2_exponent, exponent):
        """pow2_exponent = 2^exponent, below 2^(2P): its 2P bits hold a single one, and the bit at `exponent` is a one"""
        bits = ctx.num_to_bits(pow2_exponent, 2 * self.precision_bits)
        sum_of_bits_m1 = ctx.sub(ctx.sum(bits), Constant(1))
        self._assert_const(ctx, ctx.is_zero(sum_of_bits_m1), 1, "not a power of two below 2^(2P)")
        bit_m1 = ctx.sub(ctx.select_from_idx(bits, exponent), Constant(1))
        self._assert_const(ctx, ctx.is_zero(bit_m1), 1, "a power of two that is not the exponent's")

    def qexp2(self, ctx, a):
        """2^|a| as 2^int * poly(frac), and its reciprocal for a negative a.  The reciprocal is computed for either sign, so 2^|a| must be
        one qdiv divides by: below 2^(P+1) as a real"""
        P = self.precision_bits
        a_abs = self.qabs(ctx, a)
        int_part, frac_part = self._range(ctx).div_mod(a_abs, self.quantization_scale, 2 * P)
        int_part_pow2 = ctx.select_from_idx(ctx.pow_of_two(), int_part)
        y_frac = self.polynomial(ctx, frac_part, self.generate_exp2_poly())
        res_pos = ctx.mul(int_part_pow2, y_frac)
        res_neg = self.qdiv(ctx, Constant(self.quantization_scale), res_pos)
        return ctx.select(res_neg, res_pos, self.is_neg(ctx, a))

    def qlog2(self, ctx, a):
        """log2 of a cell a, 0 < a < 2^(2P-1): a = 2^exp1 * m with 1 <= m < 2 by the MSB and POW2 hints, checked; a shifted to
        [2, 4) as a real; the polynomial there, minus the shift"""
        P = self.precision_bits
        ctx = self._range(ctx)
        a_assigned = ctx.add(a, Constant(0))
        is_invalid = ctx.or_(self.is_neg(ctx, a), ctx.is_zero(a_assigned))
        self._assert_const(ctx, is_invalid, 0, "qlog2 of zero or of a negative number")
        num_bits = 2 * P
        pow1 = self._add_hint(ctx, (flex.POW2, a_assigned, 0, flex.HINT_OF_MSB))
        exp1 = self._add_hint(ctx, (flex.MSB, a_assigned, 0, 0))
        self.check_power_of_two(ctx, pow1, exp1)
        pow2 = ctx.mul(pow1, Constant(2))
        exp2 = ctx.add(exp1, Constant(1))
        self.check_power_of_two(ctx, pow2, exp2)
        a_lt_pow2 = ctx.is_less_than(a, pow2, num_bits)
        a_gt_pow1 = ctx.is_less_than(pow1, a, num_bits)
        a_ge_pow1 = ctx.or_(ctx.is_equal(a, pow1), a_gt_pow1)
        self._assert_const(ctx, ctx.and_(a_lt_pow2, a_ge_pow1), 1, "qlog2: the operand is not between the two powers of two")
        shift = ctx.sub(Constant(P + 2), exp2)
        is_shift_neg = self.is_neg(ctx, shift)
        shift_abs = self.qabs(ctx, shift)
        shift_pow2 = self._add_hint(ctx, (flex.POW2, shift_abs, 0, 0))
        self.check_power_of_two(ctx, shift_pow2, shift_abs)
        a_ls = ctx.mul(a, shift_pow2)
        a_rs, _ = ctx.div_mod_var(a, shift_pow2, num_bits, P + 1)
        a_norm = ctx.select(a_rs, a_ls, is_shift_neg)
        log_a_norm = self.polynomial(ctx, a_norm, self.generate_log_poly())
        log_shift_q = ctx.mul(ctx.neg(shift), Constant(self.quantization_scale))
        return ctx.add(log_a_norm, log_shift_q)

    def qsin(self, ctx, a):
        """sin |a| by the polynomial on [0, pi] — of |a| mod 2 pi, or minus that of (|a| mod 2 pi) - pi —, negated for a negative a"""
        a_abs = self.qabs(ctx, a)
        a_sign = self.is_neg(ctx, a)
        a_mod = self.qmod(ctx, a_abs, Constant(self.quantization(math.pi * 2.0)))
        a_mpi = self.qsub(ctx, a_mod, Constant(self.quantization(math.pi)))
        is_neg_a_mpi = self.is_neg(ctx, a_mpi)
        sin_a_mod = self.polynomial(ctx, a_mod, self.generate_sin_poly())
        sin_a_mpi = self.neg(ctx, self.polynomial(ctx, a_mpi, self.generate_sin_poly()))
        return self.cond_neg(ctx, ctx.select(sin_a_mod, sin_a_mpi, is_neg_a_mpi), a_sign)

    def qcos(self, ctx, a):
        half_pi = ctx.load_constant(self.quantization(math.pi / 2.0))
        return self.qsin(ctx, self.qadd(ctx, a, half_pi))

    def qtan(self, ctx, a):
        sin_a = self.qsin(ctx, a)
        return self.qdiv(ctx, sin_a, self.qcos(ctx, a))

    def qexp(self, ctx, a):
        """e^a = 2^(a / ln 2)"""
        ln2 = ctx.load_constant(self.quantization(math.log(2.0)))
        return self.qexp2(ctx, self.qdiv(ctx, a, ln2))

    def _exp_pair(self, ctx, a):
        ea = self.qexp(ctx, a)
        return ea, self.qexp(ctx, self.neg(ctx, a))

    def qsinh(self, ctx, a):
        ea, ena = self._exp_pair(ctx, a)
        nume = self.qsub(ctx, ea, ena)
        return self.qdiv(ctx, nume, ctx.load_constant(self.quantization(2.0)))

    def qcosh(self, ctx, a):
        ea, ena = self._exp_pair(ctx, a)
        nume = self.qadd(ctx, ea, ena)
        return self.qdiv(ctx, nume, ctx.load_constant(self.quantization(2.0)))

    def qtanh(self, ctx, a):
        sinh = self.qsinh(ctx, a)
        return self.qdiv(ctx, sinh, self.qcosh(ctx, a))

    def qlog(self, ctx, a):
        """ln a = log2 a / log2 e"""
        log2e = ctx.load_constant(self.quantization(math.log2(math.e)))
        return self.qdiv(ctx, self.qlog2(ctx, a), log2e)

    def qpow(self, ctx, x, exponent):
        """x^a = exp(a ln x)"""
        return self.qexp(ctx, self.qmul(ctx, exponent, self.qlog(ctx, x)))

    def qsqrt(self, ctx, x):
        return self.qpow(ctx, x, ctx.load_constant(self.quantization(0.5)))
