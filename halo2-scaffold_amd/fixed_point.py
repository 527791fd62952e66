"""FixedPointChip: signed fixed-point arithmetic over the builders of flex.py, after the reference's src/gadget/fixed_point.rs, name for
name.  A real x is the integer round(x * 2^P) (P = precision_bits), a negative one its negation modulo r; every method takes the context
first and operands that are cells (plain integers: cell indices) or flex.Constant values, and returns a cell.  The values halo2-base
computes outside the gates — quotients, remainders, is-zero flags — are hint items (flex.hint), so every method runs unchanged under
flex.Context (host synthesis) and under witness.RecordingContext (a witness program: the hints are evaluated on the device).

Written from the algorithm; what is restated is the sequence of builder calls, which fixes the circuit.  Left out: qexp2,
qlog2, qsin and everything built on them.  Quantisation is the host's: a closure's inputs stay integers, callers quantise before
`prove`."""
import math

from . import flex
from .flex import Constant

R = flex.R


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
