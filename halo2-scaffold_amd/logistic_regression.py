"""LogisticRegressionChip over FixedPointChip, after the reference's src/gadget/logistic_regression.rs: inference 1 / (1 + exp(-(w . x + b)))
and mini-batch gradient descent on it, and the two closures of its examples/logistic_regression.rs as the scaffold takes them.  Every
input of a closure is an integer — the callers quantise (FixedPointChip.quantization, quantize_batches) before `prove` — so both record
as witness programs; a qexp is about 10 000 cells, which is what makes these the circuits a recorded witness pays for.  The reference's
binary cross-entropy is a log line computed in floats from the witness; it is no part of the circuit and is not reproduced."""
from .fixed_point import FixedPointChip
from .flex import Constant


class LogisticRegressionChip:
    def __init__(self, lookup_bits: int = None, precision_bits: int = 63):
        self.chip = FixedPointChip(precision_bits, lookup_bits)
        self.lookup_bits = lookup_bits

    def _sigmoid(self, ctx, logit, one):
        chip = self.chip
        exp_logit = chip.qexp(ctx, chip.neg(ctx, logit))
        return chip.qdiv(ctx, one, chip.qadd(ctx, exp_logit, one))

    def inference(self, ctx, w, x, b):
        chip = self.chip
        logit = chip.qadd(ctx, chip.inner_product(ctx, w, x), b)
        return self._sigmoid(ctx, logit, Constant(chip.quantization_scale))

    def train_multi_batch(self, ctx, w, b, x, y_truth, learning_rate: int):
        """train_one_batch for every batch of x (batches of rows of cells), y_truth (batches of cells) in turn -> (w, b)"""
        w = list(w)
        for cur_x, cur_y in zip(x, y_truth):
            w, b = self.train_one_batch(ctx, w, b, cur_x, cur_y, learning_rate)
        return w, b

    def train_one_batch(self, ctx, w, b, x, y_truth, learning_rate: int):
        """one gradient step on the batch x (rows of cells), y_truth (cells) from the cells w, b -> (w, b).  learning_rate: the quantised
        rate divided by the batch size, an integer; it and the quantised one are constants of the circuit here (load_constant), so they
        belong to the key"""
        chip = self.chip
        w, x, y_truth = list(w), [list(xi) for xi in x], list(y_truth)
        assert all(len(xi) == len(w) for xi in x) and len(x) == len(y_truth)
        rate = ctx.load_constant(learning_rate)
        one = ctx.load_constant(chip.quantization_scale)
        y = [self._sigmoid(ctx, chip.qadd(ctx, chip.inner_product(ctx, w, xi), b), one) for xi in x]
        diff_y = [chip.qsub(ctx, yi, ti) for yi, ti in zip(y, y_truth)]
        for j in range(len(w)):
            partial_wj = [chip.qmul(ctx, diff_y[i], x[i][j]) for i in range(len(x))]
            diff_wj = chip.qmul(ctx, rate, chip.qsum(ctx, partial_wj))
            w[j] = chip.qsub(ctx, w[j], diff_wj)
        diff_b = chip.qmul(ctx, rate, chip.qsum(ctx, diff_y))
        return w, chip.qsub(ctx, b, diff_b)


def inference(ctx, inputs, make_public):
    """inputs (x, w, b), quantised: x and the probability are public"""
    x, w, b = inputs
    chip = LogisticRegressionChip(ctx.lookup_bits)
    xs = [ctx.load_witness(v) for v in x]
    make_public += xs
    ws = [ctx.load_witness(v) for v in w]
    make_public.append(chip.inference(ctx, ws, xs, ctx.load_witness(b)))


def train(ctx, inputs, make_public):
    """inputs (w, b, x, y, rate), quantised: x the batches of one proof, y their targets, rate = quantization(learning rate / batch
    size).  The new w and b are public.  The rate is a constant of the circuit: the one the key was made with is the one every proof
    takes, whatever a later call passes"""
    w, b, x, y, rate = inputs
    chip = LogisticRegressionChip(ctx.lookup_bits)
    ws = [ctx.load_witness(v) for v in w]
    bc = ctx.load_witness(b)
    xs = [[[ctx.load_witness(v) for v in xi] for xi in batch] for batch in x]
    ys = [[ctx.load_witness(v) for v in batch] for batch in y]
    ws, bc = chip.train_multi_batch(ctx, ws, bc, xs, ys, int(rate))
    make_public += ws + [bc]


def quantize_batches(chip: FixedPointChip, w, b, x, y, learning_rate: float):
    """real w, b, batches (x[batch][sample][feature], y[batch][sample]) and rate -> the inputs of `train`"""
    q = chip.quantization
    return ([q(v) for v in w], q(b), [[[q(v) for v in xi] for xi in batch] for batch in x], [[q(v) for v in batch] for batch in y],
            q(learning_rate / len(x[0])))
