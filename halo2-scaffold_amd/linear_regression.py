"""LinearRegressionChip over FixedPointChip, after the reference's src/gadget/linear_regression.rs: inference w . x + b and one step of
mini-batch gradient descent, and the two closures of its examples/linear_regression.rs as the scaffold takes them.  Every input of a
closure is an integer — the callers quantise (FixedPointChip.quantization) before `prove` — so both record as witness programs."""
from .fixed_point import FixedPointChip


class LinearRegressionChip:
    def __init__(self, lookup_bits: int = None, precision_bits: int = 32):
        self.chip = FixedPointChip(precision_bits, lookup_bits)
        self.lookup_bits = lookup_bits

    def inference(self, ctx, w, x, b):
        return self.chip.qadd(ctx, self.chip.inner_product(ctx, w, x), b)

    def train_one_batch(self, ctx, w, b, x, y_truth, learning_rate: int):
        """one gradient step on the batch x (rows of cells), y_truth (cells) from the cells w, b -> (w, b).  learning_rate: the
        quantised rate divided by the batch size, an integer — loaded as a witness as the reference loads it, so under a witness
        program it is one more private input."""
        chip = self.chip
        w, x, y_truth = list(w), [list(xi) for xi in x], list(y_truth)
        assert all(len(xi) == len(w) for xi in x) and len(x) == len(y_truth)
        rate = ctx.load_witness(learning_rate)
        y = [chip.qadd(ctx, chip.inner_product(ctx, xi, w), b) for xi in x]
        diff_y = [chip.qsub(ctx, yi, ti) for yi, ti in zip(y, y_truth)]
        for j in range(len(w)):
            partial_wj = [chip.qmul(ctx, diff_y[i], x[i][j]) for i in range(len(x))]
            diff_wj = chip.qmul(ctx, rate, chip.qsum(ctx, partial_wj))
            w[j] = chip.qsub(ctx, w[j], diff_wj)
        diff_b = chip.qmul(ctx, rate, chip.qsum(ctx, diff_y))
        return w, chip.qsub(ctx, b, diff_b)


def inference(ctx, inputs, make_public):
    """inputs (x, w, b), quantised: x and the prediction are public"""
    x, w, b = inputs
    chip = LinearRegressionChip(ctx.lookup_bits)
    xs = [ctx.load_witness(v) for v in x]
    make_public += xs
    ws = [ctx.load_witness(v) for v in w]
    make_public.append(chip.inference(ctx, ws, xs, ctx.load_witness(b)))


def train(ctx, inputs, make_public):
    """inputs (w, b, x, y, rate), quantised, rate = quantization(learning rate / batch size): the new w and b are public"""
    w, b, x, y, rate = inputs
    chip = LinearRegressionChip(ctx.lookup_bits)
    ws = [ctx.load_witness(v) for v in w]
    bc = ctx.load_witness(b)
    xs = [[ctx.load_witness(v) for v in xi] for xi in x]
    ys = [ctx.load_witness(v) for v in y]
    ws, bc = chip.train_one_batch(ctx, ws, bc, xs, ys, rate)
    make_public += ws + [bc]


def quantize_batch(chip: FixedPointChip, w, b, x, y, learning_rate: float):
    """real w, b, batch and rate -> the inputs of `train`"""
    q = chip.quantization
    return ([q(v) for v in w], q(b), [[q(v) for v in xi] for xi in x], [q(v) for v in y], q(learning_rate / len(x)))
