#!/usr/bin/env python3
"""The training loop of the reference's examples/linear_regression.rs: one proving key from dummy inputs, then `prove_private` for every
mini-batch of every epoch, the new parameters read off each proof's public outputs.  The key is made with witness_program=True, so the
closure runs once, at key generation; every later witness is the recorded program's, evaluated on the GPU.  The reference trains on
linfa's diabetes data set; this script draws a seeded synthetic one of the same shape (features in +-0.15, a linear target with noise).

    DEGREE=16 LOOKUP_BITS=15 python examples/linear_regression.py --epochs 2 --samples 96"""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def train_native(x, y, lr, epochs, batch_size):
    """the same loop in floats"""
    w, b = [0.0] * len(x[0]), 0.0
    for _ in range(epochs):
        for at in range(0, len(x), batch_size):
            bx, by = x[at:at + batch_size], y[at:at + batch_size]
            diff = [sum(xi[j] * w[j] for j in range(len(w))) + b - ti for xi, ti in zip(bx, by)]
            rate = lr / len(bx)
            b -= rate * sum(diff)
            w = [w[j] - rate * sum(d * xi[j] for d, xi in zip(diff, bx)) for j in range(len(w))]
    return w, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--samples", type=int, default=448)  # 14 batches of 32, as the 442 samples of the diabetes set give
    ap.add_argument("--features", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--learning-rate", type=float, default=0.01)
    ap.add_argument("--host", action="store_true", help="host synthesis for every proof instead of the witness program")
    a = ap.parse_args()
    assert a.samples % a.batch_size == 0, "one key proves batches of one size"
    os.environ.setdefault("DEGREE", "16")
    os.environ.setdefault("LOOKUP_BITS", "15")
    import torch  # noqa: F401  (first, so the library shares torch's HIP runtime)

    import _load_pkg

    h2 = _load_pkg.load()
    h2.init(0)
    from halo2_scaffold_amd import scaffold
    from halo2_scaffold_amd import linear_regression as LR
    from halo2_scaffold_amd.fixed_point import FixedPointChip

    chip = FixedPointChip(32, int(os.environ["LOOKUP_BITS"]))
    rng = random.Random("linear regression")
    truth = [rng.uniform(-500.0, 500.0) for _ in range(a.features)]
    x = [[rng.uniform(-0.15, 0.15) for _ in range(a.features)] for _ in range(a.samples)]
    y = [sum(t * v for t, v in zip(truth, xi)) + 150.0 + rng.gauss(0.0, 10.0) for xi in x]
    zeros = [[0.0] * a.features] * a.batch_size
    dummy = LR.quantize_batch(chip, [0.0] * a.features, 0.0, zeros, [0.0] * a.batch_size, a.learning_rate)
    t0 = time.perf_counter()
    pk, break_points = scaffold.gen_key(LR.train, dummy, witness_program=not a.host)
    print(f"gen_key: {time.perf_counter() - t0:.2f} s, {pk.cs.num_advice} gate + {pk.cs.num_lookup_advice} lookup-advice columns")
    w, b = [0] * a.features, 0  # field elements from here on: each proof's public outputs are the next proof's inputs
    t0 = time.perf_counter()
    for epoch in range(a.epochs):
        for at in range(0, a.samples, a.batch_size):
            _, _, qx, qy, rate = LR.quantize_batch(chip, [], 0.0, x[at:at + a.batch_size], y[at:at + a.batch_size], a.learning_rate)
            out = scaffold.prove_private(LR.train, (w, b, qx, qy, rate), pk, break_points)
            w, b = out[:a.features], out[a.features]
        print(f"epoch {epoch + 1}: b = {chip.dequantization(b):.6f}")
    proofs = a.epochs * (a.samples // a.batch_size)
    print(f"{proofs} proofs in {time.perf_counter() - t0:.2f} s")
    native_w, native_b = train_native(x, y, a.learning_rate, a.epochs, a.batch_size)
    print("w:", [round(chip.dequantization(v), 6) for v in w], "b:", round(chip.dequantization(b), 6))
    print("native w:", [round(v, 6) for v in native_w], "b:", round(native_b, 6))
    pk.release()


if __name__ == "__main__":
    main()
