#!/usr/bin/env python3
"""The training loop of the reference's examples/logistic_regression.rs: one proving key from dummy inputs, then `prove_private` for every
group of --multi-batch mini-batches of every epoch, the new parameters read off each proof's public outputs.  The key is made with
witness_program=True, so the closure runs once, at key generation; every later witness — a qexp of about 10 000 cells per sample among
it — is the recorded program's, evaluated on the GPU.  The reference trains on linfa's winequality data set (11 features, the target
quality > 6); this script draws a seeded synthetic one of the same shape.  The reference proves 12 batches of 64 samples per proof at
DEGREE 19; the defaults here are smaller.

    DEGREE=17 LOOKUP_BITS=16 python examples/logistic_regression.py --epochs 2 --samples 64 --batch-size 16 --multi-batch 2"""
import argparse
import math
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
            pred = [1.0 / (1.0 + math.exp(-(sum(xi[j] * w[j] for j in range(len(w))) + b))) for xi in bx]
            diff = [p - t for p, t in zip(pred, by)]
            rate = lr / len(bx)
            b -= rate * sum(diff)
            w = [w[j] - rate * sum(d * xi[j] for d, xi in zip(diff, bx)) for j in range(len(w))]
    return w, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--features", type=int, default=11)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--multi-batch", type=int, default=2, help="batches per proof")
    ap.add_argument("--learning-rate", type=float, default=0.001)
    ap.add_argument("--host", action="store_true", help="host synthesis for every proof instead of the witness program")
    a = ap.parse_args()
    per_proof = a.batch_size * a.multi_batch
    assert a.samples % per_proof == 0, "one key proves groups of batches of one size"
    os.environ.setdefault("DEGREE", "17")
    os.environ.setdefault("LOOKUP_BITS", "16")
    import torch  # noqa: F401  (first, so the library shares torch's HIP runtime)

    import _load_pkg

    h2 = _load_pkg.load()
    h2.init(0)
    from halo2_scaffold_amd import scaffold
    from halo2_scaffold_amd import logistic_regression as LG
    from halo2_scaffold_amd.fixed_point import FixedPointChip

    chip = FixedPointChip(63, int(os.environ["LOOKUP_BITS"]))
    rng = random.Random("logistic regression")
    truth = [rng.uniform(-2.0, 2.0) for _ in range(a.features)]
    x = [[rng.uniform(-1.0, 1.0) for _ in range(a.features)] for _ in range(a.samples)]
    y = [float(sum(t * v for t, v in zip(truth, xi)) + rng.gauss(0.0, 0.5) > 1.0) for xi in x]
    group = lambda rows, at: [rows[at + i * a.batch_size:at + (i + 1) * a.batch_size] for i in range(a.multi_batch)]
    zeros = [[[0.0] * a.features] * a.batch_size] * a.multi_batch
    dummy = LG.quantize_batches(chip, [0.0] * a.features, 0.0, zeros, [[0.0] * a.batch_size] * a.multi_batch, a.learning_rate)
    t0 = time.perf_counter()
    pk, break_points = scaffold.gen_key(LG.train, dummy, witness_program=not a.host)
    print(f"gen_key: {time.perf_counter() - t0:.2f} s, {pk.cs.num_advice} gate + {pk.cs.num_lookup_advice} lookup-advice columns")
    w, b = [0] * a.features, 0  # field elements from here on: each proof's public outputs are the next proof's inputs
    t0 = time.perf_counter()
    for epoch in range(a.epochs):
        for at in range(0, a.samples, per_proof):
            _, _, qx, qy, rate = LG.quantize_batches(chip, [], 0.0, group(x, at), group(y, at), a.learning_rate)
            out = scaffold.prove_private(LG.train, (w, b, qx, qy, rate), pk, break_points)
            w, b = out[:a.features], out[a.features]
        print(f"epoch {epoch + 1}: b = {chip.dequantization(b):.6f}")
    proofs = a.epochs * (a.samples // per_proof)
    print(f"{proofs} proofs in {time.perf_counter() - t0:.2f} s")
    native_w, native_b = train_native(x, y, a.learning_rate, a.epochs, a.batch_size)
    print("w:", [round(chip.dequantization(v), 6) for v in w], "b:", round(chip.dequantization(b), 6))
    print("native w:", [round(v, 6) for v in native_w], "b:", round(native_b, 6))
    pk.release()


if __name__ == "__main__":
    main()
