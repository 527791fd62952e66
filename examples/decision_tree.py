#!/usr/bin/env python3
"""The `main` of the reference's examples/decision_tree.rs: `mock` and `prove` of an inference down its seven-node tree, then `mock` of a
training on its data set and on its dummy set and a proof of the data set against the key of the dummy set — 10 samples x 2 features, a
tree of depth 4, at DEGREE 16 / LOOKUP_BITS 15.  Both trees are printed as the reference prints them, read off the public outputs: the
dummy set's from `mock_device` against the key, the data set's from the proof.  With --witness-program the key is made with
witness_program=True: the closure runs once, at key generation, and both witnesses — 1.2 million cells each — are the recorded program's,
evaluated on the GPU.

    python examples/decision_tree.py --witness-program"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

X = [[2.771244718, 1.784783929], [1.0, 1.0], [3.0, 2.0], [3.0, 2.0], [2.0, 2.0], [7.0, 3.0], [9.00220326, 3.339047188], [7.444542326, 0.476683375],
     [10.12493903, 3.234550982], [6.642287351, 3.319983761]]
Y = [1, 0, 0, 1, 0, 1, 1, 0, 1, 1]
X_DUMMY = [[2.771244718, 1.784783929], [1.728571309, 1.169761413], [3.678319846, 2.81281357], [3.961043357, 2.61995032], [2.999208922, 2.209014212],
           [7.497545867, 3.162953546], [9.00220326, 3.339047188], [7.444542326, 0.476683375], [10.12493903, 3.234550982], [6.642287351, 3.319983761]]
Y_DUMMY = [0, 0, 0, 0, 0, 1, 1, 1, 1, 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--witness-program", action="store_true", help="record the closures at key generation and evaluate every later witness on the GPU")
    a = ap.parse_args()
    os.environ.setdefault("DEGREE", "16")
    os.environ.setdefault("LOOKUP_BITS", "15")
    import torch  # noqa: F401  (first, so the library shares torch's HIP runtime)

    import _load_pkg

    h2 = _load_pkg.load()
    h2.init(0)
    from halo2_scaffold_amd import decision_tree as DT
    from halo2_scaffold_amd import scaffold
    from halo2_scaffold_amd.fixed_point import FixedPointChip

    chip = FixedPointChip(DT.PRECISION_BITS, int(os.environ["LOOKUP_BITS"]))
    q = chip.quantization

    def show(public):
        print("decision tree:")
        rows = DT.nodes(chip, public)
        for node in rows:
            print(node)
        print("#nodes:", len(rows))

    x, x_dummy = [q(-1.2), q(0.1)], [q(2.1), q(3.2)]
    scaffold.mock(DT.inference, x)
    _, public = scaffold.prove(DT.inference, x, x_dummy, witness_program=a.witness_program)
    print("y:", public[0])

    dataset, dataset_dummy = DT.quantize_dataset(chip, X, Y), DT.quantize_dataset(chip, X_DUMMY, Y_DUMMY)
    scaffold.mock(DT.train, dataset)
    scaffold.mock(DT.train, dataset_dummy)
    t0 = time.perf_counter()
    pk, break_points = scaffold.gen_key(DT.train, dataset_dummy, witness_program=a.witness_program)
    print(f"gen_key: {time.perf_counter() - t0:.2f} s, {pk.cs.num_advice} gate + {pk.cs.num_lookup_advice} lookup-advice columns")
    try:
        show(scaffold.mock_device(DT.train, dataset_dummy, pk))
        t0 = time.perf_counter()
        public = scaffold.prove_private(DT.train, dataset, pk, break_points)
        print(f"prove_private: {time.perf_counter() - t0:.2f} s, a proof of {len(pk.last_proof)} bytes")
        show(public)
    finally:
        pk.release()


if __name__ == "__main__":
    main()
