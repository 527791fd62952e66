#!/usr/bin/env python3
"""Generates tests/golden/shuffle_proofs.json: proofs the DEVICE prover makes of the perm, mixed and phased circuits of
tests/shuffle_cases.py (shuffle arguments: oracle/ proves none) at fixed seeds, each written only after the Python-integer verifier of
tests/shuffle_cases.py has accepted it.  tests/test_gpu_shuffle.py reproduces them byte for byte.

SELF-DERIVED vectors (the reference holds no proof bytes); needs the built library and a GPU.
Usage: python tests/golden/make_shuffle_golden.py [output path]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)
import _load_pkg  # noqa: E402
import custom_gate_cases as gate_cases  # noqa: E402
import shuffle_cases  # noqa: E402
from oracle import flex as FX  # noqa: E402

SRS_SECRET = 0x5EC2E7 + 0x48324D49
CASES = [("perm", 61), ("mixed", 62), ("phased", 63)]  # (circuit, seed)


def main():
    import torch  # noqa: F401  (one HIP runtime)

    h2 = _load_pkg.load()
    h2.init(0)
    from halo2_scaffold_amd import custom

    out = {"srs_secret": "0x%x" % SRS_SECRET, "cases": []}
    for name, seed in CASES:
        cs, asg, k = shuffle_cases.build(custom, name)
        first = shuffle_cases.first_assignment(cs, asg)
        params = h2.ParamsKZG.setup(k, SRS_SECRET)
        keys = custom.Keys(params, cs, first)
        ocs = gate_cases.oracle_cs(cs, name)
        oasg = gate_cases.oracle_assignment(ocs, first)
        vk = FX.VerifierKeys(ocs, k, SRS_SECRET, oasg.fixed, oasg.copies)
        proof = custom.create_proof(params, keys, asg, seed)
        assert shuffle_cases.verify_circuits(vk, cs, proof, [list(first.instance)]), name
        out["cases"].append({"circuit": name, "k": k, "seed": seed, "proof": proof.hex()})
        print(name, len(proof), flush=True)
        keys.release()
        params.release()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "shuffle_proofs.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
