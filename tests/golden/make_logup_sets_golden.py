#!/usr/bin/env python3
"""Generates tests/golden/logup_sets_proofs.json: proofs the DEVICE prover makes of the range3 and beside circuits of
tests/logup_sets_cases.py under a logUp key whose lookups over one table are merged (ConstraintSystem.merge_lookups, h2mi_logup_inputs;
oracle/ proves no such argument) at fixed seeds, each written only after the Python-integer verifier of tests/logup_sets_cases.py has
accepted it.  tests/test_gpu_logup_sets.py reproduces them byte for byte.

SELF-DERIVED vectors (the reference holds no proof bytes); needs the built library and a GPU.
Usage: python tests/golden/make_logup_sets_golden.py [output path]
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
from oracle import flex as FX  # noqa: E402

SRS_SECRET = 0x5EC2E7 + 0x48324D49
CASES = [("range3", 81), ("beside", 82)]  # (circuit, seed)


def main():
    import torch  # noqa: F401  (one HIP runtime)

    h2 = _load_pkg.load()
    h2.init(0)
    from halo2_scaffold_amd import custom

    import logup_sets_cases as cases

    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "logup_sets_proofs.json")
    out = {"srs_secret": "0x%x" % SRS_SECRET, "cases": []}
    for name, seed in CASES:
        cs, asg, k = cases.build(custom, name)
        params = h2.ParamsKZG.setup(k, SRS_SECRET)
        keys = custom.Keys(params, cs, asg, logup=True)
        ocs = gate_cases.oracle_cs(cs, name)
        oasg = gate_cases.oracle_assignment(ocs, asg)
        vk = FX.VerifierKeys(ocs, k, SRS_SECRET, oasg.fixed, oasg.copies)
        proof = custom.create_proof(params, keys, asg, seed)
        assert cases.verify_circuits(vk, cs, proof, [list(asg.instance)], logup=True), name
        out["cases"].append({"circuit": name, "k": k, "seed": seed, "n_inputs": [len(a) for a in cs.lookup_arguments], "proof": proof.hex()})
        print(name, len(proof), flush=True)
        keys.release()
        params.release()
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
