#!/usr/bin/env python3
"""Generates tests/golden/batch_proofs.json: proofs the DEVICE prover makes of the two circuits of tests/phase_cases.py (advice phases
and challenges: oracle/ proves neither), one circuit and two circuits per proof, each checked with the Python-integer verifiers of
tests/phase_cases.py / tests/batch_cases.py before it is written.  tests/test_batch_host.py verifies them again without a GPU.

SELF-DERIVED vectors (the reference holds no proof bytes); needs the built library and a GPU.
Usage: python tests/golden/make_batch_golden.py [output path]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)
import _load_pkg  # noqa: E402
import batch_cases  # noqa: E402
import custom_gate_cases as gate_cases  # noqa: E402
import phase_cases  # noqa: E402
from oracle import flex as FX  # noqa: E402

SRS_SECRET = 0x5EC2E7 + 0x48324D49
CASES = [("rlc", 1), ("three", 1), ("rlc", 2), ("three", 2)]


def main():
    import torch  # noqa: F401  (one HIP runtime)

    h2 = _load_pkg.load()
    h2.init(0)
    from halo2_scaffold_amd import custom

    out = {"srs_secret": "0x%x" % SRS_SECRET, "cases": []}
    for name, n in CASES:
        build, k = phase_cases.CIRCUITS[name]
        cs, synthesize = build(custom)
        first = synthesize([None] * len(cs.challenge_phase))
        params = h2.ParamsKZG.setup(k, SRS_SECRET)
        keys = custom.Keys(params, cs, first)
        ocs = gate_cases.oracle_cs(cs, name)
        oasg = gate_cases.oracle_assignment(ocs, first)
        vk = FX.VerifierKeys(ocs, k, SRS_SECRET, oasg.fixed, oasg.copies)
        seeds = [31 + 8 * i for i in range(n)]
        if n == 1:
            proof = custom.create_proof(params, keys, synthesize, seeds[0])
            assert phase_cases.verify_circuit(vk, cs, proof, oasg.instance)
            assert custom.prove_many(keys, [synthesize], seeds=seeds) == proof
        else:
            proof = custom.prove_many(keys, [synthesize] * n, seeds=seeds)
        assert batch_cases.verify_circuits(vk, cs, proof, [list(first.instance)] * n)
        out["cases"].append({"circuit": name, "k": k, "circuits": n, "seeds": seeds, "proof": proof.hex()})
        print(name, n, len(proof), flush=True)
        keys.release()
        params.release()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "batch_proofs.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
