#!/usr/bin/env python3
"""Generates tests/golden/logup_proofs.json: proofs the DEVICE prover makes of the xor and mixed circuits of tests/logup_cases.py under a
logUp key (H2MI_KEYGEN_LOGUP: oracle/ proves no such argument) at fixed seeds, each written only after the Python-integer verifier of
tests/logup_cases.py has accepted it.  tests/test_gpu_logup.py reproduces them byte for byte.

`plain_xor` is the xor circuit's proof under a key WITHOUT the flag.  It pins that such a key behaves as it did before the flag existed, so
it has to come from a library built from the commit in front of the one that added the flag: `--plain-xor-only FILE` writes just that
entry with whatever library is loaded (it needs nothing of logUp), `--plain-xor FILE` takes it over from such a file; without either the
entry of the existing output file is kept.

SELF-DERIVED vectors (the reference holds no proof bytes); needs the built library and a GPU.
Usage: python tests/golden/make_logup_golden.py [output path] [--plain-xor FILE | --plain-xor-only FILE]
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
import lookup_expr_cases  # noqa: E402
from oracle import flex as FX  # noqa: E402

SRS_SECRET = 0x5EC2E7 + 0x48324D49
CASES = [("xor", 71), ("mixed", 72)]  # (circuit, seed)
PLAIN_XOR_SEED = 73


def plain_xor(h2, custom):
    cs, asg = lookup_expr_cases.xor_circuit(custom)
    params = h2.ParamsKZG.setup(5, SRS_SECRET)
    keys = custom.Keys(params, cs, asg)
    proof = custom.create_proof(params, keys, asg, PLAIN_XOR_SEED)
    keys.release()
    params.release()
    return {"circuit": "xor", "k": 5, "seed": PLAIN_XOR_SEED, "proof": proof.hex()}


def main():
    import torch  # noqa: F401  (one HIP runtime)

    h2 = _load_pkg.load()
    h2.init(0)
    from halo2_scaffold_amd import custom

    args = sys.argv[1:]
    if "--plain-xor-only" in args:
        with open(args[args.index("--plain-xor-only") + 1], "w") as f:
            json.dump(plain_xor(h2, custom), f)
        return
    import logup_cases

    path = args[0] if args and not args[0].startswith("--") else os.path.join(HERE, "logup_proofs.json")
    if "--plain-xor" in args:
        plain = json.load(open(args[args.index("--plain-xor") + 1]))
    else:
        plain = json.load(open(path))["plain_xor"]
    out = {"srs_secret": "0x%x" % SRS_SECRET, "cases": [], "plain_xor": plain}
    for name, seed in CASES:
        cs, asg, k = logup_cases.build(custom, name)
        params = h2.ParamsKZG.setup(k, SRS_SECRET)
        keys = custom.Keys(params, cs, asg, logup=True)
        ocs = gate_cases.oracle_cs(cs, name)
        oasg = gate_cases.oracle_assignment(ocs, asg)
        vk = FX.VerifierKeys(ocs, k, SRS_SECRET, oasg.fixed, oasg.copies)
        proof = custom.create_proof(params, keys, asg, seed)
        assert logup_cases.verify_circuits(vk, cs, proof, [list(asg.instance)], logup=True), name
        out["cases"].append({"circuit": name, "k": k, "seed": seed, "proof": proof.hex()})
        print(name, len(proof), flush=True)
        keys.release()
        params.release()
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
