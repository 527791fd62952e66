#!/usr/bin/env python3
"""What the shuffle argument costs: custom.create_proof of the `mixed` circuit of tests/shuffle_cases.py (a degree-3 gate, a permutation
argument over three columns, the 2-bit XOR lookup, two shuffles) at k rows beside the same circuit and witness with the two shuffles
removed.  --runs alternating pairs after a warm-up pair against resident workspaces, host-inclusive wall clock (witness packing,
transcript, every phase call), median (min .. max) in ms — the method of DESIGN.md 4.  The proof with shuffles is verified once with the
Python-integer verifier of tests/shuffle_cases.py unless --no-verify.

    python tools/shuffle_timing.py --k 16 --runs 7"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SRS_SECRET = 0x5EC2E7 + 0x48324D49


def fmt(ts):
    return f"{statistics.median(ts):8.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--no-verify", action="store_true")
    args = ap.parse_args()
    import torch  # noqa: F401

    import _load_pkg

    h2 = _load_pkg.load()
    import custom_gate_cases as gate_cases
    import shuffle_cases
    from halo2_scaffold_amd import custom
    from halo2_scaffold_amd.params import ParamsKZG
    from oracle import flex as FX

    h2.init(0)
    k = args.k
    params = ParamsKZG.setup(k, SRS_SECRET)
    sides = {}
    for label, shuffles in (("with two shuffles", True), ("shuffles removed", False)):
        cs, asg = shuffle_cases.mixed_circuit(custom, shuffles=shuffles)
        keys = custom.Keys(params, cs, asg)
        sides[label] = (cs, asg, keys, custom.Workspace(params, keys), [])
    proofs = {}
    for run in range(args.runs + 1):
        for label, (cs, asg, keys, ws, times) in sides.items():
            t0 = time.perf_counter()
            proofs[label] = custom.create_proof(params, keys, asg, 1 + run, ws=ws)
            if run:  # the first pair warms up
                times.append((time.perf_counter() - t0) * 1e3)
    verified = "not verified"
    if not args.no_verify:
        cs, asg, keys, _, _ = sides["with two shuffles"]
        ocs = gate_cases.oracle_cs(cs, "mixed")
        oasg = gate_cases.oracle_assignment(ocs, asg)
        vk = FX.VerifierKeys(ocs, k, SRS_SECRET, oasg.fixed, oasg.copies)
        assert shuffle_cases.verify_circuits(vk, cs, proofs["with two shuffles"], [asg.instance])
        verified = "the proof with shuffles verified"
    print(f"custom.create_proof of `mixed` at k = {k}: host-inclusive wall clock in ms, median (min .. max) of {args.runs} alternating runs; {verified}")
    for label, (cs, _, _, _, times) in sides.items():
        print(f"  {label:20s} degree {cs.degree()}  {fmt(times)}   proof bytes {len(proofs[label])}", flush=True)
    a, b = (statistics.median(sides[label][4]) for label in ("with two shuffles", "shuffles removed"))
    print(f"  with / without {a / b:.3f}")
    for _, _, keys, ws, _ in sides.values():
        ws.release()
        keys.release()
    params.release()


if __name__ == "__main__":
    main()
