#!/usr/bin/env python3
"""What the witness check (h2mi_prover_check) costs inside a proof, and what the host mocks cost beside it.

Circuits: examples/range.rs (LOOKUP_BITS 16 by default) at one DEGREE as a flex key (its lookup the ABI's single-expression
h2mi_lookup, its gate the shape's program) and as a one-pair lookup program with the gate as a program (the pair of
tools/lookup_generality.py), and examples/poseidon.rs at the same DEGREE.  Per circuit: --proofs proofs with the check between the
advice and the lookups and as many without, alternating, after a warm-up pair — host time of the advice phase, of the check and of
the whole create_proof, median (min .. max), and that the two kinds of proof are the same bytes; then one proof with events around
every launch: device time of the check's kernels.  Then the baseline: flex.mock on the same assignments, and custom.mock beside
custom.check on a circuit that uses every row (the 4-bit XOR table of tests/lookup_expr_cases.py) at growing k until the host mock
takes --mock-budget seconds.

    python tools/check_timing.py --k 20 --lookup-bits 16 --proofs 7"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SRS_SECRET = 0x5EC2E7 + 0x48324D49
GROUPS = {"k_expr_check": ("k_expr_check",), "k_copy_check": ("k_copy_check",), "k_lk_member": ("k_lk_member",), "compress": ("k_expr_compress",),
          "sort": ("k_su_", "k_rs_", "k_scan_seg_lookup"), "q * a": ("k_fr_mul",)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--lookup-bits", type=int, default=16)
    ap.add_argument("--proofs", type=int, default=7)
    ap.add_argument("--mock-budget", type=float, default=20.0, help="stop growing k once custom.mock has taken this many seconds")
    args = ap.parse_args()
    import torch  # noqa: F401

    import _load_pkg

    h2 = _load_pkg.load()
    from halo2_scaffold_amd import custom, engine, flex, keygen, poseidon
    from halo2_scaffold_amd._lib import check, lib
    from halo2_scaffold_amd.keygen import _m
    from halo2_scaffold_amd.params import ParamsKZG
    from halo2_scaffold_amd.transcript import Blake2bWrite

    h2.init(0)
    k, R = args.k, flex.R
    params = ParamsKZG.setup(k, SRS_SECRET)
    cs = flex.FlexGateCS(lookup=True)
    asg = flex.range_closure(cs, 0x0123456789ABCDEF, args.lookup_bits)
    abi = cs.abi(k)
    abi.gates = engine.GATES_EXPRESSIONS
    a, q = 0, cs.col_qs[0]
    gate_ops = [(0, a, 1), (0, a, 2), (6, 0, 0), (0, a, 0), (4, 0, 0), (0, a, 3), (5, 0, 0), (1, q, 0), (6, 0, 0), (8, 0, 0)]
    lk = abi.lookups[0]
    lookup_ops = [(0, lk.input.index, 0), (1, lk.selector_fixed, 0), (6, 0, 0), (8, 0, 0), (1, lk.table_fixed, 0), (8, 0, 0)]
    fixed = list(asg.fixed)
    fixed[cs.col_table] = [v % R for v in asg.table_values]
    index = {col: j for j, col in enumerate(cs.perm_columns)}
    copies = [(index[(l[0], l[1])], l[2], index[(r[0], r[1])], r[2]) for l, r in asg.copies]
    keys = engine.Keys(abi, params, fixed, copies, gates=engine.GateProgram.build(gate_ops, []), lookups=engine.LookupProgram.build([1], lookup_ops, []))
    _, repr_ = keygen.transcript_repr(k, cs.degree, keys.fixed_commitments, keys.permutation_commitments)
    pcs = flex.FlexGateCS(lookup=False)
    pasg = poseidon.hash_two_closure(pcs, 0xFEEDFACE, 0xFEEDFACE + 1)
    circuits = [("range, flex key", flex.FlexKeys(params, cs, asg), asg),
                ("range, one-pair program", types.SimpleNamespace(keys=keys, transcript_repr=repr_, release=keys.release), asg),
                ("poseidon, flex key", flex.FlexKeys(params, pcs, pasg), pasg)]
    print(f"DEGREE {k}, LOOKUP_BITS {args.lookup_bits}: {args.proofs} proofs with the check and {args.proofs} without, alternating; host ms, median (min .. max)")
    for name, pk, witness in circuits:
        ws = flex.FlexWorkspace(params, pk)
        times = {"advice": [], "check": [], "proof with the check": [], "proof without": []}
        proofs = set()
        for i in range(args.proofs + 1):
            for with_check in (True, False):
                t = Blake2bWrite.init()
                t.common_scalar(_m(pk.transcript_repr))
                for v in witness.instance:
                    t.common_scalar(_m(v))
                trace = {}
                t0 = time.perf_counter()
                ws.prover.drive(witness.advice, witness.instance, 7, t, trace, witness_check="also" if with_check else None)
                proofs.add(t.finalize())
                ms = (time.perf_counter() - t0) * 1e3
                if not i:
                    continue  # the warm-up pair
                times["proof with the check" if with_check else "proof without"].append(ms)
                if with_check:
                    assert trace["check"] == []
                    phase = dict(trace["phase_ms"])
                    times["advice"].append(phase["advice committed"])
                    times["check"].append(phase["witness check"])
        assert len(proofs) == 1, "a proof's bytes depend on the check"
        print(f"  {name:24s}" + "".join(f"  {what}: {statistics.median(t):.3f} ({min(t):.3f} .. {max(t):.3f})" for what, t in times.items()))
        check(lib.h2mi_profile_reset(), "profile")
        check(lib.h2mi_profile_enable(1), "profile")
        assert flex.device_check(params, pk, witness, 7, ws) == []
        check(lib.h2mi_profile_enable(0), "profile")
        out = []
        for group, prefixes in GROUPS.items():
            total, launches = 0.0, 0
            for prefix in prefixes:
                ms, cnt = C.c_double(), C.c_uint64()
                check(lib.h2mi_profile_query(prefix.encode(), C.byref(ms), C.byref(cnt)), "profile")
                total, launches = total + ms.value, launches + cnt.value
            if launches:
                out.append(f"{group} {total:.3f} ms / {launches}")
        print(f"  {'':24s}  device time of the check's launches (events): " + ", ".join(out))
        t0 = time.perf_counter()
        flex.mock(witness, k)
        print(f"  {'':24s}  flex.mock on the host (it visits the assigned cells only: {sum(len(c) for c in witness.advice)} advice cells): "
              f"{(time.perf_counter() - t0) * 1e3:.1f} ms")
        ws.release()
        pk.release()
    params.release()
    import lookup_expr_cases as cases

    print("a circuit that uses every row (4-bit XOR table, one gate, one three-pair lookup): custom.mock on the host / custom.check on the device, seconds")
    for kk in range(10, k + 1):
        mcs, masg = cases.xor4_circuit(custom, kk)
        p = ParamsKZG.setup(kk, SRS_SECRET)
        ck = custom.Keys(p, mcs, masg)
        ws = custom.Workspace(p, ck)
        custom.check(p, ck, masg, 3, ws=ws)
        t0 = time.perf_counter()
        custom.check(p, ck, masg, 3, ws=ws)
        dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        custom.mock(masg, kk)
        host = time.perf_counter() - t0
        print(f"  k = {kk}: custom.mock {host:.2f} s, custom.check {dev:.4f} s (witness packing and the advice phase included)", flush=True)
        ws.release()
        ck.release()
        p.release()
        if host > args.mock_budget:
            break


if __name__ == "__main__":
    main()
