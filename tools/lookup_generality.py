#!/usr/bin/env python3
"""The price of giving a range circuit's lookup as data: examples/range.rs (LOOKUP_BITS 16 by default) proved at one DEGREE twice —
its lookup as the ABI's single-expression h2mi_lookup (fixed table sorted at keygen), and re-described as a one-pair
h2mi_lookup_program (compressed with theta, sorted inside every proof) with the gate as a program in both runs, so that the quotient
kernel is the same.  The proofs must be the same bytes.  Per description: the lookups / products / quotient phase times as the host
sees them (medians over --proofs proofs after a warm-up, alternating between the two), then one proof with events around every
launch: device time of the compress, sort and permute kernels.

    python tools/lookup_generality.py --k 20 --lookup-bits 16 --proofs 7"""
import argparse
import ctypes as C
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SRS_SECRET = 0x5EC2E7 + 0x48324D49
PHASES = ("permuted lookup columns committed", "z, random committed", "h pieces committed")
GROUPS = {"compress": ("k_expr_compress",), "sort": ("k_su_", "k_rs_"), "permute": ("k_lk_",), "scans of sort and permute": ("k_scan_seg_lookup",)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--lookup-bits", type=int, default=16)
    ap.add_argument("--proofs", type=int, default=7)
    args = ap.parse_args()
    import torch  # noqa: F401

    import _load_pkg

    h2 = _load_pkg.load()
    from halo2_scaffold_amd import engine, flex, keygen
    from halo2_scaffold_amd._lib import check, lib
    from halo2_scaffold_amd.params import ParamsKZG

    h2.init(0)
    k, R = args.k, flex.R
    cs = flex.FlexGateCS(lookup=True)
    asg = flex.range_closure(cs, 0x0123456789ABCDEF, args.lookup_bits)
    params = ParamsKZG.setup(k, SRS_SECRET)
    abi = cs.abi(k)
    abi.gates = engine.GATES_EXPRESSIONS
    a, q = 0, cs.col_qs[0]
    gate_ops = [(0, a, 1), (0, a, 2), (6, 0, 0), (0, a, 0), (4, 0, 0), (0, a, 3), (5, 0, 0), (1, q, 0), (6, 0, 0), (8, 0, 0)]  # q (a + a(wX) a(w^2 X) - a(w^3 X))
    lk = abi.lookups[0]
    lookup_ops = [(0, lk.input.index, 0), (1, lk.selector_fixed, 0), (6, 0, 0), (8, 0, 0), (1, lk.table_fixed, 0), (8, 0, 0)]
    fixed = list(asg.fixed)
    fixed[cs.col_table] = [v % R for v in asg.table_values]
    index = {col: j for j, col in enumerate(cs.perm_columns)}
    copies = [(index[(l[0], l[1])], l[2], index[(r[0], r[1])], r[2]) for l, r in asg.copies]
    runs = {}
    for name in ("h2mi_lookup", "one-pair program"):
        lp = engine.LookupProgram.build([1], lookup_ops, []) if name != "h2mi_lookup" else None
        keys = engine.Keys(abi, params, fixed, copies, gates=engine.GateProgram.build(gate_ops, []), lookups=lp)
        _, repr_ = keygen.transcript_repr(k, cs.degree, keys.fixed_commitments, keys.permutation_commitments)
        pk = types.SimpleNamespace(keys=keys, transcript_repr=repr_)
        runs[name] = (pk, flex.FlexWorkspace(params, pk), {p: [] for p in PHASES})
    witness = types.SimpleNamespace(advice=asg.advice, instance=asg.instance)
    proofs = {}
    for i in range(args.proofs + 1):
        for name, (pk, ws, times) in runs.items():
            trace = {}
            proofs[name] = flex.create_proof(params, pk, witness, 7, trace=trace, ws=ws)
            if i:  # the first proof of each is the warm-up
                for phase, ms in trace["phase_ms"]:
                    if phase in times:
                        times[phase].append(ms)
    assert proofs["h2mi_lookup"] == proofs["one-pair program"], "the two descriptions give different proofs"
    print(f"range, LOOKUP_BITS {args.lookup_bits}, DEGREE {k}: {args.proofs} proofs each, alternating; host ms per phase, median (min .. max)")
    for name, (pk, ws, times) in runs.items():
        print(f"  {name:17s}" + "".join(f"  {p.split(' committed')[0]}: {statistics.median(t):.3f} ({min(t):.3f} .. {max(t):.3f})" for p, t in times.items()))
    for name, (pk, ws, times) in runs.items():
        check(lib.h2mi_profile_reset(), "profile")
        check(lib.h2mi_profile_enable(1), "profile")
        flex.create_proof(params, pk, witness, 7, ws=ws)
        check(lib.h2mi_profile_enable(0), "profile")
        out = []
        for group, prefixes in GROUPS.items():
            total, launches = 0.0, 0
            for prefix in prefixes:
                ms, cnt = C.c_double(), C.c_uint64()
                check(lib.h2mi_profile_query(prefix.encode(), C.byref(ms), C.byref(cnt)), "profile")
                total, launches = total + ms.value, launches + cnt.value
            out.append(f"{group} {total:.3f} ms / {launches} launches")
        print(f"  {name:17s}  device time in one proof: " + ", ".join(out))
    for name, (pk, ws, times) in runs.items():
        ws.release()
        pk.keys.release()
    params.release()


if __name__ == "__main__":
    main()
