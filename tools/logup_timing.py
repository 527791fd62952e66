#!/usr/bin/env python3
"""What the logUp argument saves on the project's most expensive argument: examples/range.rs (LOOKUP_BITS 16 by default) at one DEGREE,
its lookup re-described as a one-pair h2mi_lookup_program and the gate as a program (the setup of tools/lookup_generality.py), proved
with the same witness under a plain key and under a logUp key (H2MI_KEYGEN_LOGUP).  --proofs alternating pairs after a warm-up pair
against resident workspaces: host-inclusive wall clock in total and per phase, median (min .. max) in ms — the method of DESIGN.md 4.
Both proofs of the last pair are verified in the run, each by its Python-integer verifier (tests/logup_cases.py), unless --no-verify.
Then the two new device calls by themselves, on vectors of the proof's shape (the lookup's input column and table on the rows), with
events around every launch: device time of h2mi_plonk_logup_multiplicity_dev and of h2mi_plonk_logup_sum_dev.

    python tools/logup_timing.py --k 20 --lookup-bits 16 --proofs 7"""
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
PHASES = ("advice committed", "permuted lookup columns committed", "z, random committed", "h pieces committed", "evaluations written", "shplonk done")
X = 0x0123456789ABCDEF


def fmt(ts):
    return f"{statistics.median(ts):.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--lookup-bits", type=int, default=16)
    ap.add_argument("--proofs", type=int, default=7)
    ap.add_argument("--no-verify", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401

    import _load_pkg

    h2 = _load_pkg.load()
    from halo2_scaffold_amd import engine, flex, keygen, plonk
    from halo2_scaffold_amd import field as F
    from halo2_scaffold_amd._lib import check, lib
    from halo2_scaffold_amd.device import DevBuf
    from halo2_scaffold_amd.params import ParamsKZG

    h2.init(0)
    k, R = args.k, flex.R
    cs = flex.FlexGateCS(lookup=True)
    asg = flex.range_closure(cs, X, args.lookup_bits)
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
    copies = [(index[(le[0], le[1])], le[2], index[(ri[0], ri[1])], ri[2]) for le, ri in asg.copies]
    runs = {}
    for name, logup in (("plain key", False), ("logUp key", True)):
        keys = engine.Keys(abi, params, fixed, copies, gates=engine.GateProgram.build(gate_ops, []), lookups=engine.LookupProgram.build([1], lookup_ops, []),
                           logup=logup)
        _, repr_ = keygen.transcript_repr(k, cs.degree, keys.fixed_commitments, keys.permutation_commitments)
        pk = types.SimpleNamespace(keys=keys, transcript_repr=repr_)
        runs[name] = (pk, flex.FlexWorkspace(params, pk), {p: [] for p in PHASES}, [])
    witness = types.SimpleNamespace(advice=asg.advice, instance=asg.instance)
    proofs = {}
    for i in range(args.proofs + 1):
        for name, (pk, ws, times, total) in runs.items():
            trace = {}
            t0 = time.perf_counter()
            proofs[name] = flex.create_proof(params, pk, witness, 7 + i, trace=trace, ws=ws)
            wall = (time.perf_counter() - t0) * 1e3
            if i:  # the first proof of each is the warm-up
                total.append(wall)
                for phase, ms in trace["phase_ms"]:
                    if phase in times:
                        times[phase].append(ms)
    verified = "not verified"
    if not args.no_verify:
        import logup_cases
        import lookup_expr_cases
        import phase_cases
        from oracle import flex as FX

        ocs, oasg = lookup_expr_cases.golden_range_case(None, {"x": hex(X), "lookup_bits": args.lookup_bits, "k": k})
        vk = FX.VerifierKeys(ocs, k, SRS_SECRET, oasg.fixed, oasg.copies)
        gates = phase_cases.without_challenges(ocs.gates)
        lks = phase_cases.without_challenges_lookups(lookup_expr_cases.one_pair_lookups(ocs))
        assert logup_cases.verify(vk, proofs["plain key"], [oasg.instance], gates, lks, logup=False), "the plain key's proof is rejected"
        assert logup_cases.verify(vk, proofs["logUp key"], [oasg.instance], gates, lks, logup=True), "the logUp key's proof is rejected"
        verified = "both proofs verified"
    print(f"range, LOOKUP_BITS {args.lookup_bits}, DEGREE {k}, one-pair lookup program: {args.proofs} proofs each, alternating; host-inclusive ms, "
          f"median (min .. max); {verified}")
    for name, (pk, ws, times, total) in runs.items():
        print(f"  {name:10s} create_proof {fmt(total)}   proof bytes {len(proofs[name])}")
        for p, t in times.items():
            if t:
                print(f"      {p.split(' committed')[0]:32s} {fmt(t)}")
    plain, lu = (statistics.median(runs[name][3]) for name in ("plain key", "logUp key"))
    print(f"  logUp / plain {lu / plain:.3f}", flush=True)
    # the two device calls by themselves: the lookup's input q_lookup * a and its table on the rows
    n, bf = 1 << k, cs.blinding_factors
    u = n - (bf + 1)
    rows = np.zeros((n, 4), dtype=np.uint64)
    sel, adv = asg.fixed[lk.selector_fixed], asg.advice[lk.input.index]
    for row in (sel if isinstance(sel, dict) else range(len(sel))):
        v = sel[row] * (adv.get(row, 0) if isinstance(adv, dict) else adv[row]) % R
        if v:
            rows[row] = F.fr_to_mont_limbs(v)
    table = np.zeros((n, 4), dtype=np.uint64)
    for row, v in enumerate(asg.table_values):
        if v % R:
            table[row] = F.fr_to_mont_limbs(v % R)
    d_a, d_t, d_m, d_phi = DevBuf.from_numpy(rows), DevBuf.from_numpy(table), DevBuf(n * 32), DevBuf(n * 32)

    def device_ms(call):
        call()  # warm-up: scratch allocations
        check(lib.h2mi_profile_reset(), "profile")
        check(lib.h2mi_profile_enable(1), "profile")
        call()
        check(lib.h2mi_profile_enable(0), "profile")
        ms, cnt = C.c_double(), C.c_uint64()
        check(lib.h2mi_profile_query(b"k_", C.byref(ms), C.byref(cnt)), "profile")
        return ms.value, cnt.value

    missing = []
    ms, cnt = device_ms(lambda: missing.append(plonk.logup_multiplicity(k, d_a, d_t, u, d_m)))
    assert missing == [0, 0]
    print(f"  h2mi_plonk_logup_multiplicity_dev, {u} usable rows: {ms:.3f} ms device time in {cnt} launches")
    ms, cnt = device_ms(lambda: plonk.logup_sum(k, d_a, d_t, d_m, 0x1234567, u, d_phi))
    print(f"  h2mi_plonk_logup_sum_dev: {ms:.3f} ms device time in {cnt} launches")
    for b in (d_a, d_t, d_m, d_phi):
        b.free()
    for name, (pk, ws, times, total) in runs.items():
        ws.release()
        pk.keys.release()
    params.release()


if __name__ == "__main__":
    main()
