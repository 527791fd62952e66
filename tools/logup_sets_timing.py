#!/usr/bin/env python3
"""What merging the input sets of a logUp lookup saves where K lookup-advice columns share one table: a range circuit through custom.py
with --columns lookup-advice columns (4 and 6 by default), each looked up in one fixed table 0 .. 2^LOOKUP_BITS - 1, one witness, proved
under a plain key, a logUp key, and logUp keys of the merged system (ConstraintSystem.merge_lookups at the default budget and at
max_degree = 9).  --proofs alternating rounds after a warm-up round against resident workspaces: host-inclusive wall clock in total and
per phase, median (min .. max) in ms — the method of tools/logup_timing.py.  Every proof of the last round is verified in the run by the
Python-integer verifier of tests/logup_sets_cases.py, unless --no-verify.  Then the two sets calls by themselves on vectors of the
proof's shape, with events around every launch: device time of h2mi_plonk_logup_multiplicity_sets_dev and of
h2mi_plonk_logup_sum_sets_dev.

    python tools/logup_sets_timing.py --k 20 --lookup-bits 16 --proofs 7"""
import argparse
import ctypes as C
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SRS_SECRET = 0x5EC2E7 + 0x48324D49
LIMBS = 64  # range-checked cells per lookup-advice column


def fmt(ts):
    return f"{statistics.median(ts):.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def circuit(custom, columns: int, bits: int, merge):
    """merge: None (the lookups as declared) or the budget of merge_lookups (0: its default)"""
    meta = custom.ConstraintSystem()
    cols = [meta.advice_column() for _ in range(columns)]
    table = meta.fixed_column()
    q = meta.selector()
    meta.enable_equality(cols[0])
    cur = custom.Rotation.cur()
    meta.create_gate("first limb is zero", lambda meta: [meta.query_selector(q) * meta.query_advice(cols[0], cur)])
    for j, c in enumerate(cols):
        meta.lookup("range %d" % j, lambda meta, c=c: [(meta.query_advice(c, cur), meta.query_fixed(table, cur))])
    if merge is not None:
        meta.merge_lookups(merge or None)
    region = custom.Assignment(meta)
    for v in range(1 << bits):
        region.assign_fixed(table, v, v)
    rng = random.Random(20)
    cell = region.assign_advice(cols[0], 0, 0)
    region.enable_selector(q, 0)
    for c in cols:
        for row in range(1, LIMBS):
            region.assign_advice(c, row, rng.randrange(1 << bits))
    region.copy_advice(cell, cols[0], LIMBS + 1)
    return meta, region


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--lookup-bits", type=int, default=16)
    ap.add_argument("--proofs", type=int, default=7)
    ap.add_argument("--columns", type=int, nargs="+", default=[4, 6])
    ap.add_argument("--no-verify", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401

    import _load_pkg

    h2 = _load_pkg.load()
    from halo2_scaffold_amd import custom, plonk
    from halo2_scaffold_amd import field as F
    from halo2_scaffold_amd._lib import check, lib
    from halo2_scaffold_amd.device import DevBuf
    from halo2_scaffold_amd.params import ParamsKZG

    h2.init(0)
    k, R = args.k, custom.R
    params = ParamsKZG.setup(k, SRS_SECRET)
    for columns in args.columns:
        runs = {}
        for name, merge, logup in (("plain", None, False), ("logUp", None, True), ("logUp merged", 0, True), ("logUp merged, 9", 9, True)):
            cs, asg = circuit(custom, columns, args.lookup_bits, merge)
            keys = custom.Keys(params, cs, asg, logup=logup)
            runs[name] = (cs, asg, keys, custom.Workspace(params, keys), {}, [], logup)
        proofs = {}
        for i in range(args.proofs + 1):
            for name, (cs, asg, keys, ws, times, total, logup) in runs.items():
                trace = {}
                t0 = time.perf_counter()
                proofs[name] = custom.create_proof(params, keys, asg, 7 + i, trace=trace, ws=ws)
                wall = (time.perf_counter() - t0) * 1e3
                if i:  # the first proof of each is the warm-up
                    total.append(wall)
                    for phase, ms in trace["phase_ms"]:
                        times.setdefault(phase, []).append(ms)
        verified = "not verified"
        if not args.no_verify:
            import custom_gate_cases as gate_cases
            import logup_sets_cases
            from oracle import flex as FX

            for name, (cs, asg, keys, ws, times, total, logup) in runs.items():
                ocs = gate_cases.oracle_cs(cs, name)
                oasg = gate_cases.oracle_assignment(ocs, asg)
                vk = FX.VerifierKeys(ocs, k, SRS_SECRET, oasg.fixed, oasg.copies)
                assert logup_sets_cases.verify_circuits(vk, cs, proofs[name], [asg.instance], logup=logup), f"the proof of the {name} key is rejected"
            verified = "every key's last proof verified"
        print(f"range, {columns} lookup-advice columns over one table, LOOKUP_BITS {args.lookup_bits}, DEGREE {k}: {args.proofs} proofs each, alternating; "
              f"host-inclusive ms, median (min .. max); {verified}")
        for name, (cs, asg, keys, ws, times, total, logup) in runs.items():
            print(f"  {name:16s} degree {cs.degree()} arguments {[len(a) for a in cs.lookup_arguments]} create_proof {fmt(total)}   proof bytes {len(proofs[name])}")
            for p, t in times.items():
                print(f"      {p:40s} {fmt(t)}")
        base = statistics.median(runs["plain"][5])
        for name in list(runs)[1:]:
            print(f"  {name} / plain {statistics.median(runs[name][5]) / base:.3f}", flush=True)
        for name, (cs, asg, keys, ws, times, total, logup) in runs.items():
            ws.release()
            keys.release()
        # the two device calls by themselves: `columns` input vectors of the witness's shape and the table on the rows
        n = 1 << k
        u = n - (runs["plain"][0].blinding_factors() + 1)
        asg = runs["plain"][1]
        rows = np.zeros((columns * n, 4), dtype=np.uint64)
        for j in range(columns):
            for row, v in asg.advice[j].items():
                if v:
                    rows[j * n + row] = F.fr_to_mont_limbs(v)
        table = np.zeros((n, 4), dtype=np.uint64)
        for v in range(1, 1 << args.lookup_bits):
            table[v] = F.fr_to_mont_limbs(v)
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

        for sets in (1, columns):
            missing = []
            ms, cnt = device_ms(lambda: missing.append(plonk.logup_multiplicity_sets(k, d_a, sets, d_t, u, d_m)))
            assert missing == [0, 0]
            print(f"  h2mi_plonk_logup_multiplicity_sets_dev, {sets} set(s), {u} usable rows: {ms:.3f} ms device time in {cnt} launches")
            ms, cnt = device_ms(lambda: plonk.logup_sum_sets(k, d_a, sets, d_t, d_m, 0x1234567, u, d_phi))
            print(f"  h2mi_plonk_logup_sum_sets_dev, {sets} set(s): {ms:.3f} ms device time in {cnt} launches", flush=True)
        for b in (d_a, d_t, d_m, d_phi):
            b.free()
    params.release()


if __name__ == "__main__":
    main()
