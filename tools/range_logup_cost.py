#!/usr/bin/env python3
"""What the table-logUp mode (flex.FlexKeys(..., logup=True): H2MI_KEYGEN_LOGUP on the hard-wired shape) costs against the permuted argument on the
Range builder's circuits, every ratio inside ONE run (the method of the other tools here: resident workspaces, a warm-up round, then
--proofs alternating rounds, host-inclusive wall clock of create_proof, median (min .. max) in ms):

  * range at --lookup-bits / --k (BASELINE: 16 / 22): the single-column circuit, q_lookup * a against the table;
  * the eight-lookup-column range circuit at --wide-k (11 gate + 8 lookup-advice columns, --wide-count range checks at --wide-bits);
  * each under the permuted key and under logUp keys with lookup_sets 1 and 2 (the single-column circuit has one column: both group
    it alike, and it is proven once), with proof lengths and the device bytes of key and prover;
  * the two level-A calls by themselves, h2mi_plonk_logup_rank_cols_dev + _sum_ranked_dev against _multiplicity_sets_dev + _sum_sets_dev
    on the same K = 1, 2, 6 columns of 2^--k rows (range-check limbs and zeros over the 2^--lookup-bits table), wall clock around a
    device synchronisation.

    python tools/range_logup_cost.py --k 22 --lookup-bits 16 --wide-k 16 --proofs 7 > profiles/range_logup_cost.txt"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRS_SECRET = 0x48911030
X = 0xDEADBEEFCAFE1234


def fmt(ts):
    return f"{statistics.median(ts):.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def prove_rounds(flex, params, keyed, asg, proofs):
    """keyed: [(name, FlexKeys)] -> {name: (times in ms, proof length, (key bytes, prover bytes))}"""
    ws = {name: flex.FlexWorkspace(params, keys) for name, keys in keyed}
    times = {name: [] for name, _ in keyed}
    length = {}
    for rnd in range(proofs + 1):  # round 0 warms every workspace up
        for name, keys in keyed:
            t0 = time.perf_counter()
            proof = flex.create_proof(params, keys, asg, 11 + rnd, ws=ws[name])
            if rnd:
                times[name].append((time.perf_counter() - t0) * 1e3)
            length[name] = len(proof)
    out = {name: (times[name], length[name], ws[name].prover.device_bytes()) for name, _ in keyed}
    for w in ws.values():
        w.release()
    return out


def report(title, flex, params, cs_of, closure, groupings, proofs):
    print(title)
    keyed = []
    for name, logup, sets in groupings:
        cs = cs_of()
        asg = closure(cs)
        t0 = time.perf_counter()
        keys = flex.FlexKeys(params, cs, asg, logup=logup, lookup_sets=sets)
        print(f"  keygen {name}: {time.perf_counter() - t0:.2f} s, degree {cs.degree}, arguments {getattr(cs, 'logup_runs', None)}")
        keyed.append((name, keys))
    res = prove_rounds(flex, params, keyed, asg, proofs)
    base = statistics.median(res[groupings[0][0]][0])
    for name, _, _ in groupings:
        ts, length, (kb, pb) = res[name]
        print(f"  {name:<22} create_proof {fmt(ts)} ms   x{statistics.median(ts) / base:.3f} of permuted   proof {length} B   key {kb / 2**20:.1f} MiB   "
              f"prover {pb / 2**20:.1f} MiB")
    for _, keys in keyed:
        keys.release()


def kernels(h2, k, bits, reps):
    import random

    import numpy as np
    from halo2_scaffold_amd import plonk
    from halo2_scaffold_amd._lib import lib
    from halo2_scaffold_amd.device import DevBuf
    from oracle import bn254 as o

    n, u = 1 << k, (1 << k) - 7
    rng = np.random.default_rng(5)
    one = np.array(o.int_to_limbs(o.to_mont(1, o.R)), dtype=np.uint64)
    small = np.array([o.int_to_limbs(o.to_mont(v, o.R)) for v in range(1 << bits)], dtype=np.uint64)
    table = np.zeros((n, 4), dtype=np.uint64)
    table[: 1 << bits] = small
    d_table = DevBuf.from_numpy(table)
    canon, mont, mult, first, nu = plonk.sort_unique_first(d_table, u)
    print(f"level-A calls at 2^{k} rows, {nu} distinct table values (one column in eight holds limbs on 1/16 of its rows, the rest zeros):")
    del one
    for K in (1, 2, 6):
        cols = []
        for j in range(K):
            col = np.zeros((n, 4), dtype=np.uint64)
            rows = rng.choice(u, size=u // 16, replace=False)
            col[rows] = small[rng.integers(0, 1 << bits, size=rows.size)]
            cols.append(col)
        d_cols = [DevBuf.from_numpy(c) for c in cols]
        d_flat = DevBuf.from_numpy(np.concatenate(cols))
        d_m, d_m2, d_phi, d_phi2 = (DevBuf(n * 32) for _ in range(4))
        d_ranks, d_counts = DevBuf(K * n * 4), DevBuf(nu * 4)
        beta = random.Random(K).randrange(o.R)
        t = {"rank_cols": [], "sum_ranked": [], "multiplicity_sets": [], "sum_sets": []}
        for rep in range(reps + 1):
            for name, call in (("rank_cols", lambda: plonk.logup_rank_cols(k, d_cols, canon, nu, first, u, d_ranks, d_counts, d_m)),
                               ("sum_ranked", lambda: plonk.logup_sum_ranked(k, d_ranks, K, mont, d_counts, first, nu, beta, u, d_phi)),
                               ("multiplicity_sets", lambda: plonk.logup_multiplicity_sets(k, d_flat, K, d_table, u, d_m2)),
                               ("sum_sets", lambda: plonk.logup_sum_sets(k, d_flat, K, d_table, d_m2, beta, u, d_phi2))):
                lib.h2mi_sync()
                t0 = time.perf_counter()
                call()
                lib.h2mi_sync()
                if rep:
                    t[name].append((time.perf_counter() - t0) * 1e3)
        same = d_m.to_numpy().tobytes()[: u * 32] == d_m2.to_numpy().tobytes()[: u * 32] and \
            d_phi.to_numpy().tobytes()[: (u + 1) * 32] == d_phi2.to_numpy().tobytes()[: (u + 1) * 32]
        new = statistics.median(t["rank_cols"]) + statistics.median(t["sum_ranked"])
        old = statistics.median(t["multiplicity_sets"]) + statistics.median(t["sum_sets"])
        print(f"  K = {K}: rank_cols {fmt(t['rank_cols'])} + sum_ranked {fmt(t['sum_ranked'])} = {new:.3f} ms;  multiplicity_sets {fmt(t['multiplicity_sets'])} + "
              f"sum_sets {fmt(t['sum_sets'])} = {old:.3f} ms;  ratio {new / old:.3f};  same M and phi words: {same}")
        for b in d_cols + [d_flat, d_m, d_m2, d_phi, d_phi2, d_ranks, d_counts]:
            b.free()
    for b in (d_table, canon, mont, mult, first):
        b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=22)
    ap.add_argument("--lookup-bits", type=int, default=16)
    ap.add_argument("--wide-k", type=int, default=16)
    ap.add_argument("--wide-bits", type=int, default=12)
    ap.add_argument("--wide-count", type=int, default=20000)
    ap.add_argument("--proofs", type=int, default=7)
    a = ap.parse_args()
    import torch  # noqa: F401  (first, so the library shares torch's HIP runtime)

    import _load_pkg

    h2 = _load_pkg.load()
    h2.init(0)
    from halo2_scaffold_amd import flex

    print(f"range_logup_cost: {torch.cuda.get_device_name(0)}; {a.proofs} alternating rounds after one warm-up round; times in ms, median (min .. max)")
    params = h2.ParamsKZG.setup(a.k, SRS_SECRET)
    report(f"range, LOOKUP_BITS {a.lookup_bits}, DEGREE {a.k} (one gate column, q_lookup * a):", flex, params, lambda: flex.FlexGateCS(lookup=True),
           lambda cs: flex.range_closure(cs, X, a.lookup_bits), [("permuted", False, None), ("logUp", True, None)], a.proofs)
    params.release()
    params = h2.ParamsKZG.setup(a.wide_k, SRS_SECRET)
    report(f"range x {a.wide_count}, LOOKUP_BITS {a.wide_bits}, DEGREE {a.wide_k} (11 gate + 8 lookup-advice columns):", flex, params,
           lambda: flex.FlexGateCS(True, 11, 8, k=a.wide_k), lambda cs: flex.range_closure(cs, X, a.wide_bits, a.wide_count),
           [("permuted", False, None), ("logUp lookup_sets 1", True, 1), ("logUp lookup_sets 2", True, 2)], a.proofs)
    params.release()
    kernels(h2, a.k, a.lookup_bits, a.proofs)


if __name__ == "__main__":
    main()
