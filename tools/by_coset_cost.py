#!/usr/bin/env python3
"""What H2MI_KEYGEN_BY_COSET costs and saves: for StandardPlonk at --k-plonk, the poseidon builder at --k-poseidon and the
range builder at --k-range with --lookup-bits, a resident key and a by-coset key of the same circuit side by side —

  * device bytes of the key and of one prover (h2mi_prover_device_bytes, taken after the first proof: SHPLONK's lazily grown scratch
    included; the library-wide caches — window tables, twiddles, scratch arena — are not in it),
  * create_proof, host-inclusive: a host clock from the call to a device synchronise behind it, --proofs proofs per mode after one
    warm-up proof each, the two modes ALTERNATING against one SRS, witness generation outside the clock; median (min .. max),
  * the by-coset time as a ratio to the resident time of the same run.

The first proof of each mode is compared byte for byte before anything is timed.

    python tools/by_coset_cost.py [--only plonk poseidon range]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRS_SECRET = 0x5EC2E7 + 0x48324D49


def fmt(ts):
    return f"{statistics.median(ts):.2f} ({min(ts):.2f} .. {max(ts):.2f})"


def mib(b):
    return f"{b / (1 << 20):.1f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="+", choices=["plonk", "poseidon", "range"], default=["plonk", "poseidon", "range"])
    ap.add_argument("--k-plonk", type=int, default=20)
    ap.add_argument("--k-poseidon", type=int, default=20)
    ap.add_argument("--k-range", type=int, default=22)
    ap.add_argument("--lookup-bits", type=int, default=16)
    ap.add_argument("--proofs", type=int, default=7)
    args = ap.parse_args()
    import torch  # noqa: F401

    import _load_pkg

    h2 = _load_pkg.load()
    from halo2_scaffold_amd import circuits, flex, keygen, poseidon, prover
    from halo2_scaffold_amd._lib import check, lib
    from halo2_scaffold_amd.params import ParamsKZG

    h2.init(0)

    # per mode: (key, workspace, engine.Prover, witness(i) -> a call that makes proof i)
    def plonk(k):
        params = ParamsKZG.setup(k, SRS_SECRET)
        circuit = circuits.StandardPlonk(None)
        vk = keygen.keygen_vk(params, circuit)
        modes = {}
        for by_coset in (False, True):
            pk = keygen.keygen_pk(params, vk, circuit, by_coset=by_coset)
            ws = prover.ProverWorkspace(params, pk)

            def witness(i, pk=pk, ws=ws):
                w = circuits.StandardPlonk(0xC0FFEE + i)
                return lambda: prover.create_proof(params, pk, w, 7 + i, ws=ws)

            modes[by_coset] = (pk, ws, ws.prover, witness)
        return params, modes

    def flex_shape(k, lookup, build):
        params = ParamsKZG.setup(k, SRS_SECRET)
        cs = flex.FlexGateCS(lookup=lookup)
        x0 = 0x0123456789ABCDEF
        first = build(cs, x0)
        modes = {}
        for by_coset in (False, True):
            keys = flex.FlexKeys(params, cs, first, by_coset=by_coset)
            ws = flex.FlexWorkspace(params, keys)

            def witness(i, keys=keys, ws=ws):
                asg = build(cs, (x0 + i) % (1 << 64))
                return lambda: flex.create_proof(params, keys, asg, 31337 + i, ws=ws)

            modes[by_coset] = (keys, ws, ws.prover, witness)
        return params, modes

    shapes = {
        "plonk": (f"StandardPlonk, DEGREE {args.k_plonk}", lambda: plonk(args.k_plonk)),
        "poseidon": (f"poseidon builder, DEGREE {args.k_poseidon}", lambda: flex_shape(args.k_poseidon, False, lambda c, x: poseidon.hash_two_closure(c, x, x ^ 0x5A5A5A5A))),
        "range": (f"range builder, DEGREE {args.k_range}, LOOKUP_BITS {args.lookup_bits}",
                  lambda: flex_shape(args.k_range, True, lambda c, x: flex.range_closure(c, x, args.lookup_bits))),
    }
    for name in args.only:
        title, make = shapes[name]
        params, modes = make()
        first = {}
        for by_coset, (_, _, _, witness) in modes.items():  # the warm-up proof of each mode, the same witness and seed
            first[by_coset] = witness(0)()
        check(lib.h2mi_sync(), "sync")
        assert first[False] == first[True], f"{title}: the by-coset proof differs from the resident one"
        times = {False: [], True: []}
        for i in range(1, args.proofs + 1):
            for by_coset in (False, True):
                run = modes[by_coset][3](i)  # the witness, outside the clock
                check(lib.h2mi_sync(), "sync")
                t0 = time.perf_counter()
                run()
                check(lib.h2mi_sync(), "sync")
                times[by_coset].append(1e3 * (time.perf_counter() - t0))
        print(f"{title}: {args.proofs} proofs per mode, alternating, after one warm-up each; proof bytes equal ({len(first[True])} bytes)")
        for by_coset in (False, True):
            kb, pb = modes[by_coset][2].device_bytes()
            print(f"  {'by coset' if by_coset else 'resident':9s} device MiB: key {mib(kb)}, prover {mib(pb)}, together {mib(kb + pb)};  create_proof ms {fmt(times[by_coset])}")
        res, byc = (sum(modes[m][2].device_bytes()) for m in (False, True))
        print(f"  by coset / resident: device bytes {byc / res:.3f}, create_proof time {statistics.median(times[True]) / statistics.median(times[False]):.3f}", flush=True)
        for keys, ws, _, _ in modes.values():
            ws.release()
            keys.release()
        params.release()


if __name__ == "__main__":
    main()
