#!/usr/bin/env python3
"""What ProverGWC's witness phase costs on the reference's StandardPlonk circuit, at each --k:

  (a) the fused route: h2mi_fr_gwc_witness_dev over the proof's own groups (x: 16 polynomials, omega x: 3, x_last: 2) — three launches
  (b) the same W_i composed from the existing entries, per point: zero-fill, h2mi_fr_lincomb_dev, h2mi_fr_kate_division_dev
  (c) for scale, inside whole proofs: the two SHPLONK calls against the one GWC call (its P commitments included), and create_proof

(a) and (b) alternate --reps times after a warm-up on the polynomials a proof left on the device; host clock around work that ends in a
device synchronise, and the summed device time of the launches from the library's launch profile in a run of its own.  (a) and (b) are
compared word for word first.  (c): --proofs alternating proofs per ending against one resident workspace, host-inclusive phase times
from the driver's trace.  All figures median (min .. max).

    python tools/gwc_timing.py --k 8 20"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRS_SECRET = 0x5EC2E7 + 0x48324D49


def fmt(ts):
    return f"{statistics.median(ts):.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[8, 20])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--proofs", type=int, default=7)
    args = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401

    import _load_pkg

    h2 = _load_pkg.load()
    from halo2_scaffold_amd import circuits, engine, keygen, prover
    from halo2_scaffold_amd import field as F
    from halo2_scaffold_amd._lib import check, lib
    from halo2_scaffold_amd.device import DevBuf
    from halo2_scaffold_amd.params import ParamsKZG

    h2.init(0)
    R = F.FR_MODULUS
    for k in args.k:
        n = 1 << k
        params = ParamsKZG.setup(k, SRS_SECRET)
        circuit = circuits.StandardPlonk(None)
        pk = keygen.keygen_pk(params, keygen.keygen_vk(params, circuit), circuit)
        ws = prover.ProverWorkspace(params, pk)
        witness = circuits.StandardPlonk(0xC0FFEE)
        # ---- (c) whole proofs, the two endings alternating
        phases, totals, sizes = {"shplonk": [], "gwc": []}, {"shplonk": [], "gwc": []}, {}
        for i in range(args.proofs + 1):
            for ending in ("shplonk", "gwc"):
                trace = {}
                t0 = time.perf_counter()
                proof = prover.create_proof(params, pk, witness, 7 + i, ws=ws, trace=trace, multiopen=ending)
                wall = (time.perf_counter() - t0) * 1e3
                sizes[ending] = len(proof)
                if i:  # the first proof of each is the warm-up
                    totals[ending].append(wall)
                    phases[ending].append(dict(trace["phase_ms"])[ending + " done"])
        P = ws.prover.gwc_num_points()
        print(f"StandardPlonk, DEGREE {k}: {args.proofs} proofs per ending, alternating; host-inclusive ms, median (min .. max)")
        for ending in ("shplonk", "gwc"):
            print(f"  {ending:8s} opening phase {fmt(phases[ending])}   create_proof {fmt(totals[ending])}   proof bytes {sizes[ending]}")
        print(f"  P = {P} opening points: the GWC tail is {32 * P} bytes, SHPLONK's 64", flush=True)
        # ---- (a) against (b) on the polynomials the last proof left: the groups of the proof's query list
        fixed, sigma = pk.keys.views(engine.PKBUF_FIXED_POLY, 5), pk.keys.views(engine.PKBUF_SIGMA_POLY, 3)
        adv, z = list(ws.advice_polys), list(ws.z_polys)
        groups = [[v.ptr for v in adv + z + list(fixed) + list(sigma)] + [ws.h_poly.ptr, ws.random_poly.ptr], [v.ptr for v in z], [v.ptr for v in z[:2]]]
        x, v = 0x1234567 % R, 0x7654321 % R
        omega = pow(7, (R - 1) >> k, R)
        roots = [x, x * omega % R, x * pow(omega, -6, R) % R]
        limbs = lambda vals: np.ascontiguousarray(np.stack([F.fr_to_mont_limbs(a) for a in vals]))
        z_l, zi_l = limbs(roots), limbs([pow(r, -1, R) for r in roots])
        scal = [limbs([pow(v, j, R) for j in range(len(g))]) for g in groups]
        all_ptrs = (C.c_void_p * sum(len(g) for g in groups))(*[p for g in groups for p in g])
        all_scal = np.ascontiguousarray(np.concatenate(scal))
        counts = (C.c_size_t * len(groups))(*[len(g) for g in groups])
        fused, composed, tmp = [DevBuf(n * 32) for _ in groups], [DevBuf(n * 32) for _ in groups], DevBuf(n * 32)
        fused_ptrs = (C.c_void_p * len(groups))(*[b.ptr for b in fused])

        def route_a():
            check(lib.h2mi_fr_gwc_witness_dev(all_ptrs, all_scal.ctypes.data, counts, z_l.ctypes.data, zi_l.ctypes.data, len(groups), n, fused_ptrs, None), "gwc_witness")

        def route_b():
            for i, g in enumerate(groups):
                ptrs = (C.c_void_p * len(g))(*g)
                check(lib.h2mi_memset_zero(composed[i].ptr, n * 32), "zero")
                check(lib.h2mi_fr_lincomb_dev(ptrs, scal[i].ctypes.data, len(g), n, tmp.ptr, None), "lincomb")
                check(lib.h2mi_fr_kate_division_dev(tmp.ptr, n, z_l[i].ctypes.data, zi_l[i].ctypes.data, composed[i].ptr, None), "kate_division")

        routes = {"(a) fused": route_a, "(b) composed": route_b}
        for call in routes.values():  # warm-up: power tables, scratch
            call()
        check(lib.h2mi_sync(), "sync")
        for a, b in zip(fused, composed):
            assert a.to_numpy(nbytes=n * 32).tobytes() == b.to_numpy(nbytes=n * 32).tobytes(), "the two routes differ"
        wall = {name: [] for name in routes}
        for _ in range(args.reps):
            for name, call in routes.items():
                t0 = time.perf_counter()
                call()
                check(lib.h2mi_sync(), "sync")
                wall[name].append((time.perf_counter() - t0) * 1e3)
        device = {}
        for name, call in routes.items():  # events around every launch: a run of its own
            check(lib.h2mi_profile_reset(), "profile")
            check(lib.h2mi_profile_enable(1), "profile")
            call()
            check(lib.h2mi_sync(), "sync")
            check(lib.h2mi_profile_enable(0), "profile")
            ms, cnt = C.c_double(), C.c_uint64()
            check(lib.h2mi_profile_query(b"k_", C.byref(ms), C.byref(cnt)), "profile")
            device[name] = (ms.value, cnt.value)
        print(f"  the {P} W_i by themselves ({[len(g) for g in groups]} terms), {args.reps} alternating repetitions, word for word equal:")
        for name in routes:
            print(f"    {name:13s} call to synchronise {fmt(wall[name])} ms   device time {device[name][0]:.3f} ms in {device[name][1]} launches")
        print(f"    (a) / (b) {statistics.median(wall['(a) fused']) / statistics.median(wall['(b) composed']):.3f}", flush=True)
        for b in fused + composed + [tmp]:
            b.free()
        ws.release()
        pk.release()
        params.release()


if __name__ == "__main__":
    main()
