#!/usr/bin/env python3
"""k_evaluate_h_expr alone, on the shape DESIGN.md 4.5 quotes it at: poseidon at DEGREE 8 — 31 vertical gates q (a + a(wX) a(w^2 X)
- a(w^3 X)) as a program, 33 permutation sets of one column, 512 extended points, random cosets.  One process: --warmup launches,
then --launches launches with the library's events around each; prints the microseconds per launch.  Two builds are compared by
running this from two checkouts in alternation (a parent and a branch; the process pair is the unit, the median over pairs the
figure).  --challenges N: the gates' selector is multiplied by challenge i mod N.

    python tools/expr_kernel_yardstick.py --launches 50 --warmup 10"""
import argparse
import ctypes as C
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--challenges", type=int, default=0)
    args = ap.parse_args()
    import torch  # noqa: F401

    import _load_pkg

    h2 = _load_pkg.load()
    from halo2_scaffold_amd import engine, plonk
    from halo2_scaffold_amd import field as F
    from halo2_scaffold_amd._lib import lib
    from halo2_scaffold_amd.device import DevBuf
    from oracle import bn254 as o

    h2.init(0)
    k, degree, gates, perm = 6, 8, 31, 33
    dom = h2.EvaluationDomain(degree, k)
    size = 1 << dom.extended_k
    rng = random.Random(8)
    coset = lambda: DevBuf.from_numpy(o.pack([rng.randrange(F.FR_MODULUS) for _ in range(size)], F.FR_MODULUS))
    advice, fixed = [coset() for _ in range(gates)], [coset() for _ in range(gates)]
    ops = []
    for g in range(gates):
        ops += [(0, g, 1), (0, g, 2), (6, 0, 0), (0, g, 0), (4, 0, 0), (0, g, 3), (5, 0, 0), (1, g, 0), (6, 0, 0)]
        if args.challenges:
            ops += [(engine.EXPR_CHALLENGE, g % args.challenges, 0), (6, 0, 0)]
        ops.append((8, 0, 0))
    prog = engine.GateProgram.build(ops, [])
    values, sigmas, zs = ([coset() for _ in range(perm)] for _ in range(3))
    l0, l_last, l_active, out = coset(), coset(), coset(), DevBuf(size * 32)
    kw = {"challenges": [rng.randrange(F.FR_MODULUS) for _ in range(args.challenges)]} if args.challenges else {}

    def launch():
        plonk.evaluate_h_expr(dom, prog, advice, fixed, None, values, sigmas, zs, 1, [], l0, l_last, l_active, 3, 5, 7, out, blinding_factors=5, **kw)

    for _ in range(args.warmup):
        launch()
    lib.h2mi_sync()
    lib.h2mi_profile_reset()
    lib.h2mi_profile_filter(b"k_evaluate_h_expr")
    lib.h2mi_profile_enable(1)
    for _ in range(args.launches):
        launch()
    lib.h2mi_sync()
    lib.h2mi_profile_enable(0)
    total, count = C.c_double(), C.c_uint64()
    lib.h2mi_profile_query(b"k_evaluate_h_expr", C.byref(total), C.byref(count))
    assert count.value == args.launches, count.value
    print(f"k_evaluate_h_expr us_per_launch {total.value * 1e3 / count.value:.1f} launches {count.value} challenges {args.challenges}")


if __name__ == "__main__":
    main()
