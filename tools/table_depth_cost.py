#!/usr/bin/env python3
"""What a table depth costs and saves (h2mi_bases_register_depth): for base sets of 2^k points, --k, registered
at depth 1 and at each depth of --depths (W = the window count of the size) —

  * h2mi_bases_memory (table and workspace bytes, as asked of the allocator) beside the difference of the device's free memory
    around the registration (what the allocator really took),
  * the registration itself, a host clock around the call (it synchronises),
  * one MSM of uniform scalars alone, and eight back to back: a host clock from the first call to a device synchronise behind the
    last, --reps times, depth 1 and depth D ALTERNATING on handles over the same points; median (min .. max),
  * create_proof of StandardPlonk at --k-proof from parameters of each depth, host-inclusive, --proofs proofs per depth after one
    warm-up each, depth 1 and depth D alternating; the proofs' bytes are compared first.

Every figure of a depth is also given as a ratio to depth 1 of the same run.  Written to --out as well as printed.

    python tools/table_depth_cost.py [--k 20 22] [--depths 2 4 W] [--out profiles/table_depth_cost.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRS_SECRET = 0x5EC2E7 + 0x7AB1E


def fmt(ts):
    return f"{statistics.median(ts):.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def mib(b):
    return f"{b / (1 << 20):.1f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--depths", nargs="+", default=["2", "4", "W"])
    ap.add_argument("--k-proof", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--proofs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_depth_cost.txt"))
    args = ap.parse_args()
    import torch

    import _load_pkg

    h2 = _load_pkg.load()
    from halo2_scaffold_amd import circuits, keygen, prover
    from halo2_scaffold_amd._lib import check, lib
    from halo2_scaffold_amd.device import DevBuf
    from halo2_scaffold_amd.params import ParamsKZG
    from oracle import bn254 as o

    h2.init(0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def info(h):
        c, W = C.c_uint32(), C.c_uint32()
        check(lib.h2mi_bases_info(h, C.byref(c), C.byref(W), None, None), "info")
        return c.value, W.value

    def memory(h):
        d, rows, tb, wb = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
        check(lib.h2mi_bases_memory(h, C.byref(d), C.byref(rows), C.byref(tb), C.byref(wb)), "memory")
        return d.value, rows.value, tb.value, wb.value

    def register(points, n, D):
        """-> (handle, milliseconds, bytes the device's free memory fell by)"""
        check(lib.h2mi_sync(), "sync")
        free0 = torch.cuda.mem_get_info()[0]
        h = C.c_uint64()
        t0 = time.perf_counter()
        check(lib.h2mi_bases_register_depth_dev(points.ptr, n, D, C.byref(h)), "register")
        check(lib.h2mi_sync(), "sync")
        ms = 1e3 * (time.perf_counter() - t0)
        return h.value, ms, free0 - torch.cuda.mem_get_info()[0]

    def msm_times(h, scalars, n, out, count):
        check(lib.h2mi_sync(), "sync")
        t0 = time.perf_counter()
        for j in range(count):
            check(lib.h2mi_msm_bn254_g1_dev(h, scalars.ptr, n, out.ptr + 96 * j, None), "msm")
        check(lib.h2mi_sync(), "sync")
        return 1e3 * (time.perf_counter() - t0)

    for k in args.k:
        n = 1 << k
        srs = ParamsKZG.setup(k, SRS_SECRET, register=False)
        scalars = DevBuf.from_numpy(o.random_field_limbs(n, 0x7AB1E + k))
        out = DevBuf(96 * 8)
        h1, ms1, took1 = register(srs._g_dev, n, 1)
        c, W = info(h1)
        say(f"2^{k} points: c = {c}, W = {W}; MSMs of uniform scalars, {args.reps} repetitions, depth 1 and depth D alternating")
        _, rows, tb1, wb1 = memory(h1)
        say(f"  depth 1   rows {rows:2d}  table MiB {mib(tb1)}  workspace MiB {mib(wb1)}  free memory fell by MiB {mib(took1)}  registration ms {ms1:.1f}")
        want = None
        for name in args.depths:
            D = W if name == "W" else int(name)
            h, ms, took = register(srs._g_dev, n, D)
            Dp, rows, tb, wb = memory(h)
            for hh in (h1, h):  # warm-up, and the same point from both
                msm_times(hh, scalars, n, out, 1)
                got = o.unpack_jacobian(out.to_numpy(nbytes=96))
                assert want is None or got == want, f"depth {D} at 2^{k}: another point than depth 1"
                want = got
            lone, b2b = {1: [], D: []}, {1: [], D: []}
            for _ in range(args.reps):
                for d, hh in ((1, h1), (D, h)):
                    lone[d].append(msm_times(hh, scalars, n, out, 1))
                for d, hh in ((1, h1), (D, h)):
                    b2b[d].append(msm_times(hh, scalars, n, out, 8) / 8)
            med = statistics.median
            say(f"  depth {D:<3d} rows {rows:2d}  table MiB {mib(tb)}  workspace MiB {mib(wb)}  free memory fell by MiB {mib(took)}  registration ms {ms:.1f}")
            say(f"            one MSM alone ms: depth 1 {fmt(lone[1])}, depth {D} {fmt(lone[D])};  eight back to back, ms per MSM: depth 1 {fmt(b2b[1])}, depth {D} {fmt(b2b[D])}")
            say(f"            depth {D} / depth 1: table + workspace bytes {(tb + wb) / (tb1 + wb1):.3f}, registration {ms / ms1:.3f}, "
                f"one MSM {med(lone[D]) / med(lone[1]):.3f}, back to back {med(b2b[D]) / med(b2b[1]):.3f}")
            check(lib.h2mi_bases_release(h), "release")
        check(lib.h2mi_bases_release(h1), "release")
        for b in (scalars, out):
            b.free()
        srs.release()

    k = args.k_proof
    circuit = circuits.StandardPlonk(None)

    def proving(D):
        params = ParamsKZG.setup(k, SRS_SECRET, table_depth=D)
        pk = keygen.keygen_pk(params, keygen.keygen_vk(params, circuit), circuit)
        ws = prover.ProverWorkspace(params, pk)
        return params, pk, ws, lambda i: prover.create_proof(params, pk, circuits.StandardPlonk(0xC0FFEE + i), 7 + i, ws=ws)

    p1 = proving(1)
    _, W = info(p1[0].g_handle)
    first = p1[3](0)
    say(f"StandardPlonk, DEGREE {k}: create_proof, {args.proofs} proofs per depth, depth 1 and depth D alternating, after one warm-up each")
    for name in args.depths:
        D = W if name == "W" else int(name)
        pd = proving(D)
        assert pd[3](0) == first, f"depth {D}: the proof differs from the depth-1 parameters' proof"
        times = {1: [], D: []}
        for i in range(1, args.proofs + 1):
            for d, p in ((1, p1), (D, pd)):
                check(lib.h2mi_sync(), "sync")
                t0 = time.perf_counter()
                p[3](i)
                check(lib.h2mi_sync(), "sync")
                times[d].append(1e3 * (time.perf_counter() - t0))
        b1, bd = sum(p1[0].device_bytes()), sum(pd[0].device_bytes())
        say(f"  depth {D:<3d} parameters' tables + workspaces MiB {mib(bd)} (depth 1: {mib(b1)});  create_proof ms: depth 1 {fmt(times[1])}, depth {D} {fmt(times[D])}")
        say(f"            depth {D} / depth 1: bytes {bd / b1:.3f}, create_proof {statistics.median(times[D]) / statistics.median(times[1]):.3f}")
        pd[2].release()
        pd[1].release()
        pd[0].release()
    p1[2].release()
    p1[1].release()
    p1[0].release()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
