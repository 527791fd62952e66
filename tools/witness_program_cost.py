#!/usr/bin/env python3
"""What a witness program (scaffold.gen_key(..., witness_program=True): witness.py, csrc/h2mi_witness.hip) costs against host synthesis,
every ratio inside ONE run, on two circuits: --wide-count range checks (LOOKUP_BITS --wide-bits, DEGREE --wide-k, 11 gate + 8
lookup-advice columns) and the reference's range circuit (LOOKUP_BITS --lookup-bits, DEGREE --k, one column).  Per circuit, alternating
rounds after one warm-up round, host-inclusive wall clock, median (min .. max) in ms:

  * the part before the prover: host synthesis (the closure through flex.Context, finish) + engine.pack_cells + h2mi_prover_advice,
    against the program's run + the public cells read back + pack_cells + h2mi_prover_advice — the commitments of both compared first;
  * the whole scaffold.prove_private, the closure called against the program run;
  * the program's launches from the library's profile: every k_witness_level launch with the bytes the file header of
    csrc/h2mi_witness.hip states for its ops (144 per GATE, 80 per other op) over its time as a share of the HBM roofline (8 TB/s), the
    widest level first; k_witness_levels_wg and k_witness_place as they are.
Then the narrow / wide threshold: synthetic programs of --levels levels of W copies and limbs each, W on both sides of 1024 — the time
per level inside one workgroup against the time of a grid launch per level.

    python tools/witness_program_cost.py --proofs 5 > profiles/witness_program_cost.txt"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRS_SECRET = 0x48911030
X = 0xDEADBEEFCAFE1234
STEP = 0x9E3779B97F4A7C15
HBM = 8e12


def fmt(ts):
    return f"{statistics.median(ts):.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def range_closure(ctx, xs, make_public):
    """flex.range_closure's body (reference examples/range.rs) for every value of xs"""
    for x in xs:
        xc = ctx.load_witness(x)
        make_public.append(xc)
        ctx.range_check(xc, 64, ctx.lookup_bits)
        ctx.add(xc, xc)


def launches(lib, call):
    """[(kernel, ms)] of the witness kernels during call(), in launch order, from the library's profile"""
    lib.h2mi_profile_reset(); lib.h2mi_profile_filter(b"k_witness"); lib.h2mi_profile_enable(1)
    call(); lib.h2mi_sync(); lib.h2mi_profile_enable(0)
    need = C.c_size_t()
    lib.h2mi_profile_dump(None, 0, C.byref(need))
    buf = C.create_string_buffer(need.value + 1)
    lib.h2mi_profile_dump(buf, need.value + 1, C.byref(need))
    lib.h2mi_profile_reset(); lib.h2mi_profile_filter(b"")
    return [(line.split()[0], float(line.split()[2])) for line in buf.value.decode().splitlines()]


def level_bytes(program, level):
    """the algorithmic bytes of one level: 16 (op) + 32 per operand + 32 (store) per op"""
    ends = [0] + [int(e) for e in program.level_ends]
    kinds = program.ops[ends[level]:ends[level + 1], 1] & 0xFF
    gates = int((kinds == 3).sum())
    return 144 * gates + 80 * (len(kinds) - gates)


def circuit(h2, title, k, lookup_bits, cs, xs, proofs):
    from halo2_scaffold_amd import engine, flex, scaffold, witness
    from halo2_scaffold_amd._lib import lib

    os.environ["DEGREE"], os.environ["LOOKUP_BITS"] = str(k), str(lookup_bits)
    print(title)
    params = h2.ParamsKZG.setup(k, SRS_SECRET)
    t0 = time.perf_counter()
    program, recorded = witness.Program.record(range_closure, [0] * len(xs), cs, lookup_bits)
    t_record = time.perf_counter() - t0
    keys = flex.FlexKeys(params, cs, recorded)
    pk = scaffold.ProvingKey(params, keys)
    pk.lookup_bits = lookup_bits
    break_points = [list(recorded.break_points)]
    dev = program.on_device()
    info = dev.info
    sizes = program.level_sizes
    print(f"  {program.n_cells} cells, {len(sizes)} levels (widest {max(sizes)}), {len(program.checks)} checks, columns of "
          f"{[len(p) for p in program.placement]} cells; recorded in {t_record:.2f} s; {info.n_grid_launches} grid + {info.n_wg_launches} "
          f"workgroup launches + 1; {info.device_bytes / 2**20:.1f} MiB on the device")
    prover = pk.workspace.prover
    pts = prover._points.ctypes.data
    flat = witness.flatten_inputs(xs)

    def host_part(times):
        t0 = time.perf_counter()
        asg = scaffold._synthesize(range_closure, xs, cs, lookup_bits)
        t1 = time.perf_counter()
        cells, keep = engine.pack_cells(asg.advice)
        t2 = time.perf_counter()
        inst, n_inst = prover._public_inputs(asg.instance)
        engine.check(lib.h2mi_prover_advice(prover.handle, cells, inst.ctypes.data, n_inst, 5, pts), "advice")
        lib.h2mi_sync()
        t3 = time.perf_counter()
        times.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3))
        return prover._points[:prover.counts.advice].copy(), asg.instance

    def program_part(times):
        t0 = time.perf_counter()
        columns = dev.run(flat)
        instance = dev.read(program.public)
        t1 = time.perf_counter()
        cells, keep = engine.pack_cells(columns)
        t2 = time.perf_counter()
        inst, n_inst = prover._public_inputs(instance)
        engine.check(lib.h2mi_prover_advice(prover.handle, cells, inst.ctypes.data, n_inst, 5, pts), "advice")
        lib.h2mi_sync()
        t3 = time.perf_counter()
        times.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3))
        return prover._points[:prover.counts.advice].copy(), instance

    host, prog = [], []
    a, b = host_part([]), program_part([])  # warm-up; the same commitments and public inputs both ways
    assert (a[0] == b[0]).all() and a[1] == b[1], "the program commits to another witness than host synthesis"
    for _ in range(proofs):
        host_part(host)
        program_part(prog)
    col = lambda ts, i: [t[i] for t in ts]
    print(f"  before the prover, host:    synthesis {fmt(col(host, 0))} + pack_cells {fmt(col(host, 1))} + advice call {fmt(col(host, 2))} = {fmt(col(host, 3))} ms")
    print(f"  before the prover, program: run + read {fmt(col(prog, 0))} + pack_cells {fmt(col(prog, 1))} + advice call {fmt(col(prog, 2))} = {fmt(col(prog, 3))} ms"
          f"   x{statistics.median(col(prog, 3)) / statistics.median(col(host, 3)):.4f} of host")
    whole = {"host": [], "program": []}
    for rnd in range(proofs + 1):
        for name in whole:
            pk.program = program if name == "program" else None
            t0 = time.perf_counter()
            public = scaffold.prove_private(range_closure, xs, pk, break_points)
            if rnd:
                whole[name].append((time.perf_counter() - t0) * 1e3)
            assert public == a[1]
    print(f"  prove_private, host    {fmt(whole['host'])} ms")
    print(f"  prove_private, program {fmt(whole['program'])} ms   x{statistics.median(whole['program']) / statistics.median(whole['host']):.4f} of host")
    plan = witness.segmentation(sizes)
    got = launches(lib, lambda: dev.run(flat))
    assert [g[0] for g in got] == ["k_witness_level" if p[0] == "grid" else "k_witness_levels_wg" for p in plan] + ["k_witness_place"]
    grid = sorted(((sizes[p[1]], p[1], ms) for p, (_, ms) in zip(plan, got) if p[0] == "grid"), reverse=True)
    for ops, level, ms in grid[:4]:
        nbytes = level_bytes(program, level)
        print(f"  k_witness_level, level {level}: {ops} ops, {nbytes / 1e6:.2f} MB in {ms:.4f} ms = {nbytes / (ms * 1e-3) / HBM * 100:.1f}% of the HBM roofline")
    wg = [(p[2] - p[1], ms) for p, (_, ms) in zip(plan, got) if p[0] == "wg"]
    print(f"  k_witness_level x{len(grid)}: {sum(g[2] for g in grid):.4f} ms; k_witness_levels_wg x{len(wg)} ({sum(w[0] for w in wg)} levels): {sum(w[1] for w in wg):.4f} ms; "
          f"k_witness_place ({sum(len(p) for p in program.placement)} cells, {len(program.checks)} checks): {got[-1][1]:.4f} ms")
    pk.program = program
    pk.release()


def threshold(h2, levels):
    """levels of exactly W ops (copies and 64-bit limbs of the level below by turns): up to 1024 all levels run inside one workgroup
    launch, above it every level is a grid launch"""
    from halo2_scaffold_amd import witness
    from halo2_scaffold_amd._lib import lib

    print(f"the narrow / wide threshold: {levels} levels of W ops each (copies and 64-bit limbs by turns), device time per level")
    for W in (64, 256, 512, 1024, 1025, 2048, 4096, 16384):
        rows = [(j, witness.INPUT, j % 7, 0) for j in range(W)]
        ends = [W]
        for l in range(1, levels + 1):
            for i in range(W):
                src = (l - 1) * W + (5 * i + l) % W
                rows.append((l * W + i, witness.LIMB | 64 << 8 if i % 2 else witness.COPY, src, 0))
            ends.append(len(rows))
        program = witness.Program(rows, ends, [], 7, [], [], [])
        dev = program.on_device()
        flat = list(range(1, 8))
        dev.run(flat)
        got = [g for g in launches(lib, lambda: dev.run(flat)) if g[0] != "k_witness_place"]
        ms = sum(t for _, t in got)
        print(f"  W = {W:5d}: {len(got)} launches of {sorted({name for name, _ in got})}: {ms:.4f} ms, {ms / (levels + 1) * 1e3:.2f} us per level")
        program.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=22)
    ap.add_argument("--lookup-bits", type=int, default=16)
    ap.add_argument("--wide-k", type=int, default=16)
    ap.add_argument("--wide-bits", type=int, default=12)
    ap.add_argument("--wide-count", type=int, default=20000)
    ap.add_argument("--proofs", type=int, default=5)
    ap.add_argument("--levels", type=int, default=200)
    a = ap.parse_args()
    import torch  # noqa: F401  (first, so the library shares torch's HIP runtime)

    import _load_pkg

    h2 = _load_pkg.load()
    h2.init(0)
    from halo2_scaffold_amd import flex

    print(f"witness_program_cost: {torch.cuda.get_device_name(0)}; {a.proofs} alternating rounds after one warm-up round; times in ms, median (min .. max)")
    circuit(h2, f"range x {a.wide_count}, LOOKUP_BITS {a.wide_bits}, DEGREE {a.wide_k} (11 gate + 8 lookup-advice columns):", a.wide_k, a.wide_bits,
            flex.FlexGateCS(True, 11, 8, k=a.wide_k), [(X + i * STEP) & ((1 << 64) - 1) for i in range(a.wide_count)], a.proofs)
    circuit(h2, f"range, LOOKUP_BITS {a.lookup_bits}, DEGREE {a.k} (one gate column, q_lookup * a):", a.k, a.lookup_bits, flex.FlexGateCS(lookup=True), [X],
            a.proofs)
    threshold(h2, a.levels)


if __name__ == "__main__":
    main()
