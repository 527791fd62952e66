#!/usr/bin/env python3
"""What the witness program of one linear-regression training step (linear_regression.train: --samples samples x --features features,
DEGREE --k, LOOKUP_BITS --lookup-bits, PRECISION_BITS 32 — the reference's examples/linear_regression.rs is 32 x 10 at 16 / 15) costs
against host synthesis, every ratio inside ONE run.  Alternating rounds after one warm-up round, host-inclusive wall clock, median
(min .. max) in ms:

  * the witness part: host synthesis (the closure through flex.Context, finish) + engine.pack_cells + h2mi_prover_advice, against the
    program's run + the public cells read back + pack_cells + h2mi_prover_advice — the commitments of both compared first;
  * the whole scaffold.prove_private, the closure called against the program run;
  * the program's launches from the library's profile, the widest level that holds a hint op against its algorithmic bytes
    (16 for the op + 32 per operand + 32 for the store, per op) as a share of the HBM roofline (8 TB/s).

    python tools/fixed_point_cost.py --proofs 5 > profiles/fixed_point_cost.txt"""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
SRS_SECRET = 0x48911030
HBM = 8e12


def fmt(ts):
    return f"{statistics.median(ts):.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def level_bytes(program, level):
    """the algorithmic bytes of one level, and how many of its ops are hints"""
    ends = [0] + [int(e) for e in program.level_ends]
    total = hints = 0
    for code, in program.ops[ends[level]:ends[level + 1], 1:2].tolist():
        kind = code & 0xFF
        operands = 3 if kind == 3 else 2 if kind in (8, 9) else 1
        total += 16 + 32 * operands + 32
        hints += kind >= 8
    return total, hints


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--lookup-bits", type=int, default=15)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--features", type=int, default=10)
    ap.add_argument("--proofs", type=int, default=5)
    a = ap.parse_args()
    import torch  # noqa: F401  (first, so the library shares torch's HIP runtime)

    import _load_pkg

    h2 = _load_pkg.load()
    h2.init(0)
    from witness_program_cost import launches

    from halo2_scaffold_amd import engine, flex, scaffold, witness
    from halo2_scaffold_amd import linear_regression as LR
    from halo2_scaffold_amd._lib import lib
    from halo2_scaffold_amd.fixed_point import FixedPointChip

    k, lookup_bits = a.k, a.lookup_bits
    os.environ["DEGREE"], os.environ["LOOKUP_BITS"] = str(k), str(lookup_bits)
    chip = FixedPointChip(32, lookup_bits)
    rng = random.Random("fixed point cost")
    x = [[rng.uniform(-0.15, 0.15) for _ in range(a.features)] for _ in range(a.samples)]
    y = [rng.uniform(25.0, 350.0) for _ in range(a.samples)]
    inputs = LR.quantize_batch(chip, [rng.uniform(-1.0, 1.0) for _ in range(a.features)], 0.5, x, y, 0.01)
    dummy = LR.quantize_batch(chip, [0.0] * a.features, 0.0, [[0.0] * a.features] * a.samples, [0.0] * a.samples, 0.01)
    print(f"fixed_point_cost: {torch.cuda.get_device_name(0)}; one training step of {a.samples} samples x {a.features} features, DEGREE {k}, LOOKUP_BITS "
          f"{lookup_bits}; {a.proofs} alternating rounds after one warm-up round; times in ms, median (min .. max)")
    cs = scaffold._config(LR.train, dummy, k, lookup_bits, 9)
    t0 = time.perf_counter()
    program, recorded = witness.Program.record(LR.train, dummy, cs, lookup_bits)
    t_record = time.perf_counter() - t0
    params = h2.ParamsKZG.setup(k, SRS_SECRET)
    pk = scaffold.ProvingKey(params, flex.FlexKeys(params, cs, recorded))
    pk.lookup_bits = lookup_bits
    break_points = [list(recorded.break_points)]
    dev = program.on_device()
    info = dev.info
    sizes = program.level_sizes
    kinds = program.ops[:, 1] & 0xFF
    print(f"  {program.n_cells - program.n_aux} cells in {cs.num_advice} gate + {cs.num_lookup_advice} lookup-advice columns, {program.n_aux} auxiliary cells, "
          f"{int((kinds >= 8).sum())} hint ops ({int((kinds == 8).sum())} DIVQ, {int((kinds == 9).sum())} DIVR, {int((kinds == 10).sum())} ISZERO, "
          f"{int((kinds == 11).sum())} INV), {len(sizes)} levels (widest {max(sizes)}), {len(program.checks)} checks; recorded in {t_record:.2f} s; "
          f"{info.n_grid_launches} grid + {info.n_wg_launches} workgroup launches + 1; {info.device_bytes / 2**20:.1f} MiB on the device")
    prover = pk.workspace.prover
    pts = prover._points.ctypes.data
    flat = witness.flatten_inputs(inputs)

    def part(times, host):
        t0 = time.perf_counter()
        if host:
            asg = scaffold._synthesize(LR.train, inputs, cs, lookup_bits)
            columns, instance = asg.advice, asg.instance
        else:
            columns = dev.run(flat)
            instance = dev.read(program.public)
        t1 = time.perf_counter()
        cells, keep = engine.pack_cells(columns)
        inst, n_inst = prover._public_inputs(instance)
        engine.check(lib.h2mi_prover_advice(prover.handle, cells, inst.ctypes.data, n_inst, 5, pts), "advice")
        lib.h2mi_sync()
        t2 = time.perf_counter()
        times.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3))
        return prover._points[:prover.counts.advice].copy(), instance

    host, prog = [], []
    h, p = part([], True), part([], False)
    assert (h[0] == p[0]).all() and h[1] == p[1], "the program commits to another witness than host synthesis"
    for _ in range(a.proofs):
        part(host, True)
        part(prog, False)
    col = lambda ts, i: [t[i] for t in ts]
    print(f"  witness part, host:    synthesis {fmt(col(host, 0))} + pack_cells and advice call {fmt(col(host, 1))} = {fmt(col(host, 2))} ms")
    print(f"  witness part, program: run + read {fmt(col(prog, 0))} + pack_cells and advice call {fmt(col(prog, 1))} = {fmt(col(prog, 2))} ms"
          f"   x{statistics.median(col(prog, 2)) / statistics.median(col(host, 2)):.4f} of host")
    whole = {"host": [], "program": []}
    for rnd in range(a.proofs + 1):
        for name in whole:
            pk.program = program if name == "program" else None
            t0 = time.perf_counter()
            public = scaffold.prove_private(LR.train, inputs, pk, break_points)
            if rnd:
                whole[name].append((time.perf_counter() - t0) * 1e3)
            assert public == h[1]
    print(f"  prove_private, host    {fmt(whole['host'])} ms")
    print(f"  prove_private, program {fmt(whole['program'])} ms   x{statistics.median(whole['program']) / statistics.median(whole['host']):.4f} of host")
    plan = witness.segmentation(sizes)
    got = launches(lib, lambda: dev.run(flat))
    assert [g[0] for g in got] == ["k_witness_level_hints" if s[0] == "grid" else "k_witness_levels_wg_hints" for s in plan] + ["k_witness_place"]
    grid = sorted(((level_bytes(program, s[1])[1], sizes[s[1]], s[1], ms) for s, (_, ms) in zip(plan, got) if s[0] == "grid"), reverse=True)
    for hints, ops, level, ms in grid[:3]:
        nbytes = level_bytes(program, level)[0]
        print(f"  k_witness_level_hints, level {level}: {ops} ops, {hints} of them hints, {nbytes / 1e6:.3f} MB in {ms:.4f} ms = "
              f"{nbytes / (ms * 1e-3) / HBM * 100:.2f}% of the HBM roofline")
    wg = [(s[2] - s[1], ms) for s, (_, ms) in zip(plan, got) if s[0] == "wg"]
    print(f"  k_witness_level_hints x{len(grid)}: {sum(g[3] for g in grid):.4f} ms; k_witness_levels_wg_hints x{len(wg)} ({sum(w[0] for w in wg)} levels): "
          f"{sum(w[1] for w in wg):.4f} ms; k_witness_place ({sum(len(q) for q in program.placement)} cells, {len(program.checks)} checks): {got[-1][1]:.4f} ms")
    pk.program = program
    pk.release()


if __name__ == "__main__":
    main()
