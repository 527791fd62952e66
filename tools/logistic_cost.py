#!/usr/bin/env python3
"""What the witness program of one logistic-regression training proof (logistic_regression.train: --batches batches of --samples samples
x --features features, DEGREE --k, LOOKUP_BITS --lookup-bits, PRECISION_BITS 63 — the reference's examples/logistic_regression.rs is
12 x 64 x 11 at 19 / 18) costs against host synthesis, every ratio inside ONE run.  Alternating rounds after one warm-up round,
host-inclusive wall clock, median (min .. max) in ms:

  * the witness part: host synthesis (the closure through flex.Context, finish) + engine.pack_cells + h2mi_prover_advice, against the
    program's run + the public cells read back + pack_cells + h2mi_prover_advice — the commitments of both compared first;
  * the whole scaffold.prove_private, the closure called against the program run;
  * the program's launches from the library's profile, the widest level that holds a hint op against its algorithmic bytes
    (16 for the op + 32 per operand + 32 for the store, per op) as a share of the HBM roofline (8 TB/s), and the share of that level's
    lanes that are INV ops — every wavefront of a level that mixes them with cheap lanes pays for the inversion.

    python tools/logistic_cost.py --proofs 3 > profiles/logistic_cost.txt"""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
SRS_SECRET = 0x48911030
HBM = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=19)
    ap.add_argument("--lookup-bits", type=int, default=18)
    ap.add_argument("--batches", type=int, default=1)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--features", type=int, default=11)
    ap.add_argument("--proofs", type=int, default=3)
    a = ap.parse_args()
    import torch  # noqa: F401  (first, so the library shares torch's HIP runtime)

    import _load_pkg

    h2 = _load_pkg.load()
    h2.init(0)
    from fixed_point_cost import fmt, level_bytes
    from witness_program_cost import launches

    from halo2_scaffold_amd import engine, flex, scaffold, witness
    from halo2_scaffold_amd import logistic_regression as LG
    from halo2_scaffold_amd._lib import lib
    from halo2_scaffold_amd.fixed_point import FixedPointChip

    k, lookup_bits = a.k, a.lookup_bits
    os.environ["DEGREE"], os.environ["LOOKUP_BITS"] = str(k), str(lookup_bits)
    chip = FixedPointChip(63, lookup_bits)
    rng = random.Random("logistic cost")
    batch = lambda draw: [[[draw() for _ in range(a.features)] for _ in range(a.samples)] for _ in range(a.batches)]
    x = batch(lambda: rng.uniform(-1.0, 1.0))
    y = [[float(rng.random() < 0.3) for _ in range(a.samples)] for _ in range(a.batches)]
    inputs = LG.quantize_batches(chip, [rng.uniform(-1.0, 1.0) for _ in range(a.features)], 0.5, x, y, 0.001)
    dummy = LG.quantize_batches(chip, [0.0] * a.features, 0.0, batch(lambda: 0.0), [[0.0] * a.samples] * a.batches, 0.001)
    print(f"logistic_cost: {torch.cuda.get_device_name(0)}; one proof of {a.batches} training batch(es) of {a.samples} samples x {a.features} features, "
          f"P = 63, DEGREE {k}, LOOKUP_BITS {lookup_bits}; {a.proofs} alternating rounds after one warm-up round; times in ms, median (min .. max)")
    t0 = time.perf_counter()
    cs = scaffold._config(LG.train, dummy, k, lookup_bits, 9)
    program, recorded = witness.Program.record(LG.train, dummy, cs, lookup_bits)
    t_record = time.perf_counter() - t0
    t0 = time.perf_counter()
    params = h2.ParamsKZG.setup(k, SRS_SECRET)
    pk = scaffold.ProvingKey(params, flex.FlexKeys(params, cs, recorded))
    t_key = time.perf_counter() - t0
    pk.lookup_bits = lookup_bits
    break_points = [list(recorded.break_points)]
    dev = program.on_device()
    info = dev.info
    sizes = program.level_sizes
    kinds = program.ops[:, 1] & 0xFF
    count = lambda kind: int((kinds == kind).sum())
    print(f"  {program.n_cells - program.n_aux} cells in {cs.num_advice} gate + {cs.num_lookup_advice} lookup-advice columns, {program.n_aux} auxiliary cells, "
          f"{int((kinds >= 8).sum())} hint ops ({count(8)} DIVQ, {count(9)} DIVR, {count(10)} ISZERO, {count(11)} INV, {count(13)} MSB, {count(14)} POW2), "
          f"{len(sizes)} levels (widest {max(sizes)}), {len(program.checks)} checks; configured and recorded in {t_record:.2f} s, SRS and key in {t_key:.2f} s; "
          f"{info.n_grid_launches} grid + {info.n_wg_launches} workgroup launches + 1; {info.device_bytes / 2**20:.1f} MiB on the device")
    prover = pk.workspace.prover
    pts = prover._points.ctypes.data
    flat = witness.flatten_inputs(inputs)

    def part(times, host):
        t0 = time.perf_counter()
        if host:
            asg = scaffold._synthesize(LG.train, inputs, cs, lookup_bits)
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
    import statistics

    col = lambda ts, i: [t[i] for t in ts]
    print(f"  witness part, host:    synthesis {fmt(col(host, 0))} + pack_cells and advice call {fmt(col(host, 1))} = {fmt(col(host, 2))} ms")
    print(f"  witness part, program: run + read {fmt(col(prog, 0))} + pack_cells and advice call {fmt(col(prog, 1))} = {fmt(col(prog, 2))} ms"
          f"   x{statistics.median(col(prog, 2)) / statistics.median(col(host, 2)):.4f} of host")
    whole = {"host": [], "program": []}
    for rnd in range(a.proofs + 1):
        for name in whole:
            pk.program = program if name == "program" else None
            t0 = time.perf_counter()
            public = scaffold.prove_private(LG.train, inputs, pk, break_points)
            if rnd:
                whole[name].append((time.perf_counter() - t0) * 1e3)
            assert public == h[1]
    print(f"  prove_private, host    {fmt(whole['host'])} ms")
    print(f"  prove_private, program {fmt(whole['program'])} ms   x{statistics.median(whole['program']) / statistics.median(whole['host']):.4f} of host")
    plan = witness.segmentation(sizes)
    got = launches(lib, lambda: dev.run(flat))
    assert [g[0] for g in got] == ["k_witness_level_hints" if s[0] == "grid" else "k_witness_levels_wg_hints" for s in plan] + ["k_witness_place"]
    ends = [0] + [int(e) for e in program.level_ends]
    inv_share = lambda level: int((kinds[ends[level]:ends[level + 1]] == 11).sum()) / sizes[level]
    grid = sorted(((level_bytes(program, s[1])[1], sizes[s[1]], s[1], ms) for s, (_, ms) in zip(plan, got) if s[0] == "grid"), reverse=True)
    for hints, ops, level, ms in grid[:3]:
        nbytes = level_bytes(program, level)[0]
        print(f"  k_witness_level_hints, level {level}: {ops} ops, {hints} of them hints ({inv_share(level) * 100:.1f}% of the lanes INV), {nbytes / 1e6:.3f} MB in "
              f"{ms:.4f} ms = {nbytes / (ms * 1e-3) / HBM * 100:.2f}% of the HBM roofline")
    wg = [(s[2] - s[1], ms) for s, (_, ms) in zip(plan, got) if s[0] == "wg"]
    with_inv = [g for g in grid if inv_share(g[2]) > 0]
    print(f"  k_witness_level_hints x{len(grid)}: {sum(g[3] for g in grid):.4f} ms, {sum(g[3] for g in with_inv):.4f} ms of it in the {len(with_inv)} levels that hold an INV; "
          f"k_witness_levels_wg_hints x{len(wg)} ({sum(w[0] for w in wg)} levels): {sum(w[1] for w in wg):.4f} ms; "
          f"k_witness_place ({sum(len(q) for q in program.placement)} cells, {len(program.checks)} checks): {got[-1][1]:.4f} ms")
    pk.program = program
    pk.release()


if __name__ == "__main__":
    main()
