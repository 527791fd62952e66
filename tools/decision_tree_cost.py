#!/usr/bin/env python3
"""What the witness program of one decision-tree training proof (decision_tree.train on the reference's examples/decision_tree.rs sizes:
10 samples x 2 features, 2 classes, max_depth 4, min_size 1, PRECISION_BITS 63, DEGREE --k, LOOKUP_BITS --lookup-bits; the key from its
dummy set, the proofs of its data set) costs against host synthesis, every ratio inside ONE run.  If the circuit does not fit the prover
ABI's 32 gate + 8 lookup-advice columns at --k, that is printed and the smallest DEGREE that holds it is taken.  Alternating rounds after
one warm-up round, host-inclusive wall clock, median (min .. max) in ms:

  * the witness part: host synthesis (the closure through flex.Context, finish) + engine.pack_cells + h2mi_prover_advice, against the
    program's run + the public cells read back + pack_cells + h2mi_prover_advice — the commitments of both compared first;
  * the whole scaffold.prove_private, the closure called against the program run;
  * the tape's facts: cells, auxiliary cells, hint ops by kind, levels, launches, columns, device bytes, recording time;
  * the program's launches from the library's profile: the device time of all level launches, of the levels that hold an INV and of the
    levels that hold a DIVQ / DIVR, and per launch form the share of the lanes that are INV or DIV ops — every wavefront of a level that
    mixes them with cheap lanes pays for the inversion or the division.

    python tools/decision_tree_cost.py > profiles/decision_tree_cost.txt"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
SRS_SECRET = 0x48911030
HBM = 8e12

X = [[2.771244718, 1.784783929], [1.0, 1.0], [3.0, 2.0], [3.0, 2.0], [2.0, 2.0], [7.0, 3.0], [9.00220326, 3.339047188], [7.444542326, 0.476683375],
     [10.12493903, 3.234550982], [6.642287351, 3.319983761]]
Y = [1, 0, 0, 1, 0, 1, 1, 0, 1, 1]
X_DUMMY = [[2.771244718, 1.784783929], [1.728571309, 1.169761413], [3.678319846, 2.81281357], [3.961043357, 2.61995032], [2.999208922, 2.209014212],
           [7.497545867, 3.162953546], [9.00220326, 3.339047188], [7.444542326, 0.476683375], [10.12493903, 3.234550982], [6.642287351, 3.319983761]]
Y_DUMMY = [0, 0, 0, 0, 0, 1, 1, 1, 1, 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--lookup-bits", type=int, default=None, help="default: DEGREE - 1")
    ap.add_argument("--proofs", type=int, default=5)
    a = ap.parse_args()
    import torch  # noqa: F401  (first, so the library shares torch's HIP runtime)

    import _load_pkg

    h2 = _load_pkg.load()
    h2.init(0)
    from fixed_point_cost import fmt, level_bytes
    from witness_program_cost import launches

    from halo2_scaffold_amd import decision_tree as DT
    from halo2_scaffold_amd import engine, flex, scaffold, witness
    from halo2_scaffold_amd._lib import lib
    from halo2_scaffold_amd.fixed_point import FixedPointChip

    chip = FixedPointChip(DT.PRECISION_BITS)
    inputs, dummy = DT.quantize_dataset(chip, X, Y), DT.quantize_dataset(chip, X_DUMMY, Y_DUMMY)
    k = a.k
    while True:
        lookup_bits = a.lookup_bits if a.lookup_bits is not None and k == a.k else k - 1
        t0 = time.perf_counter()
        try:
            cs = scaffold._config(DT.train, dummy, k, lookup_bits, 9)
            break
        except AssertionError as e:
            print(f"decision_tree_cost: the circuit does not fit DEGREE {k} / LOOKUP_BITS {lookup_bits} ({e}); trying DEGREE {k + 1}")
            k += 1
    os.environ["DEGREE"], os.environ["LOOKUP_BITS"] = str(k), str(lookup_bits)
    print(f"decision_tree_cost: {torch.cuda.get_device_name(0)}; one proof of a training on {len(Y)} samples x {DT.num_feature} features, {DT.num_class} classes, "
          f"max_depth {DT.max_depth}, min_size {DT.min_size}, P = {DT.PRECISION_BITS}, DEGREE {k}, LOOKUP_BITS {lookup_bits}; {a.proofs} alternating rounds after one "
          f"warm-up round; times in ms, median (min .. max)")
    program, recorded = witness.Program.record(DT.train, dummy, cs, lookup_bits)
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
    plan = witness.segmentation(sizes)
    print(f"  {program.n_cells - program.n_aux} cells in {cs.num_advice} gate + {cs.num_lookup_advice} lookup-advice columns ({len(recorded.fixed[cs.col_consts[0]])} "
          f"constants), {program.n_aux} auxiliary cells, {int((kinds >= 8).sum())} hint ops ({count(8)} DIVQ, {count(9)} DIVR, {count(10)} ISZERO, {count(11)} INV, "
          f"{count(13)} MSB, {count(14)} POW2), {count(2)} COPY ops, {len(sizes)} levels (narrowest {min(sizes)}, widest {max(sizes)}, "
          f"{sum(1 for s in sizes if s <= witness.WG_OPS)} of at most {witness.WG_OPS} ops), {len(program.checks)} checks; configured and recorded in {t_record:.2f} s, "
          f"SRS and key in {t_key:.2f} s; {info.n_grid_launches} grid + {info.n_wg_launches} workgroup launches + 1; {info.device_bytes / 2**20:.1f} MiB on the device")
    prover = pk.workspace.prover
    pts = prover._points.ctypes.data
    flat = witness.flatten_inputs(inputs)

    def part(times, host):
        t0 = time.perf_counter()
        if host:
            asg = scaffold._synthesize(DT.train, inputs, cs, lookup_bits)
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
    print("  tree:", [[int(v) if i != 1 else round(v, 9) for i, v in enumerate(node)] for node in DT.nodes(chip, h[1])])
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
            public = scaffold.prove_private(DT.train, inputs, pk, break_points)
            if rnd:
                whole[name].append((time.perf_counter() - t0) * 1e3)
            assert public == h[1]
    print(f"  prove_private, host    {fmt(whole['host'])} ms")
    print(f"  prove_private, program {fmt(whole['program'])} ms   x{statistics.median(whole['program']) / statistics.median(whole['host']):.4f} of host")
    got = launches(lib, lambda: dev.run(flat))
    assert [g[0] for g in got] == ["k_witness_level_hints" if s[0] == "grid" else "k_witness_levels_wg_hints" for s in plan] + ["k_witness_place"]
    ends = [0] + [int(e) for e in program.level_ends]
    lanes = lambda first, end, which: int(sum((kinds[ends[first]:ends[end]] == kind).sum() for kind in which))
    INV, DIV = (11,), (8, 9)
    rows = [(s[0], s[1], s[1] + 1 if s[0] == "grid" else s[2], ms) for s, (_, ms) in zip(plan, got)]  # (form, first level, end level, ms)
    total = sum(r[3] for r in rows)
    for form, name in (("grid", "k_witness_level_hints"), ("wg", "k_witness_levels_wg_hints")):
        mine = [r for r in rows if r[0] == form]
        ops = sum(ends[r[2]] - ends[r[1]] for r in mine)
        with_inv = [r for r in mine if lanes(r[1], r[2], INV)]
        with_div = [r for r in mine if lanes(r[1], r[2], DIV)]
        print(f"  {name} x{len(mine)} ({sum(r[2] - r[1] for r in mine)} levels, {ops} ops): {sum(r[3] for r in mine):.4f} ms; {len(with_inv)} launches hold an INV: "
              f"{sum(r[3] for r in with_inv):.4f} ms, {sum(lanes(r[1], r[2], INV) for r in with_inv) / max(1, sum(ends[r[2]] - ends[r[1]] for r in with_inv)) * 100:.2f}% "
              f"of their lanes INV; {len(with_div)} hold a DIVQ / DIVR: {sum(r[3] for r in with_div):.4f} ms, "
              f"{sum(lanes(r[1], r[2], DIV) for r in with_div) / max(1, sum(ends[r[2]] - ends[r[1]] for r in with_div)) * 100:.2f}% of their lanes DIV")
    inv_ms = sum(r[3] for r in rows if lanes(r[1], r[2], INV))
    div_ms = sum(r[3] for r in rows if lanes(r[1], r[2], DIV))
    either = sum(r[3] for r in rows if lanes(r[1], r[2], INV + DIV))
    print(f"  all {len(rows)} level launches: {total:.4f} ms; the launches that hold an INV {inv_ms:.4f} ms ({inv_ms / total * 100:.1f}%), a DIVQ / DIVR {div_ms:.4f} ms "
          f"({div_ms / total * 100:.1f}%), either {either:.4f} ms ({either / total * 100:.1f}%); k_witness_place ({sum(len(q) for q in program.placement)} cells, "
          f"{len(program.checks)} checks): {got[-1][1]:.4f} ms")
    grid = sorted(((level_bytes(program, r[1])[1], r) for r in rows if r[0] == "grid"), reverse=True)
    for hints, (_, level, _, ms) in grid[:3]:
        nbytes = level_bytes(program, level)[0]
        print(f"  k_witness_level_hints, level {level}: {sizes[level]} ops, {hints} of them hints ({lanes(level, level + 1, INV) / sizes[level] * 100:.1f}% of the lanes INV, "
              f"{lanes(level, level + 1, DIV) / sizes[level] * 100:.1f}% DIV), {nbytes / 1e6:.3f} MB in {ms:.4f} ms = {nbytes / (ms * 1e-3) / HBM * 100:.2f}% of the HBM roofline")
    pk.program = program
    pk.release()


if __name__ == "__main__":
    main()
