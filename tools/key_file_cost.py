#!/usr/bin/env python3
"""What a proving-key file costs and saves: for StandardPlonk at --k-plonk and the range builder at --k-range with
--lookup-bits (the BASELINE shapes), in ONE run per shape —

  * the blob's bytes beside 32 * 2^k * (n_fixed + n_perm), what the fixed and sigma columns take as 32-byte words;
  * export: h2mi_prover_pk_export, the length call and the call that writes, host clock;
  * import (engine.Keys.from_blob: blob check + h2mi_prover_pk_import) beside keygen from the caller's cells (engine.Keys: packing the
    cells + h2mi_prover_keygen), the two ALTERNATING, --runs each after one of each; median (min .. max); a proof against the imported
    key is compared byte for byte with one against the generated key before anything is timed;
  * the compaction kernels from the library's launch profile during one export: k_cells_count reads 32 bytes of every usable row of every
    fixed column, so its time gives a share of the 8 TB/s HBM roofline DESIGN.md uses; k_cells_compact reads only the tiles that hold
    cells, its time is reported as it is;
  * range only: scaffold.gen_key wall clock without a key file, writing one, and reading it (SRS read from PARAMS_DIR in all three).

    python tools/key_file_cost.py [--only plonk range] [--out profiles/key_file_cost.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRS_SECRET = 0x5EC2E7 + 0x48324D49
HBM_BYTES_PER_S = 8e12


def fmt(ts):
    return f"{statistics.median(ts):.2f} ({min(ts):.2f} .. {max(ts):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="+", choices=["plonk", "range"], default=["plonk", "range"])
    ap.add_argument("--k-plonk", type=int, default=20)
    ap.add_argument("--k-range", type=int, default=22)
    ap.add_argument("--lookup-bits", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_file_cost.txt"))
    args = ap.parse_args()
    import torch  # noqa: F401

    import _load_pkg

    h2 = _load_pkg.load()
    from halo2_scaffold_amd import circuits, engine, flex, keygen, prover, scaffold
    from halo2_scaffold_amd._lib import check, lib
    from halo2_scaffold_amd.params import ParamsKZG

    h2.init(0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def clock(call):
        check(lib.h2mi_sync(), "sync")
        t0 = time.perf_counter()
        out = call()
        check(lib.h2mi_sync(), "sync")
        return 1e3 * (time.perf_counter() - t0), out

    def kernel_ms(call):
        """{kernel: (ms, launches)} of the compaction kernels during call()"""
        assert lib.h2mi_profile_reset() == 0 and lib.h2mi_profile_filter(b"k_cells") == 0 and lib.h2mi_profile_enable(1) == 0
        try:
            call()
        finally:
            assert lib.h2mi_profile_enable(0) == 0
        out = {}
        for name in ("k_cells_count", "k_cells_prefix", "k_cells_compact"):
            ms, count = C.c_double(), C.c_uint64()
            assert lib.h2mi_profile_query(name.encode(), C.byref(ms), C.byref(count)) == 0
            out[name] = (ms.value, count.value)
        assert lib.h2mi_profile_filter(b"") == 0 and lib.h2mi_profile_reset() == 0
        return out

    def measure(title, k, params, abi, fixed, copies, prove):
        """abi / fixed / copies: what engine.Keys takes; prove(engine.Keys) -> proof bytes"""
        make = lambda: engine.Keys(abi, params, fixed, copies)
        keys = make()
        proof = prove(keys)
        blob = keys.export()
        loaded = engine.Keys.from_blob(params, blob)
        assert prove(loaded) == proof, f"{title}: the proof against the imported key differs"
        assert loaded.export() == blob
        loaded.release()
        dense = 32 * (1 << k) * (abi.n_fixed + abi.n_perm)
        say(f"{title}: blob {len(blob)} bytes, the fixed and sigma columns as words {dense} bytes: x {len(blob) / dense:.3g}; proof bytes equal ({len(proof)} bytes)")
        t_len, t_all = [], []
        for _ in range(args.runs):
            n = C.c_size_t()
            t_len.append(clock(lambda: check(lib.h2mi_prover_pk_export(keys.handle, None, 0, None, 0, C.byref(n)), "export"))[0])
            t_all.append(clock(keys.export)[0])
        say(f"  export ms: the length call {fmt(t_len)}, Keys.export (length call + writing call) {fmt(t_all)}")
        prof = kernel_ms(keys.export)
        usable = (1 << k) - abi.blinding_factors - 1
        read = 32 * usable * abi.n_fixed
        ms_count, n_count = prof["k_cells_count"]
        ms_compact, n_compact = prof["k_cells_compact"]
        per = ms_count / max(n_count, 1)
        say(f"  k_cells_count: {per:.4f} ms per launch over {abi.n_fixed} columns of {usable} rows = {read / (per * 1e-3) / 1e12:.2f} TB/s read, "
            f"{100 * read / (per * 1e-3) / HBM_BYTES_PER_S:.1f} % of the 8 TB/s roofline ({n_count} launches in one Keys.export); "
            f"k_cells_prefix {prof['k_cells_prefix'][0] / max(prof['k_cells_prefix'][1], 1):.4f} ms; k_cells_compact {ms_compact / max(n_compact, 1):.4f} ms "
            f"(reads only the tiles that hold cells)")
        keys.release()
        t_make, t_load = [], []
        for _ in range(args.runs):
            ms, made = clock(make)
            made.release()
            t_make.append(ms)
            ms, got = clock(lambda: engine.Keys.from_blob(params, blob))
            got.release()
            t_load.append(ms)
        say(f"  keygen from the caller's cells ms {fmt(t_make)}; import ms {fmt(t_load)}; import / keygen {statistics.median(t_load) / statistics.median(t_make):.3f}")

    if "plonk" in args.only:
        k = args.k_plonk
        params = ParamsKZG.setup(k, SRS_SECRET)
        circuit = circuits.StandardPlonk(None)
        syn = circuit.without_witnesses().synthesize()
        copies = [(lc, lr, rc, rr) for (lc, lr), (rc, rr) in syn.copies]
        vk = keygen.keygen_vk(params, circuit)

        def prove(keys):
            pk = keygen.ProvingKey(vk, circuit, keys)
            return prover.create_proof(params, pk, circuits.StandardPlonk(0xC0FFEE), 7)

        measure(f"StandardPlonk, DEGREE {k}", k, params, keygen.constraint_system(circuit, k), syn.fixed, copies, prove)
        params.release()
    if "range" in args.only:
        k, bits = args.k_range, args.lookup_bits
        params = ParamsKZG.setup(k, SRS_SECRET)
        cs = flex.FlexGateCS(lookup=True)
        asg = flex.range_closure(cs, 0x0123456789ABCDEF, bits)
        fixed = list(asg.fixed)  # the cells and copies as flex.FlexKeys hands them over: the table column dense
        fixed[cs.col_table] = [int(v) for v in asg.table_values]
        index = {col: j for j, col in enumerate(cs.perm_columns)}
        copies = [(index[(left[0], left[1])], left[2], index[(right[0], right[1])], right[2]) for left, right in asg.copies]

        def prove(keys):
            fk = flex.FlexKeys.__new__(flex.FlexKeys)
            fk.cs, fk.by_coset, fk.keys = cs, False, keys
            fk._finish(k)
            return flex.create_proof(params, fk, asg, 31337)

        measure(f"range builder, DEGREE {k}, LOOKUP_BITS {bits}", k, params, cs.abi(k), fixed, copies, prove)
        params.release()

        # scaffold.gen_key: the closure of examples/range.rs
        def range_example(ctx, x, make_public):
            xc = ctx.load_witness(x)
            make_public.append(xc)
            ctx.range_check(xc, 64, ctx.lookup_bits)
            ctx.add(xc, xc)

        with tempfile.TemporaryDirectory() as tmp:
            os.environ.update(DEGREE=str(k), LOOKUP_BITS=str(bits), PARAMS_DIR=tmp)
            pk, _ = scaffold.gen_key(range_example, 0)  # writes the SRS file: not what is compared
            pk.release()
            path = os.path.join(tmp, "range.key")
            rows = []
            for what, kw in (("without a key file", {}), ("writing the key file", {"key_file": path}), ("reading the key file", {"key_file": path})):
                t0 = time.perf_counter()
                pk, bp = scaffold.gen_key(range_example, 0, **kw)
                check(lib.h2mi_sync(), "sync")
                rows.append((what, time.perf_counter() - t0))
                pk.release()
            say(f"  scaffold.gen_key, DEGREE {k}, LOOKUP_BITS {bits}, wall clock s: " + "; ".join(f"{w} {t:.2f}" for w, t in rows) +
                f"; reading / without {rows[2][1] / rows[0][1]:.3f} (key file {os.path.getsize(path)} bytes)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
