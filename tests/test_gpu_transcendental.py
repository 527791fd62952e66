"""The MSB / POW2 hint ops and the transcendental circuits on the device: the two ops word for word against the plain-integer references
of tests/transcendental_cases.py (the cells read back canonical and as the Montgomery words of a column that holds every cell), the
launches against h2mi_witness_info and the segmentation rule — of the new ops, of the old four hints and of no hint at all —, and the
logistic-regression and qlog / qsin / qpow closures proven through gen_key(witness_program=True) / prove_private byte for byte against
host synthesis with the same key, seed and rng key."""
import ctypes as C

import numpy as np
import pytest

import fixed_point_cases as FC
import transcendental_cases as TC
import witness_cases as W
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

R = o.R
KERNELS = ("k_witness_level", "k_witness_level_hints", "k_witness_levels_wg", "k_witness_levels_wg_hints", "k_witness_place")


def _profiled(gpu, call) -> dict:
    """launches of each witness kernel during call(), from the library's launch profile (its queries match by prefix)"""
    lib = gpu.lib
    assert lib.h2mi_profile_reset() == 0 and lib.h2mi_profile_filter(b"k_witness") == 0 and lib.h2mi_profile_enable(1) == 0
    try:
        call()
    finally:
        assert lib.h2mi_profile_enable(0) == 0
    out = {}
    for name in KERNELS:
        ms, count = C.c_double(), C.c_uint64()
        assert lib.h2mi_profile_query(name.encode(), C.byref(ms), C.byref(count)) == 0
        out[name] = count.value
    out["k_witness_levels_wg"] -= out["k_witness_levels_wg_hints"]
    out["k_witness_level"] -= out["k_witness_levels_wg"] + out["k_witness_levels_wg_hints"] + out["k_witness_level_hints"]
    assert lib.h2mi_profile_reset() == 0 and lib.h2mi_profile_filter(b"") == 0
    return out


def _run_whole(gpu, program, inputs, want, hints: bool):
    """run a program whose one column holds every cell: the canonical values read back and the column's Montgomery words against `want`;
    the launches of the run — of the _hints kernels for a program that holds a hint op, of the plain ones otherwise — against
    h2mi_witness_info and the segmentation rule"""
    from halo2_scaffold_amd import engine, witness

    dev = program.on_device()
    out = {}
    launches = _profiled(gpu, lambda: out.update(columns=dev.run(witness.flatten_inputs(inputs))))
    info = dev.info
    grid, wg = W.segmentation(program.level_sizes)
    assert (info.n_cells, info.n_levels, info.n_grid_launches, info.n_wg_launches) == (program.n_cells, len(program.level_sizes), grid, wg)
    ran = {"k_witness_level" + ("_hints" if hints else ""): grid, "k_witness_levels_wg" + ("_hints" if hints else ""): wg, "k_witness_place": 1}
    assert launches == {name: ran.get(name, 0) for name in KERNELS}
    n = program.n_cells
    got = dev.read(list(range(n)))
    wrong = [i for i in range(n) if got[i] != want[i]]
    assert not wrong, (len(wrong), wrong[:5], [hex(got[i]) for i in wrong[:3]], [hex(want[i]) for i in wrong[:3]])
    (column,) = out["columns"]
    assert len(column) == n
    words = engine.DevView(column.values_ptr, n).to_numpy(shape=(n, 4))
    assert np.array_equal(words, o.pack(want, R))
    program.release()


@pytest.mark.parametrize("reverse", [False, True])
def test_msb_and_pow2_of_every_operand(gpu, reverse):
    """MSB and the flagged POW2 of 0 .. 3, 2^k - 1, 2^k, 2^k + 1 at the word boundaries and r - 1; POW2 of every exponent 0 .. 255, of
    256, 2^32 - 1, 2^32, 2^64 and r - 1; operands from INPUT, CONST and GATE cells.  One workgroup launch; reverse: the ops of every
    level stored in descending dst order"""
    from halo2_scaffold_amd import witness

    t, inputs, listed = TC.ops_tape()
    want = t.evaluate(inputs)
    assert all(want[cell] == value for cell, value in listed)
    _run_whole(gpu, t.program(witness, reverse=reverse), inputs, want, hints=True)


@pytest.mark.parametrize("reverse", [False, True])
def test_levels_of_1025_1024_and_1_ops(gpu, reverse):
    """1025 ops as one grid launch, 1024 and 1 in one workgroup launch, above a narrow level of inputs: MSB, POW2, flagged POW2 and the
    old unary hints by turns in every level, in both orders"""
    from halo2_scaffold_amd import witness

    sizes = [40, 1025, 1024, 1]
    t, inputs = TC.layered_ops_tape(sizes)
    program = t.program(witness, reverse=reverse)
    assert program.level_sizes == sizes and W.segmentation(sizes) == (1, 2)
    _run_whole(gpu, program, inputs, t.evaluate(inputs), hints=True)


def test_a_chain_of_msb_pow2_and_division_in_one_workgroup_launch(gpu):
    """every level reads what the level before wrote: MSB, the power of two of it, a quotient by that power, 40 levels and more"""
    from halo2_scaffold_amd import witness

    t, inputs, cell, value = TC.msb_pow2_div_chain_tape(40, (1 << 100) + 5)
    program = t.program(witness)
    want = t.evaluate(inputs)
    assert want[cell] == value and len(program.level_sizes) >= 41 and W.segmentation(program.level_sizes) == (0, 1)
    _run_whole(gpu, program, inputs, want, hints=True)


def test_programs_of_the_old_hints_and_of_none_launch_what_they_launched(gpu):
    """beside a program that holds the new ops: the four old hints run the _hints kernels under the same rule and compute what they
    computed, a program without a hint runs k_witness_level / k_witness_levels_wg only"""
    from halo2_scaffold_amd import witness

    sizes = [40, 1025, 1024, 1]
    t, inputs = FC.layered_ops_tape(sizes)
    assert not {op[0] for op in t.cells} & {TC.MSB, TC.POW2}
    _run_whole(gpu, t.program(witness), inputs, t.evaluate(inputs), hints=True)
    sizes = [5, 1025, 7]
    t, inputs = W.layered_tape(sizes, seed="no hints")
    assert W.segmentation(sizes) == (1, 2)
    _run_whole(gpu, t.program(witness), inputs, t.evaluate(inputs), hints=False)
    t, inputs = TC.layered_ops_tape([8, 1025, 3])
    _run_whole(gpu, t.program(witness), inputs, t.evaluate(inputs), hints=True)


# ---- proofs -----------------------------------------------------------------------------------------------------------------------------------
RNG_KEY = bytes(range(32))


def _shapes():
    """name -> (closure, dummy, input sets, reference of the public outputs, DEGREE, LOOKUP_BITS, cells, gate columns, lookup-advice columns).
    The smallest DEGREE / LOOKUP_BITS at which each circuit fits the prover's 32 gate and 8 lookup-advice columns, and it then spreads
    over many of both.  Logistic inference with 2 features at P = 63: 13772 cells, 2870 looked up, DEGREE 9 / LOOKUP_BITS 8, 28 + 6
    columns.  One training step of 2 samples x 2 features at P = 63: 29269 cells, 6196 looked up, DEGREE 10 / LOOKUP_BITS 9, 29 + 7
    columns.  ln a, sin b and a^c at P = 32: 40316 cells, DEGREE 11 / LOOKUP_BITS 10, 20 + 4 columns.
    Every one of them has grid launches: its widest levels hold thousands of ops."""
    from halo2_scaffold_amd import logistic_regression as LG
    from halo2_scaffold_amd.fixed_point import FixedPointChip

    chip = FixedPointChip(32)

    def mixed(ctx, inputs, make_public):
        a, b, c = (ctx.load_witness(v) for v in inputs)
        make_public.append(chip.qlog(ctx, a))
        make_public.append(chip.qsin(ctx, b))
        make_public.append(chip.qpow(ctx, a, c))

    return {"inference": (LG.inference, TC.INFERENCE_DUMMY, TC.INFERENCE_INPUTS, TC.ref_inference, 9, 8, 13772, 28, 6),
            "train": (LG.train, TC.TRAIN_DUMMY, TC.TRAIN_INPUTS, TC.ref_train, 10, 9, 29269, 29, 7),
            "mixed": (mixed, TC.MIXED_DUMMY, TC.MIXED_INPUTS, TC.ref_mixed, 11, 10, 40316, 20, 4)}


@pytest.mark.parametrize("shape,key", [("inference", {}), ("train", {}), ("mixed", {}), ("inference", {"logup": True}), ("inference", {"by_coset": True})],
                         ids=["inference", "train", "qlog-qsin-qpow", "inference-logup", "inference-by_coset"])
def test_proofs_from_the_program_are_host_synthesis_byte_for_byte(gpu, tmp_path, monkeypatch, shape, key):
    from halo2_scaffold_amd import flex, scaffold

    f, dummy, input_sets, reference, k, lookup_bits, n_cells, gate_columns, lookup_columns = _shapes()[shape]
    monkeypatch.setenv("PARAMS_DIR", str(tmp_path))
    monkeypatch.delenv("MINIMUM_ROWS", raising=False)
    monkeypatch.setenv("DEGREE", str(k))
    monkeypatch.setenv("LOOKUP_BITS", str(lookup_bits))
    calls = []

    def closure(ctx, inputs, make_public):
        calls.append(1)
        f(ctx, inputs, make_public)

    pk, bp = scaffold.gen_key(closure, TC.field_inputs(dummy), witness_program=True, **key)
    try:
        cs = pk.cs
        assert (pk.program.n_cells - pk.program.n_aux, cs.num_advice, cs.num_lookup_advice) == (n_cells, gate_columns, lookup_columns)
        assert cs.num_advice >= 2 and cs.num_lookup_advice >= 2
        kinds = {int(code) & 0xFF for code in pk.program.ops[:, 1]}
        assert ({TC.MSB, TC.POW2} <= kinds) == (shape == "mixed") and pk.program.on_device().info.n_grid_launches > 0
        pk.workspace.prover.set_rng_key(RNG_KEY)
        proofs = []
        for raw in input_sets[:2] if key else input_sets:
            inputs = TC.field_inputs(raw)
            before = len(calls)
            public = scaffold.prove_private(closure, inputs, pk, bp, logup=bool(key.get("logup")))
            assert len(calls) == before  # the closure was not called: the witness is the program's
            assert public == [TC.to_field(v) for v in reference(*raw)]
            host = scaffold._synthesize(f, inputs, cs, lookup_bits)
            assert host.instance == public and list(host.break_points) == bp[0]
            assert pk.last_proof == flex.create_proof(pk.params, pk.keys, host, pk.proofs, ws=pk.workspace)
            proofs.append(pk.last_proof)
        assert len(set(proofs)) == len(proofs)
    finally:
        pk.release()


def test_qlog_of_zero_is_refused_with_nothing_committed(gpu, tmp_path, monkeypatch):
    """the program's check names the first failing equality, on the device as on the host interpreter; nothing is proven, and the key proves
    the next input"""
    from halo2_scaffold_amd import flex, scaffold
    from halo2_scaffold_amd.fixed_point import FixedPointChip

    chip = FixedPointChip(32)

    def log(ctx, inputs, make_public):
        make_public.append(chip.qlog(ctx, ctx.load_witness(inputs[0])))

    k, lookup_bits = 11, 10
    monkeypatch.setenv("PARAMS_DIR", str(tmp_path))
    monkeypatch.delenv("MINIMUM_ROWS", raising=False)
    monkeypatch.setenv("DEGREE", str(k))
    monkeypatch.setenv("LOOKUP_BITS", str(lookup_bits))
    pk, bp = scaffold.gen_key(log, [1 << 32], witness_program=True)
    try:
        pk.workspace.prover.set_rng_key(RNG_KEY)
        good = [TC.q32(0.3)]
        want = [TC.to_field(TC.Model(32).qlog(good[0]))]
        assert scaffold.mock_device(log, good, pk) == want
        proofs = pk.proofs
        for bad in ([0], [TC.to_field(-1)], [1 << 63]):
            with pytest.raises(ValueError, match="witness out of range") as e:
                scaffold.prove_private(log, bad, pk, bp)
            with pytest.raises(ValueError, match="witness out of range") as host_side:
                pk.program.cells(bad)
            assert str(e.value) == str(host_side.value) and pk.proofs == proofs  # the same first failing check, and nothing was proven
        assert scaffold.prove_private(log, good, pk, bp) == want
        assert pk.last_proof == flex.create_proof(pk.params, pk.keys, scaffold._synthesize(log, good, pk.cs, lookup_bits), pk.proofs, ws=pk.workspace)
    finally:
        pk.release()
