"""The hint ops of witness programs and the fixed-point circuits on the device: DIVQ / DIVR / ISZERO / INV word for word against the
plain-integer references of tests/fixed_point_cases.py (the cells read back canonical and as the Montgomery words of a column that holds
every cell), the launches of the _hints kernels against h2mi_witness_info and the segmentation rule, and the regression closures proven
through gen_key(witness_program=True) / prove_private byte for byte against host synthesis with the same key, seed and rng key."""
import ctypes as C

import numpy as np
import pytest

import fixed_point_cases as FC
import witness_cases as W
from oracle import bn254 as o
from oracle import flex as FX

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
    """run a program whose one column holds every cell: the canonical values read back and the column's Montgomery words against
    `want`; the launches of the run — of the _hints kernels for a program that holds a hint op, of the plain ones otherwise — against
    h2mi_witness_info and the segmentation rule"""
    from halo2_scaffold_amd import engine, witness

    dev = program.on_device()
    out = {}
    launches = _profiled(gpu, lambda: out.update(columns=dev.run(witness.flatten_inputs(inputs))))
    info = dev.info
    grid, wg = W.segmentation(program.level_sizes)
    assert (info.n_cells, info.n_levels, info.n_grid_launches, info.n_wg_launches) == (program.n_cells, len(program.level_sizes), grid, wg)
    plan = witness.segmentation(program.level_sizes)
    assert (sum(1 for p in plan if p[0] == "grid"), sum(1 for p in plan if p[0] == "wg")) == (grid, wg)
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
def test_every_dividend_by_every_divisor_in_every_form(gpu, reverse):
    """DIVQ and DIVR, unsigned and signed, by a cell and by a constant, of every dividend x divisor pair of the cases (0, 1, the 32- and
    64-bit word boundaries, 2^252 and its neighbours, r - 1, the dividend itself and its neighbours, zero divisors, exact negative
    multiples), ISZERO and INV at the Montgomery extremes; operands from INPUT, CONST and GATE cells.  A grid launch between two
    workgroup launches; reverse: the ops of every level stored in descending dst order"""
    from halo2_scaffold_amd import witness

    t, inputs, listed = FC.ops_tape()
    want = t.evaluate(inputs)
    assert all(want[cell] == FC.ref_hint(kind, x, y, flags) for cell, kind, x, y, flags in listed)
    _run_whole(gpu, t.program(witness, reverse=reverse), inputs, want, hints=True)


def test_hint_levels_of_1025_1024_and_1_ops(gpu):
    """1025 hint ops as one grid launch, 1024 and 1 in one workgroup launch, above a narrow level of inputs"""
    from halo2_scaffold_amd import witness

    sizes = [40, 1025, 1024, 1]
    t, inputs = FC.layered_ops_tape(sizes)
    program = t.program(witness)
    assert program.level_sizes == sizes and W.segmentation(sizes) == (1, 2)
    _run_whole(gpu, program, inputs, t.evaluate(inputs), hints=True)


def test_a_chain_of_40_divisions_in_one_workgroup_launch(gpu):
    """every level divides the quotient the level before wrote, by a constant and by a cell by turns"""
    from halo2_scaffold_amd import witness

    t, inputs, cell, value = FC.quotient_chain_tape(40, R - 12345)
    program = t.program(witness)
    want = t.evaluate(inputs)
    assert want[cell] == value and W.segmentation(program.level_sizes) == (0, 1)
    _run_whole(gpu, program, inputs, want, hints=True)


def test_a_program_without_hints_launches_the_kernels_it_launched(gpu):
    """beside the programs above: narrow, wide, narrow levels of copies and limbs run k_witness_level / k_witness_levels_wg only"""
    from halo2_scaffold_amd import witness

    sizes = [5, 1025, 7]
    t, inputs = W.layered_tape(sizes, seed="no hints")
    program = t.program(witness)
    assert W.segmentation(sizes) == (1, 2)
    _run_whole(gpu, program, inputs, t.evaluate(inputs), hints=False)


# ---- proofs -----------------------------------------------------------------------------------------------------------------------------------
RNG_KEY = bytes(range(32))


def _shapes():
    """name -> (closure, dummy, input sets, reference of the public outputs, DEGREE, LOOKUP_BITS, cells, gate columns, lookup-advice columns).
    Inference with 3 features is 1197 cells, 342 of them looked up: DEGREE 8 / LOOKUP_BITS 7 lays them over 5 gate columns and 2
    lookup-advice columns, and is the largest DEGREE that does (at DEGREE 9 / LOOKUP_BITS 8 the 306 cells to look up fit one column).
    One training step of 2 samples x 2 features at DEGREE 9 / LOOKUP_BITS 8 is 3968 cells over 8 + 3 columns, its widest level a grid
    launch."""
    from halo2_scaffold_amd import linear_regression as LR

    flat_train = lambda w, b, x, y, rate: (lambda nw, nb: nw + [nb])(*FC.ref_train(w, b, x, y, rate))
    return {"inference": (LR.inference, FC.INFERENCE_DUMMY, FC.INFERENCE_INPUTS, lambda x, w, b: list(x) + [FC.ref_inference(x, w, b)], 8, 7, 1197, 5, 2),
            "train": (LR.train, FC.TRAIN_DUMMY, FC.TRAIN_INPUTS, flat_train, 9, 8, 3968, 8, 3)}


def _oracle_vk(pk, recorded, k):
    """the oracle's closed-form verifying key of the builders' several-column constraint system, from the key's own fixed cells and copies"""
    from halo2_scaffold_amd.params import gen_srs_secret

    cs = pk.cs
    ocs = FX.flex_multi_cs(True, cs.num_advice, cs.num_lookup_advice, cs.num_fixed)
    fixed = [dict(enumerate(recorded.table_values)) if cells is None else dict(cells) for cells in recorded.fixed]
    vk = FX.VerifierKeys(ocs, k, gen_srs_secret(), fixed, list(recorded.copies))
    assert vk.transcript_repr == pk.get_vk().transcript_repr
    return vk


@pytest.mark.parametrize("shape,key", [("inference", {}), ("train", {}), ("inference", {"logup": True}), ("inference", {"by_coset": True})],
                         ids=["inference", "train", "inference-logup", "inference-by_coset"])
def test_regression_proofs_from_the_program_are_host_synthesis_byte_for_byte(gpu, tmp_path, monkeypatch, shape, key):
    from halo2_scaffold_amd import flex, scaffold, witness

    f, dummy, input_sets, reference, k, lookup_bits, n_cells, gate_columns, lookup_columns = _shapes()[shape]
    monkeypatch.setenv("PARAMS_DIR", str(tmp_path))
    monkeypatch.delenv("MINIMUM_ROWS", raising=False)
    monkeypatch.setenv("DEGREE", str(k))
    monkeypatch.setenv("LOOKUP_BITS", str(lookup_bits))
    calls = []

    def closure(ctx, inputs, make_public):
        calls.append(1)
        f(ctx, inputs, make_public)

    pk, bp = scaffold.gen_key(closure, FC.field_inputs(dummy), witness_program=True, **key)
    try:
        cs = pk.cs
        assert (pk.program.n_cells - pk.program.n_aux, cs.num_advice, cs.num_lookup_advice) == (n_cells, gate_columns, lookup_columns)
        assert (pk.program.on_device().info.n_grid_launches > 0) == (shape == "train")  # the training step's widest levels are grid launches
        pk.workspace.prover.set_rng_key(RNG_KEY)
        _, recorded = witness.Program.record(f, FC.field_inputs(dummy), cs, lookup_bits)
        vk = None if key.get("logup") else _oracle_vk(pk, recorded, k)  # a by-coset key proves the plain key's bytes
        proofs = []
        for raw in input_sets:
            inputs = FC.field_inputs(raw)
            before = len(calls)
            public = scaffold.prove_private(closure, inputs, pk, bp, logup=bool(key.get("logup")))
            assert len(calls) == before  # the closure was not called: the witness is the program's
            want_public = [FC.to_field(v) for v in reference(*raw)]
            assert public == want_public
            host = scaffold._synthesize(f, inputs, cs, lookup_bits)
            assert host.instance == public and list(host.break_points) == bp[0]
            assert pk.last_proof == flex.create_proof(pk.params, pk.keys, host, pk.proofs, ws=pk.workspace)
            if vk is not None:
                assert FX.verify(vk, pk.last_proof, [public]) and not FX.verify(vk, pk.last_proof, [public[:-1] + [(public[-1] + 1) % R]])
            proofs.append(pk.last_proof)
        assert len(set(proofs)) == len(proofs)
    finally:
        pk.release()


def test_refusals_and_the_device_check(gpu, tmp_path, monkeypatch):
    """mock_device passes on good inputs and flex.check names the violation of a host assignment with one hint cell moved; an input
    that makes a divisor zero is a witness out of range before anything is committed, and the key proves the next input"""
    from halo2_scaffold_amd import flex, scaffold
    from halo2_scaffold_amd.fixed_point import FixedPointChip

    chip = FixedPointChip(FC.P)

    def quotients(ctx, inputs, make_public):  # a / b in fixed point, and a div b of the integers
        a, b = (ctx.load_witness(v) for v in inputs)
        make_public.append(chip.qdiv(ctx, a, b))
        make_public.append(ctx.div_mod_var(chip.qabs(ctx, a), chip.qabs(ctx, b), 2 * FC.P + 1, 2 * FC.P)[0])

    k, lookup_bits = 11, 8
    monkeypatch.setenv("PARAMS_DIR", str(tmp_path))
    monkeypatch.delenv("MINIMUM_ROWS", raising=False)
    monkeypatch.setenv("DEGREE", str(k))
    monkeypatch.setenv("LOOKUP_BITS", str(lookup_bits))
    pk, bp = scaffold.gen_key(quotients, [7, 2], witness_program=True)
    try:
        pk.workspace.prover.set_rng_key(RNG_KEY)
        good = [FC.to_field(-7 * FC.ONE), 2 * FC.ONE]
        want = [FC.to_field(FC.REF["qdiv"](-7 * FC.ONE, 2 * FC.ONE)), 3]
        assert scaffold.mock_device(quotients, good, pk) == want
        host = scaffold._synthesize(quotients, good, pk.cs, lookup_bits)
        flex.check(pk.params, pk.keys, host, 1, ws=pk.workspace)
        quotient = max(int(dst) for dst, code, _, _ in pk.program.ops.tolist() if code & 0xFF == flex.DIVQ)  # the integer quotient's hint cell
        column, row = next((j, int(np.nonzero(src == quotient)[0][0])) for j, src in enumerate(pk.program.placement) if quotient in src)
        assert host.advice[column][row] == want[1]
        host.advice[column][row] += 1
        with pytest.raises(ValueError, match="not satisfied"):
            flex.check(pk.params, pk.keys, host, 1, ws=pk.workspace)
        proofs = pk.proofs
        for bad in ([good[0], 0], [0, 0]):
            with pytest.raises(ValueError, match="witness out of range") as e:
                scaffold.prove_private(quotients, bad, pk, bp)
            with pytest.raises(ValueError, match="witness out of range") as host_side:
                pk.program.cells(bad)
            assert str(e.value) == str(host_side.value) and pk.proofs == proofs  # the same first failing check, and nothing was proven
        assert scaffold.prove_private(quotients, good, pk, bp) == want
        assert pk.last_proof == flex.create_proof(pk.params, pk.keys, scaffold._synthesize(quotients, good, pk.cs, lookup_bits), pk.proofs, ws=pk.workspace)
    finally:
        pk.release()
