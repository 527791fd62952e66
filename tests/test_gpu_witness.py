"""Witness programs on the device: the kernels word for word against the Python integers of tests/witness_cases.py (hand-built tapes,
the cells read back canonical and as the Montgomery words of a column that holds every cell), the launches from the library's profile
against h2mi_witness_info and the Python segmentation, and proofs whose witness comes from a program byte for byte against host
synthesis with the same key and seed."""
import ctypes as C

import numpy as np
import pytest

import witness_cases as W
from oracle import bn254 as o
from oracle import flex as FX

pytestmark = pytest.mark.gpu

R = o.R
SRS_SECRET = 0x5EC2E7 + 0x48324D49
X, Y = 0x0123456789ABCDEF, 0xFEDCBA9876543210


def _profiled(gpu, call) -> dict:
    """launches of the witness kernels during call(), from the library's launch profile"""
    lib = gpu.lib
    assert lib.h2mi_profile_reset() == 0 and lib.h2mi_profile_filter(b"k_witness") == 0 and lib.h2mi_profile_enable(1) == 0
    try:
        call()
    finally:
        assert lib.h2mi_profile_enable(0) == 0
    out = {}
    for name in ("k_witness_level", "k_witness_levels_wg", "k_witness_place"):
        ms, count = C.c_double(), C.c_uint64()
        assert lib.h2mi_profile_query(name.encode(), C.byref(ms), C.byref(count)) == 0
        out[name] = count.value
    out["k_witness_level"] -= out["k_witness_levels_wg"]  # the query matches by prefix
    assert lib.h2mi_profile_reset() == 0 and lib.h2mi_profile_filter(b"") == 0
    return out


def _run_whole(gpu, program, inputs, want):
    """run a program whose one column holds every cell: the canonical values read back and the column's Montgomery words against
    `want`; the launches of the run against h2mi_witness_info and the segmentation rule"""
    from halo2_scaffold_amd import engine, witness

    dev = program.on_device()
    out = {}
    launches = _profiled(gpu, lambda: out.update(columns=dev.run(witness.flatten_inputs(inputs))))
    info = dev.info
    grid, wg = W.segmentation(program.level_sizes)
    assert (info.n_cells, info.n_levels) == (program.n_cells, len(program.level_sizes))
    assert (launches["k_witness_level"], launches["k_witness_levels_wg"], launches["k_witness_place"]) == (grid, wg, 1) == \
        (info.n_grid_launches, info.n_wg_launches, 1)
    plan = witness.segmentation(program.level_sizes)
    assert (sum(1 for p in plan if p[0] == "grid"), sum(1 for p in plan if p[0] == "wg")) == (grid, wg)
    n = program.n_cells
    assert dev.read(list(range(n))) == want
    (column,) = out["columns"]
    assert len(column) == n
    words = engine.DevView(column.values_ptr, n).to_numpy(shape=(n, 4))
    assert np.array_equal(words, o.pack(want, R))
    program.release()


@pytest.mark.parametrize("reverse", [False, True])
def test_input_const_copy_gate_at_the_limb_extremes(gpu, reverse):
    """every a + b * c of the edge values (0, 1, r - 1, 2^64 - 1, 2^253, canonical and Montgomery words of all ones: products that
    wrap), the operands as INPUT, CONST and COPY cells; reverse: the ops of every level stored in descending dst order"""
    from halo2_scaffold_amd import witness

    t, inputs = W.values_tape()
    _run_whole(gpu, t.program(witness, reverse=reverse), inputs, t.evaluate(inputs))


def test_limb_at_every_shift_and_width(gpu):
    from halo2_scaffold_amd import witness

    t, inputs, listed = W.limb_tape()
    want = t.evaluate(inputs)
    assert all(want[c] == (v >> shift) & ((1 << bits) - 1) for c, v, shift, bits in listed)
    _run_whole(gpu, t.program(witness), inputs, want)


def test_levels_of_1_1023_1024_1025_2049_ops_narrow_wide_narrow(gpu):
    """1, 1023 and 1024 ops in one workgroup launch, 1025 and 2049 as grid launches, then narrow, wide, narrow again"""
    from halo2_scaffold_amd import witness

    sizes = [1, 1023, 1024, 1025, 2049, 5, 1025, 7]
    t, inputs = W.layered_tape(sizes)
    program = t.program(witness)
    assert program.level_sizes == sizes and W.segmentation(sizes) == (3, 3)
    _run_whole(gpu, program, inputs, t.evaluate(inputs))


def test_a_chain_of_300_levels_in_one_workgroup_launch(gpu):
    """x <- c + x^2 150 times: every level reads what the level before wrote, from another wavefront's lanes"""
    from halo2_scaffold_amd import witness

    t, inputs, cell, value = W.square_chain_tape(150, 0x1234567, R - 5)
    want = t.evaluate(inputs)
    assert want[cell] == value and W.segmentation(t.program(witness).level_sizes) == (0, 1)
    _run_whole(gpu, t.program(witness), inputs, want)


def test_a_chain_of_4100_one_op_levels_is_two_workgroup_launches(gpu):
    from halo2_scaffold_amd import witness

    t, inputs, cell = W.one_op_chain_tape(4100, 0xFEDCBA9876543211)
    program = t.program(witness)
    assert W.segmentation(program.level_sizes) == (0, 2)
    _run_whole(gpu, program, inputs, t.evaluate(inputs))


def test_placement_of_three_columns_with_repeated_sources(gpu):
    from halo2_scaffold_amd import engine, witness

    t, inputs = W.layered_tape([40, 300, 90], seed="placement")
    n = len(t.cells)
    placement = [[n - 1], [(7 * i) % n for i in range(256)], [n - 1 - (i % 100) for i in range(257)]]
    program = t.program(witness, placement=placement)
    want = t.evaluate(inputs)
    dev = program.on_device()
    columns = dev.run(inputs)
    assert [len(c) for c in columns] == [1, 256, 257]
    assert columns[1].values_ptr == columns[0].values_ptr + 32 and columns[2].values_ptr == columns[1].values_ptr + 32 * 256
    for column, src in zip(columns, placement):
        words = engine.DevView(column.values_ptr, len(src)).to_numpy(shape=(len(src), 4))
        assert np.array_equal(words, o.pack([want[s] for s in src], R))
    assert dev.info.device_bytes >= 32 * n + 32 * 514 + 16 * n + 4 * 514
    program.release()


def test_a_failing_check_first_last_alone_and_the_lowest_is_reported(gpu):
    """600 checks (more than two workgroups of the placement launch, behind 3 placed cells): pairs of inputs that agree unless told not to"""
    from halo2_scaffold_amd import witness

    n_checks = 600
    t = W.Tape()
    for j in range(2 * n_checks):
        t.input(j)
    checks = [(2 * i, 2 * i + 1) for i in range(n_checks)]
    program = t.program(witness, checks=checks, placement=[[0, 1, 2]])
    dev = program.on_device()

    def inputs(failing):
        return [1000 + j // 2 + (1 if j % 2 and j // 2 in failing else 0) for j in range(2 * n_checks)]

    assert len(dev.run(inputs(()))) == 1
    for failing, lowest in (([0], 0), ([n_checks - 1], n_checks - 1), ([311], 311), ([7, 300, 599], 7), (list(range(n_checks)), 0), ([599, 256, 257], 256)):
        with pytest.raises(ValueError, match=f"witness out of range: check {lowest} fails, cells {2 * lowest} and {2 * lowest + 1} differ"):
            dev.run(inputs(failing))
        with pytest.raises(ValueError, match=f"witness out of range: check {lowest} "):
            program.cells(inputs(failing))
    assert len(dev.run(inputs(()))) == 1 and dev.read([0, 1199]) == [1000, 1599]  # the program stays usable
    # refusals of run and read: an input not below r, a wrong count, a cell outside the program
    with pytest.raises(engine_error(gpu)) as e:
        dev.run([R] + inputs(())[1:])
    assert e.value.code == -1
    with pytest.raises(ValueError):
        dev.run([1, 2])
    with pytest.raises(engine_error(gpu)) as e:
        dev.read([1200])
    assert e.value.code == -1
    program.release()


def engine_error(gpu):
    from halo2_scaffold_amd import engine

    return engine.H2miError


def test_the_empty_program_and_released_handles(gpu):
    from halo2_scaffold_amd import witness

    program = witness.Program(np.zeros((0, 4)), [], [], 0, [], [], [])
    dev = program.on_device()
    assert dev.run([]) == [] and dev.read([]) == []
    info = dev.info
    assert (info.n_cells, info.n_levels, info.n_grid_launches, info.n_wg_launches) == (0, 0, 0, 0)
    handle = dev.handle
    program.release()
    assert gpu.lib.h2mi_witness_release(handle) == -5  # released already


# ---- proofs: byte for byte against host synthesis, same key, same seed ---------------------------------------------------------------------
def _host(flex, f, inputs, cs, lookup_bits):
    from halo2_scaffold_amd import scaffold

    return scaffold._synthesize(f, inputs, cs, lookup_bits)


def _prove_both(gpu, f, dummy, inputs_list, cs, lookup_bits, k, seed=29, **key):
    """keys from the recorded run; for every inputs of the list a proof from host synthesis and one from the program, through one
    workspace -> the proofs (asserted equal)"""
    from halo2_scaffold_amd import flex, witness

    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    program, recorded = witness.Program.record(f, dummy, cs, lookup_bits)
    keys = flex.FlexKeys(params, cs, recorded, **key)
    ws = flex.FlexWorkspace(params, keys)
    proofs = []
    try:
        for inputs in inputs_list:
            host = _host(flex, f, inputs, cs, lookup_bits)
            for multiopen in ("shplonk", "gwc"):
                want = flex.create_proof(params, keys, host, seed, ws=ws, multiopen=multiopen)
                asg = witness.assignment(program, inputs)
                assert asg.instance == host.instance
                launches = _profiled(gpu, lambda: proofs.append(flex.create_proof(params, keys, asg, seed, ws=ws, multiopen=multiopen)))
                assert proofs[-1] == want, (inputs, multiopen)
                assert launches["k_witness_place"] == 0  # the advice call reads the columns; it does not run the program
    finally:
        program.release()
        ws.release()
        keys.release()
        params.release()
    return proofs


def test_gate_closure_proof_at_k5(gpu):
    from halo2_scaffold_amd import flex

    proofs = _prove_both(gpu, W.gate_closure, 3, [X, R - 2], flex.FlexGateCS(False), None, 5)
    assert proofs[0] != proofs[2]  # two runs back to back on different inputs: each gives its own inputs' proof


@pytest.mark.parametrize("k,lookup_bits", [(8, 7), (9, 8), (13, 12), (8, 4), (8, 5)])
def test_range_closure_proofs(gpu, k, lookup_bits):
    """LOOKUP_BITS 7 (64 mod 7 = 1: assert_bit's region), 8 (8 divides 64: no top-limb step) and 12 (64 mod 12 = 4: the shifted top
    limb), each at the smallest k whose usable rows hold the 2^LOOKUP_BITS table rows (8, 9 and 13: the builders refuse a table that
    does not fit); the latter two shapes once more at k = 8, with LOOKUP_BITS 4 and 5 (64 mod 5 = 4)"""
    from halo2_scaffold_amd import flex

    _prove_both(gpu, W.range_closure, W.range_inputs(0, 1), [W.range_inputs(X, 1), W.range_inputs(Y, 1)], flex.FlexGateCS(True), lookup_bits, k)


@pytest.mark.parametrize("key", [{}, {"by_coset": True}, {"logup": True}])
def test_24_range_checks_over_11_and_4_columns_at_k7(gpu, key):
    """break duplicates and lookup-advice copies; a plain, a by-coset and a logUp key; both multi-opening endings"""
    from halo2_scaffold_amd import flex

    _prove_both(gpu, W.range_closure, W.range_inputs(5, 24), [W.range_inputs(X, 24)], flex.FlexGateCS(True, 11, 4, k=7), 4, 7, **key)


def test_an_input_beyond_64_bits_is_refused_before_any_commitment(gpu):
    from halo2_scaffold_amd import flex, witness

    k, lookup_bits, seed = 8, 5, 3
    cs = flex.FlexGateCS(True)
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    program, recorded = witness.Program.record(W.range_closure, [0, 0, 0], cs, lookup_bits)
    keys = flex.FlexKeys(params, cs, recorded)
    ws = flex.FlexWorkspace(params, keys)
    good = [X, Y, 5]
    want = flex.create_proof(params, keys, _host(flex, W.range_closure, good, cs, lookup_bits), seed, ws=ws)
    written = []
    t = flex.Blake2bWrite.init()
    write = t.write_point
    t.write_point = lambda pt: (written.append(pt), write(pt))[1]
    for bad in ([X, 1 << 64, 5], [X, Y, R - 1], [(1 << 64) + 7, 1 << 200, 5]):
        with pytest.raises(ValueError, match="witness out of range") as e:
            flex.create_proof(params, keys, witness.assignment(program, bad), seed, transcript=t, ws=ws)
        assert not written
        with pytest.raises(ValueError, match="witness out of range") as host:
            program.cells(bad)
        assert str(e.value) == str(host.value)  # the same first failing check
    assert flex.create_proof(params, keys, witness.assignment(program, good), seed, ws=ws) == want  # the prover stays usable
    program.release()
    ws.release()
    keys.release()
    params.release()


def test_through_the_scaffold_at_degree_7(gpu, tmp_path, monkeypatch):
    """gen_key(witness_program=True): prove_private and mock_device do not call the closure, return the host route's public inputs,
    and the proof is accepted by the oracle's verifier against the closed-form verifying key"""
    from halo2_scaffold_amd import scaffold
    from halo2_scaffold_amd.params import gen_srs_secret

    monkeypatch.setenv("PARAMS_DIR", str(tmp_path))
    monkeypatch.delenv("MINIMUM_ROWS", raising=False)
    monkeypatch.setenv("DEGREE", "7")
    monkeypatch.setenv("LOOKUP_BITS", "4")
    calls = []

    def range_example(ctx, x, make_public):  # examples/range.rs:10-34
        calls.append(x)
        xc = ctx.load_witness(x)
        make_public.append(xc)
        ctx.range_check(xc, 64, ctx.lookup_bits)
        ctx.add(xc, xc)

    x = 0xDEADBEEFCAFE1234
    plain, bp_plain = scaffold.gen_key(range_example, 0)
    want_public = scaffold.prove_private(range_example, x, plain, bp_plain)
    pk, bp = scaffold.gen_key(range_example, 0, witness_program=True)
    assert bp == bp_plain and pk.program is not None and plain.program is None
    assert pk.get_vk().transcript_repr == plain.get_vk().transcript_repr
    before = len(calls)
    assert scaffold.prove_private(range_example, x, pk, bp) == want_public == [x]
    assert scaffold.mock_device(range_example, x, pk) == [x]
    assert len(calls) == before  # the closure was not called
    ocs = FX.flex_gate_cs(True)
    oasg = FX.range_assignment(ocs, x, 4, 64)
    vk = FX.VerifierKeys(ocs, 7, gen_srs_secret(), oasg.fixed, oasg.copies)
    assert pk.get_vk().transcript_repr == vk.transcript_repr
    assert FX.verify(vk, pk.last_proof, [[x]]) and not FX.verify(vk, pk.last_proof, [[x + 1]])
    first = pk.last_proof
    assert scaffold.prove_private(range_example, x + 1, pk, bp) == [x + 1] and FX.verify(vk, pk.last_proof, [[x + 1]]) and pk.last_proof != first
    proofs = pk.proofs
    with pytest.raises(ValueError, match="witness out of range"):
        scaffold.prove_private(range_example, 1 << 64, pk, bp)
    assert pk.proofs == proofs and len(calls) == before
    with pytest.raises(ValueError, match="break points"):
        scaffold.prove_private(range_example, x, pk, [[3]])
    assert scaffold.prove_private(range_example, x, pk, bp) == [x] and FX.verify(vk, pk.last_proof, [[x]])
    pk.release()
    plain.release()
    # prove(..., witness_program=True) passes the flag through
    before = len(calls)
    proof, public = scaffold.prove(range_example, x, 0, witness_program=True)
    assert public == [x] and FX.verify(vk, proof, [[x]]) and len(calls) == before + 2  # configure and the recorded run; no third call
