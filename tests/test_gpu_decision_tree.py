"""The decision-tree closures on the device: the training tape's every cell word for word against the interpreter on every data set of
tests/decision_tree_cases.py, its launches — grid and workgroup form inside one program — against h2mi_witness_info and the segmentation
rule; inference and training proven through gen_key(witness_program=True) / prove_private byte for byte against host synthesis with the
same key, seed and rng key, accepted by the oracle's verifier, also under a logUp and a by-coset key; mock_device; and a key made from one
data set proving another."""
import ctypes as C

import pytest

import decision_tree_cases as DC
from oracle import bn254 as o
from oracle import flex as FX

pytestmark = pytest.mark.gpu

R = o.R
KERNELS = ("k_witness_level", "k_witness_level_hints", "k_witness_levels_wg", "k_witness_levels_wg_hints", "k_witness_place")
RNG_KEY = bytes(range(32))


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


def set_sizes(monkeypatch, DT, max_depth=DC.MAX_DEPTH, min_size=DC.MIN_SIZE, tree=DC.TREE):
    for name, value in (("num_feature", DC.NUM_FEATURE), ("num_class", DC.NUM_CLASS), ("max_depth", max_depth), ("min_size", min_size),
                        ("max_path_len", DC.MAX_PATH_LEN), ("tree", DC.field_inputs(tree))):
        monkeypatch.setattr(DT, name, value)


def _environment(monkeypatch, tmp_path, k, lookup_bits):
    monkeypatch.setenv("PARAMS_DIR", str(tmp_path))
    monkeypatch.delenv("MINIMUM_ROWS", raising=False)
    monkeypatch.setenv("DEGREE", str(k))
    monkeypatch.setenv("LOOKUP_BITS", str(lookup_bits))


# ---- the tape -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tapes():
    """(max_depth, min_size) -> the program recorded from the dummy set, shared by the data sets of that shape"""
    made = {}
    yield made
    for program in made.values():
        program.release()


def _tape(monkeypatch, _TAPES, data):
    from halo2_scaffold_amd import decision_tree as DT
    from halo2_scaffold_amd import scaffold, witness

    set_sizes(monkeypatch, DT, data.max_depth, data.min_size)
    key = (data.max_depth, data.min_size)
    if key not in _TAPES:
        cs = scaffold._config(DT.train, DC.TRAIN_DUMMY.inputs, data.k, data.lookup_bits, 9)
        _TAPES[key] = witness.Program.record(DT.train, DC.TRAIN_DUMMY.inputs, cs, data.lookup_bits)[0]
    return _TAPES[key]


@pytest.mark.parametrize("data", DC.DATA_SETS, ids=[d.name.replace(" ", "_") for d in DC.DATA_SETS])
def test_every_cell_of_the_training_tape(gpu, monkeypatch, tapes, data):
    from halo2_scaffold_amd import witness

    program = _tape(monkeypatch, tapes, data)
    want = program.cells(data.inputs)
    assert [want[c] for c in program.public] == data.public
    dev = program.on_device()
    launches = _profiled(gpu, lambda: dev.run(witness.flatten_inputs(data.inputs)))
    plan = [p[0] for p in witness.segmentation(program.level_sizes)]
    grid, wg = plan.count("grid"), plan.count("wg")
    assert grid >= 2 and wg >= 2  # both launch forms inside one program
    info = dev.info
    assert (info.n_cells, info.n_levels, info.n_grid_launches, info.n_wg_launches) == (program.n_cells, len(program.level_sizes), grid, wg)
    ran = {"k_witness_level_hints": grid, "k_witness_levels_wg_hints": wg, "k_witness_place": 1}
    assert launches == {name: ran.get(name, 0) for name in KERNELS}
    got = dev.read(list(range(len(want))))
    wrong = [i for i in range(len(want)) if got[i] != want[i]]
    assert not wrong, (len(wrong), wrong[:5], [hex(got[i]) for i in wrong[:3]], [hex(want[i]) for i in wrong[:3]])
    assert dev.read(program.public) == data.public


# ---- proofs -----------------------------------------------------------------------------------------------------------------------------------------
def _oracle_vk(pk, recorded, k):
    """the oracle's closed-form verifying key of the builders' several-column constraint system, from the key's own fixed cells and copies"""
    from halo2_scaffold_amd.params import gen_srs_secret

    cs = pk.cs
    ocs = FX.flex_multi_cs(True, cs.num_advice, cs.num_lookup_advice, cs.num_fixed)
    fixed = [dict(enumerate(recorded.table_values)) if cells is None else dict(cells) for cells in recorded.fixed]
    vk = FX.VerifierKeys(ocs, k, gen_srs_secret(), fixed, list(recorded.copies))
    assert vk.transcript_repr == pk.get_vk().transcript_repr
    return vk


def _shapes():
    """name -> (closure, dummy, [(inputs, public outputs)], DEGREE, LOOKUP_BITS, cells, gate columns, lookup-advice columns)"""
    from halo2_scaffold_amd import decision_tree as DT

    return {"inference": (DT.inference, DC.field_inputs(DC.INFERENCE_DUMMY), [(DC.field_inputs(x), [cls]) for x, cls, _ in DC.INFERENCE_INPUTS],
                          DC.INFERENCE_K, DC.INFERENCE_LOOKUP_BITS, 7625, 16, 1),
            "train": (DT.train, DC.TRAIN_DUMMY.inputs, [(DC.BY_NAME[name].inputs, DC.BY_NAME[name].public) for name in DC.PROVEN],
                      DC.TRAIN_K, DC.TRAIN_LOOKUP_BITS, 71757, 18, 5)}


@pytest.mark.parametrize("shape,key", [("inference", {}), ("train", {}), ("inference", {"logup": True}), ("train", {"logup": True}),
                                       ("inference", {"by_coset": True}), ("train", {"by_coset": True})],
                         ids=["inference", "train", "inference-logup", "train-logup", "inference-by_coset", "train-by_coset"])
def test_proofs_from_the_program_are_host_synthesis_byte_for_byte(gpu, tmp_path, monkeypatch, shape, key):
    from halo2_scaffold_amd import decision_tree as DT
    from halo2_scaffold_amd import flex, scaffold, witness

    set_sizes(monkeypatch, DT)
    f, dummy, cases, k, lookup_bits, n_cells, gate_columns, lookup_columns = _shapes()[shape]
    _environment(monkeypatch, tmp_path, k, lookup_bits)
    calls = []

    def closure(ctx, inputs, make_public):
        calls.append(1)
        f(ctx, inputs, make_public)

    pk, bp = scaffold.gen_key(closure, dummy, witness_program=True, **key)
    plain = None
    try:
        cs = pk.cs
        assert (pk.program.n_cells - pk.program.n_aux, cs.num_advice, cs.num_lookup_advice) == (n_cells, gate_columns, lookup_columns)
        pk.workspace.prover.set_rng_key(RNG_KEY)
        # the key host synthesis proves against: made without the flag, from the same dummy
        plain, plain_bp = scaffold.gen_key(f, dummy, **key)
        plain.workspace.prover.set_rng_key(RNG_KEY)
        assert plain.program is None and plain_bp == bp and plain.get_vk().transcript_repr == pk.get_vk().transcript_repr
        vk = None
        if not key:
            _, recorded = witness.Program.record(f, dummy, cs, lookup_bits)
            vk = _oracle_vk(pk, recorded, k)
        proofs = []
        for inputs, want in cases[:1] if key else cases:  # one input again under a logUp and under a by-coset key
            before = len(calls)
            assert scaffold.mock_device(closure, inputs, pk) == want
            public = scaffold.prove_private(closure, inputs, pk, bp, logup=bool(key.get("logup")))
            assert len(calls) == before and public == want  # the closure was not called: the witness is the program's
            host = scaffold._synthesize(f, inputs, plain.cs, lookup_bits)
            assert host.instance == public and list(host.break_points) == bp[0]
            assert pk.last_proof == flex.create_proof(plain.params, plain.keys, host, pk.proofs, ws=plain.workspace)
            if vk is not None:
                assert FX.verify(vk, pk.last_proof, [public]) and not FX.verify(vk, pk.last_proof, [public[:-1] + [(public[-1] + 1) % R]])
            proofs.append(pk.last_proof)
        assert len(set(proofs)) == len(proofs)
    finally:
        pk.release()
        if plain is not None:
            plain.release()


def test_a_key_made_from_one_data_set_proves_another(gpu, tmp_path, monkeypatch):
    """the tape holds the closure, not the inputs it was recorded on: the key of data set A proves B, and the public tree is B's"""
    from halo2_scaffold_amd import decision_tree as DT
    from halo2_scaffold_amd import flex, scaffold

    set_sizes(monkeypatch, DT)
    a, b = DC.BY_NAME["feature 0 separates"], DC.BY_NAME["feature 1 separates"]
    assert a.public != b.public
    _environment(monkeypatch, tmp_path, DC.TRAIN_K, DC.TRAIN_LOOKUP_BITS)
    pk, bp = scaffold.gen_key(DT.train, a.inputs, witness_program=True)
    try:
        pk.workspace.prover.set_rng_key(RNG_KEY)
        assert scaffold.prove_private(DT.train, b.inputs, pk, bp) == b.public
        host = scaffold._synthesize(DT.train, b.inputs, pk.cs, DC.TRAIN_LOOKUP_BITS)
        assert pk.last_proof == flex.create_proof(pk.params, pk.keys, host, pk.proofs, ws=pk.workspace)
        assert scaffold.prove_private(DT.train, a.inputs, pk, bp) == a.public
    finally:
        pk.release()


def test_mock_device_on_the_one_node_tree(gpu, tmp_path, monkeypatch):
    from halo2_scaffold_amd import decision_tree as DT
    from halo2_scaffold_amd import scaffold

    set_sizes(monkeypatch, DT, tree=DC.ONE_NODE_TREE)
    _environment(monkeypatch, tmp_path, DC.INFERENCE_K, DC.INFERENCE_LOOKUP_BITS)
    pk, bp = scaffold.gen_key(DT.inference, DC.field_inputs(DC.INFERENCE_DUMMY), witness_program=True)
    try:
        for x, _, _ in DC.INFERENCE_INPUTS[:2]:
            assert scaffold.mock_device(DT.inference, DC.field_inputs(x), pk) == [1]
    finally:
        pk.release()
