"""Proving-key files on the device: the compaction kernels (h2mi_fr_compact_cells_dev) word for word against Python integers;
h2mi_prover_pk_export byte for byte against the Python writer of tests/key_file_cases.py; export -> release -> import -> prove for the
kinds of key the project proves, with the proof bytes of the original key (and of the committed golden where there is one), in both
HBM layouts; the refusals that need the device; the hosts (custom.Keys, flex.FlexKeys, scaffold.gen_key)."""
import ctypes as C
import io
import json
import os
import subprocess

import numpy as np
import pytest

import assigned_cases
import custom_gate_cases as gate_cases
import instance_cases
import key_file_cases as K
import logup_cases
import logup_sets_cases
import lookup_expr_cases as lookup_cases
import phase_cases
import shuffle_cases
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

R = K.R
SRS_SECRET = 0x5EC2E7 + 0x48324D49
EINVAL, ERANGE = -1, -6
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


Compacted = K.Compacted


def _profile(gpu, call) -> dict:
    """{kernel: launches} during call(), for the kernels of the two cell routes"""
    lib = gpu.lib
    assert lib.h2mi_profile_reset() == 0 and lib.h2mi_profile_filter(b"") == 0 and lib.h2mi_profile_enable(1) == 0
    try:
        out = call()
    finally:
        assert lib.h2mi_profile_enable(0) == 0
    counts = {}
    for name in ("k_cells_count", "k_cells_prefix", "k_cells_compact", "k_cells_scatter", "k_msm", "k_ntt_pass"):  # the last two: prefixes
        ms, count = C.c_double(), C.c_uint64()
        assert lib.h2mi_profile_query(name.encode(), C.byref(ms), C.byref(count)) == 0
        counts[name] = count.value
    assert lib.h2mi_profile_reset() == 0
    return counts, out


_compact, _expect = K.compact, K.expect  # shared with tests/test_gpu_tile_regimes.py


@pytest.mark.parametrize("log_rows", [5, 11, 13])
def test_compaction_word_for_word(gpu, log_rows):
    """every pattern as a call of its own (1 column), three in one call, and 64 in one call; the host's layout, the forced row list and
    the forced 32-byte words"""
    n_rows = 1 << log_rows
    limit = n_rows - 6
    patterns = K.kernel_patterns(n_rows, limit, seed=log_rows)
    names = list(patterns)
    for name in names:
        assert _compact(gpu, [patterns[name]], n_rows, limit) == [_expect(patterns[name], limit)], name
    three = [patterns[n] for n in ("tile_edges", "empty", "alternating")]
    for flags in (0, 2, 4, 6):
        assert _compact(gpu, three, n_rows, limit, flags) == [_expect(c, limit, flags) for c in three], flags
    many = [patterns[names[i % len(names)]] for i in range(64)]
    assert _compact(gpu, many, n_rows, limit, 2) == [_expect(c, limit, 2) for c in many]
    assert _expect(patterns["just_fits"], limit)[4] == 8 and _expect(patterns["just_not_low"], limit)[4] == 32
    assert _expect(patterns["just_not_high"], limit)[4] == 32 and _expect(patterns["beyond_limit"], limit)[0] == 0


def test_compaction_counts_alone_and_refusals(gpu):
    n_rows, limit = 1 << 11, (1 << 11) - 6
    cells = K.kernel_patterns(n_rows, limit, seed=3)["alternating"]
    buf = gpu.DevBuf.from_numpy(o.pack([cells.get(r, 0) % R for r in range(n_rows)], R))
    arr = (Compacted * 1)()
    arr[0].d_column, arr[0].row_limit = buf.ptr, limit
    counts, rc = _profile(gpu, lambda: gpu.lib.h2mi_fr_compact_cells_dev(arr, 1, 0, None, None, None))
    assert rc == 0 and (arr[0].count, arr[0].last) == K.column_stats(cells, limit)[1:3]
    assert counts == {"k_cells_count": 1, "k_cells_prefix": 1, "k_cells_compact": 0, "k_cells_scatter": 0, "k_msm": 0, "k_ntt_pass": 0}
    assert gpu.lib.h2mi_fr_compact_cells_dev(arr, 65, 0, None, None, None) == EINVAL
    assert gpu.lib.h2mi_fr_compact_cells_dev(arr, 1, 8, None, None, None) == EINVAL
    arr[0].d_column = buf.ptr + 8
    assert gpu.lib.h2mi_fr_compact_cells_dev(arr, 1, 0, None, None, None) == EINVAL
    buf.free()


# ---- keys -----------------------------------------------------------------------------------------------------------------------------
def _build(custom, name):
    if name == "is_zero":
        return (*gate_cases.is_zero_circuit(custom, 5), 5, False)
    if name == "xor":
        return (*lookup_cases.xor_circuit(custom), 5, False)
    if name == "logup":
        return (*logup_cases.build(custom, "xor"), True)
    if name == "merged3":
        return (*logup_sets_cases.build(custom, "range3"), True)
    if name == "shuffles":
        return (*shuffle_cases.build(custom, "mixed"), False)
    if name == "two_phase":
        return (*phase_cases.rlc_circuit(custom), 5, False)
    if name == "eight_instances":
        return (*instance_cases.eight_cols_circuit(custom, 5), 5, False)
    if name == "rational":
        return (*assigned_cases.is_zero_circuit(custom, 7), 5, False)
    raise KeyError(name)


CUSTOM_CIRCUITS = ["is_zero", "xor", "logup", "merged3", "shuffles", "two_phase", "eight_instances", "rational"]


def _commitment_bytes(keys) -> bytes:
    return keys.fixed_commitments.tobytes() + keys.permutation_commitments.tobytes()


@pytest.mark.parametrize("name", CUSTOM_CIRCUITS)
def test_custom_keys_round_trip_with_the_same_bytes_and_proofs(gpu, name, tmp_path):
    """export == the Python writer's bytes and the size formula; export -> release -> import (both layouts, from both layouts) -> the
    same proof bytes for the same seed, SHPLONK and GWC and a batch of two; export(import(b)) == b; the commitments are the stored ones"""
    from halo2_scaffold_amd import custom

    cs, asg, k, logup = _build(custom, name)
    first = shuffle_cases.first_assignment(cs, asg)
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    prove = lambda keys: (custom.create_proof(params, keys, asg, 31), custom.create_proof(params, keys, asg, 9, multiopen="gwc"),
                          custom.prove_many(keys, [asg, asg], seeds=[40, 48], params=params) if not callable(asg) else b"")
    blobs, proofs = [], []
    for by_coset in (False, True):
        keys = custom.Keys(params, cs, first, logup=logup, by_coset=by_coset)
        proofs.append(prove(keys))
        counts, blob = _profile(gpu, lambda: keys.keys.export(b"user bytes"))
        assert counts["k_cells_compact"] == 1 and counts["k_cells_scatter"] == 0  # the length call stops after the counts
        assert keys.keys.export(b"user bytes") == blob
        want_commitments = _commitment_bytes(keys)
        keys.release()
        blobs.append(blob)
    assert blobs[0] == blobs[1] and proofs[0] == proofs[1]
    blob = blobs[0]
    fields, fixed, copies, programs = K.custom_inputs(custom, cs, first, k)
    payloads = K.sections(fields, fixed, K.moved_cells(copies), want_commitments, b"user bytes", **programs)
    assert blob == K.assemble(payloads, K.FLAG_LOGUP if logup else 0) and len(blob) == K.blob_length(payloads)
    path = tmp_path / "key.bin"
    path.write_bytes(blob)
    for by_coset in (False, True):
        keys = custom.Keys.load(params, cs, str(path), by_coset=by_coset)
        assert keys.user == b"user bytes" and keys.logup == logup and _commitment_bytes(keys) == want_commitments
        assert keys.keys.n_shuffles == len(cs.shuffles) and (keys.keys.phases is None) == (cs.phases() is None)
        assert prove(keys) == proofs[0]
        assert keys.keys.export(b"user bytes") == blob
        keys.release()
    params.release()


def test_standard_plonk_golden_round_trip(gpu):
    from halo2_scaffold_amd import circuits, engine, keygen, prover

    gold = json.load(open(os.path.join(GOLD, "standard_plonk_proofs.json")))
    case = [c for c in gold["cases"] if c["k"] == 8][0]
    k, x, seed = case["k"], int(case["witness_x"], 16), case["seed"]
    params = gpu.ParamsKZG.setup(k, int(gold["srs_secret"], 16))
    circuit = circuits.StandardPlonk(None)
    pk = keygen.keygen_pk(params, keygen.keygen_vk(params, circuit), circuit)
    assert prover.create_proof(params, pk, circuits.StandardPlonk(x), seed).hex() == case["proof"]
    blob = pk.keys.export()
    read = K.read_blob(blob)
    assert len(blob) == K.blob_length(read["payloads"]) and read["commitments"] == _commitment_bytes(pk.keys)
    # the Python writer over the circuit's own fixed cells and copies, as keygen was given them
    syn = circuit.without_witnesses().synthesize()
    fixed = [dict(col) if isinstance(col, dict) else dict(enumerate(col)) for col in syn.fixed]
    copies = [(lc, lr, rc, rr) for (lc, lr), (rc, rr) in syn.copies]
    cs = K.cs_fields(pk.keys.cs)
    assert any(fixed) and copies
    assert K.write_blob(cs, fixed, K.moved_cells(copies), _commitment_bytes(pk.keys)) == blob
    inner = pk.keys
    for by_coset in (False, True):
        counts, loaded = _profile(gpu, lambda: engine.Keys.from_blob(params, blob, by_coset=by_coset))
        assert counts["k_cells_compact"] == 0
        pk.keys = loaded
        assert prover.create_proof(params, pk, circuits.StandardPlonk(x), seed).hex() == case["proof"]
        assert prover.create_proof(params, pk, circuits.StandardPlonk(x + 1), seed + 1, multiopen="gwc")
        assert loaded.export() == blob
        loaded.release()
    pk.keys = inner
    pk.release()
    params.release()


def test_flex_range_key_round_trip_through_the_hosts(gpu, tmp_path):
    from halo2_scaffold_amd import flex

    g = json.load(open(os.path.join(GOLD, "flex_proofs.json")))
    case = min((c for c in g["cases"] if c.get("shape") == "range"), key=lambda c: c["k"])
    k, bits, x, seed = case["k"], case["lookup_bits"], int(case["x"], 16), case["seed"]
    cs = flex.FlexGateCS(lookup=True)
    asg = flex.range_closure(cs, x, bits)
    params = gpu.ParamsKZG.setup(k, int(g["srs_secret"], 16))
    keys = flex.FlexKeys(params, cs, asg)
    assert flex.create_proof(params, keys, asg, seed).hex() == case["proof"]
    path = str(tmp_path / "flex.key")
    keys.save(path, b"[[1, 2]]")
    keys.release()
    for by_coset in (False, True):
        loaded = flex.FlexKeys.load(params, path, by_coset=by_coset)
        assert loaded.user == b"[[1, 2]]" and loaded.vk_bytes().hex() == case["vk_bytes"]
        assert flex.create_proof(params, loaded, asg, seed).hex() == case["proof"]
        loaded.release()
    params.release()


def test_refusals_on_the_device_and_the_moved_cells_came_through(gpu, tmp_path):
    from halo2_scaffold_amd import custom, engine

    cs, asg = gate_cases.is_zero_circuit(custom, 5)
    k = 5
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    keys = custom.Keys(params, cs, asg)
    proof = custom.create_proof(params, keys, asg, 31)
    blob = keys.keys.export()
    keys.release()
    vk_only = engine.Keys(cs.abi(k), params, list(asg.fixed), [], vk_only=True, gates=cs.gate_program())
    with pytest.raises(gpu.H2miError) as e:
        vk_only.export()
    assert e.value.code == EINVAL
    vk_only.release()

    def good():
        loaded = custom.Keys.load(params, cs, io.BytesIO(blob))
        assert custom.create_proof(params, loaded, asg, 31) == proof
        loaded.release()

    def refused(p, b, code):
        with pytest.raises(gpu.H2miError) as e:
            engine.Keys.from_blob(p, b)
        assert e.value.code == code

    # one byte flipped inside a cell section, the checksum made right: the structure stands, the commitments do not
    read = K.read_blob(blob)
    col = next(f for f in range(read["n_fixed"]) if read["fixed"][f])
    flipped = bytearray(blob)
    flipped[read["offsets"][5 + col] + 16] ^= 2
    refused(params, K.reseal(bytes(flipped)), EINVAL)
    good()
    other = gpu.ParamsKZG.setup(k, SRS_SECRET + 1)
    refused(other, blob, EINVAL)
    other.release()
    good()
    shorter = gpu.ParamsKZG.setup(k - 1, SRS_SECRET)
    refused(shorter, blob, ERANGE)
    shorter.release()
    good()
    # H2MI_KEYGEN_LOGUP is the blob's, not a flag of the import
    h = C.c_void_p()
    buf = np.frombuffer(blob, dtype=np.uint8)
    rc = gpu.lib.h2mi_prover_pk_import(buf.ctypes.data, buf.nbytes, params.g_lagrange_handle, engine.KEYGEN_LOGUP, C.byref(h))
    assert rc == EINVAL and not h.value
    # a cs that differs in one gate is not the file's
    other_cs, _ = gate_cases.or_circuit(custom, 1, 0)
    with pytest.raises(ValueError):
        custom.Keys.load(params, other_cs, io.BytesIO(blob))
    params.release()


def test_check_on_an_imported_key_still_names_an_unsatisfied_copy_constraint(gpu):
    """the moved cells came through: the device's witness check reports the same copy failure against the imported key"""
    from halo2_scaffold_amd import flex

    cs = flex.FlexGateCS(lookup=False)
    asg = flex.halo2_lib_closure(cs, 5)
    params = gpu.ParamsKZG.setup(7, SRS_SECRET)
    keys = flex.FlexKeys(params, cs, asg)
    buf = io.BytesIO()
    keys.save(buf)
    assert K.read_blob(buf.getvalue())["moved"]
    bad = flex.halo2_lib_closure(cs, 5)
    (kind, col, row) = next(end for pair in bad.copies for end in pair if end[0] == flex.ADVICE)
    bad.advice[col][row] = (bad.advice[col][row] + 1) % R
    messages = []
    for which in ("made", "imported"):
        if which == "imported":
            keys.release()
            keys = flex.FlexKeys.load(params, io.BytesIO(buf.getvalue()))
        with pytest.raises(ValueError) as e:
            flex.check(params, keys, bad, 3)
        messages.append([f.astuple() for f in e.value.failures])
    keys.release()
    params.release()
    assert messages[0] == messages[1] and any(kind == 1 for kind, _, _, _ in messages[0]), messages  # 1: H2MI_CHECK_COPY


def test_scaffold_gen_key_with_a_key_file_never_calls_the_closure_again(gpu, tmp_path, monkeypatch):
    """examples/range.rs through scaffold.gen_key(key_file=): the second call reads the key and the break points and makes no call of
    the closure; the proof against the loaded key is accepted by the in-repo verifier with the same public inputs"""
    from halo2_scaffold_amd import scaffold
    from halo2_scaffold_amd.params import gen_srs_secret
    from oracle import flex as FX

    monkeypatch.setenv("DEGREE", "6")
    monkeypatch.setenv("LOOKUP_BITS", "4")
    monkeypatch.setenv("PARAMS_DIR", str(tmp_path / "params"))
    monkeypatch.delenv("MINIMUM_ROWS", raising=False)
    os.makedirs(tmp_path / "params")
    calls = []

    def range_example(ctx, x, make_public):  # examples/range.rs:10-34
        calls.append(x)
        xc = ctx.load_witness(x)
        make_public.append(xc)
        ctx.range_check(xc, 64, ctx.lookup_bits)
        ctx.add(xc, xc)

    x = 0xDEADBEEFCAFE1234
    path = str(tmp_path / "range.key")
    pk, bp = scaffold.gen_key(range_example, 0, key_file=path)
    assert len(calls) > 0 and os.path.exists(path)
    public = scaffold.prove_private(range_example, x, pk, bp)
    pk.release()
    calls.clear()
    pk2, bp2 = scaffold.gen_key(range_example, 0, key_file=path)
    assert calls == [] and bp2 == bp
    assert scaffold.prove_private(range_example, x, pk2, bp2) == public == [x]
    ocs = FX.flex_gate_cs(True)
    oasg = FX.range_assignment(ocs, x, 4, 64)
    vk = FX.VerifierKeys(ocs, 6, gen_srs_secret(), oasg.fixed, oasg.copies)
    assert pk2.get_vk().transcript_repr == vk.transcript_repr
    assert FX.verify(vk, pk2.last_proof, [[x]]) and not FX.verify(vk, pk2.last_proof, [[x + 1]])
    pk2.release()
    # a key made under another LOOKUP_BITS is refused, not loaded
    calls.clear()
    monkeypatch.setenv("LOOKUP_BITS", "5")
    with pytest.raises(ValueError):
        scaffold.gen_key(range_example, 0, key_file=path)
    assert calls == []


def test_import_takes_the_scatter_launch_and_issues_no_more_msms_and_transforms_than_keygen(gpu):
    """a range key whose table column is 32 dense int64 cells: import hands it to k_cells_scatter (the route the compaction is the
    inverse of), and the launch profile of the import shows no more MSM and transform launches than keygen of the same key does"""
    from halo2_scaffold_amd import flex

    k, bits = 8, 5
    cs = flex.FlexGateCS(lookup=True)
    asg = flex.range_closure(cs, 0x1234567, bits)
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    flex.FlexKeys(params, cs, asg).release()  # tables and plans are built by the first use of the SRS: not what is compared
    for by_coset in (False, True):
        made, keys = _profile(gpu, lambda: flex.FlexKeys(params, cs, asg, by_coset=by_coset))
        proof = flex.create_proof(params, keys, asg, 5)
        buf = io.BytesIO()
        keys.save(buf)
        keys.release()
        read = K.read_blob(buf.getvalue())
        assert sorted(len(col) for col in read["fixed"])[-1] >= 31  # the table 0 .. 31: dense, more than the 16 cells that ride in a patch
        imported, loaded = _profile(gpu, lambda: flex.FlexKeys.load(params, io.BytesIO(buf.getvalue()), by_coset=by_coset))
        assert imported["k_cells_scatter"] >= 1 and imported["k_cells_compact"] == 0
        assert 0 < imported["k_msm"] <= made["k_msm"] and 0 < imported["k_ntt_pass"] <= made["k_ntt_pass"], (made, imported)
        assert flex.create_proof(params, loaded, asg, 5) == proof
        loaded.release()
    params.release()


def test_cpp_example_reads_its_key_file_and_reproduces_the_python_hosts_proof(gpu, tmp_path):
    """examples/key_file.cpp: keygen, write, read into a fresh key, prove — the bytes of the Python host's proof for the same seed"""
    from halo2_scaffold_amd import circuits, keygen, prover

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "examples"), "-s", "key_file"])
    k, secret, x, seed = 5, 0x5EC2E7, 0xC0FFEE, 11
    path = tmp_path / "standard_plonk.key"
    r = subprocess.run([os.path.join(root, "examples", "key_file"), str(path), str(k), hex(secret), hex(x), str(seed)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "same_as_the_generated_key 1" in r.stdout, (r.stdout[-300:], r.stderr[-500:])
    cpp_proof = next(l.split()[1] for l in r.stdout.splitlines() if l.startswith("proof "))
    params = gpu.ParamsKZG.setup(k, secret)
    circuit = circuits.StandardPlonk(None)
    pk = keygen.keygen_pk(params, keygen.keygen_vk(params, circuit), circuit)
    assert prover.create_proof(params, pk, circuits.StandardPlonk(x), seed).hex() == cpp_proof
    assert pk.keys.export() == path.read_bytes()  # and the C++ host wrote the file the Python host writes
    pk.release()
    params.release()


def test_a_key_made_from_integer_fixed_columns_exports_the_same_file_and_round_trips(gpu):
    """the StandardPlonk key at k = 8 with its fixed columns handed to keygen as int64 cells (engine.IntCells): the same file as the key
    made from field elements, and the imported key gives the committed golden proof, the GWC ending and a batch of two as the made key"""
    from halo2_scaffold_amd import circuits, engine, keygen, prover

    gold = json.load(open(os.path.join(GOLD, "standard_plonk_proofs.json")))
    case = [c for c in gold["cases"] if c["k"] == 8][0]
    k, x, seed = case["k"], int(case["witness_x"], 16), case["seed"]
    params = gpu.ParamsKZG.setup(k, int(gold["srs_secret"], 16))
    circuit = circuits.StandardPlonk(None)
    syn = circuit.without_witnesses().synthesize()
    fixed = [dict(col) if isinstance(col, dict) else dict(enumerate(col)) for col in syn.fixed]
    copies = [(lc, lr, rc, rr) for (lc, lr), (rc, rr) in syn.copies]
    assert all(K.fits64(v % R) for col in fixed for v in col.values() if v % R)
    ints = [engine.IntCells(np.array([K.to_i64(col[r] % R) for r in sorted(col)], dtype=np.int64), rows=np.array(sorted(col), dtype=np.uint32))
            for col in fixed]
    abi = keygen.constraint_system(circuit, k)
    vk = keygen.keygen_vk(params, circuit)
    from_ints = engine.Keys(abi, params, ints, copies)
    from_words = engine.Keys(abi, params, syn.fixed, copies)
    blob = from_ints.export()
    assert blob == from_words.export()
    from_words.release()

    def proofs(keys):
        pk = keygen.ProvingKey(vk, circuit, keys)
        single = prover.create_proof(params, pk, circuits.StandardPlonk(x), seed)
        gwc = prover.create_proof(params, pk, circuits.StandardPlonk(x), seed, multiopen="gwc")
        provers = [engine.Prover(keys, params) for _ in range(2)]
        batch = engine.Batch(provers)
        try:
            from halo2_scaffold_amd.transcript import Blake2bWrite

            tr = Blake2bWrite.init()
            tr.common_scalar(keygen._m(vk.transcript_repr))  # vk.hash_into
            advices = [circuits.StandardPlonk(x + i).synthesize().advice for i in range(2)]
            batch.drive(advices, [[], []], [seed, seed + 8], tr)
            both = tr.finalize()
        finally:
            batch.release()
            for p in provers:
                p.release()
        return single, gwc, both

    want = proofs(from_ints)
    assert want[0].hex() == case["proof"]
    from_ints.release()
    for by_coset in (False, True):
        loaded = engine.Keys.from_blob(params, blob, by_coset=by_coset)
        assert proofs(loaded) == want
        loaded.release()
    params.release()
