"""Several instance columns on the device (include/h2mi_prover.h h2mi_prover_instances; tests/instance_cases.py): the multi-column coset
kernel word for word against the single-column one and against Python integers; the quotient kernels (k_evaluate_h_expr,
k_evaluate_h_expr_batch) with eight instance columns, recovered from H2MI_BUF_H on every extended-coset point; proofs byte for byte against
oracle.flex.prove, accepted by both verifiers and rejected after a change of any column or a flipped byte; the two routes of a one-column
key; the witness check's report through an instance column; the refusals; which kernels ran, from the launch profile."""
import ctypes as C
import types

import numpy as np
import pytest

import custom_gate_cases as gate_cases
import instance_cases as cases
from oracle import bn254 as o
from oracle import flex as FX

pytestmark = pytest.mark.gpu

R = o.R
SRS_SECRET = 0x5EC2E7 + 0x48324D49
EINVAL, ERANGE = -1, -6


def _vals(buf, count):
    return o.unpack(buf.to_numpy(shape=(count, 4), nbytes=count * 32), R)


def _limbs(values):
    from halo2_scaffold_amd import field as F

    return np.ascontiguousarray(np.stack([F.fr_to_mont_limbs(v % R) for v in values])) if len(values) else np.zeros((1, 4), dtype=np.uint64)


def _flipped(proof: bytes, at: int) -> bytes:
    out = bytearray(proof)
    out[at] ^= 1
    return bytes(out)


def _launches(lib, call):
    """(k_instance_coset launches, k_instance_coset_multi launches) during call(), from the library's launch profile (a query is by
    prefix: the first name counts both kernels)"""
    assert lib.h2mi_profile_reset() == 0 and lib.h2mi_profile_filter(b"") == 0 and lib.h2mi_profile_enable(1) == 0
    try:
        call()
    finally:
        assert lib.h2mi_profile_enable(0) == 0
    ms, both, multi = C.c_double(), C.c_uint64(), C.c_uint64()
    assert lib.h2mi_profile_query(b"k_instance_coset", C.byref(ms), C.byref(both)) == 0
    assert lib.h2mi_profile_query(b"k_instance_coset_multi", C.byref(ms), C.byref(multi)) == 0
    assert lib.h2mi_profile_reset() == 0
    return both.value - multi.value, multi.value


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------------
def _multi(lib, d_l0, k, ext_k, columns, outs):
    n = len(columns)
    keep = [_limbs(col) for col in columns]
    vals = (C.c_void_p * n)(*[a.ctypes.data if len(col) else None for a, col in zip(keep, columns)])
    counts = (C.c_size_t * n)(*[len(col) for col in columns])
    ptrs = (C.c_void_p * n)(*[b.ptr for b in outs])
    return lib.h2mi_plonk_instance_coset_multi_dev(d_l0.ptr, k, ext_k, vals, counts, n, ptrs, None)


@pytest.mark.parametrize("k,degree", [(5, 5), (6, 9)])  # (k, extended_k) = (5, 7) and (6, 9): rot = 4 and 8, one and two workgroups
def test_multi_column_coset_against_the_single_kernel_and_python_integers(gpu, k, degree):
    from halo2_scaffold_amd.device import DevBuf

    lib = gpu.lib
    d = o.Domain(k, degree)
    assert d.extended_k == {5: 7, 6: 9}[k]
    n, ext = 1 << k, 1 << d.extended_k
    u = n - 6
    counts = cases.eight_cols_counts(u)
    columns = cases.extreme_columns(counts, 8400 + k)
    for col in columns[1:]:
        assert set(cases.EXTREMES[: len(col)]) <= set(col)
    want = [cases.instance_coset(d, col) for col in columns]
    l0 = cases.instance_coset(d, [1])
    d_l0 = DevBuf.from_numpy(o.pack(l0, R))
    short = [c for c in range(8) if counts[c] <= 16]
    assert short == [0, 1, 2, 3, 4, 5]
    # the six short columns of eight_cols in one launch, the outputs prefilled with something else
    outs = [DevBuf.from_numpy(o.pack([7] * ext, R)) for _ in short]
    assert _multi(lib, d_l0, k, d.extended_k, [columns[c] for c in short], outs) == 0
    single = DevBuf(ext * 32)
    for c, out in zip(short, outs):
        assert _vals(out, ext) == want[c], f"column {c}: {counts[c]} values"
        vl = _limbs(columns[c])
        assert lib.h2mi_plonk_instance_coset_dev(d_l0.ptr, k, d.extended_k, vl.ctypes.data, counts[c], single.ptr, None) == 0
        assert np.array_equal(out.to_numpy(shape=(ext, 4)), single.to_numpy(shape=(ext, 4))), f"column {c}: words differ from k_instance_coset's"
    # all eight slots of the tile taken, every column at the most the kernel takes or at an odd count
    full = cases.extreme_columns([16, 16, 5, 16, 1, 16, 13, 16], 8500 + k)
    outs8 = [DevBuf(ext * 32) for _ in full]
    assert _multi(lib, d_l0, k, d.extended_k, full, outs8) == 0
    for c, out in enumerate(outs8):
        assert _vals(out, ext) == cases.instance_coset(d, full[c]), c
        vl = _limbs(full[c])
        assert lib.h2mi_plonk_instance_coset_dev(d_l0.ptr, k, d.extended_k, vl.ctypes.data, len(full[c]), single.ptr, None) == 0
        assert np.array_equal(out.to_numpy(shape=(ext, 4)), single.to_numpy(shape=(ext, 4))), c
    # the 17-value and the full-length column: the transform route (what the prover runs for them) gives the same reference
    dom = gpu.EvaluationDomain(degree, k)
    coeff, coset = DevBuf(n * 32), DevBuf(ext * 32)
    for c in (6, 7):
        rows = DevBuf.from_numpy(o.pack(columns[c] + [0] * (n - counts[c]), R))
        dom.lagrange_to_coeff_oop_dev(rows, coeff)
        dom.coeff_to_extended_oop_dev(coeff, coset)
        assert _vals(coset, ext) == want[c], c
        rows.free()
    # refusals: a 17th value, nine columns, a missing output
    assert _multi(lib, d_l0, k, d.extended_k, [columns[6]], outs[:1]) == EINVAL
    assert _multi(lib, d_l0, k, d.extended_k, [[1]] * 9, outs + outs8[:3]) == EINVAL
    assert lib.h2mi_plonk_instance_coset_multi_dev(d_l0.ptr, k, d.extended_k, None, None, 1, None, None) == EINVAL
    for b in outs + outs8 + [single, coeff, coset, d_l0]:
        b.free()


# ---- helpers: keys, and a proof's vectors in Python integers --------------------------------------------------------------------------
def _keys(gpu, cs, first, k, name, logup=False):
    from halo2_scaffold_amd import custom

    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    keys = custom.Keys(params, cs, first, logup=logup)
    ocs = cases.oracle_cs(cs, name)
    oasg = cases.oracle_assignment(ocs, cs, first)
    vk = FX.VerifierKeys(ocs, k, SRS_SECRET, oasg.fixed, oasg.copies)
    assert o.unpack_points(keys.fixed_commitments) == vk.fixed_commitments and keys.transcript_repr == vk.transcript_repr
    return custom, params, keys, vk


def _release(params, keys, *ws):
    for w in ws:
        w.release()
    keys.release()
    params.release()


def _case(gpu, name, logup=False):
    from halo2_scaffold_amd import custom

    cs, asg, k = cases.build(custom, name)
    first = cases.first_assignment(cs, asg)
    custom_, params, keys, vk = _keys(gpu, cs, first, k, name, logup)
    return custom_, cs, asg, first, k, params, keys, vk


def _check_quotient(cs, keys, provers, asgs, k, trace):
    """instance_cases.check_quotient (every extended-coset point of H2MI_BUF_H, the instance buffers), then what is particular to these
    circuits: every instance column is in h"""
    from halo2_scaffold_amd import engine

    assert not cs.lookups and not cs.shuffles
    built, args, tail, want = cases.check_quotient(cs, keys, provers, asgs, k, trace)
    size = len(want)
    # every column is in h: with any one of them zeroed the reference is another vector
    for c in range(cs.n_instance):
        if not any(built[0][0]["instance"][c]):
            continue
        zeroed = [dict(b[0], instance=[col if j != c else [0] * size for j, col in enumerate(b[0]["instance"])]) for b in built]
        assert cases.batched_quotient(*args, zeroed, *tail) != want, c
    with pytest.raises(Exception):
        provers[0].views(engine.BUF_INSTANCE, cs.n_instance + 1)[cs.n_instance]


# ---- 2. the quotient --------------------------------------------------------------------------------------------------------------------
def test_quotient_with_eight_instance_columns_single(gpu):
    """k_evaluate_h_expr: every extended-coset point against Python integers"""
    custom, cs, asg, first, k, params, keys, vk = _case(gpu, "eight_cols")
    ws = custom.Workspace(params, keys)
    trace = {}
    proof = custom.create_proof(params, keys, asg, 21, trace=trace, ws=ws)
    assert cases.verify_circuits(vk, cs, proof, [cases.columns_of(cs, asg)])
    _check_quotient(cs, keys, [ws.prover], [asg], k, trace)
    _release(params, keys, ws)


def test_quotient_with_eight_instance_columns_batch(gpu):
    """k_evaluate_h_expr_batch on two circuits whose public inputs differ: one accumulator over both circuits' terms, each circuit
    reading its own eight columns"""
    from halo2_scaffold_amd import custom

    built = [cases.eight_cols_circuit(custom, 5, variant=v) for v in (0, 1)]
    cs, asgs = built[0][0], [a for _, a in built]
    assert asgs[0].instance != asgs[1].instance
    _, params, keys, vk = _keys(gpu, cs, asgs[0], 5, "eight_cols")
    ws = custom.BatchWorkspace(params, keys, 2)
    trace = {}
    proof = custom.prove_many(keys, asgs, seeds=[5, 13], ws=ws, trace=trace)
    assert cases.verify_circuits(vk, cs, proof, [cases.columns_of(cs, a) for a in asgs])
    _check_quotient(cs, keys, ws.provers, asgs, 5, trace)
    _release(params, keys, ws)


# ---- 3. proofs ------------------------------------------------------------------------------------------------------------------------
def _tampering_is_rejected(vk, cs, proof, instances, **how):
    """one value of each instance column of each circuit in turn; one byte of the proof at four places"""
    assert cases.verify_circuits(vk, cs, proof, instances, **how)
    for i, columns in enumerate(instances):
        for c in range(cs.n_instance):
            changed = [cases.tampered(cols, c) if j == i else cols for j, cols in enumerate(instances)]
            assert not cases.verify_circuits(vk, cs, proof, changed, **how), (i, c)
    for at in (5, len(proof) // 3, 2 * len(proof) // 3 + 1, len(proof) - 1):
        assert not cases.verify_circuits(vk, cs, _flipped(proof, at), instances, **how), at


@pytest.mark.parametrize("name", ["two_cols", "eight_cols"])
def test_proofs_are_the_oracles_byte_for_byte(gpu, name):
    """oracle.flex.prove with the same seed, Python host: the same bytes; accepted by oracle.flex.verify and by the generalised verifier"""
    custom, cs, asg, first, k, params, keys, vk = _case(gpu, name)
    ocs = cases.oracle_cs(cs, name)
    oasg = cases.oracle_assignment(ocs, cs, asg)
    okeys = FX.Keys(ocs, k, SRS_SECRET, oasg.fixed, oasg.copies)
    ws = custom.Workspace(params, keys)
    seed = 11
    proof = custom.create_proof(params, keys, asg, seed, ws=ws)
    assert proof == FX.prove(okeys, oasg, seed)["proof"]
    columns = cases.columns_of(cs, asg)
    assert len(columns) == cs.n_instance == {"two_cols": 2, "eight_cols": 8}[name]
    assert FX.verify(okeys, proof, columns) and FX.verify(vk, proof, columns)
    assert not FX.verify(vk, proof, cases.tampered(columns, cs.n_instance - 1))
    _tampering_is_rejected(vk, cs, proof, [columns])
    # a second proof on the same prover, and a batch of one: the same bytes
    assert custom.create_proof(params, keys, asg, seed, ws=ws) == proof
    assert custom.prove_many(keys, [asg], seeds=[seed]) == proof
    _release(params, keys, ws)


@pytest.mark.parametrize("logup", [False, True])
def test_instance_columns_inside_a_lookup_a_shuffle_and_a_phased_gate(gpu, logup):
    custom, cs, asg, first, k, params, keys, vk = _case(gpu, "in_arguments", logup)
    assert cs.n_instance == 3 and len(cs.lookups) == 1 and len(cs.shuffles) == 1 and cs.n_phases == 2
    ws = custom.Workspace(params, keys)
    custom.check(params, keys, asg, ws=ws)  # nothing to report
    proof = custom.create_proof(params, keys, asg, 31, ws=ws)
    _tampering_is_rejected(vk, cs, proof, [cases.columns_of(cs, first)], logup=logup)
    assert not cases.verify_circuits(vk, cs, proof, [cases.columns_of(cs, first)], logup=not logup)
    _release(params, keys, ws)


def test_batch_of_two_and_the_gwc_ending(gpu):
    from halo2_scaffold_amd import custom

    built = [cases.two_cols_circuit(custom, variant=v) for v in (0, 1)]
    cs, asgs = built[0][0], [a for _, a in built]
    _, params, keys, vk = _keys(gpu, cs, asgs[0], 5, "two_cols")
    ws = custom.BatchWorkspace(params, keys, 2)
    proof = custom.prove_many(keys, asgs, seeds=[40, 48], ws=ws)
    instances = [cases.columns_of(cs, a) for a in asgs]
    assert instances[0] != instances[1]
    _tampering_is_rejected(vk, cs, proof, instances)
    assert not cases.verify_circuits(vk, cs, proof, instances[::-1]) and not cases.verify_circuits(vk, cs, proof, instances[:1])
    single = custom.Workspace(params, keys)
    gwc = custom.create_proof(params, keys, asgs[0], 9, ws=single, multiopen="gwc")
    _tampering_is_rejected(vk, cs, gwc, instances[:1], multiopen="gwc")
    assert not cases.verify_circuits(vk, cs, gwc, instances[:1])
    _release(params, keys, ws, single)


# ---- 4. a key with one instance column ----------------------------------------------------------------------------------------------------
def test_one_column_key_takes_both_routes(gpu):
    """degree6_circuit: the public inputs through h2mi_prover_instances give the bytes they give through the advice call's argument,
    which are the oracle's; the values hold for one proof only"""
    from halo2_scaffold_amd import custom, engine

    lib = gpu.lib
    cs, asg = gate_cases.degree6_circuit(custom, 3, 7)
    k = 5
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    keys = custom.Keys(params, cs, asg)
    ocs = gate_cases.oracle_cs(cs, "degree6")
    oasg = gate_cases.oracle_assignment(ocs, asg)
    okeys = FX.Keys(ocs, k, SRS_SECRET, oasg.fixed, oasg.copies)
    ws = custom.Workspace(params, keys)
    seed = 17
    old = {}
    old["counts"] = _launches(lib, lambda: old.update(proof=custom.create_proof(params, keys, asg, seed, ws=ws)))
    assert old["proof"] == FX.prove(okeys, oasg, seed)["proof"]
    assert old["counts"] == (1, 0)  # the launch a one-column key has always had
    by_columns = types.SimpleNamespace(advice=asg.advice, instance=[list(asg.instance)])  # a list of columns: h2mi_prover_instances
    new = {}
    new["counts"] = _launches(lib, lambda: new.update(proof=custom.create_proof(params, keys, by_columns, seed, ws=ws)))
    assert new["proof"] == old["proof"] and new["counts"] == (1, 0)
    n = 1 << k
    assert _vals(ws.prover.view(engine.BUF_INSTANCE), n) == list(asg.instance) + [0] * (n - len(asg.instance))
    # the next proof on the same prover, started without public inputs by either route, does not see them
    pts = np.zeros((8, 8), dtype=np.uint64)
    none = np.zeros((1, 4), dtype=np.uint64)
    cells, keep = engine.pack_cells(asg.advice)
    assert lib.h2mi_prover_advice(ws.prover.handle, cells, none.ctypes.data, 0, seed, pts.ctypes.data) == 0
    assert _vals(ws.prover.view(engine.BUF_INSTANCE), n) == [0] * n
    # both routes for one proof: refused by the advice call, and the values are gone with the refusal
    ws.prover.set_instances([list(asg.instance)])
    vl = _limbs(asg.instance)
    assert lib.h2mi_prover_advice(ws.prover.handle, cells, vl.ctypes.data, len(asg.instance), seed, pts.ctypes.data) == EINVAL
    assert lib.h2mi_prover_advice(ws.prover.handle, cells, vl.ctypes.data, len(asg.instance), seed, pts.ctypes.data) == 0
    del keep
    assert custom.create_proof(params, keys, asg, seed, ws=ws) == old["proof"]
    _release(params, keys, ws)


# ---- 5. the witness check and the refusals ---------------------------------------------------------------------------------------------------
def test_check_reports_through_instance_columns(gpu):
    from halo2_scaffold_amd import custom, engine

    cs, good = cases.two_cols_circuit(custom)
    _, bad = cases.two_cols_circuit(custom, bad="copy1")
    _, params, keys, vk = _keys(gpu, cs, good, 5, "two_cols")
    ws = custom.Workspace(params, keys)
    custom.check(params, keys, good, ws=ws)
    with pytest.raises(ValueError, match="copy constraint at cell") as e:
        custom.check(params, keys, bad, ws=ws)
    (kind, index, row, count), = [f.astuple() for f in e.value.failures]
    assert kind == engine.CHECK_COPY and count == 2 and cs.perm_columns[index] + (row,) in {("advice", 0, 7), ("instance", 1, 2)}
    _release(params, keys, ws)
    cs, good = cases.eight_cols_circuit(custom)
    _, params, keys, vk = _keys(gpu, cs, good, 5, "eight_cols")
    ws = custom.Workspace(params, keys)
    custom.check(params, keys, good, ws=ws)
    with pytest.raises(ValueError, match="gate 'all eight' not satisfied at row 9") as e:
        custom.check(params, keys, cases.eight_cols_circuit(custom, bad="gate5")[1], ws=ws)
    assert [f.astuple() for f in e.value.failures] == [(engine.CHECK_GATE, 0, 9, 1)]
    with pytest.raises(ValueError, match="copy constraint at cell") as e:
        custom.check(params, keys, cases.eight_cols_circuit(custom, bad="copy5")[1], ws=ws)
    (kind, index, row, count), = [f.astuple() for f in e.value.failures]
    assert kind == engine.CHECK_COPY and count == 2 and cs.perm_columns[index] + (row,) in {("advice", 1, 1), ("instance", 5, 4)}
    # and the prover proves the good witness afterwards
    proof = custom.create_proof(params, keys, good, 3, ws=ws)
    assert cases.verify_circuits(vk, cs, proof, [cases.columns_of(cs, good)])
    _release(params, keys, ws)


def test_refusals_leave_the_prover_usable(gpu):
    from halo2_scaffold_amd import custom, engine

    lib = gpu.lib
    cs, asg = cases.two_cols_circuit(custom)
    k = 5
    _, params, keys, vk = _keys(gpu, cs, asg, k, "two_cols")
    ws = custom.Workspace(params, keys)
    want = custom.create_proof(params, keys, asg, 23, ws=ws)
    h = ws.prover.handle
    u = (1 << k) - (cs.blinding_factors() + 1)
    columns = cases.columns_of(cs, asg)
    pts = np.zeros((8, 8), dtype=np.uint64)
    adv, keep_adv = engine.pack_cells(asg.advice)

    def instances(cols, rows_for=None):
        cells, keep = engine.pack_cells(cols)
        if rows_for is not None:
            r = np.arange(len(cols[rows_for]), dtype=np.uint32)
            keep.append(r)
            cells[rows_for].rows = r.ctypes.data
        rc = lib.h2mi_prover_instances(h, cells)
        del keep
        return rc

    assert instances([columns[0], [1] * (u + 1)]) == ERANGE  # InstanceTooLarge
    assert instances([[1] * u, [2] * u]) == 0                # the usable rows themselves are fine
    assert instances(columns, rows_for=1) == EINVAL          # rows != NULL
    assert lib.h2mi_prover_instances(h, None) == EINVAL
    assert instances([columns[0], [R]]) == EINVAL            # a canonical value that is not reduced
    # values through the advice call's argument on a key with two columns
    vl = _limbs(columns[0])
    assert lib.h2mi_prover_advice(h, adv, vl.ctypes.data, len(columns[0]), 23, pts.ctypes.data) == EINVAL
    # both routes for one proof
    assert instances(columns) == 0
    assert lib.h2mi_prover_advice(h, adv, vl.ctypes.data, len(columns[0]), 23, pts.ctypes.data) == EINVAL
    # the refused call took the columns with it: this proof has empty columns, and its witness does not satisfy the circuit
    assert lib.h2mi_prover_advice(h, adv, None, 0, 23, pts.ctypes.data) == 0
    assert [f.kind for f in ws.prover.check()] == [engine.CHECK_GATE, engine.CHECK_COPY]
    del keep_adv
    assert custom.create_proof(params, keys, asg, 23, ws=ws) == want
    assert cases.verify_circuits(vk, cs, want, [columns])
    _release(params, keys, ws)


# ---- 6. routing ---------------------------------------------------------------------------------------------------------------------------
def test_eight_columns_run_the_multi_column_kernel(gpu):
    """eight_cols: the six columns of at most 16 values in ONE k_instance_coset_multi launch, no single-column launch (the other two
    are transformed); two_cols: its two columns in one launch as well"""
    lib = gpu.lib
    for name in ("eight_cols", "two_cols"):
        custom, cs, asg, first, k, params, keys, vk = _case(gpu, name)
        ws = custom.Workspace(params, keys)
        out = {}
        counts = _launches(lib, lambda: out.update(proof=custom.create_proof(params, keys, asg, 2, ws=ws)))
        assert counts == (0, 1), name
        assert cases.verify_circuits(vk, cs, out["proof"], [cases.columns_of(cs, asg)])
        _release(params, keys, ws)
