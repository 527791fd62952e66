"""Proofs of the circuits of tests/limit_cases.py — constraint systems AT every limit of the prover ABI — made on the device and
accepted by the restated verifier of tests/logup_sets_cases.py, which handles gates, plain and logUp lookups (merged), shuffles,
phases and N circuits.  Per shape: the device key's fixed commitments and transcript_repr equal the oracle's; `custom.check` reports
nothing for the witness; the verifier accepts the proof and rejects it after a one-byte flip in every part it has (limit_cases.proof_layout); a
second proof with the same seed through the same workspace is the first byte for byte (stale scratch, the power-table cache after
evictions).  From the launch profile: the rotation shapes run one division per point of a set of five or more points (kate_chain's
chain); rot_many, whose 72 power tables exceed the cache, builds tables again in a repeated proof at the same points; `signed` runs
the sort's full re-sort, and its M and phi equal the Python integers on all usable rows.
Every comparison is exact."""
import ctypes as C

import pytest

import custom_gate_cases as gate_cases
import limit_cases as cases
import logup_sets_cases as verifier
from lookup_expr_cases import compress
from oracle import bn254 as o
from oracle import flex as FX

pytestmark = pytest.mark.gpu

R = o.R
SRS_SECRET = 0x5EC2E7 + 0x48324D49
SEED = 33
ROTATION_SHAPES = ("rot5", "rot8", "rot16", "rot17", "rot_many")


def _vals(buf, count):
    return o.unpack(buf.to_numpy(shape=(count, 4), nbytes=count * 32), R)


def _flipped(proof: bytes, at: int) -> bytes:
    out = bytearray(proof)
    out[at] ^= 1
    return bytes(out)


def _keys(gpu, cs, first, k, name, logup):
    """device keys and an independent verifying key from the oracle, as tests/test_gpu_logup_sets.py makes them"""
    from halo2_scaffold_amd import custom

    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    keys = custom.Keys(params, cs, first, logup=logup)
    ocs = gate_cases.oracle_cs(cs, name)
    oasg = gate_cases.oracle_assignment(ocs, first)
    vk = FX.VerifierKeys(ocs, k, SRS_SECRET, oasg.fixed, oasg.copies)
    assert o.unpack_points(keys.fixed_commitments) == vk.fixed_commitments and keys.transcript_repr == vk.transcript_repr
    return params, keys, vk


def _launches(gpu, call, names) -> dict:
    """kernel -> launches during call(), from the library's launch profile (tests/test_gpu_permutation.py)"""
    lib = gpu.lib
    assert lib.h2mi_profile_reset() == 0 and lib.h2mi_profile_filter(b"") == 0 and lib.h2mi_profile_enable(1) == 0
    try:
        call()
    finally:
        assert lib.h2mi_profile_enable(0) == 0
    ms, count = C.c_double(), C.c_uint64()
    out = {}
    for name in tuple(names) + ("",):
        assert lib.h2mi_profile_query(name.encode(), C.byref(ms), C.byref(count)) == 0
        out[name] = count.value
    assert lib.h2mi_profile_reset() == 0
    assert out.pop("") > 0  # the profile did record this call's launches
    return out


@pytest.mark.parametrize("name", list(cases.SHAPES))
def test_a_system_at_its_limit_proves_and_verifies(gpu, name):
    from halo2_scaffold_amd import custom, engine

    cs, witness, k, logup = cases.build(custom, name)
    first = cases.first_assignment(cs, witness)
    params, keys, vk = _keys(gpu, cs, first, k, name, logup)
    many = isinstance(witness, list)
    witnesses = witness if many else [witness]
    N = len(witnesses)
    instances = [list((w([None] * len(cs.challenge_phase)) if callable(w) else w).instance) for w in witnesses]
    ws = custom.BatchWorkspace(params, keys, N) if many else custom.Workspace(params, keys)
    check_ws = custom.Workspace(params, keys) if many else ws
    for w in witnesses:
        custom.check(params, keys, w, ws=check_ws)  # raises on the first violation
    trace = {}
    seeds = [SEED + 8 * i for i in range(N)]
    if many:
        prove = lambda tr=None: custom.prove_many(keys, witnesses, seeds=seeds, ws=ws, trace=tr)
    else:
        prove = lambda tr=None: custom.create_proof(params, keys, witness, SEED, ws=ws, trace=tr)
    kernels = ("k_kate_local", "k_pow_table", "k_su_iota", "k_fr_add_head")
    proofs = []
    launches = _launches(gpu, lambda: proofs.append(prove(trace)), kernels)
    proof = proofs[0]
    print(name, "first proof", launches, len(proof), "bytes")
    assert len(proof) == cases.proof_length(cs, N, logup)
    assert verifier.verify_circuits(vk, cs, proof, instances, logup)
    at = cases.proof_layout(cs, N, logup, len(proof))
    for part in sorted(at):  # every part the proof has
        assert not verifier.verify_circuits(vk, cs, _flipped(proof, at[part] + 1), instances, logup), part
    # the same seed through the same workspace: the same bytes
    again = _launches(gpu, lambda: proofs.append(prove()), kernels)
    print(name, "second proof", again)
    assert proofs[1] == proof
    if name in ROTATION_SHAPES:
        # one division per point of every set of five or more points (and of one), one round for a set of two to four, the opening
        assert launches["k_kate_local"] == again["k_kate_local"] == cases.expected_divisions(cs, logup)
        sets = cases.opening_sets(cs, logup)
        slices = lambda points: -(-points // cases.HEAD_SLICE)  # a remainder's head goes to the device sixteen coefficients at a time
        assert launches["k_fr_add_head"] == sum(slices(len(s)) for s in sets) + slices(max(map(len, sets)))
    if name == "rot_many":
        # the repeated proof opens at the points of the first and still builds power tables: the 72 tables of its opening points and
        # their inverses do not fit the cache, whatever it held before — it evicted inside the proof
        assert again["k_pow_table"] > 0 and 2 * len(set().union(*sets)) > 64
    if name == "signed":
        assert launches["k_su_iota"] > 0 and again["k_su_iota"] > 0  # the table's sort ran its full re-sort, in both proofs
        n, u = 1 << k, cases.usable_rows(cs, k)
        (in_sets, table), = verifier.argument_rows(cs, first, k)
        squeeze = lambda rows: [compress(t, trace["theta"]) for t in rows]
        a_sets, s_rows = [squeeze(rows) for rows in in_sets], squeeze(table)
        want_m, absent = verifier.multiplicities(a_sets, s_rows, u)
        assert not absent and max(want_m) > 200 and want_m.count(0) > 500 and len(a_sets) == 2
        assert _vals(ws.prover.views(engine.BUF_LOGUP_M, 1)[0], n)[:u] == want_m
        assert _vals(ws.prover.views(engine.BUF_LOGUP_PHI, 1)[0], n)[: u + 1] == verifier.running_sum(a_sets, s_rows, want_m, trace["beta"], u)
    ws.release()
    if many:
        check_ws.release()
    keys.release()
    params.release()
