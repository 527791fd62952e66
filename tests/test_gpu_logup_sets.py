"""LogUp lookups with several input sets over one table on the device, bit for bit against the Python integers of
tests/logup_sets_cases.py: the multiplicity column of K input columns (h2mi_plonk_logup_multiplicity_sets_dev) and the running sum
(h2mi_plonk_logup_sum_sets_dev) around the ranking kernel's 1024-thread workgroup and the scan tile, K = 2, 3, 6; the quotient kernels
with the K-input term, recovered from H2MI_BUF_H on every extended-coset point, and the quotient calls with `logup` NULL against all ones word
for word; proofs of every merged circuit accepted by the generalised verifier and rejected after one-byte flips; proof lengths and the
merged M column against the unmerged key's; a key made with an h2mi_logup_inputs of all counts 1 against tests/golden/logup_proofs.json;
an absent cell of one set in the check and in the lookups phase; the committed golden."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

import custom_gate_cases as gate_cases
import logup_cases
import logup_sets_cases as cases
from lookup_expr_cases import compress
from oracle import bn254 as o
from oracle import flex as FX

pytestmark = pytest.mark.gpu

R = o.R
SRS_SECRET = 0x5EC2E7 + 0x48324D49
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (k, usable rows): one wavefront's worth; both sides of the ranking kernel's 1024-thread workgroup, which is also the tile of the
# multiplicative chain and of the additive scan; eight tiles with a ragged last one
SIZES = [(5, 22), (11, 1023), (11, 1024), (11, 1025), (13, (1 << 13) - 7)]
SETS = [2, 3, 6]


def _vals(buf, count):
    return o.unpack(buf.to_numpy(shape=(count, 4), nbytes=count * 32), R)


def _flipped(proof: bytes, at: int) -> bytes:
    out = bytearray(proof)
    out[at] ^= 1
    return bytes(out)


# ---- 1. multiplicities ------------------------------------------------------------------------------------------------------------------
def _inputs(kind: str, K: int, u: int, rng: random.Random):
    """-> (K input columns, table rows), u rows each"""
    if kind == "repeats":  # a table with repeated values (only a value's first row counts) and values no input of any set takes
        pool = [rng.randrange(R) for _ in range(max(3, u // 3))]
        table = [rng.choice(pool) for _ in range(u)]
        used = [v for v in table if v != pool[0]] or table
        return [[rng.choice(used) for _ in range(u)] for _ in range(K)], table
    if kind == "equal":  # all inputs of all sets equal, a table whose values are their ranks: one counter takes K u hits
        return [[u - 1] * u for _ in range(K)], list(range(u))
    if kind == "edges":  # one value present in set 0 only and one in set K - 1 only; the other inputs from the rest of the table
        table = [rng.randrange(R) for _ in range(u)]
        sets = [[rng.choice(table[2:]) for _ in range(u)] for _ in range(K)]
        sets[0][u // 2], sets[K - 1][u - 1] = table[0], table[1]
        return sets, table
    if kind == "tuple":  # a theta-compressed tuple table: uniform 254-bit keys, each 4-bit XOR row several times
        theta = rng.randrange(R)
        rows = [compress((i >> 4, i & 15, (i >> 4) ^ (i & 15)), theta) for i in range(256)]
        table = [rows[rng.randrange(256)] for _ in range(u)]
        return [[rng.choice(table) for _ in range(u)] for _ in range(K)], table
    assert kind == "absent"  # one input of the LAST set that is no table value
    sets, table = _inputs("repeats", K, u, rng)
    sets[K - 1][(2 * u) // 3] = next(v for v in iter(lambda: rng.randrange(R), None) if v not in set(table))
    return sets, table


def _pack_sets(sets, n, u, rng):
    """K columns of u rows -> K consecutive vectors of n rows; the rows beyond u hold values that would count if they were read"""
    flat = []
    for col in sets:
        flat += col + [col[rng.randrange(u)] for _ in range(n - u)]
    return flat


@pytest.mark.parametrize("kind", ["repeats", "equal", "edges", "tuple", "absent"])
@pytest.mark.parametrize("K", SETS)
@pytest.mark.parametrize("k,u", SIZES)
def test_multiplicity_against_python_integers(gpu, k, u, K, kind):
    from halo2_scaffold_amd import plonk
    from halo2_scaffold_amd.device import DevBuf

    n = 1 << k
    rng = random.Random(9100 + 7 * u + 31 * K + len(kind))
    sets, table = _inputs(kind, K, u, rng)
    tail = [rng.randrange(R) for _ in range(n - u)]
    sentinel = [rng.randrange(R) for _ in range(n)]
    d_a, d_t, d_m = (DevBuf.from_numpy(o.pack(rows, R)) for rows in (_pack_sets(sets, n, u, rng), table + tail, sentinel))
    missing = plonk.logup_multiplicity_sets(k, d_a, K, d_t, u, d_m)
    want, absent = cases.multiplicities(sets, table, u)
    got = _vals(d_m, n)
    assert missing == len(absent) == (1 if kind == "absent" else 0)
    if kind == "absent":
        assert absent == [((2 * u) // 3, K - 1)]
    assert got[:u] == want and sum(want) == K * u - len(absent)
    assert got[u:] == sentinel[u:]  # the blinding rows are the caller's
    if kind == "equal":
        assert want[u - 1] == K * u and got.count(0) >= u - 1
    if kind == "repeats":
        assert any(want[r] == 0 for r in range(u))
    if kind == "edges":
        assert want[0] == 1 and want[1] == 1
    for b in (d_a, d_t, d_m):
        b.free()


def test_one_set_is_the_existing_call(gpu):
    """h2mi_plonk_logup_multiplicity_dev / _sum_dev are the sets calls with n_inputs == 1: the same words"""
    from halo2_scaffold_amd import plonk
    from halo2_scaffold_amd.device import DevBuf

    k, u = 11, 1025
    n = 1 << k
    rng = random.Random(3)
    (a,), table = _inputs("repeats", 1, u, rng)
    beta = rng.randrange(R)
    d_a, d_t = DevBuf.from_numpy(o.pack(a + [0] * (n - u), R)), DevBuf.from_numpy(o.pack(table + [0] * (n - u), R))
    outs = [DevBuf.from_numpy(o.pack([0] * n, R)) for _ in range(4)]
    assert plonk.logup_multiplicity(k, d_a, d_t, u, outs[0]) == 0 and plonk.logup_multiplicity_sets(k, d_a, 1, d_t, u, outs[1]) == 0
    plonk.logup_sum(k, d_a, d_t, outs[0], beta, u, outs[2])
    plonk.logup_sum_sets(k, d_a, 1, d_t, outs[1], beta, u, outs[3])
    m = _vals(outs[0], n)
    assert m == _vals(outs[1], n) and m[:u] == logup_cases.multiplicities(a, table, u)[0]
    assert _vals(outs[2], n) == _vals(outs[3], n)
    for b in outs + [d_a, d_t]:
        b.free()


# ---- 2. the running sum ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", SETS)
@pytest.mark.parametrize("k,u", SIZES)
def test_running_sum_against_python_integers(gpu, k, u, K):
    from halo2_scaffold_amd import plonk
    from halo2_scaffold_amd.device import DevBuf

    n = 1 << k
    rng = random.Random(9600 + u + 13 * K)
    sets, table = _inputs("tuple" if u > 1000 else "repeats", K, u, rng)
    m, absent = cases.multiplicities(sets, table, u)
    assert not absent
    beta = rng.randrange(R)
    fill = lambda: [rng.randrange(R) for _ in range(n - u)]
    sentinel = [rng.randrange(R) for _ in range(n)]
    bufs = [DevBuf.from_numpy(o.pack(rows, R)) for rows in (_pack_sets(sets, n, u, rng), table + fill(), m + fill(), sentinel)]
    plonk.logup_sum_sets(k, bufs[0], K, bufs[1], bufs[2], beta, u, bufs[3])
    got = _vals(bufs[3], n)
    want = cases.running_sum(sets, table, m, beta, u)
    assert want[0] == 0 and want[u] == 0 and len(set(want)) > u // 2
    assert got[: u + 1] == want
    assert got[u + 1:] == sentinel[u + 1:]  # the blinding rows are the caller's
    # multiplicities that do not belong to the inputs: the sum is what the recurrence says and does not return to zero
    m[0] = (m[0] + 1) % R
    d_m = DevBuf.from_numpy(o.pack(m + fill(), R))
    plonk.logup_sum_sets(k, bufs[0], K, bufs[1], d_m, beta, u, bufs[3])
    want = cases.running_sum(sets, table, m, beta, u)
    assert want[u] != 0 and _vals(bufs[3], n)[: u + 1] == want
    for b in bufs + [d_m]:
        b.free()


def test_device_call_refusals(gpu):
    from halo2_scaffold_amd import field as F
    from halo2_scaffold_amd._lib import lib
    from halo2_scaffold_amd.device import DevBuf

    buf = DevBuf(7 * 32 * 32)
    b = F.fr_to_mont_limbs(5)
    missing = C.c_uint64()
    for count in (0, 7):
        assert lib.h2mi_plonk_logup_multiplicity_sets_dev(buf.ptr, count, buf.ptr, 5, 22, buf.ptr, C.byref(missing), None) == -1
        assert lib.h2mi_plonk_logup_sum_sets_dev(buf.ptr, count, buf.ptr, buf.ptr, 5, 22, b.ctypes.data, buf.ptr, None) == -1
    assert lib.h2mi_plonk_logup_multiplicity_sets_dev(buf.ptr, 2, buf.ptr, 5, 22, buf.ptr, None, None) == -1
    assert lib.h2mi_plonk_logup_multiplicity_sets_dev(buf.ptr, 2, buf.ptr, 5, 32, buf.ptr, C.byref(missing), None) == -6
    assert lib.h2mi_plonk_logup_sum_sets_dev(buf.ptr, 2, buf.ptr, buf.ptr, 5, 32, b.ctypes.data, buf.ptr, None) == -6
    buf.free()


# ---- helpers: keys, and a proof's vectors in Python integers --------------------------------------------------------------------------
def _keys(gpu, cs, first, k, name, logup=True):
    from halo2_scaffold_amd import custom

    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    keys = custom.Keys(params, cs, first, logup=logup)
    ocs = gate_cases.oracle_cs(cs, name)
    oasg = gate_cases.oracle_assignment(ocs, first)
    vk = FX.VerifierKeys(ocs, k, SRS_SECRET, oasg.fixed, oasg.copies)
    assert o.unpack_points(keys.fixed_commitments) == vk.fixed_commitments and keys.transcript_repr == vk.transcript_repr
    return custom, params, keys, vk


def _release(params, keys, *ws):
    for w in ws:
        w.release()
    keys.release()
    params.release()


def _case(gpu, name):
    from halo2_scaffold_amd import custom

    cs, asg, k = cases.build(custom, name)
    custom_, params, keys, vk = _keys(gpu, cs, cases.first_assignment(cs, asg), k, name)
    return custom_, cs, asg, k, params, keys, vk


def _compress_coset(exprs, cols, size, rot, theta, challenges):
    out = []
    for idx in range(size):
        q = lambda kind, c, r: cols[kind][c][(idx + r * rot) % size]
        out.append(compress([e.evaluate(q, challenges) for e in exprs], theta))
    return out


def _coset_circuit(cs, keys, prover, k, theta):
    """every vector the quotient reads for one circuit of a merged logUp key, recomputed in Python integers on the extended coset from
    the ROW buffers of the prover (advice, products, M, phi) and of the key.  Nothing here is read from a device coset buffer."""
    from halo2_scaffold_amd import engine

    n = 1 << k
    dom = o.Domain(k, cs.degree())
    size, rot = 1 << dom.extended_k, 1 << (dom.extended_k - k)
    ext = lambda rows: dom.coeff_to_extended(dom.lagrange_to_coeff(rows))
    rows_of = lambda views: [_vals(v, n) for v in views]
    advice = [ext(r) for r in rows_of(prover.views(engine.BUF_ADVICE, cs.n_advice))]
    fixed = [ext(r) for r in rows_of(keys.fixed_values)]
    sigma = [ext(r) for r in rows_of(keys.sigma_values)]
    instance = ext(_vals(prover.view(engine.BUF_INSTANCE), n)) if cs.n_instance else None
    m, chunk = len(cs.perm_columns), cs.degree() - 2
    n_sets = -(-m // chunk)
    perm_zs = [ext(r) for r in rows_of(prover.views(engine.BUF_PERM_Z, n_sets))]
    by_kind = {"advice": advice, "fixed": fixed, "instance": [instance]}
    perm_values = [by_kind[kind][c] for kind, c in cs.perm_columns]
    L, S = len(cs.lookup_arguments), len(cs.shuffles)
    declared = cs.lookups
    lookups = []
    for l, arg in enumerate(cs.lookup_arguments):
        a_ins = [_compress_coset([a for a, _ in declared[j]], by_kind, size, rot, theta, ()) for j in arg]
        t_in = _compress_coset([t for _, t in declared[arg[0]]], by_kind, size, rot, theta, ())
        mult, phi = (ext(_vals(prover.views(kind, L)[l], n)) for kind in (engine.BUF_LOGUP_M, engine.BUF_LOGUP_PHI))
        lookups.append((a_ins, None, t_in, mult, None, phi))
    shuffles = []
    for i, pairs in enumerate(cs.shuffles):
        a_in = _compress_coset([a for a, _ in pairs], by_kind, size, rot, theta, ())
        s_in = _compress_coset([s for _, s in pairs], by_kind, size, rot, theta, ())
        shuffles.append((a_in, s_in, ext(_vals(prover.views(engine.BUF_SHUFFLE_Z, S)[i], n))))
    u = n - (cs.blinding_factors() + 1)
    unit = lambda row: [1 if i == row else 0 for i in range(n)]
    shared = {"perm_sigmas": sigma, "chunk": chunk, "l0": ext(unit(0)), "l_last": ext(unit(u)), "l_active": ext([1] * u + [0] * (n - u))}
    circuit = {"advice": advice, "fixed": fixed, "instance": instance, "perm_values": perm_values, "perm_zs": perm_zs, "lookups": lookups,
               "shuffles": shuffles}
    return circuit, shared, dom


def _check_quotient(cs, keys, provers, k, trace):
    from halo2_scaffold_amd import engine

    ops, consts = cs.program()
    built = [_coset_circuit(cs, keys, p, k, trace["theta"]) for p in provers]
    shared, dom = built[0][1], built[0][2]
    args = (k, dom.extended_k, dom.g_coset, dom.extended_omega, cases.keys_delta(), cs.blinding_factors(), ops, consts, [])
    want = cases.batched_quotient(*args, [b[0] for b in built], shared, trace["beta"], trace["gamma"], trace["y"], logup=True)
    size = 1 << dom.extended_k
    got = dom.coeff_to_extended(_vals(provers[0].view(engine.BUF_H), size))  # the inverse transform is a bijection
    assert len(want) == size and got == want
    # the term reads EVERY set: with the last set of the first merged argument left out the quotient is another
    l = next(i for i, arg in enumerate(cs.lookup_arguments) if len(arg) > 1)
    short = []
    for b in built:
        lk = list(b[0]["lookups"])
        lk[l] = (lk[l][0][:-1],) + lk[l][1:]
        short.append(dict(b[0], lookups=lk))
    assert cases.batched_quotient(*args, short, shared, trace["beta"], trace["gamma"], trace["y"], logup=True) != want


# ---- 3. the quotient --------------------------------------------------------------------------------------------------------------------
def _range_k(custom, K, variant=0):
    """K range columns in one argument: degree 2 + K + 1"""
    return cases.range_circuit(custom, columns=K, variant=variant, max_degree=3 + K)


@pytest.mark.parametrize("K", [2, 6])
def test_quotient_single(gpu, K):
    """k_evaluate_h_expr: every extended-coset point against the Python-integer quotient with the K-input term"""
    from halo2_scaffold_amd import custom

    cs, asg = _range_k(custom, K)
    assert cs.lookup_arguments == [list(range(K))] and cs.degree() == 3 + K
    _, params, keys, vk = _keys(gpu, cs, asg, 5, "range%d" % K)
    ws = custom.Workspace(params, keys)
    trace = {}
    proof = custom.create_proof(params, keys, asg, 21, trace=trace, ws=ws)
    assert cases.verify_circuits(vk, cs, proof, [asg.instance], logup=True)
    _check_quotient(cs, keys, [ws.prover], 5, trace)
    _release(params, keys, ws)


@pytest.mark.parametrize("K", [2, 6])
def test_quotient_batch(gpu, K):
    """k_evaluate_h_expr_batch on two circuits: one accumulator over both circuits' K-input terms"""
    from halo2_scaffold_amd import custom

    built = [_range_k(custom, K, variant=v) for v in (0, 1)]
    cs, asgs = built[0][0], [a for _, a in built]
    _, params, keys, vk = _keys(gpu, cs, asgs[0], 5, "range%d" % K)
    ws = custom.BatchWorkspace(params, keys, 2)
    trace = {}
    proof = custom.prove_many(keys, asgs, seeds=[5, 13], ws=ws, trace=trace)
    assert cases.verify_circuits(vk, cs, proof, [a.instance for a in asgs], logup=True)
    _check_quotient(cs, keys, ws.provers, 5, trace)
    _release(params, keys, ws)


def test_quotient_with_one_three_and_two_sets(gpu):
    """three lookup arguments of 1, 3 and 2 input sets beside two gates, a permutation and a shuffle"""
    from halo2_scaffold_amd import custom

    cs, asg = cases.three_arguments_circuit(custom)
    assert [len(a) for a in cs.lookup_arguments] == [1, 3, 2] and cs.degree() == 6 and cs.shuffles and cs.perm_columns
    _, params, keys, vk = _keys(gpu, cs, asg, 6, "three")
    ws = custom.Workspace(params, keys)
    trace = {}
    proof = custom.create_proof(params, keys, asg, 8, trace=trace, ws=ws)
    assert cases.verify_circuits(vk, cs, proof, [asg.instance], logup=True)
    _check_quotient(cs, keys, [ws.prover], 6, trace)
    _release(params, keys, ws)


def test_lg_entries_with_null_or_ones_are_the_existing_entries(gpu):
    """h2mi_plonk_evaluate_h_expr_dev / _batch_dev: the record with logup == NULL against the record with all ones word for word (random
    vectors: the quotient is evaluated pointwise), and the refusals of a logup field"""
    from halo2_scaffold_amd import engine, plonk
    from halo2_scaffold_amd._lib import lib
    from halo2_scaffold_amd.device import DevBuf
    from halo2_scaffold_amd.domain import EvaluationDomain

    LOGUP = 0x80000000
    k, rng = 4, random.Random(12)
    dom = EvaluationDomain(4, k)
    size = 1 << dom.extended_k
    vec = lambda: DevBuf.from_numpy(o.pack([rng.randrange(R) for _ in range(size)], R))
    bufs = [vec() for _ in range(12)]
    program = engine.GateProgram.build([(engine.ADVICE, 0, 0), (engine.FIXED, 0, 1), (6, 0, 0), (8, 0, 0)], [])  # advice0 * fixed0(wX): MUL, END
    arr = (plonk._ExprCosets * 2)()
    for i, cs in enumerate(arr):
        cs.advice[0], cs.fixed[0] = bufs[i].ptr, bufs[2].ptr
        cs.n_lookups = 2 | LOGUP
        for l in range(2):
            cs.lookup_input[l], cs.lookup_table[l] = bufs[3 + l].ptr, bufs[5 + l + i].ptr
            cs.lookup_permuted_input[l], cs.lookup_z[l] = bufs[7 + l].ptr, bufs[8 + l + i].ptr
        cs.l0, cs.l_last, cs.l_active = bufs[9].ptr, bufs[10].ptr, bufs[11].ptr
    scalars = plonk.quotient_scalars(dom, rng.randrange(R), rng.randrange(R), rng.randrange(R), 5)
    outs = [DevBuf(size * 32) for _ in range(4)]
    ones, two = engine.LogupInputs.build([1] * 8), engine.LogupInputs.build([2, 1])

    def single(logup, out):
        return lib.h2mi_plonk_evaluate_h_expr_dev(C.byref(plonk.quotient_circuits(program, arr, 1, logup=logup)), C.byref(scalars), out.ptr, None)

    def batch(logup, out):
        return lib.h2mi_plonk_evaluate_h_expr_batch_dev(C.byref(plonk.quotient_circuits(program, arr, 2, logup=logup)), C.byref(scalars), -1, out.ptr, None)

    assert single(None, outs[0]) == 0 and single(ones, outs[1]) == 0
    assert batch(None, outs[2]) == 0 and batch(ones, outs[3]) == 0
    words = [b.to_numpy(shape=(size, 4), nbytes=size * 32).tobytes() for b in outs]
    assert words[0] == words[1] and words[2] == words[3] and words[0] != words[2]
    # refusals: a count of 0 or above the maximum; another count than 1 without H2MI_LOOKUPS_LOGUP
    for counts in ([0, 1], [1, 7]):
        bad = engine.LogupInputs.build(counts)
        assert single(bad, outs[1]) == -1
        assert batch(bad, outs[3]) == -1
    for cs in arr:
        cs.n_lookups = 2
        for l in range(2):
            cs.lookup_permuted_table[l] = bufs[l].ptr
    assert single(two, outs[1]) == -1
    assert batch(two, outs[3]) == -1
    assert single(ones, outs[1]) == 0
    for b in bufs + outs:
        b.free()


# ---- 4. proofs ------------------------------------------------------------------------------------------------------------------------
def _unmerged(custom, name):
    """the same circuit and witness without merge_lookups"""
    cs, asg, k = cases.build(custom, name)
    cs._merged = None
    return cs, asg, k


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_proofs_are_accepted_and_tampering_is_rejected(gpu, name):
    """three range columns over one fixed table; the XOR tuple table looked up by two tuples with a rotation; a merged lookup beside
    gates, a permutation, a shuffle and an unmerged lookup; two phases with a challenge inside the merged inputs.  Then the lengths
    against the unmerged logUp key, and the merged M column against the sum of the unmerged key's"""
    from halo2_scaffold_amd import engine

    custom, cs, asg, k, params, keys, vk = _case(gpu, name)
    first = cases.first_assignment(cs, asg)
    ws = custom.Workspace(params, keys)
    proof = custom.create_proof(params, keys, asg, 33, ws=ws)
    instances = [first.instance]
    args = cs.lookup_arguments
    L = len(args)
    assert max(len(a) for a in args) >= 2
    assert cases.verify_circuits(vk, cs, proof, instances, logup=True)
    assert not cases.verify_circuits(vk, cs, proof, instances, logup=False)
    m_at, phi_at, ev_at = cases.proof_offsets(cs)
    last = ev_at + 32 * 3 * (L - 1)  # the last argument is a merged one in every case
    assert len(args[-1]) >= 2
    for at in (m_at + 5, m_at + 32 * (L - 1) + 9, phi_at + 3, phi_at + 32 * (L - 1) + 17, last + 1, last + 32 + 2, last + 64 + 3):
        assert not cases.verify_circuits(vk, cs, _flipped(proof, at), instances, logup=True), at
    c = ws.prover.counts
    m, chunk = len(cs.perm_columns), cs.degree() - 2
    assert c.lookups == L and c.products == -(-m // chunk) + L + len(cs.shuffles) + 1
    assert c.evaluations == logup_cases.num_evaluations(1, len(cs.advice_queries), len(cs.fixed_queries), m, -(-m // chunk), L, len(cs.shuffles), logup=True)
    n = 1 << k
    merged_m = [_vals(ws.prover.views(engine.BUF_LOGUP_M, L)[l], n) for l in range(L)]
    assert custom.prove_many(keys, [asg], seeds=[33]) == proof  # a batch of one: the batch kernel's bytes
    # the unmerged logUp key of the same circuit and witness.  Per merged group the proof loses (K - 1) x (2 points + 3 scalars); where
    # merging raised the system's degree it gains one quotient piece per step (the permutation sets are the same here: one)
    ucs, uasg, _ = _unmerged(custom, name)
    assert ucs.degree() <= cs.degree() and -(-m // (ucs.degree() - 2)) == -(-m // chunk) == 1
    _, uparams, ukeys, uvk = _keys(gpu, ucs, cases.first_assignment(ucs, uasg), k, name + " unmerged")
    uws = custom.Workspace(uparams, ukeys)
    uproof = custom.create_proof(uparams, ukeys, uasg, 33, ws=uws)
    assert logup_cases.verify_circuits(uvk, ucs, uproof, instances, logup=True)
    assert len(uproof) - len(proof) == sum(len(a) - 1 for a in args) * (2 * 32 + 3 * 32) - 32 * (cs.degree() - ucs.degree())
    assert not cases.verify_circuits(vk, cs, uproof, instances, logup=True)
    UL = len(ucs.lookups)
    unmerged_m = [_vals(uws.prover.views(engine.BUF_LOGUP_M, UL)[l], n) for l in range(UL)]
    u = n - (cs.blinding_factors() + 1)
    for arg, mm in zip(args, merged_m):  # the counts do not depend on theta: row for row the sum of its members' columns
        assert mm[:u] == [sum(unmerged_m[j][r] for j in arg) % R for r in range(u)] and sum(mm[:u]) == len(arg) * u
    _release(uparams, ukeys, uws)
    _release(params, keys, ws)


def test_a_batch_of_two(gpu):
    from halo2_scaffold_amd import custom

    built = [cases.beside_circuit(custom, variant=v) for v in (0, 1)]
    cs, asgs = built[0][0], [a for _, a in built]
    assert [len(a) for a in cs.lookup_arguments] == [1, 2]
    _, params, keys, vk = _keys(gpu, cs, asgs[0], 6, "beside")
    proof = custom.prove_many(keys, asgs, seeds=[5, 13])
    instances = [a.instance for a in asgs]
    assert cases.verify_circuits(vk, cs, proof, instances, logup=True)
    m_at, phi_at, ev_at = cases.proof_offsets(cs, 2)
    for at in (m_at + 32 * 3 + 3, phi_at + 32 * 3 + 5, ev_at + 32 * 9 + 1, ev_at + 32 * 10 + 1, ev_at + 32 * 11 + 1):  # the second circuit's merged argument
        assert not cases.verify_circuits(vk, cs, _flipped(proof, at), instances, logup=True), at
    _release(params, keys)


def test_all_counts_one_reproduces_the_logup_goldens(gpu):
    """a key made with `inputs` of every count 1 is the key `inputs` == NULL makes: every byte of tests/golden/logup_proofs.json"""
    g = json.load(open(os.path.join(GOLD, "logup_proofs.json")))
    from halo2_scaffold_amd import custom

    for entry in g["cases"]:
        cs, asg, k = logup_cases.build(custom, entry["circuit"])
        assert cs.merge_lookups(4) == [[l] for l in range(len(cs.lookups))] and cs.logup_inputs() is not None
        assert list(cs.logup_inputs().n_inputs) == [1] * 8
        _, params, keys, vk = _keys(gpu, cs, asg, k, entry["circuit"])
        assert custom.create_proof(params, keys, asg, entry["seed"]).hex() == entry["proof"]
        _release(params, keys)


# ---- 5. the check ------------------------------------------------------------------------------------------------------------------------
def test_an_absent_cell_of_one_set_is_reported_and_refused(gpu):
    from halo2_scaffold_amd import custom, engine
    from halo2_scaffold_amd import field as F
    from halo2_scaffold_amd._lib import lib

    (cs, bad), good = cases.range_circuit(custom, bad=(1, 6)), cases.range_circuit(custom)[1]
    _, params, keys, vk = _keys(gpu, cs, good, 5, "range3")
    ws = custom.Workspace(params, keys)
    custom.check(params, keys, good, ws=ws)  # nothing to report
    with pytest.raises(ValueError, match=r"lookup 'range 0 \+ range 1 \+ range 2' not satisfied at row 6") as e:
        custom.check(params, keys, bad, ws=ws)
    assert [f.astuple() for f in e.value.failures] == [(engine.CHECK_LOOKUP, 0, 6, 1)]
    with pytest.raises(ValueError, match="lookup input not in the table"):
        custom.create_proof(params, keys, bad, 9, ws=ws)
    # the C ABI itself: H2MI_EUNSAT from the lookups phase, and the proof is abandoned
    p = ws.prover
    pts, inst = np.zeros((16, 8), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64)
    cells, keep = engine.pack_cells(bad.advice)
    assert lib.h2mi_prover_advice(p.handle, cells, inst.ctypes.data, 0, 7, pts.ctypes.data) == 0
    th = F.fr_to_mont_limbs(11)
    assert lib.h2mi_prover_lookups(p.handle, th.ctypes.data, pts.ctypes.data) == engine.EUNSAT
    assert lib.h2mi_prover_products(p.handle, th.ctypes.data, th.ctypes.data, pts.ctypes.data) == -1
    del keep
    proof = custom.create_proof(params, keys, good, 9, ws=ws)
    assert cases.verify_circuits(vk, cs, proof, [good.instance], logup=True) and proof == custom.create_proof(params, keys, good, 9)
    _release(params, keys, ws)


# ---- 6. the golden -------------------------------------------------------------------------------------------------------------------------
def test_golden_proofs_are_reproduced(gpu):
    g = json.load(open(os.path.join(GOLD, "logup_sets_proofs.json")))
    assert sorted(c["circuit"] for c in g["cases"]) == ["beside", "range3"] and int(g["srs_secret"], 16) == SRS_SECRET
    for entry in g["cases"]:
        custom, cs, asg, k, params, keys, vk = _case(gpu, entry["circuit"])
        assert k == entry["k"] <= 6 and [len(a) for a in cs.lookup_arguments] == entry["n_inputs"]
        proof = custom.create_proof(params, keys, asg, entry["seed"])
        assert proof.hex() == entry["proof"]
        assert cases.verify_circuits(vk, cs, proof, [cases.first_assignment(cs, asg).instance], logup=True)
        _release(params, keys)
