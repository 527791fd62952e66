"""The logUp lookup argument on the device, bit for bit against the Python integers of tests/logup_cases.py: the multiplicity column
(h2mi_plonk_logup_multiplicity_dev) around the ranking kernel's 1024-thread workgroup and on the inputs that take each of its paths;
the running sum (h2mi_plonk_logup_sum_dev) row by row around the scan tiles; the quotient kernels (k_evaluate_h_expr,
k_evaluate_h_expr_batch) with the logUp terms, recovered from H2MI_BUF_H on every extended-coset point; proofs of every case accepted by
the generalised verifier and rejected with a byte of [M], [phi] or one of the three evaluations flipped; the counts; a key without the
flag against the bytes the parent commit's library made; unsatisfied witnesses; the flag's refusals; the committed golden."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

import custom_gate_cases as gate_cases
import keygen_call
import logup_cases as cases
import lookup_expr_cases as lookup_cases
import shuffle_cases
from lookup_expr_cases import compress
from oracle import bn254 as o
from oracle import flex as FX

pytestmark = pytest.mark.gpu

R = o.R
SRS_SECRET = 0x5EC2E7 + 0x48324D49
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (k, usable rows): one wavefront's worth; both sides of the ranking kernel's 1024-thread workgroup, which is also the tile of the
# multiplicative chain (MS_TILE) and of the additive scan (AS_TILE); eight tiles with a ragged last one
SIZES = [(5, 22), (11, 1023), (11, 1024), (11, 1025), (13, (1 << 13) - 7)]


def _vals(buf, count):
    return o.unpack(buf.to_numpy(shape=(count, 4), nbytes=count * 32), R)


# ---- 1. multiplicities ------------------------------------------------------------------------------------------------------------------
def _inputs(kind: str, u: int, rng: random.Random):
    """-> (input rows, table rows), u of each"""
    if kind == "repeats":  # a table with repeated values: only a value's first row counts
        pool = [rng.randrange(R) for _ in range(max(2, u // 3))]
        table = [rng.choice(pool) for _ in range(u)]
        return [rng.choice(table) for _ in range(u)], table
    if kind == "unused":  # table values no input takes: M = 0 on their rows
        table = list(range(u))
        rng.shuffle(table)
        return [2 * rng.randrange((u + 1) // 2) for _ in range(u)], table
    if kind == "equal":  # all inputs equal, a table whose values are their ranks: one counter receives u (the merged path)
        return [u - 1] * u, list(range(u))
    if kind == "ranks":  # uniform ranks: far more than 64 distinct ones inside a workgroup (the fallback atomics)
        table = [rng.randrange(R) for _ in range(u)]
        return [rng.choice(table) for _ in range(u)], table
    if kind == "tuple":  # a theta-compressed tuple table: uniform 254-bit keys, each 4-bit XOR row several times
        theta = rng.randrange(R)
        rows = [compress((i >> 4, i & 15, (i >> 4) ^ (i & 15)), theta) for i in range(256)]
        table = [rows[rng.randrange(256)] for _ in range(u)]
        return [rng.choice(table) for _ in range(u)], table
    assert kind == "absent"  # one input that is no table value
    a, table = _inputs("repeats", u, rng)
    a[(2 * u) // 3] = next(v for v in iter(lambda: rng.randrange(R), None) if v not in set(table))
    return a, table


@pytest.mark.parametrize("kind", ["repeats", "unused", "equal", "ranks", "tuple", "absent"])
@pytest.mark.parametrize("k,u", SIZES)
def test_multiplicity_against_python_integers(gpu, k, u, kind):
    from halo2_scaffold_amd import plonk
    from halo2_scaffold_amd.device import DevBuf

    n = 1 << k
    rng = random.Random(9000 + 7 * u + len(kind))
    a, table = _inputs(kind, u, rng)
    tail = [rng.randrange(R) for _ in range(n - u)]  # rows beyond u are not read: values that would count if they were
    sentinel = [rng.randrange(R) for _ in range(n)]
    d_a, d_t, d_m = DevBuf.from_numpy(o.pack(a + table[: n - u], R)), DevBuf.from_numpy(o.pack(table + tail, R)), DevBuf.from_numpy(o.pack(sentinel, R))
    missing = plonk.logup_multiplicity(k, d_a, d_t, u, d_m)
    want, absent = cases.multiplicities(a, table, u)
    got = _vals(d_m, n)
    assert missing == len(absent) == (1 if kind == "absent" else 0)
    assert got[:u] == want and sum(want) == u - len(absent)
    assert got[u:] == sentinel[u:]  # the blinding rows are the caller's
    if kind == "equal":
        assert want[u - 1] == u and got.count(0) >= u - 1
    if kind == "unused":
        assert any(want[r] == 0 for r in range(u))
    for b in (d_a, d_t, d_m):
        b.free()


def test_sort_unique_first_rows(gpu):
    """h2mi_fr_sort_unique_first_dev: the existing three outputs unchanged, and per distinct value its lowest position"""
    from halo2_scaffold_amd._lib import lib
    from halo2_scaffold_amd.device import DevBuf

    rng = random.Random(5)
    count = 3000
    pool = [rng.randrange(R) for _ in range(700)] + [0, 1, R - 1]
    vals = [rng.choice(pool) for _ in range(count)]
    d_in = DevBuf.from_numpy(o.pack(vals, R))
    bufs = [DevBuf(count * 32), DevBuf(count * 32), DevBuf(count * 4), DevBuf(count * 4)]
    n_first, n_plain = C.c_uint32(), C.c_uint32()
    assert lib.h2mi_fr_sort_unique_first_dev(d_in.ptr, count, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, C.byref(n_first), None) == 0
    distinct = sorted(set(vals))
    assert n_first.value == len(distinct)
    first = bufs[3].to_numpy(shape=(count,), nbytes=count * 4, dtype=np.uint32)[: len(distinct)].tolist()
    mult = bufs[2].to_numpy(shape=(count,), nbytes=count * 4, dtype=np.uint32)[: len(distinct)].tolist()
    assert first == [vals.index(v) for v in distinct] and mult == [vals.count(v) for v in distinct]
    assert _vals(bufs[1], count)[: len(distinct)] == distinct
    assert lib.h2mi_fr_sort_unique_dev(d_in.ptr, count, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, C.byref(n_plain), None) == 0 and n_plain.value == len(distinct)
    assert lib.h2mi_fr_sort_unique_first_dev(d_in.ptr, count, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, None, C.byref(n_first), None) == -1
    for b in bufs + [d_in]:
        b.free()


# ---- 2. the running sum ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,u", SIZES)
def test_running_sum_against_python_integers(gpu, k, u):
    from halo2_scaffold_amd import plonk
    from halo2_scaffold_amd.device import DevBuf

    n = 1 << k
    rng = random.Random(9500 + u)
    a, table = _inputs("tuple" if u > 1000 else "repeats", u, rng)
    m, absent = cases.multiplicities(a, table, u)
    assert not absent
    beta = rng.randrange(R)
    fill = lambda: [rng.randrange(R) for _ in range(n - u)]
    sentinel = [rng.randrange(R) for _ in range(n)]
    bufs = [DevBuf.from_numpy(o.pack(rows, R)) for rows in (a + fill(), table + fill(), m + fill(), sentinel)]
    plonk.logup_sum(k, bufs[0], bufs[1], bufs[2], beta, u, bufs[3])
    got = _vals(bufs[3], n)
    want = cases.running_sum(a, table, m, beta, u)
    assert want[0] == 0 and want[u] == 0 and len(set(want)) > u // 2
    assert got[: u + 1] == want
    assert got[u + 1:] == sentinel[u + 1:]  # the blinding rows are the caller's
    # multiplicities that do not belong to the inputs: the sum is what the recurrence says and does not return to zero
    m[0] = (m[0] + 1) % R
    d_m = DevBuf.from_numpy(o.pack(m + fill(), R))
    plonk.logup_sum(k, bufs[0], bufs[1], d_m, beta, u, bufs[3])
    want = cases.running_sum(a, table, m, beta, u)
    assert want[u] != 0 and _vals(bufs[3], n)[: u + 1] == want
    for b in bufs + [d_m]:
        b.free()


def test_device_call_refusals(gpu):
    from halo2_scaffold_amd import field as F
    from halo2_scaffold_amd._lib import lib
    from halo2_scaffold_amd.device import DevBuf

    buf = DevBuf(32 * 32)
    b = F.fr_to_mont_limbs(5)
    missing = C.c_uint64()
    assert lib.h2mi_plonk_logup_multiplicity_dev(None, buf.ptr, 5, 22, buf.ptr, C.byref(missing), None) == -1
    assert lib.h2mi_plonk_logup_multiplicity_dev(buf.ptr, buf.ptr, 5, 22, buf.ptr, None, None) == -1
    assert lib.h2mi_plonk_logup_multiplicity_dev(buf.ptr, buf.ptr, 5, 32, buf.ptr, C.byref(missing), None) == -6
    assert lib.h2mi_plonk_logup_multiplicity_dev(buf.ptr, buf.ptr, 5, 0, buf.ptr, C.byref(missing), None) == -6
    assert lib.h2mi_plonk_logup_sum_dev(buf.ptr, buf.ptr, None, 5, 22, b.ctypes.data, buf.ptr, None) == -1
    assert lib.h2mi_plonk_logup_sum_dev(buf.ptr, buf.ptr, buf.ptr, 5, 22, None, buf.ptr, None) == -1
    assert lib.h2mi_plonk_logup_sum_dev(buf.ptr, buf.ptr, buf.ptr, 5, 32, b.ctypes.data, buf.ptr, None) == -6
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


def _case(gpu, name, logup=True):
    from halo2_scaffold_amd import custom

    cs, asg, k = cases.build(custom, name)
    custom_, params, keys, vk = _keys(gpu, cs, cases.first_assignment(cs, asg), k, name, logup)
    return custom_, cs, asg, k, params, keys, vk


def _compress_coset(exprs, cols, size, rot, theta, challenges):
    out = []
    for idx in range(size):
        q = lambda kind, c, r: cols[kind][c][(idx + r * rot) % size]
        out.append(compress([e.evaluate(q, challenges) for e in exprs], theta))
    return out


def _coset_circuit(cs, keys, prover, k, theta):
    """every vector the quotient reads for one circuit of a logUp key, recomputed in Python integers on the extended coset from the ROW
    buffers of the prover (advice, products, M, phi) and of the key.  Nothing here is read from a device coset buffer."""
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
    L, S = len(cs.lookups), len(cs.shuffles)
    lookups = []
    for l, pairs in enumerate(cs.lookups):
        a_in = _compress_coset([a for a, _ in pairs], by_kind, size, rot, theta, ())
        t_in = _compress_coset([t for _, t in pairs], by_kind, size, rot, theta, ())
        mult, phi = (ext(_vals(prover.views(kind, L)[l], n)) for kind in (engine.BUF_LOGUP_M, engine.BUF_LOGUP_PHI))
        lookups.append((a_in, None, t_in, mult, None, phi))
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
    without = cases.batched_quotient(*args, [dict(b[0], lookups=[]) for b in built], shared, trace["beta"], trace["gamma"], trace["y"], logup=True)
    assert without != want  # the logUp terms are in h


# ---- 3. the quotient --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["xor", "mixed"])
def test_quotient_with_logup_terms_single(gpu, name):
    """k_evaluate_h_expr: every extended-coset point against the Python-integer quotient with logup_terms"""
    custom, cs, asg, k, params, keys, vk = _case(gpu, name)
    ws = custom.Workspace(params, keys)
    trace = {}
    proof = custom.create_proof(params, keys, asg, 21, trace=trace, ws=ws)
    assert cases.verify_circuits(vk, cs, proof, [asg.instance], logup=True)
    _check_quotient(cs, keys, [ws.prover], k, trace)
    _release(params, keys, ws)


def test_quotient_with_logup_terms_batch(gpu):
    """k_evaluate_h_expr_batch on mixed x 2: one accumulator over both circuits' gate, permutation, logUp and shuffle terms"""
    from halo2_scaffold_amd import custom

    built = [cases.mixed_circuit(custom, variant=v) for v in (0, 1)]
    cs, asgs = built[0][0], [a for _, a in built]
    _, params, keys, vk = _keys(gpu, cs, asgs[0], 6, "mixed")
    ws = custom.BatchWorkspace(params, keys, 2)
    trace = {}
    proof = custom.prove_many(keys, asgs, seeds=[5, 13], ws=ws, trace=trace)
    instances = [a.instance for a in asgs]
    assert cases.verify_circuits(vk, cs, proof, instances, logup=True)
    _check_quotient(cs, keys, ws.provers, 6, trace)
    m_at, phi_at, ev_at = cases.proof_offsets(cs, 2)
    for at in (m_at + 32 + 3, phi_at + 32 + 5, ev_at + 32 * 5 + 1):  # the second circuit's [M], [phi], M(x)
        flipped = bytearray(proof)
        flipped[at] ^= 1
        assert not cases.verify_circuits(vk, cs, bytes(flipped), instances, logup=True), at
    m, chunk = len(cs.perm_columns), cs.degree() - 2
    assert ws.batch.n_evaluations == cases.num_evaluations(2, len(cs.advice_queries), len(cs.fixed_queries), m, -(-m // chunk), 1, 1, logup=True)
    _release(params, keys, ws)


# ---- 4. proofs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_proofs_are_accepted_and_tampering_is_rejected(gpu, name):
    custom, cs, asg, k, params, keys, vk = _case(gpu, name)
    first = cases.first_assignment(cs, asg)
    ws = custom.Workspace(params, keys)
    proof = custom.create_proof(params, keys, asg, 33, ws=ws)
    instances = [first.instance]
    L = len(cs.lookups)
    assert cases.verify_circuits(vk, cs, proof, instances, logup=True)
    assert not cases.verify_circuits(vk, cs, proof, instances, logup=False)
    m_at, phi_at, ev_at = cases.proof_offsets(cs)
    # one byte of the first and of the last [M] and [phi], and of each of the last lookup's three evaluations phi(x), phi(omega x), M(x)
    last = ev_at + 32 * 3 * (L - 1)
    for at in (m_at + 5, m_at + 32 * (L - 1) + 9, phi_at + 3, phi_at + 32 * (L - 1) + 17, last + 1, last + 32 + 2, last + 64 + 3):
        flipped = bytearray(proof)
        flipped[at] ^= 1
        assert not cases.verify_circuits(vk, cs, bytes(flipped), instances, logup=True), at
    # h2mi_prover_lookups writes n_lookups points; two evaluations fewer per lookup than the same circuit's plain key
    m, chunk = len(cs.perm_columns), cs.degree() - 2
    c = ws.prover.counts
    assert c.lookups == L and c.products == -(-m // chunk) + L + len(cs.shuffles) + 1
    want = cases.num_evaluations(1, len(cs.advice_queries), len(cs.fixed_queries), m, -(-m // chunk), L, len(cs.shuffles), logup=True)
    assert c.evaluations == want
    plain = custom.Keys(params, cs, first)
    pws = custom.Workspace(params, plain)
    assert pws.prover.counts.evaluations == want + 2 * L and pws.prover.counts.lookups == 2 * L
    # the same witness under both keys, each accepted by its verifier and by no other
    plain_proof = custom.create_proof(params, plain, asg, 33, ws=pws)
    assert cases.verify_circuits(vk, cs, plain_proof, instances, logup=False) and shuffle_cases.verify_circuits(vk, cs, plain_proof, instances)
    assert not cases.verify_circuits(vk, cs, plain_proof, instances, logup=True)
    assert len(proof) == len(plain_proof) - 32 * 3 * L  # one commitment and two evaluations per lookup
    pws.release()
    plain.release()
    # a batch of one reproduces the single-circuit bytes (the batch kernel's logUp mode); another seed another proof
    assert custom.prove_many(keys, [asg], seeds=[33]) == proof
    other = custom.create_proof(params, keys, asg, 34, ws=ws)
    assert other != proof and cases.verify_circuits(vk, cs, other, instances, logup=True)
    _release(params, keys, ws)


@pytest.mark.parametrize("name", ["two", "mixed"])
def test_columns_of_a_proof_and_their_blinding_rows(gpu, name):
    """H2MI_BUF_LOGUP_M / _PHI row by row against the restatement over the Python compression of the assignment; phi[0] = phi[u] = 0;
    the blinding rows (M: rows u .., phi: rows u + 1 ..) are scalars that differ between seeds and lookups and repeat with the seed"""
    from halo2_scaffold_amd import engine

    custom, cs, asg, k, params, keys, vk = _case(gpu, name)
    n, L = 1 << k, len(cs.lookups)
    u = n - (cs.blinding_factors() + 1)
    ws = custom.Workspace(params, keys)
    blind = {}
    for seed in (3, 4, 3):
        trace = {}
        custom.create_proof(params, keys, asg, seed, trace=trace, ws=ws)
        tails = []
        for l, (ins, tabs) in enumerate(cases.lookup_rows(cs, asg, k)):
            a_rows, s_rows = [compress(t, trace["theta"]) for t in ins[:u]], [compress(t, trace["theta"]) for t in tabs[:u]]
            want_m, absent = cases.multiplicities(a_rows, s_rows, u)
            mult, phi = (_vals(ws.prover.views(kind, L)[l], n) for kind in (engine.BUF_LOGUP_M, engine.BUF_LOGUP_PHI))
            assert not absent and mult[:u] == want_m
            assert phi[: u + 1] == cases.running_sum(a_rows, s_rows, want_m, trace["beta"], u) and phi[0] == 0 and phi[u] == 0
            tails.append((mult[u:], phi[u + 1:]))
            assert len(set(mult[u:])) == n - u and len(set(phi[u + 1:])) == n - u - 1  # blinding scalars, not a fill
        if seed in blind:
            assert blind[seed] == tails
        blind[seed] = tails
    assert all(a != b for a, b in zip(blind[3], blind[4]))
    if L > 1:
        assert blind[3][0][0] != blind[3][1][0] and blind[3][0][1] != blind[3][1][1]
    with pytest.raises(Exception):
        ws.prover.views(engine.BUF_LOGUP_M, L + 1)[L]
    _release(params, keys, ws)


def test_buffer_kinds_belong_to_logup_keys(gpu):
    from halo2_scaffold_amd import engine

    custom, cs, asg, k, params, keys, vk = _case(gpu, "xor", logup=False)
    ws = custom.Workspace(params, keys)
    custom.create_proof(params, keys, asg, 5, ws=ws)
    for kind in (engine.BUF_LOGUP_M, engine.BUF_LOGUP_PHI):
        with pytest.raises(Exception):
            ws.prover.views(kind, 1)[0]
    _release(params, keys, ws)


# ---- 5. unsatisfied witnesses ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["xor", "mixed"])
def test_unsatisfied_lookup_is_refused_and_named(gpu, name):
    from halo2_scaffold_amd import custom, engine
    from halo2_scaffold_amd._lib import lib

    k = cases.CASES[name]
    if name == "xor":
        (cs, bad), good, row = lookup_cases.xor_circuit(custom, bad="different rows"), lookup_cases.xor_circuit(custom)[1], 3
    else:
        (cs, bad), good, row = cases.mixed_circuit(custom, bad=True), cases.mixed_circuit(custom)[1], 4
    _, params, keys, vk = _keys(gpu, cs, good, k, name)
    ws = custom.Workspace(params, keys)
    custom.check(params, keys, good, ws=ws)  # nothing to report
    with pytest.raises(ValueError, match="lookup 'xor' not satisfied at row %d" % row) as e:
        custom.check(params, keys, bad, ws=ws)
    assert [f.astuple() for f in e.value.failures] == [(engine.CHECK_LOOKUP, 0, row, 1)]
    with pytest.raises(ValueError, match="lookup input not in the table"):
        custom.create_proof(params, keys, bad, 9, ws=ws)
    # the C ABI itself: H2MI_EUNSAT from the lookups phase, and the proof is abandoned
    p = ws.prover
    pts, inst = np.zeros((16, 8), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64)
    from halo2_scaffold_amd import field as F

    cells, keep = engine.pack_cells(bad.advice)
    assert lib.h2mi_prover_advice(p.handle, cells, inst.ctypes.data, 0, 7, pts.ctypes.data) == 0
    th = F.fr_to_mont_limbs(11)
    assert lib.h2mi_prover_lookups(p.handle, th.ctypes.data, pts.ctypes.data) == engine.EUNSAT
    assert lib.h2mi_prover_products(p.handle, th.ctypes.data, th.ctypes.data, pts.ctypes.data) == -1
    del keep
    # the prover takes a fresh advice phase afterwards and proves a good witness: the bytes of an untouched prover
    proof = custom.create_proof(params, keys, good, 9, ws=ws)
    assert cases.verify_circuits(vk, cs, proof, [good.instance], logup=True) and proof == custom.create_proof(params, keys, good, 9)
    _release(params, keys, ws)


# ---- 6. the flag -----------------------------------------------------------------------------------------------------------------------
def test_flag_refusals_and_acceptance(gpu):
    """the flag with lookups == NULL is H2MI_EINVAL whatever else the record holds; beside a lookup program it is accepted, with phases
    and with H2MI_KEYGEN_VK_ONLY too"""
    from halo2_scaffold_amd import custom, engine
    from halo2_scaffold_amd._lib import check, lib

    cs, asg, k = cases.build(custom, "xor")
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    index = {col: j for j, col in enumerate(cs.perm_columns)}
    copies = np.ascontiguousarray(np.array([(index[(le[0], le[1])], le[2], index[(ri[0], ri[1])], ri[2]) for le, ri in asg.copies], dtype=np.uint32).reshape(-1, 4))
    cells, keep = engine.pack_cells(list(asg.fixed))
    abi, gates, lks = cs.abi(k), cs.gate_program(), cs.lookup_program()
    ph = engine.AdvicePhases.build([0] * cs.n_advice, [])
    common = dict(g_lagrange=params.g_lagrange_handle, fixed=cells, copies=copies.ctypes.data, n_copies=len(copies))
    flag = engine.KEYGEN_LOGUP
    assert keygen_call.keygen(abi, flags=flag, pk=0, **common)[0] == -1
    assert keygen_call.keygen(abi, gates=gates, flags=flag, pk=0, **common)[0] == -1
    assert keygen_call.keygen(abi, gates=gates, phases=ph, flags=flag, pk=0, **common)[0] == -1
    for more in (dict(flags=flag), dict(phases=ph, flags=flag), dict(flags=flag | engine.KEYGEN_VK_ONLY)):
        rc, handle = keygen_call.keygen(abi, gates=gates, lookups=lks, **more, **common)
        check(rc, "keygen")
        check(lib.h2mi_prover_pk_release(handle), "pk_release")
    del keep
    params.release()


# ---- 7. the goldens ---------------------------------------------------------------------------------------------------------------------
def test_golden_proofs_are_reproduced(gpu):
    """the XOR and mixed proofs of a logUp key at their seeds, byte for byte; and the XOR circuit under a key WITHOUT the flag against
    the bytes the library of the commit in front of the flag produced for it (`plain_xor`: tests/golden/make_logup_golden.py --plain-xor-only)"""
    g = json.load(open(os.path.join(GOLD, "logup_proofs.json")))
    assert sorted(c["circuit"] for c in g["cases"]) == ["mixed", "xor"] and int(g["srs_secret"], 16) == SRS_SECRET
    for entry in g["cases"]:
        custom, cs, asg, k, params, keys, vk = _case(gpu, entry["circuit"])
        assert k == entry["k"]
        proof = custom.create_proof(params, keys, asg, entry["seed"])
        assert proof.hex() == entry["proof"]
        _release(params, keys)
    entry = g["plain_xor"]
    custom, cs, asg, k, params, keys, vk = _case(gpu, "xor", logup=False)
    assert custom.create_proof(params, keys, asg, entry["seed"]).hex() == entry["proof"]
    _release(params, keys)
