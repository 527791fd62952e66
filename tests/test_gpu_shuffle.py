"""The shuffle argument on the device, bit for bit against the Python integers of tests/shuffle_cases.py: h2mi_plonk_shuffle_product_dev
around the scan tile; the quotient kernels (k_evaluate_h_expr, k_evaluate_h_expr_batch) with shuffle terms, recovered from H2MI_BUF_H on
every extended-coset point; proofs of every case accepted by the generalised verifier and rejected when a shuffle commitment or a
shuffle evaluation is tampered with; the product column's recurrence, blinding and determinism; the witness check's report and the
refusal of an unsatisfied shuffle; the committed golden."""
import json
import os
import random

import numpy as np
import pytest

import custom_gate_cases as gate_cases
import keygen_call
import shuffle_cases as cases
from lookup_expr_cases import compress
from oracle import bn254 as o
from oracle import flex as FX

pytestmark = pytest.mark.gpu

R = o.R
SRS_SECRET = 0x5EC2E7 + 0x48324D49
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _vals(buf, count):
    return o.unpack(buf.to_numpy(shape=(count, 4), nbytes=count * 32), R)


# ---- 1. the product, through h2mi_plonk_shuffle_product_dev --------------------------------------------------------------------------
# (k, usable rows): one workgroup; the scan tile MS_TILE = 1024 exactly and one beyond it; eight tiles with a ragged last one
PRODUCT_CASES = [(5, 22), (11, 1024), (11, 1025), (13, (1 << 13) - 7)]


@pytest.mark.parametrize("k,u", PRODUCT_CASES)
def test_shuffle_product_against_python_integers(gpu, k, u):
    from halo2_scaffold_amd import plonk
    from halo2_scaffold_amd.device import DevBuf

    n = 1 << k
    rng = random.Random(7000 + u)
    a = [rng.choice([0, 1, R - 1, rng.randrange(R)]) if rng.random() < 0.3 else rng.randrange(R) for _ in range(n)]
    s = a[:u]
    rng.shuffle(s)
    s += [rng.randrange(R) for _ in range(n - u)]  # rows beyond u are not read
    gamma = rng.randrange(R)
    sentinel = [rng.randrange(R) for _ in range(n)]
    d_a, d_s, d_z = DevBuf.from_numpy(o.pack(a, R)), DevBuf.from_numpy(o.pack(s, R)), DevBuf.from_numpy(o.pack(sentinel, R))
    assert plonk.shuffle_product(k, d_a, d_s, gamma, u, d_z) is True
    got = _vals(d_z, n)
    want = cases.shuffle_product(a, s, gamma, u)
    assert want[u] == 1 and got[: u + 1] == want
    assert got[u + 1:] == sentinel[u + 1:]  # the blinding rows are the caller's
    # an unequal multiset: H2MI_EUNSAT, with z written all the same
    s[u // 2] = (s[u // 2] + 1) % R
    d_s2 = DevBuf.from_numpy(o.pack(s, R))
    assert plonk.shuffle_product(k, d_a, d_s2, gamma, u, d_z) is False
    want = cases.shuffle_product(a, s, gamma, u)
    assert want[u] != 1 and _vals(d_z, n)[: u + 1] == want
    for b in (d_a, d_s, d_s2, d_z):
        b.free()


def test_shuffle_product_refusals(gpu):
    from halo2_scaffold_amd._lib import lib
    from halo2_scaffold_amd.device import DevBuf
    from halo2_scaffold_amd import field as F

    buf = DevBuf(32 * 32)
    g = F.fr_to_mont_limbs(5)
    assert lib.h2mi_plonk_shuffle_product_dev(None, buf.ptr, 5, 22, g.ctypes.data, buf.ptr, None) == -1
    assert lib.h2mi_plonk_shuffle_product_dev(buf.ptr, buf.ptr, 5, 22, None, buf.ptr, None) == -1
    assert lib.h2mi_plonk_shuffle_product_dev(buf.ptr, buf.ptr, 5, 32, g.ctypes.data, buf.ptr, None) == -6
    assert lib.h2mi_plonk_shuffle_product_dev(buf.ptr, buf.ptr, 5, 0, g.ctypes.data, buf.ptr, None) == -6
    buf.free()


# ---- helpers: keys, and a proof's vectors in Python integers --------------------------------------------------------------------------
def _keys(gpu, cs, first, k, name):
    from halo2_scaffold_amd import custom

    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    keys = custom.Keys(params, cs, first)
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
    """custom.Expression list -> the theta-compressed column on the extended coset, point by point: a rotation r reads idx + r rot"""
    out = []
    for idx in range(size):
        q = lambda kind, c, r: cols[kind][c][(idx + r * rot) % size]
        out.append(compress([e.evaluate(q, challenges) for e in exprs], theta))
    return out


def _coset_circuit(cs, keys, prover, k, theta, challenges=()):
    """every vector the quotient reads for one circuit, recomputed in Python integers on the extended coset from the ROW buffers of the
    prover (advice, products, permuted lookup columns) and of the key: -> (circuit dict, shared dict) as shuffle_cases.batched_quotient
    takes them.  Nothing here is read from a device coset buffer."""
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
        a_in = _compress_coset([a for a, _ in pairs], by_kind, size, rot, theta, challenges)
        t_in = _compress_coset([t for _, t in pairs], by_kind, size, rot, theta, challenges)
        pin, ptab, lz = (ext(_vals(prover.views(kind, L)[l], n)) for kind in (engine.BUF_LOOKUP_PERMUTED_INPUT, engine.BUF_LOOKUP_PERMUTED_TABLE,
                                                                             engine.BUF_LOOKUP_Z))
        lookups.append((a_in, None, t_in, pin, ptab, lz))
    shuffles = []
    for i, pairs in enumerate(cs.shuffles):
        a_in = _compress_coset([a for a, _ in pairs], by_kind, size, rot, theta, challenges)
        s_in = _compress_coset([s for _, s in pairs], by_kind, size, rot, theta, challenges)
        shuffles.append((a_in, s_in, ext(_vals(prover.views(engine.BUF_SHUFFLE_Z, S)[i], n))))
    u = n - (cs.blinding_factors() + 1)
    unit = lambda row: [1 if i == row else 0 for i in range(n)]
    shared = {"perm_sigmas": sigma, "chunk": chunk, "l0": ext(unit(0)), "l_last": ext(unit(u)), "l_active": ext([1] * u + [0] * (n - u))}
    circuit = {"advice": advice, "fixed": fixed, "instance": instance, "perm_values": perm_values, "perm_zs": perm_zs, "lookups": lookups,
               "shuffles": shuffles}
    return circuit, shared, dom


def _h_on_the_coset(prover, dom):
    """H2MI_BUF_H holds the quotient's coefficients (the kernel's output through the inverse transform, a bijection): back on the
    extended coset they are the kernel's values"""
    from halo2_scaffold_amd import engine

    size = 1 << dom.extended_k
    return dom.coeff_to_extended(_vals(prover.view(engine.BUF_H), size))


def _check_quotient(cs, keys, provers, k, trace):
    ops, consts = cs.program()
    built = [_coset_circuit(cs, keys, p, k, trace["theta"]) for p in provers]
    shared, dom = built[0][1], built[0][2]
    want = cases.batched_quotient(k, dom.extended_k, dom.g_coset, dom.extended_omega, cases.keys_delta(), cs.blinding_factors(), ops, consts, [],
                                  [b[0] for b in built], shared, trace["beta"], trace["gamma"], trace["y"])
    got = _h_on_the_coset(provers[0], dom)
    assert len(want) == 1 << dom.extended_k and got == want
    without = cases.batched_quotient(k, dom.extended_k, dom.g_coset, dom.extended_omega, cases.keys_delta(), cs.blinding_factors(), ops, consts, [],
                                     [dict(b[0], shuffles=[]) for b in built], shared, trace["beta"], trace["gamma"], trace["y"])
    assert without != want  # the shuffle terms are in h


# ---- 2. the quotient --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["perm", "mixed"])
def test_quotient_with_shuffle_terms_single(gpu, name):
    """k_evaluate_h_expr: every extended-coset point against batched_quotient with shuffle_terms"""
    custom, cs, asg, k, params, keys, vk = _case(gpu, name)
    ws = custom.Workspace(params, keys)
    trace = {}
    proof = custom.create_proof(params, keys, asg, 21, trace=trace, ws=ws)
    assert cases.verify_circuits(vk, cs, proof, [asg.instance])
    _check_quotient(cs, keys, [ws.prover], k, trace)
    _release(params, keys, ws)


def test_quotient_with_shuffle_terms_batch(gpu):
    """k_evaluate_h_expr_batch on mixed x 2: one accumulator over both circuits' gate, permutation, lookup and shuffle terms"""
    from halo2_scaffold_amd import custom

    built = [cases.mixed_circuit(custom, variant=v) for v in (0, 1)]
    cs, asgs = built[0][0], [a for _, a in built]
    _, params, keys, vk = _keys(gpu, cs, asgs[0], 6, "mixed")
    ws = custom.BatchWorkspace(params, keys, 2)
    trace = {}
    proof = custom.prove_many(keys, asgs, seeds=[5, 13], ws=ws, trace=trace)
    assert cases.verify_circuits(vk, cs, proof, [a.instance for a in asgs])
    _check_quotient(cs, keys, ws.provers, 6, trace)
    _release(params, keys, ws)


# ---- 3. proofs ------------------------------------------------------------------------------------------------------------------------
def _flips_rejected(vk, cs, proof, instances, n_circuits=1):
    commitment, evaluation = cases.proof_offsets(cs, n_circuits)
    S = len(cs.shuffles)
    for at in (commitment + 5, commitment + 32 * (n_circuits * S - 1) + 9, evaluation + 3, evaluation + 32 * (2 * n_circuits * S - 1) + 1):
        flipped = bytearray(proof)
        flipped[at] ^= 1
        assert not cases.verify_circuits(vk, cs, bytes(flipped), instances), at


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_proofs_are_accepted_and_tampering_is_rejected(gpu, name):
    from halo2_scaffold_amd import engine

    custom, cs, asg, k, params, keys, vk = _case(gpu, name)
    first = cases.first_assignment(cs, asg)
    ws = custom.Workspace(params, keys)
    proof = custom.create_proof(params, keys, asg, 33, ws=ws)
    instances = [first.instance]
    assert cases.verify_circuits(vk, cs, proof, instances)
    _flips_rejected(vk, cs, proof, instances)
    m, chunk = len(cs.perm_columns), cs.degree() - 2
    want = cases.num_evaluations(1, len(cs.advice_queries), len(cs.fixed_queries), m, -(-m // chunk), len(cs.lookups), len(cs.shuffles))
    assert ws.prover.counts.evaluations == want
    assert ws.prover.counts.products == -(-m // chunk) + len(cs.lookups) + len(cs.shuffles) + 1
    # a batch of one reproduces the single-circuit bytes; two provers with the same seed the same proof
    assert custom.prove_many(keys, [asg], seeds=[33]) == proof
    assert custom.create_proof(params, keys, asg, 33) == proof
    other = custom.create_proof(params, keys, asg, 34, ws=ws)
    assert other != proof and cases.verify_circuits(vk, cs, other, instances)
    assert isinstance(engine.BUF_SHUFFLE_Z, int)
    _release(params, keys, ws)


def test_batch_of_two_is_accepted_and_tampering_is_rejected(gpu):
    from halo2_scaffold_amd import custom

    built = [cases.mixed_circuit(custom, variant=v) for v in (0, 1)]
    cs, asgs = built[0][0], [a for _, a in built]
    _, params, keys, vk = _keys(gpu, cs, asgs[0], 6, "mixed")
    ws = custom.BatchWorkspace(params, keys, 2)
    proof = custom.prove_many(keys, asgs, seeds=[40, 48], ws=ws)
    instances = [a.instance for a in asgs]
    assert cases.verify_circuits(vk, cs, proof, instances)
    _flips_rejected(vk, cs, proof, instances, 2)
    m, chunk = len(cs.perm_columns), cs.degree() - 2
    assert ws.batch.n_evaluations == cases.num_evaluations(2, len(cs.advice_queries), len(cs.fixed_queries), m, -(-m // chunk), len(cs.lookups),
                                                           len(cs.shuffles))
    assert ws.provers[0].counts.products == ws.provers[1].counts.products + 1
    assert not cases.verify_circuits(vk, cs, proof, instances[:1])
    _release(params, keys, ws)


# ---- 4. the product column of a proof ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tuple", "mixed"])
def test_shuffle_z_recurrence_and_blinding(gpu, name):
    """H2MI_BUF_SHUFFLE_Z row by row: z[0] = 1, z[i+1] (S_i + gamma) = z[i] (A_i + gamma), z[u] = 1, with A and S the compressed rows
    (H2MI_BUF_SHUFFLE_INPUT / _TABLE, themselves against the Python compression on the usable rows); the blinding rows differ between
    seeds and repeat with the seed"""
    from halo2_scaffold_amd import engine

    custom, cs, asg, k, params, keys, vk = _case(gpu, name)
    n, S = 1 << k, len(cs.shuffles)
    u = n - (cs.blinding_factors() + 1)
    ws = custom.Workspace(params, keys)
    blind = {}
    for seed in (3, 4, 3):
        trace = {}
        custom.create_proof(params, keys, asg, seed, trace=trace, ws=ws)
        rows = cases.shuffle_rows(cs, asg, k)
        tails = []
        for i in range(S):
            z = _vals(ws.prover.views(engine.BUF_SHUFFLE_Z, S)[i], n)
            a_rows, s_rows = (_vals(ws.prover.views(kind, S)[i], n) for kind in (engine.BUF_SHUFFLE_INPUT, engine.BUF_SHUFFLE_TABLE))
            # on the usable rows the compression of the assignment (the blinding rows of the advice columns hold blinding scalars)
            assert a_rows[:u] == [compress(t, trace["theta"]) for t in rows[i][0][:u]]
            assert s_rows[:u] == [compress(t, trace["theta"]) for t in rows[i][1][:u]]
            assert z[0] == 1 and z[u] == 1
            for r in range(u):
                assert z[r + 1] * (s_rows[r] + trace["gamma"]) % R == z[r] * (a_rows[r] + trace["gamma"]) % R, (i, r)
            assert z[: u + 1] == cases.shuffle_product(a_rows, s_rows, trace["gamma"], u)
            tails.append(z[u + 1:])
            assert len(set(z[u + 1:])) == n - u - 1  # blinding scalars, not a fill
        if seed in blind:
            assert blind[seed] == tails
        blind[seed] = tails
    assert all(a != b for a, b in zip(blind[3], blind[4]))
    if S > 1:
        assert blind[3][0] != blind[3][1]
    with pytest.raises(Exception):
        ws.prover.views(engine.BUF_SHUFFLE_Z, S + 1)[S]
    _release(params, keys, ws)


# ---- 5. unsatisfied witnesses ----------------------------------------------------------------------------------------------------------
def _unsatisfied(custom):
    return {"cell": (cases.perm_circuit(custom, bad="cell"), cases.perm_circuit(custom)[1], 5),
            "multiplicity": (cases.perm_circuit(custom, bad="multiplicity"), cases.perm_circuit(custom)[1], 5),
            "second of two": (cases.mixed_circuit(custom, bad=1), cases.mixed_circuit(custom)[1], 6)}


@pytest.mark.parametrize("which", ["cell", "multiplicity", "second of two"])
def test_unsatisfied_shuffle_is_reported_and_refused(gpu, which):
    from halo2_scaffold_amd import custom, engine

    (cs, bad), good, k = _unsatisfied(custom)[which]
    _, params, keys, vk = _keys(gpu, cs, good, k, which)
    want = cases.expected_failures(cs, bad, k)
    assert len(want) == 1
    ws = custom.Workspace(params, keys)
    custom.check(params, keys, good, ws=ws)  # nothing to report
    with pytest.raises(ValueError, match="shuffle .* not satisfied") as e:
        custom.check(params, keys, bad, ws=ws)
    got = [f.astuple() for f in e.value.failures]
    assert got == [(engine.CHECK_SHUFFLE, *want[0])]
    if which == "multiplicity":
        assert want[0] == (0, 0, 2)
    # the products phase compares z[u] with one and abandons the proof
    with pytest.raises(ValueError, match="shuffle"):
        custom.create_proof(params, keys, bad, 9, ws=ws)
    # the prover takes a fresh advice phase afterwards and proves a good witness: the bytes of an untouched prover
    proof = custom.create_proof(params, keys, good, 9, ws=ws)
    assert cases.verify_circuits(vk, cs, proof, [good.instance]) and proof == custom.create_proof(params, keys, good, 9)
    _release(params, keys, ws)


def test_products_return_eunsat_and_need_theta(gpu):
    """the C ABI itself: h2mi_prover_products on an unsatisfied shuffle is H2MI_EUNSAT; on a key with shuffles it is H2MI_EINVAL
    without the h2mi_prover_lookups call that carries theta"""
    from halo2_scaffold_amd import custom, engine
    from halo2_scaffold_amd import field as F
    from halo2_scaffold_amd._lib import lib

    (cs, bad), good, k = _unsatisfied(custom)["cell"]
    _, params, keys, vk = _keys(gpu, cs, good, k, "cell")
    p = engine.Prover(keys.keys, params)
    pts = np.zeros((8, 8), dtype=np.uint64)
    limbs = lambda v: F.fr_to_mont_limbs(v)
    th, be, ga = limbs(11), limbs(12), limbs(13)
    inst = np.zeros((1, 4), dtype=np.uint64)

    def advice(asg):
        cells, keep = engine.pack_cells(asg.advice)
        assert lib.h2mi_prover_advice(p.handle, cells, inst.ctypes.data, 0, 7, pts.ctypes.data) == 0
        del keep

    advice(bad)
    assert lib.h2mi_prover_lookups(p.handle, th.ctypes.data, pts.ctypes.data) == 0
    assert lib.h2mi_prover_products(p.handle, be.ctypes.data, ga.ctypes.data, pts.ctypes.data) == engine.EUNSAT
    assert lib.h2mi_prover_products(p.handle, be.ctypes.data, ga.ctypes.data, pts.ctypes.data) == -1  # abandoned
    advice(good)
    assert lib.h2mi_prover_products(p.handle, be.ctypes.data, ga.ctypes.data, pts.ctypes.data) == -1  # theta has not arrived
    advice(good)
    assert lib.h2mi_prover_lookups(p.handle, None, pts.ctypes.data) == -1
    advice(good)
    assert lib.h2mi_prover_lookups(p.handle, th.ctypes.data, pts.ctypes.data) == 0
    assert lib.h2mi_prover_products(p.handle, be.ctypes.data, ga.ctypes.data, pts.ctypes.data) == 0
    assert p.counts.products == 2 and p.counts.lookups == 0
    p.release()
    _release(params, keys)


def test_keygen_without_shuffles_is_the_existing_key(gpu):
    """a raw record with shuffles == NULL (and every other optional field NULL) makes the key custom.Keys makes: the same proof bytes"""
    from halo2_scaffold_amd import custom, engine
    from halo2_scaffold_amd._lib import check, lib

    cs, asg = gate_cases.is_zero_circuit(custom, 5)
    params = gpu.ParamsKZG.setup(5, SRS_SECRET)
    keys = custom.Keys(params, cs, asg)
    want = custom.create_proof(params, keys, asg, 77)
    index = {col: j for j, col in enumerate(cs.perm_columns)}
    copies = np.ascontiguousarray(np.array([(index[(le[0], le[1])], le[2], index[(ri[0], ri[1])], ri[2]) for le, ri in asg.copies], dtype=np.uint32).reshape(-1, 4))
    cells, keep = engine.pack_cells(list(asg.fixed))
    abi, gates = cs.abi(5), cs.gate_program()
    rc, handle = keygen_call.keygen(abi, gates=gates, g_lagrange=params.g_lagrange_handle, fixed=cells, copies=copies.ctypes.data, n_copies=len(copies))
    check(rc, "keygen")
    old = keys.keys.handle
    keys.keys.handle = handle  # the same wrapper over the other key
    try:
        assert custom.create_proof(params, keys, asg, 77) == want
    finally:
        for pr in list(keys.keys._provers):
            pr.release()
        check(lib.h2mi_prover_pk_release(handle), "pk_release")
        keys.keys.handle = old
    _release(params, keys)


# ---- 6. the golden ----------------------------------------------------------------------------------------------------------------------
def test_golden_proofs_are_reproduced(gpu):
    g = json.load(open(os.path.join(GOLD, "shuffle_proofs.json")))
    assert sorted(c["circuit"] for c in g["cases"]) == ["mixed", "perm", "phased"]
    for entry in g["cases"]:
        custom, cs, asg, k, params, keys, vk = _case(gpu, entry["circuit"])
        assert k == entry["k"] and int(g["srs_secret"], 16) == SRS_SECRET
        proof = custom.create_proof(params, keys, asg, entry["seed"])
        assert proof.hex() == entry["proof"]
        _release(params, keys)
