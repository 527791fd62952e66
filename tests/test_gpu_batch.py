"""Several circuits per proof on the device: k_evaluate_h_expr_batch (csrc/h2mi_plonk.hip) bit for bit against the Python-integer
batched quotient of tests/batch_cases.py, against the single-circuit kernel the goldens pin, and its refusals; a batch of one giving the
bytes of the existing route; batches of two, three circuits of the reference's is_zero / or circuits, a multi-expression lookup, a
degree-6 circuit with public inputs, a two-phase circuit and StandardPlonk accepted by the N-circuit verifier of tests/batch_cases.py
and rejected when tampered with; the members' independence; the witness check per member; the order and argument errors."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest

import batch_cases as cases
import custom_gate_cases as gate_cases
import lookup_expr_cases as lookup_cases
import phase_cases
from oracle import bn254 as o
from oracle import flex as FX

pytestmark = pytest.mark.gpu

R = o.R
SRS_SECRET = 0x5EC2E7 + 0x48324D49
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EINVAL, EHANDLE = -1, -5


def _vals(buf, count):
    return o.unpack(buf.to_numpy(shape=(count, 4), nbytes=count * 32), R)


# ---- 1. the kernel, through h2mi_plonk_evaluate_h_expr_batch_dev ---------------------------------------------------------------------
def _device_case(gpu, kc):
    """the columns of a batch_cases.kernel_case on the device; one Python list is one buffer, so circuits that share a column share a
    pointer -> (domain, ops, constants, program, per-circuit dicts of DevBuf, shared DevBufs)"""
    from halo2_scaffold_amd import engine
    from halo2_scaffold_amd.device import DevBuf

    bufs = {}

    def dev(col):
        if col is None:
            return None
        if id(col) not in bufs:
            bufs[id(col)] = DevBuf.from_numpy(o.pack(col, R))
        return bufs[id(col)]

    constants, ops = {}, []
    for t in kc["trees"]:
        ops += t.program(constants)[0]
    consts = sorted(constants, key=constants.get)
    prog = engine.GateProgram.build(ops, consts)
    circuits = [{"advice": [dev(c) for c in cc["advice"]], "fixed": [dev(c) for c in cc["fixed"]], "instance": dev(cc["instance"]),
                 "perm_values": [dev(c) for c in cc["perm_values"]], "perm_zs": [dev(c) for c in cc["perm_zs"]],
                 "lookups": [tuple(dev(c) for c in lk) for lk in cc["lookups"]]} for cc in kc["circuits"]]
    sh = kc["shared"]
    shared = {"perm_sigmas": [dev(c) for c in sh["perm_sigmas"]], "l0": dev(sh["l0"]), "l_last": dev(sh["l_last"]), "l_active": dev(sh["l_active"])}
    dom = gpu.EvaluationDomain(kc["degree"], kc["k"])
    assert dom.extended_k == kc["extended_k"]
    return dom, ops, consts, prog, circuits, shared


@pytest.mark.parametrize("case", range(len(cases.KERNEL_CASES)))
def test_batch_kernel_against_python_integers(gpu, case):
    """every element of h, exactly; with one circuit the words of h2mi_plonk_evaluate_h_expr_dev; with three circuits also
    sum_i y^(T (N - 1 - i)) H_i over the single-circuit call's outputs H_i (T: the Horner terms of one circuit)"""
    from halo2_scaffold_amd import custom, plonk
    from halo2_scaffold_amd.device import DevBuf

    kc = cases.kernel_case(custom, case)
    dom, ops, consts, prog, circuits, sh = _device_case(gpu, kc)
    k, ext_k, N, chunk = kc["k"], kc["extended_k"], len(circuits), kc["shared"]["chunk"]
    size = 1 << ext_k
    beta, gamma, y, ch = kc["beta"], kc["gamma"], kc["y"], kc["challenges"]
    arr = plonk.expr_cosets_array(circuits, sh["perm_sigmas"], chunk, sh["l0"], sh["l_last"], sh["l_active"])
    out = DevBuf(size * 32)
    plonk.evaluate_h_expr_batch(dom, prog, arr, N, beta, gamma, y, out, blinding_factors=kc["bf"], challenges=ch)
    want = cases.batched_quotient(k, ext_k, dom.g_coset, dom.extended_omega, cases.keys_delta(), kc["bf"], ops, consts, ch, kc["circuits"], kc["shared"],
                                  beta, gamma, y)
    assert _vals(out, size) == want
    if len({id(c["advice"][0]) for c in kc["circuits"]}) < N:  # shared advice: folded once per circuit, not once per pointer
        once = cases.batched_quotient(k, ext_k, dom.g_coset, dom.extended_omega, cases.keys_delta(), kc["bf"], ops, consts, ch, kc["circuits"][:1],
                                      kc["shared"], beta, gamma, y)
        assert want != once

    def single(c):
        h = DevBuf(size * 32)
        plonk.evaluate_h_expr(dom, prog, c["advice"], c["fixed"], c["instance"], c["perm_values"], sh["perm_sigmas"], c["perm_zs"], chunk, c["lookups"],
                              sh["l0"], sh["l_last"], sh["l_active"], beta, gamma, y, h, blinding_factors=kc["bf"], challenges=ch)
        return h

    one = DevBuf(size * 32)
    plonk.evaluate_h_expr_batch(dom, prog, arr, 1, beta, gamma, y, one, blinding_factors=kc["bf"], challenges=ch)
    assert (one.to_numpy() == single(circuits[0]).to_numpy()).all()
    if N == 3:
        T = cases.horner_terms(len(kc["trees"]), len(kc["shared"]["perm_sigmas"]), chunk, len(kc["circuits"][0]["lookups"]))
        hs = [_vals(single(c), size) for c in circuits]
        assert want == [sum(pow(y, T * (N - 1 - i), R) * hs[i][idx] for i in range(N)) % R for idx in range(size)]


def test_batch_kernel_cases_cover_what_they_should(h2):
    from halo2_scaffold_amd import custom

    sizes, ns, depths, with_ch, perms, lks, shared = set(), set(), set(), set(), set(), set(), 0
    for case, (k, degree, n, depth, ch, n_perm, chunk, n_lookups, share) in enumerate(cases.KERNEL_CASES):
        kc = cases.kernel_case(custom, case)
        sizes.add(1 << kc["extended_k"])
        ns.add(len(kc["circuits"]))
        depths.add((max(t.stack_depth() for t in kc["trees"]), ch))
        perms.add(-(-n_perm // chunk) if n_perm else 0)
        lks.add(n_lookups)
        shared += share is not None
        assert 4 <= k <= 6 and kc["extended_k"] - k in (1, 2, 3)
        if n_lookups:
            assert any(lk[1] is not None for lk in kc["circuits"][0]["lookups"]) and any(lk[1] is None for lk in kc["circuits"][0]["lookups"])
    assert sizes >= {32, 256, 512} and ns == {1, 2, 3, 8} and depths == {(1, False), (1, True), (8, False), (8, True)}
    assert perms == {0, 2} and lks == {0, 2} and shared >= 3


def test_batch_entry_refusals(gpu):
    from halo2_scaffold_amd import custom, plonk
    from halo2_scaffold_amd._lib import H2miError
    from halo2_scaffold_amd.device import DevBuf

    kc = cases.kernel_case(custom, 3)  # three circuits, two permutation sets, two lookups
    dom, ops, consts, prog, circuits, sh = _device_case(gpu, kc)
    chunk = kc["shared"]["chunk"]
    out = DevBuf((1 << kc["extended_k"]) * 32)
    fresh = lambda cs=circuits: plonk.expr_cosets_array(cs, sh["perm_sigmas"], chunk, sh["l0"], sh["l_last"], sh["l_active"])

    def refused(arr, n):
        with pytest.raises(H2miError) as e:
            plonk.evaluate_h_expr_batch(dom, prog, arr, n, kc["beta"], kc["gamma"], kc["y"], out, blinding_factors=kc["bf"], challenges=kc["challenges"])
        return e.value.code == EINVAL

    plonk.evaluate_h_expr_batch(dom, prog, fresh(), 3, kc["beta"], kc["gamma"], kc["y"], out, blinding_factors=kc["bf"], challenges=kc["challenges"])
    assert refused(fresh(), 0)
    assert refused(fresh([circuits[i % 3] for i in range(9)]), 9)
    plonk.evaluate_h_expr_batch(dom, prog, fresh([circuits[i % 3] for i in range(8)]), 8, kc["beta"], kc["gamma"], kc["y"], out, blinding_factors=kc["bf"])
    for field, value in (("n_perm", 2), ("chunk_len", chunk + 1), ("n_lookups", 1)):
        arr = fresh()
        setattr(arr[1], field, value)
        assert refused(arr, 3), field
    read = next(index for op, index, _ in ops if op == cases.OP_ADVICE)
    for poke in (lambda e: e.advice.__setitem__(read, None), lambda e: e.perm_z.__setitem__(1, None), lambda e: e.perm_value.__setitem__(0, None),
                 lambda e: e.lookup_z.__setitem__(1, None), lambda e: setattr(e, "l0", None), lambda e: e.perm_sigma.__setitem__(0, None)):
        for entry in (0, 2):
            arr = fresh()
            poke(arr[entry])
            assert refused(arr, 3)
    arr = fresh()
    arr[2].lookup_input_b[0] = None  # optional: accepted
    arr[2].lookup_input_b[1] = None
    plonk.evaluate_h_expr_batch(dom, prog, arr, 3, kc["beta"], kc["gamma"], kc["y"], out, blinding_factors=kc["bf"])
    assert refused(None, 1)  # no entries at all


# ---- 2. proofs ----------------------------------------------------------------------------------------------------------------------
def _keys(gpu, cs, first, k, name="batch"):
    """-> (custom, params, keys, vk): the library's key and the restated verifying key for one custom.ConstraintSystem"""
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


def _flips_rejected(vk, cs, proof, instances, offsets):
    for at in offsets:
        flipped = bytearray(proof)
        flipped[at] ^= 1
        assert not cases.verify_circuits(vk, cs, bytes(flipped), instances), at


@pytest.mark.parametrize("name", ["is_zero", "xor"])
def test_batch_of_one_gives_the_existing_bytes(gpu, name):
    from halo2_scaffold_amd import custom

    cs, asg = gate_cases.is_zero_circuit(custom, 5) if name == "is_zero" else lookup_cases.xor_circuit(custom)
    _, params, keys, vk = _keys(gpu, cs, asg, 5)
    want = custom.create_proof(params, keys, asg, 77)
    assert custom.prove_many(keys, [asg], seeds=[77]) == want
    assert cases.verify_circuits(vk, cs, want, [asg.instance])
    _release(params, keys)


def test_batch_of_one_reproduces_a_range_golden(gpu):
    """a flex key (hard-wired vertical gates, three gate columns and a lookup-advice column): the batch quotient runs the shape's
    equivalent program, and the proof is the committed one byte for byte"""
    from halo2_scaffold_amd import custom, flex

    g = json.load(open(os.path.join(GOLD, "flex_multi_proofs.json")))
    case = next(c for c in g["cases"] if c["shape"] == "range" and c["k"] == 5)
    x, bits, k = int(case["x"], 16), case["lookup_bits"], case["k"]
    closure = lambda cs: flex.range_closure(cs, x, bits)
    cs = flex.configure(True, k, closure)
    asg = closure(cs)
    params = gpu.ParamsKZG.setup(k, int(g["srs_secret"], 16))
    keys = flex.FlexKeys(params, cs, asg)
    assert keys.vk_bytes().hex() == case["vk_bytes"]
    assert custom.prove_many(keys, [asg], seeds=[case["seed"]], params=params).hex() == case["proof"]
    _release(params, keys)


def _is_zero(custom, xs):
    built = [gate_cases.is_zero_circuit(custom, x) for x in xs]
    return built[0][0], [a for _, a in built]


def _or(custom, pairs):
    built = [gate_cases.or_circuit(custom, a, b) for a, b in pairs]
    return built[0][0], [a for _, a in built]


def _xor(custom, triple_sets):
    built = [lookup_cases.xor_circuit(custom, triples=t) for t in triple_sets]
    return built[0][0], [a for _, a in built]


def _degree6(custom, firsts):
    built = [gate_cases.degree6_circuit(custom, a0, 11) for a0 in firsts]
    return built[0][0], [a for _, a in built]


XOR_SETS = [((1, 2, 3), (3, 3, 0), (0, 2, 2), (2, 1, 3)), ((0, 0, 0), (1, 1, 0), (3, 0, 3), (2, 3, 1)), ((3, 1, 2), (2, 2, 0), (1, 3, 2), (0, 1, 1))]
ACCEPTED = {
    "is_zero x 2": (lambda c: _is_zero(c, [0, 0x1234567]), 4),
    "or x 3": (lambda c: _or(c, [(1, 1), (0, 1), (0, 0)]), 5),
    "xor x 3": (lambda c: _xor(c, XOR_SETS), 5),
    "degree6 x 2": (lambda c: _degree6(c, [3, 4]), 4),
}


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_batches_are_accepted_and_tampering_is_rejected(gpu, name):
    from halo2_scaffold_amd import custom
    from halo2_scaffold_amd import field as F

    build, k = ACCEPTED[name]
    cs, asgs = build(custom)
    for a in asgs:
        custom.mock(a, k)
    _, params, keys, vk = _keys(gpu, cs, asgs[0], k, name)
    ws = custom.BatchWorkspace(params, keys, len(asgs))
    instances = [a.instance for a in asgs]
    trace = {}
    proof = custom.prove_many(keys, asgs, ws=ws, trace=trace)
    assert cases.verify_circuits(vk, cs, proof, instances)
    n_points = len(asgs) * (cs.n_advice + 3 * len(cs.lookups)) + len(asgs) * (-(-len(cs.perm_columns) // (cs.degree() - 2))) + 1 + cs.degree() - 1
    assert len(proof) == 32 * (n_points + ws.batch.n_evaluations + 2)
    _flips_rejected(vk, cs, proof, instances, [3, 32 * cs.n_advice + 3, 32 * n_points + 5, len(proof) - 1])
    if any(instances):  # another circuit's public inputs
        assert instances[0] != instances[1] and not cases.verify_circuits(vk, cs, proof, instances[::-1])
    assert not cases.verify_circuits(vk, cs, proof, instances[:-1]) and custom.prove_many(keys, asgs, ws=ws) == proof
    # the library handed another y than the transcript's
    other = custom.prove_many(keys, asgs, ws=ws, hooks={"y": lambda y: F.fr_to_mont_limbs((F.fr_from_mont_limbs(y) + 1) % R)})
    assert len(other) == len(proof) and other != proof and not cases.verify_circuits(vk, cs, other, instances)
    _release(params, keys, ws)


def test_two_phase_batch(gpu):
    """the running linear combination twice: both circuits' phase-0 commitments precede the challenge, which both then use"""
    from halo2_scaffold_amd import custom

    values = [phase_cases.RLC_VALUES, (7, R - 1, 0, 2, 2, 9, 1, 5)]
    built = [phase_cases.rlc_circuit(custom, values=v) for v in values]
    cs, syns = built[0][0], [s for _, s in built]
    first = syns[0]([None])
    _, params, keys, vk = _keys(gpu, cs, first, 5, "rlc")
    seen, got, trace = [[], []], [], {}
    wrap = lambda i: (lambda ch: seen[i].append(ch) or syns[i](ch))
    proof = custom.prove_many(keys, [wrap(0), wrap(1)], trace=trace)
    assert cases.verify_circuits(vk, cs, proof, [[], []], got)
    (gamma,) = got
    assert seen == [[[None], [gamma]], [[None], [gamma]]] and trace["challenges"] == [gamma]
    for s in syns:
        custom.mock(s([gamma]), 5, [gamma])
    _flips_rejected(vk, cs, proof, [[], []], [3, 32 + 3, 64 + 3, 96 + 3])  # a, a' (phase 0), acc, acc' (phase 1)
    alone = custom.create_proof(params, keys, syns[0], 1)
    assert alone[:32] == proof[:32]  # circuit 0's phase-0 commitment: the same witness and seed proved alone
    _release(params, keys)


def test_standard_plonk_batch(gpu):
    """a key of the hard-wired StandardPlonk shape at k = 5: two witnesses in one proof through the shape's equivalent program; a batch
    of one gives the bytes of the shape's own kernel"""
    from halo2_scaffold_amd import circuits, custom, keygen, prover

    params = gpu.ParamsKZG.setup(5, SRS_SECRET)
    circuit = circuits.StandardPlonk(None)
    pk = keygen.keygen_pk(params, keygen.keygen_vk(params, circuit), circuit)
    keys = types.SimpleNamespace(keys=pk.keys, transcript_repr=pk.vk.transcript_repr)
    ocs = FX.standard_plonk_cs()
    oasg = FX.standard_plonk_assignment(ocs, 3)
    vk = FX.VerifierKeys(ocs, 5, SRS_SECRET, oasg.fixed, oasg.copies)
    assert vk.transcript_repr == pk.vk.transcript_repr
    wit = lambda x: types.SimpleNamespace(advice=circuits.StandardPlonk(x).synthesize().advice, instance=[])
    gates = phase_cases.without_challenges(ocs.gates)
    proof = custom.prove_many(keys, [wit(3), wit(0x55AA)], params=params)
    assert cases.verify(vk, proof, [[], []], gates, [])
    assert not cases.verify(vk, proof, [[]], gates, []) and not cases.verify(vk, proof[:-1] + bytes([proof[-1] ^ 1]), [[], []], gates, [])
    assert custom.prove_many(keys, [wit(3)], seeds=[9], params=params) == prover.create_proof(params, pk, circuits.StandardPlonk(3), 9)
    pk.release()
    params.release()


def test_members_are_independent(gpu):
    """member 0's advice commitments inside a batch are those of the same witness and seed proved alone, whatever member 1 holds"""
    from halo2_scaffold_amd import custom

    cs, asgs = _is_zero(custom, [5, 0, 9])
    _, params, keys, vk = _keys(gpu, cs, asgs[0], 4)
    ws = custom.BatchWorkspace(params, keys, 2)
    alone = custom.create_proof(params, keys, asgs[0], 21)
    a = custom.prove_many(keys, asgs[:2], seeds=[21, 40], ws=ws)
    b = custom.prove_many(keys, [asgs[0], asgs[2]], seeds=[21, 40], ws=ws)
    head = 32 * cs.n_advice
    assert a[:head] == alone[:head] == b[:head] and a[head : 2 * head] != b[head : 2 * head]
    assert cases.verify_circuits(vk, cs, a, [[], []]) and cases.verify_circuits(vk, cs, b, [[], []])
    _release(params, keys, ws)


def test_witness_check_names_the_member(gpu):
    """an unsatisfied witness in circuit 1 only: h2mi_prover_check on member 1 names the row, on member 0 it reports nothing, and the
    finished proof is rejected"""
    from halo2_scaffold_amd import custom, engine

    cs, good = gate_cases.is_zero_circuit(custom, 7)
    _, broken = gate_cases.is_zero_circuit(custom, 7, flip_out=True)
    _, params, keys, vk = _keys(gpu, cs, good, 4)
    ws = custom.BatchWorkspace(params, keys, 2)
    lib = gpu.lib
    pts = np.zeros((8, 8), dtype=np.uint64)
    for p, asg, seed in zip(ws.provers, (good, broken), (1, 9)):
        cells, keep = engine.pack_cells(asg.advice)
        assert lib.h2mi_prover_advice(p.handle, cells, None, 0, seed, pts.ctypes.data) == 0
        del keep
    assert ws.provers[0].check(5) == []
    found = ws.provers[1].check(5)
    assert [(f.kind, f.row) for f in found] == [(engine.CHECK_GATE, 0)] * len(found) and found
    proof = custom.prove_many(keys, [good, broken], ws=ws)
    assert not cases.verify_circuits(vk, cs, proof, [[], []])
    assert cases.verify_circuits(vk, cs, custom.prove_many(keys, [good, good], ws=ws), [[], []])
    _release(params, keys, ws)


# ---- 3. order and argument errors ------------------------------------------------------------------------------------------------------
def _to_products(lib, engine, F, provers, asgs, seeds, betas):
    """advice and products on each member (is_zero: no lookups), without a transcript: beta per member, gamma = 3"""
    pts = np.zeros((8, 8), dtype=np.uint64)
    gamma = np.ascontiguousarray(F.fr_to_mont_limbs(3))
    for p, asg, seed, beta in zip(provers, asgs, seeds, betas):
        cells, keep = engine.pack_cells(asg.advice)
        assert lib.h2mi_prover_advice(p.handle, cells, None, 0, seed, pts.ctypes.data) == 0
        del keep
        if beta is not None:
            b = np.ascontiguousarray(F.fr_to_mont_limbs(beta))
            assert lib.h2mi_prover_products(p.handle, b.ctypes.data, gamma.ctypes.data, pts.ctypes.data) == 0


def test_batch_order_and_argument_errors(gpu):
    from halo2_scaffold_amd import custom, engine
    from halo2_scaffold_amd import field as F

    lib = gpu.lib
    cs, asgs = _is_zero(custom, [5, 0])
    _, params, keys, vk = _keys(gpu, cs, asgs[0], 4)
    other_keys = custom.Keys(params, cs, asgs[0])
    provers = [engine.Prover(keys.keys, params) for _ in range(3)]
    stranger = engine.Prover(other_keys.keys, params)
    solo = types.SimpleNamespace(prover=provers[1])
    before = custom.create_proof(params, keys, asgs[1], 33, ws=solo)

    def create(members, n=None):
        arr = (C.c_void_p * max(len(members), 1))(*[p.handle for p in members])
        h = C.c_void_p(0xDEAD)
        rc = lib.h2mi_batch_create(arr, len(members) if n is None else n, C.byref(h))
        return rc, h.value

    assert create([provers[0], stranger]) == (EINVAL, None)            # members of two different keys
    assert create([provers[0]], 0) == (EINVAL, None) and create([provers[0]] * 9) == (EINVAL, None)
    assert create([provers[2], provers[2]]) == (EINVAL, None)          # one member twice
    assert lib.h2mi_batch_create(None, 1, None) == EINVAL
    batch = engine.Batch(provers[:2])
    assert create([provers[1], provers[2]]) == (EINVAL, None)          # a member bound already
    assert lib.h2mi_prover_destroy(provers[1].handle) == EINVAL        # ... cannot be destroyed
    products = provers[2].counts.products
    assert [p.counts.products for p in provers] == [products, products - 1, products]  # one random polynomial per proof: member 0's
    pts = np.zeros((8, 8), dtype=np.uint64)
    y = np.ascontiguousarray(F.fr_to_mont_limbs(0x1234))
    quotient = lambda: lib.h2mi_batch_quotient(batch.handle, y.ctypes.data, pts.ctypes.data)
    assert quotient() == EINVAL                                         # nothing in flight
    _to_products(lib, engine, F, provers[:2], asgs, (11, 19), (7, None))
    assert quotient() == EINVAL                                         # member 1 has not run its products
    _to_products(lib, engine, F, provers[:2], asgs, (11, 12), (7, 7))
    assert quotient() == EINVAL                                         # seeds 11 and 12: blinding streams that overlap
    _to_products(lib, engine, F, provers[:2], asgs, (11, 19), (7, 8))
    assert quotient() == EINVAL                                         # differing beta
    _to_products(lib, engine, F, provers[:2], asgs, (11, 19), (7, 7))
    for p in provers[:2]:                                               # a bound member's own joint phases: refused, nothing abandoned
        assert lib.h2mi_prover_quotient(p.handle, y.ctypes.data, pts.ctypes.data) == EINVAL
        assert lib.h2mi_prover_evaluations(p.handle, y.ctypes.data, pts.ctypes.data) == EINVAL
    assert lib.h2mi_batch_evaluations(batch.handle, y.ctypes.data, batch._evals.ctypes.data) == EINVAL  # before the quotient: abandons the proof
    assert quotient() == EINVAL
    _to_products(lib, engine, F, provers[:2], asgs, (11, 19), (7, 7))
    assert quotient() == 0 and pts[: cs.degree() - 1].any(axis=1).all()
    assert quotient() == EINVAL                                         # once per proof
    # a whole batch proof with the members' own quotient tried in the middle still verifies
    tried = []

    def products_done(b):
        tried.extend(lib.h2mi_prover_quotient(p.handle, y.ctypes.data, pts.ctypes.data) for p in b.members)

    ws = types.SimpleNamespace(batch=batch, release=lambda: None)
    proof = custom.prove_many(keys, asgs, ws=ws, hooks={"products_done": products_done})
    assert tried == [EINVAL, EINVAL] and cases.verify_circuits(vk, cs, proof, [[], []])
    batch.release()
    assert lib.h2mi_batch_destroy(C.c_void_p(0xDEAD0)) == EHANDLE
    assert [p.counts.products for p in provers] == [products] * 3
    assert custom.create_proof(params, keys, asgs[1], 33, ws=solo) == before  # a former member proves alone, the bytes it gave before
    for p in provers + [stranger]:
        p.release()
    other_keys.release()
    _release(params, keys)
