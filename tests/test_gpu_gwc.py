"""ProverGWC on the device (tests/gwc_cases.py): the grouped "linear combination + division" of
h2mi_fr_gwc_witness_dev bit for bit against Python integers at the shapes where it can go wrong, and which kernels ran from the launch
profile; proofs of every kind of constraint system through the Python hosts with multiopen="gwc", accepted by the GWC verifier and
rejected after one-byte flips; the shape of the result against the SHPLONK proof of the same key and seed; H2MI_BUF_GWC_W against the
Python-integer prover tail over the prover's own coefficient buffers; the state machine of the two endings."""
import ctypes as C
import random

import numpy as np
import pytest

import custom_gate_cases as gate_cases
import gwc_cases as G
import limit_cases
import logup_cases
import lookup_expr_cases
import phase_cases
import shuffle_cases
from oracle import bn254 as o
from oracle import flex as FX

pytestmark = pytest.mark.gpu

R = o.R
SRS_SECRET = 0x5EC2E7 + 0x48324D49
EINVAL = -1
CAP = 72    # GWC_TERMS (csrc/h2mi_poly.hip): the terms of one launch, and of one point
POINTS = 4  # KATE_MULTI_MAX: the points of one launch
LINCOMB = 24  # LINCOMB_MAX: the operands of one k_lincomb launch


def _vals(buf, count):
    return o.unpack(buf.to_numpy(shape=(count, 4), nbytes=count * 32), R)


def _flipped(proof: bytes, at: int) -> bytes:
    out = bytearray(proof)
    out[at] ^= 1
    return bytes(out)


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------------
def _limbs(values):
    from halo2_scaffold_amd import field as F

    return np.ascontiguousarray(np.stack([F.fr_to_mont_limbs(v % R) for v in values]))


def _call(lib, ptrs, scalars, counts, roots, n, outs, roots_inv=None):
    arr = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
    out = (C.c_void_p * max(len(outs), 1))(*outs)
    cnt = (C.c_size_t * max(len(counts), 1))(*counts)
    sc, z = _limbs(scalars or [0]), _limbs(roots)
    zi = _limbs([pow(r, -1, R) if r % R else 0 for r in roots] if roots_inv is None else roots_inv)
    return lib.h2mi_fr_gwc_witness_dev(arr, sc.ctypes.data, cnt, z.ctypes.data, zi.ctypes.data, len(counts), n, out, None)


def _launches(lib, call):
    """launches per kernel name during call(), from the library's launch profile"""
    assert lib.h2mi_profile_reset() == 0 and lib.h2mi_profile_filter(b"") == 0 and lib.h2mi_profile_enable(1) == 0
    try:
        rc = call()
    finally:
        assert lib.h2mi_profile_enable(0) == 0
    ms, count, found = C.c_double(), C.c_uint64(), {}
    for name in ("k_gwc_local", "k_kate_offsets", "k_gwc_finish", "k_lincomb", "k_kate_local", "k_kate_finish"):
        assert lib.h2mi_profile_query(name.encode(), C.byref(ms), C.byref(count)) == 0
        found[name] = count.value
    assert lib.h2mi_profile_reset() == 0
    return rc, found


def _slices(terms):
    """the launch slices gwc_witness forms: up to POINTS points and CAP terms, a point over CAP entering as ONE term"""
    slices, points, used = 0, 0, 0
    for t in terms:
        t = 1 if t > CAP else t
        if points == 0 or points == POINTS or used + t > CAP:
            slices, points, used = slices + 1, 0, 0
        points, used = points + 1, used + t
    return slices


def _presum_launches(terms):
    """k_lincomb launches: LINCOMB operands first, then LINCOMB - 1 beside the running sum"""
    return sum(1 + -(-(t - LINCOMB) // (LINCOMB - 1)) for t in terms if t > CAP)


# (n, terms per group, roots ("r" random, 1, R - 1), groups that share pool polynomial 0, every value R - 1)
KERNEL_CASES = {
    "n2_one_term": (2, [1], ["r"], [], False),
    "n3_four_groups_every_residue": (3, [1, 2, 3, 4], ["r", 1, R - 1, "r"], [], False),
    "n1023_five_groups_shared_poly": (1023, [3, 1, 4, 2, 2], ["r", "r", "r", 1, "r"], [0, 2, 4], False),
    "n1024_at_the_cap": (1024, [CAP], ["r"], [], False),
    "n1025_nine_groups": (1025, [1, 2, 3, 4, 5, 6, 7, 8, 9], ["r", 1, "r", R - 1, "r", "r", "r", "r", "r"], [1, 4, 8], False),
    "n2049_cap_plus_one": (2049, [CAP + 1, 2, 1, 3], ["r", "r", R - 1, "r"], [], False),
    "n5000_five_groups": (5000, [4, 3, 2, 1, 5], ["r", "r", 1, "r", R - 1], [0, 1, 3], False),
    "n1025_twice_the_cap_plus_one": (1025, [2 * CAP + 1], ["r"], [], False),
    "n2049_slices_cut_by_terms": (2049, [CAP, 1, CAP, 3], ["r", "r", "r", "r"], [], False),
    "n1025_limb_extreme_at_the_cap": (1025, [CAP], [R - 1], [], True),
    "n1024_limb_extreme_four_groups": (1024, [3, CAP - 3, 2, 1], [R - 1, "r", 1, R - 1], [], True),
}


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_witness_kernel_against_python_integers(gpu, name):
    from halo2_scaffold_amd.device import DevBuf

    n, terms, roots, shared, extreme = KERNEL_CASES[name]
    rng = random.Random(len(name) + 7 * n)
    roots = [rng.randrange(1, R) if r == "r" else r for r in roots]
    n_pool = min(max(terms), 12)  # the pool of distinct polynomials; a group's terms cycle through it from its own offset
    pool = [[R - 1] * n if extreme else [rng.randrange(R) for _ in range(n)] for _ in range(n_pool)]
    index = [[(0 if j == 0 and g in shared else (3 * g + j) % n_pool) for j in range(t)] for g, t in enumerate(terms)]
    scalars = [[R - 1 if extreme else rng.randrange(R) for _ in range(t)] for t in terms]
    d_pool = [DevBuf.from_numpy(o.pack(p, R)) for p in pool]
    sentinel = o.pack([0xDEAD] * n, R)
    d_outs = [DevBuf.from_numpy(sentinel) for _ in terms]
    before = [b.to_numpy(shape=(n, 4), nbytes=n * 32).tobytes() for b in d_pool]
    ptrs = [d_pool[i].ptr for grp in index for i in grp]
    rc, ran = _launches(gpu.lib, lambda: _call(gpu.lib, ptrs, [s for grp in scalars for s in grp], terms, roots, n, [b.ptr for b in d_outs]))
    assert rc == 0
    for g, t in enumerate(terms):
        acc = [0] * n
        for j in range(t):
            c, poly = scalars[g][j], pool[index[g][j]]
            for i in range(n):
                acc[i] += c * poly[i]
        want = o.kate_division([a % R for a in acc], roots[g]) + [0]  # n - 1 coefficients, and coefficient n - 1 written as zero
        assert _vals(d_outs[g], n) == want, g
    assert [b.to_numpy(shape=(n, 4), nbytes=n * 32).tobytes() for b in d_pool] == before  # the inputs are unchanged
    # which route ran: the fused pass 1 once per slice, k_lincomb in the over-cap case alone, today's division kernels never
    slices = _slices(terms)
    assert ran == {"k_gwc_local": slices, "k_kate_offsets": slices, "k_gwc_finish": slices, "k_lincomb": _presum_launches(terms), "k_kate_local": 0,
                   "k_kate_finish": 0}, ran
    assert (ran["k_lincomb"] > 0) == (max(terms) > CAP)
    for b in d_pool + d_outs:
        b.free()


def test_the_cases_cover_every_value_the_kernel_branches_on():
    cases = list(KERNEL_CASES.values())
    assert {c[0] for c in cases} == {2, 3, 1023, 1024, 1025, 2049, 5000}
    assert {len(c[1]) for c in cases} >= {1, 4, 5, 9}
    assert {t for c in cases for t in c[1]} >= {1, 2, 3, 4, CAP, CAP + 1, 2 * CAP + 1}
    assert {r for c in cases for r in c[2]} >= {"r", 1, R - 1}
    assert any(len(c[3]) == 3 for c in cases) and any(c[4] and CAP in c[1] for c in cases)
    assert {_slices(c[1]) for c in cases} >= {1, 2, 3, 4} and _presum_launches([CAP + 1]) == 4 and _presum_launches([2 * CAP + 1]) == 7


def test_witness_refusals(gpu):
    from halo2_scaffold_amd.device import DevBuf

    n = 8
    d_p, d_o = DevBuf.from_numpy(o.pack([1] * n, R)), DevBuf.from_numpy(o.pack([2] * n, R))
    lib = gpu.lib
    assert _call(lib, [d_p.ptr], [1], [1], [5], 1, [d_o.ptr]) == EINVAL  # n = 1
    assert _call(lib, [d_p.ptr], [1], [1, 0], [5, 6], n, [d_o.ptr, d_o.ptr]) == EINVAL  # an empty group
    assert _call(lib, [d_p.ptr], [1], [1], [0], n, [d_o.ptr]) == EINVAL  # a zero root
    assert _call(lib, [d_p.ptr], [1], [1], [5], n, [d_o.ptr], roots_inv=[0]) == EINVAL
    assert _call(lib, [None], [1], [1], [5], n, [d_o.ptr]) == EINVAL and _call(lib, [d_p.ptr], [1], [1], [5], n, [None]) == EINVAL
    assert _call(lib, [], [], [], [5], n, []) == EINVAL  # no group
    assert _vals(d_o, n) == [2] * n  # nothing was written
    assert _call(lib, [d_p.ptr], [1], [1], [5], n, [d_o.ptr]) == 0  # and the entry serves the next call
    assert _vals(d_o, n) == o.kate_division([1] * n, 5) + [0]
    d_p.free()
    d_o.free()


# ---- 2. proofs ----------------------------------------------------------------------------------------------------------------------------
def _standard_plonk(custom):
    """the reference's StandardPlonk (custom_gate_cases.standard_plonk_cs) with the witness of circuits.StandardPlonk"""
    from halo2_scaffold_amd import circuits

    cs = gate_cases.standard_plonk_cs(custom)
    syn = circuits.StandardPlonk(0xC0FFEE).synthesize()
    asg = custom.Assignment(cs)
    asg.advice, asg.fixed = [dict(c) for c in syn.advice], [dict(c) for c in syn.fixed]
    asg.copies = [((custom.ADVICE, a[0], a[1]), (custom.ADVICE, b[0], b[1])) for a, b in syn.copies]
    return cs, asg


def _rotations(custom):
    """limit_cases.rotation_circuit with one column at rotations -2 .. +2, its window column in the permutation argument beside b:
    two columns at chunks of one are two sets, so the first set is opened at x_last — six opening points at least"""
    cs, asg, _ = limit_cases.rotation_circuit(custom, 6, [(-2, 5)])
    cs.enable_equality(custom.Column(custom.ADVICE, 0))
    assert len(cs.perm_columns) > cs.degree() - 2 and {r for _, r in cs.advice_queries} >= {-2, -1, 0, 1, 2}
    return cs, asg


# name -> (k, logUp key, builder(custom) -> (cs, assignment or synthesize))
PROOF_CASES = {
    "standard_plonk": (5, False, _standard_plonk),
    "is_zero": (5, False, lambda custom: gate_cases.is_zero_circuit(custom, 5)),
    "or": (5, False, lambda custom: gate_cases.or_circuit(custom, 1, 0)),
    "degree6_public_inputs": (5, False, lambda custom: gate_cases.degree6_circuit(custom, 3, 11)),
    "xor_permuted": (5, False, lookup_expr_cases.xor_circuit),
    "xor_logup": (5, True, lookup_expr_cases.xor_circuit),
    "mixed_with_shuffles": (6, False, shuffle_cases.mixed_circuit),
    "two_phases": (5, False, phase_cases.rlc_circuit),
    "rotations_and_x_last": (6, False, _rotations),
    "xor4_two_tiles": (11, False, lambda custom: lookup_expr_cases.xor4_circuit(custom, 11)),
}


def _keys(gpu, cs, first, k, name, logup):
    from halo2_scaffold_amd import custom

    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    keys = custom.Keys(params, cs, first, logup=logup)
    ocs = gate_cases.oracle_cs(cs, name)
    oasg = gate_cases.oracle_assignment(ocs, first)
    vk = FX.VerifierKeys(ocs, k, SRS_SECRET, oasg.fixed, oasg.copies)
    assert o.unpack_points(keys.fixed_commitments) == vk.fixed_commitments and keys.transcript_repr == vk.transcript_repr
    return params, keys, vk


def _release(params, keys, *ws):
    for w in ws:
        w.release()
    keys.release()
    params.release()


def _check_shape_and_tampering(cs, vk, logup, instances, gwc, shplonk, n_points, n_evaluations):
    """-> the verifier's tail.  The GWC proof is accepted; its length and its bytes before the tail are the SHPLONK proof's; a flipped
    byte in the first [W], in the last [W] and in an evaluation is rejected"""
    tail = {}
    assert G.verify_circuits(vk, cs, gwc, instances, logup=logup, tail_out=tail)
    P = len(G.gwc_groups(tail["queries"]))
    assert n_points == P == len(tail["Ws"]) and P == len({r % vk.n for r in _query_rotations(cs, logup)})
    assert len(gwc) == len(shplonk) - 64 + 32 * P and gwc[:-32 * P] == shplonk[:-64]
    assert not G.verify_circuits(vk, cs, shplonk, instances, logup=logup)  # the other ending is another proof
    w_at = len(gwc) - 32 * P
    ev_at = w_at - 32 * n_evaluations
    for at in (w_at + 3, len(gwc) - 32 + 5, ev_at + 1, w_at - 32 + 2):  # the first [W], the last [W], the first and the last evaluation
        assert not G.verify_circuits(vk, cs, _flipped(gwc, at), instances, logup=logup), at
    return tail


def _query_rotations(cs, logup):
    """the rotations of the key's query list (limit_cases.opening_sets, flattened)"""
    return {r for s in limit_cases.opening_sets(cs, logup) for r in s}


@pytest.mark.parametrize("name", list(PROOF_CASES))
def test_gwc_proofs_are_accepted_and_tampering_is_rejected(gpu, name):
    """every kind of constraint system the library proves, ended with ProverGWC; and the SHPLONK proof of the same key and seed is the
    same before and after a GWC proof on the same prover: no state leaks between the endings"""
    from halo2_scaffold_amd import custom

    k, logup, build = PROOF_CASES[name]
    cs, asg = build(custom)[:2]
    first = shuffle_cases.first_assignment(cs, asg)
    params, keys, vk = _keys(gpu, cs, first, k, name, logup)
    ws = custom.Workspace(params, keys)
    seed = 40 + len(name)
    shplonk = custom.create_proof(params, keys, asg, seed, ws=ws)
    gwc = custom.create_proof(params, keys, asg, seed, ws=ws, multiopen="gwc")
    assert custom.create_proof(params, keys, asg, seed, ws=ws) == shplonk
    assert custom.create_proof(params, keys, asg, seed, ws=ws, multiopen="gwc") == gwc
    P = ws.prover.gwc_num_points()
    _check_shape_and_tampering(cs, vk, logup, [first.instance], gwc, shplonk, P, ws.prover.counts.evaluations)
    if name == "rotations_and_x_last":
        assert P >= 6  # two launch slices, and the x_last point
    if name == "xor4_two_tiles":
        assert vk.n == 2 * 1024
    _release(params, keys, ws)


def test_prove_many_of_two_mixed_circuits(gpu):
    from halo2_scaffold_amd import custom

    built = [shuffle_cases.mixed_circuit(custom, variant=v) for v in (0, 1)]
    cs, asgs = built[0][0], [a for _, a in built]
    params, keys, vk = _keys(gpu, cs, asgs[0], 6, "mixed", False)
    ws = custom.BatchWorkspace(params, keys, 2)
    instances = [a.instance for a in asgs]
    shplonk = custom.prove_many(keys, asgs, seeds=[5, 13], ws=ws)
    gwc = custom.prove_many(keys, asgs, seeds=[5, 13], ws=ws, multiopen="gwc")
    assert custom.prove_many(keys, asgs, seeds=[5, 13], ws=ws) == shplonk
    P = ws.batch.gwc_num_points()
    assert P == ws.provers[0].gwc_num_points() == ws.provers[1].gwc_num_points()
    _check_shape_and_tampering(cs, vk, False, instances, gwc, shplonk, P, ws.batch.n_evaluations)
    # a batch of one is the single prover's proof with this ending too
    one = custom.prove_many(keys, asgs[:1], seeds=[5], multiopen="gwc")
    assert one == custom.create_proof(params, keys, asgs[0], 5, multiopen="gwc")
    _release(params, keys, ws)


# ---- 3. the W_i ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["standard_plonk", "rotations_and_x_last"])
def test_w_buffers_against_the_python_prover_tail(gpu, name):
    """H2MI_BUF_GWC_W against gwc_witnesses over the prover's own coefficient buffers — in these two circuits every opened polynomial
    is readable through h2mi_prover_buffer — and every [W_i] of the proof against the commitment of the buffer's content"""
    from halo2_scaffold_amd import custom, engine

    k, logup, build = PROOF_CASES[name]
    cs, asg = build(custom)
    params, keys, vk = _keys(gpu, cs, asg, k, name, logup)
    ws = custom.Workspace(params, keys)
    n, p = 1 << k, ws.prover
    gwc = custom.create_proof(params, keys, asg, 19, ws=ws, multiopen="gwc")
    tail = {}
    assert G.verify_circuits(vk, cs, gwc, [asg.instance], logup=logup, tail_out=tail)
    m = len(cs.perm_columns)
    n_sets = -(-m // (cs.degree() - 2))
    polys = {("h",): _vals(p.view(engine.BUF_H_POLY), n), ("random",): _vals(p.view(engine.BUF_RANDOM_POLY), n)}
    for c, view in enumerate(p.views(engine.BUF_ADVICE_POLY, cs.n_advice)):
        polys[("advice", 0, c)] = _vals(view, n)
    for s, view in enumerate(p.views(engine.BUF_PERM_Z_POLY, n_sets)):
        polys[("z", 0, s)] = _vals(view, n)
    for c, view in enumerate(keys.fixed_polys):
        polys[("fixed", c)] = _vals(view, n)
    for j, view in enumerate(keys.sigma_polys):
        polys[("sigma", j)] = _vals(view, n)
    assert {key for key, _, _ in tail["queries"]} == set(polys)
    want = G.gwc_witnesses(polys, tail["queries"], tail["v"])
    P = p.gwc_num_points()
    assert len(want) == P
    for i, view in enumerate(p.views(engine.BUF_GWC_W, P)):
        got = _vals(view, n)
        assert got == want[i] + [0], i
        assert o.g1_mul(o.eval_polynomial(got, SRS_SECRET), o.G1_GEN) == tail["Ws"][i], i  # [W_i] = W_i(s) G
    ptr, cnt = C.c_void_p(), C.c_size_t()
    assert gpu.lib.h2mi_prover_buffer(p.handle, engine.BUF_GWC_W, P, C.byref(ptr), C.byref(cnt)) != 0  # there is no W_P
    _release(params, keys, ws)


# ---- 4. the state machine -------------------------------------------------------------------------------------------------------------------
class _Stop(Exception):
    pass


def test_the_two_endings_are_alternatives(gpu, monkeypatch):
    """after gwc_open a shplonk call is H2MI_EINVAL as after any completed proof; after shplonk_quotient a gwc_open is H2MI_EINVAL and
    abandons the proof; a fresh proof succeeds right after each refusal"""
    from halo2_scaffold_amd import custom
    from halo2_scaffold_amd import field as F

    lib = gpu.lib
    cs, asg = _standard_plonk(custom)
    params, keys, vk = _keys(gpu, cs, asg, 5, "standard_plonk", False)
    ws = custom.Workspace(params, keys)
    h, P = ws.prover.handle, ws.prover.gwc_num_points()
    ch, one = F.fr_to_mont_limbs(12345), np.zeros(8, dtype=np.uint64)
    many = np.zeros((P, 8), dtype=np.uint64)
    shplonk = custom.create_proof(params, keys, asg, 3, ws=ws)
    gwc = custom.create_proof(params, keys, asg, 3, ws=ws, multiopen="gwc")
    # behind a completed GWC proof
    assert lib.h2mi_prover_shplonk_quotient(h, ch.ctypes.data, ch.ctypes.data, one.ctypes.data) == EINVAL
    assert lib.h2mi_prover_shplonk_open(h, ch.ctypes.data, one.ctypes.data) == EINVAL
    assert lib.h2mi_prover_gwc_open(h, ch.ctypes.data, many.ctypes.data) == EINVAL
    assert custom.create_proof(params, keys, asg, 3, ws=ws) == shplonk
    # behind shplonk_quotient: the proof stops in front of shplonk_open
    real_open = lib.h2mi_prover_shplonk_open

    def stop(*args):
        raise _Stop()

    monkeypatch.setattr(lib, "h2mi_prover_shplonk_open", stop)
    with pytest.raises(_Stop):
        custom.create_proof(params, keys, asg, 3, ws=ws)
    monkeypatch.setattr(lib, "h2mi_prover_shplonk_open", real_open)
    assert lib.h2mi_prover_gwc_open(h, ch.ctypes.data, many.ctypes.data) == EINVAL
    assert real_open(h, ch.ctypes.data, one.ctypes.data) == EINVAL  # the refusal abandoned the proof
    assert custom.create_proof(params, keys, asg, 3, ws=ws, multiopen="gwc") == gwc
    # gwc_open needs the evaluations, as shplonk_quotient does, and its arguments
    assert lib.h2mi_prover_gwc_open(h, None, many.ctypes.data) == EINVAL
    assert custom.create_proof(params, keys, asg, 3, ws=ws) == shplonk
    n = C.c_size_t()
    assert lib.h2mi_prover_gwc_num_points(h, None) == EINVAL and lib.h2mi_prover_gwc_num_points(h, C.byref(n)) == 0 and n.value == P
    _release(params, keys, ws)


def test_a_bound_members_gwc_open_is_refused_and_abandons_nothing(gpu):
    from halo2_scaffold_amd import custom
    from halo2_scaffold_amd import field as F

    lib = gpu.lib
    built = [gate_cases.is_zero_circuit(custom, x) for x in (5, 0)]
    cs, asgs = built[0][0], [a for _, a in built]
    params, keys, vk = _keys(gpu, cs, asgs[0], 5, "is_zero", False)
    ws = custom.BatchWorkspace(params, keys, 2)
    want = custom.prove_many(keys, asgs, seeds=[5, 13], ws=ws, multiopen="gwc")
    ch = F.fr_to_mont_limbs(99)
    many = np.zeros((ws.batch.gwc_num_points(), 8), dtype=np.uint64)
    refused = []

    def mid_proof(batch):  # every member has run its products: the members' own joint calls are refused, the proof goes on
        refused.extend(lib.h2mi_prover_gwc_open(p.handle, ch.ctypes.data, many.ctypes.data) for p in batch.members)

    got = custom.prove_many(keys, asgs, seeds=[5, 13], ws=ws, multiopen="gwc", hooks={"products_done": mid_proof})
    assert refused == [EINVAL, EINVAL] and got == want
    assert G.verify_circuits(vk, cs, got, [a.instance for a in asgs], logup=False)
    _release(params, keys, ws)
