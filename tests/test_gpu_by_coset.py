"""The coset-by-coset quotient on the device (H2MI_KEYGEN_BY_COSET, include/h2mi_prover.h).

1. k_evaluate_h_expr_slice through h2mi_plonk_evaluate_h_expr_batch_dev with a slice: h assembled from rot launches over slices made by the transform
   export, word for word against the Python-integer quotient of tests/instance_cases.py on every extended-coset point and against the
   resident batch kernel on the same polynomials; a launch for slice c writes elements c + rot i and no other.
2. A by-coset key and a resident key of the same circuit give the same proof bytes — every shape, argument and ending the prover takes
   — and a by-coset key reproduces the committed golden proofs, a comparison that does not pass through the resident quotient.
3. The committed seeds of tests/random_circuit_cases.py: the same bytes, accepted by that module's verifier.
4. The route (rot launches of the slice kernel, no other quotient kernel), the verifying key, the buffer queries, the device-byte counter
   against the formula of tests/by_coset_cases.py, the witness check."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import assigned_cases
import by_coset_cases as cases
import custom_gate_cases as gate_cases
import instance_cases
import logup_cases
import logup_sets_cases
import lookup_expr_cases as lookup_cases
import phase_cases
import random_circuit_cases
import shuffle_cases
from oracle import bn254 as o
from oracle import flex as FX
from oracle import plonk as P

pytestmark = pytest.mark.gpu

R = o.R
SRS_SECRET = 0x5EC2E7 + 0x48324D49
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOGUP = 0x80000000  # include/h2mi.h H2MI_LOOKUPS_LOGUP
PATTERN = 0xA5A5A5A5A5A5A5A5  # what h holds before the launches: no canonical field element has this top limb


def _vals(buf, count):
    return o.unpack(buf.to_numpy(shape=(count, 4), nbytes=count * 32), R)


class _At:
    """`count` elements of a DevBuf from element `start` on, as the wrappers read a vector (its address)"""

    def __init__(self, buf, start: int):
        self.ptr = buf.ptr + 32 * start


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------------
def _entries(plonk, shared, circuits, logup, sets):
    """the argument structs of one launch over device vectors laid out as by_coset_cases.map_vectors returns them"""
    # a logUp lookup has no permuted table: the array builder is given the slot's neighbour, and the slot is cleared below
    lks = lambda c: [lk if lk[4] is not None else lk[:4] + (lk[3],) + lk[5:] for lk in c["lookups"]]
    view = [{"advice": c["advice"], "fixed": c["fixed"], "instance": None, "perm_values": c["perm_values"], "perm_zs": c["perm_zs"],
             "lookups": lks(c), "shuffles": c["shuffles"], "instances": c["instance"]} for c in circuits]
    arr = plonk.expr_cosets_array(view, shared["perm_sigmas"], shared["chunk"], shared["l0"], shared["l_last"], shared["l_active"])
    if logup:
        for e in arr:
            e.n_lookups |= LOGUP
            e.lookup_permuted_table[0] = None
    shs, lg, ins = plonk.argument_cosets(view, [sets] if logup else None)
    return arr, shs, lg, ins


@pytest.mark.parametrize("case", range(len(cases.KERNEL_CASES)))
def test_slice_kernel_against_python_integers_and_the_resident_kernel(gpu, case):
    from halo2_scaffold_amd import custom, engine, plonk
    from halo2_scaffold_amd.device import DevBuf

    kc = cases.kernel_case(custom, case)
    k, N, logup, K = kc["k"], len(kc["circuits"]), kc["logup"], kc["sets"]
    dom, od = gpu.EvaluationDomain(kc["degree"], k), o.Domain(k, kc["degree"])
    n, size = 1 << k, 1 << dom.extended_k
    rot = size >> k
    assert dom.extended_k == od.extended_k and rot == 1 << ((kc["degree"] - 2).bit_length())
    constants, ops = {}, []
    for t in kc["trees"]:
        ops += t.program(constants)[0]
    consts = sorted(constants, key=constants.get)
    prog = engine.GateProgram.build(ops, consts)
    assert {r for op, _, r in ops if op in (engine.EXPR_ADVICE, engine.EXPR_FIXED, engine.EXPR_INSTANCE)} >= {-1, 1, 3}
    beta, gamma, y, ch, bf = kc["beta"], kc["gamma"], kc["y"], kc["challenges"], kc["bf"]

    # every vector: its coefficients on the device, its extended-coset form (resident kernel), one slice buffer (refilled per slice)
    coeffs = {}

    def up(v):
        coeffs[id(v)] = d = DevBuf.from_numpy(o.pack(v, R))
        return d

    sh_c, cc_c = cases.map_vectors(kc, up)
    groups = []  # a logUp lookup's input sets lie behind one another: (coefficient buffers, extended buffer, slice buffer)

    def forms(shared, circuits, length, fill):
        made = {}

        def one(d):
            if id(d) not in made:
                made[id(d)] = DevBuf(length * 32)
                fill(d, made[id(d)])
            return made[id(d)]

        out_sh = {"perm_sigmas": [one(d) for d in shared["perm_sigmas"]], "chunk": shared["chunk"], "l0": one(shared["l0"]), "l_last": one(shared["l_last"]),
                  "l_active": one(shared["l_active"])}
        out_cc = []
        for c in circuits:
            lks = []
            for lk in c["lookups"]:
                if isinstance(lk[0], list):  # K sets in one buffer of K * length elements
                    joined = DevBuf(len(lk[0]) * length * 32)
                    for j, d in enumerate(lk[0]):
                        fill(d, _At(joined, j * length))
                    groups.append(joined)
                    lks.append((joined,) + tuple(one(d) if d is not None else None for d in lk[1:]))
                else:
                    lks.append(tuple(one(d) if d is not None else None for d in lk))
            out_cc.append({"advice": [one(d) for d in c["advice"]], "fixed": [one(d) for d in c["fixed"]], "instance": [one(d) for d in c["instance"]],
                           "perm_values": [one(d) for d in c["perm_values"]], "perm_zs": [one(d) for d in c["perm_zs"]], "lookups": lks,
                           "shuffles": [tuple(one(d) for d in sf) for sf in c["shuffles"]]})
        return out_sh, out_cc

    # the resident kernel on the whole extended coset
    sh_e, cc_e = forms(sh_c, cc_c, size, lambda d, out: dom.coeff_to_extended_oop_dev(d, out))
    resident = DevBuf(size * 32)
    arr, shs, lg, ins = _entries(plonk, sh_e, cc_e, logup, K)
    plonk.evaluate_h_expr_slice(dom, prog, arr, N, None, beta, gamma, y, resident, blinding_factors=bf, challenges=ch, shuffles=shs, logup=lg, instances=ins)

    # the reference in Python integers, from the oracle's own extended-coset forms
    sh_i, cc_i = cases.map_vectors(kc, od.coeff_to_extended)
    want = instance_cases.batched_quotient(k, od.extended_k, od.g_coset, od.extended_omega, P.FR_DELTA, bf, ops, consts, ch, cc_i, sh_i, beta, gamma, y,
                                           logup=logup)
    assert _vals(resident, size) == want

    # rot launches, one per slice; h starts as a pattern no launch may touch outside its own coset
    h = DevBuf.from_numpy(np.full((size, 4), PATTERN, dtype=np.uint64))
    pattern = [PATTERN] * 4
    for c in range(rot):
        sh_s, cc_s = forms(sh_c, cc_c, n, lambda d, out, c=c: dom.coeff_to_slice_oop_dev(d, c, out))
        arr, shs, lg, ins = _entries(plonk, sh_s, cc_s, logup, K)
        plonk.evaluate_h_expr_slice(dom, prog, arr, N, c, beta, gamma, y, h, blinding_factors=bf, challenges=ch, shuffles=shs, logup=lg, instances=ins)
        words = h.to_numpy(shape=(size, 4), nbytes=size * 32)
        for idx in range(size):
            if idx % rot > c:
                assert list(words[idx]) == pattern, f"slice {c} wrote element {idx}"
        got = o.unpack(words[[idx for idx in range(size) if idx % rot <= c]], R)
        assert got == [want[idx] for idx in range(size) if idx % rot <= c], f"slice {c}"
    assert (h.to_numpy() == resident.to_numpy()).all()


def test_slice_kernel_cases_cover_what_they_should():
    ks, rots, ns, sets = set(), set(), set(), set()
    for k, degree, n_circuits, lookup in cases.KERNEL_CASES:
        ks.add(k)
        rots.add(1 << (degree - 2).bit_length())
        ns.add(n_circuits)
        sets.add(lookup)
    assert ks == {5, 8, 9} and rots == {2, 4, 8, 16} and ns == {1, 2, 3} and sets == {"plain", 1, 3, 6}
    assert cases.N_INST == 2 and cases.N_SHUFFLES == 2 and -(-cases.N_PERM // cases.CHUNK) == 2


def test_slice_entry_refuses_a_slice_beyond_the_domain(gpu):
    from halo2_scaffold_amd import custom, engine, plonk
    from halo2_scaffold_amd._lib import H2miError
    from halo2_scaffold_amd.device import DevBuf

    dom = gpu.EvaluationDomain(5, 5)  # rot = 4
    buf = DevBuf(32 * 32)
    prog = engine.GateProgram.build([(engine.EXPR_ADVICE, 0, 0), (engine.EXPR_END, 0, 0)], [])
    arr = plonk.expr_cosets_array([{"advice": [buf], "fixed": [], "instance": None, "perm_values": [], "perm_zs": [], "lookups": []}], [], 1, buf, buf, buf)
    out = DevBuf(128 * 32)
    plonk.evaluate_h_expr_slice(dom, prog, arr, 1, 3, 1, 2, 3, out)
    with pytest.raises(H2miError) as e:
        plonk.evaluate_h_expr_slice(dom, prog, arr, 1, 4, 1, 2, 3, out)
    assert e.value.code == -6  # H2MI_ERANGE


# ---- 2. proof bytes: by coset == resident -----------------------------------------------------------------------------------------------------
def _custom_pair(gpu, cs, first, k, prove, logup=False):
    """prove(custom, params, keys) -> anything comparable, once against a resident key and once against a by-coset key of the circuit"""
    from halo2_scaffold_amd import custom

    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    out = []
    for by_coset in (False, True):
        keys = custom.Keys(params, cs, first, logup=logup, by_coset=by_coset)
        out.append((prove(custom, params, keys), keys.fixed_commitments.tobytes(), keys.permutation_commitments.tobytes(), keys.vk_bytes()))
        keys.release()
    params.release()
    assert out[0] == out[1]
    return out[0][0]


def _one(asg, seed=31, multiopen="shplonk"):
    return lambda custom, params, keys: custom.create_proof(params, keys, asg, seed, multiopen=multiopen)


def _build(custom, name):
    """-> (cs, assignment or synthesize, k, logup) of a named circuit of the case modules, at the smallest k its module uses"""
    if name == "is_zero":
        return (*gate_cases.is_zero_circuit(custom, 5), 5, False)
    if name == "or":
        return (*gate_cases.or_circuit(custom, 1, 0), 5, False)
    if name == "degree6":
        return (*gate_cases.degree6_circuit(custom, 3, 4), 5, False)
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
    if name == "eight_instances":  # columns of 0, 1, 2, 3, 15, 16, 17 and 26 public inputs: the 16-value switch from both sides
        return (*instance_cases.eight_cols_circuit(custom, 5), 5, False)
    if name == "eight_instances_58":  # the same with a column of 58
        return (*instance_cases.eight_cols_circuit(custom, 6), 6, False)
    if name == "rational":
        return (*assigned_cases.is_zero_circuit(custom, 7), 5, False)
    raise KeyError(name)


CUSTOM_CIRCUITS = ["is_zero", "or", "degree6", "xor", "logup", "merged3", "shuffles", "two_phase", "eight_instances", "eight_instances_58", "rational"]


@pytest.mark.parametrize("name", CUSTOM_CIRCUITS)
def test_same_proof_bytes_as_the_resident_key(gpu, name):
    from halo2_scaffold_amd import custom

    cs, asg, k, logup = _build(custom, name)
    first = shuffle_cases.first_assignment(cs, asg)
    proof = _custom_pair(gpu, cs, first, k, _one(asg), logup)
    assert len(proof) > 0
    if name in ("eight_instances", "eight_instances_58"):
        lens = sorted(len(c) for c in instance_cases.columns_of(cs, asg))
        assert lens[3] == 3 and lens[-1] >= 26 and min(l for l in lens if l > 16) == 17


@pytest.mark.parametrize("name", ["is_zero", "merged3"])
def test_same_proof_bytes_with_the_gwc_ending(gpu, name):
    from halo2_scaffold_amd import custom

    cs, asg, k, logup = _build(custom, name)
    _custom_pair(gpu, cs, shuffle_cases.first_assignment(cs, asg), k, _one(asg, 9, "gwc"), logup)


@pytest.mark.parametrize("n_circuits", [1, 3])
def test_same_proof_bytes_for_batches(gpu, n_circuits):
    from halo2_scaffold_amd import custom

    xs = [5, 0, 77][:n_circuits]
    built = [gate_cases.is_zero_circuit(custom, x) for x in xs]
    cs, asgs = built[0][0], [b[1] for b in built]
    prove = lambda custom, params, keys: custom.prove_many(keys, asgs, seeds=[40 + 8 * i for i in range(n_circuits)], params=params)
    proof = _custom_pair(gpu, cs, asgs[0], 5, prove)
    if n_circuits == 1:  # a batch of one is the single prover's proof
        assert proof == _custom_pair(gpu, cs, asgs[0], 5, _one(asgs[0], 40))


def test_same_proof_bytes_for_a_batch_with_public_inputs(gpu):
    """two circuits of the two-instance-column system: the leader's shared slices serve both members"""
    from halo2_scaffold_amd import custom

    built = [instance_cases.two_cols_circuit(custom, v) for v in (0, 1)]
    cs, asgs = built[0][0], [b[1] for b in built]
    _custom_pair(gpu, cs, asgs[0], 5, lambda custom, params, keys: custom.prove_many(keys, asgs, seeds=[40, 48], params=params))


def test_same_proof_bytes_at_degree_nine_and_k_13(gpu):
    """six lookup-advice columns merged into ONE logUp argument of six input sets: degree 9, rot = 8, 2^13 rows (32 workgroups per slice,
    transforms of two passes); the device-byte counter equals the formula in both modes and shows what the mode is for"""
    from halo2_scaffold_amd import custom, engine

    cs, asg = logup_sets_cases.range_circuit(custom, columns=6, max_degree=9)
    k = 13
    assert cs.degree() == 9
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    proofs, totals = [], []
    for by_coset in (False, True):
        keys = custom.Keys(params, cs, asg, logup=True, by_coset=by_coset)
        ws = custom.Workspace(params, keys)
        got = ws.prover.device_bytes()
        counts = _counts(cs.abi(k), keys.keys, [("exprs", len(arg)) for arg in cs.lookup_arguments], len(cs.shuffles), True, k)
        assert got == cases.device_bytes(counts, by_coset)
        totals.append(sum(got))
        proofs.append(custom.create_proof(params, keys, asg, 3, ws=ws))
        ws.release()
        keys.release()
    params.release()
    assert proofs[0] == proofs[1]
    # at least (rot - 1) n 32 bytes for each column and argument vector the quotient reads (l_0 / l_last / l_active, which the mode newly
    # keeps as coefficients beside their slice, are not counted among them)
    n, rot = 1 << k, 8
    assert totals[0] - totals[1] >= (rot - 1) * n * 32 * (cases.quotient_columns(counts) - 3)


# ---- hard-wired shapes, and the committed goldens -----------------------------------------------------------------------------------------
def _smallest(cases_list, shape=None):
    pool = [c for c in cases_list if shape is None or c.get("shape") == shape]
    return min(pool, key=lambda c: c["k"])


def test_standard_plonk_same_bytes_and_the_committed_golden(gpu):
    from halo2_scaffold_amd import circuits, keygen, prover

    gold = json.load(open(os.path.join(GOLD, "standard_plonk_proofs.json")))
    case = _smallest(gold["cases"])
    k, x, seed = case["k"], int(case["witness_x"], 16), case["seed"]
    params = gpu.ParamsKZG.setup(k, int(gold["srs_secret"], 16))
    circuit = circuits.StandardPlonk(None)
    vk = keygen.keygen_vk(params, circuit)
    proofs = []
    for by_coset in (False, True):
        pk = keygen.keygen_pk(params, vk, circuit, by_coset=by_coset)  # the commitments are the verifying key's, or this raises
        proofs.append(prover.create_proof(params, pk, circuits.StandardPlonk(x), seed))
        proofs.append(prover.create_proof(params, pk, circuits.StandardPlonk(x + 1), seed + 1, multiopen="gwc"))
        pk.release()
    params.release()
    assert proofs[2].hex() == case["proof"]  # by coset against the committed bytes: the resident quotient is not involved
    assert proofs[:2] == proofs[2:]


@pytest.mark.parametrize("file,shape", [("flex_proofs.json", "halo2_lib"), ("flex_proofs.json", "range"), ("flex_multi_proofs.json", "range")])
def test_flex_shapes_same_bytes_and_the_committed_goldens(gpu, file, shape):
    """the one-column gate shape, the one-column range shape with its lookup (the specialised kernels' shapes) and the many-column shape,
    each through its equivalent program on a by-coset key"""
    from halo2_scaffold_amd import flex

    g = json.load(open(os.path.join(GOLD, file)))
    case = _smallest(g["cases"], shape)
    k, bits, x, seed = case["k"], case["lookup_bits"], int(case["x"], 16), case["seed"]
    closure = (lambda cs: flex.range_closure(cs, x, bits)) if shape == "range" else (lambda cs: flex.halo2_lib_closure(cs, x))
    cs = flex.configure(shape == "range", k, closure) if file == "flex_multi_proofs.json" else flex.FlexGateCS(lookup=shape == "range")
    asg = closure(cs)
    params = gpu.ParamsKZG.setup(k, int(g["srs_secret"], 16))
    proofs = []
    for by_coset in (False, True):
        keys = flex.FlexKeys(params, cs, asg, by_coset=by_coset)
        assert keys.vk_bytes().hex() == case["vk_bytes"]
        proofs.append(flex.create_proof(params, keys, asg, seed))
        keys.release()
    params.release()
    assert proofs[1].hex() == case["proof"] and proofs[0] == proofs[1]


# ---- 3. randomly generated constraint systems ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", random_circuit_cases.GPU_SEEDS)
def test_generated_circuits_same_bytes_and_accepted(gpu, seed):
    from halo2_scaffold_amd import custom

    case = random_circuit_cases.generate(custom, seed)
    cs, k = case.cs, case.k
    none = [None] * len(cs.challenge_phase)
    first = case.synthesizers[0](none)
    wits = random_circuit_cases.witnesses(case)

    def prove(custom, params, keys):
        if len(wits) > 1:
            return custom.prove_many(keys, wits, seeds=[13 + 8 * i for i in range(len(wits))], params=params, multiopen=case.multiopen)
        return custom.create_proof(params, keys, wits[0], 13, multiopen=case.multiopen)

    try:
        proof = _custom_pair(gpu, cs, first, k, prove, case.logup)
    except Exception as e:
        raise AssertionError(f"{case.describe()}: {type(e).__name__}: {e}") from e
    ocs = instance_cases.oracle_cs(cs, "random")
    oasg = instance_cases.oracle_assignment(ocs, cs, first)
    vk = FX.VerifierKeys(ocs, k, SRS_SECRET, oasg.fixed, oasg.copies)
    instances = [instance_cases.columns_of(cs, s(none)) for s in case.synthesizers]
    assert instance_cases.verify_circuits(vk, cs, proof, instances, logup=case.logup, multiopen=case.multiopen), case.describe()


# ---- 4. route, buffers, memory, the witness check -----------------------------------------------------------------------------------------------
def _launch_counts(lib, call):
    """(launches of any quotient kernel, launches of k_evaluate_h_expr_slice) during call(): the profile's queries are by prefix"""
    assert lib.h2mi_profile_reset() == 0 and lib.h2mi_profile_filter(b"") == 0 and lib.h2mi_profile_enable(1) == 0
    try:
        call()
    finally:
        assert lib.h2mi_profile_enable(0) == 0
    ms, every, sliced = C.c_double(), C.c_uint64(), C.c_uint64()
    assert lib.h2mi_profile_query(b"k_evaluate_h", C.byref(ms), C.byref(every)) == 0
    assert lib.h2mi_profile_query(b"k_evaluate_h_expr_slice", C.byref(ms), C.byref(sliced)) == 0
    return every.value, sliced.value


@pytest.mark.parametrize("name,rot", [("is_zero", 2), ("xor", 4), ("degree6", 8)])
def test_a_by_coset_proof_runs_rot_slice_launches_and_no_other_quotient_kernel(gpu, name, rot):
    from halo2_scaffold_amd import custom

    cs, asg, k, logup = _build(custom, name)
    assert 1 << ((cs.degree() - 2).bit_length()) == rot
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    counts = {}
    for by_coset in (False, True):
        keys = custom.Keys(params, cs, asg, logup=logup, by_coset=by_coset)
        counts[by_coset] = _launch_counts(gpu.lib, lambda: custom.create_proof(params, keys, asg, 2))
        keys.release()
    params.release()
    assert counts[True] == (rot, rot) and counts[False] == (1, 0)


def test_standard_plonk_by_coset_goes_through_the_program_route(gpu):
    from halo2_scaffold_amd import circuits, keygen, prover

    params = gpu.ParamsKZG.setup(5, SRS_SECRET)
    circuit = circuits.StandardPlonk(None)
    pk = keygen.keygen_pk(params, keygen.keygen_vk(params, circuit), circuit, by_coset=True)
    assert _launch_counts(gpu.lib, lambda: prover.create_proof(params, pk, circuits.StandardPlonk(9), 1)) == (2, 2)
    pk.release()
    params.release()


def test_buffer_queries(gpu):
    """the *_COSET kinds are H2MI_EINVAL on a by-coset key and its provers; every other kind answers, and H2MI_BUF_H holds the same
    words as after the same proof on a resident key"""
    from halo2_scaffold_amd import custom, engine

    cs, asg, k, _ = _build(custom, "xor")
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    lib = gpu.lib
    hs = []
    for by_coset in (False, True):
        keys = custom.Keys(params, cs, asg, by_coset=by_coset)
        ws = custom.Workspace(params, keys)
        custom.create_proof(params, keys, asg, 4, ws=ws)
        ptr, count = C.c_void_p(), C.c_size_t()
        for kind in cases.PROVER_COSET_KINDS + cases.KEY_COSET_KINDS:
            rc = lib.h2mi_prover_buffer(ws.prover.handle, kind, 0, C.byref(ptr), C.byref(count))
            assert rc == (cases.EINVAL if by_coset else 0), kind
        for kind in cases.KEY_COSET_KINDS:
            rc = lib.h2mi_prover_pk_buffer(keys.keys.handle, kind, 0, C.byref(ptr), C.byref(count))
            assert rc == (cases.EINVAL if by_coset else 0), kind
        for kind in (engine.BUF_ADVICE, engine.BUF_ADVICE_POLY, engine.BUF_PERM_Z, engine.BUF_PERM_Z_POLY, engine.BUF_H, engine.PKBUF_FIXED,
                     engine.PKBUF_FIXED_POLY, engine.PKBUF_SIGMA, engine.PKBUF_SIGMA_POLY):
            assert lib.h2mi_prover_buffer(ws.prover.handle, kind, 0, C.byref(ptr), C.byref(count)) == 0, kind
            assert count.value == (keys.domain.extended_len() if kind == engine.BUF_H else 1 << k)
        hs.append(ws.prover.view(engine.BUF_H).to_numpy().copy())
        ws.release()
        keys.release()
    params.release()
    assert (hs[0] == hs[1]).all()


def _counts(abi, ekeys, lookups, n_shuffles, logup, k):
    from halo2_scaffold_amd import engine

    sigma = [_vals(v, 1 << k) for v in ekeys.views(engine.PKBUF_SIGMA, abi.n_perm)]
    return cases.counts_of(abi, lookups, n_shuffles, logup, sigma, P.FR_DELTA, o.omega_for(k))


@pytest.mark.parametrize("shape", ["standard_plonk", "range", "shuffles"])
def test_device_bytes_equal_the_formula_in_both_modes(gpu, shape):
    from halo2_scaffold_amd import circuits, custom, engine, flex, keygen

    sums = []
    for by_coset in (False, True):
        if shape == "standard_plonk":
            k = 6
            params = gpu.ParamsKZG.setup(k, SRS_SECRET)
            circuit = circuits.StandardPlonk(None)
            pk = keygen.keygen_pk(params, keygen.keygen_vk(params, circuit), circuit, by_coset=by_coset)
            ekeys, abi, lookups, n_shuffles, release = pk.keys, keygen.constraint_system(circuit, k), [], 0, pk.release
        elif shape == "range":
            g = json.load(open(os.path.join(GOLD, "flex_proofs.json")))
            case = _smallest(g["cases"], "range")
            k, bits = case["k"], case["lookup_bits"]
            params = gpu.ParamsKZG.setup(k, SRS_SECRET)
            cs = flex.FlexGateCS(lookup=True)
            asg = flex.range_closure(cs, int(case["x"], 16), bits)
            keys = flex.FlexKeys(params, cs, asg, by_coset=by_coset)
            abi = cs.abi(k)
            distinct = len({v % R for v in asg.table_values} | {0})  # the table's values and the zero of its unassigned usable rows
            lookups = [("column", abi.lookups[l].selector_fixed >= 0, distinct) for l in range(abi.n_lookups)]
            ekeys, n_shuffles, release = keys.keys, 0, keys.release
        else:
            cs, asg, k, _ = _build(custom, "shuffles")
            params = gpu.ParamsKZG.setup(k, SRS_SECRET)
            keys = custom.Keys(params, cs, asg, by_coset=by_coset)
            abi, lookups = cs.abi(k), [("exprs", len(arg)) for arg in cs.lookup_arguments]
            ekeys, n_shuffles, release = keys.keys, len(cs.shuffles), keys.release
        prover = engine.Prover(ekeys, params)
        got = prover.device_bytes()
        assert got == cases.device_bytes(_counts(abi, ekeys, lookups, n_shuffles, False, k), by_coset), (shape, by_coset)
        kb, pb = C.c_size_t(), C.c_size_t()  # either pointer may be NULL
        assert gpu.lib.h2mi_prover_device_bytes(prover.handle, None, C.byref(pb)) == 0 and gpu.lib.h2mi_prover_device_bytes(prover.handle, C.byref(kb), None) == 0
        assert (kb.value, pb.value) == got
        sums.append(sum(got))
        prover.release()
        release()
        params.release()
    assert sums[1] < sums[0]


@pytest.mark.parametrize("name", ["is_zero", "xor"])
def test_an_unsatisfied_witness_is_reported_as_on_a_resident_key(gpu, name):
    from halo2_scaffold_amd import custom

    if name == "is_zero":
        cs, good = gate_cases.is_zero_circuit(custom, 5)
        _, bad = gate_cases.is_zero_circuit(custom, 5, flip_out=True)
    else:
        cs, good = lookup_cases.xor_circuit(custom)
        _, bad = lookup_cases.xor_circuit(custom, bad="absent")
    params = gpu.ParamsKZG.setup(5, SRS_SECRET)
    said = []
    for by_coset in (False, True):
        keys = custom.Keys(params, cs, good, by_coset=by_coset)
        ws = custom.Workspace(params, keys)
        custom.check(params, keys, good, ws=ws)  # a satisfied witness: silent
        with pytest.raises(ValueError) as e:
            custom.check(params, keys, bad, ws=ws)
        said.append((str(e.value), [(f.kind, f.index, f.row, f.count) for f in e.value.failures]))
        ws.release()
        keys.release()
    params.release()
    assert said[0] == said[1] and said[0][1]
