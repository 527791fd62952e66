"""The quotient, product and polynomial kernels at the limb extremes (tests/extreme_cases.py; tests/test_extreme_cases_host.py proves
on the CPU that the cases are what they claim).

Every field kernel runs on the lazy 29-bit-limb layer (csrc/f29.cuh) under bounds that are written as comments; a violated bound gives
a wrong field element only for operands near it, which the uniformly random or witness-derived inputs of the other GPU tests never are.
Here every operand slot of a kernel — column, challenge, scalar, point, root — takes the extreme memory words (kernels that multiply
words as they lie) or the extreme values (kernels that convert on load), all at once ("all r - 1", "all zero", "all top", "all over")
and mixed.
  1. vector kernels on raw words: k_eval_poly(_multi), the three k_kate_*_multi passes, k_lincomb ("each group < 1.02p: at most 8
     groups"), k_instance_coset ("four normalized addends at most between carries"), k_fr_mul, k_scale_powers;
  2. quotient kernels point by point on arbitrary pattern vectors, 512 points each: k_evaluate_h_standard_plonk ("lazy: limbs < 1.5 *
     2^30, value < 3.1 p", "4p - inner_r: lazy, limbs < 2^30", "acc: lazy sum of <= 7 normalized values"), k_evaluate_h_range,
     k_evaluate_h_flex, evaluate_h_fold's shuffle and logUp terms (gen::sub: the subtrahend below 4p - 2^232), k_evaluate_h_expr(_batch),
     k_expr_compress and k_expr_check over the gate programs that sit just below and just above expr_encode's 3.9 and 8.0 — with
     3.9 raised to 4.9 the negation of four converted loads of OVER261 (4.0026 p) goes negative, and the programs that hand it to a
     product give a wrong h (a sum's carry would hide it: the contract "below 4p - 2^232" is stricter than the arithmetic needs);
  3. grand products and running sums over two tiles of 1024: perm_factors ("lazy sums below 6p") dense and through
     k_perm_sparse_small, k_lookup_numden(_sparse), k_shuffle_numden, k_logup_numden(_sets) and the mul / add scans.
The references are Python integers: oracle.bn254, tests/batch_cases.py batched_quotient and its shuffle / logUp variants,
tests/perm_scale_cases.py formula_products, oracle/lookup.py lookup_product, the recurrences of tests/shuffle_cases.py and
tests/logup_sets_cases.py.  All comparisons are exact, and the words the kernels store are canonical (below r).
k_evaluate_h_range takes at most four permutation columns, so the six columns in chunks of two run through k_evaluate_h_flex; that
kernel's entry carries no shuffles and no logUp lookups, so those terms (the shared evaluate_h_fold) run through the expression entry's record."""
import ctypes as C
import types

import numpy as np
import pytest

import batch_cases
import extreme_cases as X
import logup_sets_cases
import perm_scale_cases
import shuffle_cases
from oracle import bn254 as o
from oracle import lookup as L

pytestmark = pytest.mark.gpu

R = o.R
SENTINEL = perm_scale_cases.SENTINEL
LOGUP = 0x80000000  # include/h2mi.h H2MI_LOOKUPS_LOGUP


class _ShuffleCosets(C.Structure):
    """include/h2mi.h h2mi_shuffle_cosets"""
    _fields_ = [("n_shuffles", C.c_uint32), ("input", C.c_void_p * 8), ("shuffle", C.c_void_p * 8), ("z", C.c_void_p * 8)]


def _mont(values) -> np.ndarray:
    return np.ascontiguousarray(o.pack([v % R for v in values], R))


def _up(gpu, vec):
    return gpu.DevBuf.from_numpy(np.ascontiguousarray(vec.limbs()))


def _read(buf, count):
    """-> the field values of `count` stored words, which must be canonical"""
    limbs = buf.to_numpy(shape=(count, 4), nbytes=count * 32)
    words = o.unpack(limbs)
    assert all(w < R for w in words), "a stored word is not below r"
    return [X.word_value(w) for w in words]


def _values(limbs):
    words = o.unpack(limbs)
    assert all(w < R for w in words), "a stored word is not below r"
    return [X.word_value(w) for w in words]


def _same(got, want, what):
    if got != want:
        bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} elements differ from the Python integers, first at {bad[0]}")
    assert len(got) == len(want)


def _free(*bufs):
    for b in bufs:
        if b is not None:
            b.free()


def _launches(gpu, kernel: bytes, call):
    """launches of `kernel` during call(), from the library's launch profile"""
    lib = gpu.lib
    assert lib.h2mi_profile_reset() == 0 and lib.h2mi_profile_filter(b"") == 0 and lib.h2mi_profile_enable(1) == 0
    try:
        call()
    finally:
        assert lib.h2mi_profile_enable(0) == 0
    ms, count = C.c_double(), C.c_uint64()
    assert lib.h2mi_profile_query(kernel, C.byref(ms), C.byref(count)) == 0
    assert lib.h2mi_profile_reset() == 0
    return count.value


# ---- 1. vector kernels on raw words -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", X.EVAL_LENGTHS)
def test_eval_polys_at_the_extremes(gpu, n):
    """h2mi_fr_eval_polys_dev: 24 polynomials in one call at every point of the set; h2mi_fr_eval_polys_multi_dev: the same 24 in four
    groups, one point each (k_eval_poly_multi)"""
    vecs, calls = X.eval_case(n)
    bufs = [_up(gpu, v) for v in vecs]
    out = gpu.DevBuf(32 * X.EVAL_POLYS)
    want = {}

    def ref(i, x):
        if (i, x) not in want:
            want[(i, x)] = o.eval_polynomial(vecs[i].values, x)
        return want[(i, x)]

    for x, idx in calls:
        ptrs = (C.c_void_p * len(idx))(*[bufs[i].ptr for i in idx])
        xl = _mont([x])
        assert gpu.lib.h2mi_fr_eval_polys_dev(ptrs, len(idx), n, xl.ctypes.data, out.ptr, None) == 0
        _same(_read(out, len(idx)), [ref(i, x) for i in idx], f"eval_polys, n = {n}, point {x:#x}")
    for first in range(0, len(calls), 4):
        group = [calls[(first + g) % len(calls)] for g in range(4)]
        idx = group[0][1]
        points = [x for x, _ in group]
        ptrs = (C.c_void_p * len(idx))(*[bufs[i].ptr for i in idx])
        counts = (C.c_size_t * 4)(6, 6, 6, 6)
        P = _mont(points)
        assert gpu.lib.h2mi_fr_eval_polys_multi_dev(ptrs, counts, P.ctypes.data, 4, n, out.ptr, None) == 0
        _same(_read(out, len(idx)), [ref(i, points[j // 6]) for j, i in enumerate(idx)], f"eval_polys_multi, n = {n}, points from {first}")
    _free(out, *bufs)


@pytest.mark.parametrize("n", [n for n in X.EVAL_LENGTHS if n >= 2])
def test_kate_division_at_the_extremes(gpu, n):
    nums, roots = X.kate_case(n)
    for name, num in nums:
        limbs = np.ascontiguousarray(num.limbs())
        for b in roots:
            q = gpu.kate_division(limbs, _mont([b])[0])
            _same(_values(q), o.kate_division(num.values, b), f"kate_division, n = {n}, {name}, root {b:#x}")


@pytest.mark.parametrize("n,m", X.KATE_MULTI)
def test_kate_division_multi_at_the_extremes(gpu, n, m):
    """sum_i c_i N / (X - r_i) with the partial-fraction weights of the roots: the kernel's stated definition"""
    nums, root_sets = X.kate_multi_case(n, m)
    out = gpu.DevBuf(32 * n)
    for name, num in nums:
        d = _up(gpu, num)
        single = {}
        for roots in root_sets:
            weights = X.partial_fraction_weights(roots)
            rl, il, wl = _mont(roots), _mont([pow(r, -1, R) for r in roots]), _mont(weights)
            assert gpu.lib.h2mi_fr_kate_division_multi_dev(d.ptr, n, rl.ctypes.data, il.ctypes.data, wl.ctypes.data, m, out.ptr, None) == 0
            for r in roots:
                if r not in single:
                    single[r] = o.kate_division(num.values, r)
            want = [sum(c * single[r][i] for c, r in zip(weights, roots)) % R for i in range(n - 1)]
            _same(_read(out, n - 1), want, f"kate_division_multi, n = {n}, m = {m}, {name}")
        d.free()
    out.free()


@pytest.mark.parametrize("K", X.LINCOMB_K)
def test_lincomb_at_the_extremes(gpu, K):
    """k_lincomb: "each group < 1.02p: at most 8 groups, < 8.2p" — 24 terms, every polynomial word and every scalar at the top"""
    for name, polys, scalars in X.lincomb_case(K):
        got = gpu.lincomb([np.ascontiguousarray(p.limbs()) for p in polys], _mont(scalars))
        want = [sum(s * p.values[i] for s, p in zip(scalars, polys)) % R for i in range(X.LINCOMB_N)]
        _same(_values(got), want, f"lincomb, K = {K}, {name}")


@pytest.mark.parametrize("count", X.INSTANCE_COUNTS)
def test_instance_coset_at_the_extremes(gpu, count):
    """k_instance_coset: "four normalized addends at most between carries" — out[j] = sum_r v_r l0[(j - r rot) mod size]"""
    k, ext_k = X.INSTANCE_K, X.INSTANCE_EXT_K
    size, rot = 1 << ext_k, 1 << (ext_k - k)
    out = gpu.DevBuf(32 * size)
    for name, l0, values in X.instance_case(count):
        d = _up(gpu, l0)
        vl = _mont(values)
        assert gpu.lib.h2mi_plonk_instance_coset_dev(d.ptr, k, ext_k, vl.ctypes.data, count, out.ptr, None) == 0
        want = [sum(v * l0.values[(j - r * rot) % size] for r, v in enumerate(values)) % R for j in range(size)]
        _same(_read(out, size), want, f"instance_coset, count = {count}, {name}")
        d.free()
    out.free()


def test_fr_mul_and_scale_powers_at_the_extremes(gpu):
    n = X.VECTOR_N
    out = gpu.DevBuf(32 * n)
    for pa, pb, a, b in X.mul_case():
        da, db = _up(gpu, a), _up(gpu, b)
        assert gpu.lib.h2mi_fr_mul_dev(da.ptr, db.ptr, n, out.ptr, None) == 0
        _same(_read(out, n), [x * y % R for x, y in zip(a.values, b.values)], f"fr_mul, {pa} times {pb}")
        _free(da, db)
    out.free()
    for name, data, base, post in X.scale_case():
        d = _up(gpu, data)
        bl, pl = _mont([base]), _mont([post])
        assert gpu.lib.h2mi_fr_scale_powers_dev(d.ptr, n, bl.ctypes.data, pl.ctypes.data, None) == 0
        want, pw = [], post
        for v in data.values:
            want.append(v * pw % R)
            pw = pw * base % R
        _same(_read(d, n), want, f"scale_powers with a post factor, {name}")
        d.free()


# ---- 2. quotient kernels, point by point ------------------------------------------------------------------------------------------------
def _quotient_args(dom, k, ops, constants, challenges=()):
    return (k, dom.extended_k, dom.g_coset, dom.extended_omega, batch_cases.keys_delta(), X.BF, ops, constants, list(challenges))


def test_standard_plonk_quotient_at_the_extremes(gpu):
    """k_evaluate_h_standard_plonk takes words as they lie: 3 advice, 5 fixed, 3 sigma, 3 z vectors and l0 / l_last / l_active from the
    raw-word patterns, beta, gamma, y from the set"""
    from halo2_scaffold_amd import custom, plonk

    k = X.STANDARD_K
    dom = gpu.EvaluationDomain(3, k)
    size = 1 << dom.extended_k
    assert size == 512
    ops, constants = X.compile_programs([X.standard_plonk_program(custom)])
    out = gpu.DevBuf(32 * size)
    for rnd in X.standard_rounds():
        c = rnd["cols"]
        d = {name: _up(gpu, vec) for name, vec in c.items()}
        group = lambda prefix, count, src: [src[f"{prefix}{j}"] for j in range(count)]
        plonk.evaluate_h(dom, group("advice", 3, d), group("fixed", 5, d), group("sigma", 3, d), group("z", 3, d), d["l0"], d["l_last"], d["l_active"],
                         rnd["beta"], rnd["gamma"], rnd["y"], out)
        v = {name: vec.values for name, vec in c.items()}
        circuit = {"advice": group("advice", 3, v), "fixed": group("fixed", 5, v), "instance": None, "perm_values": group("advice", 3, v),
                   "perm_zs": group("z", 3, v), "lookups": []}
        shared = {"perm_sigmas": group("sigma", 3, v), "chunk": 1, "l0": v["l0"], "l_last": v["l_last"], "l_active": v["l_active"]}
        want = batch_cases.batched_quotient(*_quotient_args(dom, k, ops, constants), [circuit], shared, rnd["beta"], rnd["gamma"], rnd["y"])
        _same(_read(out, size), want, f"evaluate_h, {rnd['name']}")
        _free(*d.values())
    out.free()


def _vertical_gate(custom, advice: int, fixed: int):
    """q (a + a(wX) a(w^2 X) - a(w^3 X))"""
    A = lambda rot: custom.Expression("query", "advice", advice, rot)
    return (A(0) + A(1) * A(2) - A(3)) * custom.Expression("query", "fixed", fixed, 0)


@pytest.mark.parametrize("shape", range(len(X.RANGE_SHAPES)))
def test_range_quotient_at_the_extremes(gpu, shape):
    """k_evaluate_h_range: the vertical gate, a full and a ragged pair of permutation sets in chunks of two, the five lookup terms with
    the input a lookup-advice column or selector * a"""
    from halo2_scaffold_amd import custom, plonk

    n_perm, chunk, lookup = X.RANGE_SHAPES[shape]
    sets = -(-n_perm // chunk)
    k = X.RANGE_K
    dom = gpu.EvaluationDomain(4, k)
    size = 1 << dom.extended_k
    assert size == 512
    ops, constants = X.compile_programs([_vertical_gate(custom, 0, 0)])
    out = gpu.DevBuf(32 * size)
    for rnd in X.range_rounds(shape):
        c = rnd["cols"]
        d = {name: _up(gpu, vec) for name, vec in c.items()}
        group = lambda prefix, count, src: [src[f"{prefix}{j}"] for j in range(count)]
        plonk.evaluate_h_range(dom, d["a"], d.get("lookup_advice"), d["q"], d["table"], group("perm_value", n_perm, d), group("perm_sigma", n_perm, d),
                               group("perm_z", sets, d), d["lk_pin"], d["lk_ptab"], d["lk_z"], d["l0"], d["l_last"], d["l_active"], rnd["beta"], rnd["gamma"],
                               rnd["y"], out, lookup_selector=d.get("lookup_selector"), chunk_len=chunk)
        v = {name: vec.values for name, vec in c.items()}
        lk_in = (v["lookup_advice"], None) if lookup == "advice" else (v["lookup_selector"], v["a"])
        circuit = {"advice": [v["a"]], "fixed": [v["q"]], "instance": None, "perm_values": group("perm_value", n_perm, v), "perm_zs": group("perm_z", sets, v),
                   "lookups": [lk_in + (v["table"], v["lk_pin"], v["lk_ptab"], v["lk_z"])]}
        shared = {"perm_sigmas": group("perm_sigma", n_perm, v), "chunk": chunk, "l0": v["l0"], "l_last": v["l_last"], "l_active": v["l_active"]}
        want = batch_cases.batched_quotient(*_quotient_args(dom, k, ops, constants), [circuit], shared, rnd["beta"], rnd["gamma"], rnd["y"])
        _same(_read(out, size), want, f"evaluate_h_range, {n_perm} columns, lookup input {lookup}, {rnd['name']}")
        _free(*d.values())
    out.free()


def test_flex_quotient_at_the_extremes(gpu):
    """k_evaluate_h_flex: three vertical gates, six permutation columns in chunks of two, two lookups of which one has a second input
    factor; every operand converted on load, so the columns are value patterns"""
    from halo2_scaffold_amd import custom, plonk

    k = X.FLEX_K
    dom = gpu.EvaluationDomain(4, k)
    size = 1 << dom.extended_k
    assert size == 512
    G, M, chunk, NL = X.FLEX_GATES, X.FLEX_PERM, X.FLEX_CHUNK, X.FLEX_LOOKUPS
    sets = -(-M // chunk)
    ops, constants = X.compile_programs([_vertical_gate(custom, g, g) for g in range(G)])
    out = gpu.DevBuf(32 * size)
    for rnd in X.flex_rounds():
        c = rnd["cols"]
        d = {name: _up(gpu, vec) for name, vec in c.items()}
        v = {name: vec.values for name, vec in c.items()}
        group = lambda prefix, count, src: [src[f"{prefix}{j}"] for j in range(count)]
        lookups = lambda src: [(src[f"lk{l}_in"], src.get(f"lk{l}_in_b"), src[f"lk{l}_table"], src[f"lk{l}_pin"], src[f"lk{l}_ptab"], src[f"lk{l}_z"]) for l in range(NL)]
        plonk.evaluate_h_flex(dom, list(zip(group("gate_a", G, d), group("gate_q", G, d))), group("perm_value", M, d), group("perm_sigma", M, d),
                              group("perm_z", sets, d), chunk, lookups(d), d["l0"], d["l_last"], d["l_active"], rnd["beta"], rnd["gamma"], rnd["y"], out)
        circuit = {"advice": group("gate_a", G, v), "fixed": group("gate_q", G, v), "instance": None, "perm_values": group("perm_value", M, v),
                   "perm_zs": group("perm_z", sets, v), "lookups": lookups(v)}
        shared = {"perm_sigmas": group("perm_sigma", M, v), "chunk": chunk, "l0": v["l0"], "l_last": v["l_last"], "l_active": v["l_active"]}
        want = batch_cases.batched_quotient(*_quotient_args(dom, k, ops, constants), [circuit], shared, rnd["beta"], rnd["gamma"], rnd["y"])
        _same(_read(out, size), want, f"evaluate_h_flex, {rnd['name']}")
        _free(*d.values())
    out.free()


def _scalars(plonk, dom, rnd):
    """the h2mi_quotient_scalars of a round -> (record, objects to keep alive)"""
    from halo2_scaffold_amd import field as F

    mm = F.fr_to_mont_limbs
    t_inv = np.ascontiguousarray(plonk.vanishing_inverses(dom))
    scal = [mm(rnd["beta"]), mm(rnd["gamma"]), mm(rnd["y"]), mm(plonk.FR_DELTA), mm(dom.g_coset), mm(dom.extended_omega)]
    return plonk.QuotientScalars(dom.k, dom.extended_k, X.BF, *[x.ctypes.data for x in scal], t_inv.ctypes.data), (t_inv, scal)


def _records(plonk, dom, rnd, program, cosets, n_circuits, challenges=(), shuffles=None, logup=None):
    """the two records every evaluate_h_expr entry takes -> (h2mi_quotient_circuits, h2mi_quotient_scalars, objects to keep alive)"""
    qs, keep = _scalars(plonk, dom, rnd)
    ch = _mont(challenges) if len(challenges) else None
    addr = lambda x: C.addressof(x) if x is not None else None
    qc = plonk.QuotientCircuits(addr(cosets), n_circuits, addr(shuffles), addr(logup), None, addr(program), ch.ctypes.data if ch is not None else None,
                                len(challenges))
    return qc, qs, (keep, ch)


@pytest.mark.parametrize("n_sets", X.LOGUP_SETS)
def test_shuffle_and_logup_terms_at_the_extremes(gpu, n_sets):
    """evaluate_h_fold's shuffle terms and its logUp term with 1 and 6 input sets (N starts as a negation: 4p for M = 0), behind a
    one-query program, through h2mi_plonk_evaluate_h_expr_dev"""
    from halo2_scaffold_amd import engine, plonk

    k = X.FLEX_K
    dom = gpu.EvaluationDomain(4, k)
    size = 1 << dom.extended_k
    ops = [(engine.ADVICE, 0, 0), (engine.EXPR_END, 0, 0)]
    program = engine.GateProgram.build(ops, [])
    logup = engine.LogupInputs.build([n_sets])
    out = gpu.DevBuf(32 * size)
    for rnd in X.fold_rounds(n_sets):
        c = rnd["cols"]
        v = {name: vec.values for name, vec in c.items()}
        d = {name: _up(gpu, vec) for name, vec in c.items() if not name.startswith("lg_in")}
        d_sets = gpu.DevBuf.from_numpy(np.ascontiguousarray(np.concatenate([c[f"lg_in{j}"].limbs() for j in range(n_sets)])))  # set j at element j * size
        cs = plonk._ExprCosets()
        cs.advice[0] = d["advice0"].ptr
        cs.n_lookups = 1 | LOGUP
        cs.lookup_input[0], cs.lookup_table[0], cs.lookup_permuted_input[0], cs.lookup_z[0] = d_sets.ptr, d["lg_table"].ptr, d["lg_m"].ptr, d["lg_phi"].ptr
        cs.l0, cs.l_last, cs.l_active = d["l0"].ptr, d["l_last"].ptr, d["l_active"].ptr
        sh = _ShuffleCosets()
        sh.n_shuffles = X.FLEX_SHUFFLES
        for s in range(X.FLEX_SHUFFLES):
            sh.input[s], sh.shuffle[s], sh.z[s] = d[f"sf{s}_in"].ptr, d[f"sf{s}_side"].ptr, d[f"sf{s}_z"].ptr
        qc, qs, keep = _records(plonk, dom, rnd, program, cs, 1, shuffles=sh, logup=logup)
        assert gpu.lib.h2mi_plonk_evaluate_h_expr_dev(C.byref(qc), C.byref(qs), out.ptr, None) == 0
        circuit = {"advice": [v["advice0"]], "fixed": [], "instance": None, "perm_values": [], "perm_zs": [],
                   "lookups": [([v[f"lg_in{j}"] for j in range(n_sets)], None, v["lg_table"], v["lg_m"], None, v["lg_phi"])],
                   "shuffles": [(v[f"sf{s}_in"], v[f"sf{s}_side"], v[f"sf{s}_z"]) for s in range(X.FLEX_SHUFFLES)]}
        shared = {"perm_sigmas": [], "chunk": 1, "l0": v["l0"], "l_last": v["l_last"], "l_active": v["l_active"]}
        want = logup_sets_cases.batched_quotient(*_quotient_args(dom, k, ops, []), [circuit], shared, rnd["beta"], rnd["gamma"], rnd["y"], logup=True)
        _same(_read(out, size), want, f"shuffle and logUp terms, {n_sets} input sets, {rnd['name']}")
        del keep
        _free(d_sets, *d.values())
    out.free()


def _expr_program(custom):
    from halo2_scaffold_amd import engine

    trees = [t for _, t, _ in X.bound_tight_programs(custom)]
    ops, constants = X.compile_programs(trees)
    return ops, constants, engine.GateProgram.build(ops, constants)


@pytest.mark.parametrize("n_circuits,with_terms", [(1, False), (1, True), (2, False), (2, True)])
def test_expr_quotient_at_the_extremes(gpu, n_circuits, with_terms):
    """k_evaluate_h_expr (one circuit) and k_evaluate_h_expr_batch (two) on the bound-tight programs over the value patterns: without any
    argument terms through plonk.evaluate_h_expr / evaluate_h_expr_batch, and with a permutation argument, a lookup with a second input
    factor and a shuffle through records filled here"""
    from halo2_scaffold_amd import custom, plonk

    k = X.EXPR_K
    dom = gpu.EvaluationDomain(4, k)
    size = 1 << dom.extended_k
    assert size == 512
    ops, constants, program = _expr_program(custom)
    out = gpu.DevBuf(32 * size)
    for rnd in X.expr_rounds(n_circuits, with_terms):
        d = {name: _up(gpu, vec) for name, vec in rnd["cols"].items()}
        named = {id(vec): d[name] for name, vec in rnd["cols"].items()}
        circuits_d, shared_d = X.expr_circuits(rnd, n_circuits, with_terms, pick=lambda vec: named[id(vec)])
        circuits, shared = X.expr_circuits(rnd, n_circuits, with_terms)
        ch = rnd["challenges"]
        arr = plonk.expr_cosets_array(circuits_d, shared_d["perm_sigmas"], 2, shared_d["l0"], shared_d["l_last"], shared_d["l_active"])
        if not with_terms and n_circuits == 1:
            c0 = circuits_d[0]
            plonk.evaluate_h_expr(dom, program, c0["advice"], c0["fixed"], c0["instance"], [], [], [], 2, [], shared_d["l0"], shared_d["l_last"],
                                  shared_d["l_active"], rnd["beta"], rnd["gamma"], rnd["y"], out, blinding_factors=X.BF, challenges=ch)
        elif not with_terms:
            plonk.evaluate_h_expr_batch(dom, program, arr, n_circuits, rnd["beta"], rnd["gamma"], rnd["y"], out, blinding_factors=X.BF, challenges=ch)
        else:
            shs = (_ShuffleCosets * n_circuits)()
            for sh, c in zip(shs, circuits_d):
                sh.n_shuffles = len(c["shuffles"])
                for s, (a_in, s_in, z) in enumerate(c["shuffles"]):
                    sh.input[s], sh.shuffle[s], sh.z[s] = a_in.ptr, s_in.ptr, z.ptr
            qc, qs, keep = _records(plonk, dom, rnd, program, arr, n_circuits, ch, shuffles=shs)
            if n_circuits == 1:
                assert gpu.lib.h2mi_plonk_evaluate_h_expr_dev(C.byref(qc), C.byref(qs), out.ptr, None) == 0
            else:
                assert gpu.lib.h2mi_plonk_evaluate_h_expr_batch_dev(C.byref(qc), C.byref(qs), -1, out.ptr, None) == 0
            del keep
        want = shuffle_cases.batched_quotient(*_quotient_args(dom, k, ops, constants, ch), circuits, shared, rnd["beta"], rnd["gamma"], rnd["y"])
        _same(_read(out, size), want, f"evaluate_h_expr, {n_circuits} circuit(s), terms: {with_terms}, {rnd['name']}")
        _free(*d.values())
    out.free()


@pytest.mark.parametrize("domain", ["rows", "extended coset"])
def test_expr_compress_at_the_extremes(gpu, domain):
    """k_expr_compress: out[i] = sum_j e_j(i) theta^(m-1-j) over the bound-tight programs, theta from the set, on the 2^9 rows (a
    rotation is one row) and on the extended coset of 2^7 rows (a rotation is four points)"""
    from halo2_scaffold_amd import custom, plonk

    k, domain_k = (9, 9) if domain == "rows" else (X.EXPR_K, X.EXPR_K + 2)
    size, rot = 1 << domain_k, 1 << (domain_k - k)
    ops, constants, program = _expr_program(custom)
    out = gpu.DevBuf(32 * size)
    for rnd in X.expr_rounds(1, False):
        d = {name: _up(gpu, vec) for name, vec in rnd["cols"].items()}
        named = {id(vec): d[name] for name, vec in rnd["cols"].items()}
        (cd,), _ = X.expr_circuits(rnd, 1, False, pick=lambda vec: named[id(vec)])
        (cv,), _ = X.expr_circuits(rnd, 1, False)
        theta, ch = rnd["y"], rnd["challenges"]
        plonk.expr_compress(program, cd["advice"], cd["fixed"], cd["instance"], k, domain_k, theta, out, challenges=ch)
        cols = {"advice": cv["advice"], "fixed": cv["fixed"], "instance": [cv["instance"]]}
        want = []
        for idx in range(size):
            acc = 0
            for poly in batch_cases.run_postfix(ops, constants, lambda op, col, r: cols[batch_cases.KINDS[op]][col][(idx + r * rot) % size], ch):
                acc = (acc * theta + poly) % R
            want.append(acc)
        _same(_read(out, size), want, f"expr_compress on the {domain}, {rnd['name']}")
        _free(*d.values())
    out.free()


def test_expr_check_at_the_extremes(gpu):
    """k_expr_check: polynomials that vanish on every row only because a full-bound value reduces to the zero word — no row is
    reported; with one planted cell the report names the smallest row that reads it, and counts the rows that do"""
    from halo2_scaffold_amd import custom, engine, plonk

    k = X.CHECK_K
    n = 1 << k
    trees = X.check_program(custom)
    ops, constants = X.compile_programs(trees)
    program = engine.GateProgram.build(ops, constants)
    for name, cols in X.check_rounds():
        d = [_up(gpu, c) for c in cols]
        assert plonk.expr_check(program, d, [], None, k) == [(0, 0xFFFFFFFF)] * len(trees), name
        # one cell of advice1 takes another word of the alphabet: s7(advice0) - s7(advice1) fails on the seven rows that read it
        words = list(cols[1].words)
        alphabet = X.ALPHABETS["values"]
        words[X.CHECK_PLANTED_ROW] = alphabet[(alphabet.index(words[X.CHECK_PLANTED_ROW]) + 1) % len(alphabet)]
        planted = [cols[0], X.Vec(words), cols[2], cols[3]]
        d1 = _up(gpu, planted[1])
        want = []
        for t in trees:
            bad = [row for row in range(n) if t.evaluate(lambda kind, col, rot, row=row: planted[col].values[(row + rot) % n])]
            want.append((len(bad), bad[0] if bad else 0xFFFFFFFF))
        assert want[0] == (7, X.CHECK_PLANTED_ROW - 6) and want[1:] == [(0, 0xFFFFFFFF)] * 3, name
        assert plonk.expr_check(program, [d[0], d1, d[2], d[3]], [], None, k) == want, name
        _free(d1, *d)


def test_quotient_records_are_refused_before_any_launch(gpu):
    """the three argument records of the quotient calls, one circuit on 512 extended points: a NULL record, each required field NULL in
    turn, two circuits on the single-circuit call and a slice outside H2MI_WHOLE_COSET .. rot - 1 are refused with the header's codes,
    and no refused call launches a kernel"""
    from halo2_scaffold_amd import engine, plonk

    EINVAL, ERANGE = -1, -6
    k = X.EXPR_K
    dom = gpu.EvaluationDomain(4, k)
    size, rot = 1 << dom.extended_k, 1 << (dom.extended_k - k)
    assert size == 512
    col, out = gpu.DevBuf(32 * size), gpu.DevBuf(32 * size)
    program = engine.GateProgram.build([(engine.ADVICE, 0, 0), (engine.EXPR_END, 0, 0)], [])
    cs = plonk._ExprCosets()
    cs.advice[0] = cs.l0 = cs.l_last = cs.l_active = col.ptr
    qs, keep = _scalars(plonk, dom, {"beta": 2, "gamma": 3, "y": 5})
    qc = plonk.QuotientCircuits(C.addressof(cs), 1, None, None, None, C.addressof(program), None, 0)
    cols = (C.c_void_p * 1)(col.ptr)
    ec = plonk.ExprColumns(C.addressof(cols), 1, None, 0, None, C.addressof(program), None, 0, k)
    theta, report = _mont([7]), np.zeros((1, 2), dtype=np.uint32)
    lib = gpu.lib
    ref = lambda rec: C.byref(rec) if rec is not None else None
    single = lambda c, s: lib.h2mi_plonk_evaluate_h_expr_dev(ref(c), ref(s), out.ptr, None)
    batch = lambda c, s, sl=-1: lib.h2mi_plonk_evaluate_h_expr_batch_dev(ref(c), ref(s), sl, out.ptr, None)
    compress = lambda e, th=theta.ctypes.data, dst=out.ptr: lib.h2mi_plonk_expr_compress_dev(ref(e), dom.extended_k, th, dst, None)
    check = lambda e, rep=report.ctypes.data: lib.h2mi_plonk_expr_check_dev(ref(e), 1 << k, rep, None, None)

    def without(rec, field, **changed):
        """a copy of the record with one field NULL (or given another value)"""
        other = type(rec).from_buffer_copy(rec)
        for name, value in {field: None, **changed}.items():
            if name:
                setattr(other, name, value)
        return other

    def refusals():
        codes = []
        hard_wired = [(lib.h2mi_plonk_evaluate_h_standard_dev, plonk._Cosets()), (lib.h2mi_plonk_evaluate_h_range_dev, plonk._RangeCosets()),
                      (lib.h2mi_plonk_evaluate_h_flex_dev, plonk._FlexCosets())]
        for call, cosets in hard_wired:  # the scalars are looked at before the cosets' fields
            codes += [(call(C.byref(cosets), None, out.ptr, None), EINVAL), (call(None, C.byref(qs), out.ptr, None), EINVAL)]
        codes += [(single(None, qs), EINVAL), (single(qc, None), EINVAL), (batch(None, qs), EINVAL), (batch(qc, None), EINVAL)]
        for field in ("beta", "gamma", "y", "delta", "zeta", "extended_omega", "t_inv"):
            codes += [(single(qc, without(qs, field)), EINVAL), (batch(qc, without(qs, field)), EINVAL)]
            codes += [(call(C.byref(cosets), C.byref(without(qs, field)), out.ptr, None), EINVAL) for call, cosets in hard_wired]
        for field in ("circuits", "gates"):
            codes += [(single(without(qc, field), qs), EINVAL), (batch(without(qc, field), qs), EINVAL)]
        codes += [(lib.h2mi_plonk_evaluate_h_expr_dev(C.byref(qc), C.byref(qs), None, None), EINVAL),
                  (lib.h2mi_plonk_evaluate_h_expr_batch_dev(C.byref(qc), C.byref(qs), -1, None, None), EINVAL)]
        codes += [(single(without(qc, "", n_circuits=2), qs), EINVAL), (single(without(qc, "", n_circuits=0), qs), EINVAL)]
        codes += [(batch(qc, qs, rot), ERANGE), (batch(qc, qs, -2), EINVAL), (batch(qc, without(qs, "", extended_k=k + 5), 0), ERANGE)]
        codes += [(compress(None), EINVAL), (check(None), EINVAL), (compress(without(ec, "program")), EINVAL), (check(without(ec, "program")), EINVAL),
                  (compress(without(ec, "advice")), EINVAL), (check(without(ec, "advice")), EINVAL), (compress(ec, th=None), EINVAL),
                  (compress(ec, dst=None), EINVAL), (check(ec, rep=None), EINVAL)]
        return codes

    codes = []
    assert _launches(gpu, b"k_", lambda: codes.extend(refusals())) == 0
    assert len(codes) > 60 and all(got == want for got, want in codes), [i for i, (got, want) in enumerate(codes) if got != want]
    # and the records as they stand are taken: the single call, a batch of one whole and by slices, both column calls
    assert single(qc, qs) == 0 and batch(qc, qs) == 0 and all(batch(qc, qs, sl) == 0 for sl in range(rot))
    assert compress(ec) == 0 and check(ec) == 0
    del keep
    _free(col, out)


# ---- 3. grand products and running sums -------------------------------------------------------------------------------------------------
def _sentinel(gpu, n):
    return gpu.DevBuf.from_numpy(_mont([SENTINEL] * n))


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "k_perm_sparse_small"])
def test_permutation_products_at_the_extremes(gpu, sparse):
    """plonk.permutation_products over four columns in chunks of two, rows 0 .. u across two tiles: perm_factors' "lazy sums below 6p"
    with every value, sigma and challenge at an extreme; the rows beyond u stay the caller's"""
    from halo2_scaffold_amd import plonk

    k, u, n = X.PRODUCT_K, X.PRODUCT_U, 1 << X.PRODUCT_K
    for rnd in X.perm_rounds(sparse):
        dv, ds = [_up(gpu, v) for v in rnd["vals"]], [_up(gpu, s) for s in rnd["sig"]]
        dz = [_sentinel(gpu, n) for _ in range(X.PERM_M // X.PERM_CHUNK)]
        active = None
        if sparse:
            active = types.SimpleNamespace(count=len(rnd["active"]), buf=gpu.DevBuf.from_numpy(np.array(rnd["active"], dtype=np.uint32)))
        call = lambda: plonk.permutation_products(k, dv, ds, X.PERM_CHUNK, rnd["beta"], rnd["gamma"], u, dz, active=active)
        small = _launches(gpu, b"k_perm_sparse_small", call)
        assert small == (1 if sparse else 0)
        want = perm_scale_cases.formula_products(k, u, X.PERM_CHUNK, [v.values for v in rnd["vals"]], [s.values for s in rnd["sig"]], rnd["beta"], rnd["gamma"])
        for s, z in enumerate(dz):
            assert want[s][u + 1:] == [SENTINEL] * (n - u - 1)
            _same(_read(z, n), want[s], f"permutation_products, set {s}, {rnd['name']}")
        _free(*(dv + ds + dz + ([active.buf] if sparse else [])))


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_lookup_product_at_the_extremes(gpu, sparse):
    from halo2_scaffold_amd import plonk

    for rnd in X.lookup_rounds(sparse):
        k, u = rnd["k"], rnd["u"]
        n = 1 << k
        bufs = [_up(gpu, rnd[part]) for part in ("a", "t", "ap", "sp")]
        dz = _sentinel(gpu, n)
        compact = _launches(gpu, b"k_lookup_compact", lambda: plonk.lookup_product(k, *bufs, rnd["beta"], rnd["gamma"], u, dz))
        assert compact == (1 if sparse else 0)
        want = L.lookup_product(rnd["a"].values, rnd["t"].values, rnd["ap"].values, rnd["sp"].values, rnd["beta"], rnd["gamma"], u, [])
        assert len(want) == u + 1
        _same(_read(dz, n), want + [SENTINEL] * (n - u - 1), f"lookup_product, {rnd['name']}")
        _free(dz, *bufs)


def test_shuffle_product_at_the_extremes(gpu):
    from halo2_scaffold_amd import plonk

    k, u, n = X.PRODUCT_K, X.PRODUCT_U, 1 << X.PRODUCT_K
    for rnd in X.shuffle_rounds():
        da, ds, dz = _up(gpu, rnd["a"]), _up(gpu, rnd["s"]), _sentinel(gpu, n)
        want = shuffle_cases.shuffle_product(rnd["a"].values, rnd["s"].values, rnd["gamma"], u)
        assert plonk.shuffle_product(k, da, ds, rnd["gamma"], u, dz) is (want[u] == 1)  # z is written either way
        _same(_read(dz, n), want + [SENTINEL] * (n - u - 1), f"shuffle_product, {rnd['name']}")
        _free(da, ds, dz)


@pytest.mark.parametrize("n_sets", X.LOGUP_SETS)
def test_logup_sum_at_the_extremes(gpu, n_sets):
    """k_logup_numden (one set, through plonk.logup_sum too) and k_logup_numden_sets (six), the additive scan over two tiles"""
    from halo2_scaffold_amd import plonk

    k, u, n = X.PRODUCT_K, X.PRODUCT_U, 1 << X.PRODUCT_K
    for rnd in X.logup_rounds(n_sets):
        d_sets = gpu.DevBuf.from_numpy(np.ascontiguousarray(np.concatenate([a.limbs() for a in rnd["sets"]])))
        dt, dm, dphi = _up(gpu, rnd["table"]), _up(gpu, rnd["mult"]), _sentinel(gpu, n)
        plonk.logup_sum_sets(k, d_sets, n_sets, dt, dm, rnd["beta"], u, dphi)
        want = logup_sets_cases.running_sum([a.values for a in rnd["sets"]], rnd["table"].values, rnd["mult"].values, rnd["beta"], u)
        want += [SENTINEL] * (n - u - 1)
        _same(_read(dphi, n), want, f"logup_sum_sets, {n_sets} sets, {rnd['name']}")
        if n_sets == 1:
            again = _sentinel(gpu, n)
            plonk.logup_sum(k, d_sets, dt, dm, rnd["beta"], u, again)
            _same(_read(again, n), want, f"logup_sum, {rnd['name']}")
            again.free()
        _free(d_sets, dt, dm, dphi)
