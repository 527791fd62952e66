"""CPU tests of tests/extreme_cases.py: the inputs tests/test_gpu_extremes.py runs the kernels on are what they claim — every word or
value of an alphabet in every operand slot (a column, a challenge, a scalar, a point, a root) of every case, "all r - 1" and "all zero"
for every kernel, every bound-tight gate program on the intended side of expr_encode's thresholds by the restated rule, no zero
denominator in a product or sum case and no challenge passed over without one — and the references the GPU tests compare against
agree with each other on a real StandardPlonk instance.  Python integers alone."""
import pytest

import batch_cases
import extreme_cases as X
import logup_sets_cases
import shuffle_cases
from oracle import bn254 as o

R = X.R


@pytest.fixture(scope="module")
def custom(h2):
    from halo2_scaffold_amd import custom

    return custom


def _covers(vecs, alphabet):
    """every word of the alphabet occurs in the vectors a slot takes"""
    return set(X.ALPHABETS[alphabet]) <= {w for v in vecs for w in v.words}


def _has_constant(vecs, word):
    return any(set(v.words) == {word} for v in vecs)


def _slot_ok(vecs, alphabet):
    top = R - 1 if alphabet == "words" else X.value_word(R - 1)
    return _covers(vecs, alphabet) and _has_constant(vecs, top) and _has_constant(vecs, 0)


def test_alphabets_and_scalars():
    assert all(w < R for w in X.EXTREME_WORDS) and len(set(X.EXTREME_WORDS)) == 6
    limbs29 = lambda w: [(w >> (29 * i)) & ((1 << 29) - 1) for i in range(8)]
    assert limbs29(X.EXTREME_WORDS[1]) == [(1 << 29) - 1] * 8 and X.EXTREME_WORDS[1] >> 232 == (R >> 232) - 1
    assert X.EXTREME_WORDS[2] == (1 << 232) - 1 and X.EXTREME_WORDS[3:] == [0, 1, R >> 1]
    assert X.EXTREME_VALUES[:5] == [0, 1, R - 1, R - 2, (R - 1) // 2]
    assert X.TOP261 * (1 << 261) % R == R - 1 == X.converted(X.value_word(X.TOP261))  # what gen::ld / cst turn it into
    over = X.converted(X.value_word(X.OVER261))
    assert over > R and over % R == X.OVER261 * (1 << 261) % R and over - R > 0.00065 * R  # a converted load above r, ~the largest there is
    assert all(X.converted(w) < over for w in X.ALPHABETS["values"] if w != X.value_word(X.OVER261))
    assert X.converted(0) == 0 and all(X.converted(w) % R == X.word_value(w) * (1 << 261) % R for w in X.EXTREME_WORDS)
    # o.pack without a modulus keeps raw words; o.unpack with one gives the values the references take
    raw = o.pack(X.EXTREME_WORDS)
    assert o.unpack(raw) == X.EXTREME_WORDS and o.unpack(raw, R) == [X.word_value(w) for w in X.EXTREME_WORDS]
    assert o.unpack(o.pack(X.EXTREME_VALUES, R)) == X.ALPHABETS["values"] and o.unpack(o.pack(X.EXTREME_VALUES, R), R) == X.EXTREME_VALUES
    assert set(X.EXTREME_VALUES) <= set(X.SCALARS) and {X.word_value(w) for w in X.EXTREME_WORDS} <= set(X.SCALARS)
    assert len(X.SCALARS) == len(set(X.SCALARS)) == X.N_ROUNDS == 12
    assert {X.value_word(s) for s in X.SCALARS} >= set(X.EXTREME_WORDS)  # a challenge's memory word takes every raw extreme word


@pytest.mark.parametrize("alphabet", ["words", "values"])
def test_patterns(alphabet):
    top = R - 1 if alphabet == "words" else X.value_word(R - 1)
    for n in (1, 2, 7, 600):
        assert X.vector(alphabet, "all r - 1", n).words == [top] * n and X.vector(alphabet, "all zero", n).words == [0] * n
        assert X.vector(alphabet, "r - 1 / 0 alternating", n).words == [top if i % 2 == 0 else 0 for i in range(n)]
        rnd = X.vector(alphabet, "random choice", n, 1)
        assert len(rnd) == n and set(rnd.words) <= set(X.ALPHABETS[alphabet]) and rnd.words == X.vector(alphabet, "random choice", n, 1).words
        assert _slot_ok([v for _, v in X.pattern_vectors(alphabet, n, "t")], alphabet)  # however short
    assert X.vector(alphabet, "random choice", 600, 1).words != X.vector(alphabet, "random choice", 600, 2).words
    assert X.vector("values", "all top", 3).values == [X.TOP261] * 3 and X.vector("values", "all over", 3).values == [X.OVER261] * 3
    v = X.vector(alphabet, "random choice", 50, 3)
    assert v.values == [X.word_value(w) for w in v.words] == o.unpack(v.limbs(), R) and o.unpack(v.limbs()) == v.words
    assert [p for _, p in X.rounds(alphabet)].count("all r - 1") >= 2 and {p for _, p in X.rounds(alphabet)} == set(X.PATTERNS[alphabet])


# ---- vector kernels ---------------------------------------------------------------------------------------------------------------------
def test_vector_kernel_cases_fill_every_slot():
    S = set(X.SCALARS)
    for n in X.EVAL_LENGTHS:
        vecs, calls = X.eval_case(n)
        assert all(len(v) == n for v in vecs) and _slot_ok(vecs, "words")
        assert {x for x, _ in calls} == S
        for j in range(X.EVAL_POLYS):  # slot j of the 24 takes every vector
            assert {idx[j] for _, idx in calls} == set(range(len(vecs))), (n, j)
        if n >= 2:
            nums, roots = X.kate_case(n)
            assert _slot_ok([v for _, v in nums], "words") and set(roots) == S
    assert min(X.EVAL_LENGTHS) == 1 and max(X.EVAL_LENGTHS) > 4096 and {1023, 1025} <= set(X.EVAL_LENGTHS)
    for n, m in X.KATE_MULTI:
        nums, root_sets = X.kate_multi_case(n, m)
        assert _slot_ok([v for _, v in nums], "words") and n > 2 * 1024 and n % 1024
        for slot in range(m):  # every non-zero scalar in every root slot
            assert {rs[slot] for rs in root_sets} == S - {0}
        for rs in root_sets:
            assert len(set(rs)) == m and 0 not in rs  # distinct and invertible
            c = X.partial_fraction_weights(rs)
            for x in (5, R - 3):  # sum_i c_i / (x - r_i) = 1 / prod (x - r_i)
                prod = 1
                for r_i in rs:
                    prod = prod * (x - r_i) % R
                assert sum(ci * pow(x - r_i, -1, R) for ci, r_i in zip(c, rs)) % R == pow(prod, -1, R)
    assert {m for _, m in X.KATE_MULTI} == {2, 3, 4}
    for K in X.LINCOMB_K:
        calls = X.lincomb_case(K)
        assert calls[0][1][0].words == [R - 1] * X.LINCOMB_N and [X.value_word(s) for s in calls[0][2]] == [R - 1] * K
        assert calls[1][2] == [X.TOP261] * K
        for k in range(K):
            assert _slot_ok([polys[k] for _, polys, _ in calls], "words") and {sc[k] for _, _, sc in calls} == S, (K, k)
    assert X.LINCOMB_K == [1, 2, 3, 24]  # a remainder of one, of two, none; the most terms k_lincomb takes
    for count in X.INSTANCE_COUNTS:
        calls = X.instance_case(count)
        assert all(len(l0) == 512 and len(vals) == count for _, l0, vals in calls) and _slot_ok([l0 for _, l0, _ in calls], "words")
        for r in range(count):
            assert {vals[r] for _, _, vals in calls} == S
    assert X.INSTANCE_COUNTS == [4, 5, 16]  # exactly one carry of k_instance_coset's loop, one addend beyond it, the most
    pairs = X.mul_case()
    assert len(pairs) == 16 and _slot_ok([a for _, _, a, _ in pairs], "words") and _slot_ok([b for _, _, _, b in pairs], "words")
    assert ("all r - 1", "all r - 1") in {(pa, pb) for pa, pb, _, _ in pairs}
    sc = X.scale_case()
    assert _slot_ok([d for _, d, _, _ in sc], "words") and {b for _, _, b, _ in sc} == S and {p for _, _, _, p in sc} == S


# ---- quotient kernels -------------------------------------------------------------------------------------------------------------------
def _rounds_fill_every_slot(rnds, slots, alphabet, scalar_slots=("beta", "gamma", "y")):
    assert len(rnds) == X.N_ROUNDS
    for rnd in rnds:
        assert sorted(rnd["cols"]) == sorted(slots), rnd["name"]
    for name in slots:
        assert _slot_ok([rnd["cols"][name] for rnd in rnds], alphabet), name
    for rnd in rnds:  # "all r - 1" / "all zero" / "all top": every operand of the point at the extreme at once
        if rnd["pattern"].startswith("all"):
            assert len({tuple(v.words) for v in rnd["cols"].values()}) == 1, rnd["name"]
    for s in scalar_slots:
        assert {rnd[s] for rnd in rnds} == set(X.SCALARS), s


def test_quotient_cases_fill_every_slot():
    rnds = X.standard_rounds()
    _rounds_fill_every_slot(rnds, X.STANDARD_SLOTS, "words")
    assert all(len(v) == 512 for v in rnds[0]["cols"].values()) and len(X.STANDARD_SLOTS) == 17
    for shape, (n_perm, chunk, lookup) in enumerate(X.RANGE_SHAPES):
        rnds = X.range_rounds(shape)
        _rounds_fill_every_slot(rnds, X.range_slots(n_perm, chunk, lookup), "words")
        assert all(len(v) == 512 for v in rnds[0]["cols"].values())
    assert {(m, c) for m, c, _ in X.RANGE_SHAPES} == {(4, 2), (3, 2)} and {l for _, _, l in X.RANGE_SHAPES} == {"advice", "selector"}
    rnds = X.flex_rounds()
    _rounds_fill_every_slot(rnds, X.flex_slots(), "values")
    assert X.FLEX_GATES > 1 and X.FLEX_PERM == 6 and X.FLEX_CHUNK == 2 and "lk1_in_b" in X.flex_slots() and "lk0_in_b" not in X.flex_slots()
    assert X.LOGUP_SETS == [1, logup_sets_cases.MAX_LOGUP_INPUTS]
    for n_sets in X.LOGUP_SETS:
        _rounds_fill_every_slot(X.fold_rounds(n_sets), X.fold_slots(n_sets), "values")
    for n_circuits, with_terms in ((1, False), (1, True), (2, False), (2, True)):
        rnds = X.expr_rounds(n_circuits, with_terms)
        slots = X.expr_shared_slots(with_terms) + [s for c in range(n_circuits) for s in X.expr_slots(with_terms, c)]
        _rounds_fill_every_slot(rnds, slots, "values")
        for ch in range(X.N_CHALLENGES):
            assert {rnd["challenges"][ch] for rnd in rnds} == set(X.SCALARS)
        assert {"all top", "all over"} <= {rnd["pattern"] for rnd in rnds}
        circuits, shared = X.expr_circuits(rnds[0], n_circuits, with_terms)
        assert len(circuits) == n_circuits and len(shared["perm_sigmas"]) == (4 if with_terms else 0)
        assert all(len(c["lookups"]) == len(c["shuffles"]) == (1 if with_terms else 0) for c in circuits)
    for name, cols in X.check_rounds():
        assert cols[0].words == cols[1].words and all((a + b) % R == 0 for a, b in zip(cols[2].values, cols[3].values)), name
    assert _slot_ok([cols[0] for _, cols in X.check_rounds()], "values") and _slot_ok([cols[2] for _, cols in X.check_rounds()], "values")


# ---- the bound-tight programs -----------------------------------------------------------------------------------------------------------
def test_bound_tight_programs_sit_where_they_claim(custom):
    programs = X.bound_tight_programs(custom)
    assert len(programs) == 15
    seen = {("small", False): [], ("small", True): [], ("cap", False): [], ("cap", True): []}
    kinds_read, has_challenge, has_top_constant, depths = set(), False, False, set()
    for name, tree, expected in programs:
        ops, constants = tree.program()
        trace = X.encode_trace(ops)
        for kind, bound, reduced in expected:
            assert any(k == kind and round(b, 2) == bound and r == reduced for k, b, r in trace), (name, kind, bound, reduced, trace)
        for kind, bound, reduced in trace:
            assert reduced == (bound > (X.SMALL_TOP if kind == "small" else X.CAP))
            seen[(kind, reduced)].append(bound)
        kinds_read |= {op for op, _, _ in ops if op <= X.OP_INSTANCE}
        has_challenge |= any(op == X.OP_CHALLENGE for op, _, _ in ops)
        has_top_constant |= R - 1 in constants
        depths.add(tree.stack_depth())
    # both sides of both thresholds, as close as the rule's steps allow: 3 and 4 loads around 3.9; 7 loads, 4 + 4 and 8 loads around 8.0
    assert max(seen[("small", False)]) == pytest.approx(3.12) and min(seen[("small", True)]) == pytest.approx(4.16)
    assert max(seen[("cap", False)]) == 8.0 and min(seen[("cap", True)]) == pytest.approx(8.32)
    assert pytest.approx(7.28) in seen[("cap", False)]
    assert kinds_read == {X.OP_ADVICE, X.OP_FIXED, X.OP_INSTANCE} and has_challenge and has_top_constant and max(depths) == 8
    # the values the bounds stand for, in the worst case: a converted load of TOP261 is r - 1, so 4 of them pass 4p - 2^232 and 3 do not;
    # 4 converted loads of OVER261 pass 4p itself — 0 - x + 4p is then negative, whatever the limbs do — and 3 stay below 4p - 2^232;
    # (-0) + (-0) is 8p exactly
    top, over = X.converted(X.value_word(X.TOP261)), X.converted(X.value_word(X.OVER261))
    assert top == R - 1 and 3 * top < 4 * R - (1 << 232) < 4 * top and 7 * top < 8 * R == 8 * top + 8
    assert 3 * over < 4 * R - (1 << 232) and 4 * R < 4 * over and over < 1.04 * R and 7 * over < 7.28 * R
    # the check's polynomials vanish on the columns check_rounds builds, and only there
    trees = X.check_program(custom)
    for _, cols in X.check_rounds():
        q = lambda kind, col, rot, row=0: cols[col].values[(row + rot) % len(cols[col])]
        assert [t.evaluate(lambda kind, col, rot: q(kind, col, rot, 17)) for t in trees] == [0, 0, 0, 0]
    for tree in trees:
        assert any(r for k, _, r in X.encode_trace(tree.program()[0]) if k == "cap")  # a full-bound value is reduced on the way


# ---- products and sums: no zero denominator ---------------------------------------------------------------------------------------------
def _passed_over_are_zero(rnd, zero_factor):
    """every (beta, gamma) pair the round passed over does leave a zero factor, and the pair it took leaves none"""
    for beta, gamma, reason in rnd["passed"]:
        assert reason and zero_factor(beta, gamma) == reason, rnd["name"]


@pytest.mark.parametrize("sparse", [False, True])
def test_permutation_cases(sparse):
    rnds = X.perm_rounds(sparse)
    u = X.PRODUCT_U
    assert u == 2042 and u > 1024 and (X.PERM_M, X.PERM_CHUNK) == (4, 2)
    for j in range(X.PERM_M):
        assert _slot_ok([r["vals"][j] for r in rnds], "values")
        if not sparse:
            assert _slot_ok([r["sig"][j] for r in rnds], "values")
    tried = {"beta": set(), "gamma": set()}
    for r in rnds:
        v_, s_ = [v.values for v in r["vals"]], [s.values for s in r["sig"]]
        zf = lambda b, g: X.perm_zero_factor(v_, s_, u, b, g)
        assert zf(r["beta"], r["gamma"]) is None, r["name"]
        _passed_over_are_zero(r, zf)
        tried["beta"] |= {r["beta"]} | {b for b, _, _ in r["passed"]}
        tried["gamma"] |= {r["gamma"]} | {g for _, g, _ in r["passed"]}
        if sparse:
            active = r["active"]
            ident = X._identity(X.PRODUCT_K, X.PERM_M)
            moved = sorted({(j // 2) * u + i for j in range(4) for i in range(u) if s_[j][i] != ident[j][i]})
            assert set(moved) <= set(active) and len(active) <= 256 and len(active) * 8 <= 2 * u  # the wrapper's rule: k_perm_sparse_small
            assert {0, u - 1, u, 2 * u - 1} <= set(active)
    assert tried["beta"] == set(X.SCALARS) and tried["gamma"] == set(X.SCALARS)  # every scalar was taken or named as leaving a zero
    assert len({r["beta"] for r in rnds}) >= 6 and len({r["gamma"] for r in rnds}) >= 6


@pytest.mark.parametrize("sparse", [False, True])
def test_lookup_cases(sparse):
    rnds = X.lookup_rounds(sparse)
    for r in rnds:
        u = r["u"]
        zf = lambda b, g: X.lookup_zero_factor(r["a"].values, r["t"].values, r["ap"].values, r["sp"].values, u, b, g)
        assert zf(r["beta"], r["gamma"]) is None, r["name"]
        _passed_over_are_zero(r, zf)
        moving = sum(1 for i in range(u) if (r["a"].words[i], r["t"].words[i]) != (r["ap"].words[i], r["sp"].words[i]))
        if sparse:  # the library's rule for the sparse form: usable_rows >= 4096 and 4 m <= u
            assert u >= 4096 and 0 < 4 * moving <= u and moving >= X.SPARSE_LOOKUP_MOVING
        else:
            assert u == X.PRODUCT_U and (4 * moving > u or u < 4096)
    for part in ("a", "t", "ap", "sp"):
        assert _slot_ok([r[part] for r in rnds], "values") or (sparse and part in ("ap", "sp") and _covers([r[part] for r in rnds], "values"))
    assert len({r["beta"] for r in rnds}) >= 6 and len({r["gamma"] for r in rnds}) >= 6


def test_shuffle_and_logup_cases():
    u = X.PRODUCT_U
    rnds = X.shuffle_rounds()
    for r in rnds:
        assert all((r["a"].values[i] + r["gamma"]) % R and (r["s"].values[i] + r["gamma"]) % R for i in range(u)), r["name"]
        for _, gamma, reason in r["passed"]:
            assert reason and any((r["a"].values[i] + gamma) % R == 0 or (r["s"].values[i] + gamma) % R == 0 for i in range(u))
    assert _slot_ok([r["a"] for r in rnds], "values") and _slot_ok([r["s"] for r in rnds], "values") and len({r["gamma"] for r in rnds}) >= 6
    for n_sets in X.LOGUP_SETS:
        rnds = X.logup_rounds(n_sets)
        for r in rnds:
            cols = r["sets"] + [r["table"]]
            assert len(r["sets"]) == n_sets and all((c.values[i] + r["beta"]) % R for c in cols for i in range(u)), r["name"]
            for beta, _, reason in r["passed"]:
                assert reason and any((c.values[i] + beta) % R == 0 for c in cols for i in range(u))
        for slot in range(n_sets):
            assert _slot_ok([r["sets"][slot] for r in rnds], "values")
        assert _slot_ok([r["table"] for r in rnds], "values") and _slot_ok([r["mult"] for r in rnds], "values")
        assert len({r["beta"] for r in rnds}) >= 6


def test_pick_challenges_never_skips_silently():
    beta, gamma, passed = X.pick_challenges(0, lambda b, g: None)
    assert (beta, gamma, passed) == (X.scalar(0), X.scalar(3), [])
    beta, gamma, passed = X.pick_challenges(0, lambda b, g: "gamma is zero" if g == X.scalar(3) else None)
    assert (beta, gamma) == (X.scalar(0), X.scalar(4)) and passed == [(X.scalar(0), X.scalar(3), "gamma is zero")]
    with pytest.raises(X.ZeroDenominator):
        X.pick_challenges(0, lambda b, g: "always")


# ---- the references agree with each other -----------------------------------------------------------------------------------------------
def test_references_agree_on_a_standard_plonk_instance(custom):
    """batch_cases.batched_quotient (and the shuffle / logUp variants, which must reduce to it) against oracle/plonk.py's evaluate_h and
    divide_by_vanishing on a real StandardPlonk instance at k = 4"""
    from oracle import plonk as P

    inst = P.StandardPlonkInstance(4, 0xDEADBEEF)
    beta, gamma, y = X.scalar(2), X.scalar(5), X.scalar(6)
    zs = inst.permutation_products(beta, gamma)
    want = inst.divide_by_vanishing(inst.evaluate_h(zs, beta, gamma, y))
    ext = inst.to_extended
    ops, constants = X.compile_programs([X.standard_plonk_program(custom)])
    circuit = {"advice": [ext(c) for c in inst.advice], "fixed": [ext(c) for c in inst.fixed], "instance": None, "perm_zs": [ext(z) for z in zs], "lookups": []}
    circuit["perm_values"] = circuit["advice"]
    shared = {"perm_sigmas": [ext(c) for c in inst.sigma], "chunk": 1, "l0": ext(inst.l0), "l_last": ext(inst.l_last), "l_active": ext(inst.l_active)}
    d = inst.dom
    args = (4, d.extended_k, d.g_coset, d.extended_omega, P.FR_DELTA, P.BLINDING_FACTORS, ops, constants, [], [circuit], shared, beta, gamma, y)
    assert batch_cases.batched_quotient(*args) == want
    assert shuffle_cases.batched_quotient(*args) == want and logup_sets_cases.batched_quotient(*args) == want
    assert any(want) and len(want) == 32
