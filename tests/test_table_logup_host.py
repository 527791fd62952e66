"""LogUp against a table sorted at keygen, on the host: the Python-integer references of tests/table_logup_cases.py against the argument
as tests/logup_sets_cases.py states it, every named input of the kernel tests checked to reach what it is named for, and the refusals of
h2mi_table_logup_check / h2mi_prover_keygen with H2MI_KEYGEN_LOGUP on a hard-wired shape, which are decided before any device work (no GPU here)."""
import random

import pytest

import keygen_call
import logup_sets_cases as sets_cases
import table_logup_cases as cases
from oracle import bn254 as o

R = o.R
EINVAL, ENODEV = -1, -2


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("K", [1, 2, 6])
def test_references_are_the_arguments_numbers(kind, K):
    """ranks, histogram, M and the sum by rank against multiplicities / running_sum of the several-sets argument"""
    k, u = cases.SIZES[0]
    rng = random.Random(500 + K + len(kind))
    cols, table = cases.kernel_input(kind, K, u, rng)
    values, first = cases.table_data(table, u)
    assert values == sorted(set(table[:u])) and all(table[f] == v and v not in table[:f] for v, f in zip(values, first))
    ranks, counts, absent = cases.rank_columns(cols, values, u)
    assert all(r is None or values[r] == cols[j][i] for j in range(K) for i, r in enumerate(ranks[j]))
    m = cases.m_column(counts, first, u)
    want_m, want_absent = sets_cases.multiplicities(cols, table, u)
    assert m == want_m and sorted(absent) == sorted(want_absent) and sum(counts) == K * u - len(absent)
    if not absent:
        beta = rng.randrange(R)
        phi = cases.ranked_sum(ranks, values, counts, first, beta, u)
        assert phi == sets_cases.running_sum(cols, table, m, beta, u) and phi[0] == 0 and phi[u] == 0


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("K", [1, 2, 6])
@pytest.mark.parametrize("k,u", cases.SIZES)
def test_named_inputs_reach_what_they_are_named_for(k, u, K, kind):
    cols, table = cases.kernel_input(kind, K, u, random.Random(77000 + 13 * u + 101 * K + len(kind)))  # the GPU test's seeds
    assert len(cols) == K and all(len(c) == u for c in cols) and len(table) == u and u < (1 << k) and u % 64
    assert cases.reaches(kind, cols, table, u)
    assert (u > cases.RANK_WORKGROUP) == (k > 10)  # one workgroup at k = 10, two at 11 with a ragged last wavefront, eight at 13


# ---- the grouping's rules -------------------------------------------------------------------------------------------------------------
def _abi(h2, num_lookup_advice=4, degree=None, runs=None):
    from halo2_scaffold_amd import engine, flex

    cs = flex.FlexGateCS(True, 3, num_lookup_advice, k=7)
    if runs is not None:
        cs.use_logup(runs)
    abi = cs.abi(7)
    if degree is not None:
        abi.degree = degree
    return engine, abi


def test_check_accepts_and_reports_the_degree(h2):
    engine, abi = _abi(h2)
    assert engine.table_logup_check(abi) == 4  # 2 + 1 + 1: one column per argument
    for runs, degree in (([1, 1, 1, 1], 4), ([2, 2], 5), ([3, 1], 6), ([4], 7)):
        engine, abi = _abi(h2, runs=runs)
        assert abi.degree == degree and engine.LogupInputs.build(runs).check_table(abi) == degree
    engine, abi = _abi(h2, 8, runs=[6, 2])
    assert abi.degree == 9 and engine.LogupInputs.build([6, 2]).check_table(abi) == 9
    from halo2_scaffold_amd import flex

    one = flex.FlexGateCS(lookup=True)  # q_lookup * a: an input of degree 2
    assert one.use_logup() == [1] and one.degree == 5 and engine.table_logup_check(one.abi(7)) == 5


def test_flex_degree_is_untouched_without_logup(h2):
    from halo2_scaffold_amd import flex

    assert flex.FlexGateCS(lookup=True).degree == 5 and flex.FlexGateCS(True, 3, 4, k=7).degree == 4 and flex.FlexGateCS(False, 3, 0, k=7).degree == 3
    cs = flex.FlexGateCS(True, 11, 8, k=7)
    assert cs.use_logup(4) == [4, 4] and cs.degree == 7 and cs.chunk == 5
    assert cs.use_logup(3) == [3, 3, 2] and cs.use_logup(6) == [6, 2] and cs.degree == 9
    for bad in (0, 7, [4, 3], [8], [0, 8]):
        with pytest.raises(ValueError):
            cs.use_logup(bad)
    with pytest.raises(ValueError, match="no lookup"):
        flex.FlexGateCS(False, 3, 0, k=7).use_logup()


def _refused(engine, abi, counts):
    with pytest.raises(engine.H2miError) as e:
        engine.table_logup_check(abi, engine.LogupInputs.build(counts) if counts is not None else None)
    return e.value.code == EINVAL


def test_check_refusals(h2):
    engine, abi = _abi(h2, degree=9)
    # counts that do not sum to n_lookups: the struct has no length of its own, so an argument that would pass the last entry is the violation
    assert _refused(engine, abi, [2, 3]) and _refused(engine, abi, [3, 2]) and _refused(engine, abi, [5]) and _refused(engine, abi, [1, 1, 1, 2])
    assert _refused(engine, abi, [0, 4]) and _refused(engine, abi, [2, 0, 2])  # a count of 0
    engine, abi8 = _abi(h2, 8, degree=9)
    assert _refused(engine, abi8, [7, 1])  # a count of 7
    assert engine.table_logup_check(abi8, engine.LogupInputs.build([6, 2])) == 9
    # mixed tables in one argument; the same entries apart are fine
    engine, mixed = _abi(h2, degree=9)
    mixed.lookups[1].table_fixed = 1
    assert _refused(engine, mixed, [2, 2]) and _refused(engine, mixed, [4])
    assert engine.table_logup_check(mixed, engine.LogupInputs.build([1, 1, 2])) == 5
    # a degree one too low
    for runs, need in (([1, 1, 1, 1], 4), ([2, 2], 5), ([4], 7)):
        engine, low = _abi(h2, degree=need - 1)
        assert _refused(engine, low, runs)
        engine, enough = _abi(h2, degree=need)
        assert engine.table_logup_check(enough, engine.LogupInputs.build(runs)) == need
    from halo2_scaffold_amd import flex

    one = flex.FlexGateCS(lookup=True).abi(7)
    one.degree = 4
    assert _refused(engine, one, None)
    # gates given as expressions; no lookups; a merged argument whose column another one reads already
    engine, exprs = _abi(h2, degree=9)
    exprs.gates = engine.GATES_EXPRESSIONS
    assert _refused(engine, exprs, None)
    engine, none = _abi(h2, degree=9)
    none.n_lookups = 0
    assert _refused(engine, none, None)
    engine, twice = _abi(h2, degree=9)
    twice.lookups[3].input.index = twice.lookups[0].input.index
    assert _refused(engine, twice, [2, 2]) and engine.table_logup_check(twice, engine.LogupInputs.build([2, 1, 1])) == 5


def test_keygen_refuses_on_the_host(h2):
    """every violation is H2MI_EINVAL before any device work: there is no device here, and none is asked for"""
    from halo2_scaffold_amd import engine

    def keygen(abi, counts, flags):
        cells, keep = engine.pack_cells([{} for _ in range(abi.n_fixed)])
        li = engine.LogupInputs.build(counts) if counts is not None else None
        rc, _ = keygen_call.keygen(abi, inputs=li, fixed=cells, flags=flags | engine.KEYGEN_LOGUP)
        del keep
        return rc

    engine, abi = _abi(h2, degree=9)
    for flags in (engine.KEYGEN_BY_COSET, 4, 16, engine.KEYGEN_LOGUP | engine.KEYGEN_BY_COSET, 1 << 31):
        assert keygen(abi, [2, 2], flags) == EINVAL
    for counts in ([3, 2], [0, 4], [7], [5]):
        assert keygen(abi, counts, 0) == EINVAL and keygen(abi, counts, engine.KEYGEN_LOGUP) == EINVAL
    engine, low = _abi(h2, degree=4)
    assert keygen(low, [2, 2], 0) == EINVAL
    engine, mixed = _abi(h2, degree=9)
    mixed.lookups[1].table_fixed = 1
    assert keygen(mixed, [2, 2], 0) == EINVAL
    engine, exprs = _abi(h2, degree=9)
    exprs.gates = engine.GATES_EXPRESSIONS
    assert keygen(exprs, None, 0) == EINVAL
    engine, none = _abi(h2, degree=9)
    none.n_lookups = 0
    assert keygen(none, None, 0) == EINVAL
    # the flag is what selects the argument: a grouping without it is refused, the same record with it passes every host rule (and finds
    # no device here)
    cells, keep = engine.pack_cells([{} for _ in range(abi.n_fixed)])
    li = engine.LogupInputs.build([2, 2])
    assert keygen_call.keygen(abi, inputs=li, fixed=cells) == (EINVAL, None)
    assert keygen_call.keygen(abi, inputs=li, fixed=cells, flags=engine.KEYGEN_LOGUP) == (ENODEV, None)
    assert keygen_call.keygen(abi, fixed=cells, flags=4, pk=0)[0] == EINVAL
    del keep


def test_scaffold_refuses_a_key_file_with_logup(h2, tmp_path):
    from halo2_scaffold_amd import scaffold

    with pytest.raises(ValueError, match="key_file with logup=True: the key-file format has no section"):
        scaffold.gen_key(lambda *a: None, None, key_file=str(tmp_path / "range.pk"), logup=True)
    assert not (tmp_path / "range.pk").exists()
