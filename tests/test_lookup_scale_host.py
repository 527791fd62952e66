"""CPU tests of tests/lookup_scale_cases.py: the inputs the GPU tests of the lookup kernels run on reach what their names say — checked
with oracle/lookup.py and Python integers alone, so that a GPU case cannot quietly exercise another path than the one it is named for."""
import collections

import pytest

import lookup_scale_cases as cases
from oracle import lookup as L

R = cases.R
BETA, GAMMA = 0x1234567, 0x7654321


def _closes(inputs, table, a_perm, s_perm, u, beta, gamma):
    """z_u == 1 without a field inversion per row: the numerators' product equals the denominators', no denominator factor is zero"""
    num = den = 1
    for i in range(u):
        assert (a_perm[i] + beta) % R and (s_perm[i] + gamma) % R
        num = num * (inputs[i] + beta) % R * (table[i] + gamma) % R
        den = den * (a_perm[i] + beta) % R * (s_perm[i] + gamma) % R
    return num == den


def _check_permutation(case):
    u = case.u
    a_perm, s_perm = L.permute_expression_pair(case.inputs, case.table, u, case.keep_a, case.keep_s)  # raises if an input is in no table row
    assert len(a_perm) == len(s_perm) == case.n and a_perm[u:] == case.keep_a and s_perm[u:] == case.keep_s
    assert _closes(case.inputs, case.table, a_perm, s_perm, u, BETA, GAMMA)
    return a_perm, s_perm


@pytest.mark.parametrize("k", cases.KS)
def test_permute_cases_reach_what_they_are_named_for(k):
    u = cases.usable(k)
    blocks = -(-u // cases.RANK_BLOCK)
    assert blocks >= 2 and (u > 8192) == (k == 14) and u % 4 == 2
    seen = set()
    for kk, table_kind, input_kind in cases.PERMUTE_CASES:
        if kk != k:
            continue
        seen.add((table_kind, input_kind))
        case = cases.permute_case(k, table_kind, input_kind)
        what = f"{table_kind} / {input_kind}"
        ordered = cases.distinct_sorted(case.table, u)
        rank = {v: r for r, v in enumerate(ordered)}
        a_perm, s_perm = _check_permutation(case)
        # the tables
        if table_kind in cases.DISTINCT_TABLES:
            assert len(ordered) == u, what
        if table_kind == "repeats":
            tally = collections.Counter(case.table[:u])
            assert len(ordered) == u // 2 and sum(c > 1 for c in tally.values()) == 5 and max(tally.values()) > 100, what
        if table_kind == "low word":
            low = [v & 0xFFFFFFFF for v in ordered]
            assert all(w < len(ordered) for w in low), what
            assert 2 * sum(w != r for r, w in enumerate(low)) > len(ordered), what
            assert all(ordered[w] >> 32 != v >> 32 for v, w in zip(ordered, low) if rank[v] != w), what  # sorted[guess] differs above word 0
        if table_kind == "range":
            assert ordered == list(range(1 << (k - 2))) and case.table[:u].count(0) == u - len(ordered) + 1, what
        # the inputs
        distinct_inputs = set(case.inputs[:u])
        if input_kind == "uniform":
            assert len(distinct_inputs) > min(len(ordered), u) // 3, what
        if input_kind == "skewed":
            assert 0.85 * u < max(collections.Counter(case.inputs[:u]).values()) < 0.95 * u and len(distinct_inputs) > 20, what
        if input_kind == "rank 5 mod 64":
            assert all(rank[v] % cases.RANK_SLOTS == cases.COLLIDING_SLOT for v in case.inputs[:u]), what
            for b in range(blocks):
                rows = case.inputs[b * cases.RANK_BLOCK : min(u, (b + 1) * cases.RANK_BLOCK)]
                assert len({rank[v] for v in rows}) >= 8, (what, b)
        if input_kind == "ends":
            assert distinct_inputs == {ordered[0], ordered[-1]}, what
        if input_kind == "permutation":
            assert sorted(case.inputs[:u]) == ordered and a_perm[:u] == s_perm[:u], what
        else:
            assert a_perm[:u] != s_perm[:u], what  # repeated rows: the table's leftovers enter S'
        # the three absent values and where they go
        assert case.absent_rows == (0, 1024, u - 1) and len(set(case.absent.values())) == 3, what
        assert all(0 <= v < R and v not in rank for v in case.absent.values()), what
        if table_kind == "range":  # starts at zero, no gap between neighbours: nothing below, nothing between
            assert all(v > ordered[-1] for v in case.absent.values()), what
        else:
            below, above, between = case.absent["below"], case.absent["above"], case.absent["between"]
            assert below < ordered[0] and above > ordered[-1] and ordered[0] < between < ordered[-1], what
        assert [r for r in range(case.n) if case.bad_inputs[r] != case.inputs[r]] == list(case.absent_rows), what
        with pytest.raises(ValueError, match="not in the table"):
            L.permute_expression_pair(case.bad_inputs, case.table, u, case.keep_a, case.keep_s)
    assert seen == {(t, i) for t in cases.TABLES for i in cases.INPUTS if i != "permutation" or t in cases.DISTINCT_TABLES} and len(seen) == 18


def test_usable_rows_cases_take_every_residue():
    assert {u % 4 for k, u in cases.USABLE_ROWS if k == 11} == {0, 1, 2, 3}
    assert {u for _, u in cases.USABLE_ROWS} >= {1023, 1024, 1025, 8191, 8192, 8193, cases.usable(11), cases.usable(14)}
    residues = set()
    for index, (k, u) in enumerate(cases.USABLE_ROWS):
        case = cases.usable_case(index)
        assert (case.k, case.u, case.n) == (k, u, 1 << k) and u < case.n
        n_unique = len(cases.distinct_sorted(case.table, u))
        assert n_unique == cases.usable_case_distinct(index) and n_unique % 4 == index % 4 and u // 2 < n_unique < u
        residues.add(n_unique % 4)
        a_perm, s_perm = _check_permutation(case)
        assert a_perm[:u] != s_perm[:u]
    assert residues == {0, 1, 2, 3}
    assert any(len(cases.distinct_sorted(cases.usable_case(i).table, u)) > cases.SEGMENT for i, (_, u) in enumerate(cases.USABLE_ROWS))


def test_product_cases_flag_the_rows_they_claim():
    forms = set()
    for name, (k, u, m, form) in cases.PRODUCT_CASES.items():
        case = cases.product_case(name)
        assert (case.k, case.u, case.m, case.n) == (k, u, m, 1 << k) and u < case.n, name
        flagged = [i for i in range(u) if (case.inputs[i], case.table[i]) != (case.pin[i], case.ptab[i])]
        assert flagged == case.rows and len(flagged) == m, name
        kinds = {(case.inputs[i] != case.pin[i], case.table[i] != case.ptab[i]) for i in flagged}
        assert kinds == ({(True, False), (False, True), (True, True)} if m >= 3 else {(True, False)} if m else set()), name
        assert all((case.pin[i] + case.beta) % R and (case.ptab[i] + case.gamma) % R for i in range(u)), name  # no zero denominator
        assert all(case.inputs[i] != case.pin[i] and case.table[i] != case.ptab[i] for i in range(u, case.n)), name
        # the rule of h2mi_plonk_lookup_product_dev: flags from 4096 usable rows on, sparse when at most a quarter are flagged
        assert form == ("sparse" if u >= 4096 and 4 * m <= u else "dense"), name
        forms.add((form, k))
    assert forms >= {("dense", 11), ("dense", 12), ("dense", 13), ("sparse", 13), ("sparse", 14)}
    by = {name: cases.PRODUCT_CASES[name] for name in cases.PRODUCT_CASES}
    u13 = cases.usable(13)
    assert by["threshold: a quarter of the rows"][2] == u13 // 4 and by["threshold: a quarter of the rows plus one"][2] == u13 // 4 + 1
    assert 4 * (u13 // 4) <= u13 < 4 * (u13 // 4 + 1)
    assert {m for _, (k, u, m, f) in by.items() if f == "sparse" and k == 13 and u == u13} >= {0, 1, 1023, 1024, 1025}
    assert cases.usable(12) < 4096 and cases.usable(12) % 1024 and cases.usable(11) > 1024
    seg = cases.product_case("sparse, two scan segments (k = 14)")
    assert seg.rows[0] == 0 and seg.rows[-1] == seg.u - 1 and sum(r > cases.SEGMENT for r in seg.rows) >= 1025 and seg.m == 3000
