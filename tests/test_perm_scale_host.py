"""CPU tests of tests/perm_scale_cases.py: the inputs the GPU tests of the permutation grand products run on reach what their names
say — position counts, tiles, k_mulscan_offsets' run length, the form — and the two references agree with each other, checked with
Python integers and the C oracle's field operations alone, so that a GPU case cannot quietly exercise another path than the one it is
named for."""
import numpy as np
import pytest

import check_cases
import perm_scale_cases as cases

R = cases.R


@pytest.fixture(scope="module")
def custom(h2):
    from halo2_scaffold_amd import custom

    return custom


def _form(n_active, sets, u):
    """perm_products' branch behind the wrapper's rule (halo2_scaffold_amd/plonk.py permutation_products; the prover's is the same)"""
    if n_active is None or n_active * 8 > sets * u:
        return "dense"
    return "small" if n_active <= cases.SMALL_MAX else "general"


def test_sparse_cases_have_the_counts_and_positions_they_claim():
    k, u, m, chunk = (cases.SPARSE[key] for key in ("k", "u", "m", "chunk"))
    assert (k, u, m, chunk) == (13, 8186, 4, 2) and 2046 * 8 <= 2 * u < 2047 * 8
    counts = cases.SMALL_COUNTS + cases.GENERAL_COUNTS + (cases.FALLBACK_COUNT,)
    assert counts == (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2046, 2047)
    real_forms = set()
    for count in counts:
        name = f"sparse, n_active = {count}"
        case = cases.product_case(name)
        assert (case.k, case.u, case.m, case.chunk, case.sets, case.n) == (13, u, 4, 2, 2, 1 << 13), name
        active = case.active
        assert len(active) == count and active == sorted(set(active)) and 0 <= active[0] and active[-1] < 2 * u, name
        assert case.form == _form(count, 2, u), name
        assert case.form == ("small" if count <= 256 else "general" if count <= 2046 else "dense"), name
        # at a position of the list some column of the set is moved, off the list none: the list is exactly sigma's support
        assert cases.moved_positions(case) == active, name
        ident = cases.identity(k, m)
        assert all(case.sig[j][u:] != ident[j][u:] for j in range(m)), name  # the rows that are not read differ
        if count >= 63:
            rows = {0: set(), 1: set()}
            for p in active:
                rows[p // u].add(p % u)
            assert {0, u - 1} <= rows[0] and {0, u - 1} <= rows[1], name           # both ends of both sets
            assert {cases.ADJACENT_ROW, cases.ADJACENT_ROW + 1} <= rows[0], name      # two adjacent rows
            assert cases.ADJACENT_ROW in rows[1] and rows[0] & rows[1], name          # one row in both sets
            assert set(cases.pattern_positions(u, 2)) <= set(active), name
            kinds = set()
            for p in active:  # the first column alone, the second alone, both
                j0 = (p // u) * chunk
                kinds.add(tuple(case.sig[j][p % u] != ident[j][p % u] for j in (j0, j0 + 1)))
            assert kinds == ({(True, False), (False, True)} if case.real else {(True, False), (False, True), (True, True)}), name
        else:
            assert active == ([u - 1] if count == 1 else [u - 1, u]), name  # the last row of set 0 (and row 0 of set 1)
        if count >= 1025:  # positions on both sides of index 1024 of the list: the second tile of the scans is not empty
            assert active[1023] < active[1024] and len(active[1024:]) == count - 1024 >= 1, name
        total, tiles, per, used = cases.scan_shape(case)
        assert total == (2 * u if case.form == "dense" else count) and tiles == -(-total // 1024) and per == 1 and used == tiles, name
        launches = cases.expected_launches(case)
        if case.form == "general":
            assert launches["k_mulscan_offsets"] == (3 if count > 1024 else 0) and (tiles > 1) == (count > 1024), name
        want = cases.formula_products(k, u, chunk, case.vals, case.sig, case.beta, case.gamma, ident)  # raises on a zero denominator
        moves = [i for s in range(2) for i in range(u) if want[s][i + 1] != want[s][i]]
        assert len(moves) == count and want[1][0] == want[0][u], name
        assert all(z[u + 1 :] == [cases.SENTINEL] * (case.n - u - 1) for z in want), name
        assert (want[1][u] == 1) == case.real, name
        if case.real:
            real_forms.add(case.form)
    assert real_forms == {"small", "general", "dense"}  # one case per regime whose last product closes


def test_dense_cases_have_the_shapes_they_claim():
    seen = {}
    for name, spec in cases.PRODUCT_CASES.items():
        if spec["n_active"] is not None or spec.get("big"):
            continue
        case = cases.product_case(name)
        assert case.active is None and case.form == "dense" and 1 <= case.u < case.n and case.k <= 13, name
        want = cases.formula_products(case.k, case.u, case.chunk, case.vals, case.sig, case.beta, case.gamma)
        assert len(want) == case.sets and all(want[s + 1][0] == want[s][case.u] for s in range(case.sets - 1)), name
        moved = cases.moved_positions(case)
        assert 2 * len(moved) > case.sets * case.u or case.u == 1, name  # dense data: most positions move
        assert (want[-1][case.u] == 1) == case.real, name
        assert cases.recurrence_violation(case, [cases.mont_limbs(z) for z in want]) is None, name  # the two references agree
        seen[name] = (case.k, case.m, case.chunk, case.u, case.sets) + cases.scan_shape(case)[1:2]
    assert seen == {
        "dense, 64 columns (k = 6)": (6, 64, 7, 58, 10, 1),  # the column maximum; ten sets, the last with one column (64 = 9 * 7 + 1)
        "dense, one set (k = 11)": (11, 3, 5, 2042, 1, 2),   # chunk >= m
        "dense, usable_rows = 1 (k = 1)": (1, 2, 1, 1, 2, 1),
        "dense, usable_rows = 1 (k = 6)": (6, 3, 2, 1, 2, 1),
        "dense, usable_rows = 2^k - 1 (k = 10)": (10, 3, 2, 1023, 2, 2),
    }
    one = cases.single_set_case()
    assert (one.k, one.u, one.m, one.chunk, one.sets) == (11, 1025, 3, 2, 2) and one.u > cases.MS_TILE  # rows on both sides of a tile


def test_the_big_case_runs_k_mulscan_offsets_with_runs_of_two():
    name = "dense, more than 1024 tiles (k = 18)"
    case = cases.product_case(name)
    assert case.big and (case.k, case.m, case.chunk, case.sets, case.u) == (18, 5, 1, 5, 261939) and case.u < case.n
    total, tiles, per, used = cases.scan_shape(case)
    assert total == 1309695 > 1 << 20 and tiles == 1279 and tiles % 2 == 1 and total % 1024 == 1023  # a partial last tile
    assert per == 2 and used == 640 and (used - 1) * per == tiles - 1  # the last owning thread has a single tile
    assert cases.expected_launches(case) == {"k_perm_to_mont256": 0, "k_mulscan_offsets": 3, "k_perm_numden_sets": 1}
    fac = cases.factors(case)
    assert cases.zero_denominators(case, fac) == 0
    ident = cases.identity_limbs(case.k, case.m)
    for j in range(case.m):  # three cells of four moved, the others on the identity: ratios of exactly one between the others
        same = (case.sig[j][: case.u] == ident[j][: case.u]).all(axis=1)
        assert 0.2 * case.u < same.sum() < 0.3 * case.u, j
        assert np.array_equal((fac[j][0] == fac[j][1]).all(axis=1), same), j  # chunks of one: set j is column j
    w, d = cases.o.omega_for(case.k), cases.FR_DELTA
    for j, i in ((0, 0), (0, 1), (1, 2), (4, 12345), (3, case.n - 1)):  # the doubled power table against pow()
        assert cases.from_mont_limbs(ident[j][i]) == [pow(d, j, R) * pow(w, i, R) % R]


def test_recurrence_checker_accepts_the_formula_and_rejects_planted_errors():
    """at a small size (two sets over two tiles each): a column built row by row passes; one perturbed row in the last tile, a set
    that starts from another value, a first row other than one and a value at or above the modulus do not"""
    case = cases.product_case("small recurrence case", dict(k=11, m=2, chunk=1, u=cases.usable(11), n_active=None, form="dense", real=False))
    u = case.u
    fac = cases.factors(case)
    want = cases.formula_products(case.k, u, case.chunk, case.vals, case.sig, case.beta, case.gamma)
    good = [cases.mont_limbs(z[: u + 1]) for z in want]
    assert cases.recurrence_violation(case, good, fac) is None
    plant = lambda s, row, v: [np.concatenate([z[:row], cases.mont_limbs([v]), z[row + 1 :]]) if t == s else z for t, z in enumerate(good)]
    row = u - 5  # in the last tile of the concatenated rows
    assert (case.sets * u - 1) // 1024 == (u + row - 1) // 1024
    bad = cases.recurrence_violation(case, plant(1, row, (want[1][row] + 1) % R), fac)
    assert bad == f"set 1: 2 rows do not follow from the row before, the first is row {row}"
    assert cases.recurrence_violation(case, plant(1, u, (want[1][u] + 1) % R), fac).startswith("set 1: 1 rows do not follow")
    # a set that starts from the wrong value and goes on correctly from there: every later row is wrong by the same factor, the
    # recurrence inside the set holds
    scaled = [good[0], cases.mont_limbs([v * 2 % R for v in want[1][: u + 1]])]
    assert cases.recurrence_violation(case, scaled, fac) == f"set 1: row 0 is not row {u} of set 0"
    scaled0 = [cases.mont_limbs([v * 3 % R for v in want[s][: u + 1]]) for s in range(2)]
    assert cases.recurrence_violation(case, scaled0, fac) == "set 0: row 0 is not one"
    above = [z.copy() for z in good]
    above[0][7] = np.frombuffer((int.from_bytes(above[0][7].tobytes(), "little") + R).to_bytes(32, "little"), dtype=np.uint64)
    assert cases.recurrence_violation(case, above, fac) == "set 0: a value at or above the modulus"
    # and a denominator of zero is refused: sigma chosen so that v + beta sigma + gamma = 0 on one row
    case.sig[1][9] = -(case.vals[1][9] + case.gamma) * pow(case.beta, -1, R) % R
    assert cases.zero_denominators(case) == 1
    with pytest.raises(AssertionError):
        cases.recurrence_violation(case, good)


def test_proof_cases_take_the_forms_they_are_named_for(custom):
    """the position counts keygen will compute for check_cases.copies_circuit, from the assignment's copy cycles by the rule of
    plonk.ActiveRows, pinned; and each side of the prover's rule n_active * 8 <= n_sets * usable_rows"""
    forms = {}
    for (k, cycles), (n_active, form) in cases.PROOF_CASES.items():
        cs, asg, _ = check_cases.copies_circuit(custom, k, cycles)
        pos, u, sets, chunk = cases.proof_positions(cs, asg, k)
        assert (u, sets, chunk, len(cs.perm_columns)) == ((1 << k) - 6, 4, 1, 4), (k, cycles)
        assert len(pos) == n_active == 3 * cycles + (cycles + 2) // 4 + 8, (k, cycles)
        assert form == _form(n_active, sets, u), (k, cycles)
        assert {p // u for p in pos} == {0, 1, 2, 3}, (k, cycles)  # advice a, advice b, the fixed column, the instance column
        forms[(k, cycles)] = (n_active, form, -(-n_active // 1024))
    assert forms == {(11, 60): (203, "small", 1), (11, 82): (275, "general", 1), (11, 311): (1019, "general", 1), (11, 312): (1022, "dense", 1),
                     (13, 700): (2283, "general", 3)}
    u11 = (1 << 11) - 6
    assert 1019 * 8 <= 4 * u11 < 1022 * 8 and (4 * u11) // 8 == 1021  # 311 cycles: the last count under the rule; 312: the first over it
