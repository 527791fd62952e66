"""CPU tests of tests/tile_regime_cases.py: every named size reaches the regime of the one-workgroup tile-offset passes it is named for
(a size moved across a boundary fails here), and the generator's vector references — numpy limb arrays through the C oracle — agree
with the existing Python-integer references on two-tile inputs, so that the million-row GPU cases are checked against the same
statements as the small ones."""
import collections

import numpy as np
import pytest

import extreme_cases
import key_file_cases as K
import logup_sets_cases
import table_logup_cases
import tile_regime_cases as cases
from oracle import bn254 as o

R = o.R
TWO_TILES = 2 * cases.TILE - 7  # two tiles, the last ragged


def test_the_constants_and_the_run_rule():
    assert (cases.TILE, cases.THREADS, cases.LANES, cases.CELL_ROUND) == (1024, 1024, 64, 256)
    assert [cases.regime(t) for t in (1, 64, 65, 1024, 1025)] == ["A", "A", "B", "B", "C"]
    for tiles in (1, 64, 65, 1024):
        assert cases.middle_pass(tiles) == (1, tiles, 1)
    assert cases.middle_pass(1025) == (2, 513, 1) and cases.middle_pass(1026) == (2, 513, 2) and cases.middle_pass(2048) == (2, 1024, 2)
    assert cases.middle_pass(2049) == (3, 683, 3) and cases.middle_pass(1279) == (2, 640, 1) and cases.middle_pass(4096) == (4, 1024, 4)
    for tiles in range(1, 5000, 7):  # every tile has one owner: full runs, then one run of 1 .. per tiles
        per, used, last = cases.middle_pass(tiles)
        assert used <= cases.THREADS and 1 <= last <= per and (used - 1) * per + last == tiles


def test_every_named_size_reaches_what_its_name_says():
    sizes = cases.SIZES
    assert sizes == {"B-min": 65537, "B-full": (1 << 20) - 6, "C-short": 1048577, "C-even": 1026 * 1024 - 3}
    shape = lambda name: (cases.tiles_of(sizes[name]), cases.regime(cases.tiles_of(sizes[name])), *cases.middle_pass(cases.tiles_of(sizes[name])))
    last_tile = lambda name: sizes[name] - (cases.tiles_of(sizes[name]) - 1) * cases.TILE
    # B-min: the first tile count whose owners leave wavefront 0, the last tile of one element
    assert shape("B-min") == (65, "B", 1, 65, 1) and last_tile("B-min") == 1 and cases.regime(cases.tiles_of(sizes["B-min"] - 1)) == "A"
    # B-full: every thread owns exactly one tile
    assert shape("B-full") == (1024, "B", 1, 1024, 1) and cases.regime(cases.tiles_of(sizes["B-full"]) + 1) == "C"
    # C-short: runs of two, the last run one tile of one element
    assert shape("C-short") == (1025, "C", 2, 513, 1) and last_tile("C-short") == 1 and cases.regime(cases.tiles_of(sizes["C-short"] - 1)) == "B"
    # C-even: runs of two, all full, a ragged last tile
    assert shape("C-even") == (1026, "C", 2, 513, 2) and 1 < last_tile("C-even") < cases.TILE
    assert {name: cases.smallest_k(u) for name, u in sizes.items()} == {"B-min": 17, "B-full": 20, "C-short": 21, "C-even": 21}
    for name, u in sizes.items():
        k = cases.smallest_k(u)
        assert (1 << (k - 1)) - 6 < u <= (1 << k) - 6, name
    # the table of the ranked sum: more than one tile of k_assigned_tile_inverses, no multiple of 4; and once as many values as rows
    assert cases.tiles_of(cases.TABLE_VALUES) == 5 and cases.TABLE_VALUES % 4 == 3
    assert cases.regime(cases.tiles_of(sizes["B-min"])) == "B"  # n_unique = u at B-min: 65 tiles of distinct values
    # a whole proof at k = 17: 128 tiles in the running sum and in the divisions
    assert cases.regime(cases.tiles_of((1 << 17) - 6)) == "B" and cases.regime(cases.tiles_of(1 << 17)) == "B"
    assert cases.regime(cases.tiles_of((1 << 16) - 6)) == "A"


def test_the_cell_columns_reach_the_rounds_they_are_named_for():
    assert cases.CELL_TILES == (257, 512, 513)
    assert [cases.cell_rounds(t) for t in (256, 257, 512, 513)] == [(1, 256), (2, 1), (2, 256), (3, 1)]
    assert cases.cell_rounds(8) == (1, 8)  # k = 13: what the suite ran before
    for tiles in cases.CELL_TILES:
        limit = cases.cells_limit(tiles)
        assert cases.tiles_of(limit) == tiles and limit == tiles * 1024 - 6
        pats = cases.cell_patterns(tiles)
        ends = cases.tile_end_rows(tiles)
        want_tiles = sorted({t for t in (0, 255, 256, 257, tiles - 1) if t < tiles})
        assert sorted({r // 1024 for r in ends}) == want_tiles and ends[0] == 0 and ends[-1] == limit - 1
        assert all(r % 1024 in (0, 1023) or r == limit - 1 for r in ends) and {r % 1024 for r in ends} >= {0, 1023}
        ex = {name: K.expect(col, limit) for name, col in pats.items()}
        assert ex["tile_ends"][3:5] == (K.SPARSE, 8) and ex["tile_ends_wide"][2:5] == (0, K.SPARSE, 32)
        assert K.expect(pats["tile_ends"], limit, 4)[3:5] == (K.SPARSE, 32)  # both widths of the same cells
        assert ex["every_37th_tile"][0] == -(-tiles // 37) and ex["every_37th_tile"][3:5] == (K.SPARSE, 8)
        assert ex["dense_small"][1] == limit and ex["dense_small"][3:5] == (K.DENSE, 8) and ex["dense_small"][0] < limit
        wide = pats["wide_in_the_last_tile"]
        assert ex["wide_in_the_last_tile"][2:5] == (0, K.SPARSE, 32) and sum(not K.fits64(v) for v in wide.values()) == 1
        assert next(r for r, v in wide.items() if not K.fits64(v)) // 1024 == tiles - 1
        # cells in the tiles of every round, so a lost carry shifts an offset
        assert {r // 1024 // cases.CELL_ROUND for r in ends} == set(range(cases.cell_rounds(tiles)[0]))


def test_dense_small_is_the_dict_it_stands_for():
    """DenseSmall's words and expectation against key_file_cases.column_stats / expect of the same cells, on two tiles"""
    n_rows, limit = 2 * 1024, 2 * 1024 - 6
    ints = (np.arange(limit, dtype=np.uint64) * np.uint64(977)) % np.uint64(1 << 20)
    ints[::5] = 0
    ints[limit - 1] = 7
    for col in (cases.DenseSmall(ints), cases.DenseSmall(np.where(np.arange(limit) % 9 == 0, ints, 0))):  # dense, and a sparse one
        cells = col.cells()
        rows, count, last, fits = K.column_stats(cells, limit)
        got = col.expect(limit)
        assert got == K.expect(cells, limit) and got[:3] == (count, last, int(fits)) and count and fits
        assert np.array_equal(col.limbs(n_rows), K.column_limbs(cells, n_rows))
        assert o.unpack(col.limbs(n_rows), R) == [cells.get(r, 0) for r in range(n_rows)]
    assert cases.DenseSmall(ints).expect(limit)[3] == K.DENSE and cases.DenseSmall(np.where(np.arange(limit) % 9 == 0, ints, 0)).expect(limit)[3] == K.SPARSE


def test_the_limb_helpers_are_the_integer_conversions():
    vals = [0, 1, 5, (1 << 64) - 1]
    assert o.unpack(cases.to_mont(cases.small_raw(vals)), R) == vals
    mont = o.pack([0, 1, R - 1, 12345678901234567890123], R)
    assert o.unpack(cases.from_mont(mont)) == [0, 1, R - 1, 12345678901234567890123]
    assert o.unpack(cases.mont_of(R - 2).reshape(1, 4), R) == [R - 2]
    assert o.unpack(cases.extreme_words("all r - 1", 3)) == [R - 1] * 3
    assert set(o.unpack(cases.extreme_words("random choice", 500))) == set(extreme_cases.EXTREME_WORDS)


def _ints(limbs):
    return o.unpack(limbs, R)


@pytest.mark.parametrize("K_sets,absent", [(1, False), (2, False), (6, False), (6, True)])
def test_running_sum_references_agree_on_two_tiles(K_sets, absent):
    """the case's M, fraction and ranking against logup_sets_cases.multiplicities / running_sum / fraction and
    table_logup_cases.table_data / rank_columns / m_column / ranked_sum; the recurrence accepts the Python-integer sum and rejects a
    sum with one wrong row"""
    u = TWO_TILES
    c = cases.sum_case("two tiles", K_sets, n_unique=300, absent=absent, u=u)
    assert (c.k, c.n) == (11, 2048) and c.u == u
    cols, table = [_ints(col) for col in c.cols], _ints(c.table)
    m, missing = logup_sets_cases.multiplicities([col[:u] for col in cols], table, u)
    assert m == c.m.tolist() == _ints(c.m_col[:u]) and missing == c.absent and len(missing) == int(absent)
    assert collections.Counter(v for col in cols for v in col[:u] if v in set(table[:u])) == collections.Counter(
        {table[r]: m[r] for r in range(u) if m[r]})
    assert any(_ints(col[u:]) != [0] * (c.n - u) for col in c.cols) and _ints(c.m_col[u:]) != [0] * (c.n - u)
    # the fraction, row by row
    num, den = cases.fraction_limbs(c.cols, c.table, c.m_col, c.beta, u, absent=c.absent)
    want = [logup_sets_cases.fraction([col[i] for j, col in enumerate(cols) if (i, j) not in c.absent], table[i], m[i], c.beta) for i in range(u)]
    assert list(zip(_ints(num), _ints(den))) == want
    # the recurrence is the running sum
    present = [[None if (i, j) in c.absent else col[i] for i in range(u)] for j, col in enumerate(cols)]
    phi = [0]
    for i in range(u):
        step = sum(pow((col[i] + c.beta) % R, -1, R) for col in present if col[i] is not None) - m[i] * pow((table[i] + c.beta) % R, -1, R)
        phi.append((phi[-1] + step) % R)
    if not absent:
        assert phi == logup_sets_cases.running_sum([col[:u] for col in cols], table, m, c.beta, u)
    assert phi[u] == 0 and len(set(phi)) > u // 2
    assert cases.sum_violation(o.pack(phi, R), num, den, u) is None
    for row in (1, 1024, 1025, u):
        wrong = list(phi)
        wrong[row] = (wrong[row] + 1) % R
        assert "rows do not follow" in cases.sum_violation(o.pack(wrong, R), num, den, u)
    shifted = o.pack([(v + 1) % R for v in phi], R)
    assert cases.sum_violation(shifted, num, den, u) == "row 0 is not zero"
    over = o.pack(phi, R)
    over[5] = o.int_to_limbs(R)
    assert cases.sum_violation(over, num, den, u) == "a value at or above the modulus"
    # a bumped multiplicity: the sum of the recurrence no longer closes
    m_bumped, num_bumped = cases.bumped(c, num)
    assert _ints(m_bumped[:u]) == [m[0] + 1] + m[1:] and np.array_equal(m_bumped[u:], c.m_col[u:])
    assert np.array_equal(num_bumped, cases.fraction_limbs(c.cols, c.table, m_bumped, c.beta, u, absent=c.absent)[0])
    phi_bumped = [(v - pow((table[0] + c.beta) % R, -1, R)) % R if i else 0 for i, v in enumerate(phi)]  # row 0 subtracts one M / s more
    assert phi_bumped[u] != 0 and cases.sum_violation(o.pack(phi_bumped, R), num_bumped, den, u) is None
    assert "rows do not follow" in cases.sum_violation(o.pack(phi, R), num_bumped, den, u)
    # the ranking against the key's view in Python integers
    rk = cases.ranked(c)
    values, first = table_logup_cases.table_data(table, u)
    ranks, counts, absent_pairs = table_logup_cases.rank_columns([col[:u] for col in cols], values, u)
    assert o.unpack(rk.sorted) == values and rk.first.tolist() == first and rk.counts.tolist() == counts and absent_pairs == c.absent
    assert [[None if r < 0 else r for r in col.tolist()] for col in rk.ranks] == ranks
    assert table_logup_cases.m_column(counts, first, u) == m
    assert table_logup_cases.ranked_sum(ranks, values, counts, first, c.beta, u) == phi


def test_a_table_as_long_as_the_rows():
    c = cases.sum_case("two tiles", 1, n_unique="u", u=TWO_TILES)
    assert c.nu == c.u and len(set(_ints(c.table[: c.u]))) == c.u
    rk = cases.ranked(c)
    assert sorted(rk.first.tolist()) == list(range(c.u)) and int(rk.counts.sum()) == c.u


@pytest.mark.parametrize("m", [1, 3, 4])
def test_kate_references_agree_on_two_tiles(m):
    n = 2049
    c = cases.kate_case("C-short" if m != 3 else "B-full", m, n=n)
    assert {1, R - 1} <= set(c.roots) or m == 1
    cur = _ints(c.num)
    assert cur[n - 1] != 0  # the numerator fills all n coefficients
    for r in c.roots:  # exact division root by root: the remainder is zero and the quotient by all of them is Q
        assert o.eval_polynomial(cur, r) == 0
        cur = o.kate_division(cur, r)
    assert cur == _ints(c.want)[: n - m] and _ints(c.want)[n - m:] == [0] * (m - 1) and len(c.want) == n - 1
    # the stated definition on a numerator no root divides: the weighted sum of the single divisions
    for pattern in ("all r - 1", "random choice"):
        words = cases.extreme_words(pattern, n)
        roots = [1, R - 1, extreme_cases.TOP261, extreme_cases.OVER261][:m]
        single = [o.kate_division(_ints(words), r) for r in roots]
        weights = extreme_cases.partial_fraction_weights(roots)
        want = [sum(w * s[i] for w, s in zip(weights, single)) % R for i in range(n - 1)]
        assert _ints(cases.kate_multi_reference(words, roots)) == want
    assert _ints(cases.kate_multi_reference(c.num, c.roots)) == _ints(c.want)


def test_the_kate_roots_of_the_named_cases():
    for size, m in (("C-short", 1), ("C-short", 4), ("C-even", 1), ("C-even", 4), ("B-full", 3)):
        roots = cases.kate_roots(size, m)
        assert len(set(roots)) == m and all(0 < r < R for r in roots)
        assert {1, R - 1} <= set(roots) if m > 1 else roots[0] in (1, R - 1)
    assert cases.kate_roots("C-short", 1) + cases.kate_roots("C-even", 1) == [1, R - 1]


def test_gwc_reference_agrees_on_two_tiles():
    """the vector reference against the Python integers of tests/test_gpu_gwc.py's kernel test"""
    n = 2049
    c = cases.gwc_case("B-min", n=n)
    assert c.terms == [3, 1, 72, 2, 73] and set(c.roots) >= {1, R - 1} and c.index[0][0] == c.index[2][0] == c.index[4][0] == 0
    pool = [_ints(p) for p in c.pool]
    got = cases.gwc_reference(c)
    for g, t in enumerate(c.terms):
        acc = [0] * n
        for j in range(t):
            s, poly = c.scalars[g][j], pool[c.index[g][j]]
            for i in range(n):
                acc[i] += s * poly[i]
        assert _ints(got[g]) == o.kate_division([a % R for a in acc], c.roots[g]) + [0], g
    assert cases.GWC_CASES["C-short"]["terms"] == [2, 2] and cases.GWC_CAP == 72
