"""The pass scheme of a base set with a table depth (tests/table_depth_cases.py), in Python integers: every edge scalar is the
recombination of its passes at every depth the device tests register; each named case reaches what it is named for; and the byte
formula of DESIGN.md 3 behaves as a dial."""
import pytest

import table_depth_cases as T

WIDTHS = sorted({T.window(n) for n in T.SIZES} | {19, 20})


def _scalars(c, D):
    out = dict(T.edge_scalars(c))
    W = T.windows(c)
    Dp, _ = T.effective(D, W)
    for q in {0, 1, Dp - 1}:
        for i, s in enumerate(T.one_class_scalars(c, D, q)):
            out[f"class {q} #{i}"] = s
    return out


@pytest.mark.parametrize("c", WIDTHS)
def test_every_edge_scalar_is_the_recombination_of_its_passes(c):
    W = T.windows(c)
    for D in T.depths(W):
        for name, s in _scalars(c, D).items():
            digits = T.recode(s, c)
            assert len(digits) == W and all(-(1 << (c - 1)) < d <= 1 << (c - 1) for d in digits), (c, D, name)
            assert sum(d << (c * w) for w, d in enumerate(digits)) == s, (c, name)
            assert T.recombine(s, c, D) == s, (c, D, name)
            Dp, rows = T.effective(D, W)
            assert all(row < rows for entries in T.pass_digits(s, c, D) for row, _ in entries)


@pytest.mark.parametrize("c", WIDTHS)
def test_each_case_reaches_what_it_is_named_for(c):
    W, half = T.windows(c), 1 << (c - 1)
    E = T.edge_scalars(c)
    # the digit that is exactly 2^(c-1) stays positive and carries nothing; one more is the first negative digit and carries
    for w in range(W - 1):
        if f"half+1 at {w}" not in E:
            continue
        d = T.recode(E[f"half at {w}"], c)
        assert d[w] == half and not any(d[:w]) and not any(d[w + 1:])
        d = T.recode(E[f"half at {w}, plus 1"], c)
        assert (d[0] == -(half - 1) and d[1] == 1) if w == 0 else (d[0] == 1 and d[w] == half)
        d = T.recode(E[f"half+1 at {w}"], c)
        assert d[w] == -(half - 1) and d[w + 1] == 1
    # carries that run through every window: 2^(c w) - 1 is -1 in window 0 and +1 in window w
    for w in range(2, W):
        d = T.recode(E[f"2^(c{w})-1"], c)
        assert d[0] == -1 and d[w] == 1 and not any(d[1:w])
    # the top window is reached: by r - 1 itself, and by a carry out of the window below it
    assert T.recode(E["r-1"], c)[W - 1] != 0
    d = T.recode(E[f"half+1 at {W - 2}"], c)
    assert d[W - 1] == 1 and d[W - 2] < 0
    for D in T.depths(W):
        Dp, rows = T.effective(D, W)
        if Dp == 1:
            continue
        # a carry crosses a pass boundary: consecutive windows belong to different passes
        assert T.pass_of(W - 2, Dp) != T.pass_of(W - 1, Dp)
        per_pass = T.pass_digits(E[f"half+1 at {W - 2}"], c, D)  # the negative digit in one pass, its carry in the next
        assert [r for r, p in enumerate(per_pass) if p] == sorted({T.pass_of(W - 2, Dp), T.pass_of(W - 1, Dp)})
        # an empty pass exists: the one-class scalars leave entries in one pass only, and reproduce the digits they were built from
        for q in {0, 1, Dp - 1}:
            for s in T.one_class_scalars(c, D, q):
                live = [r for r, p in enumerate(T.pass_digits(s, c, D)) if p]
                assert live == [q % Dp], (c, D, q)
        # every pass of the uniform column has work, every window has its pass and row, rows are used from 0 up
        seen = {}
        for w in range(W):
            seen.setdefault(T.pass_of(w, Dp), []).append(T.row_of(w, Dp))
        assert sorted(seen) == list(range(Dp)) and all(v == list(range(len(v))) for v in seen.values())
        assert max(len(v) for v in seen.values()) == rows


def test_depths_cover_both_sides_of_the_window_count():
    for n in T.SIZES:
        W = T.windows(T.window(n))
        ds = T.depths(W)
        assert {1, 2, 3, 4, W - 1, W, W + 5} == set(ds)
        assert T.effective(W + 5, W) == (W, 1) and T.effective(W, W) == (W, 1) and T.effective(W - 1, W) == (W - 1, 2) and T.effective(1, W) == (1, W)


@pytest.mark.parametrize("n", list(T.SIZES) + [1 << 17, (1 << 17) + 1, 1 << 20, 1 << 22])
def test_the_byte_formula_is_monotone_in_the_depth(n):
    W = T.windows(T.window(n))
    prev = None
    for D in range(1, W + 6):
        Dp, rows, table, work = T.memory(n, D)
        assert (Dp, rows) == T.effective(D, W)
        if D > 1:
            assert table >= rows * (n + 1) * 64 and table == rows * (n + 1) * 64
        if prev is not None:
            assert table <= prev[0] and work <= prev[1], (n, D)
        if D == 2:
            assert table < prev[0] and work < prev[1]
        prev = (table, work)
        if D >= W:
            assert table == (n + 1) * 64


def test_the_byte_formula_at_the_sizes_design_md_quotes():
    """0.94 GiB of table per set at 2^20 (c = 17, W = 15), 3.25 GiB at 2^22 (c = 20, W = 13); the bases alone at D >= W"""
    for k, W, gib in ((20, 15, 0.94), (22, 13, 3.25)):
        n = 1 << k
        _, rows, table, _ = T.memory(n, 1)
        assert rows == W and abs(table / 2**30 - gib) < 0.01
        assert T.memory(n, W)[2] == (n + 1) * 64
        assert T.memory(n, 2)[2] == -(-W // 2) * (n + 1) * 64
