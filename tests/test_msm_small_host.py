"""tests/msm_small_cases.py checked on the host: every case has the property it is named for (the model's classification finds the class
at the stated lane, level or workgroup), the model's result is the C restatement's MSM, its digits are tests/table_depth_cases.py's
recoding, its geometry is tests/msm_schedule_cases.py's, and the combinations of tree, level and class the cases do not reach are
the listed ones."""
import pytest

import msm_schedule_cases as S
import msm_small_cases as M
import table_depth_cases as T
from oracle import bn254 as o

CASES = M.all_cases()


def test_sizes_come_from_the_geometry_rule():
    g = {n: S.small_geometry(n) for n in M.SIZES}
    assert all(x.table for x in g.values())
    assert (g[M.N_TREE].lanes, g[M.N_TREE].r, S.small_geometry(M.N_L256 - 1).lanes, g[M.N_L256].lanes) == (128, 1, 128, 256)
    assert (g[M.N_GMAX].r, g[M.N_GMAX].G, g[M.N_R2].r, S.small_geometry(M.N_R3 - 1).r, g[M.N_R3].r) == (1, S.SMALL_PARTS_MAX, 2, 2, 3)
    assert (S.small_geometry(M.N_C6 - 1).c, g[M.N_C6].c, g[M.N_MAX].c, g[M.N_MAX].r) == (7, 6, 6, 6)
    assert not S.small_geometry(M.N_MAX + 1).table


@pytest.mark.parametrize("c", [6, 7])
def test_digit_model_is_the_recoding(c):
    """the byte model (32-bit words, the zero word above the top) against the integer recoding, on the digit family's scalars, on dense
    ones and on random ones; from_digits inverts it"""
    named = M.digit_scalars(c)
    col = list(named.values()) + [M.dense_scalar(c, i) for i in range(64)] + o.unpack(o.random_field_limbs(256, 0x5A11 + c), M.R)
    assert M.windows(c) == T.windows(c)
    for s in col:
        got = [M.signed(b) for b in M.digit_bytes(s, c)]
        assert got == T.recode(s, c), hex(s)
        assert all(-(1 << (c - 1)) < d <= 1 << (c - 1) for d in got)
        if s:
            assert M.from_digits({w: d for w, d in enumerate(got) if d}, c) == s
    half = 1 << (c - 1)
    for w in range(M.windows(c) - 1):
        assert M.digit_bytes(half << (c * w), c)[w] == half  # exactly 2^(c-1): positive, no carry
        assert M.digit_bytes((half + 1) << (c * w), c)[w:w + 2] == [0x80 | (half - 1), 1]  # the first negative digit
    straddling = [w for w in range(M.windows(c)) if (w * c) % 32 + c > 32]
    assert straddling and all(f"only digit 1 in window {w}" in named for w in straddling + [M.windows(c) - 1])


@pytest.mark.parametrize("n", M.SIZES)
def test_bases_and_table_logarithms(n):
    k = M.logs(n)
    g = S.small_geometry(n)
    assert k[M.IDENTITY_AT] == 0 and all((k[i] + k[i + 2]) % M.R == 0 for i in range(0, n - 3, 4))
    assert all(k[i] == k[i + 256] for i in range(1, min(n - 256, 200), 4))
    for i in range(min(n, 600)):
        f = M.factored(n, i)
        assert (f is None) == (k[i] == 0) and (f is None or f[0] * f[1] * pow(2, g.c * f[2], M.R) % M.R == k[i])
    samples = M.table_samples(n)
    assert {0, g.W - 1} <= {w for w, _ in samples} and any(k[i] == 0 for _, i in samples)
    assert max(M.table_entry(n, 1 << (g.c - 1), w, i) for w, i in samples) < g.table_bytes // 64


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_has_its_property_and_the_oracles_result(case):
    from oracle import cref

    m = M.model_of(case)
    g = S.small_geometry(case.n_reg)
    assert m.geo == g and m.G == -(-case.n * g.W // (g.lanes * g.r)) <= g.G
    k = M.logs(case.n_reg)
    assert m.result == sum(s * ki for s, ki in zip(case.scalars, k)) % M.R == sum(m.part) % M.R
    got = cref.normalize(cref.msm(o.pack(list(case.scalars), M.R), M.bases(case.n_reg)[:case.n], 4))
    assert got.tobytes() == M.points_of([m.result]).tobytes()
    assert m.entries == sum(1 for i, s in enumerate(case.scalars) for d in T.recode(s, g.c) if d and k[i])
    exp = case.expect
    for key, cls in exp.get("chain", {}).items():
        assert m.chain.get(key) == cls, (key, m.chain.get(key), cls)
    for key, cls in exp.get("tree1", {}).items():
        assert m.tree1.get(key) == cls, (key, m.tree1.get(key))
    for key, cls in exp.get("tree2", {}).items():
        assert m.tree2.get(key) == cls, (key, m.tree2.get(key))
        assert sum(1 for p in m.part if p) == 2  # nothing else in the tree
    for (w, i), d in exp.get("digits", {}).items():
        assert M.signed(int(m.digits[w, i])) == d, (w, i)
    if "crossing" in exp:
        b, t = exp["crossing"]
        per = g.lanes * g.r
        ws = {(b * per + kk * g.lanes + t) // case.n for kk in range(g.r)}
        assert ws == {0, 1} and len(m.chain[(b, t)]) >= 2 and M.SKIPPED not in m.chain[(b, t)]
    if "G" in exp:
        assert m.G == exp["G"]
    if "live" in exp:
        assert M.live_lanes(g, case.n, m.G - 1) == exp["live"] < g.lanes and len({t for b, t in m.chain if b == m.G - 1}) == exp["live"]
    if "result" in exp:
        assert m.result == exp["result"]
    if "entries" in exp:
        assert m.entries == exp["entries"]


def test_chain_cases_cover_the_listed_steps():
    """over the three chain cases: every class of a chain step, at the first, a middle and the last step of the longest chain"""
    seen = {}
    for case in M.cases():
        if case.family == "chains":
            r = S.small_geometry(case.n_reg).r
            for steps in case.expect["chain"].values():
                for k, cls in enumerate(steps):
                    seen.setdefault(cls, set()).add((r, k))
    assert set(seen) >= {M.IDENT, M.EQUAL, M.OPPOSITE, M.GENERAL, M.SKIPPED}
    rs = {S.small_geometry(n).r for n in (M.N_R2, M.N_R3, M.N_MAX)}
    assert rs == {2, 3, 6} and {r for r, _ in seen[M.EQUAL]} == rs and {r for r, _ in seen[M.OPPOSITE]} == rs and {r for r, _ in seen[M.SKIPPED]} == rs


def test_reached_combinations_are_the_listed_ones():
    got = M.reached()
    missing = tuple(w for w in M.wanted() if w not in got)
    assert missing == M.NOT_REACHED
    # the second tree at its full width: every level has all three classes
    assert all((2, 512, 1 << e, k) in got for e in range(9) for k in (M.EQUAL, M.OPPOSITE, M.IDENT))


def test_state_columns():
    for n in M.STATE_SIZES:
        full, prefixes = M.full_column(n), M.prefix_columns(n)
        g = S.small_geometry(n)
        assert (M.model_of(full).digits != 0).all() and M.model_of(full).G == g.G
        assert [p.n for p in prefixes] == [n - 1, n // 2, 1] and M.model_of(prefixes[0]).G <= g.G and M.model_of(prefixes[1]).G < g.G and M.model_of(prefixes[2]).G == 1
        for p in prefixes:  # the prefix differs from what the full column left in every row it writes (but the top one: every digit there is 1)
            assert (M.model_of(p).digits != M.model_of(full).digits[:, :p.n])[:-1].any(axis=1).all()
    cols = M.phase_columns(M.N_TREE)
    assert len(cols) == S.HEAD_BATCH and M.model_of(cols[1]).entries == 0 and len({M.model_of(c).result for c in cols}) == 4
    assert M.model_of(M.phase_columns(M.N_L256, 1)[0]).G != M.model_of(cols[0]).G
    nine = M.nine_columns(M.N_TREE)
    assert len(nine) == S.SMALL_BATCH + 1 == M.NSLOT + 1 and len({M.model_of(c).G for c in nine}) > 3
