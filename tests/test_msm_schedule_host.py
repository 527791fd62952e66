"""tests/msm_schedule_cases.py on the host: the edges of the small-path geometry lie where the constants of csrc/h2mi_msm.hip put them,
no size outgrows the partial-sum tree or the table budget, the transition schedules cover every ordered pair of call kinds with
every slot used by both, and the model of the scheduler predicts the streaming rule's switches — independently of the library."""
import pytest

import msm_schedule_cases as S


def test_edges_lie_on_both_sides_and_differ_by_one_point():
    for name, (lo, hi) in S.EDGE_N.items():
        assert hi == lo + 1, name
        a, b = S.small_geometry(lo), S.small_geometry(hi)
        assert (a.table, a.c, a.lanes, a.r) != (b.table, b.c, b.lanes, b.r), name
    g = {name: (S.small_geometry(lo), S.small_geometry(hi)) for name, (lo, hi) in S.EDGE_N.items()}
    a, b = g["lanes 128 to 256"]
    assert (a.lanes, b.lanes, a.r, b.r) == (128, 256, 1, 1) and a.n * a.W <= 128 * 256 < b.n * b.W
    a, b = g["cells per lane 1 to 2"]
    assert (a.r, b.r) == (1, 2) and a.lanes == b.lanes == 256 and a.n * a.W <= 256 * 512 < b.n * b.W
    a, b = g["cells per lane 2 to 3"]
    assert (a.r, b.r) == (2, 3) and a.n * a.W <= 2 * 256 * 512 < b.n * b.W
    a, b = g["window 7 to 6 bits"]
    assert (a.c, b.c, a.W, b.W) == (7, 6, 37, 43) and a.table_bytes <= S.SMALL_TABLE_BUDGET < 64 * 37 * b.n * 64
    a, b = g["last size with the table"]
    assert a.table and not b.table and a.n == S.SMALL_MAX_N
    # the sizes worked out by hand from the constants
    assert list(S.EDGE_N.values()) == [(885, 886), (3542, 3543), (7084, 7085), (14169, 14170), (16384, 16385)]
    assert len(S.EDGE_SIZES) == 10 and len({n for _, n in S.EDGE_SIZES}) == 10


def test_no_size_outgrows_the_partial_sum_tree_or_the_table_budget():
    worst_G = worst_bytes = 0
    for n in range(1, S.SMALL_MAX_N + 1):
        g = S.small_geometry(n)
        assert g.table and g.W == -(-255 // g.c) and g.lanes in (128, 256) and g.r >= 1
        assert g.G * g.lanes * g.r >= n * g.W > (g.G - 1) * g.lanes * g.r, n  # every cell has a lane, the last workgroup is not empty
        worst_G, worst_bytes = max(worst_G, g.G), max(worst_bytes, g.table_bytes)
    assert worst_G <= S.SMALL_PARTS_MAX
    assert worst_bytes <= 2 << 30
    assert not S.small_geometry(S.SMALL_MAX_N + 1).table
    # the two sizes the header names: c = 7 up to 2^13 points, c = 6 and six cells per lane at 2^14
    assert S.small_geometry(1 << 13)[2:7] == (7, 37, 256, 3, 395) and S.small_geometry(1 << 14)[2:7] == (6, 43, 256, 6, 459)
    assert S.small_reduce_adds(300) == S.small_geometry(300).G * 128 and S.small_reduce_adds(1 << 13) == 395 * 256


def test_eight_kinds_and_all_64_ordered_pairs():
    assert len(S.KINDS) == 8 and len({k[1:] for k in S.KINDS}) == 8
    sched = S.transition_schedules()
    assert set(sched) == {f"{a.name}->{b.name}" for a in S.KINDS for b in S.KINDS} and len(sched) == 64
    for name, ops in sched.items():
        a, b = (S.KIND[x] for x in name.split("->"))
        calls = [op for op in ops if isinstance(op, S.Call)]
        assert [op for op in ops if not isinstance(op, S.Call)] == [S.Join("h2mi_join")] and ops[-1] == S.Join("h2mi_join"), name
        kinds = [c.kind for c in calls for _ in c.entries]
        assert kinds == [a] * 8 + [b] * 8, name
        for c in calls:
            assert len(c.entries) == (4 if c.kind.batch else 1) and len({length for _, length in c.entries}) == 1, name
            assert all(e in S.pool(1 << 13) for e in c.entries), name


@pytest.mark.parametrize("n", [1 << 13, 1 << 14])
def test_every_slot_sees_both_kinds(n):
    """in each schedule the model puts MSM i and MSM i + 8 on the same slot, whatever the paths"""
    for name, ops in S.transition_schedules(n).items():
        p = S.predict(n, ops)
        assert len(p.slots) == 16 and p.slots[:8] == list(range(8)) and p.slots[8:] == p.slots[:8], name
        a, b = (S.KIND[x] for x in name.split("->"))
        if n <= S.SMALL_STREAM_N:  # never switches by itself: every step's path is the one its kind names
            assert p.paths == [S.GENERAL if a.general else S.SMALL] * 8 + [S.GENERAL if b.general else S.SMALL] * 8, name
        else:  # the streaming rule: the first four MSMs of a small kind, none after
            assert p.paths[4:] == [S.GENERAL] * 12 and p.paths[:4] == [S.GENERAL if a.general else S.SMALL] * 4, name


def test_model_predicts_the_streaming_rule():
    s, g = S.SMALL, S.GENERAL
    for n in (8193, 16384):
        sch = S.streaming_schedules(n)
        assert S.predict(n, sch["six singles, one join"]).paths == [s] * 4 + [g] * 2
        for how in S.JOINS:
            assert S.predict(n, sch[f"small again after {how}"]).paths == [s] * 4 + [g] * 2 + [s], how
        nine = S.predict(n, sch["a phase of nine: groups of 4, 4, 1"])
        assert nine.heads == [s, g, g] and nine.paths == [s] * 4 + [g] * 5 and nine.slots == [0, 1, 2, 3, 4, 5, 6, 7, 0]
        assert S.predict(n, sch["four on a caller's stream count"]).paths == [s] * 4 + [g]
        assert S.predict(n, sch["a forced general MSM counts"]).paths == [g, s, s, s, g]
    sch = S.streaming_schedules(8192)
    for name, ops in sch.items():
        want = [g if c.kind.general else s for c in ops if isinstance(c, S.Call) for _ in c.entries]
        assert S.predict(8192, ops).paths == want, name
    assert S.STREAMING_SIZES == (8192, 8193, 16384)


def test_model_census_of_the_reductions():
    """the launches the model predicts for the deferred reductions: a flush when half the slots are pending, at a join, never twice"""
    k = S.KIND
    one = lambda kind: S.Call(k[kind], (("uniform", 8192),))
    p = S.predict(8192, [one("small-single")] * 6 + [S.Join("h2mi_join")])
    assert p.census == {S.DIGITS: 6, S.BIN_COUNT: 0, S.ACCUM: 0, S.SMALL_PAIR: 2, S.FINAL: 0, S.SEG: 0}  # four pending, then two at the join
    p = S.predict(8193, [one("small-single")] * 6 + [S.Join("h2mi_join")])
    assert p.census == {S.DIGITS: 4, S.BIN_COUNT: 2, S.ACCUM: 2, S.SMALL_PAIR: 1, S.FINAL: 1, S.SEG: 0}
    p = S.predict(8193, S.streaming_schedules(8193)["a phase of nine: groups of 4, 4, 1"])
    assert p.census == {S.DIGITS: 1, S.BIN_COUNT: 2, S.ACCUM: 2, S.SMALL_PAIR: 1, S.FINAL: 2, S.SEG: 0}
    # in order or on a caller's stream nothing is deferred: one reduction launch per call
    p = S.predict(8192, [one("small-inorder"), one("general-stream"), one("general-inorder"), one("small-stream"), S.Join("h2mi_join")])
    assert p.census == {S.DIGITS: 2, S.BIN_COUNT: 2, S.ACCUM: 2, S.SMALL_PAIR: 2, S.FINAL: 2, S.SEG: 0}
    # three handles, one list: a flush launches each kind of deferred work as a batch of its own
    sch = S.Scheduler()
    a, b, c = sch.register(300), sch.register(20000), sch.register(20000, forced_c=18)
    assert (a.table, b.table, c.table, a.wide, b.wide, c.wide) == (True, False, False, False, False, True)
    for h in (a, b, c):
        sch.msm(h)
    assert not any(sch.census[x] for x in (S.SMALL_PAIR, S.FINAL, S.SEG)) and len(sch.deferred) == 3
    sch.flush()
    assert (sch.census[S.SMALL_PAIR], sch.census[S.FINAL], sch.census[S.SEG]) == (1, 2, 1) and not sch.deferred
    before = dict(sch.census)
    sch.flush()
    assert dict(sch.census) == before


def test_pool_columns_are_what_their_names_say():
    from oracle import bn254 as o

    n = 300
    R = o.R
    val = lambda name: o.unpack(S.column(n, name), R)
    assert set(val("zero")) == {0} and set(val("r-1")) == {R - 1} and len(set(val("repeated"))) == 1
    rep3 = val("repeated3")
    assert len(set(rep3)) == 4 and [i for i, v in enumerate(rep3) if v != rep3[1]] == [0, n // 2, n - 1]
    sp = val("sparse")
    assert [i for i, v in enumerate(sp) if v] == list(range(0, n, 64))
    assert len(set(val("uniform"))) == n and val("uniform") != val("uniform2") and val("witness").count(0) > n // 2
    lengths = {length for _, length in S.pool(n)}
    assert lengths == {n, n - 5, n // 3 + 1} and 10 <= len(S.pool(n)) <= 16
    assert not S.column(n, "uniform").flags.writeable
