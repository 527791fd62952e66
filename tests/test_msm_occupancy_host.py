"""tests/msm_occupancy_cases.py without a GPU: every case's scalars are canonical and recode to digits that put the intended number of
entries where the case says; the property each case is named for holds in the model (both sides of a threshold really lie on both
sides); the model's result, computed from the discrete logarithms of the bases, is the C oracle's MSM over the same limbs, and the
weighted bucket sum of the model's bucket sums is that result again; and the constants the model restates agree with
tests/msm_schedule_cases.py and tests/table_depth_cases.py where they overlap."""
from collections import Counter

import numpy as np
import pytest

import msm_occupancy_cases as M
import msm_schedule_cases as S
import table_depth_cases as T
from oracle import bn254 as o

CASES = M.cases()
IDS = [c.id for c in CASES]


def test_constants_agree_with_the_other_models():
    assert (M.P1_TS, M.S1, M.S0_MAX, M.ACCUM_RESIDENT_CHUNKS, M.MAT_LOG, M.SHIFT_MIN_N) == (T.P1_TS, T.S1, T.S0_MAX, T.ACCUM_RESIDENT_CHUNKS, T.MAT_LOG, T.SHIFT_MIN_N)
    assert M.PART_WORDS * 4 == T.PART_BYTES
    for c in range(11, 21):
        g = M.geometry(c)
        assert g.W == T.windows(c) and g.nb == 1 << (c - 1) and g.nbins << g.lb == g.nb and g.nbins <= 512
        assert g.logNl + g.logNh + g.seg_log == c - 1 and g.wide == (c >= M.WIDE_MIN_C)
        assert sorted(g.pos(b) for b in range(0, g.nb, 97)) == sorted({g.pos(b) for b in range(0, g.nb, 97)})
        assert all(g.bucket_at(g.pos(b)) == b for b in (0, 1, 511, 512, g.nb // 3, g.nb - 1))
    for n in (1, 2047, 2048, 2049, 1 << 14):
        assert T.window(n) == S.pick_window(n) or T.FORCED_C
    assert S.pick_window(1 << 10) == 13 and S.pick_window(M.N15) == S.pick_window(M.NSHIFT) == S.pick_window(M.NMAX) == 15  # (every case registers with its width forced)
    assert [T._accum_rounds(e) for e in (0, 1, 1 << 24, (1 << 24) + 1)] == [M.accum_rounds(e) for e in (0, 1, 1 << 24, (1 << 24) + 1)]
    assert [M.chunk_len(e) for e in (0, 16384, 16385, 8 * 131072, 8 * 131072 + 1, 1 << 24)] == [1, 1, 8, 8, 9, 128]
    assert M.NSHIFT % M.P1_TS == 0 and M.NSHIFT >= M.SHIFT_MIN_N > M.N15 > M.N13


def test_from_digits_round_trips_and_rejects():
    for c in (13, 15, 17, 18, 20):
        half, W = 1 << (c - 1), M.windows(c)
        s = M.from_digits({0: half, 1: -(half - 1), 2: 1, W - 1: 1}, c)
        assert M.recode(s, c)[:3] == [half, -(half - 1), 1] and M.recode(s, c)[W - 1] == 1
        with pytest.raises(AssertionError):
            M.from_digits({3: -5}, c)  # a negative scalar
        with pytest.raises(AssertionError):
            M.from_digits({0: half + 1}, c)  # not a digit: it recodes to a negative one and a carry
        with pytest.raises(AssertionError):
            M.from_digits({W - 1: half}, c)  # beyond r


def test_bases_have_the_advertised_relations():
    k, b = M.logs(), M.bases()
    pts = o.unpack_points(b[:16])
    assert pts[M.IDENTITY_AT] is None and k[M.IDENTITY_AT] == 0
    p, q = pts[M.PAIR_AT[0]], pts[M.PAIR_AT[1]]
    assert p[0] == q[0] and (p[1] + q[1]) % o.Q == 0
    for src, dst in M.REPEAT_AT:
        assert b[src].tobytes() == b[dst].tobytes() and k[src] == k[dst]
    assert pts[1] == o.g1_mul(k[1], (1, 2))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_model(case):
    g = M.geometry(case.c)
    assert case.n <= case.n_reg <= M.NMAX and all(0 <= s < M.R for s in case.scalars)
    h, sm = M.model(case)
    assert h.entries <= 300000
    # the model's counts are the digits of the scalars it was given (shift aside)
    if not h.v:
        cnt = np.zeros(g.nb, dtype=np.int64)
        for s, m in Counter(case.scalars).items():
            for d in M.recode(s, case.c) if s else ():
                if d:
                    cnt[g.pos(abs(d) - 1)] += m
        assert (cnt == h.cnt).all()
    assert h.entries == int(h.off[-1]) == len(h.payload) and h.np0[-1] == 0 and h.np1[-1] == 0
    assert int(h.toff0[-1]) == int(h.np0.sum()) and int(h.toff1[-1]) == int(h.np1.sum())
    assert ((h.np0[:-1] > 0) == (h.cnt > 0)).all() and (h.np0[:-1] <= h.cnt).all()
    assert int(h.np0.sum()) <= -(-h.entries // h.s0) + int((h.cnt > 0).sum())
    # the labelled property
    e = case.expect
    if "s0" in e:
        assert h.s0 == e["s0"]
    if "entries" in e:
        assert h.entries == e["entries"]
    if "v" in e:
        assert h.v == e["v"] and case.shifted == (case.n == case.n_reg)
    for p, want in e.get("np0", {}).items():
        assert int(h.np0[p]) == want, (p, int(h.np0[p]), want)
    if "hot" in e:
        assert h.hot == sorted(e["hot"])
    for p in e.get("not_hot", []):
        assert p not in h.hot and int((h.np0 if g.wide else h.np1)[p]) == g.hot_min, "the cold side of the threshold sits exactly on it"
    for p in e.get("hot", []):
        assert int((h.np0 if g.wide else h.np1)[p]) > g.hot_min
    # the sums
    assert M.weighted(h, sm) == sm.result


ALL_CASES = M.all_cases()


@pytest.mark.parametrize("case", ALL_CASES, ids=[c.id for c in ALL_CASES])
def test_model_result_is_the_oracles_msm(case):
    """every case, the batch, lane / quad and slot-reuse cases of family H included: the model's result, from the discrete logarithms,
    is the C oracle's MSM over the same scalars and bases, and the model's weighted bucket sum is that result"""
    from oracle import cref

    assert M.weighted(*M.model(case)) == M.model(case)[1].result

    _, sm = M.model(case)
    nz = [i for i, s in enumerate(case.scalars) if s]
    want = cref.normalize(cref.msm(o.pack([case.scalars[i] for i in nz], M.R), M.bases()[nz], 4))
    assert M.points_of([sm.result]).tobytes() == want.tobytes()


def test_thresholds_lie_on_both_sides():
    by = {c.id: c for c in CASES}
    for pre, want in ((0, 512), (1, 513), (7, 513), (8, 512)):
        h, _ = M.model(by[f"A-c15-4096-after-{pre}"])
        assert int(h.cnt[99]) == 4096 and int(h.off[99]) == pre and int(h.np0[99]) == want and (99 in h.hot) == (want == 513)
    assert M.model(by["D-c15-16384-entries"])[0].s0 == 1 and M.model(by["D-c15-16385-entries"])[0].s0 == 8
    for s0 in (3, 128):
        h, _ = M.model(by[f"C-c13-np0-1-to-65-S0_{s0}"])
        assert h.s0 == s0 and sorted(set(h.cnt[h.cnt > 0].tolist())) == sorted(M.FOLD_NP0)
    h, _ = M.model(by["E-c15-bins-of-8191-8192-8193-16385-and-every-start-residue"])
    per_bin = 1 << h.geo.lb
    bins = h.cnt.reshape(-1, per_bin).sum(axis=1)
    assert sorted(bins[bins > 17].tolist()) == sorted(2 * [M.P2_CH - 1, M.P2_CH, M.P2_CH + 1, 2 * M.P2_CH + 1])
    starts = np.concatenate(([0], np.cumsum(bins)))[:-1]
    assert {int(starts[b]) % 16 for b in range(100, 117)} == set(range(16))
    h, _ = M.model(by["E-c18-bins-of-6143-6144-6145"])
    bins = h.cnt.reshape(-1, 1 << h.geo.lb).sum(axis=1)
    assert sorted(bins[bins > 0].tolist()) == sorted(2 * [M.P2W_CH - 1, M.P2W_CH, M.P2W_CH + 1])
    f = {c.name: M.model(c)[0] for c in CASES if c.family == "F"}
    assert f["39-of-64-sampled-rows-agree"].v == 0 and f["40-of-64-sampled-rows-agree"].v != 0 and f["n-minus-1-of-n-bases"].v == 0
    hc = f["constant-column-sum-point-alone-in-a-tile"]
    assert set((hc.payload & 0x7FFFFFFF) % hc.stride) == {M.NSHIFT}, "only the sum point has entries, and row NSHIFT opens a tile of its own"
    assert f["sampled-rows-agree-all-others-zero"].entries > 16 * (M.NSHIFT - 64)
    for c in (18, 19, 20):
        h, sm = M.model(next(x for x in CASES if x.family == "B" and x.c == c))
        g = h.geo
        assert {0, g.nb // g.L - 1, 5} <= set(sm.seg_p) and sm.seg_v[5] != 0 and all(h.cnt[g.pos(5 * g.L + j)] for j in range(g.L))
    assert [(fold, fin) for _, _, _, fold, fin in M.lane_quad_batches()] == [(True, False), (False, False), (True, True), (True, False)]
    for fam in "ADFG":
        b = M.batch_family(fam)
        assert len({c.id for c in b}) == 4 and len({(c.c, c.n_reg, c.n) for c in b}) == 1 and not any(b[3].scalars)
