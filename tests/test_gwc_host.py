"""ProverGWC's tail with no device in the loop (tests/gwc_cases.py): the Python-integer prover tail against the verifier tail on random
polynomials over the oracle's SRS, the `multiopen` keyword of the Python hosts, and the four prover-ABI symbols in _lib."""
import random
import types

import pytest

import gwc_cases as G
from oracle import bn254 as o

R = o.R
K, SECRET = 4, 0x5EC2E7
N = 1 << K


@pytest.fixture(scope="module")
def tail():
    """3 points with 4, 1 and 2 queries (one polynomial opened at two points), their commitments and the honest [W_i]"""
    rng = random.Random(0x6C19)
    g, _ = o.srs(K, SECRET)
    commit = lambda poly: o.msm_naive(poly, g[:len(poly)])
    polys = {name: [rng.randrange(R) for _ in range(N)] for name in "abcde"}
    z = [rng.randrange(1, R) for _ in range(3)]
    where = [("a", 0), ("b", 1), ("c", 0), ("a", 2), ("d", 0), ("e", 2), ("b", 0)]  # points in order of first appearance: z0, z1, z2
    queries = [(name, z[i], o.eval_polynomial(polys[name], z[i])) for name, i in where]
    points = {name: commit(poly) for name, poly in polys.items()}
    v, u = rng.randrange(R), rng.randrange(R)
    ws = G.gwc_witnesses(polys, queries, v)
    return types.SimpleNamespace(keys=types.SimpleNamespace(s=SECRET), polys=polys, queries=queries, points=points, v=v, u=u, ws=ws,
                                 Ws=[commit(w) for w in ws], z=z)


def test_groups_keep_first_appearance_and_list_order(tail):
    groups = G.gwc_groups(tail.queries)
    assert [pt for pt, _ in groups] == tail.z
    assert [[key for key, _ in members] for _, members in groups] == [["a", "c", "d", "b"], ["b"], ["a", "e"]]


def test_witnesses_divide_exactly(tail):
    """W_i (X - z_i) = sum_j v^j (p_ij - e_ij): the dropped remainder is zero"""
    for (z, members), w in zip(G.gwc_groups(tail.queries), tail.ws):
        assert len(w) == N - 1
        x = 0xABCDEF
        num, vp = 0, 1
        for key, ev in members:
            num = (num + vp * (o.eval_polynomial(tail.polys[key], x) - ev)) % R
            vp = vp * tail.v % R
        assert o.eval_polynomial(w, x) * (x - z) % R == num


def test_honest_tail_is_accepted(tail):
    assert G.gwc_check(tail.points, tail.queries, tail.v, tail.Ws, tail.u, tail.keys)


def test_flipped_evaluation_is_rejected(tail):
    for at in (0, 4, len(tail.queries) - 1):
        queries = list(tail.queries)
        key, pt, ev = queries[at]
        queries[at] = (key, pt, ev ^ 1)
        assert not G.gwc_check(tail.points, queries, tail.v, tail.Ws, tail.u, tail.keys)


def test_swapped_w_is_rejected(tail):
    Ws = [tail.Ws[1], tail.Ws[0], tail.Ws[2]]
    assert not G.gwc_check(tail.points, tail.queries, tail.v, Ws, tail.u, tail.keys)
    assert not G.gwc_check(tail.points, tail.queries, tail.v, tail.Ws[:2], tail.u, tail.keys)


def test_wrong_v_is_rejected(tail):
    assert not G.gwc_check(tail.points, tail.queries, (tail.v + 1) % R, tail.Ws, tail.u, tail.keys)


def test_unknown_multiopen_is_refused(h2):
    """every Python host refuses a scheme it does not know, in words, before it touches its other arguments"""
    from halo2_scaffold_amd import custom, engine, flex

    for good in ("shplonk", "gwc"):
        engine.check_multiopen(good)
    for call in (lambda: engine.check_multiopen("ipa"), lambda: flex.create_proof(None, None, None, 1, multiopen="ipa"),
                 lambda: custom.create_proof(None, None, None, 1, multiopen="GWC"), lambda: custom.prove_many(None, [], multiopen="bdfg21")):
        with pytest.raises(ValueError, match="multiopen must be one of"):
            call()


def test_lib_declares_the_gwc_symbols(h2):
    import ctypes as C

    from halo2_scaffold_amd import engine
    from halo2_scaffold_amd._lib import lib

    for name, nargs in (("h2mi_prover_gwc_num_points", 2), ("h2mi_prover_gwc_open", 3), ("h2mi_batch_gwc_num_points", 2), ("h2mi_batch_gwc_open", 3)):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs
    assert len(lib.h2mi_fr_gwc_witness_dev.argtypes) == 9
    assert engine.BUF_GWC_W == engine.BUF_LOGUP_PHI + 1 < engine.PKBUF_FIXED  # appended: the existing kinds keep their numbers
