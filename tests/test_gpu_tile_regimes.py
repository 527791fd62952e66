"""The one-workgroup tile-offset passes beyond 64 and beyond 1024 tiles (tests/tile_regime_cases.py; tests/test_tile_regimes_host.py
proves on the CPU that every size reaches the regime it is named for and that the vector references are the small Python-integer ones).

k_addscan_offsets through the logUp running sums (fraction route and ranked route), k_kate_offsets_multi through the multi-root
division and the GWC witness polynomials, k_cells_prefix through the key-file compaction, k_assigned_tile_inverses through a ranked sum
over a table of 65 tiles of distinct values; then whole proofs at k = 17, where the running sum and the divisions have 128 tiles.
All comparisons are exact: the stored words are canonical and equal the reference's.  Every test reads from the library's launch
profile that the middle pass ran, so a host shortcut cannot make it vacuous."""
import ctypes as C
import types

import numpy as np
import pytest

import extreme_cases
import gwc_cases
import key_file_cases as K
import tile_regime_cases as cases
from oracle import bn254 as o
from test_gpu_gwc import _call as _gwc_call
from test_gpu_gwc import _presum_launches, _slices
from test_gpu_table_logup import _Proving

pytestmark = pytest.mark.gpu

R = o.R


def _launches(gpu, names, call):
    """-> ({kernel: launches during call()}, call's result), from the library's launch profile"""
    lib = gpu.lib
    assert lib.h2mi_profile_reset() == 0 and lib.h2mi_profile_filter(b"") == 0 and lib.h2mi_profile_enable(1) == 0
    try:
        out = call()
    finally:
        assert lib.h2mi_profile_enable(0) == 0
    ms, count, found = C.c_double(), C.c_uint64(), {}
    for name in names:
        assert lib.h2mi_profile_query(name.encode(), C.byref(ms), C.byref(count)) == 0
        found[name] = count.value
    assert lib.h2mi_profile_reset() == 0
    return found, out


def _words(buf, rows):
    return buf.to_numpy(shape=(rows, 4), nbytes=rows * 32)


def _mont(values) -> np.ndarray:
    return np.ascontiguousarray(o.pack([v % R for v in values], R))


def _free(*bufs):
    for b in bufs:
        b.free()


def _check_sum(c, phi, sentinel, num, den, closes: bool):
    """rows 0 .. u by the recurrence, the rows beyond u the caller's"""
    u = c.u
    assert cases.sum_violation(phi, num, den, u) is None
    assert bool(phi[u].any()) != closes
    assert int(phi[1 : u + 1].any(axis=1).sum()) > u // 2
    assert np.array_equal(phi[u + 1 :], sentinel[u + 1 :])


# ---- (a) the additive scan behind the fractions ---------------------------------------------------------------------------------------
FRACTION_CASES = [("B-min", 1), ("B-full", 1), ("C-short", 1), ("C-even", 1), ("B-min", 6), ("C-short", 2)]


@pytest.mark.parametrize("size,K_sets", FRACTION_CASES, ids=[f"{s}-K{k}" for s, k in FRACTION_CASES])
def test_running_sum_of_fractions(gpu, size, K_sets):
    """plonk.logup_sum (one set) / plonk.logup_sum_sets (the sets 2^k rows apart) over a table of a few thousand distinct values: the
    recurrence on every usable row, phi[u] = 0 with the inputs' M and != 0 with one multiplicity bumped, a sentinel beyond row u"""
    from halo2_scaffold_amd import plonk

    c = cases.sum_case(size, K_sets)
    assert c.k == cases.smallest_k(cases.SIZES[size]) and cases.tiles_of(c.u) > cases.LANES
    k, n, u = c.k, c.n, c.u
    sentinel = cases.filler(n, 4242)
    d_a, d_t, d_m, d_phi = (gpu.DevBuf.from_numpy(a) for a in (np.concatenate(c.cols), c.table, c.m_col, sentinel))

    def run(d_mult):
        if K_sets == 1:
            return plonk.logup_sum(k, d_a, d_t, d_mult, c.beta, u, d_phi)
        return plonk.logup_sum_sets(k, d_a, K_sets, d_t, d_mult, c.beta, u, d_phi)

    ran, _ = _launches(gpu, ["k_addscan_local", "k_addscan_offsets", "k_addscan_apply"], lambda: run(d_m))
    assert ran == {"k_addscan_local": 1, "k_addscan_offsets": 1, "k_addscan_apply": 1}, ran
    num, den = cases.fraction_limbs(c.cols, c.table, c.m_col, c.beta, u)
    _check_sum(c, _words(d_phi, n), sentinel, num, den, closes=True)
    # multiplicities that do not belong to the inputs: the sum is what the recurrence says and does not return to zero
    wrong_m, wrong_num = cases.bumped(c, num)
    d_m2 = gpu.DevBuf.from_numpy(wrong_m)
    run(d_m2)
    _check_sum(c, _words(d_phi, n), sentinel, wrong_num, den, closes=False)
    _free(d_a, d_t, d_m, d_m2, d_phi)


# ---- (b) the additive scan behind the ranks -------------------------------------------------------------------------------------------
RANKED_CASES = [("B-min", 1, cases.TABLE_VALUES, False), ("B-min", 6, cases.TABLE_VALUES, False), ("B-min", 6, cases.TABLE_VALUES, True),
                ("B-min", 1, "u", False), ("C-short", 2, cases.TABLE_VALUES, False)]


@pytest.mark.parametrize("size,K_sets,n_unique,absent", RANKED_CASES, ids=[f"{s}-K{k}-nu{nu}" + ("-absent" if a else "") for s, k, nu, a in RANKED_CASES])
def test_running_sum_by_rank(gpu, size, K_sets, n_unique, absent):
    """plonk.sort_unique_first -> plonk.logup_rank_cols -> plonk.logup_sum_ranked: the sorted table, ranks, counts and M exactly, phi
    by the recurrence, and — where every input is a table value — byte for byte plonk.logup_sum_sets over the same columns.  One
    case has a single absent input in the last tile: its rank entry is unspecified, `missing` is 1 and the sum still closes.
    n_unique = u sends 65 tiles of distinct values through k_assigned_tile_inverses"""
    from halo2_scaffold_amd import plonk

    c = cases.sum_case(size, K_sets, n_unique, absent)
    rk = cases.ranked(c)
    k, n, u, nu = c.k, c.n, c.u, c.nu
    d_flat, d_table = gpu.DevBuf.from_numpy(np.concatenate(c.cols)), gpu.DevBuf.from_numpy(c.table)
    d_cols = [types.SimpleNamespace(ptr=d_flat.ptr + j * n * 32) for j in range(K_sets)]
    d_canon, d_mont, d_mult, d_first, got_nu = plonk.sort_unique_first(d_table, u)
    assert got_nu == nu
    assert np.array_equal(_words(d_canon, nu), rk.sorted) and np.array_equal(cases.from_mont(_words(d_mont, nu)), rk.sorted)
    assert np.array_equal(d_first.to_numpy(dtype=np.uint32, nbytes=4 * nu), rk.first)
    assert np.array_equal(d_mult.to_numpy(dtype=np.uint32, nbytes=4 * nu), np.bincount(c.s_idx[:u], minlength=nu)[rk.first])
    sentinel = cases.filler(n, 4343)
    d_m, d_phi = gpu.DevBuf.from_numpy(sentinel), gpu.DevBuf.from_numpy(sentinel)
    d_ranks = gpu.DevBuf.from_numpy(np.full(K_sets * n, 0xABABABAB, dtype=np.uint32))
    d_counts = gpu.DevBuf.from_numpy(np.full(nu, 0xCDCDCDCD, dtype=np.uint32))
    # ---- the ranking ----
    missing = plonk.logup_rank_cols(k, d_cols, d_canon, nu, d_first, u, d_ranks, d_counts, d_m)
    assert missing == len(c.absent) == int(absent)
    got_ranks = d_ranks.to_numpy(dtype=np.uint32).reshape(K_sets, n)
    for j in range(K_sets):
        here = c.present[j]  # an absent input's entry is unspecified
        assert np.array_equal(got_ranks[j, :u][here], rk.ranks[j][here]), j
        assert (got_ranks[j, u:] == 0xABABABAB).all()  # nothing is written for the blinding rows
    got_counts = d_counts.to_numpy(dtype=np.uint32)
    assert np.array_equal(got_counts, rk.counts) and int(got_counts.sum()) == K_sets * u - len(c.absent)
    got_m = _words(d_m, n)
    assert np.array_equal(got_m[:u], c.m_col[:u]) and np.array_equal(got_m[u:], sentinel[u:])
    # ---- the running sum ----
    names = ["k_addscan_offsets", "k_assigned_tile_inverses", "k_logup_gather", "k_logup_numden"]
    ran, _ = _launches(gpu, names, lambda: plonk.logup_sum_ranked(k, d_ranks, K_sets, d_mont, d_counts, d_first, nu, c.beta, u, d_phi))
    assert ran == {"k_addscan_offsets": 1, "k_assigned_tile_inverses": 1, "k_logup_gather": 1, "k_logup_numden": 0}, ran
    phi = _words(d_phi, n)
    num, den = cases.fraction_limbs(c.cols, c.table, c.m_col, c.beta, u, absent=c.absent)
    _check_sum(c, phi, sentinel, num, den, closes=True)  # an absent input adds to neither side: the sum still closes
    if not absent:  # every input is a table value: the fraction route over the columns, the table and M gives the same words
        d_phi2 = gpu.DevBuf.from_numpy(sentinel)
        plonk.logup_sum_sets(k, d_flat, K_sets, d_table, d_m, c.beta, u, d_phi2)
        assert d_phi2.to_numpy().tobytes() == phi.tobytes()
        d_phi2.free()
    _free(d_flat, d_table, d_canon, d_mont, d_mult, d_first, d_m, d_phi, d_ranks, d_counts)


# ---- (c) Kate division ----------------------------------------------------------------------------------------------------------------
KATE_CASES = [("C-short", 1), ("C-short", 4), ("C-even", 1), ("C-even", 4), ("B-full", 3)]
KATE_LAUNCHES = {"k_kate_local": 1, "k_kate_offsets": 1, "k_kate_finish": 1}  # one launch each, the roots in the grid


def _divide(gpu, d_num, n, roots, d_out):
    weights = extreme_cases.partial_fraction_weights(roots)
    rl, il, wl = _mont(roots), _mont([pow(r, -1, R) for r in roots]), _mont(weights)
    call = lambda: gpu.lib.h2mi_fr_kate_division_multi_dev(d_num.ptr, n, rl.ctypes.data, il.ctypes.data, wl.ctypes.data, len(roots), d_out.ptr, None)
    ran, rc = _launches(gpu, list(KATE_LAUNCHES), call)
    assert rc == 0 and ran == KATE_LAUNCHES, (rc, ran)


@pytest.mark.parametrize("size,m", KATE_CASES, ids=[f"{s}-m{m}" for s, m in KATE_CASES])
def test_division_by_the_roots_of_a_product(gpu, size, m):
    """h2mi_fr_kate_division_multi_dev on Q prod (X - r_i), 1 and r - 1 among the roots: the quotient is Q, the rest of the n - 1
    coefficients zero, coefficient n - 1 the caller's"""
    c = cases.kate_case(size, m)
    n = c.n
    assert n == cases.SIZES[size] and {1, R - 1} & set(c.roots)
    sentinel = cases.filler(n, 4444)
    d_num, d_out = gpu.DevBuf.from_numpy(c.num), gpu.DevBuf.from_numpy(sentinel)
    _divide(gpu, d_num, n, c.roots, d_out)
    got = _words(d_out, n)
    assert np.array_equal(got[: n - 1], c.want) and np.array_equal(got[n - 1], sentinel[n - 1])
    assert np.array_equal(_words(d_num, n), c.num)  # the numerator is unchanged
    _free(d_num, d_out)


@pytest.mark.parametrize("pattern", ["all r - 1", "random choice"])
def test_division_of_limb_extreme_words(gpu, pattern):
    """C-short on extreme_cases.EXTREME_WORDS as they lie, four roots at the extremes: sum_i c_i N / (X - r_i), the stated definition"""
    n = cases.SIZES["C-short"]
    roots = [1, R - 1, extreme_cases.TOP261, extreme_cases.OVER261]
    words = cases.extreme_words(pattern, n)
    d_num, d_out = gpu.DevBuf.from_numpy(words), gpu.DevBuf(32 * n)
    _divide(gpu, d_num, n, roots, d_out)
    got = _words(d_out, n - 1)
    assert cases.canonical(got) and np.array_equal(got, cases.kate_multi_reference(words, roots))
    _free(d_num, d_out)


# ---- (d) the GWC witness polynomials ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(cases.GWC_CASES))
def test_gwc_witness_polynomials(gpu, size):
    """h2mi_fr_gwc_witness_dev: at B-min five groups with the cap and one beyond it (the k_lincomb pre-sum runs), at C-short two groups
    of two terms, over shared pool polynomials; the linear combination and the division are the C oracle's"""
    c = cases.gwc_case(size)
    n, terms = c.n, c.terms
    d_pool = [gpu.DevBuf.from_numpy(p) for p in c.pool]
    sentinel = cases.filler(n, 4545)
    d_outs = [gpu.DevBuf.from_numpy(sentinel) for _ in terms]
    ptrs = [d_pool[i].ptr for grp in c.index for i in grp]
    names = ["k_gwc_local", "k_kate_offsets", "k_gwc_finish", "k_lincomb", "k_kate_local", "k_kate_finish"]
    ran, rc = _launches(gpu, names, lambda: _gwc_call(gpu.lib, ptrs, [s for grp in c.scalars for s in grp], terms, c.roots, n, [b.ptr for b in d_outs]))
    assert rc == 0
    slices = _slices(terms)
    assert ran == {"k_gwc_local": slices, "k_kate_offsets": slices, "k_gwc_finish": slices, "k_lincomb": _presum_launches(terms), "k_kate_local": 0,
                   "k_kate_finish": 0}, ran
    assert (ran["k_lincomb"] > 0) == (max(terms) > cases.GWC_CAP) == (size == "B-min")
    for g, want in enumerate(cases.gwc_reference(c)):
        got = _words(d_outs[g], n)
        assert np.array_equal(got, want), g
        assert not got[n - 1].any() and got[n - 2].any()  # coefficient n - 1 is written as zero
    _free(*d_pool, *d_outs)


# ---- (e) key-file compaction ----------------------------------------------------------------------------------------------------------
CELL_LAUNCHES = {"k_cells_count": 1, "k_cells_prefix": 1, "k_cells_compact": 1}


def _compact(gpu, columns, n_rows, limit, flags=0):
    ran, out = _launches(gpu, list(CELL_LAUNCHES), lambda: K.compact(gpu, columns, n_rows, limit, flags))
    assert ran == CELL_LAUNCHES, ran
    return out


@pytest.mark.parametrize("tiles", cases.CELL_TILES)
def test_compaction_beyond_one_round_of_tile_words(gpu, tiles):
    """h2mi_fr_compact_cells_dev on columns of 257, 512 and 513 tiles: cells at the tile ends around the round boundary in both widths,
    one cell in every 37th tile, a dense run of small integers up to the last row, one value outside 64 bits in the last tile"""
    n_rows, limit = tiles * cases.TILE, cases.cells_limit(tiles)
    assert cases.cell_rounds(tiles)[0] >= 2
    patterns = cases.cell_patterns(tiles)
    for name, col in patterns.items():
        assert _compact(gpu, [col], n_rows, limit) == [K.expect(col, limit)], name
    for flags in (2, 4):  # the forced row list; the forced 32-byte words
        assert _compact(gpu, [patterns["tile_ends"]], n_rows, limit, flags) == [K.expect(patterns["tile_ends"], limit, flags)], flags
    assert K.expect(patterns["wide_in_the_last_tile"], limit)[2:5] == (0, K.SPARSE, 32) and K.expect(patterns["dense_small"], limit)[3:5] == (K.DENSE, 8)


def test_compaction_of_four_columns_in_one_call(gpu):
    """3 tiles, 513 tiles, a column without cells, 300 tiles in ONE call: every column's tile offsets restart at zero, and nothing is
    written for the empty column"""
    tiles = [3, 513, 2, 300]
    every = lambda t, step: {tt * cases.TILE + (977 * tt) % (cases.TILE - 6): 1 + tt for tt in range(0, t, step)}
    columns = [every(3, 1), {**every(513, 1), **cases.cell_patterns(513)["tile_ends"]}, {}, every(300, 1)]
    n_rows, limits = [t * cases.TILE for t in tiles], [cases.cells_limit(t) for t in tiles]
    for flags in (0, 2):
        got = _compact(gpu, columns, n_rows, limits, flags)
        assert got == [K.expect(col, lim, flags) for col, lim in zip(columns, limits)], flags
        assert [g[0] for g in got] == [len(col) for col in columns] and len(columns[1]) > 513 and got[2] == (0, 0, 1, 0, 0, None, b"")


# ---- (f) whole proofs at 128 tiles ----------------------------------------------------------------------------------------------------
def test_whole_proofs_at_128_tiles(gpu):
    """a range-check circuit at k = 17 (LOOKUP_BITS 8) under a table-logUp key and under a program-logUp key, ended with SHPLONK and
    with GWC: the two routes' proofs are byte for byte equal, accepted by the verifier of their ending and rejected with the instance
    changed"""
    from halo2_scaffold_amd import flex

    t = _Proving(gpu, "q_lookup, k = 17", None)
    assert t.k == 17 and cases.regime(cases.tiles_of(t.keys.u)) == "B" and t.A == 1
    ws = flex.FlexWorkspace(t.params, t.keys)
    names = ["k_addscan_offsets", "k_logup_gather", "k_logup_numden", "k_kate_offsets", "k_gwc_local"]
    ran, proof = _launches(gpu, names, lambda: flex.create_proof(t.params, t.keys, t.asg, 33, ws=ws))
    assert ran["k_addscan_offsets"] == ran["k_logup_gather"] == t.A and ran["k_logup_numden"] == 0 and ran["k_kate_offsets"] >= 1 and ran["k_gwc_local"] == 0, ran
    ran, gwc = _launches(gpu, names, lambda: flex.create_proof(t.params, t.keys, t.asg, 33, ws=ws, multiopen="gwc"))
    assert ran["k_addscan_offsets"] == t.A and ran["k_gwc_local"] >= 1 and ran["k_kate_offsets"] == ran["k_gwc_local"], ran
    assert gwc[: len(proof) - 64] == proof[:-64] and gwc != proof
    # the program route: the same bytes from the fractions' running sum
    pkeys = t.program_keys()
    ppk = types.SimpleNamespace(keys=pkeys, transcript_repr=t.keys.transcript_repr)
    pws = flex.FlexWorkspace(t.params, ppk)
    ran, program_proof = _launches(gpu, names, lambda: flex.create_proof(t.params, ppk, t.asg, 33, ws=pws))
    assert ran["k_addscan_offsets"] == t.A and ran["k_logup_gather"] == 0, ran
    assert program_proof == proof
    assert flex.create_proof(t.params, ppk, t.asg, 33, ws=pws, multiopen="gwc") == gwc
    changed = [[(v + 1) % R for v in t.asg.instance]]
    assert t.verify(proof) and not t.verify(proof, changed)
    assert t.verify(gwc, ending=gwc_cases) and not t.verify(gwc, changed, ending=gwc_cases)
    assert not t.verify(gwc) and not t.verify(proof, ending=gwc_cases)  # the other ending is another proof
    pws.release()
    pkeys.release()
    ws.release()
    t.release()
