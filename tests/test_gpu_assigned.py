"""Assigned cells on the device: h2mi_fr_batch_invert_dev / h2mi_fr_assigned_evaluate_dev word for word against Python integers at every
size and zero pattern of tests/assigned_cases.py; h2mi_fr_assigned_columns_dev with several columns and shuffled rows; and the prover
with H2MI_CELLS_RATIONAL columns against the same circuit with the resolved values in plain cells — equal proof bytes, equal device
columns, the route (host patch or device chain) read from the launch profile; the ABI's refusals."""
import ctypes as C
import random

import numpy as np
import pytest

import assigned_cases as A
import phase_cases as P
from oracle import bn254 as o
from oracle.vec import FV

pytestmark = pytest.mark.gpu

R = o.R
SRS_SECRET = 0x5EC2E7 + 0x48324D49
CHAIN = ("k_assigned_tile_products", "k_assigned_tile_inverses", "k_assigned_finish")
EINVAL, ERANGE = -1, -6


def _launches(gpu, call, names=CHAIN) -> dict:
    """kernel -> launches during call(), from the library's launch profile"""
    lib = gpu.lib
    assert lib.h2mi_profile_reset() == 0 and lib.h2mi_profile_filter(b"") == 0 and lib.h2mi_profile_enable(1) == 0
    try:
        call()
    finally:
        assert lib.h2mi_profile_enable(0) == 0
    ms, count = C.c_double(), C.c_uint64()
    out = {}
    for name in names + ("",):
        assert lib.h2mi_profile_query(name.encode(), C.byref(ms), C.byref(count)) == 0
        out[name] = count.value
    assert lib.h2mi_profile_reset() == 0
    assert out.pop("") > 0  # the profile did record this call's launches
    return out


NONE = dict.fromkeys(CHAIN, 0)
ONCE = dict.fromkeys(CHAIN, 1)


def _pairs(num_limbs, den_limbs):
    return np.ascontiguousarray(np.stack([num_limbs, den_limbs], axis=1).reshape(-1, 4))


def _all_below_r(limbs) -> bool:
    """every row of an (n, 4) limb array, read as a 256-bit integer, is below r (compared limb by limb from the top)"""
    r = [(R >> (64 * j)) & ((1 << 64) - 1) for j in range(4)]
    below, equal = np.zeros(len(limbs), dtype=bool), np.ones(len(limbs), dtype=bool)
    for j in (3, 2, 1, 0):
        below |= equal & (limbs[:, j] < np.uint64(r[j]))
        equal &= limbs[:, j] == np.uint64(r[j])
    return bool(below.all())


# ---- the vector kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", A.PATTERNS)
def test_vector_kernels_word_for_word(gpu, pattern):
    """every size of the list, out of place and (batch_invert) in place; the outputs are the canonical words: arrays compared, not residues"""
    lib = gpu.lib
    for n in A.SIZES:
        num, den, inv, cells = A.vector_case(pattern, n)
        num_l, den_l = o.pack(list(num), R), o.pack(list(den), R)
        d_den, d_pairs, d_out = gpu.DevBuf.from_numpy(den_l), gpu.DevBuf.from_numpy(_pairs(num_l, den_l)), gpu.DevBuf(32 * n)
        assert lib.h2mi_fr_batch_invert_dev(d_den.ptr, n, d_out.ptr, None) == 0
        assert np.array_equal(d_out.to_numpy(shape=(n, 4)), o.pack(list(inv), R)), (pattern, n, "batch_invert")
        assert np.array_equal(d_den.to_numpy(shape=(n, 4)), den_l)  # the input is left alone
        assert lib.h2mi_fr_assigned_evaluate_dev(d_pairs.ptr, n, d_out.ptr, None) == 0
        assert np.array_equal(d_out.to_numpy(shape=(n, 4)), o.pack(list(cells), R)), (pattern, n, "assigned_evaluate")
        assert lib.h2mi_fr_batch_invert_dev(d_den.ptr, n, d_den.ptr, None) == 0  # in place
        assert np.array_equal(d_den.to_numpy(shape=(n, 4)), o.pack(list(inv), R)), (pattern, n, "batch_invert in place")
        for b in (d_den, d_pairs, d_out):
            b.free()


def test_vector_kernels_beyond_one_workgroup_of_tile_products(gpu):
    """1025 tiles and three elements: every thread of pass (b) owns a run of tiles.  out[i] in[i] == 1 where in[i] != 0 and out[i] == 0
    elsewhere, through oracle.vec (no million Python inversions); zeros at both ends, at tile edges, a whole tile, scattered"""
    lib, n, T = gpu.lib, A.BIG_N, A.TILE
    den = np.ascontiguousarray(o.random_field_limbs(n, o.SEED + 71))
    num = np.ascontiguousarray(o.random_field_limbs(n, o.SEED + 72))
    zeros = [0, n - 1, T - 1, T, 512 * T, 513 * T - 1, 1024 * T, 1024 * T - 1] + list(range(700 * T, 701 * T)) + random.Random(5).sample(range(n), 200)
    den[zeros] = 0
    is_zero = ~den.any(axis=1)
    assert is_zero.sum() >= T + 8 and not is_zero[1] and not is_zero[n - 2]
    one = np.broadcast_to(o.pack([1], R), (n, 4))
    d_den, d_pairs, d_out = gpu.DevBuf.from_numpy(den), gpu.DevBuf.from_numpy(_pairs(num, den)), gpu.DevBuf(32 * n)
    launches = _launches(gpu, lambda: lib.h2mi_fr_batch_invert_dev(d_den.ptr, n, d_out.ptr, None))
    assert launches == ONCE  # one pass (b), hence one inversion, whatever n is
    inv = d_out.to_numpy(shape=(n, 4))
    assert not inv[is_zero].any()
    assert np.array_equal((FV(inv) * FV(den)).a[~is_zero], one[~is_zero])
    assert _all_below_r(inv)  # canonical words
    assert lib.h2mi_fr_assigned_evaluate_dev(d_pairs.ptr, n, d_out.ptr, None) == 0
    cells = d_out.to_numpy(shape=(n, 4))
    assert not cells[is_zero].any() and _all_below_r(cells)
    assert np.array_equal((FV(cells) * FV(den)).a[~is_zero], num[~is_zero])
    assert np.array_equal(cells, (FV(num) * FV(inv)).a)  # and word for word what the inverses give
    for b in (d_den, d_pairs, d_out):
        b.free()


def test_vector_kernels_refuse_bad_arguments(gpu):
    lib = gpu.lib
    buf = gpu.DevBuf.from_numpy(o.pack([1, 2, 3, 4], R))
    before = buf.to_numpy(shape=(4, 4))
    assert lib.h2mi_fr_batch_invert_dev(None, 0, None, None) == 0 and lib.h2mi_fr_assigned_evaluate_dev(None, 0, None, None) == 0  # n = 0: nothing happens
    assert lib.h2mi_fr_batch_invert_dev(None, 4, buf.ptr, None) == EINVAL and lib.h2mi_fr_batch_invert_dev(buf.ptr, 4, None, None) == EINVAL
    assert lib.h2mi_fr_batch_invert_dev(buf.ptr + 8, 2, buf.ptr, None) == EINVAL
    assert lib.h2mi_fr_assigned_evaluate_dev(None, 2, buf.ptr, None) == EINVAL and lib.h2mi_fr_assigned_evaluate_dev(buf.ptr, 2, buf.ptr, None) == EINVAL
    assert np.array_equal(buf.to_numpy(shape=(4, 4)), before)
    buf.free()


class _AssignedCells(C.Structure):
    _fields_ = [("d_column", C.c_void_p), ("rows", C.c_void_p), ("pairs", C.c_void_p), ("count", C.c_size_t)]


@pytest.mark.parametrize("canonical", [0, 1])
def test_several_columns_in_one_chain(gpu, canonical):
    """h2mi_fr_assigned_columns_dev: three columns — dense, rows in shuffled (unsorted) order, a single cell — staged behind one another;
    segment boundaries inside a tile and inside a thread's four elements; rows nobody assigned keep what they held"""
    lib = gpu.lib
    rng = random.Random(77 + canonical)
    n_rows = 6000
    counts = (A.TILE + 2, 2 * A.TILE + 1, 1)
    rows = [None, rng.sample(range(n_rows), counts[1]), [n_rows - 1]]
    filler = o.pack([0xF111], R)[0]
    arr, keep, cols, want = (_AssignedCells * 3)(), [], [], []
    for j, count in enumerate(counts):
        num, den, _, cells = A.vector_case("uniform", count)
        limbs = (lambda v: o.pack(list(v))) if canonical else (lambda v: o.pack(list(v), R))
        pairs = _pairs(limbs(num), limbs(den))
        col = gpu.DevBuf.from_numpy(np.tile(filler, (n_rows, 1)))
        expect = np.tile(filler, (n_rows, 1))
        r = np.array(rows[j], dtype=np.uint32) if rows[j] is not None else None
        expect[r if r is not None else np.arange(count)] = o.pack(list(cells), R)
        keep += [pairs, r]
        arr[j].d_column, arr[j].pairs, arr[j].count = col.ptr, pairs.ctypes.data, count
        arr[j].rows = r.ctypes.data if r is not None else None
        cols.append(col)
        want.append(expect)
    bad = C.c_uint64(99)
    launches = _launches(gpu, lambda: lib.h2mi_fr_assigned_columns_dev(arr, 3, canonical, C.byref(bad), None))
    assert launches == ONCE and bad.value == 0
    for col, expect in zip(cols, want):
        assert np.array_equal(col.to_numpy(shape=(n_rows, 4)), expect)
    if canonical:  # halves that are not below r are counted: a numerator and a denominator
        p0 = keep[0]
        p0[2], p0[5] = o.pack([R])[0], o.pack([(1 << 256) - 1])[0]
        assert lib.h2mi_fr_assigned_columns_dev(arr, 3, 1, C.byref(bad), None) == 0 and bad.value == 2
        assert lib.h2mi_fr_assigned_columns_dev(arr, 3, 1, None, None) == EINVAL
    assert lib.h2mi_fr_assigned_columns_dev(arr, 65, 0, C.byref(bad), None) == EINVAL and lib.h2mi_fr_assigned_columns_dev(None, 1, 0, C.byref(bad), None) == EINVAL
    assert lib.h2mi_fr_assigned_columns_dev(None, 0, 0, None, None) == 0
    for col in cols:
        col.free()


# ---- the prover -------------------------------------------------------------------------------------------------------------------
def _rows(view, n):
    return view.to_numpy(shape=(n, 4), nbytes=n * 32)


def _prove_both(gpu, custom, cs, rational, resolved, k, seed, multiopen="shplonk", keys=None, params=None):
    """the proof through rational cells and through plain cells holding the resolved values, same key, same seed
    -> (proof, launches of the rational proof, its H2MI_BUF_ADVICE columns); asserts equal bytes, equal advice columns word for word, and
    that the plain proof launched none of the new kernels"""
    from halo2_scaffold_amd import engine

    own = params is None
    params = params or gpu.ParamsKZG.setup(k, SRS_SECRET)
    keys = keys or custom.Keys(params, cs, rational if not callable(rational) else rational([None] * len(cs.challenge_phase)))
    ws = custom.Workspace(params, keys)
    n, na = 1 << k, cs.n_advice
    out = {}

    def run(which, asg):
        out[which] = custom.create_proof(params, keys, asg, seed, ws=ws, multiopen=multiopen)
        out[which + " advice"] = [_rows(v, n) for v in ws.prover.views(engine.BUF_ADVICE, na)]

    l_rat = _launches(gpu, lambda: run("rational", rational))
    l_plain = _launches(gpu, lambda: run("plain", resolved))
    assert l_plain == NONE
    assert out["rational"] == out["plain"]
    for a, b in zip(out["rational advice"], out["plain advice"]):
        assert np.array_equal(a, b)
    ws.release()
    if own:
        keys.release()
        params.release()
    return out["rational"], l_rat, out["rational advice"]


@pytest.mark.parametrize("x", [0, 0x1234567])
def test_is_zero_with_a_rational_inverse(gpu, x):
    """the reference's is_zero at k = 5 with value_inv = Rational(1, x): the short-run host path — no new kernel runs — and the bytes of
    the same circuit with the inverse computed by the caller; for x != 0 that is the reference's own witness"""
    from halo2_scaffold_amd import custom

    cs, asg = A.is_zero_circuit(custom, x)
    _, same = A.is_zero_circuit(custom, x, resolved=True)
    custom.mock(asg, 5)
    _, launches, advice = _prove_both(gpu, custom, cs, asg, same, 5, 31 + x % 7)
    assert launches == NONE
    assert o.unpack(advice[1][:2], R) == [pow(x, -1, R) if x else 0, 0]


@pytest.mark.parametrize("shape,count,want", [("dense", 16, NONE), ("dense", 17, ONCE), ("scattered", 4096, NONE), ("scattered", 4097, ONCE)])
def test_both_sides_of_each_threshold(gpu, shape, count, want):
    """a dense column of 16 / 17 cells, a scattered one of 4096 / 4097: the first of each rides in the phase's patch launch resolved on
    the host, the second goes through the device chain — read from the launch profile"""
    from halo2_scaffold_amd import custom

    k = 6 if shape == "dense" else A.BIG_K
    usable = (1 << k) - 6
    values = A.mixed_values(custom, count, (shape, count))
    cells = A.dense(values) if shape == "dense" else A.scattered(values, usable, count)
    cs, asg = A.columns_circuit(custom, [cells])
    _, same = A.columns_circuit(custom, [cells], resolved=True)
    _, launches, advice = _prove_both(gpu, custom, cs, asg, same, k, 3)
    assert launches == want, (shape, count, launches)
    got = o.unpack(advice[0][:usable], R)
    assert got == [same.advice[0].get(r, 0) for r in range(usable)]


def _three_columns(custom):
    usable = (1 << A.BIG_K) - 6
    dense = A.dense(A.mixed_values(custom, 5000, "dense three"))
    scat = A.scattered(A.mixed_values(custom, 4500, "scattered three"), usable, "three")
    plain = A.dense([v % R for v in range(7, 7 + 3000)])
    return [dense, scat, plain], usable


@pytest.mark.parametrize("multiopen", ["shplonk", "gwc"])
def test_three_columns_one_chain_one_inversion(gpu, multiopen):
    """k = 13: two rational columns beyond 4096 cells (one dense, one on shuffled rows) and a plain one; ONE pass (a), one inversion and
    one finish for both columns; both multi-openings"""
    from halo2_scaffold_amd import custom

    columns, usable = _three_columns(custom)
    cs, asg = A.columns_circuit(custom, columns)
    _, same = A.columns_circuit(custom, columns, resolved=True)
    assert asg.advice[2] == same.advice[2] and asg.advice[0] != same.advice[0]
    _, launches, advice = _prove_both(gpu, custom, cs, asg, same, A.BIG_K, 5, multiopen=multiopen)
    assert launches == ONCE, launches
    for j in range(3):
        assert o.unpack(advice[j][:usable], R) == [same.advice[j].get(r, 0) for r in range(usable)], j


def test_rational_column_in_the_second_phase(gpu):
    """tests/phase_cases.py's two-phase circuit with its phase-1 column handed over as rationals (the host path: its cells are not on
    rows 0 .. count - 1), and a two-phase circuit whose phase-1 column is long enough for the device chain"""
    from halo2_scaffold_amd import custom

    cs, synthesize = P.rlc_circuit(custom)

    def rational(challenges):
        asg = synthesize(challenges)
        rng = random.Random(9)
        for row, v in list(asg.advice[1].items()):
            d = rng.randrange(1, R)
            asg.advice[1][row] = custom.Rational(v * d, d)
        return asg

    probe = rational([5])
    assert all(isinstance(v, custom.Rational) for v in probe.advice[1].values()) and [v.evaluate() for v in probe.advice[1].values()] == list(synthesize([5]).advice[1].values())
    _, launches, _ = _prove_both(gpu, custom, cs, rational, synthesize, 5, 13)
    assert launches == NONE
    columns = [A.dense(A.mixed_values(custom, 30, "phase 0")), A.dense(A.mixed_values(custom, 40, "phase 1"))]
    cs, asg = A.columns_circuit(custom, columns, phases=[0, 1])
    _, same = A.columns_circuit(custom, columns, resolved=True, phases=[0, 1])
    _, launches, _ = _prove_both(gpu, custom, cs, asg, same, 6, 17)
    assert launches == {name: 2 for name in CHAIN}  # one chain per advice phase


def test_a_batch_of_two(gpu):
    from halo2_scaffold_amd import custom

    members = [[A.dense(A.mixed_values(custom, 40, ("batch", i))), A.scattered(A.mixed_values(custom, 9, ("batch s", i)), 58, i)] for i in range(2)]
    built = [A.columns_circuit(custom, m) for m in members]
    plain = [A.columns_circuit(custom, m, resolved=True)[1] for m in members]
    cs = built[0][0]
    params = gpu.ParamsKZG.setup(6, SRS_SECRET)
    keys = custom.Keys(params, cs, built[0][1])
    out = {}
    l_rat = _launches(gpu, lambda: out.update(rational=custom.prove_many(keys, [b[1] for b in built], seeds=[3, 40])))
    l_plain = _launches(gpu, lambda: out.update(plain=custom.prove_many(keys, plain, seeds=[3, 40])))
    assert out["rational"] == out["plain"]
    assert l_rat == {name: 2 for name in CHAIN} and l_plain == NONE  # every member resolves its own long column; the short ones on the host
    keys.release()
    params.release()


def test_a_key_with_rational_fixed_columns(gpu):
    """fixed columns as keygen's Assembly holds them before batch_invert_assigned: a long one (the device chain, once for the key) and a
    short one (the host); commitments, vk bytes and the resident fixed rows equal the plain key's; a proof under either key is the same"""
    from halo2_scaffold_amd import custom, engine

    k, n = 6, 64
    advice = [A.dense(A.mixed_values(custom, 20, "key advice"))]
    fixed = [A.dense(A.mixed_values(custom, 33, "key fixed")), A.scattered(A.mixed_values(custom, 5, "key fixed short"), 58, "key")]
    cs, asg = A.columns_circuit(custom, advice, fixed)
    _, same = A.columns_circuit(custom, advice, fixed, resolved=True)
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    made = {}
    l_rat = _launches(gpu, lambda: made.update(rational=custom.Keys(params, cs, asg)))
    l_plain = _launches(gpu, lambda: made.update(plain=custom.Keys(params, cs, same)))
    assert l_rat == ONCE and l_plain == NONE
    kr, kp = made["rational"], made["plain"]
    assert np.array_equal(kr.fixed_commitments, kp.fixed_commitments) and np.array_equal(kr.permutation_commitments, kp.permutation_commitments)
    assert kr.vk_bytes() == kp.vk_bytes() and kr.transcript_repr == kp.transcript_repr
    for a, b, cells in zip(kr.fixed_values, kp.fixed_values, same.fixed):
        assert np.array_equal(_rows(a, n), _rows(b, n))
        assert o.unpack(_rows(a, n), R) == [cells.get(r, 0) for r in range(n)]
    assert custom.create_proof(params, kr, asg, 21) == custom.create_proof(params, kp, same, 21)
    kr.release()
    kp.release()
    params.release()


@pytest.mark.parametrize("lookup_bits,want", [(4, NONE), (5, ONCE)])
def test_a_rational_lookup_table_column(gpu, lookup_bits, want):
    """the reference's range circuit (a `cs->lookups[]` key: keygen reads the table's fixed column on the host as well, to sort it) with
    the table column handed over as rationals — every value as a true fraction, zero as nonzero over zero: 16 cells (resolved on the
    host) and 32 (the device chain).  The key's commitments and fixed rows and a proof's bytes equal the plain key's; the proof
    depends on the sorted table, not only on the column"""
    import copy

    from halo2_scaffold_amd import engine, flex

    k, x, seed = 7, 0x0123456789ABCDEF, 23
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    cs = flex.FlexGateCS(lookup=True)
    asg = flex.range_closure(cs, x, lookup_bits)
    plain = flex.FlexKeys(params, cs, asg)
    rng = random.Random(lookup_bits)
    table = []
    for v in asg.table_values:
        d = rng.randrange(1, R)
        table.append(engine.Rational(v * d, d) if v else engine.Rational(rng.randrange(1, R), 0))
    assert [q.evaluate() for q in table] == asg.table_values
    fixed = list(asg.fixed)
    fixed[cs.col_table] = table
    index = {col: j for j, col in enumerate(cs.perm_columns)}
    copies = [(index[(left[0], left[1])], left[2], index[(right[0], right[1])], right[2]) for left, right in asg.copies]
    made = {}
    launches = _launches(gpu, lambda: made.update(keys=engine.Keys(cs.abi(k), params, fixed, copies)))
    assert launches == want
    rational = copy.copy(plain)  # the same front-end object over the other library key
    rational.keys = made["keys"]
    assert np.array_equal(rational.keys.fixed_commitments, plain.fixed_commitments)
    assert np.array_equal(rational.keys.permutation_commitments, plain.permutation_commitments)
    n = 1 << k
    for a, b in zip(rational.keys.views(engine.PKBUF_FIXED, cs.n_fixed), plain.fixed_values):
        assert np.array_equal(_rows(a, n), _rows(b, n))
    assert flex.create_proof(params, rational, asg, seed) == flex.create_proof(params, plain, asg, seed)
    rational.keys.release()
    plain.release()
    params.release()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_prover_usable(gpu):
    """H2MI_CELLS_RATIONAL on h2mi_prover_instances: H2MI_EINVAL; a canonical half that is not below r: H2MI_EINVAL, on the host path and
    on the device path, in either half; a cell at the first blinding row: H2MI_ERANGE.  After each the next plain proof has its bytes."""
    from halo2_scaffold_amd import custom, engine
    from halo2_scaffold_amd._lib import H2miError

    k = 6
    usable = (1 << k) - 6
    good = A.dense(A.mixed_values(custom, 40, "refusals"))
    meta = custom.ConstraintSystem()
    a = meta.advice_column()
    inst = meta.instance_column()
    s = meta.selector()
    meta.enable_equality(a)
    meta.create_gate("public", lambda meta: [meta.query_selector(s) * (meta.query_advice(a, custom.Rotation.cur()) - meta.query_instance(inst, custom.Rotation.cur()))])

    def assignment(cells, resolved=False):
        region = custom.Assignment(meta, instance=[4, 5])
        for row, v in cells.items():
            region.assign_advice(a, row, v.evaluate() if resolved and isinstance(v, custom.Rational) else v)
        return region

    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    keys = custom.Keys(params, meta, assignment(good))
    ws = custom.Workspace(params, keys)
    want = custom.create_proof(params, keys, assignment(good, resolved=True), 7, ws=ws)
    again = lambda: custom.create_proof(params, keys, assignment(good, resolved=True), 7, ws=ws)
    assert custom.create_proof(params, keys, assignment(good), 7, ws=ws) == want

    def refused(cells, code):
        with pytest.raises(H2miError) as e:
            custom.create_proof(params, keys, assignment(cells), 7, ws=ws)
        assert e.value.code == code
        assert again() == want

    def with_bad_half(count, at, half):
        cells = A.dense(A.mixed_values(custom, count, ("bad", count)))
        q = custom.Rational(3, 5)
        setattr(q, half, R if half == "numerator" else R + 1)  # past the constructor's reduction
        cells[at] = q
        return cells

    for count in (9, 40):  # the host path, the device path
        for half in ("numerator", "denominator"):
            refused(with_bad_half(count, count // 2, half), EINVAL)
    refused({usable: custom.Rational(1, 2)}, ERANGE)  # scattered, short
    refused(dict(A.dense(A.mixed_values(custom, usable + 1, "long"))), ERANGE)  # dense, into the blinding rows
    refused({**{2 * r: custom.Rational(1, 3) for r in range(20)}, usable: 1}, ERANGE)
    # public inputs are field elements
    pairs = np.ascontiguousarray(o.pack([4, 1, 5, 1]))
    column = (engine.ColumnCells * 1)()
    column[0].values, column[0].count = pairs.ctypes.data, 2
    for flags in (engine.CELLS_CANONICAL | engine.CELLS_RATIONAL, engine.CELLS_RATIONAL):
        column[0].flags = flags
        assert gpu.lib.h2mi_prover_instances(ws.prover.handle, column) == EINVAL
        assert again() == want  # a refusal leaves nothing behind
    ws.release()
    keys.release()
    params.release()
