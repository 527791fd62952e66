"""The small path of the MSM (csrc/h2mi_msm.hip, "small base sets") at the engineered digits, lane chains and tree levels of
tests/msm_small_cases.py, compared stage by stage with that file's plain-integer model.  The MSMs run in the hooks library
(libh2mi_hooks.so: the product's objects, h2mi_dbg_msm_small_snapshot and h2mi_dbg_msm_small_table) on base sets with known discrete
logarithms, each registered once for the module.  Per case and entry form, all exact, in this order:
  1. the geometry of the base set and of this MSM;
  2. every digit byte of the rows this MSM wrote (digits[w][i]);
  3. the additions of every workgroup (cnt[b]), the arrival counter (0 again) and h2mi_msm_last_stats' bucket_adds: the model's counts;
  4. every partial sum as a group element (part[b]), the identity where the model's sum is zero;
  5. the result as a group element; where asked for, its canonical form.
A failure names the stage and the first index that differs.  The table test reads chosen entries of the digit-multiples table."""
import ctypes as C

import numpy as np
import pytest

import msm_small_cases as M
import test_gpu_msm_occupancy as OT
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

MSM_INORDER, MSM_GENERAL = OT.MSM_INORDER, OT.MSM_GENERAL
EINVAL = -1
Q = o.Q
R261 = 1 << 261


class World(OT.World):
    """the occupancy suite's world with the small path's hooks; one handle per size, registered without a forced window width"""

    def __init__(self, L):
        super().__init__(L)
        vp, sz, u64 = C.c_void_p, C.c_size_t, C.c_uint64
        for name, args in (("h2mi_dbg_msm_small_snapshot", [u64, C.c_int, C.POINTER(u64), vp, sz, C.POINTER(sz)]), ("h2mi_dbg_msm_small_table", [u64, vp, sz, vp]),
                           ("h2mi_msm_bn254_g1", [u64, vp, vp, sz, vp]), ("h2mi_join", [])):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = args, C.c_int

    def handle(self, n_reg):
        if n_reg not in self.handles:
            h = C.c_uint64()
            b = M.bases(n_reg)
            assert self.L.h2mi_bases_register(b.ctypes.data, n_reg, C.byref(h)) == 0
            self.handles[n_reg] = h.value
        return self.handles[n_reg]


@pytest.fixture(scope="module")
def world(gpu, hooks):
    w = World(hooks)
    yield w
    w.release()


class Snapshot:
    def __init__(self, L, h, back=0):
        geo, need = (C.c_uint64 * 16)(), C.c_size_t()
        rc = L.h2mi_dbg_msm_small_snapshot(h, back, geo, None, 0, C.byref(need))
        assert rc == 0, f"h2mi_dbg_msm_small_snapshot: {rc} (the MSM did not take the small path?)"
        data = np.empty(need.value, dtype=np.uint8)
        assert L.h2mi_dbg_msm_small_snapshot(h, back, geo, data.ctypes.data, need.value, None) == 0
        self.c, self.W, self.lanes, self.r, self.sG, self.n_reg, self.n, self.G, self.slot = [int(x) for x in geo[:9]]
        at = 0

        def take(nbytes):
            nonlocal at
            at += nbytes
            return data[at - nbytes:at]

        self.cnt = take(4 * (self.sG + 1)).view(np.uint32).astype(np.int64)
        self.part = take(4 * M.PART_WORDS * self.G).view(np.uint32).reshape(self.G, M.PART_WORDS)
        self.dig = take(self.W * self.n_reg).reshape(self.W, self.n_reg)
        assert at == need.value


def check_snapshot(case, snap, where):
    m = M.model_of(case)
    g = m.geo
    # 1. geometry
    assert (snap.c, snap.W, snap.lanes, snap.r, snap.sG, snap.n_reg, snap.n, snap.G) == (g.c, g.W, g.lanes, g.r, g.G, case.n_reg, case.n, m.G), f"{where}: check 1, geometry"
    # 2. digits
    got = snap.dig[:, :case.n]
    diff = np.argwhere(got != m.digits)
    if len(diff):
        w, i = (int(x) for x in diff[0])
        raise AssertionError(f"{where}: check 2, digits[{w}][{i}] = {int(got[w, i]):#04x}, model {int(m.digits[w, i]):#04x} (scalar {case.scalars[i]:#x})")
    # 3. counts
    d = OT._first_diff(snap.cnt[:m.G], m.cnt)
    assert d is None, f"{where}: check 3, cnt[{d}] = {int(snap.cnt[d])}, model {m.cnt[d]}"
    assert snap.cnt[snap.sG] == 0, f"{where}: check 3, the arrival counter is {int(snap.cnt[snap.sG])} after the MSM"
    # 4. partial sums
    ints = sorted({0, m.result} | set(m.part))
    points = dict(zip(ints, o.unpack_points(M.points_of(ints))))
    OT.check_partials(snap.part, {b: v for b, v in enumerate(m.part) if v}, points, f"{where}: check 4", lambda b: f"part[{b}]")


def expected_point(case) -> bytes:
    return M.points_of([M.model_of(case).result]).tobytes()


def run(world, cases, form="lib", check=True, general=False):
    """The MSMs of `cases` (one base set, one length) through an entry form: "host" (h2mi_msm_bn254_g1 with the handle), "lib" / "stream"
    (h2mi_msm_bn254_g1_dev on the library stream / a stream of the caller's), "inorder" (the phase entry with H2MI_MSM_INORDER), "phase"
    (the phase entry with all of them at once: consecutive slots).  `general`: H2MI_MSM_GENERAL, the result alone."""
    from oracle import cref

    L = world.L
    first, m = cases[0], len(cases)
    assert len({(c.n_reg, c.n) for c in cases}) == 1 and (m == 1 or form == "phase") and not (general and check)
    h = world.handle(first.n_reg)
    n = first.n
    where = f"{' + '.join(c.id for c in cases)} [{form}{', general' if general else ''}]"
    cols = [o.pack(list(c.scalars), M.R) for c in cases]
    out = world.buf("out", 96 * 16)
    jac = np.zeros((m, 12), dtype=np.uint64)
    if form == "host":
        rc = L.h2mi_msm_bn254_g1(h, None, cols[0].ctypes.data, n, jac.ctypes.data)
    else:
        ptrs = [world.upload(("scalars", j), col) for j, col in enumerate(cols)]
        st = C.c_void_p()
        if form == "lib" and not general:
            rc = L.h2mi_msm_bn254_g1_dev(h, ptrs[0], n, out, None)
        elif form == "stream":
            assert L.h2mi_stream_create(C.byref(st)) == 0
            rc = L.h2mi_msm_bn254_g1_dev(h, ptrs[0], n, out, st)
            assert L.h2mi_stream_destroy(st) == 0  # synchronises the stream
        else:
            arr = (C.c_void_p * m)(*ptrs)
            rc = L.h2mi_msm_bn254_g1_phase_dev(h, arr, m, n, out, (MSM_GENERAL if general else 0) | (MSM_INORDER if form == "inorder" else 0), None)
    assert rc == 0, (where, rc)
    assert L.h2mi_sync() == 0
    if form != "host":
        assert L.h2mi_memcpy_d2h(jac.ctypes.data, out, 96 * m) == 0
    got = cref.normalize(jac)
    snaps = []
    if check:
        ba = C.c_uint64()
        assert L.h2mi_msm_last_stats(h, C.byref(ba), None) == 0
        snaps = [Snapshot(L, h, m - 1 - j) for j in range(m)]
        for j, c in enumerate(cases):
            check_snapshot(c, snaps[j], f"{where}, MSM {j}" if m > 1 else where)
        want = M.model_of(cases[-1]).entries
        assert ba.value == want, f"{where}: check 3, bucket_adds {ba.value}, model {want}"
    for j, c in enumerate(cases):
        assert got[j].tobytes() == expected_point(c), f"{where}: check 5, MSM {j} is not the model's group element" + (" (checks 1 - 4 passed: the second tree)" if check else "")
    return jac, snaps


def run_canonical(world, case):
    """check 5 under h2mi_msm_set_canonical(1): the same group element as the representative with Z = 1 (the identity: Z = 0)"""
    L = world.L
    assert L.h2mi_msm_set_canonical(1) == 0
    try:
        jac, _ = run(world, [case], "lib", check=False)
    finally:
        assert L.h2mi_msm_set_canonical(0) == 0
    z = o.limbs_to_int(jac[0, 8:12])
    assert z == (0 if M.model_of(case).result == 0 else o.to_mont(1, Q)), f"{case.id}: canonical result with Z = {z:#x}"


CASES = M.cases()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_small(world, case):
    """every case through h2mi_msm_bn254_g1_dev on the library stream: checks 1 - 5, then the result again in canonical form and
    through the general pipeline on the same handle"""
    run(world, [case])
    run_canonical(world, case)
    run(world, [case], "lib", check=False, general=True)


PRINCIPAL = [c for c in CASES if c.principal]


@pytest.mark.parametrize("form", ["host", "stream", "inorder", "phase"])
@pytest.mark.parametrize("case", PRINCIPAL, ids=[c.id for c in PRINCIPAL])
def test_small_entry_forms(world, case, form):
    """the principal cases through the host-pointer entry, on a stream of the caller's, through the phase entry with
    H2MI_MSM_INORDER, and as the first of two columns of the phase entry (the second all zero): checks 1 - 5"""
    zero = M.Case("all-zero", case.family, case.n_reg, (0,) * case.n, {})
    run(world, [case, zero] if form == "phase" else [case], form)


@pytest.mark.parametrize("n_reg", M.SIZES)
def test_small_table_entries(world, n_reg):
    """for the chosen (window, point) pairs of the size's table: every multiple j = 1 .. 2^(c-1) is (j 2^(c w) m_i mod r) G, in the
    table's canonical Montgomery-2^261 words; the identity base's entries are all zeros"""
    L = world.L
    one = M.Case("one", "table", n_reg, (1,), {})
    run(world, [one])  # the table is read through the handle's last small-path MSM
    h = world.handle(n_reg)
    g = M.small_geometry(n_reg)
    js = range(1, (1 << (g.c - 1)) + 1)
    keys = [(j, w, i) for w, i in M.table_samples(n_reg) for j in js]
    idx = np.array([M.table_entry(n_reg, *k) for k in keys], dtype=np.uint64)
    words = np.zeros((len(keys), 16), dtype=np.uint32)
    assert L.h2mi_dbg_msm_small_table(h, idx.ctypes.data, len(keys), words.ctypes.data) == 0
    beyond = np.array([g.table_bytes // 64], dtype=np.uint64)
    assert L.h2mi_dbg_msm_small_table(h, beyond.ctypes.data, 1, words.ctypes.data) == -6  # H2MI_ERANGE (nothing copied)
    ks = [M.table_log(n_reg, *k) for k in keys]
    want = o.unpack_points(M.points_of(ks))
    rinv = pow(R261, -1, Q)
    for key, row, p, k in zip(keys, words.tolist(), want, ks):
        x, y = (sum(v << (32 * t) for t, v in enumerate(row[8 * half:8 * half + 8])) for half in (0, 1))
        name = f"table[j = {key[0]}][w = {key[1]}][i = {key[2]}] of {n_reg} points"
        if p is None:
            assert x == 0 and y == 0, f"{name} is not the identity"
        else:
            assert x < Q and y < Q and (x * rinv % Q, y * rinv % Q) == p, f"{name} is not {k:#x} G"


def test_small_snapshot_hooks_tell_the_paths_apart(world):
    """after a small-path MSM the general hook refuses the slot, after a general one on the same handle the small hook does"""
    L = world.L
    case = M.Case("one", "table", M.N_TREE, (1, 2, 3), {})
    h = world.handle(M.N_TREE)
    geo, need = (C.c_uint64 * 16)(), C.c_size_t()
    run(world, [case])
    assert L.h2mi_dbg_msm_snapshot(h, 0, geo, None, 0, C.byref(need)) == EINVAL
    run(world, [case], check=False, general=True)
    assert L.h2mi_dbg_msm_small_snapshot(h, 0, geo, None, 0, C.byref(need)) == EINVAL
    assert L.h2mi_dbg_msm_snapshot(h, 0, geo, None, 0, C.byref(need)) == 0
    assert L.h2mi_dbg_msm_small_snapshot(h, 1, geo, None, 0, C.byref(need)) == 0  # the slot before still holds the small one


# ---- state that survives between the MSMs of one slot -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_reg", M.STATE_SIZES)
def test_small_prefix_after_full_in_the_same_slot(world, n_reg):
    """a full-length MSM with every digit live, then as many MSMs as bring the ring back to its slot, the last a prefix MSM (n_reg - 1,
    half, 1 points: fewer workgroups, shorter rows): the prefix meets the full column's digits beyond n, its partial sums and counts
    beyond G and the arrival counter it reset, and checks 1 - 5 hold for it"""
    full = M.full_column(n_reg)
    filler = M.Case("filler", "state", n_reg, (3, 0, 5), {})
    for prefix in M.prefix_columns(n_reg):
        _, (first,) = run(world, [full])
        for _ in range(M.NSLOT - 1):
            run(world, [filler], check=False)
        _, (again,) = run(world, [prefix])
        assert again.slot == first.slot, "eight slots per handle: the ninth MSM takes the first one's"
        mp, mf = M.model_of(prefix), M.model_of(full)
        if prefix.n < n_reg:  # what the prefix MSM did not write is still the full column's
            assert (again.dig[:, prefix.n:] == mf.digits[:, prefix.n:]).all()
        assert (again.cnt[mp.G:mf.G] == mf.cnt[mp.G:]).all()


def test_small_phase_batch_of_four(world):
    """four columns, one all zero, as one batch of the phase entry: one launch of k_msm_small_digits_b, consecutive slots"""
    run(world, M.phase_columns(M.N_TREE), "phase")


def _issue(world, case, key):
    """one deferred MSM on the library stream: (handle, where its result goes)"""
    L = world.L
    h = world.handle(case.n_reg)
    out = world.buf(("out", key), 96)
    assert L.h2mi_msm_bn254_g1_dev(h, world.upload(("scalars", key), o.pack(list(case.scalars), M.R)), case.n, out, None) == 0
    return h, out


def _result(world, out) -> bytes:
    from oracle import cref

    jac = np.zeros((1, 12), dtype=np.uint64)
    assert world.L.h2mi_memcpy_d2h(jac.ctypes.data, out, 96) == 0
    return cref.normalize(jac)[0].tobytes()


def test_small_one_launch_with_members_of_different_size(world):
    """three columns of the phase entry on one handle and one MSM on a larger one, all deferred to one join: the four accumulate +
    finish pairs are ONE launch over the larger handle's workgroups, in which the smaller members' surplus workgroups return"""
    L = world.L
    assert L.h2mi_sync() == 0
    three, (big,) = M.phase_columns(M.N_TREE, 3), M.phase_columns(M.N_L256, 1)
    h = world.handle(M.N_TREE)
    ptrs = [world.upload(("scalars", j), o.pack(list(c.scalars), M.R)) for j, c in enumerate(three)]
    out = world.buf("out", 96 * 16)
    assert L.h2mi_msm_bn254_g1_phase_dev(h, (C.c_void_p * 3)(*ptrs), 3, M.N_TREE, out, 0, None) == 0
    hb, outb = _issue(world, big, "big")
    assert L.h2mi_join() == 0 and L.h2mi_sync() == 0
    for j, c in enumerate(three):
        check_snapshot(c, Snapshot(L, h, 2 - j), f"{c.id} [three + one]")
        assert _result(world, out + 96 * j) == expected_point(c), c.id
    check_snapshot(big, Snapshot(L, hb, 0), f"{big.id} [three + one]")
    assert _result(world, outb) == expected_point(big)


def test_small_nine_deferred_before_one_join(world):
    """nine MSMs of different lengths (different G) on the library stream before one join: reduce_or_defer launches them in fours (half
    the slots), the ninth at the join, in the first one's slot; every result, and checks 1 - 4 on the eight slots that still hold
    their MSM.  (A launch of more than SMALL_BATCH = 8 members cannot be built through the ABI: at most three are deferred when a
    phase group of four arrives.)"""
    L = world.L
    assert L.h2mi_sync() == 0
    nine = M.nine_columns(M.N_TREE)
    issued = [_issue(world, c, j) for j, c in enumerate(nine)]
    assert L.h2mi_join() == 0 and L.h2mi_sync() == 0
    for j, (c, (h, out)) in enumerate(zip(nine, issued)):
        assert _result(world, out) == expected_point(c), f"{c.id}: check 5"
        if j:
            check_snapshot(c, Snapshot(L, h, 8 - j), f"{c.id} [nine deferred]")
    ba = C.c_uint64()
    assert L.h2mi_msm_last_stats(issued[-1][0], C.byref(ba), None) == 0 and ba.value == M.model_of(nine[-1]).entries
