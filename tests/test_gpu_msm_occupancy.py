"""The general MSM pipeline (csrc/h2mi_msm.hip: partition, per-bin sort, chunked accumulation, fold, finish with the hot-bucket
finishers, segment sums, weighted sum) at the bucket occupancies of tests/msm_occupancy_cases.py, compared stage by stage with that
file's plain-integer model.  The MSMs run in the hooks library (libh2mi_hooks.so: the product's objects and h2mi_dbg_msm_snapshot),
on base sets registered with their window width forced, which also keeps small sets on the general pipeline.  Per case and entry
form, all exact:
  1. the result is the model's group element, with and without h2mi_msm_set_canonical;
  2. h2mi_msm_last_stats reports the model's number of bucket insertions;
  3. the chunk length, the bucket offsets, the partials and fold tasks per bucket and both scans, entry nb included, word for word;
  4. the payloads of every bucket as a multiset (the order inside a bucket is arrival order);
  5. every bucket sum as a group element, the identity for an empty bucket; for wide windows also every segment's plain and local
     weighted sum;
  6. with the shift tried, the shift word.
A failure names the stage and the first bucket that differs.  Whether fold and finish ran on quads or on single lanes is inferred
from launch_tails' rule (M.lane_quad_batches), not observed: the batches only sit on both sides of it."""
import ctypes as C
import os

import numpy as np
import pytest

import msm_occupancy_cases as M
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

MSM_INORDER, MSM_GENERAL = 2, 4
Q = o.Q
R261 = 1 << 261


def limb_val(rows: np.ndarray) -> list:
    """the integers of (m, 9) rows of 29-bit limbs (tests/g1_29_edge_cases.py limb_val, row by row)"""
    from g1_29_edge_cases import limb_val as one

    return [one(r) for r in rows.tolist()]


class World:
    """the hooks library with the entry points this module calls, one handle per (points, window width), device buffers"""

    def __init__(self, L):
        vp, sz, u64 = C.c_void_p, C.c_size_t, C.c_uint64
        for name, args in (("h2mi_bases_register", [vp, sz, C.POINTER(u64)]), ("h2mi_bases_release", [u64]),
                           ("h2mi_msm_bn254_g1_dev", [u64, vp, sz, vp, vp]), ("h2mi_msm_bn254_g1_phase_dev", [u64, vp, sz, sz, vp, C.c_uint, vp]),
                           ("h2mi_msm_last_stats", [u64, C.POINTER(u64), C.POINTER(u64)]), ("h2mi_msm_set_canonical", [C.c_int]), ("h2mi_sync", []),
                           ("h2mi_malloc", [sz, C.POINTER(vp)]), ("h2mi_free", [vp]), ("h2mi_memcpy_h2d", [vp, vp, sz]), ("h2mi_memcpy_d2h", [vp, vp, sz]),
                           ("h2mi_stream_create", [C.POINTER(vp)]), ("h2mi_stream_destroy", [vp]),
                           ("h2mi_dbg_msm_snapshot", [u64, C.c_int, C.POINTER(u64), vp, sz, C.POINTER(sz)])):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = args, C.c_int
        self.L, self.handles, self.bufs, self.all = L, {}, {}, []

    def handle(self, n_reg, c):
        if (n_reg, c) not in self.handles:
            h = C.c_uint64()
            b = M.bases(n_reg)
            os.environ["H2MI_MSM_C"] = str(c)
            try:
                assert self.L.h2mi_bases_register(b.ctypes.data, n_reg, C.byref(h)) == 0
            finally:
                del os.environ["H2MI_MSM_C"]
            self.handles[(n_reg, c)] = h.value
        return self.handles[(n_reg, c)]

    def buf(self, key, nbytes):
        if key not in self.bufs or self.bufs[key][1] < nbytes:
            p = C.c_void_p()
            assert self.L.h2mi_malloc(nbytes, C.byref(p)) == 0
            self.bufs[key] = (p.value, nbytes)  # (an outgrown buffer is freed with the rest)
            self.all.append(p.value)
        return self.bufs[key][0]

    def upload(self, key, arr):
        arr = np.ascontiguousarray(arr)
        p = self.buf(key, arr.nbytes)
        assert self.L.h2mi_memcpy_h2d(p, arr.ctypes.data, arr.nbytes) == 0
        return p

    def release(self):
        assert self.L.h2mi_sync() == 0
        for h in self.handles.values():
            assert self.L.h2mi_bases_release(h) == 0
        for p in self.all:
            self.L.h2mi_free(p)
        self.handles, self.bufs, self.all = {}, {}, []


@pytest.fixture(scope="module")
def world(gpu, hooks):
    w = World(hooks)
    yield w
    w.release()


class Snapshot:
    def __init__(self, L, h, back=0):
        geo, need = (C.c_uint64 * 16)(), C.c_size_t()
        assert L.h2mi_dbg_msm_snapshot(h, back, geo, None, 0, C.byref(need)) == 0
        data = np.empty(need.value, dtype=np.uint32)
        assert L.h2mi_dbg_msm_snapshot(h, back, geo, data.ctypes.data, need.value, None) == 0
        (self.c, self.W, self.nb, self.lb, self.nbins, self.logNl, self.logNh, self.seg_log, self.n, self.stride, self.rows, self.has_sum, self.entries, self.slot,
         self.last_small, self.nseg) = [int(x) for x in geo]
        at = 0

        def take(words):
            nonlocal at
            at += words
            return data[at - words:at]

        tab = self.nb + 1
        self.s0 = int(take(1)[0])
        self.off, self.np0, self.np1, self.toff0, self.toff1 = (take(tab).astype(np.int64) for _ in range(5))
        self.vals = take(self.entries).astype(np.int64)
        self.shift = take(8).copy()
        self.dense = take(self.nb * M.PART_WORDS).reshape(self.nb, M.PART_WORDS)
        self.dense2 = take(self.nseg * M.PART_WORDS).reshape(self.nseg, M.PART_WORDS)
        self.vsum = take(self.nseg * M.PART_WORDS).reshape(self.nseg, M.PART_WORDS)
        assert at == need.value


def _first_diff(a, b):
    d = np.nonzero(np.asarray(a) != np.asarray(b))[0]
    return int(d[0]) if len(d) else None


def check_partials(rows, want: dict, points: dict, where, name_of):
    """rows: (m, 36) XYZZ partial sums; want: index -> multiple of the generator (absent: the identity); points: multiple -> affine
    (x, y) or None.  X = x ZZ, Y = y ZZZ and ZZ^3 = ZZZ^2 on the Montgomery-2^261 words; the identity is ZZ = 0."""
    live = np.nonzero((rows[:, 18:27] != 0).any(axis=1))[0].tolist()
    idx = sorted(set(live) | set(want))
    sub = rows[idx]
    X, Y, ZZ, ZZZ = (limb_val(sub[:, 9 * j:9 * j + 9]) for j in range(4))
    for j, i in enumerate(idx):
        p = points[want.get(i, 0)]
        if p is None:
            assert ZZ[j] % Q == 0, f"{where}: {name_of(i)} is not the identity (the model has {'no entry' if i not in want else 'a sum of zero'} there)"
            continue
        assert ZZ[j] % Q != 0, f"{where}: {name_of(i)} is the identity, the model's sum is not"
        assert (X[j] - p[0] * ZZ[j]) % Q == 0 and (Y[j] - p[1] * ZZZ[j]) % Q == 0 and (pow(ZZ[j], 3, Q) - ZZZ[j] * ZZZ[j] * R261) % Q == 0, (
            f"{where}: {name_of(i)} is not the model's group element")


def check_snapshot(case, snap, where):
    h, sm = M.model(case)
    g = h.geo
    assert (snap.c, snap.W, snap.nb, snap.lb, snap.nbins, snap.logNl, snap.logNh, snap.seg_log) == (g.c, g.W, g.nb, g.lb, g.nbins, g.logNl, g.logNh, g.seg_log), f"{where}: geometry"
    assert (snap.n, snap.stride, snap.rows, snap.has_sum, snap.last_small, snap.nseg) == (
        case.n_reg, h.stride, g.W, int(case.n_reg >= M.SHIFT_MIN_N), 0, (1 << M.MAT_LOG) if g.wide else 0), f"{where}: base set"
    name = lambda p: f"bucket {g.bucket_at(p)}" + (f" (position {p})" if g.wide else "")
    # 3. the tables
    assert snap.s0 == h.s0, f"{where}: check 3, chunk length {snap.s0}, model {h.s0}"
    for what, got, want in (("off", snap.off, h.off), ("np0", snap.np0, h.np0), ("np1", snap.np1, h.np1), ("toff0", snap.toff0, h.toff0), ("toff1", snap.toff1, h.toff1)):
        d = _first_diff(got, want)
        assert d is None, f"{where}: check 3, {what} of {name(d) if d < g.nb else 'entry nb'}: {int(got[d])}, model {int(want[d])}"
    assert snap.entries == h.entries
    # 4. the payloads, bucket by bucket
    pos = np.repeat(np.arange(g.nb), np.diff(snap.off))
    got = snap.vals[np.lexsort((snap.vals, pos))]
    d = _first_diff(got, h.payload)
    assert d is None, f"{where}: check 4, payloads of {name(int(pos[d]))}: {int(got[d]):#x}, model {int(h.payload[d]):#x}"
    # 5. the sums
    ints = {0, sm.result} | set(sm.bucket.values()) | set(sm.seg_p.values()) | set(sm.seg_v.values())
    ints = sorted(ints)
    points = dict(zip(ints, o.unpack_points(M.points_of(ints))))
    check_partials(snap.dense, sm.bucket, points, f"{where}: check 5", name)
    if g.wide:
        check_partials(snap.dense2, sm.seg_p, points, f"{where}: check 5, plain segment sums", lambda s: f"segment {s} (buckets {s * g.L} .. {s * g.L + g.L - 1})")
        check_partials(snap.vsum, sm.seg_v, points, f"{where}: check 5, local weighted segment sums", lambda s: f"segment {s} (buckets {s * g.L} .. {s * g.L + g.L - 1})")
    # 6. the shift
    if case.shifted:
        got_v = o.unpack(snap.shift.view(np.uint64), M.R)[0]
        assert got_v == h.v, f"{where}: check 6, shift {got_v:#x}, model {h.v:#x}"


def expected_point(case) -> bytes:
    return M.points_of([M.model(case)[1].result]).tobytes()


def run(world, cases, form="lib", check=True):
    """The MSMs of `cases` (one base set, one length, one H2MI_MSM_S0) through an entry form: "lib" / "stream" (h2mi_msm_bn254_g1_dev
    on the library stream / a stream of the caller's), "inorder" (the phase entry with H2MI_MSM_INORDER), "batch" (the phase entry with
    all of them at once: consecutive slots).  Checks 1 (as it is configured), 2 (the last one's) and 3 - 6 of every one."""
    from oracle import cref

    L = world.L
    first, m = cases[0], len(cases)
    assert len({(c.c, c.n_reg, c.n, c.s0_fixed) for c in cases}) == 1 and (m == 1 or form == "batch")
    h = world.handle(first.n_reg, first.c)
    n = first.n
    ptrs = [world.upload(("scalars", j), o.pack(list(c.scalars), M.R)) for j, c in enumerate(cases)]
    out = world.buf("out", 96 * 8)
    where = f"{' + '.join(c.id for c in cases)} [{form}]"
    st = C.c_void_p()
    if first.s0_fixed:
        os.environ["H2MI_MSM_S0"] = str(first.s0_fixed)
    try:
        if form == "lib":
            rc = L.h2mi_msm_bn254_g1_dev(h, ptrs[0], n, out, None)
        elif form == "stream":
            assert L.h2mi_stream_create(C.byref(st)) == 0
            rc = L.h2mi_msm_bn254_g1_dev(h, ptrs[0], n, out, st)
            assert L.h2mi_stream_destroy(st) == 0  # synchronises the stream
        else:
            arr = (C.c_void_p * m)(*ptrs)
            rc = L.h2mi_msm_bn254_g1_phase_dev(h, arr, m, n, out, MSM_GENERAL | (MSM_INORDER if form == "inorder" else 0), None)
        assert rc == 0, (where, rc)
        assert L.h2mi_sync() == 0
    finally:
        if first.s0_fixed:
            del os.environ["H2MI_MSM_S0"]
    # h2mi_sync above has launched this library's deferred reductions (the hooks library is linked to bind its own symbols: its
    # join is its own queue's) and waited for them
    jac = np.zeros((m, 12), dtype=np.uint64)
    assert L.h2mi_memcpy_d2h(jac.ctypes.data, out, 96 * m) == 0
    got = cref.normalize(jac)
    if check:
        ba = C.c_uint64()
        assert L.h2mi_msm_last_stats(h, C.byref(ba), None) == 0
        assert ba.value == M.model(cases[-1])[0].entries, f"{where}: check 2, bucket insertions {ba.value}, model {M.model(cases[-1])[0].entries}"
    snaps = []
    for j, c in enumerate(cases):
        snap = Snapshot(L, h, m - 1 - j) if check else None
        if check:
            check_snapshot(c, snap, f"{where}, MSM {j}" if m > 1 else where)
        snaps.append(snap)
        assert got[j].tobytes() == expected_point(c), f"{where}: check 1, MSM {j} is not the model's group element (checks 2 - 6 passed: the weighted bucket sum)"
    return jac, snaps


def run_canonical(world, case):
    """check 1 under h2mi_msm_set_canonical(1): the same group element, as the representative with Z = 1 (the identity: Z = 0)"""
    L = world.L
    assert L.h2mi_msm_set_canonical(1) == 0
    try:
        jac, _ = run(world, [case], "lib", check=False)
    finally:
        assert L.h2mi_msm_set_canonical(0) == 0
    z = o.limbs_to_int(jac[0, 8:12])
    assert z in (0, o.to_mont(1, Q)), f"{case.id}: canonical result with Z = {z:#x}"


CASES = M.cases()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_occupancy(world, case):
    """every case of families A - G through h2mi_msm_bn254_g1_dev on the library stream: checks 1 - 6, then check 1 again with
    canonical results"""
    run(world, [case])
    run_canonical(world, case)


PRINCIPAL = [c for c in CASES if c.principal]


@pytest.mark.parametrize("form", ["stream", "inorder"])
@pytest.mark.parametrize("case", PRINCIPAL, ids=[c.id for c in PRINCIPAL])
def test_occupancy_entry_forms(world, case, form):
    """the principal case of every family on a stream of the caller's and through the phase entry with H2MI_MSM_INORDER"""
    run(world, [case], form)


@pytest.mark.parametrize("family", list("ADFG"))
def test_occupancy_phase_batch(world, family):
    """four different cases of one family, one of them all-zero scalars (no entry at all), as one batch of the phase entry: the heads
    and accumulations of all four are one set of launches, their slots consecutive"""
    run(world, M.batch_family(family), "batch")


@pytest.mark.parametrize("c,n_reg,count,fold_quads,finish_quads", M.lane_quad_batches(), ids=lambda v: str(int(v)))
def test_occupancy_lane_and_quad_workers(world, c, n_reg, count, fold_quads, finish_quads):
    """Batches of full-length columns on both sides of the two 65536 rules by which launch_tails gives a fold task / a bucket's finish
    to a quad of lanes or to one lane: c = 15 at 8192 points, 1 and 2 MSMs (fold: quads, lanes; finish: lanes), c = 13, 2 and 3 MSMs
    (finish: quads, lanes; fold: quads).  The form is inferred from that rule as M.lane_quad_batches restates it, not observed."""
    run(world, list(M.lane_quad_cases(c, n_reg, count)), "batch")


def test_occupancy_ninth_msm_reuses_the_first_slot(world):
    """nine in-order MSMs on one handle, the first dense and the ninth with a single entry: the ninth runs in the first one's
    workspace slot, and every bucket the dense MSM filled reads np0 = 0 and the identity again"""
    dense, sparse = M.slot_reuse_pair()
    _, (first,) = run(world, [dense], "inorder")
    for _ in range(7):
        run(world, [dense], "inorder", check=False)
    _, (ninth,) = run(world, [sparse], "inorder")
    assert ninth.slot == first.slot, "eight slots per handle: the ninth MSM takes the first one's"
    assert int((ninth.np0 > 0).sum()) == 1 and int((first.np0 > 0).sum()) > 20
