"""The MSM scheduler on the device (the host side of csrc/h2mi_msm.hip: take_small, msm_group, msm_small, msm_general, acquire_slot,
reduce_or_defer, flush_tails, msm_join_all, small_geometry) against tests/msm_schedule_cases.py: both sides of every edge of the
small-path geometry; the streaming rule, deterministically; every ordered pair of the eight kinds of call on one handle, so that
every workspace slot changes path, stream or form between one use and the next; one flush with all three kinds of deferred work,
and h2mi_msm_flush itself.  Every result is compared as a group element with the C oracle's MSM over the same limbs (exact), and
which path ran and when the reductions were launched is read from the library's launch profile and compared with the model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import msm_schedule_cases as S
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

MSM_INORDER, MSM_GENERAL = 2, 4
ONE = o.pack([1], o.R)[0]  # Montgomery 1: the weight that makes h2mi_fr_lincomb_dev a stream-ordered copy


class Profile:
    """with Profile(lib) as p: ... — afterwards p.names is every kernel launched inside, in issue order (h2mi_profile_dump)"""

    def __init__(self, lib):
        self.lib, self.names = lib, None

    def __enter__(self):
        lib = self.lib
        assert lib.h2mi_profile_reset() == 0 and lib.h2mi_profile_filter(b"") == 0 and lib.h2mi_profile_enable(1) == 0
        return self

    def __exit__(self, exc_type, exc, tb):
        lib = self.lib
        assert lib.h2mi_profile_enable(0) == 0
        if exc_type is None:
            need = C.c_size_t()
            assert lib.h2mi_profile_dump(None, 0, C.byref(need)) == 0
            buf = C.create_string_buffer(need.value)
            assert lib.h2mi_profile_dump(buf, need.value, None) == 0
            self.names = [line.split()[0] for line in buf.value.decode().splitlines()]
        assert lib.h2mi_profile_reset() == 0
        return False

    @property
    def heads(self):
        """the path of every group of MSMs, in issue order: a small-path group launches k_msm_small_digits once, a general one k_msm_bin_count"""
        return [S.SMALL if x == S.DIGITS else S.GENERAL for x in self.names if x in (S.DIGITS, S.BIN_COUNT)]

    @property
    def census(self):
        return {k: self.names.count(k) for k in S.CENSUS}


def _register(gpu, n, forced_c=0):
    h = C.c_uint64()
    b = S.bases(n)
    if forced_c:
        os.environ["H2MI_MSM_C"] = str(forced_c)
    try:
        assert gpu.lib.h2mi_bases_register(b.ctypes.data, n, C.byref(h)) == 0
    finally:
        if forced_c:
            del os.environ["H2MI_MSM_C"]
    return h.value


def _affine(jac):
    """(m, 12) Jacobian limbs -> m byte strings of affine limbs, what cases.expected returns"""
    from oracle import cref

    return [row.tobytes() for row in cref.normalize(np.ascontiguousarray(jac).reshape(-1, 12))]


class World:
    """what the tests of this module share on the device: handles, the pool columns of a size, scalar buffers; released at the end"""

    def __init__(self, gpu):
        self.gpu, self.lib = gpu, gpu.lib
        self.handles, self.pools, self.bufs = {}, {}, {}

    def handle(self, n):
        if n not in self.handles:
            self.handles[n] = _register(self.gpu, n)
        return self.handles[n]

    def pool(self, n):
        if n not in self.pools:
            self.pools[n] = {name: self.gpu.DevBuf.from_numpy(S.column(n, name)) for name in S.COLUMNS + (S.POISON,)}
        return self.pools[n]

    def buf(self, key, nbytes):
        if key not in self.bufs:
            self.bufs[key] = self.gpu.DevBuf(nbytes)
        return self.bufs[key]

    def copy(self, n, name, dst, stream):
        """column `name` of size n into the device buffer dst, as a kernel queued on `stream` (None: the library stream)"""
        src = (C.c_void_p * 1)(self.pool(n)[name].ptr)
        assert self.lib.h2mi_fr_lincomb_dev(src, ONE.ctypes.data, 1, n, dst.ptr, stream) == 0

    def release(self):
        assert self.lib.h2mi_sync() == 0
        for h in self.handles.values():
            assert self.lib.h2mi_bases_release(h) == 0
        for d in list(self.bufs.values()) + [b for p in self.pools.values() for b in p.values()]:
            d.free()
        self.handles, self.pools, self.bufs = {}, {}, {}


@pytest.fixture(scope="module")
def world(gpu):
    w = World(gpu)
    yield w
    w.release()


def run_schedule(world, n, ops):
    """Runs a schedule of cases (Call / Join / Flush) on the module's handle of n points.  The scalars of call k of a stream sit in
    group k mod 3 of that stream's ring of device buffers; directly after each call the buffers it read are overwritten, on the same
    stream, with the columns of the call that uses the group next (or with a column no MSM is meant to see): the digit and partition
    kernels are the only readers of the scalars.  Returns the affine results of every MSM and the launch profile."""
    lib, h = world.lib, world.handle(n)
    calls = [op for op in ops if isinstance(op, S.Call)]
    total = sum(len(c.entries) for c in calls)
    out = world.buf(("out", total), 96 * total)
    assert lib.h2mi_memset_zero(out.ptr, 96 * total) == 0
    per_stream = {False: [c for c in calls if not c.kind.caller_stream], True: [c for c in calls if c.kind.caller_stream]}
    st = C.c_void_p()
    if per_stream[True]:
        assert lib.h2mi_stream_create(C.byref(st)) == 0
    stream = {False: None, True: st.value}
    alive = st.value is not None
    ring = {}
    for own, cs in per_stream.items():
        width = max((len(c.entries) for c in cs), default=0)
        ring[own] = [[world.buf((n, own, g, j), n * 32) for j in range(width)] for g in range(3)]

    def fill(own, g, call):
        for j, d in enumerate(ring[own][g]):
            world.copy(n, call.entries[j][0] if call is not None and j < len(call.entries) else S.POISON, d, stream[own])

    try:
        for own, cs in per_stream.items():
            for g in range(min(3, len(cs))):
                fill(own, g, cs[g])
        # every schedule starts with no MSM counted on the handle, and with the result buffer cleared before a stream of the
        # caller's, which nothing orders behind the library stream, writes to it
        assert lib.h2mi_sync() == 0
        issued = {False: 0, True: 0}
        first = 0
        with Profile(lib) as prof:
            for op in ops:
                if isinstance(op, S.Flush):
                    assert lib.h2mi_msm_flush() == 0
                elif isinstance(op, S.Join):
                    if op.how == "h2mi_memcpy_d2h":
                        back = np.zeros(12, dtype=np.uint64)
                        assert lib.h2mi_memcpy_d2h(back.ctypes.data, out.ptr, 96) == 0
                    else:
                        assert getattr(lib, op.how)() == 0
                else:
                    kind, m, length = op.kind, len(op.entries), op.entries[0][1]
                    own = kind.caller_stream
                    k = issued[own]
                    issued[own] += 1
                    g = k % 3
                    flags = (MSM_GENERAL if kind.general else 0) | (MSM_INORDER if kind.inorder else 0)
                    if m == 1 and not flags:
                        rc = lib.h2mi_msm_bn254_g1_dev(h, ring[own][g][0].ptr, length, out.ptr + 96 * first, stream[own])
                    else:
                        ptrs = (C.c_void_p * m)(*[d.ptr for d in ring[own][g][:m]])
                        rc = lib.h2mi_msm_bn254_g1_phase_dev(h, ptrs, m, length, out.ptr + 96 * first, flags, stream[own])
                    assert rc == 0, (kind.name, first, rc)
                    first += m
                    fill(own, g, per_stream[own][k + 3] if k + 3 < len(per_stream[own]) else None)
            if alive:
                alive = False
                assert lib.h2mi_stream_destroy(st) == 0  # synchronises the stream
    finally:
        if alive:
            lib.h2mi_stream_destroy(st)
    return _affine(out.to_numpy(shape=(total, 12))), prof


def check_schedule(world, n, name, ops):
    """results against the oracle, MSM by MSM; the order of the head launches and the launch census against the model"""
    got, prof = run_schedule(world, n, ops)
    want = S.predict(n, ops)
    i = 0
    for op in ops:
        if isinstance(op, S.Call):
            for col, length in op.entries:
                assert got[i] == S.expected(n, col, length), (
                    f"{name} at {n} points: MSM {i} ({op.kind.name}, column {col} x {length}; model: {want.paths[i]} path, slot {want.slots[i]}) is not the oracle's group element")
                i += 1
    assert prof.heads == want.heads, f"{name} at {n} points: the paths taken, group by group"
    assert prof.census == want.census, f"{name} at {n} points: launch census"


def _slug(s):
    return re.sub(r"[^A-Za-z0-9]+", "_", s).strip("_")


# ---- 1. both sides of every edge of small_geometry -----------------------------------------------------------------------------------
@pytest.mark.parametrize("label,n", S.EDGE_SIZES, ids=[_slug(label) for label, _ in S.EDGE_SIZES])
def test_geometry_edge(gpu, label, n):
    """A base set on one side of an edge of the small-path geometry: uniform, witness-like and all-(r - 1) columns at full length and
    one point short (the ragged last workgroup of k_msm_small_accum and the tree over the G partial sums change shape here), each
    through the host-pointer entry, the device entry and a join, and the forced general pipeline on the same handle.  reduce_adds of
    the small path is G x lanes of the restated geometry: the size did sit on the side of the edge it was meant for."""
    lib = gpu.lib
    geo = S.small_geometry(n)
    h = _register(gpu, n)
    d_sc, d_out = gpu.DevBuf(n * 32), gpu.DevBuf(96)
    ptr = (C.c_void_p * 1)(d_sc.ptr)
    ba, ra = C.c_uint64(), C.c_uint64()
    digits = 0
    try:
        assert lib.h2mi_sync() == 0  # nothing an earlier test left deferred enters this census
        for col in ("uniform", "witness", "r-1"):
            for length in (n, n - 1):
                sc = np.ascontiguousarray(S.column(n, col)[:length])
                want = S.expected(n, col, length)
                where = f"{label}: column {col} x {length}"
                model = S.Scheduler()
                mh = model.register(n)
                model.host_msm(mh)
                model.msm(mh)
                model.join()
                model.msm(mh, general=True)
                model.join()
                d_sc.upload(sc)
                with Profile(lib) as prof:
                    out = np.zeros(12, dtype=np.uint64)
                    assert lib.h2mi_msm_bn254_g1(h, None, sc.ctypes.data, length, out.ctypes.data) == 0
                    assert _affine(out) == [want], f"{where}: host-pointer entry"
                    if geo.table:
                        assert lib.h2mi_msm_last_stats(h, C.byref(ba), C.byref(ra)) == 0
                        assert ra.value == geo.G * geo.lanes, f"{where}: reduce_adds after the host-pointer entry, G = {geo.G}, lanes = {geo.lanes}"
                    assert lib.h2mi_msm_bn254_g1_dev(h, d_sc.ptr, length, d_out.ptr, None) == 0 and lib.h2mi_join() == 0
                    assert _affine(d_out.to_numpy(shape=(12,))) == [want], f"{where}: device entry and join"
                    if geo.table:
                        assert lib.h2mi_msm_last_stats(h, C.byref(ba), C.byref(ra)) == 0
                        assert ra.value == S.small_reduce_adds(n) and 0 < ba.value <= length * 128, f"{where}: statistics after the device entry"
                    assert lib.h2mi_msm_bn254_g1_phase_dev(h, ptr, 1, length, d_out.ptr, MSM_GENERAL, None) == 0
                    assert _affine(d_out.to_numpy(shape=(12,))) == [want], f"{where}: H2MI_MSM_GENERAL on the same handle"
                path = S.SMALL if geo.table else S.GENERAL
                assert prof.heads == [g.path for g in model.groups] == [path, path, S.GENERAL], f"{where}: paths of the three entries"
                assert prof.census == {k: model.census[k] for k in S.CENSUS}, f"{where}: launch census"
                digits += prof.census[S.DIGITS]
        assert digits == (12 if geo.table else 0), f"{label}: k_msm_small_digits launches ({'none at all without the table' if not geo.table else 'two per column'})"
    finally:
        d_sc.free()
        d_out.free()
        assert lib.h2mi_bases_release(h) == 0  # the tables are up to 1.4 GB each


# ---- 2. the streaming rule ---------------------------------------------------------------------------------------------------------------
STREAMING = [(n, name) for n in S.STREAMING_SIZES for name in S.streaming_schedules(n)]


@pytest.mark.parametrize("n,name", STREAMING, ids=[f"{n}-{_slug(name)}" for n, name in STREAMING])
def test_streaming_rule_census(world, n, name):
    """take_small, deterministically: a handle with the table above 2^13 points takes the general pipeline once four MSMs were issued
    on it without a join — whatever their stream or flags —, the small path again after h2mi_join, h2mi_sync or h2mi_memcpy_d2h; a
    phase of nine is cut into groups of 4, 4, 1 and the path chosen per group; at 2^13 points nothing switches."""
    check_schedule(world, n, name, S.streaming_schedules(n)[name])


# ---- 3. every ordered pair of call kinds on one handle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.transition_schedules()), ids=lambda s: s.replace("->", "_then_"))
def test_transition(world, name):
    """eight MSMs of one kind, then eight of another, no join in between, on one 2^13-point handle (it has the table and never
    switches by itself): every slot is reused by the other path, stream or form while its previous MSM may still be in flight"""
    check_schedule(world, 1 << 13, name, S.transition_schedules(1 << 13)[name])


CROSSINGS = [name for name in S.transition_schedules() if len({S.KIND[x].general for x in name.split("->")}) == 2]


@pytest.mark.parametrize("name", CROSSINGS, ids=lambda s: s.replace("->", "_then_"))
def test_transition_across_paths_at_2_14(world, name):
    """the small -> general and general -> small pairs again at 2^14 points (6-bit windows, six cells per lane), where the streaming
    rule moves the small kinds to the general pipeline after their first four MSMs: the model says which"""
    check_schedule(world, 1 << 14, name, S.transition_schedules(1 << 14)[name])


# ---- 4. one flush, three kinds of deferred work; h2mi_msm_flush ------------------------------------------------------------------------
def test_one_flush_three_kinds(gpu, world):
    """Three handles — 300 points (small path), 20000 points (narrow windows, the sum point and the dominant-value shift), 20000 points
    registered with 18-bit windows (wide: the segment level) — queued round-robin on the library stream: every flush_tails sees the
    small path's pairs, narrow and wide bucket reductions together.  h2mi_msm_flush after the first round launches all three and
    returns 0 with nothing pending.  On the 20000-point handles round r takes the repeated-value column (shifted), the n - 5 prefix
    (no sum point, no shift) or a uniform column by (r mod 16) mod 3: slot 0 sees shift, no shift, shift in rounds 0, 8 and 16."""
    lib = gpu.lib
    N, ROUNDS = S.BASES_MAX, 17
    big = [("repeated", N), ("uniform", N), ("uniform", N - 5)]
    model = S.Scheduler()
    sizes = (300, N, N)
    mh = [model.register(300), model.register(N), model.register(N, forced_c=18)]
    hs = [_register(gpu, 300), _register(gpu, N), _register(gpu, N, forced_c=18)]
    out = gpu.DevBuf(96 * 3 * ROUNDS)
    try:
        cc = C.c_uint32()
        assert lib.h2mi_bases_info(hs[2], C.byref(cc), None, None, None) == 0 and cc.value == 18
        entry = lambda i, r: S.pool(300)[r % len(S.pool(300))] if i == 0 else big[((r + i - 1) % 16) % 3]
        assert [entry(1, r)[0:2] for r in (0, 8, 16)] == [big[0], big[2], big[0]]

        def queue(r):
            for i in range(3):
                col, length = entry(i, r)
                assert lib.h2mi_msm_bn254_g1_dev(hs[i], world.pool(sizes[i])[col].ptr, length, out.ptr + 96 * (3 * r + i), None) == 0
                model.msm(mh[i])

        def census_since(before):
            return {k: model.census[k] - before[k] for k in S.CENSUS}

        for n in set(sizes):
            world.pool(n)  # the uploads synchronise: none between the queued MSMs
        assert lib.h2mi_join() == 0
        with Profile(lib) as first:
            queue(0)
            assert lib.h2mi_msm_flush() == 0
        model.flush()
        assert first.census == census_since(dict.fromkeys(S.CENSUS, 0)) == {S.DIGITS: 1, S.BIN_COUNT: 2, S.ACCUM: 2, S.SMALL_PAIR: 1, S.FINAL: 2, S.SEG: 1}, (
            "one h2mi_msm_flush with a small-path pair, a narrow and a wide bucket reduction pending")
        with Profile(lib) as again:
            assert lib.h2mi_msm_flush() == 0, "h2mi_msm_flush with nothing pending"
        assert again.names == [], "h2mi_msm_flush with nothing pending launches nothing"
        before = dict(model.census)
        with Profile(lib) as rest:
            for r in range(1, ROUNDS):
                queue(r)
            assert lib.h2mi_join() == 0
        model.join()
        assert rest.census == census_since(before), "rounds 1 .. 16 and the join: launch census of the mixed flushes"
        assert rest.census[S.SMALL_PAIR] > 0 and rest.census[S.SEG] > 0 and rest.census[S.FINAL] > rest.census[S.SEG]
        full = sum(1 for r in range(ROUNDS) for i in (1, 2) if entry(i, r)[1] == N)
        assert (first.names + rest.names).count("k_msm_pick_shift") == full, "the dominant-value shift is tried by exactly the full-length MSMs of the 20000-point handles"
        got = _affine(out.to_numpy(shape=(3 * ROUNDS, 12)))
        for r in range(ROUNDS):
            for i, what in enumerate(("300 points, small path", "20000 points, narrow windows", "20000 points, 18-bit windows")):
                col, length = entry(i, r)
                assert got[3 * r + i] == S.expected(sizes[i], col, length), f"round {r}, {what}: column {col} x {length}"
    finally:
        assert lib.h2mi_sync() == 0
        out.free()
        for h in hs:
            assert lib.h2mi_bases_release(h) == 0
