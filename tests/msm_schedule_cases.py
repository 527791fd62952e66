"""The MSM scheduler of csrc/h2mi_msm.hip (take_small, msm_group, msm_small, msm_general, acquire_slot, reduce_or_defer, flush_tails,
msm_join_all, small_geometry), shared by tests/test_msm_schedule_host.py and tests/test_gpu_msm_schedule.py: a restatement of the
small-path geometry and of what register_dev derives from it, the sizes on the two sides of every edge of that geometry, a model
of what the scheduler lets an observer see (the path and the slot of every MSM, the launches of the kernels that tell the paths and
the reductions apart), the eight kinds of call, the schedules built from them, and the scalar columns every schedule draws from.
Every comparison made with these is exact: group elements against oracle/cref.py, launch counts against the model."""
import functools
from collections import Counter
from typing import NamedTuple

import numpy as np

from oracle import bn254 as o

# ---- the constants of csrc/h2mi_msm.hip, restated ---------------------------------------------------------------------------------
SMALL_MAX_N = 1 << 14  # base sets up to here may get the digit-multiples table
SMALL_C_MAX = 7  # widest window of the small path
SMALL_CELLS = 128  # gathering lanes per workgroup while there are at most 128 x 256 cells
SMALL_THREADS = 256  # beyond: every lane gathers
SMALL_PARTS_MAX = 512  # workgroups (= partial sums) of one small-path MSM
SMALL_TABLE_BUDGET = 2 << 30  # bytes of the table per base set
SMALL_STREAM_N = 1 << 13  # above this many points a handle with the table ...
SMALL_STREAM_AFTER = 4  # ... takes the general pipeline once this many MSMs were issued without a join
HEAD_BATCH = 4  # MSMs whose heads run as one set of launches
HEAD_BATCH_MAX_N = 1 << 17  # largest base set the phase entry batches
NSLOT = 8  # workspace slots per handle up to 2^17 points (four above)
SMALL_BATCH = TAIL_BATCH = 8  # reductions one launch takes
WIDE_MIN_C, WIDE_MAX_C = 18, 20  # window widths whose bucket reduction has the segment level (k_msm_seg)

# the kernels the census counts: one head launch per group tells the path, one reduction launch per batch tells when it ran
DIGITS, BIN_COUNT, ACCUM = "k_msm_small_digits", "k_msm_bin_count", "k_msm_accum"
SMALL_PAIR, FINAL, SEG = "k_msm_small_accum", "k_msm_final", "k_msm_seg"
CENSUS = (DIGITS, BIN_COUNT, ACCUM, SMALL_PAIR, FINAL, SEG)
SMALL, GENERAL = "small", "general"


def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


# ---- small_geometry and register_dev ----------------------------------------------------------------------------------------------
class Geometry(NamedTuple):
    n: int
    table: bool  # the base set gets the digit-multiples table at all
    c: int  # window bits
    W: int  # windows: ceil(255 / c)
    lanes: int  # gathering lanes per workgroup
    r: int  # cells per lane
    G: int  # workgroups = partial sums of an MSM over all n points
    table_bytes: int


def small_geometry(n: int) -> Geometry:
    """what small_geometry chooses for a base set of n points and what register_dev derives from it (sW, sG, the table's size)"""
    if n > SMALL_MAX_N:
        return Geometry(n, False, 0, 0, 0, 0, 0, 0)
    c = SMALL_C_MAX
    while c > 2 and (1 << (c - 1)) * _ceil_div(255, c) * n * 64 > SMALL_TABLE_BUDGET:
        c -= 1
    W = _ceil_div(255, c)
    cells = n * W
    lanes, r = SMALL_CELLS, 1
    if cells > SMALL_CELLS * 256:
        lanes, r = SMALL_THREADS, _ceil_div(cells, SMALL_THREADS * SMALL_PARTS_MAX)
    return Geometry(n, True, c, W, lanes, r, _ceil_div(cells, lanes * r), (1 << (c - 1)) * W * n * 64)


def small_reduce_adds(n_registered: int) -> int:
    """reduce_adds of h2mi_msm_last_stats after a small-path MSM: the trees of sG workgroups of `lanes` lanes, then over the sG sums"""
    g = small_geometry(n_registered)
    return g.G * g.lanes


def _edge(name: str, changed) -> tuple:
    """(largest n on one side, smallest on the other) of the one place in 1 .. SMALL_MAX_N + 1 where changed(before, after) holds"""
    at = [n for n in range(1, SMALL_MAX_N + 1) if changed(small_geometry(n), small_geometry(n + 1))]
    assert len(at) == 1, (name, at)
    return at[0], at[0] + 1


# every edge of the geometry: the sizes are computed from the restatement above, never typed in
EDGE_N = {
    "lanes 128 to 256": _edge("lanes", lambda a, b: a.table and b.table and a.lanes != b.lanes),
    "cells per lane 1 to 2": _edge("r 1 2", lambda a, b: (a.r, b.r) == (1, 2)),
    "cells per lane 2 to 3": _edge("r 2 3", lambda a, b: (a.r, b.r) == (2, 3)),
    "window 7 to 6 bits": _edge("c", lambda a, b: a.table and b.table and a.c != b.c),
    "last size with the table": _edge("table", lambda a, b: a.table != b.table),
}
EDGE_SIZES = [(f"{name}: {side} at {n}", n) for name, pair in EDGE_N.items() for side, n in zip(("below", "above"), pair)]


def pick_window(n: int) -> int:
    """pick_window of csrc/h2mi_msm.hip without the H2MI_MSM_C override"""
    lg = (n - 1).bit_length()
    return 20 if lg >= 22 else 17 if lg >= 20 else 16 if lg >= 17 else 15 if lg >= 11 else 13


# ---- the kinds of call ---------------------------------------------------------------------------------------------------------------
class Kind(NamedTuple):
    name: str
    general: bool  # H2MI_MSM_GENERAL
    caller_stream: bool  # on a stream of the caller's (h2mi_stream_create) instead of the library stream
    batch: bool  # the phase entry with count > 1
    inorder: bool  # H2MI_MSM_INORDER, count = 1


KINDS = [Kind(f"{path}-{form}", path == GENERAL, form == "stream", form == "batch", form == "inorder")
         for path in (SMALL, GENERAL) for form in ("single", "stream", "batch", "inorder")]
KIND = {k.name: k for k in KINDS}


class Call(NamedTuple):
    """one call of the ABI: len(entries) MSMs (one unless the kind is a batch), entry j = (column name, length) from the pool"""
    kind: Kind
    entries: tuple


class Join(NamedTuple):
    how: str  # "h2mi_join", "h2mi_sync" or "h2mi_memcpy_d2h"


class Flush(NamedTuple):
    pass


JOINS = ("h2mi_join", "h2mi_sync", "h2mi_memcpy_d2h")


# ---- the model -----------------------------------------------------------------------------------------------------------------------
class Handle:
    """a registered base set as the scheduler sees it"""

    def __init__(self, n: int, forced_c: int = 0):
        self.n = n
        self.table = small_geometry(n).table and not forced_c  # H2MI_MSM_C at registration: the general pipeline with that width
        self.wide = (forced_c or pick_window(n)) >= WIDE_MIN_C
        self.nslot = 4 if n > (1 << 17) else NSLOT
        self.next_slot = 0
        self.since_join = 0
        self.deferred_slots = set()


class Group(NamedTuple):
    handle: Handle
    path: str
    slots: tuple


class Scheduler:
    """What the host side of csrc/h2mi_msm.hip lets an observer see: every handle, and the ONE list of deferred reductions they share.
    `groups` is the log of msm_group calls (path and slots), `census` the launches of the kernels in CENSUS."""

    def __init__(self):
        self.handles = []
        self.deferred = []  # (handle, slot, kind of reduction)
        self.groups = []
        self.census = Counter()

    def register(self, n: int, forced_c: int = 0) -> Handle:
        self.handles.append(Handle(n, forced_c))
        return self.handles[-1]

    def _reduce(self, kind: str, count: int):  # run_reductions: batches of eight of one kind
        launches = _ceil_div(count, SMALL_BATCH if kind == SMALL else TAIL_BATCH)
        if kind == SMALL:
            self.census[SMALL_PAIR] += launches
        else:
            self.census[FINAL] += launches
            if kind == "wide":
                self.census[SEG] += launches

    def flush(self):
        """flush_tails (h2mi_msm_flush): the deferred reductions of every handle, each kind batched with its own"""
        kinds = Counter(kind for _, _, kind in self.deferred)
        for kind in (SMALL, "narrow", "wide"):
            if kinds[kind]:
                self._reduce(kind, kinds[kind])
        for h, slot, _ in self.deferred:
            h.deferred_slots.discard(slot)
        self.deferred.clear()

    def join(self):
        """msm_join_all: h2mi_join, h2mi_sync and h2mi_memcpy_d2h"""
        self.flush()
        for h in self.handles:
            h.since_join = 0

    def _group(self, h: Handle, m: int, general: bool, library: bool, inorder: bool) -> Group:  # msm_group
        small = h.table and not general and not (h.n > SMALL_STREAM_N and h.since_join >= SMALL_STREAM_AFTER)  # take_small
        h.since_join += m
        slots = []
        for _ in range(m):  # acquire_slot
            slot = h.next_slot
            h.next_slot = (slot + 1) % h.nslot
            if slot in h.deferred_slots:
                self.flush()
            slots.append(slot)
        if small:
            self.census[DIGITS] += 1
        else:
            self.census[BIN_COUNT] += 1
            self.census[ACCUM] += 1
        kind = SMALL if small else "wide" if h.wide else "narrow"
        if library and not inorder:  # reduce_or_defer
            for slot in slots:
                h.deferred_slots.add(slot)
                self.deferred.append((h, slot, kind))
            if len(self.deferred) >= max(1, h.nslot // 2):
                self.flush()
        else:
            self._reduce(kind, m)
        g = Group(h, SMALL if small else GENERAL, tuple(slots))
        self.groups.append(g)
        return g

    def msm(self, h: Handle, count: int = 1, general: bool = False, caller_stream: bool = False, inorder: bool = False) -> list:
        """h2mi_msm_bn254_g1_phase_dev (count = 1 without flags: also h2mi_msm_bn254_g1_dev): the groups it issues"""
        library = not caller_stream
        if count == 1 and inorder:
            return [self._group(h, 1, general, library, True)]
        if count > 1 and library and h.n <= HEAD_BATCH_MAX_N and (h.table or not h.wide):
            out, left = [], count
            while left:
                m = min(left, HEAD_BATCH, h.nslot)
                out.append(self._group(h, m, general, library, inorder))
                left -= m
            return out
        return [self._group(h, 1, general, library, False) for _ in range(count)]

    def host_msm(self, h: Handle) -> Group:
        """h2mi_msm_bn254_g1 with a handle: a lone MSM in order on the library stream, then a join"""
        g = self._group(h, 1, False, True, True)
        self.join()
        return g

    def call(self, h: Handle, c: Call) -> list:
        return self.msm(h, len(c.entries), c.kind.general, c.kind.caller_stream, c.kind.inorder)


class Prediction(NamedTuple):
    heads: list  # the path of every group, in issue order: what the order of DIGITS / BIN_COUNT launches shows
    paths: list  # the path of every MSM
    slots: list  # the slot of every MSM
    census: dict


def predict(n: int, ops) -> Prediction:
    """the model's account of a schedule (Call / Join / Flush) on one fresh handle of n points"""
    sch = Scheduler()
    h = sch.register(n)
    for op in ops:
        if isinstance(op, Call):
            sch.call(h, op)
        elif isinstance(op, Join):
            sch.join()
        else:
            sch.flush()
    return Prediction([g.path for g in sch.groups], [g.path for g in sch.groups for _ in g.slots], [s for g in sch.groups for s in g.slots],
                      {k: sch.census[k] for k in CENSUS})


# ---- the scalar columns ----------------------------------------------------------------------------------------------------------------
COLUMNS = ("uniform", "uniform2", "witness", "repeated", "repeated3", "zero", "r-1", "sparse")
POISON = "poison"  # what a scalar buffer is overwritten with when no later MSM of the schedule uses it


@functools.lru_cache(maxsize=None)
def column(n: int, name: str) -> np.ndarray:
    """(n, 4) Montgomery limbs, read-only: the column `name` of the pool of a size-n base set"""
    seed = 7000 + n
    if name == "uniform":
        a = o.random_field_limbs(n, seed)
    elif name in ("uniform2", POISON):
        a = o.random_field_limbs(n, seed + (1 if name == "uniform2" else 2))
    elif name == "witness":  # 90 % zero, 0 / 1, a few uniform values
        a = o.witness_like_limbs(n, seed + 3)
    elif name in ("repeated", "repeated3"):  # one value everywhere; with three exceptions: first, middle and last row
        a = np.tile(o.random_field_limbs(1, seed + 4)[0], (n, 1))
        if name == "repeated3":
            for i, row in zip((0, n // 2, n - 1), o.random_field_limbs(3, seed + 5)):
                a[i] = row
    elif name == "zero":
        a = np.zeros((n, 4), dtype=np.uint64)
    elif name == "r-1":
        a = np.tile(o.pack([o.R - 1], o.R)[0], (n, 1))
    elif name == "sparse":  # one row in 64 (at least one) holds a uniform value
        a = np.zeros((n, 4), dtype=np.uint64)
        a[:: 64] = o.random_field_limbs(n, seed + 6)[:: 64]
    else:
        raise KeyError(name)
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def pool(n: int) -> list:
    """the (column, length) pairs every schedule on a size-n handle draws from: every column at full length, and prefixes"""
    full = [(name, n) for name in COLUMNS]
    if n < 16:
        return full
    return full + [(name, n - 5) for name in ("uniform", "witness", "repeated", "r-1")] + [(name, n // 3 + 1) for name in ("uniform2", "repeated3", "sparse", "witness")]


BASES_MAX = 20000


@functools.lru_cache(maxsize=None)
def bases(n: int = BASES_MAX) -> np.ndarray:
    """(n, 8) affine Montgomery limbs: the first n of BASES_MAX random multiples of the generator, every base set of these tests"""
    from oracle import cref

    if n != BASES_MAX:
        return np.ascontiguousarray(bases()[:n])
    b = cref.g1_mul_gen(o.random_field_limbs(BASES_MAX, 0x5C4ED), 4)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def expected(n: int, name: str, length: int) -> bytes:
    """the affine limbs (bytes: hashable, comparable) of sum_i column(n, name)[i] * bases[i] over i < length, from the C oracle:
    computed once per (column, length), however many steps of however many schedules use it"""
    from oracle import cref

    return cref.normalize(cref.msm(column(n, name)[:length], bases()[:length], 4)).tobytes()


# ---- the schedules -----------------------------------------------------------------------------------------------------------------------
def _entries(n: int, count: int, start: int, same_length: bool) -> tuple:
    """`count` pool entries from position `start` on (a batch call has ONE length: the entries of that length, in pool order)"""
    p = pool(n)
    if same_length:
        length = p[start % len(p)][1]
        p = [e for e in p if e[1] == length]
    return tuple(p[(start + j) % len(p)] for j in range(count))


def kind_calls(n: int, kind: Kind, msms: int, start: int) -> list:
    """`msms` MSMs of one kind: single calls, or batch calls of HEAD_BATCH"""
    if not kind.batch:
        return [Call(kind, _entries(n, 1, start + i, False)) for i in range(msms)]
    assert msms % HEAD_BATCH == 0
    return [Call(kind, _entries(n, HEAD_BATCH, start + 5 * i, True)) for i in range(msms // HEAD_BATCH)]


def transition_schedules(n: int = 1 << 13) -> dict:
    """"A->B" -> eight MSMs of kind A, then eight of kind B, on one handle with no join in between (so that every one of the eight
    slots is used by A and then by B), then the join: all 64 ordered pairs"""
    out = {}
    for i, a in enumerate(KINDS):
        for j, b in enumerate(KINDS):
            start = 3 * (8 * i + j)
            out[f"{a.name}->{b.name}"] = kind_calls(n, a, NSLOT, start) + kind_calls(n, b, NSLOT, start + NSLOT) + [Join("h2mi_join")]
    return out


def streaming_schedules(n: int) -> dict:
    """the schedules that pin the streaming rule (take_small's since_join) down, by name"""
    single, stream, batch, general = KIND["small-single"], KIND["small-stream"], KIND["small-batch"], KIND["general-single"]
    one = lambda kind, i: Call(kind, _entries(n, 1, i, False))
    six = [one(single, i) for i in range(6)]
    out = {"six singles, one join": six + [Join("h2mi_join")]}
    for how in JOINS:
        out[f"small again after {how}"] = six + [Join(how), one(single, 6), Join("h2mi_join")]
    out["a phase of nine: groups of 4, 4, 1"] = [Call(batch, _entries(n, 9, 0, True)), Join("h2mi_join")]
    out["four on a caller's stream count"] = [one(stream, i) for i in range(4)] + [one(single, 4), Join("h2mi_join")]
    out["a forced general MSM counts"] = [one(general, 0)] + [one(single, i) for i in range(1, 5)] + [Join("h2mi_join")]
    return out


STREAMING_SIZES = (SMALL_STREAM_N, SMALL_STREAM_N + 1, SMALL_MAX_N)
