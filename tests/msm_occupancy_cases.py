"""The general MSM pipeline of csrc/h2mi_msm.hip at engineered bucket occupancies, shared by tests/test_msm_occupancy_host.py and
tests/test_gpu_msm_occupancy.py: scalars built from chosen signed digits, so that a chosen number of entries lands in a chosen bucket
at a chosen offset of the bucket-ordered array; a plain-integer model of what the partition head leaves behind (`head`: bucket
offsets, the chunk length, partials and fold tasks per bucket with their scans, the hot set, the sorted payloads, the shift); and
bases with known discrete logarithms, so that every bucket sum, every wide-window segment sum and the result are integers mod r
before they are points (`sums`).

The rules restated here are the ones the kernels read today (the constants below and `head`).  Where the device disagrees with this
file one of the two is wrong about a rule; the comments of csrc/h2mi_msm.hip and DESIGN.md decide which.

Python integers and numpy only; deterministic.  The recoding and window count are tests/table_depth_cases.py's, the default window
width tests/msm_schedule_cases.py's."""
import functools
from typing import NamedTuple

import numpy as np

import msm_schedule_cases as S
import table_depth_cases as T
from oracle import bn254 as o

R = o.R
recode, windows = T.recode, T.windows

# ---- the constants of csrc/h2mi_msm.hip, restated ---------------------------------------------------------------------------------------
P1_TS = T.P1_TS  # scalars per partition tile
S1 = T.S1  # partials per fold task
S0_MAX = T.S0_MAX
ACCUM_RESIDENT_CHUNKS = T.ACCUM_RESIDENT_CHUNKS
MAT_LOG = T.MAT_LOG
SHIFT_MIN_N = T.SHIFT_MIN_N
ACCUM_GATHER_ONLY_MAX = 16384  # up to this many entries: one entry per chunk
HOT_MIN = 64  # narrow windows: more fold tasks than this and a workgroup finishes the bucket
HOT_MIN_WIDE = 8  # wide windows: more partials than this (no fold level)
HOT_STRIDE = 64  # quads of a hot-bucket finisher
HOT_BLOCK = 256  # buckets one finisher workgroup scans
WIDE_MIN_C, WIDE_MAX_C = 18, 20
WIDE_BIN_BITS = 9
P2_CH = 8192  # payloads per LDS chunk of the per-bin sort
P2W_CH = 6144  # wide windows
PART_WORDS = 36  # one XYZZ partial sum: X, Y, ZZ, ZZZ as nine 29-bit limbs
LANE_QUAD_LIMIT = 65536  # launch_tails: quads while max_tasks1 * count (fold) / max_nb * 8 * count (finish) stay within this


class Geometry(NamedTuple):
    c: int
    W: int
    nb: int
    lb: int
    nbins: int
    seg_log: int
    logNl: int
    logNh: int

    @property
    def wide(self):
        return self.seg_log > 0

    @property
    def L(self):
        return 1 << self.seg_log

    @property
    def hot_min(self):
        return HOT_MIN_WIDE if self.wide else HOT_MIN

    def pos(self, b: int) -> int:
        """where bucket b sits in the bucket-ordered arrays: wide windows bin by the low nine bits"""
        return ((b & 511) << self.lb | b >> WIDE_BIN_BITS) if self.wide else b

    def bucket_at(self, p: int) -> int:
        """the bucket at position p"""
        return (p >> self.lb | (p & ((1 << self.lb) - 1)) << WIDE_BIN_BITS) if self.wide else p


def geometry(c: int) -> Geometry:
    """register_dev"""
    nb = 1 << (c - 1)
    seg_log = max(c - 1 - MAT_LOG, 0)
    logNl = (c - 1 - seg_log + 1) // 2
    lb = max(c - 1 - 9, 0)
    return Geometry(c, windows(c), nb, lb, nb >> lb, seg_log, logNl, (c - 1 - seg_log) - logNl)


def from_digits(digits: dict, c: int) -> int:
    """the scalar whose signed digits are exactly {window: digit}; the top non-zero digit must be positive"""
    s = sum(d << (c * w) for w, d in digits.items())
    assert 0 <= s < R, digits
    rd = recode(s, c)
    assert all(rd[w] == digits.get(w, 0) for w in range(windows(c))), (digits, rd)
    return s


def accum_rounds(entries: int) -> int:
    per_round = S0_MAX * ACCUM_RESIDENT_CHUNKS
    return -(-entries // per_round) if entries else 1


def chunk_len(entries: int) -> int:
    """accum_chunk_len"""
    if entries <= ACCUM_GATHER_ONLY_MAX:
        return 1
    slots = accum_rounds(entries) * ACCUM_RESIDENT_CHUNKS
    return max(8, -(-entries // slots))


def clamp_override(s0_fixed: int, n_eff: int, c: int, n_reg: int) -> int:
    """msm_general: H2MI_MSM_S0 is raised until the chunks of n_eff * W entries fit the partial buffer sized at registration"""
    g = geometry(c)
    if not 1 <= s0_fixed <= S0_MAX:
        return 0
    nW = (n_reg + 1) * g.W
    max_tasks0 = min(accum_rounds(nW) * ACCUM_RESIDENT_CHUNKS, nW) + g.nb + 1
    total = n_eff * g.W
    while s0_fixed < S0_MAX and -(-total // s0_fixed) + g.nb > max_tasks0:
        s0_fixed += 1
    assert -(-total // s0_fixed) + g.nb <= max_tasks0
    return s0_fixed


def sample_rows(n: int) -> list:
    """k_msm_pick_shift: the 64 rows it reads"""
    return [min((n // 64) * lane + n // 128, n - 1) for lane in range(64)]


def pick_shift(scalars, n: int) -> int:
    """the value held by at least 40 of the 64 sampled rows (the first such lane's), else 0"""
    smp = [scalars[i] for i in sample_rows(n)]
    for v in smp:
        if smp.count(v) >= 40:
            return v
    return 0


def shifts(n: int, n_reg: int) -> bool:
    """does an MSM of n scalars over a base set of n_reg points registered with a forced width (no digit-multiples table) try the shift"""
    return n_reg >= SHIFT_MIN_N and n == n_reg


@functools.lru_cache(maxsize=1 << 16)
def _entries_of(s: int, c: int) -> tuple:
    """(window, bucket-array position, sign bit) of every non-zero digit of s"""
    g = geometry(c)
    return tuple((w, g.pos(abs(d) - 1), 1 if d < 0 else 0) for w, d in enumerate(recode(s, c)) if d)


class Head(NamedTuple):
    geo: Geometry
    stride: int
    v: int  # the shift (0: none taken, or not tried)
    entries: int
    s0: int
    cnt: np.ndarray  # [nb]
    off: np.ndarray  # [nb + 1]
    np0: np.ndarray  # [nb + 1], last = 0
    np1: np.ndarray
    toff0: np.ndarray  # [nb + 1], last = total
    toff1: np.ndarray
    hot: list  # positions of the hot buckets
    pos: np.ndarray  # [entries] position of every entry, sorted
    payload: np.ndarray  # [entries] sign << 31 | row * stride + i, sorted inside each bucket


def head(scalars, c: int, n: int, shifted: bool = False, s0_fixed: int = 0, n_reg: int = 0) -> Head:
    """The partition of an MSM of n canonical scalars with c-bit windows over a base set of n_reg (default n) points.  `shifted`: the
    dominant value v of the 64 sampled rows is subtracted from every scalar and scalar n = v goes to the sum point (row index n).
    `s0_fixed`: the chunk length H2MI_MSM_S0 asks for (clamped as msm_general does), 0 = chosen from the entry count."""
    g = geometry(c)
    n_reg = n_reg or n
    assert len(scalars) == n <= n_reg and all(0 <= s < R for s in scalars)
    stride = n_reg + 1
    v = pick_shift(scalars, n) if shifted else 0
    eff = [(s - v) % R for s in scalars] + [v] if shifted else scalars
    pos, pay = [], []
    for i, s in enumerate(eff):
        if s:
            for w, p, neg in _entries_of(s, c):
                pos.append(p)
                pay.append(neg << 31 | (w * stride + i))
    pos, pay = np.array(pos, dtype=np.int64), np.array(pay, dtype=np.int64)
    cnt = np.bincount(pos, minlength=g.nb).astype(np.int64)
    entries = int(cnt.sum())
    s0 = clamp_override(s0_fixed, len(eff), c, n_reg) or chunk_len(entries)
    off = np.concatenate(([0], np.cumsum(cnt)))
    o_ = off[:-1]
    np0 = np.where(cnt > 0, 1 + (o_ + cnt - 1) // s0 - o_ // s0, 0)
    np1 = (np0 + S1 - 1) // S1
    scan = lambda a: np.concatenate(([0], np.cumsum(a)))
    hot = np.nonzero((np0 if g.wide else np1) > g.hot_min)[0].tolist()
    order = np.lexsort((pay, pos))
    z = np.zeros(1, dtype=np.int64)
    return Head(g, stride, v, entries, s0, cnt, off, np.concatenate((np0, z)), np.concatenate((np1, z)), scan(np0), scan(np1), hot, pos[order], pay[order])


# ---- bases with known discrete logarithms -----------------------------------------------------------------------------------------------
NMAX = 1 << 14
IDENTITY_AT, PAIR_AT, REPEAT_AT = 7, (8, 9), ((3, 5), (3, 700), (11, 12))


@functools.lru_cache(maxsize=None)
def logs() -> tuple:
    """k_i of the NMAX bases P_i = k_i G: pseudo-random, a few repeated, one zero (the identity), one pair k, r - k"""
    k = o.unpack(o.random_field_limbs(NMAX, 0x0CC0BA5E), R)
    k[IDENTITY_AT] = 0
    k[PAIR_AT[1]] = R - k[PAIR_AT[0]]
    for src, dst in REPEAT_AT:
        k[dst] = k[src]
    return tuple(k)


def points_of(ints) -> np.ndarray:
    """(m, 8) affine Montgomery limbs of k G for every k, one batched call of the C oracle; the identity is (0, 0)"""
    from oracle import cref

    ints = [k % R for k in ints]
    uniq = sorted(set(ints))
    at = {k: j for j, k in enumerate(uniq)}
    pts = cref.g1_mul_gen(o.pack(uniq, R), 4) if uniq else np.zeros((0, 8), dtype=np.uint64)
    return pts[[at[k] for k in ints]] if ints else pts


@functools.lru_cache(maxsize=None)
def bases(n: int = NMAX) -> np.ndarray:
    if n != NMAX:
        return np.ascontiguousarray(bases()[:n])
    b = points_of(logs())
    b.setflags(write=False)
    return b


class Sums(NamedTuple):
    result: int  # sum_i s_i k_i mod r
    bucket: dict  # position -> (sum of +-2^(c w) k_i over the bucket's entries) mod r, non-empty buckets only
    seg_p: dict  # wide windows: segment -> P_s mod r, segments with a non-empty bucket only
    seg_v: dict  # segment -> V_s mod r


def sums(h: Head, scalars, n_reg: int = 0) -> Sums:
    """every sum of the model as a multiple of the generator"""
    g, k = h.geo, logs()
    n_reg = n_reg or len(scalars)
    ksum = sum(k[:n_reg]) % R
    pw = [pow(2, g.c * w, R) for w in range(g.W)]
    idx = h.payload & 0x7FFFFFFF
    bucket = {}
    for p, neg, w, i in zip(h.pos.tolist(), (h.payload >> 31).tolist(), (idx // h.stride).tolist(), (idx % h.stride).tolist()):
        t = pw[w] * (ksum if i == n_reg else k[i])
        bucket[p] = bucket.get(p, 0) + (-t if neg else t)
    bucket = {p: t % R for p, t in bucket.items()}
    result = sum(s * ki for s, ki in zip(scalars, k)) % R
    seg_p, seg_v = {}, {}
    if g.wide:
        for p, t in bucket.items():
            b = g.bucket_at(p)
            s, j = b >> g.seg_log, b & (g.L - 1)
            seg_p[s] = (seg_p.get(s, 0) + t) % R
            seg_v[s] = (seg_v.get(s, 0) + (g.L - 1 - j) * t) % R
    return Sums(result, bucket, seg_p, seg_v)


def weighted(h: Head, sm: Sums) -> int:
    """sum_b (b + 1) B_b mod r: what the row / column sums (and the segment level) make of the buckets; equals Sums.result"""
    g = h.geo
    if not g.wide:
        return sum((p + 1) * t for p, t in sm.bucket.items()) % R
    return (g.L * sum((s + 1) * t for s, t in sm.seg_p.items()) - sum(sm.seg_v.values())) % R


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    family: str
    c: int
    n_reg: int  # points of the base set (the first n_reg of `bases`)
    scalars: tuple  # n <= n_reg canonical integers
    s0_fixed: int  # H2MI_MSM_S0, 0 = unset
    expect: dict  # the property the case is named for: any of s0, hot (positions), not_hot (positions), np0 {position: value}, entries, v
    principal: bool = False  # the family's case that also runs through every entry form

    @property
    def n(self):
        return len(self.scalars)

    @property
    def shifted(self):
        return shifts(self.n, self.n_reg)

    @property
    def id(self):
        return f"{self.family}-{self.name}" + (f"-S0_{self.s0_fixed}" if self.s0_fixed else "")


_MODELS = {}


def model(case: Case) -> tuple:
    """(Head, Sums) of a case, computed once"""
    key = (case.id, case.n)
    if key not in _MODELS:
        h = head(case.scalars, case.c, case.n, case.shifted, case.s0_fixed, case.n_reg)
        _MODELS[key] = (h, sums(h, case.scalars, case.n_reg))
    return _MODELS[key]


def pack_entries(entries, c: int, per: int = 0) -> list:
    """Scalars that leave exactly the given (bucket, negative) entries: `per` (default W - 1) of them per scalar, in the windows from 0
    up, the top window unused.  The last digit of a scalar is made positive (a scalar is not negative) — callers that care about a
    sign put such an entry anywhere but last in its group of `per`, or use from_digits."""
    g = geometry(c)
    per = per or g.W - 1
    assert per <= g.W - 1
    out = []
    for j in range(0, len(entries), per):
        grp = entries[j:j + per]
        dg = {w: (-(b + 1) if neg and w != len(grp) - 1 and b != g.nb - 1 else b + 1) for w, (b, neg) in enumerate(grp)}
        out.append(from_digits(dg, c))
    return out


def fill(counts: dict, alternate: bool = True) -> list:
    """the entry list with counts[b] entries in bucket b, signs alternating"""
    return [(b, alternate and j % 2 == 1) for b, m in counts.items() for j in range(m)]


def _pad(scalars: list, n: int) -> tuple:
    assert len(scalars) <= n, (len(scalars), n)
    return tuple(scalars) + (0,) * (n - len(scalars))


def _spread(scalars: list, n: int) -> tuple:
    """the scalars at evenly spaced rows of a column of n zeros: partition tiles between them stay all-zero"""
    out = [0] * n
    step = max(1, n // max(1, len(scalars)))
    assert len(scalars) * step <= n
    for j, s in enumerate(scalars):
        out[j * step] = s
    return tuple(out)


N13 = 2047  # the base set of the c = 13 cases (every case registers with its width forced: H2MI_MSM_C); no sum point, so no shift
N15 = 4000  # c = 15 without a sum point
NSHIFT = 6 * P1_TS  # 4608: with the sum point, which then sits alone in a seventh tile
NWIDE = 1500


def _family_a() -> list:
    """hot threshold, narrow windows"""
    out = []
    for c, n_reg in ((13, N13), (15, N15)):
        half = 1 << (c - 1)
        filler = [from_digits({0: half, 5: -(half - 1), 6: 1}, c)] * 5
        for tot in (512, 513):
            sc = [from_digits({3: 701}, c)] * tot + filler
            exp = {"s0": 1, "np0": {700: tot}, "hot": [700] if tot == 513 else [], "not_hot": [700] if tot == 512 else []}
            out.append(Case(f"c{c}-{tot}-in-one-bucket", "A", c, n_reg, _pad(sc, n_reg - 1), 0, exp, principal=(c == 13 and tot == 513)))
    # s0 = 8: the same 4096 entries are 512 or 513 partials by the offset the bucket starts at
    c = 15
    for pre, want in ((0, 512), (1, 513), (7, 513), (8, 512)):
        sc = [from_digits({0: 1}, c)] * pre + [from_digits({2: 100}, c)] * 4096 + [from_digits({w: 200 + w for w in range(16)}, c)] * 800
        exp = {"s0": 8, "np0": {99: want}, "hot": [99] if want == 513 else [], "not_hot": [99] if want == 512 else []}
        out.append(Case(f"c15-4096-after-{pre}", "A", c, NMAX // 2, _pad(sc, NMAX // 2 - 1), 0, exp))
    # the finisher's stride of 64 folded partials; two and three hot buckets in one 256-bucket block, another block, both ends
    c = 13
    g = geometry(c)
    counts = {0: 513, 10: 8 * 65, 20: 8 * 127, 30: 8 * 128, 300: 8 * 129, 301: 8 * 64, g.nb - 1: 513}
    exp = {"s0": 1, "np0": dict(counts), "hot": [0, 10, 20, 30, 300, g.nb - 1], "not_hot": [301]}
    out.append(Case("c13-hot-65-127-128-129-and-both-ends", "A", c, N13, _pad(pack_entries(fill(counts), c), N13 - 1), 0, exp))
    counts = {5: 513, 250: 513, 256: 520, 300: 513, 511: 600, 4000: 1100}  # two in block 0, three in block 1, one in block 15
    out.append(Case("c13-hot-two-and-three-in-a-block-and-another-block", "A", c, N13, _pad(pack_entries(fill(counts), c), N13 - 1), 0,
                    {"s0": 1, "hot": [5, 250, 256, 300, 511, 4000]}))
    return out


def _family_b() -> list:
    """wide windows"""
    out = []
    for c in (18, 19, 20):
        g = geometry(c)
        L, top = g.L, g.W - 1
        full = 5  # a segment with every bucket filled
        counts = {1000: 8, 70001 % g.nb: 9, 0: 1, L - 1: 2, g.nb - L: 3, g.nb - 1: 2}
        counts.update({full * L + j: 1 + j % 3 for j in range(L)})
        sc = pack_entries(fill(counts), c)
        sc += [from_digits({top: 1}, c), from_digits({top: 2}, c), from_digits({top: 3, 0: -5}, c)]  # the thin top window
        exp = {"s0": 1, "hot": [g.pos(70001 % g.nb)], "not_hot": [g.pos(1000)], "np0": {g.pos(1000): 8, g.pos(70001 % g.nb): 9}}
        out.append(Case(f"c{c}-8-and-9-segment-ends-full-segment-top-window", "B", c, NWIDE, _pad(sc, NWIDE - 3), 0, exp, principal=(c == 19)))
    return out


FOLD_NP0 = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65)


def _family_c() -> list:
    """fold split: np0 on both sides of every multiple of S1 that changes the balanced split"""
    c = 13
    counts = {100 + 37 * j: m for j, m in enumerate(FOLD_NP0)}
    sc = _pad(pack_entries(fill(counts), c), N13 - 1)
    out = [Case("c13-np0-1-to-65", "C", c, N13, sc, 0, {"s0": 1, "np0": dict(counts)}, principal=True)]
    out += [Case("c13-np0-1-to-65", "C", c, N13, sc, s0, {"s0": s0}) for s0 in (3, 128)]
    return out


def _family_d() -> list:
    """the chunk walk of k_msm_accum"""
    c = 15
    g = geometry(c)
    out = []
    # runs that start and end on chunk boundaries (s0 = 8), a chunk crossing three one-entry buckets, runs of empty buckets (across a
    # bin boundary: 32 buckets per bin), then enough to pass 16384 entries, then a tail that sets entries mod s0
    lead = {0: 8, 1: 16, 2: 1, 3: 1, 4: 1, 5: 5, 64: 9, 65: 7, 200: 3}
    bulk = {1000 + j: 1100 for j in range(16)}
    base_total = sum(lead.values()) + sum(bulk.values())
    for rem in (0, 1, 7):
        tail = (rem - base_total) % 8 or 8
        counts = {**lead, **bulk}
        counts[g.nb - 1] = tail
        sc = _pad(pack_entries(fill(counts), c), NMAX // 2 - 1)
        exp = {"s0": 8, "entries": base_total + tail, "np0": {0: 1, 1: 2, 2: 1, 3: 1, 4: 1, 5: 1}}
        out.append(Case(f"c15-boundaries-empty-runs-entries-mod-8-is-{rem}", "D", c, NMAX // 2, sc, 0, exp, principal=(rem == 1)))
        if rem == 1:
            out += [Case(f"c15-boundaries-empty-runs-entries-mod-8-is-{rem}", "D", c, NMAX // 2, sc, s0, {"s0": s0}) for s0 in (3, 5)]
    for s0 in (0, 3, 5):
        out.append(Case("c15-only-last-bucket", "D", c, N15, _pad(pack_entries(fill({g.nb - 1: 21}), c), N15 - 1), s0, {"s0": s0 or 1, "entries": 21}))
        out.append(Case("c15-one-entry", "D", c, N15, _spread([from_digits({4: 78}, c)], N15 - 1), s0, {"s0": s0 or 1, "entries": 1}))
    dense = [from_digits({w: 3 + w for w in range(16)}, c)] * 1024
    out.append(Case("c15-16384-entries", "D", c, N15, _pad(dense, N15 - 1), 0, {"s0": 1, "entries": 16384}))
    out.append(Case("c15-16385-entries", "D", c, N15, _pad(dense + [from_digits({0: 1}, c)], N15 - 1), 0, {"s0": 8, "entries": 16385}))
    return out


def _family_e() -> list:
    """the partition: LDS chunks of the per-bin sort, the aligned key window, the second wavefront of the scan, tiles"""
    out = []
    c = 15
    g = geometry(c)
    per_bin = 1 << g.lb
    counts = {}
    for j, m in enumerate((P2_CH - 1, P2_CH, P2_CH + 1, 2 * P2_CH + 1)):
        counts[(3 + 4 * j) * per_bin + 9] = m  # one bucket of the bin
        for q in range(per_bin):  # all buckets of another bin
            counts[(19 + 4 * j) * per_bin + q] = m // per_bin + (1 if q < m % per_bin else 0)
    for j in range(17):  # bins of 17 entries: the next bin's start takes every residue mod 16
        counts[(100 + j) * per_bin + j] = 17
    sc = pack_entries(fill(counts), c)
    out.append(Case("c15-bins-of-8191-8192-8193-16385-and-every-start-residue", "E", c, NMAX // 2, _pad(sc, NMAX // 2 - 1), 0,
                    {"entries": sum(counts.values())}, principal=True))
    out.append(Case("c15-bin-511-alone", "E", c, N15, _pad(pack_entries(fill({511 * per_bin + q: 2 + q % 3 for q in (0, 7, 31)}), c), N15 - 1), 0, {"s0": 1}))
    # wide windows: bins are the low nine bits of the bucket
    c = 18
    counts = {}
    for j, m in enumerate((P2W_CH - 1, P2W_CH, P2W_CH + 1)):
        counts[(40 + j) | (3 << 9)] = m
        for q in range(256):
            counts[(80 + j) | (q << 9)] = m // 256 + (1 if q < m % 256 else 0)
    out.append(Case("c18-bins-of-6143-6144-6145", "E", c, 3000, _pad(pack_entries(fill(counts), c), 2999), 0, {"entries": sum(counts.values())}))
    # c = 17: 128 buckets per bin, the scan's second wavefront
    c = 17
    counts = {5 * 128 + 63: 3, 5 * 128 + 64: 4, 5 * 128 + 127: 5, 6 * 128: 2, 6 * 128 + 65: 1}
    out.append(Case("c17-in-bin-buckets-63-64-127", "E", c, N15, _pad(pack_entries(fill(counts), c), N15 - 1), 0, {"s0": 1, "np0": dict(counts)}))
    # tiles
    c = 15
    # all W = 17 digits of a scalar, the top window's included (it holds digits below r >> 240: buckets of the first 387 bins)
    top = g.W - 1
    top_bins = ((R >> (c * top)) - 1) // per_bin
    one_bin = [from_digits({w: 9 * per_bin + (i + w) % per_bin + 1 for w in range(g.W)}, c) for i in range(P1_TS)]
    all_bins = [from_digits({**{w: ((16 * i + w) % 512) * per_bin + i % per_bin + 1 for w in range(top)}, top: (i % top_bins) * per_bin + i % per_bin + 1}, c)
                for i in range(P1_TS)]
    for extra in (0, 1):
        n = 4 * P1_TS + extra
        col = [0] * n
        col[:P1_TS] = one_bin
        col[3 * P1_TS:4 * P1_TS] = all_bins
        if extra:
            col[-1] = from_digits({0: 1, 1: -2, 2: 3}, c)
        out.append(Case(f"c15-first-and-last-tile-of-{n}-rows", "E", c, N15, tuple(col), 0, {"entries": 2 * g.W * P1_TS + 3 * extra}))
    return out


def _family_f() -> list:
    """the dominant-value shift: NSHIFT points, registered with the sum point"""
    c, n = 15, NSHIFT
    v = o.unpack(o.random_field_limbs(1, 0xF5)[0], R)[0]
    uni = o.unpack(o.random_field_limbs(n, 0xF6), R)
    rows = sample_rows(n)
    out = [Case("constant-column-sum-point-alone-in-a-tile", "F", c, n, (v,) * n, 0, {"v": v, "entries": len(_entries_of(v, c))}, principal=True)]
    for same in (39, 40):
        col = list(uni)
        for i in rows[64 - same:]:
            col[i] = v
        out.append(Case(f"{same}-of-64-sampled-rows-agree", "F", c, n, tuple(col), 0, {"v": v if same == 40 else 0}))
    col = [0] * n
    for i in rows:
        col[i] = v
    out.append(Case("sampled-rows-agree-all-others-zero", "F", c, n, tuple(col), 0, {"v": v}))
    out.append(Case("n-minus-1-of-n-bases", "F", c, n, tuple(uni[:n - 1]), 0, {"v": 0}))
    return out


def _family_g() -> list:
    """impulses: one entry, either sign, at the corners of the bucket matrix, in window 0 and in the top window"""
    c = 15
    g = geometry(c)
    Nl, top = 1 << g.logNl, g.W - 1
    top_max = (R >> (c * top)) - 1
    out = []
    for b in (0, 1, Nl - 1, Nl, g.nb - Nl, g.nb - 1):
        for w in (0, top):
            for neg in (False, True):
                if neg and (w == top or b == g.nb - 1):
                    continue  # the top non-zero digit of a scalar is positive, and -2^(c-1) is not a digit
                if w == top and b + 1 > top_max:
                    continue  # the top window holds 254 - c (W - 1) bits
                dg = {w: -(b + 1) if neg else b + 1}
                if neg:
                    dg[w + 1] = 1  # r - x would fill every window: a second, positive digit one window up instead
                out.append(Case(f"c15-bucket-{b}-window-{w}-{'minus' if neg else 'plus'}", "G", c, N15, _pad([0] * 1234 + [from_digits(dg, c)], N15 - 1), 0,
                                {"s0": 1, "entries": 2 if neg else 1}, principal=not out))
    return out


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = _family_a() + _family_b() + _family_c() + _family_d() + _family_e() + _family_f() + _family_g()
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return tuple(out)


def principal(family: str) -> Case:
    return next(c for c in cases() if c.family == family and c.principal)


# ---- entry forms (H) -------------------------------------------------------------------------------------------------------------------
def batch_family(family: str) -> list:
    """four different cases of one family over one base set and one length, one of them all-zero scalars"""
    first = principal(family)
    same = [c for c in cases() if c.family == family and (c.c, c.n_reg, c.n, c.s0_fixed) == (first.c, first.n_reg, first.n, 0)][:3]
    assert len(same) == 3, family
    return same + [Case("all-zero", family, first.c, first.n_reg, (0,) * first.n, 0, {"entries": 0, "s0": 1})]


def lane_quad_batches() -> list:
    """(c, n_reg, count, fold is quads, finish is quads) for phase batches on both sides of launch_tails' 65536 rules.  The form is
    inferred from that rule (tasks1 = (min(n_eff W, 131072) + nb) / 8 + nb per MSM), not observed."""
    out = []
    for c, n_reg, count in ((15, 8192, 1), (15, 8192, 2), (13, N13, 2), (13, N13, 3)):
        g = geometry(c)
        n_eff = n_reg + (1 if shifts(n_reg, n_reg) else 0)
        total = n_eff * g.W
        tasks0 = min(accum_rounds(total) * ACCUM_RESIDENT_CHUNKS, total) + g.nb
        tasks1 = tasks0 // S1 + g.nb
        out.append((c, n_reg, count, tasks1 * count <= LANE_QUAD_LIMIT, g.nb * 8 * count <= LANE_QUAD_LIMIT))
    return out


@functools.lru_cache(maxsize=None)
def lane_quad_cases(c: int, n_reg: int, count: int) -> tuple:
    """`count` different full-length columns over the base set: uniform, uniform with a quarter of the rows zero, uniform again"""
    out = []
    for j in range(count):
        col = o.unpack(o.random_field_limbs(n_reg, 0x1A9E + 16 * c + j), R)
        if j == 1:
            col = [0 if i % 4 == 1 else s for i, s in enumerate(col)]
        out.append(Case(f"c{c}-batch-of-{count}-column-{j}", "H", c, n_reg, tuple(col), 0, {}))
    return tuple(out)


def slot_reuse_pair() -> tuple:
    """(dense, sparse): the first and the ninth of nine MSMs on one handle, which share a workspace slot (eight slots per handle)"""
    dense = principal("D")
    sparse = Case("one-entry-after-a-dense-msm-in-the-same-slot", "H", dense.c, dense.n_reg, _spread([from_digits({4: 78}, dense.c)], dense.n), 0, {"entries": 1})
    return dense, sparse


def all_cases() -> tuple:
    """every case a test runs: families A - G, and of H the phase batches, the lane / quad batches and the slot-reuse pair"""
    out = {c.id: c for c in cases()}
    for fam in "ADFG":
        out.update({c.id: c for c in batch_family(fam)})
    for c, n_reg, count, _, _ in lane_quad_batches():
        out.update({x.id: x for x in lane_quad_cases(c, n_reg, count)})
    out.update({x.id: x for x in slot_reuse_pair()})
    return tuple(out.values())
