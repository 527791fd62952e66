"""The small path of the MSM (csrc/h2mi_msm.hip, "small base sets": k_msm_small_multiples, k_msm_small_digits{,_b}, k_msm_small_accum with
seg_tree_sum and small_finish) at engineered digits, lane chains and tree levels, shared by tests/test_msm_small_host.py and
tests/test_gpu_msm_small.py: a restatement of the digit bytes, of how k_msm_small_accum divides the cells among workgroups and lanes and
of the two trees, in Python integers; bases with known discrete logarithms, so that every table entry, lane sum, partial sum and result
is an integer mod r before it is a point; and the named cases, each recording the property it is built for.

The model classifies every mixed addition of every lane chain and every pair of both trees (CLASSES).  Which (tree, level, class)
combinations the cases reach is computed by `reached`, and those of `wanted` that they do not are listed in NOT_REACHED: partial sums
of different windows are equal only where the base set holds points that differ by the right power of the window.

The geometry is tests/msm_schedule_cases.py's small_geometry; every size comes from that rule (EDGE_N), none is typed in.  Python
integers and numpy only; deterministic."""
import functools
from math import gcd
from typing import NamedTuple

import numpy as np

import msm_occupancy_cases as OC
import msm_schedule_cases as S
import table_depth_cases as T
from oracle import bn254 as o

R = o.R
PART_WORDS = OC.PART_WORDS
points_of = OC.points_of
small_geometry = S.small_geometry
NSLOT = S.NSLOT

GENERAL, EQUAL, OPPOSITE, IDENT, BOTH, SKIPPED = "general", "equal", "opposite", "identity operand", "both identity", "identity point skipped"
CLASSES = (GENERAL, EQUAL, OPPOSITE, IDENT, BOTH)  # of an addition; SKIPPED: a live digit whose table point is the identity (no addition)


def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def _pow2_at_least(x: int) -> int:
    t = 1
    while t < x:
        t <<= 1
    return t


# ---- the sizes: every one from the restated rule -----------------------------------------------------------------------------------------
N_TREE = S.SMALL_CELLS  # 128 points, 128 lanes, one cell per lane: workgroup b is window b, lane t is point t
N_L256 = S.EDGE_N["lanes 128 to 256"][1]  # the first size with 256 gathering lanes
N_GMAX = S.EDGE_N["cells per lane 1 to 2"][0]  # the last size with one cell per lane: the most workgroups
N_R2 = S.EDGE_N["cells per lane 1 to 2"][1]
N_R3 = S.EDGE_N["cells per lane 2 to 3"][1]
N_C6 = S.EDGE_N["window 7 to 6 bits"][1]  # the first size with 6-bit windows
N_MAX = S.SMALL_MAX_N  # the largest table, the most cells per lane
SIZES = (N_TREE, N_L256, N_GMAX, N_R2, N_R3, N_C6, N_MAX)
assert small_geometry(N_TREE).lanes == 128 and small_geometry(N_TREE).G == small_geometry(N_TREE).W
assert [small_geometry(n).r for n in (N_L256, N_GMAX, N_R2, N_R3)] == [1, 1, 2, 3] and small_geometry(N_L256).lanes == 256
assert small_geometry(N_GMAX).G == max(small_geometry(n).G for n in range(1, N_MAX + 1)) == S.SMALL_PARTS_MAX
assert small_geometry(N_C6).c == small_geometry(N_MAX).c == 6 and small_geometry(N_R3).c == 7
assert small_geometry(N_MAX).r == max(small_geometry(n).r for n in range(1, N_MAX + 1))


# ---- digits: msm_small_digits_body ---------------------------------------------------------------------------------------------------------
def windows(c: int) -> int:
    return _ceil_div(255, c)


def digit_bytes(s: int, c: int) -> list:
    """the W bytes sign << 7 | magnitude of the canonical scalar s, read as the kernel reads them: eight 32-bit words and a zero word
    above, a window taken from the 64 bits of two neighbouring words; a digit of magnitude 0 is the byte 0 whatever its carry"""
    assert 0 <= s < R
    limbs = [(s >> (32 * k)) & 0xFFFFFFFF for k in range(8)] + [0]
    half, mask, carry, out = 1 << (c - 1), (1 << c) - 1, 0, []
    for w in range(windows(c)):
        bit = w * c
        limb, sh = bit >> 5, bit & 31
        raw = (((limbs[limb + 1] << 32 | limbs[limb]) >> sh) & mask) if limb < 8 else 0
        d = raw + carry
        mag, neg, carry = d, 0, 0
        if d > half:
            mag, neg, carry = (1 << c) - d, 1, 1
        out.append((neg << 7 | mag) if mag else 0)
    assert carry == 0
    return out


def signed(byte: int) -> int:
    return -(byte & 0x7F) if byte >> 7 else byte


def from_digits(digits: dict, c: int) -> int:
    """the scalar whose signed digits are exactly {window: digit}, in (-2^(c-1), 2^(c-1)]; the top non-zero digit must be positive"""
    s = sum(d << (c * w) for w, d in digits.items())
    assert 0 <= s < R, digits
    got = [signed(b) for b in digit_bytes(s, c)]
    assert all(got[w] == digits.get(w, 0) for w in range(windows(c))), (digits, got)
    return s


# ---- bases with known discrete logarithms -----------------------------------------------------------------------------------------------
IDENTITY_AT = 7  # in every base set
SMALL_PERIOD = 64  # the small logarithms repeat every 256 points: m_(i + 256) = m_i


@functools.lru_cache(maxsize=None)
def logs(n: int) -> tuple:
    """m_i of the bases P_i = m_i G of the size-n base set, by i mod 4 with x = i >> 2: 2^(c (x mod W)) (points that differ by powers of
    the window: partial sums of different windows can be equal), 3 + x mod 64 (small, repeating every 256 points: the cells of one lane
    of 256), then the negatives r - m of the two.  Point 7 is the identity, and so is the small point with x mod 64 = 60 + j of the
    j-th run of 256 points, j mod 4 < 3: first, second and third in the chains of three lanes."""
    g = small_geometry(n)
    out = []
    for i in range(n):
        x, kind = i >> 2, i & 3
        m = pow(2, g.c * (x % g.W), R) if kind % 2 == 0 else 3 + x % SMALL_PERIOD
        if kind == 1 and (i // 256) % 4 < 3 and x % SMALL_PERIOD == 60 + (i // 256) % 4:
            m = 0
        out.append((R - m) % R if kind >= 2 else m)
    out[IDENTITY_AT] = 0
    return tuple(out)


def factored(n: int, i: int) -> tuple:
    """(sign, mantissa, window exponent) with m_i = sign * mantissa * 2^(c * exponent), or None for the identity"""
    m = logs(n)[i]
    if m == 0:
        return None
    g = small_geometry(n)
    x, kind = i >> 2, i & 3
    sign = -1 if kind >= 2 else 1
    return (sign, 1, x % g.W) if kind % 2 == 0 else (sign, 3 + x % SMALL_PERIOD, 0)


@functools.lru_cache(maxsize=None)
def bases(n: int) -> np.ndarray:
    b = points_of(logs(n))
    b.setflags(write=False)
    return b


# ---- the partition and the trees: k_msm_small_accum, seg_tree_sum, small_finish ---------------------------------------------------------------
def pair_class(a: int, b: int) -> str:
    if a == 0 and b == 0:
        return BOTH
    if a == 0 or b == 0:
        return IDENT
    return EQUAL if a == b else OPPOSITE if (a + b) % R == 0 else GENERAL


def tree(values: list) -> tuple:
    """seg_tree_sum over one segment of len(values) = a power of two: (sum, {(h, t): class of the pair (t, t + h)} without BOTH)"""
    X, cls = list(values), {}
    h = len(X) >> 1
    while h:
        for t in range(h):
            k = pair_class(X[t], X[t + h])
            if k != BOTH:
                cls[(h, t)] = k
            X[t] = (X[t] + X[t + h]) % R
        h >>= 1
    return X[0], cls


def place(geo, n: int, w: int, i: int) -> tuple:
    """(workgroup, step k of the lane's chain, lane) of the cell of point i in window w of an MSM over n points"""
    b, rem = divmod(w * n + i, geo.lanes * geo.r)
    k, tid = divmod(rem, geo.lanes)
    return b, k, tid


def live_lanes(geo, n: int, b: int) -> int:
    return min(n * geo.W - b * geo.lanes * geo.r, geo.lanes)


class Model(NamedTuple):
    geo: S.Geometry  # of the registered base set
    n: int
    G: int  # workgroups of this MSM
    digits: np.ndarray  # [W][n] bytes
    cnt: list  # [G] additions of each workgroup's lanes
    part: list  # [G] partial sums, multiples of the generator
    result: int
    chain: dict  # (workgroup, lane) -> classes of the chain's steps, in order (SKIPPED for an identity table point)
    tree1: dict  # (workgroup, h, t) -> class, pairs of two identities left out
    tree2: dict  # (h, t) -> class, likewise

    @property
    def entries(self):
        return sum(self.cnt)


def model(n_reg: int, scalars) -> Model:
    geo, k_of = small_geometry(n_reg), logs(n_reg)
    n = len(scalars)
    assert 1 <= n <= n_reg and geo.table
    c, W, per = geo.c, geo.W, geo.lanes * geo.r
    G = _ceil_div(n * W, per)
    digits = np.zeros((W, n), dtype=np.uint8)
    live = []
    for i, s in enumerate(scalars):
        if s:
            for w, byte in enumerate(digit_bytes(s, c)):
                if byte:
                    digits[w, i] = byte
                    live.append((w * n + i, w, i, byte))
    live.sort()
    pw = [pow(2, c * w, R) for w in range(W)]
    cnt, sums, chain = [0] * G, {}, {}
    for cell, w, i, byte in live:
        b, k, tid = place(geo, n, w, i)
        steps = chain.setdefault((b, tid), [])
        if k_of[i] == 0:
            steps.append(SKIPPED)
            continue
        val = (byte & 0x7F) * pw[w] * k_of[i] % R
        if byte >> 7:
            val = R - val
        lanes = sums.setdefault(b, {})
        steps.append(pair_class(lanes.get(tid, 0), val))
        lanes[tid] = (lanes.get(tid, 0) + val) % R
        cnt[b] += 1
    part, tree1 = [0] * G, {}
    for b, lanes in sums.items():
        nlive = live_lanes(geo, n, b)
        X = [0] * _pow2_at_least(nlive)
        for tid, v in lanes.items():
            assert tid < nlive
            X[tid] = v
        part[b], cls = tree(X)
        tree1.update({(b, h, t): k for (h, t), k in cls.items()})
    result, tree2 = tree(part + [0] * (_pow2_at_least(G) - G))
    return Model(geo, n, G, digits, cnt, part, result, {key: tuple(v) for key, v in chain.items()}, tree1, tree2)


def table_log(n_reg: int, j: int, w: int, i: int) -> int:
    """the discrete logarithm of the table entry M[j][w][i] = j 2^(c w) P_i"""
    return j * pow(2, small_geometry(n_reg).c * w, R) * logs(n_reg)[i] % R


def table_entry(n_reg: int, j: int, w: int, i: int) -> int:
    """its index in the table [2^(c-1)][W][n_reg]"""
    return ((j - 1) * small_geometry(n_reg).W + w) * n_reg + i


def table_samples(n_reg: int) -> list:
    """the (w, i) whose every multiple is read: both end windows, a middle one, both end points, an identity base and one of each kind"""
    W = small_geometry(n_reg).W
    return [(0, 0), (0, 1), (1, 2), (W // 2, IDENTITY_AT), (W // 2, 3), (W - 1, n_reg - 1), (W - 1, 4 % n_reg), (W - 2, n_reg // 2)]


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    family: str
    n_reg: int
    scalars: tuple  # n <= n_reg canonical integers
    expect: dict  # the property: any of chain {(b, lane): classes}, tree1 {(b, h, t): class}, tree2 {(h, t): class}, digits
    # {(w, i): signed digit}, G, live (lanes of the last workgroup), result, entries
    principal: bool = False  # also runs through every entry form

    @property
    def n(self):
        return len(self.scalars)

    @property
    def id(self):
        return f"{self.family}-{self.name}"


_MODELS = {}


def model_of(case: Case) -> Model:
    key = (case.id, case.n_reg, case.n)
    if key not in _MODELS:
        _MODELS[key] = model(case.n_reg, case.scalars)
    return _MODELS[key]


def scalars_of(n_reg: int, n: int, digits: dict) -> tuple:
    """the column of n scalars with the digits {point: {window: digit}}, zero elsewhere"""
    c = small_geometry(n_reg).c
    assert all(i < n for i in digits)
    return tuple(from_digits(digits[i], c) if i in digits else 0 for i in range(n))


def dense_scalar(c: int, i: int) -> int:
    """a scalar with every digit live, positive and negative, differing from point to point"""
    W, half = windows(c), 1 << (c - 1)
    dg = {w: (1 + (5 * i + 3 * w) % (half - 1)) * (-1 if (i + w) % 3 == 0 else 1) for w in range(W - 1)}
    dg[W - 1] = 1
    return from_digits(dg, c)


# -- digits
def digit_scalars(c: int) -> dict:
    """name -> scalar: the edge scalars of every window (tests/table_depth_cases.py: 2^(c w) - 1, the digit 2^(c-1), that plus 1, the first
    negative digit), the ends of the field, runs of all-ones windows under a carry (bytes 0 while the carry travels), and scalars whose
    only live digit sits in a window that straddles two 32-bit words or in the top window (which reads the zero word above the top)"""
    W, half, ones = windows(c), 1 << (c - 1), (1 << c) - 1
    out = dict(T.edge_scalars(c))
    for a, b in ((0, W - 1), (3, 9), (W - 6, W - 1)):
        out[f"carry from {a} to {b}"] = ((half + 1) << (c * a)) + sum(ones << (c * w) for w in range(a + 1, b))
    for w in range(W):
        if (w * c) % 32 + c > 32 or w == W - 1:
            top = (R >> (c * w)) - 1 if w == W - 1 else half
            for d in sorted({1, top - 1, top} - {0}):
                out[f"only digit {d} in window {w}"] = from_digits({w: d}, c)
            if w < W - 1:
                out[f"all ones in window {w}"] = ones << (c * w)
    return out


def _digit_cases() -> list:
    out = []
    for n_reg in (N_TREE, N_C6):
        c = small_geometry(n_reg).c
        named = digit_scalars(c)
        names, col = list(named), [named[k] for k in named]
        per = n_reg if n_reg == N_TREE else len(col)
        for j in range(0, len(col), per):
            sc = tuple(col[j:j + per])
            exp = {"digits": {}}
            for i, s in enumerate(sc):
                name = names[j + i]
                if name.startswith("half at") and "plus" not in name:
                    exp["digits"][(int(name.split()[2]), i)] = 1 << (c - 1)
                elif name.startswith("half+1 at") and int(name.split()[2]) < windows(c) - 1:
                    exp["digits"][(int(name.split()[2]), i)] = -((1 << (c - 1)) - 1)
                elif name.startswith("carry from"):
                    a, b = int(name.split()[2]), int(name.split()[4])
                    exp["digits"].update({(w, i): 0 for w in range(a + 1, b)})
                    exp["digits"][(b, i)] = 1
            out.append(Case(f"c{c}-edge-scalars-{j // per}", "digits", n_reg, sc, exp, principal=(j == 0)))
    return out


# -- lane chains
def _chain_case(n_reg: int) -> Case:
    """One column whose live digits sit in chosen lanes of workgroup 0 (window 0: the lane of point t holds t, t + 256, ...) and in the
    workgroup whose cells cross from window 0 to window 1."""
    geo = small_geometry(n_reg)
    r, c = geo.r, geo.c
    assert geo.lanes == 256 and r >= 2 and 256 * r <= n_reg
    dg, exp = {}, {}

    def lane(t: int, digits: list, classes: tuple):
        """digits[k] for the k-th cell of lane t of workgroup 0; a negative digit carries 1 into the point's next window"""
        for k, d in enumerate(digits):
            if d:
                i = t + 256 * k
                assert place(geo, n_reg, 0, i) == (0, k, t)
                dg[i] = {0: d, 1: 1} if d < 0 else {0: d}
        exp[(0, t)] = classes

    small = lambda x: 4 * x + 1  # the point with the small logarithm 3 + x, x < 60; the same in every run of 256
    last = r - 1
    lane(small(1), [9, 9], (IDENT, EQUAL))  # acc = P, then the same point
    lane(small(2), [9, -9] + ([5] if r > 2 else []), (IDENT, OPPOSITE) + ((IDENT,) if r > 2 else ()))  # P, -P, then a third point
    if r > 2:
        lane(small(3), [7, 7, -14], (IDENT, EQUAL, OPPOSITE))  # to the identity through a doubling
    lane(small(4), [0, 0, 11][3 - min(r, 3):], (IDENT,))  # zero digits first, a live one behind them
    lane(small(5), [11] + [0] * (last - 1) + [13], (IDENT, GENERAL))  # a zero digit between two live ones (r > 2)
    lane(small(6), [3 + k for k in range(r)], (IDENT,) + (GENERAL,) * last)  # the whole chain live
    lane(small(6) + 2, [3 + k for k in range(r)], (IDENT,) + (GENERAL,) * last)  # the same over the negated bases
    for j in range(min(r, 3)):  # the identity base first, in the middle (r > 2), last: the run of 256 that holds it is j mod 4
        ks = [k for k in range(r) if k % 4 == j]
        classes, seen = [], False
        for k in range(r):
            classes.append(SKIPPED if k in ks else GENERAL if seen else IDENT)
            seen = seen or k not in ks
        lane(small(60 + j), [5 + k for k in range(r)], tuple(classes))
    # the workgroup in which the cells pass from window 0 to window 1: every lane of it that has cells of both windows
    b = n_reg // (256 * r)
    crossing = [t for t in range(256) if b * 256 * r + t < n_reg <= b * 256 * r + last * 256 + t]
    t = next(t for t in crossing if (b * 256 * r + t) % 4 == 1 and logs(n_reg)[b * 256 * r + t])
    for k in range(r):
        w, i = divmod(b * 256 * r + 256 * k + t, n_reg)
        assert w <= 1 and place(geo, n_reg, w, i) == (b, k, t)
        if logs(n_reg)[i] and i not in dg:
            dg.setdefault(i, {})[w] = 2 + k
    assert {w for i in dg for w in dg[i]} >= {0, 1}
    case = Case(f"r{r}-c{c}-lanes-of-workgroup-0-and-a-window-crossing", "chains", n_reg, scalars_of(n_reg, n_reg, dg), {"chain": exp, "crossing": (b, t)}, principal=True)
    return case


# -- trees
def _cell_value(n_reg: int, n: int, cell: int):
    """(window, point, sign, mantissa, exponent): the cell's table point is sign * mantissa * 2^(c exponent) G at digit 1"""
    w, i = divmod(cell, n)
    f = factored(n_reg, i)
    return None if f is None else (w, i, f[0], f[1], w + f[2])


def solve_pair(n_reg: int, n: int, cells_a, cells_b, opposite: bool, negative: bool = False):
    """the first (cell a, digit, cell b, digit) whose two values are equal (or opposite): None if there is none.  The digits are positive;
    with `negative` the second may be negative where the signs of the two bases ask for it (its point then has a digit 1 one window up)"""
    W = small_geometry(n_reg).W
    half = 1 << (small_geometry(n_reg).c - 1)
    by_exp = {}
    for cb in cells_b:
        vb = _cell_value(n_reg, n, cb)
        if vb:
            by_exp.setdefault(vb[4], []).append((cb, vb))
    for ca in cells_a:
        va = _cell_value(n_reg, n, ca)
        for cb, vb in by_exp.get(va[4], []) if va else []:
            flip = (va[2] * vb[2] < 0) != opposite
            if cb == ca or (flip and not (negative and vb[0] < W - 2)):
                continue
            g = gcd(va[3], vb[3])
            da, db = vb[3] // g, va[3] // g
            if da <= half and db < half:
                return ca, da, cb, -db if flip else db
    return None


def _digits_at(n: int, picks) -> dict:
    dg = {}
    for cell, d in picks:
        w, i = divmod(cell, n)
        for ww, dd in ((w, d), (w + 1, 1))[:2 if d < 0 else 1]:
            assert ww not in dg.get(i, {})
            dg.setdefault(i, {})[ww] = dd
    return dg


def _tree1_cases(n_reg: int) -> list:
    """per class, one column: level h of the first tree is engineered in a workgroup of its own (two live lanes t and t + h, nothing else
    in the workgroup), for every level and class that has a solution"""
    geo = small_geometry(n_reg)
    assert geo.r == 1
    out = []
    for opposite in (False, True):
        picks, exp, b, h = [], {}, 0, geo.lanes >> 1
        while h:
            found = None
            for bb in range(b, geo.G - 1):  # (not the ragged last one)
                base = bb * geo.lanes
                for t in range(h):
                    found = solve_pair(n_reg, n_reg, [base + t], [base + t + h], opposite, negative=True)
                    if found:
                        break
                if found:
                    b = bb + 5  # (a negative digit's carry lands in one of the next four workgroups)
                    break
            if found:
                picks += [(found[0], found[1]), (found[2], found[3])]
                exp[(bb, h, t)] = OPPOSITE if opposite else EQUAL
            h >>= 1
        kind = "opposite" if opposite else "equal"
        out.append(Case(f"first-tree-{geo.lanes}-lanes-{kind}-pairs-level-by-level", "trees", n_reg, scalars_of(n_reg, n_reg, _digits_at(n_reg, picks)),
                        {"tree1": exp}, principal=not opposite))
    return out


def _ragged_n(n_reg: int, pred) -> int:
    geo = small_geometry(n_reg)
    return next(n for n in range(2, n_reg) if _ceil_div(n * geo.W, geo.lanes * geo.r) > 1 and pred(live_lanes(geo, n, _ceil_div(n * geo.W, geo.lanes * geo.r) - 1)))


def _ragged_cases(n_reg: int) -> list:
    """prefix MSMs, every digit live, whose last workgroup has 1, a power of two (not the full width) and a power of two plus one live lanes"""
    geo = small_geometry(n_reg)
    out = []
    for name, pred in (("1", lambda v: v == 1), ("a-power-of-two", lambda v: 4 <= v < geo.lanes and v & (v - 1) == 0),
                       ("a-power-of-two-plus-one", lambda v: v >= 5 and (v - 1) & (v - 2) == 0)):
        n = _ragged_n(n_reg, pred)
        G = _ceil_div(n * geo.W, geo.lanes * geo.r)
        out.append(Case(f"last-workgroup-of-{geo.lanes}-lanes-has-{name}-live", "trees", n_reg, tuple(dense_scalar(geo.c, i) for i in range(n)),
                        {"G": G, "live": live_lanes(geo, n, G - 1)}))
    return out


def _n_with_G(n_reg: int, G: int) -> int:
    geo = small_geometry(n_reg)
    return next(n for n in range(1, n_reg + 1) if _ceil_div(n * geo.W, geo.lanes * geo.r) == G)


def _tree2_cases(n_reg: int, G: int, label: str) -> list:
    """one column per level and class that has a solution: the only two live cells sit in workgroups t and t + h, so the pair (t, t + h)
    of level h of the second tree adds two equal (opposite) partial sums and every other pair of the tree has an identity in it"""
    n = _n_with_G(n_reg, G) if G < small_geometry(n_reg).G else n_reg
    geo = small_geometry(n_reg)
    per = geo.lanes * geo.r
    assert _ceil_div(n * geo.W, per) == G
    out = []
    if G == 1:
        sc = tuple(dense_scalar(geo.c, i) for i in range(n))
        return [Case(f"second-tree-of-{label}-partial-sum", "trees", n_reg, sc, {"G": 1})]
    h = _pow2_at_least(G) >> 1
    while h:
        for opposite in (False, True):
            found = None
            for t in range(min(h, G - h)):
                cells = lambda b: range(b * per, min((b + 1) * per, n * geo.W))
                found = solve_pair(n_reg, n, cells(t), cells(t + h), opposite)
                if found:
                    break
            if found:
                kind = OPPOSITE if opposite else EQUAL
                dg = _digits_at(n, [(found[0], found[1]), (found[2], found[3])])
                out.append(Case(f"second-tree-of-{label}-partial-sums-{kind}-pair-at-level-{h}", "trees", n_reg, scalars_of(n_reg, n, dg),
                                {"G": G, "tree2": {(h, t): kind}}, principal=(h == 1 and not opposite and G == small_geometry(n_reg).G)))
        h >>= 1
    return out


def _tree_cases() -> list:
    out = _tree1_cases(N_TREE) + _tree1_cases(N_L256) + _ragged_cases(N_TREE) + _ragged_cases(N_L256)
    out += _tree2_cases(N_TREE, 1, "1") + _tree2_cases(N_TREE, 32, "32") + _tree2_cases(N_TREE, 33, "33") + _tree2_cases(N_GMAX, small_geometry(N_GMAX).G, "512")
    return out


# -- the identity
def _identity_cases() -> list:
    out = []
    for n_reg in (N_TREE, N_R2):
        c = small_geometry(n_reg).c
        n = n_reg - n_reg % 4
        col = [dense_scalar(c, i >> 2 << 1 | (i & 1)) for i in range(n)]  # points i and i + 2 are P and -P: the same scalar
        for i in range(n):  # (an identity base has no partner)
            if logs(n_reg)[i] == 0:
                col[i ^ 2] = 0
        out.append(Case(f"{n}-points-sum-to-the-identity", "identity", n_reg, tuple(col), {"result": 0}, principal=(n_reg == N_TREE)))
        out.append(Case(f"{n_reg}-zero-scalars", "identity", n_reg, (0,) * n_reg, {"result": 0, "entries": 0}))
    return out


# -- state
def full_column(n_reg: int) -> Case:
    c = small_geometry(n_reg).c
    return Case(f"{n_reg}-points-every-digit-live", "state", n_reg, tuple(dense_scalar(c, i) for i in range(n_reg)), {})


def prefix_columns(n_reg: int) -> list:
    """the prefix MSMs that follow the full column in the same slot: their digits differ from the full column's everywhere"""
    c = small_geometry(n_reg).c
    return [Case(f"prefix-{n}-of-{n_reg}", "state", n_reg, tuple(dense_scalar(c, i + 1) for i in range(n)), {}) for n in (n_reg - 1, n_reg // 2, 1)]


def phase_columns(n_reg: int, count: int = 4) -> list:
    """`count` columns of one length for the phase entry, the second all zero"""
    c = small_geometry(n_reg).c
    cols = [Case(f"phase-column-{j}-of-{n_reg}", "state", n_reg, tuple(dense_scalar(c, 3 * i + j) if (i + j) % 3 else 0 for i in range(n_reg)), {}) for j in range(count)]
    if count > 1:
        cols[1] = Case(f"phase-column-1-of-{n_reg}-all-zero", "state", n_reg, (0,) * n_reg, {"entries": 0})
    return cols


def nine_columns(n_reg: int) -> list:
    """nine columns of different lengths (different G) for nine deferred MSMs before one join"""
    c = small_geometry(n_reg).c
    return [Case(f"deferred-{j}-of-nine", "state", n_reg, tuple(dense_scalar(c, i + 2 * j) for i in range(n_reg - 13 * j)), {}) for j in range(9)]


STATE_SIZES = (N_TREE, N_R2)


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = _digit_cases() + [_chain_case(n) for n in (N_R2, N_R3, N_MAX)] + _tree_cases() + _identity_cases()
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return tuple(out)


def all_cases() -> tuple:
    out = list(cases())
    for n in STATE_SIZES:
        out += [full_column(n)] + prefix_columns(n)
    out += phase_columns(N_TREE) + phase_columns(N_TREE, 3) + phase_columns(N_L256, 1) + nine_columns(N_TREE)
    return tuple({c.id: c for c in out}.values())


# ---- what the cases reach ------------------------------------------------------------------------------------------------------------------
def reached() -> dict:
    """(tree, width, level, class) -> a case that has it, over `cases()`: tree 1 by lanes per workgroup, tree 2 by padded width"""
    out = {}
    for case in cases():
        m = model_of(case)
        for (b, h, t), k in m.tree1.items():
            out.setdefault((1, m.geo.lanes, h, k), case.id)
        for (h, t), k in m.tree2.items():
            out.setdefault((2, _pow2_at_least(m.G), h, k), case.id)
    return out


def wanted() -> list:
    """every (tree, width, level, class) with class equal / opposite / identity operand of the widths the tree cases are built for"""
    out = [(1, lanes, h, k) for lanes in (128, 256) for h in (1 << e for e in range(lanes.bit_length() - 1)) if h < lanes for k in (EQUAL, OPPOSITE, IDENT)]
    out += [(2, T2, h, k) for T2 in (32, 64, 512) for h in (1 << e for e in range(T2.bit_length() - 1)) if h < T2 for k in (EQUAL, OPPOSITE, IDENT)]
    return out


# The combinations of `wanted` that no case reaches, as the host test computes them: with 33 partial sums the one pair of the top level is
# (workgroup 0, workgroup 32), 36 windows apart, and the 111 points of that MSM hold no two bases that differ by 2^(36 c).
NOT_REACHED = ((2, 64, 32, EQUAL), (2, 64, 32, OPPOSITE))
