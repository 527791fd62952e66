"""The G1 group law of csrc/g1_29.cuh at the bounds of its coordinate invariants: operand builders and big-integer checks shared by
tests/test_g1_29_edges_host.py (the g++ build of the header) and tests/test_gpu_g1_29_edges.py (the device build and the
lane-cooperative forms of g1_29_quad.cuh), through `point_raw(op, a, b)` of the two back ends of tests/f29_cases.py.

Python integers only, deterministic.  The reference is the oracle's group law on values mod q (oracle/bn254.py g1_add / g1_neg).
A coordinate is a Montgomery-2^261 word w (it stands for w / 2^261 mod q), possibly lifted by a multiple of p; a point (x, y) has the
representatives (x l^2, y l^3, l^2, l^3).  What the cases put at the bounds the header states:
  * table coordinates whose canonical word is an extreme one (WORDS below);
  * representatives whose X or ZZ word is exactly an extreme word (l^2 chosen by a square root), whose Y or ZZZ word is the best of
    a fixed search over 2^16 l's, and whose lifted X / ZZ has limbs 0..7 all ones just under the bound;
  * every coordinate lifted by multiples of p to the top of its documented range, keeping the f29_sub margin of 2^232:
    X < 6p, Y < 4p, ZZ and ZZZ < 1.1p (xyzz29_madd) or < 1.5p (xyzz29_add / xyzz29_dbl), Z < 8p (xyzz29_from_jacobian) — one
    coordinate alone at its top, all together, all at the bottom;
  * y2 plain and as the lazy 2p - y2 with the limbs f29_sub(0, y, K2) leaves;
  * P + P, P + (-P), identity operands through those same representatives.
Checked on every element: the value (the oracle's group element, ZZ^3 = ZZZ^2, the identity all zero) and closure (normalized
limbs, values below the bound the header derives for that function — BOUNDS below, in units of p, copied from the comments of
g1_29.cuh, not fitted to the code; where a branch makes the derived bound inapplicable the function's stated invariant)."""
import functools

import numpy as np

from oracle import bn254 as o

Q = o.Q
M29 = (1 << 29) - 1
R261 = 1 << 261
_RINV = pow(R261, -1, Q)
MARGIN = 1 << 232  # f29_sub(a, b, k p) promises no underflow while value(b) < k p - 2^232

K2 = [0x30f9fa8e, 0x2208c16c, 0x38e5469d, 0x25aa45a0, 0x2b0bb2ef, 0x25b68180, 0x214dc281, 0x3cb84c67, 0x0060c89b]  # Fq29::K2


def mont(v):
    return v * R261 % Q


def unmont(w):
    return w * _RINV % Q


def limbs(v):
    """normalized limbs of an integer below 2^261"""
    assert 0 <= v < R261
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def limb_val(row):
    return sum(int(x) << (29 * i) for i, x in enumerate(row))


def lazy_neg(yw):
    """f29_sub(0, y, K2) of a canonical word: 2p - y with un-normalized limbs"""
    ly = limbs(yw)
    out = [K2[i] - ly[i] for i in range(9)]
    assert all(0 <= v < (1 << 32) for v in out) and limb_val(out) == 2 * Q - yw
    return out


def sqrt(a):
    r = pow(a, (Q + 1) // 4, Q)  # q = 3 mod 4
    return r if r * r % Q == a % Q else None


assert K2 == [v + (1 << 29) - (1 if i else 0) if i < 8 else v - 1 for i, v in enumerate(limbs(2 * Q))]

# ---- the extreme words ----------------------------------------------------------------------------------------------------------------
ONES232 = (1 << 232) - 1
WORDS = [Q - 1, (((Q >> 232) - 1) << 232) | ONES232, ONES232, 1 << 232, 1, M29, Q >> 1]
# small words: W + p is a legal ZZ under the 1.1p / the 1.5p invariant
SMALL_WORDS = [Q // 10 - 1, (((Q // 2) >> 232) << 232) - 1]
assert all(10 * (w + Q) < 11 * Q for w in (SMALL_WORDS[0], ONES232, 1 << 232, 1, M29)) and all(2 * (w + Q) < 3 * Q for w in SMALL_WORDS + [Q >> 1])

X_LIMIT, Y_LIMIT, Z_LIMIT = 6 * Q - MARGIN, 4 * Q - MARGIN, 8 * Q - MARGIN
ZZ_MADD, ZZ_ADD = (11 * Q + 9) // 10, (3 * Q + 1) // 2  # ZZ, ZZZ < 1.1p / < 1.5p as integers: value < ceil(bound)


def lift(word, limit, kmax):
    """the largest word + k p below `limit`, k <= kmax"""
    k = min(kmax, (limit - 1 - word) // Q)
    assert k >= 0
    return word + k * Q


@functools.lru_cache(None)
def curve_points():
    """both roots over extreme table x's (x's canonical Mont261 word is T, or the nearest below it with x^3 + 3 a square), the
    generator and its negative, three random multiples of it"""
    pts = []
    for T in WORDS:
        while True:
            x = unmont(T)
            y = sqrt((x * x * x + 3) % Q)
            if y and (x, y) not in pts:  # 2^232 walks down onto 2^232 - 1's point when its own x is on no curve point: go on
                break
            T -= 1
        pts += [(x, y), (x, Q - y)]
    pts += [(1, 2), (1, Q - 2)]
    rng = np.random.default_rng(2929)
    pts += [o.g1_mul(int.from_bytes(rng.bytes(31), "little") + 1, o.G1_GEN) for _ in range(3)]
    assert all(o.is_on_curve(p) for p in pts)
    return pts


def _solve_square(word, divisor, step=1):
    """l with mont(divisor * l^2) == W for the first W = word, word - step, ... that has one (upward from the word 1, which has
    nothing below it)"""
    dinv = pow(divisor, -1, Q)
    if word <= step:
        step = -step
    while True:
        lam = sqrt(unmont(word) * dinv % Q)
        if lam:
            assert mont(divisor * lam * lam % Q) == word
            return lam
        word -= step
        assert 0 < word < Q


def _ones_under(limit):
    """the largest value below `limit` whose limbs 0..7 are all ones"""
    return ((limit >> 232) << 232) - 1


SEARCH = 1 << 16


def _search_cube(factor, seed):
    """l's among a fixed window of 2^16 (its start drawn from `seed`) whose word mont(factor * l^3) — a Y or a ZZZ, which no square
    root can place — has the most all-ones low limbs (then the most set bits in them: an all-ones limb is a 2^-29 event), is the
    smallest, is the largest"""
    lam0 = int(np.random.default_rng(seed).integers(2, 1 << 62))
    f = mont(factor)
    ones, lo, hi = ((-1, -1), 0), (Q, 0), (-1, 0)
    for lam in range(lam0, lam0 + SEARCH):
        w = f * (lam * lam * lam % Q) % Q
        if w < lo[0]:
            lo = (w, lam)
        if w > hi[0]:
            hi = (w, lam)
        low = w & ONES232
        key = (sum(((low >> s) & M29) == M29 for s in range(0, 232, 29)), bin(low).count("1"))
        if key > ones[0]:
            ones = (key, lam)
    return [ones[1], lo[1], hi[1]]


@functools.lru_cache(None)
def _zz_lambdas():
    """l's that put ZZ = l^2 exactly at an extreme word, ZZ + p all ones just under 1.1p and 1.5p, and ZZZ = l^3 at the search's picks"""
    out = [_solve_square(W, 1) for W in WORDS + SMALL_WORDS]
    out += [_solve_square(_ones_under(lim) - Q, 1, MARGIN) for lim in (ZZ_MADD, ZZ_ADD)]
    return out + _search_cube(1, 29)


@functools.lru_cache(None)
def lambdas(idx):
    """the l's of point idx: its X at each extreme word and all ones just under 6p, the ZZ / ZZZ ones, and (three points) its Y"""
    x, y = curve_points()[idx]
    out = [_solve_square(W, x) for W in WORDS + SMALL_WORDS]
    A = _ones_under(X_LIMIT)
    out.append(_solve_square(A - (A // Q) * Q, x, MARGIN))
    out += _zz_lambdas()
    if idx in (0, 14, 16):
        out += _search_cube(y, 31 + idx)
    return out


def canonical_words(p, lam):
    x, y = p
    l2, l3 = lam * lam % Q, lam * lam * lam % Q
    return (mont(x * l2 % Q), mont(y * l3 % Q), mont(l2), mont(l3))


def representatives(words, zz_limit):
    """one coordinate alone at the top of its range (the others canonical), all at their tops, all at the bottom"""
    tops = (lift(words[0], X_LIMIT, 5), lift(words[1], Y_LIMIT, 3), lift(words[2], zz_limit, 1), lift(words[3], zz_limit, 1))
    reps = [tuple(words)]
    for i in range(4):
        r = list(words)
        r[i] = tops[i]
        reps.append(tuple(r))
    reps.append(tops)
    return list(dict.fromkeys(reps))


def xyzz_row(rep):
    return [v for c in rep for v in limbs(c)]


ZERO36 = [0] * 36

# ---- bounds: (X, Y, ZZ, ZZZ) in thousandths of p, from the comments of g1_29.cuh ----------------------------------------------------------
BOUNDS = {
    "madd": (5149, 1240, 1010, 1010),        # X3 < 5.149, Y3 < 1.24, ZZ3 and ZZZ3 < 1.01
    # an identity accumulator takes (x2, normalize(y2), 1, 1): Y is the lazy 2p - y2 itself, no derived bound: the acc invariant
    "madd_first": (6000, 4000, 1100, 1100),
    # the doubling branch of madd is xyzz29_dbl_affine: X3 < 5.1, Y3 < 1.2; ZZ = V < 1.1 and ZZZ = W are fresh products of U < 4,
    # not products with PP: ZZ3 < 1.01 does not apply, the acc invariant does
    "dbl_affine": (5100, 1200, 1100, 1100),
    "dbl": (5100, 1200, 1020, 1020),         # X3 < 5.1, Y3 < 1.2, ZZ3 and ZZZ3 < 1.02
    "add": (5100, 1200, 1500, 1500),         # X3 < 5.1, Y3 < 1.2; no ZZ / ZZZ output bound stated: the in / out invariant
    "pass": (6000, 4000, 1500, 1500),        # add with an identity operand returns the other one untouched: the in / out invariant
}


def _check_xyzz(row, want, cls, tag, bounds):
    """row: 36 output words.  Value: the oracle's point, ZZ^3 = ZZZ^2, the identity all zero.  Closure: normalized, below BOUNDS[cls]"""
    c = [limb_val(row[9 * i : 9 * i + 9]) for i in range(4)]
    if want is None:
        assert not any(int(v) for v in row), tag
        return
    assert all(int(v) <= M29 for i in range(4) for v in row[9 * i : 9 * i + 8]), tag
    X, Y, ZZ, ZZZ = (unmont(v) for v in c)
    assert ZZ != 0, tag
    assert pow(ZZ, 3, Q) == ZZZ * ZZZ % Q, tag
    assert (X * pow(ZZ, -1, Q) % Q, Y * pow(ZZZ, -1, Q) % Q) == want, tag
    for name, v, b in zip(("X", "Y", "ZZ", "ZZZ"), c, bounds[cls]):
        assert 1000 * v < b * Q, (tag, cls, name, v / Q)


# ---- the cases of each op: (A rows, B rows, [(want, class)]) -------------------------------------------------------------------------------
def _partner(i):
    """another point with another x (the extreme points come as +- pairs)"""
    pts = curve_points()
    j = (i + 3) % len(pts)
    assert pts[j][0] != pts[i][0]
    return j


def _table_forms(p):
    """(x2, y2) rows of the table point p and the point each stands for: plain, and y2 as the lazy 2p - y2 (which is -p)"""
    xw, yw = mont(p[0]), mont(p[1])
    return [(limbs(xw) + limbs(yw) + [0] * 18, p), (limbs(xw) + lazy_neg(yw) + [0] * 18, o.g1_neg(p))]


@functools.lru_cache(None)
def madd_cases():
    pts = curve_points()
    A, B, want = [], [], []
    for i, p in enumerate(pts):
        forms = _table_forms(pts[_partner(i)])
        for lam in lambdas(i):
            for rep in representatives(canonical_words(p, lam), ZZ_MADD):
                for row, t in forms:
                    A.append(xyzz_row(rep)); B.append(row); want.append((o.g1_add(p, t), "madd"))
        # P + P (the doubling branch), P + (-P) (the identity), each reached with y2 plain and lazy, from representatives at the
        # bounds: f29_is_zero_mod(pp) / (rr) must decide on a P = k p, R = k' p with k up to 7 / 5
        for lam in lambdas(i)[::4]:
            for rep in representatives(canonical_words(p, lam), ZZ_MADD):
                for row, t in _table_forms(p) + _table_forms(o.g1_neg(p)):
                    s = o.g1_add(p, t)
                    A.append(xyzz_row(rep)); B.append(row); want.append((s, "dbl_affine" if s else None))
        for row, t in _table_forms(p):  # an identity accumulator
            A.append(ZERO36); B.append(row); want.append((t, "madd_first"))
    return np.array(A, dtype=np.uint32), np.array(B, dtype=np.uint32), want


@functools.lru_cache(None)
def _add_reps():
    """every representative under the xyzz29_add / xyzz29_dbl invariant, with its point's index"""
    pts = curve_points()
    return [(i, rep) for i, p in enumerate(pts) for lam in lambdas(i) for rep in representatives(canonical_words(p, lam), ZZ_ADD)]


@functools.lru_cache(None)
def dbl_cases():
    pts = curve_points()
    reps = _add_reps()
    A = [xyzz_row(rep) for _, rep in reps] + [ZERO36]
    want = [(o.g1_double(pts[i]), "dbl") for i, _ in reps] + [(None, None)]
    A = np.array(A, dtype=np.uint32)
    return A, np.zeros_like(A), want


@functools.lru_cache(None)
def add_cases():
    pts = curve_points()
    reps = _add_reps()
    n = len(reps)
    A, B, want = [], [], []
    step = 1009  # walks the list against itself: every representative meets one of another point, kind and l
    assert n % step
    for t, (i, rep) in enumerate(reps):
        j, other = reps[(t * step + 17) % n]
        s = o.g1_add(pts[i], pts[j])
        cls = "add" if pts[i][0] != pts[j][0] else ("dbl" if s else None)
        A.append(xyzz_row(rep)); B.append(xyzz_row(other)); want.append((s, cls))
    # the same point as two representatives (the doubling branch), a point and its negative (the identity), identity operands
    by_point = {}
    for i, rep in reps:
        by_point.setdefault(i, []).append(rep)
    neg_of = {i: pts.index(o.g1_neg(p)) for i, p in enumerate(pts) if o.g1_neg(p) in pts}
    for i, mine in by_point.items():
        for t in range(0, len(mine), 5):
            a, b = mine[t], mine[(t * 7 + 3) % len(mine)]
            A.append(xyzz_row(a)); B.append(xyzz_row(b)); want.append((o.g1_double(pts[i]), "dbl"))
            if i in neg_of:
                theirs = by_point[neg_of[i]]
                A.append(xyzz_row(a)); B.append(xyzz_row(theirs[(t * 11 + 1) % len(theirs)])); want.append((None, None))
            A.append(xyzz_row(a)); B.append(ZERO36); want.append((pts[i], "pass"))
            A.append(ZERO36); B.append(xyzz_row(a)); want.append((pts[i], "pass"))
    A.append(ZERO36); B.append(ZERO36); want.append((None, None))
    return np.array(A, dtype=np.uint32), np.array(B, dtype=np.uint32), want


@functools.lru_cache(None)
def dbl_affine_cases():
    B, want = [], []
    for p in curve_points():
        for row, t in _table_forms(p):
            B.append(row); want.append((o.g1_double(t), "dbl_affine"))
    B = np.array(B, dtype=np.uint32)
    return np.zeros_like(B), B, want


@functools.lru_cache(None)
def jacobian_cases():
    """(X, Y, Z) = (x l^2, y l^3, l) with Z's word an extreme one, lifted: each coordinate alone at its top (X < 6p, Y < 4p, Z < 8p,
    less the margin), all together, all at the bottom; Z = 0 is the identity"""
    A, want = [], []
    for i, p in enumerate(curve_points()):
        for W in WORDS + SMALL_WORDS + [_ones_under(Z_LIMIT) % Q]:
            lam = unmont(W)
            words = (mont(p[0] * lam * lam % Q), mont(p[1] * pow(lam, 3, Q) % Q), W)
            tops = (lift(words[0], X_LIMIT, 5), lift(words[1], Y_LIMIT, 3), lift(W, Z_LIMIT, 7))
            reps = [words, tops] + [tuple(tops[k] if k == c else words[k] for k in range(3)) for c in range(3)]
            for rep in dict.fromkeys(reps):
                A.append([v for c in rep for v in limbs(c)] + [0] * 9); want.append((p, rep))
    A.append(limbs(5) + limbs(7) + [0] * 18); want.append((None, None))
    A = np.array(A, dtype=np.uint32)
    return A, np.zeros_like(A), want


@functools.lru_cache(None)
def to_affine_cases():
    pts = curve_points()
    reps = _add_reps()[::3]
    A = np.array([xyzz_row(rep) for _, rep in reps] + [ZERO36], dtype=np.uint32)
    return A, np.zeros_like(A), [pts[i] for i, _ in reps] + [None]


OPS = {0: madd_cases, 1: dbl_cases, 2: add_cases, 3: dbl_affine_cases, 4: jacobian_cases, 5: to_affine_cases}
QUAD_OF = {6: 2, 7: 1}  # xyzz29_add_quad / xyzz29_dbl_quad run the cases of xyzz29_add / xyzz29_dbl


def check_xyzz_rows(out, want, op, bounds=BOUNDS):
    assert out.shape == (len(want), 36)
    for k, (w, cls) in enumerate(want):
        _check_xyzz(out[k], w, cls, (op, k), bounds)


def check_jacobian_rows(out, want):
    """op 4: out = ZZ, ZZZ of xyzz29_from_jacobian (ZZ < 1.38, ZZZ < 1.07), then X, Y of xyzz29_to_jacobian (X < 1.06, Y < 1.04)"""
    for k, (p, rep) in enumerate(want):
        if p is None:
            assert not out[k].any(), k
            continue
        assert (out[k].reshape(4, 9)[:, :8] <= M29).all(), k
        zz, zzz, x, y = (limb_val(out[k][9 * i : 9 * i + 9]) for i in range(4))
        X, Y, Z = (unmont(v) for v in rep)
        assert unmont(zz) == Z * Z % Q and unmont(zzz) == Z * Z * Z % Q, k
        assert unmont(x) == X * Z * Z % Q and unmont(y) == Y * pow(Z, 3, Q) % Q, k
        # the pair (X', Y', Z' = ZZ) is the point again
        z2 = unmont(zz)
        assert (unmont(x) * pow(z2, -2, Q) % Q, unmont(y) * pow(z2, -3, Q) % Q) == p, k
        for name, v, b in (("ZZ", zz, 1380), ("ZZZ", zzz, 1070), ("X", x, 1060), ("Y", y, 1040)):
            assert 1000 * v < b * Q, (k, name, v / Q)


def check_affine_rows(out, want):
    """op 5: canonical x, y in the first 18 words, the rest zero; the identity is (0, 0)"""
    for k, p in enumerate(want):
        assert not out[k][18:].any(), k
        x, y = limb_val(out[k][:9]), limb_val(out[k][9:18])
        assert (out[k][:8] <= M29).all() and (out[k][9:17] <= M29).all() and x < Q and y < Q, k
        assert (None if x == 0 and y == 0 else (unmont(x), unmont(y))) == p, k


def check_op(be, op):
    """run one op's cases through a back end and check every element; returns the output words"""
    A, B, want = OPS[QUAD_OF.get(op, op)]()
    out = be.point_raw(op, A, B)
    if op == 4:
        check_jacobian_rows(out, want)
    elif op == 5:
        check_affine_rows(out, want)
    else:
        check_xyzz_rows(out, want, op)
    return out
