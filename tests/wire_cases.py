"""Cases for the wire formats (csrc/h2mi_serde.hip) and the 32-bit-limb Montgomery layer under them (csrc/fp.cuh), shared by
tests/test_wire_cases_host.py (the cases are what they claim to be; CPU) and tests/test_gpu_wire.py (the kernels against the oracle).

The serde kernels take canonical bytes, convert to Montgomery *words* (value * 2^256 mod p as eight 32-bit limbs) and compute on those
with fe_mul / fe_add / fe_sub / ...; the borrow chain fe_lt_mod decides whether an encoding is canonical.  A uniformly random value
never gives a word with a saturated limb, a word equal to p - 1 or a carry through all eight limbs, and never an encoding that agrees
with the modulus in its high limbs.  This module holds the operands that do:
  * extreme_words(p) — the Montgomery words at the limb extremes, per modulus;
  * POINTS — n = 3 * 256 + 37 affine G1 points (four workgroups, the last ragged): the smallest and largest abscissae, points whose x
    or y *word* is (within a short scan of) an extreme word, each with both signs of y, random multiples of G, and the identity at the
    ends of wavefronts and workgroups; BAD_G1 — encodings G1Affine::from_bytes refuses; MIXED — both interleaved;
  * REPR_VALUES / REPR_BAD / REPR_NEAR / REPR_EDGE — canonical integers, strings not below the modulus, their valid neighbours, and a
    vector of the last two interleaved, for both moduli;
  * FP_WORDS / FP_PAIRS — word operands for h2mi_dbg_field_op;
  * base_sets() — four sets of 300 bases that differ in order, in the last 32 bytes, or as multisets (the ad-hoc registration cache), and
    a fifth that makes the cache of four evict.
Only oracle.bn254 and oracle.formats are used (base_sets() also takes its points from oracle.cref, as the test of the cache it extends
does); seeds are fixed; nothing here needs a GPU."""
import functools
import random

import numpy as np

from oracle import bn254 as o
from oracle import formats as fm

Q, R = o.Q, o.R
FIELDS = [(0, Q), (1, R)]
MODS = {0: Q, 1: R}
M32 = 0xFFFFFFFF
SCAN_CAP = 64                # a constructed coordinate's word is at most this far below its target word
N_POINTS = 3 * 256 + 37      # four workgroups of 256, the last one ragged
N_REPR = 2 * 256 + 19        # three workgroups, the last one ragged
IDENTITY_AT = (0, 63, 64, 255, 256, N_POINTS - 1)


# ---------------------------------------------------------------- words
def limbs32(v: int):
    return [(v >> (32 * j)) & M32 for j in range(8)]


def from_limbs32(limbs) -> int:
    return sum(int(x) << (32 * j) for j, x in enumerate(limbs))


def word_of(v: int, p: int) -> int:
    """the Montgomery word of a value (what o.pack([v], p) stores)"""
    return (v << 256) % p


def value_of(w: int, p: int) -> int:
    """the value a Montgomery word stands for"""
    return w * pow(1 << 256, -1, p) % p


def extreme_words(p: int):
    """[(name, word)], every word in 1 .. p - 1, no word twice.  The word with only limb 7 saturated is not below either modulus (their top
    limb is 0x30644e72), so it is no Montgomery word and is left out; 'top-1|sat' is the largest word with a saturated limb there is."""
    top = p >> 224
    named = [("p-1", p - 1), ("p-2", p - 2), ("2^253-1", (1 << 253) - 1), ("2^224-1", (1 << 224) - 1), ("2^32-1", (1 << 32) - 1)]
    named += [(f"2^{32 * j}-1", (1 << (32 * j)) - 1) for j in range(1, 8)]
    named += [("p>>32<<32 - 1", (p >> 32 << 32) - 1), ("top-1|sat", ((top - 1) << 224) | ((1 << 224) - 1))]
    named += [(f"limb{j}=sat", M32 << (32 * j)) for j in range(8)]
    named += [("1", 1), ("R mod p", (1 << 256) % p)]
    out, seen = [], set()
    for name, w in named:
        if 0 < w < p and w not in seen:
            seen.add(w)
            out.append((name, w))
    return out


# ---------------------------------------------------------------- G1 points
def _is_square(v: int) -> bool:
    return v % Q != 0 and pow(v, (Q - 1) // 2, Q) == 1


def _valid_x(x: int) -> bool:
    return _is_square(x * x * x + 3)


def _point_at_x(x: int):
    rhs = (x * x * x + 3) % Q
    y = pow(rhs, (Q + 1) // 4, Q)
    assert y * y % Q == rhs
    return (x, y)


def _cube_root(c: int):
    """a cube root of c mod q, or None when c is no cube.  q - 1 = 3^s t: c^(1/3 mod t) is a root up to an element of the 3-Sylow
    subgroup, which is small enough to try in full.  The caller checks the result."""
    if c % Q == 0 or pow(c, (Q - 1) // 3, Q) != 1:
        return None
    t, s = Q - 1, 0
    while t % 3 == 0:
        t, s = t // 3, s + 1
    g = 2
    while pow(g, (Q - 1) // 3, Q) == 1:
        g += 1
    z = pow(g, t, Q)  # order 3^s
    r = pow(c, pow(3, -1, t), Q)
    for _ in range(3 ** s):
        if pow(r, 3, Q) == c % Q:
            return r
        r = r * z % Q
    raise AssertionError("no cube root of a cube")


def _scan_small_large():
    small, small_skipped, x = [], [], 1
    while len(small) < 8:
        (small if _valid_x(x) else small_skipped).append(x)
        x += 1
    large, large_skipped, x = [], [], Q - 1
    while len(large) < 8:
        (large if _valid_x(x) else large_skipped).append(x)
        x -= 1
    # a scan that skipped nothing goes on to the first non-residue past its last abscissa: BAD_G1 wants one next to each group
    for skipped, x, step in ((small_skipped, small[-1], 1), (large_skipped, large[-1], -1)):
        while not skipped:
            x += step
            if not _valid_x(x):
                skipped.append(x)
    return small, small_skipped, large, large_skipped


X_SMALL, X_SMALL_SKIPPED, X_LARGE, X_LARGE_SKIPPED = _scan_small_large()


def _mont_extreme_points():
    """-> (constructed, dropped).  constructed: (coordinate 'x' | 'y', name, target word, scan distance, point): the point's x (or y) has
    the Montgomery word target - distance.  dropped: (coordinate, name) of a target with no curve point within SCAN_CAP words below it."""
    def scan(coord, target):
        for d in range(min(SCAN_CAP, target - 1) + 1):  # words stay above 0
            v = value_of(target - d, Q)
            if coord == "x" and _valid_x(v):
                return d, _point_at_x(v)
            if coord == "y":
                x = _cube_root((v * v - 3) % Q)
                if x is not None:
                    return d, (x, v)
        return None

    made, dropped = [], []
    for name, target in extreme_words(Q):
        for coord in "xy":
            hit = scan(coord, target)
            if hit is None:
                dropped.append((coord, name))
            else:
                made.append((coord, name, target, hit[0], hit[1]))
    return made, dropped


# DROPPED is [('x', '1'), ('y', '1')]: the word 1 has no word below it to scan to, and 2^-256 mod q is neither the abscissa nor the
# ordinate of a curve point.  No word is dropped under the 64-step cap (MAX_SCAN is 11, the y scan for 'limb2=sat'); the word 1 stays
# in REPR_VALUES and FP_WORDS.  tests/test_wire_cases_host.py pins both statements.
CONSTRUCTED, DROPPED = _mont_extreme_points()
MAX_SCAN = max(c[3] for c in CONSTRUCTED)


def _random_multiples(count: int, seed: int):
    """k G for 248-bit random k (Jacobian ladder, one inversion per point: a quarter of the affine ladder's time)"""
    rng, g = random.Random(seed), o.jac_from_affine(o.G1_GEN)
    return [o.jac_to_affine(o.jac_mul(rng.getrandbits(248) | 1, g)) for _ in range(count)]


def _assemble_points():
    special = [_point_at_x(x) for x in X_SMALL + X_LARGE] + [c[4] for c in CONSTRUCTED]
    body = []
    for p in special:
        body += [p, o.g1_neg(p)]  # both values of the sign flag at every constructed x
    body += _random_multiples(61, 0x61)
    body += _random_multiples(N_POINTS - len(IDENTITY_AT) - len(body), 0x9AD)
    it = iter(body)
    return [None if i in IDENTITY_AT else next(it) for i in range(N_POINTS)], len(special)


POINTS, N_SPECIAL = _assemble_points()
FIRST_POINTS = [POINTS[:1], POINTS[1:2]]  # n = 1: the identity alone, and the first curve point alone


# ---------------------------------------------------------------- invalid G1 encodings
def _enc(x: int, flags: int = 0) -> bytes:
    assert x < 1 << 254
    b = bytearray(x.to_bytes(32, "little"))
    b[31] |= flags
    return bytes(b)


def _bad_g1():
    bad = [(_enc(Q), "x = q"), (_enc(Q + 1), "x = q + 1"), (_enc((1 << 254) - 1), "x = 2^254 - 1")]
    for where, skipped in (("small", X_SMALL_SKIPPED), ("large", X_LARGE_SKIPPED)):
        bad += [(_enc(x), f"non-residue abscissa among the {where} ones") for x in skipped]
        bad.append((_enc(skipped[0], fm.FLAG_SIGN), f"non-residue abscissa among the {where} ones, sign flag"))
    bad += [(_enc(0), "x = 0, no flag: 3 is a non-residue"), (_enc(0, fm.FLAG_SIGN), "x = 0, sign flag only"),
            (_enc(1, fm.FLAG_INF), "infinity flag with x = 1"), (_enc(0, fm.FLAG_INF | fm.FLAG_SIGN), "infinity and sign flags"),
            (_enc(Q, fm.FLAG_INF), "infinity flag with x = q")]
    return bad


BAD_G1 = _bad_g1()
IDENTITY_BYTES = bytes(31) + b"\x80"  # the valid identity: in POINTS, not in BAD_G1

BAD_WAVE = range(128, 192)             # one whole wavefront of workgroup 0
BAD_LONE = (333, 712, N_POINTS - 1)    # the only invalid entry of its wavefront, one per other workgroup; the ragged tail's last index
_SPREAD_WAVES = (0, 1, 3, 4, 6, 7, 8, 9, 10)  # every wavefront that is neither BAD_WAVE's nor a lone entry's


def _mixed():
    enc = [fm.g1_to_bytes(p) for p in POINTS]
    at = {}
    for j, i in enumerate(BAD_WAVE):
        at[i] = BAD_G1[j % len(BAD_G1)][0]
    for j, i in enumerate(BAD_LONE):
        at[i] = BAD_G1[(5 * j + 3) % len(BAD_G1)][0]
    for j, (b, _) in enumerate(BAD_G1):  # every invalid encoding once more, over the rest
        i = 64 * _SPREAD_WAVES[j % len(_SPREAD_WAVES)] + (7 + 11 * j) % 64
        assert i not in at
        at[i] = b
    for i, b in at.items():
        enc[i] = b
    return enc, frozenset(at)


MIXED, MIXED_BAD = _mixed()


# ---------------------------------------------------------------- field encodings
def _repr_values(p: int, seed: int):
    rng = random.Random(seed)
    vals = [0, 1, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2] + [value_of(w, p) for _, w in extreme_words(p)]
    vals += [rng.randrange(p) for _ in range(200)]
    vals += [rng.randrange(p) for _ in range(N_REPR - len(vals))]
    return vals


def _repr_bad(p: int):
    l = limbs32(p)
    return [p, p + 1, from_limbs32([M32] + l[1:]), (l[7] + 1) << 224, 1 << 255, (1 << 256) - 1]


def _repr_near(p: int):
    l = limbs32(p)
    near = [p - 1, ((l[7] - 1) << 224) | ((1 << 224) - 1)]
    near += [from_limbs32([M32] * j + [l[j] - 1] + l[j + 1:]) for j in range(1, 8)]
    return list(dict.fromkeys(near))  # j = 7 restates the second entry


def _repr_edge(p: int):
    """N_REPR encodings: the near values in rotation with a bad one at both ends of every workgroup, at every 13th index, and at three
    neighbouring lanes of one wavefront -> (integers, bad index set)"""
    near, bad = _repr_near(p), _repr_bad(p)
    at = {0, 255, 256, 511, 512, N_REPR - 1, 70, 71, 72} | set(range(5, N_REPR, 13))
    vec, k = [], 0
    for i in range(N_REPR):
        if i in at:
            vec.append(bad[k % len(bad)])
            k += 1
        else:
            vec.append(near[i % len(near)])
    return vec, frozenset(at)


REPR_VALUES = {f: _repr_values(p, 0x5E0 + f) for f, p in FIELDS}
REPR_BAD = {f: [v.to_bytes(32, "little") for v in _repr_bad(p)] for f, p in FIELDS}
REPR_NEAR = {f: [v.to_bytes(32, "little") for v in _repr_near(p)] for f, p in FIELDS}
REPR_EDGE = {f: _repr_edge(p) for f, p in FIELDS}


# ---------------------------------------------------------------- word operands of the field operations
def _fp_words(p: int):
    """the extreme words, the constants the layer itself multiplies by, and five more patterns (a lone top bit, alternating bits, a low
    limb that borrows) so that every ordered pair makes four workgroups"""
    one = (1 << 256) % p
    words = [w for _, w in extreme_words(p)] + [0, p >> 1, one, one * one % p, p - one]
    words += [2, (p + 1) >> 1, 1 << 253, int("55" * 32, 16) >> 3, p - (1 << 32)]
    assert all(0 <= w < p for w in words)
    return list(dict.fromkeys(words))


FP_WORDS = {f: _fp_words(p) for f, p in FIELDS}
FP_PAIRS = {f: [(a, b) for a in FP_WORDS[f] for b in FP_WORDS[f]] for f, _ in FIELDS}


def pack_words(words) -> np.ndarray:
    """raw words -> (n, 4) u64, as they lie in memory"""
    return o.pack(list(words))


# ---------------------------------------------------------------- base sets for the ad-hoc registration cache
N_BASES = 300


def _neg_row(row: np.ndarray) -> np.ndarray:
    """-P of a packed affine point: q - y on the Montgomery word of y (negation commutes with the Montgomery factor)"""
    out = row.copy()
    y = o.limbs_to_int(row[4:])
    assert 0 < y < Q
    out[4:] = o.int_to_limbs(Q - y)
    return out


@functools.lru_cache(maxsize=None)
def base_sets():
    """-> {name: (300, 8) u64}: 'base'; 'swapped' (entries 17 and 211 exchanged: the same multiset in another order); 'neg_last' (the last
    point negated: only the y words of the last 64 bytes change); 'cross_neg' (points 0 and 1 each replaced by the other's negative: another
    multiset of the same size); and a fifth, 'reversed' (the whole set in the opposite order), one more than the cache holds: with it the
    test reaches the eviction"""
    from oracle import cref

    base = cref.g1_mul_gen(o.random_field_limbs(N_BASES, 0x3A5E), 2)
    swapped = base.copy()
    swapped[[17, 211]] = base[[211, 17]]
    neg_last = base.copy()
    neg_last[-1] = _neg_row(base[-1])
    cross = base.copy()
    cross[0], cross[1] = _neg_row(base[1]), _neg_row(base[0])
    return {"base": base, "swapped": swapped, "neg_last": neg_last, "cross_neg": cross, "reversed": np.ascontiguousarray(base[::-1])}
