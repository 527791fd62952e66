"""The cases of tests/wire_cases.py are what they claim to be (CPU; the oracle alone decides).  tests/test_gpu_wire.py runs them
through the serde kernels, the 32-bit-limb field operations and the ad-hoc registration cache."""
import numpy as np
import pytest

from oracle import bn254 as o
from oracle import formats as fm

import wire_cases as K

Q = o.Q


# ---------------------------------------------------------------- the word list
@pytest.mark.parametrize("field,mod", K.FIELDS)
def test_extreme_words_are_montgomery_words_at_the_limb_extremes(field, mod):
    words = dict(K.extreme_words(mod))
    assert len(set(words.values())) == len(words) == 20 and all(0 < w < mod for w in words.values())
    l = K.limbs32(mod)
    assert words["p-1"] == mod - 1 and words["p-2"] == mod - 2 and words["1"] == 1 and words["R mod p"] == pow(2, 256, mod)
    for j in range(1, 8):
        assert K.limbs32(words[f"2^{32 * j}-1"]) == [K.M32] * j + [0] * (8 - j)
    assert K.limbs32(words["2^253-1"]) == [K.M32] * 7 + [(1 << 29) - 1]
    assert K.limbs32(words["p>>32<<32 - 1"]) == [K.M32, l[1] - 1] + l[2:]  # limb 1 of either modulus is not 0: the borrow stops there
    assert K.limbs32(words["top-1|sat"]) == [K.M32] * 7 + [l[7] - 1]
    for j in range(1, 7):  # limb 0 alone is 2^32 - 1; limb 7 alone is not below the modulus
        assert K.limbs32(words[f"limb{j}=sat"]) == [0] * j + [K.M32] + [0] * (7 - j)
    assert K.M32 << 224 >= mod and "limb7=sat" not in words and "limb0=sat" not in words
    for w in words.values():
        assert K.word_of(K.value_of(w, mod), mod) == w and o.unpack(K.pack_words([w]), mod) == [K.value_of(w, mod)]


# ---------------------------------------------------------------- G1 points
def test_points_are_on_the_curve_and_round_trip():
    assert len(K.POINTS) == K.N_POINTS == 3 * 256 + 37
    assert [i for i, p in enumerate(K.POINTS) if p is None] == sorted(K.IDENTITY_AT) == [0, 63, 64, 255, 256, 804]
    for p in K.POINTS:
        assert p is None or (0 <= p[0] < Q and 0 < p[1] < Q and (p[1] * p[1] - p[0] ** 3 - 3) % Q == 0)
        assert fm.g1_from_bytes(fm.g1_to_bytes(p)) == p
    assert K.FIRST_POINTS == [[None], [K.POINTS[1]]] and K.POINTS[1] is not None


def test_smallest_and_largest_abscissae():
    assert K.X_SMALL[:6] == [1, 2, 3, 5, 6, 7] and K.X_LARGE[:6] == [Q - 1 - i for i in range(6)]
    assert len(K.X_SMALL) == len(K.X_LARGE) == 8
    # the scans took the first eight valid abscissae of their range, and `skipped` is every non-residue they passed (the scan down from
    # q - 1 passed none among its eight and went on to the first one)
    def euler(x):
        return pow(x ** 3 + 3, (Q - 1) // 2, Q)

    up = range(1, max(K.X_SMALL + K.X_SMALL_SKIPPED) + 1)
    down = range(Q - 1, min(K.X_LARGE + K.X_LARGE_SKIPPED) - 1, -1)
    for scan, took, skipped in ((up, K.X_SMALL, K.X_SMALL_SKIPPED), (down, K.X_LARGE, K.X_LARGE_SKIPPED)):
        assert took == [x for x in scan if euler(x) == 1][:8] and skipped == [x for x in scan if euler(x) == Q - 1] and skipped
    assert K.X_SMALL_SKIPPED == [4] and K.X_LARGE_SKIPPED == [Q - 11]


def test_constructed_points_sit_within_the_scan_distance_of_their_target_word():
    targets = dict(K.extreme_words(Q))
    for coord, name, target, dist, p in K.CONSTRUCTED:
        assert targets[name] == target and 0 <= dist <= K.SCAN_CAP == 64
        assert K.word_of(p[0] if coord == "x" else p[1], Q) == target - dist
        assert o.is_on_curve(p)
    # every word of the list gave a point for x and for y, but the word 1 (nothing below it to scan to): no word fell to the cap
    made = {(c, n) for c, n, *_ in K.CONSTRUCTED}
    assert made | set(K.DROPPED) == {(c, n) for c in "xy" for n in targets} and not made & set(K.DROPPED)
    assert K.DROPPED == [("x", "1"), ("y", "1")]
    assert K.MAX_SCAN == max(c[3] for c in K.CONSTRUCTED) == 11


def test_every_constructed_point_has_both_signs():
    special = [(x, None) for x in K.X_SMALL + K.X_LARGE] + [c[4] for c in K.CONSTRUCTED]
    assert len(special) == K.N_SPECIAL == 16 + len(K.CONSTRUCTED)
    have = set(p for p in K.POINTS if p is not None)
    for x, y in special:
        ys = sorted(p[1] for p in have if p[0] == x)
        assert len(ys) == 2 and ys[0] + ys[1] == Q and ys[0] % 2 != ys[1] % 2 and (y is None or y in ys)
        flags = {fm.g1_to_bytes((x, yy))[31] & 0xC0 for yy in ys}
        assert flags == {0, fm.FLAG_SIGN}


# ---------------------------------------------------------------- invalid encodings
def test_bad_g1_is_refused_by_the_oracle_and_the_identity_is_not():
    assert len({b for b, _ in K.BAD_G1}) == len(K.BAD_G1)
    for b, why in K.BAD_G1:
        assert len(b) == 32
        with pytest.raises(ValueError):
            fm.g1_from_bytes(b)
    assert fm.g1_from_bytes(K.IDENTITY_BYTES) is None and K.IDENTITY_BYTES == bytes(31) + b"\x80"
    assert K.IDENTITY_BYTES not in [b for b, _ in K.BAD_G1] and fm.g1_to_bytes(None) == K.IDENTITY_BYTES
    # the construction: out-of-range abscissae, the skipped non-residues, x = 0, and the three misuses of the infinity flag
    ints = {(int.from_bytes(b, "little") & ((1 << 254) - 1), b[31] & 0xC0) for b, _ in K.BAD_G1}
    want = {(Q, 0), (Q + 1, 0), ((1 << 254) - 1, 0), (0, 0), (0, 0x40), (1, 0x80), (0, 0xC0), (Q, 0x80)}
    want |= {(x, 0) for x in K.X_SMALL_SKIPPED + K.X_LARGE_SKIPPED} | {(K.X_SMALL_SKIPPED[0], 0x40), (K.X_LARGE_SKIPPED[0], 0x40)}
    assert ints == want


def test_mixed_has_the_stated_invalid_index_set_and_nothing_else():
    assert len(K.MIXED) == K.N_POINTS
    bad = set()
    for i, b in enumerate(K.MIXED):
        try:
            assert fm.g1_from_bytes(b) == K.POINTS[i]
        except ValueError:
            bad.add(i)
    assert bad == K.MIXED_BAD
    waves = {}
    for i in bad:
        waves.setdefault(i // 64, []).append(i)
    assert sorted(waves[2]) == list(K.BAD_WAVE) == list(range(128, 192))  # one whole wavefront
    assert [waves[i // 64] for i in K.BAD_LONE] == [[i] for i in K.BAD_LONE]  # alone in their wavefronts ...
    assert [i // 256 for i in K.BAD_LONE] == [1, 2, 3] and K.BAD_LONE[-1] == K.N_POINTS - 1  # ... one per other workgroup
    assert set(waves) == set(range(13))  # no wavefront is all valid
    # every invalid encoding is used in the full wavefront and once more outside it
    assert {K.MIXED[i] for i in K.BAD_WAVE} == {b for b, _ in K.BAD_G1}
    assert {K.MIXED[i] for i in bad - set(K.BAD_WAVE) - set(K.BAD_LONE)} == {b for b, _ in K.BAD_G1}


# ---------------------------------------------------------------- field encodings
@pytest.mark.parametrize("field,mod", K.FIELDS)
def test_repr_cases(field, mod):
    vals = K.REPR_VALUES[field]
    assert len(vals) == K.N_REPR == 2 * 256 + 19 and all(0 <= v < mod for v in vals)
    assert vals[:6] == [0, 1, mod - 1, mod - 2, (mod - 1) // 2, (mod + 1) // 2]
    assert {K.word_of(v, mod) for v in vals} >= {w for _, w in K.extreme_words(mod)}
    l = K.limbs32(mod)
    bad = [K.limbs32(int.from_bytes(b, "little")) for b in K.REPR_BAD[field]]
    assert all(len(b) == 32 and int.from_bytes(b, "little") >= mod for b in K.REPR_BAD[field])
    assert bad[0] == l                                                     # the modulus
    assert bad[1] == [l[0] + 1] + l[1:]                                    # the seven high limbs are the modulus's
    assert bad[2] == [K.M32] + l[1:] and l[0] < K.M32                      # the same, the lowest limb saturated
    assert bad[3] == [0] * 7 + [l[7] + 1]                                  # above the modulus by the top limb alone
    assert bad[4] == [0] * 7 + [1 << 31] and bad[5] == [K.M32] * 8         # the top bit alone; every bit
    near = [K.limbs32(int.from_bytes(b, "little")) for b in K.REPR_NEAR[field]]
    assert all(len(b) == 32 and int.from_bytes(b, "little") < mod for b in K.REPR_NEAR[field])
    assert near[0] == [l[0] - 1] + l[1:] and near[1] == [K.M32] * 7 + [l[7] - 1]
    # below the modulus by limb j alone, everything under it saturated: j = 1 .. 6 (j = 7 is near[1])
    assert near[2:] == [[K.M32] * j + [l[j] - 1] + l[j + 1:] for j in range(1, 7)] and len(near) == 8


@pytest.mark.parametrize("field,mod", K.FIELDS)
def test_repr_edge_vector(field, mod):
    vec, bad_at = K.REPR_EDGE[field]
    assert len(vec) == K.N_REPR and {i for i, v in enumerate(vec) if v >= mod} == set(bad_at)
    assert {v for v in vec if v >= mod} == {int.from_bytes(b, "little") for b in K.REPR_BAD[field]}
    assert {v for v in vec if v < mod} == {int.from_bytes(b, "little") for b in K.REPR_NEAR[field]}
    assert {0, 255, 256, 511, 512, K.N_REPR - 1} <= bad_at                   # both ends of every workgroup
    assert all(any(i // 64 == w for i in bad_at) for w in range(9))          # every wavefront
    assert sum(i // 64 == 1 for i in bad_at) >= 3 and {70, 71, 72} <= bad_at  # several in one wavefront, in neighbouring lanes


@pytest.mark.parametrize("field,mod", K.FIELDS)
def test_fp_words_and_pairs(field, mod):
    words = K.FP_WORDS[field]
    one = pow(2, 256, mod)
    assert len(set(words)) == len(words) == 29 and all(0 <= w < mod for w in words)
    assert set(words) >= {w for _, w in K.extreme_words(mod)} | {0, mod >> 1, one, one * one % mod, mod - one}
    pairs = K.FP_PAIRS[field]
    assert len(pairs) == len(set(pairs)) == 29 * 29 > 3 * 256 and set(pairs) == {(a, b) for a in words for b in words}
    # the carries the list is there for: a sum that carries through all eight limbs, a difference that borrows through all of them
    assert (mod - 1, 1) in pairs and (0, 1) in pairs and (mod - 1, mod - 1) in pairs


# ---------------------------------------------------------------- base sets
def test_base_sets_differ_as_stated():
    sets = K.base_sets()
    assert list(sets) == ["base", "swapped", "neg_last", "cross_neg", "reversed"]
    raw = {k: v.tobytes() for k, v in sets.items()}
    assert len(set(raw.values())) == 5 and {len(b) for b in raw.values()} == {K.N_BASES * 64} and K.N_BASES == 300
    pts = {k: o.unpack_points(v) for k, v in sets.items()}
    base = pts["base"]
    assert all(p is not None and o.is_on_curve(p) for p in base) and len(set(base)) == 300
    sw = list(base)
    sw[17], sw[211] = base[211], base[17]
    assert pts["swapped"] == sw and sorted(pts["swapped"]) == sorted(base)              # the same multiset in another order
    assert pts["neg_last"] == base[:-1] + [o.g1_neg(base[-1])]
    diff = np.flatnonzero(np.frombuffer(raw["neg_last"], dtype=np.uint8) != np.frombuffer(raw["base"], dtype=np.uint8))
    assert len(diff) and diff.min() >= 300 * 64 - 32                                     # only the last y words change
    assert pts["cross_neg"] == [o.g1_neg(base[1]), o.g1_neg(base[0])] + base[2:]
    assert sorted(pts["cross_neg"]) != sorted(base)                                      # another multiset of the same size
    assert pts["reversed"] == base[::-1] and sets["reversed"].flags["C_CONTIGUOUS"]
