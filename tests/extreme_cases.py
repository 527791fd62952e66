"""Operands at the limb extremes, shared by tests/test_extreme_cases_host.py, tests/test_gpu_extremes.py and tests/test_gpu_ntt_plans.py.

Every field kernel runs on the lazy 29-bit-limb layer (csrc/f29.cuh), whose correctness rests on bounds written as comments ("lazy:
limbs < 1.5 * 2^30", "the subtrahend must be < 4p - 2^232", expr_encode's static bound per stack value).  A violated bound gives a wrong
field element only for operands near it, and uniformly random operands never get there.  This module holds the operands that do:
  * EXTREME_WORDS — raw Montgomery-2^256 memory words, for the kernels that take words as they lie (f29_unpack of the word is the
    multiplier's operand): r - 1, the largest word below r whose limbs 0..7 are all 2^29 - 1, 2^232 - 1, 0, 1, r >> 1;
  * EXTREME_VALUES — field values, for the kernels that convert on load (gen::ld, cst: a multiplication by 2^517 mod r that leaves the
    value times 2^261, between 0 and ~1.0007 r): 0, 1, r - 1, r - 2, (r - 1) / 2, TOP261, the value whose CONVERTED form is r - 1, and
    OVER261, the value whose converted form is the largest there is above r — a lazy sum of converted loads is largest when every
    value is OVER261, a negation is largest (4p exactly) when the value is 0;
  * the vector patterns over either alphabet, the challenge / point / root / scalar set drawn from both, and the gate programs that
    sit just below and just above expr_encode's thresholds, with a restatement of its rule that says on which side.
A vector is a `Vec`: the memory words the kernel gets and the field values the Python-integer references get.  Nothing here needs a GPU."""
import random
import zlib

import numpy as np

from oracle import bn254 as o

R = o.R
M232 = (1 << 232) - 1
# raw Mont256 words (not values): all below r
EXTREME_WORDS = [o.R - 1, (((o.R >> 232) - 1) << 232) | M232, M232, 0, 1, o.R >> 1]

_RINV256 = pow(1 << 256, -1, R)


def word_value(w: int) -> int:
    """the field value a memory word stands for (what o.unpack(raw, o.R) gives)"""
    return w * _RINV256 % R


def value_word(v: int) -> int:
    """the memory word of a field value (what o.pack([v], o.R) gives)"""
    return (v << 256) % R


def converted(word: int) -> int:
    """what gen::ld / cst make of a memory word, exactly: f29_mul(word, 2^266 mod r) = (word T + m r) / 2^261 with the one m below 2^261
    that makes the division exact.  Congruent to value 2^261 and below ~1.0007 r — so not always below r"""
    t = pow(2, 266, R)
    m = -(word * t) * pow(R, -1, 1 << 261) % (1 << 261)
    return (word * t + m * R) >> 261


def _largest_converted_load() -> int:
    """the value whose converted load is the largest there is above r.  converted(w) = x + r needs x = 32 w mod r below w T / 2^261, and
    that is largest for w = (x + 31 r) / 32 just below r: walk x down from the bound in steps of 32 until the product agrees"""
    x = ((31 * R // 32) * pow(2, 266, R)) >> 261
    x -= (x + 31 * R) % 32
    while converted((x + 31 * R) // 32) != x + R:
        x -= 32
    return word_value((x + 31 * R) // 32)


TOP261 = -pow(1 << 261, -1, R) % R  # TOP261 * 2^261 = r - 1 (mod r): the converted load with every limb at its canonical maximum
OVER261 = _largest_converted_load()  # its converted load is ~1.00065 r: four of them pass 4p, which f29_sub's 4p - x cannot take
EXTREME_VALUES = [0, 1, R - 1, R - 2, (R - 1) // 2, TOP261, OVER261]
ALPHABETS = {"words": list(EXTREME_WORDS), "values": [value_word(v) for v in EXTREME_VALUES]}  # both as memory words
# "all top", "all over": the value alphabet's largest canonical and largest converted loads (the word alphabet's is r - 1 itself)
PATTERNS = {"words": ("all r - 1", "all zero", "r - 1 / 0 alternating", "random choice"),
            "values": ("all r - 1", "all zero", "r - 1 / 0 alternating", "random choice", "all top", "all over")}
# challenges (beta, gamma, y, theta), evaluation points, division roots, lincomb scalars, instance values — as field values: the extreme
# values, and the values whose memory word is a raw extreme word
SCALARS = list(dict.fromkeys(EXTREME_VALUES + [word_value(w) for w in EXTREME_WORDS]))


def _seed(*key) -> int:
    return zlib.crc32(repr(key).encode())


class Vec:
    """memory words (integers below r) with their field values"""

    def __init__(self, words):
        self.words = list(words)
        self.values = [word_value(w) for w in self.words]

    def __len__(self):
        return len(self.words)

    def limbs(self) -> np.ndarray:
        return o.pack(self.words)  # raw: no Montgomery encoding


def vector(alphabet: str, pattern: str, n: int, *key) -> Vec:
    """`pattern` over ALPHABETS[alphabet], n elements; *key seeds "random choice" (other patterns ignore it)"""
    words = ALPHABETS[alphabet]
    top = R - 1 if alphabet == "words" else value_word(R - 1)
    if pattern == "all r - 1":
        return Vec([top] * n)
    if pattern == "all zero":
        return Vec([0] * n)
    if pattern == "r - 1 / 0 alternating":
        return Vec([top if i % 2 == 0 else 0 for i in range(n)])
    if pattern in ("all top", "all over"):
        assert alphabet == "values"
        return Vec([value_word(TOP261 if pattern == "all top" else OVER261)] * n)
    assert pattern == "random choice"
    rng = random.Random(_seed(alphabet, n, *key))
    return Vec([rng.choice(words) for _ in range(n)])


def pattern_vectors(alphabet: str, n: int, *key):
    """-> [(name, Vec)] for a slot that takes one vector per call: the constant patterns, and "random choice" once per word of the
    alphabet, vector s beginning with the alphabet rotated by s — so every word occurs in the slot however short the vectors are"""
    words = ALPHABETS[alphabet]
    out = [(p, vector(alphabet, p, n)) for p in PATTERNS[alphabet] if p != "random choice"]
    for s in range(len(words)):
        head = [words[(e + s) % len(words)] for e in range(min(n, len(words)))]
        out.append((f"random choice {s}", Vec(head + vector(alphabet, "random choice", n, *key, s).words[len(head):])))
    return out


def values_vec(values) -> Vec:
    return Vec([value_word(v % R) for v in values])


def canonical(limbs) -> bool:
    """every element of an (n, 4) limb array, read as an integer, is below r"""
    return all(w < R for w in o.unpack(limbs))


def scalar(i: int) -> int:
    return SCALARS[i % len(SCALARS)]


N_ROUNDS = len(SCALARS)  # a slot that takes scalar(i + offset) in round i has held every scalar after N_ROUNDS rounds


def rounds(alphabet: str, n_rounds: int = N_ROUNDS):
    """-> [(round, pattern)]: the patterns in turn, so every pattern occurs at least twice in N_ROUNDS rounds"""
    pats = PATTERNS[alphabet]
    assert n_rounds >= len(pats)
    return [(i, pats[i % len(pats)]) for i in range(n_rounds)]


# ---- vector kernels on raw words (csrc/h2mi_poly.hip, k_scale_powers) -------------------------------------------------------------------
EVAL_LENGTHS = [1, 2, 3, 1023, 1025, 2051, 5000]  # k_eval_poly: T = 256 threads up to 2^12 coefficients, 512 at 5000; both sides of a tile
EVAL_POLYS = 24
KATE_MULTI = [(n, m) for n in (2051, 3073) for m in (2, 3, 4)]
LINCOMB_K = [1, 2, 3, 24]
LINCOMB_N = 600
INSTANCE_COUNTS = [4, 5, 16]
INSTANCE_K, INSTANCE_EXT_K = 7, 9  # 512 points, rot = 4
VECTOR_N = 600  # k_fr_mul, k_scale_powers: three workgroups, the last one ragged


def eval_case(n: int):
    """-> (the distinct coefficient vectors, [(point, the 24 polynomials of the call as indices into them)]): slot j of call p holds
    vector (j + p) mod 9, so every slot holds every vector once the points are through"""
    vecs = [v for _, v in pattern_vectors("words", n, "eval")]
    return vecs, [(x, [(j + p) % len(vecs) for j in range(EVAL_POLYS)]) for p, x in enumerate(SCALARS)]


def kate_case(n: int):
    """-> ([(pattern, numerator Vec)], roots): every pattern, every scalar as the root"""
    return pattern_vectors("words", n, "kate"), list(SCALARS)


def kate_multi_case(n: int, m: int):
    """-> ([(pattern, numerator Vec)], [root tuples]): windows of m consecutive non-zero scalars, so every one is root 0 .. m - 1 once"""
    nz = [s for s in SCALARS if s]
    sets = [tuple(nz[(i + j) % len(nz)] for j in range(m)) for i in range(len(nz))]
    return [(p, vector("words", p, n, "kate multi")) for p in PATTERNS["words"]], sets


def partial_fraction_weights(roots):
    """c_i = 1 / prod_{j != i} (r_i - r_j)"""
    out = []
    for i, ri in enumerate(roots):
        d = 1
        for j, rj in enumerate(roots):
            if j != i:
                d = d * (ri - rj) % R
        out.append(pow(d, -1, R))  # raises on equal roots
    return out


def lincomb_case(K: int):
    """-> [(name, K Vec, K scalars)]: every polynomial and every scalar at the top word first (the scalar whose memory word is r - 1,
    then the scalar whose converted form is r - 1), then N_ROUNDS rounds of the patterns with the scalars rotating through SCALARS"""
    n = LINCOMB_N
    top = [vector("words", "all r - 1", n)] * K
    out = [("all r - 1 words, every scalar the word r - 1", top, [word_value(R - 1)] * K),
           ("all r - 1 words, every scalar TOP261", top, [TOP261] * K)]
    for i, pattern in rounds("words"):
        out.append((f"round {i}: {pattern}", [vector("words", pattern, n, "lincomb", K, i, j) for j in range(K)], [scalar(i + j) for j in range(K)]))
    return out


def instance_case(count: int):
    """-> [(name, l0 Vec of 2^INSTANCE_EXT_K words, count values)]"""
    size = 1 << INSTANCE_EXT_K
    top = vector("words", "all r - 1", size)
    out = [("all r - 1 words, every value the word r - 1", top, [word_value(R - 1)] * count), ("all r - 1 words, every value TOP261", top, [TOP261] * count)]
    for i, pattern in rounds("words"):
        out.append((f"round {i}: {pattern}", vector("words", pattern, size, "instance", count, i), [scalar(i + j) for j in range(count)]))
    return out


def mul_case():
    """-> [(pattern a, pattern b, Vec a, Vec b)]: every pair of patterns"""
    pats = PATTERNS["words"]
    return [(pa, pb, vector("words", pa, VECTOR_N, "mul a"), vector("words", pb, VECTOR_N, "mul b")) for pa in pats for pb in pats]


def scale_case():
    """-> [(name, data Vec, base, post factor)]"""
    return [(f"round {i}: {pattern}", vector("words", pattern, VECTOR_N, "scale", i), scalar(i), scalar(i + 4)) for i, pattern in rounds("words")]


# ---- quotient kernels, point by point (csrc/h2mi_plonk.hip) -----------------------------------------------------------------------------
# The columns of a round are named slots; the kernels work point by point, so they are arbitrary pattern vectors and no transforms of
# a witness.  beta, gamma, y (theta) of round i are scalar(i), scalar(i + 3), scalar(i + 7): every scalar in every slot after N_ROUNDS.
BF = 5


def challenges_of(i: int):
    return {"beta": scalar(i), "gamma": scalar(i + 3), "y": scalar(i + 7)}


def columns(alphabet: str, pattern: str, size: int, names, *key):
    """-> {name: Vec}: one vector per slot ("random choice": its own seed each)"""
    return {name: vector(alphabet, pattern, size, *key, name) for name in names}


def standard_plonk_program(custom):
    """the reference's StandardPlonk gate q_a a + q_b b + q_c c + q_ab a b + constant as a tree over advice 0 .. 2, fixed 0 .. 4"""
    A = lambda j: custom.Expression("query", "advice", j, 0)
    F = lambda j: custom.Expression("query", "fixed", j, 0)
    return F(0) * A(0) + F(1) * A(1) + F(2) * A(2) + F(3) * A(0) * A(1) + F(4)


STANDARD_K = 8  # degree 3: 512 points on the extended coset, two workgroups
STANDARD_SLOTS = [f"advice{j}" for j in range(3)] + [f"fixed{j}" for j in range(5)] + [f"sigma{j}" for j in range(3)] + [f"z{j}" for j in range(3)] + ["l0", "l_last", "l_active"]


def standard_rounds():
    """k_evaluate_h_standard_plonk: words as they lie"""
    size = 1 << (STANDARD_K + 1)
    return [dict(challenges_of(i), name=f"round {i}: {pattern}", pattern=pattern, cols=columns("words", pattern, size, STANDARD_SLOTS, "standard", i))
            for i, pattern in rounds("words")]


RANGE_K = 7  # degree 4 (chunks of two): 512 points
# (permutation columns, chunk, lookup input: "advice" — a lookup-advice column — or "selector" — selector * a): the sets are a full
# chunk and a ragged one; the kernel takes at most four permutation columns
RANGE_SHAPES = [(4, 2, "advice"), (3, 2, "selector")]


def range_slots(n_perm: int, chunk: int, lookup: str):
    sets = -(-n_perm // chunk)
    return (["a", "q", "table", "lk_pin", "lk_ptab", "lk_z", "l0", "l_last", "l_active", "lookup_advice" if lookup == "advice" else "lookup_selector"]
            + [f"perm_value{j}" for j in range(n_perm)] + [f"perm_sigma{j}" for j in range(n_perm)] + [f"perm_z{s}" for s in range(sets)])


def range_rounds(shape: int):
    n_perm, chunk, lookup = RANGE_SHAPES[shape]
    size = 1 << (RANGE_K + 2)
    return [dict(challenges_of(i), name=f"round {i}: {pattern}", pattern=pattern,
                 cols=columns("words", pattern, size, range_slots(n_perm, chunk, lookup), "range", shape, i)) for i, pattern in rounds("words")]


FLEX_K = 7
FLEX_GATES, FLEX_PERM, FLEX_CHUNK, FLEX_LOOKUPS = 3, 6, 2, 2  # degree 4: 512 points; lookup 1 has a second input factor
FLEX_SHUFFLES = 2
LOGUP_SETS = [1, 6]


def flex_slots():
    sets = -(-FLEX_PERM // FLEX_CHUNK)
    out = [f"gate_a{g}" for g in range(FLEX_GATES)] + [f"gate_q{g}" for g in range(FLEX_GATES)]
    out += [f"perm_value{j}" for j in range(FLEX_PERM)] + [f"perm_sigma{j}" for j in range(FLEX_PERM)] + [f"perm_z{s}" for s in range(sets)]
    for l in range(FLEX_LOOKUPS):
        out += [f"lk{l}_{part}" for part in ("in", "table", "pin", "ptab", "z")]
    return out + ["lk1_in_b", "l0", "l_last", "l_active"]


def flex_rounds():
    """k_evaluate_h_flex: several gates, six permutation columns in chunks of two, two lookups (one with a second input factor);
    every operand converted on load"""
    size = 1 << (FLEX_K + 2)
    return [dict(challenges_of(i), name=f"round {i}: {pattern}", pattern=pattern, cols=columns("values", pattern, size, flex_slots(), "flex", i))
            for i, pattern in rounds("values")]


def fold_slots(n_sets: int):
    """what evaluate_h_fold reads beyond k_evaluate_h_flex's own entry: shuffles, and one logUp lookup of n_sets input sets"""
    out = ["advice0", "l0", "l_last", "l_active", "lg_table", "lg_m", "lg_phi"] + [f"lg_in{j}" for j in range(n_sets)]
    for s in range(FLEX_SHUFFLES):
        out += [f"sf{s}_in", f"sf{s}_side", f"sf{s}_z"]
    return out


def fold_rounds(n_sets: int):
    size = 1 << (FLEX_K + 2)
    return [dict(challenges_of(i), name=f"round {i}: {pattern}", pattern=pattern, cols=columns("values", pattern, size, fold_slots(n_sets), "fold", n_sets, i))
            for i, pattern in rounds("values")]


# ---- bound-tight gate programs ----------------------------------------------------------------------------------------------------------
OP_ADVICE, OP_FIXED, OP_INSTANCE, OP_CONSTANT, OP_ADD, OP_SUB, OP_MUL, OP_NEG, OP_END, OP_CHALLENGE = range(10)  # include/h2mi.h
SMALL_TOP, CAP = 3.9, 8.0  # expr_encode: reduce above 3.9 before SUB / NEG (f29_sub's K4 takes a subtrahend below 4p - 2^232), above 8.0 after ADD / SUB
EXPR_ADVICE, EXPR_FIXED = 4, 2
EXPR_K = 7  # degree 4: 512 points
N_CHALLENGES = 2


def encode_trace(ops):
    """expr_encode's rule restated: a load is 1.04, a constant or challenge 1, a product 1 + 0.006 a b, a sum a + b, a difference a + 4,
    a negation 4, a reduction 1 + 0.006 a.  -> [(threshold "small" | "cap", the bound it saw, reduced?)] in program order"""
    b, out = [], []

    def check(kind, limit):
        reduced = b[-1] > limit
        out.append((kind, b[-1], reduced))
        if reduced:
            b[-1] = 1.0 + 0.006 * b[-1]

    for op, _, _ in ops:
        if op <= OP_INSTANCE:
            b.append(1.04)
        elif op in (OP_CONSTANT, OP_CHALLENGE):
            b.append(1.0)
        elif op == OP_ADD:
            top = b.pop()
            b[-1] += top
            check("cap", CAP)
        elif op == OP_SUB:
            check("small", SMALL_TOP)
            b.pop()
            b[-1] += 4.0
            check("cap", CAP)
        elif op == OP_MUL:
            top = b.pop()
            b[-1] = 1.0 + 0.006 * b[-1] * top
        elif op == OP_NEG:
            check("small", SMALL_TOP)
            b[-1] = 4.0
        else:
            assert op == OP_END and len(b) == 1
            b = []
    return out


def bound_tight_programs(custom):
    """-> [(name, custom.Expression, expectation)]; expectation: what encode_trace must say of the program, as a list of
    (threshold, bound, reduced?) it must CONTAIN (bounds to two decimals).  Queries walk the four advice and two fixed columns at
    rotations -2 .. 2, so neighbouring terms read different cells."""
    counter = [0]

    def Q():
        i = counter[0]
        counter[0] += 1
        kind, col = ("instance", 0) if i % 7 == 6 else ("advice", i % EXPR_ADVICE) if i % 3 else ("fixed", i % EXPR_FIXED)
        return custom.Expression("query", kind, col, (i % 5) - 2)

    def S(count):
        e = Q()
        for _ in range(count - 1):
            e = e + Q()
        return e

    NN = lambda: (-Q()) + (-Q())  # 4 + 4: 8.0 exactly, the cap's own value
    ch = lambda i: custom.Expression("challenge", i)
    top = custom.Expression.constant(R - 1)
    leaves = [S(7), NN(), S(3), -S(3), ch(1) * S(4), top + Q(), S(7)]  # the depth-8 stack: x0 - (x1 - (.. - (x6 - q)))
    chain = Q()
    for e in reversed(leaves):
        chain = e - chain
    return [
        ("7 queries times 7 queries", S(7) * S(7), [("cap", 7.28, False)]),
        ("8 queries", S(8), [("cap", 7.28, False), ("cap", 8.32, True)]),
        ("(-a) + (-b) times (-c) + (-d)", NN() * NN(), [("cap", 8.0, False)]),
        ("(-a) + (-b) as a subtrahend", ch(0) - NN(), [("cap", 8.0, False), ("small", 8.0, True)]),
        ("subtrahend of 3 queries", top - S(3), [("small", 3.12, False)]),
        ("subtrahend of 4 queries", ch(1) - S(4), [("small", 4.16, True)]),
        ("product plus two queries as a subtrahend", Q() - (Q() * Q() + Q() + Q()), [("small", 3.09, False)]),
        ("negated 3 queries", -S(3), [("small", 3.12, False)]),
        ("negated 4 queries", -S(4), [("small", 4.16, True)]),
        # consumed by a product: 0 - x + 4p is negative for x above 4p (four converted loads of OVER261), and only a sum's carry could
        # hide that; a product takes the limbs as they are
        ("negated 3 queries times a query", (-S(3)) * Q(), [("small", 3.12, False)]),
        ("negated 4 queries times a query", (-S(4)) * Q(), [("small", 4.16, True)]),
        ("zero minus 4 queries, times a challenge", (custom.Expression.constant(0) - S(4)) * ch(0), [("small", 4.16, True)]),
        ("challenge times 7 queries minus the constant r - 1", ch(0) * S(7) - top, [("cap", 7.28, False), ("small", 1.0, False)]),
        ("8 queries minus 8 queries", S(8) - S(8), [("cap", 8.32, True), ("small", 1.05, False)]),
        ("depth-8 stack", chain, [("cap", 7.28, False), ("cap", 8.0, False), ("small", 6.04, True), ("small", 8.0, True), ("cap", 11.28, True), ("cap", 12.0, True)]),
    ]


def compile_programs(trees):
    """-> (ops, constants) of the trees as one program (custom.Expression.program, a shared constant table)"""
    constants, ops = {}, []
    for t in trees:
        ops += t.program(constants)[0]
    return ops, sorted(constants, key=constants.get)


def expr_slots(with_terms: bool, circuit: int = 0):
    out = [f"c{circuit}_advice{j}" for j in range(EXPR_ADVICE)] + [f"c{circuit}_instance"]
    if with_terms:
        out += [f"c{circuit}_perm_value{j}" for j in range(2)] + [f"c{circuit}_perm_z{s}" for s in range(2)]  # four columns in chunks of two: two own, two advice
        out += [f"c{circuit}_lk_{part}" for part in ("pin", "ptab", "z")] + [f"c{circuit}_sf_{part}" for part in ("in", "side", "z")]
    return out


def expr_shared_slots(with_terms: bool):
    return [f"fixed{j}" for j in range(EXPR_FIXED)] + ["l0", "l_last", "l_active"] + ([f"perm_sigma{j}" for j in range(4)] if with_terms else [])


def expr_rounds(n_circuits: int, with_terms: bool):
    """k_evaluate_h_expr (one circuit) / k_evaluate_h_expr_batch: the bound-tight programs over the value patterns; with_terms: a
    permutation argument of four columns in chunks of two, one lookup (input advice0 times fixed1) and one shuffle"""
    size = 1 << (EXPR_K + 2)
    out = []
    for i, pattern in rounds("values"):
        names = expr_shared_slots(with_terms) + [s for c in range(n_circuits) for s in expr_slots(with_terms, c)]
        rnd = dict(challenges_of(i), name=f"round {i}: {pattern}", pattern=pattern, cols=columns("values", pattern, size, names, "expr", n_circuits, with_terms, i))
        rnd["challenges"] = [scalar(i + 5), scalar(i + 9)]
        out.append(rnd)
    return out


def expr_circuits(rnd, n_circuits: int, with_terms: bool, pick=lambda vec: vec.values):
    """a round's columns in the shape batched_quotient takes (pick = values) or the device wrappers take (pick = an upload)
    -> (circuits, shared)"""
    c = {name: pick(vec) for name, vec in rnd["cols"].items()}
    fixed = [c[f"fixed{j}"] for j in range(EXPR_FIXED)]
    shared = {"perm_sigmas": [c[f"perm_sigma{j}"] for j in range(4)] if with_terms else [], "chunk": 2, "l0": c["l0"], "l_last": c["l_last"], "l_active": c["l_active"]}
    circuits = []
    for i in range(n_circuits):
        advice = [c[f"c{i}_advice{j}"] for j in range(EXPR_ADVICE)]
        cc = {"advice": advice, "fixed": fixed, "instance": c[f"c{i}_instance"], "perm_values": [], "perm_zs": [], "lookups": [], "shuffles": []}
        if with_terms:
            cc["perm_values"] = [c[f"c{i}_perm_value0"], c[f"c{i}_perm_value1"], advice[1], fixed[0]]
            cc["perm_zs"] = [c[f"c{i}_perm_z{s}"] for s in range(2)]
            cc["lookups"] = [(advice[0], fixed[1], advice[2], c[f"c{i}_lk_pin"], c[f"c{i}_lk_ptab"], c[f"c{i}_lk_z"])]
            cc["shuffles"] = [(c[f"c{i}_sf_in"], c[f"c{i}_sf_side"], c[f"c{i}_sf_z"])]
        circuits.append(cc)
    return circuits, shared


def check_program(custom):
    """k_expr_check: polynomials that are zero on every row only because a full-bound value reduces to the zero word — equal columns
    s7 - s7' (7.28 + 4: reduced by the cap), (-a) + (-a') + (b + b') with b = -a (8 + 2.08: reduced), 4 (a + a') with a' = -a.
    -> trees over advice 0 .. 3; advice1 = advice0, advice3 = -advice2 on every row make all of them vanish"""
    A = lambda col, rot: custom.Expression("query", "advice", col, rot)
    s7 = lambda col: sum((A(col, r) for r in range(1, 7)), A(col, 0))
    pair = lambda rot: A(2, rot) + A(3, rot)
    return [s7(0) - s7(1), ((-A(2, 0)) + (-A(2, 1))) + ((-A(3, 0)) + (-A(3, 1))), pair(0) + pair(1) + pair(2) + pair(3), -(pair(0) + pair(1) + pair(2) + pair(3))]


CHECK_K = 9  # 512 rows
CHECK_PLANTED_ROW = 300  # in the second workgroup


def check_rounds():
    """-> [(name, [advice0 .. advice3] as Vec)] with advice1 = advice0 and advice3 = -advice2"""
    n = 1 << CHECK_K
    out = []
    for pattern in PATTERNS["values"]:
        a0, a2 = vector("values", pattern, n, "check", 0), vector("values", pattern, n, "check", 2)
        out.append((pattern, [a0, Vec(a0.words), a2, values_vec([-v for v in a2.values])]))
    return out


# ---- grand products and running sums ----------------------------------------------------------------------------------------------------
PRODUCT_K = 11
PRODUCT_U = (1 << PRODUCT_K) - (BF + 1)  # 2042 usable rows: two tiles of 1024
SPARSE_LOOKUP_K = 13  # the sparse form of the lookup product wants usable_rows >= 4096 and at most a quarter of the rows moving
SPARSE_LOOKUP_MOVING = 1500
PERM_M, PERM_CHUNK = 4, 2
PERM_SMALL_ACTIVE = 40  # k_perm_sparse_small: at most 256 positions


class ZeroDenominator(Exception):
    pass


def pick_challenges(i: int, admissible):
    """beta, gamma of round i — scalar(i), scalar(i + 3) — unless admissible(beta, gamma) names a zero factor; then the next gamma from
    the set, then the next beta.  -> (beta, gamma, [(beta, gamma, reason)] the pairs passed over).  Raises when no pair is left: a zero
    denominator is never silently skipped"""
    passed = []
    for db in range(len(SCALARS)):
        for dg in range(len(SCALARS)):
            beta, gamma = scalar(i + db), scalar(i + 3 + dg)
            reason = admissible(beta, gamma)
            if reason is None:
                return beta, gamma, passed
            passed.append((beta, gamma, reason))
    raise ZeroDenominator(f"round {i}: every pair of the set leaves a zero factor")


def _identity(k, m):
    import perm_scale_cases

    return perm_scale_cases.identity(k, m)


def perm_zero_factor(vals, sig, u, beta, gamma, rows=None, k=PRODUCT_K):
    """the first zero numerator or denominator factor of the permutation products over rows 0 .. u (or `rows`), or None"""
    ident = _identity(k, len(vals))
    for j in range(len(vals)):
        for i in (range(u) if rows is None else rows):
            if (vals[j][i] + beta * sig[j][i] + gamma) % R == 0:
                return f"v + beta sigma + gamma = 0 at column {j}, row {i}"
            if (vals[j][i] + beta * ident[j][i] + gamma) % R == 0:
                return f"v + beta delta^j omega^i + gamma = 0 at column {j}, row {i}"
    return None


def perm_rounds(sparse: bool):
    """plonk.permutation_products over four columns in chunks of two.  dense: every sigma a pattern vector.  sparse: sigma is the
    identity but at PERM_SMALL_ACTIVE positions (both ends of both sets among them), where it is a pattern word
    -> [round]: name, vals / sig (Vec), beta, gamma, passed, active (sorted positions set * u + row, or None)"""
    n, u = 1 << PRODUCT_K, PRODUCT_U
    out = []
    for i, pattern in rounds("values"):
        vals = [vector("values", pattern, n, "perm v", sparse, i, j) for j in range(PERM_M)]
        sig = [vector("values", pattern, n, "perm s", sparse, i, j) for j in range(PERM_M)]
        active = None
        if sparse:
            rng = random.Random(_seed("perm active", i))
            sets = PERM_M // PERM_CHUNK
            active = sorted({0, u - 1, (sets - 1) * u, sets * u - 1} | {rng.randrange(sets * u) for _ in range(PERM_SMALL_ACTIVE - 4)})
            ident = _identity(PRODUCT_K, PERM_M)
            moved = {}
            for p in active:  # one column of the set, or both
                s, row = divmod(p, u)
                for j in ((s * PERM_CHUNK, s * PERM_CHUNK + 1) if p % 3 == 0 else (s * PERM_CHUNK + p % 2,)):
                    moved[(j, row)] = sig[j].values[row]
            sig = [values_vec([moved.get((j, r), ident[j][r]) for r in range(n)]) for j in range(PERM_M)]
        v_, s_ = [v.values for v in vals], [s.values for s in sig]
        beta, gamma, passed = pick_challenges(i, lambda b, g: perm_zero_factor(v_, s_, u, b, g))
        out.append(dict(name=f"round {i}: {pattern}", pattern=pattern, vals=vals, sig=sig, beta=beta, gamma=gamma, passed=passed, active=active))
    return out


def lookup_zero_factor(a, t, ap, sp, u, beta, gamma):
    for i in range(u):
        for name, x, c in (("a + beta", a[i], beta), ("t + gamma", t[i], gamma), ("a' + beta", ap[i], beta), ("s' + gamma", sp[i], gamma)):
            if (x + c) % R == 0:
                return f"{name} = 0 at row {i}"
    return None


def lookup_rounds(sparse: bool):
    """plonk.lookup_product on four pattern columns (the kernel computes a recurrence and does not ask whether the permuted pair is a
    permutation).  sparse: k = 13, the permuted pair equals the pair but on SPARSE_LOOKUP_MOVING rows"""
    k = SPARSE_LOOKUP_K if sparse else PRODUCT_K
    n, u = 1 << k, (1 << k) - (BF + 1)
    out = []
    for i, pattern in rounds("values"):
        a, t, ap, sp = (vector("values", pattern, n, "lookup", sparse, i, name) for name in ("a", "t", "ap", "sp"))
        if sparse:
            rng = random.Random(_seed("lookup moving", i))
            moving = set(rng.sample(range(u), SPARSE_LOOKUP_MOVING)) | {0, u - 1}
            alphabet = ALPHABETS["values"]
            fresh = lambda row, w: w if row not in moving else alphabet[(alphabet.index(w) + 1 + row % (len(alphabet) - 1)) % len(alphabet)]
            ap = Vec([fresh(r, w) if r % 2 else w for r, w in enumerate(a.words)])
            sp = Vec([w if r % 2 else fresh(r, w) for r, w in enumerate(t.words)])
        beta, gamma, passed = pick_challenges(i, lambda b, g: lookup_zero_factor(a.values, t.values, ap.values, sp.values, u, b, g))
        out.append(dict(name=f"round {i}: {pattern}", pattern=pattern, k=k, u=u, a=a, t=t, ap=ap, sp=sp, beta=beta, gamma=gamma, passed=passed))
    return out


def shuffle_rounds():
    """the shuffle product z[i+1] = z[i] (A_i + gamma) / (S_i + gamma)"""
    n, u = 1 << PRODUCT_K, PRODUCT_U
    out = []
    for i, pattern in rounds("values"):
        a, s = vector("values", pattern, n, "shuffle a", i), vector("values", pattern, n, "shuffle s", i)

        def bad(_, g):
            for row in range(u):
                if (a.values[row] + g) % R == 0 or (s.values[row] + g) % R == 0:
                    return f"A + gamma or S + gamma = 0 at row {row}"
            return None

        _, gamma, passed = pick_challenges(i, bad)
        out.append(dict(name=f"round {i}: {pattern}", pattern=pattern, a=a, s=s, gamma=gamma, passed=passed))
    return out


def logup_rounds(n_sets: int):
    """the logUp sum phi[i+1] = phi[i] + sum_j 1 / (A_j,i + beta) - M_i / (S_i + beta); M is a pattern vector like the others (the
    kernel computes the recurrence whatever M holds)"""
    n, u = 1 << PRODUCT_K, PRODUCT_U
    out = []
    for i, pattern in rounds("values"):
        sets = [vector("values", pattern, n, "logup a", n_sets, i, j) for j in range(n_sets)]
        table, mult = vector("values", pattern, n, "logup t", n_sets, i), vector("values", pattern, n, "logup m", n_sets, i)

        def bad(b, _):
            for row in range(u):
                if (table.values[row] + b) % R == 0 or any((a.values[row] + b) % R == 0 for a in sets):
                    return f"A + beta or S + beta = 0 at row {row}"
            return None

        beta, _, passed = pick_challenges(i, bad)
        out.append(dict(name=f"round {i}: {pattern}", pattern=pattern, sets=sets, table=table, mult=mult, beta=beta, passed=passed))
    return out
