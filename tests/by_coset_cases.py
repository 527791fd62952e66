"""Coset-by-coset quotient (H2MI_KEYGEN_BY_COSET), shared by tests/test_by_coset_host.py and tests/test_gpu_by_coset.py.  The circuits
are the existing case modules'; what is new here is the memory formula of DESIGN.md 3 for both layouts — the bytes of the device vectors a
key and one prover own, from the constraint system's counts — and the inputs of the slice kernel's cases: polynomials of degree below
2^k, so that every column has both an extended-coset form and 2^(extended_k - k) slices."""
import random

from oracle import bn254 as o

R = o.R
KEYGEN_BY_COSET = 8  # include/h2mi_prover.h H2MI_KEYGEN_BY_COSET
EINVAL = -1
# the *_COSET buffer kinds of include/h2mi_prover.h: (prover kinds, key kinds)
PROVER_COSET_KINDS = (2, 6)  # H2MI_BUF_ADVICE_COSET, H2MI_BUF_PERM_Z_COSET
KEY_COSET_KINDS = (66, 69, 70, 71, 72)  # H2MI_PKBUF_FIXED_COSET, _SIGMA_COSET, _L0_COSET, _L_LAST_COSET, _L_ACTIVE_COSET


# ---- the memory formula, in bytes ------------------------------------------------------------------------------------------
def gwc_points(advice_queries, fixed_queries, k, n_sets, n_lookups, n_shuffles, blinding_factors, logup) -> int:
    """the distinct rotations a proof opens at (h and the random polynomial at 0): the commitments of a GWC tail"""
    n = 1 << k
    rots = {0} | {r % n for _, r in advice_queries} | {r % n for _, r in fixed_queries}
    if n_sets or n_lookups or n_shuffles:
        rots.add(1)
    if n_sets > 1:
        rots.add(-(blinding_factors + 1) % n)
    if n_lookups and not logup:
        rots.add(-1 % n)
    return len(rots)


def device_bytes(c: dict, by_coset: bool):
    """-> (key bytes, prover bytes) right after h2mi_prover_create.  c: k, degree, blinding_factors, n_advice, n_fixed, n_instance,
    n_perm, n_shuffles, logup, gwc_points; lookups: per lookup ("exprs", input sets) for a lookup given as a program or ("column", has a
    selector, distinct table values) for the single-column form; n_active: the distinct (permutation set, usable row) pairs the copy
    constraints move; n_moved: the cells they move.  With n = 2^k, E = 2^extended_k and C the length of a `coset` vector — E resident, n
    by coset — in field elements of 32 bytes:
      key    = 2 n (F + m) + [resident: E (F + m + 3) | by coset: 3 n] + index vectors
      prover = (A + sets) (2 n + C) + I (n + C) + lookups + shuffles + 11 n + E + 3 P + [by coset: n (F + m + 3 + I)]"""
    k, degree, bf = c["k"], c["degree"], c["blinding_factors"]
    A, F, I, m, S, logup = c["n_advice"], c["n_fixed"], c["n_instance"], c["n_perm"], c["n_shuffles"], c["logup"]
    n = 1 << k
    ext_k = k
    while (1 << ext_k) < n * (degree - 1):
        ext_k += 1
    E, u = 1 << ext_k, n - (bf + 1)
    C = n if by_coset else E
    chunk = degree - 2
    sets = -(-m // chunk) if m else 0
    L = len(c["lookups"])
    table = lambda rows: 2 * rows + rows // 8 + 1  # sorted canonical, sorted Montgomery, multiplicities (32 bits each)
    key = 2 * n * (F + m) + (3 * n if by_coset else E * (F + m + 3))
    key += (c["n_active"] // 8 + 1 if m else 0) + (c["n_moved"] // 2 + 1 if c["n_moved"] else 0)
    forms = 2 * n + C
    prover = (A + sets) * forms + I * (n + C)
    for lk in c["lookups"]:
        if lk[0] == "exprs":
            key += 0
            prover += (lk[1] + 1) * (n + C) + table(u)  # both sides compressed on the rows and on the coset; the sorted table of a proof
        else:
            key += table(lk[2])
            prover += n if lk[1] else 0  # selector * advice on the rows
        prover += forms * (2 if logup else 3)  # M and phi, or the permuted pair and the product
    prover += S * (2 * n + 2 * C + forms)
    P = max(A, (1 if logup else 2) * L, sets + L + S + 1, degree - 1, 8, c["gwc_points"])
    prover += 11 * n + E + 3 * P  # the random polynomial, h_poly, SHPLONK's nine vectors; h; 96 bytes per result slot
    if by_coset:
        prover += n * (F + m + 3 + I)  # the slices of the key's shared columns; every instance column's coefficients
    return 32 * key, 32 * prover


# three shapes worked out by hand from the allocation list (tests/test_by_coset_host.py): counts -> ((key, prover) resident, by coset)
HAND_SHAPES = [
    # StandardPlonk at k = 5: n = 32, E = 64
    ({"k": 5, "degree": 3, "blinding_factors": 5, "n_advice": 3, "n_fixed": 5, "n_instance": 0, "n_perm": 3, "n_shuffles": 0, "logup": False,
      "gwc_points": 2, "lookups": [], "n_active": 0, "n_moved": 0}, (38944, 38656), (19488, 43776)),
    # degree 9 at k = 6 (n = 64, E = 512): two instance columns, a logUp lookup of three input sets, a shuffle
    ({"k": 6, "degree": 9, "blinding_factors": 5, "n_advice": 2, "n_fixed": 3, "n_instance": 2, "n_perm": 4, "n_shuffles": 1, "logup": True,
      "gwc_points": 3, "lookups": [("exprs", 3)], "n_active": 10, "n_moved": 20}, (192928, 313984), (35232, 137856)),
    # a range-like shape at k = 7, degree 4 (n = 128, E = 512): a single-column lookup with a selector over 16 table values
    ({"k": 7, "degree": 4, "blinding_factors": 5, "n_advice": 2, "n_fixed": 3, "n_instance": 1, "n_perm": 3, "n_shuffles": 0, "logup": False,
      "gwc_points": 4, "lookups": [("column", True, 16)], "n_active": 0, "n_moved": 0}, (197760, 258816), (62592, 201472)),
]


def quotient_columns(c: dict) -> int:
    """the vectors the quotient reads for ONE circuit, the key's shared ones included: what by coset keeps as a slice of n elements"""
    chunk = c["degree"] - 2
    sets = -(-c["n_perm"] // chunk) if c["n_perm"] else 0
    cols = c["n_advice"] + c["n_fixed"] + c["n_instance"] + c["n_perm"] + sets + 3
    for lk in c["lookups"]:
        cols += (lk[1] + 1 if lk[0] == "exprs" else 0) + (2 if c["logup"] else 3)
    return cols + 3 * c["n_shuffles"]


def counts_of(abi, lookups, n_shuffles: int, logup: bool, sigma_rows, delta: int, omega: int) -> dict:
    """the counts device_bytes takes, off an engine.ConstraintSystem and the key's sigma columns (Python integers, one list per column):
    a cell is moved when its sigma value is not the identity's DELTA^j omega^i"""
    n, bf = 1 << abi.k, abi.blinding_factors
    u, chunk = n - (bf + 1), abi.degree - 2
    moved, active = 0, set()
    for j, col in enumerate(sigma_rows):
        ident = pow(delta, j, R)
        for i, v in enumerate(col):
            if v != ident:
                moved += 1
                if i < u:
                    active.add((j // chunk, i))
            ident = ident * omega % R
    sets = -(-abi.n_perm // chunk) if abi.n_perm else 0
    aq = [(abi.advice_queries[i].column, abi.advice_queries[i].rotation) for i in range(abi.n_advice_queries)]
    fq = [(abi.fixed_queries[i].column, abi.fixed_queries[i].rotation) for i in range(abi.n_fixed_queries)]
    return {"k": abi.k, "degree": abi.degree, "blinding_factors": bf, "n_advice": abi.n_advice, "n_fixed": abi.n_fixed, "n_instance": abi.n_instance,
            "n_perm": abi.n_perm, "n_shuffles": n_shuffles, "logup": logup, "lookups": lookups, "n_active": len(active), "n_moved": moved,
            "gwc_points": gwc_points(aq, fq, abi.k, sets, len(lookups), n_shuffles, bf, logup)}


# ---- the index convention: a slice of the extended coset -----------------------------------------------------------------------------------
def coset_slice(dom, coeffs, c: int):
    """the n-point transform of `coeffs` with pre-scale zeta extended_omega^c over the rows' generator: coefficient j times shift^j, then
    the plain transform"""
    shift = dom.g_coset * pow(dom.extended_omega, c, R) % R
    scaled, s = [], 1
    for a in coeffs:
        scaled.append(a * s % R)
        s = s * shift % R
    return o.ntt(scaled, dom.omega)


# ---- the slice kernel's cases ---------------------------------------------------------------------------------------------------------------
# (k, cs degree -> rot = 2^(extended_k - k), circuits, lookups: "plain" or the input sets K of a logUp lookup).  32, 256 and 512 rows: a
# partial workgroup, exactly one, two; rot 2, 4, 8, 16; 1, 2 and 3 circuits; K = 1, 3, 6 (the set stride) and the permuted pair
KERNEL_CASES = [
    (5, 3, 1, "plain"),
    (5, 9, 3, 3),
    (5, 17, 2, 6),
    (8, 5, 2, 1),
    (8, 3, 1, "plain"),
    (9, 5, 1, "plain"),
    (9, 3, 3, 1),
    (9, 17, 1, 3),
]
N_ADV, N_FIX, N_INST, N_PERM, CHUNK, N_SHUFFLES, BF = 3, 2, 2, 3, 2, 2, 5


def kernel_case(custom, case: int):
    """-> dict: the program (rotations -1, +1, +3; both instance columns; a challenge), and per vector its COEFFICIENTS (random, degree
    below 2^k): `shared` and `circuits` laid out as instance_cases.batched_quotient takes them — a permutation of two sets, one lookup
    (plain, or logUp with K input sets), two shuffles, two instance columns"""
    k, degree, n_circuits, lookup = KERNEL_CASES[case]
    rng = random.Random(9900 + case)
    n = 1 << k
    Q = lambda kind, index, r: custom.Expression("query", kind, index, r)
    ch = custom.Expression("challenge", 0)
    trees = [Q("advice", 0, -1) * Q("fixed", 0, 1) + Q("instance", 1, 3) * ch - Q("advice", 1, 0),
             Q("instance", 0, -1) - Q("advice", 2, 3) * Q("fixed", 1, -1),
             Q("advice", 2, 1) + custom.Expression.constant(rng.randrange(R))]
    poly = lambda: [rng.randrange(R) for _ in range(n)]
    fixed = [poly() for _ in range(N_FIX)]
    shared = {"perm_sigmas": [poly() for _ in range(N_PERM)], "chunk": CHUNK, "l0": poly(), "l_last": poly(), "l_active": poly()}
    circuits = []
    for _ in range(n_circuits):
        c = {"advice": [poly() for _ in range(N_ADV)], "fixed": fixed, "instance": [poly() for _ in range(N_INST)]}
        c["perm_values"] = [c["advice"][0], fixed[0], c["instance"][1]]
        c["perm_zs"] = [poly() for _ in range(-(-N_PERM // CHUNK))]
        if lookup == "plain":
            c["lookups"] = [(poly(), fixed[1], poly(), poly(), poly(), poly())]  # a second input factor too
        else:
            c["lookups"] = [([poly() for _ in range(lookup)], None, poly(), poly(), None, poly())]
        c["shuffles"] = [(poly(), poly(), poly()) for _ in range(N_SHUFFLES)]
        circuits.append(c)
    return {"k": k, "degree": degree, "trees": trees, "challenges": [rng.randrange(R)], "shared": shared, "circuits": circuits, "logup": lookup != "plain",
            "sets": 1 if lookup == "plain" else lookup, "beta": rng.randrange(R), "gamma": rng.randrange(R), "y": rng.randrange(R), "bf": BF}


def map_vectors(kc: dict, f):
    """kernel_case's `shared` and `circuits` with f applied to every vector; one input list gives one output (shared vectors stay shared)"""
    seen = {}

    def g(v):
        if v is None:
            return None
        if id(v) not in seen:
            seen[id(v)] = f(v)
        return seen[id(v)]

    sh = kc["shared"]
    shared = {"perm_sigmas": [g(v) for v in sh["perm_sigmas"]], "chunk": sh["chunk"], "l0": g(sh["l0"]), "l_last": g(sh["l_last"]), "l_active": g(sh["l_active"])}
    circuits = []
    for c in kc["circuits"]:
        lookups = [([g(a) for a in lk[0]] if isinstance(lk[0][0], list) else g(lk[0]),) + tuple(g(v) for v in lk[1:]) for lk in c["lookups"]]
        circuits.append({"advice": [g(v) for v in c["advice"]], "fixed": [g(v) for v in c["fixed"]], "instance": [g(v) for v in c["instance"]],
                         "perm_values": [g(v) for v in c["perm_values"]], "perm_zs": [g(v) for v in c["perm_zs"]], "lookups": lookups,
                         "shuffles": [tuple(g(v) for v in sf) for sf in c["shuffles"]]})
    return shared, circuits
