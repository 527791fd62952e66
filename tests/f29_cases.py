"""Cases of the lazy 29-bit-limb field / curve layer (csrc/f29.cuh, g1_29.cuh): the operand builders and the big-integer checks
behind tests/test_f29_host.py (the g++ build of the headers) and tests/test_gpu_f29.py (the same code as the device compiles it,
through the h2mi_dbg_f29_* hooks).  Every check takes a backend with the same eight calls (HostBackend / DeviceBackend below):
    mul(field, mode, A, B, n)  reduce_loose(field, limbs)  mul_raw(field, a, b)  sqr_raw(field, a)
    mul2_raw(field, a, b, c, d)  mul3_raw(field, ops)  chains([(pts, signs), ...], tree)  point_raw(op, a, b)
Every comparison is exact: against Python integers modulo p, `got * 2^261 == want (mod p)`, `got < want // 2^261 + p + 1`, limbs
0..7 below 2^29, canonical outputs below p.  All operands stay inside the contracts f29.cuh states."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import bn254 as o

FIELDS = [(0, o.Q), (1, o.R)]
M29 = (1 << 29) - 1
LAZY_MAX = int(1.9 * (1 << 30))  # f29_mul: limbs(a) < 1.9 * 2^30
TOP25 = (1 << 25) - 1            # top limb of a normalized operand: value < 2^257 (< 8p)

_VP, _SZ = C.c_void_p, C.c_size_t
_SIGNATURES = {
    "mul": [C.c_int, C.c_int, _VP, _VP, _VP, _SZ],
    "reduce_loose": [C.c_int, _VP, _VP, _SZ],
    "mul_raw": [C.c_int, _VP, _VP, _VP, _SZ],
    "sqr_raw": [C.c_int, _VP, _VP, _SZ],
    "mul2_raw": [C.c_int] + [_VP] * 5 + [_SZ],
    "mul3_raw": [C.c_int, _VP, _VP, _SZ],
    "point_raw": [C.c_int, _VP, _VP, _VP, _SZ],
}


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SRC = os.path.join(ROOT, "tests", "host", "f29_host.cpp")
HOST_SO = os.path.join(ROOT, "tests", "host", "libf29host.so")


def host_lib():
    """the g++ build of the headers (tests/host/f29_host.cpp), rebuilt when a source is newer"""
    deps = [HOST_SRC] + [os.path.join(ROOT, "halo2-scaffold_amd", "csrc", f) for f in ("f29.cuh", "g1_29.cuh", "f29_consts.inc", "f29_testops.cuh")]
    if not os.path.exists(HOST_SO) or os.path.getmtime(HOST_SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", HOST_SO, HOST_SRC])
    return C.CDLL(HOST_SO)


class _Backend:
    """the seven elementwise calls over a library; `symbols`: its entry point for each; `checked`: they return a status that must be 0"""

    def __init__(self, lib, symbols, checked):
        self.lib, self.checked = lib, checked
        self.fn = {}
        for name, args in _SIGNATURES.items():
            f = getattr(lib, symbols[name])
            f.argtypes, f.restype = args, (C.c_int if checked else None)
            self.fn[name] = f

    def _call(self, name, *args):
        rc = self.fn[name](*args)
        assert not self.checked or rc == 0, (name, rc)

    def mul(self, field, mode, A, B, n=None):
        n = len(A) if n is None else n
        out = np.zeros((n, 4), dtype=np.uint64)
        self._call("mul", field, mode, A.ctypes.data, B.ctypes.data, out.ctypes.data, n)
        return out

    def _raw(self, name, field, *ops):
        ops = [np.ascontiguousarray(x, dtype=np.uint32) for x in ops]
        n = len(ops[0])
        assert all(x.shape == (n, 9) for x in ops)
        out = np.zeros((n, 9), dtype=np.uint32)
        self._call(name, field, *[x.ctypes.data for x in ops], out.ctypes.data, n)
        return out

    def reduce_loose(self, field, limbs):
        return self._raw("reduce_loose", field, limbs)

    def mul_raw(self, field, a, b):
        return self._raw("mul_raw", field, a, b)

    def sqr_raw(self, field, a):
        return self._raw("sqr_raw", field, a)

    def mul2_raw(self, field, a, b, c, d):
        return self._raw("mul2_raw", field, a, b, c, d)

    def mul3_raw(self, field, ops):
        ops = np.ascontiguousarray(ops, dtype=np.uint32)
        n = ops.shape[1]
        assert ops.shape == (6, n, 9)
        out = np.zeros((n, 9), dtype=np.uint32)
        self._call("mul3_raw", field, ops.ctypes.data, out.ctypes.data, n)
        return out

    def point_raw(self, op, a, b):
        """one g1_29.cuh point operation per element on raw coordinates (f29t_point_raw_one; the cases: tests/g1_29_edge_cases.py):
        a, b and the result hold 36 words per element"""
        a, b = (np.ascontiguousarray(x, dtype=np.uint32) for x in (a, b))
        n = len(a)
        assert a.shape == (n, 36) and b.shape == (n, 36)
        out = np.zeros((n, 36), dtype=np.uint32)
        self._call("point_raw", op, a.ctypes.data, b.ctypes.data, out.ctypes.data, n)
        return out


class HostBackend(_Backend):
    """tests/host/f29_host.cpp compiled with g++ (f29t_*)"""

    def __init__(self, lib):
        symbols = {"mul": "f29t_mul", "reduce_loose": "f29t_reduce_loose", "mul_raw": "f29t_mul_raw", "sqr_raw": "f29t_sqr_raw",
                   "mul2_raw": "f29t_mul2_raw", "mul3_raw": "f29t_mul3_raw", "point_raw": "f29t_point_raw"}
        super().__init__(lib, symbols, checked=False)
        lib.f29t_madd_chain.argtypes, lib.f29t_madd_chain.restype = [_VP, _VP, _SZ, _VP, C.c_int], None

    def chains(self, cases, tree=0):
        outs = np.zeros((len(cases), 16), dtype=np.uint64)
        for i, (pts, signs) in enumerate(cases):
            P = o.pack_points(pts)
            S = np.array(signs, dtype=np.uint8)
            self.lib.f29t_madd_chain(P.ctypes.data, S.ctypes.data, len(pts), outs[i].ctypes.data, tree)
        return outs


class DeviceBackend(_Backend):
    """libh2mi_hooks.so on the GPU (h2mi_dbg_f29_*, h2mi_dbg_g1_29_chains): all chains of a call in one launch"""

    def __init__(self, lib):
        symbols = {"mul": "h2mi_dbg_f29_mul", "reduce_loose": "h2mi_dbg_f29_reduce_loose", "mul_raw": "h2mi_dbg_f29_mul_raw",
                   "sqr_raw": "h2mi_dbg_f29_sqr_raw", "mul2_raw": "h2mi_dbg_f29_mul2_raw", "mul3_raw": "h2mi_dbg_f29_mul3_raw",
                   "point_raw": "h2mi_dbg_g1_29_raw_op"}
        super().__init__(lib, symbols, checked=True)
        lib.h2mi_dbg_g1_29_chains.argtypes, lib.h2mi_dbg_g1_29_chains.restype = [_VP, _VP, _VP, _SZ, _VP, C.c_int], C.c_int

    def chains(self, cases, tree=0):
        pts = [p for c in cases for p in c[0]]
        P = o.pack_points(pts)
        S = np.array([s for c in cases for s in c[1]], dtype=np.uint8)
        offsets = np.cumsum([0] + [len(c[0]) for c in cases]).astype(np.uint64)
        outs = np.zeros((len(cases), 16), dtype=np.uint64)
        rc = self.lib.h2mi_dbg_g1_29_chains(P.ctypes.data, S.ctypes.data, offsets.ctypes.data, len(cases), outs.ctypes.data, tree)
        assert rc == 0, rc
        return outs


def limb_val(row):
    return sum(int(x) << (29 * i) for i, x in enumerate(row))


# ---- operand builders ---------------------------------------------------------------------------------------------------------------
def edge(mod):
    return [0, 1, 2, mod - 1, mod - 2, (1 << 253) % mod, (1 << 232) - 1, 1 << 232, (1 << 29) - 1, 1 << 29, ((1 << 254) - 1) % mod]


def mul_mode_values(field, mod):
    rng = np.random.default_rng(7 + field)
    vals_a = edge(mod) + [int.from_bytes(rng.bytes(32), "little") % mod for _ in range(3000)]
    vals_b = list(reversed(edge(mod))) + [int.from_bytes(rng.bytes(32), "little") % mod for _ in range(3000)]
    return vals_a, vals_b


def reduce_loose_values(field, mod):
    rng = np.random.default_rng(11 + field)
    vals = [0, 1, mod - 1, mod, mod + 1, 2 * mod - 1, 2 * mod, 3 * mod - 1, 3 * mod, 31 * mod + 5, 64 * mod - 1, 63 * mod, (1 << 232) - 1, 1 << 232]
    vals += [k * mod + d for k in range(0, 64, 7) for d in (0, 1, mod - 1)]
    vals += [int.from_bytes(rng.bytes(33), "little") % (64 * mod) for _ in range(20000)]
    limbs = np.array([[(v >> (29 * i)) & M29 if i < 8 else v >> 232 for i in range(9)] for v in vals], dtype=np.uint32)
    return vals, limbs


def extreme_values(mod):
    pats = [mod - 1, mod - 2, (1 << 254) - 1, ((1 << 254) - 1) - mod, int("1" * 253, 2), int("10" * 126, 2), int("01" * 127, 2),
            M29 * sum(1 << (29 * i) for i in range(8)), (1 << 232) - 1, (mod >> 1), (mod >> 1) + 1]
    return [p % mod for p in pats]


def mul2_operands():
    """random operands and the largest limbs the contract of f29_mul2 allows: a < 1.5 * 2^30, c < 2^30, b and d < 2^29 per limb"""
    rng = np.random.default_rng(29)
    n = 4000
    lim = {"a": 3 << 29, "b": 1 << 29, "c": 1 << 30, "d": 1 << 29}
    ops = {k: rng.integers(0, v, size=(n, 9), dtype=np.uint32) for k, v in lim.items()}
    for k, v in lim.items():
        ops[k][:8] = v - 1        # every limb at its maximum, all four operands together
        ops[k][8:16, ::2] = v - 1
    ops["b"][:, 8] &= TOP25  # top limbs of normalized values below 8p
    ops["d"][:, 8] &= TOP25
    return ops


def mul3_operands():
    """every limb of all six operands of f29_mul3 at 2^29 - 1 and random normalized operands"""
    rng = np.random.default_rng(31)
    n = 3000
    ops = rng.integers(0, 1 << 29, size=(6, n, 9), dtype=np.uint32)
    ops[:, :8, :] = M29
    ops[:, 8:16, ::2] = M29
    ops[:, 16:, 8] &= TOP25
    return ops


def mul_raw_operands():
    """f29_mul at its stated limit: a lazy (limbs up to int(1.9 * 2^30) - 1) against b normalized (limbs up to 2^29 - 1, top limb masked
    so that b < 8p): every limb of both at its maximum, every second limb at its maximum (both phases), random operands under the limits"""
    rng = np.random.default_rng(37)
    n = 4000
    lim = {"a": LAZY_MAX, "b": 1 << 29}
    ops = {k: rng.integers(0, v, size=(n, 9), dtype=np.uint32) for k, v in lim.items()}
    for k, v in lim.items():
        ops[k][:8] = v - 1
        ops[k][8:16, ::2] = v - 1
        ops[k][16:24, 1::2] = v - 1
    ops["a"][24:32] = LAZY_MAX - 1    # the lazy maximum against random normalized operands, and the reverse
    ops["b"][32:40] = M29
    ops["b"][:, 8] &= TOP25
    return ops


def sqr_raw_operands():
    """f29_sqr of normalized operands: all nine limbs at 2^29 - 1, every second limb at 2^29 - 1 (both phases), the same with the top
    limb masked (value < 8p), random operands with the top limb masked"""
    rng = np.random.default_rng(41)
    n = 4000
    a = rng.integers(0, 1 << 29, size=(n, 9), dtype=np.uint32)
    a[24:, 8] &= TOP25
    a[:8] = M29
    a[8:16, ::2] = M29
    a[16:24, 1::2] = M29
    a[24:32] = M29
    a[24:32, 8] = TOP25
    return a


# ---- checks ------------------------------------------------------------------------------------------------------------------------
def check_mul_modes(be, field, mod):
    vals_a, vals_b = mul_mode_values(field, mod)
    A, B = o.pack(vals_a, mod), o.pack(vals_b, mod)
    assert o.unpack(be.mul(field, 0, A, B), mod) == [x * y % mod for x, y in zip(vals_a, vals_b)]
    assert o.unpack(be.mul(field, 1, A, B), mod) == [x * y % mod for x, y in zip(vals_a, vals_b)]
    assert o.unpack(be.mul(field, 2, A, B), mod) == [(x + y) * (x - y) % mod for x, y in zip(vals_a, vals_b)]
    assert o.unpack(be.mul(field, 4, A, B), mod) == [x * x % mod for x in vals_a]
    assert o.unpack(be.mul(field, 5, A, B, 64), mod) == [pow(x, -1, mod) if x else 0 for x in vals_a[:64]]
    out = be.mul(field, 3, A, B)
    assert np.array_equal(out, A)
    assert all(v < mod for v in o.unpack(out))


def check_reduce_loose(be, field, mod):
    """the multiplication-free final reduction of the NTT: any normalized value below 64p -> canonical."""
    vals, limbs = reduce_loose_values(field, mod)
    out = be.reduce_loose(field, limbs)
    assert [limb_val(r) for r in out] == [v % mod for v in vals]
    assert (out[:, :8] < (1 << 29)).all()


def xyzz_to_affine(out):
    X, Y, ZZ, ZZZ = (o.limbs_to_int(out[4 * i : 4 * i + 4]) * pow(o.MONT_R, -1, o.Q) % o.Q for i in range(4))
    if ZZ == 0:
        assert not out.any()  # the identity is written as all zeros
        return None
    assert pow(ZZ, 3, o.Q) == ZZZ * ZZZ % o.Q
    return (X * pow(ZZ, -1, o.Q) % o.Q, Y * pow(ZZZ, -1, o.Q) % o.Q)


def _signed_sum(pts, signs):
    want = None
    for p, s in zip(pts, signs):
        want = o.g1_add(want, o.g1_neg(p) if s else p)
    return want


def _check_chains(be, cases, tree=0):
    outs = be.chains(cases, tree)
    for i, (pts, signs) in enumerate(cases):
        assert xyzz_to_affine(outs[i]) == _signed_sum(pts, signs), (tree, i)


def madd_chain_cases():
    rng = np.random.default_rng(3)
    pts = [o.g1_mul(int(rng.integers(1, 1 << 62)), o.G1_GEN) for _ in range(200)]
    signs = [int(rng.integers(0, 2)) for _ in pts]
    big = [o.g1_mul(o.R - 1 - i, o.G1_GEN) for i in range(5)]
    return [
        (pts, signs),                                      # long chain: the accumulator invariants must hold
        (pts[:1], [1]),                                    # single negated point
        ([pts[0], pts[0]], [0, 0]),                        # P + P  (doubling branch)
        ([pts[0], pts[0]], [1, 1]),                        # (-P) + (-P)
        ([pts[0], pts[0]], [0, 1]),                        # P - P = identity
        ([pts[0], pts[0], pts[1]], [0, 1, 0]),             # identity then restart
        ([pts[0], pts[0], pts[0], pts[0]], [0, 0, 0, 0]),  # 2P then +P then +P
        ([None, pts[2], None, pts[3]], [0, 0, 1, 1]),      # identity table entries skipped
        ([o.G1_GEN] * 33, [0] * 33),                       # n*G: first addition doubles, rest are generic
        (big + pts[:5], [0] * 10),
    ]


def check_madd_chain_random_and_special_cases(be):
    _check_chains(be, madd_chain_cases())


def tree_cases():
    """{tree: [(pts, signs), ...]} for the XYZZ + XYZZ folds"""
    rng = np.random.default_rng(11)
    pts = [o.g1_mul(int(rng.integers(1, 1 << 62)), o.G1_GEN) for _ in range(300)]
    signs = [int(rng.integers(0, 2)) for _ in pts]
    cases = {}
    for tree in (2, 4, 8, 16):
        cases[tree] = [(pts, signs),
                       (pts[:tree], signs[:tree]),   # one point per group
                       (pts[:3], signs[:3])]         # mostly empty groups (identity operands)
    cases[16].append(([pts[0]] * 16, [0] * 16))      # all groups equal: every fold step doubles
    cases[2].append(([pts[0], pts[0]], [0, 1]))      # groups cancel
    return cases


def check_full_add_and_double_trees(be):
    """XYZZ + XYZZ additions (the fold / bucket-reduction kernels) incl. doubling and cancellation branches."""
    for tree, cases in tree_cases().items():
        _check_chains(be, cases, tree)


def long_chain_case():
    rng = np.random.default_rng(99)
    base = [o.g1_mul(int(rng.integers(1, 1 << 62)), o.G1_GEN) for _ in range(50)]
    pts, signs = [], []
    for i in range(5000):
        pts.append(base[int(rng.integers(0, 50))])
        signs.append(int(rng.integers(0, 2)))
    return pts, signs


def check_long_chain_keeps_invariants(be):
    """5,000 mixed additions into one accumulator: the loose-reduction invariants of g1_29.cuh must hold
    indefinitely (a drift in the value bounds would eventually corrupt the sum)."""
    pts, signs = long_chain_case()
    out = be.chains([(pts, signs)], 0)[0]
    # expected: sum over the 50 base points of (count_plus - count_minus) * P
    coef = {}
    for p, s in zip(pts, signs):
        coef[p] = coef.get(p, 0) + (-1 if s else 1)
    want = None
    for p, c in coef.items():
        want = o.g1_add(want, o.g1_mul(c % o.R, p))
    assert xyzz_to_affine(out) == want


def check_extreme_limb_patterns(be):
    """field elements whose 29-bit limbs are all-ones / alternating / near the modulus: worst cases for the
    64-bit column accumulators of f29_mul and f29_sqr."""
    for field, mod in FIELDS:
        pats = extreme_values(mod)
        A = o.pack([a for a in pats for _ in pats], mod)
        B = o.pack([b for _ in pats for b in pats], mod)
        av, bv = o.unpack(A, mod), o.unpack(B, mod)
        assert o.unpack(be.mul(field, 0, A, B), mod) == [x * y % mod for x, y in zip(av, bv)]
        assert o.unpack(be.mul(field, 2, A, B), mod) == [(x + y) * (x - y) % mod for x, y in zip(av, bv)]
        assert o.unpack(be.mul(field, 4, A, B), mod) == [x * x % mod for x in av]


def _check_montgomery_rows(out, wants, mod):
    """out[i] is a normalized representative of wants[i] / 2^261 below wants[i] // 2^261 + p + 1"""
    assert (out[:, :8] < (1 << 29)).all()
    for i, want in enumerate(wants):
        got = limb_val(out[i])
        assert got * (1 << 261) % mod == want % mod, i
        assert got < want // (1 << 261) + mod + 1, i


def check_mul2_at_the_contract_limits(be):
    """f29_mul2 = (a b + c d) / 2^261 with one reduction (the Y3 of the mixed addition): random operands and the
    largest limbs its contract allows (a < 1.5 * 2^30, c < 2^30, b and d < 2^29 per limb) — the 64-bit column
    accumulators must not wrap."""
    ops = mul2_operands()
    v = {k: [limb_val(r) for r in ops[k]] for k in "abcd"}
    wants = [a * b + c * d for a, b, c, d in zip(v["a"], v["b"], v["c"], v["d"])]
    for field, mod in FIELDS:
        _check_montgomery_rows(be.mul2_raw(field, ops["a"], ops["b"], ops["c"], ops["d"]), wants, mod)


def check_mul3_at_the_contract_limits(be):
    """f29_mul3 = (a b + c d + e f) / 2^261 (three terms of a linear combination, one reduction): every limb of all six
    operands at 2^29 - 1 and random normalized operands."""
    ops = mul3_operands()
    v = [[limb_val(r) for r in ops[q]] for q in range(6)]
    wants = [v[0][i] * v[1][i] + v[2][i] * v[3][i] + v[4][i] * v[5][i] for i in range(ops.shape[1])]
    for field, mod in FIELDS:
        _check_montgomery_rows(be.mul3_raw(field, ops), wants, mod)


def check_mul_raw_at_the_contract_limit(be, field, mod):
    """f29_mul = a b / 2^261 at the limit its header states: limbs(a) < 1.9 * 2^30 (lazy) against b normalized — a column of
    9 * 1.9 * 2^59 + 9 * 2^58 = 21.6 * 2^59 must not wrap the 64-bit accumulator, on either compiler's code."""
    ops = mul_raw_operands()
    assert ops["a"].max() == LAZY_MAX - 1 and ops["b"][:, :8].max() == M29
    wants = [limb_val(a) * limb_val(b) for a, b in zip(ops["a"], ops["b"])]
    _check_montgomery_rows(be.mul_raw(field, ops["a"], ops["b"]), wants, mod)


def check_sqr_raw_at_the_contract_limit(be, field, mod):
    """f29_sqr = a^2 / 2^261 with the cross products taken against 2a: every limb of a at 2^29 - 1 (2a at 2^30 - 2)."""
    a = sqr_raw_operands()
    assert a.max() == M29
    wants = [limb_val(r) ** 2 for r in a]
    _check_montgomery_rows(be.sqr_raw(field, a), wants, mod)
