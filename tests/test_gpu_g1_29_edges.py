"""The G1 group law (csrc/g1_29.cuh, g1_29_quad.cuh) at the bounds of its coordinate invariants, as the DEVICE compiles it.

tests/test_g1_29_edges_host.py runs the cases of tests/g1_29_edge_cases.py on a g++ build of the header.  Here the same raw-limb
operands — coordinates at X < 6p, Y < 4p, ZZ / ZZZ < 1.1p / 1.5p, Z < 8p, extreme words, limbs all ones, the lazy y2 — go through
h2mi_dbg_g1_29_raw_op of libh2mi_hooks.so: the device form of f29_mac_first, another compiler, and for ops 6 / 7 the four-lane forms
with their DPP exchange.  Same value and closure checks as on the host, and the two builds must agree limb for limb.  Then the same
extreme points go through the product's kernels (MSM small path and general pipeline, ad-hoc MSM, group FFT, Jacobian sum / fold)."""
import ctypes as C
import functools

import numpy as np
import pytest

import f29_cases as K
import g1_29_edge_cases as E
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

Q = o.Q


@pytest.fixture(scope="module")
def dev(hooks):
    return K.DeviceBackend(hooks)


@pytest.fixture(scope="module")
def cpu():
    return K.HostBackend(K.host_lib())


@pytest.mark.parametrize("op", sorted(E.OPS))
def test_point_op_at_the_invariant_bounds(dev, cpu, op):
    """value and closure of every element on the device, and the g++ build's words limb for limb"""
    out = E.check_op(dev, op)
    A, B, _ = E.OPS[op]()
    assert np.array_equal(out, cpu.point_raw(op, A, B))


@pytest.mark.parametrize("op", sorted(E.QUAD_OF))
def test_quad_forms_at_the_invariant_bounds(dev, op):
    """op 6 xyzz29_add_quad, 7 xyzz29_dbl_quad on the cases of xyzz29_add / xyzz29_dbl, held to the same checks: the oracle's group
    element, ZZ^3 = ZZZ^2, the identity all zero, normalized limbs, the bounds g1_29.cuh derives for the one-lane forms.  (The
    doubling branch of the quad addition runs xyzz29_dbl_quad, an identity operand returns the other untouched.)"""
    E.check_op(dev, op)


@pytest.mark.parametrize("op", sorted(E.QUAD_OF))
def test_quad_forms_equal_the_one_lane_forms_limb_for_limb(dev, op):
    """ops 6 / 7 against ops 2 / 1 on all 36 words: the four lanes form every product from the operands the one-lane form gives it —
    Y3 included, through one shared reduction (f29_mul2) — so the two are the same integer functions and a difference is a finding
    (a lane's role, the DPP exchange, a reduction taken another way)."""
    A, B, _ = E.OPS[E.QUAD_OF[op]]()
    quad, one = dev.point_raw(op, A, B), dev.point_raw(E.QUAD_OF[op], A, B)
    differ = [k for k in range(len(quad)) if not np.array_equal(quad[k], one[k])]
    assert not differ, (op, len(differ), len(quad), differ[:8])


# ---- the same points through the product's kernels --------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _base_set():
    """64 bases: the extreme-coordinate points (P / -P pairs among them), the identity, a duplicate, random multiples of G"""
    pts = list(E.curve_points())
    pts += [None, pts[0], pts[5]]
    rng = np.random.default_rng(64)
    pts += [o.g1_mul(int.from_bytes(rng.bytes(31), "little") + 1, o.G1_GEN) for _ in range(64 - len(pts))]
    return pts


def _scalar_sets(n, seed):
    return [np.tile(o.pack([1], o.R)[0], (n, 1)), np.tile(o.pack([o.R - 1], o.R)[0], (n, 1)), o.random_field_limbs(n, seed)]


def test_msm_over_extreme_coordinate_bases(gpu):
    """a registered 64-point set of extreme-coordinate bases through the small path and the general pipeline, scalars 1, r - 1, random"""
    from test_gpu_parity import _both_msm_paths

    pts = list(_base_set())
    bases = o.pack_points(pts)
    h = C.c_uint64()
    assert gpu.lib.h2mi_bases_register(bases.ctypes.data, len(pts), C.byref(h)) == 0
    for sc in _scalar_sets(len(pts), 2929):
        _both_msm_paths(gpu, h.value, np.ascontiguousarray(sc), len(pts), o.msm_naive(o.unpack(sc, o.R), pts))
    assert gpu.lib.h2mi_bases_release(h.value) == 0


def test_ad_hoc_msm_over_extreme_coordinate_bases(gpu):
    """the same bases ad hoc through best_multiexp, padded with random points to 4096; the extreme part of the reference is the
    oracle's, the padding's the C restatement's"""
    from oracle import cref

    pts = list(_base_set())
    n = 4096
    pad = cref.g1_mul_gen(o.random_field_limbs(n - len(pts), 4096), 4)
    bases = np.concatenate([o.pack_points(pts), pad])
    for sc in _scalar_sets(n, 2930):
        want = o.g1_add(o.msm_naive(o.unpack(sc[: len(pts)], o.R), pts), o.unpack_jacobian(cref.msm(sc[len(pts) :], pad, 2)))
        assert o.unpack_jacobian(gpu.best_multiexp(sc, bases)) == want


@pytest.mark.parametrize("log_n", [3, 5])
def test_group_fft_over_extreme_coordinate_points(gpu, log_n):
    """h2mi_fft_bn254_g1_dev over the extreme points (the identity, a duplicate and P / -P neighbours among them) against the naive
    group DFT out_i = sum_j w^(i j) P_j; then the inverse with the n^-1 scale, in place, back to the input"""
    from halo2_scaffold_amd import field as F
    from halo2_scaffold_amd.device import DevBuf

    n = 1 << log_n
    src = list(_base_set())
    pts = [src[0], src[1], None, src[0]] + src[2 : n - 2]  # P, -P, the identity, P again, then the rest
    assert len(pts) == n
    w = o.omega_for(log_n)
    want = [o.msm_naive([pow(w, i * j, o.R) for j in range(n)], pts) for i in range(n)]
    packed = o.pack_points(pts)
    d_in, d_out = DevBuf.from_numpy(packed), DevBuf(n * 64)
    wl = F.fr_to_mont_limbs(w)
    assert gpu.lib.h2mi_fft_bn254_g1_dev(d_in.ptr, d_out.ptr, log_n, wl.ctypes.data, None, None) == 0
    assert o.unpack_points(d_out.to_numpy(shape=(n, 8))) == want
    wil, nil = F.fr_to_mont_limbs(F.fr_inv(w)), F.fr_to_mont_limbs(F.fr_inv(n))
    assert gpu.lib.h2mi_fft_bn254_g1_dev(d_out.ptr, d_out.ptr, log_n, wil.ctypes.data, nil.ctypes.data, None) == 0
    assert np.array_equal(d_out.to_numpy(shape=(n, 8)), packed)
    d_in.free()
    d_out.free()


def test_jacobian_sum_and_fold_with_extreme_z_words(gpu):
    """h2mi_g1_sum_jacobian and h2mi_g1_fold_groups on Jacobian inputs (x z^2, y z^3, z) whose Z is an extreme word — as the ABI's
    canonical Mont256 word, and as the Mont261 word the kernels compute on — over the extreme points, the identity (Z = 0), the
    same point as two representatives and a point next to its negative"""
    lib = gpu.lib
    src = E.curve_points()
    zs = [W * pow(1 << bits, -1, Q) % Q for bits in (256, 261) for W in E.WORDS + E.SMALL_WORDS]
    pts = [src[i % len(src)] for i in range(len(zs))] + [None, src[0], src[0], src[1]]
    zs += [1, zs[0], zs[1], zs[2]]
    n = len(pts)

    def reps(points, shift):
        return np.stack([o.pack_jacobian(p, z=zs[(i + shift) % n]) for i, p in enumerate(points)])

    def total(points):
        acc = None
        for p in points:
            acc = o.g1_add(acc, p)
        return acc

    jac = reps(pts, 0)
    assert [o.limbs_to_int(jac[i, 8:12]) for i in range(len(E.WORDS))] == E.WORDS
    out = np.zeros(12, dtype=np.uint64)
    for lo, hi in ((0, n), (0, 1), (n - 4, n), (n - 3, n - 1)):  # all; one; identity, P, P, -P; P, P
        part = np.ascontiguousarray(jac[lo:hi])
        assert lib.h2mi_g1_sum_jacobian(part.ctypes.data, hi - lo, out.ctypes.data) == 0
        assert o.unpack_jacobian(out) == total(pts[lo:hi]), (lo, hi)
    # fold: rank 1 holds the same points as other representatives (every column doubles), rank 2 their negatives (every column
    # cancels), rank 3 other points
    others = pts[3:] + pts[:3]
    ranks = [(pts, 0), (pts, 1), ([o.g1_neg(p) for p in pts], 2), (others, 5)]
    groups = np.stack([reps(points, shift) for points, shift in ranks])
    for world in (2, 3, 4):
        got = np.zeros((n, 12), dtype=np.uint64)
        assert lib.h2mi_g1_fold_groups(np.ascontiguousarray(groups[:world]).ctypes.data, world, n, got.ctypes.data) == 0
        assert [o.unpack_jacobian(g) for g in got] == [total([r[0][j] for r in ranks[:world]]) for j in range(n)], world
