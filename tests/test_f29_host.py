"""CPU tests of the lazy 29-bit-limb field / curve layer (csrc/f29.cuh, g1_29.cuh) compiled with g++.

The GPU kernels inline this code; verifying it on the host against the big-integer oracle covers limb bounds, the
Mont256 <-> Mont261 conversions and every special case of the mixed addition without needing a GPU.  The cases and checks live
in tests/f29_cases.py; tests/test_gpu_f29.py runs the same ones through the device build (whose f29_mac_first is inline asm)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import bn254 as o

import f29_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    return K.host_lib()


@pytest.fixture(scope="module")
def be(host):
    return K.HostBackend(host)


def test_generated_constants_are_current():
    gen = subprocess.check_output(["python", os.path.join(ROOT, "halo2-scaffold_amd", "csrc", "gen_f29_consts.py")], text=True)
    assert gen == open(os.path.join(ROOT, "halo2-scaffold_amd", "csrc", "f29_consts.inc")).read()


@pytest.mark.parametrize("field,mod", K.FIELDS)
def test_f29_mul_modes(be, field, mod):
    K.check_mul_modes(be, field, mod)


@pytest.mark.parametrize("field,mod", K.FIELDS)
def test_reduce_loose(be, field, mod):
    K.check_reduce_loose(be, field, mod)


def test_madd_chain_random_and_special_cases(be):
    K.check_madd_chain_random_and_special_cases(be)


def test_full_add_and_double_trees(be):
    K.check_full_add_and_double_trees(be)


def test_long_chain_keeps_invariants(be):
    K.check_long_chain_keeps_invariants(be)


def test_extreme_limb_patterns(be):
    K.check_extreme_limb_patterns(be)


def test_mul2_shared_reduction_at_the_contract_limits(be):
    K.check_mul2_at_the_contract_limits(be)


def test_mul3_shared_reduction_at_the_contract_limits(be):
    K.check_mul3_at_the_contract_limits(be)


@pytest.mark.parametrize("field,mod", K.FIELDS)
def test_mul_raw_at_the_contract_limit(be, field, mod):
    K.check_mul_raw_at_the_contract_limit(be, field, mod)


@pytest.mark.parametrize("field,mod", K.FIELDS)
def test_sqr_raw_at_the_contract_limit(be, field, mod):
    K.check_sqr_raw_at_the_contract_limit(be, field, mod)


def test_pair_affine_chain_matches_oracle(host):
    """the pair-affine accumulation (g1_29.cuh affine29_pair_add: pairs of points added in affine coordinates with shared inversions,
    their sums entering the XYZZ accumulator) against the oracle's group law: random points and signs, every sign combination, pairs
    that must be routed around the affine formula (P + P, P - P, an identity member), an odd count, and the lazy-value bounds of the
    accumulator exercised by long chains."""
    host.f29t_pair_chain.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    rng = np.random.default_rng(17)
    base = [o.g1_mul(int(rng.integers(1, 1 << 62)), o.G1_GEN) for _ in range(40)]

    def run(pts, signs):
        P = o.pack_points(pts)
        S = np.array(signs, dtype=np.uint8)
        out = np.zeros(16, dtype=np.uint64)
        host.f29t_pair_chain(P.ctypes.data, S.ctypes.data, len(pts), out.ctypes.data)
        want = None
        for p, s in zip(pts, signs):
            want = o.g1_add(want, o.g1_neg(p) if s else p)
        assert K.xyzz_to_affine(out) == want

    for n in (1, 2, 3, 4, 7, 40):
        for trial in range(4):
            pts = [base[int(rng.integers(0, 40))] for _ in range(n)]
            run(pts, [int(rng.integers(0, 2)) for _ in range(n)])
    a, b = base[0], base[1]
    for s1 in (0, 1):
        for s2 in (0, 1):
            run([a, b], [s1, s2])
            run([a, a], [s1, s2])          # doubling or cancellation: two singles
            run([None, b], [s1, s2])       # identity members
            run([a, None, None, b, a], [s1, s2, 0, 1, s2])
    run([a, o.g1_neg(a)], [0, 0])
    run([a, b, b, a, a, b], [0, 1, 0, 1, 1, 0])   # pair sums that cancel the accumulator
    pts = [base[i % 40] for i in range(600)]
    run(pts, [(i * 7 // 3) & 1 for i in range(600)])
