"""The lazy 29-bit-limb layer (csrc/f29.cuh, g1_29.cuh) as the DEVICE compiles it, at the limits of its contracts.

tests/test_f29_host.py drives f29_mul / sqr / mul2 / mul3 / reduce_loose / inv and the xyzz29 chains at their extreme limb patterns on
a g++ build of the headers.  The device code is a different path: f29_mac_first is v_mad_u64_u32 inline asm there, and everything else
comes out of another compiler.  The kernels that inline this layer (MSM, NTT, polynomial helpers) only ever feed it random field
elements, whose limbs are uniform and nowhere near a bound.  Here the same cases (tests/f29_cases.py) run through the
h2mi_dbg_f29_* hooks of libh2mi_hooks.so: one thread per element, operands read from global memory, the same per-element bodies the
host harness compiles (csrc/f29_testops.cuh).

Every comparison is exact (Python integers).  On the raw-limb operations host and device outputs are also required to be equal limb
for limb: they are deterministic integer functions of one header, so a difference is a finding.  A change that makes the device form
differ on purpose (another reduction, another output range) edits that assert and says why."""
import numpy as np
import pytest

import f29_cases as K
from oracle import bn254 as o

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hooks):
    return K.DeviceBackend(hooks)


@pytest.fixture(scope="module")
def cpu():
    return K.HostBackend(K.host_lib())  # the g++ build of the same headers


@pytest.mark.parametrize("field,mod", K.FIELDS)
def test_f29_mul_modes(dev, field, mod):
    K.check_mul_modes(dev, field, mod)


@pytest.mark.parametrize("field,mod", K.FIELDS)
def test_reduce_loose(dev, field, mod):
    K.check_reduce_loose(dev, field, mod)


def test_extreme_limb_patterns(dev):
    K.check_extreme_limb_patterns(dev)


def test_mul2_shared_reduction_at_the_contract_limits(dev):
    K.check_mul2_at_the_contract_limits(dev)


def test_mul3_shared_reduction_at_the_contract_limits(dev):
    K.check_mul3_at_the_contract_limits(dev)


@pytest.mark.parametrize("field,mod", K.FIELDS)
def test_mul_raw_at_the_contract_limit(dev, field, mod):
    K.check_mul_raw_at_the_contract_limit(dev, field, mod)


@pytest.mark.parametrize("field,mod", K.FIELDS)
def test_sqr_raw_at_the_contract_limit(dev, field, mod):
    K.check_sqr_raw_at_the_contract_limit(dev, field, mod)


def test_madd_chain_random_and_special_cases(dev):
    K.check_madd_chain_random_and_special_cases(dev)


def test_full_add_and_double_trees(dev):
    K.check_full_add_and_double_trees(dev)


def test_long_chain_keeps_invariants(dev):
    K.check_long_chain_keeps_invariants(dev)


@pytest.mark.parametrize("field,mod", K.FIELDS)
def test_device_equals_host_limb_for_limb(dev, cpu, field, mod):
    """the raw-limb operations and every f29t_mul mode: the two builds of one header give the same words"""
    _, limbs = K.reduce_loose_values(field, mod)
    assert np.array_equal(dev.reduce_loose(field, limbs), cpu.reduce_loose(field, limbs))
    m = K.mul_raw_operands()
    assert np.array_equal(dev.mul_raw(field, m["a"], m["b"]), cpu.mul_raw(field, m["a"], m["b"]))
    s = K.sqr_raw_operands()
    assert np.array_equal(dev.sqr_raw(field, s), cpu.sqr_raw(field, s))
    m2 = K.mul2_operands()
    assert np.array_equal(dev.mul2_raw(field, *(m2[k] for k in "abcd")), cpu.mul2_raw(field, *(m2[k] for k in "abcd")))
    m3 = K.mul3_operands()
    assert np.array_equal(dev.mul3_raw(field, m3), cpu.mul3_raw(field, m3))
    va, vb = K.mul_mode_values(field, mod)
    ext = K.extreme_values(mod)
    A = o.pack(va + [a for a in ext for _ in ext], mod)
    B = o.pack(vb + [b for _ in ext for b in ext], mod)
    for mode in (0, 1, 2, 4, 3):
        assert np.array_equal(dev.mul(field, mode, A, B), cpu.mul(field, mode, A, B)), mode
    assert np.array_equal(dev.mul(field, 5, A, B, 64), cpu.mul(field, 5, A, B, 64))


def test_device_chains_equal_host_word_for_word(dev, cpu):
    """the XYZZ outputs of the chains (a representative, not just the point): same words from both builds"""
    cases = K.madd_chain_cases()
    assert np.array_equal(dev.chains(cases, 0), cpu.chains(cases, 0))
    for tree, cs in K.tree_cases().items():
        assert np.array_equal(dev.chains(cs, tree), cpu.chains(cs, tree)), tree
