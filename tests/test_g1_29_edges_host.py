"""The G1 group law (csrc/g1_29.cuh) at the bounds of its coordinate invariants, on the g++ build of the header.

Every other point-level test feeds the formulas canonical affine points, whose accumulators sit well inside X < 6p, Y < 4p, ZZ and
ZZZ < 1.1p / 1.5p, Z < 8p.  These bounds are contracts between kernels (accumulators travel through memory as loosely reduced
limbs), and the biased subtractions, the lazy operands and the equality tests of the formulas are only right inside them.  Here
every operation takes raw-limb operands placed AT the bounds (tests/g1_29_edge_cases.py) and every result is checked for its value
against the oracle's group law and for closure: normalized limbs below the bound the header derives, which is what makes the
invariant inductive.  tests/test_gpu_g1_29_edges.py runs the same cases on the device."""
import os
import subprocess

import numpy as np
import pytest

import f29_cases as K
import g1_29_edge_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def be():
    return K.HostBackend(K.host_lib())


def test_cases_sit_at_the_documented_bounds():
    """the builders deliver what they promise: operands inside the contract and within 2^232 + p of its edge, extreme words exact"""
    Q = E.Q
    A, B, want = E.madd_cases()
    coords = [[E.limb_val(r[9 * i : 9 * i + 9]) for r in A] for i in range(4)]
    assert max(coords[0]) < E.X_LIMIT and max(coords[1]) < E.Y_LIMIT and max(coords[2]) < E.ZZ_MADD and max(coords[3]) < E.ZZ_MADD
    assert max(coords[0]) >= E.X_LIMIT - Q and max(coords[1]) >= E.Y_LIMIT - Q
    assert max(coords[2]) >= E.ZZ_MADD - E.MARGIN and E.X_LIMIT - max(coords[0]) <= E.MARGIN  # the all-ones words just under the bound
    assert (A.reshape(-1, 4, 9)[:, :, :8] <= E.M29).all() and (B[:, :8] <= E.M29).all() and B[:, 9:18].max() > E.M29  # y2 lazy among them
    words = {v % Q for v in coords[2]}
    for W in E.WORDS:  # ZZ's word is the extreme one, or the nearest to it (a few steps away) that is a square
        assert any(W + d in words for d in range(-64, 65)), hex(W)
    assert any((w & E.ONES232) == E.ONES232 for w in words)  # limbs 0..7 all ones
    A2, B2, _ = E.add_cases()
    for M in (A2, B2):
        zz = [E.limb_val(r[18:27]) for r in M]
        assert max(zz) < E.ZZ_ADD and max(zz) >= E.ZZ_ADD - E.MARGIN and (M.reshape(-1, 4, 9)[:, :, :8] <= E.M29).all()
    J, _, _ = E.jacobian_cases()
    z = [E.limb_val(r[18:27]) for r in J]
    assert max(z) < E.Z_LIMIT and E.Z_LIMIT - max(z) <= E.MARGIN
    assert {c for _, c in want} == {"madd", "dbl_affine", "madd_first", None}


@pytest.mark.parametrize("op", sorted(E.OPS))
def test_point_op_at_the_invariant_bounds(be, op):
    """op 0 xyzz29_madd, 1 xyzz29_dbl, 2 xyzz29_add, 3 xyzz29_dbl_affine, 4 xyzz29_from_jacobian / xyzz29_to_jacobian, 5 xyzz29_to_affine"""
    E.check_op(be, op)


def test_point_ops_clean_under_sanitizers(be, tmp_path):
    """the same cases through a stand-alone AddressSanitizer + UndefinedBehaviorSanitizer build of the harness
    (tests/host/g1_29_edges_main.cpp): no report, and the same words as the plain build"""
    exe, cases, results = tmp_path / "g1_29_edges_main", tmp_path / "cases.bin", tmp_path / "results.bin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), os.path.join(ROOT, "tests", "host", "g1_29_edges_main.cpp")])
    want = []
    with open(cases, "wb") as f:
        for op in sorted(E.OPS):
            A, B, _ = E.OPS[op]()
            f.write(np.array([op, len(A)], dtype=np.uint32).tobytes() + A.tobytes() + B.tobytes())
            want.append(be.point_raw(op, A, B))
    r = subprocess.run([str(exe), str(cases), str(results)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-500:], r.stderr[-2000:])
    assert np.array_equal(np.fromfile(results, dtype=np.uint32).reshape(-1, 36), np.concatenate(want))
