"""The wire-format kernels (csrc/h2mi_serde.hip), the 32-bit-limb Montgomery layer under them (csrc/fp.cuh) and the fingerprint of
the ad-hoc registration cache (adhoc_handle in csrc/h2mi_msm.hip), on the cases of tests/wire_cases.py: more than one workgroup with a
ragged tail, coordinates whose Montgomery words sit at the limb extremes, encodings that agree with the modulus in their high limbs,
whole wavefronts of invalid encodings, both moduli of the repr kernels, and base sets that differ in order or in their last bytes only.
Every comparison is exact, against oracle/formats.py and Python integers.  tests/test_wire_cases_host.py proves the cases."""
import ctypes as C
import io
import struct

import numpy as np
import pytest

from oracle import bn254 as o
from oracle import formats as fm

import wire_cases as K

pytestmark = pytest.mark.gpu

EINVAL = -1


def _rows(enc) -> np.ndarray:
    return np.frombuffer(b"".join(enc), dtype=np.uint8).reshape(-1, 32).copy()


@pytest.fixture(scope="module")
def packed():
    """POINTS as the device holds them, and their encodings by the oracle: computed once, read by every test, changed by none"""
    aff = o.pack_points(K.POINTS)
    enc = _rows([fm.g1_to_bytes(p) for p in K.POINTS])
    aff.setflags(write=False)
    enc.setflags(write=False)
    return aff, enc


# ---------------------------------------------------------------- 1. compress
def _compress_both(gpu, aff):
    from halo2_scaffold_amd import serde

    n = len(aff)
    host = np.full((n, 32), 0xA5, dtype=np.uint8)
    assert gpu.lib.h2mi_g1_compress(aff.ctypes.data, n, host.ctypes.data) == 0
    d_in, d_out = gpu.DevBuf.from_numpy(aff), gpu.DevBuf.from_numpy(np.full((n + 1, 32), 0xA5, dtype=np.uint8))
    assert gpu.lib.h2mi_g1_compress_dev(d_in.ptr, n, d_out.ptr, None) == 0
    assert gpu.lib.h2mi_sync() == 0
    dev = d_out.to_numpy(dtype=np.uint8, shape=(n + 1, 32))
    assert (dev[n] == 0xA5).all()  # nothing written past the n-th encoding
    assert np.array_equal(serde.g1_to_bytes_dev(d_in, n).to_numpy(dtype=np.uint8, shape=(n, 32)), dev[:n])
    d_in.free()
    d_out.free()
    return host, dev[:n]


def test_compress_host_and_dev_forms_match_the_oracle(gpu, packed):
    aff, enc = packed
    host, dev = _compress_both(gpu, aff)
    assert np.array_equal(host, dev)
    bad = np.flatnonzero((host != enc).any(axis=1))
    assert not len(bad), (bad[:8], [K.POINTS[i] for i in bad[:2]])
    for one in K.FIRST_POINTS:  # n = 1: the identity alone, a curve point alone
        host, dev = _compress_both(gpu, o.pack_points(one))
        assert host.tobytes() == dev.tobytes() == fm.g1_to_bytes(one[0])


# ---------------------------------------------------------------- 2. decompress
def _decompress_host(gpu, rows, out):
    cnt = C.c_uint64(1 << 40)
    assert gpu.lib.h2mi_g1_decompress(rows.ctypes.data, len(rows), out.ctypes.data, C.byref(cnt)) == 0
    return cnt.value


def _decompress_dev(gpu, rows, d_out):
    d_in, cnt = gpu.DevBuf.from_numpy(rows), C.c_uint64(1 << 40)
    assert gpu.lib.h2mi_g1_decompress_dev(d_in.ptr, len(rows), d_out.ptr, C.byref(cnt)) == 0
    d_in.free()
    return cnt.value, d_out.to_numpy(shape=(d_out.nbytes // 64, 8))


def test_decompress_valid_encodings_both_forms(gpu, packed):
    aff, enc = packed
    n = len(aff)
    out = np.full((n, 8), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    assert _decompress_host(gpu, enc, out) == 0 and np.array_equal(out, aff)
    d_out = gpu.DevBuf.from_numpy(np.full((n + 1, 8), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64))
    cnt, dev = _decompress_dev(gpu, enc, d_out)
    assert cnt == 0 and np.array_equal(dev[:n], aff) and (dev[n] == 0x5A5A5A5A5A5A5A5A).all()
    d_out.free()
    for one in K.FIRST_POINTS:
        one_out = np.ones((1, 8), dtype=np.uint64)
        assert _decompress_host(gpu, _rows([fm.g1_to_bytes(one[0])]), one_out) == 0 and np.array_equal(one_out, o.pack_points(one))


def test_decompress_mixed_vector_counts_and_zeroes_the_invalid_rows(gpu, packed):
    from halo2_scaffold_amd import serde

    aff, enc = packed
    n = len(aff)
    mixed = _rows(K.MIXED)
    bad = np.zeros(n, dtype=bool)
    bad[sorted(K.MIXED_BAD)] = True
    want = aff.copy()
    want[bad] = 0

    # host-pointer form: the output buffer holds the decoding of the valid vector first, so a row the kernel skipped would show; then the
    # same vector a second time into the same buffer: the counter is per call
    out = np.zeros((n, 8), dtype=np.uint64)
    assert _decompress_host(gpu, enc, out) == 0
    assert out[bad].any(axis=1).sum() == sum(K.POINTS[i] is not None for i in K.MIXED_BAD) >= len(K.MIXED_BAD) - 6  # (an identity is zero anyway)
    for _ in range(2):
        assert _decompress_host(gpu, mixed, out) == len(K.MIXED_BAD)
        assert not out[bad].any() and np.array_equal(out, want)
    d_out = gpu.DevBuf.from_numpy(aff)
    for _ in range(2):
        cnt, dev = _decompress_dev(gpu, mixed, d_out)
        assert cnt == len(K.MIXED_BAD) and not dev[bad].any() and np.array_equal(dev, want)
    with pytest.raises(serde.DecodeError):
        serde.g1_from_bytes(mixed)
    d_in = gpu.DevBuf.from_numpy(mixed)
    with pytest.raises(serde.DecodeError):
        serde.g1_from_bytes_dev(d_in, n, d_out)
    # every invalid encoding alone (n = 1), with its reason
    for b, why in K.BAD_G1:
        one = np.ones((1, 8), dtype=np.uint64)
        assert _decompress_host(gpu, _rows([b]), one) == 1 and not one.any(), why
    d_in.free()
    d_out.free()


# ---------------------------------------------------------------- 3. entry refusals
def test_serde_entries_refuse_empty_and_null_arguments(gpu, packed):
    aff, enc = packed
    lib, cnt = gpu.lib, C.c_uint64()
    out32, out64 = np.zeros((4, 32), dtype=np.uint8), np.zeros((4, 8), dtype=np.uint64)
    d_a, d_b = gpu.DevBuf(4 * 64), gpu.DevBuf(4 * 64)
    a, e, by = aff.ctypes.data, enc.ctypes.data, C.byref(cnt)
    refused = [
        lib.h2mi_g1_compress(a, 0, out32.ctypes.data), lib.h2mi_g1_compress(None, 4, out32.ctypes.data), lib.h2mi_g1_compress(a, 4, None),
        lib.h2mi_g1_compress_dev(d_a.ptr, 0, d_b.ptr, None), lib.h2mi_g1_compress_dev(None, 4, d_b.ptr, None), lib.h2mi_g1_compress_dev(d_a.ptr, 4, None, None),
        lib.h2mi_g1_decompress(e, 0, out64.ctypes.data, by), lib.h2mi_g1_decompress(None, 4, out64.ctypes.data, by),
        lib.h2mi_g1_decompress(e, 4, None, by), lib.h2mi_g1_decompress(e, 4, out64.ctypes.data, None),
        lib.h2mi_g1_decompress_dev(d_a.ptr, 0, d_b.ptr, by), lib.h2mi_g1_decompress_dev(None, 4, d_b.ptr, by),
        lib.h2mi_g1_decompress_dev(d_a.ptr, 4, None, by), lib.h2mi_g1_decompress_dev(d_a.ptr, 4, d_b.ptr, None),
    ]
    for field in (0, 1, 2):
        refused += [lib.h2mi_fe_to_repr_dev(field, d_a.ptr, 0, d_b.ptr, None), lib.h2mi_fe_to_repr_dev(field, None, 4, d_b.ptr, None),
                    lib.h2mi_fe_to_repr_dev(field, d_a.ptr, 4, None, None),
                    lib.h2mi_fe_from_repr_dev(field, d_a.ptr, 0, d_b.ptr, by), lib.h2mi_fe_from_repr_dev(field, None, 4, d_b.ptr, by),
                    lib.h2mi_fe_from_repr_dev(field, d_a.ptr, 4, None, by), lib.h2mi_fe_from_repr_dev(field, d_a.ptr, 4, d_b.ptr, None)]
    refused += [lib.h2mi_fe_to_repr_dev(2, d_a.ptr, 4, d_b.ptr, None), lib.h2mi_fe_from_repr_dev(2, d_a.ptr, 4, d_b.ptr, by),
                lib.h2mi_fe_to_repr_dev(-1, d_a.ptr, 4, d_b.ptr, None), lib.h2mi_fe_from_repr_dev(-1, d_a.ptr, 4, d_b.ptr, by)]
    assert refused == [EINVAL] * len(refused)
    assert not out32.any() and not out64.any()
    d_a.free()
    d_b.free()


# ---------------------------------------------------------------- 4. repr kernels, both moduli
@pytest.mark.parametrize("field,mod", K.FIELDS)
def test_repr_kernels_both_fields(gpu, field, mod):
    vals = K.REPR_VALUES[field]
    n = len(vals)
    mont = o.pack(vals, mod)
    d_in, d_rep, d_back = gpu.DevBuf.from_numpy(mont), gpu.DevBuf(n * 32), gpu.DevBuf(n * 32)
    assert gpu.lib.h2mi_fe_to_repr_dev(field, d_in.ptr, n, d_rep.ptr, None) == 0
    assert gpu.lib.h2mi_sync() == 0
    rep = d_rep.to_numpy(dtype=np.uint8, shape=(n, 32))
    assert [bytes(r) for r in rep] == [fm.fe_to_repr(v) for v in vals]
    cnt = C.c_uint64(1 << 40)
    assert gpu.lib.h2mi_fe_from_repr_dev(field, d_rep.ptr, n, d_back.ptr, C.byref(cnt)) == 0
    assert cnt.value == 0 and np.array_equal(d_back.to_numpy(shape=(n, 4)), mont)

    # valid neighbours of the modulus and strings not below it, interleaved through all three workgroups; d_back still holds the
    # (non-zero) decoding above, so a row the kernel did not write would show
    vec, bad_at = K.REPR_EDGE[field]
    assert len(vec) == n
    want = o.pack([0 if i in bad_at else v for i, v in enumerate(vec)], mod)
    d_edge = gpu.DevBuf.from_numpy(o.pack(vec))  # canonical integers as they lie: the 32 bytes
    for _ in range(2):  # the counter is per call
        assert gpu.lib.h2mi_fe_from_repr_dev(field, d_edge.ptr, n, d_back.ptr, C.byref(cnt)) == 0
        got = d_back.to_numpy(shape=(n, 4))
        wrong = np.flatnonzero((got != want).any(axis=1))
        assert not len(wrong), [(int(i), hex(vec[i]), i in bad_at) for i in wrong[:4]]
        assert cnt.value == len(bad_at)
    # each string alone: the bad ones count and decode to zero, the near ones decode and encode back to themselves
    for b in K.REPR_BAD[field] + K.REPR_NEAR[field]:
        v = int.from_bytes(b, "little")
        d_one = gpu.DevBuf.from_numpy(np.frombuffer(b, dtype=np.uint64))
        assert gpu.lib.h2mi_fe_from_repr_dev(field, d_one.ptr, 1, d_back.ptr, C.byref(cnt)) == 0
        one = d_back.to_numpy(shape=(1, 4), nbytes=32)
        assert (cnt.value, o.limbs_to_int(one[0])) == ((1, 0) if v >= mod else (0, K.word_of(v, mod))), hex(v)
        if v < mod:
            assert gpu.lib.h2mi_fe_to_repr_dev(field, d_back.ptr, 1, d_one.ptr, None) == 0 and gpu.lib.h2mi_sync() == 0
            assert d_one.to_numpy(dtype=np.uint8).tobytes() == b
        d_one.free()
    for d in (d_in, d_rep, d_back, d_edge):
        d.free()


# ---------------------------------------------------------------- 5. field operations on extreme words
@pytest.mark.parametrize("field,mod", K.FIELDS)
def test_field_ops_on_extreme_words(gpu, hooks, field, mod):
    def run(op, a_words, b_words=None):
        A = K.pack_words(a_words)
        B = K.pack_words(b_words) if b_words is not None else None
        out = np.full((len(A), 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        rc = hooks.h2mi_dbg_field_op(field, op, A.ctypes.data, B.ctypes.data if B is not None else None, out.ctypes.data, len(A))
        assert rc == 0, gpu.lib.h2mi_strerror(rc)
        got = o.unpack(out)
        assert all(w < mod for w in got), (op, [hex(w) for w in got if w >= mod][:3])  # fully reduced, whatever else
        return got

    def check(op, got, want_values, operands):
        want = [K.word_of(v, mod) for v in want_values]
        wrong = [i for i in range(len(want)) if got[i] != want[i]]
        assert not wrong, (op, len(wrong), [tuple(hex(w) for w in operands[i]) for i in wrong[:3]])

    pairs = K.FP_PAIRS[field]
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    va, vb = [K.value_of(w, mod) for w in a], [K.value_of(w, mod) for w in b]
    check("mul", run(0, a, b), [x * y % mod for x, y in zip(va, vb)], pairs)
    check("add", run(1, a, b), [(x + y) % mod for x, y in zip(va, vb)], pairs)
    check("sub", run(2, a, b), [(x - y) % mod for x, y in zip(va, vb)], pairs)
    words = K.FP_WORDS[field]
    vals = [K.value_of(w, mod) for w in words]
    ones = [(w,) for w in words]
    check("sqr", run(3, words), [x * x % mod for x in vals], ones)
    check("neg", run(7, words), [(-x) % mod for x in vals], ones)
    check("dbl", run(8, words), [2 * x % mod for x in vals], ones)
    inv = [pow(x, -1, mod) if x else 0 for x in vals]
    check("inv_ds", run(9, words), inv, ones)
    check("inv_gcd", run(10, words), inv, ones)
    # from_mont: word -> canonical limbs of its value; to_mont: the same words read as canonical values -> v * 2^256 mod p
    assert run(5, words) == vals
    assert run(6, words) == [K.word_of(w, mod) for w in words]


# ---------------------------------------------------------------- 6. SRS file
def _non_residue_x():
    return K.X_SMALL_SKIPPED[0].to_bytes(32, "little")


def _srs_round_trip(gpu, k, s, want):
    from halo2_scaffold_amd import serde

    n = 1 << k
    params = gpu.ParamsKZG.setup(k, s)
    buf = io.BytesIO()
    params.write(buf)
    raw = buf.getvalue()
    assert len(raw) == len(want) == 4 + 2 * n * 32 + 128
    diff = [i for i in range(2 * n) if raw[4 + 32 * i: 36 + 32 * i] != want[4 + 32 * i: 36 + 32 * i]]
    assert not diff and raw == want, diff[:8]
    again = gpu.ParamsKZG.read(io.BytesIO(raw))
    assert again.k == k and np.array_equal(again.get_g(), params.get_g()) and np.array_equal(again.get_g_lagrange(), params.get_g_lagrange())
    assert (again.g2_bytes, again.s_g2_bytes) == (params.g2_bytes, params.s_g2_bytes)
    params.release()
    again.release()
    return raw, serde


def test_srs_file_k8_matches_oracle_and_refuses_corruption(gpu):
    """k = 8: each point vector is one full workgroup.  The file's point 300 lies in g_lagrange (its entry 44)."""
    k, s = 8, 0x5EED0008
    raw, serde = _srs_round_trip(gpu, k, s, fm.srs_bytes(k, s))
    bad = bytearray(raw)
    bad[4 + 32 * 300: 4 + 32 * 301] = _non_residue_x()
    with pytest.raises(serde.DecodeError):
        gpu.ParamsKZG.read(io.BytesIO(bytes(bad)))
    with pytest.raises(serde.DecodeError):
        gpu.ParamsKZG.read(io.BytesIO(raw[:-1]))


def test_srs_file_k9_two_workgroups_per_vector(gpu):
    """k = 9: 512 points per vector, two workgroups for each kernel launch of write and read; entry 300 of g_lagrange is in the second.
    The points come from the C oracle (the Python one takes 10 s at this size), the bytes from oracle/formats.py."""
    from oracle import cref

    k, s = 9, 0x5EED0009
    pw, lag = o.srs_scalars(k, s)
    pts = o.unpack_points(cref.g1_mul_gen(o.pack(pw + lag, o.R), 2))
    assert pts[0] == o.G1_GEN and pts[1] == o.g1_mul(s, o.G1_GEN) and pts[512 + 300] == o.g1_mul(lag[300], o.G1_GEN)
    want = struct.pack("<I", k) + b"".join(fm.g1_to_bytes(p) for p in pts) + fm.g2_to_bytes(fm.G2_GEN) + fm.g2_to_bytes(fm.g2_mul(s))
    raw, serde = _srs_round_trip(gpu, k, s, want)
    bad = bytearray(raw)
    bad[4 + 32 * (512 + 300): 4 + 32 * (512 + 301)] = _non_residue_x()
    with pytest.raises(serde.DecodeError):
        gpu.ParamsKZG.read(io.BytesIO(bytes(bad)))
    with pytest.raises(serde.DecodeError):
        gpu.ParamsKZG.read(io.BytesIO(raw[:-1]))


# ---------------------------------------------------------------- 7. fingerprint of the ad-hoc registration cache
def test_adhoc_fingerprint_tells_reordered_and_last_word_changes_apart(gpu):
    from oracle import cref

    sets = K.base_sets()
    sc = o.random_field_limbs(K.N_BASES, 0xF1A6)
    builds = C.c_uint64()

    def nbuilds():
        assert gpu.lib.h2mi_msm_adhoc_builds(C.byref(builds)) == 0
        return builds.value

    def commit(name):
        assert o.unpack_jacobian(gpu.best_multiexp(sc, sets[name])) == o.unpack_jacobian(cref.msm(sc, sets[name], 2)), name
        return nbuilds()

    b0 = nbuilds()
    for i, name in enumerate(("base", "swapped", "neg_last", "cross_neg")):
        assert commit(name) == b0 + i + 1, name  # a set the cache has not seen: registered, not answered from a stale table
    assert commit("base") == b0 + 4  # the first set is still cached
    # a fifth set evicts the least recently used one ('swapped') and no other: the four that stay answer without a rebuild.  (The eviction
    # used to drop a second, live entry as well — found by this test when it ran after others had filled the cache.)
    assert commit("reversed") == b0 + 5
    for name in ("neg_last", "cross_neg", "base", "reversed"):
        assert commit(name) == b0 + 5, name
    assert commit("swapped") == b0 + 6
