"""The NTT against the C oracle (oracle/cref.py), every output, at every plan the library picks — and at the limb extremes.

choose_split / get_plan / ntt_dev configure the transform differently at almost every size: one pass up to 2^10, two passes
(ceil(k/2), floor(k/2)) for 2^11..2^20 (from 2^14 every pass in the compile-time <1024, m> kernel form), three passes from 2^21
((8,8,5), (8,8,6), (8,8,7), (8,8,8), (9,8,8)), fused first / last rounds from 2^18, a full twiddle table up to 2^22, a two-level
table with tile-ordered twiddle matrices at 2^23 and 2^24, no twiddle matrices from 2^25.  tests/test_gpu_parity.py compares full
outputs with an oracle up to 2^13 and checks properties (sampled outputs, sums, round trips) above; a forward / inverse pair wrong
in mutually inverse ways passes a round trip.  Here:
  1. every log_n in 14..25, fixed seed: best_fft in place == cref.ntt on the same Montgomery limbs, all n rows.  (2^26, 2^27: 2 to
     4 GiB per vector and tens of seconds of oracle time; their splits (9,9,8), (9,9,9) use the kernel forms of 2^17, 2^18, 2^25.)
  2. at the plan boundaries the options: inverse with the fused n^-1 post-scale, coset pre-scale by FR_ZETA, both together, and
     the zero-extending out-of-place entry with a source length that is neither a power of two nor a multiple of the 1024-element
     tile — each against the oracle's transform of the explicitly scaled / padded vector.
  3. limb extremes: the data of a transform are raw Mont256 words, unpacked into 29-bit limbs and fed to the butterflies'
     lazy a = x +- t chains without normalisation; uniformly random inputs never put a limb near a bound.  The words are chosen
     per element among r - 1, the largest word below r whose limbs 0..7 are all 2^29 - 1, 2^232 - 1, 0, 1, r >> 1.
All comparisons are exact (np.array_equal on the words)."""
import numpy as np
import pytest

from extreme_cases import EXTREME_WORDS  # raw Mont256 words (not values): all below r
from oracle import bn254 as o, cref

pytestmark = pytest.mark.gpu

THREADS = 16  # of the C oracle's transform
FULL_SIZES = list(range(14, 26))
OPTION_SIZES = [14, 17, 18, 19, 20, 21, 23]
EXTREME_SIZES = [4, 7, 9, 10, 13, 16, 19, 20, 21]


def _mont(v):
    return o.pack([v % o.R], o.R)[0]


def _roots(log_n):
    w = o.omega_for(log_n)
    return _mont(w), _mont(pow(w, -1, o.R)), _mont(pow(1 << log_n, -1, o.R))


def _same(got, ref, what):
    if not np.array_equal(got, ref):
        bad = np.flatnonzero((got != ref).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} of {len(ref)} rows differ from the oracle, first at row {bad[0]}")


def _oracle(a, omega, log_n, post=None):
    """cref.ntt of a copy of a, then (post) every output times the Montgomery word `post`"""
    ref = a.copy()
    cref.ntt(ref, omega, log_n, THREADS)
    if post is not None:
        ref = cref.field_op(1, 0, ref, np.tile(post, (len(ref), 1)))
    return ref


def _powers(base, n):
    """(base^i) for i < n as Montgomery words, by repeated doubling: pw[m : 2m] = pw[: m] * base^m"""
    pw = np.zeros((n, 4), dtype=np.uint64)
    pw[0] = _mont(1)
    m = 1
    while m < n:
        pw[m : 2 * m] = cref.field_op(1, 0, pw[:m], np.tile(_mont(pow(base, m, o.R)), (m, 1)))
        m *= 2
    return pw


def _ext(gpu, a, log_n, omega, pre, post):
    x = a.copy()
    rc = gpu.lib.h2mi_ntt_ext_bn254_fr(x.ctypes.data, log_n, omega.ctypes.data, pre.ctypes.data if pre is not None else None,
                                       post.ctypes.data if post is not None else None)
    assert rc == 0, gpu.lib.h2mi_strerror(rc)
    return x


@pytest.mark.parametrize("log_n", FULL_SIZES)
def test_forward_matches_c_oracle_on_every_row(gpu, log_n):
    n = 1 << log_n
    wl, _, _ = _roots(log_n)
    x = o.random_field_limbs(n, o.SEED + 100 + log_n)
    ref = _oracle(x, wl, log_n)
    gpu.best_fft(x, wl, log_n)
    _same(x, ref, f"best_fft 2^{log_n}")


@pytest.mark.parametrize("log_n", OPTION_SIZES)
def test_options_match_c_oracle(gpu, log_n):
    n = 1 << log_n
    wl, wil, ninv = _roots(log_n)
    zeta = _mont(o.FR_ZETA)
    a = o.random_field_limbs(n, o.SEED + 200 + log_n)
    _same(_ext(gpu, a, log_n, wil, None, ninv), _oracle(a, wil, log_n, post=ninv), f"inverse with n^-1, 2^{log_n}")
    scaled = cref.field_op(1, 0, a, _powers(o.FR_ZETA, n))
    _same(_ext(gpu, a, log_n, wl, zeta, None), _oracle(scaled, wl, log_n), f"coset pre-scale, 2^{log_n}")
    _same(_ext(gpu, a, log_n, wil, zeta, ninv), _oracle(scaled, wil, log_n, post=ninv), f"pre- and post-scale, 2^{log_n}")
    # zero-extended out of place: source length neither a power of two nor a multiple of the 1024-element tile
    src_len = n // 4 + 3
    padded = np.zeros((n, 4), dtype=np.uint64)
    padded[:src_len] = a[:src_len]
    d_src, d_dst = gpu.DevBuf.from_numpy(np.ascontiguousarray(a[:src_len])), gpu.DevBuf(n * 32)
    try:
        rc = gpu.lib.h2mi_ntt_bn254_fr_oop_dev(d_src.ptr, src_len, d_dst.ptr, log_n, wl.ctypes.data, None, None, None)
        assert rc == 0, gpu.lib.h2mi_strerror(rc)
        _same(d_dst.to_numpy(shape=(n, 4)), _oracle(padded, wl, log_n), f"out of place from {src_len} rows, 2^{log_n}")
        assert np.array_equal(d_src.to_numpy(shape=(src_len, 4)), a[:src_len])
    finally:
        d_src.free()
        d_dst.free()


def _extreme_vectors(n, seed):
    words = o.pack(EXTREME_WORDS)  # raw words: no Montgomery encoding
    assert all(v < o.R for v in EXTREME_WORDS)
    pick = np.random.default_rng(seed).integers(0, len(EXTREME_WORDS), size=n)
    alt = np.zeros((n, 4), dtype=np.uint64)
    alt[0::2] = words[0]
    return {"random choice": np.ascontiguousarray(words[pick]), "all r - 1": np.tile(words[0], (n, 1)), "r - 1 / 0 alternating": alt}


@pytest.mark.parametrize("log_n", EXTREME_SIZES)
def test_limb_extremes_match_c_oracle(gpu, log_n):
    """every DFT length 2^4 .. 2^10, both kernel forms, fused and unfused rounds, three passes: forward and inverse with n^-1"""
    n = 1 << log_n
    wl, wil, ninv = _roots(log_n)
    for name, a in _extreme_vectors(n, 300 + log_n).items():
        x = a.copy()
        gpu.best_fft(x, wl, log_n)
        _same(x, _oracle(a, wl, log_n), f"{name}, forward 2^{log_n}")
        _same(_ext(gpu, a, log_n, wil, None, ninv), _oracle(a, wil, log_n, post=ninv), f"{name}, inverse with n^-1, 2^{log_n}")
