"""Quotient step of create_proof for the reference's StandardPlonk circuit, on the device.

Mirror of halo2_proofs plonk/evaluation.rs `evaluate_h` followed by `divide_by_vanishing_poly`, specialised
to the constraint system of reference src/circuits/standard_plonk.rs:29-48 (one degree-3 gate, equality on
a, b, c => three permutation sets of one column).  Inputs are extended-domain DevBufs; the per-domain
scalars (coset generator, DELTA, the few inverses of X^n - 1 on the coset) are computed on the host as
EvaluationDomain::new / keygen do.
"""
import ctypes as C

import numpy as np

from . import field as F
from ._lib import check, lib
from ._lib import check as _check
from .device import DevBuf
from .domain import EvaluationDomain

FR_DELTA = pow(F.FR_MULTIPLICATIVE_GENERATOR, 1 << F.FR_S, F.FR_MODULUS)  # halo2curves Fr::DELTA
BLINDING_FACTORS = 5  # ConstraintSystem::blinding_factors() for this circuit


class _Cosets(C.Structure):
    _fields_ = [("advice", C.c_void_p * 3), ("fixed", C.c_void_p * 5), ("sigma", C.c_void_p * 3), ("z", C.c_void_p * 3),
                ("l0", C.c_void_p), ("l_last", C.c_void_p), ("l_active", C.c_void_p)]


def vanishing_inverses(domain: EvaluationDomain) -> np.ndarray:
    """(X^n - 1)^-1 on the extended coset: 2^(extended_k - k) distinct values."""
    r = F.FR_MODULUS
    rot = 1 << (domain.extended_k - domain.k)
    vals = []
    for i in range(rot):
        X = domain.g_coset * pow(domain.extended_omega, i, r) % r
        vals.append(F.fr_inv((pow(X, domain.n, r) - 1) % r))
    return np.stack([F.fr_to_mont_limbs(v) for v in vals])


def evaluate_h(domain: EvaluationDomain, advice, fixed, sigma, z, l0: DevBuf, l_last: DevBuf, l_active: DevBuf, beta: int, gamma: int, y: int,
               out: DevBuf, stream=None) -> None:
    """h(X) on the extended coset (already divided by X^n - 1) into `out`; all operands are DevBufs of
    extended_len() elements."""
    assert len(advice) == 3 and len(fixed) == 5 and len(sigma) == 3 and len(z) == 3
    cs = _Cosets()
    for i in range(3):
        cs.advice[i], cs.sigma[i], cs.z[i] = advice[i].ptr, sigma[i].ptr, z[i].ptr
    for i in range(5):
        cs.fixed[i] = fixed[i].ptr
    cs.l0, cs.l_last, cs.l_active = l0.ptr, l_last.ptr, l_active.ptr
    qs = quotient_scalars(domain, beta, gamma, y)
    check(lib.h2mi_plonk_evaluate_h_standard_dev(C.byref(cs), C.byref(qs), out.ptr, stream), "evaluate_h")


def permutation_product(k: int, values, sigmas, column_indices, beta: int, gamma: int, usable_rows: int, d_z: DevBuf,
                        d_start: DevBuf = None, d_last: DevBuf = None) -> None:
    """One chunk of the permutation argument's grand product on the device (plonk/permutation/prover.rs): fills
    d_z[0 .. usable_rows] from the chunk's columns (`values`, Lagrange basis) and their permutation columns
    (`sigmas`); `column_indices[j]` is column j's position in the argument (its identity image is
    delta^index * omega^row).  The blinding rows of d_z are left as the caller set them."""
    m = len(values)
    assert m == len(sigmas) == len(column_indices) and 1 <= m <= 64
    r = F.FR_MODULUS
    vp = (C.c_void_p * m)(*[b.ptr for b in values])
    sp = (C.c_void_p * m)(*[b.ptr for b in sigmas])
    bd = np.ascontiguousarray(np.stack([F.fr_to_mont_limbs(beta * pow(FR_DELTA, int(c), r) % r) for c in column_indices]))
    b_, g_ = F.fr_to_mont_limbs(beta), F.fr_to_mont_limbs(gamma)
    w = F.fr_to_mont_limbs(F.omega_for(k))
    check(lib.h2mi_plonk_permutation_product_dev(vp, sp, m, k, usable_rows, b_.ctypes.data, g_.ctypes.data, bd.ctypes.data, w.ctypes.data,
                                                 d_start.ptr if d_start is not None else None, d_z.ptr,
                                                 d_last.ptr if d_last is not None else None, None), "permutation_product")


class ActiveRows:
    """keygen-time support of the copy constraints for h2mi_plonk_permutation_products_sparse_dev: the sorted positions
    set * usable_rows + row at which some column of the set is moved by the permutation (`mapping`: the non-identity
    entries of permutation/keygen.rs `Assembly`, keyed (column index in the argument, row)).  Rows the permutation leaves
    alone contribute num / den = 1 exactly, so the grand products only change at these positions."""

    def __init__(self, mapping, chunk_len: int, usable_rows: int):
        pos = sorted({(col // chunk_len) * usable_rows + row for (col, row), target in mapping.items() if target != (col, row) and row < usable_rows})
        self.count = len(pos)
        self.buf = DevBuf.from_numpy(np.array(pos if pos else [0], dtype=np.uint32))

    def free(self):
        self.buf.free()


def permutation_products(k: int, values, sigmas, chunk_len: int, beta: int, gamma: int, usable_rows: int, d_zs, active: ActiveRows = None) -> None:
    """Every set of the permutation argument in one device pass (plonk/permutation/prover.rs `Argument::commit`):
    `values` / `sigmas` are the equality-enabled columns in argument order, chunked by `chunk_len` = cs.degree() - 2;
    d_zs[s] receives rows 0 .. usable_rows of set s, chained through the previous set's last value.  With `active`
    (ActiveRows from keygen) the products are computed over the constrained positions only — same values."""
    m = len(values)
    sets = -(-m // chunk_len)
    assert m == len(sigmas) and 1 <= m <= 64 and len(d_zs) == sets
    r = F.FR_MODULUS
    vp = (C.c_void_p * m)(*[b.ptr for b in values])
    sp = (C.c_void_p * m)(*[b.ptr for b in sigmas])
    zp = (C.c_void_p * sets)(*[b.ptr for b in d_zs])
    bd = np.ascontiguousarray(np.stack([F.fr_to_mont_limbs(beta * pow(FR_DELTA, j, r) % r) for j in range(m)]))
    b_, g_ = F.fr_to_mont_limbs(beta), F.fr_to_mont_limbs(gamma)
    w = F.fr_to_mont_limbs(F.omega_for(k))
    if active is not None and active.count * 8 <= sets * usable_rows:  # dense supports gain nothing from the indirection
        check(lib.h2mi_plonk_permutation_products_sparse_dev(vp, sp, m, chunk_len, k, usable_rows, b_.ctypes.data, g_.ctypes.data, bd.ctypes.data,
                                                             w.ctypes.data, active.buf.ptr, active.count, zp, None), "permutation_products_sparse")
        return
    check(lib.h2mi_plonk_permutation_products_dev(vp, sp, m, chunk_len, k, usable_rows, b_.ctypes.data, g_.ctypes.data, bd.ctypes.data, w.ctypes.data,
                                                  zp, None), "permutation_products")


# ---- lookup argument, single-expression lookups (the range check of the reference's RangeWithInstanceCircuitBuilder,
# src/scaffold.rs:434-485 with LOOKUP_BITS, :44-48) -----------------------------------------------------------------------
class LookupTable:
    """keygen-time description of a fixed lookup table column for the device's counting sort: the distinct values of
    its usable rows in ascending (canonical integer) order, their multiplicities, uploaded once."""

    def __init__(self, table_values, usable_rows: int):
        """table_values: the fixed column as integers (as the circuit assigns them), at least usable_rows of them"""
        counts = {}
        for v in table_values[:usable_rows]:
            v %= F.FR_MODULUS
            counts[v] = counts.get(v, 0) + 1
        vals = sorted(counts)
        self.n_unique = len(vals)
        self.usable_rows = usable_rows
        can = np.zeros((self.n_unique, 4), dtype=np.uint64)
        mont = np.zeros((self.n_unique, 4), dtype=np.uint64)
        for i, v in enumerate(vals):
            can[i] = [(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]
            mont[i] = F.fr_to_mont_limbs(v)
        self.sorted_canonical = DevBuf.from_numpy(can)
        self.sorted_mont = DevBuf.from_numpy(mont)
        self.mult = DevBuf.from_numpy(np.array([counts[v] for v in vals], dtype=np.uint32))

    def free(self):
        for b in (self.sorted_canonical, self.sorted_mont, self.mult):
            b.free()


def lookup_permute(k: int, d_input: DevBuf, table: LookupTable, d_permuted_input: DevBuf, d_permuted_table: DevBuf) -> int:
    """lookup/prover.rs permute_expression_pair on the device; rows beyond usable_rows are left to the caller (blinding).
    Returns the number of inputs that are not table values (the crate raises ConstraintSystemFailure when non-zero)."""
    missing = C.c_uint64()
    _check(lib.h2mi_plonk_lookup_permute_dev(d_input.ptr, table.sorted_canonical.ptr, table.sorted_mont.ptr, table.mult.ptr, table.n_unique, k,
                                             table.usable_rows, d_permuted_input.ptr, d_permuted_table.ptr, C.byref(missing), None),
           "lookup_permute")
    return missing.value


def lookup_product(k: int, d_input: DevBuf, d_table: DevBuf, d_permuted_input: DevBuf, d_permuted_table: DevBuf, beta: int, gamma: int,
                   usable_rows: int, d_z: DevBuf) -> None:
    b_, g_ = F.fr_to_mont_limbs(beta), F.fr_to_mont_limbs(gamma)
    _check(lib.h2mi_plonk_lookup_product_dev(d_input.ptr, d_table.ptr, d_permuted_input.ptr, d_permuted_table.ptr, k, usable_rows, b_.ctypes.data,
                                             g_.ctypes.data, d_z.ptr, None), "lookup_product")


def shuffle_product(k: int, d_input: DevBuf, d_shuffle: DevBuf, gamma: int, usable_rows: int, d_z: DevBuf) -> bool:
    """h2mi_plonk_shuffle_product_dev: z[0] = 1, z[i+1] = z[i] (A_i + gamma) / (S_i + gamma) on rows 0 .. usable_rows of d_z over the
    compressed rows of the two sides -> True when z[usable_rows] is one (the sides are the same multiset), False for H2MI_EUNSAT; z is
    written either way"""
    rc = lib.h2mi_plonk_shuffle_product_dev(d_input.ptr, d_shuffle.ptr, k, usable_rows, F.fr_to_mont_limbs(gamma).ctypes.data, d_z.ptr, None)
    if rc == -7:  # H2MI_EUNSAT
        return False
    _check(rc, "shuffle_product")
    return True


# ---- logUp, the logarithmic-derivative lookup argument [Haboeck; the `mv-lookup` feature of halo2_proofs forks — restated from memory,
# pinned to DESIGN.md 4.5 and tests/logup_cases.py].  Transcript: [M] per lookup behind theta, [phi] per lookup in the lookup product's
# slot behind beta and gamma; evaluations per lookup phi(x), phi(omega x), M(x); lookups.open the same three. -----------------------------
def logup_multiplicity(k: int, d_input: DevBuf, d_table: DevBuf, usable_rows: int, d_m: DevBuf) -> int:
    """h2mi_plonk_logup_multiplicity_dev: d_m[r] = #{i < usable_rows: input[i] = table[r]} on the first usable row r that holds its
    table value, zero on the other usable rows (Montgomery); the blinding rows are left to the caller.  Returns the number of inputs
    that are not table values (the lookup is unsatisfied when non-zero)."""
    missing = C.c_uint64()
    _check(lib.h2mi_plonk_logup_multiplicity_dev(d_input.ptr, d_table.ptr, k, usable_rows, d_m.ptr, C.byref(missing), None), "logup_multiplicity")
    return missing.value


def logup_sum(k: int, d_input: DevBuf, d_table: DevBuf, d_m: DevBuf, beta: int, usable_rows: int, d_phi: DevBuf) -> None:
    """h2mi_plonk_logup_sum_dev: phi[0] = 0, phi[i+1] = phi[i] + 1 / (A_i + beta) - M_i / (S_i + beta) on rows 0 .. usable_rows of d_phi"""
    _check(lib.h2mi_plonk_logup_sum_dev(d_input.ptr, d_table.ptr, d_m.ptr, k, usable_rows, F.fr_to_mont_limbs(beta).ctypes.data, d_phi.ptr, None),
           "logup_sum")


def logup_multiplicity_sets(k: int, d_inputs: DevBuf, n_inputs: int, d_table: DevBuf, usable_rows: int, d_m: DevBuf) -> int:
    """h2mi_plonk_logup_multiplicity_sets_dev: d_inputs holds n_inputs consecutive vectors of 2^k elements; d_m[r] = sum over the sets of
    #{i < usable_rows: A_j[i] = table[r]} on the first usable row r that holds its table value.  Returns the inputs of any set that are
    not table values."""
    missing = C.c_uint64()
    _check(lib.h2mi_plonk_logup_multiplicity_sets_dev(d_inputs.ptr, n_inputs, d_table.ptr, k, usable_rows, d_m.ptr, C.byref(missing), None),
           "logup_multiplicity_sets")
    return missing.value


def logup_sum_sets(k: int, d_inputs: DevBuf, n_inputs: int, d_table: DevBuf, d_m: DevBuf, beta: int, usable_rows: int, d_phi: DevBuf) -> None:
    """h2mi_plonk_logup_sum_sets_dev: phi[0] = 0, phi[i+1] = phi[i] + sum_j 1 / (A_j,i + beta) - M_i / (S_i + beta) on rows 0 ..
    usable_rows of d_phi"""
    _check(lib.h2mi_plonk_logup_sum_sets_dev(d_inputs.ptr, n_inputs, d_table.ptr, d_m.ptr, k, usable_rows, F.fr_to_mont_limbs(beta).ctypes.data,
                                             d_phi.ptr, None), "logup_sum_sets")


def logup_rank_cols(k: int, d_columns, d_sorted_canonical: DevBuf, n_unique: int, d_first: DevBuf, usable_rows: int, d_ranks: DevBuf,
                    d_counts: DevBuf, d_m: DevBuf) -> int:
    """h2mi_plonk_logup_rank_cols_dev: the usable rows of the listed columns (DevBufs anywhere in memory, 1 .. 6 of them) ranked against
    a table sorted elsewhere, in one launch: d_ranks[j 2^k + i] (u32), the joint histogram d_counts (u32 x n_unique) and the M column
    d_m (counts[r] on row first[r]).  Returns the inputs of any column that are no table value."""
    ptrs = (C.c_void_p * len(d_columns))(*[b.ptr for b in d_columns])
    missing = C.c_uint64()
    _check(lib.h2mi_plonk_logup_rank_cols_dev(ptrs, len(d_columns), d_sorted_canonical.ptr, n_unique, d_first.ptr, k, usable_rows, d_ranks.ptr,
                                              d_counts.ptr, d_m.ptr, C.byref(missing), None), "logup_rank_cols")
    return missing.value


def logup_sum_ranked(k: int, d_ranks: DevBuf, n_inputs: int, d_sorted_mont: DevBuf, d_counts: DevBuf, d_first: DevBuf, n_unique: int, beta: int,
                     usable_rows: int, d_phi: DevBuf) -> None:
    """h2mi_plonk_logup_sum_ranked_dev: the running sum of h2mi_plonk_logup_sum_sets_dev from the ranks: T[r] = 1 / (sorted[r] + beta) by one
    inversion, row i adds sum_j T[rank_j[i]], row first[r] subtracts counts[r] T[r]; rows 0 .. usable_rows of d_phi"""
    _check(lib.h2mi_plonk_logup_sum_ranked_dev(d_ranks.ptr, n_inputs, d_sorted_mont.ptr, d_counts.ptr, d_first.ptr, n_unique, k, usable_rows,
                                               F.fr_to_mont_limbs(beta).ctypes.data, d_phi.ptr, None), "logup_sum_ranked")


class _RangeCosets(C.Structure):
    _fields_ = [("a", C.c_void_p), ("lookup_advice", C.c_void_p), ("lookup_selector", C.c_void_p), ("q", C.c_void_p), ("table", C.c_void_p),
                ("perm_value", C.c_void_p * 4), ("perm_sigma", C.c_void_p * 4), ("perm_z", C.c_void_p * 4), ("lookup_permuted_input", C.c_void_p),
                ("lookup_permuted_table", C.c_void_p), ("lookup_z", C.c_void_p), ("l0", C.c_void_p), ("l_last", C.c_void_p), ("l_active", C.c_void_p),
                ("n_perm", C.c_uint32), ("chunk_len", C.c_uint32), ("has_lookup", C.c_uint32)]


def evaluate_h_range(domain: EvaluationDomain, a: DevBuf, lookup_advice: DevBuf, q: DevBuf, table: DevBuf, perm_values, perm_sigmas, perm_zs,
                     lk_input: DevBuf, lk_table: DevBuf, lk_z: DevBuf, l0: DevBuf, l_last: DevBuf, l_active: DevBuf, beta: int, gamma: int, y: int,
                     out: DevBuf, blinding_factors: int = BLINDING_FACTORS, lookup_selector: DevBuf = None, chunk_len: int = None) -> None:
    """h(X) on the extended coset (already divided by X^n - 1) for the halo2-lib constraint systems.  Lookup input: the
    column `lookup_advice` (chunks of two by default), or `lookup_selector` * a (halo2-base with one advice column: degree
    5, chunks of three), or none (all lookup arguments None: degree 3, chunks of one)."""
    m = len(perm_values)
    has_lookup = lookup_advice is not None or lookup_selector is not None
    chunk = chunk_len if chunk_len is not None else (3 if lookup_selector is not None else 2 if has_lookup else 1)
    assert 1 <= m <= 4 and len(perm_sigmas) == m and len(perm_zs) == -(-m // chunk)
    cs = _RangeCosets()
    cs.a, cs.q = a.ptr, q.ptr
    cs.chunk_len, cs.has_lookup = chunk, 1 if has_lookup else 0
    if has_lookup:
        cs.table = table.ptr
        if lookup_selector is not None:
            cs.lookup_selector = lookup_selector.ptr
        else:
            cs.lookup_advice = lookup_advice.ptr
        cs.lookup_permuted_input, cs.lookup_permuted_table, cs.lookup_z = lk_input.ptr, lk_table.ptr, lk_z.ptr
    for j in range(m):
        cs.perm_value[j], cs.perm_sigma[j] = perm_values[j].ptr, perm_sigmas[j].ptr
    for s in range(len(perm_zs)):
        cs.perm_z[s] = perm_zs[s].ptr
    cs.l0, cs.l_last, cs.l_active = l0.ptr, l_last.ptr, l_active.ptr
    cs.n_perm = m
    qs = quotient_scalars(domain, beta, gamma, y, blinding_factors)
    _check(lib.h2mi_plonk_evaluate_h_range_dev(C.byref(cs), C.byref(qs), out.ptr, None), "evaluate_h_range")


class _FlexCosets(C.Structure):
    """include/h2mi.h h2mi_flex_cosets"""
    G, P, L = 32, 64, 8  # H2MI_FLEX_MAX_GATES / _PERM / _LOOKUPS
    _fields_ = [("n_gates", C.c_uint32), ("gate_a", C.c_void_p * G), ("gate_q", C.c_void_p * G), ("n_perm", C.c_uint32), ("chunk_len", C.c_uint32),
                ("perm_value", C.c_void_p * P), ("perm_sigma", C.c_void_p * P), ("perm_z", C.c_void_p * P), ("n_lookups", C.c_uint32),
                ("lookup_input", C.c_void_p * L), ("lookup_input_b", C.c_void_p * L), ("lookup_table", C.c_void_p * L),
                ("lookup_permuted_input", C.c_void_p * L), ("lookup_permuted_table", C.c_void_p * L), ("lookup_z", C.c_void_p * L),
                ("l0", C.c_void_p), ("l_last", C.c_void_p), ("l_active", C.c_void_p)]


def _fill_arguments(cs, perm_values, perm_sigmas, perm_zs, chunk_len: int, lookups, l0: DevBuf, l_last: DevBuf, l_active: DevBuf) -> None:
    """the permutation, lookup and Lagrange fields that h2mi_flex_cosets and h2mi_expr_cosets share"""
    m = len(perm_values)
    assert m <= _FlexCosets.P and len(perm_sigmas) == m and len(perm_zs) == (-(-m // chunk_len) if m else 0) and len(lookups) <= _FlexCosets.L
    cs.n_perm, cs.chunk_len = m, chunk_len
    for j in range(m):
        cs.perm_value[j], cs.perm_sigma[j] = perm_values[j].ptr, perm_sigmas[j].ptr
    for s, z in enumerate(perm_zs):
        cs.perm_z[s] = z.ptr
    cs.n_lookups = len(lookups)
    for l, (a_in, b_in, table, pin, ptab, z) in enumerate(lookups):
        cs.lookup_input[l], cs.lookup_table[l] = a_in.ptr, table.ptr
        cs.lookup_input_b[l] = b_in.ptr if b_in is not None else None
        cs.lookup_permuted_input[l], cs.lookup_permuted_table[l], cs.lookup_z[l] = pin.ptr, ptab.ptr, z.ptr
    cs.l0, cs.l_last, cs.l_active = l0.ptr, l_last.ptr, l_active.ptr


def evaluate_h_flex(domain: EvaluationDomain, gates, perm_values, perm_sigmas, perm_zs, chunk_len: int, lookups, l0: DevBuf, l_last: DevBuf,
                    l_active: DevBuf, beta: int, gamma: int, y: int, out: DevBuf, blinding_factors: int = BLINDING_FACTORS) -> None:
    """h(X) on the extended coset for the GENERAL halo2-base shapes (h2mi_plonk_evaluate_h_flex_dev): `gates` = [(advice coset, selector
    coset)] (<= 32 vertical gates), the permutation argument over <= 64 columns, `lookups` = [(input coset, second input factor or None,
    table coset, permuted input, permuted table, product)] (<= 8) — what builder.config() configures when one column overflows."""
    assert 1 <= len(gates) <= _FlexCosets.G
    cs = _FlexCosets()
    cs.n_gates = len(gates)
    for g, (a, q) in enumerate(gates):
        cs.gate_a[g], cs.gate_q[g] = a.ptr, q.ptr
    _fill_arguments(cs, perm_values, perm_sigmas, perm_zs, chunk_len, lookups, l0, l_last, l_active)
    qs = quotient_scalars(domain, beta, gamma, y, blinding_factors)
    _check(lib.h2mi_plonk_evaluate_h_flex_dev(C.byref(cs), C.byref(qs), out.ptr, None), "evaluate_h_flex")


class _ExprCosets(C.Structure):
    """include/h2mi.h h2mi_expr_cosets"""
    A, Fx, P, L = 64, 64, 64, 8  # H2MI_EXPR_MAX_ADVICE / _FIXED, H2MI_FLEX_MAX_PERM / _LOOKUPS
    _fields_ = [("advice", C.c_void_p * A), ("fixed", C.c_void_p * Fx), ("instance", C.c_void_p), ("n_perm", C.c_uint32), ("chunk_len", C.c_uint32),
                ("perm_value", C.c_void_p * P), ("perm_sigma", C.c_void_p * P), ("perm_z", C.c_void_p * P), ("n_lookups", C.c_uint32),
                ("lookup_input", C.c_void_p * L), ("lookup_input_b", C.c_void_p * L), ("lookup_table", C.c_void_p * L),
                ("lookup_permuted_input", C.c_void_p * L), ("lookup_permuted_table", C.c_void_p * L), ("lookup_z", C.c_void_p * L),
                ("l0", C.c_void_p), ("l_last", C.c_void_p), ("l_active", C.c_void_p)]


class _ShuffleCosets(C.Structure):
    """include/h2mi.h h2mi_shuffle_cosets"""
    _fields_ = [("n_shuffles", C.c_uint32), ("input", C.c_void_p * 8), ("shuffle", C.c_void_p * 8), ("z", C.c_void_p * 8)]


class _InstanceCosets(C.Structure):
    """include/h2mi.h h2mi_instance_cosets"""
    _fields_ = [("n_instance", C.c_uint32), ("column", C.c_void_p * 8)]


class _LogupCosets(C.Structure):
    """include/h2mi.h h2mi_logup_cosets"""
    _fields_ = [("n_inputs", C.c_uint32 * _ExprCosets.L)]


# The three argument records of include/h2mi.h, field for field (tests/test_quotient_records_host.py compares the layouts with the C
# compiler's).  A record built by the helpers below holds what its pointers name in `_keep`.
class QuotientScalars(C.Structure):
    """include/h2mi.h h2mi_quotient_scalars"""
    _fields_ = [("k", C.c_uint32), ("extended_k", C.c_uint32), ("blinding_factors", C.c_uint32), ("beta", C.c_void_p), ("gamma", C.c_void_p),
                ("y", C.c_void_p), ("delta", C.c_void_p), ("zeta", C.c_void_p), ("extended_omega", C.c_void_p), ("t_inv", C.c_void_p)]


class QuotientCircuits(C.Structure):
    """include/h2mi.h h2mi_quotient_circuits"""
    _fields_ = [("circuits", C.c_void_p), ("n_circuits", C.c_uint32), ("shuffles", C.c_void_p), ("logup", C.c_void_p), ("instances", C.c_void_p),
                ("gates", C.c_void_p), ("challenges", C.c_void_p), ("n_challenges", C.c_uint32)]


class ExprColumns(C.Structure):
    """include/h2mi.h h2mi_expr_columns"""
    _fields_ = [("advice", C.c_void_p), ("n_advice", C.c_uint32), ("fixed", C.c_void_p), ("n_fixed", C.c_uint32), ("instances", C.c_void_p),
                ("program", C.c_void_p), ("challenges", C.c_void_p), ("n_challenges", C.c_uint32), ("k", C.c_uint32)]


def _addr(obj):
    return C.addressof(obj) if obj is not None else None


def _challenge_limbs(challenges):
    """-> (the values as n x 4 Montgomery limbs or None, n)"""
    if challenges is None or len(challenges) == 0:
        return None, 0
    return np.ascontiguousarray(np.stack([F.fr_to_mont_limbs(v) for v in challenges])), len(challenges)


def quotient_scalars(domain: EvaluationDomain, beta: int, gamma: int, y: int, blinding_factors: int = BLINDING_FACTORS) -> QuotientScalars:
    """the h2mi_quotient_scalars of a domain and a transcript's beta, gamma, y: DELTA, the coset generator, extended_omega and the
    inverses of X^n - 1 on the coset are the domain's"""
    bufs = [F.fr_to_mont_limbs(v) for v in (beta, gamma, y, FR_DELTA, domain.g_coset, domain.extended_omega)]
    bufs.append(np.ascontiguousarray(vanishing_inverses(domain)))
    qs = QuotientScalars(domain.k, domain.extended_k, blinding_factors, *[b.ctypes.data for b in bufs])
    qs._keep = bufs
    return qs


def quotient_circuits(program, cosets, n_circuits: int, challenges=(), shuffles=None, logup=None, instances=None) -> QuotientCircuits:
    """the h2mi_quotient_circuits of a proof: `cosets` an h2mi_expr_cosets or an array of them (expr_cosets_array), `shuffles`, `logup`,
    `instances` as argument_cosets gives them (each may be None), `challenges` a list of integers (None or empty: none)"""
    ch, n_ch = _challenge_limbs(challenges)
    qc = QuotientCircuits(_addr(cosets), n_circuits, _addr(shuffles), _addr(logup), _addr(instances), _addr(program),
                          ch.ctypes.data if ch is not None else None, n_ch)
    qc._keep = (cosets, shuffles, logup, instances, program, ch)
    return qc


def expr_columns(program, advice, fixed, instance, k: int, challenges=None) -> ExprColumns:
    """the h2mi_expr_columns of a program over `advice` / `fixed` (lists of DevBuf, None for a column the program does not read) on one
    domain; `instance`: a DevBuf or None (the one instance column), or an h2mi_instance_cosets"""
    ptrs = lambda cols: (C.c_void_p * max(len(cols), 1))(*[c.ptr if c is not None else None for c in cols])
    adv, fix = ptrs(advice), ptrs(fixed)
    if not isinstance(instance, _InstanceCosets):
        instance = _InstanceCosets(1, (C.c_void_p * 8)(instance.ptr if instance is not None else None))
    ch, n_ch = _challenge_limbs(challenges)
    ec = ExprColumns(C.addressof(adv), len(advice), C.addressof(fix), len(fixed), C.addressof(instance), _addr(program),
                     ch.ctypes.data if ch is not None else None, n_ch, k)
    ec._keep = (adv, fix, instance, program, ch)
    return ec


def expr_cosets_array(circuits, perm_sigmas, chunk_len: int, l0: DevBuf, l_last: DevBuf, l_active: DevBuf):
    """-> an array of h2mi_expr_cosets, one entry per circuit of a proof.  circuits: per circuit a dict with `advice`, `fixed` (lists of
    DevBuf, None for a column the program does not read), `instance` (or None), `perm_values`, `perm_zs`, `lookups` as evaluate_h_flex
    takes them; what the proof shares — perm_sigmas, chunk_len, the Lagrange cosets — is given once and stated in every entry."""
    arr = (_ExprCosets * max(len(circuits), 1))()
    for cs, c in zip(arr, circuits):
        assert len(c["advice"]) <= _ExprCosets.A and len(c["fixed"]) <= _ExprCosets.Fx
        for j, a in enumerate(c["advice"]):
            cs.advice[j] = a.ptr if a is not None else None
        for j, f in enumerate(c["fixed"]):
            cs.fixed[j] = f.ptr if f is not None else None
        cs.instance = c["instance"].ptr if c.get("instance") is not None else None
        _fill_arguments(cs, c["perm_values"], perm_sigmas, c["perm_zs"], chunk_len, c["lookups"], l0, l_last, l_active)
    return arr


def argument_cosets(circuits, logup_sets=None):
    """-> (h2mi_shuffle_cosets array or None, h2mi_logup_cosets or None, h2mi_instance_cosets array) for the circuits of a proof: per
    circuit `shuffles` [(input, shuffle side, product)] and `instances` [DevBuf or None] beside what expr_cosets_array reads;
    logup_sets: the input sets per lookup of a logUp proof (the entries' n_lookups then carry H2MI_LOOKUPS_LOGUP: set by the caller)"""
    n = max(len(circuits), 1)
    shs, ins = (_ShuffleCosets * n)(), (_InstanceCosets * n)()
    for sh, ic, c in zip(shs, ins, circuits):
        sh.n_shuffles = len(c.get("shuffles", ()))
        for i, (a_in, s_in, z) in enumerate(c.get("shuffles", ())):
            sh.input[i], sh.shuffle[i], sh.z[i] = a_in.ptr, s_in.ptr, z.ptr
        ic.n_instance = len(c.get("instances", ()))
        for i, col in enumerate(c.get("instances", ())):
            ic.column[i] = col.ptr if col is not None else None
    lg = None
    if logup_sets is not None:
        lg = _LogupCosets()
        for l in range(_ExprCosets.L):
            lg.n_inputs[l] = logup_sets[l] if l < len(logup_sets) else 1
    return (shs if any(sh.n_shuffles for sh in shs) else None), lg, ins


def evaluate_h_expr(domain: EvaluationDomain, program, advice, fixed, instance, perm_values, perm_sigmas, perm_zs, chunk_len: int, lookups,
                    l0: DevBuf, l_last: DevBuf, l_active: DevBuf, beta: int, gamma: int, y: int, out: DevBuf,
                    blinding_factors: int = BLINDING_FACTORS, challenges=None, shuffles=None, logup=None, instances=None) -> None:
    """h(X) on the extended coset of ONE circuit with the gates given as a postfix program (h2mi_plonk_evaluate_h_expr_dev): `program` an
    engine.GateProgram over the coset forms `advice` / `fixed` (lists, None for a column the program does not read) and `instance`
    (or None); permutation argument and lookups as evaluate_h_flex takes them, both optional.  challenges: a list of integers, the
    values CHALLENGE ops push (None: none); shuffles, logup, instances: argument_cosets' results for this one circuit."""
    cosets = expr_cosets_array([dict(advice=advice, fixed=fixed, instance=instance, perm_values=perm_values, perm_zs=perm_zs, lookups=lookups)],
                               perm_sigmas, chunk_len, l0, l_last, l_active)
    qc = quotient_circuits(program, cosets, 1, challenges, shuffles, logup, instances)
    qs = quotient_scalars(domain, beta, gamma, y, blinding_factors)
    _check(lib.h2mi_plonk_evaluate_h_expr_dev(C.byref(qc), C.byref(qs), out.ptr, None), "evaluate_h_expr")


def evaluate_h_expr_slice(domain: EvaluationDomain, program, cosets, n_circuits: int, slice_index, beta: int, gamma: int, y: int, out: DevBuf,
                          blinding_factors: int = BLINDING_FACTORS, challenges=(), shuffles=None, logup=None, instances=None) -> None:
    """h2mi_plonk_evaluate_h_expr_batch_dev with a slice: the numerator of the circuits on ONE coset of 2^k points — every column of
    `cosets` (expr_cosets_array), `shuffles`, `logup` and `instances` (argument_cosets) is slice `slice_index` of its extended-coset vector
    (coeff_to_slice_oop_dev), `out` the whole vector of 2^extended_k elements, of which elements slice_index + rot i are written.
    slice_index None: the resident call over whole extended-coset vectors (H2MI_WHOLE_COSET), same arguments."""
    qc = quotient_circuits(program, cosets, n_circuits, challenges, shuffles, logup, instances)
    qs = quotient_scalars(domain, beta, gamma, y, blinding_factors)
    _check(lib.h2mi_plonk_evaluate_h_expr_batch_dev(C.byref(qc), C.byref(qs), -1 if slice_index is None else slice_index, out.ptr, None),
           "evaluate_h_expr_batch" if slice_index is None else "evaluate_h_expr_slice")


def evaluate_h_expr_batch(domain: EvaluationDomain, program, cosets, n_circuits: int, beta: int, gamma: int, y: int, out: DevBuf,
                          blinding_factors: int = BLINDING_FACTORS, challenges=(), shuffles=None, logup=None, instances=None) -> None:
    """h(X) of SEVERAL circuits in one proof (h2mi_plonk_evaluate_h_expr_batch_dev): one accumulator folded with y over every circuit's
    gate, permutation, lookup and shuffle terms in circuit order, one division by X^n - 1.  cosets: expr_cosets_array's result (the first
    n_circuits entries are read); program and challenges are the proof's; shuffles, logup, instances: argument_cosets' results."""
    evaluate_h_expr_slice(domain, program, cosets, n_circuits, None, beta, gamma, y, out, blinding_factors, challenges, shuffles, logup, instances)


def expr_compress(program, advice, fixed, instance, k: int, domain_k: int, theta: int, out: DevBuf, challenges=None) -> None:
    """h2mi_plonk_expr_compress_dev: out[i] = sum_j e_j(i) theta^(m-1-j) over the m polynomials of `program` (an engine.GateProgram) on
    the 2^domain_k points the columns are given on (expr_columns' arguments); challenges: as evaluate_h_expr takes them."""
    cols = expr_columns(program, advice, fixed, instance, k, challenges)
    _check(lib.h2mi_plonk_expr_compress_dev(C.byref(cols), domain_k, F.fr_to_mont_limbs(theta).ctypes.data, out.ptr, None), "expr_compress")


def expr_check(program, advice, fixed, instance, k: int, n_rows: int = None, challenges=None):
    """h2mi_plonk_expr_check_dev: per polynomial of `program` (an engine.GateProgram) -> (the number of rows below n_rows on which it
    is not zero, the smallest such row or 0xffffffff); columns on the 2^k rows as expr_compress takes them, n_rows = 2^k by default"""
    cols = expr_columns(program, advice, fixed, instance, k, challenges)
    report = np.zeros((max(sum(1 for i in range(program.n_ops) if program.ops[i].op == 8), 1), 2), dtype=np.uint32)
    n_polys = C.c_uint32()
    _check(lib.h2mi_plonk_expr_check_dev(C.byref(cols), (1 << k) if n_rows is None else n_rows, report.ctypes.data, C.byref(n_polys), None),
           "expr_check")
    return [(int(c), int(f)) for c, f in report[: n_polys.value]]


def copy_check(values, cells: DevBuf, n_cells: int):
    """h2mi_plonk_copy_check_dev: values — the permutation argument's columns on the rows (DevBuf); cells — n_cells x 4 uint32 on the
    device, (column, row, image column, image row) -> (unequal cells, the smallest index of one or 0xffffffff)"""
    report = np.zeros(2, dtype=np.uint32)
    ptrs = (C.c_void_p * max(len(values), 1))(*[v.ptr for v in values])
    _check(lib.h2mi_plonk_copy_check_dev(ptrs, len(values), cells.ptr, n_cells, report.ctypes.data, None), "copy_check")
    return int(report[0]), int(report[1])


def lookup_member(inputs: DevBuf, sorted_canonical: DevBuf, n_unique: int, usable_rows: int):
    """h2mi_plonk_lookup_member_dev -> (rows below usable_rows whose input is none of the n_unique sorted table values, the smallest)"""
    report = np.zeros(2, dtype=np.uint32)
    _check(lib.h2mi_plonk_lookup_member_dev(inputs.ptr, sorted_canonical.ptr, n_unique, usable_rows, report.ctypes.data, None), "lookup_member")
    return int(report[0]), int(report[1])


def sort_unique(values: DevBuf, count: int):
    """h2mi_fr_sort_unique_dev over the first `count` elements -> (canonical values, Montgomery values, u32 multiplicities, n_unique):
    the table arguments of h2mi_plonk_lookup_permute_dev"""
    canon, mont, mult = DevBuf(count * 32), DevBuf(count * 32), DevBuf(count * 4)
    n_unique = C.c_uint32()
    _check(lib.h2mi_fr_sort_unique_dev(values.ptr, count, canon.ptr, mont.ptr, mult.ptr, C.byref(n_unique), None), "sort_unique")
    return canon, mont, mult, n_unique.value


def sort_unique_first(values: DevBuf, count: int):
    """h2mi_fr_sort_unique_first_dev -> (canonical values, Montgomery values, u32 multiplicities, u32 first positions, n_unique): the table
    arguments of h2mi_plonk_logup_rank_cols_dev / _sum_ranked_dev"""
    canon, mont, mult, first = DevBuf(count * 32), DevBuf(count * 32), DevBuf(count * 4), DevBuf(count * 4)
    n_unique = C.c_uint32()
    _check(lib.h2mi_fr_sort_unique_first_dev(values.ptr, count, canon.ptr, mont.ptr, mult.ptr, first.ptr, C.byref(n_unique), None), "sort_unique_first")
    return canon, mont, mult, first, n_unique.value
