"""GPU tests of the lookup argument on the device (BASELINE config 3: range.rs with LOOKUP_BITS): the
permuted input / table columns (a counting sort against the fixed table instead of the crate's sort + BTreeMap walk), the
lookup grand product and `evaluate_h` of the range-check constraint system (degree 4, extended domain 4n) against
oracle/lookup.py — element for element at k <= 8, through the quotient identity at k = 16; then the permuted columns and the grand
product alone, row by row, at the sizes where their kernels take more than one workgroup, tile or scan segment (k = 11 .. 14)."""
import types

import numpy as np
import pytest

import lookup_scale_cases as scale
from oracle import bn254 as o
from oracle import lookup as L
from oracle.plonk import BLINDING_FACTORS

pytestmark = pytest.mark.gpu


def _vals(buf, count):
    return o.unpack(buf.to_numpy(shape=(count, 4), nbytes=count * 32), o.R)


def _dev(gpu, values):
    return gpu.DevBuf.from_numpy(o.pack(values, o.R))


@pytest.mark.parametrize("k,case", [(5, "mixed"), (6, "one value"), (7, "all distinct"), (8, "two values"), (8, "mixed"), (8, "zeros in table")])
def test_lookup_permuted_columns_match_oracle(gpu, k, case):
    """permute_expression_pair on the device == the crate's construction restated in the oracle, for input multisets that
    stress it: every row the same value (one run, every other row repeated), all distinct (no repeated row: S' = A'),
    two values, and a table that itself holds a repeated value (the zero padding of a range table)."""
    from halo2_scaffold_amd import plonk as gp

    n = 1 << k
    u = n - (BLINDING_FACTORS + 1)
    rng = np.random.default_rng(k + len(case))
    if case == "zeros in table":
        tbl = list(range(1 << (k - 2))) + [0] * (n - (1 << (k - 2)))  # a range table padded with zeros
        inputs = [int(rng.integers(0, 1 << (k - 2))) for _ in range(u)]
    else:
        tbl = [(i * 0x9E3779B97F4A7C15 + 12345) % o.R for i in range(n)]  # arbitrary distinct field elements
        if case == "one value":
            inputs = [tbl[7]] * u
        elif case == "all distinct":
            inputs = list(rng.permutation(tbl[:u]))
        elif case == "two values":
            inputs = [tbl[3] if rng.random() < 0.3 else tbl[u - 1] for _ in range(u)]
        else:
            inputs = [tbl[int(rng.integers(0, u // 3))] for _ in range(u)]
    inputs = [int(v) for v in inputs]
    blind = list(range(1000, 1000 + BLINDING_FACTORS + 1))
    want_a, want_s = L.permute_expression_pair(inputs + [0] * (n - u), tbl, u, blind, blind)
    table = gp.LookupTable(tbl, u)
    d_in = _dev(gpu, inputs + [0] * (n - u))
    d_a, d_s = _dev(gpu, [0] * u + blind), _dev(gpu, [0] * u + blind)  # blinding rows are the caller's
    assert gp.lookup_permute(k, d_in, table, d_a, d_s) == 0
    assert _vals(d_a, n) == want_a
    assert _vals(d_s, n) == want_s
    # an input outside the table is counted (the crate fails the proof)
    bad = list(inputs)
    bad[u // 2] = (max(tbl) + 1) % o.R
    bad[0] = (max(tbl) + 2) % o.R
    d_bad = _dev(gpu, bad + [0] * (n - u))
    assert gp.lookup_permute(k, d_bad, table, d_a, d_s) == 2
    for b in (d_in, d_a, d_s, d_bad):
        b.free()
    table.free()


@pytest.mark.parametrize("k,bits,extra", [(5, 3, 0), (6, 4, 2), (8, 6, 2)])
def test_lookup_product_and_evaluate_h_range_match_oracle(gpu, k, bits, extra):
    """lookup grand product, permutation products in chunks of two and the whole quotient numerator of the range-check
    constraint system (gate + permutation terms + five lookup terms, divided by X^n - 1) == oracle, element for element;
    then the quotient identity on the device-produced h(X)."""
    from halo2_scaffold_amd import plonk as gp

    inst = L.RangeInstance(k, bits, seed=10 + k, extra_cols=extra)
    n, u = inst.n, inst.u
    beta, gamma, y, x = 0xBE7A + k, 0x6A33A, 0x1234567, 0xFEDCBA987654321
    a_perm, s_perm = inst.permuted()
    z_lk = L.lookup_product(inst.la, inst.table, a_perm, s_perm, beta, gamma, u, inst.blind(BLINDING_FACTORS))
    zs = inst.permutation_products(beta, gamma)
    # device: permuted columns, lookup product, permutation products
    table = gp.LookupTable(inst.table, u)
    d_la, d_t = _dev(gpu, inst.la), _dev(gpu, inst.table)
    d_ap, d_sp = _dev(gpu, [0] * u + a_perm[u:]), _dev(gpu, [0] * u + s_perm[u:])
    assert gp.lookup_permute(k, d_la, table, d_ap, d_sp) == 0
    assert _vals(d_ap, n) == a_perm and _vals(d_sp, n) == s_perm
    d_zl = _dev(gpu, [0] * (u + 1) + z_lk[u + 1 :])
    gp.lookup_product(k, d_la, d_t, d_ap, d_sp, beta, gamma, u, d_zl)
    assert _vals(d_zl, n) == z_lk
    d_cols = [_dev(gpu, c) for c in inst.perm_cols]
    d_sig = [_dev(gpu, c) for c in inst.sigma]
    d_zs = [_dev(gpu, [0] * (u + 1) + z[u + 1 :]) for z in zs]
    gp.permutation_products(k, d_cols, d_sig, L.CS_DEGREE - 2, beta, gamma, u, d_zs)
    assert [_vals(z, n) for z in d_zs] == zs
    # extended cosets on the device, evaluate_h
    dom = gpu.EvaluationDomain(L.CS_DEGREE, k)
    ext = dom.extended_len()
    assert ext == 4 * n

    def to_ext(d_lagr):
        p, e = gpu.DevBuf(n * 32), gpu.DevBuf(ext * 32)
        dom.lagrange_to_coeff_oop_dev(d_lagr, p)
        dom.coeff_to_extended_oop_dev(p, e)
        p.free()
        return e

    e_a, e_la, e_q, e_t = to_ext(d_cols[0]), to_ext(d_la), to_ext(_dev(gpu, inst.q)), to_ext(d_t)
    e_cols = [to_ext(c) for c in d_cols]
    e_sig = [to_ext(c) for c in d_sig]
    e_zs = [to_ext(z) for z in d_zs]
    e_ap, e_sp, e_zl = to_ext(d_ap), to_ext(d_sp), to_ext(d_zl)
    e_l0, e_ll, e_la_ = to_ext(_dev(gpu, inst.l0)), to_ext(_dev(gpu, inst.l_last)), to_ext(_dev(gpu, inst.l_active))
    out = gpu.DevBuf(ext * 32)
    gp.evaluate_h_range(dom, e_a, e_la, e_q, e_t, e_cols, e_sig, e_zs, e_ap, e_sp, e_zl, e_l0, e_ll, e_la_, beta, gamma, y, out)
    want = inst.divide_by_vanishing(inst.evaluate_h(zs, a_perm, s_perm, z_lk, beta, gamma, y))
    assert _vals(out, ext) == want
    dom.extended_to_coeff_dev(out)
    hc = _vals(out, ext)
    assert not any(hc[3 * n :])  # degree bound: the division was exact
    assert L.check_quotient_identity(inst, zs, a_perm, s_perm, z_lk, hc[: 3 * n], beta, gamma, y, x)


def test_range_quotient_identity_at_2pow16(gpu):
    """size-independent check at DEGREE = 16 with LOOKUP_BITS = 12: everything after the witness is produced on the
    device (permuted columns, both grand products, 17 coset transforms, evaluate_h_range, the coset iNTT) and the
    verifier's equation is evaluated at a random point with the device's eval_polynomial on the device-resident
    polynomials.  A tampered lookup column (one value swapped for another table value) must break it."""
    import ctypes as C

    from halo2_scaffold_amd import field as F
    from halo2_scaffold_amd import plonk as gp

    k, bits = 16, 12
    inst = L.RangeInstance(k, bits, seed=77, gates=3000, extra_cols=2)
    n, u = inst.n, inst.u
    beta, gamma, y = 0xB0B0B0B, 0xCACACA, 0xD0D0D0D0
    dom = gpu.EvaluationDomain(L.CS_DEGREE, k)
    ext = dom.extended_len()
    blind = inst.blind(3 * (BLINDING_FACTORS + 1) + 2 * BLINDING_FACTORS)
    table = gp.LookupTable(inst.table, u)
    d = lambda vals: _dev(gpu, vals)
    polys = {}

    def to_poly_and_ext(key, d_lagr):
        p, e = gpu.DevBuf(n * 32), gpu.DevBuf(ext * 32)
        dom.lagrange_to_coeff_oop_dev(d_lagr, p)
        dom.coeff_to_extended_oop_dev(p, e)
        polys[key] = p
        return e

    def run(la_values):
        d_la, d_t = d(la_values), d(inst.table)
        d_ap, d_sp = d([0] * u + blind[:6]), d([0] * u + blind[6:12])
        missing = gp.lookup_permute(k, d_la, table, d_ap, d_sp)
        d_zl = d([0] * (u + 1) + blind[12:17])
        gp.lookup_product(k, d_la, d_t, d_ap, d_sp, beta, gamma, u, d_zl)
        cols = [inst.a, la_values] + inst.extras
        d_cols = [d(c) for c in cols]
        d_sig = [d(c) for c in inst.sigma]
        d_zs = [d([0] * (u + 1) + blind[17 + 5 * s : 22 + 5 * s]) for s in range(2)]
        gp.permutation_products(k, d_cols, d_sig, 2, beta, gamma, u, d_zs)
        e_cols = [to_poly_and_ext(("col", j), c) for j, c in enumerate(d_cols)]
        e_sig = [to_poly_and_ext(("sigma", j), c) for j, c in enumerate(d_sig)]
        e_zs = [to_poly_and_ext(("z", s), z) for s, z in enumerate(d_zs)]
        e_q, e_t = to_poly_and_ext("q", d(inst.q)), to_poly_and_ext("table", d_t)
        e_ap, e_sp, e_zl = to_poly_and_ext("a_perm", d_ap), to_poly_and_ext("s_perm", d_sp), to_poly_and_ext("z_lk", d_zl)
        e_l0, e_ll, e_lact = to_poly_and_ext("l0", d(inst.l0)), to_poly_and_ext("l_last", d(inst.l_last)), to_poly_and_ext("l_active", d(inst.l_active))
        h = gpu.DevBuf(ext * 32)
        gp.evaluate_h_range(dom, e_cols[0], e_cols[1], e_q, e_t, e_cols, e_sig, e_zs, e_ap, e_sp, e_zl, e_l0, e_ll, e_lact, beta, gamma, y, h)
        dom.extended_to_coeff_dev(h)
        top = h.to_numpy(shape=(n, 4), nbytes=n * 32, offset=3 * n * 32)
        return missing, h, not top.any(), _vals(d_zl, u + 1)[u], _vals(d_zs[1], u + 1)[u]

    out32 = gpu.DevBuf(32)

    def ev_dev(buf, point, offset=0):
        pl = F.fr_to_mont_limbs(point)
        assert gpu.lib.h2mi_fr_eval_poly_dev(buf.ptr + offset * 32, n, pl.ctypes.data, out32.ptr, None) == 0
        return _vals(out32, 1)[0]

    key_of = {id(inst.a): ("col", 0), id(inst.q): "q", id(inst.table): "table", id(inst.l0): "l0", id(inst.l_last): "l_last",
              id(inst.l_active): "l_active"}
    for j, c in enumerate(inst.sigma):
        key_of[id(c)] = ("sigma", j)
    for j, c in enumerate(inst.extras):
        key_of[id(c)] = ("col", 2 + j)

    def check(la_values, h):
        key_of[id(la_values)] = ("col", 1)
        inst.la = la_values
        inst.perm_cols = [inst.a, la_values] + inst.extras
        ev = lambda obj, pt: ev_dev(polys[obj if isinstance(obj, (str, tuple)) else key_of[id(obj)]], pt)
        pt = 0x1F2E3D4C5B6A79881726354453627180 % o.R
        ptn = pow(pt, n, o.R)
        h_at = (ev_dev(h, pt) + ptn * ev_dev(h, pt, n) + ptn * ptn % o.R * ev_dev(h, pt, 2 * n)) % o.R

        class HC:  # check_quotient_identity evaluates h_coeffs with the oracle's Horner: hand it the value instead
            pass

        orig = o.eval_polynomial
        o.eval_polynomial = lambda coeffs, point: h_at if coeffs is HC else orig(coeffs, point)
        try:
            return L.check_quotient_identity(inst, [("z", 0), ("z", 1)], "a_perm", "s_perm", "z_lk", HC, beta, gamma, y, pt, ev=ev)
        finally:
            o.eval_polynomial = orig

    la_good = list(inst.la)
    missing, h, exact, zl_end, zp_end = run(la_good)
    assert missing == 0 and exact and zl_end == 1 and zp_end == 1
    assert check(la_good, h)
    # tamper: a lookup cell that is copy-constrained to a gate cell gets another (valid) table value: the lookup still
    # closes, the permutation argument does not, the numerator is no longer divisible and the identity fails
    la_bad = list(inst.la)
    la_bad[3] = (la_bad[3] + 1) % (1 << bits)
    missing, h_bad, exact_bad, zl_end, zp_end = run(la_bad)
    assert missing == 0 and zl_end == 1 and zp_end != 1
    assert not exact_bad or not check(la_bad, h_bad)


# ---- beyond one workgroup: tests/lookup_scale_cases.py (checked on the CPU by tests/test_lookup_scale_host.py) ------------------------
def _upload(gpu, values):
    return gpu.DevBuf.from_numpy(scale.mont_limbs(values))


def _assert_column(buf, want, what):
    """the buffer's bytes == the Montgomery form of `want`; a mismatch names the first row"""
    got = buf.to_numpy(shape=(len(want), 4), nbytes=len(want) * 32)
    if np.array_equal(got, scale.mont_limbs(want)):
        return
    values = scale.from_mont_limbs(got)
    rows = [r for r in range(len(want)) if values[r] != want[r]]
    assert not rows, f"{what}: {len(rows)} rows differ, the first at row {rows[0]}: {values[rows[0]]:#x} != {want[rows[0]]:#x}"
    raise AssertionError(f"{what}: equal as field elements, but not in the canonical Montgomery form")


def _check_permute(gpu, case):
    """both routes into h2mi_plonk_lookup_permute_dev — the table sorted on the host (gp.LookupTable) and on the device
    (plonk.sort_unique of the Montgomery column) — against the oracle on all n rows; the rows beyond u are the caller's"""
    from halo2_scaffold_amd import plonk as gp

    k, n, u = case.k, case.n, case.u
    want_a, want_s = L.permute_expression_pair(case.inputs, case.table, u, case.keep_a, case.keep_s)
    d_in, d_tab = _upload(gpu, case.inputs), _upload(gpu, case.table)
    host = gp.LookupTable(case.table, u)
    canon, mont, mult, n_unique = gp.sort_unique(d_tab, u)
    assert n_unique == host.n_unique == len(set(case.table[:u]))
    device = types.SimpleNamespace(sorted_canonical=canon, sorted_mont=mont, mult=mult, n_unique=n_unique, usable_rows=u)
    routes = (("host table", host), ("device table", device))
    for route, table in routes:
        d_a, d_s = _upload(gpu, [0] * u + case.keep_a), _upload(gpu, [0] * u + case.keep_s)
        assert gp.lookup_permute(k, d_in, table, d_a, d_s) == 0, route
        _assert_column(d_a, want_a, f"A' ({route})")
        _assert_column(d_s, want_s, f"S' ({route})")
        d_a.free()
        d_s.free()
    return d_in, routes, (canon, mont, mult, d_tab, host)


def _free(d_in, keep):
    canon, mont, mult, d_tab, host = keep
    for b in (d_in, canon, mont, mult, d_tab):
        b.free()
    host.free()


@pytest.mark.parametrize("k,table_kind,input_kind", scale.PERMUTE_CASES, ids=[f"k{k}-{t}-{i}".replace(" ", "_") for k, t, i in scale.PERMUTE_CASES])
def test_lookup_permute_beyond_one_workgroup(gpu, k, table_kind, input_kind):
    """k_lk_rank with two and more workgroups — the binary search on arbitrary tables, the guess `rank = low word` landing on a real
    entry that differs above word 0, every rank of a workgroup in one slot of its 64-slot table (the global-atomic fallback), the two
    ends of the search — and, at k = 14, the counter scans in two segments.  Then three inputs that are in no table row (below the
    smallest, above the largest, between two neighbours; rows 0, 1024 and u - 1): exactly three are counted."""
    from halo2_scaffold_amd import plonk as gp

    case = scale.permute_case(k, table_kind, input_kind)
    d_in, routes, keep = _check_permute(gpu, case)
    d_bad = _upload(gpu, case.bad_inputs)
    d_a, d_s = gpu.DevBuf(case.n * 32), gpu.DevBuf(case.n * 32)
    for route, table in routes:
        assert gp.lookup_permute(k, d_bad, table, d_a, d_s) == 3, route
    for b in (d_bad, d_a, d_s):
        b.free()
    _free(d_in, keep)


@pytest.mark.parametrize("index", range(len(scale.USABLE_ROWS)), ids=[f"k{k}-u{u}-distinct{scale.usable_case_distinct(i)}" for i, (k, u) in enumerate(scale.USABLE_ROWS)])
def test_lookup_permute_usable_rows_and_scan_pads(gpu, index):
    """usable_rows as a free argument: every residue modulo 4 of it and of the table's distinct count (the scans run over lengths
    rounded up to 4 and k_lk_fill_table reads the total at index u: the pads must be zero), one row either side of a k_lk_rank
    workgroup (1024) and of a scan segment (8192)"""
    d_in, _, keep = _check_permute(gpu, scale.usable_case(index))
    _free(d_in, keep)


def _compact_launches(gpu, call):
    """launches of k_lookup_compact (the sparse form's position list) during call(), from the library's launch profile"""
    import ctypes as C

    lib = gpu.lib
    assert lib.h2mi_profile_reset() == 0 and lib.h2mi_profile_filter(b"") == 0 and lib.h2mi_profile_enable(1) == 0
    try:
        call()
    finally:
        assert lib.h2mi_profile_enable(0) == 0
    ms, count, every = C.c_double(), C.c_uint64(), C.c_uint64()
    assert lib.h2mi_profile_query(b"k_lookup_compact", C.byref(ms), C.byref(count)) == 0
    assert lib.h2mi_profile_query(b"", C.byref(ms), C.byref(every)) == 0
    assert lib.h2mi_profile_reset() == 0
    assert every.value > 0  # the profile did record this call's launches
    return count.value


@pytest.mark.parametrize("name", list(scale.PRODUCT_CASES), ids=[name.replace(" ", "_") for name in scale.PRODUCT_CASES])
def test_lookup_product_every_regime(gpu, name):
    """h2mi_plonk_lookup_product_dev on four columns of which exactly m rows have a ratio other than one, rows 0 .. u against the
    oracle's row-by-row product: the dense form over several tiles of 1024 (tile offsets, the reverse scan over a partial last tile),
    both sides of `usable_rows >= 4096 && 4 m <= u`, the empty position list, position counts around a tile, positions in the second
    scan segment of the compaction.  Which form ran is read from the library's launch profile (one k_lookup_compact launch in the
    sparse form with m > 0, none otherwise), so that a case cannot pass through the other branch."""
    from halo2_scaffold_amd import plonk as gp

    case = scale.product_case(name)
    n, u = case.n, case.u
    want = L.lookup_product(case.inputs, case.table, case.pin, case.ptab, case.beta, case.gamma, u, [])
    assert len(want) == u + 1
    assert sum(want[i + 1] != want[i] for i in range(u)) == case.m
    bufs = [_upload(gpu, col) for col in (case.inputs, case.table, case.pin, case.ptab)]
    d_z = _upload(gpu, [scale.SENTINEL] * n)
    launches = _compact_launches(gpu, lambda: gp.lookup_product(case.k, *bufs, case.beta, case.gamma, u, d_z))
    _assert_column(d_z, want + [scale.SENTINEL] * (n - u - 1), "z")  # z_0 .. z_u; the rows beyond are the caller's
    assert launches == (1 if case.form == "sparse" and case.m else 0)
    for b in bufs + [d_z]:
        b.free()
