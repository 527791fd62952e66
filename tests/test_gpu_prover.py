"""GPU tests of the data-true prover pipeline: keygen_vk / keygen_pk /
create_proof of the reference's StandardPlonk circuit on the device against the oracle's restatement
(oracle/prover.py) — element for element and byte for byte at small sizes, and at the reference's timed size
through the checks the reference itself relies on (the proof verifies: examples/standard_plonk.rs:57-64) plus the
quotient identity evaluated at a fresh random point with the device's eval_polynomial."""
import numpy as np
import pytest

import perm_scale_cases
from oracle import bn254 as o
from oracle import plonk as P
from oracle import prover as OP

pytestmark = pytest.mark.gpu

SRS_SECRET = 0x5EC2E7 + 0x48324D49


def _setup(gpu, k):
    from halo2_scaffold_amd import circuits, keygen

    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    circuit = circuits.StandardPlonk(None)
    vk = keygen.keygen_vk(params, circuit)
    pk = keygen.keygen_pk(params, vk, circuit)
    return params, vk, pk


def _vals(buf, count):
    return o.unpack(buf.to_numpy(shape=(count, 4), nbytes=count * 32), o.R)


@pytest.mark.parametrize("k", [4, 5, 8])
def test_keygen_matches_oracle(gpu, k):
    """device keygen (fixed columns, sigma polynomials from Assembly::copy, l_0 / l_last / l_active, their coefficient
    and extended forms, the eight vk commitments, transcript_repr) == oracle, element for element."""
    params, vk, pk = _setup(gpu, k)
    opk = OP.ProvingKey(k, SRS_SECRET)
    inst, dom = opk.inst, opk.dom
    n, ext = 1 << k, 1 << dom.extended_k
    assert o.unpack_points(vk.fixed_commitments) == opk.fixed_commitments
    assert o.unpack_points(vk.permutation_commitments) == opk.permutation_commitments
    assert vk.transcript_repr == opk.transcript_repr and vk.to_bytes() == opk.vk_bytes()
    cf = OP.VerifierKey.closed_form(k, SRS_SECRET)
    assert cf.fixed_commitments == opk.fixed_commitments and cf.permutation_commitments == opk.permutation_commitments
    for j in range(5):
        assert _vals(pk.fixed.polys[j], n) == opk.fixed_polys[j]
        assert _vals(pk.fixed.cosets[j], ext) == dom.coeff_to_extended(opk.fixed_polys[j])
    for j in range(3):
        assert _vals(pk.permutation.values[j], n) == inst.sigma[j]
        assert _vals(pk.permutation.polys[j], n) == opk.sigma_polys[j]
        assert _vals(pk.permutation.cosets[j], ext) == dom.coeff_to_extended(opk.sigma_polys[j])
    for dev, lag in ((pk.l0, inst.l0), (pk.l_last, inst.l_last), (pk.l_active, inst.l_active)):
        assert _vals(dev, ext) == inst.to_extended(lag)
    pk.release()
    params.release()


@pytest.mark.parametrize("k", [5, 8])
def test_create_proof_bytes_match_oracle(gpu, k):
    """k = 5 is the reference's own size (examples/standard_plonk.rs:26).  Same witness, same seeded rng streams,
    same SRS: the device prover's proof bytes equal the oracle prover's, the oracle verifier accepts them, and
    rejects them after any single-bit change."""
    from halo2_scaffold_amd import circuits, prover

    params, vk, pk = _setup(gpu, k)
    xw, seed = 0xDEADBEEF12345, 77
    trace = {}
    proof = prover.create_proof(params, pk, circuits.StandardPlonk(xw), seed, trace=trace)
    opk = OP.ProvingKey(k, SRS_SECRET)
    want = OP.create_proof(opk, xw, seed)
    for name in ("theta", "beta", "gamma", "y", "x"):
        assert trace[name] == want["challenges"][name], name
    ws = trace["ws"]
    n = 1 << k
    assert [_vals(z, n) for z in ws.z] == want["zs"]
    assert _vals(ws.h, 2 * n) == want["h_coeffs"]
    assert _vals(ws.shplonk.h_x, n) == want["h_x"] and _vals(ws.shplonk.h2_x, n) == want["h2_x"]
    assert proof == want["proof"]
    assert len(proof) == 31 * 32  # 9 + 2 commitments, 20 evaluations
    assert OP.verify_proof(opk, proof)
    for pos in (3, 32 * 4 + 7, 32 * 9 + 1, 32 * 20, len(proof) - 5):
        bad = bytearray(proof)
        bad[pos] ^= 0x04
        assert not OP.verify_proof(opk, bytes(bad)), pos
    # a second proof through the same workspace (buffers reused) with another witness / seed
    proof2 = prover.create_proof(params, pk, circuits.StandardPlonk(12345), 5, ws=ws)
    assert proof2 == OP.create_proof(opk, 12345, 5)["proof"] and proof2 != proof
    ws.release()
    pk.release()
    params.release()


def test_device_proofs_equal_committed_golden_bytes(gpu):
    """tests/golden/standard_plonk_proofs.json (k = 5: the reference's own size; k = 8: BASELINE configs[0])"""
    import json
    import os

    from halo2_scaffold_amd import circuits, prover

    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "standard_plonk_proofs.json")))
    assert int(gold["srs_secret"], 16) == SRS_SECRET
    for case in gold["cases"]:
        params, vk, pk = _setup(gpu, case["k"])
        assert vk.to_bytes().hex() == case["vk_bytes"]
        proof = prover.create_proof(params, pk, circuits.StandardPlonk(int(case["witness_x"], 16)), case["seed"])
        assert proof.hex() == case["proof"]
        pk.release()
        params.release()


def test_unsatisfied_witness_is_rejected(gpu):
    """a witness that breaks the gate (c_1 != x^2) gives a quotient with a remainder: the oracle verifier rejects"""
    from halo2_scaffold_amd import circuits, prover

    k = 6
    params, vk, pk = _setup(gpu, k)

    class Broken(circuits.StandardPlonk):
        def synthesize(self):
            s = super().synthesize()
            s.advice[self.C_][1] = (s.advice[self.C_][1] + 1) % o.R
            return s

    good = prover.create_proof(params, pk, circuits.StandardPlonk(99), 3)
    bad = prover.create_proof(params, pk, Broken(99), 3)
    vkey = OP.VerifierKey(k, SRS_SECRET, o.unpack_points(vk.fixed_commitments), o.unpack_points(vk.permutation_commitments))
    assert OP.verify_proof(vkey, good) and not OP.verify_proof(vkey, bad)
    pk.release()
    params.release()


@pytest.mark.parametrize("k", [16, 20])
def test_create_proof_full_size_verifies_and_quotient_identity(gpu, k):
    """DEGREE = 16 (BASELINE configs[1]) and 20 (the headline size).  Size-independent checks:
      * the vk commitments equal the closed forms derived from the circuit definition (sparse columns);
      * the oracle verifier accepts the proof — every challenge re-derived from the bytes, gate and permutation
        expressions recomputed from the 20 opened evaluations, SHPLONK's final equation in G1 with the known s;
      * the quotient identity at a FRESH random point, every term evaluated by the device's eval_polynomial on the
        polynomials the prover left in HBM (advice, permutation products, fixed, sigma, the h pieces)."""
    from halo2_scaffold_amd import arithmetic  # noqa: F401
    from halo2_scaffold_amd import circuits, field as F, prover

    params, vk, pk = _setup(gpu, k)
    cf = OP.VerifierKey.closed_form(k, SRS_SECRET)
    assert o.unpack_points(vk.fixed_commitments) == cf.fixed_commitments
    assert o.unpack_points(vk.permutation_commitments) == cf.permutation_commitments
    assert vk.transcript_repr == cf.transcript_repr
    xw, seed = 0xABCDEF0123456789ABCDEF, 2024
    trace = {}
    proof = prover.create_proof(params, pk, circuits.StandardPlonk(xw), seed, trace=trace)
    assert OP.verify_proof(cf, proof)
    # ... and as the reference's verifier finishes: the pairing check over the SRS's two G2 elements, no secret involved
    # (the product's ParamsKZG carries exactly these two elements in its SRS file form)
    from oracle import formats as fm

    g2, s_g2 = fm.G2_GEN, fm.g2_mul(SRS_SECRET)
    assert params.g2_bytes == fm.g2_to_bytes(g2) and params.s_g2_bytes == fm.g2_to_bytes(s_g2)
    no_secret = OP.VerifierKey(k, None, o.unpack_points(vk.fixed_commitments), o.unpack_points(vk.permutation_commitments))
    assert OP.verify_proof(no_secret, proof, g2=g2, s_g2=s_g2)
    bad = bytearray(proof)
    bad[32 * 10 + 3] ^= 1  # an opened evaluation
    assert not OP.verify_proof(cf, bytes(bad))
    # ---- quotient identity at a fresh point, from the device-resident polynomials ----------------------------------
    ws = trace["ws"]
    n = 1 << k
    dom = o.Domain(k, P.CS_DEGREE)
    beta, gamma, y = trace["beta"], trace["gamma"], trace["y"]
    pt = 0x1F2E3D4C5B6A79881726354453627180FEDCBA % o.R
    out = gpu.DevBuf(32)

    def ev(buf, point, offset=0):
        pl = F.fr_to_mont_limbs(point)  # named: must outlive the call
        assert gpu.lib.h2mi_fr_eval_poly_dev(buf.ptr + offset * 32, n, pl.ctypes.data, out.ptr, None) == 0
        return o.unpack(out.to_numpy(shape=(1, 4)), o.R)[0]

    pt_next = pt * dom.omega % o.R
    pt_last = pt * pow(dom.omega, -(P.BLINDING_FACTORS + 1) % n, o.R) % o.R
    a = [ev(p, pt) for p in ws.advice_polys]
    f = [ev(p, pt) for p in pk.fixed.polys]
    s = [ev(p, pt) for p in pk.permutation.polys]
    z = [ev(p, pt) for p in ws.z_polys]
    z_next = [ev(p, pt_next) for p in ws.z_polys]
    z_last = [ev(p, pt_last) for p in ws.z_polys]
    ptn = pow(pt, n, o.R)
    li = lambda row: (ptn - 1) * pow(n, -1, o.R) % o.R * pow(dom.omega, row, o.R) % o.R * pow((pt - pow(dom.omega, row, o.R)) % o.R, -1, o.R) % o.R
    u = n - (P.BLINDING_FACTORS + 1)
    l0, l_last = li(0), li(u)
    l_active = (1 - l_last - sum(li(r) for r in range(u + 1, n))) % o.R
    v = (f[0] * a[0] + f[1] * a[1] + f[2] * a[2] + f[3] * a[0] * a[1] + f[4]) % o.R
    v = (v * y + (1 - z[0]) * l0) % o.R
    v = (v * y + (z[2] * z[2] - z[2]) * l_last) % o.R
    for m in (1, 2):
        v = (v * y + (z[m] - z_last[m - 1]) * l0) % o.R
    cur = beta * pt % o.R
    for m in range(3):
        left = z_next[m] * (a[m] + beta * s[m] + gamma) % o.R
        right = z[m] * (a[m] + cur + gamma) % o.R
        cur = cur * P.FR_DELTA % o.R
        v = (v * y + (left - right) * l_active) % o.R
    hx = (ev(ws.h, pt) + ptn * ev(ws.h, pt, offset=n)) % o.R  # h = h_0 + X^n h_1
    assert v == hx * (ptn - 1) % o.R
    # the witness really sits in the committed column: a(omega^1) = x, c(omega^2) = x^2 + 72
    assert _vals(ws.advice[0], 3) == [xw % o.R] * 3
    assert o.unpack(ws.advice[2].to_numpy(shape=(3, 4), nbytes=96), o.R)[2] == (xw * xw + 72) % o.R
    out.free()
    ws.release()
    pk.release()
    params.release()


@pytest.mark.parametrize("k,m,chunk", [(6, 3, 1), (9, 4, 2), (11, 5, 2), (12, 8, 3)])
def test_permutation_products_all_sets_match_formula(gpu, k, m, chunk):
    """h2mi_plonk_permutation_products_dev: every set of a permutation argument in one pass (m columns chunked by
    cs.degree() - 2, sets chained through their last value) against the row-by-row big-integer construction of
    plonk/permutation/prover.rs; blinding rows stay as the caller left them.  (9, 4, 2) is the range-lookup shape."""
    from halo2_scaffold_amd import plonk as gp

    n = 1 << k
    u = n - 6
    w = o.omega_for(k)
    wp = [pow(w, i, o.R) for i in range(n)]
    rng = np.random.default_rng(k)
    vals = [o.unpack(o.random_field_limbs(n, 300 + j), o.R) for j in range(m)]
    # a real permutation: a few transpositions between cells of the columns on top of the identity
    ident = lambda j, i: pow(P.FR_DELTA, j, o.R) * wp[i] % o.R
    sig = [[ident(j, i) for i in range(n)] for j in range(m)]
    for _ in range(20):
        (j1, i1), (j2, i2) = [(int(rng.integers(m)), int(rng.integers(u))) for _ in range(2)]
        sig[j1][i1], sig[j2][i2] = sig[j2][i2], sig[j1][i1]
        vals[j2][i2] = vals[j1][i1]  # equal cells, so the product still telescopes where it should
    beta, gamma = 0xBEEF + k, 0xCAFE
    sets = -(-m // chunk)
    want = perm_scale_cases.formula_products(k, u, chunk, vals, sig, beta, gamma, sentinel=0xDEAD)  # row by row, 0xDEAD beyond row u
    assert len(want) == sets
    dv = [gpu.DevBuf.from_numpy(o.pack(v, o.R)) for v in vals]
    ds = [gpu.DevBuf.from_numpy(o.pack(v, o.R)) for v in sig]
    dz = [gpu.DevBuf.from_numpy(o.pack([0xDEAD] * n, o.R)) for _ in range(sets)]
    gp.permutation_products(k, dv, ds, chunk, beta, gamma, u, dz)
    for s in range(sets):
        assert _vals(dz[s], n) == want[s], s
    # the sparse form (h2mi_plonk_permutation_products_sparse_dev): the support of the permutation handed over as keygen
    # knows it — here read off sigma — gives the same columns from the ~40 constrained rows alone
    mapping = {(j, i): None for j in range(m) for i in range(u) if sig[j][i] != ident(j, i)}
    active = gp.ActiveRows(mapping, chunk, u)
    assert 0 < active.count <= 40
    for b in dz:
        b.upload(o.pack([0xDEAD] * n, o.R))
    gp.permutation_products(k, dv, ds, chunk, beta, gamma, u, dz, active=active)
    for s in range(sets):
        assert _vals(dz[s], n) == want[s], s
    active.free()
    # no constrained row at all (identity permutation): every product is one on rows 0 .. u, the rest untouched
    di = [gpu.DevBuf.from_numpy(o.pack([ident(j, i) for i in range(n)], o.R)) for j in range(m)]
    empty = gp.ActiveRows({}, chunk, u)
    assert empty.count == 0
    for b in dz:
        b.upload(o.pack([0xDEAD] * n, o.R))
    gp.permutation_products(k, dv, di, chunk, beta, gamma, u, dz, active=empty)
    for s in range(sets):
        assert _vals(dz[s], n) == [1] * (u + 1) + [0xDEAD] * (n - u - 1), s
    empty.free()
    for b in dv + ds + dz + di:
        b.free()


def test_eval_polys_batched_matches_oracle(gpu):
    import ctypes as C

    from halo2_scaffold_amd import field as F

    for n, count in [(1, 1), (300, 5), (1 << 13, 24), (70001, 3)]:
        polys = [o.random_field_limbs(n, 900 + i) for i in range(count)]
        bufs = [gpu.DevBuf.from_numpy(p) for p in polys]
        out = gpu.DevBuf(32 * count)
        pt = 0x123456789ABCDEF0FEDCBA987654321 % o.R
        ptl = F.fr_to_mont_limbs(pt)
        ptrs = (C.c_void_p * count)(*[b.ptr for b in bufs])
        assert gpu.lib.h2mi_fr_eval_polys_dev(ptrs, count, n, ptl.ctypes.data, out.ptr, None) == 0
        got = _vals(out, count)
        assert got == [o.eval_polynomial(o.unpack(p, o.R), pt) for p in polys]
        for b in bufs + [out]:
            b.free()
    assert gpu.lib.h2mi_fr_eval_polys_dev(None, 1, 4, None, None, None) == -1


@pytest.mark.parametrize("n,m", [(64, 2), (1000, 3), (1 << 13, 4), (70001, 4), ((1 << 19) + 5, 2)])  # the last: split tables with >= 1024 low entries, a partial last tile
def test_kate_division_multi_matches_chained_divisions(gpu, n, m):
    """h2mi_fr_kate_division_multi_dev: N / prod (X - r_i) in one round (partial fractions over independent divisions) equals
    the oracle's chain of kate_division calls — what SHPLONK's div_by_vanishing computes — coefficient for coefficient,
    including the exact zeros at the top."""
    from halo2_scaffold_amd import field as F

    rng = np.random.default_rng(n + m)
    roots = [int.from_bytes(rng.bytes(32), "little") % o.R for _ in range(m)]
    quot = o.unpack(o.random_field_limbs(n - m, 77 + n), o.R)
    num = quot
    for r in roots:  # N = Q * prod (X - r)
        nxt = [0] * (len(num) + 1)
        for i, c in enumerate(num):
            nxt[i + 1] = (nxt[i + 1] + c) % o.R
            nxt[i] = (nxt[i] - c * r) % o.R
        num = nxt
    assert len(num) == n
    want = num
    for r in roots:
        want = o.kate_division(want, r)
    assert want == quot
    d_in = gpu.DevBuf.from_numpy(o.pack(num, o.R))
    d_out = gpu.DevBuf.from_numpy(o.pack([0xBAD] * n, o.R))
    weights = []
    for i, r in enumerate(roots):
        d = 1
        for k, rk in enumerate(roots):
            if k != i:
                d = d * (r - rk) % o.R
        weights.append(pow(d, -1, o.R))
    rl = np.ascontiguousarray(np.stack([F.fr_to_mont_limbs(r) for r in roots]))
    ri = np.ascontiguousarray(np.stack([F.fr_to_mont_limbs(pow(r, -1, o.R)) for r in roots]))
    wl = np.ascontiguousarray(np.stack([F.fr_to_mont_limbs(w) for w in weights]))
    assert gpu.lib.h2mi_fr_kate_division_multi_dev(d_in.ptr, n, rl.ctypes.data, ri.ctypes.data, wl.ctypes.data, m, d_out.ptr, None) == 0
    got = _vals(d_out, n)
    assert got[: n - m] == quot and got[n - m : n - 1] == [0] * (m - 1) and got[n - 1] == 0xBAD  # the last slot is not written
    assert gpu.lib.h2mi_fr_kate_division_multi_dev(d_in.ptr, n, rl.ctypes.data, ri.ctypes.data, wl.ctypes.data, 5, d_out.ptr, None) == -1
    d_in.free()
    d_out.free()


@pytest.mark.parametrize("k,degree,count", [(5, 3, 1), (6, 5, 3), (7, 3, 16), (6, 5, 0)])
def test_instance_coset_matches_transforms(gpu, k, degree, count):
    """h2mi_plonk_instance_coset_dev: the extended-coset form of an instance column holding `count` public inputs, formed from
    l_0's coset (sum_r v_r * l0_coset[(j - r rot) mod 2^ext_k]), equals coeff_to_extended(lagrange_to_coeff(column)) of the
    oracle's EvaluationDomain value for value."""
    from halo2_scaffold_amd import field as F

    d = o.Domain(k, degree)
    n, ext = 1 << k, 1 << d.extended_k
    l0 = d.coeff_to_extended(d.lagrange_to_coeff([1] + [0] * (n - 1)))
    vals = o.unpack(o.random_field_limbs(max(count, 1), 321 + k), o.R)[:count]
    want = d.coeff_to_extended(d.lagrange_to_coeff(vals + [0] * (n - count)))
    d_l0 = gpu.DevBuf.from_numpy(o.pack(l0, o.R))
    d_out = gpu.DevBuf(ext * 32)
    vl = np.ascontiguousarray(np.stack([F.fr_to_mont_limbs(v) for v in vals])) if count else np.zeros((1, 4), dtype=np.uint64)
    assert gpu.lib.h2mi_plonk_instance_coset_dev(d_l0.ptr, k, d.extended_k, vl.ctypes.data, count, d_out.ptr, None) == 0
    assert _vals(d_out, ext) == want
    assert gpu.lib.h2mi_plonk_instance_coset_dev(d_l0.ptr, k, d.extended_k, vl.ctypes.data, 17, d_out.ptr, None) == -1
    d_l0.free()
    d_out.free()


def test_lookup_product_sparse_equals_dense(gpu):
    """the lookup grand product over the flagged rows only (rows whose ratio differs from one) against the dense form of the
    same call (the library has no switch that forces the dense form: instead both are compared with the oracle's row-by-row
    product) at a size where the sparse form is taken: k = 13, a range-check-like input (a handful of limbs,
    zeros elsewhere) in a 2^8-row table."""
    from halo2_scaffold_amd import plonk as gp
    from oracle import lookup as L

    k, bits = 13, 8
    n = 1 << k
    u = n - 7
    inputs = [0] * u
    for i, v in enumerate([3, 200, 255, 17, 17, 0, 99]):
        inputs[5 + 3 * i] = v
    table = list(range(1 << bits)) + [0] * (u - (1 << bits))
    blind = o.unpack(o.random_field_limbs(14, 5), o.R)
    a_perm, s_perm = L.permute_expression_pair(inputs, table, u, blind[:7], blind[7:])
    beta, gamma = 0x1234567 % o.R, 0x7654321 % o.R
    want = L.lookup_product(inputs, table, a_perm, s_perm, beta, gamma, u, o.unpack(o.random_field_limbs(6, 9), o.R))
    pad = lambda col: gpu.DevBuf.from_numpy(o.pack(list(col) + [0] * (n - len(col)), o.R))
    d_in, d_tab, d_ap, d_sp = pad(inputs), pad(table), pad(a_perm), pad(s_perm)
    d_z = gpu.DevBuf.from_numpy(o.pack([0xDEAD] * n, o.R))
    gp.lookup_product(k, d_in, d_tab, d_ap, d_sp, beta, gamma, u, d_z)
    got = _vals(d_z, n)
    assert got[: u + 1] == want[: u + 1]           # z_0 .. z_u; the blinding rows are the caller's
    assert got[u + 1 :] == [0xDEAD] * (n - u - 1)
    changes = sum(1 for i in range(u) if want[i + 1] != want[i])
    assert 0 < changes <= 2 * (1 << bits) + 16       # the product moves on a few hundred of 8185 rows: the sparse form was taken
    for b in (d_in, d_tab, d_ap, d_sp, d_z):
        b.free()
