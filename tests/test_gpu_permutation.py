"""GPU tests of the permutation argument's grand products (csrc/h2mi_plonk.hip perm_products) in every regime and at
scale, on the cases of tests/perm_scale_cases.py (checked on the CPU by tests/test_perm_scale_host.py): the one-workgroup form of a
short position list, the general sparse form over one and several tiles, the dense form up to 1279 tiles (k_mulscan_offsets with runs
of two tiles), 64 columns by value, one set, the usable-row extremes; the single-set entry chained across a tile; and whole proofs
whose keys take each form.  Which form ran is read from the library's launch profile, so that a case cannot pass through another
branch.  Every comparison is exact: integers, rows and bytes."""
import ctypes as C
import re
import types

import numpy as np
import pytest

import check_cases
import custom_gate_cases as gate_cases
import perm_scale_cases as scale
import phase_cases
from oracle import flex as FX

pytestmark = pytest.mark.gpu

SRS_SECRET = 0x5EC2E7 + 0x48324D49
PROFILED = ("k_perm_sparse_small", "k_mulscan_local", "k_perm_to_mont256", "k_mulscan_offsets", "k_perm_numden_sets")


def _launches(gpu, call, names=PROFILED) -> dict:
    """kernel -> launches during call(), from the library's launch profile (a name is matched as a prefix: the ones asked for here
    are the prefix of no other kernel)"""
    lib = gpu.lib
    assert lib.h2mi_profile_reset() == 0 and lib.h2mi_profile_filter(b"") == 0 and lib.h2mi_profile_enable(1) == 0
    try:
        call()
    finally:
        assert lib.h2mi_profile_enable(0) == 0
    ms, count = C.c_double(), C.c_uint64()
    out = {}
    for name in names + ("",):
        assert lib.h2mi_profile_query(name.encode(), C.byref(ms), C.byref(count)) == 0
        out[name] = count.value
    assert lib.h2mi_profile_reset() == 0
    assert out.pop("") > 0  # the profile did record this call's launches
    return out


def _assert_form(launches: dict, want: dict, what: str):
    print(what, launches)
    assert {name: launches[name] for name in want} == want, what


def _upload(gpu, column):
    return gpu.DevBuf.from_numpy(column if isinstance(column, np.ndarray) else scale.mont_limbs(column))


def _assert_sets(bufs, want, what):
    """every buffer's bytes == the Montgomery form of its column in `want`; a mismatch names the first differing set and row"""
    for s, (buf, column) in enumerate(zip(bufs, want)):
        got = buf.to_numpy(shape=(len(column), 4), nbytes=len(column) * 32)
        if np.array_equal(got, scale.mont_limbs(column)):
            continue
        values = scale.from_mont_limbs(got)
        rows = [r for r in range(len(column)) if values[r] != column[r]]
        assert not rows, f"{what}: set {s}: {len(rows)} rows differ, the first at row {rows[0]}: {values[rows[0]]:#x} != {column[rows[0]]:#x}"
        raise AssertionError(f"{what}: set {s}: equal as field elements, but not in the canonical Montgomery form")


def _active_rows(gp, case):
    """plonk.ActiveRows from sigma's support, as keygen hands it over; the positions are the case's list"""
    ident = scale.identity(case.k, case.m)
    mapping = {(j, i): None for j in range(case.m) for i in range(case.u) if case.sig[j][i] != ident[j][i]}
    active = gp.ActiveRows(mapping, case.chunk, case.u)
    assert active.count == len(case.active) and active.buf.to_numpy(dtype=np.uint32, nbytes=4 * active.count).tolist() == case.active
    return active


@pytest.mark.parametrize("name", list(scale.PRODUCT_CASES), ids=[re.sub(r"[^A-Za-z0-9]+", "_", name).strip("_") for name in scale.PRODUCT_CASES])
def test_permutation_products_every_regime(gpu, name):
    """plonk.permutation_products on the cases of tests/perm_scale_cases.py.  Up to k = 13 rows 0 .. u of every set against the
    row-by-row big-integer construction, the rows beyond u untouched; the case of 1279 tiles against the recurrence (z_0[0] = 1,
    z_s[i + 1] den = z_s[i] num, z_(s+1)[0] = z_s[u], no denominator zero: the same statement as equality).  Position lists of 1, 2,
    63 .. 256 entries take k_perm_sparse_small, 257 .. 2046 the general sparse form (k_mulscan_offsets from 1025 on), 2047 — over an
    eighth of the positions — falls back to the dense form in the wrapper; the lists hold both ends of both sets, adjacent rows and
    one row in both sets."""
    from halo2_scaffold_amd import plonk as gp

    case = scale.product_case(name)
    n, u = case.n, case.u
    dv, ds = [_upload(gpu, c) for c in case.vals], [_upload(gpu, c) for c in case.sig]
    dz = [_upload(gpu, [scale.SENTINEL] * n) for _ in range(case.sets)]
    active = _active_rows(gp, case) if case.active is not None else None
    launches = _launches(gpu, lambda: gp.permutation_products(case.k, dv, ds, case.chunk, case.beta, case.gamma, u, dz, active=active))
    if case.big:
        zs = [z.to_numpy(shape=(n, 4), nbytes=n * 32) for z in dz]
        assert scale.recurrence_violation(case, zs) is None
        sentinel = scale.mont_limbs([scale.SENTINEL])[0]
        assert all((z[u + 1 :] == sentinel).all() for z in zs)  # the rows beyond u are the caller's
    else:
        want = scale.formula_products(case.k, u, case.chunk, case.vals, case.sig, case.beta, case.gamma)
        assert (want[-1][u] == 1) == case.real
        _assert_sets(dz, want, name)
    _assert_form(launches, scale.expected_launches(case), name)
    if active is not None:
        active.free()
    for b in dv + ds + dz:
        b.free()


def test_single_set_entry_chains_across_a_tile(gpu):
    """h2mi_plonk_permutation_product_dev (one set per call, chained by the caller through `last` -> `start`) shares the scans: 1025
    usable rows at k = 11, so that both sets run over two tiles and row 1025 lies in the second"""
    from halo2_scaffold_amd import plonk as gp

    case = scale.single_set_case()
    k, n, u, chunk = case.k, case.n, case.u, case.chunk
    want = scale.formula_products(k, u, chunk, case.vals, case.sig, case.beta, case.gamma)
    dv, ds = [_upload(gpu, c) for c in case.vals], [_upload(gpu, c) for c in case.sig]
    dz = [_upload(gpu, [scale.SENTINEL] * n) for _ in range(case.sets)]
    carry = [_upload(gpu, [scale.SENTINEL]) for _ in range(case.sets)]

    def run():
        for s in range(case.sets):
            cols = list(range(s * chunk, min(case.m, (s + 1) * chunk)))
            gp.permutation_product(k, [dv[j] for j in cols], [ds[j] for j in cols], cols, case.beta, case.gamma, u, dz[s],
                                   d_start=carry[s - 1] if s else None, d_last=carry[s])

    launches = _launches(gpu, run, ("k_perm_numden", "k_mulscan_local", "k_mulscan_offsets", "k_perm_sparse_small"))
    _assert_sets(dz, want, "single-set entry")
    _assert_sets(carry, [[z[u]] for z in want], "the value handed to the next set")
    _assert_form(launches, {"k_perm_numden": 2, "k_mulscan_local": 6, "k_mulscan_offsets": 6, "k_perm_sparse_small": 0}, "single-set entry")
    for b in dv + ds + dz + carry:
        b.free()


@pytest.mark.parametrize("k,cycles", list(scale.PROOF_CASES), ids=[f"k{k}-{c}_cycles" for k, c in scale.PROOF_CASES])
def test_copies_proofs_take_every_permutation_form(gpu, k, cycles):
    """check_cases.copies_circuit through custom.create_proof: keygen's position list (203, 275, 1019, 1022, 2283 positions) and the
    prover's rule n_active * 8 <= n_sets * usable_rows pick the small, the general sparse (one tile, the last count under the rule,
    three tiles) and the dense form.  The oracle's verifier accepts the proof and rejects that of a witness with one cell of a cycle
    changed; the prover's product columns equal the row-by-row formula evaluated on the device's own columns."""
    from halo2_scaffold_amd import custom, engine

    n_active, form = scale.PROOF_CASES[(k, cycles)]
    cs, asg, _ = check_cases.copies_circuit(custom, k, cycles)
    positions, u, sets, chunk = scale.proof_positions(cs, asg, k)
    assert len(positions) == n_active and (sets, chunk) == (4, 1)
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    keys = custom.Keys(params, cs, asg)
    ws = custom.Workspace(params, keys)
    trace, proofs = {}, []
    launches = _launches(gpu, lambda: proofs.append(custom.create_proof(params, keys, asg, 31, trace=trace, ws=ws)))
    # the product columns, from what the device holds
    n = 1 << k
    ints = lambda view: scale.from_mont_limbs(view.to_numpy(shape=(n, 4), nbytes=n * 32))
    advice = [ints(v) for v in ws.prover.views(engine.BUF_ADVICE, cs.n_advice)]
    columns = {"advice": advice, "fixed": [ints(v) for v in keys.fixed_values], "instance": [ints(ws.prover.view(engine.BUF_INSTANCE))]}
    vals = [columns[kind][c] for kind, c in cs.perm_columns]
    sig = [ints(v) for v in keys.sigma_values]
    ident = scale.identity(k, len(sig))
    assert sorted({(j // chunk) * u + i for j in range(len(sig)) for i in range(u) if sig[j][i] != ident[j][i]}) == positions  # keygen's sigma
    want = scale.formula_products(k, u, chunk, vals, sig, trace["beta"], trace["gamma"], ident)
    assert want[-1][u] == 1 and sum(z[i + 1] != z[i] for z in want for i in range(u)) == n_active
    _assert_sets(ws.prover.views(engine.BUF_PERM_Z, sets), [z[: u + 1] for z in want], f"z of ({k}, {cycles})")
    _assert_form(launches, scale.expected_launches(types.SimpleNamespace(form=form, active=positions, sets=sets, u=u)), f"({k}, {cycles})")
    # the verifier
    ocs = gate_cases.oracle_cs(cs, "copies")
    oasg = gate_cases.oracle_assignment(ocs, asg)
    vk = FX.VerifierKeys(ocs, k, SRS_SECRET, oasg.fixed, oasg.copies)
    assert keys.transcript_repr == vk.transcript_repr
    assert phase_cases.verify_circuit(vk, cs, proofs[0], oasg.instance)
    _, bad, members = check_cases.copies_circuit(custom, k, cycles, change=(cycles - 3, 1))
    assert bad.instance == asg.instance and sum(bad.advice[c] != asg.advice[c] for c in range(cs.n_advice)) == 1 and len(members) >= 3
    assert not phase_cases.verify_circuit(vk, cs, custom.create_proof(params, keys, bad, 31, ws=ws), oasg.instance)
    ws.release()
    keys.release()
    params.release()


CENSUS = ("k_shuffle_numden", "k_lookup_numden", "k_lookup_flag", "k_logup_numden", "k_logup_numden_sets", "k_mulscan_local", "k_mulscan_offsets",
          "k_mulscan_apply", "k_fr_inv_one", "k_perm_ratio", "k_perm_write_sets", "k_addscan_local", "k_addscan_offsets", "k_addscan_apply")


@pytest.mark.parametrize("k,u", [(5, 22), (11, 1025)], ids=["one_tile", "two_tiles"])
def test_single_output_entries_launch_census(gpu, k, u):
    """The launches of the four entries with one output (shuffle product, dense lookup product, logUp sum of one set and of three) over
    one scan tile of 1024 rows and over two: the fractions-to-ratios block they share (two multiplicative scans, one inversion, the
    ratios), then a third multiplicative scan and the write, or for logUp the additive scan.  The values are arbitrary and nonzero
    (tests/test_gpu_shuffle.py, test_gpu_lookup.py, test_gpu_logup.py and test_gpu_logup_sets.py check values); a lookup product
    below 4096 rows flags nothing.  Names are matched as prefixes: k_logup_numden counts k_logup_numden_sets too, hence the difference."""
    from halo2_scaffold_amd import plonk as gp

    n, more = 1 << k, int(u > 1024)  # beyond one tile every scan adds its offsets pass, the multiplicative ones an apply pass as well
    cols = [_upload(gpu, [c * n + i + 1 for i in range(n)]) for c in range(4)]
    three = _upload(gpu, [7 * n + i for i in range(3 * n)])
    out = _upload(gpu, [scale.SENTINEL] * n)
    shared = {"k_fr_inv_one": 1, "k_perm_ratio": 1, "k_lookup_flag": 0}
    product = dict(shared, k_mulscan_local=3, k_mulscan_offsets=3 * more, k_mulscan_apply=3 * more, k_perm_write_sets=1, k_addscan_local=0,
                   k_addscan_offsets=0, k_addscan_apply=0, k_logup_numden=0, k_logup_numden_sets=0)
    running_sum = dict(shared, k_mulscan_local=2, k_mulscan_offsets=2 * more, k_mulscan_apply=2 * more, k_perm_write_sets=0, k_addscan_local=1,
                       k_addscan_offsets=more, k_addscan_apply=1, k_shuffle_numden=0, k_lookup_numden=0)
    entries = {
        "shuffle product": (lambda: gp.shuffle_product(k, cols[0], cols[1], 5, u, out), dict(product, k_shuffle_numden=1, k_lookup_numden=0)),
        "lookup product": (lambda: gp.lookup_product(k, cols[0], cols[1], cols[2], cols[3], 5, 9, u, out), dict(product, k_shuffle_numden=0, k_lookup_numden=1)),
        "logUp sum, one set": (lambda: gp.logup_sum(k, cols[0], cols[1], cols[2], 5, u, out), dict(running_sum, k_logup_numden=1, k_logup_numden_sets=0)),
        "logUp sum, three sets": (lambda: gp.logup_sum_sets(k, three, 3, cols[1], cols[2], 5, u, out), dict(running_sum, k_logup_numden=0, k_logup_numden_sets=1)),
    }
    for what, (call, want) in entries.items():
        launches = _launches(gpu, call, CENSUS)
        launches["k_logup_numden"] -= launches["k_logup_numden_sets"]
        _assert_form(launches, want, f"{what}, (k, u) = ({k}, {u})")
    for b in cols + [three, out]:
        b.free()
