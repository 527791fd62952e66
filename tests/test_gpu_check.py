"""The witness check on the device.  Level A: h2mi_plonk_expr_check_dev on the planted programs and the redundant zeros of
tests/check_cases.py (counts and first rows exactly), its refusals, and the copy / membership calls on small vectors.  Level B:
h2mi_prover_check through custom.check / flex.check / engine.Prover.check on circuits given as data, the hard-wired shapes, copy
constraints beyond one workgroup, a gate left on over the blinding rows; that a proof's bytes do not depend on the call; when the
call is refused.  Every comparison is exact: integers and rows."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

import check_cases as cases
import custom_gate_cases as gate_cases
import phase_cases
from custom_gate_cases import OP_ADVICE, OP_END, OP_FIXED
from oracle import bn254 as o
from oracle import flex as FX

pytestmark = pytest.mark.gpu

R = o.R
SRS_SECRET = 0x5EC2E7 + 0x48324D49
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EINVAL, ERANGE, EUNSAT = -1, -6, -7
GATE, COPY, LOOKUP, NONE = cases.GATE, cases.COPY, cases.LOOKUP, cases.NONE


# ---- level A ---------------------------------------------------------------------------------------------------------------------------
def _run_case(case):
    from halo2_scaffold_amd import engine, plonk
    from halo2_scaffold_amd.device import DevBuf

    bufs = {key: DevBuf.from_numpy(o.pack(col, R)) for key, col in case["data"].items()}
    cols = lambda kind: [bufs[(kind, j)] for j in range(1 + max([j for kd, j in bufs if kd == kind], default=-1))]
    prog = engine.GateProgram.build(case["ops"], case["consts"])
    inst = bufs.get(("instance", 0))
    got = plonk.expr_check(prog, cols("advice"), cols("fixed"), inst, case["k"], case["n_rows"], challenges=case["challenges"])
    print(case["k"], case["n_rows"], got)
    return got


@pytest.mark.parametrize("k", [4, 6, 8, 9, 11])  # a partial wavefront, one wavefront, one workgroup, two workgroups, eight workgroups
def test_planted_polynomials(gpu, k):
    from halo2_scaffold_amd import custom

    n = 1 << k
    for n_rows in (n, n - 6):
        case = cases.planted_case(custom, k, 0, n_rows=n_rows)
        assert {2, 8} <= set(case["depths"])
        assert _run_case(case) == case["want"]


def test_many_polynomials_in_one_program(gpu):
    from halo2_scaffold_amd import custom

    case = cases.many_polynomials_case(custom)
    assert len(case["want"]) >= 40 and case["k"] == 9
    assert _run_case(case) == case["want"]


def test_redundant_zeros(gpu):
    """values the kernel holds as unreduced multiples of r, or as r itself, are zero"""
    case = cases.redundant_zero_case()
    assert _run_case(case) == [(0, NONE)] * 8
    # and the same columns do fail a polynomial that is not zero: a - a + 1, (r - 1) + 2
    case["ops"] = [(OP_ADVICE, 0, 0), (OP_ADVICE, 0, 0), (cases.OP_SUB, 0, 0), (cases.OP_CONSTANT, 9, 0), (cases.OP_ADD, 0, 0), (OP_END, 0, 0),
                   (OP_ADVICE, 2, 0), (cases.OP_CONSTANT, 9, 0), (cases.OP_ADD, 0, 0), (cases.OP_CONSTANT, 9, 0), (cases.OP_ADD, 0, 0), (OP_END, 0, 0)]
    n = 1 << case["k"]
    assert _run_case(case) == [(n, 0), (n, 0)]


def test_expr_check_refusals(gpu):
    """the refusals of h2mi_plonk_expr_check_dev, and n_rows outside [1, 2^k]"""
    from halo2_scaffold_amd import engine, plonk
    from halo2_scaffold_amd.device import DevBuf

    col = DevBuf(32 * 32)
    cols = (C.c_void_p * 1)(col.ptr)
    inst = plonk._InstanceCosets(1)  # one instance column, which the programs do not read: {1, {NULL}}
    report = np.zeros((4, 2), dtype=np.uint32)
    ch = np.zeros((17, 4), dtype=np.uint64)
    OP_CHALLENGE = phase_cases.OP_CHALLENGE

    def call(ops, k=5, n_rows=32, n_adv=1, challenges=0, out=report.ctypes.data):
        prog = engine.GateProgram.build(ops, [])
        rec = plonk.ExprColumns(C.addressof(cols), n_adv, None, 0, C.addressof(inst), C.addressof(prog), ch.ctypes.data if challenges else None,
                                challenges, k)
        return gpu.lib.h2mi_plonk_expr_check_dev(C.byref(rec), n_rows, out, None, None)

    ok = [(OP_ADVICE, 0, 0), (OP_END, 0, 0)]
    assert call(ok) == 0
    assert call([(OP_ADVICE, 1, 0), (OP_END, 0, 0)]) == EINVAL     # a column that is not there
    assert call([(OP_FIXED, 0, 0), (OP_END, 0, 0)]) == EINVAL
    assert call([(OP_ADVICE, 0, 32), (OP_END, 0, 0)]) == EINVAL    # a rotation of 2^k
    assert call([(OP_ADVICE, 0, 0)]) == EINVAL                     # no END
    assert call([(OP_CHALLENGE, 0, 0), (OP_END, 0, 0)]) == EINVAL  # a challenge the launch does not have
    assert call([(OP_CHALLENGE, 1, 0), (OP_END, 0, 0)], challenges=1) == EINVAL
    assert call([(OP_CHALLENGE, 0, 0), (OP_END, 0, 0)], challenges=17) == EINVAL
    assert call([(OP_CHALLENGE, 0, 0), (OP_END, 0, 0)], challenges=1) == 0
    assert call(ok, out=None) == EINVAL
    assert call(ok, n_rows=0) == ERANGE and call(ok, n_rows=33) == ERANGE and call(ok, k=0, n_rows=1) == ERANGE and call(ok, k=29) == ERANGE


@pytest.mark.parametrize("count", [5, 64, 700])
def test_copy_and_membership_calls(gpu, count):
    """h2mi_plonk_copy_check_dev and h2mi_plonk_lookup_member_dev on small vectors: nothing to report, then two planted cells / rows
    (for 700: in different workgroups)"""
    from halo2_scaffold_amd import plonk
    from halo2_scaffold_amd.device import DevBuf

    rng = random.Random(count)
    a = [rng.randrange(R) for _ in range(count)]
    b = list(a)
    cells = [(0, i, 1, i) for i in range(count)] + [(1, i, 0, i) for i in range(count)]  # a_i -> b_i -> a_i, sorted by (column, row)
    d_cells = DevBuf.from_numpy(np.array(cells, dtype=np.uint32))
    bufs = lambda: [DevBuf.from_numpy(o.pack(col, R)) for col in (a, b)]
    assert plonk.copy_check(bufs(), d_cells, len(cells)) == (0, NONE)
    planted = sorted({count // 2, count - 1})
    for i in planted:
        b[i] = (b[i] + 1) % R
    assert plonk.copy_check(bufs(), d_cells, len(cells)) == (2 * len(planted), planted[0])
    table = sorted(set(rng.randrange(R) for _ in range(max(count // 2, 2))) | {0})
    inputs = [rng.choice(table) for _ in range(count)]
    sorted_buf = DevBuf.from_numpy(o.pack(table))  # canonical words
    run = lambda: plonk.lookup_member(DevBuf.from_numpy(o.pack(inputs, R)), sorted_buf, len(table), count)
    assert run() == (0, NONE)
    for i in planted:
        inputs[i] = next(v for v in range(1, 1000) if v not in table)
    assert run() == (len(planted), planted[0])


# ---- level B ---------------------------------------------------------------------------------------------------------------------------
def _release(params, keys, ws):
    ws.release()
    keys.release()
    params.release()


def _same(failures, report, perm_columns):
    """the device's failures against the host's report: GATE and LOOKUP entries exactly, the COPY entry a cell of an unequal constraint"""
    print([f.astuple() for f in failures], report)
    assert len(failures) == len(report)
    for f, want in zip(failures, report):
        if want[0] == COPY:
            kind, column = perm_columns[f.index]
            assert f.kind == COPY and (kind, column, f.row) in want[1] and f.count >= 1
        else:
            assert f.astuple() == want


def _raises(check, first):
    with pytest.raises(ValueError) as e:
        check()
    assert str(e.value).startswith(first), (str(e.value), first)
    return e.value.failures


@pytest.mark.parametrize("name", sorted(cases.DATA_CIRCUITS))
def test_circuits_as_data(gpu, name):
    from halo2_scaffold_amd import custom

    k, build, broken = cases.DATA_CIRCUITS[name]
    cs, good = build(custom)
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    keys = custom.Keys(params, cs, good)
    ws = custom.Workspace(params, keys)
    custom.check(params, keys, good, 3, ws=ws)
    bad = broken(custom)
    report = cases.host_report(bad, k)
    failures = _raises(lambda: custom.check(params, keys, bad, 3, ws=ws), cases.first_violation(report, cs))
    _same(failures, report, cs.perm_columns)
    custom.check(params, keys, good, 4, ws=ws)  # the prover goes on
    assert ws.prover.check is not None and custom.check(params, keys, good, 4) is None  # and a workspace of the call's own
    _release(params, keys, ws)


@pytest.mark.parametrize("name", ["rlc", "three"])
def test_phase_circuits(gpu, name):
    """a phase-1 witness made with a wrong challenge: the gate that reads it (rlc), the gate and the lookup (three) — where the
    lookups phase itself then returns H2MI_EUNSAT"""
    from halo2_scaffold_amd import custom

    build, k = phase_cases.CIRCUITS[name]
    cs, synthesize = build(custom)
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    keys = custom.Keys(params, cs, synthesize([None] * len(cs.challenge_phase)))
    ws = custom.Workspace(params, keys)
    custom.check(params, keys, synthesize, 9, ws=ws)
    _, wrong = build(custom, 1)
    trace = {}
    with pytest.raises(ValueError) as e:
        custom.check(params, keys, wrong, 9, ws=ws, trace=trace)
    ch = trace["challenges"]
    report = cases.host_report(wrong(ch), k, ch)
    assert str(e.value).startswith(cases.first_violation(report, cs))
    _same(e.value.failures, report, cs.perm_columns)
    if name == "three":
        assert [f.kind for f in e.value.failures] == [GATE, LOOKUP]
        with pytest.raises(ValueError, match="ConstraintSystemFailure"):
            custom.create_proof(params, keys, wrong, 9, ws=ws)
    custom.check(params, keys, synthesize, 9, ws=ws)
    _release(params, keys, ws)


def test_older_shapes(gpu):
    """the halo2-lib shapes through the shape's program: halo2_lib, range in one column (q_lookup a) and over several (lookup-advice
    columns), a broken gate in gate column 1, a looked-up 2^LOOKUP_BITS; at k = 11 the membership kernel takes eight workgroups"""
    from halo2_scaffold_amd import flex

    for name, (k, cs, good, bad) in cases.flex_cases(flex).items():
        params = gpu.ParamsKZG.setup(k, SRS_SECRET)
        keys = flex.FlexKeys(params, cs, good)
        ws = flex.FlexWorkspace(params, keys)
        flex.check(params, keys, good, 5, ws=ws)
        report = cases.flex_host_report(bad, k)
        failures = _raises(lambda: flex.check(params, keys, bad, 5, ws=ws), cases.first_violation(report, cs, flex_shape=True))
        _same(failures, report, cs.perm_columns)
        if name.startswith("limbs"):  # nothing but the lookup is wrong, and the prover's lookups phase says so too
            assert [f.kind for f in failures] == [LOOKUP]
            with pytest.raises(ValueError, match="not in the table"):
                flex.create_proof(params, keys, bad, 5, ws=ws)
        _release(params, keys, ws)


def test_standard_plonk(gpu):
    from halo2_scaffold_amd import circuits, keygen, prover
    from halo2_scaffold_amd.transcript import Blake2bWrite

    params = gpu.ParamsKZG.setup(5, SRS_SECRET)
    circuit = circuits.StandardPlonk(None)
    pk = keygen.keygen_pk(params, keygen.keygen_vk(params, circuit), circuit)
    ws = prover.ProverWorkspace(params, pk)

    def check(advice):
        t = Blake2bWrite.init()
        t.common_scalar(keygen._m(pk.vk.transcript_repr))
        return [f.astuple() for f in ws.prover.drive(advice, [], 11, t, witness_check="only")]

    syn = circuits.StandardPlonk(0xC0FFEE).synthesize()
    assert check(syn.advice) == []
    syn.advice[2][2] = (syn.advice[2][2] + 1) % R  # c on row 2: x^2 + 72, in no copy constraint
    assert check(syn.advice) == [(GATE, 0, 2, 1)]
    syn = circuits.StandardPlonk(0xC0FFEE).synthesize()
    syn.advice[1][1] = 5  # b on row 1, a copy of x: the gate on row 1 and the copy constraint
    got = check(syn.advice)
    assert got[0] == (GATE, 0, 1, 1) and len(got) == 2 and got[1][0] == COPY and got[1][3] == 2 and got[1][1:3] in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2))
    ws.release()
    pk.release()
    params.release()


@pytest.mark.parametrize("k,cycles", [(9, 120), (11, 500)])
def test_copy_constraints_beyond_one_workgroup(gpu, k, cycles):
    from halo2_scaffold_amd import custom

    cs, good, _ = cases.copies_circuit(custom, k, cycles)
    assert len({cell for pair in good.copies for cell in pair}) > (256 if k == 9 else 1024)
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    keys = custom.Keys(params, cs, good)
    ws = custom.Workspace(params, keys)
    custom.check(params, keys, good, 1, ws=ws)
    for change in ((cycles - 3, 1), (1, 2), (5, 0)):  # a cycle of three in the last workgroup, of four (a fixed cell), of four (an instance cell)
        _, bad, members = cases.copies_circuit(custom, k, cycles, change)
        runs = []
        for _ in range(2):
            with pytest.raises(ValueError, match="copy constraint at cell") as e:
                custom.check(params, keys, bad, 1, ws=ws)
            runs.append([f.astuple() for f in e.value.failures])
        assert runs[0] == runs[1] and len(runs[0]) == 1
        kind, index, row, count = runs[0][0]
        # one cell of a cycle differs from the others: the two cells of the cycle whose image under the permutation has another value
        assert kind == COPY and count == 2 and cs.perm_columns[index] + (row,) in members
    _release(params, keys, ws)


def test_a_gate_left_on_over_the_blinding_rows(gpu):
    """a (a - 1) without a selector: custom.mock is content, the device names the first blinding row, and the verifier rejects the proof"""
    from halo2_scaffold_amd import custom

    k = 5
    cs, asg = cases.boolean_circuit(custom)
    custom.mock(asg, k)
    n, u = 1 << k, (1 << k) - (cs.blinding_factors() + 1)
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    keys = custom.Keys(params, cs, asg)
    ws = custom.Workspace(params, keys)
    failures = _raises(lambda: custom.check(params, keys, asg, 7, ws=ws), f"gate 'boolean' not satisfied at row {u}")
    assert [f.astuple() for f in failures] == [(GATE, 0, u, n - u)] and u <= failures[0].row < n
    proof = custom.create_proof(params, keys, asg, 7, ws=ws)
    ocs = gate_cases.oracle_cs(cs, "boolean")
    oasg = gate_cases.oracle_assignment(ocs, asg)
    vk = FX.VerifierKeys(ocs, k, SRS_SECRET, oasg.fixed, oasg.copies)
    assert keys.transcript_repr == vk.transcript_repr
    assert not phase_cases.verify_circuit(vk, cs, proof, oasg.instance)
    _release(params, keys, ws)


def _hooked(hooks):
    """a transcript that calls hooks[i]() in front of its i-th squeeze: 0 is theta (one-phase keys), 1 beta, 2 gamma, 3 y"""
    from halo2_scaffold_amd.transcript import Blake2bWrite

    class Hooked(Blake2bWrite):
        squeezes = 0

        def squeeze_challenge(self):
            if self.squeezes in hooks:
                hooks[self.squeezes]()
            self.squeezes += 1
            return super().squeeze_challenge()

    return Hooked.init()


@pytest.mark.parametrize("name", ["is_zero", "xor"])
def test_a_proof_does_not_depend_on_the_check(gpu, name):
    from halo2_scaffold_amd import custom
    from halo2_scaffold_amd import field as F

    k, build, _ = cases.DATA_CIRCUITS[name]
    cs, asg = build(custom)
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    keys = custom.Keys(params, cs, asg)
    ws = custom.Workspace(params, keys)
    want = custom.create_proof(params, keys, asg, 21, ws=ws)
    seen = []
    theta = F.fr_to_mont_limbs(0xBEEF)
    got = custom.create_proof(params, keys, asg, 21, transcript=_hooked({0: lambda: seen.append(ws.prover.check(theta)), 1: lambda: seen.append(ws.prover.check(5))}),
                              ws=ws)
    assert seen == [[], []] and got == want
    _release(params, keys, ws)


def test_the_range_golden_with_a_check_in_it(gpu):
    from halo2_scaffold_amd import flex
    from halo2_scaffold_amd.keygen import _m
    from halo2_scaffold_amd.transcript import Blake2bWrite

    g = json.load(open(os.path.join(GOLD, "flex_proofs.json")))
    case = next(c for c in g["cases"] if c["shape"] == "range")
    k, bits, x = case["k"], case["lookup_bits"], int(case["x"], 16)
    params = gpu.ParamsKZG.setup(k, int(g["srs_secret"], 16))
    cs = flex.FlexGateCS(lookup=True)
    asg = flex.range_closure(cs, x, bits)
    keys = flex.FlexKeys(params, cs, asg)
    ws = flex.FlexWorkspace(params, keys)
    t = Blake2bWrite.init()
    t.common_scalar(_m(keys.transcript_repr))
    for v in asg.instance:
        t.common_scalar(_m(v))
    trace = {}
    ws.prover.drive(asg.advice, asg.instance, case["seed"], t, trace, witness_check="also")
    assert trace["check"] == [] and t.finalize().hex() == case["proof"]
    _release(params, keys, ws)


def test_order_and_arguments(gpu):
    """H2MI_EINVAL before the advice, after the products, without theta on a key with data lookups, without the challenges on a key
    that has some — each leaving the proof in flight as it was; a report longer than `cap`"""
    from halo2_scaffold_amd import custom, engine
    from halo2_scaffold_amd import field as F

    lib = gpu.lib
    theta = np.ascontiguousarray(F.fr_to_mont_limbs(5))
    out, n_out = (engine.CheckFailure * 4)(), C.c_size_t(99)
    raw = lambda h, th=theta.ctypes.data, cap=4: (lib.h2mi_prover_check(h, th, out, cap, C.byref(n_out)), n_out.value)
    # a key with lookups as data
    k, build, _ = cases.DATA_CIRCUITS["xor"]
    cs, asg = build(custom)
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    keys = custom.Keys(params, cs, asg)
    ws = custom.Workspace(params, keys)
    h = ws.prover.handle
    assert raw(h) == (EINVAL, 0)  # no proof in flight
    want = custom.create_proof(params, keys, asg, 21, ws=ws)
    assert raw(h) == (EINVAL, 0)  # a finished proof
    seen = []
    hooks = {0: lambda: seen.append([raw(h, None), raw(h), lib.h2mi_prover_check(h, theta.ctypes.data, None, 1, C.byref(n_out)),
                                     lib.h2mi_prover_check(h, theta.ctypes.data, out, 4, None)]),
             3: lambda: seen.append(raw(h))}  # in front of y: after the products
    assert custom.create_proof(params, keys, asg, 21, transcript=_hooked(hooks), ws=ws) == want
    assert seen == [[(EINVAL, 0), (0, 0), EINVAL, EINVAL], (EINVAL, 0)]
    _release(params, keys, ws)
    # cap below the number of failures: is_zero with its output flipped fails both polynomials
    k, build, broken = cases.DATA_CIRCUITS["is_zero"]
    cs, asg = build(custom)
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    keys = custom.Keys(params, cs, asg)
    ws = custom.Workspace(params, keys)
    h = ws.prover.handle
    seen = []

    def short():
        out[1].kind = 77
        seen.append((raw(h, None, 1), out[0].astuple(), out[1].kind, raw(h, None, 0)))

    bad = broken(custom)
    proof = custom.create_proof(params, keys, bad, 8, transcript=_hooked({0: short}), ws=ws)
    assert seen == [((EUNSAT, 2), (GATE, 0, 0, 1), 77, (EUNSAT, 2))]
    assert proof == custom.create_proof(params, keys, bad, 8, ws=ws) and len(proof) > 0  # EUNSAT does not abandon the proof either
    _release(params, keys, ws)
    # a key with challenges: not before h2mi_prover_set_challenges, and the refusal leaves the proof where it was
    build, k = phase_cases.CIRCUITS["rlc"]
    cs, synthesize = build(custom)
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    keys = custom.Keys(params, cs, synthesize([None]))
    ws = custom.Workspace(params, keys)
    h = ws.prover.handle
    gamma = 0xABCDEF
    asg = synthesize([gamma])
    only_a, keep_a = engine.pack_cells([asg.advice[0], {}])
    only_acc, keep_acc = engine.pack_cells([{}, asg.advice[1]])
    pts = np.zeros((8, 8), dtype=np.uint64)
    g = np.ascontiguousarray(F.fr_to_mont_limbs(gamma))
    assert lib.h2mi_prover_advice_phase(h, 0, only_a, None, 0, 31, pts.ctypes.data) == 0
    assert raw(h) == (EINVAL, 0)  # between two advice phases
    assert lib.h2mi_prover_advice_phase(h, 1, only_acc, None, 0, 31, pts.ctypes.data) == 0
    assert raw(h) == (EINVAL, 0)  # the challenges are not set
    assert lib.h2mi_prover_set_challenges(h, g.ctypes.data) == 0
    assert raw(h, None) == (0, 0)  # no lookups: theta is not read
    assert lib.h2mi_prover_products(h, theta.ctypes.data, theta.ctypes.data, pts.ctypes.data) == 0
    del keep_a, keep_acc
    _release(params, keys, ws)


def test_cpp_host(gpu):
    """flex::check of include/h2mi_flex.hpp (examples/witness_check.cpp): the range closure satisfied, then with the output cell of its
    second gate spoilt — the gate column's polynomial and the row flex.mock names, and the workspace proves afterwards"""
    import subprocess

    from halo2_scaffold_amd import flex

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "examples"), "-s"])
    exe = os.path.join(root, "examples", "witness_check")
    k, bits, x = 7, 4, 0xDEADBEEFCAFE1234
    run = lambda spoil: subprocess.run([exe, str(k), str(bits), str(x), hex(SRS_SECRET), spoil], capture_output=True, text=True, timeout=300)
    r = run("none")
    assert r.returncode == 0 and "check ok" in r.stdout and "proof_bytes 992" in r.stdout, r.stdout[-500:] + r.stderr[-1500:]
    cs = flex.FlexGateCS(lookup=True)
    bad = flex.range_closure(cs, x, bits)
    bad.advice[0][sorted(bad.fixed[cs.col_q])[1] + 3] += 1
    report = cases.flex_host_report(bad, k)
    kind, index, row, count = report[0]
    assert kind == GATE
    r = run("gate")
    assert r.returncode == 3 and "proof_bytes 992" in r.stdout, r.stdout[-500:] + r.stderr[-1500:]
    assert f"check failed: check: gate polynomial 0 not satisfied at row {row} ({count} rows, {len(report)} failures in all)" in r.stdout, r.stdout


def test_scaffold_mock_device(gpu, tmp_path, monkeypatch):
    """scaffold.mock_device: `mock` against the key gen_key made — satisfied closures return their public inputs, one whose witness
    does not satisfy its own gate fails with the row scaffold.mock names, and the key proves afterwards"""
    from halo2_scaffold_amd import scaffold

    monkeypatch.setenv("PARAMS_DIR", str(tmp_path))
    monkeypatch.delenv("MINIMUM_ROWS", raising=False)
    monkeypatch.setenv("DEGREE", "6")
    monkeypatch.setenv("LOOKUP_BITS", "4")

    def closure(ctx, x, make_public):  # the witness of x * x is wrong for x = 5 only: the shape does not depend on the input
        c = ctx.load_witness(x)
        make_public.append(c)
        ctx.range_check(c, 8, ctx.lookup_bits)
        ctx.assign_region_last([("constant", 0), ("existing", c), ("existing", c), ("witness", x * x + (x == 5))], [0])

    pk, bp = scaffold.gen_key(closure, 0)
    assert scaffold.mock_device(closure, 9, pk) == [9]
    with pytest.raises(ValueError) as host:
        scaffold.mock(closure, 5)
    with pytest.raises(ValueError) as device:
        scaffold.mock_device(closure, 5, pk)
    assert str(host.value).startswith("gate not satisfied at row ") and str(device.value).startswith(str(host.value) + " (1 rows)")
    assert scaffold.mock_device(closure, 9, pk) == [9] and scaffold.prove_private(closure, 9, pk, bp) == [9] and len(pk.last_proof) == 992
    pk.release()
