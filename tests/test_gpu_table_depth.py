"""MSM base sets with a table depth on the device (h2mi_bases_register_depth{,_dev}, h2mi_bases_memory; csrc/h2mi_msm.hip "table
depth") against tests/table_depth_cases.py.

1. Result: every case column at every size and depth through every entry point — equal as a group element to the C restatement's
   MSM, and with h2mi_msm_set_canonical(1) byte for byte to the depth-1 handle's output; MSMs over the first m < n bases; the scalar
   buffer overwritten on the same stream directly behind every call; compact and full handles interleaved without a join.
2. Wide windows (H2MI_MSM_C = 19, 20 around the registrations, in a child process): the same at 2^13 + 1 points.
3. Route, from the launch profile: D' partition heads and one k_msm_combine per MSM, never the latency path; depth 1 is today's handle.
4. Memory and arguments: h2mi_bases_memory against the formula of the case module; refusals.
5. Proofs from parameters with a table depth: the bytes of the depth-1 parameters' proofs, and the committed golden where there is one."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import msm_schedule_cases as S
import table_depth_cases as T
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MSM_SPARSE, MSM_INORDER, MSM_GENERAL = 1, 2, 4
EINVAL, EHANDLE = -1, -5
ONE = o.pack([1], o.R)[0]  # Montgomery 1: the weight that makes h2mi_fr_lincomb_dev a stream-ordered copy
COMBINE, PICK_SHIFT = "k_msm_combine", "k_msm_pick_shift"
SRS_SECRET = 0x5EC2E7 + 0x7AB1E


class Profile:
    """with Profile(lib) as p: ... — afterwards p.names is every kernel launched inside, in issue order (h2mi_profile_dump)"""

    def __init__(self, lib):
        self.lib, self.names = lib, None

    def __enter__(self):
        lib = self.lib
        assert lib.h2mi_profile_reset() == 0 and lib.h2mi_profile_filter(b"") == 0 and lib.h2mi_profile_enable(1) == 0
        return self

    def __exit__(self, exc_type, exc, tb):
        lib = self.lib
        assert lib.h2mi_profile_enable(0) == 0
        if exc_type is None:
            need = C.c_size_t()
            assert lib.h2mi_profile_dump(None, 0, C.byref(need)) == 0
            buf = C.create_string_buffer(need.value)
            assert lib.h2mi_profile_dump(buf, need.value, None) == 0
            self.names = [line.split()[0] for line in buf.value.decode().splitlines()]
        assert lib.h2mi_profile_reset() == 0
        return False


def _affine(jac):
    """(m, 12) Jacobian limbs -> m byte strings of affine limbs, what cases.expected returns"""
    from oracle import cref

    return [row.tobytes() for row in cref.normalize(np.ascontiguousarray(jac).reshape(-1, 12))]


def _memory(lib, h):
    d, rows, tb, wb = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
    assert lib.h2mi_bases_memory(h, C.byref(d), C.byref(rows), C.byref(tb), C.byref(wb)) == 0
    return d.value, rows.value, tb.value, wb.value


class World:
    """what the tests of this module share on the device: one handle per (size, depth), the case columns, scratch buffers"""

    def __init__(self, gpu):
        self.gpu, self.lib = gpu, gpu.lib
        self.handles, self.cols, self.bufs, self.bases = {}, {}, {}, {}

    def handle(self, n, D):
        if (n, D) not in self.handles:
            if n not in self.bases:
                self.bases[n] = self.gpu.DevBuf.from_numpy(S.bases(n))
            h = C.c_uint64()
            assert self.lib.h2mi_bases_register_depth_dev(self.bases[n].ptr, n, D, C.byref(h)) == 0
            self.handles[(n, D)] = h.value
        return self.handles[(n, D)]

    def col(self, n, name, key=0):
        if (n, name, key) not in self.cols:
            a = S.column(n, S.POISON) if name == S.POISON else T.column(n, name, key)
            self.cols[(n, name, key)] = self.gpu.DevBuf.from_numpy(a)
        return self.cols[(n, name, key)]

    def buf(self, key, nbytes):
        if key not in self.bufs:
            self.bufs[key] = self.gpu.DevBuf(nbytes)
        return self.bufs[key]

    def copy(self, n, src, dst, stream):
        """a column of n scalars into dst, as a kernel queued on `stream` (None: the library stream)"""
        ptrs = (C.c_void_p * 1)(src.ptr)
        assert self.lib.h2mi_fr_lincomb_dev(ptrs, ONE.ctypes.data, 1, n, dst.ptr, stream) == 0

    def release(self):
        assert self.lib.h2mi_sync() == 0
        for h in self.handles.values():
            assert self.lib.h2mi_bases_release(h) == 0
        for d in list(self.bufs.values()) + list(self.cols.values()) + list(self.bases.values()):
            d.free()
        self.handles, self.cols, self.bufs, self.bases = {}, {}, {}, {}


@pytest.fixture(scope="module")
def world(gpu):
    w = World(gpu)
    yield w
    w.release()


class Run:
    """MSMs queued on one handle; every dev-form call reads a scratch buffer that is filled on the call's stream just before and
    overwritten on the same stream directly behind the call"""

    def __init__(self, world, n, D, out_key="out"):
        self.w, self.lib, self.n, self.D = world, world.lib, n, D
        self.h = world.handle(n, D)
        self.out = world.buf(out_key, 96 * 64)  # more slots than any test queues
        assert self.lib.h2mi_memset_zero(self.out.ptr, 96 * 64) == 0
        assert self.lib.h2mi_sync() == 0
        self.want, self.host = [], {}

    def _slot(self, want):
        self.want.append(want)
        return len(self.want) - 1

    def dev(self, cols, length, stream=None, flags=None):
        """one call: h2mi_msm_bn254_g1_dev (flags None, one column) or the phase entry with len(cols) columns"""
        w, n = self.w, self.n
        scratch = [w.buf((n, stream is not None, j), n * 32) for j in range(len(cols))]
        for d, (name, key) in zip(scratch, cols):
            w.copy(n, w.col(n, name, key), d, stream)
        first = len(self.want)
        for name, key in cols:
            self._slot(T.expected(n, name, key, length))
        if flags is None:
            rc = self.lib.h2mi_msm_bn254_g1_dev(self.h, scratch[0].ptr, length, self.out.ptr + 96 * first, stream)
        else:
            ptrs = (C.c_void_p * len(cols))(*[d.ptr for d in scratch])
            rc = self.lib.h2mi_msm_bn254_g1_phase_dev(self.h, ptrs, len(cols), length, self.out.ptr + 96 * first, flags, stream)
        assert rc == 0, (cols, length, flags, rc)
        for d in scratch:
            w.copy(n, w.col(n, S.POISON), d, stream)

    def host_form(self, col, length):
        name, key = col
        out = np.zeros(12, dtype=np.uint64)
        a = T.column(self.n, name, key)[:length]
        assert self.lib.h2mi_msm_bn254_g1(self.h, None, a.ctypes.data, length, out.ctypes.data) == 0
        self.host[self._slot(T.expected(self.n, name, key, length))] = out

    def check(self, what):
        assert self.lib.h2mi_sync() == 0
        got = self.out.to_numpy(shape=(len(self.want), 12), nbytes=96 * len(self.want)).copy()
        for i, v in self.host.items():
            got[i] = v
        for i, (g, want) in enumerate(zip(_affine(got), self.want)):
            assert g == want, f"{what}: MSM {i} at {self.n} points, depth {self.D}, is not the C restatement's group element"


CASES = [(n, D) for n in T.SIZES for D in T.depths(T.windows(T.window(n)))]


# ---- 1. result ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", CASES)
def test_every_column_through_every_entry_point(gpu, world, n, D):
    lib = world.lib
    W = T.windows(T.window(n))
    Dp, _ = T.effective(D, W)
    cols = T.columns(D)
    st = C.c_void_p()
    assert lib.h2mi_stream_create(C.byref(st)) == 0
    try:
        run = Run(world, n, D)
        with Profile(lib) as prof:
            for col in cols:  # the single form on the library stream and on a caller's
                run.dev([col], n)
                run.dev([col], n, stream=st.value)
            for flags in (0, MSM_SPARSE, MSM_INORDER, MSM_GENERAL):  # the phase entry, count = 3: every column under each flag
                run.dev(cols[0:3], n, flags=flags)
                run.dev(cols[2:5], n, flags=flags)
                run.dev(cols[3:0:-1], n, stream=st.value, flags=flags)
            run.dev([cols[0]], n, flags=MSM_INORDER)
            assert lib.h2mi_stream_wait(None, st.value) == 0
            for col in cols:
                run.host_form(col, n)
            run.check("full length")
        msms = len(run.want)
        if Dp > 1:  # the route: D' heads and one combine per MSM, never the latency path; the shift per pass
            assert prof.names.count(S.BIN_COUNT) == Dp * msms and prof.names.count(COMBINE) == msms and S.DIGITS not in prof.names
            assert prof.names.count(S.ACCUM) == Dp * msms and prof.names.count(S.FINAL) == Dp * msms
            assert prof.names.count(PICK_SHIFT) == (Dp * msms if n >= T.SHIFT_MIN_N else 0)
        else:
            assert COMBINE not in prof.names
        # the first m < n bases: the sum point is not part of such an MSM, the shift stays off
        run = Run(world, n, D)
        with Profile(lib) as prof:
            for m in sorted({n - 1, 1} - {0, n}):
                for col in (("uniform", 0), ("shift3", 0), ("edges", 0)):
                    run.dev([col], m)
                    run.dev([col], m, stream=st.value)
                run.host_form(("shift3", 0), m)
            assert lib.h2mi_stream_wait(None, st.value) == 0
            run.check("first m bases")
        assert PICK_SHIFT not in prof.names
    finally:
        assert lib.h2mi_stream_destroy(st) == 0


@pytest.mark.parametrize("n,D", CASES)
def test_canonical_output_is_the_depth_1_handles_bytes(gpu, world, n, D):
    lib = world.lib
    cols = T.columns(D)
    outs = []
    assert lib.h2mi_msm_set_canonical(1) == 0
    try:
        for depth in (1, D):
            run = Run(world, n, depth)
            for col in cols:
                run.dev([col], n)
            run.dev(cols[:3], n, flags=MSM_GENERAL)
            assert lib.h2mi_sync() == 0
            outs.append(run.out.to_numpy(shape=(len(run.want), 12), nbytes=96 * len(run.want)).copy())
            run.check("canonical")
    finally:
        assert lib.h2mi_msm_set_canonical(0) == 0
    assert outs[0].tobytes() == outs[1].tobytes()
    assert all(list(row[8:]) == list(o.pack([1], o.Q)[0]) or not any(row[8:]) for row in outs[1])  # Z = 1 (or the identity)


@pytest.mark.parametrize("n", [769, 4097])
def test_two_compact_handles_and_a_full_one_interleaved_without_a_join(gpu, world, n):
    lib = world.lib
    W = T.windows(T.window(n))
    cols = T.columns(2)[:4]
    runs = [Run(world, n, D, out_key=("mix", D)) for D in (2, W, 1)]  # each its own result buffer
    st = C.c_void_p()
    assert lib.h2mi_stream_create(C.byref(st)) == 0
    try:
        for i in range(8):
            for r in runs:
                # scratch buffers are shared by the three handles: each call's scalars are overwritten before the next handle's call
                r.dev([cols[i % 4]], n, stream=st.value if i % 3 == 2 else None)
        assert lib.h2mi_stream_wait(None, st.value) == 0
        for r in runs:
            r.check("interleaved")
    finally:
        assert lib.h2mi_stream_destroy(st) == 0


# ---- 2. wide windows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [19, 20])
def test_wide_windows_forced_around_the_registrations(gpu, c):
    """low-bit binning, 16-bit keys and segmented sums under the window filter: the result and canonical tests of this module at
    2^13 + 1 points, D = 2 and W, in a child process whose registrations all take H2MI_MSM_C"""
    n, W = (1 << 13) + 1, T.windows(c)
    sel = " or ".join(f"{t}[{n}-{D}]" for t in ("test_every_column_through_every_entry_point", "test_canonical_output_is_the_depth_1_handles_bytes") for D in (2, W))
    env = dict(os.environ, H2MI_MSM_C=str(c), OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_table_depth.py", "-x", "-q", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "4 passed" in r.stdout, r.stdout[-2500:] + r.stderr[-1500:]


# ---- 3. route and statistics ------------------------------------------------------------------------------------------------------------------
def test_depth_1_at_256_points_is_todays_handle(gpu, world):
    lib, n = world.lib, 256
    base = world.gpu.DevBuf.from_numpy(S.bases(n))
    plain, viad = C.c_uint64(), C.c_uint64()
    assert lib.h2mi_bases_register_dev(base.ptr, n, C.byref(plain)) == 0
    assert lib.h2mi_bases_register_depth(S.bases(n).ctypes.data, n, 1, C.byref(viad)) == 0
    try:
        assert _memory(lib, plain.value) == _memory(lib, viad.value) == T.memory(n, 1)
        sc = world.gpu.DevBuf.from_numpy(S.column(n, "uniform"))
        out = world.gpu.DevBuf(96)
        with Profile(lib) as prof:
            assert lib.h2mi_msm_bn254_g1_dev(viad.value, sc.ptr, n, out.ptr, None) == 0
            assert lib.h2mi_sync() == 0
        assert prof.names.count(S.DIGITS) == 1 and prof.names.count(S.SMALL_PAIR) == 1 and COMBINE not in prof.names and S.BIN_COUNT not in prof.names
        assert _affine(out.to_numpy(shape=(1, 12)))[0] == S.expected(n, "uniform", n)
        sc.free()
        out.free()
    finally:
        assert lib.h2mi_bases_release(plain.value) == 0 and lib.h2mi_bases_release(viad.value) == 0
        base.free()


@pytest.mark.parametrize("n", [767, 4097])
def test_bucket_adds_equal_the_depth_1_handles(gpu, world, n):
    """h2mi_msm_last_stats sums over the passes: the insertions of the general pipeline on the depth-1 handle for the same scalars, and
    the non-zero digits of the model.  (At 4097 points only a compact handle has the sum point — a depth-1 handle of that size has the
    latency path's table instead — so the columns compared there are the ones on which the shift stays at zero.)"""
    lib = world.lib
    c = T.window(n)
    W = T.windows(c)
    names = ("uniform", "edges") if n >= T.SHIFT_MIN_N else T.FIXED_COLUMNS
    out = world.buf(("stats", 0), 96)
    for name in names:
        model = T.insertions(o.unpack(T.column(n, name), o.R), c)
        seen = []
        for D in (1, 2, 4, W):
            h = world.handle(n, D)
            ptrs = (C.c_void_p * 1)(world.col(n, name).ptr)
            assert lib.h2mi_msm_bn254_g1_phase_dev(h, ptrs, 1, n, out.ptr, MSM_GENERAL, None) == 0
            ba, ra = C.c_uint64(), C.c_uint64()
            assert lib.h2mi_msm_last_stats(h, C.byref(ba), C.byref(ra)) == 0
            seen.append(ba.value)
            assert ra.value > 0
        assert seen == [model] * 4, (n, name)


# ---- 4. memory and arguments ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", T.SIZES)
def test_bases_memory_equals_the_formula_and_info_the_depth_1_handles(gpu, world, n):
    lib = world.lib
    W = T.windows(T.window(n))

    def info(h):
        c, w, nb, nn = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        assert lib.h2mi_bases_info(h, C.byref(c), C.byref(w), C.byref(nb), C.byref(nn)) == 0
        return c.value, w.value, nb.value, nn.value

    first = info(world.handle(n, 1))
    assert first == (T.window(n), W, 1 << (T.window(n) - 1), n)
    prev = None
    for D in T.depths(W):
        h = world.handle(n, D)
        got = _memory(lib, h)
        assert got == T.memory(n, D), (n, D)
        assert got[0] == min(D, W)
        assert info(h) == first
        assert prev is None or (got[2] <= prev[2] and got[3] <= prev[3])
        prev = got
        for keep in range(4):  # any pointer may be NULL
            args = [C.byref(t()) if i == keep else None for i, t in enumerate((C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64))]
            assert lib.h2mi_bases_memory(h, *args) == 0
    assert prev[2] == (n + 1) * 64


def test_refusals(gpu, world):
    lib, n = world.lib, 769
    base = world.gpu.DevBuf.from_numpy(S.bases(n))
    h = C.c_uint64(77)
    assert lib.h2mi_bases_register_depth_dev(base.ptr, n, 0, C.byref(h)) == EINVAL
    assert lib.h2mi_bases_register_depth(S.bases(n).ctypes.data, n, 0, C.byref(h)) == EINVAL
    assert lib.h2mi_bases_register_depth_dev(None, n, 2, C.byref(h)) == EINVAL and lib.h2mi_bases_register_depth_dev(base.ptr, n, 2, None) == EINVAL
    assert h.value == 77
    assert lib.h2mi_bases_register_depth(S.bases(n).ctypes.data, n, 3, C.byref(h)) == 0  # the host-pointer form
    assert _memory(lib, h.value) == T.memory(n, 3)
    assert lib.h2mi_bases_release(h.value) == 0
    assert lib.h2mi_bases_memory(h.value, None, None, None, None) == EHANDLE
    out = world.buf(("stats", 0), 96)
    assert lib.h2mi_msm_bn254_g1_dev(h.value, base.ptr, 1, out.ptr, None) == EHANDLE
    base.free()


_MULTI = r"""
import ctypes as C, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
import torch  # noqa: F401
import _load_pkg
h2 = _load_pkg.load()
import msm_schedule_cases as S
lib = h2.lib
assert lib.h2mi_init_devices(2) == 0 and lib.h2mi_device_count() == 2
b = S.bases(769)
h = C.c_uint64()
assert lib.h2mi_bases_register_depth(b.ctypes.data, 769, 2, C.byref(h)) == -1
d = h2.DevBuf.from_numpy(b)
assert lib.h2mi_bases_register_depth_dev(d.ptr, 769, 25, C.byref(h)) == -1
assert lib.h2mi_bases_register_depth_dev(d.ptr, 769, 0, C.byref(h)) == -1
assert lib.h2mi_bases_register_depth(b.ctypes.data, 769, 1, C.byref(h)) == 0  # depth 1 shards as ever
depth, rows = C.c_uint32(), C.c_uint32()
assert lib.h2mi_bases_memory(h.value, C.byref(depth), C.byref(rows), None, None) == 0 and (depth.value, rows.value) == (1, 20)
assert lib.h2mi_bases_release(h.value) == 0
print("DEPTH_MULTI_OK")
"""


def test_a_depth_above_1_is_refused_under_several_devices(gpu, tmp_path):
    script = tmp_path / "multi.py"
    script.write_text(_MULTI.format(root=ROOT))
    env = dict(os.environ, H2MI_VIRTUAL_DEVICES="1", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "DEPTH_MULTI_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


# ---- 5. proofs ----------------------------------------------------------------------------------------------------------------------------------
def _with_depths(gpu, k, secret, prove):
    """prove(params) -> bytes, from parameters of depth 1, 2 and W: the three results and the parameters' device bytes"""
    W = T.windows(T.window(1 << k))
    out, mem = [], []
    for D in (1, 2, W):
        params = gpu.ParamsKZG.setup(k, secret, table_depth=D)
        assert _memory(gpu.lib, params.g_handle)[0] == D and _memory(gpu.lib, params.g_lagrange_handle)[0] == D
        mem.append(params.device_bytes())
        out.append(prove(params))
        params.release()
    assert out[1] == out[0] and out[2] == out[0]
    assert mem[0][0] > mem[1][0] > mem[2][0] and mem[0][1] > mem[1][1] >= mem[2][1]  # device_bytes falls with D
    assert mem[2][0] == 2 * ((1 << k) + 1) * 64
    return out[0]


@pytest.mark.parametrize("k", [8, 13])
def test_standard_plonk_proofs(gpu, k):
    """k = 8: the committed golden.  k = 13: the grand products take the dominant-value shift, in every pass.  Both endings."""
    from halo2_scaffold_amd import circuits, keygen, prover

    gold = json.load(open(os.path.join(GOLD, "standard_plonk_proofs.json")))
    case = [c for c in gold["cases"] if c["k"] == 8][0]
    x, seed = int(case["witness_x"], 16), case["seed"]

    def prove(params):
        circuit = circuits.StandardPlonk(None)
        pk = keygen.keygen_pk(params, keygen.keygen_vk(params, circuit), circuit)
        proofs = prover.create_proof(params, pk, circuits.StandardPlonk(x), seed) + prover.create_proof(params, pk, circuits.StandardPlonk(x + 1), seed + 1, multiopen="gwc")
        pk.release()
        return proofs

    proofs = _with_depths(gpu, k, int(gold["srs_secret"], 16), prove)
    if k == 8:
        assert proofs[: len(case["proof"]) // 2].hex() == case["proof"]


def test_range_closure_with_a_lookup_on_a_by_coset_key(gpu):
    from halo2_scaffold_amd import flex

    k, bits, x = 10, 8, 0x1234

    def prove(params):
        cs = flex.FlexGateCS(lookup=True)
        asg = flex.range_closure(cs, x, bits)
        keys = flex.FlexKeys(params, cs, asg, by_coset=True)
        proof = keys.vk_bytes() + flex.create_proof(params, keys, asg, 5)
        keys.release()
        return proof

    assert len(_with_depths(gpu, k, SRS_SECRET, prove)) > 0


def test_a_batch_of_two(gpu):
    import custom_gate_cases as gate_cases
    from halo2_scaffold_amd import custom

    built = [gate_cases.is_zero_circuit(custom, x) for x in (5, 0)]
    cs, asgs = built[0][0], [b[1] for b in built]

    def prove(params):
        keys = custom.Keys(params, cs, asgs[0])
        proof = custom.prove_many(keys, asgs, seeds=[40, 48], params=params)
        keys.release()
        return proof

    assert len(_with_depths(gpu, 5, SRS_SECRET, prove)) > 0
