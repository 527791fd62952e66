"""Witness cells from device memory and as 64-bit integers: h2mi_fr_scatter_cells_dev word for word against the Python integers of
tests/device_cells_cases.py (every format x row list x count, 64 columns in one call, rows at the limit, unreduced canonical values);
proofs whose advice comes from device memory (h2mi_malloc buffers, torch tensors) or from int64 arrays byte for byte against the same
witness handed over as host cells; the memory overwritten behind the advice call; the refusals; the route from the launch profile."""
import ctypes as C
import random

import numpy as np
import pytest

import assigned_cases as A
import device_cells_cases as D
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

R = o.R
SRS_SECRET = 0x5EC2E7 + 0x48324D49
EINVAL, ERANGE = -1, -6
KERNEL = "k_cells_scatter"
BIG_ROWS = 3 * (2**13 - 6) + 2  # room for the longest column at stride 3


def _launches(gpu, call, allow_none=False) -> int:
    """launches of k_cells_scatter during call(), from the library's launch profile"""
    lib = gpu.lib
    assert lib.h2mi_profile_reset() == 0 and lib.h2mi_profile_filter(b"") == 0 and lib.h2mi_profile_enable(1) == 0
    try:
        call()
    finally:
        assert lib.h2mi_profile_enable(0) == 0
    ms, count, every = C.c_double(), C.c_uint64(), C.c_uint64()
    assert lib.h2mi_profile_query(KERNEL.encode(), C.byref(ms), C.byref(count)) == 0
    assert lib.h2mi_profile_query(b"", C.byref(ms), C.byref(every)) == 0
    assert lib.h2mi_profile_reset() == 0
    assert allow_none or every.value > 0  # the profile did record this call's launches
    return count.value if not allow_none else (count.value, every.value)


# ---- the kernel, through h2mi_fr_scatter_cells_dev: h2mi_malloc memory, no torch ------------------------------------------------------
class _Column:
    """one source of a scatter call: the destination (n_rows sentinel words and one more behind its end), the values, the rows"""

    def __init__(self, gpu, fmt, kind, count, n_rows, row_limit=None, rows=None, src=None):
        self.fmt, self.count, self.n_rows = fmt, count, n_rows
        self.row_limit = n_rows if row_limit is None else row_limit
        self.src, self.want = D.case(fmt, count) if count else (None, np.zeros((0, 4), dtype=np.uint64))
        if src is not None:
            self.src = src
        self.rows = D.rows(kind, count, self.row_limit) if rows is None and count and kind != "dense" else rows
        self.dst = gpu.DevBuf.from_numpy(np.tile(D.SENTINEL, (n_rows + 1, 1)))
        self.d_values = gpu.DevBuf.from_numpy(self.src) if count else None
        self.d_rows = gpu.DevBuf.from_numpy(self.rows) if self.rows is not None else None

    def fill(self, source):
        source.d_column, source.count, source.row_limit, source.format = self.dst.ptr, self.count, self.row_limit, D.FORMATS[self.fmt]
        source.values = self.d_values.ptr if self.d_values else None
        source.rows = self.d_rows.ptr if self.d_rows else None

    def got(self):
        return self.dst.to_numpy(shape=(self.n_rows + 1, 4))

    def expected(self):
        return D.expected_column(self.n_rows + 1, self.rows, self.want)

    def reset(self):
        self.dst.upload(np.tile(D.SENTINEL, (self.n_rows + 1, 1)))

    def free(self):
        for b in (self.dst, self.d_values, self.d_rows):
            if b:
                b.free()


def _scatter(gpu, columns, n=None):
    from halo2_scaffold_amd import engine

    arr = (engine.CellsSource * max(len(columns), 1))()
    for i, col in enumerate(columns):
        col.fill(arr[i])
    status = (C.c_uint64 * 2)(77, 77)
    rc = gpu.lib.h2mi_fr_scatter_cells_dev(arr, len(columns) if n is None else n, status, None)
    return rc, (status[0], status[1])


@pytest.mark.parametrize("kind", ["dense"] + D.ROW_LISTS)
@pytest.mark.parametrize("fmt", list(D.FORMATS))
def test_kernel_word_for_word(gpu, fmt, kind):
    """every count of the list; rows nobody names, and the word behind the column's end, keep their sentinel"""
    for count in D.COUNTS:
        col = _Column(gpu, fmt, kind, count, BIG_ROWS)
        rc, status = _scatter(gpu, [col])
        assert rc == 0 and status == (0, 0), (fmt, kind, count, rc, status)
        assert np.array_equal(col.got(), col.expected()), (fmt, kind, count)
        col.free()


def test_sixty_four_columns_in_one_call(gpu):
    """one launch for 64 columns of every format and row list with lengths 0, 1, 65, 4097, ..: workgroups straddle columns, empty
    columns lie between them; the same columns one call each give the same words"""
    columns = [_Column(gpu, fmt, kind, count, n_rows) for fmt, kind, count, n_rows in D.many_columns()]
    out = {}
    launches = _launches(gpu, lambda: out.update(answer=_scatter(gpu, columns)))
    assert out["answer"] == (0, (0, 0)) and launches == 1
    together = [col.got() for col in columns]
    for col, got in zip(columns, together):
        assert np.array_equal(got, col.expected()), (col.fmt, col.count)
        col.reset()
    for col, got in zip(columns, together):
        assert _scatter(gpu, [col]) == (0, (0, 0))
        assert np.array_equal(col.got(), got), (col.fmt, col.count)
        col.free()


@pytest.mark.parametrize("fmt", list(D.FORMATS))
def test_rows_at_the_limit_are_counted_not_written(gpu, fmt):
    """a row equal to row_limit at the first, a middle and the last position of a 300-cell column; then rows far beyond it"""
    limit, count = 1000, 300
    rows = D.rows("random", count, limit).copy()
    for far in (limit, 0xFFFFFFFF):
        rows[[0, 150, 299]] = far
        col = _Column(gpu, fmt, None, count, limit, rows=rows)
        rc, status = _scatter(gpu, [col])
        assert rc == 0 and status == (3, 0)
        keep = np.ones(count, dtype=bool)
        keep[[0, 150, 299]] = False
        want = D.expected_column(limit + 1, rows[keep], col.want[keep])
        assert np.array_equal(col.got(), want)
        assert np.array_equal(col.got()[limit], D.SENTINEL)  # the word behind the column's end
        col.free()
    # a dense run longer than the limit: the cells beyond it are counted
    col = _Column(gpu, fmt, "dense", 65, 65, row_limit=60)
    rc, status = _scatter(gpu, [col])
    assert rc == 0 and status == (5, 0)
    assert np.array_equal(col.got()[:60], col.want[:60]) and np.array_equal(col.got()[60:], np.tile(D.SENTINEL, (6, 1)))
    col.free()


def test_unreduced_canonical_values_are_counted_and_zeroed(gpu):
    src, want = (a.copy() for a in D.case("canonical", 257))
    src[3], src[200] = D.limbs(R), D.limbs((1 << 256) - 1)
    want[3] = want[200] = 0
    col = _Column(gpu, "canonical", "reversed", 257, 400, src=src)
    col.want = want
    rc, status = _scatter(gpu, [col])
    assert rc == 0 and status == (0, 2)
    assert np.array_equal(col.got(), col.expected())
    # the same words as Montgomery cells are carried verbatim and counted nowhere
    col2 = _Column(gpu, "montgomery", "reversed", 257, 400, src=src)
    col2.want = src
    assert _scatter(gpu, [col2]) == (0, (0, 0)) and np.array_equal(col2.got(), col2.expected())
    col.free()
    col2.free()


def test_scatter_refuses_bad_arguments(gpu):
    from halo2_scaffold_amd import engine

    lib = gpu.lib
    col = _Column(gpu, "i64", "ascending", 10, 40)
    arr = (engine.CellsSource * 65)()
    status = (C.c_uint64 * 2)()
    col.fill(arr[0])
    assert lib.h2mi_fr_scatter_cells_dev(arr, 1, None, None) == EINVAL  # status_out is required
    assert lib.h2mi_fr_scatter_cells_dev(None, 1, status, None) == EINVAL and lib.h2mi_fr_scatter_cells_dev(arr, 65, status, None) == EINVAL
    assert lib.h2mi_fr_scatter_cells_dev(None, 0, status, None) == 0
    for field, bad in (("d_column", col.dst.ptr + 8), ("d_column", None), ("values", col.d_values.ptr + 4), ("values", None), ("rows", col.d_rows.ptr + 2),
                       ("format", 2), ("format", 3), ("format", 5)):
        col.fill(arr[0])
        setattr(arr[0], field, bad)
        assert lib.h2mi_fr_scatter_cells_dev(arr, 1, status, None) == EINVAL, (field, bad)
    col.fill(arr[0])
    arr[0].format, arr[0].values = 1, col.d_values.ptr + 8  # 32-byte values: 16 bytes
    assert lib.h2mi_fr_scatter_cells_dev(arr, 1, status, None) == EINVAL
    assert np.array_equal(col.got(), np.tile(D.SENTINEL, (41, 1)))  # nothing was written by any refused call
    col.free()


# ---- proofs: the same witness from the device and as today's host cells ----------------------------------------------------------------
class _Witness:
    """what create_proof reads off an assignment"""

    def __init__(self, advice, instance):
        self.advice, self.instance = advice, instance


def _i64(values):
    """field elements that are small integers modulo r, as int64"""
    out = [v if v < 2**63 else v - R for v in values]
    assert all(-(2**63) <= v < 2**63 for v in out)
    return np.array(out, dtype=np.int64)


def _device_column(gpu, cells: dict, fmt: str, keep: list, use_torch=False, rows_dtype="int32", shuffle=None, force_rows=False):
    """{row: value} -> engine.DeviceCells over h2mi_malloc buffers (or torch tensors made on the device); rows 0 .. count - 1 go
    without a row list (unless force_rows), any other set of rows as a list in shuffled order"""
    from halo2_scaffold_amd import engine

    rows = sorted(cells)
    dense = rows == list(range(len(rows))) and not force_rows
    if not dense:
        random.Random(f"order {shuffle} {len(rows)}").shuffle(rows)
    vals = [cells[r] % R for r in rows]
    values = _i64(vals) if fmt == "i64" else o.pack(vals) if fmt == "canonical" else o.pack(vals, R)
    if use_torch:
        import torch

        tv = torch.from_numpy(values.view(np.int64)).to("cuda:0")
        tr = None if dense else torch.tensor(rows, dtype=getattr(torch, rows_dtype), device="cuda:0")
        col = engine.DeviceCells(tv, rows=tr, fmt=fmt)
        keep += [tv, tr]
    else:
        bv = gpu.DevBuf.from_numpy(values)
        br = None if dense else gpu.DevBuf.from_numpy(np.array(rows, dtype=np.uint32))
        col = engine.DeviceCells(bv, rows=br, fmt=fmt, count=len(rows))
        keep += [bv, br]
    assert len(col) == len(rows)
    return col


def _clobber(keep):
    """garbage into every device buffer a witness was made of"""
    for b in keep:
        if b is None:
            continue
        if hasattr(b, "upload"):
            b.upload(np.full(b.nbytes, 0xA5, dtype=np.uint8))
        else:
            import torch

            b.fill_(-0x5A5A5A5A5A5A5A5B if b.dtype == torch.int64 else -0x5A5A5A5B)
            torch.cuda.synchronize()


def _clobbering_transcript(flex, keep):
    """a transcript that overwrites the witness's device memory when the first advice commitment is written: the advice call has
    returned, every later phase is still to come"""
    t = flex.Blake2bWrite.init()
    write, fired = t.write_point, []

    def write_point(pt):
        if not fired:
            fired.append(True)
            _clobber(keep)
        return write(pt)

    t.write_point = write_point
    t.fired = fired
    return t


FORMS = ("montgomery", "canonical")


def _converted(gpu, asg, formats, keep, **kw):
    """an assignment's advice, column j through formats[j]: a DeviceCells format, "host" (left as it is), "ints" (engine.IntCells)"""
    from halo2_scaffold_amd import engine

    out = []
    for j, cells in enumerate(asg.advice):
        f = formats[j % len(formats)] if not isinstance(formats, dict) else formats.get(j, "host")
        if f == "host" or (f != "ints" and not cells):
            out.append(cells)
        elif f == "ints":
            rows = sorted(cells)
            dense = rows == list(range(len(rows)))
            out.append(engine.IntCells(_i64([cells[r] % R for r in rows]), None if dense else np.array(rows, dtype=np.uint32)))
        else:
            out.append(_device_column(gpu, cells, f, keep, shuffle=j, **kw))
    return _Witness(out, asg.instance)


def test_custom_gate_circuit_with_every_column_below_16_cells(gpu):
    """src/circuits/is_zero.rs at k = 5: three columns of one or two cells — no host shortcut for device memory, one launch"""
    from halo2_scaffold_amd import custom

    cs, asg = A.is_zero_circuit(custom, 0x1234567, resolved=True)
    params = gpu.ParamsKZG.setup(5, SRS_SECRET)
    keys = custom.Keys(params, cs, asg)
    ws = custom.Workspace(params, keys)
    want = custom.create_proof(params, keys, asg, 31, ws=ws)
    for formats in (("montgomery", "canonical", "i64"), ("canonical", "montgomery", "montgomery")):
        keep, out = [], {}
        wit = _converted(gpu, asg, formats, keep, use_torch=formats[2] == "i64")  # h2mi_malloc buffers, and torch tensors
        assert _launches(gpu, lambda: out.update(proof=custom.create_proof(params, keys, wit, 31, ws=ws))) == 1
        assert out["proof"] == want
    custom.check(params, keys, wit, ws=ws)  # the witness check reads the same columns
    ws.release()
    keys.release()
    params.release()


@pytest.mark.parametrize("k", [9, 13])
def test_range_proof_from_torch_tensors(gpu, k):
    """the reference's range circuit with LOOKUP_BITS 8: its advice column as 32-byte limbs (canonical, Montgomery) and, where every cell
    fits, as int64 — torch tensors made on the device, with and without row lists (int32 and int64); the tensors are overwritten behind
    the advice call"""
    from halo2_scaffold_amd import flex

    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    cs = flex.FlexGateCS(lookup=True)
    asg = flex.range_closure(cs, 0x0123456789ABCDEF, 8)
    keys = flex.FlexKeys(params, cs, asg)
    ws = flex.FlexWorkspace(params, keys)
    want = flex.create_proof(params, keys, asg, 23, ws=ws)
    small = all(v % R < 2**63 or R - v % R <= 2**63 for cells in asg.advice for v in cells.values())  # 64-bit limbs and sums: int64 will do
    for fmt, rows_dtype in (("canonical", "int32"), ("montgomery", "int64")) + ((("i64", "int64"), ("i64", "int32")) if small else ()):
        keep, out = [], {}
        wit = _converted(gpu, asg, (fmt,), keep, use_torch=True, rows_dtype=rows_dtype, force_rows=rows_dtype == "int64" or k == 13)
        t = _clobbering_transcript(flex, keep)
        assert _launches(gpu, lambda: out.update(proof=flex.create_proof(params, keys, wit, 23, transcript=t, ws=ws))) == 1
        assert t.fired and out["proof"] == want
    ws.release()
    keys.release()
    params.release()


def _mixed_columns():
    """seven columns at k = 13: host dict, device Montgomery dense, device canonical scattered, device I64, host IntCells short, host
    IntCells long scattered, empty"""
    usable = (1 << 13) - 6
    rng = random.Random("mixed device cells")
    field = lambda n: [rng.randrange(R) for _ in range(n)]
    small = lambda n: [rng.randrange(-(2**63), 2**63) % R for _ in range(n)]
    columns = [A.dense(field(12)), A.dense(field(5000)), A.scattered(field(4500), usable, "canonical"), A.dense(small(100) + [v % R for v in D.I64_EDGES]),
               A.dense(small(10)), A.scattered(small(4200), usable, "ints"), {}]
    formats = {0: "host", 1: "montgomery", 2: "canonical", 3: "i64", 4: "ints", 5: "ints", 6: "montgomery"}
    return columns, formats


def test_one_call_that_mixes_every_route(gpu):
    """... and overwrites the device buffers behind the advice call: the proof bytes are those of the host witness; the call launched
    k_cells_scatter exactly once; the host witness alone launched it never"""
    from halo2_scaffold_amd import custom, engine, flex

    columns, formats = _mixed_columns()
    cs, asg = A.columns_circuit(custom, columns)
    params = gpu.ParamsKZG.setup(13, SRS_SECRET)
    keys = custom.Keys(params, cs, asg)
    ws = custom.Workspace(params, keys)
    out = {}
    assert _launches(gpu, lambda: out.update(want=custom.create_proof(params, keys, asg, 5, ws=ws))) == 0
    host_columns = [v.to_numpy(shape=(1 << 13, 4)) for v in ws.prover.views(engine.BUF_ADVICE, cs.n_advice)]
    keep = []
    wit = _converted(gpu, asg, formats, keep)
    wit.advice[6] = engine.DeviceCells(0, count=0)  # an empty column: none of its pointers is looked at
    assert isinstance(wit.advice[0], dict) and isinstance(wit.advice[5], engine.IntCells) and len(wit.advice[5]) == 4200
    t = _clobbering_transcript(flex, keep)
    assert _launches(gpu, lambda: out.update(proof=custom.create_proof(params, keys, wit, 5, transcript=t, ws=ws))) == 1
    assert t.fired and out["proof"] == out["want"]
    for a, v in zip(host_columns, ws.prover.views(engine.BUF_ADVICE, cs.n_advice)):
        assert np.array_equal(a, v.to_numpy(shape=(1 << 13, 4)))
    # the GWC ending, and a by-coset key
    wit = _converted(gpu, asg, formats, keep)
    assert custom.create_proof(params, keys, wit, 5, ws=ws, multiopen="gwc") == custom.create_proof(params, keys, asg, 5, ws=ws, multiopen="gwc")
    ws.release()
    by_coset = custom.Keys(params, cs, asg, by_coset=True)
    assert custom.create_proof(params, by_coset, wit, 5) == out["want"]
    by_coset.release()
    keys.release()
    params.release()


def test_a_column_of_4097_scattered_cells(gpu):
    from halo2_scaffold_amd import custom

    usable = (1 << 13) - 6
    rng = random.Random("4097")
    cs, asg = A.columns_circuit(custom, [A.scattered([rng.randrange(R) for _ in range(4097)], usable, 4097)])
    params = gpu.ParamsKZG.setup(13, SRS_SECRET)
    keys = custom.Keys(params, cs, asg)
    want = custom.create_proof(params, keys, asg, 9)
    for fmt in FORMS:
        keep = []
        assert custom.create_proof(params, keys, _converted(gpu, asg, (fmt,), keep), 9) == want
    keys.release()
    params.release()


def test_short_and_long_host_integers(gpu):
    """host IntCells on both sides of each threshold: 16 / 17 dense cells, 4096 / 4097 listed ones — the short runs ride in the patch
    launch, the long ones take the kernel; the bytes are those of the same values as field elements"""
    from halo2_scaffold_amd import custom

    usable = (1 << 13) - 6
    rng = random.Random("thresholds")
    small = lambda n: [rng.randrange(-(2**63), 2**63) % R for _ in range(n)]
    params = gpu.ParamsKZG.setup(13, SRS_SECRET)
    for cells, want_launches in ((A.dense(small(16)), 0), (A.dense(small(17)), 1), (A.scattered(small(4096), usable, "short"), 0),
                                 (A.scattered(small(4097), usable, "long"), 1)):
        cs, asg = A.columns_circuit(custom, [cells])
        keys = custom.Keys(params, cs, asg)
        out = {}
        wit = _converted(gpu, asg, ("ints",), [])
        assert _launches(gpu, lambda: out.update(proof=custom.create_proof(params, keys, wit, 3))) == want_launches, len(cells)
        assert out["proof"] == custom.create_proof(params, keys, asg, 3)
        keys.release()
    params.release()


def test_second_phase_column_on_the_device(gpu):
    from halo2_scaffold_amd import custom

    rng = random.Random("phases")
    columns = [A.dense([rng.randrange(R) for _ in range(30)]), A.dense([rng.randrange(R) for _ in range(40)])]
    cs, asg = A.columns_circuit(custom, columns, phases=[0, 1])
    params = gpu.ParamsKZG.setup(6, SRS_SECRET)
    keys = custom.Keys(params, cs, asg)
    want = custom.create_proof(params, keys, asg, 17)
    keep, out = [], {}
    wit = _converted(gpu, asg, {1: "canonical"}, keep)
    assert _launches(gpu, lambda: out.update(proof=custom.create_proof(params, keys, wit, 17))) == 1  # the second phase's call alone
    assert out["proof"] == want
    wit = _converted(gpu, asg, {0: "montgomery", 1: "montgomery"}, keep)
    assert _launches(gpu, lambda: out.update(proof=custom.create_proof(params, keys, wit, 17))) == 2  # one launch per advice phase
    assert out["proof"] == want
    keys.release()
    params.release()


def test_a_batch_of_two_one_member_from_the_device(gpu):
    from halo2_scaffold_amd import custom

    rng = random.Random("batch")
    members = [[A.dense([rng.randrange(R) for _ in range(40)]), A.scattered([rng.randrange(R) for _ in range(9)], 58, i)] for i in range(2)]
    built = [A.columns_circuit(custom, m) for m in members]
    cs = built[0][0]
    params = gpu.ParamsKZG.setup(6, SRS_SECRET)
    keys = custom.Keys(params, cs, built[0][1])
    want = custom.prove_many(keys, [b[1] for b in built], seeds=[3, 40])
    keep, out = [], {}
    wit = _converted(gpu, built[1][1], ("montgomery", "canonical"), keep)
    assert _launches(gpu, lambda: out.update(proof=custom.prove_many(keys, [built[0][1], wit], seeds=[3, 40]))) == 1
    assert out["proof"] == want
    keys.release()
    params.release()


def test_a_key_whose_fixed_columns_and_table_are_integers(gpu):
    """the range circuit's key with every fixed column that holds small integers handed over as engine.IntCells, the lookup table (256
    dense cells: the kernel; keygen sorts it on the host through the same conversion) among them: the vk bytes, the resident fixed rows
    and a proof are the plain key's"""
    import copy

    from halo2_scaffold_amd import engine, flex

    k, seed = 9, 23
    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    cs = flex.FlexGateCS(lookup=True)
    asg = flex.range_closure(cs, 0x0123456789ABCDEF, 8)
    plain = flex.FlexKeys(params, cs, asg)
    fixed = list(asg.fixed)
    fixed[cs.col_table] = dict(enumerate(asg.table_values))
    converted = 0
    for j, cells in enumerate(fixed):
        if cells and all(v % R < 2**63 or R - v % R <= 2**63 for v in cells.values()):
            rows = sorted(cells)
            dense = rows == list(range(len(rows)))
            fixed[j] = engine.IntCells(_i64([cells[r] % R for r in rows]), None if dense else np.array(rows, dtype=np.uint32))
            converted += 1
    assert converted >= 2 and isinstance(fixed[cs.col_table], engine.IntCells)
    index = {col: j for j, col in enumerate(cs.perm_columns)}
    copies = [(index[(left[0], left[1])], left[2], index[(right[0], right[1])], right[2]) for left, right in asg.copies]
    made = {}
    assert _launches(gpu, lambda: made.update(keys=engine.Keys(cs.abi(k), params, fixed, copies))) == 1
    ints = copy.copy(plain)  # the same front-end object over the other library key
    ints.keys = made["keys"]
    assert np.array_equal(ints.keys.fixed_commitments, plain.fixed_commitments)
    assert np.array_equal(ints.keys.permutation_commitments, plain.permutation_commitments)
    vk, repr_ = flex.transcript_repr(k, cs.degree, ints.keys.fixed_commitments, ints.keys.permutation_commitments)
    assert vk == plain.vk_bytes() and repr_ == plain.transcript_repr
    n = 1 << k
    for a, b in zip(ints.keys.views(engine.PKBUF_FIXED, cs.n_fixed), plain.fixed_values):
        assert np.array_equal(a.to_numpy(shape=(n, 4), nbytes=n * 32), b.to_numpy(shape=(n, 4), nbytes=n * 32))
    assert flex.create_proof(params, ints, asg, seed) == flex.create_proof(params, plain, asg, seed)
    ints.keys.release()
    plain.release()
    params.release()


def test_public_inputs_as_integers(gpu):
    """h2mi_prover_instances takes H2MI_CELLS_I64 from the host: the proof of the same public inputs as field elements"""
    from halo2_scaffold_amd import custom, engine

    meta = custom.ConstraintSystem()
    a = meta.advice_column()
    inst = [meta.instance_column(), meta.instance_column()]
    s = meta.selector()
    meta.enable_equality(a)
    cur = custom.Rotation.cur()
    meta.create_gate("public", lambda meta: [meta.query_selector(s) * (meta.query_advice(a, cur) - meta.query_instance(inst[0], cur) - meta.query_instance(inst[1], cur))])
    public = [[4, R - 5], [7]]
    region = custom.Assignment(meta, instance=public)
    region.assign_advice(a, 0, 11)
    region.enable_selector(s, 0)
    params = gpu.ParamsKZG.setup(5, SRS_SECRET)
    keys = custom.Keys(params, meta, region)
    ws = custom.Workspace(params, keys)
    want = custom.create_proof(params, keys, region, 7, ws=ws)
    # the same proof driven by hand: the public inputs through IntCells, then the advice call with none of its own
    t = custom.flex.Blake2bWrite.init()
    t.common_scalar(custom.flex._m(keys.transcript_repr))
    for v in engine.instance_values(public):
        t.common_scalar(custom.flex._m(v))
    p = ws.prover
    p.set_instances([engine.IntCells(np.array([4, -5], dtype=np.int64)), engine.IntCells(np.array([7], dtype=np.int64))])
    p.drive(region.advice, [], 7, t)
    assert t.finalize() == want
    ws.release()
    keys.release()
    params.release()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_device_cells_refuse_unfit_device_tensors(gpu):
    """tensors that are on the device but not contiguous, of a wrong dtype or of a wrong shape: ValueError before any pointer is taken"""
    import torch

    from halo2_scaffold_amd import engine

    limbs = torch.zeros((8, 4), dtype=torch.int64, device="cuda:0")
    ints = torch.zeros(8, dtype=torch.int64, device="cuda:0")
    assert gpu.lib.h2mi_primary_device() == 0
    assert len(engine.DeviceCells(limbs)) == 8 and len(engine.DeviceCells(ints, fmt="i64", rows=ints.to(torch.int32))) == 8
    for values, kw in ((limbs.t(), {}), (limbs[::2], {}), (limbs[:, :2], {}), (ints[::2], {"fmt": "i64"}), (limbs.to(torch.int32), {}), (limbs.double(), {}),
                       (ints, {}), (limbs, {"fmt": "i64"}), (ints.to(torch.int32), {"fmt": "i64"}), (limbs, {"count": 7})):
        with pytest.raises(ValueError):
            engine.DeviceCells(values, **kw)
    for rows in (ints[:4], ints.to(torch.int16), ints.double(), torch.zeros(16, dtype=torch.int32, device="cuda:0")[::2], torch.zeros(8, dtype=torch.int32)):
        with pytest.raises(ValueError):
            engine.DeviceCells(limbs, rows=rows)
    # an int64 row list is converted once, on the device; what does not fit a row stays out of range
    wide = torch.tensor([0, 5, -1, 1 << 40, (1 << 32) + 3, 7, 2, 1], dtype=torch.int64, device="cuda:0")
    col = engine.DeviceCells(limbs, rows=wide)
    got = col._tensors[-1]
    assert got.dtype == torch.int32 and got.cpu().tolist() == [0, 5, -1, 0x7FFFFFFF, 0x7FFFFFFF, 7, 2, 1]


_TWO_DEVICE_WORKER = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import torch  # first: one HIP runtime
import _load_pkg
h2 = _load_pkg.load()
from halo2_scaffold_amd import custom, engine
from halo2_scaffold_amd._lib import H2miError, check
import assigned_cases as A
check(h2.lib.h2mi_init_devices(2), "init_devices")
assert h2.lib.h2mi_device_count() == 2 and h2.lib.h2mi_primary_device() == 0
R = engine.F.FR_MODULUS
cells = {{r: (r * 0x123456789 - (1 << 40)) % R for r in range(40)}}  # 40 dense cells: the kernel's route for host integers
cs, asg = A.columns_circuit(custom, [cells])
params = h2.ParamsKZG.setup(8, 0x5EC2E7)
keys = custom.Keys(params, cs, asg)
ws = custom.Workspace(params, keys)
want = custom.create_proof(params, keys, asg, 5, ws=ws)
class W: pass
w = W(); w.instance = asg.instance
w.advice = [engine.IntCells(np.array([r * 0x123456789 - (1 << 40) for r in range(40)], dtype=np.int64))]
assert custom.create_proof(params, keys, w, 5, ws=ws) == want  # host integers are taken with any number of devices
buf = h2.DevBuf.from_numpy(np.zeros((40, 4), dtype=np.uint64))
for fmt in ("montgomery", "canonical", "i64"):
    w.advice = [engine.DeviceCells(buf, fmt=fmt, count=40)]
    try:
        custom.create_proof(params, keys, w, 5, ws=ws)
        raise SystemExit("device cells were taken under two devices")
    except H2miError as e:
        assert e.code == -1, e.code
    assert custom.create_proof(params, keys, asg, 5, ws=ws) == want
print("TWO_DEVICES_OK")
"""


def test_device_cells_are_refused_with_more_than_one_device(gpu, tmp_path):
    """a child process under h2mi_init_devices(2) (virtual on a one-GPU box): H2MI_CELLS_DEVICE is H2MI_EINVAL from the advice call and
    the prover stays usable; host int64 cells are taken as ever"""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "two_devices.py"
    script.write_text(_TWO_DEVICE_WORKER.format(root=root, tests=os.path.join(root, "tests")))
    env = dict(os.environ, H2MI_VIRTUAL_DEVICES="1", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "TWO_DEVICES_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_refusals_leave_the_prover_usable(gpu):
    """a bad device row and a bad canonical value each return their code from the advice call; the flag rules on advice, instances and
    keygen; a dense device run of u + 1 cells is refused before any launch.  After each the next proof on the same prover has its bytes."""
    from halo2_scaffold_amd import custom, engine
    from halo2_scaffold_amd._lib import H2miError

    k = 6
    usable = (1 << k) - 6
    rng = random.Random("refusals")
    good = A.dense([rng.randrange(R) for _ in range(40)])
    meta = custom.ConstraintSystem()
    a = meta.advice_column()
    inst = meta.instance_column()
    s = meta.selector()
    meta.enable_equality(a)
    meta.create_gate("public", lambda meta: [meta.query_selector(s) * (meta.query_advice(a, custom.Rotation.cur()) - meta.query_instance(inst, custom.Rotation.cur()))])

    def assignment(cells):
        region = custom.Assignment(meta, instance=[4, 5])
        for row, v in cells.items():
            region.assign_advice(a, row, v)
        return region

    params = gpu.ParamsKZG.setup(k, SRS_SECRET)
    keys = custom.Keys(params, meta, assignment(good))
    ws = custom.Workspace(params, keys)
    want = custom.create_proof(params, keys, assignment(good), 7, ws=ws)
    keep = []
    again = lambda: custom.create_proof(params, keys, _converted(gpu, assignment(good), ("canonical",), keep), 7, ws=ws)
    assert again() == want

    def refused(wit, code, before_any_launch=False):
        def call():
            with pytest.raises(H2miError) as e:
                custom.create_proof(params, keys, wit, 7, ws=ws)
            assert e.value.code == code

        scatter, every = _launches(gpu, call, allow_none=True)
        assert not before_any_launch or (scatter, every) == (0, 0)
        assert again() == want

    # a listed row at the first blinding row, among good ones; a far one; every format
    for fmt in ("montgomery", "canonical", "i64"):
        for bad_row in (usable, (1 << k) - 1, 1 << k, 0xFFFFFFFF):
            cells = {2 * r: 3 + r for r in range(20)}
            wit = _converted(gpu, assignment(cells), (fmt,), keep)
            rows = np.array([2 * r for r in range(20)], dtype=np.uint32)
            rows[7] = bad_row
            d_rows = gpu.DevBuf.from_numpy(rows)
            keep.append(d_rows)
            wit.advice[0] = engine.DeviceCells(wit.advice[0].values_ptr, rows=d_rows, fmt=fmt, count=20)
            refused(wit, ERANGE)
    # a canonical value that is not below r: r itself, 2^256 - 1; short and long columns
    for count, bad in ((9, R), (40, (1 << 256) - 1)):
        limbs = o.pack([5 + i for i in range(count)])
        limbs[count // 2] = D.limbs(bad)
        buf = gpu.DevBuf.from_numpy(limbs)
        keep.append(buf)
        refused(_Witness([engine.DeviceCells(buf, fmt="canonical")], [4, 5]), EINVAL)
    # a dense device run of u + 1 cells: H2MI_ERANGE before any launch
    buf = gpu.DevBuf.from_numpy(o.pack(list(range(usable + 1))))
    keep.append(buf)
    for fmt in FORMS:
        refused(_Witness([engine.DeviceCells(buf, fmt=fmt)], [4, 5]), ERANGE, before_any_launch=True)
    assert custom.create_proof(params, keys, _Witness([engine.DeviceCells(buf, fmt="canonical", count=usable)], [4, 5]), 7, ws=ws) \
        == custom.create_proof(params, keys, assignment(dict(enumerate(range(usable)))), 7, ws=ws)
    # the flag rules, on the advice call ...
    lib, h = gpu.lib, ws.prover.handle
    pts, inst_limbs = np.zeros((8, 8), dtype=np.uint64), o.pack([4, 5], R)
    column = (engine.ColumnCells * 1)()
    column[0].values, column[0].count = buf.ptr, 4
    for flags in (engine.CELLS_DEVICE | engine.CELLS_RATIONAL, engine.CELLS_I64 | engine.CELLS_CANONICAL, engine.CELLS_I64 | engine.CELLS_RATIONAL, 16,
                  engine.CELLS_DEVICE | 32):
        column[0].flags = flags
        assert lib.h2mi_prover_advice(h, column, inst_limbs.ctypes.data, 2, 7, pts.ctypes.data) == EINVAL, flags
        assert again() == want
    column[0].flags, column[0].values = engine.CELLS_DEVICE, buf.ptr + 8  # a misaligned device pointer
    assert lib.h2mi_prover_advice(h, column, inst_limbs.ctypes.data, 2, 7, pts.ctypes.data) == EINVAL and again() == want
    column[0].values = buf.ptr
    # ... on the public inputs ...
    for flags in (engine.CELLS_DEVICE, engine.CELLS_DEVICE | engine.CELLS_I64, engine.CELLS_I64 | engine.CELLS_CANONICAL, 16):
        column[0].flags = flags
        assert lib.h2mi_prover_instances(h, column) == EINVAL
        assert again() == want  # a refusal leaves nothing behind
    # ... and at keygen
    for first in (engine.DeviceCells(buf, fmt="canonical", count=4), engine.DeviceCells(buf, fmt="i64", count=4)):
        with pytest.raises(H2miError) as e:
            engine.Keys(meta.abi(k), params, [first] + [{}] * (meta.n_fixed - 1), [], gates=meta.gate_program())
        assert e.value.code == EINVAL
    assert again() == want
    ws.release()
    keys.release()
    params.release()
