"""CPU tests of the device-cells hand-over (H2MI_CELLS_I64 / H2MI_CELLS_DEVICE): the shared cases against pow / %, the Python packing
(engine.IntCells, engine.DeviceCells, pack_cells) and the host-only validator h2mi_column_cells_check.  No cell memory is read and no
device is needed: the pointers of the device columns are made-up addresses."""
import ctypes as C

import numpy as np
import pytest

import device_cells_cases as D
import keygen_call

EINVAL, ERANGE = -1, -6


@pytest.fixture(scope="module")
def engine(h2):
    from halo2_scaffold_amd import engine

    return engine


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def test_cases_check_themselves():
    rinv = pow(1 << 256, -1, D.R)
    value = lambda word: sum(int(w) << (64 * j) for j, w in enumerate(word))
    assert D.R == 21888242871839275222246405745257275088548364400416034343698204186575808495617
    for v in D.I64_EDGES:
        assert -(2**63) <= v < 2**63
        got = value(D.mont(v)) * rinv % D.R
        assert got == (v if v >= 0 else D.R - abs(v)) and value(D.mont(v)) < D.R
    assert value(D.mont(-(2**63))) * rinv % D.R == D.R - 2**63
    assert all(0 <= v < D.R for v in D.CANONICAL_EDGES) and (1 << 256) % D.R in D.CANONICAL_EDGES
    assert value(D.mont((1 << 256) % D.R)) == pow(2, 512, D.R)  # the Montgomery form of 2^256 mod r is R^2
    assert [v for v in D.CANONICAL_EDGES if v in (D.MASK64, D.MASK64 << 64, D.MASK64 << 128)] and (D.MASK64 << 192) >= D.R
    assert any(v >= D.R for v in D.MONTGOMERY_EDGES)  # unreduced words are carried verbatim
    for fmt in D.FORMATS:
        for count in (1, 65, 300):
            src, want = D.case(fmt, count)
            assert src.shape == ((count,) if fmt == "i64" else (count, 4)) and want.shape == (count, 4)
            assert src.dtype == (np.int64 if fmt == "i64" else np.uint64) and want.dtype == np.uint64
            vals = D.values(fmt, count)
            for i in (0, count // 2, count - 1):
                if fmt == "montgomery":
                    assert value(want[i]) == vals[i]
                else:
                    assert value(want[i]) * rinv % D.R == vals[i] % D.R and value(want[i]) < D.R
    assert D.COUNTS == sorted(D.COUNTS) and {1, 64, 65, 4096, 4097, 2**13 - 6} <= set(D.COUNTS)


def test_row_lists():
    limit = 3 * (2**13 - 6) + 2
    for count in D.COUNTS:
        assert D.rows("dense", count, limit) is None
        for kind in D.ROW_LISTS:
            r = D.rows(kind, count, limit)
            assert r.dtype == np.uint32 and len(set(r.tolist())) == count and int(r.max()) < limit
        if count > 1:
            ends = D.rows("ends", count, limit).tolist()
            assert 0 in ends and limit - 1 in ends
        assert D.rows("reversed", count, limit)[0] == count - 1
    src, want = D.case("i64", 5)
    out = D.expected_column(9, np.array([8, 0, 3, 4, 6], dtype=np.uint32), want)
    assert np.array_equal(out[8], want[0]) and np.array_equal(out[1], D.SENTINEL) and np.array_equal(out[6], want[4])
    assert len(D.many_columns()) == 64 and {c[2] for c in D.many_columns()} >= {0, 1, 65, 4097}


# ---- Python packing ------------------------------------------------------------------------------------------------------------------
def test_constants_and_struct(engine):
    assert (engine.CELLS_CANONICAL, engine.CELLS_RATIONAL, engine.CELLS_I64, engine.CELLS_DEVICE) == (1, 2, 4, 8)
    assert (engine.CELLS_FOR_ADVICE, engine.CELLS_FOR_INSTANCE, engine.CELLS_FOR_FIXED) == (0, 1, 2)
    assert C.sizeof(engine.CellsSource) == 40 and engine.CellsSource.format.offset == 36


def test_int_cells_packing(engine):
    a = np.array([5, -1, 2**40], dtype=np.int64)
    rows = np.array([7, 2, 9], dtype=np.uint32)
    arr, keep = engine.pack_cells([engine.IntCells(a), engine.IntCells(a, rows), engine.IntCells(np.zeros(0, dtype=np.int64))])
    assert (arr[0].flags, arr[0].count, arr[0].rows) == (engine.CELLS_I64, 3, None)  # no rows for a dense column
    assert np.array_equal(np.ctypeslib.as_array(C.cast(arr[0].values, C.POINTER(C.c_int64)), (3,)), a)  # the array itself crosses
    assert (arr[1].flags, arr[1].count) == (engine.CELLS_I64, 3) and arr[1].rows and arr[1].values
    assert np.array_equal(np.ctypeslib.as_array(C.cast(arr[1].rows, C.POINTER(C.c_uint32)), (3,)), rows)
    assert (arr[2].count, arr[2].values, arr[2].rows) == (0, None, None)
    engine.cells_check(arr, 3, engine.CELLS_FOR_ADVICE)
    engine.cells_check(arr, 3, engine.CELLS_FOR_FIXED)
    engine.cells_check(arr, 1, engine.CELLS_FOR_INSTANCE)
    # a strided view is copied, not read with the wrong stride
    arr, keep = engine.pack_cells([engine.IntCells(np.arange(10, dtype=np.int64)[::2])])
    assert np.array_equal(np.ctypeslib.as_array(C.cast(arr[0].values, C.POINTER(C.c_int64)), (5,)), [0, 2, 4, 6, 8])
    for bad in (np.array([1, 2], dtype=np.int32), np.array([1.0]), np.zeros((2, 2), dtype=np.int64), [1 << 70]):
        with pytest.raises(ValueError):
            engine.IntCells(bad)
    for bad_rows in (np.array([1, 2, 3], dtype=np.int64), np.array([1, 2], dtype=np.uint32)):
        with pytest.raises(ValueError):
            engine.IntCells(a, bad_rows)


def test_device_cells_packing_from_addresses(engine):
    base = 0x7F0000000000
    for fmt, flags in (("montgomery", 8), ("canonical", 9), ("i64", 12)):
        arr, keep = engine.pack_cells([engine.DeviceCells(base, fmt=fmt, count=11), engine.DeviceCells(base, rows=base + 4096, fmt=fmt, count=11)])
        assert (arr[0].flags, arr[0].count, arr[0].values, arr[0].rows) == (flags, 11, base, None)
        assert (arr[1].flags, arr[1].count, arr[1].values, arr[1].rows) == (flags, 11, base, base + 4096)
        engine.cells_check(arr, 2, engine.CELLS_FOR_ADVICE)
    view = engine.DevView(base, 6)  # six field elements: 192 bytes
    assert len(engine.DeviceCells(view)) == 6 and len(engine.DeviceCells(view, fmt="i64")) == 24 and len(engine.DeviceCells(view, fmt="i64", count=5)) == 5
    arr, _ = engine.pack_cells([engine.DeviceCells(base, count=0)])
    assert (arr[0].count, arr[0].values) == (0, None)
    with pytest.raises(ValueError):
        engine.DeviceCells(base)  # an address needs count
    with pytest.raises(ValueError):
        engine.DeviceCells(view, count=7)
    with pytest.raises(ValueError):
        engine.DeviceCells(base, fmt="rational", count=1)
    with pytest.raises(ValueError):
        engine.DeviceCells([1, 2, 3])


def test_device_cells_refuse_host_tensors(engine):
    import torch

    limbs = torch.zeros((6, 4), dtype=torch.int64)
    for values, kw in ((limbs, {}), (limbs[:, 0], {"fmt": "i64"}), (limbs.t(), {}), (torch.zeros(6, dtype=torch.int64), {"fmt": "i64"})):
        with pytest.raises(ValueError):
            engine.DeviceCells(values, **kw)  # a CPU tensor, contiguous or not
    with pytest.raises(ValueError):
        engine.DeviceCells(0x7F0000000000, rows=torch.zeros(6, dtype=torch.int32), count=6)


def test_pack_cells_keeps_the_existing_forms_byte_for_byte(engine):
    """dict and list columns give the structures and the bytes they always gave, alone or beside new-style columns"""
    plain = [{0: 5, 1: 6, 2: 7}, {9: 1, 4: D.R - 1}, [3, 4, 5], {}, [engine.Rational(1, 3), 2]]
    ints = engine.IntCells(np.array([1, -2, 3], dtype=np.int64))
    dev = engine.DeviceCells(0x7F0000000000, fmt="i64", count=4)

    def image(arr, i):
        c = arr[i]
        width = 64 if c.flags & engine.CELLS_RATIONAL else 32
        values = C.string_at(c.values, c.count * width) if c.count else b""
        rows = C.string_at(c.rows, c.count * 4) if c.rows else None
        return c.count, c.flags, values, rows

    alone, keep_a = engine.pack_cells(plain)
    mixed, keep_m = engine.pack_cells([ints, plain[0], dev, plain[1], plain[2], ints, plain[3], plain[4], dev])
    for i, j in enumerate((1, 3, 4, 6, 7)):
        assert image(alone, i) == image(mixed, j)
    assert image(alone, 0) == (3, engine.CELLS_CANONICAL, b"".join(v.to_bytes(32, "little") for v in (5, 6, 7)), None)
    assert image(alone, 1)[3] == np.array([4, 9], dtype=np.uint32).tobytes() and image(alone, 3) == (0, 0, b"", None)
    assert image(alone, 4)[1] == engine.CELLS_CANONICAL | engine.CELLS_RATIONAL
    assert (mixed[0].flags, mixed[2].flags, mixed[5].flags, mixed[8].flags) == (4, 12, 4, 12)


# ---- h2mi_column_cells_check -------------------------------------------------------------------------------------------------------
def _column(engine, flags, count=3, values=0x1000, rows=None):
    arr = (engine.ColumnCells * 1)()
    arr[0].flags, arr[0].count, arr[0].values, arr[0].rows = flags, count, values, rows
    return arr


def test_column_cells_check_flag_rules(h2, engine):
    chk = h2.lib.h2mi_column_cells_check
    A, I, F = engine.CELLS_FOR_ADVICE, engine.CELLS_FOR_INSTANCE, engine.CELLS_FOR_FIXED
    CAN, RAT, I64, DEV = 1, 2, 4, 8
    allowed = {A: {0, CAN, RAT, CAN | RAT, I64, DEV, DEV | CAN, DEV | I64}, F: {0, CAN, RAT, CAN | RAT, I64}, I: {0, CAN, I64}}
    for where, ok in allowed.items():
        for flags in range(16):
            assert chk(_column(engine, flags), 1, where) == (0 if flags in ok else EINVAL), (where, flags)
        for flags in (16, 32, 1 << 31, 16 | I64, 0x100 | DEV):  # unknown bits, alone and beside known ones
            assert chk(_column(engine, flags), 1, where) == EINVAL
    for where in (3, 7, 0xFFFFFFFF):
        assert chk(_column(engine, 0), 1, where) == EINVAL
    # every column is looked at, and none when there are none
    two = (engine.ColumnCells * 2)()
    two[0].flags, two[0].count, two[0].values = 0, 1, 0x1000
    two[1].flags, two[1].count, two[1].values = I64 | CAN, 1, 0x1000
    assert chk(two, 1, A) == 0 and chk(two, 2, A) == EINVAL
    assert chk(None, 0, A) == 0 and chk(None, 1, A) == EINVAL


def test_column_cells_check_pointers_and_counts(h2, engine):
    chk = h2.lib.h2mi_column_cells_check
    A, I, F = engine.CELLS_FOR_ADVICE, engine.CELLS_FOR_INSTANCE, engine.CELLS_FOR_FIXED
    CAN, I64, DEV = 1, 4, 8
    for where in (A, I, F):
        assert chk(_column(engine, 0, count=3, values=None), 1, where) == EINVAL  # NULL values with count > 0
        assert chk(_column(engine, 0, count=0, values=None), 1, where) == 0
        assert chk(_column(engine, I64, values=0x1004), 1, where) == EINVAL  # I64 values: 8 bytes
        assert chk(_column(engine, I64, values=0x1008), 1, where) == 0
        assert chk(_column(engine, CAN, values=0x1008), 1, where) == 0  # host field elements are uint64_t words
        assert chk(_column(engine, CAN, values=0x1004), 1, where) == EINVAL
        assert chk(_column(engine, 0, count=(1 << 28) + 1), 1, where) == ERANGE and chk(_column(engine, 0, count=1 << 28), 1, where) == 0
    for where in (A, F):
        assert chk(_column(engine, 0, rows=0x2004), 1, where) == 0
        assert chk(_column(engine, 0, rows=0x2002), 1, where) == EINVAL  # rows: 4 bytes
        assert chk(_column(engine, I64, rows=0x2001), 1, where) == EINVAL
    assert chk(_column(engine, 0, rows=0x2004), 1, I) == EINVAL  # public inputs lie on rows 0 .. count - 1
    # device columns: 16 bytes for 32-byte values, 8 for I64, 4 for rows
    for flags in (DEV, DEV | CAN):
        assert chk(_column(engine, flags, values=0x1010), 1, A) == 0
        assert chk(_column(engine, flags, values=0x1008), 1, A) == EINVAL
    assert chk(_column(engine, DEV | I64, values=0x1008), 1, A) == 0 and chk(_column(engine, DEV | I64, values=0x100C), 1, A) == EINVAL
    assert chk(_column(engine, DEV | I64, values=0x1008, rows=0x2004), 1, A) == 0
    assert chk(_column(engine, DEV | I64, values=0x1008, rows=0x2006), 1, A) == EINVAL
    assert chk(_column(engine, DEV, count=4, values=None), 1, A) == EINVAL


def test_the_entry_points_apply_the_check_before_any_device_work(h2, engine):
    """keygen answers H2MI_EINVAL to cells the check refuses whether or not there is a device: the check comes first"""
    cs = engine.ConstraintSystem.build(5, 3, 5, 0, 3, 5, engine.GATES_STANDARD_PLONK, [], [(engine.ADVICE, 0)], [], [(0, 0)], [(0, 0)])
    fixed = (engine.ColumnCells * 5)()
    for flags in (engine.CELLS_DEVICE, engine.CELLS_DEVICE | engine.CELLS_I64, engine.CELLS_I64 | engine.CELLS_CANONICAL, 16):
        fixed[2].flags = flags
        assert keygen_call.keygen(cs, g_lagrange=1, fixed=fixed, pk=0) == (EINVAL, None)
