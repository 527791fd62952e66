"""Cost of the witness hand-over: h2mi_prover_advice with three columns of 2^k - 6 cells as host Montgomery cells (the baseline, measured in
the same run), host int64 (H2MI_CELLS_I64), device 32-byte cells and device int64 (H2MI_CELLS_DEVICE), dense and scattered (every usable
row, in shuffled order).  Alternating, best of three; each form as a ratio to the host Montgomery form of the same run; k_cells_scatter's
own time from the launch profile and the bytes it moved over that time as a share of the HBM roofline (8 TB/s).  Sizes from argv
(default 16 20 22).  The four forms hold the same values: their commitments are compared before anything is timed."""
import ctypes as C, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch  # noqa: F401  (torch first: one HIP runtime)
import _load_pkg
h2 = _load_pkg.load(); h2.init(0)
from halo2_scaffold_amd import custom, engine
lib = h2.lib
HBM = 8e12
def t(fn, R):
    for _ in range(2): fn()
    lib.h2mi_sync(); t0 = time.perf_counter()
    for _ in range(R): fn()
    lib.h2mi_sync(); return (time.perf_counter() - t0) / R
def scatter_ms(fn):
    """(device ms, launches) of k_cells_scatter during one call, from the library's launch profile"""
    lib.h2mi_profile_reset(); lib.h2mi_profile_filter(b"k_cells_scatter"); lib.h2mi_profile_enable(1)
    fn(); lib.h2mi_sync(); lib.h2mi_profile_enable(0)
    ms, count = C.c_double(), C.c_uint64()
    lib.h2mi_profile_query(b"k_cells_scatter", C.byref(ms), C.byref(count)); lib.h2mi_profile_reset(); lib.h2mi_profile_filter(b"")
    return ms.value, count.value
def circuit(n_columns=3):
    meta = custom.ConstraintSystem()
    cols = [meta.advice_column() for _ in range(n_columns)]
    s = meta.selector(); meta.enable_equality(cols[0])
    meta.create_gate("unused", lambda meta: [meta.query_selector(s) * (meta.query_advice(cols[0], 0) * meta.query_advice(cols[1], 0) - meta.query_advice(cols[2], 0))])
    return meta, custom.Assignment(meta)
for log in [int(x) for x in sys.argv[1:]] or [16, 20, 22]:
    cells = (1 << log) - 6  # the usable rows of a column of 2^log rows
    rng = np.random.default_rng(log)
    ints = [rng.integers(-(1 << 63), (1 << 63) - 1, size=cells, dtype=np.int64, endpoint=True) for _ in range(3)]
    perm = [rng.permutation(cells).astype(np.uint32) for _ in range(3)]
    d_ints, d_rows = [h2.DevBuf.from_numpy(a) for a in ints], [h2.DevBuf.from_numpy(r) for r in perm]
    # the same values as Montgomery words: converted once by the kernel under test (its words are the test-suite's business)
    d_words = [h2.DevBuf(32 * cells) for _ in range(3)]
    src = (engine.CellsSource * 3)()
    for j in range(3):
        src[j].d_column, src[j].values, src[j].count, src[j].row_limit, src[j].format = d_words[j].ptr, d_ints[j].ptr, cells, cells, engine.CELLS_I64
    status = (C.c_uint64 * 2)()
    engine.check(lib.h2mi_fr_scatter_cells_dev(src, 3, status, None), "scatter"); assert tuple(status) == (0, 0)
    words = [np.ascontiguousarray(b.to_numpy(shape=(cells, 4))) for b in d_words]
    params = h2.ParamsKZG.setup(log, 0x5EC2E7)
    cs, asg = circuit()
    keys = custom.Keys(params, cs, asg); ws = custom.Workspace(params, keys)
    pts = ws.prover._points.ctypes.data
    def advice(flags, values, rows):
        cc = (engine.ColumnCells * 3)()
        for j in range(3):
            cc[j].values, cc[j].count, cc[j].flags = values[j], cells, flags
            if rows is not None: cc[j].rows = rows[j]
        return lambda: engine.check(lib.h2mi_prover_advice(ws.prover.handle, cc, None, 0, 5, pts), "advice")
    host_rows, dev_rows = [r.ctypes.data for r in perm], [b.ptr for b in d_rows]
    R = 5 if log <= 20 else 3
    for shape in ("dense", "scattered"):
        hr, dr = (None, None) if shape == "dense" else (host_rows, dev_rows)
        forms = {"host montgomery": advice(0, [w.ctypes.data for w in words], hr), "host i64": advice(engine.CELLS_I64, [a.ctypes.data for a in ints], hr),
                 "device 32-byte": advice(engine.CELLS_DEVICE, [b.ptr for b in d_words], dr), "device i64": advice(engine.CELLS_DEVICE | engine.CELLS_I64, [b.ptr for b in d_ints], dr)}
        points = {}
        for name, run in forms.items():
            run(); points[name] = ws.prover._points[:3].copy()
            assert np.array_equal(points[name], points["host montgomery"]), f"{name} commits to different points"
        times = {name: [] for name in forms}
        for _ in range(3):  # alternating, the best of three
            for name, run in forms.items(): times[name].append(t(run, R))
        base = min(times["host montgomery"])
        for name, run in forms.items():
            best = min(times[name])
            line = f"log={log} {shape:9s} 3 x {cells} cells  {name:15s} {best*1e3:8.3f} ms  x{best/base:5.2f} of host montgomery  (all runs: {[round(x*1e3, 2) for x in times[name]]})"
            ms, launches = scatter_ms(run)
            if launches:
                per_cell = (8 if "i64" in name else 32) + 32 + (4 if shape == "scattered" else 0)
                line += f"  k_cells_scatter x{launches}: {ms:7.4f} ms, {per_cell} B per cell = {3*cells*per_cell/1e6:7.1f} MB, {3*cells*per_cell/(ms*1e-3)/HBM*100:5.1f}% of the HBM roofline"
            print(line, flush=True)
    ws.release(); keys.release(); params.release()
    for b in d_ints + d_rows + d_words: b.free()
