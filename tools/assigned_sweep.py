"""Timing of assigned cells (H2MI_CELLS_RATIONAL): the device resolve chain alone, the same chain fed from host memory (upload + resolve),
h2mi_prover_advice with rational against plain cells, and the CPU batched inversion a fork pays today (oracle.vec's C batch_inv: on one thread, and in 16 chunks per column on 16 threads).
3 columns of 2^log cells per size; sizes from argv (default 16 20 22)."""
import ctypes as C, os, sys, time
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import _load_pkg
h2 = _load_pkg.load(); h2.init(0)
from halo2_scaffold_amd import custom, engine, synth
from oracle.vec import FV
lib = h2.lib
CHAIN = ("k_assigned_tile_products", "k_assigned_tile_inverses", "k_assigned_finish")
def t(fn, R=10):
    for _ in range(2): fn()
    lib.h2mi_sync(); t0 = time.perf_counter()
    for _ in range(R): fn()
    lib.h2mi_sync(); return (time.perf_counter() - t0) / R
def kernel_ms(fn):
    """device time per kernel of one call, from the library's launch profile"""
    lib.h2mi_profile_reset(); lib.h2mi_profile_filter(b""); lib.h2mi_profile_enable(1)
    fn(); lib.h2mi_sync(); lib.h2mi_profile_enable(0)
    ms, count, out = C.c_double(), C.c_uint64(), {}
    for name in CHAIN:
        lib.h2mi_profile_query(name.encode(), C.byref(ms), C.byref(count)); out[name] = (round(ms.value, 4), count.value)
    lib.h2mi_profile_reset(); return out
class AssignedCells(C.Structure):
    _fields_ = [("d_column", C.c_void_p), ("rows", C.c_void_p), ("pairs", C.c_void_p), ("count", C.c_size_t)]
def circuit(n_columns=3):
    meta = custom.ConstraintSystem()
    cols = [meta.advice_column() for _ in range(n_columns)]
    s = meta.selector(); meta.enable_equality(cols[0])
    meta.create_gate("unused", lambda meta: [meta.query_selector(s) * (meta.query_advice(cols[0], 0) * meta.query_advice(cols[1], 0) - meta.query_advice(cols[2], 0))])
    return meta, custom.Assignment(meta)
for log in [int(x) for x in sys.argv[1:]] or [16, 20, 22]:
    cells = (1 << log) - 6  # the usable rows of a column of 2^log rows
    total = 3 * cells
    pairs = [np.ascontiguousarray(synth.uniform_fr(2 * cells, 11 + j)) for j in range(3)]  # Montgomery words: (numerator, denominator) per cell
    for p in pairs: p[1::2 * 97] = 0  # a zero denominator every 97 cells
    # 1. the chain alone, device resident
    d_pairs, d_out = h2.DevBuf.from_numpy(np.concatenate(pairs)), h2.DevBuf(32 * total)
    chain = lambda: lib.h2mi_fr_assigned_evaluate_dev(d_pairs.ptr, total, d_out.ptr, None)
    t_chain, k_chain = t(chain), kernel_ms(chain)
    resolved = d_out.to_numpy(shape=(total, 4))
    # 2. the same from host memory into three columns: upload of 64 B per cell + the chain; against the upload of resolved cells
    columns = [h2.DevBuf(32 << log) for _ in range(3)]
    arr = (AssignedCells * 3)()
    for j in range(3): arr[j].d_column, arr[j].pairs, arr[j].count = columns[j].ptr, pairs[j].ctypes.data, cells
    t_cols = t(lambda: lib.h2mi_fr_assigned_columns_dev(arr, 3, 0, None, None))
    plain = [np.ascontiguousarray(resolved[j * cells:(j + 1) * cells]) for j in range(3)]
    t_up = t(lambda: [lib.h2mi_memcpy_h2d(columns[j].ptr, plain[j].ctypes.data, 32 * cells) for j in range(3)])
    for j in range(3): assert np.array_equal(columns[j].to_numpy(shape=(cells, 4), nbytes=32 * cells), plain[j])
    for b in columns + [d_pairs, d_out]: b.free()
    # 3. what the crate spends today: batch_invert_assigned on the CPU — oracle.vec's C loop, serial in itself, on ONE thread and on 16:
    # every column cut into 16 chunks, each with its own inversion (the crate's split of a column over its threads), the 48 chunks on a
    # pool of 16 threads (the C calls release the interpreter lock); the chunks are laid out before the clock starts
    dens = [FV(np.ascontiguousarray(p[1::2])) for p in pairs]
    t0 = time.perf_counter(); [(FV(np.ascontiguousarray(p[0::2])) * d.batch_inv()) for p, d in zip(pairs, dens)]; t_cpu = time.perf_counter() - t0
    chunks = [(FV(np.ascontiguousarray(c[:, :4])), FV(np.ascontiguousarray(c[:, 4:]))) for p in pairs for c in np.array_split(p.reshape(-1, 8), 16)]  # a row per cell
    with ThreadPoolExecutor(16) as pool:
        list(pool.map(lambda nd: nd[0] * nd[1].batch_inv(), chunks[:16]))  # threads started, library loaded
        t0 = time.perf_counter(); got = list(pool.map(lambda nd: nd[0] * nd[1].batch_inv(), chunks)); t_cpu16 = time.perf_counter() - t0
    assert np.array_equal(np.concatenate([g.a for g in got]), resolved), "the CPU pass and the device chain differ"
    print(f"log={log}: CPU batch_inv + mul on 16 threads (48 chunks, one inversion each) {t_cpu16*1e3:8.1f} ms, equal to the device chain's cells", flush=True)
    print(f"log={log} 3 x {cells} cells: chain alone {t_chain*1e3:8.3f} ms (kernels {k_chain}; {96*total/t_chain/8e12*100:4.1f}% of the HBM roofline at 96 B per cell: "
          f"pairs read twice less the numerators once, cell written) | from host: pairs {t_cols*1e3:8.3f} ms, resolved cells {t_up*1e3:8.3f} ms | CPU batch_inv + mul, one thread {t_cpu*1e3:8.1f} ms", flush=True)
    # 4. h2mi_prover_advice, rational against plain cells (Montgomery words either way)
    params = h2.ParamsKZG.setup(log, 0x5EC2E7)
    cs, asg = circuit()
    keys = custom.Keys(params, cs, asg); ws = custom.Workspace(params, keys)
    pts = ws.prover._points.ctypes.data
    def advice(flags, values):
        cc = (engine.ColumnCells * 3)()
        for j in range(3): cc[j].values, cc[j].count, cc[j].flags = values[j].ctypes.data, cells, flags
        return lambda: engine.check(lib.h2mi_prover_advice(ws.prover.handle, cc, None, 0, 5, pts), "advice")
    run_r, run_p = advice(engine.CELLS_RATIONAL, pairs), advice(0, plain)
    run_r(); pr = ws.prover._points.copy(); run_p(); assert np.array_equal(pr, ws.prover._points), "rational and plain cells commit to different points"
    R = 5 if log <= 20 else 3
    tr, tp = [], []
    for _ in range(3):  # alternating, the best of three
        tr.append(t(run_r, R)); tp.append(t(run_p, R))
    print(f"log={log}: h2mi_prover_advice rational {min(tr)*1e3:8.3f} ms, plain {min(tp)*1e3:8.3f} ms (all runs: {[round(x*1e3, 2) for x in tr]} / {[round(x*1e3, 2) for x in tp]}); "
          f"chain kernels inside the call {kernel_ms(run_r)}", flush=True)
    ws.release(); keys.release(); params.release()
