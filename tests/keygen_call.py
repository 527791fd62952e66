"""One raw h2mi_prover_keygen call from keyword arguments, for the tests that assert its return codes: the record is filled field by field
as a C caller fills it (what is not named stays NULL / 0) and the handle comes back beside the code."""
import ctypes as C


def keygen(cs, gates=None, lookups=None, inputs=None, phases=None, shuffles=None, g_lagrange=0, fixed=None, copies=None, n_copies=0, flags=0,
           pk=0xDEAD):
    """-> (return code, *pk_out).  cs and the five programs: ctypes structs or None; fixed: a ColumnCells array (engine.pack_cells) or None;
    copies: an address or None.  pk: what *pk_out holds before the call, so that `handle is None` shows the library wrote NULL."""
    from halo2_scaffold_amd import engine
    from halo2_scaffold_amd._lib import lib

    opt = lambda s: C.pointer(s) if s is not None else None
    args = engine.KeygenArgs(opt(cs), opt(gates), opt(lookups), opt(inputs), opt(phases), opt(shuffles), g_lagrange, C.cast(fixed, C.c_void_p), copies,
                             n_copies, flags)
    out = C.c_void_p(pk)
    rc = lib.h2mi_prover_keygen(C.byref(args), C.byref(out))
    return rc, out.value
