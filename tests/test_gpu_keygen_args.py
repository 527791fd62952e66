"""h2mi_prover_keygen on the device: the records the one entry accepts — every optional field NULL, each program beside the constraint
system, the logUp flag with input sets, and the table logUp of a hard-wired shape with a grouping — each made from a raw h2mi_keygen_args,
rc == 0, a handle that releases.  The refusals are tests/test_keygen_args_host.py's.  k = 5 but for the flex range shape: the Range builder's
smallest circuit here is the 11 + 4 column one of tests/test_gpu_table_logup.py at k = 7."""
import numpy as np
import pytest

import custom_gate_cases as gate_cases
import keygen_call
import logup_sets_cases
import phase_cases
import shuffle_cases

pytestmark = pytest.mark.gpu

SRS_SECRET = 0x5EC2E7 + 0x48324D49


def _custom_record(custom, engine, cs, asg, k):
    """what custom.Keys hands engine.Keys, as keyword arguments of keygen_call.keygen"""
    asg = shuffle_cases.first_assignment(cs, asg)
    index = {col: j for j, col in enumerate(cs.perm_columns)}
    copies = np.ascontiguousarray(np.array([(index[(le[0], le[1])], le[2], index[(ri[0], ri[1])], ri[2]) for le, ri in asg.copies], dtype=np.uint32).reshape(-1, 4))
    cells, keep = engine.pack_cells(list(asg.fixed))
    return dict(cs=cs.abi(k), gates=cs.gate_program(), lookups=cs.lookup_program(), phases=cs.phases(), shuffles=cs.shuffle_program(), fixed=cells,
                copies=copies.ctypes.data, n_copies=len(copies)), (keep, copies)


def _records(custom, engine, flex, keygen, circuits):
    """-> [(name, k, keyword arguments, what they point into)]"""
    out = []
    cells, keep = engine.pack_cells([{} for _ in range(5)])
    out.append(("StandardPlonk, every optional field NULL", 5, dict(cs=keygen.constraint_system(circuits.StandardPlonk, 5), fixed=cells), keep))
    cs, asg = gate_cases.is_zero_circuit(custom, 3)
    rec, keep = _custom_record(custom, engine, cs, asg, 5)
    assert rec["gates"] is not None and rec["lookups"] is None and rec["phases"] is None and rec["shuffles"] is None
    out.append(("is_zero: gates", 5, rec, keep))
    cs, asg = logup_sets_cases.range_circuit(custom)
    rec, keep = _custom_record(custom, engine, cs, asg, 5)
    rec.update(inputs=cs.logup_inputs(), flags=engine.KEYGEN_LOGUP)
    assert rec["lookups"] is not None and list(rec["inputs"].n_inputs)[:1] == [3]
    out.append(("range3: a lookup program, H2MI_KEYGEN_LOGUP, three input sets", 5, rec, keep))
    build, k = phase_cases.CIRCUITS["rlc"]
    assert k == 5
    rec, keep = _custom_record(custom, engine, *build(custom), k)
    assert rec["phases"] is not None and rec["phases"].n_phases == 2
    out.append(("rlc: two phases", k, rec, keep))
    cs, asg = shuffle_cases.perm_circuit(custom)
    rec, keep = _custom_record(custom, engine, cs, asg, shuffle_cases.CASES["perm"])
    assert rec["shuffles"] is not None and shuffle_cases.CASES["perm"] == 5
    out.append(("perm: a shuffle", 5, rec, keep))
    # the Range builder with 11 gate and 4 lookup-advice columns, the lookups grouped two and two: what flex.FlexKeys(..., logup=True, lookup_sets=2) passes
    cs = flex.FlexGateCS(True, 11, 4, k=7)
    asg = flex.range_closure(cs, 0xF1E2D3C4B5A6978, 4, 24)
    sets = engine.LogupInputs.build(cs.use_logup(2))
    assert cs.logup_runs == [2, 2]
    fixed = list(asg.fixed)
    fixed[cs.col_table] = list(asg.table_values)
    index = {col: j for j, col in enumerate(cs.perm_columns)}
    copies = np.ascontiguousarray(np.array([(index[(le[0], le[1])], le[2], index[(ri[0], ri[1])], ri[2]) for le, ri in asg.copies], dtype=np.uint32).reshape(-1, 4))
    cells, keep = engine.pack_cells(fixed)
    out.append(("flex range 11 + 4: the table logUp, grouping [2, 2]", 7,
                dict(cs=cs.abi(7), inputs=sets, fixed=cells, copies=copies.ctypes.data, n_copies=len(copies), flags=engine.KEYGEN_LOGUP), (keep, copies)))
    return out


def test_every_kind_of_record_makes_a_key(gpu):
    from halo2_scaffold_amd import circuits, custom, engine, flex, keygen

    params = {k: gpu.ParamsKZG.setup(k, SRS_SECRET) for k in (5, 7)}
    records = _records(custom, engine, flex, keygen, circuits)
    assert len(records) == 6
    for name, k, rec, keep in records:
        rc, handle = keygen_call.keygen(g_lagrange=params[k].g_lagrange_handle, **rec)
        assert rc == 0 and handle, name
        assert gpu.lib.h2mi_prover_pk_release(handle) == 0, name
        del keep
    for p in params.values():
        p.release()
