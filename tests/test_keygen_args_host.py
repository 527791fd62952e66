"""h2mi_keygen_args (include/h2mi_prover.h), the one record h2mi_prover_keygen takes, on the host alone: its ctypes mirror
(engine.KeygenArgs) against the layout the system C compiler gives the struct, and the refusals the entry decides before any device work
for the records that combine what used to travel apart — the table logUp (H2MI_KEYGEN_LOGUP on a hard-wired shape) beside programs, phases
or H2MI_KEYGEN_BY_COSET, an unknown shape with the flag, input sets without a lookup program, no record at all."""
import ctypes as C
import os
import subprocess

import custom_gate_cases as gate_cases
import keygen_call
import logup_cases
import shuffle_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = -1, -2
FIELDS = ["cs", "gates", "lookups", "inputs", "phases", "shuffles", "g_lagrange_handle", "fixed", "copies", "n_copies", "flags"]


def test_record_layout_is_the_c_compilers(tmp_path, h2):
    from halo2_scaffold_amd import engine

    lines = ['  printf("sizeof %zu\\n", sizeof(h2mi_keygen_args));']
    lines += [f'  printf("{f} %zu\\n", offsetof(h2mi_keygen_args, {f}));' for f in FIELDS]
    src = tmp_path / "record.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "h2mi_prover.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "record"
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert [name for name, _ in engine.KeygenArgs._fields_] == FIELDS  # every field of the mirror is compared, in the header's order
    want = {"sizeof": str(C.sizeof(engine.KeygenArgs))}
    want.update({f: str(getattr(engine.KeygenArgs, f).offset) for f in FIELDS})
    assert got == want


def _flex_abi(engine, degree=9):
    """a FLEX_VERTICAL constraint system with four single-expression lookups over one table: valid for the groupings None and [2, 2]"""
    from halo2_scaffold_amd import flex

    abi = flex.FlexGateCS(True, 3, 4, k=7).abi(7)
    abi.degree = degree
    return abi


def test_refusals_of_the_combined_records(h2):
    """each row: the code, and *pk_out written NULL.  A record that passes every host rule finds no device: H2MI_ENODEV."""
    import torch

    from halo2_scaffold_amd import custom, engine
    from halo2_scaffold_amd._lib import lib

    accepted = None if torch.cuda.is_available() else ENODEV  # with a device an accepted record goes on to the SRS handle: tests/test_gpu_keygen_args.py
    LOGUP, BY_COSET, VK_ONLY = engine.KEYGEN_LOGUP, engine.KEYGEN_BY_COSET, engine.KEYGEN_VK_ONLY
    abi = _flex_abi(engine)
    cells, keep = engine.pack_cells([{} for _ in range(abi.n_fixed)])
    sets = engine.LogupInputs.build([2, 2])
    assert engine.table_logup_check(abi, sets) == 5

    def table(**more):
        more.setdefault("flags", LOGUP)
        return keygen_call.keygen(abi, fixed=cells, **more)

    # the table logUp takes the grouping and nothing else: any program, phases or shuffles beside it is refused before the grouping is read
    is_zero, _ = gate_cases.is_zero_circuit(custom, 5)
    xor, _, _ = logup_cases.build(custom, "xor")
    programs = {"gates": is_zero.gate_program(), "lookups": xor.lookup_program(), "phases": engine.AdvicePhases.build([0] * abi.n_advice, []),
                "shuffles": shuffle_cases.perm_circuit(custom)[0].shuffle_program()}
    for field, value in programs.items():
        assert table(**{field: value}) == (EINVAL, None), field
        assert table(inputs=sets, **{field: value}) == (EINVAL, None), field
    for flags in (LOGUP | BY_COSET, LOGUP | BY_COSET | VK_ONLY):
        assert table(flags=flags) == (EINVAL, None) and table(inputs=sets, flags=flags) == (EINVAL, None)
    # ... and alone it passes every host rule, with or without a grouping, with VK_ONLY beside the flag
    if accepted is not None:
        assert table() == (accepted, None) and table(inputs=sets) == (accepted, None) and table(inputs=sets, flags=LOGUP | VK_ONLY) == (accepted, None)
    # a shape no rule knows, with the flag: the table logUp's check refuses it (not EXPRESSIONS, so not the program rules)
    unknown = _flex_abi(engine)
    unknown.gates = 7
    assert keygen_call.keygen(unknown, fixed=cells, flags=LOGUP) == (EINVAL, None)
    assert keygen_call.keygen(unknown, inputs=sets, fixed=cells, flags=LOGUP) == (EINVAL, None)
    # outside the table logUp: input sets without a lookup program, with and without the flag, on both kinds of shape
    ones = engine.LogupInputs.build([1] * 4)
    exprs = is_zero.abi(5)
    ecells, ekeep = engine.pack_cells([{} for _ in range(exprs.n_fixed)])
    assert keygen_call.keygen(abi, inputs=ones, fixed=cells) == (EINVAL, None)
    assert keygen_call.keygen(exprs, gates=programs["gates"], inputs=ones, fixed=ecells) == (EINVAL, None)
    assert keygen_call.keygen(exprs, gates=programs["gates"], inputs=ones, fixed=ecells, flags=LOGUP) == (EINVAL, None)
    if accepted is not None:
        assert keygen_call.keygen(exprs, gates=programs["gates"], fixed=ecells) == (accepted, None)
    # no record, no constraint system, nowhere to put the key: H2MI_EINVAL, and what *pk_out held is not touched
    pk = C.c_void_p(0xDEAD)
    assert lib.h2mi_prover_keygen(None, C.byref(pk)) == EINVAL and pk.value == 0xDEAD
    assert keygen_call.keygen(None, fixed=cells) == (EINVAL, 0xDEAD)
    args = engine.KeygenArgs(C.pointer(abi), fixed=C.cast(cells, C.c_void_p))
    assert lib.h2mi_prover_keygen(C.byref(args), None) == EINVAL
    del keep, ekeep
