"""The argument records of the quotient calls (include/h2mi.h: h2mi_quotient_scalars, h2mi_quotient_circuits, h2mi_expr_columns) against
their ctypes mirrors in halo2_scaffold_amd/plonk.py: sizeof and every offsetof as the system C compiler lays the structs out.  A mirror
with a transposed or missing field hands a kernel a wrong pointer; here it fails without a GPU."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = {
    "h2mi_quotient_scalars": ["k", "extended_k", "blinding_factors", "beta", "gamma", "y", "delta", "zeta", "extended_omega", "t_inv"],
    "h2mi_quotient_circuits": ["circuits", "n_circuits", "shuffles", "logup", "instances", "gates", "challenges", "n_challenges"],
    "h2mi_expr_columns": ["advice", "n_advice", "fixed", "n_fixed", "instances", "program", "challenges", "n_challenges", "k"],
}


def test_record_layouts_are_the_c_compilers(tmp_path, h2):
    from halo2_scaffold_amd import plonk

    mirrors = {"h2mi_quotient_scalars": plonk.QuotientScalars, "h2mi_quotient_circuits": plonk.QuotientCircuits,
               "h2mi_expr_columns": plonk.ExprColumns}
    lines = []
    for struct, fields in FIELDS.items():
        lines.append(f'  printf("{struct} %zu\\n", sizeof({struct}));')
        lines += [f'  printf("{struct}.{f} %zu\\n", offsetof({struct}, {f}));' for f in fields]
    src = tmp_path / "records.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "h2mi.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "records"
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    want = {}
    for struct, fields in FIELDS.items():
        mirror = mirrors[struct]
        assert [name for name, _ in mirror._fields_] == fields  # every field of the mirror is compared, in the header's order
        want[struct] = str(ctypes.sizeof(mirror))
        for f in fields:
            want[f"{struct}.{f}"] = str(getattr(mirror, f).offset)
    assert got == want
