"""The witness check (h2mi_plonk_expr_check_dev, h2mi_prover_check), shared by tests/test_check_host.py and tests/test_gpu_check.py:
every case with the report it must give, computed here with Python integers.

Level A: programs `tree - c` whose fixed column c holds the tree's value on every row but a planted set, so that the count and the
first row of every polynomial are known exactly; programs whose value is an UNREDUCED multiple of r on every row.
Level B: `host_report` / `flex_host_report` restate what the device reports — per gate polynomial the failing usable rows, the copy
constraints between unequal cells, per lookup the usable rows whose input tuple is on no usable table row — for the circuits of the
existing case files and the ones built here: a copy-constraint circuit with cycles of three and four cells over advice, fixed and
instance columns, an ungated boolean gate, single-limb range checks whose looked-up cell can be pushed out of the table without
breaking a gate."""
import random

import custom_gate_cases as gate_cases
import phase_cases
from custom_gate_cases import OP_ADD, OP_ADVICE, OP_CONSTANT, OP_END, OP_FIXED, OP_MUL, OP_NEG, OP_SUB
from oracle import bn254 as o

R = o.R
NONE = 0xFFFFFFFF
GATE, COPY, LOOKUP = 0, 1, 2  # h2mi_check_failure.kind
KINDS = {0: "advice", 1: "fixed", 2: "instance"}
N_ADV, N_FIX, N_CH = 3, 2, 2  # random columns of the level-A cases; fixed columns 2 .. hold the planted values


# ---- level A -------------------------------------------------------------------------------------------------------------------------
def planted_sets(n: int, n_rows: int):
    """the planted row sets the issue names, cut to the 2^k rows: none; {0}; {n - 1}; {63, 64}; {255, 256}; all rows; and one with a
    row at or beyond n_rows, which is not counted"""
    sets = [set(), {0}, {n - 1}, {63, 64}, {255, 256}, set(range(n)), {5, min(n_rows, n - 1), n - 1}]
    return [{r for r in s if r < n} for s in sets]


def _chain(custom, queries):
    """q0 - (q1 - (q2 - ...)): SUB keeps its order, so the stack is as deep as the chain is long"""
    e = queries[-1]
    for q in reversed(queries[:-1]):
        e = q - e
    return e


def planted_case(custom, k: int, seed: int, sets=None, n_rows: int = None):
    """-> dict(k, n_rows, data {(kind, column): [values]}, ops, consts, challenges, want [(count, first)], depths).  Polynomial j is
    tree_j - fixed[N_FIX + j]; trees use every operator, rotations -3 .. 3 that wrap, constants and challenge operands; tree 0 is a
    bare query (stack depth 1 before the subtraction) and tree 1 a chain eight deep."""
    rng = random.Random(9000 + 97 * k + seed)
    n = 1 << k
    n_rows = n if n_rows is None else n_rows
    sets = planted_sets(n, n_rows) if sets is None else sets
    rots = list(range(-3, 4))
    columns = [("advice", j, rots) for j in range(N_ADV)] + [("fixed", j, rots) for j in range(N_FIX)] + [("instance", 0, rots)]
    query = lambda: (lambda c: custom.Expression("query", c[0], c[1], rng.choice(c[2])))(rng.choice(columns))
    trees = []
    for j in range(len(sets)):
        if j == 0:
            t = custom.Expression("query", "advice", 0, -3)
        elif j == 1:
            picks = [rng.choice(columns) for _ in range(8)]  # every rotation -3 .. 3, each wrapping on some row
            t = _chain(custom, [custom.Expression("query", c[0], c[1], rot) for c, rot in zip(picks, rots + [0])])
        elif j == 2:  # every operator, a constant, a challenge
            t = -(query() * query()) + custom.Expression.constant(rng.randrange(R)) * query() + custom.Expression("challenge", 1) * query()
        else:
            while True:
                t = gate_cases.random_tree(custom, rng, rng.randrange(1, 5), columns, leaf_bias=0.25)
                if t.stack_depth() <= 8:
                    break
            if j % 2 == 0:
                t = t + custom.Expression("challenge", j % N_CH) * query()
        trees.append(t)
    challenges = [rng.randrange(R), R - 1]
    column = lambda: [rng.choice([0, 1, R - 1]) if rng.random() < 0.3 else rng.randrange(R) for _ in range(n)]
    data = {("advice", j): column() for j in range(N_ADV)}
    data.update({("fixed", j): column() for j in range(N_FIX)})
    data[("instance", 0)] = column()
    value = lambda kind, c, row: data[(kind, c)][row % n]
    constants, ops, want = {}, [], []
    for j, (t, planted) in enumerate(zip(trees, sets)):
        vals = [t.evaluate(lambda kind, c, rot, row=row: value(kind, c, row + rot), challenges) for row in range(n)]
        data[("fixed", N_FIX + j)] = [(v + 1) % R if row in planted else v for row, v in enumerate(vals)]
        ops += (t - custom.Expression("query", "fixed", N_FIX + j, 0)).program(constants)[0]
        counted = sorted(r for r in planted if r < n_rows)
        want.append((len(counted), counted[0] if counted else NONE))
    consts = sorted(constants, key=constants.get)
    return dict(k=k, n_rows=n_rows, data=data, ops=ops, consts=consts, challenges=challenges, want=want,
                depths=[max(t.stack_depth(), 2) for t in trees])


def many_polynomials_case(custom, k: int = 9, n_polys: int = 44):
    """one program of n_polys polynomials with different planted sets: polynomial 0 and the last one planted, some not at all, some on
    a row of the upper half only (k = 9: the second workgroup), sizes 1 .. 9"""
    n = 1 << k
    rng = random.Random(4444)
    sets = []
    for j in range(n_polys):
        if j % 5 == 2:
            sets.append(set())
        elif j % 5 == 3:
            sets.append({rng.randrange(n // 2, n)})
        else:
            sets.append(set(rng.sample(range(n), 1 + j % 9)))
    assert sets[0] and sets[-1]
    return planted_case(custom, k, 1, sets=sets)


def report_by_evaluation(case):
    """the same report from the program alone: run the postfix on every row (run_postfix of tests/phase_cases.py)"""
    n = 1 << case["k"]
    bad = None
    for row in range(n):
        polys = phase_cases.run_postfix(case["ops"], case["consts"], lambda op, c, r: case["data"][(KINDS[op], c)][(row + r) % n], case["challenges"])
        bad = bad or [[] for _ in polys]
        for j, v in enumerate(polys):
            if v and row < case["n_rows"]:
                bad[j].append(row)
    return [(len(rows), rows[0] if rows else NONE) for rows in bad]


def redundant_zero_case(k: int = 6):
    """programs that are zero on every row but whose value the kernel holds as an unreduced multiple of r, or as r itself:
    a - a; a b - b a; NEG a + a; eight copies of a column of r - 1 plus the constant 8 (8 r); a column of zeros; the column of r - 1
    plus one; and 256 constants that sum to zero, added one by one.  advice 0, 1 random, 2 = r - 1 everywhere, 3 = zero everywhere."""
    rng = random.Random(606)
    n = 1 << k
    data = {("advice", 0): [rng.randrange(R) for _ in range(n)], ("advice", 1): [rng.choice([0, 1, R - 1, rng.randrange(R)]) for _ in range(n)],
            ("advice", 2): [R - 1] * n, ("advice", 3): [0] * n}
    A = lambda c, r=0: (OP_ADVICE, c, r)
    ADD, SUB, MUL, NEG, END = (OP_ADD, 0, 0), (OP_SUB, 0, 0), (OP_MUL, 0, 0), (OP_NEG, 0, 0), (OP_END, 0, 0)
    consts = [rng.randrange(R) for _ in range(256)]
    consts[8], consts[9] = 8, 1
    consts[255] = -sum(consts[:255]) % R  # the 256 constants sum to zero
    ops = [A(0), A(0), SUB, END,
           A(0), A(1, 2), MUL, A(1, 2), A(0), MUL, SUB, END,
           A(0, -1), NEG, A(0, -1), ADD, END]
    ops += [A(2)] + sum(([A(2, i - 3), ADD] for i in range(7)), []) + [(OP_CONSTANT, 8, 0), ADD, END]
    ops += [A(3), END, A(2), (OP_CONSTANT, 9, 0), ADD, END, A(3, 1), A(2), MUL, END]
    ops += [(OP_CONSTANT, 0, 0)] + sum(([(OP_CONSTANT, i, 0), ADD] for i in range(1, 256)), []) + [END]
    return dict(k=k, n_rows=n, data=data, ops=ops, consts=consts, challenges=[], want=[(0, NONE)] * 8)


# ---- level B: what the device must report ------------------------------------------------------------------------------------------------
def host_report(asg, k: int, challenges=()):
    """custom.mock's three loops, kept going: -> [(GATE, polynomial, first failing usable row, failing usable rows)] +
    [(COPY, cells of the unequal copy constraints)] (at most one) + [(LOOKUP, lookup, first row, rows)]"""
    cs = asg.cs
    n = 1 << k
    u = n - (cs.blinding_factors() + 1)
    value = {"advice": lambda c, r: asg.advice[c].get(r, 0), "fixed": lambda c, r: asg.fixed[c].get(r, 0),
             "instance": lambda c, r: asg.instance[r] if r < len(asg.instance) else 0}
    at = lambda e, row: e.evaluate(lambda kind, c, rot: value[kind](c, (row + rot) % n), challenges)
    out = []
    for j, poly in enumerate(cs.polynomials):
        rows = [row for row in range(u) if at(poly, row)]
        if rows:
            out.append((GATE, j, rows[0], len(rows)))
    cells = set()
    for left, right in asg.copies:
        if value[left[0]](left[1], left[2]) % R != value[right[0]](right[1], right[2]) % R:
            cells |= {left, right}
    if cells:
        out.append((COPY, cells))
    for l, pairs in enumerate(cs.lookups):
        table = {tuple(at(t, row) for _, t in pairs) for row in range(u)}
        rows = [row for row in range(u) if tuple(at(a, row) for a, _ in pairs) not in table]
        if rows:
            out.append((LOOKUP, l, rows[0], len(rows)))
    return out


def flex_host_report(asg, k: int):
    """the same for the halo2-lib shapes (flex.mock's loops): the vertical gate per gate column on the rows its selector enables, the
    copy constraints, per lookup (q_lookup a, or a lookup-advice column) the usable rows whose value is not in the table"""
    cs = asg.cs
    n = 1 << k
    u = n - (cs.blinding_factors + 1)
    out = []
    for j, cq in enumerate(cs.col_qs):
        a = asg.advice[j]
        rows = [r for r in sorted(asg.fixed[cq]) if (a.get(r, 0) + a.get(r + 1, 0) * a.get(r + 2, 0) - a.get(r + 3, 0)) % R]
        if rows:
            out.append((GATE, j, rows[0], len(rows)))
    value = {"advice": lambda c, r: asg.advice[c].get(r, 0), "fixed": lambda c, r: asg.fixed[c].get(r, 0),
             "instance": lambda c, r: asg.instance[r] if r < len(asg.instance) else 0}
    cells = set()
    for left, right in asg.copies:
        if value[left[0]](left[1], left[2]) % R != value[right[0]](right[1], right[2]) % R:
            cells |= {left, right}
    if cells:
        out.append((COPY, cells))
    if cs.lookup:
        table = set(v % R for v in asg.table_values) | {0}
        if cs.num_advice == 1:
            inputs = [{r: asg.advice[0].get(r, 0) for r in asg.fixed[cs.col_qlookup]}]
        else:
            inputs = [asg.advice[cs.num_advice + l] for l in range(cs.num_lookup_advice)]
        for l, cells_ in enumerate(inputs):
            rows = sorted(r for r, v in cells_.items() if r < u and v % R not in table)
            if rows:
                out.append((LOOKUP, l, rows[0], len(rows)))
    return out


def first_violation(report, cs, flex_shape=False):
    """the first entry of a report in the words custom.mock / flex.mock raise (a copy constraint: the words they start with)"""
    kind = report[0][0]
    if kind == COPY:
        return "copy constraint"
    _, index, row, _ = report[0]
    if flex_shape:
        return f"gate not satisfied at row {row}" + (f" of column {index}" if len(cs.col_qs) > 1 else "") if kind == GATE else f"lookup not satisfied at row {row}"
    return f"gate {cs.gate_names[index]!r} not satisfied at row {row}" if kind == GATE else f"lookup {cs.lookup_names[index]!r} not satisfied at row {row}"


# ---- circuits given as data: (k, build(custom) -> (cs, good), break(custom) -> assignment of the same circuit that fails) ---------------
def _wrong_cell(build, column: int, row: int):
    def broken(custom):
        _, asg = build(custom)
        asg.advice[column][row] = (asg.advice[column][row] + 1) % R
        return asg

    return broken


def _data_circuits():
    import lookup_expr_cases as lk

    is_zero = lambda custom: gate_cases.is_zero_circuit(custom, 3)
    or_ = lambda custom: gate_cases.or_circuit(custom, 1, 0)
    degree6 = lambda custom: gate_cases.degree6_circuit(custom, 3, 7)
    return {
        "is_zero": (5, is_zero, lambda custom: gate_cases.is_zero_circuit(custom, 3, flip_out=True)[1]),
        "or": (5, or_, lambda custom: gate_cases.or_circuit(custom, 1, 0, flip_out=True)[1]),
        "degree6": (5, degree6, _wrong_cell(degree6, 0, 2)),
        "xor": (5, lk.xor_circuit, lambda custom: lk.xor_circuit(custom, bad="absent")[1]),
        "any": (5, lk.any_circuit, _wrong_cell(lk.any_circuit, 1, 2)),  # b on row 2: row 3 looks it up through b(w^-1 X)
    }


DATA_CIRCUITS = _data_circuits()


def boolean_circuit(custom, bits=(1, 0, 1, 1, 0, 0, 1)):
    """a (a - 1) with NO selector: satisfied on the usable rows by a boolean witness (unassigned rows are zero), not on the blinding
    rows, where the prover writes random scalars — MockProver does not look there, the verifier does"""
    meta = custom.ConstraintSystem()
    a = meta.advice_column()
    meta.enable_equality(a)
    cur = custom.Rotation.cur()
    meta.create_gate("boolean", lambda meta: [meta.query_advice(a, cur) * (meta.query_advice(a, cur) - custom.Expression.constant(1))])
    region = custom.Assignment(meta)
    cells = [region.assign_advice(a, row, v) for row, v in enumerate(bits)]
    region.copy_advice(cells[0], a, len(bits) + 2)
    return meta, region


def copies_circuit(custom, k: int, cycles: int, change=None):
    """copy constraints alone (and one gated boolean gate, for a key needs a gate): `cycles` cycles of three advice cells; every
    fourth cycle also holds a fixed cell (four cells), the first eight an instance cell.  More than 3 * cycles moved cells.
    change: (cycle, member 0 .. 2) — that advice cell gets another value.  -> (cs, assignment, the cells of cycle `change[0]`)"""
    meta = custom.ConstraintSystem()
    a, b = meta.advice_column(), meta.advice_column()
    f = meta.fixed_column()
    inst = meta.instance_column()
    s = meta.selector()
    for column in (a, b, f, inst):
        meta.enable_equality(column)
    cur = custom.Rotation.cur()
    meta.create_gate("boolean", lambda meta: [meta.query_selector(s) * meta.query_advice(b, cur) * (meta.query_advice(b, cur) - custom.Expression.constant(1))])
    u = (1 << k) - (meta.blinding_factors() + 1)
    assert 2 * cycles <= u
    rng = random.Random(k * 1000 + cycles)
    values = [rng.randrange(R) for _ in range(cycles)]
    region = custom.Assignment(meta, instance=values[:8])
    region.assign_advice(b, u - 1, 1)
    region.enable_selector(s, u - 1)
    members = None
    for c, v in enumerate(values):
        # two cells in column a, one in column b; the cycle is closed by constraining first == second, second == third
        cells = [region.assign_advice(a, 2 * c, v), region.assign_advice(a, 2 * c + 1, v), region.assign_advice(b, c, v)]
        region.constrain_equal(cells[0], cells[1])
        region.constrain_equal(cells[2], cells[1])
        where = [("advice", 0, 2 * c), ("advice", 0, 2 * c + 1), ("advice", 1, c)]
        if c % 4 == 1:
            region.constrain_equal(region.assign_fixed(f, c, v), cells[2])
            where.append(("fixed", 0, c))
        if c < 8:
            region.constrain_instance(cells[0], inst, c)
            where.append(("instance", 0, c))
        if change is not None and change[0] == c:
            members = where
    if change is not None:
        kind, column, row = members[change[1]]
        region.advice[column][row] = (region.advice[column][row] + 1) % R
    return meta, region, members


# ---- the older shapes ---------------------------------------------------------------------------------------------------------------------
def single_limb_range_closure(flex, cs, lookup_bits: int, count: int, marked: int = None, marked_value: int = None):
    """`count` witnesses, each range-checked in ONE limb (range_check(x, lookup_bits): the witness cell and its limb cell, tied by a
    copy constraint, in no gate) with a few gates in between; nothing public.  marked: that witness and every copy of it become
    marked_value after the fact — gates and copy constraints still hold, the lookup does not when the value is not in the table."""
    asg = flex.Assignment(cs)
    ctx = flex.Context(asg)
    rng = random.Random(1234 + count)
    values = [rng.randrange(1 << lookup_bits) for _ in range(count)]
    tag = None
    for i, v in enumerate(values):
        if i == marked:
            v = tag = next(t for t in range(2, 1 << lookup_bits) if t not in values and t not in [2 * w for w in values])  # a value no other cell holds
        cell = ctx.load_witness(v)
        ctx.range_check(cell, lookup_bits, lookup_bits)
        if i % 3 == 0:
            ctx.add(cell, cell)
    ctx.finish([])
    flex.load_lookup_table(asg, lookup_bits)
    if marked is not None:
        # x + x on a marked witness would tie it into a gate: keep the marked one off those
        assert marked % 3 != 0
        for column in asg.advice:
            for row, v in column.items():
                if v == tag:
                    column[row] = marked_value
    return asg


def flex_cases(flex):
    """name -> (k, cs, satisfied assignment, broken assignment): the halo2_lib closure (Gate builder) with a wrong output cell; the
    range closure in one column (q_lookup a) and over 3 + 1 columns with a wrong cell in gate column 1; single-limb range checks in
    one column, over several columns (a lookup-advice column) and at k = 11 (a table of 1024 values, the marked cell in the fourth
    workgroup of 256 rows) with one looked-up value of 2^LOOKUP_BITS"""
    out = {}
    cs = flex.FlexGateCS(lookup=False)
    bad = flex.halo2_lib_closure(cs, 12)
    bad.advice[0][sorted(bad.fixed[cs.col_q])[1] + 3] += 1
    out["halo2_lib"] = (6, cs, flex.halo2_lib_closure(cs, 12), bad)
    cs = flex.FlexGateCS(lookup=True)
    bad = flex.range_closure(cs, 0xDEADBEEFCAFE1234, 4)
    bad.advice[0][sorted(bad.fixed[cs.col_q])[2] + 3] += 1
    out["range"] = (7, cs, flex.range_closure(cs, 0xDEADBEEFCAFE1234, 4), bad)
    closure = lambda c: flex.range_closure(c, 0xDEADBEEFCAFE1234, 4)
    cs = flex.configure(True, 5, closure)
    assert cs.num_advice > 1 and cs.num_lookup_advice >= 1
    bad = closure(cs)
    bad.advice[1][sorted(bad.fixed[cs.col_qs[1]])[1] + 3] += 1
    out["range_multi"] = (5, cs, closure(cs), bad)
    for name, k, bits, count, marked in (("limbs", 7, 4, 9, 4), ("limbs_multi", 5, 4, 12, 7), ("limbs_k11", 11, 10, 300, 250)):
        closure = lambda c, bits=bits, count=count: single_limb_range_closure(flex, c, bits, count)
        cs = flex.configure(True, k, closure) if name == "limbs_multi" else flex.FlexGateCS(lookup=True)
        out[name] = (k, cs, closure(cs), single_limb_range_closure(flex, cs, bits, count, marked, 1 << bits))
    return out
