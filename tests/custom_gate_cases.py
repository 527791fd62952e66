"""Circuits with gates given as data, shared by tests/test_custom_gates_host.py and tests/test_gpu_custom_gates.py: the reference's
StandardPlonk, is_zero and or circuits through custom.ConstraintSystem (configure() / synthesize() call for call), a degree-6 circuit
with a negative rotation and an instance query inside a gate, the vertical gate as raw ops, and the small tools both files use
(a postfix stack machine, random expression trees, the oracle's view of a custom constraint system)."""
import random

from oracle import bn254 as o
from oracle import flex as FX

R = o.R
OP_ADVICE, OP_FIXED, OP_INSTANCE, OP_CONSTANT, OP_ADD, OP_SUB, OP_MUL, OP_NEG, OP_END = range(9)  # include/h2mi.h H2MI_EXPR_*


def run_postfix(ops, constants, q):
    """the stack machine of include/h2mi.h on Python integers: -> (one value per polynomial, deepest stack)"""
    stack, out, deepest = [], [], 0
    for op, index, rotation in ops:
        if op <= OP_INSTANCE:
            stack.append(q(op, index, rotation) % R)
        elif op == OP_CONSTANT:
            stack.append(constants[index] % R)
        elif op == OP_NEG:
            stack.append(-stack.pop() % R)
        elif op == OP_END:
            assert len(stack) == 1
            out.append(stack.pop())
        else:
            b, a = stack.pop(), stack.pop()
            stack.append((a + b if op == OP_ADD else a - b if op == OP_SUB else a * b) % R)
        deepest = max(deepest, len(stack))
    assert not stack
    return out, deepest


# ---- the reference's circuits ----------------------------------------------------------------------------------------------------
def standard_plonk_cs(custom):
    """src/circuits/standard_plonk.rs:27-48"""
    meta = custom.ConstraintSystem()
    a, b, c = (meta.advice_column() for _ in range(3))
    q_a, q_b, q_c, q_ab, constant = (meta.fixed_column() for _ in range(5))
    for column in (a, b, c):
        meta.enable_equality(column)

    def gate(meta):
        a_, b_, c_ = (meta.query_advice(col, custom.Rotation.cur()) for col in (a, b, c))
        qa, qb, qc, qab, k = (meta.query_fixed(col, custom.Rotation.cur()) for col in (q_a, q_b, q_c, q_ab, constant))
        return [qa * a_ + qb * b_ + qc * c_ + qab * a_ * b_ + k]

    meta.create_gate("standard plonk", gate)
    return meta


def is_zero_circuit(custom, x, flip_out=False):
    """src/circuits/is_zero.rs: configure (:29-53) and synthesize (:87-145) -> (cs, assignment)"""
    meta = custom.ConstraintSystem()
    cx, cy, cout = (meta.advice_column() for _ in range(3))
    selector = meta.selector()
    for column in (cx, cout):
        meta.enable_equality(column)

    def gate(meta):
        x_, y_, out_ = (meta.query_advice(col, custom.Rotation.cur()) for col in (cx, cy, cout))
        s = meta.query_selector(selector)
        xy = x_ * y_
        return [s * (xy + out_ - custom.Expression.constant(1)), s * x_ * out_]

    meta.create_gate("ISZERO gate", gate)
    region = custom.Assignment(meta)
    x %= R
    region.assign_advice(cx, 0, x)
    region.assign_advice(cy, 0, 1 if x == 0 else pow(x, -1, R))
    out_val = 1 if x == 0 else 0
    out = region.assign_advice(cout, 0, out_val ^ 1 if flip_out else out_val)
    region.enable_selector(selector, 0)
    region.copy_advice(out, cx, 1)
    return meta, region


def or_circuit(custom, a, b, flip_out=False):
    """src/circuits/or.rs: configure (:26-51) and synthesize (:87-162)"""
    meta = custom.ConstraintSystem()
    witness = meta.advice_column()
    selector = meta.selector()
    meta.enable_equality(witness)

    def gate(meta):
        a_ = meta.query_advice(witness, custom.Rotation.cur())
        b_ = meta.query_advice(witness, custom.Rotation(1))
        out = meta.query_advice(witness, custom.Rotation(2))
        sel = meta.query_selector(selector)
        return [sel * (a_ + b_ - a_ * b_ - out)]

    meta.create_gate("OR gate", gate)
    region = custom.Assignment(meta)
    region.assign_advice(witness, 0, a)
    region.assign_advice(witness, 1, b)
    out_val = 1 if (a or b) else 0
    region.assign_advice(witness, 2, out_val ^ 1 if flip_out else out_val)
    region.enable_selector(selector, 0)
    return meta, region


def degree6_circuit(custom, a0, c0, steps=3):
    """beyond degree 3: gates s (a(w^-1 X)^5 + c - a) and s2 (a - instance): a chain a_(i+1) = a_i^5 + c_(i+1) down one advice column
    with the round constants in a fixed column (the gate on row i + 1 reads the row above: a negative rotation); the first value is
    public through a copy constraint, the last through a gate that queries the instance column on its own row.
    Degree 6: extended domain 8n, five h pieces, one permutation chunk of up to four columns."""
    meta = custom.ConstraintSystem()
    a = meta.advice_column()
    c = meta.fixed_column()
    inst = meta.instance_column()
    s, s2 = meta.selector(), meta.selector()
    for column in (a, c, inst):
        meta.enable_equality(column)

    def chain(meta):
        prev, cur = meta.query_advice(a, custom.Rotation.prev()), meta.query_advice(a, custom.Rotation.cur())
        return [meta.query_selector(s) * (prev * prev * prev * prev * prev + meta.query_fixed(c, custom.Rotation.cur()) - cur)]

    def public(meta):
        return [meta.query_selector(s2) * (meta.query_advice(a, custom.Rotation.cur()) - meta.query_instance(inst, custom.Rotation.cur()))]

    meta.create_gate("fifth power chain", chain)
    meta.create_gate("public output", public)
    vals = [a0 % R]
    for i in range(steps):
        vals.append((pow(vals[-1], 5, R) + c0 + i) % R)
    region = custom.Assignment(meta, instance=[vals[0]] + [0] * (steps - 1) + [vals[-1]])  # the output on the row of its cell
    first = region.assign_advice(a, 0, vals[0])
    region.constrain_instance(first, inst, 0)
    for i in range(steps):
        region.assign_advice(a, i + 1, vals[i + 1])
        region.assign_fixed(c, i + 1, c0 + i)
        region.enable_selector(s, i + 1)
    region.enable_selector(s2, steps)
    return meta, region


# ---- the oracle's view ----------------------------------------------------------------------------------------------------------
def oracle_cs(cs, name="custom"):
    """a custom.ConstraintSystem as oracle.flex.ConstraintSystem: the same numbers, the gates as callables"""
    return FX.ConstraintSystem(name, cs.n_advice, cs.n_fixed, cs.n_instance, cs.gates, list(cs.perm_columns), [], list(cs.advice_queries),
                               list(cs.fixed_queries), list(cs.instance_queries), cs.degree(), cs.blinding_factors())


def oracle_assignment(ocs, asg):
    oasg = FX.Assignment(ocs)
    oasg.advice = [dict(c) for c in asg.advice]
    oasg.fixed = [dict(c) for c in asg.fixed]
    oasg.instance = [list(asg.instance)] if ocs.n_instance else []
    oasg.copies = list(asg.copies)
    return oasg


# ---- raw programs -----------------------------------------------------------------------------------------------------------------
def vertical_gate_ops(gate_columns):
    """halo2-base's vertical gate q (a + a(wX) a(w^2 X) - a(w^3 X)) per (advice column, selector column), k_evaluate_h_flex's gates"""
    ops = []
    for a, q in gate_columns:
        ops += [(OP_ADVICE, a, 1), (OP_ADVICE, a, 2), (OP_MUL, 0, 0), (OP_ADVICE, a, 0), (OP_ADD, 0, 0), (OP_ADVICE, a, 3), (OP_SUB, 0, 0),
                (OP_FIXED, q, 0), (OP_MUL, 0, 0), (OP_END, 0, 0)]
    return ops


def random_tree(custom, rng: random.Random, depth: int, columns, leaf_bias=0.3):
    """a random Expression over `columns` = [(kind, index, [rotations])], using every operator"""
    if depth == 0 or rng.random() < leaf_bias:
        if rng.random() < 0.25:
            return custom.Expression.constant(rng.choice([0, 1, R - 1, rng.randrange(R)]))
        kind, index, rots = rng.choice(columns)
        return custom.Expression("query", kind, index, rng.choice(rots))
    op = rng.choice(["add", "sub", "mul", "neg"])
    if op == "neg":
        return -random_tree(custom, rng, depth - 1, columns, leaf_bias)
    a, b = random_tree(custom, rng, depth - 1, columns, leaf_bias), random_tree(custom, rng, depth - 1, columns, leaf_bias)
    return a + b if op == "add" else a - b if op == "sub" else a * b


def tree_stack_depth(e):
    """the stack a tree needs when the deeper operand of ADD / MUL is evaluated first — written here independently of custom.py"""
    t = e.node[0]
    if t in ("constant", "query"):
        return 1
    if t == "neg":
        return tree_stack_depth(e.node[1])
    a, b = tree_stack_depth(e.node[1]), tree_stack_depth(e.node[2])
    if t == "sub":
        return max(a, 1 + b)
    return max(max(a, b), 1 + min(a, b))
