"""Randomly generated constraint systems with a satisfying witness by construction: the generator behind tests/test_random_circuits_host.py
(CPU), tests/test_gpu_random_circuits.py and fuzz_cases.Fuzzer.fuzz_custom.  The hand-written circuits of the other *_cases.py files
put one feature of the data-driven prover into a circuit each; `generate(custom, seed)` draws gates, lookups (plain, logUp, merged),
shuffles, advice phases, challenges, instance columns, batches and the multi-opening TOGETHER, so that the host-side bookkeeping all of
them share (query-list order, column numbering behind the selectors, blinding_factors, the extended domain, transcript and opening
order, merge_lookups' chunking, the four programs' constants and challenge operands) is varied by something that did not write it.

How a witness is satisfied by construction:
  columns   are created in a topological order.  FREE columns (advice of every phase, user fixed, instance) hold drawn values, a third
            of them from instance_cases.EXTREMES.  A DEFINED advice column a_j of phase p belongs to one polynomial
            s (a_j(w^t X) - f): f is a random tree (constant, negation, sum, difference, product, scaled, query, challenge) over
            columns created before it of phases <= p and challenges usable after a phase < p; cell a_j[r + t] := f(row r).
  blinding  a proof holds random scalars on rows u .. n-1 of every advice column, where `mock` reads zero.  Every polynomial and every
            gated lookup input therefore carries a selector (or a fixed column of non-zero factors) that is on only where r + rot lies
            in [0, u) for each of its advice queries; ungated expressions (shuffle inputs, degree-1 lookup inputs) read advice columns at
            rotation 0 only.  `blinded(case, asg, rng)` fills those rows the way a proof does: mock must still accept.
  lookups   the table side reads SINK columns no gate reads.  An advice sink is filled inside synthesize() after the inputs are known
            (phase >= everything the inputs read); a fixed sink holds the union of every circuit's inputs, which then read phase-0
            columns only.  The table has the distinct input tuples in shuffled order on drawn rows, repeats, unused tuples, and the zero
            tuple the switched-off rows need.  Pair 0 of every lookup adds a PRIVATE free advice column nothing else reads: the cell a
            planted fault changes.  An UNGATED lookup (degree-1 inputs, what six merged sets need) reads private columns only, which hold
            tuples of a small pool on every usable row.
  degrees   no tree multiplies by a column that is the zero polynomial (an instance column without values, an all-zero column): the
            declared degree would exceed the reached one and the top piece of h(X) vanish — see empty_term and zero_column_circuit.
  shuffles  the input tuple on all u rows; the sink advice columns hold a drawn permutation of those tuples.
  copies    into a scratch advice column of the last phase (copy_advice, chains, a cell with itself, a fixed cell), public inputs
            through constrain_instance at row 0, at a column's last value and beyond an empty column's values.
Everything is a function of the seed: random.Random(seed) and generators derived from it, no time, no global state.

`plant(case, rng)` changes exactly one cell of circuit 0 and says what `mock` and the device check must name."""
import random

from instance_cases import EXTREMES, R

MAX_STACK = 8        # H2MI_MAX_EXPR_STACK
MAX_DEGREE = 9       # the largest degree the prover takes
MAX_INSTANCE = 8     # H2MI_MAX_INSTANCE
MAX_SHUFFLES = 8     # H2MI_MAX_SHUFFLES
MAX_LOOKUPS = 8      # H2MI_MAX_LOOKUPS
MAX_LOGUP_INPUTS = 6  # H2MI_MAX_LOGUP_INPUTS
MAX_CHALLENGES = 16  # H2MI_MAX_CHALLENGES
MAX_CIRCUITS = 8     # H2MI_MAX_CIRCUITS
MIN_USABLE = 8       # k is raised until this many rows are usable
PINS = ("instances8", "shuffles8", "lookups8", "merged6", "degree9", "challenges16", "batch8", "blinding")
PAIR_FEATURES = ("phases>1", "lookup", "logup_merged", "shuffle", "instances>1", "batch>1", "gwc")
ADVICE, FIXED, INSTANCE = "advice", "fixed", "instance"


def required_features():
    """what a committed seed list must cover: every feature once, and every pair of PAIR_FEATURES together"""
    single = ["phases=1", "phases=2", "phases=3", "challenge_in_gate", "challenge_in_lookup", "lookup_any_advice_table", "fixed_table",
              "multi_pair_lookup", "plain_lookup", "logup", "merged", "shuffle", "multi_pair_shuffle", "instances=0", "instances=1", "instances=2-7",
              "instances=8", "instance_in_gate", "instance_in_lookup", "instance_in_shuffle", "batch=1", "batch=2", "batch=8", "gwc",
              "k=4", "k=5", "k=6", "degree<=4", "degree=5", "degree=6-8", "degree=9"] + ["pin:" + p for p in PINS]
    pairs = [(a, b) for i, a in enumerate(PAIR_FEATURES) for b in PAIR_FEATURES[i + 1:]]
    return single, pairs


def _field(rng):
    """a field element: about a third from the extremes"""
    return rng.choice(EXTREMES) if rng.random() < 1 / 3 else rng.randrange(R)


def _challenges_of(e, out=None):
    """the challenge indices an Expression reads"""
    out = set() if out is None else out
    if e.node[0] == "challenge":
        out.add(e.node[1])
    for sub in e.node[1:]:
        if hasattr(sub, "node"):
            _challenges_of(sub, out)
    return out


def _queries_of(e, out=None):
    """the (kind, column, rotation) queries an Expression (selectors unresolved) reads"""
    out = set() if out is None else out
    if e.node[0] == "query":
        out.add(tuple(e.node[1:]))
    for sub in e.node[1:]:
        if hasattr(sub, "node"):
            _queries_of(sub, out)
    return out


class Case:
    """one generated case: cs, k, synthesizers (one synthesize(challenges) -> Assignment per circuit of the batch), logup, merged,
    multiopen, features, describe(); the rest is what plant() and blinded() need"""

    def __init__(self, seed):
        self.seed = seed
        self.cs = self.k = None
        self.synthesizers = []
        self.logup = self.merged = False
        self.multiopen = "shplonk"
        self.features = set()
        self.pin = None
        self.defined = []   # per defined column {"column", "poly" (index), "name", "t", "rows", "needs"}
        self.copied = []    # the scratch rows a simple copy_advice fills: (copy index, scratch row)
        self.lookups = []   # per declared lookup {"private" (column index), "rows", "needs"}
        self.shuffles = []  # per shuffle {"sinks" (column indices), "needs"}

    @property
    def n(self):
        return 1 << self.k

    @property
    def u(self):
        return self.n - (self.cs.blinding_factors() + 1)

    def simple(self):
        """only gates, copies and instance columns: what oracle.flex proves"""
        cs = self.cs
        return not cs.lookups and not cs.shuffles and cs.n_phases == 1 and not cs.challenge_phase

    def describe(self):
        cs = self.cs
        return (f"seed {self.seed}: k={self.k} u={self.u} degree={cs.degree()} advice={cs.n_advice} phases={cs.advice_phase} "
                f"fixed={cs.n_user_fixed}+{cs.n_selectors} instance={cs.n_instance} challenges={cs.challenge_phase} polys={len(cs.polynomials)} "
                f"lookups={[len(p) for p in cs.lookups]} arguments={cs.lookup_arguments} logup={self.logup} merged={self.merged} "
                f"shuffles={[len(p) for p in cs.shuffles]} perm={len(cs.perm_columns)} batch={len(self.synthesizers)} {self.multiopen} pin={self.pin}")


class _Builder:
    def __init__(self, custom, seed):
        self.custom, self.rng = custom, random.Random(seed)
        self.case = Case(seed)
        self.meta = custom.ConstraintSystem()
        self.readable = []        # (Column, phase): what an expression may read; phase 0 for fixed and instance columns
        self.selector_rows = []   # (Selector, rows)
        self.fixed_cells = {}     # user fixed column index -> {row: value}: the same in every circuit
        self.steps = []           # the witness in creation order: callables (region, value, challenges, circuit)
        self.eq_later = []
        self.free_advice, self.instances = [], []
        self.fixed_tables = []    # filled after every circuit's phase-0 witness is known
        self.todo = []            # structure whose rows wait for k: callables run by finish()
        self.empty = []           # the instance columns that stay without values

    # ---- draws ---------------------------------------------------------------------------------------------------------------------
    def draw_shape(self):
        rng = self.rng
        c = self.case
        c.pin = rng.choice(PINS) if rng.random() < 1 / 8 else None
        pin = c.pin
        self.k = rng.choice([4, 5, 5, 6])
        self.n_phases = rng.choice([1, 1, 1, 2, 2, 3])
        self.n_challenges = 0 if self.n_phases == 1 and rng.random() < 0.7 else rng.randint(1, 4)
        self.n_instance = rng.choice([0, 0, 1, 1, 1, 2, 2, 3, 5, 7])
        self.batch = rng.choice([1, 1, 1, 1, 2, 2, 2, 3])
        self.n_lookups = rng.choice([0, 0, 1, 1, 2, 3])
        self.n_shuffles = rng.choice([0, 0, 0, 1, 1, 2])
        self.n_defined = rng.randint(1, 4)
        self.n_free = rng.randint(1, 3)
        self.n_user_fixed = rng.randint(0, 2)
        self.top_degree = rng.choice([2, 2, 3, 3, 3, 3, 4, 4, 4, 5, 5, 6, 7, 8])  # of one drawn polynomial, selector included
        c.multiopen = "gwc" if rng.random() < 0.35 else "shplonk"
        small = pin in ("instances8", "shuffles8", "lookups8", "merged6", "batch8", "challenges16")
        if small:  # the pinned dimension is what costs: the rest stays small
            self.n_defined, self.n_free, self.top_degree = min(self.n_defined, 2), min(self.n_free, 2), min(self.top_degree, 4)
            self.n_lookups, self.n_shuffles, self.batch = min(self.n_lookups, 1), min(self.n_shuffles, 1), min(self.batch, 2)
        if pin == "instances8":
            self.n_instance = MAX_INSTANCE
        elif pin == "shuffles8":
            self.n_shuffles = MAX_SHUFFLES
        elif pin == "lookups8":
            self.n_lookups = MAX_LOOKUPS
        elif pin == "merged6":
            self.n_lookups = MAX_LOGUP_INPUTS
        elif pin == "degree9":
            self.top_degree = MAX_DEGREE
        elif pin == "challenges16":
            self.n_challenges = MAX_CHALLENGES
        elif pin == "batch8":
            self.batch, self.k, self.n_instance = MAX_CIRCUITS, 4, min(self.n_instance, 2)
        if self.top_degree >= 8 or pin in ("lookups8", "shuffles8"):
            self.k = min(self.k, 5)  # the extended domain is 8 n: the Python verifier's time goes with it
        c.logup = self.n_lookups > 0 and (pin == "merged6" or rng.random() < 0.5)
        c.merged = c.logup and pin != "lookups8" and (pin == "merged6" or rng.random() < 0.7)

    def constant(self):
        rng = self.rng
        return rng.choice(EXTREMES) if rng.random() < 1 / 3 else rng.choice([2, 3, 5, 7, rng.randrange(R)])

    def rotation(self, kind, flat):
        if kind == ADVICE and flat:
            return 0
        return self.rng.choice([0, 0, 0, 0, 1, 1, -1, -1, 2, -2, 3])

    # ---- expressions ------------------------------------------------------------------------------------------------------------------
    def leaf(self, degree, env):
        """degree 0: a constant or a challenge; degree 1: a query"""
        rng, meta, E = self.rng, self.meta, self.custom.Expression
        if degree == 0:
            if env["challenges"] and rng.random() < 0.5:
                return meta.query_challenge(rng.choice(env["challenges"]))
            return E.constant(self.constant())
        column = rng.choice(env["columns"])
        rot = self.custom.Rotation(self.rotation(column.kind, env["flat"]))
        return {ADVICE: meta.query_advice, FIXED: meta.query_fixed, INSTANCE: meta.query_instance}[column.kind](column, rot)

    def tree(self, degree, size, env):
        """a random expression of exactly `degree` with about `size` leaves"""
        rng, E = self.rng, self.custom.Expression
        if size <= 1 or (degree == 0 and rng.random() < 0.4):
            e = self.leaf(min(degree, 1), env)
            for _ in range(degree - 1):  # a product chain reaches the degree whatever the size
                e = e * self.leaf(1, env)
            return e
        kind = rng.choice(["neg", "sum", "sum", "diff", "diff", "product", "product", "scaled"])
        if kind == "product" and degree >= 2:
            d = rng.randint(1, degree - 1)
            return self.tree(d, size // 2, env) * self.tree(degree - d, size - size // 2, env)
        if kind == "neg":
            return -self.tree(degree, size - 1, env)
        if kind == "scaled" or kind == "product":
            return E.constant(self.constant() or 1) * self.tree(degree, size - 1, env)  # not by zero: the degree is exact
        a, b = self.tree(degree, size // 2, env), self.tree(rng.randint(0, degree), size - size // 2, env)
        if rng.random() < 0.5:
            a, b = b, a
        return a + b if kind == "sum" else a - b

    def expression(self, degree, env, wrap=lambda e: e):
        """a tree of that degree whose wrapped form (the polynomial keygen sees) stays within the operand stack: a deeper draw is drawn
        again, smaller — the refusal of the program check is never what stops it"""
        size = self.rng.randint(max(1, degree), degree + 4)
        while True:
            e = self.tree(degree, size, env)
            if wrap(e).stack_depth() <= MAX_STACK:
                return e
            size = max(1, size - 1) if self.rng.random() < 0.7 else size

    def empty_term(self, f):
        """f, sometimes plus a query of an instance column without values.  Such a column is the zero polynomial, so no tree multiplies
        by it: a product with it would leave the constraint system's degree above what its polynomials reach, the top piece of h(X)
        would be zero, and its commitment — the identity — is a point no transcript writes (create_proof fails, as the crate's does)"""
        if self.empty and self.rng.random() < 0.3:
            return f + self.meta.query_instance(self.rng.choice(self.empty), self.custom.Rotation(self.rotation(INSTANCE, False)))
        return f

    def env(self, phase, flat=False, kinds=(ADVICE, FIXED, INSTANCE)):
        """what an expression whose value a column of `phase` holds may read"""
        cols = [c for c, p in self.readable if p <= phase and c.kind in kinds]
        chal = [ch for ch in self.challenges if ch.phase < phase]
        return {"columns": cols, "challenges": chal, "flat": flat}

    # ---- columns -------------------------------------------------------------------------------------------------------------------
    def equality(self, column, now=None):
        now = self.rng.random() < 0.5 if now is None else now
        if now:
            self.meta.enable_equality(column)
        else:
            self.eq_later.append(column)

    def free_columns(self):
        rng, meta = self.rng, self.meta
        order = [("a", 0)] * self.n_free + [("f", 0)] * self.n_user_fixed + [("i", 0)] * self.n_instance
        rng.shuffle(order)
        order = [("a", 0)] + order + [("a", p) for p in range(1, self.n_phases)]  # a later phase needs a column in the one before
        self.eq_columns = []
        for what, phase in order:
            if what == "a":
                col = meta.advice_column_in(phase)
                self.free_advice.append(col)
            elif what == "f":
                col = meta.fixed_column()
                self.fixed_cells[col.index] = None  # drawn once k is known
            else:
                col = meta.instance_column()
                self.instances.append(col)
                if rng.random() < 0.25:  # a column without values is the zero polynomial: see empty_term
                    self.empty.append(col)
            if col not in self.empty:
                self.readable.append((col, phase))
            if col in self.empty or rng.random() < (0.6 if what == "i" else 0.4):
                self.eq_columns.append(col)
                self.equality(col)
        phases = list(range(self.n_phases))
        self.challenges = [meta.challenge_usable_after(rng.choice(phases)) for _ in range(self.n_challenges)]

    def gating(self):
        """the factor that switches a polynomial off: a selector, or a user fixed column of non-zero factors created here — behind the
        user's fixed columns so far, in front of every selector"""
        meta = self.meta
        if self.rng.random() < 0.25:
            col = meta.fixed_column()
            self.fixed_cells[col.index] = {}
            return meta.query_fixed(col, self.custom.Rotation.cur()), ("fixed", col)
        s = meta.selector()
        return meta.query_selector(s), ("selector", s)

    def switch_on(self, gate, rows):
        rng = self.rng
        if gate[0] == "selector":
            self.selector_rows.append((gate[1], list(rows)))
        else:
            self.fixed_cells[gate[1].index].update({r: rng.choice([1, R - 1, rng.randrange(1, R)]) for r in rows})

    def safe_rows(self, queries, extra=()):
        """the rows r with r + rot in [0, u) for every advice query (and every extra rotation)"""
        u = self.case.u
        rots = [rot for kind, _, rot in queries if kind == ADVICE] + list(extra)
        return [r for r in range(u) if all(0 <= r + rot < u for rot in rots)]

    # ---- gates -----------------------------------------------------------------------------------------------------------------------
    def defined_columns(self, count, degree=None, wide=False):
        """`count` defined columns in ONE create_gate"""
        rng, meta, custom = self.rng, self.meta, self.custom
        polys = []
        name = f"gate {len(meta.gate_names)}"
        for _ in range(count):
            phase = rng.randrange(self.n_phases)
            if self.n_phases > 1 and rng.random() < 0.5:
                phase = max(phase, 1)
            env = self.env(phase)
            deg = degree if degree is not None else rng.randint(1, self.top_degree)
            gate_e, gate = self.gating()
            col = meta.advice_column_in(phase)
            t = rng.choice([0, 0, 0, 1, -1])
            mine = meta.query_advice(col, custom.Rotation(t))
            if wide:  # one free advice column at six rotations: blinding_factors 8
                a = self.free_advice[0]
                f = meta.query_advice(a, custom.Rotation(-2))
                for rot in (-1, 0, 1, 2, 3):
                    f = f + custom.Expression.constant(self.constant()) * meta.query_advice(a, custom.Rotation(rot))
            else:
                f = self.empty_term(self.expression(deg - 1, env, wrap=lambda e: gate_e * (mine - (e + e))))
            poly = gate_e * (mine - f) if rng.random() < 0.7 else (f - mine) * gate_e
            index = len(meta.gate_names) + len(polys)
            polys.append(poly)
            needs = _challenges_of(f)
            if needs:
                self.case.features.add("challenge_in_gate")
            if any(kind == INSTANCE for kind, _, _ in _queries_of(f)):
                self.case.features.add("instance_in_gate")
            info = {"column": col.index, "poly": index, "name": name, "t": t, "rows": None, "needs": needs}
            self.case.defined.append(info)
            self.readable.append((col, phase))
            if rng.random() < 0.25:
                self.eq_columns.append(col)
                self.equality(col)
            self.todo.append(lambda info=info, f=f, gate=gate, col=col, t=t: self.place_defined(info, f, gate, col, t))
        meta.create_gate(name, lambda meta: polys)

    def place_defined(self, info, f, gate, col, t):
        rng = self.rng
        rows = self.safe_rows(_queries_of(f), extra=[t])
        keep = [r for r in rows if rng.random() < 0.85] or rows[:1]
        info["rows"] = keep
        self.switch_on(gate, keep)
        u = self.case.u
        written = {r + t for r in keep}
        filler = [{r: _field(rng) for r in range(u) if r not in written and rng.random() < 0.4} for _ in range(self.batch)]
        resolved = lambda: f.resolve(self.meta.n_user_fixed)

        def step(region, value, challenges, circuit, planted):
            for r, v in filler[circuit].items():
                region.assign_advice(col, r, v)
            if any(challenges[c] is None for c in info["needs"]):
                return  # Value::unknown: the cells stay zero in this run
            e = resolved()
            for r in keep:
                v = e.evaluate(lambda kind, c, rot: value(kind, c, r + rot), challenges)
                if planted == ("gate", info["poly"], r):
                    v = (v + 1) % R
                region.assign_advice(col, r + t, v)

        self.steps.append(step)

    # ---- lookups ---------------------------------------------------------------------------------------------------------------------
    def table(self, pairs, fixed, squared):
        """sink columns and the table-side expressions over them"""
        rng, meta, custom = self.rng, self.meta, self.custom
        sinks, exprs, rots = [], [], []
        ts = meta.selector() if squared else None
        for _ in range(pairs):
            if fixed:
                col = meta.fixed_column()
                self.fixed_cells[col.index] = {}
                rot = rng.choice([0, 0, 1, -1])
                q = meta.query_fixed(col, custom.Rotation(rot))
            else:
                col = meta.advice_column_in(self.n_phases - 1)  # the last phase: at or behind everything an input reads
                rot = 0 if self.case.pin == "merged6" else rng.choice([0, 0, 0, 1, -1])
                q = meta.query_advice(col, custom.Rotation(rot))
            sinks.append(col)
            rots.append(rot)
            exprs.append(meta.query_selector(ts) * q if squared else q)
        return {"sinks": sinks, "exprs": exprs, "rots": rots, "selector": ts, "fixed": fixed, "users": [], "slots": None}

    def lookup_arguments(self):
        """the lookups, in groups over one table"""
        rng = self.rng
        left = self.n_lookups
        groups = []
        while left:
            share = left if self.case.pin == "merged6" else 1 if rng.random() < 0.5 else rng.randint(1, min(left, 3))
            groups.append(share)
            left -= share
        return groups

    def lookup_group(self, share):
        """`share` lookups over one table"""
        rng, meta, custom = self.rng, self.meta, self.custom
        pairs = rng.choice([1, 1, 2, 3])
        flat_all = self.case.pin == "merged6"  # six degree-1 inputs: 2 + 6 + 1 = 9
        fixed = not flat_all and share * self.batch <= 5 and rng.random() < 0.4  # a fixed table holds every circuit's inputs
        squared = not flat_all and rng.random() < 0.3
        table = self.table(pairs, fixed, squared)
        if pairs > 1:
            self.case.features.add("multi_pair_lookup")
        self.case.features.add("fixed_table" if fixed else "lookup_any_advice_table")
        phase = 0 if fixed else self.n_phases - 1
        table_degree = 2 if squared else 1
        for _ in range(share):
            flat = flat_all or rng.random() < 0.2
            # read by this lookup only: pair 0's private column (every pair's, for an ungated lookup)
            privates = [meta.advice_column() for _ in range(pairs if flat else 1)]
            sel = None if flat else meta.selector()
            env = self.env(phase)
            inputs = []
            for i in range(pairs):
                if flat:  # degree 1 and no selector: on every usable row a tuple of a small pool, whatever else the row holds
                    e = meta.query_advice(privates[i], custom.Rotation.cur())
                    if rng.random() < 0.4:
                        e = e + custom.Expression.constant(self.constant()) if rng.random() < 0.5 else custom.Expression.constant(rng.randrange(1, R)) * e
                else:
                    gate_e = meta.query_selector(sel)
                    room = MAX_DEGREE - 2 - table_degree - 1  # of the tree behind the selector
                    deg = min(room, rng.choice([1, 1, 1, 2, 2, 3]))
                    tree = self.expression(deg, env, wrap=lambda e: gate_e * (e + e))
                    if i == 0:
                        tree = tree + meta.query_advice(privates[0], custom.Rotation.cur())
                    e = gate_e * tree if rng.random() < 0.6 else tree * gate_e
                inputs.append(e)
            needs = set().union(*[_challenges_of(e) for e in inputs])
            if needs:
                self.case.features.add("challenge_in_lookup")
            if any(kind == INSTANCE for e in inputs for kind, _, _ in _queries_of(e)):
                self.case.features.add("instance_in_lookup")
            index = meta.lookup_any(f"lookup {len(meta.lookup_names)}", lambda meta: list(zip(inputs, table["exprs"])))
            info = {"private": privates[0].index, "rows": None, "needs": needs, "index": index, "flat": flat, "absent": rng.randrange(1, R)}
            self.case.lookups.append(info)
            table["users"].append({"info": info, "inputs": inputs, "selector": sel, "privates": privates, "flat": flat})
        self.todo.append(lambda: self.place_table(table))

    def place_table(self, table):
        """rows and values: the inputs' selectors, the private columns, then the table — inside synthesize() for advice sinks, over
        every circuit's phase-0 witness for fixed ones"""
        rng = self.rng
        u, B = self.case.u, self.batch
        valid = [r for r in range(u) if all(0 <= r + rot < u for rot in table["rots"])]
        users = table["users"]
        need = len(users) * (B if table["fixed"] else 1)
        assert need <= len(valid) - 1, "the draw of lookup_group keeps a table's lookups within its rows"
        slots = sorted(rng.sample(valid, max(need, len(valid) - 1 - rng.randint(0, 2))))  # one valid row at least stays the zero tuple
        table["slots"] = slots
        if table["selector"] is not None:
            self.selector_rows.append((table["selector"], slots))
        budget = max(1, len(slots) // need)  # distinct tuples each lookup of each circuit may bring
        for user in users:
            info, privates = user["info"], user["privates"]
            if user["flat"]:
                info["rows"] = list(range(u))
                pool = [[_field(rng) for _ in privates] for _ in range(min(budget, 3))]  # shared by the circuits; each picks its own rows
                picks = [[[rng.choice(pool) for _ in range(u)] for _ in range(B)]]
                picks = [[[tup[i] for tup in picks[0][c]] for c in range(B)] for i in range(len(privates))]
            else:
                safe = self.safe_rows(set().union(*[_queries_of(e) for e in user["inputs"]]))
                info["rows"] = sorted(rng.sample(safe, min(len(safe), rng.randint(1, min(budget, 6)))))
                self.selector_rows.append((user["selector"], info["rows"]))
                picks = [[[_field(rng) for _ in range(u)] for _ in range(B)]]

            def step(region, value, challenges, circuit, planted, info=info, privates=privates, picks=picks):
                for private, mine in zip(privates, picks):
                    for r in info["rows"]:
                        region.assign_advice(private, r, mine[circuit][r])

            self.steps.append(step)
        order_seed = rng.randrange(1 << 62)
        needs = set().union(*[user["info"]["needs"] for user in users])

        def tuples(value, challenges):
            """the distinct non-zero input tuples of every lookup over this table, in first-use order"""
            seen = []
            for user in users:
                exprs = [e.resolve(self.meta.n_user_fixed) for e in user["inputs"]]
                for r in range(u):
                    tup = tuple(e.evaluate(lambda kind, c, rot: value(kind, c, r + rot), challenges) for e in exprs)
                    if any(tup) and tup not in seen:
                        seen.append(tup)
            return seen

        def fill(seen, assign):
            order = random.Random(order_seed)
            assert len(seen) <= len(slots), "more distinct input tuples than table rows: the generator's budget is wrong"
            rows = list(seen)
            while len(rows) < len(slots):  # repeats, unused tuples, the zero tuple
                what = order.random()
                rows.append(order.choice(seen) if seen and what < 0.4 else tuple(0 for _ in table["sinks"]) if what < 0.6 else
                            tuple(_field(order) for _ in table["sinks"]))
            order.shuffle(rows)
            for r, tup in zip(slots, rows):
                for sink, rot, v in zip(table["sinks"], table["rots"], tup):
                    assign(sink, r + rot, v)

        if table["fixed"]:
            self.fixed_tables.append((tuples, fill, table))
        else:
            def step(region, value, challenges, circuit, planted):
                if any(challenges[c] is None for c in needs):
                    return
                fill(tuples(value, challenges), region.assign_advice)

            self.steps.append(step)

    # ---- shuffles --------------------------------------------------------------------------------------------------------------------
    def shuffle(self):
        rng, meta, custom = self.rng, self.meta, self.custom
        pairs = rng.choice([1, 1, 2])
        if pairs > 1:
            self.case.features.add("multi_pair_shuffle")
        env = self.env(self.n_phases - 1, flat=True)
        inputs = [self.expression(rng.randint(1, 3), env) for _ in range(pairs)]
        sinks = [meta.advice_column_in(self.n_phases - 1) for _ in range(pairs)]
        sides = [meta.query_advice(s, custom.Rotation.cur()) for s in sinks]
        index = meta.shuffle(f"shuffle {len(meta.shuffle_names)}", lambda meta: list(zip(inputs, sides)))
        needs = set().union(*[_challenges_of(e) for e in inputs])
        if any(kind == INSTANCE for e in inputs for kind, _, _ in _queries_of(e)):
            self.case.features.add("instance_in_shuffle")
        info = {"sinks": [s.index for s in sinks], "needs": needs, "index": index}
        self.case.shuffles.append(info)

        def place():
            u = self.case.u
            perm = list(range(u))
            rng.shuffle(perm)
            info["perm"] = perm

            def step(region, value, challenges, circuit, planted):
                if any(challenges[c] is None for c in needs):
                    return
                exprs = [e.resolve(meta.n_user_fixed) for e in inputs]
                for r in range(u):
                    for i, (sink, e) in enumerate(zip(sinks, exprs)):
                        v = e.evaluate(lambda kind, c, rot: value(kind, c, r + rot), challenges)
                        if planted == ("shuffle", index, perm[r]) and i == 0:
                            v = (v + 1) % R
                        region.assign_advice(sink, perm[r], v)

            self.steps.append(step)

        self.todo.append(place)

    # ---- copies ----------------------------------------------------------------------------------------------------------------------
    def copies(self):
        """the plan of copy constraints: into a scratch column of the last phase"""
        rng, meta = self.rng, self.meta
        scratch = meta.advice_column_in(self.n_phases - 1)
        meta.enable_equality(scratch)
        for col in self.eq_later:
            meta.enable_equality(col)
        self.scratch = scratch

        def place():
            u = self.case.u
            rows = list(range(u))
            rng.shuffle(rows)
            plan = []
            sources = [c for c in self.eq_columns if c.kind != INSTANCE]
            for _ in range(rng.randint(0, 3)):
                if sources and len(rows) > 4:
                    plan.append(("copy", rng.choice(sources), rng.randrange(u), rows.pop()))
            if sources and rng.random() < 0.5 and len(rows) > 6:
                plan.append(("chain", rng.choice(sources), rng.randrange(u), [rows.pop() for _ in range(rng.randint(2, 3))]))
            if sources and rng.random() < 0.4:
                plan.append(("self", rng.choice(sources), rng.randrange(u)))
            for j, col in enumerate(self.instances):
                if col in self.eq_columns and len(rows) > 2:
                    count = self.instance_counts[j]
                    row = rng.choice([0, max(count - 1, 0), count - 1 if count else min(2, u - 1)]) if rng.random() < 0.8 else rng.randrange(u)
                    plan.append(("instance", col, row, rows.pop()))
            self.copy_plan = plan
            # the copies' order in Assignment.copies, for plant(): one entry per simple copy_advice
            at = 0
            for item in plan:
                if item[0] == "copy":
                    self.case.copied.append((at, item[3]))
                at += len(item[3]) if item[0] == "chain" else 1

        self.todo.append(place)

    def run_copies(self, region, value, circuit, planted):
        custom = self.custom
        cell = lambda col, row: custom.Cell(col.kind, col.index, row, value(col.kind, col.index, row))
        for item in self.copy_plan:
            if item[0] == "copy":
                new = region.copy_advice(cell(item[1], item[2]), self.scratch, item[3])
                if planted == ("copy", item[3]):
                    region.assign_advice(self.scratch, item[3], new.value + 1)
            elif item[0] == "chain":
                c = cell(item[1], item[2])
                for row in item[3]:
                    c = region.copy_advice(c, self.scratch, row)
            elif item[0] == "self":
                region.constrain_equal(cell(item[1], item[2]), cell(item[1], item[2]))
            else:
                col, row, at = item[1:]
                region.constrain_instance(region.assign_advice(self.scratch, at, value(INSTANCE, col.index, row)), col, row)

    # ---- the whole -------------------------------------------------------------------------------------------------------------------
    def structure(self):
        rng = self.rng
        self.draw_shape()
        self.free_columns()
        items = ["gate"] * self.n_defined + [("lookups", g) for g in self.lookup_arguments()] + ["shuffle"] * self.n_shuffles
        rng.shuffle(items)
        if self.case.pin == "blinding":
            items.insert(rng.randrange(len(items) + 1), "wide")
        if self.case.pin == "degree9":
            items.insert(rng.randrange(len(items) + 1), "nine")
        i = 0
        while i < len(items):
            item = items[i]
            i += 1
            if item == "gate":
                count = 1
                while i < len(items) and items[i] == "gate" and rng.random() < 0.4:  # several polynomials in one create_gate
                    count, i = count + 1, i + 1
                self.defined_columns(count)
            elif item == "wide":
                self.defined_columns(1, wide=True)
            elif item == "nine":
                self.defined_columns(1, degree=MAX_DEGREE)
            elif item == "shuffle":
                self.shuffle()
            else:
                self.lookup_group(item[1])
        self.copies()
        if self.case.merged:
            self.meta.merge_lookups(MAX_DEGREE if self.case.pin == "merged6" or rng.random() < 0.5 else None)

    def finish(self):
        rng, meta, case = self.rng, self.meta, self.case
        case.cs, case.k = meta, self.k
        while case.u < MIN_USABLE:
            case.k += 1
        u, B = case.u, self.batch
        for index, cells in self.fixed_cells.items():  # the free fixed columns
            if cells is None:
                self.fixed_cells[index] = {r: _field(rng) for r in range(u) if rng.random() < 0.8}
        choices = sorted({c for c in (0, 1, 2, 3, 15, 16, 17, u - 1, u) if c <= u})
        self.instance_counts = [0 if col in self.empty else rng.choice(choices[1:]) for col in self.instances]
        self.instance_values = [[[_field(rng) for _ in range(count)] for count in self.instance_counts] for _ in range(B)]
        for column in [col for circuit in self.instance_values for col in circuit] + [cells for cells in self.fixed_cells.values() if cells]:
            if not any(column[r] for r in (column if isinstance(column, dict) else range(len(column)))) and len(column):
                column[max(column) if isinstance(column, dict) else -1] = R - 1  # all zeros is the zero polynomial too: see empty_term
        free_values = [{col.index: {r: _field(rng) for r in range(u) if rng.random() < 0.85} for col in self.free_advice} for _ in range(B)]

        def free_step(region, value, challenges, circuit, planted):
            for col in self.free_advice:
                for r, v in free_values[circuit][col.index].items():
                    region.assign_advice(col, r, v)

        placed = self.steps
        self.steps = [free_step]
        for todo in self.todo:  # in creation order: a column's step runs behind those of the columns it reads
            todo()
        assert not placed
        none = [None] * len(meta.challenge_phase)
        for tuples, fill, table in self.fixed_tables:  # the union of every circuit's inputs (they read phase-0 columns only)
            seen = []
            for circuit in range(B):
                asg = self.synthesize(circuit, none)
                value = self.value_of(asg)
                seen += [t for t in tuples(value, none) if t not in seen]
            fill(seen, lambda col, row, v: self.fixed_cells[col.index].__setitem__(row, v))
        case.synthesizers = [(lambda challenges, circuit=circuit: self.synthesize(circuit, challenges)) for circuit in range(B)]
        case._builder = self
        self.features()

    def value_of(self, asg):
        n = self.case.n
        inst = self.custom.instance_columns(asg)
        get = {ADVICE: lambda c, r: asg.advice[c].get(r, 0), FIXED: lambda c, r: asg.fixed[c].get(r, 0),
               INSTANCE: lambda c, r: inst[c][r] if r < len(inst[c]) else 0}
        return lambda kind, c, r: get[kind](c, r % n)

    def synthesize(self, circuit, challenges, planted=None):
        custom, meta = self.custom, self.meta
        challenges = list(challenges) + [None] * (len(meta.challenge_phase) - len(challenges))
        columns = self.instance_values[circuit]
        region = custom.Assignment(meta, instance=columns if meta.n_instance > 1 else columns[0] if columns else (), challenges=challenges)
        for index, cells in self.fixed_cells.items():
            for r, v in cells.items():
                region.assign_fixed(custom.Column(FIXED, index), r, v)
        for selector, rows in self.selector_rows:
            for r in rows:
                region.enable_selector(selector, r)
        value = self.value_of(region)
        for step in self.steps:
            step(region, value, challenges, circuit, planted)
        self.run_copies(region, value, circuit, planted)
        if planted is not None and planted[0] == "lookup":  # behind the table's step: the table holds the inputs as they were
            info = self.case.lookups[planted[1]]
            private = custom.Column(ADVICE, info["private"])
            region.assign_advice(private, planted[2], value(ADVICE, info["private"], planted[2]) + info["absent"])
        return region

    def features(self):
        case, cs, f = self.case, self.meta, self.case.features
        f.add(f"phases={cs.n_phases}")
        f.add(f"k={case.k}")
        ni, B, d = cs.n_instance, self.batch, cs.degree()
        f.add("instances=" + ("0" if ni == 0 else "1" if ni == 1 else "8" if ni == 8 else "2-7"))
        f.add("batch=" + (str(B) if B in (1, 2, 8) else "3-7"))
        f.add("degree" + ("<=4" if d <= 4 else "=5" if d == 5 else "=9" if d == 9 else "=6-8"))
        if cs.lookups:
            f.add("lookup")
        if case.logup:
            f.add("logup")
        elif cs.lookups:
            f.add("plain_lookup")
        if case.merged and any(len(arg) > 1 for arg in cs.lookup_arguments):
            f.update(["merged", "logup_merged"])
        if cs.shuffles:
            f.add("shuffle")
        if case.multiopen == "gwc":
            f.add("gwc")
        if cs.n_phases > 1:
            f.add("phases>1")
        if ni > 1:
            f.add("instances>1")
        if B > 1:
            f.add("batch>1")
        reached = {"instances8": ni == MAX_INSTANCE, "shuffles8": len(cs.shuffles) == MAX_SHUFFLES, "lookups8": len(cs.lookup_arguments) == MAX_LOOKUPS,
                   "merged6": max([len(arg) for arg in cs.lookup_arguments], default=0) == MAX_LOGUP_INPUTS, "degree9": d == MAX_DEGREE,
                   "challenges16": len(cs.challenge_phase) == MAX_CHALLENGES, "batch8": B == MAX_CIRCUITS, "blinding": cs.blinding_factors() > 5}
        if case.pin is not None:
            assert reached[case.pin], f"the pin {case.pin} is not at its limit: {case.describe()}"
            f.add("pin:" + case.pin)


def generate(custom, seed: int) -> Case:
    """the case of a seed: a pure function of it"""
    b = _Builder(custom, seed)
    b.structure()
    b.finish()
    return b.case


def challenges_for(case, seed: int = 0):
    """challenge values for a host run: what the transcript would squeeze, here drawn"""
    rng = random.Random(7919 * case.seed + seed)
    return [rng.randrange(1, R) for _ in case.cs.challenge_phase]


class _Blinded(dict):
    """an advice column's cells as mock reads them (`get`), with values on the blinding rows that the row check (`max`) does not see"""

    def __init__(self, cells, beyond):
        super().__init__(cells)
        self.beyond = beyond

    def get(self, row, default=0):
        return self.beyond[row] if row in self.beyond else super().get(row, default)


def blinded(case, asg, rng):
    """the assignment with rows u .. n-1 of every advice column holding random scalars, as in a proof.  mock refuses CELLS beyond the
    usable rows, so the values sit behind the cells: every read of mock's finds them, its NotEnoughRowsAvailable check does not"""
    asg.advice = [_Blinded(cells, {r: rng.randrange(R) for r in range(case.u, case.n)}) for cells in asg.advice]
    return asg


def plant(case, rng):
    """-> (faulty synthesize of circuit 0, expected): exactly one cell changed.  expected: {"kind": "gate" | "copy" | "lookup" |
    "shuffle", "index": polynomial / Assignment.copies / declared lookup / shuffle index, "name", "row" (gates and lookups: the only
    failing row; copies: the scratch row; shuffles: the changed sink row)}"""
    b = case._builder
    kinds = ["gate"] + (["copy"] if case.copied else []) + (["lookup"] if case.lookups else []) + (["shuffle"] if case.shuffles else [])
    kind = rng.choice(kinds)
    if kind == "gate":
        info = rng.choice(case.defined)
        row = rng.choice(info["rows"])
        planted = ("gate", info["poly"], row)
        expected = {"kind": kind, "index": info["poly"], "name": info["name"], "row": row}
    elif kind == "copy":
        at, row = rng.choice(case.copied)
        planted = ("copy", row)
        expected = {"kind": kind, "index": at, "name": None, "row": row}
    elif kind == "lookup":
        info = rng.choice(case.lookups)
        row = rng.choice(info["rows"])
        planted = ("lookup", info["index"], row)
        expected = {"kind": kind, "index": info["index"], "name": case.cs.lookup_names[info["index"]], "row": row}
    else:
        info = rng.choice(case.shuffles)
        row = rng.randrange(case.u)
        planted = ("shuffle", info["index"], row)
        expected = {"kind": kind, "index": info["index"], "name": case.cs.shuffle_names[info["index"]], "row": row}
    return (lambda challenges: b.synthesize(0, challenges, planted)), expected


def zero_column_circuit(custom, values=()):
    """What the first sweeps of generated circuits ran into, reduced: the gate s (a - i b c) has degree 4, and with the instance
    column i left without values (or all zero) the polynomial i(X) is zero, the gate reaches degree 2 and nothing else degree 4: the
    top piece of h(X) is the zero polynomial and its commitment the identity.  -> (cs, assignment), k = 4"""
    meta = custom.ConstraintSystem()
    a, b, c = meta.advice_column(), meta.advice_column(), meta.advice_column()
    i = meta.instance_column()
    s = meta.selector()
    cur = custom.Rotation.cur()
    meta.create_gate("a = i b c", lambda meta: [meta.query_selector(s) * (meta.query_advice(a, cur) - meta.query_instance(i, cur) * meta.query_advice(b, cur)
                                                                          * meta.query_advice(c, cur))])
    region = custom.Assignment(meta, instance=list(values))
    for row in range(6):
        region.assign_advice(b, row, 3 + row)
        region.assign_advice(c, row, R - 1 - row)
        region.assign_advice(a, row, (values[row] if row < len(values) else 0) * (3 + row) * (R - 1 - row))
        region.enable_selector(s, row)
    return meta, region


def mock_message(case, asg, expected) -> str:
    """what custom.mock raises for a planted fault"""
    kind, name, row = expected["kind"], expected["name"], expected["row"]
    if kind == "gate":
        return f"gate {name!r} not satisfied at row {row}"
    if kind == "copy":
        left, right = asg.copies[expected["index"]]
        return f"copy constraint {left} == {right} not satisfied"
    if kind == "lookup":
        return f"lookup {name!r} not satisfied at row {row}"
    return f"shuffle {name!r} not satisfied: the two sides are not the same multiset over the usable rows"


def pick_seeds(custom, candidates, limit: int = 24):
    """the greedy search behind GPU_SEEDS: the seed that covers the most of what is still missing, cheapest first among equals, until
    every feature and every pair of PAIR_FEATURES has occurred.  Run on the CPU (python -c "..." from tests/) after any change of the
    generator's draws; the result is committed below."""
    single, pairs = required_features()
    missing = set(single) | set(pairs)
    made = {seed: generate(custom, seed) for seed in candidates}
    cover = {seed: {f for f in single if f in c.features} | {p for p in pairs if p[0] in c.features and p[1] in c.features} for seed, c in made.items()}
    cost = {seed: (c.n << (c.cs.degree() - 2).bit_length()) * len(c.synthesizers) * (1 + c.cs.n_advice) for seed, c in made.items()}
    picked = []
    while missing and len(picked) < limit:
        best = max(made, key=lambda seed: (len(cover[seed] & missing), -cost[seed], -seed))
        if not cover[best] & missing:
            break
        picked.append(best)
        missing -= cover[best]
    return picked, missing


# pick_seeds over range(600), ordered by cost (the first eight also have their quotients recomputed in Python integers), and seven more
# of the cheapest seeds below 300 that mix at least four of PAIR_FEATURES
GPU_SEEDS = [190, 364, 205, 474, 221, 200, 536, 266, 125, 259, 255, 68, 592, 49, 370, 499, 598, 193]


def shuffle_failure(case, asg, index: int, challenges=()):
    """what the device check reports for shuffle `index` of an assignment: (index, smallest failing row, failing rows) over the usable
    rows whose input tuple is rarer on the shuffle side (shuffle_cases.expected_failures, for any number of instance columns)"""
    from collections import Counter

    value, u = case._builder.value_of(asg), case.u
    at = lambda e, row: e.evaluate(lambda kind, c, rot: value(kind, c, row + rot), challenges)
    pairs = case.cs.shuffles[index]
    ins = [tuple(at(a, row) for a, _ in pairs) for row in range(u)]
    shs = [tuple(at(s, row) for _, s in pairs) for row in range(u)]
    have, want = Counter(ins), Counter(shs)
    bad = [row for row in range(u) if have[ins[row]] > want[ins[row]]]
    return (index, bad[0], len(bad)) if bad else None


def witnesses(case):
    """what create_proof / prove_many / check take, per circuit: synthesize(challenges) for a constraint system with phases or
    challenges, the Assignment itself for one without (the prover's single advice call)"""
    if case.cs.phases() is not None:
        return list(case.synthesizers)
    return [s([]) for s in case.synthesizers]
