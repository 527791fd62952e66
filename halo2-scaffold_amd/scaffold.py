"""The reference's `src/scaffold.rs`, name for name, over the device prover: `mock`, `gen_key`, `prove_private`, `prove`.

The reference's examples are closures `f(ctx, input, make_public)` handed to these four functions (examples/halo2_lib.rs:62-71,
examples/range.rs:36-43, examples/linear_regression.rs:126-195); DEGREE, LOOKUP_BITS and MINIMUM_ROWS come from the environment
(src/scaffold.rs:44-50), the SRS from `gen_srs(k)` (read or created under PARAMS_DIR / ./params), the column counts from
`builder.config(k, Some(minimum_rows))`.  Here `ctx` is `flex.Context` (halo2-base's Context with the Gate / Range instructions as
methods: `ctx.mul`, `ctx.add`, `ctx.range_check(a, bits, lookup_bits)`, ...), `make_public` a list of its cells; the Range builder is
taken whenever LOOKUP_BITS is set, as in the reference.  Differences, by necessity: `prove_private` / `prove` do not run the crate's
`verify_proof` (there is no verifier in the product: the oracle's is test infrastructure) and return the proof bytes next to the
public inputs; blinding comes from a fresh 256-bit key per prover (`h2mi_prover_set_rng_key`), standing where the reference passes
`OsRng`.  Errors: an unsatisfied circuit raises ValueError from `mock` (MockProver's assert_satisfied), a lookup input outside the
table raises ValueError from the prover (ConstraintSystemFailure), "LOOKUP_BITS needs to be less than DEGREE" is asserted as there.
Added: `mock_device(f, private_inputs, pk)` — `mock` against a key `gen_key` made, on the device (flex.check): at DEGREE 20 - 22 the
prover says nothing about an unsatisfied gate or copy constraint, and its proof would be accepted by no verifier.
Added: `gen_key(..., witness_program=True)` records the closure's run as a witness program (witness.py); `prove_private` and
`mock_device` on such a key evaluate it on the device and do not call the closure.
"""
import json
import os

from . import flex, witness
from .params import gen_srs


def _env():
    k = int(os.environ.get("DEGREE", "18"))
    lookup_bits = int(os.environ["LOOKUP_BITS"]) if "LOOKUP_BITS" in os.environ else None
    if lookup_bits is not None:
        assert lookup_bits < k, "LOOKUP_BITS needs to be less than DEGREE"
    return k, lookup_bits, int(os.environ.get("MINIMUM_ROWS", "9"))


def _synthesize(f, inputs, cs, lookup_bits):
    """run the closure in a fresh context over `cs` -> the assignment (cells, copies, public inputs[, the Range builder's table])"""
    asg = flex.Assignment(cs)
    ctx = flex.Context(asg)
    ctx.lookup_bits = lookup_bits  # what RangeChip::default(lookup_bits) would carry
    make_public = []
    f(ctx, inputs, make_public)
    ctx.finish(make_public)
    if cs.lookup:
        flex.load_lookup_table(asg, lookup_bits)
    return asg


def _config(f, inputs, k, lookup_bits, minimum_rows):
    return flex.configure(lookup_bits is not None, k, lambda cs: _synthesize(f, inputs, cs, lookup_bits), minimum_rows)


def mock(f, private_inputs):
    """src/scaffold.rs:39-93: configure the circuit for the closure, then MockProver::run(k, &circuit, vec![public]).assert_satisfied()"""
    k, lookup_bits, minimum_rows = _env()
    cs = _config(f, private_inputs, k, lookup_bits, minimum_rows)
    flex.mock(_synthesize(f, private_inputs, cs, lookup_bits), k)


class ProvingKey:
    """what gen_key hands to prove_private: the device-resident keys, the SRS they were made against and one reusable prover"""

    def __init__(self, params, keys):
        self.params, self.keys = params, keys
        self.workspace = flex.FlexWorkspace(params, keys)
        self.workspace.prover.set_rng_key(os.urandom(32))  # the reference passes OsRng
        self.proofs = 0
        self.last_proof = None
        self.program = None  # gen_key(..., witness_program=True): the closure as a witness.Program

    @property
    def cs(self):
        return self.keys.cs

    def get_vk(self):
        return self.keys

    def release(self):
        if self.program is not None:
            self.program.release()
        self.workspace.release()
        self.keys.release()
        self.params.release()


def gen_key(f, dummy_inputs, by_coset: bool = False, table_depth: int = 1, key_file=None, logup: bool = False, lookup_sets=None,
            witness_program: bool = False):
    """src/scaffold.rs:95-156: the circuit's shape from a run on dummy inputs (GateThreadBuilder::keygen + builder.config), the SRS
    from gen_srs(k), keygen_vk + keygen_pk -> (pk, break_points).  by_coset: flex.FlexKeys' (no extended-coset columns on the device);
    table_depth: ParamsKZG's (every table_depth-th row of the MSM tables, as many passes per commitment).
    key_file ("in production the proving key is generated only once"): a path.  Where the file exists the key and the break points
    are read from it (flex.FlexKeys.load) and the closure is NOT called; where it does not, the key is generated as without the
    argument and written there, the break points and LOOKUP_BITS as JSON in the file's user section (a file made under another
    LOOKUP_BITS is refused with ValueError, as one made for another DEGREE is).  None: nothing is read or written.
    logup / lookup_sets: flex.FlexKeys' (the range checks proven by logUp against the key's sorted table, lookup_sets lookup-advice
    columns per argument).  Such a key has no file form: together with key_file it is a ValueError.
    witness_program: the run on the dummy inputs is recorded (witness.Program.record) and kept as pk.program; prove_private and
    mock_device on such a key do not call the closure again: they run the program on the device.  A closure a tape cannot express is
    refused here with ValueError.  The tape is not part of the key file: together with key_file it is a ValueError."""
    if logup and key_file is not None:
        raise ValueError("key_file with logup=True: the key-file format has no section for a logUp key of the builders' lookups")
    if witness_program and key_file is not None:
        raise ValueError("key_file with witness_program=True: the witness program is not part of the key file")
    k, lookup_bits, minimum_rows = _env()
    if key_file is not None and os.path.exists(key_file):
        params = gen_srs(k, table_depth=table_depth)
        try:
            keys = flex.FlexKeys.load(params, key_file, by_coset=by_coset)
        except Exception:
            params.release()
            raise
        stored = json.loads(keys.user.decode())
        if stored["lookup_bits"] != lookup_bits:  # the key's range table would disagree with ctx.lookup_bits at prove time
            keys.release()
            params.release()
            raise ValueError(f"key file: made with LOOKUP_BITS {stored['lookup_bits']}, the environment says {lookup_bits}")
        pk = ProvingKey(params, keys)
        pk.lookup_bits = lookup_bits
        return pk, stored["break_points"]
    cs = _config(f, dummy_inputs, k, lookup_bits, minimum_rows)
    program = None
    if witness_program:
        program, asg = witness.Program.record(f, dummy_inputs, cs, lookup_bits)
    else:
        asg = _synthesize(f, dummy_inputs, cs, lookup_bits)
    params = gen_srs(k, table_depth=table_depth)
    pk = ProvingKey(params, flex.FlexKeys(params, cs, asg, by_coset=by_coset, logup=logup, lookup_sets=lookup_sets))
    pk.lookup_bits = lookup_bits
    pk.program = program
    break_points = [list(asg.break_points)]
    if key_file is not None:
        pk.keys.save(key_file, json.dumps({"break_points": break_points, "lookup_bits": lookup_bits}).encode())
    return pk, break_points


def _witness(f, private_inputs, pk: ProvingKey, lookup_bits):
    """the witness of the private inputs: the closure run on the host, or — a key made with witness_program=True — its program run on the
    device without calling the closure (witness.assignment: columns in HBM, the public cells read back; ValueError("witness out of
    range ...") for a failed check, before anything is committed)"""
    if pk.program is None:
        return _synthesize(f, private_inputs, pk.cs, lookup_bits)
    asg = witness.assignment(pk.program, private_inputs)
    asg.break_points = list(pk.program.break_points)
    return asg


def prove_private(f, private_inputs, pk: ProvingKey, break_points, logup: bool = False, lookup_sets=None):
    """src/scaffold.rs:158-244: witness generation with the stored break points (GateThreadBuilder::prover), create_proof -> the public
    inputs (the proof bytes are kept in pk.last_proof).  logup / lookup_sets: what gen_key was given — the argument is the key's, so a
    pair that is not the key's is a ValueError"""
    same = bool(logup) == bool(getattr(pk.keys, "logup", False))
    if same and logup and lookup_sets is not None:
        runs = list(pk.cs.logup_runs)
        same = pk.cs.use_logup(lookup_sets) == runs
        pk.cs.use_logup(runs)  # the key's own grouping again, whatever was asked
    if not same:
        raise ValueError("prove_private: logup / lookup_sets are not the ones the key was generated with")
    _, lookup_bits, _ = _env()
    asg = _witness(f, private_inputs, pk, lookup_bits)
    if [list(asg.break_points)] != [list(b) for b in break_points]:
        raise ValueError("the circuit's break points differ from the ones stored at keygen: the closure's shape depends on its inputs")
    pk.proofs += 1
    pk.last_proof = flex.create_proof(pk.params, pk.keys, asg, pk.proofs, ws=pk.workspace)  # the seed is the keyed stream's per-proof nonce
    return list(asg.instance)


def mock_device(f, private_inputs, pk: ProvingKey):
    """`mock` at proving sizes: the witness of the private inputs checked on the device against the key `gen_key` made (flex.check:
    gates, copy constraints, lookups; ValueError naming the first violation) -> the public inputs.  No proof is made and none is
    verified; the advice commitments of the proof the check rides on are paid, and the nonce it takes is not used again."""
    _, lookup_bits, _ = _env()
    asg = _witness(f, private_inputs, pk, lookup_bits)
    pk.proofs += 1
    flex.check(pk.params, pk.keys, asg, pk.proofs, ws=pk.workspace)
    return list(asg.instance)


def prove(f, private_inputs, dummy_inputs, by_coset: bool = False, table_depth: int = 1, logup: bool = False, lookup_sets=None,
          witness_program: bool = False):
    """src/scaffold.rs:246-366: keygen on dummy inputs, then one proof of the private inputs -> (proof bytes, public inputs).
    witness_program: gen_key's (the proof's witness comes from the recorded program, on the device)"""
    pk, break_points = gen_key(f, dummy_inputs, by_coset=by_coset, table_depth=table_depth, logup=logup, lookup_sets=lookup_sets,
                               witness_program=witness_program)
    try:
        public_io = prove_private(f, private_inputs, pk, break_points, logup=logup)
        return pk.last_proof, public_io
    finally:
        pk.release()
