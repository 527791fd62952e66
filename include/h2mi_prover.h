/* h2mi_prover.h — the device-resident Halo2/KZG prover of libh2mi.so behind a phase-level C ABI.
 *
 * What it replaces.  The reference's callers make ONE call,
 *     create_proof::<KZGCommitmentScheme<Bn256>, ProverSHPLONK<'_, Bn256>, Challenge255<G1Affine>, _, Blake2bWrite<..>, _>(
 *         &params, &pk, &[circuit], &[instances], rng, &mut transcript)
 * (reference examples/standard_plonk.rs:40-50, src/scaffold.rs:190-200, 322-331), after keygen_vk / keygen_pk
 * (examples/standard_plonk.rs:33-34, src/scaffold.rs:132,135,284,287).  Inside the crate that call alternates between
 * the transcript (absorb commitments, squeeze a challenge) and heavy vector work that depends on the challenge just
 * squeezed.  This header cuts create_proof at exactly those points:
 *
 *     caller (Rust fork / C++ / Python)                      libh2mi.so
 *     ---------------------------------                      -----------------------------------------------------------
 *     witness generation (synthesize)      --- cells --->    h2mi_prover_advice      columns to HBM, blinding rows, commitments
 *     transcript: write points, squeeze theta
 *                                          --- theta --->    h2mi_prover_lookups     permuted input / table columns, commitments
 *     write points, squeeze beta, gamma    --- beta,gamma -> h2mi_prover_products    grand products, random polynomial, commitments
 *     write points, squeeze y              --- y --------->  h2mi_prover_quotient    evaluate_h / (X^n - 1), h pieces, commitments
 *     write points, squeeze x              --- x --------->  h2mi_prover_evaluations every queried evaluation, in write order
 *     write scalars, squeeze y', v         --- y', v ---->   h2mi_prover_shplonk_quotient   h(X) of ProverSHPLONK, commitment
 *     write point, squeeze u               --- u --------->  h2mi_prover_shplonk_open       L(X) / (X - u), commitment
 *     write point, finalize
 *
 * The caller owns witness generation and the Blake2b transcript (and therefore vk.transcript_repr, which the crate derives
 * from its own Debug text: nothing in the library depends on it).  The library owns every pass over a vector: workspaces,
 * streams, MSM batching, flush / join order, the coefficient and extended-coset forms, SHPLONK's rotation sets.  Only
 * 64-byte points and 32-byte scalars cross the boundary after the witness.
 *
 * `circuits` is a slice there.  One prover object (h2mi_prover_t) holds ONE circuit of a proof; several circuits against one key go
 * into one proof through a batch (h2mi_batch_t, below): the per-circuit phases — advice, lookups, products — stay on each member,
 * with the caller's transcript putting their points in the crate's order, and the joint ones — quotient, evaluations, SHPLONK — are
 * called once on the batch.  The fixed columns, the sigma columns, the random polynomial and h(X) are then opened once, not N times.
 *
 * The constraint system is DATA (h2mi_constraint_system).  Shapes accepted are the ones the reference proves:
 *   H2MI_GATES_STANDARD_PLONK  src/circuits/standard_plonk.rs:29-48 — q_a a + q_b b + q_c c + q_ab a b + constant
 *   H2MI_GATES_FLEX_VERTICAL   halo2-base's FlexGate through scaffold::prove (src/scaffold.rs:246-366, 379-485):
 *                              per gate column q (a + a(wX) a(w^2 X) - a(w^3 X)); up to H2MI_MAX_GATES (32) gate columns, up to
 *                              H2MI_MAX_LOOKUPS (8) single-expression lookups (a lookup-advice column, or q_lookup * a), one instance
 *                              column, up to H2MI_MAX_PERM (64) equality-enabled columns: every column count
 *                              `builder.config(k, Some(minimum_rows))` takes for a circuit that fills a few dozen columns
 *   H2MI_GATES_EXPRESSIONS     any `meta.create_gate(...)` (src/circuits/is_zero.rs, or.rs; the StandardPlonk and vertical gates too):
 *                              the gate polynomials as a postfix program beside the struct (h2mi_gate_program, h2mi.h: the `gates`
 *                              of h2mi_keygen_args) which ONE kernel interprets on the extended coset — any query of an advice,
 *                              fixed or instance column at any rotation, constants, + - *, degree up to 9 (permutation chunks up to
 *                              7); permutation and column limits as for FLEX_VERTICAL, but up to H2MI_MAX_INSTANCE (h2mi.h: 8)
 *                              instance columns, any of them in the permutation argument, in gates and on either side of a lookup
 *                              or shuffle (public inputs per column: h2mi_prover_instances).  Its lookups are either the
 *                              single-expression ones of FLEX_VERTICAL (cs->lookups[], a fixed table sorted once at keygen: the fast
 *                              path of range checks) or DATA as well — any `meta.lookup` / `meta.lookup_any`: per lookup a list of
 *                              (input expression, table expression) pairs in the same postfix form (h2mi_lookup_program: the record's
 *                              `lookups`), compressed with theta and sorted inside each proof.  Advice columns
 *                              of a later phase and challenges (h2mi_advice_phases: the record's `phases`): the
 *                              advice is then committed phase by phase (h2mi_prover_advice_phase) with the caller squeezing the
 *                              challenges in between, and gates and lookups may read them.  Shuffle arguments (`meta.shuffle` of
 *                              the PSE line of halo2_proofs, h2mi_shuffle_program: the record's `shuffles`): per
 *                              shuffle a list of (input expression, shuffle expression) pairs whose tuples must be the same multiset
 *                              over the usable rows; one grand product each, committed behind the lookups' products
 * Every function returns H2MI_OK or a negative H2MI_E* code (h2mi.h); no exception crosses the boundary.  Field elements
 * and points use the layouts of h2mi.h (4 / 8 uint64 limbs, Montgomery form).  A prover object is used by one thread at a time.
 */
#ifndef H2MI_PROVER_H
#define H2MI_PROVER_H

#include "h2mi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define H2MI_COL_ADVICE 0u
#define H2MI_COL_FIXED 1u
#define H2MI_COL_INSTANCE 2u
typedef struct {
  uint32_t kind;  /* H2MI_COL_* */
  uint32_t index; /* index within its kind */
} h2mi_column;
typedef struct {
  uint32_t column;  /* index within the kind the query list belongs to */
  int32_t rotation; /* Rotation(r): the query opens the column at omega^r x */
} h2mi_query;

#define H2MI_GATES_STANDARD_PLONK 1u
#define H2MI_GATES_FLEX_VERTICAL 2u
#define H2MI_GATES_EXPRESSIONS 3u /* cs->gates; n_gates / gate_advice / gate_selector are ignored: the gates are an h2mi_gate_program */

#define H2MI_MAX_GATES H2MI_FLEX_MAX_GATES     /* 32 */
#define H2MI_MAX_PERM H2MI_FLEX_MAX_PERM       /* 64 */
#define H2MI_MAX_LOOKUPS H2MI_FLEX_MAX_LOOKUPS /* 8 */
#define H2MI_MAX_ADVICE 64
#define H2MI_MAX_FIXED 64
#define H2MI_MAX_QUERIES 192

typedef struct {
  h2mi_column input;        /* the lookup's input column (advice) */
  int32_t selector_fixed;   /* >= 0: the input expression is fixed[selector_fixed] * input (halo2-base's single-column q_lookup); -1: the column itself */
  uint32_t table_fixed;     /* the fixed column holding the table */
} h2mi_lookup;

/* ConstraintSystem<Fr> after configure(): the numbers create_proof reads off `pk.vk.cs` */
typedef struct {
  uint32_t k;                 /* rows = 2^k */
  uint32_t n_advice, n_fixed; /* at most H2MI_MAX_ADVICE / H2MI_MAX_FIXED */
  uint32_t n_instance;        /* instance columns: 0 .. H2MI_MAX_INSTANCE (8) */
  uint32_t degree;            /* cs.degree(): extended domain 2^ceil(log2((degree - 1) n)), degree - 1 h pieces, permutation chunks of degree - 2 */
  uint32_t blinding_factors;  /* cs.blinding_factors() */
  uint32_t gates;             /* H2MI_GATES_* */
  uint32_t n_gates;           /* FLEX_VERTICAL: vertical gates (1 .. H2MI_MAX_GATES); STANDARD_PLONK: ignored (advice 0..2, fixed 0..4) */
  uint32_t gate_advice[H2MI_MAX_GATES];   /* advice column of gate g */
  uint32_t gate_selector[H2MI_MAX_GATES]; /* fixed column holding its selector */
  uint32_t n_perm;                         /* equality-enabled columns, in permutation-argument order */
  h2mi_column perm_columns[H2MI_MAX_PERM];
  uint32_t n_lookups;
  h2mi_lookup lookups[H2MI_MAX_LOOKUPS];
  uint32_t n_advice_queries, n_fixed_queries; /* in creation order: the order create_proof writes their evaluations */
  h2mi_query advice_queries[H2MI_MAX_QUERIES];
  h2mi_query fixed_queries[H2MI_MAX_QUERIES];
} h2mi_constraint_system;

/* assigned cells of one column: `count` values at `rows` (any order, each row once), or at rows 0 .. count - 1 when rows
 * is NULL; every other row of the column is zero.  values: count x 4 limbs.  H2MI_CELLS_CANONICAL in `flags`: the values
 * are canonical little-endian integers below r and the device converts them (for hosts without Montgomery arithmetic). */
#define H2MI_CELLS_CANONICAL 1u
/* H2MI_CELLS_RATIONAL: the column is handed over as the circuit ASSIGNED it, before batch_invert_assigned [RECALL halo2_proofs
 * v2023_02_02 plonk/assigned.rs Assigned::{Zero, Trivial, Rational}, Assigned::evaluate, poly.rs batch_invert_assigned, ff's BatchInvert
 * (zeros stay in place) — restated from memory like every crate convention here].  values: count x 8 limbs, numerator then denominator
 * per cell; the cell's value is numerator * denominator^-1, or 0 where the denominator is 0 (whatever the numerator).  Trivial(x)
 * travels as (x, 1), Zero as (0, 1) or as no cell at all.  With H2MI_CELLS_CANONICAL both halves are canonical integers below r (a half
 * that is not: H2MI_EINVAL, as for plain cells).  rows means what it means without the flag.  Accepted wherever fixed or advice cells
 * enter (h2mi_prover_keygen, h2mi_prover_advice, h2mi_prover_advice_phase, hence batches); h2mi_prover_instances refuses it
 * (H2MI_EINVAL): public inputs are field elements.  Short runs (rows NULL: up to 16 cells; a row list: up to 4096 — the runs that ride
 * in the phase's patch launch) are resolved on the host with one zero-skipping batched inversion per column; longer ones are uploaded
 * as pairs and all such columns of one call are resolved by ONE device chain with ONE field inversion (h2mi_fr_assigned_columns_dev;
 * two chains when canonical and Montgomery columns are mixed).  Everything downstream sees the resolved column, byte for byte what
 * the same values uploaded resolved give; the fixed column behind a cs->lookups[] table, which keygen also reads on the host to sort
 * it, is resolved there as well.  Each row once, as without the flag — and here it matters more: on the plain route the last of two
 * cells that name one row wins, on the device chain they are written in no order.  The chain stages 64 bytes per cell of all long
 * rational columns of the call in one slice of the library's grow-only scratch (three columns at k = 20: 192 MB): where that does not
 * fit the call is H2MI_ENOMEM although the resolved columns would. */
#define H2MI_CELLS_RATIONAL 2u
/* H2MI_CELLS_I64: values holds `count` signed 64-bit two's-complement integers, 8 bytes per cell (read through the pointer as int64_t;
 * 8-byte aligned), for the columns whose cells are small: range-check limbs, lookup advice, multiplicities, selectors, fixed-point
 * values, lookup tables.  The cell's value is v mod r: v for v >= 0, r - |v| for v < 0, -2^63 |-> r - 2^63.  rows means what it means
 * without the flag.  With H2MI_CELLS_CANONICAL or H2MI_CELLS_RATIONAL: H2MI_EINVAL.  Accepted wherever cells enter: 
 * h2mi_prover_keygen (the fixed column behind a cs->lookups[] table included), h2mi_prover_instances, h2mi_prover_advice,
 * h2mi_prover_advice_phase, hence batches.  Short runs (rows NULL: up to 16 cells; a row list: up to 4096) are converted on the host and
 * ride in the phase's patch launch like plain cells; longer ones are staged as they are — 8 bytes per cell plus 4 per listed row, where
 * plain scattered cells upload 32 bytes per row of their span — in the library's grow-only scratch (H2MI_ENOMEM where that does not
 * fit, as for the rational chain) and converted by the ONE launch that also serves the call's device columns (k_cells_scatter,
 * h2mi_fr_scatter_cells_dev).  Everything downstream sees the column byte for byte as the same values uploaded as field elements give. */
#define H2MI_CELLS_I64 4u
/* H2MI_CELLS_DEVICE: values, and rows when not NULL, are DEVICE addresses — any pointer the library's device can read: h2mi_malloc, a
 * torch tensor's data_ptr().  For callers whose witness is in HBM already.  Alone (32-byte Montgomery words, not range-checked, as on
 * the host), with H2MI_CELLS_CANONICAL or with H2MI_CELLS_I64; with H2MI_CELLS_RATIONAL: H2MI_EINVAL.  Accepted by h2mi_prover_advice and
 * h2mi_prover_advice_phase (hence batch members) only: h2mi_prover_instances (the caller hashes public inputs on the host and the library
 * keeps a host copy) and h2mi_prover_keygen (a key is made once, and a lookup table is sorted on the host) return H2MI_EINVAL, and
 * so does every entry after h2mi_init_devices with more than one device.  Pointers: 32-byte values 16-byte aligned, I64 values 8, rows 4
 * (H2MI_EINVAL).  The library reads the memory on its own stream: the caller has ordered its producer before the call, by a host
 * synchronise or by a wait placed on h2mi_library_stream.  The memory is free again when the call returns.  There is no host shortcut,
 * whatever the count: all non-empty device columns of a call, and its long I64 runs, are written by one k_cells_scatter launch.  What
 * the host routes find on the host is found on the device here and still returned by the same call, with no commitment and the proof
 * abandoned, the prover usable: H2MI_ERANGE for a listed row at or beyond 2^k - blinding_factors - 1 (a dense run longer than that is
 * refused before any launch), H2MI_EINVAL for a canonical value not below r.  Nothing is written outside the column's usable rows
 * whatever rows holds.  Each row once: cells that name the same row are written in no order, as on the rational chain. */
#define H2MI_CELLS_DEVICE 8u
typedef struct {
  const uint32_t* rows;
  const uint64_t* values;
  size_t count;
  uint32_t flags;
} h2mi_column_cells;
/* The rules above, on the host alone (it works without a GPU and reads no cell memory): what every entry point that takes cells applies
 * first.  `where` says which: H2MI_CELLS_FOR_ADVICE (h2mi_prover_advice / _advice_phase), _FOR_INSTANCE (h2mi_prover_instances),
 * _FOR_FIXED (h2mi_prover_keygen).  H2MI_EINVAL: cells NULL with n_columns > 0; an unknown `where`; a flag bit beyond the four
 * above; H2MI_CELLS_I64 with _CANONICAL or _RATIONAL; H2MI_CELLS_DEVICE with _RATIONAL or anywhere but on advice; for instances
 * H2MI_CELLS_RATIONAL or a row list; count > 0 with values NULL; a misaligned pointer — rows 4 bytes, values 8, the 32-byte values of a
 * device column 16.  H2MI_ERANGE: a count above 2^28, more rows than any column has (the usable rows are the entry points' to check). */
#define H2MI_CELLS_FOR_ADVICE 0u
#define H2MI_CELLS_FOR_INSTANCE 1u
#define H2MI_CELLS_FOR_FIXED 2u
int h2mi_column_cells_check(const h2mi_column_cells* cells, uint32_t n_columns, unsigned where);

typedef struct h2mi_pk_s* h2mi_pk_t;         /* keygen_pk's ProvingKey, resident in HBM */
typedef struct h2mi_prover_s* h2mi_prover_t; /* the buffers, streams and phase state of one create_proof at a time; reused from proof to proof */

/* ---- keygen_vk + keygen_pk (examples/standard_plonk.rs:33-34; src/scaffold.rs:284,287) ----------------------------------------
 * ONE call, h2mi_prover_keygen, takes ONE record, h2mi_keygen_args (at the end of this section, behind the structs it points to): the
 * constraint system, what the circuit has beside it — each an optional pointer — and the cells.  The key keeps its own copy of every
 * program and struct: the caller's memory is free after the call.
 * fixed: cs->n_fixed columns as the circuit's synthesize() (without witnesses) assigns them — selectors included, as the columns keygen
 * appends for them; a lookup's table column is the whole table.  copies: n_copies x 4 uint32 = (left column, left row, right column,
 * right row) per constrain_equal call, in call order, columns as indices into cs->perm_columns (permutation/keygen.rs Assembly::copy;
 * the order decides the sigma polynomials).  g_lagrange_handle: the FULL Lagrange SRS (h2mi_bases_register*) of 2^k points — keygen
 * commits the fixed and sigma columns against it.  flags: H2MI_KEYGEN_VK_ONLY builds only what keygen_vk returns (the commitments).
 * H2MI_ERANGE: a fixed cell or a copy constraint on a row at or beyond 2^k - blinding_factors - 1 (the crate's NotEnoughRowsAvailable).
 * The pk holds: fixed / sigma columns in Lagrange, coefficient and extended-coset form, l_0 / l_last / l_active cosets, the support
 * of the copy constraints, each lookup table's sorted distinct values. */
#define H2MI_KEYGEN_VK_ONLY 1u
/* H2MI_KEYGEN_LOGUP: every program lookup of the key is proven with the logarithmic-derivative argument ("logUp": Haboeck; the
 * `mv-lookup` feature of the Scroll and ezkl lines of halo2_proofs) in place of the permuted columns and the grand product.  Like the
 * shuffle it is RESTATED FROM MEMORY: DESIGN.md 4.5 and tests/logup_cases.py are the pin, not a crate.  Selection is per key — all of
 * its lookups or none.  A lookup of the key may hold several input tuples over its one table (h2mi_logup_inputs, below).
 * With cs->gates == H2MI_GATES_EXPRESSIONS it needs `lookups` (H2MI_EINVAL without); on a hard-wired shape it selects the table logUp
 * described with h2mi_table_logup_check below.  h2mi_lookup_program, its check, the required degree, blinding_factors and the query lists
 * are what they are without it.  Per lookup, with A and S the two sides compressed with theta and u the usable rows:
 *   M[r] = #{i < u : A[i] = S[r]} on the FIRST usable row r that holds its table value, 0 on every other usable row, blinding scalars
 *          on rows u .. 2^k - 1 (the permuted columns' stream: (blinding_factors + 1) scalars per lookup, in lookup order);
 *   phi[0] = 0, phi[i+1] = phi[i] + 1 / (A_i + beta) - M_i / (S_i + beta) for i < u, blinding scalars on rows u + 1 .. 2^k - 1 (the
 *          lookup products' stream: blinding_factors scalars per lookup); phi[u] = 0; gamma is not used.
 * h2mi_prover_lookups returns n_lookups points ([M], in lookup order) instead of 2 n_lookups and refuses an input that is no table
 * value with H2MI_EUNSAT, as without the flag; h2mi_prover_products returns [phi] in the lookup product's slot.  Quotient, per lookup
 * in the place of its five terms: l_0 phi, l_last phi, l_active ((phi(wX) - phi(X)) (A + beta)(S + beta) - ((S + beta) - M (A + beta))).
 * Evaluations per lookup in the place of its five: phi(x), phi(omega x), M(x); lookups.open: phi at x, phi at omega x, M at x.
 * h2mi_prover_check tests membership and does not depend on the argument.  Batches: M and phi per member, one joint quotient. */
#define H2MI_KEYGEN_LOGUP 2u
/* H2MI_KEYGEN_BY_COSET: the quotient is evaluated one coset of 2^k points at a time, and no column is kept in extended-coset form
 * (DESIGN.md 3 and 4.5 hold the memory formulas of both layouts).  Accepted alone or with H2MI_KEYGEN_LOGUP on a lookup
 * program (with the table logUp of a hard-wired shape: H2MI_EINVAL); with H2MI_KEYGEN_VK_ONLY it changes nothing.  The key holds its
 * fixed and sigma columns in Lagrange and coefficient
 * form and l_0 / l_last / l_active as coefficients; commitments, tables, moved cells and programs are the resident key's, and so is what
 * h2mi_prover_vk_commitments returns.  A prover on such a key holds no vector of 2^extended_k elements but h: per vector the numerator
 * reads, one slice of 2^k elements (a logUp lookup's input sets: sets 2^k, one slice behind the other), the slices of the key's shared
 * columns among them — in a batch the leader's are read, and the key stays immutable.  h2mi_prover_quotient / h2mi_batch_quotient then
 * run, for each slice c < 2^(extended_k - k): every column's coefficients to slice c (a 2^k-point transform with shift
 * zeta extended_omega^c), the lookups' and shuffles' sides compressed on the slices, ONE launch of the interpreting kernel over all
 * members (h2mi_plonk_evaluate_h_expr_batch_dev with a slice; a hard-wired shape through its equivalent program, as batches do).  Every phase and every
 * byte of the proof is the resident key's; instance columns always take the coefficient route.  The price is time: the fixed and sigma
 * slices are recomputed in every proof.  h2mi_prover_buffer / _pk_buffer: see the *_COSET kinds below. */
#define H2MI_KEYGEN_BY_COSET 8u /* bit 4 stays unassigned: keygen refuses it with H2MI_EINVAL, as it always has */
/* The gates as a program (`gates`): cs->gates == H2MI_GATES_EXPRESSIONS needs one, every other shape refuses one (H2MI_EINVAL).
 * h2mi_gate_program_check is the validation keygen applies, on the host alone (it works without a GPU): H2MI_EINVAL unless every op is
 * known, every column index is within n_advice / n_fixed / n_instance and every constant index within n_constants, |rotation| < 2^k,
 * the stack never underflows nor exceeds H2MI_MAX_EXPR_STACK and holds exactly one value at each END, the program ends with END and
 * holds at least one polynomial, every advice / fixed (column, rotation) it reads is in cs->advice_queries / cs->fixed_queries (no
 * verifier could check the proof otherwise), and every polynomial's degree (a query 1, a constant 0; ADD / SUB the larger, MUL the
 * sum) is at most cs->degree.  It reports the largest polynomial degree and the deepest stack (either pointer may be NULL). */
int h2mi_gate_program_check(const h2mi_constraint_system* cs, const h2mi_gate_program* gates, uint32_t* degree_out, uint32_t* max_stack_out);
/* The gate program equivalent to a hard-wired shape (host only, works without a GPU): for cs->gates == H2MI_GATES_STANDARD_PLONK the one
 * polynomial q_a a + q_b b + q_c c + q_ab a b + constant over advice 0..2 and fixed 0..4; for H2MI_GATES_FLEX_VERTICAL one polynomial
 * q_g (a + a(wX) a(w^2 X) - a(w^3 X)) per gate column g < cs->n_gates over (cs->gate_advice[g], cs->gate_selector[g]), in
 * evaluate_h's order.  Only cs->gates, n_gates, gate_advice and gate_selector are read.  The ops are written to `ops` (room for
 * ops_cap; H2MI_SHAPE_PROGRAM_MAX_OPS always suffices) and the constants to `constants` (constants_cap x 4 limbs; neither shape has
 * any today, so NULL / 0 is accepted); the counts go to n_ops_out / n_constants_out in every case, and H2MI_ERANGE says that a buffer
 * was too small and nothing was written.  H2MI_EINVAL for H2MI_GATES_EXPRESSIONS (the caller holds that program) or an unknown shape.
 * This is the program h2mi_prover_check runs for a key of those shapes, built once at keygen. */
#define H2MI_SHAPE_PROGRAM_MAX_OPS (10 * H2MI_MAX_GATES)
int h2mi_shape_gate_program(const h2mi_constraint_system* cs, h2mi_expr_op* ops, uint32_t ops_cap, uint32_t* n_ops_out, uint64_t* constants,
                            uint32_t constants_cap, uint32_t* n_constants_out);
/* Lookups as a program beside the constraint system: `meta.lookup(|meta| vec![(input, table), ..])` with any expressions on both sides,
 * advice in the table (lookup_any) and rotations included.  The argument compresses each side with the challenge theta, A = theta^(m-1)
 * a_0 + .. + a_(m-1) and S likewise (on all 2^k rows, rotations modulo 2^k), permutes and multiplies over the usable rows; transcript
 * order, quotient terms, openings and blinding streams are those of the single-expression lookups.
 * h2mi_lookup_program_check (host only, works without a GPU): H2MI_EINVAL unless n_lookups == cs->n_lookups (1 .. H2MI_MAX_LOOKUPS), every
 * n_pairs >= 1, exprs passes the rules of h2mi_gate_program_check except the degree rule (every advice / fixed query in the query
 * lists), holds exactly 2 * sum n_pairs polynomials, and every lookup's required degree max(4, 2 + max(1, input degrees) + max(1, table
 * degrees)) is at most cs->degree.  degree_out (may be NULL): the largest required degree.
 * `lookups` requires cs->gates == H2MI_GATES_EXPRESSIONS. */
typedef struct {
  uint32_t n_lookups;                 /* == cs->n_lookups; cs->lookups[] is then ignored */
  uint32_t n_pairs[H2MI_MAX_LOOKUPS]; /* >= 1 */
  h2mi_gate_program exprs;            /* per lookup: its n_pairs input polynomials, then its n_pairs table polynomials */
} h2mi_lookup_program;
int h2mi_lookup_program_check(const h2mi_constraint_system* cs, const h2mi_lookup_program* lookups, uint32_t* degree_out);
/* Advice phases and challenges beside the constraint system: `meta.advice_column_in(SecondPhase)`, `meta.challenge_usable_after(phase)`
 * and Expression::Challenge [RECALL halo2_proofs v2023_02_02 plonk/circuit.rs, plonk/prover.rs — restated from memory like the rest].
 * create_proof commits the advice columns phase by phase and squeezes, after each phase, the challenges usable after it; the next
 * phase's witness, any gate and either side of any lookup may read them (H2MI_EXPR_CHALLENGE, h2mi.h: degree 0).  Query lists,
 * blinding_factors, degree and the order of the evaluations do not depend on phases.
 * h2mi_advice_phases_check (host only, works without a GPU): H2MI_EINVAL unless cs->gates == H2MI_GATES_EXPRESSIONS, n_phases is 1 ..
 * H2MI_MAX_ADVICE_PHASES, every advice column's and every challenge's phase is below n_phases, every phase below n_phases holds a column
 * (the crate: a column in phase p > 0 needs one in phase p - 1, a challenge after p needs a column in p), n_challenges <=
 * H2MI_MAX_CHALLENGES, and `gates` / `lookups` (may be NULL) pass h2mi_gate_program_check / h2mi_lookup_program_check with CHALLENGE
 * ops of an index below n_challenges allowed — those two functions by themselves know of no challenges and refuse the op.
 * With n_phases == 1 and no challenges the key is the one `phases` == NULL makes. */
typedef struct {
  uint32_t n_phases;                                 /* 1 .. H2MI_MAX_ADVICE_PHASES */
  uint32_t advice_phase[H2MI_MAX_ADVICE];            /* phase of advice column j (cs->n_advice entries) */
  uint32_t n_challenges;                             /* <= H2MI_MAX_CHALLENGES, numbered in creation order */
  uint32_t challenge_phase[H2MI_MAX_CHALLENGES];     /* challenge i is squeezed after the commitments of this phase */
} h2mi_advice_phases;
int h2mi_advice_phases_check(const h2mi_constraint_system* cs, const h2mi_gate_program* gates, const h2mi_lookup_program* lookups,
                             const h2mi_advice_phases* phases);
/* Shuffle arguments beside the constraint system: `meta.shuffle(name, |meta| vec![(input, shuffle), ..])` [RECALL halo2_proofs, PSE
 * line, plonk/shuffle.rs, plonk/shuffle/prover.rs, plonk/shuffle/verifier.rs — restated from memory like everything else here, and
 * pinned only to the restatement in DESIGN.md 4.5 and tests/shuffle_cases.py, not to the crate].  Two tuples of expressions take the
 * same multiset of values over the usable rows.  Per shuffle of m >= 1 pairs A = theta^(m-1) a_0 + .. + a_(m-1) and S likewise from
 * the shuffle side (all 2^k rows, rotations modulo 2^k: the lookups' folding); z[0] = 1, z[i+1] = z[i] (A_i + gamma) / (S_i + gamma)
 * for i < u = 2^k - blinding_factors - 1, rows u + 1 .. 2^k - 1 blinding scalars, z[u] = 1 for a satisfied witness.  beta is not used.
 * Required degree 2 + max(1, input degrees, shuffle degrees), part of cs->degree.  create_proof commits the shuffle products behind
 * the lookup products and in front of the random polynomial; evaluate_h adds per shuffle, behind the circuit's lookup terms, l_0 (1 -
 * z), l_last (z^2 - z), l_active (z(wX) (S + gamma) - z(X) (A + gamma)); per shuffle z(x), z(omega x) are written behind the lookups'
 * evaluations and opened behind lookups.open.
 * h2mi_shuffle_program_check (host only, works without a GPU): H2MI_EINVAL unless n_shuffles is 1 .. H2MI_MAX_SHUFFLES (h2mi.h: 8), every
 * n_pairs >= 1, exprs passes the rules of h2mi_gate_program_check except the degree rule, holds exactly 2 * sum n_pairs polynomials,
 * and every shuffle's required degree is at most cs->degree.  degree_out (may be NULL): the largest required degree.  It knows of no
 * challenges and refuses H2MI_EXPR_CHALLENGE; h2mi_shuffle_phases_check is the same with CHALLENGE ops of an index below
 * phases->n_challenges allowed (phases == NULL: exactly the call above), as h2mi_advice_phases_check is for gates and lookups.
 * `shuffles` requires cs->gates == H2MI_GATES_EXPRESSIONS. */
typedef struct {
  uint32_t n_shuffles;                  /* 1 .. H2MI_MAX_SHUFFLES */
  uint32_t n_pairs[H2MI_MAX_SHUFFLES];  /* >= 1 */
  h2mi_gate_program exprs;              /* per shuffle: its n_pairs input polynomials, then its n_pairs shuffle-side polynomials */
} h2mi_shuffle_program;
int h2mi_shuffle_program_check(const h2mi_constraint_system* cs, const h2mi_shuffle_program* shuffles, uint32_t* degree_out);
int h2mi_shuffle_phases_check(const h2mi_constraint_system* cs, const h2mi_shuffle_program* shuffles, const h2mi_advice_phases* phases,
                              uint32_t* degree_out);
/* Several input sets over one table in a logUp lookup [the merging of lookups that share a table, restated from memory like the
 * argument itself: DESIGN.md 4.5 and tests/logup_sets_cases.py are the pin, not a crate].  Lookup l has K = n_inputs[l] input tuples A_1
 * .. A_K and one table tuple S, all of n_pairs[l] components; with an h2mi_logup_inputs, lookups->exprs holds per lookup its n_inputs x
 * n_pairs input polynomials (set by set), then its n_pairs table polynomials.  Every tuple is compressed with theta on all 2^k rows.
 *   M[r] = sum_j #{i < u : A_j[i] = S[r]} on the lowest usable row r that holds its table value, 0 on every other usable row; blinding
 *          rows, stream and offsets as with one set.  An input of ANY set that is no table value: H2MI_EUNSAT from h2mi_prover_lookups.
 *   phi[0] = 0, phi[i+1] = phi[i] + sum_j 1 / (A_j,i + beta) - M_i / (S_i + beta); phi[u] = 0.
 *   Quotient, per lookup: l_0 phi, l_last phi, l_active ((phi(wX) - phi(X)) D - N), with a_j = A_j + beta, s = S + beta, D = s prod_j a_j,
 *          N = s sum_j prod_{m != j} a_m - M prod_j a_j — by the recurrence (N, D) = (-M, s), then per input N <- N a_j + D, D <- D a_j.
 *   Required degree 2 + sum_j max(1, deg A_j) + max(1, deg S), deg A_j the largest degree among tuple j's components; with cs->degree
 *          <= 9 that allows H2MI_MAX_LOGUP_INPUTS (6) sets of degree-1 inputs.
 * A merged lookup is ONE argument: one [M], one [phi], three evaluations and three openings whatever K; counts, evaluation numbers and
 * buffer kinds are per argument.  Against K unmerged logUp lookups the proof loses (K - 1) x (2 points + 3 scalars); where the merge
 * raises cs->degree it gains one quotient piece per step.  The prover holds K + 1 compressed row vectors and K + 1 extended-coset vectors per lookup.
 * h2mi_logup_inputs_check (host only, works without a GPU): the rules of h2mi_lookup_program_check with sum (n_inputs + 1) n_pairs
 * polynomials and the degree rule above; every count in 1 .. H2MI_MAX_LOGUP_INPUTS; CHALLENGE ops of an index below phases->n_challenges
 * allowed (phases == NULL: none).  inputs == NULL: one set per lookup.  degree_out (may be NULL): the largest required degree.
 * Keygen: `inputs` without `lookups`, or a count other than 1 without H2MI_KEYGEN_LOGUP: H2MI_EINVAL.  All ones: the key inputs == NULL makes.
 * h2mi_prover_check tests the membership of every set: a lookup's entry counts the absent (row, set) pairs and names the smallest row. */
typedef struct {
  uint32_t n_inputs[H2MI_MAX_LOOKUPS]; /* 1 .. H2MI_MAX_LOGUP_INPUTS for the lookups->n_lookups lookups; the rest is not read */
} h2mi_logup_inputs;
int h2mi_logup_inputs_check(const h2mi_constraint_system* cs, const h2mi_lookup_program* lookups, const h2mi_logup_inputs* inputs,
                            const h2mi_advice_phases* phases, uint32_t* degree_out);
/* logUp for the single-expression lookups of a HARD-WIRED shape (cs->lookups[], the range checks of H2MI_GATES_FLEX_VERTICAL): the argument
 * stated for h2mi_logup_inputs above — the same M, phi, quotient terms, evaluations, openings, blinding streams and offsets — with every
 * tuple of ONE component, so theta does not enter: A_j is entry j's advice column, or fixed[selector_fixed] * advice, and S is the fixed
 * table column.  The table is fixed, so the key holds its distinct values sorted once, with first[r], the lowest usable row that holds
 * distinct value r (the padding zeros of the column count as rows); a proof then compresses nothing and sorts nothing: per argument ONE
 * h2mi_plonk_logup_rank_cols_dev over the input columns where they lie, and the running sum by rank (h2mi_plonk_logup_sum_ranked_dev: one
 * inversion per distinct table value, a gather per row).  The quotient runs through the shape's equivalent program
 * (h2mi_shape_gate_program), as batches do, with the advice columns' own extended cosets as the inputs.
 * Grouping: sets == NULL makes one argument per entry of cs->lookups; otherwise argument a takes the next sets->n_inputs[a] entries, in
 * order.  h2mi_table_logup_check (host only, works without a GPU) is the validation keygen applies before any device work; H2MI_EINVAL:
 * cs->gates == H2MI_GATES_EXPRESSIONS (such lookups are a program: `lookups`) or unknown; no lookups; a lookup's columns out
 * of range; a count of 0 or above H2MI_MAX_LOGUP_INPUTS; counts that do not sum to cs->n_lookups (the struct states no length: the counts are read
 * until they reach cs->n_lookups, and an argument that would pass the last entry is the violation); entries of one argument with different
 * table_fixed; cs->degree below an argument's 2 + sum_j deg A_j + 1, deg A_j = 2 with a selector and 1 without; and, for an argument of
 * SEVERAL entries, an entry with a selector or an advice column that another such argument (or the same one) reads already — the
 * quotient takes the K inputs as consecutive vectors, which the prover arranges by placing those columns' cosets behind one another.
 * degree_out (may be NULL): the largest required degree.  A permutation chunk of cs->degree - 2 columns may be longer than the three the
 * shape's own kernels take.
 * Keygen makes this key for H2MI_KEYGEN_LOGUP on a cs->gates other than H2MI_GATES_EXPRESSIONS, with `inputs` as the grouping (`sets`
 * here); H2MI_KEYGEN_VK_ONLY is accepted beside it, and H2MI_KEYGEN_BY_COSET or any of `gates`, `lookups`, `phases`, `shuffles` is
 * H2MI_EINVAL.  Two arguments over one fixed column share one sorted table in the key.  A proof of this key is byte for
 * byte the proof of the key made from the same circuit written as programs (gates = H2MI_GATES_EXPRESSIONS with
 * h2mi_shape_gate_program's program, one lookup per argument whose input polynomials are the entries' queries and whose table
 * polynomial is the fixed query, the same counts, H2MI_KEYGEN_LOGUP), for the same seed and challenges.  h2mi_prover_lookups returns one
 * [M] per argument and H2MI_EUNSAT for an input of any entry that is no table value; h2mi_prover_get_counts, h2mi_prover_buffer
 * (H2MI_BUF_LOGUP_M / _PHI per argument), h2mi_prover_check (per argument: the absent (row, entry) pairs), both multi-openings and
 * batches work as for any logUp key.  Beside a logUp key's M and phi a prover holds per argument 4 bytes per entry and row (the ranks)
 * and 4 per distinct table value, and no compressed vector.  h2mi_prover_pk_export of such a key is H2MI_EINVAL: the blob format has no
 * section for the grouping. */
int h2mi_table_logup_check(const h2mi_constraint_system* cs, const h2mi_logup_inputs* sets, uint32_t* degree_out);
/* The one keygen call.  Refusals, in this order: H2MI_EINVAL for args, pk_out or cs NULL, cs->n_fixed without fixed, n_copies without
 * copies, a flag bit beyond the three above; then, with *pk_out = NULL, the rules of the table logUp or — on every other record —
 * H2MI_EINVAL for H2MI_KEYGEN_LOGUP or `inputs` without `lookups` and for a count other than 1 without the flag; h2mi_column_cells_check;
 * H2MI_ENODEV without a device; the constraint system's and its programs' rules (the *_check functions among them). */
typedef struct {
  const h2mi_constraint_system* cs;
  const h2mi_gate_program* gates;       /* NULL: a hard-wired shape (cs->gates says which) */
  const h2mi_lookup_program* lookups;   /* NULL: the single-expression lookups cs->lookups[] */
  const h2mi_logup_inputs* inputs;      /* NULL: one input set per lookup; with the table logUp: one argument per entry of cs->lookups */
  const h2mi_advice_phases* phases;     /* NULL: one phase, no challenges */
  const h2mi_shuffle_program* shuffles; /* NULL: no shuffle argument */
  uint64_t g_lagrange_handle;
  const h2mi_column_cells* fixed;       /* NULL only with cs->n_fixed == 0 */
  const uint32_t* copies;               /* NULL only with n_copies == 0 */
  size_t n_copies;
  unsigned flags;                       /* H2MI_KEYGEN_* */
} h2mi_keygen_args;
int h2mi_prover_keygen(const h2mi_keygen_args* args, h2mi_pk_t* pk_out);
int h2mi_prover_pk_release(h2mi_pk_t pk); /* H2MI_EINVAL while a prover created against it is alive */
/* VerifyingKey::{fixed_commitments, permutation.commitments}: affine points (8 limbs each); either pointer may be NULL */
int h2mi_prover_vk_commitments(h2mi_pk_t pk, uint64_t* fixed_out /* n_fixed x 8 */, uint64_t* permutation_out /* n_perm x 8 */);

/* ---- proving-key files: "in production the proving key is generated only once" (the reference on gen_key) ------------------------------
 * A key leaves HBM as ONE self-describing blob and comes back without the circuit's synthesis.  The blob (DESIGN.md 3 is the normative
 * layout; little-endian, 8-byte-aligned sections with 64-bit lengths): magic and version, the logUp flag, its length, a 64-bit checksum
 * of everything else, the constraint system field by field, the gate / lookup / shuffle programs with the logUp input-set counts and the
 * advice phases where the key has them, per fixed column its nonzero cells as the device compacts them (h2mi_fr_compact_cells_dev, h2mi.h:
 * signed 64-bit integers where every cell fits, canonical 32-byte words otherwise; rows 0 .. last - 1 where that is no longer than a row
 * list), the cells the permutation moves (16 bytes each, sorted), the fixed and permutation commitments, and `user`.  Nothing else:
 * coefficients, cosets, l_0 / l_last / l_active, the active rows and the sorted tables are recomputed.
 * h2mi_prover_pk_export: `user` is an opaque section of up to 1 MiB for the host (break points, builder parameters).  buf == NULL: *len_out
 * is the blob's length and nothing is written; otherwise the blob goes to buf[0 .. cap) — H2MI_ERANGE, with *len_out set, when it does
 * not fit.  The same key exports the same bytes every time, and a resident and a by-coset key of one circuit export the same bytes.
 * H2MI_EINVAL: a H2MI_KEYGEN_VK_ONLY key (it holds no moved cells), user_len above 1 MiB.  With several devices the primary's columns
 * are read.
 * h2mi_prover_pk_blob_check: on the host alone (it works without a GPU), every validation import applies before its first device call —
 * the format's (lengths and counts against the blob's length and the ABI limits, rows strictly ascending and usable, moved cells sorted
 * and inside n_perm and the usable rows, no unknown version or flag bit, the checksum) and the constraint system's and its programs'
 * (what keygen applies, the *_check functions among it).  cs_out / user_out / user_len_out (each may be NULL) receive the
 * blob's constraint system — fields the shape does not read are zero — and its user section, a pointer into buf.
 * h2mi_prover_pk_import: flags 0 or H2MI_KEYGEN_BY_COSET — the layout in HBM is the importer's choice, whatever the exporter's was;
 * H2MI_KEYGEN_LOGUP is the blob's and not accepted here.  The cells go through the route keygen has (h2mi_column_cells with H2MI_CELLS_I64
 * or H2MI_CELLS_CANONICAL), the stored moved cells stand where keygen assembles the permutation, and from there on import IS keygen:
 * sigma columns, active rows, commitments, transforms, tables.  The recomputed commitments must be the stored ones: H2MI_EINVAL
 * otherwise — a damaged cell section and an SRS other than the key's are both found there.  H2MI_ERANGE: the Lagrange SRS is shorter
 * than 2^k, as at keygen.  A refused import leaves no key and no device allocation behind.  Multi-device modes: keygen's rules. */
int h2mi_prover_pk_export(h2mi_pk_t pk, const void* user, size_t user_len, void* buf, size_t cap, size_t* len_out);
int h2mi_prover_pk_blob_check(const void* buf, size_t len, h2mi_constraint_system* cs_out, const void** user_out, size_t* user_len_out);
int h2mi_prover_pk_import(const void* buf, size_t len, uint64_t g_lagrange_handle, unsigned flags, h2mi_pk_t* pk_out);

/* ---- one prover per (pk, SRS) ----------------------------------------------------------------------------------------------
 * g_handle / g_lagrange_handle: the base sets commitments are made against.  base_lo, base_count: they hold bases
 * [base_lo, base_lo + base_count) of the 2^k — the whole SRS (0, 2^k), or one rank's contiguous slice of it in the
 * one-process-per-GPU deployment: every commitment is then this rank's PARTIAL point and a combiner must be set. */
int h2mi_prover_create(h2mi_pk_t pk, uint64_t g_handle, uint64_t g_lagrange_handle, size_t base_lo, size_t base_count, h2mi_prover_t* prover_out);
int h2mi_prover_destroy(h2mi_prover_t prover);
/* sliced SRS: the phase's commitments are written as 96-byte Jacobian partial points to d_partial + 96 slot (slot < the largest of
 * h2mi_prover_counts' advice / lookups / products / quotient — the size both buffers must have, in points; 8 covers the reference's
 * StandardPlonk and one-column halo2-lib shapes); when a phase
 * reads its points back the library joins its MSM pipeline, calls combine(ctx, count) — which must leave the sums over all ranks of
 * slots 0 .. count - 1 at d_combined + 96 slot, ordered on the library's stream (h2mi_library_stream) or complete on return: an RCCL
 * all-gather + h2mi_g1_fold_groups_dev — and reads d_combined.  A nonzero return from combine fails the phase with H2MI_EHIP.
 * The callback runs on the calling thread, inside the phase call. */
typedef int (*h2mi_combine_fn)(void* ctx, size_t count);
int h2mi_prover_set_combiner(h2mi_prover_t prover, void* d_partial, void* d_combined, h2mi_combine_fn combine, void* ctx);

/* Where the blinding scalars come from (the crate takes them from its `rng` argument).  Default: counter-based SplitMix64 streams of the
 * 32-bit `seed` given to h2mi_prover_advice — reproducible, what the goldens and benchmarks use, NOT hiding against anyone who can guess
 * 32 bits.  With a key: every blinding scalar of the following proofs is Fr::from_u512 of one ChaCha20 block (RFC 7539 block function with
 * a 64-bit block counter and a 64-bit stream id, the layout of rand_chacha's ChaCha20Rng; one block per scalar, as `Fr::random(rng)`
 * consumes it) under this 256-bit key: block counter = the scalar's index, stream id = nonce << 3 | purpose (1 advice blinding rows,
 * 2 permutation products, 3 the vanishing argument's random polynomial, 4 permuted lookup columns, 5 lookup products, 6 shuffle
 * products), nonce = the `seed`
 * argument of h2mi_prover_advice (then below 2^61: a per-proof counter).  A fork fills the key from its rng once per prover.
 * key = NULL returns to the seeded streams.  Abandons a proof in flight. */
int h2mi_prover_set_rng_key(h2mi_prover_t prover, const uint8_t key[32]);

/* ---- the phases, in create_proof's order.  Every phase must be called once per proof, in this order (H2MI_EINVAL otherwise);
 * h2mi_prover_advice starts a new proof at any time.  points_out receive affine points, 8 limbs each, in the order create_proof writes
 * them to the transcript; the identity comes back as (0, 0) (the crate's transcript refuses it).  Each call returns when its points /
 * scalars are on the host; work that needs no further challenge (coefficient and extended forms of the columns just committed) keeps
 * running on the device behind it. */

/* advice[c]: the witness cells of advice column c (cs->n_advice of them), rows below 2^k - blinding_factors - 1.  instance: the public
 * inputs of the instance column of a key with at most one (count values, Montgomery; the caller hashes them into its transcript itself;
 * a key with several instance columns: h2mi_prover_instances, below, and 0 values here).  seed: stands where the
 * crate takes `rng` — every blinding scalar is drawn from counter-based SplitMix64 streams of this seed (h2mi_fr_random_dev's
 * generator: seed + 1 advice blinding rows, + 2 permutation products, + 3 the vanishing argument's random polynomial, + 4 permuted
 * lookup columns, + 5 lookup products, + 6 shuffle products; seed < 2^32), or — after h2mi_prover_set_rng_key — the per-proof nonce of the keyed ChaCha20
 * streams (< 2^61).
 * points_out: n_advice commitments. */
int h2mi_prover_advice(h2mi_prover_t prover, const h2mi_column_cells* advice, const uint64_t* instance, size_t n_instance_values, uint64_t seed,
                       uint64_t* points_out);
/* The public inputs of a circuit with several instance columns (`&[&[col_0], &[col_1], ..]` of create_proof), one entry per instance
 * column (cs->n_instance of them; NULL is accepted when there are none): `count` values on rows 0 .. count - 1 — rows must be NULL
 * (H2MI_EINVAL) — Montgomery, or canonical integers with H2MI_CELLS_CANONICAL; the other rows of the column are zero.  H2MI_ERANGE: a
 * column with more values than usable rows, 2^k - blinding_factors - 1 (the crate's InstanceTooLarge).  The library copies the values:
 * the caller's memory is free after the call.  The caller hashes them into its transcript itself: column by column, each column's
 * values in row order.
 * Called before h2mi_prover_advice (h2mi_prover_advice_phase with phase 0) and holds for THAT proof only, whether the call takes it or
 * refuses: a proof started without it has empty columns, except for what the `instance` argument of the advice call puts into column
 * 0.  That argument stays the route of a key with one instance column, where both routes are valid and give the same proof; values
 * through it on a key with several instance columns, or through both routes for one proof, are H2MI_EINVAL from the advice call.  A
 * refusal here leaves nothing behind and does not touch a proof in flight.  Columns of at most 16 values take no transform (one
 * launch for all of them, h2mi_plonk_instance_coset_multi_dev), longer ones are transformed one by one.
 * Batches: every member has its own instance columns; the call goes to the member, like its advice. */
int h2mi_prover_instances(h2mi_prover_t prover, const h2mi_column_cells* instance /* cs->n_instance entries */);
/* The same, one advice phase at a time (a key made with `phases`; on a one-phase key phase 0 IS h2mi_prover_advice, and
 * h2mi_prover_advice on a key with more phases is H2MI_EINVAL).  Per phase p = 0 .. n_phases - 1 the caller synthesizes with the
 * challenges known so far, calls this, writes points_out to its transcript and squeezes, in index order, the challenges whose phase
 * is p.  advice: cs->n_advice entries; only the columns of phase p are read, and an entry of another phase's column must have count ==
 * 0 (H2MI_EINVAL).  instance and seed are read at phase 0, which starts a new proof at any time.  points_out: this phase's commitments
 * in column order (h2mi_prover_get_phase_counts).  Phases come in order, each once: anything else is H2MI_EINVAL and abandons the
 * proof.  A column's blinding scalars do not depend on its phase.  The coefficient and extended forms of the phase's columns run on
 * the device while the caller generates the next phase's witness. */
int h2mi_prover_advice_phase(h2mi_prover_t prover, uint32_t phase, const h2mi_column_cells* advice, const uint64_t* instance,
                             size_t n_instance_values, uint64_t seed, uint64_t* points_out);
/* The values of all the circuit's challenges (n_challenges x 4 limbs, Montgomery), once per proof: after the last advice phase and
 * before h2mi_prover_lookups / h2mi_prover_products (any other time: H2MI_EINVAL, the proof is abandoned).  Required when the key has
 * challenges — the next phase is H2MI_EINVAL without it.  The library reads them in the lookups' compression and in the quotient;
 * witness generation, which reads them first, is the caller's. */
int h2mi_prover_set_challenges(h2mi_prover_t prover, const uint64_t* values);
/* The witness check, on the device at proving sizes: does the witness of the proof in flight satisfy the circuit, and where not?  What
 * MockProver::run(..).assert_satisfied() answers on the host; NOT a verification of anything (there is no verifier in this library).
 * When: after the last advice phase — on a key with challenges also after h2mi_prover_set_challenges — and before
 * h2mi_prover_products; at any other time H2MI_EINVAL.  The call is optional and read-only: phase state, buffers and blinding streams,
 * and therefore every byte of the proof, are the same with or without it, and no return value abandons the proof.  It runs behind the
 * advice fill on the library stream, on scratch of its own (allocated by the first call), and returns when the report is on the host.
 * H2MI_OK: nothing to report.  H2MI_EUNSAT: *n_out failures, the first `cap` of them written to `out`, in this order:
 *   H2MI_CHECK_GATE    per gate polynomial that is not zero somewhere: index = the polynomial in program order (a key of a hard-wired
 *                      shape: the program of h2mi_shape_gate_program), row = the smallest failing row, count = the failing rows.  All 2^k
 *                      rows of the BLINDED columns are tested — the condition under which the quotient is a polynomial.  A first row at
 *                      or beyond 2^k - blinding_factors - 1 says that the gate is not switched off on the blinding rows: MockProver does
 *                      not look there, the verifier does.
 *   H2MI_CHECK_COPY    at most one: count = the cells whose value differs from the cell the permutation maps them to, (index, row) = the
 *                      smallest such cell, index its column in the permutation argument's order.
 *   H2MI_CHECK_LOOKUP  per failing lookup: index = the lookup, row = the smallest usable row whose input is not a table value on a
 *                      usable row, count = such rows.  Lookups given as a program: both sides are compressed with `theta` on the rows and
 *                      the table side sorted, as the lookups phase does; theta must not be NULL and may be the transcript's or any
 *                      random value — two different tuples among u rows of m expressions collide, and hide a failure, with probability
 *                      about u^2 m / r (below 2^-190 at 2^28 rows).  The single-expression lookups compare q * a (or the column) with
 *                      the key's keygen-sorted table and ignore theta.
 *   H2MI_CHECK_SHUFFLE per failing shuffle, behind the lookups: index = the shuffle, count = the usable rows whose compressed input value
 *                      occurs more often among the inputs than on the shuffle side (not at all included), row = the smallest such row.
 *                      Both sides hold u rows, so unequal multisets always yield at least one such row.  Both sides are compressed
 *                      with `theta` on the rows and sorted (the lookups' sort and rank kernels); theta has the role and the collision
 *                      bound it has for program lookups.
 * Multi-device modes: the vectors are on the primary device, as for the lookups. */
#define H2MI_CHECK_GATE 0u
#define H2MI_CHECK_COPY 1u
#define H2MI_CHECK_LOOKUP 2u
#define H2MI_CHECK_SHUFFLE 3u
typedef struct { uint32_t kind /* H2MI_CHECK_* */, index, row, count; } h2mi_check_failure;
int h2mi_prover_check(h2mi_prover_t prover, const uint64_t theta[4], h2mi_check_failure* out, size_t cap, size_t* n_out);
/* theta compresses the lookups of a key made with a lookup program (each side's expressions folded with it on the rows, the
 * table's usable rows sorted on the device); the single-expression lookups do not use it.
 * points_out: per lookup the permuted input, then the permuted table commitment (2 x n_lookups; nothing without lookups — the call
 * may then be skipped — except on a key with shuffles, whose two sides the products phase compresses with this theta: there the call is
 * required, with theta, and returns no points when there are no lookups; h2mi_prover_products is H2MI_EINVAL without it).
 * H2MI_EUNSAT: a lookup input (a compressed input tuple) is not a table value (a table row). */
int h2mi_prover_lookups(h2mi_prover_t prover, const uint64_t theta[4], uint64_t* points_out);
/* points_out: the permutation argument's ceil(n_perm / (degree - 2)) grand products, one product per lookup, one product per shuffle,
 * then the vanishing argument's random polynomial: the order create_proof commits (and writes) them in.  H2MI_EUNSAT: a shuffle's
 * product over the usable rows is not one (one comparison of z[u]); the proof is abandoned. */
int h2mi_prover_products(h2mi_prover_t prover, const uint64_t beta[4], const uint64_t gamma[4], uint64_t* points_out);
/* points_out: the degree - 1 pieces of h(X) */
int h2mi_prover_quotient(h2mi_prover_t prover, const uint64_t y[4], uint64_t* points_out);
/* evals_out: every evaluation create_proof writes, in its order: advice queries, fixed queries, the random polynomial, the sigma
 * polynomials, per permutation product z(x), z(omega x) and — all but the last — z(omega^-(blinding_factors + 1) x), per lookup
 * z(x), z(omega x), A'(x), A'(omega^-1 x), S'(x), per shuffle z(x), z(omega x).  h2mi_prover_num_evaluations gives the count (4 limbs each). */
int h2mi_prover_num_evaluations(h2mi_prover_t prover, size_t* count_out);
int h2mi_prover_evaluations(h2mi_prover_t prover, const uint64_t x[4], uint64_t* evals_out);
/* ProverSHPLONK::create_proof (poly/kzg/multiopen/shplonk/prover.rs) over the queries create_proof collects, cut at its two commitments */
int h2mi_prover_shplonk_quotient(h2mi_prover_t prover, const uint64_t y[4], const uint64_t v[4], uint64_t point_out[8]);
int h2mi_prover_shplonk_open(h2mi_prover_t prover, const uint64_t u[4], uint64_t point_out[8]);
/* ProverGWC::create_proof (poly/kzg/multiopen/gwc [RECALL], as DESIGN.md 4.5 states it): the OTHER ending of a proof, in place of the
 * two SHPLONK calls — for callers whose verifier is a Gwc19 one.  The queries are grouped by point in order of first appearance (no
 * deduplication); per group W_i(X) = (sum_j v^j p_ij(X) - sum_j v^j e_ij) / (X - z_i), committed without blinding; points_out receives
 * [W_0] .. [W_(P-1)], written to the transcript in this order with nothing squeezed between them.  P = h2mi_prover_gwc_num_points: the
 * distinct rotations (modulo 2^k) of the key's queries — from the key alone, valid from h2mi_prover_create on.  The proof's tail is
 * 32 P bytes where SHPLONK's is 64.  Requires the evaluations to be the last phase, as h2mi_prover_shplonk_quotient does, and completes
 * the proof: a h2mi_prover_shplonk_* call behind it is H2MI_EINVAL as after any completed proof, and h2mi_prover_gwc_open behind
 * h2mi_prover_shplonk_quotient is H2MI_EINVAL and abandons the proof.  The W_i commitments are one phase of P MSMs (a combiner's buffers
 * hold the largest of the other phases: with one set the P go in that many at a time). */
int h2mi_prover_gwc_num_points(h2mi_prover_t prover, size_t* count_out);
int h2mi_prover_gwc_open(h2mi_prover_t prover, const uint64_t v[4], uint64_t* points_out /* count x 8 */);

/* ---- several circuits per proof: create_proof(&params, &pk, &[c_0, .., c_(N-1)], &[instances_0, ..], rng, &mut transcript) ----------
 * A batch binds N <= H2MI_MAX_CIRCUITS (h2mi.h: 8) ordinary provers of h2mi_prover_create, member i holding circuit i.  All members are
 * against the same pk with the same SRS handles and slice, none with a proof in flight (its last phase call, if any, was
 * h2mi_prover_shplonk_open or a refusal) and none bound already: H2MI_EINVAL otherwise (H2MI_EHANDLE for a dead handle).  While bound, a
 * member cannot be destroyed (H2MI_EINVAL, as h2mi_prover_pk_release is while a prover is alive); h2mi_batch_destroy makes the members
 * ordinary provers again and abandons a proof in flight.
 *
 * Per circuit, on its member, unchanged: h2mi_prover_advice / _advice_phase, _set_challenges, _check, _lookups, _products — one circuit
 * each, in any interleaving between members that respects each member's own order.  The caller's transcript orders the points as
 * create_proof does [RECALL halo2_proofs v2023_02_02 plonk/prover.rs]: per advice phase every circuit's commitments of that phase in
 * circuit order, then that phase's challenges; theta; every circuit's permuted lookup pairs; beta, gamma; every circuit's permutation
 * products; every circuit's lookup products; every circuit's shuffle products; the random polynomial; y; the h pieces; x; the evaluations; SHPLONK.
 * There is ONE random polynomial per proof: member 0's products phase draws and commits it as ever (last in its points_out); a bound
 * member with index > 0 neither draws nor commits one, so its points_out is one point shorter (h2mi_prover_get_counts says so) and
 * its H2MI_BUF_RANDOM_POLY is stale.  A caller that writes member 0's points first keeps the random polynomial's back until every
 * member's products are written.
 * A bound member's own h2mi_prover_quotient, _evaluations, _shplonk_quotient, _shplonk_open and _gwc_open return H2MI_EINVAL and abandon nothing.
 *
 * Joint, on the batch, each once per proof and in this order (H2MI_EINVAL otherwise, and the proof is abandoned — except for the
 * refusals of h2mi_batch_quotient listed next, which leave every member where it was):
 *   h2mi_batch_quotient         requires every member behind its h2mi_prover_products, all with the same beta and gamma and, on a key with
 *                               challenges, the same challenge values; and refuses members whose blinding streams could overlap — two
 *                               columns of one proof would be opened with the same blinding: seeded streams are seed + purpose (1 .. 6), so
 *                               two members' seeds must be at least 8 apart; under the same rng key two members need different nonces.
 *                               One kernel folds every circuit's gate, permutation, lookup and shuffle terms into h in circuit order
 *                               (h2mi_plonk_evaluate_h_expr_batch_dev); a key of a hard-wired shape goes through the equivalent program of
 *                               h2mi_shape_gate_program, which computes the same field elements as the shape's own kernel.
 *                               points_out: the degree - 1 pieces of h(X).
 *   h2mi_batch_evaluations      evals_out: every circuit's advice queries in circuit order; the fixed queries; the random polynomial; the
 *                               sigma polynomials; every circuit's permutation sets (per set as h2mi_prover_evaluations); every circuit's
 *                               lookups (per lookup likewise); every circuit's shuffles (per shuffle z(x), z(omega x)).
 *                               h2mi_batch_num_evaluations = N advice queries + fixed queries + 1 + n_perm
 *                               + N (3 n_sets - 1 if n_sets > 0) + N 5 n_lookups + N 2 n_shuffles.
 *   h2mi_batch_shplonk_quotient, h2mi_batch_shplonk_open
 *                               over the queries in create_proof's order: per circuit advice, permutation.open, lookups.open,
 *                               shuffles.open (z at x, then at omega x); then fixed,
 *                               sigma, h, the random polynomial.
 * The joint vectors are member 0's: h2mi_prover_buffer(member 0, H2MI_BUF_H / _H_POLY / _RANDOM_POLY / _SHPLONK_H / _SHPLONK_H2) reads
 * the batch's; every member's per-circuit buffers stay readable through the member.  The joint commitments go through member 0's result
 * slots and combiner (multi-device modes: the vectors are on the primary device). */
typedef struct h2mi_batch_s* h2mi_batch_t;
int h2mi_batch_create(const h2mi_prover_t* members, uint32_t n, h2mi_batch_t* batch_out);
int h2mi_batch_destroy(h2mi_batch_t batch);
int h2mi_batch_quotient(h2mi_batch_t batch, const uint64_t y[4], uint64_t* points_out);
int h2mi_batch_num_evaluations(h2mi_batch_t batch, size_t* count_out);
int h2mi_batch_evaluations(h2mi_batch_t batch, const uint64_t x[4], uint64_t* evals_out);
int h2mi_batch_shplonk_quotient(h2mi_batch_t batch, const uint64_t y[4], const uint64_t v[4], uint64_t point_out[8]);
int h2mi_batch_shplonk_open(h2mi_batch_t batch, const uint64_t u[4], uint64_t point_out[8]);
/* the GWC ending of a batch's proof, in place of the two calls above: h2mi_prover_gwc_open over every circuit's queries */
int h2mi_batch_gwc_num_points(h2mi_batch_t batch, size_t* count_out);
int h2mi_batch_gwc_open(h2mi_batch_t batch, const uint64_t v[4], uint64_t* points_out);

/* number of points the phases return, so that a caller can size buffers from the constraint system alone (products: without the random
 * polynomial for a bound member behind the first) */
typedef struct {
  uint32_t advice, lookups, products, quotient, evaluations;
} h2mi_prover_counts;
int h2mi_prover_get_counts(h2mi_prover_t prover, h2mi_prover_counts* out);
/* per advice phase: the commitments h2mi_prover_advice_phase returns (they sum to h2mi_prover_counts.advice) and the challenges to
 * squeeze behind them */
typedef struct {
  uint32_t n_phases, n_challenges;
  uint32_t advice[H2MI_MAX_ADVICE_PHASES];
  uint32_t challenges[H2MI_MAX_ADVICE_PHASES];
} h2mi_prover_phase_counts;
int h2mi_prover_get_phase_counts(h2mi_prover_t prover, h2mi_prover_phase_counts* out);

/* ---- device-resident intermediates, for callers that check or reuse them (the test-suite evaluates the quotient identity on them):
 * d_ptr_out / count_out receive the vector's address and its length in field elements.  Valid until the prover / pk is destroyed;
 * contents are those of the last proof. */
enum {
  H2MI_BUF_ADVICE = 0, H2MI_BUF_ADVICE_POLY, H2MI_BUF_ADVICE_COSET, H2MI_BUF_INSTANCE /* index < n_instance: that column's rows */,
  H2MI_BUF_PERM_Z, H2MI_BUF_PERM_Z_POLY, H2MI_BUF_PERM_Z_COSET,
  H2MI_BUF_LOOKUP_PERMUTED_INPUT, H2MI_BUF_LOOKUP_PERMUTED_TABLE, H2MI_BUF_LOOKUP_Z,
  H2MI_BUF_RANDOM_POLY, H2MI_BUF_H /* (degree - 1) n coefficients: piece i at i n */, H2MI_BUF_H_POLY,
  H2MI_BUF_SHPLONK_H, H2MI_BUF_SHPLONK_H2,
  H2MI_BUF_SHUFFLE_Z, H2MI_BUF_SHUFFLE_Z_POLY, H2MI_BUF_SHUFFLE_INPUT /* compressed rows */, H2MI_BUF_SHUFFLE_TABLE /* compressed rows */,
  H2MI_BUF_LOGUP_M /* a logUp key's multiplicity column of lookup `index`, rows */, H2MI_BUF_LOGUP_PHI /* its running sum, rows */,
  H2MI_BUF_GWC_W /* W_index of the last h2mi_prover_gwc_open, n coefficients (a batch: member 0's); shares SHPLONK's scratch */,
  H2MI_PKBUF_FIXED = 64, H2MI_PKBUF_FIXED_POLY, H2MI_PKBUF_FIXED_COSET, H2MI_PKBUF_SIGMA, H2MI_PKBUF_SIGMA_POLY, H2MI_PKBUF_SIGMA_COSET,
  H2MI_PKBUF_L0_COSET, H2MI_PKBUF_L_LAST_COSET, H2MI_PKBUF_L_ACTIVE_COSET
};
/* A key made with H2MI_KEYGEN_BY_COSET holds no extended-coset column: the *_COSET kinds (H2MI_BUF_ADVICE_COSET, H2MI_BUF_PERM_Z_COSET,
 * H2MI_PKBUF_FIXED_COSET, _SIGMA_COSET, _L0_COSET, _L_LAST_COSET, _L_ACTIVE_COSET) are H2MI_EINVAL for it and for its provers.  Every
 * other kind is what it is for a resident key, H2MI_BUF_H included. */
int h2mi_prover_buffer(h2mi_prover_t prover, uint32_t kind, uint32_t index, void** d_ptr_out, size_t* count_out);
int h2mi_prover_pk_buffer(h2mi_pk_t pk, uint32_t kind, uint32_t index, void** d_ptr_out, size_t* count_out);

/* The bytes of the device vectors the prover's key (key_bytes_out) and the prover itself (prover_bytes_out) own: every column, form and
 * scratch vector allocated for them, 32 bytes per field element, as allocated so far (h2mi_prover_check's scratch and a long instance
 * column's coefficients appear with their first use).  Not counted: what the library shares among all keys — window tables of the
 * registered bases, twiddle and power tables, the scratch arena.  Either pointer may be NULL.  Resident and by-coset keys alike. */
int h2mi_prover_device_bytes(h2mi_prover_t prover, size_t* key_bytes_out, size_t* prover_bytes_out);

#ifdef __cplusplus
}
#endif
#endif /* H2MI_PROVER_H */
