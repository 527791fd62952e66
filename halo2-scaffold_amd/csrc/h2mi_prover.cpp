// h2mi_prover.cpp — the device-resident prover behind include/h2mi_prover.h: keygen_vk / keygen_pk and create_proof, cut at
// the transcript's challenges (reference examples/standard_plonk.rs:33-34,40-50; src/scaffold.rs:284,287,322-331).
//
// Host code only: every pass over a vector is one of the library's own *_dev entry points (h2mi.h), called here in
// create_proof's order [halo2_proofs v2023_02_02 plonk/{keygen,prover}.rs, plonk/permutation/*, plonk/lookup/*, plonk/vanishing/*,
// poly/kzg/multiopen/shplonk* — an un-vendored dependency of the reference (Cargo.toml:13), restated from memory; the oracle
// (oracle/prover.py, oracle/flex.py) is the same restatement and the parity tests compare proof bytes].  What this file decides is
// the SCHEDULE: which stream a launch goes to, when queued bucket reductions are flushed, which commitments share one set of
// launches — the part rounds 2-4 tuned on the two former hosts (include/h2mi_plonk.hpp, halo2-scaffold_amd/prover.py + flex.py),
// which are now thin callers of these phases.
#include <algorithm>
#include <array>
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <set>
#include <vector>

#include "../../include/h2mi_prover.h"
#include "h2mi_expr.hpp"
#include "h2mi_hostmath.hpp"
#include "h2mi_keyfile.hpp"

namespace {

using namespace h2mi;
using namespace h2mi::plonk;
using arithmetic::DeviceVec;
typedef std::unique_ptr<DeviceVec> Dev;

Dev vec(size_t count) { return Dev(new DeviceVec(count)); }
Dev zeros(size_t count) {
  Dev d = vec(count);
  check(h2mi_memset_zero(d->p, count * 32), "zero");
  return d;
}
inline void* at(const DeviceVec& d, size_t row) { return (char*)d.p + row * 32; }

// long runs of rational cells (H2MI_CELLS_RATIONAL), collected across the columns of a phase or a keygen: ONE device chain and one
// field inversion for all of them (h2mi_fr_assigned_columns_dev), each column's cells landing in its own column.  Columns whose
// halves are canonical integers and columns of Montgomery words are two chains: the conversion is per launch
struct RationalList {
  std::vector<h2mi_assigned_cells> cols[2];
  void add(const DeviceVec& d, const h2mi_column_cells& c) { cols[c.flags & H2MI_CELLS_CANONICAL ? 1 : 0].push_back({d.p, c.rows, c.values, c.count}); }
  void flush() {
    for (int canonical = 0; canonical < 2; canonical++) {
      std::vector<h2mi_assigned_cells> list;
      list.swap(cols[canonical]);
      if (list.empty()) continue;
      uint64_t bad = 0;
      check(h2mi_fr_assigned_columns_dev(list.data(), (uint32_t)list.size(), canonical, &bad, nullptr), "assigned cells");
      if (bad) throw Error(H2MI_EINVAL, "a cell value is not reduced modulo r");
    }
  }
};

// columns whose cells are in device memory (H2MI_CELLS_DEVICE) and long host runs of 64-bit integers (H2MI_CELLS_I64), collected across
// the columns of a phase or a keygen: ONE k_cells_scatter launch for all of them (h2mi_fr_scatter_cells_staged_dev stages the host ones in
// the stream's scratch).  Rows and canonical values that only the device can see are refused here, from the kernel's status words: the
// flush precedes the phase's commitments, so a refused call returns none
struct ScatterList {
  std::vector<h2mi_cells_source> cols;
  uint64_t host_mask = 0;
  void add(const DeviceVec& d, const h2mi_column_cells& c, size_t row_limit) {
    if (cols.size() == 64) flush();
    if (!(c.flags & H2MI_CELLS_DEVICE)) host_mask |= (uint64_t)1 << cols.size();
    cols.push_back({d.p, c.rows, c.values, c.count, (uint32_t)row_limit, c.flags & (H2MI_CELLS_CANONICAL | H2MI_CELLS_I64)});
  }
  void flush() {
    if (cols.empty()) return;
    std::vector<h2mi_cells_source> list;
    list.swap(cols);
    const uint64_t mask = host_mask;
    host_mask = 0;
    uint64_t status[2] = {0, 0};
    check(h2mi_fr_scatter_cells_staged_dev(list.data(), (uint32_t)list.size(), mask, status, nullptr), "scatter cells");
    if (status[0]) throw Error(H2MI_ERANGE, "assignment reaches into the blinding rows (NotEnoughRowsAvailable)");
    if (status[1]) throw Error(H2MI_EINVAL, "a cell value is not reduced modulo r");
  }
};

// cells that travel in kernel arguments (h2mi_fr_patch_cells_dev: one launch per 64), collected across the columns of a phase
struct PatchList {
  std::vector<void*> cells;
  std::vector<Fr> vals;
  RationalList rational;  // what the same columns resolve on the device
  ScatterList scatter;    // what the same columns take from device memory, or as long runs of 64-bit integers
  void add(const DeviceVec& d, size_t row, const Fr& v) {
    cells.push_back(at(d, row));
    vals.push_back(v);
  }
  // the blinding rows u + 1 .. 2^k - 1 behind product (or running sum) i of its phase: scalars bf i .. bf i + bf - 1 of its stream
  void add_tail(const DeviceVec& z, size_t u, uint32_t bf, const std::vector<Fr>& blind, size_t i) {
    for (uint32_t r = 0; r < bf; r++) add(z, u + 1 + r, blind[bf * i + r]);
  }
  void flush() {
    rational.flush();
    scatter.flush();
    if (!cells.empty()) check(h2mi_fr_patch_cells_dev(cells.data(), (const uint64_t*)vals.data(), cells.size(), nullptr), "patch_cells");
    cells.clear();
    vals.clear();
  }
};

// the 32-byte value at c.values + 4 * word: cell `word` of a plain column, half `word` of a rational one (numerator 2 i, denominator 2 i + 1)
// (a column of 64-bit integers, H2MI_CELLS_I64: cell `word` is v mod r — |v| in the low limb, the product with R^2, negated for v < 0)
Fr cell_value(const h2mi_column_cells& c, size_t word) {
  Fr v;
  if (c.flags & H2MI_CELLS_I64) {
    int64_t x;
    std::memcpy(&x, (const char*)c.values + 8 * word, 8);
    v = fr::mul(Fr{{x < 0 ? 0 - (uint64_t)x : (uint64_t)x, 0, 0, 0}}, fr::R2);
    return x < 0 ? fr::neg(v) : v;
  }
  std::memcpy(v.l, c.values + 4 * word, 32);
  if (!(c.flags & H2MI_CELLS_CANONICAL)) return v;
  for (int j = 3; j >= 0; j--) {
    if (v.l[j] < fr::MODULUS[j]) return fr::mul(v, fr::R2);
    if (v.l[j] > fr::MODULUS[j]) break;
  }
  throw Error(H2MI_EINVAL, "a cell value is not reduced modulo r");
}
// a short run of rational cells on the host: numerator / denominator, 0 where the denominator is 0 [RECALL Assigned::evaluate,
// batch_invert_assigned], one zero-skipping batched inversion per column.  (The launch-bound proofs of 2^5 .. 2^8 rows: the device
// chain is three launches and an upload.)
std::vector<Fr> resolve_rational(const h2mi_column_cells& c) {
  std::vector<Fr> v(c.count);
  for (size_t i = 0; i < c.count; i++) v[i] = cell_value(c, 2 * i + 1);
  v = fr::batch_invert_skip_zero(v);
  for (size_t i = 0; i < c.count; i++) v[i] = fr::mul(cell_value(c, 2 * i), v[i]);
  return v;
}

// h2mi_column_cells_check, as the entry points apply it; device memory is read on the primary device's stream only
void check_cells(const h2mi_column_cells* cells, uint32_t n_columns, unsigned where) {
  if (const int rc = h2mi_column_cells_check(cells, n_columns, where)) throw Error(rc, "column cells");
  for (uint32_t i = 0; i < n_columns; i++)
    if ((cells[i].flags & H2MI_CELLS_DEVICE) && h2mi_device_count() > 1) throw Error(H2MI_EINVAL, "device cells with more than one device");
}

// a column of n rows: zero, then the assigned cells.  Short runs ride in the phase's patch launch, long dense runs are one
// upload (canonical values converted where they land), long scattered runs are staged over their span.  Rational cells mirror that:
// short runs are resolved here and patched, long ones (dense or scattered) join the call's one device chain.  So do 64-bit integers:
// short runs are converted here and patched, long ones join the call's one scatter launch — as every non-empty device column does.
void fill_column(DeviceVec& d, size_t n, const h2mi_column_cells& c, size_t row_limit, PatchList& pl) {
  check(h2mi_memset_zero(d.p, n * 32), "zero");
  if (c.count == 0) return;
  if (!c.values) throw Error(H2MI_EINVAL, "column cells without values");
  const bool rational = (c.flags & H2MI_CELLS_RATIONAL) != 0, i64 = (c.flags & H2MI_CELLS_I64) != 0;
  if (c.flags & H2MI_CELLS_DEVICE) {  // no host shortcut: the values are not here, whatever the count.  The rows are the kernel's to check
    if (!c.rows && c.count > row_limit) throw Error(H2MI_ERANGE, "assignment reaches into the blinding rows (NotEnoughRowsAvailable)");
    pl.scatter.add(d, c, row_limit);
    return;
  }
  if (!c.rows) {
    if (c.count > row_limit) throw Error(H2MI_ERANGE, "assignment reaches into the blinding rows (NotEnoughRowsAvailable)");
    if (c.count <= 16) {
      const std::vector<Fr> resolved = rational ? resolve_rational(c) : std::vector<Fr>();
      for (size_t i = 0; i < c.count; i++) pl.add(d, i, rational ? resolved[i] : cell_value(c, i));
      return;
    }
    if (rational) {
      pl.rational.add(d, c);
      return;
    }
    if (i64) {  // 8 bytes per cell cross, and the launch that serves the call's device columns converts them
      pl.scatter.add(d, c, row_limit);
      return;
    }
    check(h2mi_memcpy_h2d(d.p, c.values, c.count * 32), "column cells");
    if (c.flags & H2MI_CELLS_CANONICAL) {
      uint64_t bad = 0;
      check(h2mi_fe_from_repr_dev(1, d.p, c.count, d.p, &bad), "from_repr");
      if (bad) throw Error(H2MI_EINVAL, "a cell value is not reduced modulo r");
    }
    return;
  }
  uint32_t lo = c.rows[0], hi = c.rows[0];
  for (size_t i = 0; i < c.count; i++) {
    lo = std::min(lo, c.rows[i]);
    hi = std::max(hi, c.rows[i]);
  }
  if (hi >= row_limit) throw Error(H2MI_ERANGE, "assignment reaches into the blinding rows (NotEnoughRowsAvailable)");
  if (c.count <= 4096) {
    const std::vector<Fr> resolved = rational ? resolve_rational(c) : std::vector<Fr>();
    for (size_t i = 0; i < c.count; i++) pl.add(d, c.rows[i], rational ? resolved[i] : cell_value(c, i));
    return;
  }
  if (rational) {
    pl.rational.add(d, c);
    return;
  }
  if (i64) {  // 12 bytes per cell instead of 32 per row of the span
    pl.scatter.add(d, c, row_limit);
    return;
  }
  std::vector<Fr> stage((size_t)hi - lo + 1, fr_zero());
  for (size_t i = 0; i < c.count; i++) stage[c.rows[i] - lo] = cell_value(c, i);
  check(h2mi_memcpy_h2d(at(d, lo), stage.data(), stage.size() * 32), "column cells");
}

void to_poly(const poly::EvaluationDomain& dom, const DeviceVec& lagr, DeviceVec& poly, h2mi_stream_t stream = nullptr) {
  check(h2mi_ntt_bn254_fr_oop_dev(lagr.p, (size_t)1 << dom.k(), poly.p, dom.k(), dom.get_omega_inv().l, nullptr, dom.get_ifft_divisor().l, stream),
        "lagrange_to_coeff");
}
void to_poly_and_coset(const poly::EvaluationDomain& dom, const DeviceVec& lagr, DeviceVec& poly, DeviceVec& coset, h2mi_stream_t stream = nullptr) {
  to_poly(dom, lagr, poly, stream);
  check(h2mi_ntt_bn254_fr_oop_dev(poly.p, (size_t)1 << dom.k(), coset.p, dom.extended_k(), dom.get_extended_omega().l, dom.get_g_coset().l, nullptr, stream),
        "coeff_to_extended");
}

// commit device-resident columns against a registered base set -> affine points on the host (keygen: fixed and sigma columns)
std::vector<G1Affine> commit_points(uint64_t handle, const std::vector<Dev>& cols, size_t n) {
  const size_t k = cols.size();
  std::vector<G1Affine> pts(k);
  if (!k) return pts;
  DeviceVec out(3 * k), aff(2 * k);  // 96 B / 64 B per point
  for (size_t i = 0; i < k; i++) check(h2mi_msm_bn254_g1_dev(handle, cols[i]->p, n, (char*)out.p + 96 * i, nullptr), "commit");
  check(h2mi_join(), "join");
  check(h2mi_g1_batch_normalize_dev(out.p, k, aff.p, nullptr), "batch_normalize");
  check(h2mi_memcpy_d2h(pts.data(), aff.p, k * 64), "d2h");
  return pts;
}

// ---- the constraint system ---------------------------------------------------------------------------------------------------
static_assert(H2MI_EXPR_MAX_ADVICE == H2MI_MAX_ADVICE && H2MI_EXPR_MAX_FIXED == H2MI_MAX_FIXED, "h2mi_expr_cosets holds every column of a constraint system");
static_assert(H2MI_EXPR_ADVICE == H2MI_COL_ADVICE && H2MI_EXPR_FIXED == H2MI_COL_FIXED && H2MI_EXPR_INSTANCE == H2MI_COL_INSTANCE, "query ops are the column kinds");

// the rules of h2mi_gate_program_check (include/h2mi_prover.h)
int check_program(const h2mi_constraint_system& cs, const h2mi_gate_program* gates, h2::ExprShape* shape, uint32_t n_challenges = 0) {
  if (cs.k == 0 || cs.k > H2MI_MAX_LOG_N || cs.n_advice > H2MI_MAX_ADVICE || cs.n_fixed > H2MI_MAX_FIXED || cs.n_instance > H2MI_MAX_INSTANCE ||
      cs.n_advice_queries > H2MI_MAX_QUERIES || cs.n_fixed_queries > H2MI_MAX_QUERIES)
    return H2MI_EINVAL;
  auto listed = [](const h2mi_query* q, uint32_t count, uint32_t column, int32_t rotation) {
    for (uint32_t i = 0; i < count; i++)
      if (q[i].column == column && q[i].rotation == rotation) return true;
    return false;
  };
  h2::ExprShape sh;
  const int rc = h2::expr_walk(gates, cs.k, n_challenges, [&](uint32_t kind, uint32_t index, int32_t rotation) {
    if (kind == H2MI_EXPR_ADVICE) return index < cs.n_advice && listed(cs.advice_queries, cs.n_advice_queries, index, rotation);
    if (kind == H2MI_EXPR_FIXED) return index < cs.n_fixed && listed(cs.fixed_queries, cs.n_fixed_queries, index, rotation);
    return index < cs.n_instance;  // instance columns are not opened (KZG): no query list
  }, &sh);
  if (rc) return rc;
  if (sh.degree > cs.degree) return H2MI_EINVAL;
  if (shape) *shape = sh;
  return H2MI_OK;
}

// An expression block cut into arguments (lookups or shuffles): per argument the sub-programs of its input sets and of its table
// (shuffle) side, which point into exprs.ops and share its constants, and the largest degree among each part's polynomials.
constexpr uint32_t MAX_ARGUMENTS = std::max(H2MI_MAX_LOOKUPS, H2MI_MAX_SHUFFLES);
struct ArgumentSlices {
  uint32_t sets[MAX_ARGUMENTS];  // one but for a logUp lookup with several input sets
  h2mi_gate_program input[MAX_ARGUMENTS][H2MI_MAX_LOGUP_INPUTS], table[MAX_ARGUMENTS];
  uint32_t in_degree[MAX_ARGUMENTS][H2MI_MAX_LOGUP_INPUTS], tab_degree[MAX_ARGUMENTS];
};
// exprs holds per argument its sets[i] (NULL: one) x n_pairs[i] input polynomials, set by set, then its n_pairs[i] table polynomials
int slice_program(const h2mi_constraint_system& cs, const h2mi_gate_program& exprs, uint32_t n_args, const uint32_t* n_pairs, const uint32_t* sets,
                  uint32_t n_challenges, ArgumentSlices& out) {
  h2::ExprShape all;
  {
    h2mi_constraint_system any = cs;  // the structural rules and the query lists; the degree rule is per argument, the caller's
    any.degree = 0xffffffffu;
    const int rc = check_program(any, &exprs, &all, n_challenges);
    if (rc) return rc;
  }
  uint32_t want = 0;
  for (uint32_t i = 0; i < n_args; i++) {
    out.sets[i] = sets ? sets[i] : 1u;
    if (n_pairs[i] == 0 || n_pairs[i] > H2MI_MAX_EXPR_OPS) return H2MI_EINVAL;
    want += (out.sets[i] + 1) * n_pairs[i];
  }
  if (all.n_polys != want) return H2MI_EINVAL;
  uint32_t pos = 0;
  auto take = [&](uint32_t polys, h2mi_gate_program& sub) {  // the next `polys` polynomials -> their largest degree
    const uint32_t first = pos;
    for (uint32_t seen = 0; seen < polys; pos++) seen += exprs.ops[pos].op == H2MI_EXPR_END;
    sub = {exprs.ops + first, pos - first, exprs.constants, exprs.n_constants};
    h2::ExprShape sh;
    h2::expr_walk(&sub, cs.k, n_challenges, [](uint32_t, uint32_t, int32_t) { return true; }, &sh);  // validated above
    return sh.degree;
  };
  for (uint32_t i = 0; i < n_args; i++) {
    for (uint32_t j = 0; j < out.sets[i]; j++) out.in_degree[i][j] = take(n_pairs[i], out.input[i][j]);
    out.tab_degree[i] = take(n_pairs[i], out.table[i]);
  }
  return H2MI_OK;
}

// the rules of h2mi_lookup_program_check (include/h2mi_prover.h).
// With an h2mi_logup_inputs (the rules of h2mi_logup_inputs_check): lookup l holds sets[l] input tuples, input[l][j] is tuple j, and the
// required degree is the logUp rule 2 + sum_j max(1, deg A_j) + max(1, deg S) — with one set the number the lookup rule gives.
int check_lookup_program(const h2mi_constraint_system& cs, const h2mi_lookup_program* lp, uint32_t* degree_out, ArgumentSlices* slices,
                         uint32_t n_challenges = 0, const h2mi_logup_inputs* li = nullptr) {
  if (!lp || lp->n_lookups == 0 || lp->n_lookups > H2MI_MAX_LOOKUPS || lp->n_lookups != cs.n_lookups) return H2MI_EINVAL;
  for (uint32_t l = 0; li && l < lp->n_lookups; l++)
    if (li->n_inputs[l] == 0 || li->n_inputs[l] > H2MI_MAX_LOGUP_INPUTS) return H2MI_EINVAL;
  ArgumentSlices own, &sl = slices ? *slices : own;
  const int rc = slice_program(cs, lp->exprs, lp->n_lookups, lp->n_pairs, li ? li->n_inputs : nullptr, n_challenges, sl);
  if (rc) return rc;
  uint32_t degree = 0;
  for (uint32_t l = 0; l < lp->n_lookups; l++) {
    uint32_t in = 0;
    for (uint32_t j = 0; j < sl.sets[l]; j++) in += std::max(sl.in_degree[l][j], 1u);
    // [RECALL plonk/lookup.rs Argument::required_degree]; several sets: DESIGN.md 4.5
    const uint32_t d = std::max(4u, 2 + in + std::max(sl.tab_degree[l], 1u));
    if (d > cs.degree) return H2MI_EINVAL;
    degree = std::max(degree, d);
  }
  if (degree_out) *degree_out = degree;
  return H2MI_OK;
}

// the rules of h2mi_shuffle_program_check (include/h2mi_prover.h) [RECALL halo2_proofs (PSE line) plonk/shuffle.rs Argument::required_degree,
// restated from memory and pinned to DESIGN.md 4.5]
int check_shuffle_program(const h2mi_constraint_system& cs, const h2mi_shuffle_program* sp, uint32_t* degree_out, ArgumentSlices* slices,
                          uint32_t n_challenges = 0) {
  if (!sp || sp->n_shuffles == 0 || sp->n_shuffles > H2MI_MAX_SHUFFLES) return H2MI_EINVAL;
  ArgumentSlices own, &sl = slices ? *slices : own;
  const int rc = slice_program(cs, sp->exprs, sp->n_shuffles, sp->n_pairs, nullptr, n_challenges, sl);
  if (rc) return rc;
  uint32_t degree = 0;
  for (uint32_t i = 0; i < sp->n_shuffles; i++) {
    const uint32_t d = 2 + std::max({1u, sl.in_degree[i][0], sl.tab_degree[i]});
    if (d > cs.degree) return H2MI_EINVAL;
    degree = std::max(degree, d);
  }
  if (degree_out) *degree_out = degree;
  return H2MI_OK;
}

// the rules of h2mi_advice_phases_check (include/h2mi_prover.h) [RECALL halo2_proofs v2023_02_02 plonk/circuit.rs advice_column_in,
// challenge_usable_after]: a column in phase p > 0 needs one in phase p - 1 and a challenge usable after p needs a column in p — with
// n_phases stated, that is: every phase below n_phases holds a column, every column and every challenge names a phase below it
int check_phases(const h2mi_constraint_system& cs, const h2mi_gate_program* gates, const h2mi_lookup_program* lookups, const h2mi_advice_phases& ph,
                 const h2mi_logup_inputs* inputs = nullptr) {
  if (cs.gates != H2MI_GATES_EXPRESSIONS || !gates) return H2MI_EINVAL;
  if (ph.n_phases == 0 || ph.n_phases > H2MI_MAX_ADVICE_PHASES || ph.n_challenges > H2MI_MAX_CHALLENGES || cs.n_advice > H2MI_MAX_ADVICE) return H2MI_EINVAL;
  uint32_t columns[H2MI_MAX_ADVICE_PHASES] = {0, 0, 0};
  for (uint32_t j = 0; j < cs.n_advice; j++) {
    if (ph.advice_phase[j] >= ph.n_phases) return H2MI_EINVAL;
    columns[ph.advice_phase[j]]++;
  }
  for (uint32_t p = 0; p < ph.n_phases; p++)
    if (!columns[p]) return H2MI_EINVAL;
  for (uint32_t i = 0; i < ph.n_challenges; i++)
    if (ph.challenge_phase[i] >= ph.n_phases) return H2MI_EINVAL;
  int rc = check_program(cs, gates, nullptr, ph.n_challenges);
  if (!rc && lookups) rc = check_lookup_program(cs, lookups, nullptr, nullptr, ph.n_challenges, inputs);
  return rc;
}

// H2MI_KEYGEN_LOGUP on a hard-wired shape: logUp over cs->lookups[], with `inputs` as the grouping (h2mi_table_logup_check)
bool table_mode(const h2mi_keygen_args& args) { return (args.flags & H2MI_KEYGEN_LOGUP) && args.cs->gates != H2MI_GATES_EXPRESSIONS; }

void validate(const h2mi_keygen_args& args) {
  const h2mi_constraint_system& cs = *args.cs;
  auto bad = [](const char* what) { throw Error(H2MI_EINVAL, std::string("constraint system: ") + what); };
  const uint32_t n_ch = args.phases ? args.phases->n_challenges : 0;
  if (args.phases && check_phases(cs, args.gates, args.lookups, *args.phases, args.inputs)) bad("advice phases / challenges");
  if (cs.k == 0 || cs.k > H2MI_MAX_LOG_N) throw Error(H2MI_ERANGE, "constraint system: k");
  if (cs.degree < 3 || cs.degree > 9) bad("degree");
  if (((uint64_t)1 << cs.k) <= (uint64_t)cs.blinding_factors + 2) throw Error(H2MI_ERANGE, "constraint system: no usable rows");
  if (cs.n_advice == 0 || cs.n_advice > H2MI_MAX_ADVICE || cs.n_fixed > H2MI_MAX_FIXED || cs.n_instance > H2MI_MAX_INSTANCE) bad("column counts");
  if (cs.n_perm > H2MI_MAX_PERM || cs.n_lookups > H2MI_MAX_LOOKUPS) bad("permutation / lookup counts");
  if (cs.n_advice_queries > H2MI_MAX_QUERIES || cs.n_fixed_queries > H2MI_MAX_QUERIES) bad("query counts");
  for (uint32_t j = 0; j < cs.n_perm; j++) {
    const h2mi_column& c = cs.perm_columns[j];
    const uint32_t lim = c.kind == H2MI_COL_ADVICE ? cs.n_advice : c.kind == H2MI_COL_FIXED ? cs.n_fixed : c.kind == H2MI_COL_INSTANCE ? cs.n_instance : 0;
    if (c.index >= lim) bad("permutation column");
  }
  for (uint32_t i = 0; i < cs.n_advice_queries; i++)
    if (cs.advice_queries[i].column >= cs.n_advice) bad("advice query");
  for (uint32_t i = 0; i < cs.n_fixed_queries; i++)
    if (cs.fixed_queries[i].column >= cs.n_fixed) bad("fixed query");
  if (cs.gates == H2MI_GATES_STANDARD_PLONK) {
    // the circuit of reference src/circuits/standard_plonk.rs:29-48, which the specialised quotient kernel evaluates
    if (cs.n_advice != 3 || cs.n_fixed != 5 || cs.n_instance != 0 || cs.n_lookups != 0 || cs.degree != 3 || cs.n_perm != 3) bad("not the StandardPlonk shape");
    for (uint32_t j = 0; j < 3; j++)
      if (cs.perm_columns[j].kind != H2MI_COL_ADVICE || cs.perm_columns[j].index != j) bad("StandardPlonk's permutation runs over a, b, c");
  } else if (cs.gates == H2MI_GATES_FLEX_VERTICAL || cs.gates == H2MI_GATES_EXPRESSIONS) {
    if (cs.gates == H2MI_GATES_EXPRESSIONS) {
      // the permutation products take any chunk length, and so does the quotient kernel that interprets the program
      if (!args.gates) bad("gates given as expressions need a gate program");
      if (check_program(cs, args.gates, nullptr, n_ch)) bad("gate program");
    } else {
      if (cs.n_gates == 0 || cs.n_gates > H2MI_MAX_GATES) bad("gate count");
      for (uint32_t g = 0; g < cs.n_gates; g++)
        if (cs.gate_advice[g] >= cs.n_advice || cs.gate_selector[g] >= cs.n_fixed) bad("gate columns");
      // (a table-logUp key's quotient is the interpreting kernel's, which takes any chunk; merged arguments need the degree)
      if (cs.n_perm && cs.degree - 2 > 3 && !table_mode(args)) bad("permutation chunks longer than three columns");
    }
    if (args.lookups) {  // the lookups as a program: cs.lookups[] is not read
      if (cs.gates != H2MI_GATES_EXPRESSIONS) bad("a lookup program takes H2MI_GATES_EXPRESSIONS");
      if (check_lookup_program(cs, args.lookups, nullptr, nullptr, n_ch, args.inputs)) bad("lookup program");
    }
    for (uint32_t l = 0; !args.lookups && l < cs.n_lookups; l++) {
      const h2mi_lookup& lk = cs.lookups[l];
      if (lk.input.kind != H2MI_COL_ADVICE || lk.input.index >= cs.n_advice || lk.table_fixed >= cs.n_fixed) bad("lookup columns");
      if (lk.selector_fixed >= (int32_t)cs.n_fixed || lk.selector_fixed < -1) bad("lookup selector");
    }
  } else {
    bad("unknown gate shape");
  }
  uint32_t ext_k = cs.k;
  while (((uint64_t)1 << ext_k) < ((uint64_t)1 << cs.k) * (cs.degree - 1)) ext_k++;
  if (ext_k - cs.k > 4 || ext_k > H2MI_MAX_LOG_N) throw Error(H2MI_ERANGE, "constraint system: extended domain");
  if ((args.gates || args.lookups) && cs.gates != H2MI_GATES_EXPRESSIONS) bad("a gate or lookup program takes H2MI_GATES_EXPRESSIONS");
  if (args.shuffles) {
    if (cs.gates != H2MI_GATES_EXPRESSIONS) bad("a shuffle program takes H2MI_GATES_EXPRESSIONS");
    if (check_shuffle_program(cs, args.shuffles, nullptr, nullptr, n_ch)) bad("shuffle program");
  }
}

// the rules of h2mi_table_logup_check (include/h2mi_prover.h): the single-expression lookups of a hard-wired shape grouped, in order,
// into logUp arguments over their fixed tables -> per argument its first entry of cs.lookups and its number of entries
struct TableLogup {
  uint32_t n_args = 0;
  uint32_t first[H2MI_MAX_LOOKUPS], sets[H2MI_MAX_LOOKUPS];
};
int check_table_logup(const h2mi_constraint_system& cs, const h2mi_logup_inputs* li, uint32_t* degree_out, TableLogup* out) {
  if (cs.gates != H2MI_GATES_STANDARD_PLONK && cs.gates != H2MI_GATES_FLEX_VERTICAL) return H2MI_EINVAL;  // a program's lookups are a lookup program
  if (cs.n_lookups == 0 || cs.n_lookups > H2MI_MAX_LOOKUPS || cs.n_advice > H2MI_MAX_ADVICE || cs.n_fixed > H2MI_MAX_FIXED) return H2MI_EINVAL;
  for (uint32_t l = 0; l < cs.n_lookups; l++) {
    const h2mi_lookup& lk = cs.lookups[l];
    if (lk.input.kind != H2MI_COL_ADVICE || lk.input.index >= cs.n_advice || lk.table_fixed >= cs.n_fixed) return H2MI_EINVAL;
    if (lk.selector_fixed >= (int32_t)cs.n_fixed || lk.selector_fixed < -1) return H2MI_EINVAL;
  }
  TableLogup g;
  uint32_t used = 0, degree = 0;
  uint64_t merged = 0;  // advice columns that are an input of an argument with several: their extended cosets lie behind one another
  while (used < cs.n_lookups) {
    const uint32_t K = li ? li->n_inputs[g.n_args] : 1u;
    if (K == 0 || K > H2MI_MAX_LOGUP_INPUTS || K > cs.n_lookups - used) return H2MI_EINVAL;
    uint32_t d = 2 + 1;  // 2 + sum_j deg A_j + deg S [DESIGN.md 4.5]
    for (uint32_t j = 0; j < K; j++) {
      const h2mi_lookup& lk = cs.lookups[used + j];
      if (lk.table_fixed != cs.lookups[used].table_fixed) return H2MI_EINVAL;
      d += lk.selector_fixed >= 0 ? 2 : 1;
      if (K > 1) {  // the quotient reads the K input cosets as consecutive vectors: plain columns, each in one place only
        if (lk.selector_fixed >= 0 || ((merged >> lk.input.index) & 1u)) return H2MI_EINVAL;
        merged |= (uint64_t)1 << lk.input.index;
      }
    }
    if (d > cs.degree) return H2MI_EINVAL;
    degree = std::max(degree, d);
    g.first[g.n_args] = used;
    g.sets[g.n_args++] = K;
    used += K;
  }
  if (degree_out) *degree_out = degree;
  if (out) *out = g;
  return H2MI_OK;
}

struct Table {  // a lookup table's distinct usable values in ascending canonical order, for the device's counting sort
  Dev sorted, sorted_mont, mult;
  Dev first;  // a table-logUp key: per distinct value the lowest usable row that holds it (u32)
  uint32_t n_unique = 0;
  void alloc(size_t rows) {  // room for `rows` distinct values (h2mi_fr_sort_unique_dev inside a proof fills it)
    sorted = vec(rows);
    sorted_mont = vec(rows);
    mult = vec(rows / 8 + 1);
  }
};

}  // namespace

struct h2mi_pk_s {
  h2mi_constraint_system cs;
  poly::EvaluationDomain domain;
  size_t n, ext;
  uint32_t u, chunk, n_sets;
  bool vk_only = false;
  // H2MI_KEYGEN_BY_COSET: no extended-coset vector; l_0 / l_last / l_active as coefficients, every slice is a prover's
  bool by_coset = false;
  Dev l0_poly, l_last_poly, l_active_poly;
  int users = 0;  // provers created against this key and not yet destroyed
  Fr delta;
  std::vector<Dev> fixed_values, fixed_polys, fixed_cosets, sigma_values, sigma_polys, sigma_cosets;
  Dev l0, l_last, l_active, active_rows;
  uint32_t n_active = 0;
  Table tables[H2MI_MAX_LOOKUPS];
  std::vector<G1Affine> fixed_commitments, permutation_commitments;
  // H2MI_GATES_EXPRESSIONS: the key's own copy of the gate program
  std::vector<h2mi_expr_op> gate_ops;
  std::vector<uint64_t> gate_constants;
  h2mi_gate_program gate_program = {nullptr, 0, nullptr, 0};
  // lookups given as a program (h2mi_keygen_args.lookups): the key's own copy, cut into each lookup's input and table polynomials
  bool lookup_exprs = false;
  // H2MI_KEYGEN_LOGUP: every program lookup of the key is a logUp argument (multiplicities M and a running sum phi)
  bool logup = false;
  std::vector<h2mi_expr_op> lookup_ops;
  std::vector<uint64_t> lookup_constants;
  ArgumentSlices lookup_slices;
  // table logUp: logUp over the single-expression lookups of a hard-wired shape (logup && !lookup_exprs).  cs.n_lookups
  // is then the number of ARGUMENTS and cs.lookups[a] the first input of argument a; the caller's entries live here, argument by
  // argument, and tables[tl_table[a]] is argument a's table — arguments over one fixed column share one
  bool table_logup = false;
  uint32_t tl_sets[H2MI_MAX_LOOKUPS] = {0};
  h2mi_lookup tl_inputs[H2MI_MAX_LOOKUPS][H2MI_MAX_LOGUP_INPUTS];
  uint32_t tl_table[H2MI_MAX_LOOKUPS] = {0};
  // shuffle arguments (h2mi_keygen_args.shuffles): the key's own copy, cut into each shuffle's input and shuffle-side polynomials
  uint32_t n_shuffles = 0;
  std::vector<h2mi_expr_op> shuffle_ops;
  std::vector<uint64_t> shuffle_constants;
  ArgumentSlices shuffle_slices;
  // the pair counts of both programs as the caller stated them: what h2mi_prover_pk_export writes beside the ops
  uint32_t lookup_pairs[H2MI_MAX_LOOKUPS] = {0}, shuffle_pairs[H2MI_MAX_SHUFFLES] = {0};
  // advice phases and challenges (h2mi_keygen_args.phases); without them: one phase, no challenges
  h2mi_advice_phases phases;
  uint32_t phase_columns[H2MI_MAX_ADVICE_PHASES] = {0, 0, 0};
  // h2mi_prover_check: the cells the permutation moves, {column, row, image column, image row} sorted by (column, row), on the host
  // and on the device; the gate polynomials as a program whatever the shape (the key's own, or the hard-wired shape's equivalent)
  std::vector<uint32_t> moved_cells;
  Dev moved_cells_dev;
  std::vector<h2mi_expr_op> shape_ops;
  h2mi_gate_program check_gates = {nullptr, 0, nullptr, 0};
  explicit h2mi_pk_s(const h2mi_constraint_system& c)
      : cs(c), domain(c.degree, c.k), n((size_t)1 << c.k), ext(domain.extended_len()), u((uint32_t)n - (c.blinding_factors + 1)),
        chunk(c.degree - 2), n_sets(c.n_perm ? (c.n_perm + c.degree - 3) / (c.degree - 2) : 0), delta(fr_delta()) {}
};

namespace {

std::mutex g_reg_mu;
std::set<const void*> g_live_pks, g_live_provers, g_live_batches;
template <class T>
bool alive(const std::set<const void*>& s, T p) {
  std::lock_guard<std::mutex> lk(g_reg_mu);
  return p && s.count((const void*)p);
}

// with_first: also Table::first, per distinct value the lowest usable row that holds it — the padding zeros count as rows
void build_table(h2mi_pk_s& pk, Table& t, const h2mi_column_cells& cells, bool with_first = false) {
  // values on the usable rows, canonical and Montgomery; unassigned usable rows hold zero
  std::vector<std::pair<Fr, Fr>> vals;  // (canonical, montgomery)
  vals.reserve(cells.count);
  std::map<std::array<uint64_t, 4>, uint32_t> lowest;  // canonical value -> its lowest row (with_first)
  auto seen_at = [&](const Fr& canonical, uint32_t row) {
    const std::array<uint64_t, 4> key = {canonical.l[0], canonical.l[1], canonical.l[2], canonical.l[3]};
    auto it = lowest.find(key);
    if (it == lowest.end()) lowest[key] = row;
    else it->second = std::min(it->second, row);
  };
  std::vector<bool> assigned(with_first ? pk.u : 0, false);
  // this pass reads the caller's cells on the host (the sort below is the host's too): a rational table column is resolved here,
  // whatever its length, with the values the device column holds
  const std::vector<Fr> resolved = (cells.flags & H2MI_CELLS_RATIONAL) && cells.count ? resolve_rational(cells) : std::vector<Fr>();
  for (size_t i = 0; i < cells.count; i++) {
    const uint32_t row = cells.rows ? cells.rows[i] : (uint32_t)i;
    if (row >= pk.u) throw Error(H2MI_ERANGE, "lookup table larger than the usable rows (LOOKUP_BITS must be below DEGREE)");
    const Fr m = resolved.empty() ? cell_value(cells, i) : resolved[i];
    vals.push_back({to_canonical(m), m});
    if (with_first) {
      seen_at(vals.back().first, row);
      assigned[row] = true;
    }
  }
  const uint64_t zeros_extra = pk.u - cells.count;
  if (with_first && zeros_extra) seen_at(fr_zero(), (uint32_t)(std::find(assigned.begin(), assigned.end(), false) - assigned.begin()));
  auto less = [](const std::pair<Fr, Fr>& a, const std::pair<Fr, Fr>& b) {
    for (int i = 3; i >= 0; i--)
      if (a.first.l[i] != b.first.l[i]) return a.first.l[i] < b.first.l[i];
    return false;
  };
  if (!std::is_sorted(vals.begin(), vals.end(), less)) std::sort(vals.begin(), vals.end(), less);
  std::vector<Fr> canon, mont;
  std::vector<uint32_t> mult;
  if (zeros_extra && (vals.empty() || !(vals[0].first == fr_zero()))) {
    canon.push_back(fr_zero());
    mont.push_back(fr_zero());
    mult.push_back(0);
  }
  for (size_t i = 0; i < vals.size(); i++) {
    if (!canon.empty() && canon.back() == vals[i].first) {
      mult.back()++;
    } else {
      canon.push_back(vals[i].first);
      mont.push_back(vals[i].second);
      mult.push_back(1);
    }
  }
  if (zeros_extra) mult[0] += (uint32_t)zeros_extra;  // zero sorts first
  t.n_unique = (uint32_t)mult.size();
  t.alloc(mult.size());
  check(h2mi_memcpy_h2d(t.sorted->p, canon.data(), canon.size() * 32), "table");
  check(h2mi_memcpy_h2d(t.sorted_mont->p, mont.data(), mont.size() * 32), "table");
  check(h2mi_memcpy_h2d(t.mult->p, mult.data(), mult.size() * 4), "table");
  if (with_first) {
    std::vector<uint32_t> first;
    for (const Fr& c : canon) first.push_back(lowest.at({c.l[0], c.l[1], c.l[2], c.l[3]}));
    t.first = vec(first.size() / 8 + 1);
    check(h2mi_memcpy_h2d(t.first->p, first.data(), first.size() * 4), "table");
  }
}

// a caller's program copied into vectors the key owns -> the view over the copy
h2mi_gate_program own_program(const h2mi_gate_program& g, std::vector<h2mi_expr_op>& ops, std::vector<uint64_t>& constants) {
  ops.assign(g.ops, g.ops + g.n_ops);
  if (g.n_constants) constants.assign(g.constants, g.constants + 4 * (size_t)g.n_constants);
  return {ops.data(), g.n_ops, constants.data(), g.n_constants};
}

// One body, two front ends.  keygen proper (h2mi_prover_keygen): the caller's fixed cells and its copy constraints, from which the
// permutation is assembled.  Import (h2mi_prover_pk_import): the cells of a key file, handed over in the same h2mi_column_cells, and
// `stored_moved` — the moved cells a key once assembled, {column, row, image column, image row} ascending — in place of the assembly.
// From the moved cells on both run the same code: sigma columns, active rows, commitments, transforms, tables.  Import also hands over
// the blob's `stored_commitments` (n_fixed + n_perm points of 64 bytes): they are compared as soon as the key's own exist, before any
// transform is issued or any coefficient or coset vector allocated, so a blob that is refused there has cost the columns and two batches
// of MSMs.  The grouping of a table-logUp record (table_mode: args.inputs checked and resolved by check_table_logup) travels the same way.
struct KeygenExtra {
  const std::vector<std::array<uint32_t, 4>>* stored_moved = nullptr;
  const uint8_t* stored_commitments = nullptr;
  const TableLogup* table_logup = nullptr;
};
std::unique_ptr<h2mi_pk_s> keygen(const h2mi_keygen_args& args, const KeygenExtra& extra = {}) {
  validate(args);
  const h2mi_constraint_system& cs = *args.cs;
  std::unique_ptr<h2mi_pk_s> pkp(new h2mi_pk_s(cs));
  h2mi_pk_s& pk = *pkp;
  if (extra.table_logup) {  // from here on the key's lookups are the ARGUMENTS, each named by its first input
    const TableLogup& g = *extra.table_logup;
    pk.table_logup = pk.logup = true;
    pk.cs.n_lookups = g.n_args;
    for (uint32_t a = 0; a < g.n_args; a++) {
      pk.tl_sets[a] = g.sets[a];
      for (uint32_t j = 0; j < g.sets[a]; j++) pk.tl_inputs[a][j] = cs.lookups[g.first[a] + j];
      pk.cs.lookups[a] = cs.lookups[g.first[a]];
    }
  }
  std::memset(&pk.phases, 0, sizeof(pk.phases));
  pk.phases.n_phases = 1;
  if (args.phases) pk.phases = *args.phases;
  for (uint32_t j = 0; j < cs.n_advice; j++) pk.phase_columns[pk.phases.advice_phase[j]]++;
  if (args.gates) pk.gate_program = own_program(*args.gates, pk.gate_ops, pk.gate_constants);
  if (args.lookups) {
    pk.lookup_exprs = true;
    h2mi_lookup_program own = *args.lookups;
    std::memcpy(pk.lookup_pairs, args.lookups->n_pairs, sizeof(pk.lookup_pairs));
    own.exprs = own_program(args.lookups->exprs, pk.lookup_ops, pk.lookup_constants);
    // an h2mi_logup_inputs is copied into the slices (their `sets`): the key reads the caller's struct here and never again
    if (check_lookup_program(cs, &own, nullptr, &pk.lookup_slices, pk.phases.n_challenges, args.inputs)) throw Error(H2MI_EINVAL, "lookup program");
  }
  if (args.shuffles) {
    pk.n_shuffles = args.shuffles->n_shuffles;
    h2mi_shuffle_program own = *args.shuffles;
    std::memcpy(pk.shuffle_pairs, args.shuffles->n_pairs, sizeof(pk.shuffle_pairs));
    own.exprs = own_program(args.shuffles->exprs, pk.shuffle_ops, pk.shuffle_constants);
    if (check_shuffle_program(cs, &own, nullptr, &pk.shuffle_slices, pk.phases.n_challenges)) throw Error(H2MI_EINVAL, "shuffle program");
  }
  pk.vk_only = (args.flags & H2MI_KEYGEN_VK_ONLY) != 0;
  pk.by_coset = !pk.vk_only && (args.flags & H2MI_KEYGEN_BY_COSET) != 0;
  pk.logup = pk.table_logup || (args.lookups && (args.flags & H2MI_KEYGEN_LOGUP) != 0);
  if (args.gates) {
    pk.check_gates = pk.gate_program;
  } else {  // a hard-wired shape: its gates as the program the witness check interprets
    uint32_t n_ops = 0, n_constants = 0;
    pk.shape_ops.resize(H2MI_SHAPE_PROGRAM_MAX_OPS);
    if (h2mi_shape_gate_program(&cs, pk.shape_ops.data(), H2MI_SHAPE_PROGRAM_MAX_OPS, &n_ops, nullptr, 0, &n_constants)) throw Error(H2MI_EINVAL, "shape program");
    pk.shape_ops.resize(n_ops);
    pk.check_gates = {pk.shape_ops.data(), n_ops, nullptr, 0};
  }
  const poly::EvaluationDomain& dom = pk.domain;
  const size_t n = pk.n;
  const uint32_t u = pk.u, m = cs.n_perm;
  {
    uint64_t base_n = 0;
    check(h2mi_bases_info(args.g_lagrange_handle, nullptr, nullptr, nullptr, &base_n), "g_lagrange handle");
    if (base_n < n) throw Error(H2MI_ERANGE, "keygen: the Lagrange SRS is shorter than 2^k");
  }
  PatchList pl;
  // fixed columns as synthesize() assigns them.  keygen's Assembly refuses a fixed cell or a copy constraint outside the usable rows
  // (Error::NotEnoughRowsAvailable [RECALL plonk/keygen.rs assign_fixed / copy]): the permutation argument's product does not run over
  // the blinding rows, so a cycle through one would not be enforced and the proof would not verify
  for (uint32_t c = 0; c < cs.n_fixed; c++) {
    Dev d = vec(n);
    fill_column(*d, n, args.fixed[c], u, pl);
    pk.fixed_values.push_back(std::move(d));
  }
  pl.flush();
  // sigma_j[i] = DELTA^(j') omega^(i') for (j', i') = mapping[(j, i)]  (permutation/keygen.rs build_vk / build_pk)
  PermutationAssembly asm_;
  for (size_t i = 0; i < args.n_copies; i++) {
    const uint32_t* c = args.copies + 4 * i;
    if (c[0] >= m || c[2] >= m) throw Error(H2MI_EINVAL, "copy constraint on a column without equality enabled");
    if (c[1] >= u || c[3] >= u) throw Error(H2MI_ERANGE, "copy constraint beyond the usable rows (NotEnoughRowsAvailable)");
    asm_.copy(Cell(c[0], c[1]), Cell(c[2], c[3]));
  }
  if (m) {
    DeviceVec omega_pows(n);
    check(h2mi_fr_powers_dev(omega_pows.p, n, dom.get_omega().l, nullptr), "powers");
    std::vector<Fr> dpow(m, fr::ONE);
    for (uint32_t j = 1; j < m; j++) dpow[j] = fr::mul(dpow[j - 1], pk.delta);
    for (uint32_t j = 0; j < m; j++) {
      Dev d = vec(n);
      const void* ptrs[1] = {omega_pows.p};
      check(h2mi_fr_lincomb_dev(ptrs, dpow[j].l, 1, n, d->p, nullptr), "identity permutation");
      pk.sigma_values.push_back(std::move(d));
    }
    std::vector<uint32_t> pos;
    std::vector<std::array<uint32_t, 4>> moved;
    auto place = [&](uint32_t from_col, uint32_t from_row, uint32_t to_col, uint32_t to_row) {  // one moved cell, whichever front end names it
      pl.add(*pk.sigma_values[from_col], from_row, fr::mul(dpow[to_col], fr::pow_u64(dom.get_omega(), to_row)));
      if (from_row < u) pos.push_back((from_col / pk.chunk) * u + from_row);
      if (!pk.vk_only) moved.push_back({from_col, from_row, to_col, to_row});
    };
    if (extra.stored_moved) {
      for (const std::array<uint32_t, 4>& mv : *extra.stored_moved) place(mv[0], mv[1], mv[2], mv[3]);  // the parser has bounded every column and row
    } else {
      asm_.for_each([&](const Cell& from, const Cell& to) {
        if (!(from == to)) place(from.first, from.second, to.first, to.second);
      });
    }
    pl.flush();
    if (!moved.empty()) {  // what h2mi_prover_check compares: 16 bytes per moved cell, uploaded once
      std::sort(moved.begin(), moved.end());
      pk.moved_cells.resize(4 * moved.size());
      std::memcpy(pk.moved_cells.data(), moved.data(), 16 * moved.size());
      pk.moved_cells_dev = vec(moved.size() / 2 + 1);
      check(h2mi_memcpy_h2d(pk.moved_cells_dev->p, pk.moved_cells.data(), 16 * moved.size()), "moved cells");
    }
    check(h2mi_sync(), "sync");  // omega_pows is released below
    std::sort(pos.begin(), pos.end());
    pos.erase(std::unique(pos.begin(), pos.end()), pos.end());
    pk.n_active = (uint32_t)pos.size();
    pk.active_rows = vec(pos.size() / 8 + 1);
    if (!pos.empty()) check(h2mi_memcpy_h2d(pk.active_rows->p, pos.data(), pos.size() * 4), "active rows");
  }
  pk.fixed_commitments = commit_points(args.g_lagrange_handle, pk.fixed_values, n);
  pk.permutation_commitments = commit_points(args.g_lagrange_handle, pk.sigma_values, n);
  if (extra.stored_commitments) {  // a damaged cell section, or an SRS that is not the one the key was made against
    const bool same = (cs.n_fixed == 0 || !std::memcmp(pk.fixed_commitments.data(), extra.stored_commitments, 64 * (size_t)cs.n_fixed)) &&
                      (m == 0 || !std::memcmp(pk.permutation_commitments.data(), extra.stored_commitments + 64 * (size_t)cs.n_fixed, 64 * (size_t)m));
    if (!same) {
      h2mi_sync();  // nothing queued may still read the vectors released with the key
      throw Error(H2MI_EINVAL, "key file: the commitments recomputed from its cells are not the stored ones");
    }
  }
  if (pk.vk_only) return pkp;
  for (auto& col : pk.fixed_values) {
    Dev p = vec(n), e = pk.by_coset ? nullptr : vec(pk.ext);
    if (pk.by_coset) to_poly(dom, *col, *p);
    else to_poly_and_coset(dom, *col, *p, *e);
    pk.fixed_polys.push_back(std::move(p));
    if (!pk.by_coset) pk.fixed_cosets.push_back(std::move(e));
  }
  for (auto& col : pk.sigma_values) {
    Dev p = vec(n), e = pk.by_coset ? nullptr : vec(pk.ext);
    if (pk.by_coset) to_poly(dom, *col, *p);
    else to_poly_and_coset(dom, *col, *p, *e);
    pk.sigma_polys.push_back(std::move(p));
    if (!pk.by_coset) pk.sigma_cosets.push_back(std::move(e));
  }
  {  // l_0, l_last (row u), l_active = ones on the usable rows: extended-coset forms only (a by-coset key: coefficients only)
    Dev l0 = zeros(n), ll = zeros(n), la = vec(n), tmp = pk.by_coset ? nullptr : vec(n);
    pl.add(*l0, 0, fr::ONE);
    pl.add(*ll, u, fr::ONE);
    pl.flush();
    check(h2mi_fr_fill_dev(la->p, n, fr::ONE.l, nullptr), "fill");
    check(h2mi_memset_zero(at(*la, u), (n - u) * 32), "zero");
    if (pk.by_coset) {
      pk.l0_poly = vec(n);
      pk.l_last_poly = vec(n);
      pk.l_active_poly = vec(n);
      to_poly(dom, *l0, *pk.l0_poly);
      to_poly(dom, *ll, *pk.l_last_poly);
      to_poly(dom, *la, *pk.l_active_poly);
    } else {
      pk.l0 = vec(pk.ext);
      pk.l_last = vec(pk.ext);
      pk.l_active = vec(pk.ext);
      to_poly_and_coset(dom, *l0, *tmp, *pk.l0);
      to_poly_and_coset(dom, *ll, *tmp, *pk.l_last);
      to_poly_and_coset(dom, *la, *tmp, *pk.l_active);
    }
    check(h2mi_sync(), "sync");
  }
  // a lookup given as expressions has no keygen-time table: theta, or an advice column in it, is known only inside a proof
  for (uint32_t l = 0; !pk.lookup_exprs && !pk.table_logup && l < cs.n_lookups; l++) build_table(pk, pk.tables[l], args.fixed[cs.lookups[l].table_fixed]);
  // a table-logUp key: one sorted table (with its first rows) per distinct fixed column, whatever the number of arguments over it
  for (uint32_t a = 0; pk.table_logup && a < pk.cs.n_lookups; a++) {
    pk.tl_table[a] = a;
    for (uint32_t b = 0; b < a; b++)
      if (pk.cs.lookups[b].table_fixed == pk.cs.lookups[a].table_fixed) pk.tl_table[a] = std::min(pk.tl_table[a], pk.tl_table[b]);
    if (pk.tl_table[a] == a) build_table(pk, pk.tables[a], args.fixed[pk.cs.lookups[a].table_fixed], /*with_first=*/true);
  }
  return pkp;
}

// ---- ProverSHPLONK (poly/kzg/multiopen/shplonk.rs construct_intermediate_sets + shplonk/prover.rs) -----------------------------
struct ProverQuery {
  const DeviceVec* poly;
  Fr point, eval;
};
struct RotationSet {
  std::vector<Fr> points;                                              // ascending canonical value (BTreeSet<Fr>)
  std::vector<std::pair<const DeviceVec*, std::vector<Fr>>> members;  // (polynomial, evaluation at each point)
};
// coefficient lists (low to high) of the Lagrange basis polynomials of `pts`: the part of an interpolation that depends on the
// points alone — once per rotation set, with ONE inversion
std::vector<std::vector<Fr>> lagrange_basis(const std::vector<Fr>& pts) {
  const size_t m = pts.size();
  std::vector<std::vector<Fr>> nums;
  std::vector<Fr> dens;
  for (size_t j = 0; j < m; j++) {
    std::vector<Fr> num = {fr::ONE};
    Fr den = fr::ONE;
    for (size_t t = 0; t < m; t++) {
      if (t == j) continue;
      std::vector<Fr> nxt(num.size() + 1, fr_zero());
      for (size_t i = 0; i < num.size(); i++) {  // num *= (X - pts[t])
        nxt[i + 1] = fr::add(nxt[i + 1], num[i]);
        nxt[i] = fr::sub(nxt[i], fr::mul(num[i], pts[t]));
      }
      num = nxt;
      den = fr::mul(den, fr::sub(pts[j], pts[t]));
    }
    nums.push_back(num);
    dens.push_back(den);
  }
  const std::vector<Fr> inv = fr::batch_invert(dens);
  for (size_t j = 0; j < m; j++)
    for (Fr& c : nums[j]) c = fr::mul(c, inv[j]);
  return nums;
}
std::vector<Fr> interpolate(const std::vector<std::vector<Fr>>& basis, const std::vector<Fr>& evals) {
  std::vector<Fr> out(basis.size(), fr_zero());
  for (size_t j = 0; j < basis.size(); j++)
    for (size_t i = 0; i < basis[j].size(); i++) out[i] = fr::add(out[i], fr::mul(basis[j][i], evals[j]));
  return out;
}
Fr horner(const std::vector<Fr>& c, const Fr& x) {
  Fr acc = fr_zero();
  for (size_t i = c.size(); i-- > 0;) acc = fr::add(fr::mul(acc, x), c[i]);
  return acc;
}
Fr vanishing_at(const std::vector<Fr>& roots, const Fr& z) {
  Fr acc = fr::ONE;
  for (const Fr& r : roots) acc = fr::mul(acc, fr::sub(z, r));
  return acc;
}
bool contains(const std::vector<Fr>& v, const Fr& x) { return std::find(v.begin(), v.end(), x) != v.end(); }
// out = sum_k scalars[k] polys[k]; beyond one launch's 24 operands the sum continues in place (out re-enters with weight one: the
// kernel reads and writes row i in one thread, and every partial sum is the canonical value, so the split changes no bit)
void lincomb(const std::vector<const DeviceVec*>& polys, const std::vector<Fr>& scalars, size_t n, DeviceVec& out, h2mi_stream_t stream = nullptr) {
  constexpr size_t MAX = 24;
  for (size_t k0 = 0; k0 < polys.size();) {
    std::vector<const void*> ptrs;
    std::vector<Fr> sc;
    if (k0) {
      ptrs.push_back(out.p);
      sc.push_back(fr::ONE);
    }
    while (k0 < polys.size() && ptrs.size() < MAX) {
      ptrs.push_back(polys[k0]->p);
      sc.push_back(scalars[k0]);
      k0++;
    }
    check(h2mi_fr_lincomb_dev(ptrs.data(), (const uint64_t*)sc.data(), ptrs.size(), n, out.p, stream), "lincomb");
  }
}
void add_head(DeviceVec& poly, const std::vector<Fr>& head, h2mi_stream_t stream = nullptr) {
  // the entry takes at most 16 coefficients per call (they travel as kernel arguments): a rotation set of more points goes in slices
  for (size_t at = 0; at < head.size(); at += 16)
    check(h2mi_fr_add_head_dev((char*)poly.p + 32 * at, (const uint64_t*)(head.data() + at), std::min<size_t>(16, head.size() - at), stream), "add_head");
}
// out = src / prod (X - root); `out` must have been zeroed (the quotient has n - #roots coefficients, the rest stay zero).
// Two to four roots: ONE round of independent divisions weighted by the partial-fraction coefficients; otherwise a chain through
// tmp / tmp2.
void kate_chain(DeviceVec& src, size_t n, const std::vector<Fr>& roots, DeviceVec& tmp, DeviceVec& out, h2mi_stream_t stream, DeviceVec* tmp2) {
  if (roots.size() >= 2 && roots.size() <= 4) {
    std::vector<Fr> both(roots);  // the roots and the partial-fraction denominators, inverted together
    for (size_t i = 0; i < roots.size(); i++) {
      Fr d = fr::ONE;
      for (size_t k = 0; k < roots.size(); k++)
        if (k != i) d = fr::mul(d, fr::sub(roots[i], roots[k]));
      both.push_back(d);
    }
    both = fr::batch_invert(both);
    const std::vector<Fr> inv(both.begin(), both.begin() + roots.size()), w(both.begin() + roots.size(), both.end());
    check(h2mi_fr_kate_division_multi_dev(src.p, n, (const uint64_t*)roots.data(), (const uint64_t*)inv.data(), (const uint64_t*)w.data(), roots.size(),
                                          out.p, stream),
          "kate_division_multi");
    return;
  }
  DeviceVec* cur = &src;
  DeviceVec* bufs[2] = {&tmp, tmp2 ? tmp2 : &src};
  size_t len = n;
  for (size_t i = 0; i < roots.size(); i++) {
    DeviceVec* dst = i + 1 == roots.size() ? &out : bufs[i % 2];
    Fr binv = fr::invert(roots[i]);
    check(h2mi_fr_kate_division_dev(cur->p, len, roots[i].l, binv.l, dst->p, stream), "kate_division");
    cur = dst;
    len--;
  }
}

struct Forms {  // a column of the proof in Lagrange, coefficient and extended-coset form
  Dev value, poly, coset;
  void alloc(size_t n, size_t ext) {
    value = vec(n);
    poly = vec(n);
    coset = vec(ext);
  }
};

// ADVICE: every advice phase is committed; ADVICE_PHASES: some are (h2mi_prover_s::advice_done of them)
enum Phase { IDLE = 0, ADVICE, LOOKUPS, PRODUCTS, QUOTIENT, EVALUATIONS, SHPLONK_Q, ADVICE_PHASES };

}  // namespace

struct h2mi_batch_s;

struct h2mi_prover_s {
  h2mi_pk_s* pk;
  uint64_t g, gl;
  size_t lo, cnt;
  // several circuits per proof: the batch this prover is bound into and its place there.  Member 0 leads: the proof's one random
  // polynomial, h, the evaluations and SHPLONK's vectors, the result slots and the combiner of the joint phases are its own
  h2mi_batch_s* batch = nullptr;
  uint32_t batch_index = 0;
  // sliced SRS
  void *d_partial = nullptr, *d_combined = nullptr;
  h2mi_combine_fn combine = nullptr;
  void* combine_ctx = nullptr;
  // buffers
  std::vector<Forms> advice, z;
  // the instance columns (cs.n_instance of each): rows, extended coset, and — allocated when a column first holds more than 16 values
  // and takes the transform route — coefficients
  std::vector<Dev> instance, instance_poly, instance_coset;
  // a by-coset key: every `coset` vector of this prover is ONE slice of 2^k elements, filled per slice by the quotient phase, and the
  // slices of the key's shared columns live here — a batch reads its leader's (`lead`, set by the quotient phase; else this prover)
  std::vector<Dev> fixed_slices, sigma_slices;
  Dev l0_slice, l_last_slice, l_active_slice;
  const h2mi_prover_s* lead = nullptr;
  // h2mi_prover_instances: the public inputs of the NEXT proof, per column, Montgomery; consumed (or dropped) by its phase-0 call
  std::vector<std::vector<Fr>> pending_instances;
  bool have_pending_instances = false;
  // both sides of an argument given as expressions, compressed with theta: on the rows, and the same on the extended coset
  struct Sides {
    Dev input, table, in_coset, tab_coset;
  };
  struct Lk {
    // lookups given as expressions: both sides compressed (a logUp lookup's input sets behind one another), and the table's distinct
    // values are sorted inside the proof.  The single-column form holds selector * column rows in c.input and nothing else; without
    // a selector the advice column itself is the input
    Sides c;
    Forms a, s, z;
    Table sorted;
    // a table-logUp key: every input's rank in the key's sorted table (u32 x inputs x 2^k) and the joint histogram (u32 x n_unique),
    // written by the lookups phase and gathered by the products phase
    Dev ranks, counts;
  } lk[H2MI_MAX_LOOKUPS];
  // a table-logUp key: per argument with several inputs ONE vector that holds their advice columns' extended cosets behind one another
  // (the `coset` of those columns is a window into it), so that the quotient reads the inputs where the transforms put them
  std::vector<Dev> coset_blocks;
  // shuffle arguments: both sides compressed, the product in its three forms
  struct Sf {
    Sides c;
    Forms z;
  } sf[H2MI_MAX_SHUFFLES];
  // h2mi_prover_check's own scratch, allocated by its first call: a lookup's input and table rows, the table's sorted distinct values
  // (a shuffle: both sides' rows, and the distinct values of both)
  Dev check_in, check_tab;
  Table check_sorted, check_sorted_in;
  Fr theta;
  bool have_theta = false;  // a key with shuffles: h2mi_prover_lookups has delivered theta for this proof
  // the circuit's challenges (h2mi_prover_set_challenges): read by the lookups' compression and by the quotient
  std::vector<Fr> challenges;
  bool have_challenges = false;
  uint32_t advice_done = 0;
  Dev random_poly, h, h_poly, points, evals;
  // SHPLONK: three lanes (the library stream and two side streams), each with its own scratch
  Dev nx[3], tmp[3], h_x, l_x, h2_x;
  std::vector<Dev> q, s;
  h2mi_stream_t lane[2] = {nullptr, nullptr}, side = nullptr;
  // state of the proof in flight
  Phase phase = IDLE;
  // blinding source: counter-based SplitMix64 streams of `seed` (reproducible; tests, benchmarks, the goldens), or — once a key is
  // set — ChaCha20 blocks under a 256-bit key, one block per scalar as Fr::random draws them, `seed` the per-proof nonce
  bool keyed = false;
  uint8_t key[32] = {0};
  uint64_t seed = 0;
  bool advice_sparse = true;
  Fr beta, gamma;
  std::vector<ProverQuery> queries;
  size_t n_written = 0;
  std::vector<RotationSet> sets;
  std::vector<Fr> super_points;
  std::vector<std::vector<Fr>> remainders;
  Fr v;

  ~h2mi_prover_s() {
    for (h2mi_stream_t st : {lane[0], lane[1], side})
      if (st) h2mi_stream_destroy(st);
  }
  // the key's shared columns as the quotient reads them: the key's extended cosets, or the leader's slices
  const h2mi_prover_s& shared() const { return lead ? *lead : *this; }
  const void* fixed_coset(uint32_t j) const { return pk->by_coset ? shared().fixed_slices[j]->p : pk->fixed_cosets[j]->p; }
  const void* sigma_coset(uint32_t j) const { return pk->by_coset ? shared().sigma_slices[j]->p : pk->sigma_cosets[j]->p; }
  const void* l0_coset() const { return pk->by_coset ? shared().l0_slice->p : pk->l0->p; }
  const void* l_last_coset() const { return pk->by_coset ? shared().l_last_slice->p : pk->l_last->p; }
  const void* l_active_coset() const { return pk->by_coset ? shared().l_active_slice->p : pk->l_active->p; }
  // the length of a `coset` vector: the extended domain, or one slice of it
  size_t coset_len() const { return pk->by_coset ? pk->n : pk->ext; }
  const DeviceVec& lookup_input(uint32_t l) const {
    if (pk->lookup_exprs) return *lk[l].c.input;
    const h2mi_lookup& d = pk->cs.lookups[l];
    return d.selector_fixed >= 0 ? *lk[l].c.input : *advice[d.input.index].value;
  }
  const DeviceVec& lookup_table(uint32_t l) const { return pk->lookup_exprs ? *lk[l].c.table : *pk->fixed_values[pk->cs.lookups[l].table_fixed]; }
  // one side of lookup l compressed with theta, on the rows (coset = false) or on the extended coset
  // (`at`: the element of `out` the vector starts at — the input sets of a logUp lookup lie behind one another)
  void compress(const h2mi_gate_program& prog, bool coset, DeviceVec& out, const Fr* th = nullptr, size_t at = 0) const {
    const h2mi_constraint_system& cs = pk->cs;
    const void *adv[H2MI_MAX_ADVICE], *fix[H2MI_MAX_FIXED];
    for (uint32_t j = 0; j < cs.n_advice; j++) adv[j] = coset ? advice[j].coset->p : advice[j].value->p;
    for (uint32_t j = 0; j < cs.n_fixed; j++) fix[j] = coset ? fixed_coset(j) : pk->fixed_values[j]->p;
    const h2mi_instance_cosets inst = instance_columns(coset);
    const h2mi_expr_columns cols = {adv, cs.n_advice, fix, cs.n_fixed, &inst, &prog, challenge_limbs(), pk->phases.n_challenges, cs.k};
    check(h2mi_plonk_expr_compress_dev(&cols, coset && !pk->by_coset ? pk->domain.extended_k() : cs.k, (th ? *th : theta).l, (char*)out.p + at * 32,
                                       nullptr),
          "expr_compress");
  }
  // every instance column on the rows (coset = false) or on the extended coset, as the interpreting kernels take them
  h2mi_instance_cosets instance_columns(bool coset) const {
    h2mi_instance_cosets ic;
    std::memset(&ic, 0, sizeof(ic));
    ic.n_instance = pk->cs.n_instance;
    for (uint32_t i = 0; i < ic.n_instance; i++) ic.column[i] = coset ? instance_coset[i]->p : instance[i]->p;
    return ic;
  }
  // both sides of argument i of `sl` (a lookup given as expressions, a shuffle) on the rows or on the extended coset: input set j
  // lands one domain's length behind set j - 1 in `in`, the table (shuffle) side in `tab`
  void compress_sides(const ArgumentSlices& sl, uint32_t i, bool coset, DeviceVec& in, DeviceVec& tab, const Fr* th = nullptr) const {
    for (uint32_t j = 0; j < sl.sets[i]; j++) compress(sl.input[i][j], coset, in, th, j * (coset ? coset_len() : pk->n));
    compress(sl.table[i], coset, tab, th);
  }
  // a permutation column on the rows (coset = false) or on the extended coset
  const void* perm_column(const h2mi_column& c, bool coset) const {
    if (c.kind == H2MI_COL_ADVICE) return coset ? advice[c.index].coset->p : advice[c.index].value->p;
    if (c.kind == H2MI_COL_INSTANCE) return coset ? instance_coset[c.index]->p : instance[c.index]->p;
    return coset ? fixed_coset(c.index) : pk->fixed_values[c.index]->p;
  }
  const uint64_t* challenge_limbs() const { return pk->phases.n_challenges ? (const uint64_t*)challenges.data() : nullptr; }
  // a key with challenges: the phases behind the advice need their values
  void require_challenges() {
    if (pk->phases.n_challenges && !have_challenges) {
      phase = IDLE;
      throw Error(H2MI_EINVAL, "h2mi_prover_set_challenges has not been called");
    }
  }
  void* out_slot(size_t slot) const { return (char*)(d_partial ? d_partial : points->p) + 96 * slot; }
  const void* col(const DeviceVec& d, size_t offset_elems = 0) const { return (const char*)d.p + (offset_elems + lo) * 32; }

  void commit(bool lagrange, const void* column, size_t slot) {
    check(h2mi_msm_bn254_g1_dev(lagrange ? gl : g, column, cnt, out_slot(slot), nullptr), "commit");
  }
  // the commitments of one phase into slots slot0 ..: ONE call, so that small circuits get one set of launches for all of them.
  // sparse: the columns are mostly zeros or one repeated value; inorder: the group is everything its phase commits and is read back next
  void commit_phase(bool lagrange, const std::vector<const void*>& cols, size_t slot0, bool sparse, bool inorder) {
    const unsigned flags = (sparse ? H2MI_MSM_SPARSE : 0u) | (inorder ? H2MI_MSM_INORDER : 0u);
    check(h2mi_msm_bn254_g1_phase_dev(lagrange ? gl : g, cols.data(), cols.size(), cnt, out_slot(slot0), flags, nullptr), "commit");
  }
  // fetch the k Jacobian results of a phase (the copy joins the MSM pipeline; sliced SRS: the caller's all-gather + fold first),
  // G1::batch_normalize on the host (microseconds for a handful of points; a lone device thread takes 0.3 ms)
  void read_points(size_t k, uint64_t* out) {
    if (!k) return;
    if (!out) throw Error(H2MI_EINVAL, "points_out");
    std::vector<G1> jac(k);
    if (d_partial) {
      check(h2mi_join(), "join");
      if (combine(combine_ctx, k)) throw Error(H2MI_EHIP, "the combiner failed");
      check(h2mi_memcpy_d2h(jac.data(), d_combined, k * 96), "d2h");
    } else {
      check(h2mi_memcpy_d2h(jac.data(), points->p, k * 96), "d2h");
    }
    const std::vector<G1Affine> aff = normalize_host_batch(jac);
    std::memcpy(out, aff.data(), k * 64);
  }
  void forms(Forms& f, h2mi_stream_t stream) {
    if (pk->by_coset) to_poly(pk->domain, *f.value, *f.poly, stream);  // its slices are the quotient phase's
    else to_poly_and_coset(pk->domain, *f.value, *f.poly, *f.coset, stream);
  }
  // `count` blinding scalars for purpose 1 .. 6 (advice rows, permutation products, the random polynomial, permuted lookup columns,
  // lookup products, shuffle products): the streams seed + purpose of the seeded generator, or ChaCha20 stream id (nonce << 3 | purpose) under the key
  std::vector<Fr> blinding(uint32_t purpose, size_t count) const {
    return keyed ? chacha_fr(key, (seed << 3) | purpose, count) : uniform_fr(seed + purpose, count);
  }
  // one random polynomial per proof: a bound member behind the first neither draws nor commits one
  bool draws_random() const { return !batch || batch_index == 0; }
  void random_vector(uint32_t purpose, DeviceVec& out, size_t count) const {
    if (keyed) check(h2mi_fr_random_chacha_dev(out.p, count, key, (seed << 3) | purpose, 0, nullptr), "random_poly");
    else check(h2mi_fr_random_dev(out.p, count, seed + purpose, 0, nullptr), "random_poly");
  }
};

// N provers over one key whose circuits go into ONE proof (h2mi_batch_create).  The per-circuit phases stay on the members; the joint
// phases run over `members` in order with members[0] leading, and their phase state is the leader's (PRODUCTS -> QUOTIENT ->
// EVALUATIONS -> SHPLONK_Q -> IDLE) while the others wait in PRODUCTS
struct h2mi_batch_s {
  std::vector<h2mi_prover_s*> members;
};

namespace {

// the circuits of one proof, in order; [0] leads.  A prover outside a batch is the list of length one
typedef std::vector<h2mi_prover_s*> Circuits;

// commitments of the largest phase: the result slots a prover (and a combiner's two buffers) must hold
uint32_t max_phase_points(const h2mi_pk_s& pk) {
  const h2mi_constraint_system& cs = pk.cs;
  return std::max({cs.n_advice, (pk.logup ? 1 : 2) * cs.n_lookups, pk.n_sets + cs.n_lookups + pk.n_shuffles + 1, cs.degree - 1, 8u});
}

size_t gwc_num_points(const h2mi_pk_s& pk);  // the commitments of a GWC tail (below, with the phase)

std::unique_ptr<h2mi_prover_s> create_prover(h2mi_pk_s* pk, uint64_t g, uint64_t gl, size_t lo, size_t cnt) {
  if (pk->vk_only) throw Error(H2MI_EINVAL, "prover_create: the key was built with H2MI_KEYGEN_VK_ONLY");
  if (cnt == 0 || lo + cnt > pk->n) throw Error(H2MI_ERANGE, "prover_create: base slice");
  for (uint64_t h : {g, gl}) {
    uint64_t base_n = 0;
    check(h2mi_bases_info(h, nullptr, nullptr, nullptr, &base_n), "bases handle");
    if (base_n < cnt) throw Error(H2MI_ERANGE, "prover_create: base set shorter than the slice");
  }
  std::unique_ptr<h2mi_prover_s> pp(new h2mi_prover_s);
  h2mi_prover_s& p = *pp;
  p.pk = pk;
  p.g = g;
  p.gl = gl;
  p.lo = lo;
  p.cnt = cnt;
  const h2mi_constraint_system& cs = pk->cs;
  const size_t n = pk->n, ext = pk->by_coset ? pk->n : pk->ext;  // a by-coset key: every `coset` vector is one slice
  p.advice.resize(cs.n_advice);
  for (uint32_t a = 0; pk->table_logup && a < cs.n_lookups; a++) {
    const uint32_t K = pk->tl_sets[a];
    if (K == 1) continue;
    p.coset_blocks.push_back(vec(K * ext));
    for (uint32_t j = 0; j < K; j++) {  // each such column is an input of one merged argument only (h2mi_table_logup_check)
      Forms& f = p.advice[pk->tl_inputs[a][j].input.index];
      f.value = vec(n);
      f.poly = vec(n);
      f.coset = Dev(new DeviceVec(*p.coset_blocks.back(), j * ext, ext));
    }
  }
  for (Forms& f : p.advice)
    if (!f.value) f.alloc(n, ext);
  p.z.resize(pk->n_sets);
  for (Forms& f : p.z) f.alloc(n, ext);
  p.instance_poly.resize(cs.n_instance);
  for (uint32_t i = 0; i < cs.n_instance; i++) {
    p.instance.push_back(vec(n));
    p.instance_coset.push_back(vec(ext));
    if (pk->by_coset) p.instance_poly[i] = vec(n);  // always the coefficient route
  }
  if (pk->by_coset) {
    for (uint32_t j = 0; j < cs.n_fixed; j++) p.fixed_slices.push_back(vec(n));
    for (uint32_t j = 0; j < cs.n_perm; j++) p.sigma_slices.push_back(vec(n));
    p.l0_slice = vec(n);
    p.l_last_slice = vec(n);
    p.l_active_slice = vec(n);
  }
  for (uint32_t l = 0; l < cs.n_lookups; l++) {
    if (pk->lookup_exprs) {
      const size_t sets = pk->lookup_slices.sets[l];  // a logUp lookup's input sets, contiguous: one unless the key was made with an h2mi_logup_inputs
      p.lk[l].c = {vec(sets * n), vec(n), vec(sets * ext), vec(ext)};
      p.lk[l].sorted.alloc(pk->u);
    } else if (cs.lookups[l].selector_fixed >= 0) {
      p.lk[l].c.input = vec(n);
    }
    if (pk->table_logup) {
      p.lk[l].ranks = vec(pk->tl_sets[l] * n / 8 + (pk->tl_sets[l] * n % 8 ? 1 : 0));
      p.lk[l].counts = vec(pk->tables[pk->tl_table[l]].n_unique / 8 + 1);
    }
    p.lk[l].a.alloc(n, ext);
    if (!pk->logup) p.lk[l].s.alloc(n, ext);  // a logUp key: `a` holds M, `z` the running sum, there is no permuted table
    p.lk[l].z.alloc(n, ext);
  }
  for (uint32_t i = 0; i < pk->n_shuffles; i++) {
    p.sf[i].c = {vec(n), vec(n), vec(ext), vec(ext)};
    p.sf[i].z.alloc(n, ext);
  }
  p.random_poly = vec(n);
  p.h = vec(pk->ext);
  p.h_poly = vec(n);
  p.points = vec(3 * std::max<size_t>(max_phase_points(*pk), gwc_num_points(*pk)));  // 96 B per commitment of the largest phase (GWC's tail included)
  for (int i = 0; i < 3; i++) {
    p.nx[i] = vec(n);
    p.tmp[i] = vec(n);
  }
  p.h_x = vec(n);
  p.l_x = vec(n);
  p.h2_x = vec(n);
  for (int i = 0; i < 2; i++) check(h2mi_stream_create(&p.lane[i]), "stream_create");
  check(h2mi_stream_create(&p.side), "stream_create");
  return pp;
}

// theta as the caller delivers it
Fr take_theta(const uint64_t* theta, const char* refusal = "theta") {
  if (!theta) throw Error(H2MI_EINVAL, refusal);
  Fr th;
  std::memcpy(th.l, theta, 32);
  return th;
}

void require_phase(h2mi_prover_s& p, Phase want) {
  if (p.phase != want) {
    p.phase = IDLE;
    throw Error(H2MI_EINVAL, "prover phases out of order");
  }
}

// ---- phase 1: advice columns, one call per advice phase [RECALL halo2_proofs v2023_02_02 plonk/prover.rs create_proof: per phase
// synthesize, keep that phase's columns, blind and commit them in column order, write the points, squeeze that phase's challenges] ----
void phase_advice(h2mi_prover_s& p, uint32_t ph, const h2mi_column_cells* advice, const uint64_t* instance, size_t n_inst, uint64_t seed,
                  uint64_t* points_out) {
  const h2mi_pk_s& pk = *p.pk;
  const h2mi_constraint_system& cs = pk.cs;
  const h2mi_advice_phases& phases = pk.phases;
  const size_t n = pk.n;
  const uint32_t bf = cs.blinding_factors, u = pk.u, na = cs.n_advice;
  const Phase was = p.phase;
  p.phase = IDLE;  // whatever is refused below abandons the proof
  // the public inputs of this proof, per instance column: what h2mi_prover_instances left (it holds for this proof only, taken or
  // refused), or column 0 through the older arguments
  std::vector<std::vector<Fr>> inst;
  const bool by_columns = ph == 0 && p.have_pending_instances;
  if (ph == 0) {
    inst.swap(p.pending_instances);
    p.have_pending_instances = false;
  }
  check_cells(advice, na, H2MI_CELLS_FOR_ADVICE);
  if (ph >= phases.n_phases) throw Error(H2MI_EINVAL, "advice phase beyond the key's");
  if (ph > 0 && (was != ADVICE_PHASES || p.advice_done != ph)) throw Error(H2MI_EINVAL, "advice phases out of order");
  for (uint32_t j = 0; j < na; j++)
    if (phases.advice_phase[j] != ph && advice[j].count) throw Error(H2MI_EINVAL, "cells for an advice column of another phase");
  PatchList pl;
  if (ph == 0) {  // a new proof: the seed and the public inputs
    if (seed >> (p.keyed ? 61 : 32)) throw Error(H2MI_EINVAL, p.keyed ? "nonce must be below 2^61" : "seed must be below 2^32");
    if (n_inst && (!cs.n_instance || !instance)) throw Error(H2MI_EINVAL, "public inputs without an instance column");
    if (n_inst && cs.n_instance > 1) throw Error(H2MI_EINVAL, "several instance columns: the public inputs go through h2mi_prover_instances");
    if (n_inst && by_columns) throw Error(H2MI_EINVAL, "public inputs both through h2mi_prover_instances and through the advice call");
    if (n_inst > u) throw Error(H2MI_ERANGE, "more public inputs than usable rows");
    p.seed = seed;
    p.have_challenges = false;
    p.have_theta = false;
    inst.resize(cs.n_instance);
    if (n_inst) {
      inst[0].resize(n_inst);
      std::memcpy(inst[0].data(), instance, n_inst * 32);
    }
    for (uint32_t i = 0; i < cs.n_instance; i++) {
      h2mi_column_cells ic = {nullptr, (const uint64_t*)inst[i].data(), inst[i].size(), 0};
      fill_column(*p.instance[i], n, ic, u, pl);
    }
  }
  // witness cells + blinding rows.  Assigned cells and blinding rows of every column travel in ONE launch's arguments when the
  // columns are short (h2mi_fr_patch_cells_dev) instead of a dozen 32-byte copies in front of the phase's commitments.  Column j's
  // blinding row r is scalar j (bf + 1) + r of the stream whatever the column's phase
  const std::vector<Fr> blind = p.blinding(1, (size_t)na * (bf + 1));
  size_t assigned = 0;
  std::vector<uint32_t> mine;  // this phase's columns, in column order
  for (uint32_t j = 0; j < na; j++) {
    if (phases.advice_phase[j] != ph) continue;
    mine.push_back(j);
    DeviceVec& colv = *p.advice[j].value;
    fill_column(colv, n, advice[j], u, pl);
    assigned = std::max(assigned, advice[j].count);
    for (uint32_t r = 0; r <= bf; r++) pl.add(colv, u + r, blind[(size_t)j * (bf + 1) + r]);
  }
  pl.flush();
  // the sparse promise (batched launches at every size) holds for the padded witness columns of the reference's circuits; a
  // column assigned on more than a quarter of its rows takes the pipelined loop.  Decided per phase from that phase's columns: a
  // later phase's running sums are typically dense where the first phase's columns are not
  p.advice_sparse = assigned * 4 <= n;
  {
    std::vector<const void*> cols;
    for (uint32_t j : mine) cols.push_back(p.col(*p.advice[j].value));
    p.commit_phase(true, cols, 0, p.advice_sparse, /*inorder=*/true);
  }
  check(h2mi_msm_flush(), "flush");  // the bucket reductions start now, not when the host reaches the join
  // The coefficient / extended forms of the advice and instance columns depend on no challenge (create_proof computes them after
  // y): on the side stream they run beside the transcript round trips, the caller's witness generation for the next advice phase,
  // the lookups' counting sorts and the grand products' chains of small scans instead of queueing behind the next phases' commitments
  check(h2mi_stream_wait(p.side, nullptr), "stream_wait");
  for (uint32_t j : mine) p.forms(p.advice[j], p.side);
  if (ph == 0 && cs.n_instance) {
    // a column of a handful of public inputs: sum_r v_r * (l_0's coset rotated by r rows), no transform — one column by the launch
    // it has always had, the short columns of a key with several in ONE launch; a longer column goes through the transforms
    const void* short_vals[H2MI_MAX_INSTANCE];
    size_t short_counts[H2MI_MAX_INSTANCE];
    void* short_out[H2MI_MAX_INSTANCE];
    uint32_t n_short = 0;
    for (uint32_t i = 0; i < cs.n_instance; i++) {
      if (pk.by_coset) {  // the shortcut reads an extended l_0: whatever its length the column goes through its coefficients
        to_poly(pk.domain, *p.instance[i], *p.instance_poly[i], p.side);
      } else if (inst[i].size() <= 16) {
        short_vals[n_short] = inst[i].data();
        short_counts[n_short] = inst[i].size();
        short_out[n_short++] = p.instance_coset[i]->p;
      } else {
        if (!p.instance_poly[i]) p.instance_poly[i] = vec(n);
        to_poly_and_coset(pk.domain, *p.instance[i], *p.instance_poly[i], *p.instance_coset[i], p.side);
      }
    }
    if (cs.n_instance == 1 && n_short)
      check(h2mi_plonk_instance_coset_dev(pk.l0->p, cs.k, pk.domain.extended_k(), (const uint64_t*)short_vals[0], short_counts[0], short_out[0], p.side),
            "instance coset");
    else if (n_short)
      check(h2mi_plonk_instance_coset_multi_dev(pk.l0->p, cs.k, pk.domain.extended_k(), (const uint64_t* const*)short_vals, short_counts, n_short, short_out,
                                                p.side),
            "instance coset");
  }
  p.read_points(mine.size(), points_out);
  p.advice_done = ph + 1;
  p.phase = p.advice_done == phases.n_phases ? ADVICE : ADVICE_PHASES;
}

// ---- phase 2: lookups' permuted columns (plonk/lookup/prover.rs commit_permuted) -----------------------------------------------
void phase_lookups(h2mi_prover_s& p, const uint64_t* theta, uint64_t* points_out) {
  const h2mi_pk_s& pk = *p.pk;
  const h2mi_constraint_system& cs = pk.cs;
  const size_t n = pk.n;
  const uint32_t bf = cs.blinding_factors, u = pk.u, L = cs.n_lookups;
  require_phase(p, ADVICE);
  p.require_challenges();
  p.phase = IDLE;
  if (pk.n_shuffles) {  // the shuffles are compressed with theta in the products phase: this call carries it, lookups or none
    p.theta = take_theta(theta);
    p.have_theta = true;
  }
  if (L && pk.table_logup) {
    // logUp against the key's sorted tables [DESIGN.md 4.5]: nothing is compressed and nothing sorted — per argument ONE ranking launch
    // over its input columns where they lie (ranks and the joint histogram stay for the products phase), M scattered by the table's first
    // rows.  Blinding rows and commitments: the program route's below, word for word
    const std::vector<Fr> mb = p.blinding(4, (size_t)(bf + 1) * L);
    PatchList pl;
    std::vector<const void*> cols;
    for (uint32_t a = 0; a < L; a++) {
      const void* inputs[H2MI_MAX_LOGUP_INPUTS];
      for (uint32_t j = 0; j < pk.tl_sets[a]; j++) {
        const h2mi_lookup& d = pk.tl_inputs[a][j];
        inputs[j] = p.advice[d.input.index].value->p;
        if (d.selector_fixed >= 0) {  // q_lookup * a: an argument of one input (h2mi_table_logup_check)
          check(h2mi_fr_mul_dev(pk.fixed_values[d.selector_fixed]->p, inputs[j], n, p.lk[a].c.input->p, nullptr), "lookup input");
          inputs[j] = p.lk[a].c.input->p;
        }
      }
      const Table& t = pk.tables[pk.tl_table[a]];
      DeviceVec& mult = *p.lk[a].a.value;
      uint64_t missing = 0;
      check(h2mi_plonk_logup_rank_cols_dev(inputs, pk.tl_sets[a], t.sorted->p, t.n_unique, t.first->p, cs.k, u, p.lk[a].ranks->p, p.lk[a].counts->p, mult.p,
                                           &missing, nullptr),
            "logup_rank_cols");
      if (missing) throw Error(H2MI_EUNSAT, "lookup input not in the table (ConstraintSystemFailure)");
      for (uint32_t r = 0; r <= bf; r++) pl.add(mult, u + r, mb[(size_t)(bf + 1) * a + r]);
      cols.push_back(p.col(mult));
    }
    pl.flush();
    p.commit_phase(true, cols, 0, /*sparse=*/false, /*inorder=*/true);
    check(h2mi_msm_flush(), "flush");
    check(h2mi_stream_wait(p.side, nullptr), "stream_wait");
    for (uint32_t a = 0; a < L; a++) p.forms(p.lk[a].a, p.side);
    p.read_points(L, points_out);
  } else if (L && pk.logup) {
    // logUp [restated in DESIGN.md 4.5]: compress -> multiplicities -> blinding rows -> one in-order commitment group of L columns.
    // M's blinding rows u .. 2^k - 1 come from the permuted columns' stream (purpose 4): bf + 1 scalars per lookup, in lookup order
    p.theta = take_theta(theta);
    const std::vector<Fr> mb = p.blinding(4, (size_t)(bf + 1) * L);
    PatchList pl;
    std::vector<const void*> cols;
    for (uint32_t l = 0; l < L; l++) {
      const h2mi_prover_s::Sides& c = p.lk[l].c;
      p.compress_sides(pk.lookup_slices, l, false, *c.input, *c.table);
      DeviceVec& mult = *p.lk[l].a.value;
      uint64_t missing = 0;
      check(h2mi_plonk_logup_multiplicity_sets_dev(c.input->p, pk.lookup_slices.sets[l], c.table->p, cs.k, u, mult.p, &missing, nullptr), "logup_multiplicity");
      if (missing) throw Error(H2MI_EUNSAT, "lookup input not in the table (ConstraintSystemFailure)");
      for (uint32_t r = 0; r <= bf; r++) pl.add(mult, u + r, mb[(size_t)(bf + 1) * l + r]);
      cols.push_back(p.col(mult));
    }
    pl.flush();
    p.commit_phase(true, cols, 0, /*sparse=*/false, /*inorder=*/true);
    check(h2mi_msm_flush(), "flush");
    check(h2mi_stream_wait(p.side, nullptr), "stream_wait");
    for (uint32_t l = 0; l < L; l++) p.forms(p.lk[l].a, p.side);
    p.read_points(L, points_out);
  } else if (L) {
    const std::vector<Fr> lb = p.blinding(4, (size_t)2 * (bf + 1) * L);
    PatchList pl;
    std::vector<const void*> cols;
    if (pk.lookup_exprs) p.theta = take_theta(theta);
    for (uint32_t l = 0; l < L; l++) {
      const h2mi_lookup& d = cs.lookups[l];
      if (pk.lookup_exprs) {
        // both sides compressed on all 2^k rows; the table's usable rows sorted here, inside the proof
        p.compress_sides(pk.lookup_slices, l, false, *p.lk[l].c.input, *p.lk[l].c.table);
        Table& ts = p.lk[l].sorted;
        check(h2mi_fr_sort_unique_dev(p.lk[l].c.table->p, u, ts.sorted->p, ts.sorted_mont->p, ts.mult->p, &ts.n_unique, nullptr), "sort_unique");
      } else if (d.selector_fixed >= 0) {  // the input expression's rows: q_lookup * a, zero wherever the selector is off
        check(h2mi_fr_mul_dev(pk.fixed_values[d.selector_fixed]->p, p.advice[d.input.index].value->p, n, p.lk[l].c.input->p, nullptr), "lookup input");
      }
      DeviceVec &a_perm = *p.lk[l].a.value, &s_perm = *p.lk[l].s.value;
      uint64_t missing = 0;
      const Table& t = pk.lookup_exprs ? p.lk[l].sorted : pk.tables[l];
      check(h2mi_plonk_lookup_permute_dev(p.lookup_input(l).p, t.sorted->p, t.sorted_mont->p, t.mult->p, t.n_unique, cs.k, u, a_perm.p, s_perm.p,
                                          &missing, nullptr),
            "lookup_permute");
      if (missing) throw Error(H2MI_EUNSAT, "lookup input not in the table (ConstraintSystemFailure)");
      const size_t o0 = (size_t)2 * (bf + 1) * l;
      for (uint32_t r = 0; r <= bf; r++) pl.add(a_perm, u + r, lb[o0 + r]);
      for (uint32_t r = 0; r <= bf; r++) pl.add(s_perm, u + r, lb[o0 + bf + 1 + r]);
      cols.push_back(p.col(a_perm));
      cols.push_back(p.col(s_perm));
    }
    pl.flush();
    p.commit_phase(true, cols, 0, /*sparse=*/false, /*inorder=*/true);  // the permuted pairs are all this phase commits
    check(h2mi_msm_flush(), "flush");
    check(h2mi_stream_wait(p.side, nullptr), "stream_wait");
    for (uint32_t l = 0; l < L; l++) {
      p.forms(p.lk[l].a, p.side);
      p.forms(p.lk[l].s, p.side);
    }
    p.read_points(2 * L, points_out);
  }
  p.phase = LOOKUPS;
}

// ---- the witness check between the advice and the lookups (h2mi_prover_check): gates, copies, lookups on the rows -----------------
// Reads the advice / instance / fixed columns behind the advice fill on the library stream, writes only scratch of its own, and
// leaves the phase state alone: the proof in flight goes on whatever it finds or refuses.
std::vector<h2mi_check_failure> run_check(h2mi_prover_s& p, const uint64_t* theta) {
  const h2mi_pk_s& pk = *p.pk;
  const h2mi_constraint_system& cs = pk.cs;
  const size_t n = pk.n;
  const uint32_t u = pk.u, L = cs.n_lookups, m = cs.n_perm;
  if (p.phase != ADVICE && p.phase != LOOKUPS) throw Error(H2MI_EINVAL, "check: between the last advice phase and the products");
  if (pk.phases.n_challenges && !p.have_challenges) throw Error(H2MI_EINVAL, "check: h2mi_prover_set_challenges has not been called");
  const Fr th = (L && pk.lookup_exprs) || pk.n_shuffles ? take_theta(theta, "check: theta") : fr_zero();
  std::vector<h2mi_check_failure> out;
  const void *adv[H2MI_MAX_ADVICE], *fix[H2MI_MAX_FIXED];
  for (uint32_t j = 0; j < cs.n_advice; j++) adv[j] = p.advice[j].value->p;
  for (uint32_t j = 0; j < cs.n_fixed; j++) fix[j] = pk.fixed_values[j]->p;
  {  // every gate polynomial on all 2^k rows of the blinded columns: the condition under which the quotient is a polynomial
    uint32_t n_polys = 0;
    for (uint32_t i = 0; i < pk.check_gates.n_ops; i++) n_polys += pk.check_gates.ops[i].op == H2MI_EXPR_END;
    std::vector<uint32_t> report(2 * (size_t)n_polys);
    const h2mi_instance_cosets inst = p.instance_columns(false);
    const h2mi_expr_columns cols = {adv, cs.n_advice, fix, cs.n_fixed, &inst, &pk.check_gates, p.challenge_limbs(), pk.phases.n_challenges, cs.k};
    check(h2mi_plonk_expr_check_dev(&cols, (uint32_t)n, report.data(), nullptr, nullptr), "expr_check");
    for (uint32_t j = 0; j < n_polys; j++)
      if (report[2 * j]) out.push_back({H2MI_CHECK_GATE, j, report[2 * j + 1], report[2 * j]});
  }
  if (m && !pk.moved_cells.empty()) {
    const void* vals[H2MI_MAX_PERM];
    for (uint32_t j = 0; j < m; j++) {
      const h2mi_column& c = cs.perm_columns[j];
      vals[j] = p.perm_column(c, false);
    }
    uint32_t report[2];
    check(h2mi_plonk_copy_check_dev(vals, m, pk.moved_cells_dev->p, (uint32_t)(pk.moved_cells.size() / 4), report, nullptr), "copy_check");
    if (report[0]) out.push_back({H2MI_CHECK_COPY, pk.moved_cells[4 * (size_t)report[1]], pk.moved_cells[4 * (size_t)report[1] + 1], report[0]});
  }
  // one input column against a table's sorted distinct values -> the lookup's entry grows by the absent rows and keeps the smallest
  auto member = [&](const void* input, const Table& t, uint32_t& absent, uint32_t& first_row) {
    uint32_t report[2];
    check(h2mi_plonk_lookup_member_dev(input, t.sorted->p, t.n_unique, u, report, nullptr), "lookup_member");
    absent += report[0];
    first_row = std::min(first_row, report[1]);
  };
  for (uint32_t l = 0; l < L; l++) {
    uint32_t absent = 0, first_row = 0xffffffffu;
    if (pk.lookup_exprs) {  // what the lookups phase does with the transcript's theta, on scratch of this call's own
      if (!p.check_in) {
        p.check_in = vec(n);
        p.check_tab = vec(n);
        p.check_sorted.alloc(u);
      }
      p.compress(pk.lookup_slices.table[l], false, *p.check_tab, &th);
      Table& ts = p.check_sorted;
      check(h2mi_fr_sort_unique_dev(p.check_tab->p, u, ts.sorted->p, ts.sorted_mont->p, ts.mult->p, &ts.n_unique, nullptr), "sort_unique");
      // every input set of a merged logUp lookup against the one sorted table: the entry counts the absent (row, set) pairs
      for (uint32_t j = 0; j < pk.lookup_slices.sets[l]; j++) {
        p.compress(pk.lookup_slices.input[l][j], false, *p.check_in, &th);
        member(p.check_in->p, ts, absent, first_row);
      }
    } else {
      // a table-logUp key: every input of the argument against its table, the entry counting the absent (row, input) pairs
      for (uint32_t j = 0; j < (pk.table_logup ? pk.tl_sets[l] : 1u); j++) {
        const h2mi_lookup& d = pk.table_logup ? pk.tl_inputs[l][j] : cs.lookups[l];
        const void* input = p.advice[d.input.index].value->p;
        if (d.selector_fixed >= 0) {
          if (!p.check_in) p.check_in = vec(n);
          check(h2mi_fr_mul_dev(pk.fixed_values[d.selector_fixed]->p, input, n, p.check_in->p, nullptr), "lookup input");
          input = p.check_in->p;
        }
        member(input, pk.tables[pk.table_logup ? pk.tl_table[l] : l], absent, first_row);
      }
    }
    if (absent) out.push_back({H2MI_CHECK_LOOKUP, l, first_row, absent});
  }
  for (uint32_t i = 0; i < pk.n_shuffles; i++) {  // both sides compressed and sorted; a row fails when its value is rarer on the other side
    if (!p.check_in) p.check_in = vec(n);
    if (!p.check_tab) p.check_tab = vec(n);
    for (Table* t : {&p.check_sorted, &p.check_sorted_in})
      if (!t->sorted) t->alloc(u);
    p.compress_sides(pk.shuffle_slices, i, false, *p.check_in, *p.check_tab, &th);
    Table &ti = p.check_sorted_in, &ts = p.check_sorted;
    check(h2mi_fr_sort_unique_dev(p.check_in->p, u, ti.sorted->p, ti.sorted_mont->p, ti.mult->p, &ti.n_unique, nullptr), "sort_unique");
    check(h2mi_fr_sort_unique_dev(p.check_tab->p, u, ts.sorted->p, ts.sorted_mont->p, ts.mult->p, &ts.n_unique, nullptr), "sort_unique");
    uint32_t report[2];
    check(h2mi_plonk_shuffle_member_dev(p.check_in->p, ti.sorted->p, ti.mult->p, ti.n_unique, ts.sorted->p, ts.mult->p, ts.n_unique, u, report, nullptr),
          "shuffle_member");
    if (report[0]) out.push_back({H2MI_CHECK_SHUFFLE, i, report[1], report[0]});
  }
  return out;
}

// ---- phase 3: grand products + the vanishing argument's random polynomial ----------------------------------------------------
void phase_products(h2mi_prover_s& p, const Fr& beta, const Fr& gamma, uint64_t* points_out) {
  const h2mi_pk_s& pk = *p.pk;
  const h2mi_constraint_system& cs = pk.cs;
  const size_t n = pk.n;
  const uint32_t bf = cs.blinding_factors, u = pk.u, L = cs.n_lookups, m = cs.n_perm, n_sets = pk.n_sets;
  const uint32_t S = pk.n_shuffles;
  if (p.phase == ADVICE && L == 0 && S == 0) p.phase = LOOKUPS;  // nothing to permute and no theta to deliver: the lookup phase may be skipped
  require_phase(p, LOOKUPS);
  p.require_challenges();
  p.phase = IDLE;
  p.beta = beta;
  p.gamma = gamma;
  // shuffle arguments [RECALL halo2_proofs (PSE line) plonk/shuffle/prover.rs, restated in DESIGN.md 4.5]: both sides compressed on
  // the rows, the product, its blinding rows.  In front of everything this phase queues: an unsatisfied shuffle (z[u] != 1) abandons
  // the proof with no commitment in flight.  Their commitments follow the lookups' below, in transcript order.
  if (S) {
    if (!p.have_theta) throw Error(H2MI_EINVAL, "a key with shuffles takes theta through h2mi_prover_lookups");
    const std::vector<Fr> szb = p.blinding(6, (size_t)bf * S);
    PatchList pl;
    for (uint32_t i = 0; i < S; i++) {
      h2mi_prover_s::Sf& sf = p.sf[i];
      p.compress_sides(pk.shuffle_slices, i, false, *sf.c.input, *sf.c.table);
      const int rc = h2mi_plonk_shuffle_product_dev(sf.c.input->p, sf.c.table->p, cs.k, u, gamma.l, sf.z.value->p, nullptr);
      if (rc == H2MI_EUNSAT) throw Error(H2MI_EUNSAT, "shuffle: the two sides are not the same multiset (ConstraintSystemFailure)");
      check(rc, "shuffle_product");
      pl.add_tail(*sf.z.value, u, bf, szb, i);
    }
    pl.flush();
  }
  // logUp running sums [restated in DESIGN.md 4.5], like the shuffles' products in front of everything this phase queues; their
  // blinding rows u + 1 .. 2^k - 1 come from the lookup products' stream (purpose 5): bf scalars per lookup, in lookup order
  if (L && pk.logup) {
    const std::vector<Fr> pb = p.blinding(5, (size_t)bf * L);
    PatchList pl;
    for (uint32_t l = 0; l < L; l++) {
      DeviceVec& phi = *p.lk[l].z.value;
      if (pk.table_logup) {  // by rank: one inversion per distinct table value, a gather per row
        const Table& t = pk.tables[pk.tl_table[l]];
        check(h2mi_plonk_logup_sum_ranked_dev(p.lk[l].ranks->p, pk.tl_sets[l], t.sorted_mont->p, p.lk[l].counts->p, t.first->p, t.n_unique, cs.k, u, beta.l,
                                              phi.p, nullptr),
              "logup_sum_ranked");
      } else {
        check(h2mi_plonk_logup_sum_sets_dev(p.lk[l].c.input->p, pk.lookup_slices.sets[l], p.lk[l].c.table->p, p.lk[l].a.value->p, cs.k, u, beta.l, phi.p, nullptr),
              "logup_sum");
      }
      pl.add_tail(phi, u, bf, pb, l);
    }
    pl.flush();
  }
  // the random polynomial's commitment is written after the grand products' but depends on nothing: queued first, the one dense
  // MSM of this phase accumulates beside their latency-bound scans.  Result slot: where the transcript expects it.
  const bool random = p.draws_random();
  if (random) {
    p.random_vector(3, *p.random_poly, n);
    p.commit(false, p.col(*p.random_poly), n_sets + L + S);
  }
  // permutation argument: every set in one device pass, over the copy constraints' support when that is sparse
  const bool perm_sparse = (uint64_t)pk.n_active * 8 <= (uint64_t)n_sets * u;
  if (m) {
    std::vector<const void*> vals, sigs;
    std::vector<void*> zptr;
    std::vector<Fr> bd;
    Fr dp = fr::ONE;
    for (uint32_t j = 0; j < m; j++) {
      vals.push_back(p.perm_column(cs.perm_columns[j], false));
      sigs.push_back(pk.sigma_values[j]->p);
      bd.push_back(fr::mul(beta, dp));
      dp = fr::mul(dp, pk.delta);
    }
    for (uint32_t s = 0; s < n_sets; s++) zptr.push_back(p.z[s].value->p);
    if (perm_sparse)
      check(h2mi_plonk_permutation_products_sparse_dev(vals.data(), sigs.data(), m, pk.chunk, cs.k, u, beta.l, gamma.l, (const uint64_t*)bd.data(),
                                                       pk.domain.get_omega().l, pk.active_rows->p, pk.n_active, zptr.data(), nullptr),
            "permutation_products");
    else
      check(h2mi_plonk_permutation_products_dev(vals.data(), sigs.data(), m, pk.chunk, cs.k, u, beta.l, gamma.l, (const uint64_t*)bd.data(),
                                                pk.domain.get_omega().l, zptr.data(), nullptr),
            "permutation_products");
    const std::vector<Fr> zblind = p.blinding(2, (size_t)n_sets * bf);
    PatchList pl;
    for (uint32_t s = 0; s < n_sets; s++) pl.add_tail(*p.z[s].value, u, bf, zblind, s);
    pl.flush();
  }
  std::vector<const void*> zcols;
  for (uint32_t s = 0; s < n_sets; s++) zcols.push_back(p.col(*p.z[s].value));
  if (cs.gates == H2MI_GATES_STANDARD_PLONK) {
    // StandardPlonk's schedule (measured in rounds 3-4 at 2^5 .. 2^20 rows): the products' forms queue BEHIND their commitments on
    // the library stream — on the side stream they ran beside the commitments' partition and bucket-reduction chain, whose latency
    // is what the phase waits for, and slowed it (2^16 rows: +0.2 ms)
    if (n_sets) p.commit_phase(true, zcols, 0, perm_sparse, false);
    check(h2mi_msm_flush(), "flush");
    for (uint32_t s = 0; s < n_sets; s++) p.forms(p.z[s], nullptr);
    check(h2mi_stream_wait(nullptr, p.side), "stream_wait");  // evaluate_h and the openings read the advice forms
    p.read_points(n_sets + (random ? 1 : 0), points_out);
  } else {
    // the halo2-lib shapes' schedule (measured at DEGREE 20 / 22): forms on the side stream, ordered behind the columns and AHEAD
    // of their commitments' partition kernels, which a dense accumulation in flight starves for milliseconds at DEGREE 22
    check(h2mi_stream_wait(p.side, nullptr), "stream_wait");
    for (uint32_t s = 0; s < n_sets; s++) p.forms(p.z[s], p.side);
    if (n_sets) p.commit_phase(true, zcols, 0, perm_sparse, false);
    size_t slot = n_sets;
    if (L && pk.logup) {
      for (uint32_t l = 0; l < L; l++) {  // built above; the commitment in the lookup product's slot, the forms on the side stream
        check(h2mi_stream_wait(p.side, nullptr), "stream_wait");
        p.forms(p.lk[l].z, p.side);
        p.commit(true, p.col(*p.lk[l].z.value), slot++);
      }
    } else if (L) {
      const std::vector<Fr> lzb = p.blinding(5, (size_t)bf * L);
      for (uint32_t l = 0; l < L; l++) {
        DeviceVec& lz = *p.lk[l].z.value;
        check(h2mi_plonk_lookup_product_dev(p.lookup_input(l).p, p.lookup_table(l).p, p.lk[l].a.value->p, p.lk[l].s.value->p, cs.k,
                                            u, beta.l, gamma.l, lz.p, nullptr),
              "lookup_product");
        PatchList pl;
        pl.add_tail(lz, u, bf, lzb, l);
        pl.flush();
        check(h2mi_stream_wait(p.side, nullptr), "stream_wait");
        p.forms(p.lk[l].z, p.side);
        p.commit(true, p.col(lz), slot++);
      }
    }
    for (uint32_t i = 0; i < S; i++) {
      check(h2mi_stream_wait(p.side, nullptr), "stream_wait");
      p.forms(p.sf[i].z, p.side);
      p.commit(true, p.col(*p.sf[i].z.value), slot++);
    }
    if (random) slot++;  // the random polynomial's commitment, queued before the grand products
    check(h2mi_msm_flush(), "flush");
    p.read_points(slot, points_out);
    // joined AFTER the read-back: the copy runs on the library stream, and a join in front of it made the transcript wait for every
    // transform of the side stream instead of the bucket reductions only
    check(h2mi_stream_wait(nullptr, p.side), "stream_wait");
  }
  p.phase = PRODUCTS;
}

// ---- phase 4: the quotient (plonk/evaluation.rs evaluate_h + vanishing division), its pieces committed ---------------------------
// every extended-coset vector of one circuit as the interpreting quotient kernels take them: the columns a program may query through
// one pointer table, the permutation argument, the lookups (given as expressions: compressed on the extended coset here)
void fill_expr_cosets(h2mi_prover_s& p, h2mi_expr_cosets& ec, h2mi_shuffle_cosets& sc, h2mi_logup_cosets& lg, h2mi_instance_cosets& ic) {
  const h2mi_pk_s& pk = *p.pk;
  const h2mi_constraint_system& cs = pk.cs;
  const uint32_t L = cs.n_lookups, m = cs.n_perm, n_sets = pk.n_sets;
  std::memset(&ec, 0, sizeof(ec));
  for (uint32_t j = 0; j < cs.n_advice; j++) ec.advice[j] = p.advice[j].coset->p;
  for (uint32_t j = 0; j < cs.n_fixed; j++) ec.fixed[j] = p.fixed_coset(j);
  ic = p.instance_columns(true);
  ec.instance = ic.column[0];  // what the calls without an h2mi_instance_cosets read
  ec.n_perm = m;
  ec.chunk_len = pk.chunk;
  for (uint32_t j = 0; j < m; j++) {
    ec.perm_value[j] = p.perm_column(cs.perm_columns[j], true);
    ec.perm_sigma[j] = p.sigma_coset(j);
  }
  for (uint32_t s = 0; s < n_sets; s++) ec.perm_z[s] = p.z[s].coset->p;
  ec.n_lookups = L | (pk.logup ? H2MI_LOOKUPS_LOGUP : 0u);
  // a table-logUp key: the K inputs are the advice columns' own cosets, K consecutive vectors from the first one's (create_prover)
  for (uint32_t l = 0; l < H2MI_FLEX_MAX_LOOKUPS; l++)
    lg.n_inputs[l] = l < L && pk.lookup_exprs ? pk.lookup_slices.sets[l] : l < L && pk.table_logup ? pk.tl_sets[l] : 1u;
  for (uint32_t l = 0; l < L; l++) {
    const h2mi_lookup& lk = cs.lookups[l];
    if (pk.lookup_exprs) {
      // compressed on the extended coset itself: a product of columns is no polynomial of degree < n, so transforming the
      // compressed rows would give another function
      p.compress_sides(pk.lookup_slices, l, true, *p.lk[l].c.in_coset, *p.lk[l].c.tab_coset);
      ec.lookup_input[l] = p.lk[l].c.in_coset->p;
      ec.lookup_table[l] = p.lk[l].c.tab_coset->p;
    } else {
      ec.lookup_input[l] = p.advice[lk.input.index].coset->p;
      ec.lookup_input_b[l] = lk.selector_fixed >= 0 ? p.fixed_coset(lk.selector_fixed) : nullptr;
      ec.lookup_table[l] = p.fixed_coset(lk.table_fixed);
    }
    ec.lookup_permuted_input[l] = p.lk[l].a.coset->p;
    ec.lookup_permuted_table[l] = pk.logup ? nullptr : p.lk[l].s.coset->p;
    ec.lookup_z[l] = p.lk[l].z.coset->p;
  }
  ec.l0 = p.l0_coset();
  ec.l_last = p.l_last_coset();
  ec.l_active = p.l_active_coset();
  std::memset(&sc, 0, sizeof(sc));
  sc.n_shuffles = pk.n_shuffles;
  for (uint32_t i = 0; i < pk.n_shuffles; i++) {  // compressed on the extended coset itself, as the lookups given as expressions are
    p.compress_sides(pk.shuffle_slices, i, true, *p.sf[i].c.in_coset, *p.sf[i].c.tab_coset);
    sc.input[i] = p.sf[i].c.in_coset->p;
    sc.shuffle[i] = p.sf[i].c.tab_coset->p;
    sc.z[i] = p.sf[i].z.coset->p;
  }
}
// the circuits of a proof for those kernels: the record and what it points into (the lookups' and shuffles' sides are compressed here)
struct QuotientCircuits {
  std::vector<h2mi_expr_cosets> ec;
  std::vector<h2mi_shuffle_cosets> sc;
  std::vector<h2mi_instance_cosets> ic;
  h2mi_logup_cosets lg;  // the key's: the same for every member
  h2mi_quotient_circuits rec;
  explicit QuotientCircuits(const Circuits& all) : ec(all.size()), sc(all.size()), ic(all.size()) {
    for (size_t i = 0; i < all.size(); i++) fill_expr_cosets(*all[i], ec[i], sc[i], lg, ic[i]);
    const h2mi_prover_s& p = *all[0];
    rec = {ec.data(), (uint32_t)ec.size(), p.pk->n_shuffles ? sc.data() : nullptr, &lg, ic.data(), &p.pk->check_gates, p.challenge_limbs(),
           p.pk->phases.n_challenges};
  }
};
// what every quotient call of a proof knows of the domain and the transcript
h2mi_quotient_scalars quotient_scalars(const h2mi_pk_s& pk, const h2mi_prover_s& p, const Fr& y) {
  const poly::EvaluationDomain& d = pk.domain;
  return {d.k(), d.extended_k(), pk.cs.blinding_factors, p.beta.l, p.gamma.l, y.l, pk.delta.l, d.get_g_coset().l, d.get_extended_omega().l,
          (const uint64_t*)d.t_inv().data()};  // (X^n - 1)^-1 on the coset: cached in the domain
}

// a joint phase of a batch: the members behind the leader must still be where their products left them (one that has started another
// proof since has overwritten its columns)
void require_members(const Circuits& all) {
  for (size_t i = 1; i < all.size(); i++)
    if (all[i]->phase != PRODUCTS) {
      all[0]->phase = IDLE;
      throw Error(H2MI_EINVAL, "a member of the batch has left the proof");
    }
}
// the proof is complete, or abandoned: every circuit's next proof starts with its advice
void finish_members(const Circuits& all) {
  for (h2mi_prover_s* c : all) c->phase = IDLE;
}

// the numerator of one circuit by the kernel of its shape (the single prover's route, unchanged)
void evaluate_h_single(h2mi_prover_s& p, const Fr& y);

// The numerator of a by-coset key, single prover or batch.  Extended-coset point c + rot i is (zeta w_ext^c) w^i: per slice c every
// column's coefficients go to the 2^k points of that coset (one transform each, shift zeta w_ext^c), the lookups' and shuffles' sides
// are compressed on the slices, and ONE launch folds every circuit's terms into h[c + rot i] — whatever the key's shape, through the
// program keygen built for the witness check, as batches do.  The shared columns' slices are the leader's.
void evaluate_h_by_coset(const Circuits& all, const Fr& y) {
  h2mi_prover_s& lead = *all[0];
  const h2mi_pk_s& pk = *lead.pk;
  const h2mi_constraint_system& cs = pk.cs;
  const poly::EvaluationDomain& d = pk.domain;
  const size_t n = pk.n;
  const uint32_t rot = 1u << (d.extended_k() - d.k());
  const h2mi_quotient_scalars scalars = quotient_scalars(pk, lead, y);
  for (h2mi_prover_s* c : all) c->lead = &lead;
  Fr shift = d.get_g_coset();
  for (uint32_t c = 0; c < rot; c++, shift = fr::mul(shift, d.get_extended_omega())) {
    auto slice = [&](const DeviceVec& poly, DeviceVec& out) {
      check(h2mi_ntt_bn254_fr_oop_dev(poly.p, n, out.p, d.k(), d.get_omega().l, shift.l, nullptr, nullptr), "coeff_to_slice");
    };
    for (uint32_t j = 0; j < cs.n_fixed; j++) slice(*pk.fixed_polys[j], *lead.fixed_slices[j]);
    for (uint32_t j = 0; j < cs.n_perm; j++) slice(*pk.sigma_polys[j], *lead.sigma_slices[j]);
    slice(*pk.l0_poly, *lead.l0_slice);
    slice(*pk.l_last_poly, *lead.l_last_slice);
    slice(*pk.l_active_poly, *lead.l_active_slice);
    for (h2mi_prover_s* m : all) {
      for (Forms& f : m->advice) slice(*f.poly, *f.coset);
      for (Forms& f : m->z) slice(*f.poly, *f.coset);
      for (uint32_t i = 0; i < cs.n_instance; i++) slice(*m->instance_poly[i], *m->instance_coset[i]);
      for (uint32_t l = 0; l < cs.n_lookups; l++) {
        slice(*m->lk[l].a.poly, *m->lk[l].a.coset);
        if (!pk.logup) slice(*m->lk[l].s.poly, *m->lk[l].s.coset);
        slice(*m->lk[l].z.poly, *m->lk[l].z.coset);
      }
      for (uint32_t i = 0; i < pk.n_shuffles; i++) slice(*m->sf[i].z.poly, *m->sf[i].z.coset);
    }
    const QuotientCircuits qc(all);  // compresses on the slices
    check(h2mi_plonk_evaluate_h_expr_batch_dev(&qc.rec, &scalars, (int32_t)c, lead.h->p, nullptr), "evaluate_h");
  }
  for (h2mi_prover_s* c : all) c->lead = nullptr;
}

void phase_quotient(const Circuits& all, const Fr& y, uint64_t* points_out) {
  h2mi_prover_s& p = *all[0];
  const h2mi_pk_s& pk = *p.pk;
  const h2mi_constraint_system& cs = pk.cs;
  const poly::EvaluationDomain& d = pk.domain;
  const size_t n = pk.n;
  require_phase(p, PRODUCTS);
  require_members(all);
  p.phase = IDLE;
  DeviceVec& h = *p.h;
  if (pk.by_coset) {
    evaluate_h_by_coset(all, y);
  } else if (!p.batch) {
    evaluate_h_single(p, y);
  } else {
    // several circuits (or a batch of one): ONE launch folds every circuit's terms into h, whatever the key's shape — a hard-wired
    // shape through the equivalent program keygen built for the witness check, which computes the same field elements
    const QuotientCircuits qc(all);
    const h2mi_quotient_scalars scalars = quotient_scalars(pk, p, y);
    check(h2mi_plonk_evaluate_h_expr_batch_dev(&qc.rec, &scalars, H2MI_WHOLE_COSET, h.p, nullptr), "evaluate_h");
  }
  check(h2mi_ntt_bn254_fr_dev(h.p, d.extended_k(), d.get_extended_omega_inv().l, nullptr, nullptr, nullptr), "extended_to_coeff");
  check(h2mi_fr_scale_powers_dev(h.p, pk.ext, d.get_g_coset_inv().l, d.get_extended_ifft_divisor().l, nullptr), "distribute_powers_zeta");
  const uint32_t pieces = cs.degree - 1;
  std::vector<const void*> cols;
  for (uint32_t i = 0; i < pieces; i++) cols.push_back(p.col(h, (size_t)i * n));
  p.commit_phase(false, cols, 0, /*sparse=*/false, /*inorder=*/true);
  p.read_points(pieces, points_out);
  p.phase = QUOTIENT;
}

void evaluate_h_single(h2mi_prover_s& p, const Fr& y) {
  const h2mi_pk_s& pk = *p.pk;
  const h2mi_constraint_system& cs = pk.cs;
  const uint32_t L = cs.n_lookups, m = cs.n_perm, n_sets = pk.n_sets;
  DeviceVec& h = *p.h;
  const h2mi_quotient_scalars scalars = quotient_scalars(pk, p, y);
  if (cs.gates == H2MI_GATES_STANDARD_PLONK) {
    h2mi_standard_plonk_cosets sc;
    for (int i = 0; i < 3; i++) {
      sc.advice[i] = p.advice[i].coset->p;
      sc.sigma[i] = pk.sigma_cosets[i]->p;
      sc.z[i] = p.z[i].coset->p;
    }
    for (int i = 0; i < 5; i++) sc.fixed[i] = pk.fixed_cosets[i]->p;
    sc.l0 = pk.l0->p;
    sc.l_last = pk.l_last->p;
    sc.l_active = pk.l_active->p;
    check(h2mi_plonk_evaluate_h_standard_dev(&sc, &scalars, h.p, nullptr), "evaluate_h");
  } else if (cs.gates == H2MI_GATES_EXPRESSIONS || pk.table_logup) {
    // gates given as a program: the interpreting kernel reads any column of the proof through one pointer table.  A table-logUp key of
    // a hard-wired shape goes the same way through the shape's equivalent program, as batches do: the shapes' own kernels have no logUp term
    const QuotientCircuits qc({&p});
    check(h2mi_plonk_evaluate_h_expr_dev(&qc.rec, &scalars, h.p, nullptr), "evaluate_h");
  } else if (cs.n_gates == 1 && m >= 1 && m <= 4 && L <= 1) {
    // one gate column: the specialised kernel (its level bookkeeping is written for this shape; faster per point than the general one)
    h2mi_range_cosets rc;
    std::memset(&rc, 0, sizeof(rc));
    rc.a = p.advice[cs.gate_advice[0]].coset->p;
    rc.q = pk.fixed_cosets[cs.gate_selector[0]]->p;
    for (uint32_t j = 0; j < m; j++) {
      rc.perm_value[j] = p.perm_column(cs.perm_columns[j], true);
      rc.perm_sigma[j] = pk.sigma_cosets[j]->p;
    }
    for (uint32_t s = 0; s < n_sets; s++) rc.perm_z[s] = p.z[s].coset->p;
    rc.l0 = pk.l0->p;
    rc.l_last = pk.l_last->p;
    rc.l_active = pk.l_active->p;
    rc.n_perm = m;
    rc.chunk_len = pk.chunk;
    rc.has_lookup = L ? 1 : 0;
    if (L) {
      const h2mi_lookup& lk = cs.lookups[0];
      if (lk.selector_fixed >= 0) {
        if (lk.input.index != cs.gate_advice[0]) throw Error(H2MI_EINVAL, "the selector form looks up the gate column");
        rc.lookup_selector = pk.fixed_cosets[lk.selector_fixed]->p;
      } else {
        rc.lookup_advice = p.advice[lk.input.index].coset->p;
      }
      rc.table = pk.fixed_cosets[lk.table_fixed]->p;
      rc.lookup_permuted_input = p.lk[0].a.coset->p;
      rc.lookup_permuted_table = p.lk[0].s.coset->p;
      rc.lookup_z = p.lk[0].z.coset->p;
    }
    check(h2mi_plonk_evaluate_h_range_dev(&rc, &scalars, h.p, nullptr), "evaluate_h");
  } else {
    // several gate columns: the general quotient kernel (one gate per column, one lookup per lookup-advice column)
    h2mi_flex_cosets fc;
    std::memset(&fc, 0, sizeof(fc));
    fc.n_gates = cs.n_gates;
    for (uint32_t g = 0; g < cs.n_gates; g++) {
      fc.gate_a[g] = p.advice[cs.gate_advice[g]].coset->p;
      fc.gate_q[g] = pk.fixed_cosets[cs.gate_selector[g]]->p;
    }
    fc.n_perm = m;
    fc.chunk_len = pk.chunk;
    for (uint32_t j = 0; j < m; j++) {
      fc.perm_value[j] = p.perm_column(cs.perm_columns[j], true);
      fc.perm_sigma[j] = pk.sigma_cosets[j]->p;
    }
    for (uint32_t s = 0; s < n_sets; s++) fc.perm_z[s] = p.z[s].coset->p;
    fc.n_lookups = L;
    for (uint32_t l = 0; l < L; l++) {
      const h2mi_lookup& lk = cs.lookups[l];
      fc.lookup_input[l] = p.advice[lk.input.index].coset->p;
      fc.lookup_input_b[l] = lk.selector_fixed >= 0 ? pk.fixed_cosets[lk.selector_fixed]->p : nullptr;
      fc.lookup_table[l] = pk.fixed_cosets[lk.table_fixed]->p;
      fc.lookup_permuted_input[l] = p.lk[l].a.coset->p;
      fc.lookup_permuted_table[l] = p.lk[l].s.coset->p;
      fc.lookup_z[l] = p.lk[l].z.coset->p;
    }
    fc.l0 = pk.l0->p;
    fc.l_last = pk.l_last->p;
    fc.l_active = pk.l_active->p;
    check(h2mi_plonk_evaluate_h_flex_dev(&fc, &scalars, h.p, nullptr), "evaluate_h");
  }
}

// per circuit: its advice queries, its permutation sets, its lookups, its shuffles; once per proof: the fixed queries, the random polynomial, sigma
size_t num_evaluations(const h2mi_pk_s& pk, size_t n_circuits = 1) {
  const h2mi_constraint_system& cs = pk.cs;
  return n_circuits * cs.n_advice_queries + cs.n_fixed_queries + 1 + cs.n_perm +
         n_circuits * ((pk.n_sets ? 3 * (size_t)pk.n_sets - 1 : 0) + (pk.logup ? 3 : 5) * (size_t)cs.n_lookups + 2 * (size_t)pk.n_shuffles);
}

// ---- phase 5: every evaluation create_proof writes -------------------------------------------------------------------------------
// [RECALL halo2_proofs v2023_02_02 plonk/prover.rs] with several circuits: the advice evaluations of every circuit in order, the
// fixed ones, the random polynomial, sigma, every circuit's permutation sets, every circuit's lookups
void phase_evaluations(const Circuits& all, const Fr& x, uint64_t* evals_out) {
  h2mi_prover_s& p = *all[0];
  const h2mi_pk_s& pk = *p.pk;
  const h2mi_constraint_system& cs = pk.cs;
  const poly::EvaluationDomain& d = pk.domain;
  const size_t n = pk.n;
  const uint32_t bf = cs.blinding_factors, L = cs.n_lookups, n_sets = pk.n_sets, pieces = cs.degree - 1;
  require_phase(p, QUOTIENT);
  require_members(all);
  p.phase = IDLE;
  if (!evals_out) throw Error(H2MI_EINVAL, "evals_out");
  const Fr omega = d.get_omega(), omega_inv = d.get_omega_inv();
  const Fr xn = fr::pow_u64(x, n);
  auto rot = [&](int64_t r) { return r == 0 ? x : fr::mul(x, pow_signed(omega, omega_inv, r)); };
  const Fr x_next = rot(1), x_last = rot(-(int64_t)(bf + 1)), x_inv = rot(-1);
  DeviceVec &h = *p.h, &h_poly = *p.h_poly, &random_poly = *p.random_poly;
  {  // h(X) = sum_i xn^i h_i(X): the polynomial vanishing.open() queries
    std::vector<const void*> ptrs;
    std::vector<Fr> sc;
    Fr pw = fr::ONE;
    for (uint32_t i = 0; i < pieces; i++) {
      ptrs.push_back(at(h, (size_t)i * n));
      sc.push_back(pw);
      pw = fr::mul(pw, xn);
    }
    check(h2mi_fr_lincomb_dev(ptrs.data(), (const uint64_t*)sc.data(), pieces, n, h_poly.p, nullptr), "h_poly");
  }
  struct Q {
    const DeviceVec* poly;
    Fr point;
  };
  std::vector<Q> written;
  for (const h2mi_prover_s* c : all)
    for (uint32_t i = 0; i < cs.n_advice_queries; i++) written.push_back({c->advice[cs.advice_queries[i].column].poly.get(), rot(cs.advice_queries[i].rotation)});
  for (uint32_t i = 0; i < cs.n_fixed_queries; i++) written.push_back({pk.fixed_polys[cs.fixed_queries[i].column].get(), rot(cs.fixed_queries[i].rotation)});
  written.push_back({&random_poly, x});
  for (auto& sp : pk.sigma_polys) written.push_back({sp.get(), x});
  for (const h2mi_prover_s* c : all)
    for (uint32_t i = 0; i < n_sets; i++) {
      written.push_back({c->z[i].poly.get(), x});
      written.push_back({c->z[i].poly.get(), x_next});
      if (i + 1 < n_sets) written.push_back({c->z[i].poly.get(), x_last});
    }
  for (const h2mi_prover_s* c : all)
    for (uint32_t l = 0; l < L; l++) {
      written.push_back({c->lk[l].z.poly.get(), x});
      written.push_back({c->lk[l].z.poly.get(), x_next});
      written.push_back({c->lk[l].a.poly.get(), x});
      if (pk.logup) continue;  // phi(x), phi(omega x), M(x)
      written.push_back({c->lk[l].a.poly.get(), x_inv});
      written.push_back({c->lk[l].s.poly.get(), x});
    }
  for (const h2mi_prover_s* c : all)  // every circuit's shuffles behind every circuit's lookups
    for (uint32_t i = 0; i < pk.n_shuffles; i++) {
      written.push_back({c->sf[i].z.poly.get(), x});
      written.push_back({c->sf[i].z.poly.get(), x_next});
    }
  std::vector<Q> todo = written;
  todo.push_back({&h_poly, x});  // opened but not written (the verifier recomputes it)
  // every evaluation in ONE call: groups of up to 24 distinct polynomials per distinct point (h2mi_fr_eval_polys_multi_dev)
  struct Slot {
    const DeviceVec* poly;
    Fr point;
  };
  std::vector<Slot> slots;
  std::vector<const void*> polys;
  std::vector<size_t> counts;
  std::vector<Fr> group_pts, distinct;
  for (const Q& q : todo)
    if (!contains(distinct, q.point)) distinct.push_back(q.point);
  for (const Fr& pt : distinct) {
    const size_t first = slots.size();
    for (const Q& q : todo) {
      if (!(q.point == pt)) continue;
      bool seen = false;
      for (size_t i = first; i < slots.size(); i++) seen = seen || slots[i].poly == q.poly;
      if (seen) continue;
      slots.push_back({q.poly, pt});
      polys.push_back(q.poly->p);
    }
    for (size_t c0 = first; c0 < slots.size(); c0 += 24) {
      counts.push_back(std::min<size_t>(24, slots.size() - c0));
      group_pts.push_back(pt);
    }
  }
  if (!p.evals || p.evals->n < slots.size()) p.evals = vec(slots.size() + 8);
  check(h2mi_fr_eval_polys_multi_dev(polys.data(), counts.data(), (const uint64_t*)group_pts.data(), counts.size(), n, p.evals->p, nullptr), "eval");
  std::vector<Fr> ev(slots.size());
  check(h2mi_memcpy_d2h(ev.data(), p.evals->p, slots.size() * 32), "d2h");
  auto value_of = [&](const DeviceVec* poly, const Fr& pt) {
    for (size_t i = 0; i < slots.size(); i++)
      if (slots[i].poly == poly && slots[i].point == pt) return ev[i];
    throw Error(H2MI_EINVAL, "query without an evaluation");
  };
  for (size_t i = 0; i < written.size(); i++) {
    const Fr v = value_of(written[i].poly, written[i].point);
    std::memcpy(evals_out + 4 * i, v.l, 32);
  }
  p.n_written = written.size();
  // the queries in create_proof's order (per circuit: advice; permutation.open: every set at x and omega x, then all but the last
  // at omega^last x in reverse; lookups — then fixed; sigma; vanishing.open: h, the random polynomial)
  p.queries.clear();
  auto q = [&](const DeviceVec* poly, const Fr& pt) { p.queries.push_back({poly, pt, value_of(poly, pt)}); };
  for (const h2mi_prover_s* c : all) {
    for (uint32_t i = 0; i < cs.n_advice_queries; i++) q(c->advice[cs.advice_queries[i].column].poly.get(), rot(cs.advice_queries[i].rotation));
    for (uint32_t i = 0; i < n_sets; i++) {
      q(c->z[i].poly.get(), x);
      q(c->z[i].poly.get(), x_next);
    }
    for (uint32_t i = n_sets > 0 ? n_sets - 1 : 0; i-- > 0;) q(c->z[i].poly.get(), x_last);
    for (uint32_t l = 0; l < L && pk.logup; l++) {  // lookups.open of a logUp key: phi at x, phi at omega x, M at x
      q(c->lk[l].z.poly.get(), x);
      q(c->lk[l].z.poly.get(), x_next);
      q(c->lk[l].a.poly.get(), x);
    }
    for (uint32_t l = 0; l < L && !pk.logup; l++) {
      q(c->lk[l].z.poly.get(), x);
      q(c->lk[l].a.poly.get(), x);
      q(c->lk[l].s.poly.get(), x);
      q(c->lk[l].a.poly.get(), x_inv);
      q(c->lk[l].z.poly.get(), x_next);
    }
    for (uint32_t i = 0; i < pk.n_shuffles; i++) {  // shuffles.open
      q(c->sf[i].z.poly.get(), x);
      q(c->sf[i].z.poly.get(), x_next);
    }
  }
  for (uint32_t i = 0; i < cs.n_fixed_queries; i++) q(pk.fixed_polys[cs.fixed_queries[i].column].get(), rot(cs.fixed_queries[i].rotation));
  for (auto& sp : pk.sigma_polys) q(sp.get(), x);
  q(&h_poly, x);
  q(&random_poly, x);
  p.phase = EVALUATIONS;
}

// a lone commitment whose point the caller reads next: in order on one stream, nothing deferred
void shplonk_commit(h2mi_prover_s& p, const DeviceVec& poly, uint64_t* point_out) {
  std::vector<const void*> cols = {p.col(poly)};
  p.commit_phase(false, cols, 0, false, /*inorder=*/true);
  p.read_points(1, point_out);
}

// ---- phase 6: ProverSHPLONK up to the commitment of h(X) = sum_i v^i Q_i(X) ------------------------------------------------------
void phase_shplonk_quotient(const Circuits& all, const Fr& y, const Fr& v, uint64_t* point_out) {
  h2mi_prover_s& p = *all[0];  // the queries name every circuit's polynomials; the scratch, the lanes and the commitment are the leader's
  const size_t n = p.pk->n;
  require_phase(p, EVALUATIONS);
  require_members(all);
  p.phase = IDLE;
  // construct_intermediate_sets
  std::vector<std::pair<const DeviceVec*, std::vector<std::pair<Fr, Fr>>>> by_poly;  // first-appearance order
  std::vector<Fr>& super_points = p.super_points;
  super_points.clear();
  for (const ProverQuery& q : p.queries) {
    if (!contains(super_points, q.point)) super_points.push_back(q.point);
    auto it = std::find_if(by_poly.begin(), by_poly.end(), [&](const auto& e) { return e.first == q.poly; });
    if (it == by_poly.end()) {
      by_poly.push_back({q.poly, {{q.point, q.eval}}});
    } else if (std::none_of(it->second.begin(), it->second.end(), [&](const auto& pe) { return pe.first == q.point; })) {
      it->second.push_back({q.point, q.eval});
    }
  }
  std::sort(super_points.begin(), super_points.end(), canonical_less);
  std::vector<RotationSet>& sets = p.sets;
  sets.clear();
  for (auto& e : by_poly) {
    std::vector<Fr> pts;
    for (auto& pe : e.second) pts.push_back(pe.first);
    std::sort(pts.begin(), pts.end(), canonical_less);
    auto rs = std::find_if(sets.begin(), sets.end(), [&](const RotationSet& s) { return s.points == pts; });
    if (rs == sets.end()) {
      sets.push_back(RotationSet{pts, {}});
      rs = sets.end() - 1;
    }
    std::vector<Fr> evals;
    for (const Fr& pt : rs->points) evals.push_back(std::find_if(e.second.begin(), e.second.end(), [&](const auto& pe) { return pe.first == pt; })->second);
    rs->members.push_back({e.first, evals});
  }
  p.v = v;
  {  // the divisions below need the power tables of every opening point and of its inverse: built now, in one launch
    std::vector<Fr> bases = super_points;
    const std::vector<Fr> inv = fr::batch_invert(super_points);
    bases.insert(bases.end(), inv.begin(), inv.end());
    if (!bases.empty() && bases.size() <= 32) check(h2mi_fr_powtab_prefetch_dev((const uint64_t*)bases.data(), bases.size(), n, nullptr), "powtab_prefetch");
  }
  while (p.q.size() < sets.size()) p.q.push_back(vec(n));
  while (p.s.size() < sets.size()) p.s.push_back(vec(n));
  // quotient contributions Q_i = (sum_j y^j (P_ij - R_ij)) / Z_i.  The sets are independent chains of small launches (one linear
  // combination, one division round per set): set i runs on lane i mod 3, so the longest chain, not their sum, is waited for
  p.remainders.clear();
  for (size_t i = 0; i < sets.size(); i++) check(h2mi_memset_zero(p.q[i]->p, n * 32), "zero");
  for (h2mi_stream_t st : p.lane) check(h2mi_stream_wait(st, nullptr), "stream_wait");
  for (size_t i = 0; i < sets.size(); i++) {
    const RotationSet& rs = sets[i];
    const size_t lane = i % 3;
    h2mi_stream_t stream = lane ? p.lane[lane - 1] : nullptr;
    std::vector<Fr> ypow(rs.members.size(), fr::ONE);
    for (size_t j = 1; j < ypow.size(); j++) ypow[j] = fr::mul(ypow[j - 1], y);
    std::vector<const DeviceVec*> polys;
    for (auto& mb : rs.members) polys.push_back(mb.first);
    lincomb(polys, ypow, n, *p.s[i], stream);
    std::vector<Fr> rsum(rs.points.size(), fr_zero());
    const std::vector<std::vector<Fr>> basis = lagrange_basis(rs.points);
    for (size_t j = 0; j < rs.members.size(); j++) {
      const std::vector<Fr> r = interpolate(basis, rs.members[j].second);
      for (size_t t = 0; t < r.size(); t++) rsum[t] = fr::sub(rsum[t], fr::mul(ypow[j], r[t]));
    }
    add_head(*p.s[i], rsum, stream);
    std::vector<Fr> rem;
    for (const Fr& c : rsum) rem.push_back(fr::neg(c));
    p.remainders.push_back(rem);  // R_i(X) = sum_j y^j R_ij(X), low to high
    kate_chain(*p.s[i], n, rs.points, *p.tmp[lane], *p.q[i], stream, p.nx[lane].get());
  }
  for (h2mi_stream_t st : p.lane) check(h2mi_stream_wait(nullptr, st), "stream_wait");
  {
    std::vector<const DeviceVec*> polys;
    std::vector<Fr> vpow(sets.size(), fr::ONE);
    for (size_t i = 1; i < vpow.size(); i++) vpow[i] = fr::mul(vpow[i - 1], v);
    for (size_t i = 0; i < sets.size(); i++) polys.push_back(p.q[i].get());
    lincomb(polys, vpow, n, *p.h_x);
  }
  shplonk_commit(p, *p.h_x, point_out);
  p.phase = SHPLONK_Q;
}

// ---- phase 7: the linearisation L(X) at u, divided by (X - u) -------------------------------------------------------------------
void phase_shplonk_open(const Circuits& all, const Fr& u, uint64_t* point_out) {
  h2mi_prover_s& p = *all[0];
  const size_t n = p.pk->n;
  require_phase(p, SHPLONK_Q);
  require_members(all);
  p.phase = IDLE;
  const std::vector<RotationSet>& sets = p.sets;
  const std::vector<Fr>& super_points = p.super_points;
  const Fr zt_eval = vanishing_at(super_points, u);
  std::vector<Fr> z_diffs;
  for (const RotationSet& rs : sets) {
    std::vector<Fr> diffs;
    for (const Fr& pt : super_points)
      if (!contains(rs.points, pt)) diffs.push_back(pt);
    z_diffs.push_back(vanishing_at(diffs, u));
  }
  const Fr norm = fr::invert(z_diffs[0]);  // "normalize coefficients by the coefficient of the first polynomial"
  // sum_j y^j (P_ij(X) - R_ij(u)) = S_i(X) + R_i(X) - R_i(u) with S_i the vector the quotient step left in s[i] — one linear
  // combination over the rotation sets' sums and h(X) instead of every opened polynomial again, and a low-degree head
  std::vector<const DeviceVec*> polys;
  std::vector<Fr> scalars;
  size_t head_len = 0;
  for (const RotationSet& rs : sets) head_len = std::max(head_len, rs.points.size());
  std::vector<Fr> head(head_len, fr_zero());
  Fr vp = fr::ONE;
  for (size_t i = 0; i < sets.size(); i++) {
    const Fr w = fr::mul(fr::mul(vp, z_diffs[i]), norm);
    polys.push_back(p.s[i].get());
    scalars.push_back(w);
    for (size_t t = 0; t < p.remainders[i].size(); t++) head[t] = fr::add(head[t], fr::mul(w, p.remainders[i][t]));
    head[0] = fr::sub(head[0], fr::mul(w, horner(p.remainders[i], u)));
    vp = fr::mul(vp, p.v);
  }
  polys.push_back(p.h_x.get());
  scalars.push_back(fr::neg(fr::mul(zt_eval, norm)));
  lincomb(polys, scalars, n, *p.l_x);
  add_head(*p.l_x, head);
  check(h2mi_memset_zero(p.h2_x->p, n * 32), "zero");
  kate_chain(*p.l_x, n, {u}, *p.tmp[0], *p.h2_x, nullptr, nullptr);
  shplonk_commit(p, *p.h2_x, point_out);
  finish_members(all);  // the proof is complete; the next one starts with h2mi_prover_advice
}

// ---- ProverGWC (poly/kzg/multiopen/gwc, restated from memory: DESIGN.md 4.5) — the other ending of a proof ----------------------------
// the opening points of a key's query list: its distinct rotations modulo 2^k (the queries of phase_evaluations, by the key alone)
size_t gwc_num_points(const h2mi_pk_s& pk) {
  const h2mi_constraint_system& cs = pk.cs;
  const int64_t n = (int64_t)pk.n;
  std::vector<int64_t> rots = {0};  // h and the random polynomial, at least
  auto add = [&](int64_t r) {
    r = ((r % n) + n) % n;
    if (std::find(rots.begin(), rots.end(), r) == rots.end()) rots.push_back(r);
  };
  for (uint32_t i = 0; i < cs.n_advice_queries; i++) add(cs.advice_queries[i].rotation);
  for (uint32_t i = 0; i < cs.n_fixed_queries; i++) add(cs.fixed_queries[i].rotation);
  if (pk.n_sets || cs.n_lookups || pk.n_shuffles) add(1);
  if (pk.n_sets > 1) add(-(int64_t)(cs.blinding_factors + 1));
  if (cs.n_lookups && !pk.logup) add(-1);
  return rots.size();
}
// W_i lives in the SHPLONK scratch (a proof uses one ending): q[0], s[0], q[1], s[1], ..
Dev& gwc_w(h2mi_prover_s& p, size_t i) {
  std::vector<Dev>& v = i % 2 ? p.s : p.q;
  while (v.size() <= i / 2) v.push_back(vec(p.pk->n));
  return v[i / 2];
}

// v in, [W_0] .. [W_(P-1)] out: group the queries by point in order of first appearance, W_i = (sum_j v^j p_ij) / (X - z_i) — the
// division drops the remainder sum_j v^j e_ij, so the evaluations stay on the host — and commit the W_i as one phase
void phase_gwc_open(const Circuits& all, const Fr& v, uint64_t* points_out) {
  h2mi_prover_s& p = *all[0];  // the queries name every circuit's polynomials; the scratch and the commitments are the leader's
  const size_t n = p.pk->n;
  require_phase(p, EVALUATIONS);
  require_members(all);
  p.phase = IDLE;
  if (!points_out) throw Error(H2MI_EINVAL, "points_out");
  std::vector<Fr> pts;
  std::vector<std::vector<const DeviceVec*>> groups;
  for (const ProverQuery& q : p.queries) {
    size_t g = std::find(pts.begin(), pts.end(), q.point) - pts.begin();
    if (g == pts.size()) {
      pts.push_back(q.point);
      groups.emplace_back();
    }
    groups[g].push_back(q.poly);
  }
  const size_t P = pts.size();
  if (P != gwc_num_points(*p.pk) || contains(pts, fr_zero())) throw Error(H2MI_EINVAL, "gwc: the opening points coincide or vanish");
  const std::vector<Fr> inv = fr::batch_invert(pts);
  std::vector<const void*> polys;
  std::vector<Fr> scalars;
  std::vector<size_t> counts;
  std::vector<void*> outs;
  for (size_t i = 0; i < P; i++) {
    Fr vp = fr::ONE;
    for (const DeviceVec* poly : groups[i]) {
      polys.push_back(poly->p);
      scalars.push_back(vp);
      vp = fr::mul(vp, v);
    }
    counts.push_back(groups[i].size());
    outs.push_back(gwc_w(p, i)->p);
  }
  check(h2mi_fr_gwc_witness_dev(polys.data(), (const uint64_t*)scalars.data(), counts.data(), (const uint64_t*)pts.data(), (const uint64_t*)inv.data(), P, n,
                                outs.data(), nullptr),
        "gwc_witness");
  // one phase of P commitments; a combiner's buffers hold the largest of the other phases, so there the phase goes in that many at a time
  const size_t slots = p.d_partial ? max_phase_points(*p.pk) : P;
  for (size_t c0 = 0; c0 < P; c0 += slots) {
    const size_t cnt = std::min(slots, P - c0);
    std::vector<const void*> cols;
    for (size_t i = 0; i < cnt; i++) cols.push_back(p.col(*gwc_w(p, c0 + i)));
    p.commit_phase(false, cols, 0, /*sparse=*/false, /*inorder=*/true);
    p.read_points(cnt, points_out + 8 * c0);
  }
  finish_members(all);  // the proof is complete; the next one starts with h2mi_prover_advice
}

Fr load_fr(const uint64_t* l) {
  Fr a;
  std::memcpy(a.l, l, 32);
  return a;
}

// no exception crosses the C boundary
template <class F>
int guarded(F f) {
  try {
    f();
    return H2MI_OK;
  } catch (const Error& e) {
    return e.code;
  } catch (const std::bad_alloc&) {
    return H2MI_ENOMEM;
  } catch (...) {
    return H2MI_EINVAL;
  }
}

int pick(const std::vector<Dev>& v, uint32_t index, void** d_ptr, size_t* count) {
  if (index >= v.size() || !v[index]) return H2MI_ERANGE;
  *d_ptr = v[index]->p;
  if (count) *count = v[index]->n;
  return H2MI_OK;
}
int pick(const Dev& d, uint32_t index, void** d_ptr, size_t* count) {
  if (index != 0 || !d) return H2MI_ERANGE;
  *d_ptr = d->p;
  if (count) *count = d->n;
  return H2MI_OK;
}

// ---- proving-key files (h2mi_keyfile.hpp holds the format; DESIGN.md 3 describes it) ---------------------------------------------------
// a parsed blob as the record keygen takes; the program pointers are NULL where the key has none
struct BlobArgs {
  h2mi_gate_program gates;
  h2mi_lookup_program lookups;
  h2mi_shuffle_program shuffles;
  h2mi_logup_inputs inputs;
  h2mi_keygen_args args;
  explicit BlobArgs(const keyfile::Blob& b) {
    std::memset(&args, 0, sizeof(args));
    args.cs = &b.cs;
    args.flags = b.logup ? H2MI_KEYGEN_LOGUP : 0u;
    if (b.has_gates) {
      gates = b.gates.view();
      args.gates = &gates;
    }
    if (b.has_lookups) {
      std::memset(&lookups, 0, sizeof(lookups));
      lookups.n_lookups = b.n_lookups;
      std::memcpy(lookups.n_pairs, b.lookup_pairs, sizeof(lookups.n_pairs));
      lookups.exprs = b.lookup_exprs.view();
      std::memcpy(inputs.n_inputs, b.lookup_inputs, sizeof(inputs.n_inputs));
      args.lookups = &lookups;
      args.inputs = &inputs;
    }
    if (b.has_shuffles) {
      std::memset(&shuffles, 0, sizeof(shuffles));
      shuffles.n_shuffles = b.n_shuffles;
      std::memcpy(shuffles.n_pairs, b.shuffle_pairs, sizeof(shuffles.n_pairs));
      shuffles.exprs = b.shuffle_exprs.view();
      args.shuffles = &shuffles;
    }
    if (b.has_phases) args.phases = &b.phases;
  }
};

// everything import checks before it touches the device: the format's own rules, then the constraint system's and its programs'
void check_blob(const uint8_t* blob, size_t len, keyfile::Blob& b) {
  if (keyfile::parse(blob, len, b)) throw Error(H2MI_EINVAL, "key file: not a well-formed proving-key blob");
  validate(BlobArgs(b).args);
}

void* arena_alloc(void* ctx, size_t bytes) {
  std::vector<uint64_t>* v = (std::vector<uint64_t>*)ctx;
  v->assign((bytes + 7) / 8, 0);
  return v->data();
}

// the key as one blob; with_cells == false: the same sections with zeros where the cells would be, for the length alone (the counts
// take the first two launches of the compaction, not the third)
void export_key(h2mi_pk_s& pk, const uint8_t* user, size_t user_len, bool with_cells, std::vector<uint8_t>& out) {
  const h2mi_constraint_system& cs = pk.cs;
  std::vector<h2mi_cells_compacted> cols(cs.n_fixed);
  for (uint32_t f = 0; f < cs.n_fixed; f++) {
    std::memset(&cols[f], 0, sizeof(cols[f]));
    cols[f].d_column = pk.fixed_values[f]->p;  // the primary device's, in every multi-device mode
    cols[f].row_limit = pk.u;
  }
  std::vector<uint64_t> arena;
  check(h2mi_fr_compact_cells_dev(cols.data(), cs.n_fixed, 0, with_cells ? arena_alloc : nullptr, &arena, nullptr), "compact cells");
  keyfile::Writer w;
  w.header(pk.logup ? keyfile::FLAG_LOGUP : 0);
  w.constraint_system(cs, pk.lookup_exprs);
  w.begin();
  if (cs.gates == H2MI_GATES_EXPRESSIONS) w.program(pk.gate_program);
  w.end();
  w.begin();
  if (pk.lookup_exprs) {
    w.u32(cs.n_lookups);
    for (uint32_t l = 0; l < cs.n_lookups; l++) w.u32(pk.lookup_pairs[l]);
    for (uint32_t l = 0; l < cs.n_lookups; l++) w.u32(pk.lookup_slices.sets[l]);
    w.program({pk.lookup_ops.data(), (uint32_t)pk.lookup_ops.size(), pk.lookup_constants.data(), (uint32_t)(pk.lookup_constants.size() / 4)});
  }
  w.end();
  w.begin();
  if (pk.n_shuffles) {
    w.u32(pk.n_shuffles);
    for (uint32_t i = 0; i < pk.n_shuffles; i++) w.u32(pk.shuffle_pairs[i]);
    w.program({pk.shuffle_ops.data(), (uint32_t)pk.shuffle_ops.size(), pk.shuffle_constants.data(), (uint32_t)(pk.shuffle_constants.size() / 4)});
  }
  w.end();
  w.begin();
  if (pk.phases.n_phases > 1 || pk.phases.n_challenges) {
    w.u32(pk.phases.n_phases);
    w.u32(pk.phases.n_challenges);
    for (uint32_t j = 0; j < cs.n_advice; j++) w.u32(pk.phases.advice_phase[j]);
    for (uint32_t i = 0; i < pk.phases.n_challenges; i++) w.u32(pk.phases.challenge_phase[i]);
  }
  w.end();
  for (uint32_t f = 0; f < cs.n_fixed; f++) {
    const h2mi_cells_compacted& c = cols[f];
    const uint32_t layout = keyfile::layout_of(c.count, c.last, c.width);
    if (with_cells) {
      if (layout != c.layout) throw Error(H2MI_EINVAL, "key file: the compaction's layout is not the format's");
      w.column(layout, c.width, c.count, c.last, c.values, c.rows);
    } else {
      w.begin();
      w.u32(layout); w.u32(layout ? c.width : 0); w.u32((uint32_t)c.count); w.u32(c.last);
      w.b.resize(w.b.size() + (layout == keyfile::LAYOUT_DENSE ? (size_t)c.last * c.width : (size_t)c.count * (c.width + 4)), 0);
      w.end();
    }
  }
  w.begin();
  w.bytes(pk.moved_cells.data(), pk.moved_cells.size() * 4);
  w.end();
  w.begin();
  w.bytes(pk.fixed_commitments.data(), pk.fixed_commitments.size() * 64);
  w.bytes(pk.permutation_commitments.data(), pk.permutation_commitments.size() * 64);
  w.end();
  w.begin();
  w.bytes(user, user_len);
  w.end();
  w.finish();
  out.swap(w.b);
}

std::unique_ptr<h2mi_pk_s> import_key(const uint8_t* blob, size_t len, uint64_t g_lagrange, unsigned flags) {
  keyfile::Blob b;
  check_blob(blob, len, b);
  if (h2mi_device_count() == 0) throw Error(H2MI_ENODEV, "no device");
  BlobArgs p(b);
  const h2mi_constraint_system& cs = b.cs;
  // the blob's own cells as the caller's would arrive: dense runs without a row list, sparse ones with theirs, as 64-bit integers or
  // as canonical words — fill_column / k_cells_scatter from here on, and build_table reads them on the host
  std::vector<h2mi_column_cells> fixed(cs.n_fixed);
  for (uint32_t f = 0; f < cs.n_fixed; f++) {
    const keyfile::Column& c = b.fixed[f];
    h2mi_column_cells& out = fixed[f];
    out = {nullptr, nullptr, 0, 0};
    if (c.layout == keyfile::LAYOUT_EMPTY) continue;
    out.values = (const uint64_t*)(blob + c.values_at);
    out.flags = c.width == 8 ? H2MI_CELLS_I64 : H2MI_CELLS_CANONICAL;
    out.count = c.layout == keyfile::LAYOUT_DENSE ? c.last : c.count;
    if (c.layout == keyfile::LAYOUT_SPARSE) out.rows = (const uint32_t*)(blob + c.rows_at);
  }
  check_cells(fixed.data(), cs.n_fixed, H2MI_CELLS_FOR_FIXED);
  std::vector<std::array<uint32_t, 4>> moved(b.n_moved);
  if (b.n_moved) std::memcpy(moved.data(), blob + b.moved_at, 16 * b.n_moved);
  // keygen compares the commitments it recomputes with the stored ones and throws H2MI_EINVAL where they differ
  p.args.g_lagrange_handle = g_lagrange;
  p.args.fixed = fixed.data();
  p.args.flags |= flags;
  return keygen(p.args, {&moved, blob + b.commitments_at, nullptr});
}

}  // namespace

extern "C" {

int h2mi_prover_pk_export(h2mi_pk_t pk, const void* user, size_t user_len, void* buf, size_t cap, size_t* len_out) {
  if (!len_out || (user_len && !user) || user_len > keyfile::MAX_USER_BYTES) return H2MI_EINVAL;
  *len_out = 0;
  if (!alive(g_live_pks, pk)) return H2MI_EHANDLE;
  if (pk->vk_only) return H2MI_EINVAL;  // it holds no moved cells: not a key anything could prove with
  if (pk->table_logup) return H2MI_EINVAL;  // the blob format has no section for the grouping of a hard-wired shape's lookups
  int range = H2MI_OK;
  const int rc = guarded([&] {
    std::vector<uint8_t> blob;
    export_key(*pk, (const uint8_t*)user, user_len, buf != nullptr, blob);
    *len_out = blob.size();
    if (!buf) return;
    if (blob.size() > cap) range = H2MI_ERANGE;
    else std::memcpy(buf, blob.data(), blob.size());
  });
  return rc ? rc : range;
}

int h2mi_prover_pk_blob_check(const void* buf, size_t len, h2mi_constraint_system* cs_out, const void** user_out, size_t* user_len_out) {
  if (!buf) return H2MI_EINVAL;
  return guarded([&] {
    keyfile::Blob b;
    check_blob((const uint8_t*)buf, len, b);
    if (cs_out) *cs_out = b.cs;
    if (user_out) *user_out = (const uint8_t*)buf + b.user_at;
    if (user_len_out) *user_len_out = b.user_len;
  });
}

int h2mi_prover_pk_import(const void* buf, size_t len, uint64_t g_lagrange_handle, unsigned flags, h2mi_pk_t* pk_out) {
  if (!buf || !pk_out || (flags & ~H2MI_KEYGEN_BY_COSET)) return H2MI_EINVAL;
  *pk_out = nullptr;
  return guarded([&] {
    std::vector<uint64_t> aligned;  // the cell sections are read through uint64_t / uint32_t pointers
    const uint8_t* blob = (const uint8_t*)buf;
    if ((uintptr_t)buf & 7u) {
      aligned.resize((len + 7) / 8);
      std::memcpy(aligned.data(), buf, len);
      blob = (const uint8_t*)aligned.data();
    }
    std::unique_ptr<h2mi_pk_s> pk = import_key(blob, len, g_lagrange_handle, flags);
    std::lock_guard<std::mutex> lk(g_reg_mu);
    g_live_pks.insert(pk.get());
    *pk_out = pk.release();
  });
}

int h2mi_prover_keygen(const h2mi_keygen_args* args, h2mi_pk_t* pk_out) {
  if (!args || !pk_out || !args->cs || (args->cs->n_fixed && !args->fixed) || (args->n_copies && !args->copies)) return H2MI_EINVAL;
  const h2mi_keygen_args& a = *args;
  if (a.flags & ~(H2MI_KEYGEN_VK_ONLY | H2MI_KEYGEN_LOGUP | H2MI_KEYGEN_BY_COSET)) return H2MI_EINVAL;
  *pk_out = nullptr;
  TableLogup groups;
  KeygenExtra extra;
  if (table_mode(a)) {
    if ((a.flags & H2MI_KEYGEN_BY_COSET) || a.gates || a.lookups || a.phases || a.shuffles) return H2MI_EINVAL;
    if (const int rc = check_table_logup(*a.cs, a.inputs, nullptr, &groups)) return rc;  // every rule of the grouping, before any device work
    extra.table_logup = &groups;
  } else {
    if (((a.flags & H2MI_KEYGEN_LOGUP) || a.inputs) && !a.lookups) return H2MI_EINVAL;
    for (uint32_t l = 0; a.inputs && l < a.lookups->n_lookups && l < H2MI_MAX_LOOKUPS; l++)  // several sets are a logUp key's
      if (a.inputs->n_inputs[l] != 1 && !(a.flags & H2MI_KEYGEN_LOGUP)) return H2MI_EINVAL;
  }
  if (const int rc = h2mi_column_cells_check(a.fixed, a.cs->n_fixed, H2MI_CELLS_FOR_FIXED)) return rc;
  if (h2mi_device_count() == 0) return H2MI_ENODEV;  // no CPU fallback: the prover exists on a GPU or not at all
  return guarded([&] {
    std::unique_ptr<h2mi_pk_s> pk = keygen(a, extra);
    std::lock_guard<std::mutex> lk(g_reg_mu);
    g_live_pks.insert(pk.get());
    *pk_out = pk.release();
  });
}

int h2mi_column_cells_check(const h2mi_column_cells* cells, uint32_t n_columns, unsigned where) {
  if (where != H2MI_CELLS_FOR_ADVICE && where != H2MI_CELLS_FOR_INSTANCE && where != H2MI_CELLS_FOR_FIXED) return H2MI_EINVAL;
  if (n_columns && !cells) return H2MI_EINVAL;
  for (uint32_t i = 0; i < n_columns; i++) {
    const h2mi_column_cells& c = cells[i];
    const uint32_t f = c.flags;
    if (f & ~(H2MI_CELLS_CANONICAL | H2MI_CELLS_RATIONAL | H2MI_CELLS_I64 | H2MI_CELLS_DEVICE)) return H2MI_EINVAL;
    if ((f & H2MI_CELLS_I64) && (f & (H2MI_CELLS_CANONICAL | H2MI_CELLS_RATIONAL))) return H2MI_EINVAL;
    if ((f & H2MI_CELLS_DEVICE) && ((f & H2MI_CELLS_RATIONAL) || where != H2MI_CELLS_FOR_ADVICE)) return H2MI_EINVAL;
    if (where == H2MI_CELLS_FOR_INSTANCE && ((f & H2MI_CELLS_RATIONAL) || c.rows)) return H2MI_EINVAL;
    if (c.count && !c.values) return H2MI_EINVAL;
    const uintptr_t value_align = (f & H2MI_CELLS_DEVICE) && !(f & H2MI_CELLS_I64) ? 15u : 7u;
    if (((uintptr_t)c.values & value_align) || ((uintptr_t)c.rows & 3u)) return H2MI_EINVAL;
    if (c.count > ((size_t)1 << H2MI_MAX_LOG_N)) return H2MI_ERANGE;
  }
  return H2MI_OK;
}

int h2mi_gate_program_check(const h2mi_constraint_system* cs, const h2mi_gate_program* gates, uint32_t* degree_out, uint32_t* max_stack_out) {
  if (!cs || !gates) return H2MI_EINVAL;
  h2::ExprShape sh;
  const int rc = check_program(*cs, gates, &sh);
  if (rc) return rc;
  if (degree_out) *degree_out = sh.degree;
  if (max_stack_out) *max_stack_out = sh.max_stack;
  return H2MI_OK;
}

int h2mi_shape_gate_program(const h2mi_constraint_system* cs, h2mi_expr_op* ops, uint32_t ops_cap, uint32_t* n_ops_out, uint64_t* constants,
                            uint32_t constants_cap, uint32_t* n_constants_out) {
  (void)constants;
  (void)constants_cap;
  if (!cs || !n_ops_out || !n_constants_out || (ops_cap && !ops)) return H2MI_EINVAL;
  std::vector<h2mi_expr_op> prog;
  auto q = [&](uint32_t kind, uint32_t column, int32_t rotation = 0) { prog.push_back({kind, column, rotation}); };
  auto op = [&](uint32_t code) { prog.push_back({code, 0, 0}); };
  if (cs->gates == H2MI_GATES_STANDARD_PLONK) {  // q_a a + q_b b + q_c c + q_ab a b + constant: advice 0..2, fixed 0..4
    for (uint32_t i = 0; i < 3; i++) {
      q(H2MI_EXPR_FIXED, i);
      q(H2MI_EXPR_ADVICE, i);
      op(H2MI_EXPR_MUL);
      if (i) op(H2MI_EXPR_ADD);
    }
    q(H2MI_EXPR_FIXED, 3);
    q(H2MI_EXPR_ADVICE, 0);
    op(H2MI_EXPR_MUL);
    q(H2MI_EXPR_ADVICE, 1);
    op(H2MI_EXPR_MUL);
    op(H2MI_EXPR_ADD);
    q(H2MI_EXPR_FIXED, 4);
    op(H2MI_EXPR_ADD);
    op(H2MI_EXPR_END);
  } else if (cs->gates == H2MI_GATES_FLEX_VERTICAL) {  // per gate column q (a + a(wX) a(w^2 X) - a(w^3 X)), in evaluate_h's order
    if (cs->n_gates == 0 || cs->n_gates > H2MI_MAX_GATES) return H2MI_EINVAL;
    for (uint32_t g = 0; g < cs->n_gates; g++) {
      const uint32_t a = cs->gate_advice[g];
      q(H2MI_EXPR_ADVICE, a, 1);
      q(H2MI_EXPR_ADVICE, a, 2);
      op(H2MI_EXPR_MUL);
      q(H2MI_EXPR_ADVICE, a, 0);
      op(H2MI_EXPR_ADD);
      q(H2MI_EXPR_ADVICE, a, 3);
      op(H2MI_EXPR_SUB);
      q(H2MI_EXPR_FIXED, cs->gate_selector[g]);
      op(H2MI_EXPR_MUL);
      op(H2MI_EXPR_END);
    }
  } else {
    return H2MI_EINVAL;  // H2MI_GATES_EXPRESSIONS: the caller holds the program
  }
  *n_ops_out = (uint32_t)prog.size();
  *n_constants_out = 0;  // neither shape pushes a constant
  if (prog.size() > ops_cap) return H2MI_ERANGE;
  std::memcpy(ops, prog.data(), prog.size() * sizeof(h2mi_expr_op));
  return H2MI_OK;
}

int h2mi_lookup_program_check(const h2mi_constraint_system* cs, const h2mi_lookup_program* lookups, uint32_t* degree_out) {
  if (!cs || !lookups) return H2MI_EINVAL;
  return check_lookup_program(*cs, lookups, degree_out, nullptr);
}

int h2mi_advice_phases_check(const h2mi_constraint_system* cs, const h2mi_gate_program* gates, const h2mi_lookup_program* lookups,
                             const h2mi_advice_phases* phases) {
  if (!cs || !gates || !phases) return H2MI_EINVAL;
  return check_phases(*cs, gates, lookups, *phases);
}

int h2mi_shuffle_program_check(const h2mi_constraint_system* cs, const h2mi_shuffle_program* shuffles, uint32_t* degree_out) {
  if (!cs || !shuffles) return H2MI_EINVAL;
  return check_shuffle_program(*cs, shuffles, degree_out, nullptr);
}

int h2mi_shuffle_phases_check(const h2mi_constraint_system* cs, const h2mi_shuffle_program* shuffles, const h2mi_advice_phases* phases,
                              uint32_t* degree_out) {
  if (!cs || !shuffles) return H2MI_EINVAL;
  if (phases && phases->n_challenges > H2MI_MAX_CHALLENGES) return H2MI_EINVAL;
  return check_shuffle_program(*cs, shuffles, degree_out, nullptr, phases ? phases->n_challenges : 0);
}

int h2mi_logup_inputs_check(const h2mi_constraint_system* cs, const h2mi_lookup_program* lookups, const h2mi_logup_inputs* inputs,
                            const h2mi_advice_phases* phases, uint32_t* degree_out) {
  if (!cs || !lookups) return H2MI_EINVAL;
  if (phases && phases->n_challenges > H2MI_MAX_CHALLENGES) return H2MI_EINVAL;
  return check_lookup_program(*cs, lookups, degree_out, nullptr, phases ? phases->n_challenges : 0, inputs);
}

int h2mi_table_logup_check(const h2mi_constraint_system* cs, const h2mi_logup_inputs* sets, uint32_t* degree_out) {
  if (!cs) return H2MI_EINVAL;
  return check_table_logup(*cs, sets, degree_out, nullptr);
}

int h2mi_prover_pk_release(h2mi_pk_t pk) {
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    if (!pk || !g_live_pks.count(pk)) return H2MI_EHANDLE;
    if (pk->users) return H2MI_EINVAL;  // destroy its provers first
    g_live_pks.erase(pk);
  }
  h2mi_sync();  // nothing queued may still read the key's vectors
  delete pk;
  return H2MI_OK;
}

int h2mi_prover_vk_commitments(h2mi_pk_t pk, uint64_t* fixed_out, uint64_t* permutation_out) {
  if (!alive(g_live_pks, pk)) return H2MI_EHANDLE;
  if (fixed_out && !pk->fixed_commitments.empty()) std::memcpy(fixed_out, pk->fixed_commitments.data(), pk->fixed_commitments.size() * 64);
  if (permutation_out && !pk->permutation_commitments.empty())
    std::memcpy(permutation_out, pk->permutation_commitments.data(), pk->permutation_commitments.size() * 64);
  return H2MI_OK;
}

int h2mi_prover_create(h2mi_pk_t pk, uint64_t g_handle, uint64_t g_lagrange_handle, size_t base_lo, size_t base_count, h2mi_prover_t* prover_out) {
  if (!prover_out) return H2MI_EINVAL;
  *prover_out = nullptr;
  if (h2mi_device_count() == 0) return H2MI_ENODEV;
  if (!alive(g_live_pks, pk)) return H2MI_EHANDLE;
  return guarded([&] {
    std::unique_ptr<h2mi_prover_s> p = create_prover(pk, g_handle, g_lagrange_handle, base_lo, base_count);
    std::lock_guard<std::mutex> lk(g_reg_mu);
    g_live_provers.insert(p.get());
    pk->users++;
    *prover_out = p.release();
  });
}

int h2mi_prover_destroy(h2mi_prover_t prover) {
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    if (!prover || !g_live_provers.count(prover)) return H2MI_EHANDLE;
    if (prover->batch) return H2MI_EINVAL;  // destroy the batch it is bound into first
    g_live_provers.erase(prover);
    prover->pk->users--;
  }
  h2mi_sync();
  delete prover;
  return H2MI_OK;
}

int h2mi_prover_set_combiner(h2mi_prover_t prover, void* d_partial, void* d_combined, h2mi_combine_fn combine, void* ctx) {
  if (!alive(g_live_provers, prover)) return H2MI_EHANDLE;
  if (!d_partial && !d_combined && !combine) {  // back to whole-SRS commitments
    prover->d_partial = prover->d_combined = nullptr;
    prover->combine = nullptr;
    return H2MI_OK;
  }
  if (!d_partial || !d_combined || !combine) return H2MI_EINVAL;
  prover->d_partial = d_partial;
  prover->d_combined = d_combined;
  prover->combine = combine;
  prover->combine_ctx = ctx;
  return H2MI_OK;
}

int h2mi_prover_set_rng_key(h2mi_prover_t prover, const uint8_t key[32]) {
  if (!alive(g_live_provers, prover)) return H2MI_EHANDLE;
  prover->keyed = key != nullptr;
  if (key) std::memcpy(prover->key, key, 32);
  else std::memset(prover->key, 0, 32);
  prover->phase = IDLE;  // a proof in flight would mix two sources
  return H2MI_OK;
}

int h2mi_prover_get_counts(h2mi_prover_t prover, h2mi_prover_counts* out) {
  if (!alive(g_live_provers, prover)) return H2MI_EHANDLE;
  if (!out) return H2MI_EINVAL;
  const h2mi_pk_s& pk = *prover->pk;
  out->advice = pk.cs.n_advice;
  out->lookups = (pk.logup ? 1 : 2) * pk.cs.n_lookups;
  out->products = pk.n_sets + pk.cs.n_lookups + pk.n_shuffles + (prover->draws_random() ? 1 : 0);
  out->quotient = pk.cs.degree - 1;
  out->evaluations = (uint32_t)num_evaluations(pk);
  return H2MI_OK;
}

int h2mi_prover_instances(h2mi_prover_t prover, const h2mi_column_cells* instance) {
  if (!alive(g_live_provers, prover)) return H2MI_EHANDLE;
  h2mi_prover_s& p = *prover;
  p.pending_instances.clear();  // a refusal leaves nothing behind: the next proof's columns are then empty
  p.have_pending_instances = false;
  const h2mi_constraint_system& cs = p.pk->cs;
  if (cs.n_instance && !instance) return H2MI_EINVAL;
  return guarded([&] {
    check_cells(instance, cs.n_instance, H2MI_CELLS_FOR_INSTANCE);
    std::vector<std::vector<Fr>> cols(cs.n_instance);
    for (uint32_t i = 0; i < cs.n_instance; i++) {
      const h2mi_column_cells& c = instance[i];
      if (c.rows) throw Error(H2MI_EINVAL, "an instance column's values lie on rows 0 .. count - 1");
      if (c.flags & H2MI_CELLS_RATIONAL) throw Error(H2MI_EINVAL, "public inputs are field elements, not rational cells");
      if (c.count && !c.values) throw Error(H2MI_EINVAL, "column cells without values");
      if (c.count > p.pk->u) throw Error(H2MI_ERANGE, "more public inputs than usable rows (InstanceTooLarge)");
      cols[i].resize(c.count);
      for (size_t r = 0; r < c.count; r++) cols[i][r] = cell_value(c, r);
    }
    p.pending_instances.swap(cols);
    p.have_pending_instances = true;
  });
}
int h2mi_prover_advice(h2mi_prover_t prover, const h2mi_column_cells* advice, const uint64_t* instance, size_t n_instance_values, uint64_t seed,
                       uint64_t* points_out) {
  if (!alive(g_live_provers, prover)) return H2MI_EHANDLE;
  if (!advice) return H2MI_EINVAL;
  if (prover->pk->phases.n_phases > 1) {  // the advice of such a key is committed phase by phase
    prover->phase = IDLE;
    prover->pending_instances.clear();
    prover->have_pending_instances = false;
    return H2MI_EINVAL;
  }
  return guarded([&] { phase_advice(*prover, 0, advice, instance, n_instance_values, seed, points_out); });
}
int h2mi_prover_advice_phase(h2mi_prover_t prover, uint32_t phase, const h2mi_column_cells* advice, const uint64_t* instance, size_t n_instance_values,
                             uint64_t seed, uint64_t* points_out) {
  if (!alive(g_live_provers, prover)) return H2MI_EHANDLE;
  if (!advice) return H2MI_EINVAL;
  return guarded([&] { phase_advice(*prover, phase, advice, instance, n_instance_values, seed, points_out); });
}
int h2mi_prover_set_challenges(h2mi_prover_t prover, const uint64_t* values) {
  if (!alive(g_live_provers, prover)) return H2MI_EHANDLE;
  const uint32_t nc = prover->pk->phases.n_challenges;
  if (prover->phase != ADVICE || (nc && !values)) {
    prover->phase = IDLE;
    return H2MI_EINVAL;
  }
  prover->challenges.resize(nc);
  if (nc) std::memcpy(prover->challenges.data(), values, (size_t)nc * 32);
  prover->have_challenges = true;
  return H2MI_OK;
}
int h2mi_prover_get_phase_counts(h2mi_prover_t prover, h2mi_prover_phase_counts* out) {
  if (!alive(g_live_provers, prover)) return H2MI_EHANDLE;
  if (!out) return H2MI_EINVAL;
  const h2mi_pk_s& pk = *prover->pk;
  std::memset(out, 0, sizeof(*out));
  out->n_phases = pk.phases.n_phases;
  out->n_challenges = pk.phases.n_challenges;
  for (uint32_t p = 0; p < pk.phases.n_phases; p++) out->advice[p] = pk.phase_columns[p];
  for (uint32_t i = 0; i < pk.phases.n_challenges; i++) out->challenges[pk.phases.challenge_phase[i]]++;
  return H2MI_OK;
}
int h2mi_prover_lookups(h2mi_prover_t prover, const uint64_t theta[4], uint64_t* points_out) {
  if (!alive(g_live_provers, prover)) return H2MI_EHANDLE;
  return guarded([&] { phase_lookups(*prover, theta, points_out); });  // theta compresses lookups given as expressions only
}
int h2mi_prover_check(h2mi_prover_t prover, const uint64_t theta[4], h2mi_check_failure* out, size_t cap, size_t* n_out) {
  if (!alive(g_live_provers, prover)) return H2MI_EHANDLE;
  if (!n_out || (cap && !out)) return H2MI_EINVAL;
  *n_out = 0;
  std::vector<h2mi_check_failure> found;
  const int rc = guarded([&] { found = run_check(*prover, theta); });
  if (rc) return rc;
  *n_out = found.size();
  for (size_t i = 0; i < found.size() && i < cap; i++) out[i] = found[i];
  return found.empty() ? H2MI_OK : H2MI_EUNSAT;
}
int h2mi_prover_products(h2mi_prover_t prover, const uint64_t beta[4], const uint64_t gamma[4], uint64_t* points_out) {
  if (!alive(g_live_provers, prover)) return H2MI_EHANDLE;
  if (!beta || !gamma) return H2MI_EINVAL;
  return guarded([&] { phase_products(*prover, load_fr(beta), load_fr(gamma), points_out); });
}
int h2mi_prover_quotient(h2mi_prover_t prover, const uint64_t y[4], uint64_t* points_out) {
  if (!alive(g_live_provers, prover)) return H2MI_EHANDLE;
  if (!y || prover->batch) return H2MI_EINVAL;  // a bound member's joint phases are its batch's: nothing is abandoned
  return guarded([&] { phase_quotient({prover}, load_fr(y), points_out); });
}
int h2mi_prover_num_evaluations(h2mi_prover_t prover, size_t* count_out) {
  if (!alive(g_live_provers, prover)) return H2MI_EHANDLE;
  if (!count_out) return H2MI_EINVAL;
  *count_out = num_evaluations(*prover->pk);
  return H2MI_OK;
}
int h2mi_prover_evaluations(h2mi_prover_t prover, const uint64_t x[4], uint64_t* evals_out) {
  if (!alive(g_live_provers, prover)) return H2MI_EHANDLE;
  if (!x || prover->batch) return H2MI_EINVAL;
  return guarded([&] { phase_evaluations({prover}, load_fr(x), evals_out); });
}
int h2mi_prover_shplonk_quotient(h2mi_prover_t prover, const uint64_t y[4], const uint64_t v[4], uint64_t point_out[8]) {
  if (!alive(g_live_provers, prover)) return H2MI_EHANDLE;
  if (!y || !v || prover->batch) return H2MI_EINVAL;
  return guarded([&] { phase_shplonk_quotient({prover}, load_fr(y), load_fr(v), point_out); });
}
int h2mi_prover_shplonk_open(h2mi_prover_t prover, const uint64_t u[4], uint64_t point_out[8]) {
  if (!alive(g_live_provers, prover)) return H2MI_EHANDLE;
  if (!u || prover->batch) return H2MI_EINVAL;
  return guarded([&] { phase_shplonk_open({prover}, load_fr(u), point_out); });
}
int h2mi_prover_gwc_num_points(h2mi_prover_t prover, size_t* count_out) {
  if (!alive(g_live_provers, prover)) return H2MI_EHANDLE;
  if (!count_out) return H2MI_EINVAL;
  *count_out = gwc_num_points(*prover->pk);
  return H2MI_OK;
}
int h2mi_prover_gwc_open(h2mi_prover_t prover, const uint64_t v[4], uint64_t* points_out) {
  if (!alive(g_live_provers, prover)) return H2MI_EHANDLE;
  if (!v || prover->batch) return H2MI_EINVAL;
  return guarded([&] { phase_gwc_open({prover}, load_fr(v), points_out); });
}

// ---- several circuits per proof ----------------------------------------------------------------------------------------------------
int h2mi_batch_create(const h2mi_prover_t* members, uint32_t n, h2mi_batch_t* batch_out) {
  if (!batch_out) return H2MI_EINVAL;
  *batch_out = nullptr;
  if (!members || n == 0 || n > H2MI_MAX_CIRCUITS) return H2MI_EINVAL;
  std::lock_guard<std::mutex> lk(g_reg_mu);
  for (uint32_t i = 0; i < n; i++) {
    const h2mi_prover_s* m = members[i];
    if (!m || !g_live_provers.count(m)) return H2MI_EHANDLE;
    const h2mi_prover_s* m0 = members[0];
    if (m->batch || m->phase != IDLE) return H2MI_EINVAL;  // bound already, or a proof in flight
    if (m->pk != m0->pk || m->g != m0->g || m->gl != m0->gl || m->lo != m0->lo || m->cnt != m0->cnt) return H2MI_EINVAL;
    for (uint32_t j = 0; j < i; j++)
      if (members[j] == m) return H2MI_EINVAL;
  }
  h2mi_batch_s* b = new (std::nothrow) h2mi_batch_s;
  if (!b) return H2MI_ENOMEM;
  b->members.assign(members, members + n);
  for (uint32_t i = 0; i < n; i++) {
    members[i]->batch = b;
    members[i]->batch_index = i;
  }
  g_live_batches.insert(b);
  *batch_out = b;
  return H2MI_OK;
}

int h2mi_batch_destroy(h2mi_batch_t batch) {
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    if (!batch || !g_live_batches.erase(batch)) return H2MI_EHANDLE;
    for (h2mi_prover_s* m : batch->members) {  // ordinary provers again; a proof in flight is abandoned
      m->batch = nullptr;
      m->batch_index = 0;
      m->phase = IDLE;
    }
  }
  delete batch;
  return H2MI_OK;
}

int h2mi_batch_quotient(h2mi_batch_t batch, const uint64_t y[4], uint64_t* points_out) {
  if (!alive(g_live_batches, batch)) return H2MI_EHANDLE;
  if (!y) return H2MI_EINVAL;
  const Circuits& all = batch->members;
  // what makes N circuits one proof, checked before anything is touched: a refusal here abandons nothing
  for (const h2mi_prover_s* m : all) {
    const h2mi_prover_s& m0 = *all[0];
    if (m->phase != PRODUCTS) return H2MI_EINVAL;
    if (!(m->beta == m0.beta) || !(m->gamma == m0.gamma)) return H2MI_EINVAL;
    if (m->pk->phases.n_challenges && !std::equal(m->challenges.begin(), m->challenges.end(), m0.challenges.begin(), m0.challenges.end())) return H2MI_EINVAL;
  }
  // blinding streams that could overlap would open two columns with the same blinding: seeded streams are seed + purpose (1 .. 6),
  // keyed ones nonce << 3 | purpose under the key
  for (size_t i = 0; i < all.size(); i++)
    for (size_t j = 0; j < i; j++) {
      const h2mi_prover_s &a = *all[i], &b = *all[j];
      if (a.keyed != b.keyed) continue;
      if (a.keyed ? (!std::memcmp(a.key, b.key, 32) && a.seed == b.seed) : (a.seed > b.seed ? a.seed - b.seed : b.seed - a.seed) < 8) return H2MI_EINVAL;
    }
  return guarded([&] { phase_quotient(all, load_fr(y), points_out); });
}
int h2mi_batch_num_evaluations(h2mi_batch_t batch, size_t* count_out) {
  if (!alive(g_live_batches, batch)) return H2MI_EHANDLE;
  if (!count_out) return H2MI_EINVAL;
  *count_out = num_evaluations(*batch->members[0]->pk, batch->members.size());
  return H2MI_OK;
}
int h2mi_batch_evaluations(h2mi_batch_t batch, const uint64_t x[4], uint64_t* evals_out) {
  if (!alive(g_live_batches, batch)) return H2MI_EHANDLE;
  if (!x) return H2MI_EINVAL;
  return guarded([&] { phase_evaluations(batch->members, load_fr(x), evals_out); });
}
int h2mi_batch_shplonk_quotient(h2mi_batch_t batch, const uint64_t y[4], const uint64_t v[4], uint64_t point_out[8]) {
  if (!alive(g_live_batches, batch)) return H2MI_EHANDLE;
  if (!y || !v) return H2MI_EINVAL;
  return guarded([&] { phase_shplonk_quotient(batch->members, load_fr(y), load_fr(v), point_out); });
}
int h2mi_batch_shplonk_open(h2mi_batch_t batch, const uint64_t u[4], uint64_t point_out[8]) {
  if (!alive(g_live_batches, batch)) return H2MI_EHANDLE;
  if (!u) return H2MI_EINVAL;
  return guarded([&] { phase_shplonk_open(batch->members, load_fr(u), point_out); });
}
int h2mi_batch_gwc_num_points(h2mi_batch_t batch, size_t* count_out) {
  if (!alive(g_live_batches, batch)) return H2MI_EHANDLE;
  if (!count_out) return H2MI_EINVAL;
  *count_out = gwc_num_points(*batch->members[0]->pk);
  return H2MI_OK;
}
int h2mi_batch_gwc_open(h2mi_batch_t batch, const uint64_t v[4], uint64_t* points_out) {
  if (!alive(g_live_batches, batch)) return H2MI_EHANDLE;
  if (!v) return H2MI_EINVAL;
  return guarded([&] { phase_gwc_open(batch->members, load_fr(v), points_out); });
}

int h2mi_prover_buffer(h2mi_prover_t prover, uint32_t kind, uint32_t index, void** d_ptr_out, size_t* count_out) {
  if (!alive(g_live_provers, prover)) return H2MI_EHANDLE;
  if (!d_ptr_out) return H2MI_EINVAL;
  h2mi_prover_s& p = *prover;
  auto form = [&](std::vector<Forms>& v, int which) -> int {
    if (which == 2 && p.pk->by_coset) return H2MI_EINVAL;  // a slice is no extended coset
    if (index >= v.size()) return H2MI_ERANGE;
    const Dev& d = which == 0 ? v[index].value : which == 1 ? v[index].poly : v[index].coset;
    return pick(d, 0, d_ptr_out, count_out);
  };
  switch (kind) {
    case H2MI_BUF_ADVICE: return form(p.advice, 0);
    case H2MI_BUF_ADVICE_POLY: return form(p.advice, 1);
    case H2MI_BUF_ADVICE_COSET: return form(p.advice, 2);
    case H2MI_BUF_INSTANCE: return pick(p.instance, index, d_ptr_out, count_out);
    case H2MI_BUF_PERM_Z: return form(p.z, 0);
    case H2MI_BUF_PERM_Z_POLY: return form(p.z, 1);
    case H2MI_BUF_PERM_Z_COSET: return form(p.z, 2);
    case H2MI_BUF_LOOKUP_PERMUTED_INPUT: return index < p.pk->cs.n_lookups ? pick(p.lk[index].a.value, 0, d_ptr_out, count_out) : H2MI_ERANGE;
    case H2MI_BUF_LOOKUP_PERMUTED_TABLE: return index < p.pk->cs.n_lookups ? pick(p.lk[index].s.value, 0, d_ptr_out, count_out) : H2MI_ERANGE;
    case H2MI_BUF_LOOKUP_Z: return index < p.pk->cs.n_lookups ? pick(p.lk[index].z.value, 0, d_ptr_out, count_out) : H2MI_ERANGE;
    case H2MI_BUF_RANDOM_POLY: return pick(p.random_poly, index, d_ptr_out, count_out);
    case H2MI_BUF_H: return pick(p.h, index, d_ptr_out, count_out);
    case H2MI_BUF_H_POLY: return pick(p.h_poly, index, d_ptr_out, count_out);
    case H2MI_BUF_SHPLONK_H: return pick(p.h_x, index, d_ptr_out, count_out);
    case H2MI_BUF_SHPLONK_H2: return pick(p.h2_x, index, d_ptr_out, count_out);
    case H2MI_BUF_SHUFFLE_Z: return index < p.pk->n_shuffles ? pick(p.sf[index].z.value, 0, d_ptr_out, count_out) : H2MI_ERANGE;
    case H2MI_BUF_SHUFFLE_Z_POLY: return index < p.pk->n_shuffles ? pick(p.sf[index].z.poly, 0, d_ptr_out, count_out) : H2MI_ERANGE;
    case H2MI_BUF_SHUFFLE_INPUT: return index < p.pk->n_shuffles ? pick(p.sf[index].c.input, 0, d_ptr_out, count_out) : H2MI_ERANGE;
    case H2MI_BUF_LOGUP_M: return p.pk->logup && index < p.pk->cs.n_lookups ? pick(p.lk[index].a.value, 0, d_ptr_out, count_out) : H2MI_ERANGE;
    case H2MI_BUF_LOGUP_PHI: return p.pk->logup && index < p.pk->cs.n_lookups ? pick(p.lk[index].z.value, 0, d_ptr_out, count_out) : H2MI_ERANGE;
    case H2MI_BUF_SHUFFLE_TABLE: return index < p.pk->n_shuffles ? pick(p.sf[index].c.table, 0, d_ptr_out, count_out) : H2MI_ERANGE;
    case H2MI_BUF_GWC_W: return index < gwc_num_points(*p.pk) ? pick(index % 2 ? p.s : p.q, index / 2, d_ptr_out, count_out) : H2MI_ERANGE;
    default: return h2mi_prover_pk_buffer(p.pk, kind, index, d_ptr_out, count_out);
  }
}

int h2mi_prover_device_bytes(h2mi_prover_t prover, size_t* key_bytes_out, size_t* prover_bytes_out) {
  if (!alive(g_live_provers, prover)) return H2MI_EHANDLE;
  const h2mi_prover_s& p = *prover;
  const h2mi_pk_s& pk = *p.pk;
  size_t total = 0;
  auto one = [&](const Dev& d) { total += d ? d->n * 32 : 0; };
  auto many = [&](const std::vector<Dev>& v) { for (const Dev& d : v) one(d); };
  auto forms = [&](const Forms& f) { one(f.value); one(f.poly); one(f.coset); };
  auto table = [&](const Table& t) { one(t.sorted); one(t.sorted_mont); one(t.mult); one(t.first); };
  many(pk.fixed_values); many(pk.fixed_polys); many(pk.fixed_cosets); many(pk.sigma_values); many(pk.sigma_polys); many(pk.sigma_cosets);
  for (const Dev* d : {&pk.l0, &pk.l_last, &pk.l_active, &pk.l0_poly, &pk.l_last_poly, &pk.l_active_poly, &pk.active_rows, &pk.moved_cells_dev}) one(*d);
  for (const Table& t : pk.tables) table(t);
  if (key_bytes_out) *key_bytes_out = total;
  total = 0;
  for (const Forms& f : p.advice) forms(f);
  for (const Forms& f : p.z) forms(f);
  many(p.instance); many(p.instance_poly); many(p.instance_coset); many(p.fixed_slices); many(p.sigma_slices); many(p.q); many(p.s);
  for (const h2mi_prover_s::Lk& l : p.lk) {
    for (const Dev* d : {&l.c.input, &l.c.table, &l.c.in_coset, &l.c.tab_coset}) one(*d);
    forms(l.a); forms(l.s); forms(l.z);
    table(l.sorted);
    one(l.ranks); one(l.counts);  // a table-logUp key: 4 bytes per input and row, 4 per distinct table value (rounded up to 32 bytes)
  }
  for (const h2mi_prover_s::Sf& f : p.sf) {
    for (const Dev* d : {&f.c.input, &f.c.table, &f.c.in_coset, &f.c.tab_coset}) one(*d);
    forms(f.z);
  }
  for (const Dev* d : {&p.l0_slice, &p.l_last_slice, &p.l_active_slice, &p.check_in, &p.check_tab, &p.random_poly, &p.h, &p.h_poly, &p.points, &p.evals,
                       &p.nx[0], &p.nx[1], &p.nx[2], &p.tmp[0], &p.tmp[1], &p.tmp[2], &p.h_x, &p.l_x, &p.h2_x})
    one(*d);
  table(p.check_sorted); table(p.check_sorted_in);
  if (prover_bytes_out) *prover_bytes_out = total;
  return H2MI_OK;
}

int h2mi_prover_pk_buffer(h2mi_pk_t pk, uint32_t kind, uint32_t index, void** d_ptr_out, size_t* count_out) {
  if (!alive(g_live_pks, pk)) return H2MI_EHANDLE;
  if (!d_ptr_out) return H2MI_EINVAL;
  if (pk->by_coset && (kind == H2MI_PKBUF_FIXED_COSET || kind == H2MI_PKBUF_SIGMA_COSET || kind == H2MI_PKBUF_L0_COSET || kind == H2MI_PKBUF_L_LAST_COSET ||
                       kind == H2MI_PKBUF_L_ACTIVE_COSET))
    return H2MI_EINVAL;  // the key holds no extended-coset vector
  switch (kind) {
    case H2MI_PKBUF_FIXED: return pick(pk->fixed_values, index, d_ptr_out, count_out);
    case H2MI_PKBUF_FIXED_POLY: return pick(pk->fixed_polys, index, d_ptr_out, count_out);
    case H2MI_PKBUF_FIXED_COSET: return pick(pk->fixed_cosets, index, d_ptr_out, count_out);
    case H2MI_PKBUF_SIGMA: return pick(pk->sigma_values, index, d_ptr_out, count_out);
    case H2MI_PKBUF_SIGMA_POLY: return pick(pk->sigma_polys, index, d_ptr_out, count_out);
    case H2MI_PKBUF_SIGMA_COSET: return pick(pk->sigma_cosets, index, d_ptr_out, count_out);
    case H2MI_PKBUF_L0_COSET: return pick(pk->l0, index, d_ptr_out, count_out);
    case H2MI_PKBUF_L_LAST_COSET: return pick(pk->l_last, index, d_ptr_out, count_out);
    case H2MI_PKBUF_L_ACTIVE_COSET: return pick(pk->l_active, index, d_ptr_out, count_out);
    default: return H2MI_EINVAL;
  }
}

}  // extern "C"
