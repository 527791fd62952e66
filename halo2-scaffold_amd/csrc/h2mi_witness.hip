// libh2mi.so — witness programs: a builder closure recorded once as a tape, evaluated on the device for every proof (h2mi_witness_*,
// include/h2mi.h).
//
// A program is one op per cell of the closure's flat cell list (INPUT, CONST, COPY, GATE, LIMB), sorted into levels: an op reads only
// cells of lower levels, so a level is one parallel step.  k_witness_level runs one wide level with a lane per op; k_witness_levels_wg
// runs a run of consecutive narrow levels in ONE workgroup with a barrier between levels (a deep, narrow circuit would otherwise be a
// launch per level); k_witness_place gathers the cells into the dense Montgomery columns h2mi_prover_advice takes as H2MI_CELLS_DEVICE
// and, in the same launch, evaluates the equality checks no COPY op makes true.
// Algorithmic bytes: k_witness_level moves per cell the 16-byte op, the operands (GATE: three 32-byte cells; COPY, LIMB, INPUT, CONST:
// one) and one 32-byte store — 16 + 96 + 32 = 144 bytes for a GATE, 16 + 32 + 32 = 80 for every other kind; k_witness_place moves
// 4 + 32 + 32 = 68 bytes per placed cell and 8 + 64 per check.  Against that stand at most two Montgomery products per cell, so in the
// limit the kernels are bound by memory traffic like k_cells_scatter (h2mi_cells.hip), and they are shaped like it: a lane owns a cell
// and moves its word as two 16-byte accesses (fe_load / fe_store).  The operand gathers are as scattered as the closure makes them.
// Measured: a level of 180 000 ops is 12.6 us, 14 % of the HBM roofline on these bytes — latency-bound at that size.
// The columns of a program lie behind one another in one buffer, so the gather needs no search for its column: placed cell e of the
// concatenated placement lands at word e.  The arithmetic is the fp.cuh layer's: canonical -> Montgomery is the product with R^2,
// Montgomery -> canonical the product with 1.
// Hint ops (DIVQ, DIVR, ISZERO, INV, MSB, POW2: the values halo2-base computes outside the gates — quotients, remainders, is-zero flags,
// inverses, the index of a value's highest set bit and a power of two chosen by a cell)
// live in a second instantiation of the two level kernels, k_witness_level_hints / k_witness_levels_wg_hints, launched for the programs
// that hold one; a program without them runs the kernels it always ran.  Division is restoring long division on the canonical words,
// one quotient bit per round: dividend and remainder shift left as one 512-bit register (16 shifts), the divisor is subtracted with
// borrow (8) and the difference taken where it did not borrow (8 selects, the quotient bit enters the dividend's low word) — about 36
// instructions a round, 256 rounds, ~9 k instructions per op, beside one product out of Montgomery form per cell operand and one back
// in.  Nothing cleverer is needed for a value computed once per lane: the inversion beside it (fe_inv_ds, ~15 k instructions, out of
// line as everywhere it is used) costs more.  A signed dividend (above 2^252: the fixed-point chip's negative numbers) is divided as
// its magnitude r - x and the quotient rounded toward minus infinity afterwards.  MSB is a count of leading zeros on the highest nonzero
// canonical word; POW2 builds its one-bit word with a select per word, as LIMB picks its words (an indexed register array would go to
// scratch): both are a product out of Montgomery form, a dozen instructions and a product back in.
#include <algorithm>
#include <memory>
#include <set>
#include <utility>

#include "fp.cuh"
#include "h2mi_fr_tables.h"

namespace h2 {

constexpr uint32_t WP_INPUT = 0, WP_CONST = 1, WP_COPY = 2, WP_GATE = 3, WP_LIMB = 4;  // H2MI_WITNESS_*
constexpr uint32_t WP_DIVQ = 8, WP_DIVR = 9, WP_ISZERO = 10, WP_INV = 11;  // the hint ops; 5 .. 7 stay unassigned
constexpr uint32_t WP_MSB = 13, WP_POW2 = 14;                              // 12 is reserved
constexpr uint32_t WP_DIV_CONST = 1, WP_DIV_SIGNED = 2;                     // H2MI_WITNESS_DIV_*: the flags of DIVQ / DIVR, in the bits byte
constexpr uint32_t WP_POW2_OF_MSB = 1;                                      // H2MI_WITNESS_POW2_OF_MSB: the flag of POW2, in the bits byte
constexpr uint32_t WP_BLOCK = 256;
constexpr uint32_t WP_WG = 1024;         // H2MI_WITNESS_WG_OPS: the workgroup limit
constexpr uint32_t WP_WG_LEVELS = 4096;  // H2MI_WITNESS_WG_LEVELS
constexpr uint32_t WP_NO_FAILURE = 0xffffffffu;

// x / y and x mod y of plain 256-bit integers by restoring long division, y != 0: (rem : x) shifts left one bit a round, the quotient
// bit enters x's low word.  rem < y <= 2^256 - 1 before every shift; the bit shifted out of rem's top word joins the comparison.
__device__ __forceinline__ void divmod_256(fe& x, const fe& y, fe& rem) {
  rem = fe_zero();
  for (uint32_t round = 0; round < 256; round++) {
    const uint32_t out = rem.v[7] >> 31;
#pragma unroll
    for (int i = 7; i > 0; i--) rem.v[i] = (rem.v[i] << 1) | (rem.v[i - 1] >> 31);
    rem.v[0] = (rem.v[0] << 1) | (x.v[7] >> 31);
#pragma unroll
    for (int i = 7; i > 0; i--) x.v[i] = (x.v[i] << 1) | (x.v[i - 1] >> 31);
    x.v[0] <<= 1;
    uint32_t borrow;
    const fe d = raw_sub(rem, y, borrow);
    const bool take = out || !borrow;
    rem = fe_select(take, d, rem);
    x.v[0] |= take ? 1u : 0u;
  }
}

// DIVQ / DIVR of include/h2mi.h on canonical words -> the canonical result
__device__ __forceinline__ fe witness_div(fe x, const fe& y, bool want_q, bool is_signed) {
  const fe zero = fe_zero();
  uint32_t low = 0;
#pragma unroll
  for (int i = 0; i < 7; i++) low |= x.v[i];
  const bool neg = is_signed && (x.v[7] > 0x10000000u || (x.v[7] == 0x10000000u && low != 0));  // x > 2^252: read as x - r
  const fe mod = fe_const<Fr>(Fr::MOD);
  uint32_t bo;
  if (neg) x = raw_sub(mod, x, bo);  // the magnitude, 0 < r - x < r
  fe rem;
  divmod_256(x, y, rem);  // x is the quotient now
  if (neg) {              // floor(-m / y) = -(m / y) - (m mod y != 0); the remainder y - m mod y, or 0
    const bool exact = fe_is_zero(rem);
    fe one = zero;
    one.v[0] = exact ? 0u : 1u;
    uint32_t carry;
    x = raw_sub(mod, raw_add(x, one, carry), bo);  // ceil(m / y) is in 1 .. m: r minus it is in [0, r)
    rem = fe_select(exact, rem, raw_sub(y, rem, bo));
  }
  const fe r = want_q ? x : rem;
  return fe_select(fe_is_zero(y), zero, r);
}

// the index of the highest set bit of a canonical word, 0 .. 253; 1 for zero (MSB of include/h2mi.h)
__device__ __forceinline__ uint32_t msb_256(const fe& x) {
  uint32_t idx = 1;
#pragma unroll
  for (uint32_t i = 0; i < 8; i++)  // the highest nonzero word is the last to write
    if (x.v[i]) idx = 32 * i + 31 - (uint32_t)__clz((int)x.v[i]);
  return idx;
}

// MSB / POW2 of include/h2mi.h on the canonical word -> the canonical result
__device__ __forceinline__ fe witness_bit(const fe& x, bool want_pow2, bool of_msb) {
  uint32_t high = 0;
#pragma unroll
  for (int i = 1; i < 8; i++) high |= x.v[i];
  const uint32_t msb = msb_256(x);
  const uint32_t e = of_msb ? msb : x.v[0];
  const bool in_table = of_msb || (high == 0 && e <= 253);  // 2^253 < r < 2^254
  fe r = fe_zero();
  if (!want_pow2) {
    r.v[0] = msb;
    return r;
  }
  const uint32_t w = e >> 5, bit = in_table ? 1u << (e & 31u) : 0u;
#pragma unroll
  for (uint32_t i = 0; i < 8; i++) r.v[i] = i == w ? bit : 0u;  // selects, not an indexed register array
  return r;
}

// the hint ops: the values a builder computes outside the gates (include/h2mi.h)
__device__ __forceinline__ void witness_hint(const uint4 op, uint32_t kind, fe* cells, const fe* consts) {
  const fe x = fe_load(cells + op.z);
  fe r;
  if (kind == WP_ISZERO) {
    r = fe_is_zero(x) ? fe_one<Fr>() : fe_zero();  // reduced: zero is the zero word
  } else if (kind == WP_INV) {
    r = fe_is_zero(x) ? fe_one<Fr>() : fe_inv_ds<Fr>(x);
  } else if (kind >= WP_MSB) {
    r = fe_to_mont<Fr>(witness_bit(fe_from_mont<Fr>(x), kind == WP_POW2, ((op.y >> 8) & WP_POW2_OF_MSB) != 0));
  } else {
    const uint32_t flags = (op.y >> 8) & 0xffu;
    const fe y = (flags & WP_DIV_CONST) ? fe_load(consts + op.w) : fe_from_mont<Fr>(fe_load(cells + op.w));  // the constants are canonical
    r = fe_to_mont<Fr>(witness_div(fe_from_mont<Fr>(x), y, kind == WP_DIVQ, (flags & WP_DIV_SIGNED) != 0));
  }
  fe_store(cells + op.x, r);
}

// op = (dst, kind | bits << 8 | shift << 16, a, b).  Every index was checked on the host (h2mi_witness_check): nothing here can reach
// outside cells[0 .. n_cells), values[0 .. n_inputs) or consts[0 .. n_constants).  HINTS: the instantiation that also knows the hint ops.
template <bool HINTS>
__device__ __forceinline__ void witness_op(const uint4 op, fe* cells, const fe* values, const fe* consts) {
  const uint32_t dst = op.x, kind = op.y & 0xffu;
  if constexpr (HINTS) {
    if (kind >= WP_DIVQ) {
      witness_hint(op, kind, cells, consts);
      return;
    }
  }
  if (kind == WP_COPY) {
    fe_store(cells + dst, fe_load(cells + op.z));
    return;
  }
  // one product serves every other kind: GATE b * c, LIMB cell * 1 (out of Montgomery form), INPUT / CONST value * R^2 (into it)
  fe x, y = fe_zero(), acc = fe_zero();
  y.v[0] = 1;
  if (kind == WP_GATE) {
    acc = fe_load(cells + dst - 3);
    x = fe_load(cells + dst - 2);
    y = fe_load(cells + dst - 1);
  } else if (kind == WP_LIMB) {
    x = fe_load(cells + op.z);
  } else {
    x = fe_load((kind == WP_INPUT ? values : consts) + op.z);
    y = fe_const<Fr>(Fr::R2);
  }
  fe r = fe_mul<Fr>(x, y);
  if (kind == WP_GATE) {
    r = fe_add<Fr>(acc, r);
  } else if (kind == WP_LIMB) {  // bits [shift, shift + bits) of the canonical word: at most 64 of them, out of at most three 32-bit words
    const uint32_t bits = (op.y >> 8) & 0xffu, shift = (op.y >> 16) & 0xffu;
    const uint32_t w = shift >> 5, off = shift & 31u;
    uint32_t x0 = 0, x1 = 0, x2 = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) {  // selects, not an indexed register array
      if (i == w) x0 = r.v[i];
      if (i == w + 1) x1 = r.v[i];
      if (i == w + 2) x2 = r.v[i];
    }
    unsigned long long v = ((unsigned long long)x1 << 32) | x0;
    if (off) v = (v >> off) | ((unsigned long long)x2 << (64 - off));
    if (bits < 64) v &= (1ull << bits) - 1ull;
    fe limb = fe_zero();
    limb.v[0] = (uint32_t)v;
    limb.v[1] = (uint32_t)(v >> 32);
    r = fe_to_mont<Fr>(limb);
  }
  fe_store(cells + dst, r);
}

// one wide level: a lane per op
__global__ void __launch_bounds__(WP_BLOCK) k_witness_level(const uint4* ops, uint32_t count, fe* cells, const fe* values, const fe* consts) {
  const uint32_t e = blockIdx.x * WP_BLOCK + threadIdx.x;
  if (e < count) witness_op<false>(ops[e], cells, values, consts);
}
__global__ void __launch_bounds__(WP_BLOCK) k_witness_level_hints(const uint4* ops, uint32_t count, fe* cells, const fe* values, const fe* consts) {
  const uint32_t e = blockIdx.x * WP_BLOCK + threadIdx.x;
  if (e < count) witness_op<true>(ops[e], cells, values, consts);
}

// levels l0 .. l1 - 1, none of more than WP_WG ops, in ONE workgroup: a level's stores are visible to the next level's loads behind the
// barrier (the workgroup's waves share one L1; __syncthreads() carries the workgroup-scope release and acquire)
__global__ void __launch_bounds__(WP_WG) k_witness_levels_wg(const uint4* ops, const uint32_t* level_ends, uint32_t l0, uint32_t l1, fe* cells,
                                                             const fe* values, const fe* consts) {
  uint32_t begin = l0 ? level_ends[l0 - 1] : 0u;
  for (uint32_t l = l0; l < l1; l++) {  // uniform trip count: every thread reaches every barrier
    const uint32_t end = level_ends[l];
    if (end - begin <= WP_WG && threadIdx.x < end - begin) witness_op<false>(ops[begin + threadIdx.x], cells, values, consts);
    begin = end;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(WP_WG) k_witness_levels_wg_hints(const uint4* ops, const uint32_t* level_ends, uint32_t l0, uint32_t l1, fe* cells,
                                                             const fe* values, const fe* consts) {
  uint32_t begin = l0 ? level_ends[l0 - 1] : 0u;
  for (uint32_t l = l0; l < l1; l++) {  // uniform trip count: every thread reaches every barrier
    const uint32_t end = level_ends[l];
    if (end - begin <= WP_WG && threadIdx.x < end - begin) witness_op<true>(ops[begin + threadIdx.x], cells, values, consts);
    begin = end;
    __syncthreads();
  }
}

// the gather into the dense columns (placed cell e -> word e of the column buffer), then the checks: status = the lowest failing index
__global__ void __launch_bounds__(WP_BLOCK) k_witness_place(const fe* cells, const uint32_t* src, uint64_t n_placed, fe* columns, const uint2* checks,
                                                            uint32_t n_checks, uint32_t* status) {
  const uint64_t e = (uint64_t)blockIdx.x * WP_BLOCK + threadIdx.x;
  if (e < n_placed) {
    fe_store(columns + e, fe_load(cells + src[e]));
    return;
  }
  const uint64_t i = e - n_placed;
  if (i >= n_checks) return;
  const uint2 c = checks[i];
  if (!fe_eq(fe_load(cells + c.x), fe_load(cells + c.y))) atomicMin(status, (uint32_t)i);  // both reduced: equal values are equal words
}

// canonical values of listed cells (h2mi_witness_read)
__global__ void __launch_bounds__(WP_BLOCK) k_witness_read(const fe* cells, const uint32_t* idx, uint32_t n, fe* out) {
  const uint32_t e = blockIdx.x * WP_BLOCK + threadIdx.x;
  if (e < n) fe_store(out + e, fe_from_mont<Fr>(fe_load(cells + idx[e])));
}

static bool below_r(const uint64_t* w) {
  static const uint64_t r[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
  for (int i = 3; i >= 0; i--)
    if (w[i] != r[i]) return w[i] < r[i];
  return false;
}

static int witness_check(const h2mi_witness_desc* d) {
  if (!d) return H2MI_EINVAL;
  if (d->n_ops > ((uint64_t)1 << H2MI_MAX_LOG_N) || d->n_columns > H2MI_WITNESS_MAX_COLUMNS) return H2MI_ERANGE;
  if ((d->n_ops && (!d->ops || !d->level_ends)) || (d->n_constants && !d->constants) || (d->n_checks && !d->checks) || (d->n_columns && !d->counts))
    return H2MI_EINVAL;
  const uint32_t n = d->n_ops;
  if ((n == 0) != (d->n_levels == 0)) return H2MI_EINVAL;
  uint64_t placed = 0;
  for (uint32_t j = 0; j < d->n_columns; j++) {
    if (d->counts[j] > ((uint64_t)1 << H2MI_MAX_LOG_N)) return H2MI_ERANGE;
    placed += d->counts[j];
  }
  if (placed && !d->placement) return H2MI_EINVAL;
  for (uint32_t l = 0; l < d->n_levels; l++)  // no empty level, and the last one ends the ops
    if (d->level_ends[l] <= (l ? d->level_ends[l - 1] : 0u) || d->level_ends[l] > n) return H2MI_EINVAL;
  if (d->n_levels && d->level_ends[d->n_levels - 1] != n) return H2MI_EINVAL;
  for (uint32_t c = 0; c < d->n_constants; c++)
    if (!below_r(d->constants + 4 * (size_t)c)) return H2MI_EINVAL;
  constexpr uint32_t UNSET = 0xffffffffu;
  std::vector<uint32_t> level_of(n, UNSET);  // per cell: the level of the op that writes it
  for (uint32_t l = 0, at = 0; l < d->n_levels; l++)
    for (; at < d->level_ends[l]; at++) {
      const h2mi_witness_op& op = d->ops[at];
      if (op.dst >= n || level_of[op.dst] != UNSET) return H2MI_EINVAL;  // outside the cells, or named twice
      level_of[op.dst] = l;
    }
  // n ops with n distinct dst below n: every cell is named.  An operand's level must be strictly below its reader's
  for (uint32_t at = 0; at < n; at++) {
    const h2mi_witness_op& op = d->ops[at];
    const uint32_t kind = op.code & 0xffu, bits = (op.code >> 8) & 0xffu, shift = (op.code >> 16) & 0xffu, level = level_of[op.dst];
    if (op.code >> 24) return H2MI_EINVAL;
    switch (kind) {
      case WP_INPUT:
        if (op.a >= d->n_inputs) return H2MI_EINVAL;
        break;
      case WP_CONST:
        if (op.a >= d->n_constants) return H2MI_EINVAL;
        break;
      case WP_LIMB:
        if (bits < 1 || bits > 64 || shift + bits > 254) return H2MI_EINVAL;
        [[fallthrough]];
      case WP_COPY:
        if (op.a >= n || level_of[op.a] >= level) return H2MI_EINVAL;
        break;
      case WP_DIVQ:
      case WP_DIVR:  // bits: the flags; b: a constant or a cell of a lower level, by the flag
        if (shift || (bits & ~(WP_DIV_CONST | WP_DIV_SIGNED)) || op.a >= n || level_of[op.a] >= level) return H2MI_EINVAL;
        if (bits & WP_DIV_CONST ? op.b >= d->n_constants : (op.b >= n || level_of[op.b] >= level)) return H2MI_EINVAL;
        break;
      case WP_ISZERO:
      case WP_INV:
      case WP_MSB:
        if (bits || shift || op.b || op.a >= n || level_of[op.a] >= level) return H2MI_EINVAL;
        break;
      case WP_POW2:  // bits: the flag
        if ((bits & ~WP_POW2_OF_MSB) || shift || op.b || op.a >= n || level_of[op.a] >= level) return H2MI_EINVAL;
        break;
      case WP_GATE:
        if (op.dst < 3) return H2MI_EINVAL;
        for (uint32_t back = 1; back <= 3; back++)
          if (level_of[op.dst - back] >= level) return H2MI_EINVAL;
        break;
      default:
        return H2MI_EINVAL;
    }
  }
  for (uint64_t e = 0; e < placed; e++)
    if (d->placement[e] >= n) return H2MI_EINVAL;
  for (uint64_t i = 0; i < 2 * (uint64_t)d->n_checks; i++)
    if (d->checks[i] >= n) return H2MI_EINVAL;
  return H2MI_OK;
}

struct Segment {
  uint32_t l0, l1;  // levels l0 .. l1 - 1: one wide level as a grid launch, or a run of narrow ones in one workgroup
  bool grid;
};

struct WitnessProgram {
  uint32_t n_cells = 0, n_levels = 0, n_inputs = 0, n_constants = 0, n_checks = 0, n_columns = 0, n_grid = 0, n_wg = 0;
  uint64_t placed = 0, device_bytes = 0;
  bool ran = false;
  bool hints = false;  // holds a hint op: its levels run in the _hints instantiations
  std::vector<uint32_t> level_ends;
  std::vector<uint64_t> column_start;  // in words of the column buffer
  std::vector<Segment> plan;
  DevMem ops, d_level_ends, consts, values, cells, placement, columns, checks, status;
  DevMem read_idx, read_vals;  // h2mi_witness_read's staging, grown to the longest list asked for (the public cells, proof after proof)
  uint32_t read_cap = 0;
};

static std::set<WitnessProgram*> g_programs;  // the live handles (under the library mutex)

// the segmentation rule of include/h2mi.h
static void witness_plan(WitnessProgram& w) {
  uint32_t run0 = 0;  // first level of the current run of narrow levels
  auto close = [&](uint32_t end) {
    for (uint32_t l = run0; l < end; l += WP_WG_LEVELS) {
      w.plan.push_back({l, std::min(end, l + WP_WG_LEVELS), false});
      w.n_wg++;
    }
  };
  for (uint32_t l = 0; l < w.n_levels; l++) {
    const uint32_t size = w.level_ends[l] - (l ? w.level_ends[l - 1] : 0u);
    if (size <= WP_WG) continue;
    close(l);
    w.plan.push_back({l, l + 1, true});
    w.n_grid++;
    run0 = l + 1;
  }
  close(w.n_levels);
}

static int witness_alloc(WitnessProgram& w, DevMem& m, size_t bytes) {
  const hipError_t err = m.alloc(bytes);
  if (err == hipErrorOutOfMemory) return H2MI_ENOMEM;
  H2_HIP(err);
  w.device_bytes += bytes ? bytes : 1;
  return H2MI_OK;
}

static int witness_create(const h2mi_witness_desc* d, h2mi_witness_t* out) {
  if (!out) return H2MI_EINVAL;
  *out = nullptr;
  int rc = witness_check(d);
  if (rc) return rc;
  H2_REQUIRE_INIT();
  if (h2mi_device_count() > 1) return H2MI_EINVAL;  // as for H2MI_CELLS_DEVICE: the columns are read on the primary device's stream only
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  hipStream_t s = ctx().stream;
  std::unique_ptr<WitnessProgram> w(new WitnessProgram);
  w->n_cells = d->n_ops;
  w->n_levels = d->n_levels;
  w->n_inputs = d->n_inputs;
  w->n_constants = d->n_constants;
  w->n_checks = d->n_checks;
  w->n_columns = d->n_columns;
  w->level_ends.assign(d->level_ends, d->level_ends + d->n_levels);
  w->column_start.assign(d->n_columns + 1, 0);
  for (uint32_t j = 0; j < d->n_columns; j++) w->column_start[j + 1] = w->column_start[j] + d->counts[j];
  w->placed = w->column_start[d->n_columns];
  for (uint32_t at = 0; at < d->n_ops; at++) w->hints |= (d->ops[at].code & 0xffu) >= WP_DIVQ;
  witness_plan(*w);
  const struct {
    DevMem& m;
    const void* src;
    size_t bytes;
  } parts[] = {{w->ops, d->ops, (size_t)d->n_ops * 16},
               {w->d_level_ends, d->level_ends, (size_t)d->n_levels * 4},
               {w->consts, d->constants, (size_t)d->n_constants * 32},
               {w->placement, d->placement, (size_t)w->placed * 4},
               {w->checks, d->checks, (size_t)d->n_checks * 8},
               {w->values, nullptr, (size_t)d->n_inputs * 32},
               {w->cells, nullptr, (size_t)d->n_ops * 32},
               {w->columns, nullptr, (size_t)w->placed * 32},
               {w->status, nullptr, 4}};
  for (const auto& p : parts) {
    if ((rc = witness_alloc(*w, p.m, p.bytes))) return rc;
    if (p.src && p.bytes) H2_HIP(hipMemcpyAsync(p.m.p, p.src, p.bytes, hipMemcpyHostToDevice, s));
  }
  H2_HIP(hipStreamSynchronize(s));  // the descriptor's arrays are the caller's again
  g_programs.insert(w.get());
  *out = w.release();
  return H2MI_OK;
}

static WitnessProgram* witness_of(h2mi_witness_t h) {
  WitnessProgram* w = reinterpret_cast<WitnessProgram*>(h);
  return g_programs.count(w) ? w : nullptr;
}

static int witness_run(h2mi_witness_t h, const uint64_t* inputs, void** d_columns_out, uint32_t* first_failed_check) {
  H2_REQUIRE_INIT();
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  WitnessProgram* w = witness_of(h);
  if (!w) return H2MI_EHANDLE;
  if ((w->n_inputs && !inputs) || (w->n_columns && !d_columns_out) || !first_failed_check) return H2MI_EINVAL;
  if (h2mi_device_count() > 1) return H2MI_EINVAL;
  *first_failed_check = WP_NO_FAILURE;
  for (uint32_t j = 0; j < w->n_inputs; j++)
    if (!below_r(inputs + 4 * (size_t)j)) return H2MI_EINVAL;
  hipStream_t s = ctx().stream;
  w->ran = false;
  if (w->n_inputs) H2_HIP(hipMemcpyAsync(w->values.p, inputs, (size_t)w->n_inputs * 32, hipMemcpyHostToDevice, s));
  H2_HIP(hipMemsetAsync(w->status.p, 0xff, 4, s));
  const uint4* ops = w->ops.as<uint4>();
  fe* cells = w->cells.as<fe>();
  const fe *values = w->values.as<fe>(), *consts = w->consts.as<fe>();
  for (const Segment& g : w->plan) {
    if (g.grid) {
      const uint32_t begin = g.l0 ? w->level_ends[g.l0 - 1] : 0u, count = w->level_ends[g.l0] - begin;
      if (w->hints)
        H2_LAUNCH("k_witness_level_hints", k_witness_level_hints, ceil_div_u32(count, WP_BLOCK), WP_BLOCK, 0, s, ops + begin, count, cells, values, consts);
      else
        H2_LAUNCH("k_witness_level", k_witness_level, ceil_div_u32(count, WP_BLOCK), WP_BLOCK, 0, s, ops + begin, count, cells, values, consts);
    } else if (w->hints) {
      H2_LAUNCH("k_witness_levels_wg_hints", k_witness_levels_wg_hints, 1, WP_WG, 0, s, ops, (const uint32_t*)w->d_level_ends.as<uint32_t>(), g.l0, g.l1,
                cells, values, consts);
    } else {
      H2_LAUNCH("k_witness_levels_wg", k_witness_levels_wg, 1, WP_WG, 0, s, ops, (const uint32_t*)w->d_level_ends.as<uint32_t>(), g.l0, g.l1, cells,
                values, consts);
    }
  }
  const uint64_t total = w->placed + w->n_checks;
  if (total)
    H2_LAUNCH("k_witness_place", k_witness_place, ceil_div_u32(total, WP_BLOCK), WP_BLOCK, 0, s, (const fe*)cells,
              (const uint32_t*)w->placement.as<uint32_t>(), w->placed, w->columns.as<fe>(), (const uint2*)w->checks.as<uint2>(), w->n_checks,
              w->status.as<uint32_t>());
  uint32_t failed = WP_NO_FAILURE;
  H2_HIP(hipMemcpyAsync(&failed, w->status.p, 4, hipMemcpyDeviceToHost, s));
  H2_HIP(hipStreamSynchronize(s));  // the check status is the call's answer; `inputs` is the caller's again
  for (uint32_t j = 0; j < w->n_columns; j++) d_columns_out[j] = w->columns.as<fe>() + w->column_start[j];
  w->ran = true;
  if (failed != WP_NO_FAILURE) {
    *first_failed_check = failed;
    return H2MI_EUNSAT;
  }
  return H2MI_OK;
}

static int witness_read(h2mi_witness_t h, const uint32_t* cells, uint32_t n, uint64_t* out) {
  H2_REQUIRE_INIT();
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  WitnessProgram* w = witness_of(h);
  if (!w) return H2MI_EHANDLE;
  if (n == 0) return H2MI_OK;
  if (!cells || !out || !w->ran) return H2MI_EINVAL;
  for (uint32_t i = 0; i < n; i++)
    if (cells[i] >= w->n_cells) return H2MI_EINVAL;
  hipStream_t s = ctx().stream;
  if (n > w->read_cap) {  // nothing queued uses the old staging: every read ends with a wait for the stream
    for (DevMem* m : {&w->read_idx, &w->read_vals}) {
      if (m->p) H2_IGNORE(hipFree(m->p));
      m->p = nullptr;
    }
    w->read_cap = 0;
    for (auto p : {std::make_pair(&w->read_idx, (size_t)n * 4), std::make_pair(&w->read_vals, (size_t)n * 32)}) {
      const hipError_t err = p.first->alloc(p.second);
      if (err == hipErrorOutOfMemory) return H2MI_ENOMEM;
      H2_HIP(err);
    }
    w->read_cap = n;
  }
  DevMem &idx = w->read_idx, &vals = w->read_vals;
  H2_HIP(hipMemcpyAsync(idx.p, cells, (size_t)n * 4, hipMemcpyHostToDevice, s));
  H2_LAUNCH("k_witness_read", k_witness_read, ceil_div_u32(n, WP_BLOCK), WP_BLOCK, 0, s, (const fe*)w->cells.as<fe>(), (const uint32_t*)idx.as<uint32_t>(), n,
            vals.as<fe>());
  H2_HIP(hipMemcpyAsync(out, vals.p, (size_t)n * 32, hipMemcpyDeviceToHost, s));
  H2_HIP(hipStreamSynchronize(s));
  return H2MI_OK;
}

// h2mi_shutdown: the device memory of the programs still alive goes with the device; their handles are unknown from here on
void witness_teardown() {
  for (WitnessProgram* w : g_programs) delete w;
  g_programs.clear();
}

}  // namespace h2

using namespace h2;

extern "C" {

int h2mi_witness_check(const h2mi_witness_desc* d) { return witness_check(d); }

int h2mi_witness_create(const h2mi_witness_desc* d, h2mi_witness_t* out) { return witness_create(d, out); }

int h2mi_witness_info(h2mi_witness_t h, h2mi_witness_info_t* out) {
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  WitnessProgram* w = witness_of(h);
  if (!w) return H2MI_EHANDLE;
  if (!out) return H2MI_EINVAL;
  out->n_cells = w->n_cells;
  out->n_levels = w->n_levels;
  out->n_grid_launches = w->n_grid;
  out->n_wg_launches = w->n_wg;
  out->device_bytes = w->device_bytes;
  return H2MI_OK;
}

int h2mi_witness_run(h2mi_witness_t h, const uint64_t* inputs, void** d_columns_out, uint32_t* first_failed_check) {
  return witness_run(h, inputs, d_columns_out, first_failed_check);
}

int h2mi_witness_read(h2mi_witness_t h, const uint32_t* cells, uint32_t n, uint64_t* out) { return witness_read(h, cells, n, out); }

int h2mi_witness_release(h2mi_witness_t h) {
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  WitnessProgram* w = witness_of(h);
  if (!w) return H2MI_EHANDLE;
  if (ctx().inited) {
    const int rc = bind_thread();
    if (rc) return rc;
    H2_IGNORE(hipStreamSynchronize(ctx().stream));  // nothing queued reads its buffers any more
  }
  g_programs.erase(w);
  delete w;
  return H2MI_OK;
}

}  // extern "C"
