// h2mi_keyfile.hpp — the proving-key blob of h2mi_prover_pk_export / _import / _blob_check: its writer and its parser, on the host alone.
//
// DESIGN.md 3 is the normative description of the format; tests/key_file_cases.py restates it in Python and pins the bytes.  No HIP
// include, no library call: the file compiles with a plain C++17 compiler, and the parser is what runs under the sanitizers
// (tests/host/sanitize_keyfile.cpp).  Everything is read with memcpy at checked offsets: the blob needs no alignment here (import
// aligns its copy, because the cell sections are then handed over as h2mi_column_cells).  The parser applies the STRUCTURAL rules — every
// count against the blob's length and the ABI limits before anything is sized from it, rows ascending and usable, moved cells sorted
// and inside the permutation — and h2mi_prover.cpp puts the rules of the constraint system and of its programs (validate, the *_check
// functions) behind it; h2mi_prover_pk_blob_check and h2mi_prover_pk_import run both, in this order, before any device call.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/h2mi_prover.h"

namespace h2mi {
namespace keyfile {

constexpr uint64_t MAGIC = 0x0a4b502e494d3248ull;  // the bytes "H2MI.PK\n"
constexpr uint32_t VERSION = 1;
constexpr uint32_t FLAG_LOGUP = 1u;  // H2MI_KEYGEN_LOGUP is part of the key; every other bit is refused
constexpr size_t HEADER_BYTES = 32;  // magic, version, flags, length, checksum
constexpr size_t MAX_USER_BYTES = (size_t)1 << 20;
constexpr uint32_t LAYOUT_EMPTY = 0, LAYOUT_DENSE = 1, LAYOUT_SPARSE = 2;

inline size_t pad8(size_t b) { return (b + 7) & ~(size_t)7; }

// over the blob's 64-bit little-endian words with the checksum's own word taken as zero: FNV-1a, a word where it takes a byte
inline uint64_t checksum(const uint8_t* blob, size_t len) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i + 8 <= len; i += 8) {
    uint64_t w = 0;
    if (i != 24)
      for (int b = 7; b >= 0; b--) w = (w << 8) | blob[i + b];
    h = (h ^ w) * 0x100000001b3ull;
  }
  return h;
}

// the dense / sparse rule of a column with `count` cells, the last of them on row last - 1, at `width` bytes per value
inline uint32_t layout_of(uint64_t count, uint64_t last, uint64_t width) {
  if (count == 0) return LAYOUT_EMPTY;
  return last * width <= count * (4 + width) ? LAYOUT_DENSE : LAYOUT_SPARSE;
}

// a canonical 32-byte little-endian word: 0 — zero; 1 — nonzero and a signed 64-bit integer holds it (v <= 2^63 - 1, or v >= r - 2^63
// as -(r - v)); 2 — nonzero, below r, and none does; -1 — not below r
inline int classify(const uint8_t* word) {
  static const uint64_t MOD[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
  uint64_t v[4], n[4];
  for (int i = 0; i < 4; i++) {
    v[i] = 0;
    for (int b = 7; b >= 0; b--) v[i] = (v[i] << 8) | word[8 * i + b];
  }
  if (!(v[0] | v[1] | v[2] | v[3])) return 0;
  uint64_t borrow = 0;  // n = r - v
  for (int i = 0; i < 4; i++) {
    const uint64_t d = MOD[i] - v[i], e = d - borrow;
    borrow = (MOD[i] < v[i]) | (d < borrow);
    n[i] = e;
  }
  if (borrow || !(n[0] | n[1] | n[2] | n[3])) return -1;
  if (!(v[1] | v[2] | v[3]) && v[0] <= 0x7fffffffffffffffull) return 1;
  if (!(n[1] | n[2] | n[3]) && n[0] <= 0x8000000000000000ull) return 1;
  return 2;
}

// ---- writer --------------------------------------------------------------------------------------------------------------------------
struct Writer {
  std::vector<uint8_t> b;
  size_t open_at = 0;
  void u32(uint32_t v) {
    for (int i = 0; i < 4; i++) b.push_back((uint8_t)(v >> (8 * i)));
  }
  void u64(uint64_t v) {
    for (int i = 0; i < 8; i++) b.push_back((uint8_t)(v >> (8 * i)));
  }
  void bytes(const void* p, size_t n) {
    if (n) b.insert(b.end(), (const uint8_t*)p, (const uint8_t*)p + n);
  }
  void header(uint32_t flags) {
    u64(MAGIC);
    u32(VERSION);
    u32(flags);
    u64(0);  // length and checksum: finish()
    u64(0);
  }
  void begin() {  // a section: its payload's length, the payload, zeros up to the next multiple of 8
    open_at = b.size();
    u64(0);
  }
  void end() {
    const uint64_t len = b.size() - open_at - 8;
    for (int i = 0; i < 8; i++) b[open_at + i] = (uint8_t)(len >> (8 * i));
    b.resize(pad8(b.size()), 0);
  }
  void program(const h2mi_gate_program& g) {
    u32(g.n_ops);
    u32(g.n_constants);
    for (uint32_t i = 0; i < g.n_ops; i++) {
      u32(g.ops[i].op);
      u32(g.ops[i].index);
      u32((uint32_t)g.ops[i].rotation);
    }
    bytes(g.constants, 32 * (size_t)g.n_constants);
  }
  // field by field; what the shape does not read (n_gates and the gate columns off FLEX_VERTICAL, lookups[] beside a lookup program) is
  // written as zero / left out, so that two keys of one circuit export the same bytes whatever the caller left in those fields
  void constraint_system(const h2mi_constraint_system& cs, bool lookup_program) {
    const uint32_t n_gates = cs.gates == H2MI_GATES_FLEX_VERTICAL ? cs.n_gates : 0;
    begin();
    u32(cs.k); u32(cs.n_advice); u32(cs.n_fixed); u32(cs.n_instance); u32(cs.degree); u32(cs.blinding_factors);
    u32(cs.gates); u32(n_gates); u32(cs.n_perm); u32(cs.n_lookups); u32(cs.n_advice_queries); u32(cs.n_fixed_queries);
    for (uint32_t g = 0; g < n_gates; g++) u32(cs.gate_advice[g]);
    for (uint32_t g = 0; g < n_gates; g++) u32(cs.gate_selector[g]);
    for (uint32_t j = 0; j < cs.n_perm; j++) { u32(cs.perm_columns[j].kind); u32(cs.perm_columns[j].index); }
    for (uint32_t l = 0; l < cs.n_lookups; l++) {
      const h2mi_lookup z = {{0, 0}, 0, 0}, &lk = lookup_program ? z : cs.lookups[l];
      u32(lk.input.kind); u32(lk.input.index); u32((uint32_t)lk.selector_fixed); u32(lk.table_fixed);
    }
    for (uint32_t i = 0; i < cs.n_advice_queries; i++) { u32(cs.advice_queries[i].column); u32((uint32_t)cs.advice_queries[i].rotation); }
    for (uint32_t i = 0; i < cs.n_fixed_queries; i++) { u32(cs.fixed_queries[i].column); u32((uint32_t)cs.fixed_queries[i].rotation); }
    end();
  }
  // a fixed column's cells as h2mi_fr_compact_cells_dev reports them: dense — `last` values; sparse — `count` values, then `count` rows
  void column(uint32_t layout, uint32_t width, uint64_t count, uint32_t last, const void* values, const uint32_t* rows) {
    begin();
    u32(layout); u32(layout ? width : 0); u32((uint32_t)count); u32(last);
    if (layout == LAYOUT_DENSE) bytes(values, (size_t)last * width);
    if (layout == LAYOUT_SPARSE) {
      bytes(values, (size_t)count * width);
      for (uint64_t i = 0; i < count; i++) u32(rows[i]);
    }
    end();
  }
  void finish() {
    const uint64_t len = b.size();
    for (int i = 0; i < 8; i++) b[16 + i] = (uint8_t)(len >> (8 * i));
    const uint64_t sum = checksum(b.data(), b.size());
    for (int i = 0; i < 8; i++) b[24 + i] = (uint8_t)(sum >> (8 * i));
  }
};

// ---- parser --------------------------------------------------------------------------------------------------------------------------
struct Program {
  std::vector<h2mi_expr_op> ops;
  std::vector<uint64_t> constants;
  h2mi_gate_program view() const { return {ops.data(), (uint32_t)ops.size(), constants.data(), (uint32_t)(constants.size() / 4)}; }
};
struct Column {
  uint32_t layout = 0, width = 0, count = 0, last = 0;
  size_t values_at = 0, rows_at = 0;  // offsets into the blob
};
struct Blob {
  h2mi_constraint_system cs;
  bool logup = false, has_gates = false, has_lookups = false, has_shuffles = false, has_phases = false;
  Program gates, lookup_exprs, shuffle_exprs;
  uint32_t n_lookups = 0, lookup_pairs[H2MI_MAX_LOOKUPS], lookup_inputs[H2MI_MAX_LOOKUPS];
  uint32_t n_shuffles = 0, shuffle_pairs[H2MI_MAX_SHUFFLES];
  h2mi_advice_phases phases;
  std::vector<Column> fixed;
  size_t moved_at = 0, n_moved = 0;  // 16 bytes each
  size_t commitments_at = 0;         // (n_fixed + n_perm) x 64 bytes
  size_t user_at = 0, user_len = 0;
  Blob() {
    std::memset(&cs, 0, sizeof(cs));
    std::memset(&phases, 0, sizeof(phases));
    std::memset(lookup_pairs, 0, sizeof(lookup_pairs));
    std::memset(lookup_inputs, 0, sizeof(lookup_inputs));
    std::memset(shuffle_pairs, 0, sizeof(shuffle_pairs));
  }
};

// a cursor over one section's payload: every read is checked against the payload's end, and the section must be used up exactly
struct Cursor {
  const uint8_t* p;
  size_t at, end;
  bool ok = true;
  uint32_t u32() {
    if (!ok || end - at < 4) { ok = false; return 0; }
    uint32_t v = 0;
    for (int i = 3; i >= 0; i--) v = (v << 8) | p[at + i];
    at += 4;
    return v;
  }
  uint64_t u64() {
    const uint64_t lo = u32(), hi = u32();
    return lo | (hi << 32);
  }
  bool take(size_t n, size_t* where) {  // n bytes, left where they are
    if (!ok || end - at < n) return ok = false;
    *where = at;
    at += n;
    return true;
  }
  bool done() const { return ok && at == end; }
};

namespace detail {
inline bool section(const uint8_t* blob, size_t len, size_t& at, Cursor& out) {
  if (len - at < 8) return false;
  Cursor head = {blob, at, at + 8};
  const uint64_t n = head.u64();
  if (n > len - at - 8) return false;
  out = Cursor{blob, at + 8, at + 8 + (size_t)n};
  const size_t next = at + 8 + pad8((size_t)n);
  if (next > len) return false;
  for (size_t i = out.end; i < next; i++)
    if (blob[i]) return false;  // the padding is zero: one encoding per key
  at = next;
  return true;
}
inline bool program(Cursor& c, Program& out) {
  const uint32_t n_ops = c.u32(), n_constants = c.u32();
  if (!c.ok || n_ops > H2MI_MAX_EXPR_OPS || n_constants > H2MI_MAX_EXPR_CONSTANTS) return false;
  if (c.end - c.at != 12 * (size_t)n_ops + 32 * (size_t)n_constants) return false;
  out.ops.resize(n_ops);
  for (uint32_t i = 0; i < n_ops; i++) {
    out.ops[i].op = c.u32();
    out.ops[i].index = c.u32();
    out.ops[i].rotation = (int32_t)c.u32();
  }
  out.constants.resize(4 * (size_t)n_constants);
  for (size_t i = 0; i < out.constants.size(); i++) out.constants[i] = c.u64();
  return c.done();
}
}  // namespace detail

// H2MI_OK, or H2MI_EINVAL for anything the format does not allow.  Nothing of `out` is to be used after a refusal.
inline int parse(const uint8_t* blob, size_t len, Blob& out) {
  if (!blob || len < HEADER_BYTES || (len & 7)) return H2MI_EINVAL;
  Cursor h = {blob, 0, HEADER_BYTES};
  if (h.u64() != MAGIC || h.u32() != VERSION) return H2MI_EINVAL;
  const uint32_t flags = h.u32();
  if (flags & ~FLAG_LOGUP) return H2MI_EINVAL;
  if (h.u64() != len) return H2MI_EINVAL;  // a truncated or padded file
  if (h.u64() != checksum(blob, len)) return H2MI_EINVAL;
  out.logup = (flags & FLAG_LOGUP) != 0;
  size_t at = HEADER_BYTES;
  Cursor c = {blob, 0, 0};
  h2mi_constraint_system& cs = out.cs;
  // -- the constraint system
  if (!detail::section(blob, len, at, c)) return H2MI_EINVAL;
  cs.k = c.u32(); cs.n_advice = c.u32(); cs.n_fixed = c.u32(); cs.n_instance = c.u32(); cs.degree = c.u32(); cs.blinding_factors = c.u32();
  cs.gates = c.u32(); cs.n_gates = c.u32(); cs.n_perm = c.u32(); cs.n_lookups = c.u32(); cs.n_advice_queries = c.u32(); cs.n_fixed_queries = c.u32();
  if (!c.ok || cs.k == 0 || cs.k > H2MI_MAX_LOG_N || cs.n_advice > H2MI_MAX_ADVICE || cs.n_fixed > H2MI_MAX_FIXED || cs.n_instance > H2MI_MAX_INSTANCE ||
      cs.n_gates > H2MI_MAX_GATES || cs.n_perm > H2MI_MAX_PERM || cs.n_lookups > H2MI_MAX_LOOKUPS || cs.n_advice_queries > H2MI_MAX_QUERIES ||
      cs.n_fixed_queries > H2MI_MAX_QUERIES || cs.degree < 3 || cs.degree > 9)
    return H2MI_EINVAL;
  if (cs.gates != H2MI_GATES_FLEX_VERTICAL && cs.n_gates) return H2MI_EINVAL;
  if ((((uint64_t)1) << cs.k) <= (uint64_t)cs.blinding_factors + 2) return H2MI_EINVAL;
  const uint32_t u = (uint32_t)((((uint64_t)1) << cs.k) - cs.blinding_factors - 1);  // the usable rows
  for (uint32_t g = 0; g < cs.n_gates; g++) cs.gate_advice[g] = c.u32();
  for (uint32_t g = 0; g < cs.n_gates; g++) cs.gate_selector[g] = c.u32();
  for (uint32_t j = 0; j < cs.n_perm; j++) { cs.perm_columns[j].kind = c.u32(); cs.perm_columns[j].index = c.u32(); }
  for (uint32_t l = 0; l < cs.n_lookups; l++) {
    cs.lookups[l].input.kind = c.u32(); cs.lookups[l].input.index = c.u32();
    cs.lookups[l].selector_fixed = (int32_t)c.u32(); cs.lookups[l].table_fixed = c.u32();
  }
  for (uint32_t i = 0; i < cs.n_advice_queries; i++) { cs.advice_queries[i].column = c.u32(); cs.advice_queries[i].rotation = (int32_t)c.u32(); }
  for (uint32_t i = 0; i < cs.n_fixed_queries; i++) { cs.fixed_queries[i].column = c.u32(); cs.fixed_queries[i].rotation = (int32_t)c.u32(); }
  if (!c.done()) return H2MI_EINVAL;
  // -- the programs: an empty section where the key has none
  if (!detail::section(blob, len, at, c)) return H2MI_EINVAL;
  out.has_gates = c.end != c.at;
  if (out.has_gates && !detail::program(c, out.gates)) return H2MI_EINVAL;
  if (out.has_gates != (cs.gates == H2MI_GATES_EXPRESSIONS)) return H2MI_EINVAL;
  if (!detail::section(blob, len, at, c)) return H2MI_EINVAL;
  out.has_lookups = c.end != c.at;
  if (out.has_lookups) {
    out.n_lookups = c.u32();
    if (!c.ok || !out.has_gates || out.n_lookups == 0 || out.n_lookups != cs.n_lookups) return H2MI_EINVAL;
    for (uint32_t l = 0; l < out.n_lookups; l++) out.lookup_pairs[l] = c.u32();
    for (uint32_t l = 0; l < out.n_lookups; l++) {
      out.lookup_inputs[l] = c.u32();
      if (out.lookup_inputs[l] == 0 || out.lookup_inputs[l] > H2MI_MAX_LOGUP_INPUTS || (out.lookup_inputs[l] != 1 && !out.logup)) return H2MI_EINVAL;
    }
    if (!detail::program(c, out.lookup_exprs)) return H2MI_EINVAL;
  }
  if (out.logup && !out.has_lookups) return H2MI_EINVAL;
  if (!detail::section(blob, len, at, c)) return H2MI_EINVAL;
  out.has_shuffles = c.end != c.at;
  if (out.has_shuffles) {
    out.n_shuffles = c.u32();
    if (!c.ok || !out.has_gates || out.n_shuffles == 0 || out.n_shuffles > H2MI_MAX_SHUFFLES) return H2MI_EINVAL;
    for (uint32_t i = 0; i < out.n_shuffles; i++) out.shuffle_pairs[i] = c.u32();
    if (!detail::program(c, out.shuffle_exprs)) return H2MI_EINVAL;
  }
  if (!detail::section(blob, len, at, c)) return H2MI_EINVAL;
  out.has_phases = c.end != c.at;
  out.phases.n_phases = 1;
  if (out.has_phases) {
    out.phases.n_phases = c.u32();
    out.phases.n_challenges = c.u32();
    if (!c.ok || !out.has_gates || out.phases.n_phases == 0 || out.phases.n_phases > H2MI_MAX_ADVICE_PHASES || out.phases.n_challenges > H2MI_MAX_CHALLENGES)
      return H2MI_EINVAL;
    if (out.phases.n_phases == 1 && out.phases.n_challenges == 0) return H2MI_EINVAL;  // such a key has no phase section
    for (uint32_t j = 0; j < cs.n_advice; j++) out.phases.advice_phase[j] = c.u32();
    for (uint32_t i = 0; i < out.phases.n_challenges; i++) out.phases.challenge_phase[i] = c.u32();
    if (!c.done()) return H2MI_EINVAL;
  }
  // -- the fixed columns' cells
  out.fixed.resize(cs.n_fixed);
  for (uint32_t f = 0; f < cs.n_fixed; f++) {
    Column& col = out.fixed[f];
    if (!detail::section(blob, len, at, c)) return H2MI_EINVAL;
    col.layout = c.u32(); col.width = c.u32(); col.count = c.u32(); col.last = c.u32();
    if (!c.ok) return H2MI_EINVAL;
    if (col.layout == LAYOUT_EMPTY) {
      if (col.width || col.count || col.last || !c.done()) return H2MI_EINVAL;
      continue;
    }
    if ((col.width != 8 && col.width != 32) || col.count == 0 || col.count > col.last || col.last > u) return H2MI_EINVAL;
    if (col.layout != layout_of(col.count, col.last, col.width)) return H2MI_EINVAL;  // dense, sparse or unknown: the rule decides
    const size_t n_values = col.layout == LAYOUT_DENSE ? col.last : col.count;
    if (!c.take(n_values * col.width, &col.values_at)) return H2MI_EINVAL;
    if (col.layout == LAYOUT_SPARSE && !c.take((size_t)col.count * 4, &col.rows_at)) return H2MI_EINVAL;
    if (!c.done()) return H2MI_EINVAL;
    // one encoding per column: `count` nonzero values, the last of them at the end, below r, and 32 bytes each only where one needs them
    size_t nonzero = 0, wide = 0;
    int cl = 0;
    for (size_t i = 0; i < n_values; i++) {
      const uint8_t* v = blob + col.values_at + i * col.width;
      if (col.width == 8) {
        cl = 0;
        for (int b = 0; b < 8; b++) cl |= v[b] != 0;
      } else {
        cl = classify(v);
      }
      if (cl < 0) return H2MI_EINVAL;
      nonzero += cl != 0;
      wide += cl == 2;
    }
    if (nonzero != col.count || cl == 0 || (col.width == 32 && wide == 0)) return H2MI_EINVAL;
    if (col.layout == LAYOUT_DENSE) continue;
    Cursor rows = {blob, col.rows_at, col.rows_at + (size_t)col.count * 4};
    uint64_t next = 0;  // the smallest row the next cell may name
    for (uint32_t i = 0; i < col.count; i++) {
      const uint32_t row = rows.u32();
      if (row < next || row >= u) return H2MI_EINVAL;  // descending, repeated, or in the blinding rows
      next = (uint64_t)row + 1;
    }
    if (next != col.last) return H2MI_EINVAL;
  }
  // -- the cells the permutation moves: (column, row, image column, image row), ascending by (column, row)
  if (!detail::section(blob, len, at, c)) return H2MI_EINVAL;
  if ((c.end - c.at) % 16) return H2MI_EINVAL;
  out.n_moved = (c.end - c.at) / 16;
  out.moved_at = c.at;
  if (out.n_moved > (uint64_t)cs.n_perm * u) return H2MI_EINVAL;
  uint64_t prev = 0;
  for (size_t i = 0; i < out.n_moved; i++) {
    const uint32_t c0 = c.u32(), r0 = c.u32(), c1 = c.u32(), r1 = c.u32();
    if (c0 >= cs.n_perm || c1 >= cs.n_perm || r0 >= u || r1 >= u) return H2MI_EINVAL;
    const uint64_t key = ((uint64_t)c0 << 32) | r0;
    if (i && key <= prev) return H2MI_EINVAL;
    prev = key;
  }
  // -- the commitments, the user section, and nothing behind them
  if (!detail::section(blob, len, at, c)) return H2MI_EINVAL;
  if (!c.take(64 * ((size_t)cs.n_fixed + cs.n_perm), &out.commitments_at) || !c.done()) return H2MI_EINVAL;
  if (!detail::section(blob, len, at, c)) return H2MI_EINVAL;
  out.user_len = c.end - c.at;
  out.user_at = c.at;
  if (out.user_len > MAX_USER_BYTES || at != len) return H2MI_EINVAL;
  return H2MI_OK;
}

}  // namespace keyfile
}  // namespace h2mi
