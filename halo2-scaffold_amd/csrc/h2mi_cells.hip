// libh2mi.so — witness cells from device memory into the prover's columns (h2mi_fr_scatter_cells_dev, include/h2mi.h).
//
// What create_proof's `advice[column][row] = value` becomes for a caller whose witness lives in HBM already, or whose cells are
// 64-bit integers: ONE launch of k_cells_scatter over all cells of all columns of a call.  The kernel is bound by memory traffic
// (one Montgomery product against 40 .. 68 bytes per cell), so its shape follows the accesses: a lane owns a cell and moves its
// 32-byte word as two 16-byte accesses (fe_load / fe_store: 16 bytes per lane is the widest access), so each wave instruction of a
// dense run carries 1 KiB and the pair of them covers 2 KiB of whole cache lines.  The other form that stores 1 KiB per instruction —
// two adjacent lanes per cell, each owning one 16-byte half, the word exchanged between them — was measured beside this one and
// lost (0.066 against 0.044 ms for three dense columns of 2^20 32-byte cells); it is not kept.
// The conversions are the fp.cuh layer's: canonical -> Montgomery is the product with R^2 of k_fe_from_repr (h2mi_serde.hip).
#include "fp.cuh"
#include "h2mi_fr_tables.h"

namespace h2 {

constexpr uint32_t CS_MAX_SEGS = 64;       // = H2MI_MAX_ADVICE / H2MI_MAX_FIXED: every column of a call in one launch
constexpr uint32_t CS_FMT_CANONICAL = 1u;  // H2MI_CELLS_CANONICAL
constexpr uint32_t CS_FMT_I64 = 4u;        // H2MI_CELLS_I64
constexpr uint32_t CS_BLOCK = 256;

// where cell e of the call lives and lands: segment s covers e in [start[s], start[s + 1]).  2.6 KB by value.
struct CellSegs {
  fe* dst[CS_MAX_SEGS];
  const uint32_t* rows[CS_MAX_SEGS];
  const void* values[CS_MAX_SEGS];
  uint64_t start[CS_MAX_SEGS + 1];
  uint32_t row_limit[CS_MAX_SEGS];
  uint32_t format[CS_MAX_SEGS];
  uint32_t n_segs;
};

// status[0]: cells whose row is at or beyond their column's row_limit (skipped); status[1]: canonical values not below r (zeroed)
__global__ void __launch_bounds__(CS_BLOCK) k_cells_scatter(const CellSegs segs, uint64_t total, unsigned long long* status) {
  const uint64_t e = (uint64_t)blockIdx.x * CS_BLOCK + threadIdx.x;
  if (e >= total) return;
  uint32_t lo = 0, hi = segs.n_segs - 1;  // the last segment that starts at or before e: empty segments share their start with the
  while (lo < hi) {                       // next one and are passed over
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (e >= segs.start[mid]) lo = mid;
    else hi = mid - 1;
  }
  const uint32_t s = lo;
  const uint64_t off = e - segs.start[s];
  const uint32_t format = segs.format[s];
  uint64_t row = off;
  if (segs.rows[s]) row = segs.rows[s][off];
  if (row >= segs.row_limit[s]) {  // nothing is written outside the column's first row_limit rows, whatever the row list holds
    atomicAdd(&status[0], 1ull);
    return;
  }
  fe a;
  bool neg = false;
  if (format == CS_FMT_I64) {
    const long long v = reinterpret_cast<const long long*>(segs.values[s])[off];
    const unsigned long long mag = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;  // -2^63 -> 2^63
    a = fe_zero();
    a.v[0] = (uint32_t)mag;
    a.v[1] = (uint32_t)(mag >> 32);
    neg = v < 0;
  } else {
    a = fe_load(reinterpret_cast<const fe*>(segs.values[s]) + off);
  }
  fe r = a;  // Montgomery words are carried verbatim
  if (format == CS_FMT_CANONICAL) {
    uint32_t borrow;
    raw_sub_mod<Fr>(a, borrow);
    r = fe_zero();
    if (borrow) r = fe_to_mont<Fr>(a);
    else atomicAdd(&status[1], 1ull);
  } else if (format == CS_FMT_I64) {
    r = fe_to_mont<Fr>(a);
    if (neg) r = fe_neg<Fr>(r);
  }
  fe_store(segs.dst[s] + row, r);
}

static int scatter_cells(const h2mi_cells_source* cols, uint32_t n_cols, uint64_t host_mask, uint64_t status_out[2], h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (!status_out) return H2MI_EINVAL;
  status_out[0] = status_out[1] = 0;
  if (n_cols == 0) return H2MI_OK;
  if (!cols || n_cols > CS_MAX_SEGS) return H2MI_EINVAL;
  uint64_t total = 0;
  size_t stage_bytes = 0;  // host sources: values (padded to 16 bytes per source), then rows
  for (uint32_t i = 0; i < n_cols; i++) {
    const h2mi_cells_source& c = cols[i];
    if (c.count == 0) continue;
    if (c.format != 0 && c.format != CS_FMT_CANONICAL && c.format != CS_FMT_I64) return H2MI_EINVAL;
    const bool host = (host_mask >> i) & 1u;
    const uintptr_t value_align = c.format == CS_FMT_I64 ? 7u : 15u;
    if (!c.d_column || ((uintptr_t)c.d_column & 15u) || !c.values) return H2MI_EINVAL;
    if (!host && (((uintptr_t)c.values & value_align) || ((uintptr_t)c.rows & 3u))) return H2MI_EINVAL;
    total += c.count;
    if (total > ((uint64_t)1 << 32)) return H2MI_ERANGE;
    if (host) stage_bytes += ((c.count * (c.format == CS_FMT_I64 ? 8 : 32) + 15) & ~(size_t)15) + (c.rows ? ((c.count * 4 + 15) & ~(size_t)15) : 0);
  }
  if (total == 0) return H2MI_OK;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  hipStream_t s = pick_stream(stream);
  int rc = ensure_tmp(1 + (stage_bytes + 31) / 32, s);  // the status words, then the staged sources
  if (rc) return rc;
  unsigned long long* status = reinterpret_cast<unsigned long long*>(tmp_base());
  char* stage = reinterpret_cast<char*>(tmp_base() + 1);
  H2_HIP(hipMemsetAsync(status, 0, 16, s));
  CellSegs segs;
  memset(&segs, 0, sizeof(segs));
  segs.n_segs = n_cols;
  uint64_t at = 0;
  for (uint32_t i = 0; i < n_cols; i++) {
    const h2mi_cells_source& c = cols[i];
    segs.start[i] = at;
    if (c.count == 0) continue;
    segs.dst[i] = (fe*)c.d_column;
    segs.values[i] = c.values;
    segs.rows[i] = c.rows;
    segs.row_limit[i] = c.row_limit;
    segs.format[i] = c.format;
    if ((host_mask >> i) & 1u) {
      const size_t vb = c.count * (c.format == CS_FMT_I64 ? 8 : 32);
      H2_HIP(hipMemcpyAsync(stage, c.values, vb, hipMemcpyHostToDevice, s));
      segs.values[i] = stage;
      stage += (vb + 15) & ~(size_t)15;
      if (c.rows) {
        H2_HIP(hipMemcpyAsync(stage, c.rows, c.count * 4, hipMemcpyHostToDevice, s));
        segs.rows[i] = reinterpret_cast<const uint32_t*>(stage);
        stage += (c.count * 4 + 15) & ~(size_t)15;
      }
    }
    at += c.count;
  }
  segs.start[n_cols] = total;
  H2_LAUNCH("k_cells_scatter", k_cells_scatter, ceil_div_u32(total, CS_BLOCK), CS_BLOCK, 0, s, segs, total, status);
  rc = release_tmp(s);
  if (rc) return rc;
  unsigned long long v[2] = {0, 0};
  H2_HIP(hipMemcpyAsync(v, status, 16, hipMemcpyDeviceToHost, s));
  H2_HIP(hipStreamSynchronize(s));  // the status is the call's answer; the host sources are free from here on as well
  status_out[0] = v[0];
  status_out[1] = v[1];
  return H2MI_OK;
}

}  // namespace h2

using namespace h2;

extern "C" {

int h2mi_fr_scatter_cells_dev(const h2mi_cells_source* cols, uint32_t n_cols, uint64_t status_out[2], h2mi_stream_t stream) {
  return scatter_cells(cols, n_cols, 0, status_out, stream);
}
int h2mi_fr_scatter_cells_staged_dev(const h2mi_cells_source* cols, uint32_t n_cols, uint64_t host_mask, uint64_t status_out[2], h2mi_stream_t stream) {
  return scatter_cells(cols, n_cols, host_mask, status_out, stream);
}

}  // extern "C"
