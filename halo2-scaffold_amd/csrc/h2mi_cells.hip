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
#include "scan.cuh"

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

// ---- the inverse: a device column -> its nonzero cells in row order (h2mi_fr_compact_cells_dev, include/h2mi.h) ---------------------------
//
// What a proving-key file stores of a fixed column.  The order is the row order and no byte depends on scheduling, so the
// compaction is a scan and holds no atomic: k_cells_count leaves one word per tile of CC_TILE rows, k_cells_prefix turns each column's
// words into exclusive offsets and the column's (count, last, fits64), k_cells_compact re-reads the tiles that hold anything and writes
// each cell at tile offset + its rank inside the tile (wave ballots, ranked through LDS).  Two passes over the data at most: the second
// skips a tile without cells (a sparse column) or beyond `last` (a dense one) on its word alone.  All columns of a call share the three
// launches; work is partitioned over the tiles of all columns, as k_cells_scatter partitions over cells.  A lane owns a row and moves
// its word as two 16-byte loads; a tile is CC_ROWS sweeps of the block over 256 consecutive rows, so its row order is (sweep, wave, lane).
// Montgomery -> canonical is fe_from_mont, the conversion of k_fe_to_repr (h2mi_serde.hip).
constexpr uint32_t CC_ROWS = 4;                     // rows per thread
constexpr uint32_t CC_TILE = CS_BLOCK * CC_ROWS;    // 1024 rows per workgroup
constexpr uint32_t CC_COUNT_MASK = 0x7ffu;          // tile word: cells (0 .. 1024) | last nonzero row of the tile + 1 (0 .. 1024) << 11 |
constexpr uint32_t CC_LAST_SHIFT = 11;              //            a value outside the 64-bit range << 31
constexpr uint32_t CC_NOFIT = 0x80000000u;
constexpr uint32_t CC_DENSE = 1u, CC_SPARSE = 2u;   // layout of a column's output (h2mi_cells_compacted.layout)

struct CompactSegs {
  const fe* src[CS_MAX_SEGS];
  void* values[CS_MAX_SEGS];        // pass 2: 8 or 32 bytes per cell
  uint32_t* rows[CS_MAX_SEGS];      // pass 2, sparse only
  uint32_t tile_start[CS_MAX_SEGS + 1];
  uint32_t row_limit[CS_MAX_SEGS];
  uint32_t last[CS_MAX_SEGS];       // pass 2, dense: rows 0 .. last - 1 are written, zeros included
  uint8_t layout[CS_MAX_SEGS];      // pass 2: 0 (nothing to write), CC_DENSE, CC_SPARSE
  uint8_t width[CS_MAX_SEGS];       // pass 2: 8 (int64) or 32 (canonical words)
  uint32_t n_segs;
};

__device__ __forceinline__ uint32_t compact_seg_of(const CompactSegs& segs, uint32_t tile) {
  uint32_t lo = 0, hi = segs.n_segs - 1;  // the last column whose tiles start at or before `tile`: columns without tiles are passed over
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (tile >= segs.tile_start[mid]) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}
// canonical v != 0 as a signed 64-bit integer: v <= 2^63 - 1 is v, v >= r - 2^63 is -(r - v) (what H2MI_CELLS_I64 decodes)
__device__ __forceinline__ bool canon_to_i64(const fe& v, unsigned long long& out) {
  uint32_t hi = 0;
#pragma unroll
  for (int i = 2; i < 8; i++) hi |= v.v[i];
  if (hi == 0 && v.v[1] < 0x80000000u) {
    out = ((unsigned long long)v.v[1] << 32) | v.v[0];
    return true;
  }
  uint32_t borrow;
  const fe n = raw_sub(fe_const<Fr>(Fr::MOD), v, borrow);  // 1 .. r - 1 for a reduced nonzero v
  hi = 0;
#pragma unroll
  for (int i = 2; i < 8; i++) hi |= n.v[i];
  const unsigned long long mag = ((unsigned long long)n.v[1] << 32) | n.v[0];
  out = 0ull - mag;
  return hi == 0 && mag <= 0x8000000000000000ull;
}

// pass 1: one word per tile
__global__ void __launch_bounds__(CS_BLOCK) k_cells_count(const CompactSegs segs, uint32_t* tile_words) {
  __shared__ uint32_t s_count[CS_BLOCK / 64], s_last[CS_BLOCK / 64], s_nofit[CS_BLOCK / 64];
  const uint32_t tile = blockIdx.x, s = compact_seg_of(segs, tile);
  const uint32_t row0 = (tile - segs.tile_start[s]) * CC_TILE, limit = segs.row_limit[s];
  const fe* src = segs.src[s];
  uint32_t count = 0, last = 0, nofit = 0;
#pragma unroll
  for (uint32_t j = 0; j < CC_ROWS; j++) {
    const uint32_t in_tile = j * CS_BLOCK + threadIdx.x, row = row0 + in_tile;
    if (row >= limit) continue;
    const fe a = fe_load(src + row);
    if (fe_is_zero(a)) continue;
    count++;
    last = in_tile + 1;
    unsigned long long as_i64;
    if (!canon_to_i64(fe_from_mont<Fr>(a), as_i64)) nofit = 1;
  }
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) {
    count += __shfl_xor(count, d);
    last = max(last, (uint32_t)__shfl_xor(last, d));
    nofit |= __shfl_xor(nofit, d);
  }
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_count[wave] = count;
    s_last[wave] = last;
    s_nofit[wave] = nofit;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    count = last = nofit = 0;
#pragma unroll
    for (uint32_t w = 0; w < CS_BLOCK / 64; w++) {
      count += s_count[w];
      last = max(last, s_last[w]);
      nofit |= s_nofit[w];
    }
    tile_words[tile] = count | (last << CC_LAST_SHIFT) | (nofit ? CC_NOFIT : 0u);
  }
}

// between the passes: one workgroup per column walks its tile words in order.  tile_off[t] = the cells of the column's earlier tiles;
// stats[4 s ..] = count, last, fits64, 0
__global__ void __launch_bounds__(CS_BLOCK) k_cells_prefix(const CompactSegs segs, const uint32_t* tile_words, uint32_t* tile_off, uint32_t* stats) {
  __shared__ uint32_t s_wave[CS_BLOCK / 64], s_last[CS_BLOCK / 64], s_nofit[CS_BLOCK / 64];
  const uint32_t s = blockIdx.x, t0 = segs.tile_start[s], t1 = segs.tile_start[s + 1];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry = 0, last = 0, nofit = 0;
  for (uint32_t base = t0; base < t1; base += CS_BLOCK) {  // uniform trip count: the barriers below are reached by every thread
    const uint32_t t = base + threadIdx.x;
    const uint32_t w = t < t1 ? tile_words[t] : 0u;
    const uint32_t c = w & CC_COUNT_MASK;
    if (c) last = (t - t0) * CC_TILE + ((w >> CC_LAST_SHIFT) & CC_COUNT_MASK);  // t ascends per thread: the latest tile wins
    nofit |= w & CC_NOFIT;
    const uint32_t inc = wave_incl_scan(c);
    __syncthreads();  // the previous round's s_wave has been read
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = carry, total = 0;
#pragma unroll
    for (uint32_t i = 0; i < CS_BLOCK / 64; i++) {
      if (i < wave) before += s_wave[i];
      total += s_wave[i];
    }
    if (t < t1) tile_off[t] = before + inc - c;
    carry += total;
  }
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) {
    last = max(last, (uint32_t)__shfl_xor(last, d));
    nofit |= __shfl_xor(nofit, d);
  }
  __syncthreads();
  if (lane == 0) {
    s_last[wave] = last;
    s_nofit[wave] = nofit;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    last = nofit = 0;
#pragma unroll
    for (uint32_t i = 0; i < CS_BLOCK / 64; i++) {
      last = max(last, s_last[i]);
      nofit |= s_nofit[i];
    }
    stats[4 * s] = carry;
    stats[4 * s + 1] = last;
    stats[4 * s + 2] = nofit ? 0u : 1u;
    stats[4 * s + 3] = 0;
  }
}

// pass 2: the cells, where the host's layout rule puts them.  Sparse: cell number tile_off + rank lands at rows[.] / values[.]; dense:
// row i < last lands at values[i], zeros included.  Nothing is written at or beyond count (sparse) or last (dense).
__global__ void __launch_bounds__(CS_BLOCK) k_cells_compact(const CompactSegs segs, const uint32_t* tile_words, const uint32_t* tile_off) {
  __shared__ uint32_t s_rank[CC_ROWS * (CS_BLOCK / 64)];
  const uint32_t tile = blockIdx.x, s = compact_seg_of(segs, tile);
  const uint32_t layout = segs.layout[s], width = segs.width[s];
  const uint32_t row0 = (tile - segs.tile_start[s]) * CC_TILE;
  // uniform over the workgroup: a tile the column's layout takes nothing from is not read again
  if (layout == 0 || (layout == CC_SPARSE && (tile_words[tile] & CC_COUNT_MASK) == 0) || (layout == CC_DENSE && row0 >= segs.last[s])) return;
  const uint32_t limit = layout == CC_DENSE ? segs.last[s] : segs.row_limit[s];  // last <= row_limit
  const fe* src = segs.src[s];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  fe a[CC_ROWS];
  bool nz[CC_ROWS];
  uint32_t rank[CC_ROWS];
#pragma unroll
  for (uint32_t j = 0; j < CC_ROWS; j++) {
    const uint32_t row = row0 + j * CS_BLOCK + threadIdx.x;
    a[j] = fe_zero();
    if (row < limit) a[j] = fe_load(src + row);
    nz[j] = !fe_is_zero(a[j]);
    const unsigned long long m = __ballot(nz[j]);
    rank[j] = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_rank[j * (CS_BLOCK / 64) + wave] = __popcll(m);
  }
  __syncthreads();
  const uint32_t off = tile_off[tile];
  unsigned long long* v64 = reinterpret_cast<unsigned long long*>(segs.values[s]);
  fe* v256 = reinterpret_cast<fe*>(segs.values[s]);
#pragma unroll
  for (uint32_t j = 0; j < CC_ROWS; j++) {
    const uint32_t row = row0 + j * CS_BLOCK + threadIdx.x;
    uint32_t before = 0;  // the cells of the sweeps and waves in front of this one
#pragma unroll
    for (uint32_t i = 0; i < CC_ROWS * (CS_BLOCK / 64); i++)
      if (i < j * (CS_BLOCK / 64) + wave) before += s_rank[i];
    const bool write = layout == CC_DENSE ? row < limit : nz[j];
    if (!write) continue;
    const uint32_t at = layout == CC_DENSE ? row : off + before + rank[j];
    if (layout == CC_SPARSE) segs.rows[s][at] = row;
    const fe c = nz[j] ? fe_from_mont<Fr>(a[j]) : a[j];
    if (width == 8) {
      unsigned long long x = 0;
      if (nz[j]) canon_to_i64(c, x);
      v64[at] = x;
    } else {
      fe_store(v256 + at, c);
    }
  }
}

constexpr size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }

static int compact_cells(h2mi_cells_compacted* cols, uint32_t n_cols, unsigned flags, h2mi_compact_alloc_fn alloc, void* alloc_ctx, h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (n_cols == 0) return H2MI_OK;
  if (!cols || n_cols > CS_MAX_SEGS || (flags & ~(H2MI_COMPACT_SPARSE | H2MI_COMPACT_WORDS))) return H2MI_EINVAL;
  CompactSegs segs;
  memset(&segs, 0, sizeof(segs));
  segs.n_segs = n_cols;
  uint64_t tiles = 0;
  for (uint32_t i = 0; i < n_cols; i++) {
    h2mi_cells_compacted& c = cols[i];
    c.count = 0;
    c.last = c.fits64 = c.layout = c.width = 0;
    c.rows = nullptr;
    c.values = nullptr;
    if (c.row_limit && (!c.d_column || ((uintptr_t)c.d_column & 15u))) return H2MI_EINVAL;
    if (c.row_limit > ((uint64_t)1 << H2MI_MAX_LOG_N)) return H2MI_ERANGE;
    segs.src[i] = (const fe*)c.d_column;
    segs.row_limit[i] = c.row_limit;
    segs.tile_start[i] = (uint32_t)tiles;
    tiles += (c.row_limit + CC_TILE - 1) / CC_TILE;
  }
  segs.tile_start[n_cols] = (uint32_t)tiles;  // <= 64 x 2^18
  for (uint32_t i = 0; i < n_cols; i++) cols[i].fits64 = 1;
  if (tiles == 0) return H2MI_OK;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  hipStream_t s = pick_stream(stream);
  // the tile words and offsets live beside the scratch: sizing the scratch from the counts may move it between the passes
  DevMem book;
  {
    hipError_t err = book.alloc((2 * tiles + 4 * CS_MAX_SEGS) * 4);
    if (err == hipErrorOutOfMemory) return H2MI_ENOMEM;
    H2_HIP(err);
  }
  // every way out of this function first waits for what it queued: the kernels read `book`, which is released behind this guard
  struct Drain {
    hipStream_t s;
    ~Drain() { H2_IGNORE(hipStreamSynchronize(s)); }
  } drain{s};
  uint32_t* tile_words = book.as<uint32_t>();
  uint32_t* tile_off = tile_words + tiles;
  uint32_t* d_stats = tile_off + tiles;
  H2_LAUNCH("k_cells_count", k_cells_count, (uint32_t)tiles, CS_BLOCK, 0, s, segs, tile_words);
  H2_LAUNCH("k_cells_prefix", k_cells_prefix, n_cols, CS_BLOCK, 0, s, segs, (const uint32_t*)tile_words, tile_off, d_stats);
  uint32_t stats[4 * CS_MAX_SEGS];
  H2_HIP(hipMemcpyAsync(stats, d_stats, 16 * n_cols, hipMemcpyDeviceToHost, s));
  H2_HIP(hipStreamSynchronize(s));  // the counts size the output
  size_t bytes = 0;
  std::vector<size_t> v_at(n_cols), r_at(n_cols);
  for (uint32_t i = 0; i < n_cols; i++) {
    h2mi_cells_compacted& c = cols[i];
    c.count = stats[4 * i];
    c.last = stats[4 * i + 1];
    c.fits64 = stats[4 * i + 2];
    if (c.count == 0) continue;
    c.width = (c.fits64 && !(flags & H2MI_COMPACT_WORDS)) ? 8 : 32;
    // the layout rule of DESIGN.md 3: dense where the rows 0 .. last - 1 cost no more than the row list does
    c.layout = (!(flags & H2MI_COMPACT_SPARSE) && (uint64_t)c.last * c.width <= c.count * (4 + (uint64_t)c.width)) ? CC_DENSE : CC_SPARSE;
    v_at[i] = bytes;
    bytes += pad16((c.layout == CC_DENSE ? (size_t)c.last : (size_t)c.count) * c.width);
    r_at[i] = bytes;
    if (c.layout == CC_SPARSE) bytes += pad16((size_t)c.count * 4);
  }
  if (!alloc || bytes == 0) return H2MI_OK;  // the counts alone
  char* arena = (char*)alloc(alloc_ctx, bytes);
  if (!arena) return H2MI_ENOMEM;
  {
    const int rc = ensure_tmp((bytes + 31) / 32, s);
    if (rc) return rc;
  }
  char* d_out = reinterpret_cast<char*>(tmp_base());
  for (uint32_t i = 0; i < n_cols; i++) {
    h2mi_cells_compacted& c = cols[i];
    if (c.count == 0) continue;
    segs.layout[i] = (uint8_t)c.layout;
    segs.width[i] = (uint8_t)c.width;
    segs.last[i] = c.last;
    segs.values[i] = d_out + v_at[i];
    c.values = arena + v_at[i];
    if (c.layout == CC_SPARSE) {
      segs.rows[i] = reinterpret_cast<uint32_t*>(d_out + r_at[i]);
      c.rows = reinterpret_cast<uint32_t*>(arena + r_at[i]);
    }
  }
  H2_LAUNCH("k_cells_compact", k_cells_compact, (uint32_t)tiles, CS_BLOCK, 0, s, segs, (const uint32_t*)tile_words, (const uint32_t*)tile_off);
  {
    const int rc = release_tmp(s);
    if (rc) return rc;
    // the padding between the columns' parts is never written by the kernel: only the parts cross
    for (uint32_t i = 0; i < n_cols; i++) {
      const h2mi_cells_compacted& c = cols[i];
      if (c.count == 0) continue;
      const size_t vb = (c.layout == CC_DENSE ? (size_t)c.last : (size_t)c.count) * c.width;
      H2_HIP(hipMemcpyAsync(arena + v_at[i], d_out + v_at[i], vb, hipMemcpyDeviceToHost, s));
      if (c.layout == CC_SPARSE) H2_HIP(hipMemcpyAsync(arena + r_at[i], d_out + r_at[i], (size_t)c.count * 4, hipMemcpyDeviceToHost, s));
    }
  }
  H2_HIP(hipStreamSynchronize(s));  // the cells are the call's answer
  return H2MI_OK;
}

}  // namespace h2

using namespace h2;

extern "C" {

int h2mi_fr_compact_cells_dev(h2mi_cells_compacted* cols, uint32_t n_cols, unsigned flags, h2mi_compact_alloc_fn alloc, void* alloc_ctx, h2mi_stream_t stream) {
  return compact_cells(cols, n_cols, flags, alloc, alloc_ctx, stream);
}

int h2mi_fr_scatter_cells_dev(const h2mi_cells_source* cols, uint32_t n_cols, uint64_t status_out[2], h2mi_stream_t stream) {
  return scatter_cells(cols, n_cols, 0, status_out, stream);
}
int h2mi_fr_scatter_cells_staged_dev(const h2mi_cells_source* cols, uint32_t n_cols, uint64_t host_mask, uint64_t status_out[2], h2mi_stream_t stream) {
  return scatter_cells(cols, n_cols, host_mask, status_out, stream);
}

}  // extern "C"
