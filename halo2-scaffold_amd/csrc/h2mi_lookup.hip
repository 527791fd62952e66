// libh2mi.so — the lookup argument's permuted columns on the device (BASELINE config 3).
//
// halo2_proofs plonk/lookup/prover.rs `permute_expression_pair` (reached from create_proof's `lookups.commit_permuted`;
// the reference selects a lookup table with LOOKUP_BITS, src/scaffold.rs:44-48,462): A' = the usable input rows sorted,
// S' = the table rearranged so that S'[j] = A'[j] wherever A' starts a new run and the table values not consumed that
// way fill the repeated rows.  The crate sorts 2^k field elements and walks a BTreeMap on one thread.
//
// Here (single-expression lookups: one input column against one fixed column, the range-check case): every valid input
// value IS a table value, and the table is fixed, so its distinct values are sorted once at keygen (host) and a proof
// needs no sort at all — a counting sort against that table:
//   k_lk_rank         rank of every input in the sorted table (binary search on canonical 256-bit values), histogram
//   scan              run starts of A'
//   k_lk_leftover     table multiplicity minus one for every value that occurs among the inputs; scan -> positions
//   k_lk_fill_input   A'[j] = value of the run containing j; marks repeated rows; scan -> repeated rows before j
//   k_lk_fill_table   S'[j] = A'[j] on a run start, else the (number of repeated rows after j)-th leftover value
//                     (the crate pops repeated rows from the END while walking the leftovers in ascending order)
// Integer / byte work over HBM-resident vectors: no field multiplication except the Montgomery -> canonical conversion
// of the inputs.
#include <algorithm>
#include <vector>

#include "fp.cuh"
#include "h2mi_internal.h"
#include "scan.cuh"

namespace h2 {

using Fr = FrP;

__device__ __forceinline__ int cmp256(const fe& a, const fe& b) {  // canonical little-endian words
#pragma unroll
  for (int i = 7; i >= 0; i--) {
    if (a.v[i] != b.v[i]) return a.v[i] < b.v[i] ? -1 : 1;
  }
  return 0;
}

// The histogram is built for the input a range check produces: a few limbs and then millions of zero rows, i.e. nearly
// every thread increments the same counter.  A device-scope atomic on one address retires at ~90 M/s here (measured:
// 47 ms for 2^22 rows), so equal ranks are first merged within the wavefront (ballot; one iteration when the wave is
// uniform), then within the workgroup through a 64-slot LDS table keyed by rank (a slot taken by another rank falls
// back to the global atomic), and only the table is flushed to HBM: 2^22 zero rows -> 4096 global atomics.
constexpr uint32_t LK_SLOTS = 64, LK_EMPTY = 0xFFFFFFFFu;
// `src`: this thread's input element, NULL for a thread beyond the rows.  -> the element's rank, LK_EMPTY for an input that is no table
// value and for a thread beyond the rows (k_lk_rank_cols stores it; the other kernels drop it)
__device__ __forceinline__ uint32_t lk_rank_body(const fe* src, const fe* sorted, uint32_t n_unique, uint32_t* cnt, uint32_t* missing) {
  __shared__ uint32_t hkey[LK_SLOTS], hcnt[LK_SLOTS];
  if (threadIdx.x < LK_SLOTS) {
    hkey[threadIdx.x] = LK_EMPTY;
    hcnt[threadIdx.x] = 0;
  }
  __syncthreads();
  uint32_t lo = LK_EMPTY, rank = LK_EMPTY;
  bool active = false;
  if (src) {
    const fe v = fe_from_mont<Fr>(fe_load(src));
    // first index with sorted[idx] >= v.  A range-check table holds 0 .. 2^bits - 1, where a value IS its rank: the guess "rank = low
    // word of v" is tried first (one load instead of seventeen dependent ones); any other table falls through to the binary search
    const uint32_t guess = min(v.v[0], n_unique - 1);
    if (cmp256(fe_load(&sorted[guess]), v) == 0) {
      lo = guess;
    } else {
      uint32_t hi = n_unique;
      lo = 0;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cmp256(fe_load(&sorted[mid]), v) < 0) lo = mid + 1;
        else hi = mid;
      }
    }
    if (lo < n_unique && cmp256(fe_load(&sorted[lo]), v) == 0) {
      active = true;
      rank = lo;
    } else {
      atomicAdd(missing, 1u);
    }
  }
  const uint32_t lane = threadIdx.x & 63u;
  for (;;) {
    const unsigned long long m = __ballot(active);
    if (!m) break;
    const int leader = __ffsll(m) - 1;
    const uint32_t v = (uint32_t)__shfl((int)lo, leader);
    const unsigned long long same = __ballot(active && lo == v);
    if ((int)lane == leader) {
      const uint32_t c = (uint32_t)__popcll(same);
      const uint32_t slot = v & (LK_SLOTS - 1);
      const uint32_t prev = atomicCAS(&hkey[slot], LK_EMPTY, v);
      if (prev == LK_EMPTY || prev == v) atomicAdd(&hcnt[slot], c);
      else atomicAdd(&cnt[v], c);
    }
    if (active && lo == v) active = false;
  }
  __syncthreads();
  if (threadIdx.x < LK_SLOTS && hkey[threadIdx.x] != LK_EMPTY) atomicAdd(&cnt[hkey[threadIdx.x]], hcnt[threadIdx.x]);
  return rank;
}
__global__ void __launch_bounds__(1024) k_lk_rank(const fe* input, uint32_t u, const fe* sorted, uint32_t n_unique, uint32_t* cnt, uint32_t* missing) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  lk_rank_body(i < u ? &input[i] : nullptr, sorted, n_unique, cnt, missing);
}
// logUp over several input sets [restated in DESIGN.md 4.5]: the usable rows of gridDim.y consecutive vectors (`stride` elements apart)
// ranked in ONE launch into the same histogram and the same counter of absent inputs.  blockIdx.y is the set, so a workgroup (and its
// LDS table) stays inside one set, no index passes 32 bits and the all-equal input still costs one global atomic per workgroup
__global__ void __launch_bounds__(1024) k_lk_rank_sets(const fe* inputs, size_t stride, uint32_t u, const fe* sorted, uint32_t n_unique, uint32_t* cnt,
                                                       uint32_t* missing) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  lk_rank_body(i < u ? &inputs[(size_t)blockIdx.y * stride + i] : nullptr, sorted, n_unique, cnt, missing);
}

// logUp against a table sorted at keygen (h2mi_plonk_logup_rank_cols_dev) [restated in DESIGN.md 4.5]: the columns come through a
// pointer list (advice columns are no consecutive vectors), blockIdx.y is the column as above, and every usable row's rank is KEPT:
// ranks[j 2^k + i], which the ranked running sum gathers by.  An absent input stores LK_EMPTY there
struct RankCols {
  const fe* col[H2MI_MAX_LOGUP_INPUTS];
};
__global__ void __launch_bounds__(1024) k_lk_rank_cols(RankCols cols, size_t stride, uint32_t u, const fe* sorted, uint32_t n_unique, uint32_t* cnt,
                                                       uint32_t* missing, uint32_t* ranks) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t rank = lk_rank_body(i < u ? &cols.col[blockIdx.y][i] : nullptr, sorted, n_unique, cnt, missing);
  if (i < u) ranks[(size_t)blockIdx.y * stride + i] = rank;
}

// Membership alone, for the witness check (h2mi_prover_check): is the input of usable row i one of the table's distinct values?  The
// binary search of k_lk_rank without its histogram.  report = {absent rows, the smallest of them}, from {0, 0xffffffff}; votes are
// merged within the wavefront first (lane order is row order), so a witness whose inputs are all in the table issues no atomic.
__global__ void __launch_bounds__(256) k_lk_member(const fe* input, uint32_t u, const fe* sorted, uint32_t n_unique, uint32_t* report) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool absent = false;
  if (i < u) {
    const fe v = fe_from_mont<Fr>(fe_load(&input[i]));
    uint32_t lo = min(v.v[0], n_unique - 1);  // a range-check table: the value is its rank
    if (cmp256(fe_load(&sorted[lo]), v) != 0) {
      uint32_t hi = n_unique;
      lo = 0;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cmp256(fe_load(&sorted[mid]), v) < 0) lo = mid + 1;
        else hi = mid;
      }
      absent = lo >= n_unique || cmp256(fe_load(&sorted[lo]), v) != 0;
    }
  }
  const unsigned long long m = __ballot(absent);
  if (m && (threadIdx.x & 63u) == (uint32_t)(__ffsll(m) - 1)) {
    atomicAdd(&report[0], (uint32_t)__popcll(m));
    atomicMin(&report[1], i);
  }
}

// The shuffle argument's witness check: both sides hold u values, sorted into distinct values with multiplicities.  Row i fails when
// its input value occurs more often among the inputs than on the shuffle side (absent there: zero times).  k_lk_member's binary search,
// once per side; the same vote.
__device__ __forceinline__ uint32_t sf_mult_of(const fe& v, const fe* sorted, const uint32_t* mult, uint32_t n_unique) {
  uint32_t lo = 0, hi = n_unique;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (cmp256(fe_load(&sorted[mid]), v) < 0) lo = mid + 1;
    else hi = mid;
  }
  return lo < n_unique && cmp256(fe_load(&sorted[lo]), v) == 0 ? mult[lo] : 0u;
}
__global__ void __launch_bounds__(256) k_sf_member(const fe* input, uint32_t u, const fe* in_sorted, const uint32_t* in_mult, uint32_t n_in,
                                                    const fe* sh_sorted, const uint32_t* sh_mult, uint32_t n_sh, uint32_t* report) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool excess = false;
  if (i < u) {
    const fe v = fe_from_mont<Fr>(fe_load(&input[i]));
    excess = sf_mult_of(v, in_sorted, in_mult, n_in) > sf_mult_of(v, sh_sorted, sh_mult, n_sh);
  }
  const unsigned long long m = __ballot(excess);
  if (m && (threadIdx.x & 63u) == (uint32_t)(__ffsll(m) - 1)) {
    atomicAdd(&report[0], (uint32_t)__popcll(m));
    atomicMin(&report[1], i);
  }
}

__global__ void __launch_bounds__(256) k_lk_leftover(const uint32_t* cnt, const uint32_t* mult, uint32_t n_unique, uint32_t* left, uint32_t* missing) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_unique) return;
  const uint32_t used = cnt[r] ? 1u : 0u;
  if (used > mult[r]) {  // cannot happen for values found in the table; keeps the arithmetic unsigned-safe
    atomicAdd(missing, 1u);
    left[r] = 0;
  } else {
    left[r] = mult[r] - used;
  }
}

// largest r < m with start[r] <= x, where start is an exclusive scan (non-decreasing) and start[m] = total > x
__device__ __forceinline__ uint32_t run_of(const uint32_t* start, uint32_t m, uint32_t x) {
  uint32_t lo = 0, hi = m;  // first index in [0, m] with start[idx] > x
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (start[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

__global__ void __launch_bounds__(256) k_lk_fill_input(const uint32_t* start, uint32_t n_unique, const fe* sorted_mont, uint32_t u, fe* a_perm,
                                                       uint32_t* repeated) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= u) return;
  const uint32_t r = run_of(start, n_unique, j);
  fe_store(&a_perm[j], fe_load(&sorted_mont[r]));
  repeated[j] = j != start[r] ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_lk_fill_table(const uint32_t* repeated, const uint32_t* rep_before, const uint32_t* lstart, uint32_t n_unique,
                                                       const fe* sorted_mont, const fe* a_perm, uint32_t u, fe* s_perm) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= u) return;
  if (!repeated[j]) {
    fe_store(&s_perm[j], fe_load(&a_perm[j]));
    return;
  }
  const uint32_t after = rep_before[u] - rep_before[j] - 1;  // repeated rows with a larger index
  fe_store(&s_perm[j], fe_load(&sorted_mont[run_of(lstart, n_unique, after)]));
}

// ---- per-proof tables: the distinct values of a vector, sorted (h2mi_fr_sort_unique_dev) -----------------------------------------
// A table that is compressed with theta, or holds advice, is known only inside the proof, so the keygen-time host sort above does
// not apply.  LSD radix sort, 8-bit digits, over an INDEX permutation (the 32-byte keys are converted to canonical form once and
// never move): per digit a tile histogram laid out [digit][tile], ONE exclusive scan of it (scan.cuh) = every tile's output
// offset for every digit, and a stable scatter.  k_su_canon also ORs key ^ key[0] over all keys: the host reads those 32 bytes back
// once and launches passes only for the byte positions on which the keys differ at all — 2 of 32 for a 16-bit counting table, none
// when all keys are equal, and no round trip per pass.  The chosen bytes are packed into one 64-bit word per key that moves with
// its index, so a pass reads and writes 12 coalesced bytes per key.  With more than eight differing bytes (theta-compressed tables:
// uniform keys) the sort runs on the top 2 log2(count) + 16 bits of them, rounded up to bytes — enough to order uniform keys but
// for a chance of about 2^-15 (the top byte of a 254-bit value carries six bits) — and k_su_heads counts neighbours the prefix left unresolved; that count comes back with n_unique, and only if it
// is not zero the keys are sorted again on every differing byte, by gathering passes.  Then run heads -> scan -> distinct values
// and multiplicities.
constexpr uint32_t RS_ITEMS = 4, RS_TILE = 256 * RS_ITEMS;
__device__ __forceinline__ uint32_t rs_digit(const uint32_t* canon, uint32_t i, uint32_t byte) {
  return (canon[8 * (size_t)i + (byte >> 2)] >> ((byte & 3u) * 8u)) & 0xffu;
}
__global__ void __launch_bounds__(256) k_su_canon(const fe* in, uint32_t count, fe* canon, uint32_t* idx, uint32_t* diff /* 8 */) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (i < count) {
    const fe v = fe_from_mont<Fr>(fe_load(&in[i])), first = fe_from_mont<Fr>(fe_load(&in[0]));
    fe_store(&canon[i], v);
    idx[i] = i;
#pragma unroll
    for (int w = 0; w < 8; w++) d[w] = v.v[w] ^ first.v[w];
  }
#pragma unroll
  for (int w = 0; w < 8; w++) {
#pragma unroll
    for (int o = 32; o; o >>= 1) d[w] |= (uint32_t)__shfl_xor((int)d[w], o);
  }
  // same-address atomics retire at ~90 M/s (see k_lk_rank): a wavefront adds only bits the mask does not show yet — it saturates
  // after a few wavefronts, and a stale read costs one redundant atomic, never a missing bit
  if ((threadIdx.x & 63u) == 0) {
#pragma unroll
    for (int w = 0; w < 8; w++)
      if (d[w] & ~((volatile uint32_t*)diff)[w]) atomicOr(&diff[w], d[w]);
  }
}
// A pass reads its digit from the 32-byte key through the index (PACKED = false: exact for any input), or from a 64-bit word that
// holds up to eight chosen key bytes and travels with the index (PACKED = true: coalesced 12 bytes per key instead of a gather).
struct RsBytes {
  uint8_t pos[8];
};
__global__ void __launch_bounds__(256) k_rs_pack(const uint32_t* canon, uint32_t count, RsBytes bytes, uint32_t nb, uint64_t* packed) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  uint64_t v = 0;
  for (uint32_t j = 0; j < nb; j++) v |= (uint64_t)rs_digit(canon, i, bytes.pos[j]) << (8 * j);
  packed[i] = v;
}
template <bool PACKED>
__global__ void __launch_bounds__(256) k_rs_hist(const uint32_t* canon, const uint64_t* packed, const uint32_t* idx, uint32_t count, uint32_t byte,
                                                 uint32_t ntiles, uint32_t* hist) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * RS_TILE;
  for (uint32_t r = 0; r < RS_ITEMS; r++) {
    const uint32_t j = base + r * 256 + threadIdx.x;
    if (j < count) atomicAdd(&h[PACKED ? (uint32_t)(packed[j] >> (8 * byte)) & 0xffu : rs_digit(canon, idx[j], byte)], 1u);
  }
  __syncthreads();
  hist[threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}
// stable: a tile is taken in RS_ITEMS rounds of 256 consecutive positions; within a round a key's place among the equal digits is
// (equal digits in earlier wavefronts) + (equal digits in lower lanes of its own: eight ballots match the digit)
template <bool PACKED>
__global__ void __launch_bounds__(256) k_rs_scatter(const uint32_t* canon, const uint64_t* packed, uint64_t* packed_out, const uint32_t* src, uint32_t* dst,
                                                    uint32_t count, uint32_t byte, uint32_t ntiles, const uint32_t* offs) {
  __shared__ uint32_t base[256], wcnt[4][256];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  base[tid] = offs[tid * ntiles + blockIdx.x];
#pragma unroll
  for (int w = 0; w < 4; w++) wcnt[w][tid] = 0;
  __syncthreads();
  for (uint32_t r = 0; r < RS_ITEMS; r++) {
    const uint32_t j = blockIdx.x * RS_TILE + r * 256 + tid;
    const bool active = j < count;
    const uint32_t id = active ? src[j] : 0u;
    const uint64_t pk = PACKED && active ? packed[j] : 0ull;
    const uint32_t d = !active ? 0u : PACKED ? (uint32_t)(pk >> (8 * byte)) & 0xffu : rs_digit(canon, id, byte);
    unsigned long long peers = __ballot(active);
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
    if (active && rank == 0) wcnt[wave][d] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (active) {
      uint32_t pos = base[d] + rank;
      for (uint32_t w = 0; w < wave; w++) pos += wcnt[w][d];
      if (pos < count) {  // always true (the offsets are a scan of this pass's histogram)
        dst[pos] = id;
        if (PACKED) packed_out[pos] = pk;
      }
    }
    __syncthreads();
    base[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
#pragma unroll
    for (int w = 0; w < 4; w++) wcnt[w][tid] = 0;
    __syncthreads();
  }
}
__global__ void __launch_bounds__(256) k_su_iota(uint32_t* idx, uint32_t count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) idx[i] = i;
}
// packed != NULL: the keys were sorted on a prefix of their differing bytes; two neighbours with equal prefixes and different keys
// are a tie the prefix did not resolve (counted: the caller then sorts again on every byte)
__global__ void __launch_bounds__(256) k_su_heads(const fe* canon, const uint32_t* idx, const uint64_t* packed, uint32_t count, uint32_t* head, uint32_t* ties) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  const bool differ = j == 0 || cmp256(fe_load(&canon[idx[j]]), fe_load(&canon[idx[j - 1]])) != 0;
  head[j] = differ ? 1u : 0u;
  if (packed && j && differ && packed[j] == packed[j - 1]) atomicAdd(ties, 1u);
}
__global__ void __launch_bounds__(256) k_su_emit(const fe* canon, const fe* in, const uint32_t* idx, const uint32_t* head, const uint32_t* rank, uint32_t count,
                                                 fe* out_canon, fe* out_mont, uint32_t* start, uint32_t* first) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count || !head[j]) return;
  const uint32_t r = rank[j], i = idx[j];  // r < count: at most one head per position
  fe_store(&out_canon[r], fe_load(&canon[i]));
  fe_store(&out_mont[r], fe_load(&in[i]));
  start[r] = j;
  // the sort is stable over an index permutation that starts as the identity: a run's head is its value's lowest position in `in`
  if (first) first[r] = i;
}
// logUp multiplicities [restated in DESIGN.md 4.5]: the count of every distinct table value goes to the table's first row that holds
// it, as a field element in the memory format (Montgomery); d_m is zero everywhere else (cleared by the caller)
__global__ void __launch_bounds__(256) k_logup_scatter(const uint32_t* cnt, const uint32_t* first, uint32_t n_unique, uint32_t u, fe* m) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_unique || !cnt[r]) return;
  const uint32_t row = first[r];
  if (row >= u) return;  // always false: first rows are positions of the u sorted values
  fe c = fe_zero();
  c.v[0] = cnt[r];
  fe_store(&m[row], fe_to_mont<Fr>(c));
}
__global__ void __launch_bounds__(256) k_su_mult(const uint32_t* start, const uint32_t* total, uint32_t count, uint32_t* mult) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x, n_unique = *total;
  if (r >= n_unique || r >= count) return;
  mult[r] = (r + 1 < n_unique ? start[r + 1] : count) - start[r];
}

// words of scratch h2mi_fr_sort_unique_dev lays out for `count` keys (every part starts on a multiple of 4)
static size_t su_scratch_words(uint32_t count) {
  const uint32_t c4 = (count + 3u) & ~3u, hm = 256 * ceil_div_u32(count, RS_TILE);
  const uint32_t nseg = ceil_div_u32(std::max(hm, c4), SCAN_SEG_BINS) + 1, nseg4 = (nseg + 3u) & ~3u;
  return 8 * (size_t)count + 6 * (size_t)c4 + 2 * ((size_t)hm + 4) + 3 * ((size_t)c4 + 4) + nseg4 + 8;
}

static uint32_t* g_lk_scratch = nullptr;
static size_t g_lk_words = 0;
static hipEvent_t g_lk_event = nullptr;     // last use of the scratch: a caller on another stream queues behind it
static hipStream_t g_lk_stream = nullptr;

static int scan_u32(const uint32_t* in, uint32_t* out, uint32_t m /* multiple of 4 */, uint32_t* segsum, hipStream_t s) {
  const uint32_t nseg = ceil_div_u32(m, SCAN_SEG_BINS);
  if (nseg > 1) H2_LAUNCH("k_scan_segsum", k_scan_segsum<SCAN_SEG_BINS>, nseg, 1024, 0, s, in, m, segsum);
  H2_LAUNCH("k_scan_seg_lookup", k_scan_seg<SCAN_SEG_BINS>, dim3(nseg, 1), 1024, 0, s, in, out, (const uint32_t*)nullptr, (uint32_t*)nullptr, m, (const uint32_t*)segsum);
  return H2MI_OK;
}

// the scratch grows behind a device synchronisation (a launch of an earlier call may still read it)
static int lk_scratch_reserve(size_t words) {
  if (g_lk_words >= words) return H2MI_OK;
  if (g_lk_scratch) {
    H2_HIP(hipDeviceSynchronize());
    H2_HIP(hipFree(g_lk_scratch));
    g_lk_scratch = nullptr;
    g_lk_words = 0;
  }
  hipError_t e = hipMalloc((void**)&g_lk_scratch, words * 4);
  if (e == hipErrorOutOfMemory) return H2MI_ENOMEM;
  H2_HIP(e);
  g_lk_words = words;
  return H2MI_OK;
}

// h2mi_shutdown: the scratch and its event belong to the device that is being torn down
void lookup_teardown() {
  if (g_lk_scratch) H2_IGNORE(hipFree(g_lk_scratch));
  if (g_lk_event) H2_IGNORE(hipEventDestroy(g_lk_event));
  g_lk_scratch = nullptr;
  g_lk_words = 0;
  g_lk_event = nullptr;
  g_lk_stream = nullptr;
}

}  // namespace h2

using namespace h2;

extern "C" {

int h2mi_plonk_lookup_permute_dev(const void* d_input, const void* d_table_sorted, const void* d_table_sorted_mont, const void* d_table_mult,
                                  uint32_t n_unique, uint32_t k, uint32_t usable_rows, void* d_permuted_input, void* d_permuted_table,
                                  uint64_t* not_in_table_out, h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  // not_in_table_out is mandatory: with inputs outside the table the permuted columns are not a permutation at all (the
  // crate fails the proof with ConstraintSystemFailure), so a caller must not be able to overlook the count
  if (!d_input || !d_table_sorted || !d_table_sorted_mont || !d_table_mult || !d_permuted_input || !d_permuted_table || !not_in_table_out ||
      n_unique == 0)
    return H2MI_EINVAL;
  if (k == 0 || k > H2MI_MAX_LOG_N || usable_rows == 0 || usable_rows >= ((uint64_t)1 << k) || n_unique > usable_rows) return H2MI_ERANGE;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  {
    int rc0 = use_device(0);  // single-process n-device mode: the argument's vectors live on the primary device
    if (rc0) return rc0;
  }
  hipStream_t s = pick_stream(stream);
  const uint32_t u = usable_rows;
  const uint32_t mu = (n_unique + 3u) & ~3u, uu = (u + 3u) & ~3u;  // scan lengths (multiples of 4; the pads are zero)
  const uint32_t nseg = ceil_div_u32(std::max(mu, uu), SCAN_SEG_BINS) + 1;
  // scratch (words): cnt[mu+4] start[mu+4] left[mu+4] lstart[mu+4] rep[uu+4] rep_before[uu+4] segsum[nseg] missing[4]
  const size_t words = 4 * ((size_t)mu + 4) + 2 * ((size_t)uu + 4) + nseg + 4;
  {
    int rcs = lk_scratch_reserve(words);
    if (rcs) return rcs;
  }
  uint32_t* cnt = g_lk_scratch;
  uint32_t* start = cnt + mu + 4;
  uint32_t* left = start + mu + 4;
  uint32_t* lstart = left + mu + 4;
  uint32_t* rep = lstart + mu + 4;
  uint32_t* rep_before = rep + uu + 4;
  uint32_t* segsum = rep_before + uu + 4;
  uint32_t* missing = segsum + nseg;
  if (g_lk_event && g_lk_stream != s) H2_HIP(hipStreamWaitEvent(s, g_lk_event, 0));
  H2_HIP(hipMemsetAsync(g_lk_scratch, 0, words * 4, s));
  const fe* in = (const fe*)d_input;
  const fe* sorted = (const fe*)d_table_sorted;
  const fe* sorted_mont = (const fe*)d_table_sorted_mont;
  H2_LAUNCH("k_lk_rank", k_lk_rank, ceil_div_u32(u, 1024), 1024, 0, s, in, u, sorted, n_unique, cnt, missing);
  int rc = scan_u32(cnt, start, mu, segsum, s);
  if (rc) return rc;
  H2_LAUNCH("k_lk_leftover", k_lk_leftover, ceil_div_u32(n_unique, 256), 256, 0, s, (const uint32_t*)cnt, (const uint32_t*)d_table_mult, n_unique, left, missing);
  rc = scan_u32(left, lstart, mu, segsum, s);
  if (rc) return rc;
  H2_LAUNCH("k_lk_fill_input", k_lk_fill_input, ceil_div_u32(u, 256), 256, 0, s, (const uint32_t*)start, n_unique, sorted_mont, u, (fe*)d_permuted_input, rep);
  rc = scan_u32(rep, rep_before, uu, segsum, s);
  if (rc) return rc;
  // rep_before[uu] holds the total; the fill kernel reads it at index u: identical when u is a multiple of 4, else the
  // zero pads make rep_before[u] == rep_before[uu]
  H2_LAUNCH("k_lk_fill_table", k_lk_fill_table, ceil_div_u32(u, 256), 256, 0, s, (const uint32_t*)rep, (const uint32_t*)rep_before, (const uint32_t*)lstart,
            n_unique, sorted_mont, (const fe*)d_permuted_input, u, (fe*)d_permuted_table);
  if (!g_lk_event) H2_HIP(hipEventCreateWithFlags(&g_lk_event, hipEventDisableTiming));
  H2_HIP(hipEventRecord(g_lk_event, s));
  g_lk_stream = s;
  uint32_t m = 0;  // the crate fails the proof (ConstraintSystemFailure) when an input is not in the table
  H2_HIP(hipMemcpyAsync(&m, missing, 4, hipMemcpyDeviceToHost, s));
  H2_HIP(hipStreamSynchronize(s));
  *not_in_table_out = m;
  return H2MI_OK;
}

int h2mi_plonk_lookup_member_dev(const void* d_input, const void* d_table_sorted, uint32_t n_unique, uint32_t usable_rows, uint32_t report_out[2],
                                 h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (!d_input || !d_table_sorted || !report_out || n_unique == 0) return H2MI_EINVAL;
  if (usable_rows == 0 || usable_rows > (1u << H2MI_MAX_LOG_N) || n_unique > usable_rows) return H2MI_ERANGE;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  {
    int rc0 = use_device(0);
    if (rc0) return rc0;
  }
  hipStream_t s = pick_stream(stream);
  {
    int rcs = lk_scratch_reserve(4);
    if (rcs) return rcs;
  }
  // the first two words of the scratch; a permutation of an earlier call on another stream may still read them
  if (g_lk_event && g_lk_stream != s) H2_HIP(hipStreamWaitEvent(s, g_lk_event, 0));
  const uint32_t init[2] = {0, 0xffffffffu};
  H2_HIP(hipMemcpyAsync(g_lk_scratch, init, 8, hipMemcpyHostToDevice, s));
  H2_LAUNCH("k_lk_member", k_lk_member, ceil_div_u32(usable_rows, 256), 256, 0, s, (const fe*)d_input, usable_rows, (const fe*)d_table_sorted, n_unique,
            g_lk_scratch);
  H2_HIP(hipMemcpyAsync(report_out, g_lk_scratch, 8, hipMemcpyDeviceToHost, s));
  H2_HIP(hipStreamSynchronize(s));
  return H2MI_OK;
}

int h2mi_plonk_shuffle_member_dev(const void* d_input, const void* d_input_sorted, const void* d_input_mult, uint32_t n_input_unique,
                                  const void* d_shuffle_sorted, const void* d_shuffle_mult, uint32_t n_shuffle_unique, uint32_t usable_rows,
                                  uint32_t report_out[2], h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (!d_input || !d_input_sorted || !d_input_mult || !d_shuffle_sorted || !d_shuffle_mult || !report_out || n_input_unique == 0 || n_shuffle_unique == 0)
    return H2MI_EINVAL;
  if (usable_rows == 0 || usable_rows > (1u << H2MI_MAX_LOG_N) || n_input_unique > usable_rows || n_shuffle_unique > usable_rows) return H2MI_ERANGE;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  {
    int rc0 = use_device(0);
    if (rc0) return rc0;
  }
  hipStream_t s = pick_stream(stream);
  {
    int rcs = lk_scratch_reserve(4);
    if (rcs) return rcs;
  }
  if (g_lk_event && g_lk_stream != s) H2_HIP(hipStreamWaitEvent(s, g_lk_event, 0));
  const uint32_t init[2] = {0, 0xffffffffu};
  H2_HIP(hipMemcpyAsync(g_lk_scratch, init, 8, hipMemcpyHostToDevice, s));
  H2_LAUNCH("k_sf_member", k_sf_member, ceil_div_u32(usable_rows, 256), 256, 0, s, (const fe*)d_input, usable_rows, (const fe*)d_input_sorted,
            (const uint32_t*)d_input_mult, n_input_unique, (const fe*)d_shuffle_sorted, (const uint32_t*)d_shuffle_mult, n_shuffle_unique, g_lk_scratch);
  H2_HIP(hipMemcpyAsync(report_out, g_lk_scratch, 8, hipMemcpyDeviceToHost, s));
  H2_HIP(hipStreamSynchronize(s));
  return H2MI_OK;
}

// h2mi_fr_sort_unique_dev's body; d_first (optional, u32 x count): per distinct value the lowest position of d_in that holds it
static int sort_unique(const void* d_in, uint32_t count, void* d_sorted_canonical, void* d_sorted_mont, void* d_mult, void* d_first,
                       uint32_t* n_unique_out, h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (!d_in || !d_sorted_canonical || !d_sorted_mont || !d_mult || !n_unique_out) return H2MI_EINVAL;
  if (count == 0 || count > (1u << H2MI_MAX_LOG_N)) return H2MI_ERANGE;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  {
    int rc0 = use_device(0);
    if (rc0) return rc0;
  }
  hipStream_t s = pick_stream(stream);
  const uint32_t c4 = (count + 3u) & ~3u, ntiles = ceil_div_u32(count, RS_TILE), hm = 256 * ntiles;  // hm: a multiple of 4
  const uint32_t nseg = ceil_div_u32(std::max(hm, c4), SCAN_SEG_BINS) + 1, nseg4 = (nseg + 3u) & ~3u;
  // scratch (words; every part starts on a multiple of 4): canon[8 count] packed0[2 c4] packed1[2 c4] idx0[c4] idx1[c4] hist[hm+4]
  // offs[hm+4] head[c4+4] rank[c4+4] start[c4+4] segsum[nseg4] diff[8]
  const size_t words = su_scratch_words(count);
  {
    int rcs = lk_scratch_reserve(words);
    if (rcs) return rcs;
  }
  uint32_t* canon_w = g_lk_scratch;
  uint64_t* packed[2] = {(uint64_t*)(canon_w + 8 * (size_t)count), (uint64_t*)(canon_w + 8 * (size_t)count + 2 * (size_t)c4)};
  uint32_t* idx[2] = {canon_w + 8 * (size_t)count + 4 * (size_t)c4, canon_w + 8 * (size_t)count + 5 * (size_t)c4};
  uint32_t* hist = idx[1] + c4;
  uint32_t* offs = hist + hm + 4;
  uint32_t* head = offs + hm + 4;
  uint32_t* rank = head + c4 + 4;  // rank[c4]: n_unique (the scan's total); rank[c4 + 1]: ties the prefix sort left
  uint32_t* start = rank + c4 + 4;
  uint32_t* segsum = start + c4 + 4;
  uint32_t* diff = segsum + nseg4;
  fe* canon = (fe*)canon_w;
  const fe* in = (const fe*)d_in;
  const size_t tail_words = 3 * ((size_t)c4 + 4) + nseg4 + 8;
  if (g_lk_event && g_lk_stream != s) H2_HIP(hipStreamWaitEvent(s, g_lk_event, 0));
  H2_HIP(hipMemsetAsync(head, 0, tail_words * 4, s));  // the scans' pads, the tie count, the difference mask
  const uint32_t grid = ceil_div_u32(count, 256);
  H2_LAUNCH("k_su_canon", k_su_canon, grid, 256, 0, s, in, count, canon, idx[0], diff);
  uint32_t mask[8];
  H2_HIP(hipMemcpyAsync(mask, diff, 32, hipMemcpyDeviceToHost, s));
  H2_HIP(hipStreamSynchronize(s));
  std::vector<uint32_t> differing;  // byte positions on which the keys differ at all, ascending: elsewhere a pass is the identity
  for (uint32_t byte = 0; byte < 32; byte++)
    if ((mask[byte >> 2] >> ((byte & 3u) * 8u)) & 0xffu) differing.push_back(byte);
  uint32_t log_count = 0;
  while (((uint64_t)1 << log_count) < count) log_count++;
  const uint32_t prefix = std::min<uint32_t>(8, (2 * log_count + 16 + 7) / 8);  // bytes of a prefix sort
  const bool exact = differing.size() <= 8;                                      // every differing byte fits the packed word
  const uint32_t nb = exact ? (uint32_t)differing.size() : prefix;
  int cur = 0;
  if (nb) {
    RsBytes bytes;
    memset(&bytes, 0, sizeof(bytes));
    for (uint32_t j = 0; j < nb; j++) bytes.pos[j] = (uint8_t)differing[differing.size() - nb + j];  // the top nb of them, ascending
    H2_LAUNCH("k_rs_pack", k_rs_pack, grid, 256, 0, s, (const uint32_t*)canon_w, count, bytes, nb, packed[0]);
    for (uint32_t j = 0; j < nb; j++) {
      H2_LAUNCH("k_rs_hist", k_rs_hist<true>, ntiles, 256, 0, s, (const uint32_t*)canon_w, (const uint64_t*)packed[cur], (const uint32_t*)idx[cur], count, j,
                ntiles, hist);
      int rc = scan_u32(hist, offs, hm, segsum, s);
      if (rc) return rc;
      H2_LAUNCH("k_rs_scatter", k_rs_scatter<true>, ntiles, 256, 0, s, (const uint32_t*)canon_w, (const uint64_t*)packed[cur], packed[cur ^ 1],
                (const uint32_t*)idx[cur], idx[cur ^ 1], count, j, ntiles, (const uint32_t*)offs);
      cur ^= 1;
    }
  }
  uint32_t result[2] = {0, 0};  // n_unique, unresolved ties
  auto finish = [&](const uint64_t* pk) -> int {
    H2_LAUNCH("k_su_heads", k_su_heads, grid, 256, 0, s, (const fe*)canon, (const uint32_t*)idx[cur], pk, count, head, rank + c4 + 1);
    int rc = scan_u32(head, rank, c4, segsum, s);
    if (rc) return rc;
    H2_LAUNCH("k_su_emit", k_su_emit, grid, 256, 0, s, (const fe*)canon, in, (const uint32_t*)idx[cur], (const uint32_t*)head, (const uint32_t*)rank, count,
              (fe*)d_sorted_canonical, (fe*)d_sorted_mont, start, (uint32_t*)d_first);
    H2_LAUNCH("k_su_mult", k_su_mult, grid, 256, 0, s, (const uint32_t*)start, (const uint32_t*)(rank + c4), count, (uint32_t*)d_mult);
    H2_HIP(hipMemcpyAsync(result, rank + c4, 8, hipMemcpyDeviceToHost, s));
    H2_HIP(hipStreamSynchronize(s));
    return H2MI_OK;
  };
  int rc = finish(exact || !nb ? nullptr : (const uint64_t*)packed[cur]);
  if (rc) return rc;
  if (result[1]) {  // keys that agree on the whole prefix: sort again on every differing byte
    H2_HIP(hipMemsetAsync(head, 0, (tail_words - 8) * 4, s));
    cur = 0;
    H2_LAUNCH("k_su_iota", k_su_iota, grid, 256, 0, s, idx[0], count);
    for (uint32_t byte : differing) {
      H2_LAUNCH("k_rs_hist", k_rs_hist<false>, ntiles, 256, 0, s, (const uint32_t*)canon_w, (const uint64_t*)nullptr, (const uint32_t*)idx[cur], count, byte,
                ntiles, hist);
      rc = scan_u32(hist, offs, hm, segsum, s);
      if (rc) return rc;
      H2_LAUNCH("k_rs_scatter", k_rs_scatter<false>, ntiles, 256, 0, s, (const uint32_t*)canon_w, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                (const uint32_t*)idx[cur], idx[cur ^ 1], count, byte, ntiles, (const uint32_t*)offs);
      cur ^= 1;
    }
    rc = finish(nullptr);
    if (rc) return rc;
  }
  if (!g_lk_event) H2_HIP(hipEventCreateWithFlags(&g_lk_event, hipEventDisableTiming));
  H2_HIP(hipEventRecord(g_lk_event, s));
  g_lk_stream = s;
  const uint32_t total = result[0];
  *n_unique_out = total;
  return H2MI_OK;
}

int h2mi_fr_sort_unique_dev(const void* d_in, uint32_t count, void* d_sorted_canonical, void* d_sorted_mont, void* d_mult, uint32_t* n_unique_out,
                            h2mi_stream_t stream) {
  return sort_unique(d_in, count, d_sorted_canonical, d_sorted_mont, d_mult, nullptr, n_unique_out, stream);
}

int h2mi_fr_sort_unique_first_dev(const void* d_in, uint32_t count, void* d_sorted_canonical, void* d_sorted_mont, void* d_mult, void* d_first,
                                  uint32_t* n_unique_out, h2mi_stream_t stream) {
  if (!d_first) return H2MI_EINVAL;
  return sort_unique(d_in, count, d_sorted_canonical, d_sorted_mont, d_mult, d_first, n_unique_out, stream);
}

int h2mi_plonk_logup_multiplicity_dev(const void* d_input, const void* d_table, uint32_t k, uint32_t usable_rows, void* d_m, uint64_t* not_in_table_out,
                                      h2mi_stream_t stream) {
  return h2mi_plonk_logup_multiplicity_sets_dev(d_input, 1, d_table, k, usable_rows, d_m, not_in_table_out, stream);
}

int h2mi_plonk_logup_multiplicity_sets_dev(const void* d_inputs, uint32_t n_inputs, const void* d_table, uint32_t k, uint32_t usable_rows, void* d_m,
                                           uint64_t* not_in_table_out, h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (!d_inputs || !d_table || !d_m || !not_in_table_out) return H2MI_EINVAL;  // the count is mandatory, as for the permuted columns
  if (n_inputs == 0 || n_inputs > H2MI_MAX_LOGUP_INPUTS) return H2MI_EINVAL;
  if (k == 0 || k > H2MI_MAX_LOG_N || usable_rows == 0 || usable_rows >= ((uint64_t)1 << k)) return H2MI_ERANGE;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  {
    int rc0 = use_device(0);
    if (rc0) return rc0;
  }
  hipStream_t s = pick_stream(stream);
  const uint32_t u = usable_rows, u4 = (u + 3u) & ~3u;
  // behind the sort's own scratch (words): sorted[8 u4] sorted_mont[8 u4] mult[u4] first[u4] cnt[u4] missing[4]; reserved in one piece
  // BEFORE the sort, whose own reservation then finds room and moves nothing.  The input sets need none: they share cnt and missing
  const size_t base = (su_scratch_words(u) + 3u) & ~(size_t)3u, words = base + 19 * (size_t)u4 + 4;
  {
    int rcs = lk_scratch_reserve(words);
    if (rcs) return rcs;
  }
  uint32_t* sorted = g_lk_scratch + base;
  uint32_t* sorted_mont = sorted + 8 * (size_t)u4;
  uint32_t* mult = sorted_mont + 8 * (size_t)u4;
  uint32_t* first = mult + u4;
  uint32_t* cnt = first + u4;
  uint32_t* missing = cnt + u4;
  uint32_t n_unique = 0;
  int rc = sort_unique(d_table, u, sorted, sorted_mont, mult, first, &n_unique, stream);  // ONE sort, whatever n_inputs; waits for an earlier call on another stream
  if (rc) return rc;
  if (n_unique == 0 || n_unique > u) return H2MI_EHIP;
  H2_HIP(hipMemsetAsync(cnt, 0, ((size_t)u4 + 4) * 4, s));
  H2_HIP(hipMemsetAsync(d_m, 0, (size_t)u * 32, s));  // rows 0 .. u - 1; the blinding rows behind them are the caller's
  if (n_inputs == 1) {
    H2_LAUNCH("k_lk_rank", k_lk_rank, ceil_div_u32(u, 1024), 1024, 0, s, (const fe*)d_inputs, u, (const fe*)sorted, n_unique, cnt, missing);
  } else {
    H2_LAUNCH("k_lk_rank_sets", k_lk_rank_sets, dim3(ceil_div_u32(u, 1024), n_inputs), 1024, 0, s, (const fe*)d_inputs, (size_t)1 << k, u,
              (const fe*)sorted, n_unique, cnt, missing);
  }
  H2_LAUNCH("k_logup_scatter", k_logup_scatter, ceil_div_u32(n_unique, 256), 256, 0, s, (const uint32_t*)cnt, (const uint32_t*)first, n_unique, u, (fe*)d_m);
  if (!g_lk_event) H2_HIP(hipEventCreateWithFlags(&g_lk_event, hipEventDisableTiming));
  H2_HIP(hipEventRecord(g_lk_event, s));
  g_lk_stream = s;
  uint32_t m = 0;
  H2_HIP(hipMemcpyAsync(&m, missing, 4, hipMemcpyDeviceToHost, s));
  H2_HIP(hipStreamSynchronize(s));
  *not_in_table_out = m;
  return H2MI_OK;
}

int h2mi_plonk_logup_rank_cols_dev(const void* const* d_inputs, uint32_t n_inputs, const void* d_sorted_canonical, uint32_t n_unique, const void* d_first,
                                   uint32_t k, uint32_t usable_rows, void* d_ranks, void* d_counts, void* d_m, uint64_t* not_in_table_out,
                                   h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (!d_inputs || !d_sorted_canonical || !d_first || !d_ranks || !d_counts || !d_m || !not_in_table_out || n_unique == 0) return H2MI_EINVAL;
  if (n_inputs == 0 || n_inputs > H2MI_MAX_LOGUP_INPUTS) return H2MI_EINVAL;
  RankCols cols;
  memset(&cols, 0, sizeof(cols));
  for (uint32_t j = 0; j < n_inputs; j++) {
    if (!d_inputs[j]) return H2MI_EINVAL;
    cols.col[j] = (const fe*)d_inputs[j];
  }
  if (k == 0 || k > H2MI_MAX_LOG_N || usable_rows == 0 || usable_rows >= ((uint64_t)1 << k) || n_unique > usable_rows) return H2MI_ERANGE;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  {
    int rc0 = use_device(0);
    if (rc0) return rc0;
  }
  hipStream_t s = pick_stream(stream);
  const uint32_t u = usable_rows;
  {
    int rcs = lk_scratch_reserve(4);  // the counter of absent inputs; the histogram and the ranks are the caller's
    if (rcs) return rcs;
  }
  uint32_t* missing = g_lk_scratch;
  if (g_lk_event && g_lk_stream != s) H2_HIP(hipStreamWaitEvent(s, g_lk_event, 0));
  H2_HIP(hipMemsetAsync(missing, 0, 16, s));
  H2_HIP(hipMemsetAsync(d_counts, 0, (size_t)n_unique * 4, s));
  H2_HIP(hipMemsetAsync(d_m, 0, (size_t)u * 32, s));  // rows 0 .. u - 1; the blinding rows behind them are the caller's
  H2_LAUNCH("k_lk_rank_cols", k_lk_rank_cols, dim3(ceil_div_u32(u, 1024), n_inputs), 1024, 0, s, cols, (size_t)1 << k, u, (const fe*)d_sorted_canonical,
            n_unique, (uint32_t*)d_counts, missing, (uint32_t*)d_ranks);
  H2_LAUNCH("k_logup_scatter", k_logup_scatter, ceil_div_u32(n_unique, 256), 256, 0, s, (const uint32_t*)d_counts, (const uint32_t*)d_first, n_unique, u,
            (fe*)d_m);
  if (!g_lk_event) H2_HIP(hipEventCreateWithFlags(&g_lk_event, hipEventDisableTiming));
  H2_HIP(hipEventRecord(g_lk_event, s));
  g_lk_stream = s;
  uint32_t m = 0;
  H2_HIP(hipMemcpyAsync(&m, missing, 4, hipMemcpyDeviceToHost, s));
  H2_HIP(hipStreamSynchronize(s));
  *not_in_table_out = m;
  return H2MI_OK;
}

}  // extern "C"
