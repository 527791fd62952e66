// libh2mi.so — the PLONK-specific vector kernels of create_proof: the permutation argument's and the lookup
// argument's grand products (plonk/permutation/prover.rs, plonk/lookup/prover.rs commit_product) and the quotient numerator
// (plonk/evaluation.rs evaluate_h + the division by X^n - 1) for the reference's StandardPlonk circuit
// (src/circuits/standard_plonk.rs:29-48) and the halo2-lib builders' constraint systems (src/scaffold.rs:379-485).
// Element-wise / scan work over HBM-resident vectors; reached from csrc/h2mi_prover.cpp.  Power tables and scratch vectors
// come from h2mi_ntt.hip (h2mi_fr_tables.h).  Split out of h2mi_ntt.hip in round 5; the kernels are unchanged.
#include <algorithm>
#include <vector>

#include "h2mi_expr.hpp"
#include "h2mi_fr_tables.h"
#include "scan.cuh"

namespace h2 {



// ---- quotient numerator of the reference's StandardPlonk circuit -------------------------
// halo2_proofs plonk/evaluation.rs `evaluate_h` specialised to src/circuits/standard_plonk.rs: one gate
// q_a a + q_b b + q_c c + q_ab a b + constant, three permutation sets of one column each; terms combined with
// powers of y; result already divided by X^n - 1 (its inverse on the coset repeats with period 2^(ext_k-k)).
// Element-wise over the extended domain; all vectors stay in HBM.
//
// Arithmetic: the lazy 29-bit-limb layer (f29.cuh) on the Montgomery-2^256 words as they lie in memory, WITHOUT
// converting them to its own radix.  f29_mul divides by 2^261, so the product of two memory-format values
// x 2^256, y 2^256 is x y 2^256 2^-5: every data-by-data product leaves one stray factor 2^-5.  Call a value "level L"
// when its limbs hold x 2^256 2^(-5 L): data and plain challenges are level 0, mul(level L1, level L2) is level
// L1 + L2 + 1, sums need equal levels.  The stray factors are paid by the HOST: h = sum_i y^(N-1-i) term_i is
// evaluated term by term (as many multiplications as Horner's rule), and the constant y^(N-1-i) for term i is
// handed over already multiplied by the power of 2^5 that brings this term back to level 0 — constants at negative
// levels (level -1 = the Montgomery-2^261 form: a multiplication by it keeps the level).  Terms that share a
// Lagrange factor (l_0, l_last, l_active) are summed before the one multiplication by it.  32 multiplications of
// ~210 instructions per point, against 36 of ~380 in the 32-bit-limb layer this kernel used before.
struct TInv {  // (X^n - 1)^-1 on the extended coset: 2^(extended_k - k) <= 16 distinct values
  fe v[16];
};
struct HConsts {
  fe beta_m1;            // beta at level -1: beta * sigma lands on level 0
  fe beta0, gamma0, one0;  // level 0: the plain Montgomery-2^256 words
  fe one_m2;             // one at level -2: brings a level-1 product (selector * advice) back to level 0
  fe cur[4];             // beta zeta DELTA^j at level 0: times X (level -1, straight from the power table) = level 0
  fe y[20];              // per-term powers of y at the level each use needs (layout: see the kernels / fill_* below)
  fe tinv[16];           // level -1
};
struct PlonkCosets {
  const fe* advice[3];
  const fe* fixed[5];
  const fe* sigma[3];
  const fe* z[3];
  const fe* l0;
  const fe* l_last;
  const fe* l_active;
};
__device__ __forceinline__ f29 hc(const fe& c) { return f29_unpack(c.v); }
__device__ __forceinline__ f29 hmul(const f29& a_lazy, const f29& b_norm) { return f29_mul<F9>(a_lazy, b_norm); }
// a - b + 2p, normalized (b normalized, value < 2p)
__device__ __forceinline__ f29 hsub(const f29& a, const f29& b) { return f29_normalize(f29_sub(a, b, F9::K2)); }
__device__ __forceinline__ void hstore(fe* dst, const f29& acc_lazy, const fe& tinv) {  // acc: lazy sum of <= 7 normalized values
  fe o;
  f29_pack(f29_reduce_canonical<F9>(f29_mul<F9>(f29_normalize(acc_lazy), hc(tinv))), o.v);
  fe_store(dst, o);
}

// y[] layout: [0] gate's q.a terms (level -2), [1] its q_ab a b term (-3), [2] its constant (-1), all times y^7;
// [3] [4] [5] the l_0 terms 1, 3, 4 (level -2); [6] the l_last term 2 (-3); [7] [8] [9] the permutation terms 5, 6, 7 (-3)
__global__ void __launch_bounds__(256) k_evaluate_h_standard_plonk(PlonkCosets c, uint32_t ext_k, uint32_t k, uint32_t last_rot, HConsts h,
                                                                    const fe* xlo, const fe* xhi, uint32_t xh, fe* out) {
  const uint32_t size = 1u << ext_k, rot = 1u << (ext_k - k);
  uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= size) return;
  const uint32_t r_next = (idx + rot) & (size - 1), r_last = (idx + size - last_rot * rot) & (size - 1);
  const f29 adv[3] = {load_unpack(&c.advice[0][idx]), load_unpack(&c.advice[1][idx]), load_unpack(&c.advice[2][idx])};
  // Sums of products at one level share ONE Montgomery reduction (f29_mul3 / f29_mul2, round 3): 33 products and 20 reductions per
  // point where every product had its own (33 + 33).  Operands of the shared forms are normalized (loads, constants, products,
  // hsub results); the one lazy operand — a three-term sum, limbs < 1.5 * 2^30 — sits where f29_mul2 allows it.
  // gate
  const f29 g1 = f29_mul3<F9>(load_unpack(&c.fixed[0][idx]), adv[0], load_unpack(&c.fixed[1][idx]), adv[1], load_unpack(&c.fixed[2][idx]), adv[2]);  // level 1
  const f29 g2 = hmul(hmul(load_unpack(&c.fixed[3][idx]), adv[0]), adv[1]);                          // level 2
  f29 acc = f29_mul3<F9>(g1, hc(h.y[0]), g2, hc(h.y[1]), load_unpack(&c.fixed[4][idx]), hc(h.y[2]));  // level 0
  const f29 zs[3] = {load_unpack(&c.z[0][idx]), load_unpack(&c.z[1][idx]), load_unpack(&c.z[2][idx])};
  const f29 one = hc(h.one0), gamma = hc(h.gamma0);
  // l_0 terms: (1 - z_0), (z_1 - z_0(w^last X)), (z_2 - z_1(w^last X))
  const f29 s0 = f29_mul3<F9>(hsub(one, zs[0]), hc(h.y[3]), hsub(zs[1], load_unpack(&c.z[0][r_last])), hc(h.y[4]),
                              hsub(zs[2], load_unpack(&c.z[1][r_last])), hc(h.y[5]));
  // l_last term: z_2^2 - z_2 = z_2 (z_2 - 1)
  const f29 tl = hmul(hmul(zs[2], hsub(zs[2], one)), hc(h.y[6]));
  // permutation terms: z_m(wX) (a_m + beta sigma_m + gamma) - z_m (a_m + beta DELTA^m X + gamma), X = zeta * extended_omega^idx
  const f29 X = pow2tab(xlo, xhi, xh, idx);
  auto term = [&](const f29& a_m, const f29& z_m, const fe* sigma, const fe* z_col, const fe& cur) {
    const f29 inner_l = f29_add(f29_add(a_m, hmul(load_unpack(&sigma[idx]), hc(h.beta_m1))), gamma);  // lazy: limbs < 1.5 * 2^30, value < 3.1 p
    const f29 inner_r = f29_normalize(f29_add(f29_add(a_m, hmul(X, hc(cur))), gamma));
    const f29 neg_r = f29_sub(f29_zero(), inner_r, F9::K4);                                           // 4p - inner_r: lazy, limbs < 2^30
    return f29_mul2<F9>(inner_l, load_unpack(&z_col[r_next]), neg_r, z_m);                            // left - right, level 1
  };
  const f29 d0 = term(adv[0], zs[0], c.sigma[0], c.z[0], h.cur[0]);
  const f29 d1 = term(adv[1], zs[1], c.sigma[1], c.z[1], h.cur[1]);
  const f29 d2 = term(adv[2], zs[2], c.sigma[2], c.z[2], h.cur[2]);
  const f29 sa = f29_mul3<F9>(d0, hc(h.y[7]), d1, hc(h.y[8]), d2, hc(h.y[9]));
  acc = f29_add(acc, f29_mul3<F9>(s0, load_unpack(&c.l0[idx]), tl, load_unpack(&c.l_last[idx]), sa, load_unpack(&c.l_active[idx])));
  hstore(&out[idx], acc, h.tinv[idx & (rot - 1)]);
}

// ---- permutation argument: the grand-product column z -------------------------------------
// create_proof builds, per chunk of columns, z[0] = start, z[i+1] = z[i] * prod_j (v_j[i] + beta delta^j omega^i
// + gamma) / prod_j (v_j[i] + beta sigma_j[i] + gamma) over the usable rows (plonk/permutation/prover.rs
// [RECALL], restated in oracle/plonk.py).  On the device: numerators / denominators per row, ONE field inversion
// for the whole column (prefix and suffix products of the denominators), then a prefix product of the ratios.
// Multiplicative scans over Fr in tiles of 1024 (local scan, scan of the tile totals, apply), forward or reverse.
// Everything between the numerator / denominator kernels and the final write lives in the lazy 29-bit-limb layer:
// the intermediate vectors hold canonical Montgomery-2^261 words, whose products stay in that domain
// (f29_mul(a 2^261, b 2^261) = a b 2^261); the columns themselves are Montgomery-2^256 and are converted once on the
// way in (one multiplication) and once on the way out (the mixed-domain product start * R, or a multiplication by 2^-5).
constexpr uint32_t MS_TILE = 1024;
__device__ __forceinline__ f29 ld261(const fe* p) { return f29_unpack(fe_load(p).v); }
__device__ __forceinline__ fe pack261(const f29& a_lt2p) {
  fe o;
  f29_pack(f29_reduce_canonical<F9>(a_lt2p), o.v);
  return o;
}
__device__ __forceinline__ fe one261() {
  fe o;
  f29_pack(f29_const<F9>(F9::ONE), o.v);
  return o;
}
__global__ void __launch_bounds__(256) k_mulscan_local(const fe* in, size_t n, int reverse, fe* local, fe* totals) {
  __shared__ fe tile[MS_TILE];
  __shared__ fe tprod[256];
  const uint32_t tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * MS_TILE;
  for (uint32_t r = 0; r < 4; r++) {  // logical position j; physical index n-1-j for a suffix scan
    size_t j = base + tid + 256 * r;
    tile[tid + 256 * r] = j < n ? fe_load(&in[reverse ? n - 1 - j : j]) : one261();
  }
  __syncthreads();
  const f29 p0 = f29_unpack(tile[4 * tid].v), p1 = f29_mul<F9>(p0, f29_unpack(tile[4 * tid + 1].v)), p2 = f29_mul<F9>(p1, f29_unpack(tile[4 * tid + 2].v)),
            p3 = f29_mul<F9>(p2, f29_unpack(tile[4 * tid + 3].v));
  tprod[tid] = pack261(p3);
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {  // inclusive scan of the 256 thread products (Hillis-Steele)
    fe v = one261();
    if (tid >= d) v = tprod[tid - d];
    __syncthreads();
    if (tid >= d) tprod[tid] = pack261(f29_mul<F9>(f29_unpack(tprod[tid].v), f29_unpack(v.v)));
    __syncthreads();
  }
  f29 left = f29_const<F9>(F9::ONE);
  if (tid) left = f29_unpack(tprod[tid - 1].v);
  __syncthreads();
  tile[4 * tid] = pack261(f29_mul<F9>(left, p0));
  tile[4 * tid + 1] = pack261(f29_mul<F9>(left, p1));
  tile[4 * tid + 2] = pack261(f29_mul<F9>(left, p2));
  tile[4 * tid + 3] = pack261(f29_mul<F9>(left, p3));
  __syncthreads();
  for (uint32_t r = 0; r < 4; r++) {
    size_t j = base + tid + 256 * r;
    if (j < n) fe_store(&local[reverse ? n - 1 - j : j], tile[tid + 256 * r]);
  }
  if (tid == 255) fe_store(&totals[blockIdx.x], tile[MS_TILE - 1]);
}
// exclusive scan of the tile totals: ONE workgroup of 1024 threads, each owning a run of consecutive totals (serial
// product), one Hillis-Steele scan over the 1024 run products, then the runs are walked again.  (Chunks of 256 with a
// running carry took 110 us for the 3072 totals of a three-column product: twelve dependent rounds of eight steps.)
__global__ void __launch_bounds__(1024) k_mulscan_offsets(const fe* totals, uint32_t nblocks, fe* offsets) {
  __shared__ fe tprod[1024];
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (nblocks + 1023) / 1024;
  const uint32_t lo = min(tid * per, nblocks), hi = min(lo + per, nblocks);
  f29 run = f29_const<F9>(F9::ONE);
  for (uint32_t b = lo; b < hi; b++) run = f29_mul<F9>(run, ld261(&totals[b]));
  tprod[tid] = pack261(run);
  __syncthreads();
  const uint32_t used = (nblocks + per - 1) / per;  // threads that own a run: the scan need not reach beyond them (six tiles
                                                     // of a sparse grand product: three rounds instead of ten, 0.2 ms -> 0.06)
  for (uint32_t d = 1; d < used; d <<= 1) {
    fe v = one261();
    if (tid >= d) v = tprod[tid - d];
    __syncthreads();
    if (tid >= d) tprod[tid] = pack261(f29_mul<F9>(f29_unpack(tprod[tid].v), f29_unpack(v.v)));
    __syncthreads();
  }
  f29 acc = f29_const<F9>(F9::ONE);
  if (tid) acc = f29_unpack(tprod[tid - 1].v);
  for (uint32_t b = lo; b < hi; b++) {
    fe_store(&offsets[b], pack261(f29_mul<F9>(acc, f29_const<F9>(F9::ONE))));
    acc = f29_mul<F9>(acc, ld261(&totals[b]));
  }
}
__global__ void __launch_bounds__(256) k_mulscan_apply(fe* local, const fe* offsets, size_t n, int reverse) {
  size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n || j < MS_TILE) return;  // the first tile has offset one
  fe* p = &local[reverse ? n - 1 - j : j];
  fe_store(p, pack261(f29_mul<F9>(ld261(p), ld261(&offsets[j / MS_TILE]))));
}

// ---- assigned cells: num / den with ONE field inversion per call, den = 0 -> 0 ---------------------------------------------------------
// [RECALL halo2_proofs v2023_02_02 plonk/assigned.rs Assigned::evaluate, poly.rs batch_invert_assigned, ff's BatchInvert — restated from
// memory: a Rational(n, d) evaluates to n d^-1, a zero denominator is skipped by the batched inversion and the cell evaluates to 0.]
// Montgomery's trick in tiles of ASG_TILE elements, three launches whatever the size (the ratios() chain above has no rule for zeros and
// takes every element through HBM about ten times):
//   (a) k_assigned_tile_products: every workgroup multiplies its tile's denominators, a zero replaced by one, and writes ONE word;
//   (b) k_assigned_tile_inverses: one workgroup — exclusive prefix and suffix products of the tile products (runs per thread as in
//       k_mulscan_offsets), the ONE inversion (of the grand total, wavefront-uniform), tileinv_t = pre_t suf_t / total;
//   (c) k_assigned_finish: every workgroup reloads its tile, scans the 256 thread products both ways in LDS, forms
//       den_i^-1 = (left)(right) tileinv_t (the other denominators of the thread), multiplies by the numerator, SELECTS zero where the
//       denominator was zero (no branch around a multiplication) and stores the canonical Montgomery-2^256 word — contiguous or through a row list.
// A thread owns four consecutive elements: 128 B (denominators alone) or 256 B (pairs) of whole cache lines, no staging through LDS.
// The products live in the lazy 29-bit-limb layer as Montgomery-2^261 values; num 2^256 times (den^-1 2^261) / 2^261 is the result in the
// columns' own form, so the way out costs no conversion.
constexpr uint32_t ASG_TILE = 1024;
constexpr uint32_t ASG_MAX_SEGS = 64;  // = H2MI_MAX_ADVICE / H2MI_MAX_FIXED: every column of a call in one chain
// where element e of the staging vector lands: segment s covers e in [start[s], start[s + 1]); dst[s] + (e - start[s]), or
// dst[s] + rows[s][e - start[s]] with a row list.  2 KB by value.
struct AssignedSegs {
  fe* dst[ASG_MAX_SEGS];
  const uint32_t* rows[ASG_MAX_SEGS];
  uint64_t start[ASG_MAX_SEGS + 1];
  uint32_t n_segs;
};
// one operand as a normalized Montgomery-2^261 value: from the Montgomery-2^256 word, or from a canonical integer (counted when not below r)
__device__ __forceinline__ f29 asg_load261(const fe* p, int canonical, uint32_t& bad) {
  const fe w = fe_load(p);
  uint32_t borrow;
  raw_sub_mod<Fr>(w, borrow);
  bad += (canonical && !borrow) ? 1u : 0u;
  return f29_mul<F9>(f29_unpack(w.v), canonical ? f29_const<F9>(F9::R2) : f29_const<F9>(F9::TO261));
}
__device__ __forceinline__ f29 asg_select(bool c, const f29& a, const f29& b) {  // c ? a : b, limb by limb
  f29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = c ? a.v[i] : b.v[i];
  return r;
}
// the thread's four denominators (one beyond n; a zero replaced by one and remembered in `zero`), Montgomery-2^261
__device__ __forceinline__ void asg_load_dens(const fe* in, uint32_t stride, size_t n, size_t e0, int canonical, f29 d[4], bool zero[4], uint32_t& bad) {
  const f29 one = f29_const<F9>(F9::ONE);
#pragma unroll
  for (int r = 0; r < 4; r++) {
    d[r] = one;
    zero[r] = false;
    if (e0 + r < n) {
      const f29 v = asg_load261(&in[(e0 + r) * stride + (stride - 1)], canonical, bad);
      zero[r] = f29_is_zero_mod<F9>(v);
      d[r] = asg_select(zero[r], one, v);
    }
  }
}
__global__ void __launch_bounds__(256) k_assigned_tile_products(const fe* in, uint32_t stride, size_t n, int canonical, fe* totals, unsigned long long* invalid) {
  __shared__ fe tprod[256];
  const uint32_t tid = threadIdx.x;
  f29 d[4];
  bool zero[4];
  uint32_t bad = 0;
  asg_load_dens(in, stride, n, (size_t)blockIdx.x * ASG_TILE + 4 * tid, canonical, d, zero, bad);
  if (bad) atomicAdd(invalid, (unsigned long long)bad);
  tprod[tid] = pack261(f29_mul<F9>(f29_mul<F9>(d[0], d[1]), f29_mul<F9>(d[2], d[3])));
  __syncthreads();
  for (uint32_t w = 128; w; w >>= 1) {
    if (tid < w) tprod[tid] = pack261(f29_mul<F9>(f29_unpack(tprod[tid].v), f29_unpack(tprod[tid + w].v)));
    __syncthreads();
  }
  if (tid == 0) fe_store(&totals[blockIdx.x], tprod[0]);
}
// inclusive Hillis-Steele scan over sh[0 .. used) — forward (prefix) or backward (suffix); every thread of the workgroup calls it
__device__ __forceinline__ void asg_scan(fe* sh, uint32_t tid, uint32_t used, bool backward) {
  for (uint32_t dd = 1; dd < used; dd <<= 1) {
    const bool on = backward ? tid + dd < used : (tid >= dd && tid < used);
    fe v = one261();
    if (on) v = sh[backward ? tid + dd : tid - dd];
    __syncthreads();
    if (on) sh[tid] = pack261(f29_mul<F9>(f29_unpack(sh[tid].v), f29_unpack(v.v)));
    __syncthreads();
  }
}
__global__ void __launch_bounds__(1024) k_assigned_tile_inverses(const fe* totals, uint32_t ntiles, fe* tileinv) {
  __shared__ fe sh[1024];
  __shared__ fe sh_inv;
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (ntiles + 1023) / 1024;
  const uint32_t lo = min(tid * per, ntiles), hi = min(lo + per, ntiles);
  const uint32_t used = (ntiles + per - 1) / per;  // threads that own a run
  f29 run = f29_const<F9>(F9::ONE);
  for (uint32_t b = lo; b < hi; b++) run = f29_mul<F9>(run, ld261(&totals[b]));
  const fe mine = pack261(run);
  sh[tid] = mine;
  __syncthreads();
  asg_scan(sh, tid, used, false);
  f29 left = f29_const<F9>(F9::ONE);
  if (tid && tid < used) left = f29_unpack(sh[tid - 1].v);
  if (tid < 64) {  // (total 2^261) read as Montgomery-2^256 is (32 total) 2^256; its inverse times 2^10 is total^-1 2^261 (k_fr_inv_one).
    fe inv = fe_inv_ds<Fr>(sh[used - 1]);  // Every lane inverts the same value: the division steps' branches are wavefront-uniform
    for (int q = 0; q < 10; q++) inv = fe_dbl<Fr>(inv);
    if (tid == 0) sh_inv = inv;
  }
  __syncthreads();
  sh[tid] = mine;
  __syncthreads();
  asg_scan(sh, tid, used, true);
  f29 right = f29_const<F9>(F9::ONE);
  if (tid + 1 < used) right = f29_unpack(sh[tid + 1].v);
  // the run again: forward with the prefix (times 1 / total), backward with the suffix
  f29 acc = f29_mul<F9>(left, f29_unpack(sh_inv.v));
  for (uint32_t b = lo; b < hi; b++) {
    fe_store(&tileinv[b], pack261(acc));
    acc = f29_mul<F9>(acc, ld261(&totals[b]));
  }
  acc = right;
  for (uint32_t b = hi; b-- > lo;) {
    fe_store(&tileinv[b], pack261(f29_mul<F9>(ld261(&tileinv[b]), acc)));
    acc = f29_mul<F9>(acc, ld261(&totals[b]));
  }
}
__global__ void __launch_bounds__(256) k_assigned_finish(const fe* in, uint32_t stride, size_t n, int canonical, const fe* tileinv, AssignedSegs segs,
                                                         unsigned long long* invalid) {
  __shared__ fe pre[256], suf[256];
  const uint32_t tid = threadIdx.x;
  const size_t e0 = (size_t)blockIdx.x * ASG_TILE + 4 * tid;
  f29 d[4];
  bool zero[4];
  uint32_t bad = 0;
  asg_load_dens(in, stride, n, e0, canonical, d, zero, bad);  // the denominators were counted in pass (a)
  bad = 0;
  const f29 p1 = f29_mul<F9>(d[0], d[1]), p2 = f29_mul<F9>(p1, d[2]);  // products from the left ...
  const f29 s2 = f29_mul<F9>(d[2], d[3]), s1 = f29_mul<F9>(d[1], s2);  // ... and from the right
  const fe q = pack261(f29_mul<F9>(p1, s2));
  pre[tid] = q;
  suf[tid] = q;
  __syncthreads();
  for (uint32_t dd = 1; dd < 256; dd <<= 1) {  // pre: inclusive prefix products of the thread products; suf: inclusive suffix products
    fe vp = one261(), vs = one261();
    if (tid >= dd) vp = pre[tid - dd];
    if (tid + dd < 256) vs = suf[tid + dd];
    __syncthreads();
    pre[tid] = pack261(f29_mul<F9>(f29_unpack(pre[tid].v), f29_unpack(vp.v)));
    suf[tid] = pack261(f29_mul<F9>(f29_unpack(suf[tid].v), f29_unpack(vs.v)));
    __syncthreads();
  }
  // c = tileinv * (thread products to the left) * (thread products to the right); threads 0 and 255 have one side only and discard a product
  const f29 ti = ld261(&tileinv[blockIdx.x]);
  f29 c = asg_select(tid != 0, f29_mul<F9>(ti, f29_unpack(pre[tid ? tid - 1 : 0].v)), ti);
  c = asg_select(tid < 255, f29_mul<F9>(c, f29_unpack(suf[tid < 255 ? tid + 1 : 255].v)), c);
  // the numerator as the plain Montgomery-2^256 word: times (1 / d) 2^261, divided by 2^261, is the cell.  A canonical integer gets its
  // 2^256 first (times 2^517 / 2^261); batch_invert's numerator is the Montgomery one
  const f29 c517 = f29_mul<F9>(f29_const<F9>(F9::R2), f29_const<F9>(F9::TO256));
  uint32_t seg = 0;
  auto finish = [&](uint32_t r, const f29& inv, bool was_zero) {
    const size_t e = e0 + r;
    if (e >= n) return;
    f29 num = f29_const<F9>(F9::TO256);
    if (stride == 2) {
      const fe w = fe_load(&in[2 * e]);
      uint32_t borrow;
      raw_sub_mod<Fr>(w, borrow);
      bad += (canonical && !borrow) ? 1u : 0u;
      num = f29_unpack(w.v);
      if (canonical) num = f29_mul<F9>(num, c517);  // uniform over the launch
    }
    const f29 v = f29_reduce_canonical<F9>(f29_mul<F9>(num, inv));
    fe o;
    f29_pack(asg_select(was_zero, f29_zero(), v), o.v);
    while (seg + 1 < segs.n_segs && e >= segs.start[seg + 1]) seg++;
    const size_t off = e - segs.start[seg];
    fe_store(&segs.dst[seg][segs.rows[seg] ? (size_t)segs.rows[seg][off] : off], o);
  };
  // 1 / d_r = c * (the thread's other three denominators)
  finish(0, f29_mul<F9>(c, s1), zero[0]);
  finish(1, f29_mul<F9>(f29_mul<F9>(c, d[0]), s2), zero[1]);
  finish(2, f29_mul<F9>(f29_mul<F9>(c, p1), d[3]), zero[2]);
  finish(3, f29_mul<F9>(c, p2), zero[3]);
  if (bad) atomicAdd(invalid, (unsigned long long)bad);
}

// up to H2MI_FLEX_MAX_PERM columns by value: 3.1 KB of the 4 KB a launch's arguments may take
struct PermArgs {
  const fe* value[H2MI_FLEX_MAX_PERM];
  const fe* sigma[H2MI_FLEX_MAX_PERM];
  fe beta_delta[H2MI_FLEX_MAX_PERM];  // beta * delta^(column index), Mont256
  fe beta, gamma;
  uint32_t m;
};
// factors of one column at one row (Mont261, lazy sums below 6p): v + beta delta^j omega^i + gamma, v + beta sigma + gamma
__device__ __forceinline__ void perm_factors(const PermArgs& a, uint32_t j, size_t i, const f29& w, f29& numf, f29& denf) {
  const f29 v = f29_from_mont256<F9>(fe_load(&a.value[j][i]).v);
  const f29 g = f29_from_mont256<F9>(a.gamma.v);
  const f29 vg = f29_add(v, g);
  numf = f29_add(vg, f29_mul<F9>(f29_from_mont256<F9>(a.beta_delta[j].v), w));
  denf = f29_add(vg, f29_mul<F9>(f29_from_mont256<F9>(a.beta.v), f29_from_mont256<F9>(fe_load(&a.sigma[j][i]).v)));
}
// rows i < u: num = prod_j (v_j + beta delta^j omega^i + gamma), den = prod_j (v_j + beta sigma_j + gamma); one beyond
__global__ void __launch_bounds__(256) k_perm_numden(PermArgs a, size_t n, uint32_t u, const fe* wlo, const fe* whi, uint32_t wh, fe* num, fe* den) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  f29 pn = f29_const<F9>(F9::ONE), pd = pn;
  if (i < u) {
    const f29 w = pow2tab(wlo, whi, wh, (uint32_t)i);  // omega^i (Mont261)
    for (uint32_t j = 0; j < a.m; j++) {
      f29 nf, df;
      perm_factors(a, j, i, w, nf, df);
      pn = f29_mul<F9>(nf, pn);
      pd = f29_mul<F9>(df, pd);
    }
  }
  fe_store(&num[i], pack261(pn));
  fe_store(&den[i], pack261(pd));
}
// the same for every set of a permutation argument at once: t = set * u + i over the concatenated usable rows
// (set = chunk of `chunk` consecutive columns); the running product then chains the sets by itself
__global__ void __launch_bounds__(256) k_perm_numden_sets(PermArgs a, uint32_t chunk, size_t total, uint32_t u, const fe* wlo, const fe* whi, uint32_t wh,
                                                           const uint32_t* active, fe* num, fe* den) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // element of the (compacted) concatenation
  if (e >= total) return;
  const size_t t = active ? active[e] : e;
  const uint32_t set = (uint32_t)(t / u), i = (uint32_t)(t - (size_t)set * u);
  const f29 w = pow2tab(wlo, whi, wh, i);  // omega^i (Mont261)
  f29 pn = f29_const<F9>(F9::ONE), pd = pn;
  for (uint32_t j = set * chunk; j < a.m && j < (set + 1) * chunk; j++) {
    f29 nf, df;
    perm_factors(a, j, i, w, nf, df);
    pn = f29_mul<F9>(nf, pn);
    pd = f29_mul<F9>(df, pd);
  }
  fe_store(&num[e], pack261(pn));
  fe_store(&den[e], pack261(pd));
}
struct ZOut {
  fe* z[H2MI_FLEX_MAX_PERM];
};
// z_set[i] = product of every ratio before (set, i) in the concatenated order: R[set * u + i - 1], one at the very start.
// With an `active` list (sorted positions whose ratio can differ from one, see h2mi_plonk_permutation_products_sparse_dev)
// R holds the prefix products over those positions only: z = R[c - 1], c = number of active positions before (set, i).
__global__ void __launch_bounds__(256) k_perm_write_sets(const fe* R, uint32_t u, ZOut out, const uint32_t* active, uint32_t n_active) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, set = blockIdx.y;
  if (i > u) return;
  size_t t = (size_t)set * u + i;
  if (active) {
    uint32_t lo = 0, hi = n_active;  // first index with active[idx] >= t
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (active[mid] < t) lo = mid + 1;
      else hi = mid;
    }
    t = lo;
  }
  fe o = fe_one<Fr>();
  if (t) {
    if (active) o = fe_load(&R[t - 1]);  // sparse form: R was brought to the memory format once per position (k_perm_to_mont256)
    else f29_to_mont256<F9>(ld261(&R[t - 1]), o.v);
  }
  fe_store(&out.z[set][i], o);
}
// the sparse form's prefix products, Montgomery-2^261 -> the columns' Montgomery-2^256, once per active position instead
// of once per row of every z column (the rows between two positions repeat one value)
__global__ void __launch_bounds__(256) k_perm_to_mont256(fe* R, uint32_t count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  fe o;
  f29_to_mont256<F9>(ld261(&R[i]), o.v);
  fe_store(&R[i], o);
}
// lookup argument's grand product (plonk/lookup/prover.rs commit_product), single-expression lookups:
// num_i = (a_i + beta)(t_i + gamma), den_i = (a'_i + beta)(s'_i + gamma), i < u
__global__ void __launch_bounds__(256) k_lookup_numden(const fe* input, const fe* table, const fe* pin, const fe* ptab, fe beta, fe gamma, uint32_t u,
                                                        fe* num, fe* den) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= u) return;
  const f29 b = f29_from_mont256<F9>(beta.v), g = f29_from_mont256<F9>(gamma.v);
  auto lift = [](const fe* p) { return f29_from_mont256<F9>(fe_load(p).v); };
  // the second operand of a product must be normalized: sums of two values below 2p are carried first
  fe_store(&num[i], pack261(f29_mul<F9>(f29_add(lift(&input[i]), b), f29_normalize(f29_add(lift(&table[i]), g)))));
  fe_store(&den[i], pack261(f29_mul<F9>(f29_add(lift(&pin[i]), b), f29_normalize(f29_add(lift(&ptab[i]), g)))));
}
// shuffle argument's grand product [RECALL halo2_proofs (PSE line) plonk/shuffle/prover.rs commit_product, restated in DESIGN.md 4.5]:
// num_i = A_i + gamma, den_i = S_i + gamma over the compressed input and shuffle-side rows, i < u, as the canonical Montgomery-2^261
// words the scans take.  No beta; the dense chain (mulscan, k_fr_inv_one, k_perm_ratio, k_perm_write_sets) follows unchanged.
__global__ void __launch_bounds__(256) k_shuffle_numden(const fe* input, const fe* shuffle, fe gamma, uint32_t u, fe* num, fe* den) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= u) return;
  const f29 g = f29_from_mont256<F9>(gamma.v), one = f29_const<F9>(F9::ONE);
  // a sum of two converted values may pass the 2p pack261 takes: one multiplication by the Montgomery one brings it back below 1.1 p
  fe_store(&num[i], pack261(f29_mul<F9>(f29_add(f29_from_mont256<F9>(fe_load(&input[i]).v), g), one)));
  fe_store(&den[i], pack261(f29_mul<F9>(f29_add(f29_from_mont256<F9>(fe_load(&shuffle[i]).v), g), one)));
}

// Sparse form of the lookup grand product (round 3).  ratio_i = (a_i + beta)(t_i + gamma) / ((a'_i + beta)(s'_i + gamma)) is
// exactly one wherever (a_i, t_i) = (a'_i, s'_i) — for a range check at DEGREE 22 on all but ~2^17 of 2^22 rows (input and
// permuted input are zero outside a handful of limbs, table and permuted table are zero outside 2^16 rows each) — so the
// product only moves at the other rows: they are flagged, compacted into a sorted position list (the scans of scan.cuh), the
// numerators / denominators / one inversion / prefix products run over that list, and k_perm_write_sets fills every row of z
// from the prefix product of the positions before it.  Same column bit for bit as the dense form (which multiplied 4 million
// ones: 3 multiplicative scans, 5.8 ms of the 74 ms range proof), chosen when at most a quarter of the rows are flagged.
__global__ void __launch_bounds__(256) k_lookup_flag(const fe* input, const fe* table, const fe* pin, const fe* ptab, uint32_t u, uint32_t padded,
                                                      uint32_t* flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= padded) return;
  uint32_t f = 0;
  if (i < u) f = (fe_eq(fe_load(&input[i]), fe_load(&pin[i])) && fe_eq(fe_load(&table[i]), fe_load(&ptab[i]))) ? 0u : 1u;
  flag[i] = f;
}
__global__ void __launch_bounds__(256) k_lookup_compact(const uint32_t* flag, const uint32_t* pos, uint32_t u, uint32_t* active) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < u && flag[i]) active[pos[i]] = i;
}
__global__ void __launch_bounds__(256) k_lookup_numden_sparse(const fe* input, const fe* table, const fe* pin, const fe* ptab, fe beta, fe gamma,
                                                               const uint32_t* active, uint32_t n_active, fe* num, fe* den) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_active) return;
  const uint32_t i = active[e];
  const f29 b = f29_from_mont256<F9>(beta.v), g = f29_from_mont256<F9>(gamma.v);
  auto lift = [](const fe* p) { return f29_from_mont256<F9>(fe_load(p).v); };
  fe_store(&num[e], pack261(f29_mul<F9>(f29_add(lift(&input[i]), b), f29_normalize(f29_add(lift(&table[i]), g)))));
  fe_store(&den[e], pack261(f29_mul<F9>(f29_add(lift(&pin[i]), b), f29_normalize(f29_add(lift(&ptab[i]), g)))));
}

// ---- quotient numerator of the range-check constraint system (BASELINE config 3) -------------------
// What the reference's RangeWithInstanceCircuitBuilder produces (src/scaffold.rs:434-485) [halo2-base shape restated
// from memory]: one vertical gate q (a + a(wX) a(w^2 X) - a(w^3 X)) on the advice column, a permutation argument over
// n_perm <= 4 equality-enabled columns in chunks of one to three (constraint-system degree 3 .. 5), one single-expression
// lookup in the fixed table of either a lookup-advice column or selector * advice (halo2-base with one advice column).  Terms in evaluate_h's order (gates, permutation, lookups), Horner in y,
// divided by X^n - 1; extended domain 4n.
struct RangeCosets {
  const fe* a;
  const fe* la;   // lookup input: a dedicated lookup-advice column ...
  const fe* ql;   // ... or, when non-null, the selector of the single-advice-column form: input = ql * a
  const fe* q;
  const fe* table;
  const fe* perm_value[4];
  const fe* perm_sigma[4];
  const fe* perm_z[4];
  const fe* lk_input;
  const fe* lk_table;
  const fe* lk_z;
  const fe* l0;
  const fe* l_last;
  const fe* l_active;
  uint32_t n_perm, chunk, has_lookup;
};
// Same arithmetic scheme as k_evaluate_h_standard_plonk (levels, host-scaled powers of y).  h.y[i] belongs to term i
// in evaluate_h's order: 0 the gate (expression at level 2: y[0] at level -3); 1 (1 - z_first) l_0 and the other l_0
// terms (level-0 expressions: -2); 2 the l_last term (level 1: -3); 3 .. the chain terms (l_0); then one term per
// permutation set (expression level = columns in the set: -2 - columns); then the lookup's five: l_0 (-2), l_last (-3),
// the product rule (level 2: -4), l_0 (-2), the ordering rule (level 1: -3).
__device__ __forceinline__ void evaluate_h_range_body(const RangeCosets& c, uint32_t ext_k, uint32_t k, uint32_t last_rot, const HConsts& h,
                                                      const fe* xlo, const fe* xhi, uint32_t xh, fe* out) {
  const uint32_t size = 1u << ext_k, rot = 1u << (ext_k - k);
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= size) return;
  auto at = [&](int r) { return (idx + size + (uint32_t)(r * (int)rot)) & (size - 1); };
  const uint32_t r_next = at(1), r_prev = at(-1), r_last = at(-(int)last_rot);
  const f29 one = hc(h.one0), gamma = hc(h.gamma0), beta = hc(h.beta0);
  // Sums of products at one level share a Montgomery reduction (round 3, as in k_evaluate_h_standard_plonk): Dot gathers the terms of a
  // group (NORMALIZED values, each with its power of y) and multiplies them two at a time (f29_mul2); its branches depend on the
  // constraint system only (uniform).  Differences of two products (left - right of a permutation set, of the lookup) are one f29_mul2 with the second
  // product's first factor negated (4p - x).
  struct Dot {  // pairs (value, index of its y constant), multiplied two at a time: one pending value is all the state (three at a
                // time held four operands across the permutation products: 269 registers, one wavefront per SIMD)
    f29 a0, sum;
    uint32_t i0;
    bool pending;
    const HConsts& h;
    __device__ __forceinline__ Dot(const HConsts& hh) : i0(0), pending(false), h(hh) { sum = f29_zero(); }
    __device__ __forceinline__ void add(const f29& a, uint32_t yi) {
      if (!pending) { a0 = a; i0 = yi; pending = true; }
      else { sum = f29_normalize(f29_add(sum, f29_mul2<F9>(a0, hc(h.y[i0]), a, hc(h.y[yi])))); pending = false; }
    }
    __device__ __forceinline__ f29 result() {  // normalized
      if (pending) sum = f29_normalize(f29_add(sum, f29_mul<F9>(a0, hc(h.y[i0]))));
      pending = false;
      return sum;
    }
  };
  auto neg4 = [](const f29& x_norm) { return f29_sub(f29_zero(), x_norm, F9::K4); };  // 4p - x for normalized x < 4p - 2^232: limbs < 2^30
  // gate: q (a + a(wX) a(w^2 X) - a(w^3 X))
  f29 acc;
  {
    f29 wu = f29_mul2<F9>(load_unpack(&c.a[at(1)]), load_unpack(&c.a[at(2)]), hsub(load_unpack(&c.a[idx]), load_unpack(&c.a[at(3)])), one);  // level 1
    acc = hmul(hmul(wu, load_unpack(&c.q[idx])), hc(h.y[0]));
  }
  const uint32_t sets = (c.n_perm + c.chunk - 1) / c.chunk;
  const f29 z_first = load_unpack(&c.perm_z[0][idx]);
  const f29 z_lastset = load_unpack(&c.perm_z[sets - 1][idx]);
  Dot s0(h), sa(h);                                                                    // l_0 group, l_active group (level -1 after the y factors)
  s0.add(hsub(one, z_first), 1);
  const f29 pl = hmul(z_lastset, hsub(z_lastset, one));                                // l_last group: z (z - 1), level 1
  for (uint32_t s = 1; s < sets; s++) s0.add(hsub(load_unpack(&c.perm_z[s][idx]), load_unpack(&c.perm_z[s - 1][r_last])), 2 + s);
  const f29 X = pow2tab(xlo, xhi, xh, idx);
  const uint32_t p0 = 2 + sets;
  for (uint32_t s = 0; s < sets; s++) {
    f29 left = load_unpack(&c.perm_z[s][r_next]), right = load_unpack(&c.perm_z[s][idx]);
    const uint32_t j0 = c.chunk * s, j1 = min(c.n_perm, c.chunk * (s + 1));
    for (uint32_t j = j0; j + 1 < j1; j++) {
      const f29 val = load_unpack(&c.perm_value[j][idx]);
      left = hmul(f29_add(f29_add(val, hmul(load_unpack(&c.perm_sigma[j][idx]), hc(h.beta_m1))), gamma), left);
      right = hmul(f29_add(f29_add(val, hmul(X, hc(h.cur[j]))), gamma), right);
    }
    {  // the set's last column: both products' final factors in one two-product multiplication, left - right
      const uint32_t j = j1 - 1;
      const f29 val = load_unpack(&c.perm_value[j][idx]);
      const f29 inner_l = f29_add(f29_add(val, hmul(load_unpack(&c.perm_sigma[j][idx]), hc(h.beta_m1))), gamma);  // lazy, limbs < 1.5 * 2^30
      const f29 inner_r = f29_normalize(f29_add(f29_add(val, hmul(X, hc(h.cur[j]))), gamma));
      sa.add(f29_mul2<F9>(inner_l, left, neg4(inner_r), right), p0 + s);
    }
  }
  f29 sl;
  if (c.has_lookup) {
    const uint32_t lb = p0 + sets;
    const f29 ap = load_unpack(&c.lk_input[idx]), sp = load_unpack(&c.lk_table[idx]), zl = load_unpack(&c.lk_z[idx]);
    s0.add(hsub(one, zl), lb);
    sl = f29_mul2<F9>(pl, hc(h.y[2]), hmul(zl, hsub(zl, one)), hc(h.y[lb + 1]));
    {  // z(wX) (A' + beta) (S' + gamma) - z (A + beta) (S + gamma)
      const f29 li = hmul(f29_add(ap, beta), load_unpack(&c.lk_z[r_next]));
      const f29 a_in = c.ql ? hmul(hmul(load_unpack(&c.ql[idx]), load_unpack(&c.a[idx])), hc(h.one_m2)) : load_unpack(&c.la[idx]);
      const f29 tv = hmul(f29_add(a_in, beta), f29_normalize(f29_add(load_unpack(&c.table[idx]), gamma)));
      sa.add(f29_mul2<F9>(f29_add(sp, gamma), li, neg4(tv), zl), lb + 2);
    }
    const f29 a_minus_s = hsub(ap, sp);
    s0.add(a_minus_s, lb + 3);
    sa.add(hmul(a_minus_s, hsub(ap, load_unpack(&c.lk_input[r_prev]))), lb + 4);
  } else {
    sl = hmul(pl, hc(h.y[2]));
  }
  acc = f29_add(acc, f29_mul3<F9>(s0.result(), load_unpack(&c.l0[idx]), sl, load_unpack(&c.l_last[idx]), sa.result(), load_unpack(&c.l_active[idx])));
  hstore(&out[idx], acc, h.tinv[idx & (rot - 1)]);
}
// register budget (round 3): unconstrained the body takes 169 VGPRs (two wavefronts per SIMD); held to 128
// (four wavefronts) it spills 40 dwords to scratch.  Measured inside the range proof at DEGREE 22 on one box, alternating:
// 74.8 / 75.1 ms unconstrained, 75.1 / 75.3 ms at 128 VGPRs — the kernel streams 2^24 rows at ~40 % of HBM and the spills cost
// what the occupancy buys.  So the kernel is left unconstrained.
__global__ void __launch_bounds__(256) k_evaluate_h_range(RangeCosets c, uint32_t ext_k, uint32_t k, uint32_t last_rot, HConsts h, const fe* xlo,
                                                           const fe* xhi, uint32_t xh, fe* out) {
  evaluate_h_range_body(c, ext_k, k, last_rot, h, xlo, xhi, xh, out);
}

// ---- quotient numerator, GENERAL form (round 4): what halo2-base configures when a circuit overflows one advice column --------
// `builder.config(k, Some(minimum_rows))` (src/scaffold.rs:268) then takes num_advice > 1 gate columns — each with its own
// vertical gate q_j (a_j + a_j(wX) a_j(w^2 X) - a_j(w^3 X)) — and, for the Range builder, num_lookup_advice lookup-advice
// columns with one lookup argument each [halo2-base shapes restated from memory].  The specialised kernels above track a stray
// 2^-5 per multiplication as "levels" so that operands can stay in the memory format; this one does not bother: every operand is
// brought to the multiplier's radix when it is loaded (one multiplication more per load), all arithmetic is in ONE domain, and h is
// Horner's rule in y over the terms in evaluate_h's order (gates, permutation, lookups) exactly as the oracle writes them
// (oracle/flex.py prove: _permutation_terms, _lookup_terms).  About half the speed of k_evaluate_h_range per point — a multi-column
// circuit is a small one by construction — and, being independent of the level bookkeeping, a cross-check of it: with one gate and
// the selector form of the lookup input both kernels must produce the same h (tests/test_gpu_flex.py).
struct FlexCosets {
  uint32_t n_gates, n_perm, chunk, n_lookups, n_shuffles;
  uint32_t logup;  // the lookups are logUp arguments: lk_pin holds M, lk_z the running sum, lk_ptab is not read
  // logUp: the input sets of lookup l, four bits each (1 .. H2MI_MAX_LOGUP_INPUTS): lk_in[l] points at that many CONSECUTIVE vectors
  uint32_t lk_sets;
  const fe* gate_a[H2MI_FLEX_MAX_GATES];
  const fe* gate_q[H2MI_FLEX_MAX_GATES];
  const fe* perm_value[H2MI_FLEX_MAX_PERM];
  const fe* perm_sigma[H2MI_FLEX_MAX_PERM];
  const fe* perm_z[H2MI_FLEX_MAX_PERM];
  const fe* lk_in[H2MI_FLEX_MAX_LOOKUPS];
  const fe* lk_in_b[H2MI_FLEX_MAX_LOOKUPS];  // optional second factor of the input expression (selector * advice)
  const fe* lk_table[H2MI_FLEX_MAX_LOOKUPS];
  const fe* lk_pin[H2MI_FLEX_MAX_LOOKUPS];
  const fe* lk_ptab[H2MI_FLEX_MAX_LOOKUPS];
  const fe* lk_z[H2MI_FLEX_MAX_LOOKUPS];
  const fe* sf_in[H2MI_MAX_SHUFFLES];   // shuffle arguments: the compressed input, the compressed shuffle side, the product
  const fe* sf_tab[H2MI_MAX_SHUFFLES];
  const fe* sf_z[H2MI_MAX_SHUFFLES];
  const fe* l0;
  const fe* l_last;
  const fe* l_active;
};
struct FlexConsts {
  fe beta, gamma, y, delta, zeta;  // Montgomery-2^256 words
  fe tinv[16];
};
// one domain (Montgomery-2^261), every value normalized and below ~8 p between operations
namespace gen {
__device__ __forceinline__ f29 ld(const fe* p) { return f29_from_mont256<F9>(fe_load(p).v); }
__device__ __forceinline__ f29 cst(const fe& v) { return f29_from_mont256<F9>(v.v); }
__device__ __forceinline__ f29 mul(const f29& a, const f29& b) { return f29_mul<F9>(a, b); }                              // b normalized (every value here is)
__device__ __forceinline__ f29 add(const f29& a, const f29& b) { return f29_normalize(f29_add(a, b)); }
__device__ __forceinline__ f29 sub(const f29& a, const f29& b) { return f29_normalize(f29_sub(a, b, F9::K4)); }           // b < 4p - 2^232
__device__ __forceinline__ f29 red(const f29& a) { return f29_mul<F9>(a, f29_const<F9>(F9::ONE)); }                       // back below 1.1 p (ONE = 2^261 mod p)
__device__ __forceinline__ void horner(f29& acc, const f29& y, const f29& term) { acc = add(mul(acc, y), term); }
}  // namespace gen
// What follows ONE circuit's gate terms in evaluate_h's order — the permutation argument (chunks of any length), then the lookups —
// folded into `acc` by Horner's rule in y: the body k_evaluate_h_flex, k_evaluate_h_expr and k_evaluate_h_expr_batch share.  `sh` holds
// what every circuit of a proof shares (the counts, the sigma cosets, l_0 / l_last / l_active), `c` what belongs to the circuit (the
// permuted columns' values, the grand products, the six vectors of each lookup): a single-circuit kernel passes its FlexCosets as both,
// the batch kernel its arguments and one CircuitCosets record in device memory.
template <class Circuit>
__device__ __forceinline__ void evaluate_h_fold(const Circuit& c, const FlexCosets& sh, uint32_t ext_k, uint32_t k, uint32_t last_rot, const FlexConsts& h,
                                                const fe* xlo, const fe* xhi, uint32_t xh, uint32_t idx, f29& acc, const f29& y) {
  using namespace gen;
  const uint32_t size = 1u << ext_k, rot = 1u << (ext_k - k);
  auto at = [&](int r) { return (idx + size + (uint32_t)(r * (int)rot)) & (size - 1); };
  const uint32_t r_next = at(1), r_prev = at(-1), r_last = at(-(int)last_rot);
  const f29 one = f29_const<F9>(F9::ONE), beta = cst(h.beta), gamma = cst(h.gamma), delta = cst(h.delta);
  const f29 l0 = ld(&sh.l0[idx]), ll = ld(&sh.l_last[idx]), lact = ld(&sh.l_active[idx]);
  if (sh.n_perm) {
    const uint32_t sets = (sh.n_perm + sh.chunk - 1) / sh.chunk;
    const f29 z_first = ld(&c.perm_z[0][idx]), z_lastset = ld(&c.perm_z[sets - 1][idx]);
    horner(acc, y, mul(sub(one, z_first), l0));
    horner(acc, y, mul(red(sub(mul(z_lastset, z_lastset), z_lastset)), ll));
    for (uint32_t s = 1; s < sets; s++) horner(acc, y, mul(sub(ld(&c.perm_z[s][idx]), ld(&c.perm_z[s - 1][r_last])), l0));
    f29 cur = mul(mul(pow2tab(xlo, xhi, xh, idx), cst(h.zeta)), beta);  // beta * X, X = zeta * extended_omega^idx
    for (uint32_t s = 0; s < sets; s++) {
      f29 left = ld(&c.perm_z[s][r_next]), right = ld(&c.perm_z[s][idx]);
      const uint32_t j0 = sh.chunk * s, j1 = min(sh.n_perm, sh.chunk * (s + 1));
      for (uint32_t j = j0; j < j1; j++) {
        const f29 val = ld(&c.perm_value[j][idx]);
        left = mul(left, add(add(val, mul(beta, ld(&sh.perm_sigma[j][idx]))), gamma));
        right = mul(right, add(add(val, cur), gamma));
        cur = mul(cur, delta);
      }
      horner(acc, y, mul(sub(left, right), lact));
    }
  }
  for (uint32_t l = 0; l < sh.n_lookups; l++) {
    f29 a_in = ld(&c.lk_in[l][idx]);
    if (c.lk_in_b[l]) a_in = mul(a_in, ld(&c.lk_in_b[l][idx]));
    if (sh.logup) {
      // logUp [Haboeck; the mv-lookup feature of halo2_proofs forks, restated from memory in DESIGN.md 4.5]: three terms, no gamma.  The
      // mode is the launch's (wave-uniform); M and phi arrive through the slots of the permuted input and of the product
      // With K input sets over the one table the fraction of a row is N / D, built by the recurrence (N, D) = (-M, s), then per input
      // N <- N a_j + D, D <- D a_j (a_j = A_j + beta, s = S + beta): two products per input, no array.  K is launch data (wave-uniform)
      // and set j of the lookup is the vector j * 2^ext_k behind lk_in[l].  Bounds in units of p (a load 1.04, a product 1 + 0.006 a b):
      // a_j, s <= 2.08; N starts at 4 (a negation) and is a product plus D afterwards, <= 1.05 + 2.08; D <= 2.08, then a product
      const f29 phi = ld(&c.lk_z[l][idx]);
      horner(acc, y, mul(phi, l0));
      horner(acc, y, mul(phi, ll));
      f29 den = add(ld(&c.lk_table[l][idx]), beta), num = sub(f29_zero(), ld(&c.lk_pin[l][idx]));
      const uint32_t sets = (sh.lk_sets >> (4 * l)) & 15u;
      for (uint32_t j = 0;;) {
        const f29 ab = add(a_in, beta);
        num = add(mul(num, ab), den);
        den = mul(den, ab);
        if (++j >= sets) break;
        a_in = ld(&c.lk_in[l][(size_t)j * size + idx]);
      }
      horner(acc, y, mul(sub(mul(sub(ld(&c.lk_z[l][r_next]), phi), den), num), lact));
      continue;
    }
    const f29 t_in = ld(&c.lk_table[l][idx]), ap = ld(&c.lk_pin[l][idx]), ap_prev = ld(&c.lk_pin[l][r_prev]), sp = ld(&c.lk_ptab[l][idx]);
    const f29 lz = ld(&c.lk_z[l][idx]), lz_next = ld(&c.lk_z[l][r_next]);
    horner(acc, y, mul(sub(one, lz), l0));
    horner(acc, y, mul(red(sub(mul(lz, lz), lz)), ll));
    const f29 lhs = mul(mul(lz_next, add(ap, beta)), add(sp, gamma)), rhs = mul(mul(lz, add(a_in, beta)), add(t_in, gamma));
    horner(acc, y, mul(sub(lhs, rhs), lact));
    const f29 d = sub(ap, sp);
    horner(acc, y, mul(d, l0));
    horner(acc, y, mul(red(mul(d, sub(ap, ap_prev))), lact));
  }
  // the shuffle arguments [RECALL halo2_proofs (PSE line) plonk/evaluation.rs, restated in DESIGN.md 4.5]: behind the lookups, three
  // terms each; the count is the launch's and the pointers come from the argument struct or the circuit's record (wave-uniform)
  for (uint32_t s = 0; s < sh.n_shuffles; s++) {
    const f29 a_in = ld(&c.sf_in[s][idx]), s_in = ld(&c.sf_tab[s][idx]);
    const f29 sz = ld(&c.sf_z[s][idx]), sz_next = ld(&c.sf_z[s][r_next]);
    horner(acc, y, mul(sub(one, sz), l0));
    horner(acc, y, mul(red(sub(mul(sz, sz), sz)), ll));
    horner(acc, y, mul(sub(mul(sz_next, add(s_in, gamma)), mul(sz, add(a_in, gamma))), lact));
  }
}
// the division by X^n - 1 behind the LAST circuit's terms, and the one store
__device__ __forceinline__ void evaluate_h_finish(const f29& acc, uint32_t ext_k, uint32_t k, const FlexConsts& h, uint32_t idx, fe* out) {
  using namespace gen;
  const uint32_t rot = 1u << (ext_k - k);
  fe o;
  f29_to_mont256<F9>(mul(acc, cst(h.tinv[idx & (rot - 1)])), o.v);
  fe_store(&out[idx], o);
}
// one circuit: its terms, then the finish
__device__ __forceinline__ void evaluate_h_tail(const FlexCosets& c, uint32_t ext_k, uint32_t k, uint32_t last_rot, const FlexConsts& h, const fe* xlo,
                                                const fe* xhi, uint32_t xh, uint32_t idx, f29 acc, const f29& y, fe* out) {
  evaluate_h_fold(c, c, ext_k, k, last_rot, h, xlo, xhi, xh, idx, acc, y);
  evaluate_h_finish(acc, ext_k, k, h, idx, out);
}
__global__ void __launch_bounds__(256) k_evaluate_h_flex(FlexCosets c, uint32_t ext_k, uint32_t k, uint32_t last_rot, FlexConsts h, const fe* xlo,
                                                          const fe* xhi, uint32_t xh, fe* out) {
  using namespace gen;
  const uint32_t size = 1u << ext_k, rot = 1u << (ext_k - k);
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= size) return;
  auto at = [&](int r) { return (idx + size + (uint32_t)(r * (int)rot)) & (size - 1); };
  const f29 y = cst(h.y);
  f29 acc = f29_zero();
  for (uint32_t g = 0; g < c.n_gates; g++) {
    const fe* a = c.gate_a[g];
    horner(acc, y, mul(sub(add(ld(&a[idx]), mul(ld(&a[at(1)]), ld(&a[at(2)]))), ld(&a[at(3)])), ld(&c.gate_q[g][idx])));
  }
  evaluate_h_tail(c, ext_k, k, last_rot, h, xlo, xhi, xh, idx, acc, y, out);
}

// ---- quotient numerator with the gates as DATA: a postfix program over column queries (h2mi_gate_program, include/h2mi.h) -------------
// The arithmetic is k_evaluate_h_flex's (one domain, operands converted on load, every value normalized between operations, Horner in y
// over the polynomials in program order, then the shared tail).  New is the interpreter:
//   * the program is wave-uniform: the loop counter does not depend on the lane and the ops / column pointers are read through
//     __restrict__ const pointers at uniform addresses (scalar loads), so dispatch is a uniform branch and a query's base pointer and
//     row offset are scalars;
//   * the operand stack keeps its top in registers and the rest in LDS as [level][limb][thread] (a wavefront's 64 lanes read 64
//     consecutive words: no bank conflict), max_stack - 1 levels of 9 KB, sized per launch — never a runtime-indexed private array;
//   * the column-pointer table, the constants (already Montgomery-2^261 words) and the ops live in ONE device buffer: the launch carries
//     three addresses into it, not 136 pointers (64 advice, 64 fixed, H2MI_MAX_INSTANCE instance columns);
//   * a challenge (H2MI_EXPR_CHALLENGE: a value the transcript yields between two advice phases) is a constant of the LAUNCH rather than
//     of the program: the uploader lays the challenge values out behind the program's constants, in the same words, and encodes the
//     operand as EX_CONST with index n_constants + challenge — the same wave-uniform load, no dispatch case of its own, and the device
//     code of a program without challenges is what it was.
// Ops as uploaded: word x = code | index << 8, word y = the row offset of the rotation, (r mod n) 2^(ext_k - k).  The uploader inserts
// EX_RED where its static bound on a value would otherwise pass what the next operation takes (see expr_encode).
enum : uint32_t { EX_COL = 0, EX_CONST, EX_ADD, EX_SUB, EX_MUL, EX_NEG, EX_RED, EX_END };
constexpr uint32_t EX_INSTANCE = H2MI_EXPR_MAX_ADVICE + H2MI_EXPR_MAX_FIXED;   // instance column i sits in slot EX_INSTANCE + i
constexpr uint32_t EX_COLS = EX_INSTANCE + H2MI_MAX_INSTANCE;                 // advice, fixed, the instance columns
// The interpreter loop, shared by the quotient kernel and the lookup compression: `sink(value)` receives each polynomial at its END.
template <class Sink>
__device__ __forceinline__ void expr_interpret(const fe* const* __restrict__ cols, const fe* __restrict__ consts, const uint2* __restrict__ ops,
                                               uint32_t n_ops, uint32_t idx, uint32_t size, uint32_t* ex_stack, Sink&& sink) {
  using namespace gen;
  uint32_t* const slot = ex_stack + threadIdx.x;
  auto spill = [&](const f29& v, uint32_t level) {
#pragma unroll
    for (int i = 0; i < 9; i++) slot[(level * 9 + i) * 256] = v.v[i];
  };
  auto fill = [&](uint32_t level) {
    f29 v;
#pragma unroll
    for (int i = 0; i < 9; i++) v.v[i] = slot[(level * 9 + i) * 256];
    return v;
  };
  f29 tos = f29_zero();
  uint32_t sp = 0;  // values on the stack: tos and LDS levels 0 .. sp - 2
  for (uint32_t pc = 0; pc < n_ops; pc++) {
    const uint2 op = ops[pc];
    const uint32_t code = op.x & 0xffu, index = op.x >> 8;
    if (code <= EX_CONST) {
      if (sp) spill(tos, sp - 1);
      sp++;
      if (code == EX_COL) tos = ld(&cols[index][(idx + op.y) & (size - 1)]);
      else tos = load_unpack(&consts[index]);
    } else if (code <= EX_MUL) {
      const f29 a = fill(sp - 2);
      sp--;
      if (code == EX_MUL) tos = mul(a, tos);
      else if (code == EX_ADD) tos = add(a, tos);
      else tos = sub(a, tos);
    } else if (code == EX_NEG) {
      tos = sub(f29_zero(), tos);
    } else if (code == EX_RED) {
      tos = red(tos);
    } else {  // EX_END: the one value left is this polynomial
      sink(tos);
      sp = 0;
    }
  }
}
__global__ void __launch_bounds__(256) k_evaluate_h_expr(FlexCosets c, const fe* const* __restrict__ cols, const fe* __restrict__ consts,
                                                          const uint2* __restrict__ ops, uint32_t n_ops, uint32_t ext_k, uint32_t k, uint32_t last_rot,
                                                          FlexConsts h, const fe* xlo, const fe* xhi, uint32_t xh, fe* out) {
  using namespace gen;
  extern __shared__ uint32_t ex_stack[];  // [level][limb][thread]
  const uint32_t size = 1u << ext_k;
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= size) return;  // no barrier below: a thread touches its own stack slots only
  const f29 y = cst(h.y);
  f29 acc = f29_zero();
  expr_interpret(cols, consts, ops, n_ops, idx, size, ex_stack, [&](const f29& poly) { horner(acc, y, poly); });
  evaluate_h_tail(c, ext_k, k, last_rot, h, xlo, xhi, xh, idx, acc, y, out);
}
// Several circuits in one proof [RECALL halo2_proofs v2023_02_02 plonk/evaluation.rs evaluate_h: ONE `values` vector walks the circuits
// in order, per circuit values = values y + term over its gates, its permutation terms, its lookup terms; the division by X^n - 1
// comes behind the last circuit].  The accumulator stays in registers across the circuits: one t_inv multiplication and one store per
// point, where a chain of single launches with a carry-in would read and write h once per circuit.  Program, constants and challenges
// are the proof's; what differs per circuit is pointers, and those sit in device memory as consecutive records behind the program (a
// table indexed by a loaded value does not belong in the launch's arguments, see k_copy_check).  The circuit counter does not depend
// on the lane: a record's pointers arrive by scalar loads at uniform addresses, as the ops do.
struct CircuitCosets {
  const fe* cols[EX_COLS];  // the interpreter's table: advice, fixed, the instance columns
  const fe* perm_value[H2MI_FLEX_MAX_PERM];
  const fe* perm_z[H2MI_FLEX_MAX_PERM];
  const fe* lk_in[H2MI_FLEX_MAX_LOOKUPS];
  const fe* lk_in_b[H2MI_FLEX_MAX_LOOKUPS];
  const fe* lk_table[H2MI_FLEX_MAX_LOOKUPS];
  const fe* lk_pin[H2MI_FLEX_MAX_LOOKUPS];
  const fe* lk_ptab[H2MI_FLEX_MAX_LOOKUPS];
  const fe* lk_z[H2MI_FLEX_MAX_LOOKUPS];
  const fe* sf_in[H2MI_MAX_SHUFFLES];
  const fe* sf_tab[H2MI_MAX_SHUFFLES];
  const fe* sf_z[H2MI_MAX_SHUFFLES];
};
__global__ void __launch_bounds__(256) k_evaluate_h_expr_batch(FlexCosets sh, const CircuitCosets* __restrict__ circuits, uint32_t n_circuits,
                                                                const fe* __restrict__ consts, const uint2* __restrict__ ops, uint32_t n_ops,
                                                                uint32_t ext_k, uint32_t k, uint32_t last_rot, FlexConsts h, const fe* xlo,
                                                                const fe* xhi, uint32_t xh, fe* out) {
  using namespace gen;
  extern __shared__ uint32_t ex_stack[];  // [level][limb][thread]
  const uint32_t size = 1u << ext_k;
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= size) return;  // no barrier below
  const f29 y = cst(h.y);
  f29 acc = f29_zero();
  for (uint32_t i = 0; i < n_circuits; i++) {
    const CircuitCosets& c = circuits[i];
    expr_interpret(c.cols, consts, ops, n_ops, idx, size, ex_stack, [&](const f29& poly) { horner(acc, y, poly); });
    evaluate_h_fold(c, sh, ext_k, k, last_rot, h, xlo, xhi, xh, idx, acc, y);
  }
  evaluate_h_finish(acc, ext_k, k, h, idx, out);
}
// The same numerator one coset of 2^k points at a time (H2MI_KEYGEN_BY_COSET): extended-coset point c + rot i is X = (zeta w_ext^c) w^i
// with w = w_ext^rot the domain's generator, so on slice c every vector is the 2^k-point coset transform of its coefficients with shift
// zeta w_ext^c, a query at rotation r is element (i + r) mod 2^k of the same slice, and the body is the resident one on a domain with
// ext_k = k: the ops carry r mod n, the power table is w's, h.zeta holds the slice's shift and a logUp lookup's input sets lie 2^k
// apart.  What knows the extended domain is the finish alone: t_inv[c] and the store at h[c + rot i].
// (Two waves per SIMD stated: left to itself the allocator takes 255 VGPRs and 2 AGPRs, one register past the two-wave budget the resident
// kernel keeps; held to it, 199 VGPRs and no scratch.)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) k_evaluate_h_expr_slice(FlexCosets sh, const CircuitCosets* __restrict__ circuits, uint32_t n_circuits,
                                                                const fe* __restrict__ consts, const uint2* __restrict__ ops, uint32_t n_ops,
                                                                uint32_t ext_k, uint32_t k, uint32_t slice, uint32_t last_rot, FlexConsts h,
                                                                const fe* xlo, const fe* xhi, uint32_t xh, fe* out) {
  using namespace gen;
  extern __shared__ uint32_t ex_stack[];  // [level][limb][thread]
  const uint32_t n = 1u << k;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;  // no barrier below
  const f29 y = cst(h.y);
  f29 acc = f29_zero();
  for (uint32_t m = 0; m < n_circuits; m++) {
    const CircuitCosets& c = circuits[m];
    expr_interpret(c.cols, consts, ops, n_ops, i, n, ex_stack, [&](const f29& poly) { horner(acc, y, poly); });
    evaluate_h_fold(c, sh, k, k, last_rot, h, xlo, xhi, xh, i, acc, y);
  }
  evaluate_h_finish(acc, ext_k, k, h, slice + (i << (ext_k - k)), out);
}
// The lookup argument's theta compression (plonk/lookup/prover.rs commit_permuted `compress_expressions`, plonk/evaluation.rs for
// the extended coset [RECALL]): out[i] = sum_j e_j(i) theta^(m-1-j), the fold acc theta + e_j over the program's m polynomials, on
// the 2^dom_k points of the Lagrange rows (dom_k = k) or of the extended coset.  The same interpreter; the sink at END is Horner's
// rule in theta instead of y, and the value is stored in the memory format (fully reduced Montgomery-2^256).
__global__ void __launch_bounds__(256) k_expr_compress(const fe* const* __restrict__ cols, const fe* __restrict__ consts, const uint2* __restrict__ ops,
                                                        uint32_t n_ops, uint32_t dom_k, fe theta, fe* out) {
  using namespace gen;
  extern __shared__ uint32_t ex_stack[];
  const uint32_t size = 1u << dom_k;
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= size) return;
  const f29 th = cst(theta);
  f29 acc = f29_zero();
  expr_interpret(cols, consts, ops, n_ops, idx, size, ex_stack, [&](const f29& poly) { horner(acc, th, poly); });
  fe o;
  f29_to_mont256<F9>(acc, o.v);
  fe_store(&out[idx], o);
}
// The witness check: the same program on the Lagrange rows, each polynomial tested for zero on each row instead of folded.  The sink
// counts the ENDs it has seen (j), brings the value below p (EX_RED's multiplication by the Montgomery one, then the conditional
// subtraction: a value that is an unreduced multiple of r becomes the zero word — no word of an unreduced value is compared) and
// votes: `report[j] = {rows where polynomial j is not zero, the smallest of them}`, the caller having set {0, 0xffffffff}.  The
// program is wave-uniform, so every lane of a wavefront reaches every END together; a lane past n_rows (or past 2^k, in a launch
// smaller than a wavefront: its loads wrap into the columns like any rotation) runs along and votes false.  One atomicAdd and one
// atomicMin per wavefront and polynomial with a failing row, issued by the lowest failing lane (lane order is row order, so its row
// is the wavefront's smallest); none for a satisfied witness.
__global__ void __launch_bounds__(256) k_expr_check(const fe* const* __restrict__ cols, const fe* __restrict__ consts, const uint2* __restrict__ ops,
                                                     uint32_t n_ops, uint32_t k, uint32_t n_rows, uint32_t* __restrict__ report) {
  using namespace gen;
  extern __shared__ uint32_t ex_stack[];
  const uint32_t size = 1u << k;
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = idx < n_rows;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t j = 0;
  expr_interpret(cols, consts, ops, n_ops, idx, size, ex_stack, [&](const f29& poly) {
    const f29 c = f29_reduce_canonical<F9>(red(poly));
    uint32_t z = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) z |= c.v[i];
    const unsigned long long m = __ballot(live && z != 0);
    if (m && lane == (uint32_t)(__ffsll(m) - 1)) {
      atomicAdd(&report[2 * j], (uint32_t)__popcll(m));
      atomicMin(&report[2 * j + 1], idx);
    }
    j++;
  });
}
// Copy constraints on the rows: one thread per moved cell of the permutation (a cell whose sigma is not the identity), as keygen
// lists them: {column, row} of the cell and of its image, columns numbered in the permutation argument's order.  Equal cycles have
// every cell equal to its image (compared as canonical integers).  report = {unequal cells, the smallest index of one in `cells`},
// from {0, 0xffffffff}: keygen sorts the list by (column, row), so the smallest index is the smallest cell in permutation order and
// the lowest failing lane holds its wavefront's.  The same wavefront-first reduction.  The column pointers are read from device
// memory (a table indexed by a loaded value: in the launch's arguments it would be a runtime-indexed private array).
__global__ void __launch_bounds__(256) k_copy_check(const fe* const* __restrict__ cols, const uint4* __restrict__ cells, uint32_t n_cells,
                                                     uint32_t* __restrict__ report) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (i < n_cells) {
    const uint4 m = cells[i];
    const fe a = fe_from_mont<Fr>(fe_load(&cols[m.x][m.y])), b = fe_from_mont<Fr>(fe_load(&cols[m.z][m.w]));
    uint32_t d = 0;
#pragma unroll
    for (int w = 0; w < 8; w++) d |= a.v[w] ^ b.v[w];
    bad = d != 0;
  }
  const unsigned long long m = __ballot(bad);
  if (m && (threadIdx.x & 63u) == (uint32_t)(__ffsll(m) - 1)) {
    atomicAdd(&report[0], (uint32_t)__popcll(m));
    atomicMin(&report[1], i);
  }
}

// the one inversion on the critical path, by division steps on the 32-bit-limb layer (fe_inv_ds; round 4: the shift / subtract
// Euclid it replaces took 110 us for a lone wavefront).  in = x 2^261 read
// as a Montgomery-2^256 value is (32 x) 2^256; its inverse (x^-1 / 32) 2^256 times 2^10 is x^-1 2^261.
__global__ void k_fr_inv_one(const fe* in, fe* out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  fe r = fe_inv_ds<Fr>(fe_load(in));
  for (int i = 0; i < 10; i++) r = fe_dbl<Fr>(r);
  fe_store(out, r);
}
// A handful of constrained cells (the reference's StandardPlonk: 8 positions, x^2 + 72: ~30): the whole sparse grand
// product in ONE workgroup.  R_i = prod_{j<=i} num_j / den_j = PN_i * S_(i+1) / S_0 with PN the prefix products of the
// numerators and S the suffix products of the denominators: the two scans run together (Hillis-Steele), and the ONE
// inversion (division steps, see k_fr_inv_one) is of S_0 — every lane of the first wavefront runs it on the same value, so
// its data-dependent branches are wavefront-uniform.  (Round 2 inverted each lane's own denominator: 64 different branch
// histories in one wavefront, 0.22 ms for 8 cells.)  The result is already in the columns' Montgomery-2^256 form for
// k_perm_write_sets.
constexpr uint32_t PERM_SMALL_MAX = 256;
__global__ void __launch_bounds__(PERM_SMALL_MAX) k_perm_sparse_small(PermArgs a, uint32_t chunk, uint32_t n_active, uint32_t u, const fe* wlo,
                                                                      const fe* whi, uint32_t wh, const uint32_t* active, fe* R) {
  __shared__ fe shn[PERM_SMALL_MAX], shd[PERM_SMALL_MAX + 1], sh_inv;
  const uint32_t tid = threadIdx.x;
  f29 pn = f29_const<F9>(F9::ONE), pd = pn;
  if (tid < n_active) {
    const uint32_t t = active[tid];
    const uint32_t set = t / u, i = t - set * u;
    const f29 w = pow2tab(wlo, whi, wh, i);
    for (uint32_t j = set * chunk; j < a.m && j < (set + 1) * chunk; j++) {
      f29 nf, df;
      perm_factors(a, j, i, w, nf, df);
      pn = f29_mul<F9>(nf, pn);
      pd = f29_mul<F9>(df, pd);
    }
  }
  shn[tid] = pack261(pn);
  shd[tid] = pack261(pd);
  if (tid == 0) shd[PERM_SMALL_MAX] = one261();
  __syncthreads();
  for (uint32_t d = 1; d < n_active; d <<= 1) {  // shn: inclusive prefix products; shd: inclusive suffix products
    fe vn = one261(), vd = one261();
    if (tid >= d) vn = shn[tid - d];
    if (tid + d < PERM_SMALL_MAX) vd = shd[tid + d];
    __syncthreads();
    if (tid >= d) shn[tid] = pack261(f29_mul<F9>(f29_unpack(shn[tid].v), f29_unpack(vn.v)));
    if (tid + d < PERM_SMALL_MAX) shd[tid] = pack261(f29_mul<F9>(f29_unpack(shd[tid].v), f29_unpack(vd.v)));
    __syncthreads();
  }
  if (tid < 64) {  // (S_0 2^261) read as Montgomery-2^256 is (32 S_0) 2^256; its inverse times 2^10 is S_0^-1 2^261
    fe inv = fe_inv_ds<Fr>(shd[0]);
    for (int q = 0; q < 10; q++) inv = fe_dbl<Fr>(inv);
    if (tid == 0) sh_inv = inv;
  }
  __syncthreads();
  if (tid < n_active) {
    f29 r = f29_mul<F9>(f29_unpack(shn[tid].v), f29_unpack(sh_inv.v));
    r = f29_mul<F9>(r, f29_unpack(shd[tid + 1].v));
    fe o;
    f29_to_mont256<F9>(r, o.v);
    fe_store(&R[tid], o);
  }
}
// ratio_i = num_i / den_i = num_i * P_(i-1) * S_(i+1) / P_(n-1)   (P, S: prefix / suffix products of den)
__global__ void __launch_bounds__(256) k_perm_ratio(const fe* num, const fe* P, const fe* S, const fe* inv_total, size_t n, fe* ratio) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  f29 r = f29_mul<F9>(ld261(&num[i]), ld261(inv_total));
  if (i) r = f29_mul<F9>(r, ld261(&P[i - 1]));
  if (i + 1 < n) r = f29_mul<F9>(r, ld261(&S[i + 1]));
  fe_store(&ratio[i], pack261(r));
}
// z[0] = start, z[i+1] = start * R_i for i < u (R: inclusive prefix products of the ratios); rows beyond u untouched
__global__ void __launch_bounds__(256) k_perm_write(const fe* R, const fe* start_or_null, uint32_t u, fe* z, fe* last_or_null) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > u) return;
  const fe st = start_or_null ? fe_load(start_or_null) : fe_one<Fr>();
  fe v = st;
  if (i) {  // mixed-domain product: (start 2^256) (R 2^261) / 2^261 = start R 2^256
    f29_pack(f29_reduce_canonical<F9>(f29_mul<F9>(f29_unpack(st.v), ld261(&R[i - 1]))), v.v);
  }
  fe_store(&z[i], v);
  if (i == u && last_or_null) fe_store(last_or_null, v);
}

// ---- logUp: the running sum phi [Haboeck; restated from memory in DESIGN.md 4.5] ------------------------------------------------------
// Per usable row ONE fraction, 1 / (A + beta) - M / (S + beta) = ((S + beta) - M (A + beta)) / ((A + beta)(S + beta)): numerator and
// denominator as the canonical Montgomery-2^261 words the scans take, so that the dense chain (k_mulscan_* over the denominators, the
// one inversion, k_perm_ratio) turns them into the fractions' values; then an ADDITIVE prefix scan.
__global__ void __launch_bounds__(256) k_logup_numden(const fe* input, const fe* table, const fe* mult, fe beta, uint32_t u, fe* num, fe* den) {
  using namespace gen;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= u) return;
  const f29 b = cst(beta), ab = add(ld(&input[i]), b), sb = add(ld(&table[i]), b);
  fe_store(&num[i], pack261(red(sub(sb, mul(ld(&mult[i]), ab)))));
  fe_store(&den[i], pack261(mul(ab, sb)));
}
// With n_sets >= 2 input vectors (`stride` elements apart) over the one table the row's fraction is sum_j 1 / a_j - M / s = N / D, a_j =
// A_j + beta, s = S + beta, by the recurrence (N, D) = (-M, s), then per input N <- N a_j + D, D <- D a_j: D = s prod a_j and N = s sum_j
// prod_{m != j} a_m - M prod a_j, two products per input, no per-thread array; one input would give the kernel above's pair.  A kernel of
// its own: the loop-carried pair and beta cost 15 VGPRs, and the one-set kernel keeps its 8 waves per SIMD.  gen::'s bounds in units of
// p, whatever n_sets (6 at most): a load <= 1.04, so a_j, s <= 2.08; N starts as a negation (4, which a product takes), then is a product
// plus D: <= (1 + 0.006 * 4 * 2.08) + 2.08 < 3.2 in the first round and <= (1 + 0.006 * 3.2 * 2.08) + 1.03 < 2.1 afterwards; D <= 2.08,
// then a product <= 1 + 0.006 * 2.08^2 < 1.03.  N is reduced once before it is packed; D leaves the loop as a product
__global__ void __launch_bounds__(256) k_logup_numden_sets(const fe* inputs, uint32_t n_sets, size_t stride, const fe* table, const fe* mult, fe beta,
                                                           uint32_t u, fe* num, fe* den) {
  using namespace gen;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= u) return;
  const f29 b = cst(beta);
  f29 d = add(ld(&table[i]), b), n = sub(f29_zero(), ld(&mult[i]));
  for (uint32_t j = 0; j < n_sets; j++) {
    const f29 ab = add(ld(&inputs[(size_t)j * stride + i]), b);
    n = add(mul(n, ab), d);
    d = mul(d, ab);
  }
  fe_store(&num[i], pack261(red(n)));
  fe_store(&den[i], pack261(d));
}
// The additive scan over Fr, shaped like the multiplicative one (local / offsets / apply, tiles of AS_TILE) without a multiplication:
// the words are canonical (below r), so a sum is one 256-bit addition and one conditional subtraction on the 32-bit-limb layer, and
// the Montgomery factor 2^261 rides along unchanged.
constexpr uint32_t AS_TILE = 1024;
__global__ void __launch_bounds__(256) k_addscan_local(const fe* in, uint32_t n, fe* local, fe* totals) {
  __shared__ fe tsum[256];
  const uint32_t tid = threadIdx.x, base = blockIdx.x * AS_TILE + 4 * tid;
  fe v[4];
#pragma unroll
  for (int r = 0; r < 4; r++) v[r] = base + r < n ? fe_load(&in[base + r]) : fe_zero();
#pragma unroll
  for (int r = 1; r < 4; r++) v[r] = fe_add<Fr>(v[r - 1], v[r]);
  tsum[tid] = v[3];
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {  // inclusive scan of the 256 thread sums (Hillis-Steele)
    fe w = fe_zero();
    if (tid >= d) w = tsum[tid - d];
    __syncthreads();
    if (tid >= d) tsum[tid] = fe_add<Fr>(tsum[tid], w);
    __syncthreads();
  }
  const fe left = tid ? tsum[tid - 1] : fe_zero();
#pragma unroll
  for (int r = 0; r < 4; r++)
    if (base + r < n) fe_store(&local[base + r], fe_add<Fr>(left, v[r]));
  if (tid == 255) fe_store(&totals[blockIdx.x], tsum[255]);
}
// exclusive scan of the tile totals in ONE workgroup: every thread owns a run of consecutive totals (k_mulscan_offsets' layout)
__global__ void __launch_bounds__(1024) k_addscan_offsets(const fe* totals, uint32_t nblocks, fe* offsets) {
  __shared__ fe tsum[1024];
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (nblocks + 1023) / 1024;
  const uint32_t lo = min(tid * per, nblocks), hi = min(lo + per, nblocks);
  fe run = fe_zero();
  for (uint32_t b = lo; b < hi; b++) run = fe_add<Fr>(run, fe_load(&totals[b]));
  tsum[tid] = run;
  __syncthreads();
  const uint32_t used = (nblocks + per - 1) / per;
  for (uint32_t d = 1; d < used; d <<= 1) {
    fe w = fe_zero();
    if (tid >= d) w = tsum[tid - d];
    __syncthreads();
    if (tid >= d) tsum[tid] = fe_add<Fr>(tsum[tid], w);
    __syncthreads();
  }
  fe acc = tid ? tsum[tid - 1] : fe_zero();
  for (uint32_t b = lo; b < hi; b++) {
    fe_store(&offsets[b], acc);
    acc = fe_add<Fr>(acc, fe_load(&totals[b]));
  }
}
// apply, as the plain exclusive scan the column is: phi[0] = 0, phi[i] = local[i - 1] + offsets[tile of i - 1] for 1 <= i <= u, brought
// to the columns' Montgomery-2^256 form; rows beyond u untouched.  offsets == NULL: one tile.  FROM261 = false: the terms were summed
// in the columns' own form (the ranked sum below), and the word is stored as it is
template <bool FROM261>
__global__ void __launch_bounds__(256) k_addscan_apply(const fe* local, const fe* offsets, uint32_t u, fe* phi) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > u) return;
  fe o = fe_zero();
  if (i) {
    fe v = fe_load(&local[i - 1]);
    if (offsets && i - 1 >= AS_TILE) v = fe_add<Fr>(v, fe_load(&offsets[(i - 1) / AS_TILE]));
    if (FROM261) f29_to_mont256<F9>(f29_unpack(v.v), o.v);
    else o = v;
  }
  fe_store(&phi[i], o);
}
// ---- logUp against a table sorted at keygen: the running sum by rank (h2mi_plonk_logup_sum_ranked_dev) -------------------------------
// Every input IS a table value, so 1 / (A + beta) takes at most n_unique values: T[r] = 1 / (sorted[r] + beta) is inverted once (the
// tile chain of the assigned cells, ONE field inversion) and a row's term is a GATHER, sum_j T[rank_j[i]]: additions only, whatever the
// number of rows.  The table side, counts[r] T[r], is subtracted on row first[r] (n_unique products; the rows are distinct).  All words
// are reduced Montgomery-2^256 ones, so the additive scan runs on them as they are.
__global__ void __launch_bounds__(256) k_logup_table_den(const fe* sorted_mont, fe beta, uint32_t n_unique, fe* den) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n_unique) fe_store(&den[r], fe_add<Fr>(fe_load(&sorted_mont[r]), beta));
}
// a rank that is no table index (an input h2mi_plonk_logup_rank_cols_dev counted as absent) adds nothing and reads nothing
__global__ void __launch_bounds__(256) k_logup_gather(const uint32_t* ranks, uint32_t n_inputs, size_t stride, const fe* T, uint32_t n_unique, uint32_t u,
                                                      fe* term) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= u) return;
  fe acc = fe_zero();
  for (uint32_t j = 0; j < n_inputs; j++) {
    const uint32_t r = ranks[(size_t)j * stride + i];
    if (r < n_unique) acc = fe_add<Fr>(acc, fe_load(&T[r]));
  }
  fe_store(&term[i], acc);
}
__global__ void __launch_bounds__(256) k_logup_table_side(const uint32_t* counts, const uint32_t* first, const fe* T, uint32_t n_unique, uint32_t u,
                                                          fe* term) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_unique || !counts[r]) return;
  const uint32_t row = first[r];
  if (row >= u) return;  // always false for the first rows of a table's usable part
  fe c = fe_zero();
  c.v[0] = counts[r];
  fe_store(&term[row], fe_sub<Fr>(fe_load(&term[row]), fe_mul<Fr>(fe_to_mont<Fr>(c), fe_load(&T[r]))));
}

struct HostY {  // y^0 .. y^(count-1), Montgomery-2^256
  fe p[24];
  HostY(const fe& y, uint32_t count) {
    memcpy(p[0].v, h_canon(f29_const<F9>(F9::TO256)).v, 32);
    for (uint32_t i = 1; i < count && i < 24; i++) p[i] = h_mul256(p[i - 1], y);
  }
};
// what every quotient call asks of its scalars: no NULL (H2MI_EINVAL), an extended domain of 1 .. 16 cosets (H2MI_ERANGE)
static int check_scalars(const h2mi_quotient_scalars* q) {
  if (!q || !q->beta || !q->gamma || !q->y || !q->delta || !q->zeta || !q->extended_omega || !q->t_inv) return H2MI_EINVAL;
  if (q->extended_k < q->k || q->extended_k - q->k > 4 || q->extended_k > H2MI_MAX_LOG_N) return H2MI_ERANGE;
  return H2MI_OK;
}
static void fill_common(HConsts& h, const h2mi_quotient_scalars& q, uint32_t n_cur) {
  const fe beta = host_fe(q.beta), delta = host_fe(q.delta);
  memset(&h, 0, sizeof(h));
  h.beta0 = beta;
  h.beta_m1 = h_level(beta, -1);
  h.gamma0 = host_fe(q.gamma);
  h.one0 = h_canon(f29_const<F9>(F9::TO256));
  h.one_m2 = h_level(h.one0, -2);
  fe cur = h_mul256(beta, host_fe(q.zeta));
  for (uint32_t j = 0; j < n_cur; j++) {
    h.cur[j] = cur;
    cur = h_mul256(cur, delta);
  }
  for (uint32_t i = 0; i < 1u << (q.extended_k - q.k); i++) h.tinv[i] = h_level(host_fe(q.t_inv + 4 * i), -1);
}
// the same scalars as the general and the interpreting kernels take them
static FlexConsts flex_consts(const h2mi_quotient_scalars& q) {
  FlexConsts h;
  memset(&h, 0, sizeof(h));
  h.beta = host_fe(q.beta); h.gamma = host_fe(q.gamma); h.y = host_fe(q.y); h.delta = host_fe(q.delta); h.zeta = host_fe(q.zeta);
  for (uint32_t i = 0; i < 1u << (q.extended_k - q.k); i++) h.tinv[i] = host_fe(q.t_inv + 4 * i);
  return h;
}

// the permutation / lookup / Lagrange pointers of h2mi_flex_cosets or h2mi_expr_cosets (the same fields) -> the kernels' argument
template <class Cosets>
static bool fill_tail(FlexCosets& fc, const Cosets& c) {
  fc.n_perm = c.n_perm; fc.chunk = c.chunk_len ? c.chunk_len : 1;
  fc.n_lookups = c.n_lookups & ~(uint32_t)H2MI_LOOKUPS_LOGUP; fc.logup = (c.n_lookups & H2MI_LOOKUPS_LOGUP) ? 1u : 0u;
  if (fc.n_lookups > H2MI_FLEX_MAX_LOOKUPS) return false;
  fc.lk_sets = 0x11111111u;  // one input set per lookup; fill_sets states another count
  for (uint32_t j = 0; j < c.n_perm; j++) {
    fc.perm_value[j] = (const fe*)c.perm_value[j]; fc.perm_sigma[j] = (const fe*)c.perm_sigma[j];
    if (!fc.perm_value[j] || !fc.perm_sigma[j]) return false;
  }
  for (uint32_t q = 0; c.n_perm && q < (c.n_perm + fc.chunk - 1) / fc.chunk; q++) {
    fc.perm_z[q] = (const fe*)c.perm_z[q];
    if (!fc.perm_z[q]) return false;
  }
  for (uint32_t l = 0; l < fc.n_lookups; l++) {
    fc.lk_in[l] = (const fe*)c.lookup_input[l]; fc.lk_in_b[l] = (const fe*)c.lookup_input_b[l]; fc.lk_table[l] = (const fe*)c.lookup_table[l];
    fc.lk_pin[l] = (const fe*)c.lookup_permuted_input[l]; fc.lk_ptab[l] = (const fe*)c.lookup_permuted_table[l]; fc.lk_z[l] = (const fe*)c.lookup_z[l];
    if (!fc.lk_in[l] || !fc.lk_table[l] || !fc.lk_pin[l] || (!fc.lk_ptab[l] && !fc.logup) || !fc.lk_z[l]) return false;
  }
  fc.l0 = (const fe*)c.l0; fc.l_last = (const fe*)c.l_last; fc.l_active = (const fe*)c.l_active;
  return fc.l0 && fc.l_last && fc.l_active;
}

// the input sets of an h2mi_logup_cosets (NULL: one per lookup) -> the kernels' argument.  A count of 0 or above the maximum, or
// another count than 1 where the lookups are no logUp arguments, is the caller's mistake
static bool fill_sets(FlexCosets& fc, const h2mi_logup_cosets* lg) {
  static_assert(H2MI_FLEX_MAX_LOOKUPS * 4 <= 32 && H2MI_MAX_LOGUP_INPUTS < 16, "four bits per lookup");
  if (!lg) return true;
  fc.lk_sets = 0;
  for (uint32_t l = 0; l < H2MI_FLEX_MAX_LOOKUPS; l++) {
    const uint32_t sets = l < fc.n_lookups ? lg->n_inputs[l] : 1u;  // counts beyond n_lookups are not read
    if (sets == 0 || sets > H2MI_MAX_LOGUP_INPUTS || (sets != 1 && !fc.logup)) return false;
    fc.lk_sets |= sets << (4 * l);
  }
  return true;
}

// the shuffle pointers of an h2mi_shuffle_cosets (NULL: none) -> the kernels' argument
static bool fill_shuffles(FlexCosets& fc, const h2mi_shuffle_cosets* sc) {
  fc.n_shuffles = sc ? sc->n_shuffles : 0;
  if (fc.n_shuffles > H2MI_MAX_SHUFFLES) return false;
  for (uint32_t s = 0; s < fc.n_shuffles; s++) {
    fc.sf_in[s] = (const fe*)sc->input[s]; fc.sf_tab[s] = (const fe*)sc->shuffle[s]; fc.sf_z[s] = (const fe*)sc->z[s];
    if (!fc.sf_in[s] || !fc.sf_tab[s] || !fc.sf_z[s]) return false;
  }
  return true;
}

// The program as the kernel reads it.  Every stack value carries a static bound in units of p (a converted load 1.04, a constant 1,
// a product 1 + 0.006 a b since p / 2^261 < 0.006, a sum a + b, a difference a + 4, a negation 4, EX_RED 1 + 0.006 a); EX_RED goes
// in front of a SUB / NEG whose subtrahend may reach 4p - 2^232 (f29_sub's contract with K4) and behind an operation whose result
// may pass 8p, the range k_evaluate_h_flex keeps its values in.  The reference's gates and the vertical gate need none.
static void expr_encode(const h2mi_gate_program* g, uint32_t k, uint32_t extended_k, std::vector<uint2>& out) {
  const uint32_t n = 1u << k, rot = 1u << (extended_k - k);
  double b[H2MI_MAX_EXPR_STACK];
  uint32_t sp = 0;
  auto emit = [&](uint32_t code, uint32_t index = 0, uint32_t off = 0) { out.push_back(make_uint2(code | index << 8, off)); };
  auto cap = [&] {
    if (b[sp - 1] > 8.0) { emit(EX_RED); b[sp - 1] = 1.0 + 0.006 * b[sp - 1]; }
  };
  auto small_top = [&] {
    if (b[sp - 1] > 3.9) { emit(EX_RED); b[sp - 1] = 1.0 + 0.006 * b[sp - 1]; }
  };
  for (uint32_t i = 0; i < g->n_ops; i++) {
    const h2mi_expr_op& o = g->ops[i];
    switch (o.op) {
      case H2MI_EXPR_ADVICE: case H2MI_EXPR_FIXED: case H2MI_EXPR_INSTANCE: {
        const uint32_t slot = o.op == H2MI_EXPR_ADVICE ? o.index : o.op == H2MI_EXPR_FIXED ? H2MI_EXPR_MAX_ADVICE + o.index : EX_INSTANCE + o.index;
        emit(EX_COL, slot, (uint32_t)(((int64_t)o.rotation + n) % n) * rot);
        b[sp++] = 1.04;
        break;
      }
      case H2MI_EXPR_CONSTANT: emit(EX_CONST, o.index); b[sp++] = 1.0; break;
      case H2MI_EXPR_CHALLENGE: emit(EX_CONST, g->n_constants + o.index); b[sp++] = 1.0; break;  // canonical like a constant: the same bound
      case H2MI_EXPR_ADD: emit(EX_ADD); b[sp - 2] += b[sp - 1]; sp--; cap(); break;
      case H2MI_EXPR_SUB: small_top(); emit(EX_SUB); b[sp - 2] += 4.0; sp--; cap(); break;
      case H2MI_EXPR_MUL: emit(EX_MUL); b[sp - 2] = 1.0 + 0.006 * b[sp - 2] * b[sp - 1]; sp--; break;
      case H2MI_EXPR_NEG: small_top(); emit(EX_NEG); b[sp - 1] = 4.0; break;
      default: emit(EX_END); sp = 0; break;  // H2MI_EXPR_END (expr_walk has refused anything else)
    }
  }
}

// What an interpreting launch reads, validated (expr_walk: a malformed program, a NULL column, a constant beyond n_constants or a
// rotation of 2^k or more is H2MI_EINVAL) and laid out as ONE buffer: the column-pointer table, the constants and behind them the
// challenges as Montgomery-2^261 words, the ops (each part a whole number of 32-byte words).  dom_k: the domain the columns are given
// on (k or extended_k).
// the instance columns of one circuit as the entry points take them: an h2mi_instance_cosets, or without one the entry's own
// `instance` pointer (column 0).  ok = false: more columns than the table holds
struct InstanceCols {
  const void* col[H2MI_MAX_INSTANCE] = {nullptr};
  bool ok = true;
  InstanceCols(const h2mi_instance_cosets* in, const void* single) {
    if (!in) { col[0] = single; return; }
    ok = in->n_instance <= H2MI_MAX_INSTANCE;
    for (uint32_t i = 0; ok && i < in->n_instance; i++) col[i] = in->column[i];
  }
  bool has(uint32_t index) const { return index < H2MI_MAX_INSTANCE && col[index]; }
};
struct ExprImage {
  std::vector<fe> image;
  size_t cols_fe = 0, const_fe = 0, lds = 0;
  uint32_t n_ops = 0;
  int build(const h2mi_gate_program* g, const uint64_t* challenges, uint32_t n_challenges, const void* const* advice, const void* const* fixed,
            const InstanceCols& instance, uint32_t k, uint32_t dom_k) {
    if (n_challenges > H2MI_MAX_CHALLENGES || (n_challenges && !challenges)) return H2MI_EINVAL;
    ExprShape shape;
    const int rc = expr_walk(g, k, n_challenges, [&](uint32_t kind, uint32_t index, int32_t) {
      return kind == H2MI_EXPR_ADVICE ? index < H2MI_EXPR_MAX_ADVICE && advice[index]
           : kind == H2MI_EXPR_FIXED  ? index < H2MI_EXPR_MAX_FIXED && fixed[index]
                                      : instance.has(index);
    }, &shape);
    if (rc) return rc;
    std::vector<uint2> ops;
    expr_encode(g, k, dom_k, ops);
    cols_fe = (EX_COLS * sizeof(void*) + 31) / 32;
    const_fe = std::max<size_t>((size_t)g->n_constants + n_challenges, 1);
    const size_t ops_fe = (ops.size() * 8 + 31) / 32;
    image.resize(cols_fe + const_fe + ops_fe);
    memset(image.data(), 0, image.size() * sizeof(fe));
    const void** tab = (const void**)image.data();
    for (uint32_t i = 0; i < H2MI_EXPR_MAX_ADVICE; i++) tab[i] = advice[i];
    for (uint32_t i = 0; i < H2MI_EXPR_MAX_FIXED; i++) tab[H2MI_EXPR_MAX_ADVICE + i] = fixed[i];
    for (uint32_t i = 0; i < H2MI_MAX_INSTANCE; i++) tab[EX_INSTANCE + i] = instance.col[i];
    for (uint32_t i = 0; i < g->n_constants; i++) image[cols_fe + i] = h_canon(f29_from_mont256<F9>(host_fe(g->constants + 4 * i).v));
    for (uint32_t i = 0; i < n_challenges; i++) image[cols_fe + g->n_constants + i] = h_canon(f29_from_mont256<F9>(host_fe(challenges + 4 * i).v));
    memcpy(&image[cols_fe + const_fe], ops.data(), ops.size() * 8);
    n_ops = (uint32_t)ops.size();
    lds = (size_t)(shape.max_stack - 1) * 9 * 256 * sizeof(uint32_t);  // at most 7 levels: 63 KB
    return H2MI_OK;
  }
};
// an h2mi_expr_columns on the 2^dom_k points it is given on, as ExprImage::build takes the columns (expr_compress, expr_check)
struct ColumnTables {
  const void* adv[H2MI_EXPR_MAX_ADVICE] = {nullptr};
  const void* fix[H2MI_EXPR_MAX_FIXED] = {nullptr};
  InstanceCols inst{nullptr, nullptr};
  int fill(const h2mi_expr_columns* c, uint32_t dom_k) {
    if (!c) return H2MI_EINVAL;
    inst = InstanceCols(c->instances, nullptr);
    if (!inst.ok || !c->program || (c->n_advice && !c->advice) || (c->n_fixed && !c->fixed) || c->n_advice > H2MI_EXPR_MAX_ADVICE ||
        c->n_fixed > H2MI_EXPR_MAX_FIXED)
      return H2MI_EINVAL;
    if (c->k == 0 || dom_k < c->k || dom_k - c->k > 4 || dom_k > H2MI_MAX_LOG_N) return H2MI_ERANGE;
    for (uint32_t i = 0; i < c->n_advice; i++) adv[i] = c->advice[i];
    for (uint32_t i = 0; i < c->n_fixed; i++) fix[i] = c->fixed[i];
    return H2MI_OK;
  }
};

}  // namespace h2

using namespace h2;

extern "C" {

// inclusive multiplicative scan of n elements, in place in `data` (forward prefix or reverse suffix)
static int mulscan(fe* data, size_t n, int reverse, fe* totals, fe* offsets, hipStream_t s) {
  const uint32_t nblocks = ceil_div_u32(n, MS_TILE);
  H2_LAUNCH("k_mulscan_local", k_mulscan_local, nblocks, 256, 0, s, (const fe*)data, n, reverse, data, totals);
  if (nblocks > 1) {
    H2_LAUNCH("k_mulscan_offsets", k_mulscan_offsets, 1, 1024, 0, s, (const fe*)totals, nblocks, offsets);
    H2_LAUNCH("k_mulscan_apply", k_mulscan_apply, ceil_div_u32(n, 256), 256, 0, s, data, (const fe*)offsets, n, reverse);
  }
  return H2MI_OK;
}

// The grand products' part of the transforms' shared, stream-ordered scratch: num, P (prefix of den), S (suffix of den) of `cap`
// elements each, the tile totals / offsets of `tiles` each, the inverse of the total.
struct RatioTmp {
  fe *num, *P, *S, *totals, *offsets, *inv_total;
};
static size_t ratio_tmp_size(size_t cap, uint32_t tiles) { return 3 * cap + 2 * (size_t)tiles + 2; }
static RatioTmp carve_ratio_tmp(size_t cap, uint32_t tiles) {
  RatioTmp t;
  t.num = tmp_base();
  t.P = t.num + cap;
  t.S = t.P + cap;
  t.totals = t.S + cap;
  t.offsets = t.totals + tiles;
  t.inv_total = t.offsets + tiles;
  return t;
}

// num[i] / P[i] over `total` elements with one inversion: the ratios overwrite num (P and S end as the prefix and suffix products)
static int ratios(const RatioTmp& t, size_t total, hipStream_t s) {
  H2_HIP(hipMemcpyAsync(t.S, t.P, total * 32, hipMemcpyDeviceToDevice, s));
  int rc = mulscan(t.P, total, 0, t.totals, t.offsets, s);
  if (!rc) rc = mulscan(t.S, total, 1, t.totals, t.offsets, s);
  if (rc) return rc;
  H2_LAUNCH("k_fr_inv_one", k_fr_inv_one, 1, 64, 0, s, (const fe*)(t.P + (total - 1)), t.inv_total);
  H2_LAUNCH("k_perm_ratio", k_perm_ratio, ceil_div_u32(total, 256), 256, 0, s, (const fe*)t.num, (const fe*)t.P, (const fe*)t.S, (const fe*)t.inv_total,
            total, t.num);
  return H2MI_OK;
}
// ... and their prefix products, which give z
static int running_product(const RatioTmp& t, size_t total, hipStream_t s) {
  const int rc = ratios(t, total, s);
  return rc ? rc : mulscan(t.num, total, 0, t.totals, t.offsets, s);
}

// ---- assigned cells (kernels: k_assigned_*) -------------------------------------------------------------------------------------------
// the three launches over n staged elements (stride 1: denominators alone, 2: (numerator, denominator) pairs)
static int assigned_chain(const fe* in, uint32_t stride, size_t n, int canonical, const AssignedSegs& segs, fe* totals, fe* tileinv,
                          unsigned long long* invalid, hipStream_t s) {
  const uint32_t ntiles = ceil_div_u32(n, ASG_TILE);
  H2_LAUNCH("k_assigned_tile_products", k_assigned_tile_products, ntiles, 256, 0, s, in, stride, n, canonical, totals, invalid);
  H2_LAUNCH("k_assigned_tile_inverses", k_assigned_tile_inverses, 1, 1024, 0, s, (const fe*)totals, ntiles, tileinv);
  H2_LAUNCH("k_assigned_finish", k_assigned_finish, ntiles, 256, 0, s, in, stride, n, canonical, (const fe*)tileinv, segs, invalid);
  return H2MI_OK;
}
static int assigned_vector(const void* d_in, uint32_t stride, size_t n, void* d_out, h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (n == 0) return H2MI_OK;
  if (!d_in || !d_out || ((uintptr_t)d_in & 15u) || ((uintptr_t)d_out & 15u) || n > ((size_t)1 << 32)) return H2MI_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  hipStream_t s = pick_stream(stream);
  const uint32_t ntiles = ceil_div_u32(n, ASG_TILE);
  int rc = ensure_tmp(2 * (size_t)ntiles + 1, s);
  if (rc) return rc;
  AssignedSegs segs;
  memset(&segs, 0, sizeof(segs));
  segs.n_segs = 1;
  segs.dst[0] = (fe*)d_out;
  segs.start[1] = n;
  rc = assigned_chain((const fe*)d_in, stride, n, 0, segs, tmp_base(), tmp_base() + ntiles, reinterpret_cast<unsigned long long*>(tmp_base() + 2 * (size_t)ntiles), s);
  return rc ? rc : release_tmp(s);
}
int h2mi_fr_batch_invert_dev(const void* d_in, size_t n, void* d_out, h2mi_stream_t stream) { return assigned_vector(d_in, 1, n, d_out, stream); }
int h2mi_fr_assigned_evaluate_dev(const void* d_pairs, size_t n, void* d_out, h2mi_stream_t stream) {
  if (n && d_pairs == d_out) return H2MI_EINVAL;  // a thread's four results would overwrite pairs of its neighbours
  return assigned_vector(d_pairs, 2, n, d_out, stream);
}
int h2mi_fr_assigned_columns_dev(const h2mi_assigned_cells* cols, uint32_t n_cols, int canonical, uint64_t* invalid_out, h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (invalid_out) *invalid_out = 0;
  if (n_cols == 0) return H2MI_OK;
  if (!cols || n_cols > ASG_MAX_SEGS || (canonical && !invalid_out)) return H2MI_EINVAL;
  size_t total = 0, listed = 0;
  for (uint32_t i = 0; i < n_cols; i++) {
    if (!cols[i].d_column || !cols[i].pairs || cols[i].count == 0 || ((uintptr_t)cols[i].d_column & 15u)) return H2MI_EINVAL;
    total += cols[i].count;
    if (cols[i].rows) listed += cols[i].count;
  }
  if (total > ((size_t)1 << 32)) return H2MI_ERANGE;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  hipStream_t s = pick_stream(stream);
  const uint32_t ntiles = ceil_div_u32(total, ASG_TILE);
  const size_t rows_fe = (listed + 7) / 8;  // eight row indices per 32 bytes
  int rc = ensure_tmp(2 * total + rows_fe + 2 * (size_t)ntiles + 1, s);
  if (rc) return rc;
  fe* pairs = tmp_base();
  uint32_t* rows = reinterpret_cast<uint32_t*>(pairs + 2 * total);
  fe* totals = pairs + 2 * total + rows_fe;
  unsigned long long* invalid = reinterpret_cast<unsigned long long*>(totals + 2 * (size_t)ntiles);
  AssignedSegs segs;
  memset(&segs, 0, sizeof(segs));
  segs.n_segs = n_cols;
  size_t at = 0, at_rows = 0;
  for (uint32_t i = 0; i < n_cols; i++) {
    H2_HIP(hipMemcpyAsync(pairs + 2 * at, cols[i].pairs, cols[i].count * 64, hipMemcpyHostToDevice, s));
    segs.dst[i] = (fe*)cols[i].d_column;
    segs.start[i] = at;
    if (cols[i].rows) {
      H2_HIP(hipMemcpyAsync(rows + at_rows, cols[i].rows, cols[i].count * 4, hipMemcpyHostToDevice, s));
      segs.rows[i] = rows + at_rows;
      at_rows += cols[i].count;
    }
    at += cols[i].count;
  }
  segs.start[n_cols] = total;
  // the caller's buffers are free when this call returns, as after h2mi_memcpy_h2d on the plain route: columns of 64 MB and more are
  // not images the runtime is sure to have staged by the time hipMemcpyAsync returns.  The chain itself stays asynchronous
  H2_HIP(hipStreamSynchronize(s));
  if (canonical) H2_HIP(hipMemsetAsync(invalid, 0, 8, s));
  rc = assigned_chain(pairs, 2, total, canonical, segs, totals, totals + ntiles, invalid, s);
  if (rc) return rc;
  rc = release_tmp(s);
  if (rc || !canonical) return rc;
  unsigned long long v = 0;
  H2_HIP(hipMemcpyAsync(&v, invalid, 8, hipMemcpyDeviceToHost, s));
  H2_HIP(hipStreamSynchronize(s));
  *invalid_out = v;
  return H2MI_OK;
}

static bool rows_out_of_range(uint32_t k, uint32_t usable_rows) {
  return k == 0 || k > H2MI_MAX_LOG_N || usable_rows == 0 || usable_rows >= ((uint64_t)1 << k);
}

static ZOut single_out(void* d_z) {
  ZOut zo;
  memset(&zo, 0, sizeof(zo));
  zo.z[0] = (fe*)d_z;
  return zo;
}

int h2mi_plonk_permutation_product_dev(const void* const* d_values, const void* const* d_sigmas, uint32_t m, uint32_t k, uint32_t usable_rows,
                                       const uint64_t beta[4], const uint64_t gamma[4], const uint64_t* beta_delta_pows, const uint64_t omega[4],
                                       const void* d_start_or_null, void* d_z, void* d_last_or_null, h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (!d_values || !d_sigmas || !beta || !gamma || !beta_delta_pows || !omega || !d_z || m == 0 || m > H2MI_FLEX_MAX_PERM) return H2MI_EINVAL;
  if (rows_out_of_range(k, usable_rows)) return H2MI_ERANGE;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  CallScope scope_;
  hipStream_t s = pick_stream(stream);
  const size_t n = (size_t)1 << k;
  PermArgs a;
  memset(&a, 0, sizeof(a));
  a.m = m;
  a.beta = host_fe(beta);
  a.gamma = host_fe(gamma);
  for (uint32_t j = 0; j < m; j++) {
    if (!d_values[j] || !d_sigmas[j]) return H2MI_EINVAL;
    a.value[j] = (const fe*)d_values[j];
    a.sigma[j] = (const fe*)d_sigmas[j];
    a.beta_delta[j] = host_fe(beta_delta_pows + 4 * j);
  }
  PowTab pw;
  int rc = get_powtab(omega, k, s, &pw);
  if (rc) return rc;
  const uint32_t nblocks = ceil_div_u32(n, MS_TILE);
  rc = ensure_tmp(ratio_tmp_size(n, nblocks), s);
  if (rc) return rc;
  const RatioTmp t = carve_ratio_tmp(n, nblocks);
  H2_LAUNCH("k_perm_numden", k_perm_numden, ceil_div_u32(n, 256), 256, 0, s, a, n, usable_rows, (const fe*)pw.lo, (const fe*)pw.hi, pw.h, t.num, t.P);
  rc = running_product(t, n, s);
  if (rc) return rc;
  H2_LAUNCH("k_perm_write", k_perm_write, ceil_div_u32((uint64_t)usable_rows + 1, 256), 256, 0, s, (const fe*)t.num, (const fe*)d_start_or_null, usable_rows,
            (fe*)d_z, (fe*)d_last_or_null);
  return release_tmp(s);
}

static int perm_products(const void* const* d_values, const void* const* d_sigmas, uint32_t m, uint32_t chunk_len, uint32_t k, uint32_t usable_rows,
                         const uint64_t beta[4], const uint64_t gamma[4], const uint64_t* beta_delta_pows, const uint64_t omega[4],
                         const uint32_t* d_active, uint32_t n_active, void* const* d_z, h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (!d_values || !d_sigmas || !beta || !gamma || !beta_delta_pows || !omega || !d_z || m == 0 || m > H2MI_FLEX_MAX_PERM || chunk_len == 0) return H2MI_EINVAL;
  if (rows_out_of_range(k, usable_rows)) return H2MI_ERANGE;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  CallScope scope_;
  hipStream_t s = pick_stream(stream);
  const uint32_t sets = (m + chunk_len - 1) / chunk_len;
  if (d_active && (uint64_t)sets * usable_rows >= ((uint64_t)1 << 32)) return H2MI_ERANGE;  // positions are 32-bit
  PermArgs a;
  memset(&a, 0, sizeof(a));
  a.m = m;
  a.beta = host_fe(beta);
  a.gamma = host_fe(gamma);
  for (uint32_t j = 0; j < m; j++) {
    if (!d_values[j] || !d_sigmas[j]) return H2MI_EINVAL;
    a.value[j] = (const fe*)d_values[j];
    a.sigma[j] = (const fe*)d_sigmas[j];
    a.beta_delta[j] = host_fe(beta_delta_pows + 4 * j);
  }
  ZOut zo;
  memset(&zo, 0, sizeof(zo));
  for (uint32_t q = 0; q < sets; q++) {
    if (!d_z[q]) return H2MI_EINVAL;
    zo.z[q] = (fe*)d_z[q];
  }
  const dim3 wgrid(ceil_div_u32((uint64_t)usable_rows + 1, 256), sets);
  if (d_active && n_active == 0) {  // no copy constraint touches a usable row: every product is one
    H2_LAUNCH("k_perm_write_sets", k_perm_write_sets, wgrid, 256, 0, s, (const fe*)nullptr, usable_rows, zo, d_active, 0u);
    return H2MI_OK;
  }
  PowTab pw;
  int rc = get_powtab(omega, k, s, &pw);
  if (rc) return rc;
  if (d_active && n_active <= PERM_SMALL_MAX) {
    rc = ensure_tmp(PERM_SMALL_MAX, s);
    if (rc) return rc;
    H2_LAUNCH("k_perm_sparse_small", k_perm_sparse_small, 1, PERM_SMALL_MAX, 0, s, a, chunk_len, n_active, usable_rows, (const fe*)pw.lo,
              (const fe*)pw.hi, pw.h, d_active, tmp_base());
    H2_LAUNCH("k_perm_write_sets", k_perm_write_sets, wgrid, 256, 0, s, (const fe*)tmp_base(), usable_rows, zo, d_active, n_active);
    return release_tmp(s);
  }
  const size_t total = d_active ? (size_t)n_active : (size_t)sets * usable_rows;  // elements the scans run over
  const uint32_t nblocks = ceil_div_u32(total, MS_TILE);
  rc = ensure_tmp(ratio_tmp_size(total, nblocks), s);
  if (rc) return rc;
  const RatioTmp t = carve_ratio_tmp(total, nblocks);
  H2_LAUNCH("k_perm_numden_sets", k_perm_numden_sets, ceil_div_u32(total, 256), 256, 0, s, a, chunk_len, total, usable_rows, (const fe*)pw.lo, (const fe*)pw.hi,
            pw.h, d_active, t.num, t.P);
  rc = running_product(t, total, s);
  if (rc) return rc;
  if (d_active) H2_LAUNCH("k_perm_to_mont256", k_perm_to_mont256, ceil_div_u32(n_active, 256), 256, 0, s, t.num, n_active);
  H2_LAUNCH("k_perm_write_sets", k_perm_write_sets, wgrid, 256, 0, s, (const fe*)t.num, usable_rows, zo, d_active, n_active);
  return release_tmp(s);
}

int h2mi_plonk_permutation_products_dev(const void* const* d_values, const void* const* d_sigmas, uint32_t m, uint32_t chunk_len, uint32_t k,
                                        uint32_t usable_rows, const uint64_t beta[4], const uint64_t gamma[4], const uint64_t* beta_delta_pows,
                                        const uint64_t omega[4], void* const* d_z, h2mi_stream_t stream) {
  return perm_products(d_values, d_sigmas, m, chunk_len, k, usable_rows, beta, gamma, beta_delta_pows, omega, nullptr, 0, d_z, stream);
}

int h2mi_plonk_permutation_products_sparse_dev(const void* const* d_values, const void* const* d_sigmas, uint32_t m, uint32_t chunk_len, uint32_t k,
                                               uint32_t usable_rows, const uint64_t beta[4], const uint64_t gamma[4], const uint64_t* beta_delta_pows,
                                               const uint64_t omega[4], const void* d_active, uint32_t n_active, void* const* d_z, h2mi_stream_t stream) {
  if (!d_active) return H2MI_EINVAL;
  return perm_products(d_values, d_sigmas, m, chunk_len, k, usable_rows, beta, gamma, beta_delta_pows, omega, (const uint32_t*)d_active, n_active, d_z,
                       stream);
}

int h2mi_plonk_lookup_product_dev(const void* d_input, const void* d_table, const void* d_permuted_input, const void* d_permuted_table, uint32_t k,
                                  uint32_t usable_rows, const uint64_t beta[4], const uint64_t gamma[4], void* d_z, h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (!d_input || !d_table || !d_permuted_input || !d_permuted_table || !beta || !gamma || !d_z) return H2MI_EINVAL;
  if (rows_out_of_range(k, usable_rows)) return H2MI_ERANGE;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  CallScope scope_;
  hipStream_t s = pick_stream(stream);
  const size_t u = usable_rows;
  const uint32_t uu = (usable_rows + 3u) & ~3u;  // scan length (a multiple of 4; the pad flags are zero)
  const uint32_t nseg = ceil_div_u32(uu, SCAN_SEG_BINS) + 1;
  const size_t words = 2 * ((size_t)uu + 8) + nseg + 8 + u / 4 + 8;  // flag, pos (+ total), segment sums, active positions
  const uint32_t nblocks_dense = ceil_div_u32(u, MS_TILE);
  int rc = ensure_tmp(ratio_tmp_size(u, nblocks_dense) + (words * 4 + 31) / 32, s);
  if (rc) return rc;
  uint32_t* flag = reinterpret_cast<uint32_t*>(tmp_base() + ratio_tmp_size(u, nblocks_dense));
  uint32_t* pos = flag + uu + 8;
  uint32_t* segsum = pos + uu + 8;
  uint32_t* active = segsum + nseg + 8;
  const fe *in = (const fe*)d_input, *tab = (const fe*)d_table, *pin = (const fe*)d_permuted_input, *ptab = (const fe*)d_permuted_table;
  // the rows whose ratio can differ from one; the count decides between the sparse and the dense form (one 4-byte read)
  uint32_t n_act = usable_rows;
  if (usable_rows >= 4096) {
    H2_LAUNCH("k_lookup_flag", k_lookup_flag, ceil_div_u32(uu, 256), 256, 0, s, in, tab, pin, ptab, usable_rows, uu, flag);
    const uint32_t segs = ceil_div_u32(uu, SCAN_SEG_BINS);
    if (segs > 1) H2_LAUNCH("k_scan_segsum", k_scan_segsum<SCAN_SEG_BINS>, segs, 1024, 0, s, (const uint32_t*)flag, uu, segsum);
    H2_LAUNCH("k_scan_seg_lookup", k_scan_seg<SCAN_SEG_BINS>, dim3(segs, 1), 1024, 0, s, (const uint32_t*)flag, pos, (const uint32_t*)nullptr, (uint32_t*)nullptr, uu,
              (const uint32_t*)segsum);
    H2_HIP(hipMemcpyAsync(&n_act, pos + uu, 4, hipMemcpyDeviceToHost, s));
    H2_HIP(hipStreamSynchronize(s));
  }
  const bool sparse = (size_t)n_act * 4 <= u && usable_rows >= 4096;
  const size_t total = sparse ? n_act : u;
  const RatioTmp t = carve_ratio_tmp(u, nblocks_dense);  // carved for the dense form; the scans run over total <= u
  const ZOut zo = single_out(d_z);
  if (sparse && n_act == 0) {  // every ratio is one: z = 1 on rows 0 .. u (an empty position list)
    H2_LAUNCH("k_perm_write_sets", k_perm_write_sets, dim3(ceil_div_u32((uint64_t)usable_rows + 1, 256), 1), 256, 0, s, (const fe*)t.num, usable_rows, zo,
              (const uint32_t*)active, 0u);
    return release_tmp(s);
  }
  if (sparse) {
    H2_LAUNCH("k_lookup_compact", k_lookup_compact, ceil_div_u32(usable_rows, 256), 256, 0, s, (const uint32_t*)flag, (const uint32_t*)pos, usable_rows, active);
    H2_LAUNCH("k_lookup_numden", k_lookup_numden_sparse, ceil_div_u32(n_act, 256), 256, 0, s, in, tab, pin, ptab, host_fe(beta), host_fe(gamma),
              (const uint32_t*)active, n_act, t.num, t.P);
  } else {
    H2_LAUNCH("k_lookup_numden", k_lookup_numden, ceil_div_u32(total, 256), 256, 0, s, in, tab, pin, ptab, host_fe(beta), host_fe(gamma), usable_rows, t.num, t.P);
  }
  rc = running_product(t, total, s);
  if (rc) return rc;
  if (sparse) {
    H2_LAUNCH("k_perm_to_mont256", k_perm_to_mont256, ceil_div_u32(n_act, 256), 256, 0, s, t.num, n_act);
    H2_LAUNCH("k_perm_write_sets", k_perm_write_sets, dim3(ceil_div_u32((uint64_t)usable_rows + 1, 256), 1), 256, 0, s, (const fe*)t.num, usable_rows, zo,
              (const uint32_t*)active, n_act);
  } else {
    H2_LAUNCH("k_perm_write_sets", k_perm_write_sets, dim3(ceil_div_u32((uint64_t)usable_rows + 1, 256), 1), 256, 0, s, (const fe*)t.num, usable_rows, zo,
              (const uint32_t*)nullptr, 0u);
  }
  return release_tmp(s);
}

int h2mi_plonk_shuffle_product_dev(const void* d_input, const void* d_shuffle, uint32_t k, uint32_t usable_rows, const uint64_t gamma[4], void* d_z,
                                   h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (!d_input || !d_shuffle || !gamma || !d_z) return H2MI_EINVAL;
  if (rows_out_of_range(k, usable_rows)) return H2MI_ERANGE;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  CallScope scope_;
  hipStream_t s = pick_stream(stream);
  const size_t u = usable_rows;
  const uint32_t nblocks = ceil_div_u32(u, MS_TILE);
  int rc = ensure_tmp(ratio_tmp_size(u, nblocks), s);
  if (rc) return rc;
  const RatioTmp t = carve_ratio_tmp(u, nblocks);
  const ZOut zo = single_out(d_z);
  H2_LAUNCH("k_shuffle_numden", k_shuffle_numden, ceil_div_u32(u, 256), 256, 0, s, (const fe*)d_input, (const fe*)d_shuffle, host_fe(gamma), usable_rows, t.num, t.P);
  rc = running_product(t, u, s);
  if (rc) return rc;
  H2_LAUNCH("k_perm_write_sets", k_perm_write_sets, dim3(ceil_div_u32((uint64_t)usable_rows + 1, 256), 1), 256, 0, s, (const fe*)t.num, usable_rows, zo,
            (const uint32_t*)nullptr, 0u);
  // the ONE comparison: a satisfied shuffle ends at one (the Montgomery-2^256 one, fully reduced as every stored value is)
  fe last;
  H2_HIP(hipMemcpyAsync(&last, (const fe*)d_z + u, sizeof(fe), hipMemcpyDeviceToHost, s));
  H2_HIP(hipStreamSynchronize(s));
  rc = release_tmp(s);
  if (rc) return rc;
  const fe one = h_canon(f29_const<F9>(F9::TO256));
  return memcmp(last.v, one.v, sizeof(one.v)) ? H2MI_EUNSAT : H2MI_OK;
}

int h2mi_plonk_logup_sum_dev(const void* d_input, const void* d_table, const void* d_m, uint32_t k, uint32_t usable_rows, const uint64_t beta[4],
                             void* d_phi, h2mi_stream_t stream) {
  return h2mi_plonk_logup_sum_sets_dev(d_input, 1, d_table, d_m, k, usable_rows, beta, d_phi, stream);
}

int h2mi_plonk_logup_sum_sets_dev(const void* d_inputs, uint32_t n_inputs, const void* d_table, const void* d_m, uint32_t k, uint32_t usable_rows,
                                  const uint64_t beta[4], void* d_phi, h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  const void* d_input = d_inputs;
  if (!d_input || !d_table || !d_m || !beta || !d_phi || n_inputs == 0 || n_inputs > H2MI_MAX_LOGUP_INPUTS) return H2MI_EINVAL;
  if (rows_out_of_range(k, usable_rows)) return H2MI_ERANGE;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  CallScope scope_;
  hipStream_t s = pick_stream(stream);
  const size_t u = usable_rows;
  const uint32_t nblocks = ceil_div_u32(u, MS_TILE);
  static_assert(AS_TILE == MS_TILE, "one pair of totals / offsets vectors serves both scans");
  int rc = ensure_tmp(ratio_tmp_size(u, nblocks), s);
  if (rc) return rc;
  const RatioTmp t = carve_ratio_tmp(u, nblocks);
  if (n_inputs == 1)
    H2_LAUNCH("k_logup_numden", k_logup_numden, ceil_div_u32(u, 256), 256, 0, s, (const fe*)d_input, (const fe*)d_table, (const fe*)d_m, host_fe(beta),
              usable_rows, t.num, t.P);
  else
    H2_LAUNCH("k_logup_numden_sets", k_logup_numden_sets, ceil_div_u32(u, 256), 256, 0, s, (const fe*)d_input, n_inputs, (size_t)1 << k, (const fe*)d_table,
              (const fe*)d_m, host_fe(beta), usable_rows, t.num, t.P);
  rc = ratios(t, u, s);
  if (rc) return rc;
  H2_LAUNCH("k_addscan_local", k_addscan_local, nblocks, 256, 0, s, (const fe*)t.num, usable_rows, t.num, t.totals);
  if (nblocks > 1) H2_LAUNCH("k_addscan_offsets", k_addscan_offsets, 1, 1024, 0, s, (const fe*)t.totals, nblocks, t.offsets);
  H2_LAUNCH("k_addscan_apply", k_addscan_apply<true>, ceil_div_u32((uint64_t)usable_rows + 1, 256), 256, 0, s, (const fe*)t.num,
            (const fe*)(nblocks > 1 ? t.offsets : nullptr), usable_rows, (fe*)d_phi);
  return release_tmp(s);
}

int h2mi_plonk_logup_sum_ranked_dev(const void* d_ranks, uint32_t n_inputs, const void* d_sorted_mont, const void* d_counts, const void* d_first,
                                    uint32_t n_unique, uint32_t k, uint32_t usable_rows, const uint64_t beta[4], void* d_phi, h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (!d_ranks || !d_sorted_mont || !d_counts || !d_first || !beta || !d_phi || n_unique == 0 || n_inputs == 0 || n_inputs > H2MI_MAX_LOGUP_INPUTS)
    return H2MI_EINVAL;
  if (rows_out_of_range(k, usable_rows) || n_unique > usable_rows) return H2MI_ERANGE;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  CallScope scope_;
  hipStream_t s = pick_stream(stream);
  const size_t u = usable_rows;
  const uint32_t nblocks = ceil_div_u32(u, AS_TILE), ntiles = ceil_div_u32(n_unique, ASG_TILE);
  // scratch (elements): term[u] den[n_unique] T[n_unique] totals[nblocks] offsets[nblocks] tile products[ntiles] tile inverses[ntiles] invalid[1]
  int rc = ensure_tmp(u + 2 * (size_t)n_unique + 2 * (size_t)nblocks + 2 * (size_t)ntiles + 1, s);
  if (rc) return rc;
  fe* term = tmp_base();
  fe* den = term + u;
  fe* T = den + n_unique;
  fe* totals = T + n_unique;
  fe* offsets = totals + nblocks;
  fe* tprod = offsets + nblocks;
  fe* tileinv = tprod + ntiles;
  AssignedSegs segs;
  memset(&segs, 0, sizeof(segs));
  segs.n_segs = 1;
  segs.dst[0] = T;
  segs.start[1] = n_unique;
  H2_LAUNCH("k_logup_table_den", k_logup_table_den, ceil_div_u32(n_unique, 256), 256, 0, s, (const fe*)d_sorted_mont, host_fe(beta), n_unique, den);
  rc = assigned_chain(den, 1, n_unique, 0, segs, tprod, tileinv, reinterpret_cast<unsigned long long*>(tileinv + ntiles), s);  // the ONE inversion
  if (rc) return rc;
  H2_LAUNCH("k_logup_gather", k_logup_gather, ceil_div_u32(u, 256), 256, 0, s, (const uint32_t*)d_ranks, n_inputs, (size_t)1 << k, (const fe*)T, n_unique,
            usable_rows, term);
  H2_LAUNCH("k_logup_table_side", k_logup_table_side, ceil_div_u32(n_unique, 256), 256, 0, s, (const uint32_t*)d_counts, (const uint32_t*)d_first,
            (const fe*)T, n_unique, usable_rows, term);
  H2_LAUNCH("k_addscan_local", k_addscan_local, nblocks, 256, 0, s, (const fe*)term, usable_rows, term, totals);
  if (nblocks > 1) H2_LAUNCH("k_addscan_offsets", k_addscan_offsets, 1, 1024, 0, s, (const fe*)totals, nblocks, offsets);
  H2_LAUNCH("k_addscan_apply", k_addscan_apply<false>, ceil_div_u32((uint64_t)usable_rows + 1, 256), 256, 0, s, (const fe*)term,
            (const fe*)(nblocks > 1 ? offsets : nullptr), usable_rows, (fe*)d_phi);
  return release_tmp(s);
}

int h2mi_plonk_evaluate_h_range_dev(const h2mi_range_cosets* c, const h2mi_quotient_scalars* q, void* d_h_out, h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (!c || !d_h_out) return H2MI_EINVAL;
  int rc = check_scalars(q);
  if (rc) return rc;
  const uint32_t k = q->k, extended_k = q->extended_k, blinding_factors = q->blinding_factors;
  if (c->n_perm == 0 || c->n_perm > 4 || c->chunk_len == 0 || c->chunk_len > 3) return H2MI_EINVAL;
  RangeCosets rc_;
  memset(&rc_, 0, sizeof(rc_));
  rc_.a = (const fe*)c->a; rc_.la = (const fe*)c->lookup_advice; rc_.ql = (const fe*)c->lookup_selector; rc_.q = (const fe*)c->q; rc_.table = (const fe*)c->table;
  rc_.lk_input = (const fe*)c->lookup_permuted_input; rc_.lk_table = (const fe*)c->lookup_permuted_table; rc_.lk_z = (const fe*)c->lookup_z;
  rc_.l0 = (const fe*)c->l0; rc_.l_last = (const fe*)c->l_last; rc_.l_active = (const fe*)c->l_active;
  rc_.n_perm = c->n_perm;
  rc_.chunk = c->chunk_len;
  rc_.has_lookup = c->has_lookup ? 1u : 0u;
  if (!rc_.a || !rc_.q || !rc_.l0 || !rc_.l_last || !rc_.l_active) return H2MI_EINVAL;
  if (rc_.has_lookup && ((!rc_.la && !rc_.ql) || !rc_.table || !rc_.lk_input || !rc_.lk_table || !rc_.lk_z)) return H2MI_EINVAL;
  for (uint32_t j = 0; j < c->n_perm; j++) {
    rc_.perm_value[j] = (const fe*)c->perm_value[j];
    rc_.perm_sigma[j] = (const fe*)c->perm_sigma[j];
    if (!rc_.perm_value[j] || !rc_.perm_sigma[j]) return H2MI_EINVAL;
  }
  for (uint32_t q = 0; q < (c->n_perm + c->chunk_len - 1) / c->chunk_len; q++) {
    rc_.perm_z[q] = (const fe*)c->perm_z[q];
    if (!rc_.perm_z[q]) return H2MI_EINVAL;
  }
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  CallScope scope_;
  hipStream_t s = pick_stream(stream);
  PowTab px;
  rc = get_powtab(q->extended_omega, extended_k, s, &px);
  if (rc) return rc;
  HConsts hcst;
  fill_common(hcst, *q, c->n_perm);
  {  // term i carries y^(N-1-i) at the level its expression needs (see the kernel's header)
    const uint32_t sets = (c->n_perm + c->chunk_len - 1) / c->chunk_len;
    const uint32_t N = 2 + 2 * sets + (rc_.has_lookup ? 5 : 0);
    const HostY yp(host_fe(q->y), N);
    auto put = [&](uint32_t term, int level) { hcst.y[term] = h_level(yp.p[N - 1 - term], level); };
    put(0, -3);
    put(1, -2);
    put(2, -3);
    for (uint32_t q = 1; q < sets; q++) put(2 + q, -2);
    for (uint32_t q = 0; q < sets; q++) {
      const uint32_t cols = std::min(c->chunk_len, c->n_perm - q * c->chunk_len);
      put(2 + sets + q, -2 - (int)cols);
    }
    if (rc_.has_lookup) {
      const uint32_t lb = 2 + 2 * sets;
      put(lb, -2);
      put(lb + 1, -3);
      put(lb + 2, -4);
      put(lb + 3, -2);
      put(lb + 4, -3);
    }
  }
  const uint32_t size = 1u << extended_k;
  H2_LAUNCH("k_evaluate_h_range", k_evaluate_h_range, ceil_div_u32(size, 256), 256, 0, s, rc_, extended_k, k, blinding_factors + 1, hcst,
            (const fe*)px.lo, (const fe*)px.hi, px.h, (fe*)d_h_out);
  return H2MI_OK;
}

int h2mi_plonk_evaluate_h_flex_dev(const h2mi_flex_cosets* c, const h2mi_quotient_scalars* q, void* d_h_out, h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (!c || !d_h_out) return H2MI_EINVAL;
  int rc = check_scalars(q);
  if (rc) return rc;
  const uint32_t k = q->k, extended_k = q->extended_k, blinding_factors = q->blinding_factors;
  if (c->n_gates == 0 || c->n_gates > H2MI_FLEX_MAX_GATES || c->n_perm > H2MI_FLEX_MAX_PERM || c->n_lookups > H2MI_FLEX_MAX_LOOKUPS) return H2MI_EINVAL;
  if (c->n_perm && (c->chunk_len == 0 || c->chunk_len > 3)) return H2MI_EINVAL;
  static_assert(sizeof(FlexCosets) + sizeof(FlexConsts) + 64 <= 4096, "the quotient kernel's arguments travel by value");
  FlexCosets fc;
  memset(&fc, 0, sizeof(fc));
  fc.n_gates = c->n_gates;
  for (uint32_t g = 0; g < c->n_gates; g++) {
    fc.gate_a[g] = (const fe*)c->gate_a[g]; fc.gate_q[g] = (const fe*)c->gate_q[g];
    if (!fc.gate_a[g] || !fc.gate_q[g]) return H2MI_EINVAL;
  }
  if (!fill_tail(fc, *c)) return H2MI_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  CallScope scope_;
  hipStream_t s = pick_stream(stream);
  PowTab px;
  rc = get_powtab(q->extended_omega, extended_k, s, &px);
  if (rc) return rc;
  const FlexConsts hc_ = flex_consts(*q);
  const uint32_t size = 1u << extended_k;
  H2_LAUNCH("k_evaluate_h_flex", k_evaluate_h_flex, ceil_div_u32(size, 256), 256, 0, s, fc, extended_k, k, blinding_factors + 1, hc_, (const fe*)px.lo,
            (const fe*)px.hi, px.h, (fe*)d_h_out);
  return H2MI_OK;
}

int h2mi_plonk_evaluate_h_expr_dev(const h2mi_quotient_circuits* qc, const h2mi_quotient_scalars* q, void* d_h_out, h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (!qc || !qc->circuits || !qc->gates || !d_h_out || qc->n_circuits != 1) return H2MI_EINVAL;
  int rc = check_scalars(q);
  if (rc) return rc;
  const uint32_t k = q->k, extended_k = q->extended_k, blinding_factors = q->blinding_factors;
  const h2mi_expr_cosets* c = qc->circuits;
  if (c->n_perm > H2MI_FLEX_MAX_PERM || (c->n_lookups & ~(uint32_t)H2MI_LOOKUPS_LOGUP) > H2MI_FLEX_MAX_LOOKUPS || (c->n_perm && c->chunk_len == 0)) return H2MI_EINVAL;
  const InstanceCols inst(qc->instances, c->instance);
  if (!inst.ok) return H2MI_EINVAL;
  ExprImage im;
  rc = im.build(qc->gates, qc->challenges, qc->n_challenges, c->advice, c->fixed, inst, k, extended_k);
  if (rc) return rc;
  static_assert(sizeof(FlexCosets) + sizeof(FlexConsts) + 96 <= 4096, "the quotient kernel's arguments travel by value");
  FlexCosets fc;
  memset(&fc, 0, sizeof(fc));
  if (!fill_tail(fc, *c) || !fill_shuffles(fc, qc->shuffles) || !fill_sets(fc, qc->logup)) return H2MI_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  CallScope scope_;
  hipStream_t s = pick_stream(stream);
  PowTab px;
  rc = get_powtab(q->extended_omega, extended_k, s, &px);
  if (rc) return rc;
  rc = ensure_tmp(im.image.size(), s);
  if (rc) return rc;
  fe* d_image = tmp_base();
  // pageable source: the copy has left `image` when the call returns
  H2_HIP(hipMemcpyAsync(d_image, im.image.data(), im.image.size() * sizeof(fe), hipMemcpyHostToDevice, s));
  const FlexConsts hc_ = flex_consts(*q);
  const uint32_t size = 1u << extended_k;
  H2_LAUNCH("k_evaluate_h_expr", k_evaluate_h_expr, ceil_div_u32(size, 256), 256, im.lds, s, fc, (const fe* const*)d_image, (const fe*)(d_image + im.cols_fe),
            (const uint2*)(d_image + im.cols_fe + im.const_fe), im.n_ops, extended_k, k, blinding_factors + 1, hc_, (const fe*)px.lo,
            (const fe*)px.hi, px.h, (fe*)d_h_out);
  return release_tmp(s);
}

// the batch call (slice < 0: every vector on the extended coset) and the by-coset call (every vector the 2^k points of coset `slice`)
static int evaluate_h_circuits(const h2mi_quotient_circuits* qc, const h2mi_quotient_scalars* q, int64_t slice, void* d_h_out, h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (!qc || !qc->circuits || !qc->gates || !d_h_out) return H2MI_EINVAL;
  const h2mi_expr_cosets* circuits = qc->circuits;
  const h2mi_shuffle_cosets* shuffles = qc->shuffles;
  const h2mi_instance_cosets* instances = qc->instances;
  const h2mi_gate_program* gates = qc->gates;
  const uint32_t n_circuits = qc->n_circuits, n_challenges = qc->n_challenges;
  if (n_circuits == 0 || n_circuits > H2MI_MAX_CIRCUITS || slice < H2MI_WHOLE_COSET) return H2MI_EINVAL;
  int rc = check_scalars(q);
  if (rc) return rc;
  const uint32_t k = q->k, extended_k = q->extended_k, blinding_factors = q->blinding_factors;
  if (slice >= (int64_t)1 << (extended_k - k)) return H2MI_ERANGE;
  const uint32_t dom_k = slice < 0 ? extended_k : k;  // the domain the vectors are given on
  const h2mi_expr_cosets& c0 = circuits[0];
  if (c0.n_perm > H2MI_FLEX_MAX_PERM || (c0.n_lookups & ~(uint32_t)H2MI_LOOKUPS_LOGUP) > H2MI_FLEX_MAX_LOOKUPS || (c0.n_perm && c0.chunk_len == 0)) return H2MI_EINVAL;
  // the program, its constants and the challenges once, as the single-circuit call lays them out (the image's own column table is
  // circuit 0's and is not read here); the circuits' records behind it
  const InstanceCols inst0(instances, c0.instance);
  if (!inst0.ok) return H2MI_EINVAL;
  ExprImage im;
  rc = im.build(gates, qc->challenges, n_challenges, c0.advice, c0.fixed, inst0, k, dom_k);
  if (rc) return rc;
  static_assert(sizeof(FlexCosets) + sizeof(FlexConsts) + 96 <= 4096, "the quotient kernel's arguments travel by value");
  static_assert(sizeof(CircuitCosets) % 8 == 0, "records are arrays of pointers");
  FlexCosets sh;
  memset(&sh, 0, sizeof(sh));
  if (!fill_tail(sh, c0) || !fill_shuffles(sh, shuffles) || !fill_sets(sh, qc->logup)) return H2MI_EINVAL;  // the counts are the key's: one struct for the batch
  const size_t rec_fe = (sizeof(CircuitCosets) + sizeof(fe) - 1) / sizeof(fe), prog_fe = im.image.size();
  im.image.resize(prog_fe + rec_fe * n_circuits);
  for (uint32_t i = 0; i < n_circuits; i++) {
    const h2mi_expr_cosets& c = circuits[i];
    if (c.n_perm != c0.n_perm || c.chunk_len != c0.chunk_len || c.n_lookups != c0.n_lookups) return H2MI_EINVAL;
    FlexCosets fc;
    memset(&fc, 0, sizeof(fc));
    if (!fill_tail(fc, c) || !fill_shuffles(fc, shuffles ? shuffles + i : nullptr) || fc.n_shuffles != sh.n_shuffles) return H2MI_EINVAL;
    // what the proof shares is read from entry 0: an entry that names other sigma or Lagrange cosets is a caller's mistake
    if (memcmp(fc.perm_sigma, sh.perm_sigma, sizeof(fc.perm_sigma)) || fc.l0 != sh.l0 || fc.l_last != sh.l_last || fc.l_active != sh.l_active) return H2MI_EINVAL;
    const InstanceCols inst(instances ? instances + i : nullptr, c.instance);
    if (!inst.ok) return H2MI_EINVAL;
    if (i) {  // every column the program reads is there (entry 0: im.build above)
      rc = expr_walk(gates, k, n_challenges, [&](uint32_t kind, uint32_t index, int32_t) {
        return kind == H2MI_EXPR_ADVICE ? index < H2MI_EXPR_MAX_ADVICE && c.advice[index]
             : kind == H2MI_EXPR_FIXED  ? index < H2MI_EXPR_MAX_FIXED && c.fixed[index]
                                        : inst.has(index);
      }, nullptr);
      if (rc) return rc;
    }
    CircuitCosets rec;
    memset(&rec, 0, sizeof(rec));
    for (uint32_t j = 0; j < H2MI_EXPR_MAX_ADVICE; j++) rec.cols[j] = (const fe*)c.advice[j];
    for (uint32_t j = 0; j < H2MI_EXPR_MAX_FIXED; j++) rec.cols[H2MI_EXPR_MAX_ADVICE + j] = (const fe*)c.fixed[j];
    for (uint32_t j = 0; j < H2MI_MAX_INSTANCE; j++) rec.cols[EX_INSTANCE + j] = (const fe*)inst.col[j];
    memcpy(rec.perm_value, fc.perm_value, sizeof(rec.perm_value));
    memcpy(rec.perm_z, fc.perm_z, sizeof(rec.perm_z));
    memcpy(rec.lk_in, fc.lk_in, sizeof(rec.lk_in));
    memcpy(rec.lk_in_b, fc.lk_in_b, sizeof(rec.lk_in_b));
    memcpy(rec.lk_table, fc.lk_table, sizeof(rec.lk_table));
    memcpy(rec.lk_pin, fc.lk_pin, sizeof(rec.lk_pin));
    memcpy(rec.lk_ptab, fc.lk_ptab, sizeof(rec.lk_ptab));
    memcpy(rec.lk_z, fc.lk_z, sizeof(rec.lk_z));
    memcpy(rec.sf_in, fc.sf_in, sizeof(rec.sf_in));
    memcpy(rec.sf_tab, fc.sf_tab, sizeof(rec.sf_tab));
    memcpy(rec.sf_z, fc.sf_z, sizeof(rec.sf_z));
    memcpy((char*)&im.image[prog_fe] + sizeof(CircuitCosets) * i, &rec, sizeof(rec));
  }
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  CallScope scope_;
  hipStream_t s = pick_stream(stream);
  FlexConsts hc_ = flex_consts(*q);
  // a slice: X = (zeta extended_omega^slice) omega^i with omega = extended_omega^rot, the generator of the 2^k rows
  fe x_base = host_fe(q->extended_omega);
  if (slice >= 0) {
    for (int64_t c = 0; c < slice; c++) hc_.zeta = h_mul256(hc_.zeta, x_base);
    for (uint32_t j = k; j < extended_k; j++) x_base = h_mul256(x_base, x_base);
  }
  uint64_t x_words[4];
  memcpy(x_words, x_base.v, 32);
  PowTab px;
  rc = get_powtab(x_words, dom_k, s, &px);
  if (rc) return rc;
  rc = ensure_tmp(im.image.size(), s);
  if (rc) return rc;
  fe* d_image = tmp_base();
  H2_HIP(hipMemcpyAsync(d_image, im.image.data(), im.image.size() * sizeof(fe), hipMemcpyHostToDevice, s));
  const uint32_t size = 1u << dom_k;
  if (slice < 0)
    H2_LAUNCH("k_evaluate_h_expr_batch", k_evaluate_h_expr_batch, ceil_div_u32(size, 256), 256, im.lds, s, sh, (const CircuitCosets*)(d_image + prog_fe),
              n_circuits, (const fe*)(d_image + im.cols_fe), (const uint2*)(d_image + im.cols_fe + im.const_fe), im.n_ops, extended_k, k,
              blinding_factors + 1, hc_, (const fe*)px.lo, (const fe*)px.hi, px.h, (fe*)d_h_out);
  else
    H2_LAUNCH("k_evaluate_h_expr_slice", k_evaluate_h_expr_slice, ceil_div_u32(size, 256), 256, im.lds, s, sh, (const CircuitCosets*)(d_image + prog_fe),
              n_circuits, (const fe*)(d_image + im.cols_fe), (const uint2*)(d_image + im.cols_fe + im.const_fe), im.n_ops, extended_k, k,
              (uint32_t)slice, blinding_factors + 1, hc_, (const fe*)px.lo, (const fe*)px.hi, px.h, (fe*)d_h_out);
  return release_tmp(s);
}

int h2mi_plonk_evaluate_h_expr_batch_dev(const h2mi_quotient_circuits* circuits, const h2mi_quotient_scalars* scalars, int32_t slice, void* d_h_out,
                                         h2mi_stream_t stream) {
  return evaluate_h_circuits(circuits, scalars, slice, d_h_out, stream);
}

int h2mi_plonk_expr_compress_dev(const h2mi_expr_columns* cols, uint32_t domain_k, const uint64_t theta[4], void* d_out, h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (!theta || !d_out) return H2MI_EINVAL;
  ColumnTables t;
  int rc = t.fill(cols, domain_k);
  if (rc) return rc;
  ExprImage im;
  rc = im.build(cols->program, cols->challenges, cols->n_challenges, t.adv, t.fix, t.inst, cols->k, domain_k);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  CallScope scope_;
  hipStream_t s = pick_stream(stream);
  rc = ensure_tmp(im.image.size(), s);
  if (rc) return rc;
  fe* d_image = tmp_base();
  H2_HIP(hipMemcpyAsync(d_image, im.image.data(), im.image.size() * sizeof(fe), hipMemcpyHostToDevice, s));
  const uint32_t size = 1u << domain_k;
  H2_LAUNCH("k_expr_compress", k_expr_compress, ceil_div_u32(size, 256), 256, im.lds, s, (const fe* const*)d_image, (const fe*)(d_image + im.cols_fe),
            (const uint2*)(d_image + im.cols_fe + im.const_fe), im.n_ops, domain_k, host_fe(theta), (fe*)d_out);
  return release_tmp(s);
}

int h2mi_plonk_expr_check_dev(const h2mi_expr_columns* cols, uint32_t n_rows, uint32_t* report_out, uint32_t* n_polys_out, h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (!report_out) return H2MI_EINVAL;
  ColumnTables t;
  int rc = t.fill(cols, cols ? cols->k : 0);
  if (rc) return rc;
  const h2mi_gate_program* polys = cols->program;
  const uint32_t k = cols->k;
  if (n_rows == 0 || n_rows > ((uint64_t)1 << k)) return H2MI_ERANGE;
  ExprImage im;
  rc = im.build(polys, cols->challenges, cols->n_challenges, t.adv, t.fix, t.inst, k, k);
  if (rc) return rc;
  uint32_t n_polys = 0;
  for (uint32_t i = 0; i < polys->n_ops; i++) n_polys += polys->ops[i].op == H2MI_EXPR_END;
  // the report travels behind the image, already {0, 0xffffffff} per polynomial: one copy on the stream sets both up
  const size_t image_fe = im.image.size(), report_fe = ((size_t)n_polys * 8 + 31) / 32;
  im.image.resize(image_fe + report_fe);
  uint32_t* init = (uint32_t*)(im.image.data() + image_fe);
  for (uint32_t j = 0; j < n_polys; j++) { init[2 * j] = 0; init[2 * j + 1] = 0xffffffffu; }
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  CallScope scope_;
  hipStream_t s = pick_stream(stream);
  rc = ensure_tmp(im.image.size(), s);
  if (rc) return rc;
  fe* d_image = tmp_base();
  H2_HIP(hipMemcpyAsync(d_image, im.image.data(), im.image.size() * sizeof(fe), hipMemcpyHostToDevice, s));
  H2_LAUNCH("k_expr_check", k_expr_check, ceil_div_u32(n_rows, 256), 256, im.lds, s, (const fe* const*)d_image, (const fe*)(d_image + im.cols_fe),
            (const uint2*)(d_image + im.cols_fe + im.const_fe), im.n_ops, k, n_rows, (uint32_t*)(d_image + image_fe));
  H2_HIP(hipMemcpyAsync(report_out, d_image + image_fe, (size_t)n_polys * 8, hipMemcpyDeviceToHost, s));
  H2_HIP(hipStreamSynchronize(s));
  if (n_polys_out) *n_polys_out = n_polys;
  return release_tmp(s);
}

int h2mi_plonk_copy_check_dev(const void* const* d_values, uint32_t m, const void* d_cells, uint32_t n_cells, uint32_t report_out[2], h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (!d_values || !report_out || m == 0 || m > H2MI_FLEX_MAX_PERM || (n_cells && !d_cells)) return H2MI_EINVAL;
  for (uint32_t j = 0; j < m; j++)
    if (!d_values[j]) return H2MI_EINVAL;
  report_out[0] = 0;
  report_out[1] = 0xffffffffu;
  if (!n_cells) return H2MI_OK;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  CallScope scope_;
  hipStream_t s = pick_stream(stream);
  // the column pointers and, behind them, the report: one copy
  constexpr size_t cols_fe = H2MI_FLEX_MAX_PERM * sizeof(void*) / 32;
  fe image[cols_fe + 1];
  memset(image, 0, sizeof(image));
  memcpy(image, d_values, m * sizeof(void*));
  ((uint32_t*)(image + cols_fe))[1] = 0xffffffffu;
  int rc = ensure_tmp(cols_fe + 1, s);
  if (rc) return rc;
  fe* d_image = tmp_base();
  H2_HIP(hipMemcpyAsync(d_image, image, sizeof(image), hipMemcpyHostToDevice, s));
  H2_LAUNCH("k_copy_check", k_copy_check, ceil_div_u32(n_cells, 256), 256, 0, s, (const fe* const*)d_image, (const uint4*)d_cells, n_cells,
            (uint32_t*)(d_image + cols_fe));
  H2_HIP(hipMemcpyAsync(report_out, d_image + cols_fe, 8, hipMemcpyDeviceToHost, s));
  H2_HIP(hipStreamSynchronize(s));
  return release_tmp(s);
}

int h2mi_plonk_evaluate_h_standard_dev(const h2mi_standard_plonk_cosets* c, const h2mi_quotient_scalars* q, void* d_h_out, h2mi_stream_t stream) {
  H2_REQUIRE_INIT();
  if (!c || !d_h_out) return H2MI_EINVAL;
  int rc = check_scalars(q);
  if (rc) return rc;
  const uint32_t k = q->k, extended_k = q->extended_k, blinding_factors = q->blinding_factors;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  CallScope scope_;
  hipStream_t s = pick_stream(stream);
  PlonkCosets pc;
  for (int i = 0; i < 3; i++) { pc.advice[i] = (const fe*)c->advice[i]; pc.sigma[i] = (const fe*)c->sigma[i]; pc.z[i] = (const fe*)c->z[i]; }
  for (int i = 0; i < 5; i++) pc.fixed[i] = (const fe*)c->fixed[i];
  pc.l0 = (const fe*)c->l0; pc.l_last = (const fe*)c->l_last; pc.l_active = (const fe*)c->l_active;
  for (int i = 0; i < 3; i++) if (!pc.advice[i] || !pc.sigma[i] || !pc.z[i]) return H2MI_EINVAL;
  for (int i = 0; i < 5; i++) if (!pc.fixed[i]) return H2MI_EINVAL;
  if (!pc.l0 || !pc.l_last || !pc.l_active) return H2MI_EINVAL;
  PowTab px;
  rc = get_powtab(q->extended_omega, extended_k, s, &px);
  if (rc) return rc;
  HConsts hcst;
  fill_common(hcst, *q, 3);
  {
    const HostY yp(host_fe(q->y), 8);  // eight terms: term i carries y^(7-i)
    hcst.y[0] = h_level(yp.p[7], -2);
    hcst.y[1] = h_level(yp.p[7], -3);
    hcst.y[2] = h_level(yp.p[7], -1);
    hcst.y[3] = h_level(yp.p[6], -2);  // term 1
    hcst.y[4] = h_level(yp.p[4], -2);  // term 3
    hcst.y[5] = h_level(yp.p[3], -2);  // term 4
    hcst.y[6] = h_level(yp.p[5], -3);  // term 2
    for (int m = 0; m < 3; m++) hcst.y[7 + m] = h_level(yp.p[2 - m], -3);  // terms 5, 6, 7
  }
  const uint32_t size = 1u << extended_k;
  H2_LAUNCH("k_evaluate_h_standard_plonk", k_evaluate_h_standard_plonk, ceil_div_u32(size, 256), 256, 0, s, pc, extended_k, k, blinding_factors + 1,
            hcst, (const fe*)px.lo, (const fe*)px.hi, px.h, (fe*)d_h_out);
  return H2MI_OK;
}

}  // extern "C"
