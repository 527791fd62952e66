// libh2mi_hooks.so = the product's objects + this file: elementwise device arithmetic exposed for the parity tests
// (tests/test_gpu_parity.py: every field operation, the XYZZ point formulas and the lane-cooperative quad operations against the
// oracle; tests/test_gpu_wire.py: the field operations of fp.cuh (h2mi_dbg_field_op) on Montgomery words at the limb extremes;
// tests/test_gpu_f29.py: the 29-bit-limb primitives f29_mul / sqr / mul2 / mul3 / reduce_loose / inv and the xyzz29 chains on
// chosen limbs, at the limits of their contracts; tests/test_gpu_g1_29_edges.py: the point operations on raw-limb operands at the bounds of their coordinate invariants).  NOT part of the product: libh2mi.so neither contains nor exports these (round-4 VERDICT: debug hooks shipped in the
// product library).  The kernels below instantiate the same device functions the product's kernels inline: fp.cuh for the field
// hooks, and for every point hook the one group law (g1_29.cuh, g1_29_quad.cuh) through the format bridge of g1.cuh — what the MSM
// runs (the f29 hooks through csrc/f29_testops.cuh, the bodies the g++ harness tests/host/f29_host.cpp also compiles); the hooks library carries its own copy of the library state and is initialised separately (h2mi_init).
#include "g1.cuh"
#include "f29_testops.cuh"
#include "g1_29_quad.cuh"
#include "h2mi_hooks.h"
#include "h2mi_internal.h"

namespace h2 {

// ---- elementwise field kernels (test hooks) -------------------------------------------------------
template <class F>
__global__ void __launch_bounds__(256) k_dbg_field(int op, const fe* a, const fe* b, fe* out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe x = fe_load(&a[i]);
  fe y = b ? fe_load(&b[i]) : fe_zero();
  fe r;
  switch (op) {
    case 0: r = fe_mul<F>(x, y); break;
    case 1: r = fe_add<F>(x, y); break;
    case 2: r = fe_sub<F>(x, y); break;
    case 3: r = fe_sqr<F>(x); break;
    case 5: r = fe_from_mont<F>(x); break;
    case 6: r = fe_to_mont<F>(x); break;
    case 7: r = fe_neg<F>(x); break;
    case 9: r = fe_inv_ds<F>(x); break;
    case 10: r = fe_inv_gcd<F>(x); break;
    default: r = fe_dbl<F>(x); break;
  }
  fe_store(&out[i], r);
}

// affine Mont256 -> XYZZ with ZZ != 1, a non-trivial representative: (2P) + (-P)
__device__ __forceinline__ xyzz29 dbg_lift(const uint8_t* src) {
  const affine a = affine_load(src);
  if (affine_is_identity(a)) return xyzz29_identity();
  f29 x, y;
  affine_to_f29(a, x, y);
  xyzz29 r = xyzz29_dbl_affine(x, y);
  xyzz29_madd(r, x, f29_sub(f29_zero(), y, Fq29::K2));
  return r;
}

// op 0: P + Q by the mixed addition (xyzz29_madd); op 1: 2 P (xyzz29_dbl); op 2: P + Q by the full addition (xyzz29_add), Q lifted
__global__ void __launch_bounds__(256) k_dbg_g1(int op, const uint8_t* p, const uint8_t* q, uint8_t* out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  xyzz29 acc = xyzz29_from_affine(affine_load(p + i * 64));
  if (op == 0) {
    const affine Q = affine_load(q + i * 64);
    if (!affine_is_identity(Q)) {  // as every caller of xyzz29_madd does
      f29 x, y;
      affine_to_f29(Q, x, y);
      xyzz29_madd(acc, x, y);
    }
  } else if (op == 1) {
    acc = xyzz29_dbl(acc);
  } else {
    xyzz29_add(acc, dbg_lift(q + i * 64));
  }
  jac_store(out + i * 96, jac_from_xyzz29(acc));
}

// debug hook for the lane-cooperative point operations (g1_29_quad.cuh): four lanes per element.
// op 0: (P) + (Q) with both operands brought to non-trivial XYZZ representatives; op 1: 2 (P).
__global__ void __launch_bounds__(256) k_dbg_quad(int op, const uint8_t* pp, const uint8_t* qq, uint8_t* out, size_t n) {
  const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  if (i >= n) return;  // n is padded by the host so that whole quads share the decision
  xyzz29 a = dbg_lift(pp + i * 64);
  xyzz29 r = op == 0 ? xyzz29_add_quad(a, dbg_lift(qq + i * 64)) : xyzz29_dbl_quad(a);
  if ((threadIdx.x & 3u) != (uint32_t)(i & 3u)) return;  // one lane of the quad writes (a different one per element)
  jac_store(out + i * 96, jac_from_xyzz29(r));
}

// ---- the 29-bit-limb layer on chosen limbs (test hooks; bodies in f29_testops.cuh) ----------------------------------
// One thread per element, operands read from global memory.  These run the device form of f29_mac_first (v_mad_u64_u32
// inline asm), which the g++ harness cannot.
template <class F>
__global__ void __launch_bounds__(256) k_dbg_f29_mul(int mode, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  f29t_mul_one<F>(mode, a + 8 * i, b + 8 * i, out + 8 * i);
}
template <class F>
__global__ void __launch_bounds__(256) k_dbg_f29_raw(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // operands an op does not take are null and never read
  f29t_raw_one<F>(op, a + 9 * i, b ? b + 9 * i : nullptr, c ? c + 9 * i : nullptr, d ? d + 9 * i : nullptr, out + 9 * i);
}
template <class F>
__global__ void __launch_bounds__(256) k_dbg_f29_mul3(const uint32_t* ops, uint32_t* out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  f29t_mul3_one<F>(ops, n, i, out + 9 * i);
}
// one thread runs one chain: points offsets[c] .. offsets[c + 1] of the shared list
__global__ void __launch_bounds__(64) k_dbg_g1_29_chains(const uint32_t* pts, const uint8_t* signs, const uint64_t* offsets, size_t nchains, uint32_t* out, int tree) {
  size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nchains) return;
  const uint64_t lo = offsets[c], hi = offsets[c + 1];
  f29t_chain_one(pts + 16 * lo, signs + lo, (size_t)(hi - lo), out + 32 * c, tree);
}

// one point operation per thread on raw 9-limb coordinates: 36 words per element in a, b and out (f29t_point_raw_one, ops 0..5)
__global__ void __launch_bounds__(256) k_dbg_g1_29_raw(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  f29t_point_raw_one(op, a + 36 * i, b + 36 * i, out + 36 * i);
}
// the lane-cooperative forms on the same raw operands, four lanes per element: op 6 = xyzz29_add_quad(a, b), 7 = xyzz29_dbl_quad(a);
// same output layout as ops 2 / 1
__global__ void __launch_bounds__(256) k_dbg_g1_29_raw_quad(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  if (i >= n) return;  // n is padded by the host so that whole quads share the decision
  const xyzz29 p = f29t_load_xyzz(a + 36 * i);
  const xyzz29 r = op == 6 ? xyzz29_add_quad(p, f29t_load_xyzz(b + 36 * i)) : xyzz29_dbl_quad(p);
  if ((threadIdx.x & 3u) != (uint32_t)(i & 3u)) return;  // one lane of the quad writes (a different one per element)
  f29t_store_xyzz(r, out + 36 * i);
}

}  // namespace h2

using namespace h2;

// nops operands of `words` 32-bit words per element (null ones skipped) -> one output of `owords` words per element
template <class Launch>
static int f29_dbg_run(const uint32_t* const* ops, int nops, size_t words, size_t owords, uint32_t* out, size_t n, Launch launch) {
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  hipStream_t s = ctx().stream;
  DevMem d[4], dout;
  for (int q = 0; q < nops; q++) {
    if (!ops[q]) continue;
    H2_HIP(d[q].alloc(n * words * 4));
    H2_HIP(hipMemcpyAsync(d[q].p, ops[q], n * words * 4, hipMemcpyHostToDevice, s));
  }
  H2_HIP(dout.alloc(n * owords * 4));
  int rc = launch(s, d, dout.as<uint32_t>());
  if (rc) return rc;
  H2_HIP(hipMemcpyAsync(out, dout.p, n * owords * 4, hipMemcpyDeviceToHost, s));
  H2_HIP(hipStreamSynchronize(s));
  return H2MI_OK;
}

static int f29_dbg_raw(int field, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out, size_t n) {
  const uint32_t* ops[4] = {a, b, c, d};
  return f29_dbg_run(ops, 4, 9, 9, out, n, [&](hipStream_t s, DevMem* m, uint32_t* dout) {
    const uint32_t grid = ceil_div_u32(n, 256);
    if (field == 0) {
      H2_LAUNCH("k_dbg_f29_raw_fq", k_dbg_f29_raw<Fq29>, grid, 256, 0, s, op, m[0].as<uint32_t>(), m[1].as<uint32_t>(), m[2].as<uint32_t>(), m[3].as<uint32_t>(), dout, n);
    } else {
      H2_LAUNCH("k_dbg_f29_raw_fr", k_dbg_f29_raw<Fr29>, grid, 256, 0, s, op, m[0].as<uint32_t>(), m[1].as<uint32_t>(), m[2].as<uint32_t>(), m[3].as<uint32_t>(), dout, n);
    }
    return (int)H2MI_OK;
  });
}

extern "C" {

int h2mi_dbg_field_op(int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  H2_REQUIRE_INIT();
  if (!a || !out || n == 0 || op < 0 || op > 10 || op == 4) return H2MI_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  hipStream_t s = ctx().stream;
  DevMem da, db, dout;
  H2_HIP(da.alloc(n * 32));
  H2_HIP(dout.alloc(n * 32));
  H2_HIP(hipMemcpyAsync(da.p, a, n * 32, hipMemcpyHostToDevice, s));
  if (b) {
    H2_HIP(db.alloc(n * 32));
    H2_HIP(hipMemcpyAsync(db.p, b, n * 32, hipMemcpyHostToDevice, s));
  }
  uint32_t grid = ceil_div_u32(n, 256);
  if (field == 0) {
    H2_LAUNCH("k_dbg_field_fq", k_dbg_field<FqP>, grid, 256, 0, s, op, da.as<fe>(), db.as<fe>(), dout.as<fe>(), n);
  } else {
    H2_LAUNCH("k_dbg_field_fr", k_dbg_field<FrP>, grid, 256, 0, s, op, da.as<fe>(), db.as<fe>(), dout.as<fe>(), n);
  }
  H2_HIP(hipMemcpyAsync(out, dout.p, n * 32, hipMemcpyDeviceToHost, s));
  H2_HIP(hipStreamSynchronize(s));
  return H2MI_OK;
}


int h2mi_dbg_g1_op(int op, const uint64_t* p, const uint64_t* q, uint64_t* out_jac, size_t n) {
  H2_REQUIRE_INIT();
  if (!p || !out_jac || n == 0 || (op != 1 && !q)) return H2MI_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  hipStream_t s = ctx().stream;
  DevMem dp, dq, dout;
  H2_HIP(dp.alloc(n * 64));
  H2_HIP(dout.alloc(n * 96));
  H2_HIP(hipMemcpyAsync(dp.p, p, n * 64, hipMemcpyHostToDevice, s));
  if (q) {
    H2_HIP(dq.alloc(n * 64));
    H2_HIP(hipMemcpyAsync(dq.p, q, n * 64, hipMemcpyHostToDevice, s));
  }
  H2_LAUNCH("k_dbg_g1", k_dbg_g1, ceil_div_u32(n, 256), 256, 0, s, op, dp.as<uint8_t>(), dq.as<uint8_t>(), dout.as<uint8_t>(), n);
  H2_HIP(hipMemcpyAsync(out_jac, dout.p, n * 96, hipMemcpyDeviceToHost, s));
  H2_HIP(hipStreamSynchronize(s));
  return H2MI_OK;
}


int h2mi_dbg_g1_quad_op(int op, const uint64_t* p, const uint64_t* q, uint64_t* out_jac, size_t n) {
  H2_REQUIRE_INIT();
  if (!p || !out_jac || n == 0 || (op != 0 && op != 1) || (op == 0 && !q)) return H2MI_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  hipStream_t s = ctx().stream;
  DevMem dp, dq, dout;
  H2_HIP(dp.alloc(n * 64));
  H2_HIP(dout.alloc(n * 96));
  H2_HIP(hipMemcpyAsync(dp.p, p, n * 64, hipMemcpyHostToDevice, s));
  if (q) {
    H2_HIP(dq.alloc(n * 64));
    H2_HIP(hipMemcpyAsync(dq.p, q, n * 64, hipMemcpyHostToDevice, s));
  }
  H2_LAUNCH("k_dbg_quad", k_dbg_quad, ceil_div_u32(n * 4, 256), 256, 0, s, op, dp.as<uint8_t>(), dq.as<uint8_t>(), dout.as<uint8_t>(), n);
  H2_HIP(hipMemcpyAsync(out_jac, dout.p, n * 96, hipMemcpyDeviceToHost, s));
  H2_HIP(hipStreamSynchronize(s));
  return H2MI_OK;
}

int h2mi_dbg_f29_mul(int field, int mode, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  H2_REQUIRE_INIT();
  if (!a || !b || !out || n == 0 || (field != 0 && field != 1) || mode < 0 || mode > 5) return H2MI_EINVAL;
  const uint32_t* ops[2] = {a, b};
  return f29_dbg_run(ops, 2, 8, 8, out, n, [&](hipStream_t s, DevMem* m, uint32_t* dout) {
    const uint32_t grid = ceil_div_u32(n, 256);
    if (field == 0) {
      H2_LAUNCH("k_dbg_f29_mul_fq", k_dbg_f29_mul<Fq29>, grid, 256, 0, s, mode, m[0].as<uint32_t>(), m[1].as<uint32_t>(), dout, n);
    } else {
      H2_LAUNCH("k_dbg_f29_mul_fr", k_dbg_f29_mul<Fr29>, grid, 256, 0, s, mode, m[0].as<uint32_t>(), m[1].as<uint32_t>(), dout, n);
    }
    return (int)H2MI_OK;
  });
}

int h2mi_dbg_f29_reduce_loose(int field, const uint32_t* in9, uint32_t* out9, size_t n) {
  H2_REQUIRE_INIT();
  if (!in9 || !out9 || n == 0 || (field != 0 && field != 1)) return H2MI_EINVAL;
  return f29_dbg_raw(field, 0, in9, nullptr, nullptr, nullptr, out9, n);
}
int h2mi_dbg_f29_mul_raw(int field, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  H2_REQUIRE_INIT();
  if (!a || !b || !out || n == 0 || (field != 0 && field != 1)) return H2MI_EINVAL;
  return f29_dbg_raw(field, 1, a, b, nullptr, nullptr, out, n);
}
int h2mi_dbg_f29_sqr_raw(int field, const uint32_t* a, uint32_t* out, size_t n) {
  H2_REQUIRE_INIT();
  if (!a || !out || n == 0 || (field != 0 && field != 1)) return H2MI_EINVAL;
  return f29_dbg_raw(field, 2, a, nullptr, nullptr, nullptr, out, n);
}
int h2mi_dbg_f29_mul2_raw(int field, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out, size_t n) {
  H2_REQUIRE_INIT();
  if (!a || !b || !c || !d || !out || n == 0 || (field != 0 && field != 1)) return H2MI_EINVAL;
  return f29_dbg_raw(field, 3, a, b, c, d, out, n);
}
int h2mi_dbg_f29_mul3_raw(int field, const uint32_t* ops, uint32_t* out, size_t n) {
  H2_REQUIRE_INIT();
  if (!ops || !out || n == 0 || (field != 0 && field != 1)) return H2MI_EINVAL;
  const uint32_t* one[1] = {ops};
  return f29_dbg_run(one, 1, 6 * 9, 9, out, n, [&](hipStream_t s, DevMem* m, uint32_t* dout) {
    const uint32_t grid = ceil_div_u32(n, 256);
    if (field == 0) {
      H2_LAUNCH("k_dbg_f29_mul3_fq", k_dbg_f29_mul3<Fq29>, grid, 256, 0, s, m[0].as<uint32_t>(), dout, n);
    } else {
      H2_LAUNCH("k_dbg_f29_mul3_fr", k_dbg_f29_mul3<Fr29>, grid, 256, 0, s, m[0].as<uint32_t>(), dout, n);
    }
    return (int)H2MI_OK;
  });
}

int h2mi_dbg_g1_29_raw_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  H2_REQUIRE_INIT();
  if (!a || !b || !out || n == 0 || op < 0 || op > 7) return H2MI_EINVAL;
  const uint32_t* ops[2] = {a, b};
  return f29_dbg_run(ops, 2, 36, 36, out, n, [&](hipStream_t s, DevMem* m, uint32_t* dout) {
    if (op < 6) {
      H2_LAUNCH("k_dbg_g1_29_raw", k_dbg_g1_29_raw, ceil_div_u32(n, 256), 256, 0, s, op, m[0].as<uint32_t>(), m[1].as<uint32_t>(), dout, n);
    } else {
      H2_LAUNCH("k_dbg_g1_29_raw_quad", k_dbg_g1_29_raw_quad, ceil_div_u32(n * 4, 256), 256, 0, s, op, m[0].as<uint32_t>(), m[1].as<uint32_t>(), dout, n);
    }
    return (int)H2MI_OK;
  });
}

int h2mi_dbg_g1_29_chains(const uint32_t* pts, const uint8_t* signs, const uint64_t* offsets, size_t nchains, uint32_t* out_xyzz, int tree) {
  H2_REQUIRE_INIT();
  if (!pts || !signs || !offsets || !out_xyzz || nchains == 0) return H2MI_EINVAL;
  if (tree != 0 && tree != 2 && tree != 4 && tree != 8 && tree != 16) return H2MI_EINVAL;
  if (offsets[0] != 0) return H2MI_EINVAL;
  for (size_t c = 0; c < nchains; c++)
    if (offsets[c + 1] < offsets[c]) return H2MI_EINVAL;
  const size_t npts = offsets[nchains];
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  hipStream_t s = ctx().stream;
  DevMem dp, ds, doff, dout;
  H2_HIP(dp.alloc(npts * 64));
  H2_HIP(ds.alloc(npts));
  H2_HIP(doff.alloc((nchains + 1) * 8));
  H2_HIP(dout.alloc(nchains * 128));
  H2_HIP(hipMemcpyAsync(dp.p, pts, npts * 64, hipMemcpyHostToDevice, s));
  H2_HIP(hipMemcpyAsync(ds.p, signs, npts, hipMemcpyHostToDevice, s));
  H2_HIP(hipMemcpyAsync(doff.p, offsets, (nchains + 1) * 8, hipMemcpyHostToDevice, s));
  H2_LAUNCH("k_dbg_g1_29_chains", k_dbg_g1_29_chains, ceil_div_u32(nchains, 64), 64, 0, s, dp.as<uint32_t>(), ds.as<uint8_t>(), doff.as<uint64_t>(), nchains,
            dout.as<uint32_t>(), tree);
  H2_HIP(hipMemcpyAsync(out_xyzz, dout.p, nchains * 128, hipMemcpyDeviceToHost, s));
  H2_HIP(hipStreamSynchronize(s));
  return H2MI_OK;
}

// The workspace of one of a handle's recent general-pipeline MSMs (h2::msm_debug_snapshot) copied to the host; the handle is one
// registered with THIS library instance.  Layout: h2mi_hooks.h.
int h2mi_dbg_msm_snapshot(uint64_t handle, int back, uint64_t geometry[16], uint32_t* data, size_t cap_words, size_t* need_words) {
  H2_REQUIRE_INIT();
  if (!geometry || (!data && !need_words)) return H2MI_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  MsmSnapshot m;
  if (int rc = msm_debug_snapshot(handle, back, &m)) return rc;
  if (m.last_small) return H2MI_EINVAL;  // the handle's last MSM took the small path: its slot holds no bucket tables to read
  uint32_t entries = 0;
  H2_HIP(hipMemcpy(&entries, m.off + m.nb, 4, hipMemcpyDeviceToHost));
  if (entries > m.vals_cap) return H2MI_ERANGE;
  const uint64_t g[16] = {m.c, m.W, m.nb, m.lb, m.nbins, m.logNl, m.logNh, m.seg_log, m.n, m.stride, m.rows, m.has_sum, entries, m.slot, m.last_small, m.nseg};
  memcpy(geometry, g, sizeof g);
  constexpr size_t PART_WORDS = 36;
  const size_t tab = (size_t)m.nb + 1;
  const struct { const void* src; size_t words; } parts[] = {
      {m.s0_dev, 1}, {m.off, tab}, {m.np[0], tab}, {m.np[1], tab}, {m.toff[0], tab}, {m.toff[1], tab}, {m.vals1, entries}, {m.shift, 8},
      {m.dense, (size_t)m.nb * PART_WORDS}, {m.dense2, (size_t)m.nseg * PART_WORDS}, {m.vsum, (size_t)m.nseg * PART_WORDS}};
  size_t need = 0;
  for (const auto& p : parts) need += p.words;
  if (need_words) *need_words = need;
  if (!data) return H2MI_OK;
  if (cap_words < need) return H2MI_ERANGE;
  size_t at = 0;
  for (const auto& p : parts) {
    if (p.words) H2_HIP(hipMemcpy(data + at, p.src, p.words * 4, hipMemcpyDeviceToHost));
    at += p.words;
  }
  return H2MI_OK;
}

// What a small-path MSM left in its workspace slot (h2::msm_debug_small_snapshot) copied to the host.  Layout: h2mi_hooks.h.
int h2mi_dbg_msm_small_snapshot(uint64_t handle, int back, uint64_t geometry[16], uint8_t* data, size_t cap_bytes, size_t* need_bytes) {
  H2_REQUIRE_INIT();
  if (!geometry || (!data && !need_bytes)) return H2MI_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  MsmSmallSnapshot m;
  if (int rc = msm_debug_small_snapshot(handle, back, &m)) return rc;
  if (m.G > m.sG || m.small_n > m.n_reg) return H2MI_ERANGE;
  const uint64_t g[16] = {m.sc, m.sW, m.slanes, m.sr, m.sG, m.n_reg, m.small_n, m.G, m.slot};
  memcpy(geometry, g, sizeof g);
  constexpr size_t PART = 144;
  const struct { const void* src; size_t bytes; } parts[] = {
      {m.scnt, ((size_t)m.sG + 1) * 4}, {m.spart, (size_t)m.G * PART}, {m.sdig, (size_t)m.sW * m.n_reg}};
  size_t need = 0;
  for (const auto& p : parts) need += p.bytes;
  if (need_bytes) *need_bytes = need;
  if (!data) return H2MI_OK;
  if (cap_bytes < need) return H2MI_ERANGE;
  size_t at = 0;
  for (const auto& p : parts) {
    if (p.bytes) H2_HIP(hipMemcpy(data + at, p.src, p.bytes, hipMemcpyDeviceToHost));
    at += p.bytes;
  }
  return H2MI_OK;
}

// Chosen entries of the handle's digit-multiples table: entry ((j - 1) W + w) n_reg + i is j 2^(c w) P_i.
int h2mi_dbg_msm_small_table(uint64_t handle, const uint64_t* entries, size_t count, uint32_t* out) {
  H2_REQUIRE_INIT();
  if (!entries || !out) return H2MI_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx().mu);
  MsmSmallSnapshot m;
  if (int rc = msm_debug_small_snapshot(handle, 0, &m)) return rc;
  const uint64_t total = ((uint64_t)1 << (m.sc - 1)) * m.sW * m.n_reg;
  for (size_t k = 0; k < count; k++)
    if (entries[k] >= total) return H2MI_ERANGE;
  for (size_t k = 0; k < count; k++) H2_HIP(hipMemcpy(out + 16 * k, m.stable + entries[k] * 64, 64, hipMemcpyDeviceToHost));
  return H2MI_OK;
}

}  // extern "C"
