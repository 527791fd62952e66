// The ABI's BN254 G1 point layouts and their conversion to the arithmetic layer (g1_29.cuh: the group law, XYZZ coordinates on
// the 29-bit-limb field).
//
// Replaces (on the device) halo2curves::bn256::{G1Affine, G1} — reference call site src/scaffold.rs:14, SURVEY.md 8a row a7.
// Layouts at the C-ABI are the crate's:
//   G1Affine = {x, y} 64 B Montgomery-2^256, identity encoded as (0, 0)
//   G1       = {x, y, z} 96 B Jacobian Montgomery-2^256, identity z = 0
// Nothing here computes on a point: a kernel loads one of the two layouts, crosses the bridge below into xyzz29 (Montgomery-2^261,
// loosely reduced), runs xyzz29_madd / xyzz29_add / xyzz29_dbl, and crosses back to store.  Device only (the layouts are made of
// `fe`); g1_29.cuh stays free of `fe`, so the g++ harness compiles it.  (`affine` is also the container of the tables only kernels
// read, whose 8 words per coordinate are packed canonical Montgomery-2^261 limbs: f29_unpack / f29_pack, no bridge.)
#pragma once
#include "fp.cuh"
#include "g1_29.cuh"

namespace h2 {

using Fq = FqP;

struct affine {
  fe x, y;
};
struct jac {
  fe x, y, z;
};

__device__ __forceinline__ bool affine_is_identity(const affine& p) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) o |= p.x.v[i] | p.y.v[i];
  return o == 0;
}
__device__ __forceinline__ affine affine_load(const void* p) {
  affine a;
  a.x = fe_load(p);
  a.y = fe_load(reinterpret_cast<const char*>(p) + 32);
  return a;
}
__device__ __forceinline__ void affine_store(void* p, const affine& a) {
  fe_store(p, a.x);
  fe_store(reinterpret_cast<char*>(p) + 32, a.y);
}
__device__ __forceinline__ bool jac_is_identity(const jac& j) { return fe_is_zero(j.z); }
__device__ __forceinline__ void jac_store(void* p, const jac& j) {
  char* c = reinterpret_cast<char*>(p);
  fe_store(c, j.x); fe_store(c + 32, j.y); fe_store(c + 64, j.z);
}
__device__ __forceinline__ jac jac_load(const void* p) {
  const char* c = reinterpret_cast<const char*>(p);
  jac j;
  j.x = fe_load(c); j.y = fe_load(c + 32); j.z = fe_load(c + 64);
  return j;
}

// ---- the bridge: Montgomery-2^256 words in memory <-> xyzz29 ---------------------------------------------------------------
// One coordinate in: any 8 words (< 2^256 = 5.3p) -> f29_from_mont256 < 1 + eps * 5.3 = 1.04 -> canonical (< 1), normalized.
__device__ __forceinline__ f29 coord_from_mont256(const fe& a) { return f29_reduce_canonical<Fq29>(f29_from_mont256<Fq29>(a.v)); }

// affine256 -> (x, y): canonical Montgomery-2^261, what xyzz29_madd / xyzz29_dbl_affine take as a table point.  The identity
// (0, 0) maps to (0, 0); xyzz29_madd's caller skips it.
__device__ __forceinline__ void affine_to_f29(const affine& a, f29& x, f29& y) {
  x = coord_from_mont256(a.x);
  y = coord_from_mont256(a.y);
}
// affine256 -> XYZZ with ZZ = ZZZ = 1; (0, 0) -> identity.  Out: every coordinate canonical.
__device__ __forceinline__ xyzz29 xyzz29_from_affine(const affine& a) {
  if (affine_is_identity(a)) return xyzz29_identity();
  xyzz29 r;
  affine_to_f29(a, r.x, r.y);
  r.zz = f29_const<Fq29>(Fq29::ONE);
  r.zzz = f29_const<Fq29>(Fq29::ONE);
  return r;
}
// Jacobian256 -> XYZZ; Z = 0 -> identity.  X, Y, Z canonical going in, so out: X, Y < 1, ZZ, ZZZ < 1.006 (xyzz29_from_jacobian) —
// inside the xyzz29_add / xyzz29_dbl invariant X < 6, Y < 4, ZZ, ZZZ < 1.5.
__device__ __forceinline__ xyzz29 xyzz29_from_jac(const jac& j) {
  if (jac_is_identity(j)) return xyzz29_identity();
  return xyzz29_from_jacobian(coord_from_mont256(j.x), coord_from_mont256(j.y), coord_from_mont256(j.z));
}
// XYZZ (the xyzz29_dbl invariant) -> Jacobian256, canonical words: (X * ZZ, Y * ZZZ, ZZ) — no inversion; `canonical`: the
// representative with Z = 1 (one inversion; h2mi_msm_set_canonical).  Identity -> (0, R, 0), the crate's G1::identity() = (0, 1, 0).
// f29_to_mont256 takes normalized values < ~100p: xyzz29_to_jacobian's are < 1.5, xyzz29_to_affine's canonical.
__device__ __forceinline__ jac jac_from_xyzz29(const xyzz29& p, bool canonical = false) {
  jac j;
  if (xyzz29_is_identity(p)) {
    j.x = fe_zero(); j.y = fe_one<Fq>(); j.z = fe_zero();
    return j;
  }
  if (canonical) {
    f29 x, y;
    xyzz29_to_affine(p, x, y);
    f29_to_mont256<Fq29>(x, j.x.v);
    f29_to_mont256<Fq29>(y, j.y.v);
    j.z = fe_one<Fq>();
  } else {
    f29 x, y, z;
    xyzz29_to_jacobian(p, x, y, z);
    f29_to_mont256<Fq29>(x, j.x.v);
    f29_to_mont256<Fq29>(y, j.y.v);
    f29_to_mont256<Fq29>(z, j.z.v);
  }
  return j;
}
// XYZZ -> affine256, canonical words (one inversion); identity -> (0, 0), which is what xyzz29_to_affine returns for it and
// what f29_to_mont256 maps to zero words.
__device__ __forceinline__ affine affine_from_xyzz29(const xyzz29& p) {
  f29 x, y;
  xyzz29_to_affine(p, x, y);
  affine a;
  f29_to_mont256<Fq29>(x, a.x.v);
  f29_to_mont256<Fq29>(y, a.y.v);
  return a;
}

}  // namespace h2
