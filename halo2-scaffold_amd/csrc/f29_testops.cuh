// Per-element bodies of the f29 / g1_29 test entry points, written once and compiled twice: by g++ into the host harness
// (tests/host/f29_host.cpp, f29t_*) and by hipcc into the device hooks (h2mi_hooks.hip, h2mi_dbg_f29_*), so that both drive
// the same sequence of Fq29 / Fr29 calls on the same element layout.  Test infrastructure only: nothing in libh2mi.so's
// kernels includes this file.
#pragma once
#include <stddef.h>

#include "g1_29.cuh"

namespace h2 {

// one element of f29t_mul / h2mi_dbg_f29_mul: a, b, out are 8-word Mont256 values
template <class F>
H2_HD void f29t_mul_one(int mode, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  if (mode == 0) {  // Mont256 x Mont256 -> Mont256 through the internal Mont261 domain
    f29 x = f29_from_mont256<F>(a), y = f29_from_mont256<F>(b);
    f29_to_mont256<F>(f29_mul<F>(x, y), out);
  } else if (mode == 1) {  // NTT butterfly style: data stays Mont256, twiddle is Mont261
    f29 d = f29_unpack(a), w = f29_from_mont256<F>(b);
    f29 r = f29_reduce_canonical<F>(f29_mul<F>(d, w));
    f29_pack(r, out);
  } else if (mode == 2) {  // lazy chain: (a + b) * (a - b + 2p) with un-normalized first operand
    f29 x = f29_from_mont256<F>(a), y = f29_from_mont256<F>(b);
    f29 s = f29_normalize(f29_add(x, y));
    f29 d = f29_sub(x, y, F::K2);
    f29_to_mont256<F>(f29_mul<F>(d, s), out);
  } else if (mode == 4) {  // dedicated squaring of a normalized input
    f29 x = f29_from_mont256<F>(a);
    f29_to_mont256<F>(f29_sqr<F>(x), out);
  } else if (mode == 5) {  // Fermat inversion
    f29 x = f29_from_mont256<F>(a);
    f29_to_mont256<F>(f29_inv<F>(x), out);
  } else {  // pack(unpack(x)) round trip
    f29 x = f29_unpack(a);
    f29_pack(x, out);
  }
}

H2_HD f29 f29t_load9(const uint32_t* p) {
  f29 x;
  for (int k = 0; k < 9; k++) x.v[k] = p[k];
  return x;
}
H2_HD void f29t_store9(const f29& x, uint32_t* p) {
  for (int k = 0; k < 9; k++) p[k] = x.v[k];
}

// raw 9-limb operands, 9 words per element in and out.  op 0: f29_reduce_loose(a) (normalized, value < 64p);
// 1: f29_mul(a, b) (limbs(a) < 1.9 * 2^30, b normalized); 2: f29_sqr(a) (a normalized); 3: f29_mul2(a, b, c, d)
template <class F>
H2_HD void f29t_raw_one(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out) {
  f29 r;
  if (op == 0) r = f29_reduce_loose<F>(f29t_load9(a));
  else if (op == 1) r = f29_mul<F>(f29t_load9(a), f29t_load9(b));
  else if (op == 2) r = f29_sqr<F>(f29t_load9(a));
  else r = f29_mul2<F>(f29t_load9(a), f29t_load9(b), f29t_load9(c), f29t_load9(d));
  f29t_store9(r, out);
}
// f29_mul3 on element i of ops[6][n][9]: out = (a*b + c*d + e*f) / 2^261
template <class F>
H2_HD void f29t_mul3_one(const uint32_t* ops, size_t n, size_t i, uint32_t* out) {
  f29 x[6];
  for (int q = 0; q < 6; q++) x[q] = f29t_load9(ops + ((size_t)q * n + i) * 9);
  f29t_store9(f29_mul3<F>(x[0], x[1], x[2], x[3], x[4], x[5]), out);
}

H2_HD xyzz29 f29t_load_xyzz(const uint32_t* p) {
  xyzz29 r;
  r.x = f29t_load9(p); r.y = f29t_load9(p + 9); r.zz = f29t_load9(p + 18); r.zzz = f29t_load9(p + 27);
  return r;
}
H2_HD void f29t_store_xyzz(const xyzz29& r, uint32_t* p) {
  f29t_store9(r.x, p); f29t_store9(r.y, p + 9); f29t_store9(r.zz, p + 18); f29t_store9(r.zzz, p + 27);
}

// one point operation of g1_29.cuh on RAW operands: 9 limbs per coordinate, loaded exactly as given (no reduction, no
// canonicalisation), so a test can put every coordinate at the bounds the header states.  a, b: 36 words per element each (an XYZZ
// point fills them; an affine (x, y) the first 18, a Jacobian (X, Y, Z) the first 27), out: 36 words.
//   0: xyzz29_madd(acc = a, x2 = b[0..9), y2 = b[9..18))        1: xyzz29_dbl(a)        2: xyzz29_add(a, b)
//   3: xyzz29_dbl_affine(x = b[0..9), y_any = b[9..18))
//   4: xyzz29_from_jacobian(a) then xyzz29_to_jacobian of it: out = ZZ, ZZZ of the first, then X, Y of the second (X, Y and Z of
//      the pair are copies of inputs / of ZZ); the identity gives all zeros
//   5: xyzz29_to_affine(a): x, y in the first 18 words, the rest zero
H2_HD void f29t_point_raw_one(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  for (int k = 0; k < 36; k++) out[k] = 0;
  if (op == 0) {
    xyzz29 acc = f29t_load_xyzz(a);
    xyzz29_madd(acc, f29t_load9(b), f29t_load9(b + 9));
    f29t_store_xyzz(acc, out);
  } else if (op == 1) {
    f29t_store_xyzz(xyzz29_dbl(f29t_load_xyzz(a)), out);
  } else if (op == 2) {
    xyzz29 acc = f29t_load_xyzz(a);
    xyzz29_add(acc, f29t_load_xyzz(b));
    f29t_store_xyzz(acc, out);
  } else if (op == 3) {
    f29t_store_xyzz(xyzz29_dbl_affine(f29t_load9(b), f29t_load9(b + 9)), out);
  } else if (op == 4) {
    const xyzz29 p = xyzz29_from_jacobian(f29t_load9(a), f29t_load9(a + 9), f29t_load9(a + 18));
    if (xyzz29_is_identity(p)) return;
    f29 x, y, z;
    xyzz29_to_jacobian(p, x, y, z);
    f29t_store9(p.zz, out);
    f29t_store9(p.zzz, out + 9);
    f29t_store9(x, out + 18);
    f29t_store9(y, out + 27);
  } else {
    f29 x, y;
    xyzz29_to_affine(f29t_load_xyzz(a), x, y);
    f29t_store9(x, out);
    f29t_store9(y, out + 9);
  }
}

// table format of an affine point (Mont256, 16 words): canonical Mont261 packed words, read back as the kernels read them;
// false for the identity (0, 0), which the caller skips
H2_HD bool f29t_table_point(const uint32_t* p, bool neg, f29& x2, f29& y2) {
  uint32_t any = 0;
  for (int k = 0; k < 16; k++) any |= p[k];
  if (any == 0) return false;
  uint32_t xw[8], yw[8];
  f29_pack(f29_reduce_canonical<Fq29>(f29_from_mont256<Fq29>(p)), xw);
  f29_pack(f29_reduce_canonical<Fq29>(f29_from_mont256<Fq29>(p + 8)), yw);
  x2 = f29_unpack(xw);
  y2 = f29_unpack(yw);
  if (neg) y2 = f29_sub(f29_zero(), y2, Fq29::K2);
  return true;
}

// accumulate n affine points (Mont256, 16 words each; (0,0) skipped) with signs[i] != 0 meaning -P_i; writes the XYZZ result
// as 4 x 8 words Mont256 (canonical), all zeros for the identity.  tree == 0: one accumulator, mixed additions only.
// tree in {2, 4, 8, 16}: exercise the full XYZZ addition / doubling: the points are dealt to `tree` groups, each accumulated
// with mixed additions, then the group sums are folded pairwise (and at 16 the sum goes through S + S - 2S + S)
H2_HD void f29t_chain_one(const uint32_t* pts, const uint8_t* signs, size_t n, uint32_t* out_xyzz, int tree) {
  xyzz29 acc = xyzz29_identity();
  f29 x2, y2;
  if (!tree) {
    for (size_t i = 0; i < n; i++)
      if (f29t_table_point(pts + 16 * i, signs[i] != 0, x2, y2)) xyzz29_madd(acc, x2, y2);
  } else {
    xyzz29 groups[16];
    for (int g = 0; g < tree; g++) groups[g] = xyzz29_identity();
    for (size_t i = 0; i < n; i++)
      if (f29t_table_point(pts + 16 * i, signs[i] != 0, x2, y2)) xyzz29_madd(groups[i % tree], x2, y2);
    for (int stride = 1; stride < tree; stride *= 2)
      for (int g = 0; g + stride < tree; g += 2 * stride) xyzz29_add(groups[g], groups[g + stride]);
    acc = groups[0];
    if (tree == 16) {  // (S + S) - via add's doubling branch - then + (-2S) computed by dbl ... keep S: S + S - S - S + S
      xyzz29 s2 = acc;
      xyzz29_add(s2, acc);              // doubling branch of add
      xyzz29 d = xyzz29_dbl(acc);       // explicit doubling
      d.y = f29_normalize(f29_sub(f29_zero(), d.y, Fq29::K4));  // -2S
      xyzz29_add(s2, d);                // 2S + (-2S) = identity
      xyzz29_add(s2, acc);              // identity + S = S
      acc = s2;
    }
  }
  if (xyzz29_is_identity(acc)) {
    for (int k = 0; k < 32; k++) out_xyzz[k] = 0;
    return;
  }
  f29_to_mont256<Fq29>(acc.x, out_xyzz);
  f29_to_mont256<Fq29>(acc.y, out_xyzz + 8);
  f29_to_mont256<Fq29>(acc.zz, out_xyzz + 16);
  f29_to_mont256<Fq29>(acc.zzz, out_xyzz + 24);
}

}  // namespace h2
