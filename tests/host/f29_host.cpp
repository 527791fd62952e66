// Host-side harness for the plain-C++ field/curve layer (halo2-scaffold_amd/csrc/f29.cuh, g1_29.cuh):
// the same code the GPU kernels inline, compiled with g++ so the arithmetic is verified on the CPU
// against the big-integer oracle before it ever runs on a GPU.  Test infrastructure only.
#include <vector>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../halo2-scaffold_amd/csrc/f29_testops.cuh"

using namespace h2;

// The per-element bodies (f29t_*_one, f29t_chain_one) live in csrc/f29_testops.cuh: the device hooks h2mi_dbg_f29_* of
// csrc/h2mi_hooks.hip run the same bodies on the GPU (tests/test_gpu_f29.py), with the same arguments and element layout.
extern "C" {
void f29t_mul(int field, int mode, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  for (size_t i = 0; i < n; i++) {
    if (field == 0) f29t_mul_one<Fq29>(mode, a + 8 * i, b + 8 * i, out + 8 * i);
    else f29t_mul_one<Fr29>(mode, a + 8 * i, b + 8 * i, out + 8 * i);
  }
}

static void raw(int field, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out, size_t n) {
  for (size_t i = 0; i < n; i++) {
    const uint32_t *pb = b ? b + 9 * i : nullptr, *pc = c ? c + 9 * i : nullptr, *pd = d ? d + 9 * i : nullptr;
    if (field == 0) f29t_raw_one<Fq29>(op, a + 9 * i, pb, pc, pd, out + 9 * i);
    else f29t_raw_one<Fr29>(op, a + 9 * i, pb, pc, pd, out + 9 * i);
  }
}

// f29_reduce_loose on raw normalized 9-limb values (value < 64p): in 9 words, out 9 words per element
void f29t_reduce_loose(int field, const uint32_t* in, uint32_t* out, size_t n) { raw(field, 0, in, nullptr, nullptr, nullptr, out, n); }

// f29_mul on raw limb patterns (9 words each): out = a*b / 2^261, normalized limbs; limbs(a) < 1.9 * 2^30, b normalized
void f29t_mul_raw(int field, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) { raw(field, 1, a, b, nullptr, nullptr, out, n); }

// f29_sqr on raw normalized limb patterns (9 words each): out = a*a / 2^261, normalized limbs
void f29t_sqr_raw(int field, const uint32_t* a, uint32_t* out, size_t n) { raw(field, 2, a, nullptr, nullptr, nullptr, out, n); }

// f29_mul2 on raw limb patterns (9 words each): out = (a*b + c*d) / 2^261, normalized limbs
void f29t_mul2_raw(int field, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out, size_t n) {
  raw(field, 3, a, b, c, d, out, n);
}

// f29_mul3 on raw limb patterns (six operands, 9 words each): out = (a*b + c*d + e*f) / 2^261
void f29t_mul3_raw(int field, const uint32_t* ops /* [6][n][9] */, uint32_t* out, size_t n) {
  for (size_t i = 0; i < n; i++) {
    if (field == 0) f29t_mul3_one<Fq29>(ops, n, i, out + 9 * i);
    else f29t_mul3_one<Fr29>(ops, n, i, out + 9 * i);
  }
}

// one point operation of g1_29.cuh per element on raw 9-limb coordinates (f29t_point_raw_one: ops 0..5); a, b, out hold 36 words
// per element (b may be null for the ops that take no second operand)
void f29t_point_raw(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  for (size_t i = 0; i < n; i++) f29t_point_raw_one(op, a + 36 * i, b ? b + 36 * i : nullptr, out + 36 * i);
}

// accumulate n affine points (Mont256, 16 words each; (0,0) skipped) with signs[i] != 0 meaning -P_i;
// writes the XYZZ result as 4 x 8 words Mont256 (canonical); `tree`: see f29t_chain_one
void f29t_madd_chain(const uint32_t* pts, const uint8_t* signs, size_t n, uint32_t* out_xyzz, int tree) {
  f29t_chain_one(pts, signs, n, out_xyzz, tree);
}

// the pair-affine accumulation on the host: consecutive points are added in pairs in AFFINE coordinates (affine29_pair_add, the
// inverses of x2 - x1 by Montgomery's trick over the whole list, as the kernels share them), each pair's sum enters the XYZZ
// accumulator by a mixed addition; a pair with equal x (P + P, P - P) or an identity member goes in as two singles — the routing
// k_msm_pa_forward / k_msm_pa_backward apply.  Same input / output format as f29t_madd_chain.
void f29t_pair_chain(const uint32_t* pts, const uint8_t* signs, size_t n, uint32_t* out_xyzz) {
  std::vector<f29> xs(n), ys(n);
  std::vector<bool> ident(n);
  for (size_t i = 0; i < n; i++) {
    const uint32_t* p = pts + 16 * i;
    bool id = true;
    for (int k = 0; k < 16; k++) id = id && p[k] == 0;
    ident[i] = id;
    uint32_t xw[8], yw[8];
    f29_pack(f29_reduce_canonical<Fq29>(f29_from_mont256<Fq29>(p)), xw);
    f29_pack(f29_reduce_canonical<Fq29>(f29_from_mont256<Fq29>(p + 8)), yw);
    xs[i] = f29_unpack(xw);
    ys[i] = f29_unpack(yw);
  }
  auto same_x = [&](size_t a, size_t b) {
    bool eq = true;
    for (int k = 0; k < 9; k++) eq = eq && xs[a].v[k] == xs[b].v[k];
    return eq;
  };
  const size_t npairs = n / 2;
  std::vector<bool> valid(npairs);
  std::vector<f29> before(npairs);
  f29 prod = f29_const<Fq29>(Fq29::ONE);
  for (size_t j = 0; j < npairs; j++) {
    valid[j] = !ident[2 * j] && !ident[2 * j + 1] && !same_x(2 * j, 2 * j + 1);
    if (!valid[j]) continue;
    before[j] = prod;
    prod = f29_mul<Fq29>(prod, affine29_pair_diff(xs[2 * j], xs[2 * j + 1]));
  }
  f29 run = f29_inv<Fq29>(prod);
  xyzz29 acc = xyzz29_identity();
  auto single = [&](size_t i) {
    if (ident[i]) return;
    f29 y = ys[i];
    if (signs[i]) y = f29_sub(f29_zero(), y, Fq29::K2);
    xyzz29_madd(acc, xs[i], y);
  };
  if (n & 1) single(n - 1);
  for (size_t j = npairs; j-- > 0;) {
    if (!valid[j]) {
      single(2 * j + 1);
      single(2 * j);
      continue;
    }
    const f29 dinv = f29_mul<Fq29>(run, before[j]);
    run = f29_mul<Fq29>(run, affine29_pair_diff(xs[2 * j], xs[2 * j + 1]));
    f29 x3, y3;
    affine29_pair_add(xs[2 * j], ys[2 * j], signs[2 * j] != 0, xs[2 * j + 1], ys[2 * j + 1], signs[2 * j + 1] != 0, dinv, x3, y3);
    xyzz29_madd(acc, x3, y3);
  }
  if (xyzz29_is_identity(acc)) {
    memset(out_xyzz, 0, 128);
    return;
  }
  f29_to_mont256<Fq29>(acc.x, out_xyzz);
  f29_to_mont256<Fq29>(acc.y, out_xyzz + 8);
  f29_to_mont256<Fq29>(acc.zz, out_xyzz + 16);
  f29_to_mont256<Fq29>(acc.zzz, out_xyzz + 24);
}
}
