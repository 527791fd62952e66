/* h2mi_hooks.h — test hooks of libh2mi_hooks.so (the product's objects + csrc/h2mi_hooks.hip); never part of libh2mi.so.
 * Elementwise device arithmetic on host arrays, used by the parity tests only: the 32-bit-limb field operations and whole point
 * operations of the one group law (tests/test_gpu_parity.py), and the 29-bit-limb layer the hot kernels compute in, on chosen limbs
 * (h2mi_dbg_f29_*, tests/test_gpu_f29.py). */
#ifndef H2MI_HOOKS_H
#define H2MI_HOOKS_H
#include "../../include/h2mi.h"
#ifdef __cplusplus
extern "C" {
#endif
int h2mi_dbg_field_op(int field /*0=Fq,1=Fr*/, int op /*0=mul,1=add,2=sub,3=sqr,5=from_mont,6=to_mont,7=neg,8=dbl,9=inv by division steps,10=inv by binary Euclid*/,
                      const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
/* the group law the MSM runs (csrc/g1_29.cuh) through the format bridge of csrc/g1.cuh.  op 0: out = P + Q (affine inputs, via
 * xyzz29_madd); 1: 2P (xyzz29_dbl); 2: P + Q via xyzz29_add, Q as a representative with ZZ != 1; output Jacobian (12 limbs each) */
int h2mi_dbg_g1_op(int op, const uint64_t* p_affine, const uint64_t* q_affine, uint64_t* out_jac, size_t n);
/* the lane-cooperative point operations of the bucket reduction (csrc/g1_29_quad.cuh), four lanes per
 * element: op 0 = P[i] + Q[i] (XYZZ + XYZZ), op 1 = 2 P[i]; affine Montgomery in, Jacobian out */
int h2mi_dbg_g1_quad_op(int op, const uint64_t* p, const uint64_t* q_or_null, uint64_t* out_jac, size_t n);
/* ---- the lazy 29-bit-limb layer (csrc/f29.cuh, g1_29.cuh) on the device.  Each hook mirrors an entry point of the g++ harness
 * tests/host/f29_host.cpp (f29t_*): same arguments, same element layout, the same per-element body (csrc/f29_testops.cuh), one
 * thread per element, operands read from global memory.  field: 0 = Fq29, 1 = Fr29.  The operands must respect the contracts
 * stated in f29.cuh; the hooks do not check them. */
/* a, b, out: 8 words per element (Mont256).  mode 0: a*b through Mont261; 1: NTT style, data a (Mont256, unpacked) x twiddle b
 * (converted to Mont261), canonical; 2: the lazy chain (a - b + 2p, un-normalized) * (a + b); 4: f29_sqr(a); 5: f29_inv(a)
 * (Fermat); 3: pack(unpack(a)) */
int h2mi_dbg_f29_mul(int field, int mode, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n);
/* raw 9-limb operands and results, 9 words per element */
int h2mi_dbg_f29_reduce_loose(int field, const uint32_t* in9, uint32_t* out9, size_t n);   /* normalized, value < 64p -> canonical */
int h2mi_dbg_f29_mul_raw(int field, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n); /* limbs(a) < 1.9 * 2^30, b normalized */
int h2mi_dbg_f29_sqr_raw(int field, const uint32_t* a, uint32_t* out, size_t n);           /* a normalized */
int h2mi_dbg_f29_mul2_raw(int field, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out, size_t n);
int h2mi_dbg_f29_mul3_raw(int field, const uint32_t* ops /* [6][n][9] */, uint32_t* out, size_t n);
/* one point operation of csrc/g1_29.cuh per element on RAW coordinates (9 limbs each, loaded as given: no reduction, no
 * canonicalisation), so that operands can sit at the bounds the header states; a, b and out hold 36 words per element (an XYZZ
 * point fills them, an affine (x, y) the first 18, a Jacobian (X, Y, Z) the first 27; an operand an op does not take is ignored
 * but must be there).  Ops 0..5 are f29t_point_raw_one, one thread per element, as f29t_point_raw of the g++ harness: 0 =
 * xyzz29_madd(a, b.x, b.y); 1 = xyzz29_dbl(a); 2 = xyzz29_add(a, b); 3 = xyzz29_dbl_affine(b.x, b.y); 4 = xyzz29_from_jacobian(a)
 * then xyzz29_to_jacobian (out = ZZ, ZZZ, X', Y'); 5 = xyzz29_to_affine(a).  Ops 6 / 7 are the lane-cooperative
 * xyzz29_add_quad(a, b) / xyzz29_dbl_quad(a) of csrc/g1_29_quad.cuh, four lanes per element, the writing lane rotating. */
int h2mi_dbg_g1_29_raw_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n);
/* f29t_madd_chain, batched: chain c accumulates the affine points (Mont256, 16 words each; (0,0) skipped) offsets[c] ..
 * offsets[c + 1] of pts with signs[i] != 0 meaning -P_i, one thread per chain, all chains in one launch; offsets has nchains + 1
 * entries starting at 0.  tree = 0: mixed additions into one accumulator; 2 / 4 / 8 / 16: that many group accumulators folded
 * pairwise with the full XYZZ addition (at 16 also the doubling and cancellation sequence).  out_xyzz: 4 x 8 words Mont256 per
 * chain, all zeros for the identity.
 * The pair-affine chain (f29t_pair_chain) has no device hook: no product kernel uses affine29_pair_add any more, so it stays a
 * host-only test of the header. */
int h2mi_dbg_g1_29_chains(const uint32_t* pts, const uint8_t* signs, const uint64_t* offsets, size_t nchains, uint32_t* out_xyzz, int tree);
/* What the general MSM pipeline left in a workspace slot (tests/test_gpu_msm_occupancy.py): the slot of the last MSM of `handle`
 * (back = 0) or of the back-th one before it; the handle must have been registered with this library instance.  Flushes the deferred
 * reductions and synchronises, as h2mi_msm_last_stats.  H2MI_EINVAL when the handle's last MSM took the small path (no bucket
 * tables).  Two calls, like h2mi_profile_dump: data = NULL returns the size in *need_words, then data receives that many 32-bit words.
 * geometry: c, W, nb, lb, nbins, logNl, logNh, seg_log, n, payload row stride, rows, has_sum, entries, slot, last MSM took the small
 *           path, nseg (segments of wide windows, else 0).
 * data, in this order: s0 [1]; off, np0, np1, toff0, toff1 [nb + 1 each]; the payloads in bucket order [entries]; shift [8, Montgomery];
 *           dense [nb x 36]; dense2, vsum [nseg x 36 each].  A partial sum is 36 words: X, Y, ZZ, ZZZ as nine 29-bit limbs, Montgomery-2^261. */
int h2mi_dbg_msm_snapshot(uint64_t handle, int back, uint64_t geometry[16], uint32_t* data, size_t cap_words, size_t* need_words);
/* The same for a small-path MSM (tests/test_gpu_msm_small.py).  H2MI_EINVAL when the slot's last MSM did not take the small path.
 * Two calls as above, sizes in bytes.
 * geometry: c, W, gathering lanes per workgroup, cells per lane, workgroups of a full-length MSM (sG), registered points, points of
 *           this MSM, its workgroups G, slot; the rest 0.
 * data, in this order: the entries each workgroup added [sG + 1 words, the last one the arrival counter; beyond G: what earlier MSMs
 *           left]; the partial sums [G x 144 bytes: 36 words as above]; the digit bytes sign << 7 | magnitude [W][registered points]
 *           (columns beyond this MSM's points: what earlier MSMs left). */
int h2mi_dbg_msm_small_snapshot(uint64_t handle, int back, uint64_t geometry[16], uint8_t* data, size_t cap_bytes, size_t* need_bytes);
/* `count` chosen entries of the digit-multiples table of a handle whose last MSM took the small path: entry ((j - 1) W + w) n + i is
 * the affine point j 2^(c w) P_i, j = 1 .. 2^(c-1), as 16 canonical Montgomery-2^261 words (x, y), all zeros for the identity.
 * H2MI_ERANGE for an entry beyond the table. */
int h2mi_dbg_msm_small_table(uint64_t handle, const uint64_t* entries, size_t count, uint32_t* out);
#ifdef __cplusplus
}
#endif
#endif
