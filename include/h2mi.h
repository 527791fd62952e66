/* h2mi.h — C ABI of libh2mi.so: BN254 MSM + NTT backend for AMD Instinct MI355X (gfx950).
 *
 * Drop-in boundary for the hot path of the Halo2/KZG prover that DCMMC/halo2-scaffold drives through
 * create_proof() (reference examples/standard_plonk.rs:41-49, src/scaffold.rs:191-199,322-331).  The
 * reference itself has no FFI seam; the seam is Cargo's [patch] of its halo2_proofs dependency
 * (reference Cargo.toml:13,16), whose arithmetic::{best_multiexp, best_fft}, poly::EvaluationDomain and
 * poly::kzg::commitment::ParamsKZG call the functions below (binding shown in INTEGRATION.md).
 *
 * Data layouts are those of halo2curves::bn256 (reference src/scaffold.rs:14):
 *   Fr, Fq    4 x uint64 little-endian limbs, MONTGOMERY form (R = 2^256), fully reduced
 *   G1Affine  {x, y} = 8 x uint64; the identity is (0, 0)
 *   G1        {x, y, z} = 12 x uint64 Jacobian (x/z^2, y/z^3); the identity has z = 0
 *
 * Conventions: every function returns H2MI_OK (0) or a negative H2MI_E* code; h2mi_strerror() names
 * it.  No C++ exception crosses this boundary.  Pointers named d_* are DEVICE pointers (HBM of the
 * process's GPU); all others are host pointers owned by the caller for the duration of the call.
 * Multi-GPU, two ways: one process per GPU (h2mi_init picks the GPU; the job combines the 96-byte partial MSM
 * results itself: RCCL all-gather + h2mi_g1_fold_groups_dev), or ONE process driving n GPUs
 * (h2mi_init_devices: the bases are sharded at registration and every MSM folds its partial results internally).
 * Calls are serialised by an internal mutex, so any thread may call.
 * There is NO CPU fallback: without a usable GPU every compute entry point returns H2MI_ENODEV.
 */
#ifndef H2MI_H
#define H2MI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define H2MI_OK 0
#define H2MI_EINVAL (-1)   /* bad argument (null pointer, size 0 where not allowed, log_n out of range) */
#define H2MI_ENODEV (-2)   /* no usable GPU / h2mi_init not called                                      */
#define H2MI_ENOMEM (-3)   /* device or host allocation failed                                          */
#define H2MI_EHIP (-4)     /* a HIP runtime call or kernel launch failed                                */
#define H2MI_EHANDLE (-5)  /* unknown or released bases handle                                          */
#define H2MI_ERANGE (-6)   /* n larger than the registered base count / unsupported size                */
#define H2MI_EUNSAT (-7)   /* h2mi_prover.h: the witness does not satisfy the circuit where the prover can see it
                              (a lookup input that is not a table value: the crate's Error::ConstraintSystemFailure) */

#define H2MI_MAX_LOG_N 28  /* largest NTT the device path accepts: the field's two-adicity (2^28 x 32 B = 8 GiB per buffer) */

typedef void* h2mi_stream_t; /* a hipStream_t, or NULL for the library's own stream */

/* ---- lifecycle ---------------------------------------------------------------------------------- */
/* Select GPU `device` (ordinal visible to this process) and create the library's stream.  Idempotent
 * for the same device.  Replaces nothing in the reference (which has no device); the Rust shim calls
 * it once from a `std::sync::Once`. */
int h2mi_init(int device);
/* One prover process, n devices (SURVEY.md 8b `h2mi_init(n_devices)`; the reference is one process calling
 * create_proof once, src/scaffold.rs:246-366): devices 0 .. n-1, device 0 the primary.  Afterwards
 *   h2mi_bases_register{,_dev}   shard the base set: one contiguous slice (and its window tables) per device;
 *   h2mi_msm_bn254_g1{,_dev}     launch every slice from the calling thread and fold the 96-byte partial results on
 *                                the primary device (host form: at once; _dev form, stream = NULL only: at the next
 *                                h2mi_join / h2mi_sync / h2mi_memcpy_d2h, like every queued MSM);
 * transforms, polynomial helpers and every d_* pointer stay on the primary device (NTT is single-GPU by design).
 * H2MI_VIRTUAL_DEVICES=1 lets n exceed the number of GPUs (entry i runs on GPU i mod count): a one-GPU rehearsal of
 * the sharding, scalar distribution and fold.  Mutually exclusive with h2mi_init. */
int h2mi_init_devices(int n_devices);
int h2mi_device_count(void); /* devices this process drives (0 before init) */
int h2mi_primary_device(void); /* the ordinal of the device every d_* pointer lives on (-1 before init): what a host compares a foreign
                                  allocation's device with before it hands the pointer over (H2MI_CELLS_DEVICE, h2mi_prover.h) */
void h2mi_shutdown(void);
const char* h2mi_strerror(int code);
const char* h2mi_version(void);

/* ---- device memory (so a host can keep vectors resident between calls) ---------- */
int h2mi_malloc(size_t bytes, void** d_ptr);
int h2mi_free(void* d_ptr);
int h2mi_memcpy_h2d(void* d_dst, const void* src, size_t bytes);
/* queued on the library's stream without waiting for it (pageable `src` is staged by the runtime before the call
 * returns): for the small patches a prover writes into device-resident columns (assigned cells, blinding rows) */
int h2mi_memcpy_h2d_async(void* d_dst, const void* src, size_t bytes);
/* `count` 32-byte field elements (Montgomery limbs, host memory) written to `count` device addresses (16-byte aligned) by ONE kernel
 * launch per 64 cells — the cells travel in the launch's arguments, so `values` may be reused at once.  For the handful of assigned
 * cells and blinding rows a prover patches into zeroed columns (create_proof's `advice[column][row] = value`): a dozen 32-byte
 * hipMemcpyAsync calls cost ~10 us each on the library stream in front of a phase's first commitment.  Stream-ordered on `stream`
 * (NULL = the library stream); cells given twice keep one of the values. */
int h2mi_fr_patch_cells_dev(void* const* d_cells, const uint64_t* values, size_t count, h2mi_stream_t stream);
int h2mi_memcpy_d2h(void* dst, const void* d_src, size_t bytes);
int h2mi_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes);
int h2mi_memset_zero(void* d_ptr, size_t bytes); /* asynchronous on the library's stream */
int h2mi_sync(void); /* wait for all work queued on the library's streams */
/* device-side join: later work on the library's stream waits for every MSM queued so far to be complete.
 * An MSM queued on the library's stream (h2mi_msm_bn254_g1_dev with stream = NULL) only runs its bucket
 * partition and accumulation at once; the latency-bound bucket reduction is deferred and run for all MSMs
 * queued since the last join as one batch, so the 96-byte results are written only by h2mi_join / h2mi_sync /
 * h2mi_memcpy_d2h / h2mi_msm_flush — or when half of a handle's workspace slots are pending: two MSMs for base sets
 * above 2^17 points (four slots), four below (eight slots).  A prover calls h2mi_join where the transcript
 * needs the commitments of a phase.  MSMs on a caller-provided stream complete in order on that stream.
 * Base sets of at most 2^14 points defer their whole accumulate-and-finish launch the same way (H2MI_MSM_GENERAL below). */
int h2mi_join(void);
/* start the deferred bucket reductions of the MSMs queued so far NOW, on the library's reduction stream, without ordering
 * the library's stream behind them (h2mi_join still does that, later): a prover that has queued the commitments of a phase
 * and goes on to queue work that does not need them (the columns' transforms) calls this first, so the reductions run
 * beside that work instead of starting when the host reaches h2mi_join. */
int h2mi_msm_flush(void);
/* ---- side streams.  Every *_dev entry point takes a stream (NULL = the library's own, on which calls execute in issue
 * order).  A second stream lets work that does not depend on the next transcript challenge — e.g. the coefficient and
 * extended forms of the advice columns, needed only by evaluate_h — run beside the library stream's chain instead of
 * queueing behind it.  h2mi_stream_wait(waiter, signaller) makes everything queued later on `waiter` start after
 * everything queued so far on `signaller` (NULL = the library stream on either side); it does not block the host. */
int h2mi_stream_create(h2mi_stream_t* stream_out);
int h2mi_stream_destroy(h2mi_stream_t stream);
int h2mi_stream_wait(h2mi_stream_t waiter, h2mi_stream_t signaller);

/* the library's own stream (a hipStream_t), so that a host can order foreign work — an RCCL collective, its own
 * kernels — against the library's without a host synchronisation */
int h2mi_library_stream(void** stream_out);

/* ---- bases (the KZG SRS): ParamsKZG::{g, g_lagrange}, SURVEY.md 8a row a5 ------------------------
 * Replaces the `&params.g` / `&params.g_lagrange` slices that ParamsKZG::commit / commit_lagrange pass
 * to best_multiexp (reached from reference examples/standard_plonk.rs:33,34,41-49).  Registration
 * copies the n affine points to HBM and builds the per-window multiples table 2^(c*w) * P_i (all
 * windows then share one bucket set), once; commits afterwards move only scalars. */
int h2mi_bases_register(const uint64_t* bases /* n*8 limbs */, size_t n, uint64_t* handle_out);
int h2mi_bases_register_dev(const void* d_bases /* n*64 B */, size_t n, uint64_t* handle_out);
int h2mi_bases_release(uint64_t handle);
/* window bits c, window count W, bucket count, registered n */
int h2mi_bases_info(uint64_t handle, uint32_t* c, uint32_t* windows, uint32_t* buckets, uint64_t* n);
/* Registration with a TABLE DEPTH: the full table is W x (n + 1) x 64 B per base set (0.94 GiB at n = 2^20, 3.25 GiB at 2^22) and lets
 * all windows share one bucket set.  At table depth D the handle keeps only every D'-th window row, D' = min(D, W): rows =
 * ceil(W / D') rows 2^(c D' j) P_i, and one workspace slot sized for rows x (n + 1) entries instead of four or eight for W x (n + 1).
 * An MSM on it runs D' passes, pass r over the windows w = r mod D' (partition, accumulation and bucket reduction as ever, against row
 * floor(w / D')), and one last kernel combines the pass results as sum_r 2^(c r) R_r.  The mode trades time for memory:
 * the accumulation work is unchanged, the partition head and the bucket reduction run D' times (profiles/table_depth_cost.txt).
 *   table_depth == 0    H2MI_EINVAL
 *   table_depth == 1    exactly h2mi_bases_register{,_dev}
 *   table_depth >= W    the bases alone (1 / W of the table)
 * MSMs on such a handle run in order on the stream they are given (NULL = the library's) with nothing deferred to the next join: the
 * result is written in stream order, and the scalars may be overwritten by work queued on that stream after the call.  The handle never
 * has the latency path's table; the flags of h2mi_msm_bn254_g1_phase_dev are accepted and change nothing, and a group is the loop
 * over its members.  Results are the same group elements as at depth 1 (and with h2mi_msm_set_canonical(1) the same bytes).
 * After h2mi_init_devices with more than one device a depth above 1 is H2MI_EINVAL: sharded compact base sets are not built yet.
 * The ad-hoc cache of h2mi_msm_bn254_g1 (handle == 0) keeps full tables. */
int h2mi_bases_register_depth(const uint64_t* bases /* n*8 limbs */, size_t n, uint32_t table_depth, uint64_t* handle_out);
int h2mi_bases_register_depth_dev(const void* d_bases /* n*64 B */, size_t n, uint32_t table_depth, uint64_t* handle_out);
/* what the handle holds on the device: effective depth D', table rows, bytes of the table(s) incl. the latency
 * path's, bytes of the slots' workspaces (the bytes asked of the allocator; a sharded handle: summed over its slices,
 * depth and rows of the first); any pointer may be NULL */
int h2mi_bases_memory(uint64_t handle, uint32_t* table_depth, uint32_t* table_rows, uint64_t* table_bytes, uint64_t* workspace_bytes);

/* ---- MSM: halo2_proofs::arithmetic::best_multiexp(coeffs, bases) -> C::Curve ---------------------
 * Replaces best_multiexp for C = bn256::G1Affine; computes sum_i s_i * P_i over
 * the first n registered bases.  Scalars are Fr values exactly as they sit in memory (Montgomery).
 * The result is a Jacobian representative of the exact group element (the caller batch-normalises
 * before hashing, as create_proof does); identity is returned as (0, R, 0) = G1::identity().
 * Which representative (X : Y : Z) comes back is NOT reproducible between two calls on the same input:
 * the order of additions inside a bucket follows arrival order in the bucket partition (the reference's
 * representative likewise depends on its thread count).  h2mi_msm_set_canonical(1) makes every MSM end
 * with a normalisation to Z = 1 (bit-reproducible output, about 0.17 ms more latency per MSM).
 * The reference asserts coeffs.len() == bases.len(); here n > registered n returns H2MI_ERANGE. */
int h2mi_msm_bn254_g1(uint64_t handle_or_0, const uint64_t* bases_or_null /* used when handle==0 */,
                      const uint64_t* scalars /* n*4 limbs */, size_t n, uint64_t out_jacobian[12]);
/* handle == 0 (best_multiexp on a plain slice of bases) does NOT rebuild the window tables on every call: the bases
 * are uploaded, fingerprinted on the device over every byte and looked up in a cache of the four most recent ad-hoc
 * registrations, so repeated calls with the same slice pay the 64 B x n upload only.  Register explicitly
 * (h2mi_bases_register) to avoid that too.  h2mi_msm_adhoc_builds: how many ad-hoc registrations have been built. */
int h2mi_msm_adhoc_builds(uint64_t* builds_out);
/* device-resident form: scalars and the 96-byte result live in HBM; asynchronous on `stream`. */
int h2mi_msm_bn254_g1_dev(uint64_t handle, const void* d_scalars, size_t n, void* d_out_jacobian,
                          h2mi_stream_t stream);
/* `count` MSMs of n scalars each over ONE registered base set — the commitments of a prover phase (create_proof commits a phase's advice
 * columns, then its grand products, then the quotient's pieces, each group before one challenge: reference examples/standard_plonk.rs:41-49
 * through halo2_proofs' create_proof).  Result j goes to d_out_jacobian + 96 j; the results are the ones `count` calls of
 * h2mi_msm_bn254_g1_dev in the same order would produce.  For base sets of up to 2^17 points on the library stream the partition and the
 * accumulation of up to four MSMs run as ONE set of launches (the host could not issue a small MSM's eight launches as fast as the device
 * ran them: DESIGN.md 4.1); larger base sets, caller streams and sharded handles take the loop.  The scalars must stay untouched until work
 * queued on `stream` after this call would run (as for the single form).  flags:
 *   H2MI_MSM_SPARSE   the caller's promise that the columns are SPARSE — mostly zeros, or one value repeated almost everywhere (witness
 *                     columns of a padded circuit, permutation / lookup grand products): the kernels of such an MSM are short at every
 *                     size, so the batched launches are used above 2^17 points as well (narrow windows; 20-bit windows take the loop).
 *                     Results do not depend on the promise; dense columns passed with it only lose the overlap between one MSM's partition
 *                     and the previous one's accumulation.
 *   H2MI_MSM_INORDER  the group is all its phase commits and its points are read back next (a lone commitment: count = 1): partition,
 *                     accumulation AND bucket reductions run in order on one stream, nothing is deferred to the join — the library's
 *                     three-stream split overlaps CONSECUTIVE MSMs and costs a lone one ~50 us of stream hops.  A dense group above 2^17
 *                     points keeps the pipelined loop, whose overlap is worth more; sharded handles take the ordinary path.
 *   H2MI_MSM_GENERAL  take the general (bucket) pipeline even for a base set that has the latency path's table.  Base sets of at most 2^14
 *                     points take a latency path of their own (narrow windows against a table of every digit multiple — up to 2 GB per
 *                     handle, skipped when it does not fit —, two short kernels: DESIGN.md 4.1), which wins a lone commitment and a phase
 *                     of four; above 2^13 points the general pipeline wins once MSMs stream back to back.  Without this flag the library
 *                     switches such a handle over by itself after four MSMs have been issued without a join (h2mi_join / h2mi_sync /
 *                     h2mi_memcpy_d2h); a caller that knows it streams says so up front.  Results do not depend on the path. */
#define H2MI_MSM_SPARSE 1u
#define H2MI_MSM_INORDER 2u
#define H2MI_MSM_GENERAL 4u
int h2mi_msm_bn254_g1_phase_dev(uint64_t handle, const void* const* d_scalars, size_t count, size_t n, void* d_out_jacobian, unsigned flags,
                                h2mi_stream_t stream);
/* 1: MSM results are normalised to Z = 1 on the device (reproducible bits); 0 (default): raw sum. */
int h2mi_msm_set_canonical(int on);
/* number of bucket insertions (non-zero signed digits) the last MSM on this handle performed, and the
 * running-sum reduction adds — the numerator of "G1-adds/s" (SURVEY.md 8d).  Synchronises. */
int h2mi_msm_last_stats(uint64_t handle, uint64_t* bucket_adds, uint64_t* reduce_adds);
/* sum of k Jacobian points (k*12 limbs, host) -> one Jacobian point: the combine step of the sliced
 * multi-GPU MSM (the fold `results.iter().fold(identity, |a, b| a + b)` of best_multiexp). */
int h2mi_g1_sum_jacobian(const uint64_t* points, size_t k, uint64_t out_jacobian[12]);
/* the same fold for k MSMs at once: points[r*k + j] is rank r's partial result of MSM j -> out[j] */
int h2mi_g1_fold_groups(const uint64_t* points /* world*k*12 */, size_t world, size_t k, uint64_t* out /* k*12 */);
/* the same fold on device-resident points (e.g. the buffer an RCCL all-gather filled), asynchronous on `stream`:
 * the per-phase combine of a sliced multi-GPU prover never leaves HBM */
int h2mi_g1_fold_groups_dev(const void* d_points /* world*k*96 B */, size_t world, size_t k, void* d_out /* k*96 B */, h2mi_stream_t stream);
/* batch Jacobian -> affine (G1::batch_normalize, used by create_proof before transcript writes) */
int h2mi_g1_batch_normalize(const uint64_t* jac /* k*12 */, size_t k, uint64_t* affine_out /* k*8 */);
int h2mi_g1_batch_normalize_dev(const void* d_jac /* k*96 B */, size_t k, void* d_affine_out /* k*64 B */, h2mi_stream_t stream);

/* ---- NTT: halo2_proofs::arithmetic::best_fft(a, omega, log_n) ------------------------------------
 * Replaces best_fft for G = bn256::Fr: in-place DFT out[i] = sum_j a[j] *
 * omega^(i*j), natural order in and out.  The reference asserts a.len() == 1 << log_n; the caller
 * passes log_n and the buffer must hold 2^log_n elements.  log_n in [0, H2MI_MAX_LOG_N]. */
int h2mi_ntt_bn254_fr(uint64_t* a /* n*4 limbs, in place */, const uint64_t omega[4], uint32_t log_n);
/* EvaluationDomain helpers fused into the first / last pass:
 *   a[i] *= pre_scale_base^i  (distribute_powers_zeta with base = g_coset), then the DFT,
 *   then a[i] *= post_scale   (the ifft divisor n^-1).  Either pointer may be NULL. */
int h2mi_ntt_ext_bn254_fr(uint64_t* a, uint32_t log_n, const uint64_t omega[4],
                          const uint64_t* pre_scale_base_or_null, const uint64_t* post_scale_or_null);
/* device-resident form, asynchronous on `stream`; omega / scale constants are host pointers. */
int h2mi_ntt_bn254_fr_dev(void* d_a, uint32_t log_n, const uint64_t omega[4],
                          const uint64_t* pre_scale_base_or_null, const uint64_t* post_scale_or_null,
                          h2mi_stream_t stream);
/* out-of-place, zero-extending form: reads src_len <= 2^log_n elements from d_src (the rest count as zero),
 * writes the 2^log_n results to d_dst; d_src is left untouched and must not overlap d_dst.  This is
 * EvaluationDomain::coeff_to_extended without the clone and the zero padding (src_len = n, log_n =
 * extended_k, pre = g_coset), and lagrange_to_coeff on a column the prover still needs in Lagrange form. */
int h2mi_ntt_bn254_fr_oop_dev(const void* d_src, size_t src_len, void* d_dst, uint32_t log_n, const uint64_t omega[4],
                              const uint64_t* pre_scale_base_or_null, const uint64_t* post_scale_or_null,
                              h2mi_stream_t stream);
/* a[i] *= base^i on the device (EvaluationDomain::distribute_powers_zeta after an inverse coset NTT) */
int h2mi_fr_scale_powers_dev(void* d_a, size_t n, const uint64_t base[4], const uint64_t* post_scale_or_null,
                             h2mi_stream_t stream);

/* ---- opening-argument helpers on device-resident coefficient vectors ------------------
 * halo2_proofs::arithmetic::eval_polynomial(poly, point): out = sum_i poly[i] * point^i  (32 B at d_out) */
int h2mi_fr_eval_poly_dev(const void* d_poly, size_t n, const uint64_t point[4], void* d_out, h2mi_stream_t stream);
/* the same for `count` <= 24 polynomials of n coefficients at ONE point (create_proof evaluates every queried
 * column at x): one launch; result k at d_out + 32 k */
int h2mi_fr_eval_polys_dev(const void* const* d_polys, size_t count, size_t n, const uint64_t point[4], void* d_out, h2mi_stream_t stream);
/* every evaluation a proof writes, in ONE call: `ngroups` groups of polynomials (d_polys holds them group after group, group g has
 * group_counts[g] members) opened at points[g] (ngroups x 4 limbs); d_out receives the values in d_polys' order.  Up to 4 points and 24
 * polynomials share one power-table launch, one evaluation launch and one row sum (create_proof opens at x, omega x and omega^-(b+1) x:
 * nine launches through the per-point form); larger requests are served group by group. */
int h2mi_fr_eval_polys_multi_dev(const void* const* d_polys, const size_t* group_counts, const uint64_t* points, size_t ngroups, size_t n, void* d_out,
                                 h2mi_stream_t stream);
/* builds the cached power tables of `count` <= 32 bases (count x 4 limbs) at the size the helpers use for n-coefficient vectors, the
 * missing ones in one launch: with an opening argument's roots and their inverses known up front, the divisions that follow find their
 * tables instead of building them one launch at a time.  Purely a scheduling hint: results never depend on it. */
int h2mi_fr_powtab_prefetch_dev(const uint64_t* bases, size_t count, size_t n, h2mi_stream_t stream);
/* halo2_proofs::arithmetic::kate_division(a, b): quotient of a(X) by (X - b), n - 1 coefficients at d_out
 * (the remainder a(b) is dropped, as in the crate).  The caller passes b^-1 (one CPU inversion). */
int h2mi_fr_kate_division_dev(const void* d_poly, size_t n, const uint64_t b[4], const uint64_t b_inv[4], void* d_out,
                              h2mi_stream_t stream);
/* division by prod_{i < m} (X - roots[i]), m <= 4 distinct roots, of a polynomial they all vanish at — what SHPLONK's
 * div_by_vanishing does with one kate_division per point (poly/kzg/multiopen/shplonk/prover.rs [RECALL]) — in ONE round:
 * d_out[j] = sum_i weights[i] * (a / (X - roots[i]))[j] for j < n - 1, with weights[i] = 1 / prod_{k != i} (roots[i] - roots[k])
 * computed by the caller (partial fractions; the m quotients are independent, the chain of m dependent divisions is not).
 * roots, roots_inv, weights: m x 4 limbs, Montgomery.  d_out[n - 1] is left untouched; the top m - 1 written coefficients
 * come out as exact zeros.
 * Footprint: the m quotients are materialised side by side in the calling stream's scratch vector before they are summed —
 * m x (n + n / 512 + 1024) field elements (m = 4, n = 2^22: 0.5 GB; n = 2^25: 4 GB), one such scratch per stream that
 * issues divisions (SHPLONK's three lanes).  The scratch is grow-only; its first growth synchronises the device. */
int h2mi_fr_kate_division_multi_dev(const void* d_poly, size_t n, const uint64_t* roots, const uint64_t* roots_inv, const uint64_t* weights,
                                    size_t m, void* d_out, h2mi_stream_t stream);
/* out[i] = sum_k scalars[k] * polys[k][i], count <= 24 (the challenge-weighted sums of SHPLONK) */
int h2mi_fr_lincomb_dev(const void* const* d_polys, const uint64_t* scalars /* count*4 */, size_t count, size_t n, void* d_out,
                        h2mi_stream_t stream);
/* ProverGWC's witness polynomials (poly/kzg/multiopen/gwc [RECALL]), all points in one call:
 * d_outs[g] = (sum_j scalars_gj * poly_gj) / (X - roots[g]) for `ngroups` groups laid out as in h2mi_fr_eval_polys_multi_dev (d_polys
 * and scalars hold the groups behind one another, group g has group_counts[g] members; roots, roots_inv: ngroups x 4 limbs, Montgomery,
 * the inverses from the caller).  Each d_outs[g] holds n coefficients: the n - 1 of the quotient and a zero at n - 1.  The remainder —
 * the sum's value at the root — is dropped as kate_division drops it: the quotient does not read the numerator's constant term, so
 * the evaluations need not be subtracted first.  A polynomial may appear in several groups; outputs must not alias inputs or each
 * other.  Three launches per slice of up to 4 points and 72 terms, the summed polynomials never stored; a group of more than 72 terms
 * is summed by the linear-combination kernel into scratch first (same bits).  H2MI_EINVAL: n < 2, no group, an empty group, a null
 * pointer, a zero root or inverse.  Scratch: 4 x (n + n / 512 + 1024) field elements per stream, plus n per group over 72 terms. */
int h2mi_fr_gwc_witness_dev(const void* const* d_polys, const uint64_t* scalars, const size_t* group_counts, const uint64_t* roots,
                            const uint64_t* roots_inv, size_t ngroups, size_t n, void* const* d_outs, h2mi_stream_t stream);

/* poly[i] += head[i] for i < count <= 16: the low-degree remainder terms R(X) / r = R(u) that SHPLONK subtracts
 * from a (linear combination of) opened polynomial(s) — poly/kzg/multiopen/shplonk/prover.rs
 * `quotient_contribution` / `linearisation_contribution`. */
int h2mi_fr_add_head_dev(void* d_poly, const uint64_t* head /* count*4 */, size_t count, h2mi_stream_t stream);
/* out[i] = a[i] * b[i] over n elements (in place allowed): the row values of a product of columns, e.g. the lookup input
 * q_lookup * a of halo2-base's single-advice-column range check */
int h2mi_fr_mul_dev(const void* d_a, const void* d_b, size_t n, void* d_out, h2mi_stream_t stream);
/* ff's BatchInvert: out[i] = in[i]^-1, and out[i] = 0 where in[i] = 0 (a zero is skipped, it does not spoil its neighbours) [RECALL ff
 * 0.13 BatchInvert / BatchInverter::invert_with_external_scratch, restated from memory].  Inputs are fully reduced Montgomery words;
 * outputs are the canonical Montgomery words.  ONE field inversion per call whatever n is: Montgomery's trick in tiles of 1024 (three
 * launches: tile products, the inverses of the tile products, the finish per tile).  In place (d_out == d_in) is allowed.  n = 0: nothing
 * happens; n > 2^32, a null or misaligned pointer: H2MI_EINVAL. */
int h2mi_fr_batch_invert_dev(const void* d_in, size_t n, void* d_out, h2mi_stream_t stream);
/* Assigned::evaluate over a vector [RECALL halo2_proofs v2023_02_02 plonk/assigned.rs, poly.rs batch_invert_assigned]: pairs holds
 * n x (numerator, denominator), 64 bytes per element; out[i] = numerator[i] * denominator[i]^-1, or 0 where the denominator is 0
 * (whatever the numerator).  Trivial(x) is (x, 1).  The same chain and the same one inversion as h2mi_fr_batch_invert_dev; d_out must
 * not be d_pairs. */
int h2mi_fr_assigned_evaluate_dev(const void* d_pairs, size_t n, void* d_out, h2mi_stream_t stream);
/* The same for the rational cells of up to 64 COLUMNS in one chain (what h2mi_column_cells with H2MI_CELLS_RATIONAL resolves to,
 * h2mi_prover.h): every column's pairs (HOST memory, count x 8 limbs) are staged behind one another in the stream's scratch, resolved
 * with one inversion, and cell i of a column lands at d_column + rows[i] (or + i when rows is NULL; 32-byte elements; the caller has
 * checked the rows against the column's length).  canonical != 0: both halves are canonical integers; *invalid_out counts the halves
 * that are not below r (the call then waits for the stream; invalid_out is required).  The call waits for its uploads, so the host
 * buffers are free when it returns; the chain itself is stream-ordered.  The rows of one column must be distinct: cells that name the
 * same row are written by different threads in no order.  All columns of a call are staged in ONE slice of 64 bytes per cell (plus 4
 * per listed row) in the stream's grow-only scratch, which keeps that size afterwards: a call whose cells would fit as resolved
 * columns can still end in H2MI_ENOMEM — split the columns over several calls then (each pays one inversion).  More than 2^32 cells in
 * one call: H2MI_ERANGE. */
typedef struct {
  void* d_column;
  const uint32_t* rows;
  const uint64_t* pairs;
  size_t count;
} h2mi_assigned_cells;
int h2mi_fr_assigned_columns_dev(const h2mi_assigned_cells* cols, uint32_t n_cols, int canonical, uint64_t* invalid_out, h2mi_stream_t stream);
/* Witness cells that are in DEVICE memory already, written into up to 64 columns by ONE launch (k_cells_scatter; what h2mi_column_cells
 * with H2MI_CELLS_DEVICE, or a long host run with H2MI_CELLS_I64, becomes: h2mi_prover.h).  Cell i of a source lands at d_column + 32 rows[i]
 * (or + 32 i when rows is NULL), converted where `format` asks: 0 — 32-byte Montgomery words, carried verbatim (not range-checked);
 * H2MI_CELLS_CANONICAL (1) — 32-byte canonical integers, times R^2 as h2mi_fe_from_repr_dev does; H2MI_CELLS_I64 (4) — signed 64-bit
 * integers v, the cell is v mod r (|v| in the low limb, the same product, negated when v < 0).  Work is partitioned over the total cell
 * count, not per column; rows of a destination that no cell names are left untouched.  status_out[0] counts the cells whose row is at or
 * beyond row_limit: they are skipped, so nothing is written outside a column's first row_limit rows whatever `rows` holds.
 * status_out[1] counts the canonical values not below r: they are written as zero.  status_out is required and the call waits for the
 * stream to deliver it.  Rows of one source must be distinct: cells that name the same row are written in no order.  Pointers: d_column
 * and 32-byte values 16-byte aligned, I64 values 8, rows 4; a source with count == 0 is skipped and none of its pointers is looked at.
 * H2MI_EINVAL: a null or misaligned pointer, an unknown format, n_cols > 64; H2MI_ERANGE: more than 2^32 cells in one call. */
typedef struct {
  void* d_column;        /* 32-byte elements */
  const uint32_t* rows;  /* device; NULL = rows 0 .. count-1 */
  const void* values;    /* device */
  size_t count;
  uint32_t row_limit;    /* rows at or beyond it are counted, not written */
  uint32_t format;       /* 0, H2MI_CELLS_CANONICAL or H2MI_CELLS_I64 */
} h2mi_cells_source;
int h2mi_fr_scatter_cells_dev(const h2mi_cells_source* cols, uint32_t n_cols, uint64_t status_out[2], h2mi_stream_t stream);
/* The same with some sources in HOST memory: bit i of host_mask says that cols[i].values and cols[i].rows are host pointers.  They are
 * staged behind one another in the stream's grow-only scratch (8 or 32 bytes per cell, plus 4 per listed row), which keeps that size
 * afterwards: H2MI_ENOMEM where it does not fit.  The host buffers are free when the call returns.  Still one launch. */
int h2mi_fr_scatter_cells_staged_dev(const h2mi_cells_source* cols, uint32_t n_cols, uint64_t host_mask, uint64_t status_out[2], h2mi_stream_t stream);
/* The inverse: up to 64 device columns of Montgomery Fr words -> each column's nonzero cells below its row_limit, in ascending row order
 * (what a proving-key file stores of a fixed column: h2mi_prover_pk_export).  Three launches serve all columns of the call:
 * k_cells_count (one word per tile of 1024 rows), k_cells_prefix (each column's offsets and its count / last / fits64), k_cells_compact
 * (the cells; it reads only the tiles that hold any).  No atomic decides a position: the output does not depend on scheduling.
 * Per column the call reports count (nonzero cells), last (last nonzero row + 1) and fits64 (every nonzero canonical value v has v <=
 * 2^63 - 1 or v >= r - 2^63; 1 for an empty column), and picks
 *   width   8 when fits64 — the cell is the signed 64-bit integer v, or -(r - v), exactly what H2MI_CELLS_I64 decodes — else 32: the
 *           canonical little-endian word, below r, as H2MI_CELLS_CANONICAL reads it;
 *   layout  H2MI_COMPACT_LAYOUT_DENSE when last * width <= count * (4 + width): `values` holds rows 0 .. last - 1, zeros included, and
 *           there is no row list; H2MI_COMPACT_LAYOUT_SPARSE otherwise: `rows` holds count uint32 rows, `values` their count cells;
 *           0 for an empty column (count 0: nothing is written for it).
 * flags: H2MI_COMPACT_SPARSE forces the sparse layout, H2MI_COMPACT_WORDS forces width 32.  With alloc == NULL the call ends after the
 * counts (two launches).  Otherwise the library calls alloc(alloc_ctx, bytes) ONCE, with the exact size of the output — per non-empty
 * column its values, then its row list, each part padded to 16 bytes — and sets every column's values / rows to point into the block
 * it returned (NULL: H2MI_ENOMEM).  The block is host memory: the cells are staged in the stream's grow-only scratch and copied, the
 * padding is not written.  Nothing is
 * written beyond the stated parts.  The call waits for the stream.  The columns are read twice and must not change meanwhile; their words
 * must be reduced below r.  H2MI_EINVAL: n_cols > 64, a null or misaligned column with row_limit > 0, an unknown flag; H2MI_ERANGE:
 * row_limit > 2^28. */
#define H2MI_COMPACT_SPARSE 2u
#define H2MI_COMPACT_WORDS 4u
#define H2MI_COMPACT_LAYOUT_DENSE 1u
#define H2MI_COMPACT_LAYOUT_SPARSE 2u
typedef struct {
  const void* d_column; /* in: 32-byte Montgomery words, at least row_limit of them */
  uint32_t row_limit;   /* in: rows at or beyond it are not read */
  uint32_t last;        /* out */
  uint64_t count;       /* out */
  uint32_t fits64;      /* out */
  uint32_t layout;      /* out: 0, H2MI_COMPACT_LAYOUT_DENSE, H2MI_COMPACT_LAYOUT_SPARSE */
  uint32_t width;       /* out: 8 or 32 (0 for an empty column) */
  uint32_t* rows;       /* out: into the allocated block; NULL unless sparse */
  void* values;         /* out: into the allocated block */
} h2mi_cells_compacted;
typedef void* (*h2mi_compact_alloc_fn)(void* ctx, size_t bytes);
int h2mi_fr_compact_cells_dev(h2mi_cells_compacted* cols, uint32_t n_cols, unsigned flags, h2mi_compact_alloc_fn alloc, void* alloc_ctx,
                              h2mi_stream_t stream);
/* Witness programs: a builder closure whose shape does not depend on its inputs is a fixed straight-line program over field elements.
 * Recorded once (the Python recorder is halo2-scaffold_amd/witness.py), it is evaluated on the device for every proof and its cells land
 * in dense Montgomery columns that h2mi_prover_advice takes as H2MI_CELLS_DEVICE (h2mi_prover.h) — no cell crosses the host.
 * The program describes a flat list of n_ops cells, one op per cell: op = (dst, kind | bits << 8 | shift << 16, a, b), 16 bytes; the top
 * byte of the code is zero.
 *   H2MI_WITNESS_INPUT  cells[dst] = inputs[a]          (h2mi_witness_run's inputs: canonical, below r)
 *   H2MI_WITNESS_CONST  cells[dst] = constants[a]       (canonical, below r)
 *   H2MI_WITNESS_COPY   cells[dst] = cells[a]
 *   H2MI_WITNESS_GATE   cells[dst] = cells[dst - 3] + cells[dst - 2] * cells[dst - 1]      (the fourth cell of a vertical gate)
 *   H2MI_WITNESS_LIMB   cells[dst] = (canonical(cells[a]) >> shift) & (2^bits - 1), 1 <= bits <= 64, shift + bits <= 254
 * The hint ops — the values a builder computes outside the gates and assigns as witnesses.  With x = canonical(cells[a]), 0 <= x < r:
 *   H2MI_WITNESS_DIVQ   cells[dst] = the quotient, H2MI_WITNESS_DIVR the remainder, of x by y.  The bits byte holds the flags:
 *                       H2MI_WITNESS_DIV_CONST: y = constants[b], otherwise y = canonical(cells[b]) — b is the second operand;
 *                       H2MI_WITNESS_DIV_SIGNED: a dividend x > 2^252 is read as x~ = x - r (the fixed-point chip's negative numbers).
 *                       Unsigned: q = floor(x / y), rem = x - y q.  Signed: q = floor(x~ / y), rounded toward minus infinity and stored
 *                       modulo r, rem = x~ - y q in [0, y).  y = 0 gives 0 for both.  shift = 0; any other flag bit is refused.
 *   H2MI_WITNESS_ISZERO cells[dst] = 1 if x = 0, else 0.                        No flags, shift = 0, b = 0.
 *   H2MI_WITNESS_INV    cells[dst] = x^-1 mod r, and 1 for x = 0 (what halo2-base's is_zero assigns there).  No flags, shift = 0, b = 0.
 *   H2MI_WITNESS_MSB    cells[dst] = the index of the highest set bit of x, 0 .. 253; x = 0 gives 1 (what the fold over the bits in the
 *                       reference's qlog2 yields there).  No flags, shift = 0, b = 0.
 *   H2MI_WITNESS_POW2   cells[dst] = 2^x for x <= 253, and 0 for every larger x up to r - 1.  One flag in the bits byte,
 *                       H2MI_WITNESS_POW2_OF_MSB: cells[dst] = 2^MSB(x) — so that a power of two can be assigned before its exponent,
 *                       from the same cell.  shift = 0, b = 0; any other flag bit is refused.
 * Kinds 5 .. 7 are unassigned and refused, kind 12 is reserved and refused, as is every kind above H2MI_WITNESS_POW2.  A program that holds a hint op runs its levels in
 * a second instantiation of the two level kernels, k_witness_level_hints / k_witness_levels_wg_hints, under the same launch rule; a
 * program without one launches what it always launched.
 * Cells that no column places are allowed: a recorder uses them for values derived outside the columns and for gates it evaluates once
 * more to compare them, by a check, with a fourth cell that is not a GATE op.
 * Levels: ops[level_ends[l - 1] .. level_ends[l]) are level l (level_ends[-1] = 0, no level is empty, the last one ends at n_ops); an op
 * reads only cells written at strictly lower levels: cell a of COPY, LIMB and the hints, cell b of a DIVQ / DIVR whose divisor is a
 * cell, the three cells before dst of a GATE.  checks: n_checks pairs (a, b) of cells that must hold equal values (the
 * equalities no COPY makes true, such as range_check's constrain_equal of the value with its recomposed limbs).  Placement: column j of
 * the n_columns dense output columns is cells[placement[start_j + row]] for row < counts[j], start_j = counts[0] + .. + counts[j - 1].
 * Launches (the rule is part of the interface): a level of more than H2MI_WITNESS_WG_OPS ops is one k_witness_level launch; every
 * maximal run of consecutive levels of at most H2MI_WITNESS_WG_OPS ops is a sequence of k_witness_levels_wg launches — ONE workgroup,
 * a barrier between levels — of at most H2MI_WITNESS_WG_LEVELS levels each; one k_witness_place launch gathers the columns and
 * evaluates the checks.
 * h2mi_witness_check (host only, works without a GPU; h2mi_witness_create applies it first): H2MI_EINVAL for an unknown kind, a dst
 * named twice or never, an operand whose level is not strictly below its reader's, level_ends that do not ascend to n_ops, a GATE with
 * dst < 3, shift / bits outside their bounds, an unknown flag or a shift on a hint, flags or b on ISZERO / INV / MSB, b on POW2, an INPUT or CONST index
 * (DIVQ / DIVR with H2MI_WITNESS_DIV_CONST: b) out of range, a constant not below r, a placement source or a
 * check index >= n_ops, a null array with a nonzero count; H2MI_ERANGE for more than 2^28 cells, more than 2^28 cells in one column or
 * more than H2MI_WITNESS_MAX_COLUMNS columns.
 * h2mi_witness_create uploads the program once and allocates the cells and column buffers (H2MI_EINVAL with more than one device
 * under h2mi_init_devices, as for H2MI_CELLS_DEVICE).  h2mi_witness_run takes n_inputs x 4 canonical limbs (host memory; H2MI_EINVAL
 * for one not below r), enqueues everything on the library's stream, and returns in d_columns_out the n_columns device addresses of the
 * columns: they belong to the program and stay valid until its next run or its release; an advice call that follows is ordered behind
 * the run on the same stream and has consumed them when it returns.  The run ends with one small transfer of the check status: a
 * failed check is H2MI_EUNSAT with the lowest failing check index in *first_failed_check (0xffffffff otherwise), and the columns of
 * such a run are not to be used.  h2mi_witness_read: the canonical values (n x 4 limbs) of the listed cells after a run — the public
 * inputs are read this way. */
#define H2MI_WITNESS_INPUT 0u
#define H2MI_WITNESS_CONST 1u
#define H2MI_WITNESS_COPY 2u
#define H2MI_WITNESS_GATE 3u
#define H2MI_WITNESS_LIMB 4u
#define H2MI_WITNESS_DIVQ 8u
#define H2MI_WITNESS_DIVR 9u
#define H2MI_WITNESS_ISZERO 10u
#define H2MI_WITNESS_INV 11u
#define H2MI_WITNESS_MSB 13u /* 12 is reserved */
#define H2MI_WITNESS_POW2 14u
#define H2MI_WITNESS_POW2_OF_MSB 1u /* flag of POW2, in the bits byte */
#define H2MI_WITNESS_DIV_CONST 1u  /* flags of DIVQ / DIVR, in the bits byte */
#define H2MI_WITNESS_DIV_SIGNED 2u
#define H2MI_WITNESS_WG_OPS 1024u    /* the workgroup limit */
#define H2MI_WITNESS_WG_LEVELS 4096u /* keeps any one kernel short whatever the circuit's depth */
#define H2MI_WITNESS_MAX_COLUMNS 64u /* = H2MI_MAX_ADVICE of h2mi_prover.h */
typedef struct { uint32_t dst; uint32_t code; uint32_t a; uint32_t b; } h2mi_witness_op;
typedef struct {
  const h2mi_witness_op* ops;
  const uint32_t* level_ends;
  const uint64_t* constants;  /* n_constants x 4 canonical limbs */
  const uint32_t* checks;     /* n_checks pairs */
  const uint32_t* placement;  /* counts[0] + .. + counts[n_columns - 1] cell indices */
  const uint32_t* counts;
  uint32_t n_ops;             /* = the number of cells */
  uint32_t n_levels;
  uint32_t n_constants;
  uint32_t n_inputs;
  uint32_t n_checks;
  uint32_t n_columns;
} h2mi_witness_desc;
typedef struct {
  uint32_t n_cells;
  uint32_t n_levels;
  uint32_t n_grid_launches; /* k_witness_level (or k_witness_level_hints) launches of one run */
  uint32_t n_wg_launches;   /* k_witness_levels_wg (or k_witness_levels_wg_hints) launches of one run */
  uint64_t device_bytes;    /* held by the program: ops, cells, columns, placement, checks, constants, inputs */
} h2mi_witness_info_t;
typedef void* h2mi_witness_t;
int h2mi_witness_check(const h2mi_witness_desc* d);
int h2mi_witness_create(const h2mi_witness_desc* d, h2mi_witness_t* out);
int h2mi_witness_info(h2mi_witness_t w, h2mi_witness_info_t* out);
int h2mi_witness_run(h2mi_witness_t w, const uint64_t* inputs, void** d_columns_out, uint32_t* first_failed_check);
int h2mi_witness_read(h2mi_witness_t w, const uint32_t* cells, uint32_t n, uint64_t* out);
int h2mi_witness_release(h2mi_witness_t w);
/* out[i] = value for i < n (Lagrange vectors such as l_active of keygen_pk) */
int h2mi_fr_fill_dev(void* d_out, size_t n, const uint64_t value[4], h2mi_stream_t stream);
/* Seeded stand-in for the prover's sweeps of `Scalar::random(rng)` (blinding rows; the vanishing argument's random
 * polynomial, plonk/vanishing/prover.rs `Argument::commit`; the reference passes OsRng, examples/standard_plonk.rs:48,
 * so its bytes are not reproducible — SURVEY.md 0).  Counter-based SplitMix64: element i has limbs
 * splitmix64(seed << 32 | 4 (start + i) + j), j = 0..3, top limb masked to 62 bits, reduced once; seed < 2^32. */
int h2mi_fr_random_dev(void* d_out, size_t n, uint64_t seed, uint64_t start, h2mi_stream_t stream);
/* the same sweep from a 256-bit key, for proofs that have to hide their witness: element i = Fr::from_u512 of ChaCha20 block start + i
 * (RFC 7539 block function; 64-bit block counter, 64-bit stream id `stream_id`: the layout of rand_chacha's ChaCha20Rng, whose eight
 * next_u64 per Fr::random are one block [RECALL halo2curves]); key: 32 bytes, host memory.  h2mi_prover_set_rng_key (h2mi_prover.h) uses it. */
int h2mi_fr_random_chacha_dev(void* d_out, size_t n, const uint8_t key[32], uint64_t stream_id, uint64_t start, h2mi_stream_t stream);

/* ---- quotient numerator for the reference's StandardPlonk circuit -------------------------
 * halo2_proofs plonk/evaluation.rs `evaluate_h` + vanishing division, specialised to the circuit of reference
 * src/circuits/standard_plonk.rs (one degree-3 gate over 3 advice + 5 fixed columns, 3 permutation sets of one
 * column).  All vectors are extended-domain evaluations (2^extended_k elements) resident in HBM.  The result (h on
 * the extended coset, already divided) goes to d_h_out; h2mi_ntt_bn254_fr_dev + h2mi_fr_scale_powers_dev bring it
 * to coefficients. */
/* What every quotient call knows of the domain and the transcript, in the order of evaluate_h's own parameters.  Every
 * pointer: 4 limbs, Montgomery, host memory; t_inv: the 2^(extended_k - k) values of (X^n - 1)^-1 on the coset, 4 limbs
 * each.  Every quotient call refuses a NULL record or a NULL field of it with H2MI_EINVAL, and extended_k < k,
 * extended_k - k > 4 or extended_k > H2MI_MAX_LOG_N with H2MI_ERANGE. */
typedef struct {
  uint32_t k, extended_k, blinding_factors;
  const uint64_t *beta, *gamma, *y, *delta, *zeta, *extended_omega;
  const uint64_t* t_inv;
} h2mi_quotient_scalars;
typedef struct {
  const void* advice[3];  /* a, b, c */
  const void* fixed[5];   /* q_a, q_b, q_c, q_ab, constant */
  const void* sigma[3];   /* permutation polynomials of a, b, c */
  const void* z[3];       /* permutation products */
  const void* l0;
  const void* l_last;
  const void* l_active;
} h2mi_standard_plonk_cosets;
int h2mi_plonk_evaluate_h_standard_dev(const h2mi_standard_plonk_cosets* cosets, const h2mi_quotient_scalars* scalars, void* d_h_out,
                                       h2mi_stream_t stream);

/* the permutation argument's grand-product column for one chunk of m <= 64 columns (plonk/permutation/prover.rs,
 * the z vectors are produced where they are consumed): z[0] = start (one if NULL),
 *   z[i+1] = z[i] * prod_j (v_j[i] + beta delta^(c_j) omega^i + gamma) / prod_j (v_j[i] + beta sigma_j[i] + gamma),  i < usable_rows;
 * rows usable_rows+1 .. 2^k-1 of d_z (the blinding rows) are left untouched; z[usable_rows] also goes to d_last
 * (32 B, device) as the next chunk's start.  beta_delta_pows[j] = beta * delta^(index of column j in the argument).
 * One field inversion per call (prefix / suffix products of the denominators); a zero denominator makes the
 * result meaningless, where the crate would panic.  Asynchronous on `stream`. */
int h2mi_plonk_permutation_product_dev(const void* const* d_values, const void* const* d_sigmas, uint32_t m, uint32_t k,
                                       uint32_t usable_rows, const uint64_t beta[4], const uint64_t gamma[4],
                                       const uint64_t* beta_delta_pows /* m*4 */, const uint64_t omega[4],
                                       const void* d_start_or_null, void* d_z, void* d_last_or_null, h2mi_stream_t stream);

/* every set of the permutation argument in one pass: m <= 64 (H2MI_FLEX_MAX_PERM) columns in argument order, chunked by chunk_len
 * (= cs.degree() - 2) into ceil(m / chunk_len) sets; d_z[s] receives rows 0 .. usable_rows of set s, each set
 * starting at the previous set's last value (plonk/permutation/prover.rs chains them through `last_z`); blinding
 * rows untouched.  One scan over the concatenated sets instead of one call (twelve launches) per set. */
int h2mi_plonk_permutation_products_dev(const void* const* d_values, const void* const* d_sigmas, uint32_t m, uint32_t chunk_len, uint32_t k,
                                        uint32_t usable_rows, const uint64_t beta[4], const uint64_t gamma[4],
                                        const uint64_t* beta_delta_pows /* m*4 */, const uint64_t omega[4], void* const* d_z,
                                        h2mi_stream_t stream);
/* The same with the support of the copy constraints known (a keygen-time fact): `d_active` holds, sorted ascending, the
 * positions set * usable_rows + row (uint32) at which some column of the set has sigma != the identity permutation — the
 * only rows whose ratio can differ from one.  Numerators, denominators, the inversion and the scans then run over these
 * n_active positions only and every z row is filled from the prefix product of the positions before it: same values, work
 * proportional to the constrained cells plus one write per row (the halo2-lib examples constrain 10 .. 10^4 of 2^20 rows).
 * n_active = 0: every product is one. */
int h2mi_plonk_permutation_products_sparse_dev(const void* const* d_values, const void* const* d_sigmas, uint32_t m, uint32_t chunk_len, uint32_t k,
                                               uint32_t usable_rows, const uint64_t beta[4], const uint64_t gamma[4],
                                               const uint64_t* beta_delta_pows, const uint64_t omega[4], const void* d_active, uint32_t n_active,
                                               void* const* d_z, h2mi_stream_t stream);

/* ---- lookup argument (plonk/lookup/prover.rs), single-expression lookups: the range check the reference's
 * RangeWithInstanceCircuitBuilder configures with LOOKUP_BITS (src/scaffold.rs:44-48,434-485; examples/range.rs:10-34).
 * commit_permuted's permute_expression_pair on the device: d_permuted_input[0 .. usable_rows) = the usable input rows
 * sorted (Fr's Ord: canonical integer order), d_permuted_table = the table rearranged against it (the input value where
 * a run starts, the unconsumed table values — ascending — on the repeated rows, last repeated row first); rows beyond
 * usable_rows (the blinding rows) are left untouched.  The fixed table is described by its distinct usable values in
 * ascending order (canonical little-endian integers AND the same values in Montgomery form) and their multiplicities,
 * prepared once at keygen: a proof needs no sort, only a counting sort against them.  not_in_table_out (mandatory; the
 * call synchronises on it) receives the number of inputs that are not table values — the crate fails the proof then, and
 * the permuted columns are meaningless: H2MI_EINVAL without it. */
int h2mi_plonk_lookup_permute_dev(const void* d_input, const void* d_table_sorted_canonical, const void* d_table_sorted_mont,
                                  const void* d_table_mult /* u32 x n_unique */, uint32_t n_unique, uint32_t k, uint32_t usable_rows,
                                  void* d_permuted_input, void* d_permuted_table, uint64_t* not_in_table_out, h2mi_stream_t stream);
/* The table side of that call for a table that is NOT fixed — compressed with the proof's theta, or holding advice (lookup_any): the
 * distinct values of d_in[0 .. count) (Montgomery) in ascending canonical-integer order, as the three arrays
 * h2mi_plonk_lookup_permute_dev takes (canonical values, the same values in Montgomery form, u32 multiplicities; each with room for
 * `count` entries) and their number.  A radix sort over an index permutation, on the device, for any input (all keys equal, keys
 * that differ in one word, a 16-bit counting table, uniform keys): digit positions on which every key agrees cost nothing.  The
 * call synchronises `stream` twice (32 bytes that say where the keys differ, then n_unique), and once more in the rare case that keys
 * which differ in more than eight bytes were not told apart by the prefix they are sorted on first.  count in [1, 2^H2MI_MAX_LOG_N]. */
int h2mi_fr_sort_unique_dev(const void* d_in, uint32_t count, void* d_sorted_canonical, void* d_sorted_mont, void* d_mult /* u32 x count */,
                            uint32_t* n_unique_out, h2mi_stream_t stream);
/* extended-coset form of an instance column from the proving key's l_0 coset, without transforms: the column holds `count`
 * <= 16 public inputs on rows 0 .. count - 1 (what the scaffold's builders constrain: src/scaffold.rs:411, 480) and zeros
 * elsewhere, so its coset values are sum_r values[r] * l0_coset[(j - r 2^(extended_k - k)) mod 2^extended_k] — the same field
 * elements coeff_to_extended(lagrange_to_coeff(column)) yields.  values: count x 4 limbs, Montgomery. */
int h2mi_plonk_instance_coset_dev(const void* d_l0_coset, uint32_t k, uint32_t extended_k, const uint64_t* values, size_t count, void* d_out,
                                  h2mi_stream_t stream);
/* The same for the n_columns <= H2MI_MAX_INSTANCE instance columns of one circuit in ONE launch: column c holds counts[c] <= 16 public
 * inputs values[c] (counts[c] x 4 limbs, Montgomery; may be NULL with a count of 0: the column is zero) and its coset form goes to
 * d_out[c], 2^extended_k elements.  Every thread loads each rotated l_0 value once for all the columns.  The scaled values travel in a
 * device buffer written on `stream`.  Column c's words are those of the call above on values[c].  d_out entries must not overlap. */
#define H2MI_MAX_INSTANCE 8
int h2mi_plonk_instance_coset_multi_dev(const void* d_l0_coset, uint32_t k, uint32_t extended_k, const uint64_t* const* values, const size_t* counts,
                                        uint32_t n_columns, void* const* d_out, h2mi_stream_t stream);
/* commit_product: z[0] = 1, z[i+1] = z[i] (a_i + beta)(t_i + gamma) / ((a'_i + beta)(s'_i + gamma)), i < usable_rows;
 * blinding rows untouched; one field inversion per call.  From 4096 usable rows the product runs over the rows whose ratio can
 * differ from one ((a_i, t_i) != (a'_i, s'_i): all but ~2^17 of 2^22 rows of a range check are skipped) when they are at most
 * a quarter of all rows; the call reads that count back, i.e. it waits for the work queued on `stream` before it (the library's
 * other streams keep running) */
int h2mi_plonk_lookup_product_dev(const void* d_input, const void* d_table, const void* d_permuted_input, const void* d_permuted_table, uint32_t k,
                                  uint32_t usable_rows, const uint64_t beta[4], const uint64_t gamma[4], void* d_z, h2mi_stream_t stream);
/* The shuffle argument's product [RECALL halo2_proofs (PSE line) plonk/shuffle/prover.rs commit_product — restated from memory like
 * the rest, pinned to DESIGN.md 4.5 and not to the crate]: z[0] = 1, z[i+1] = z[i] (A_i + gamma) / (S_i + gamma), i < usable_rows, over
 * the compressed input rows d_input and the compressed shuffle-side rows d_shuffle; rows 0 .. usable_rows of d_z are written, the
 * blinding rows untouched; one field inversion per call.  Dense form only: a shuffle that leaves most rows in place has no use.
 * H2MI_EUNSAT: z[usable_rows] is not one — the two sides are not the same multiset (z is written all the same); the call reads that one
 * element back, i.e. it waits for the work queued on `stream`.  A row with S_i + gamma = 0 (probability usable_rows / r over gamma)
 * gets no special handling: the one inversion is then of zero and z is meaningless. */
int h2mi_plonk_shuffle_product_dev(const void* d_input, const void* d_shuffle, uint32_t k, uint32_t usable_rows, const uint64_t gamma[4], void* d_z,
                                   h2mi_stream_t stream);
/* ---- logUp: the logarithmic-derivative lookup argument [Haboeck, "Multivariate lookups based on logarithmic derivatives"; the
 * `mv-lookup` feature of the Scroll and ezkl lines of halo2_proofs — restated from memory like the shuffle, pinned to DESIGN.md 4.5 and
 * tests/logup_cases.py and not to a crate].  One input tuple per lookup here (several: the _sets calls below); d_input / d_table are the two sides compressed with theta on the
 * 2^k rows (h2mi_plonk_expr_compress_dev at domain_k = k), Montgomery.
 * h2mi_fr_sort_unique_first_dev is h2mi_fr_sort_unique_dev with one more output: d_first[r] (u32 x count) = the lowest position of
 * d_in that holds distinct value r (the sort is stable over an index permutation).
 * Multiplicities: d_m[r] = the number of rows i < usable_rows with d_input[i] = d_table[r] for every row r < usable_rows that is the
 * FIRST usable row holding its table value, zero on every other row below usable_rows — as field elements in Montgomery form; rows at
 * and beyond usable_rows (the blinding rows) are left untouched.  The table's usable rows are sorted into distinct values on the
 * device, the inputs ranked against them with equal ranks merged per wavefront and workgroup (k_lk_rank), the counts scattered to
 * the first rows.  not_in_table_out (mandatory; the call synchronises on it): the inputs that are no table value — the lookup is
 * unsatisfied then and d_m does not sum to usable_rows. */
int h2mi_fr_sort_unique_first_dev(const void* d_in, uint32_t count, void* d_sorted_canonical, void* d_sorted_mont, void* d_mult /* u32 x count */,
                                  void* d_first /* u32 x count */, uint32_t* n_unique_out, h2mi_stream_t stream);
int h2mi_plonk_logup_multiplicity_dev(const void* d_input, const void* d_table, uint32_t k, uint32_t usable_rows, void* d_m,
                                      uint64_t* not_in_table_out, h2mi_stream_t stream);
/* The running sum: phi[0] = 0, phi[i+1] = phi[i] + 1 / (A_i + beta) - M_i / (S_i + beta), i < usable_rows; rows 0 .. usable_rows of
 * d_phi are written (phi[usable_rows] = 0 when d_m holds the multiplicities of a satisfied lookup), the blinding rows untouched.  One
 * fraction per row, ONE field inversion per call (prefix and suffix products of the denominators), then an additive prefix scan.
 * Dense form only.  A zero denominator (probability about 2 usable_rows / r over beta) gets no special handling: phi is then
 * meaningless. */
int h2mi_plonk_logup_sum_dev(const void* d_input, const void* d_table, const void* d_m, uint32_t k, uint32_t usable_rows, const uint64_t beta[4],
                             void* d_phi, h2mi_stream_t stream);
/* Several input sets over ONE table (the merged form): d_inputs points at n_inputs (1 .. H2MI_MAX_LOGUP_INPUTS)
 * consecutive vectors of 2^k elements, set j at element j 2^k, each compressed with theta.
 *   M[r] = sum_j #{i < usable_rows : A_j[i] = S[r]} on the lowest usable row r that holds its table value, 0 on the other usable rows:
 *          ONE sort of the table, every set ranked into the same histogram in one launch; not_in_table_out counts the inputs of ANY
 *          set that are no table value.
 *   phi[i+1] = phi[i] + sum_j 1 / (A_j,i + beta) - M_i / (S_i + beta): the row's fraction N / D by the recurrence (N, D) = (-M, S + beta),
 *          then per input N <- N (A_j + beta) + D, D <- D (A_j + beta); the inversion chain and the additive scan are the one-set call's.
 * The two calls above are these with n_inputs == 1.  H2MI_EINVAL: n_inputs == 0 or above the maximum. */
#define H2MI_MAX_LOGUP_INPUTS 6
int h2mi_plonk_logup_multiplicity_sets_dev(const void* d_inputs, uint32_t n_inputs, const void* d_table, uint32_t k, uint32_t usable_rows, void* d_m,
                                           uint64_t* not_in_table_out, h2mi_stream_t stream);
int h2mi_plonk_logup_sum_sets_dev(const void* d_inputs, uint32_t n_inputs, const void* d_table, const void* d_m, uint32_t k, uint32_t usable_rows,
                                  const uint64_t beta[4], void* d_phi, h2mi_stream_t stream);
/* The same argument against a table whose distinct values were sorted ELSEWHERE (a fixed table: once, at keygen), for input columns that
 * are table values as they stand (one component, no theta) [DESIGN.md 4.5, pinned to tests/table_logup_cases.py].  No sort, no
 * compressed vector and no per-row fraction inside a proof.
 * h2mi_plonk_logup_rank_cols_dev: d_inputs lists n_inputs (1 .. H2MI_MAX_LOGUP_INPUTS) device columns of 2^k elements, anywhere in memory
 * (Montgomery).  d_sorted_canonical: the n_unique distinct values of the table's usable rows, ascending, canonical 256-bit words;
 * d_first[r]: the lowest usable row that holds distinct value r (both as h2mi_fr_sort_unique_first_dev gives them).  ONE ranking launch
 * whatever n_inputs:
 *   d_ranks[j 2^k + i] = the rank of input j at usable row i (u32; rows >= usable_rows are not written; unspecified for an input that
 *     is no table value);
 *   d_counts[r] = the joint histogram, sum_j #{i < usable_rows : A_j[i] = sorted[r]} (u32 x n_unique, cleared by the call);
 *   d_m[first[r]] = counts[r] as a field element (Montgomery), every other usable row 0, rows >= usable_rows untouched: the M column
 *     h2mi_plonk_logup_multiplicity_sets_dev writes for the same columns and table;
 *   *not_in_table_out = the inputs of any column that are no table value (mandatory; the call synchronises the stream on it).
 * H2MI_EINVAL: a NULL pointer (a listed column included), n_unique == 0, n_inputs == 0 or above the maximum.  H2MI_ERANGE: k,
 * usable_rows out of range or n_unique > usable_rows.
 * h2mi_plonk_logup_sum_ranked_dev: the running sum from those ranks.  T[r] = 1 / (sorted[r] + beta), r < n_unique, by ONE field inversion
 * per call; usable row i contributes sum_j T[rank_j[i]], row first[r] also - counts[r] T[r]; phi[0] = 0 and phi[i + 1] = phi[i] + that,
 * on rows 0 .. usable_rows of d_phi, the rows behind untouched.  d_sorted_mont: the distinct values in the memory format.  The words
 * are those h2mi_plonk_logup_sum_sets_dev writes for the same columns and multiplicities (both store reduced Montgomery words).  A rank
 * that is no index below n_unique contributes nothing.  A zero denominator (sorted[r] = -beta) gets no special handling, as there: phi
 * is then meaningless. */
int h2mi_plonk_logup_rank_cols_dev(const void* const* d_inputs, uint32_t n_inputs, const void* d_sorted_canonical, uint32_t n_unique,
                                   const void* d_first /* u32 x n_unique */, uint32_t k, uint32_t usable_rows,
                                   void* d_ranks /* u32 x n_inputs x 2^k */, void* d_counts /* u32 x n_unique */, void* d_m,
                                   uint64_t* not_in_table_out, h2mi_stream_t stream);
int h2mi_plonk_logup_sum_ranked_dev(const void* d_ranks, uint32_t n_inputs, const void* d_sorted_mont, const void* d_counts, const void* d_first,
                                    uint32_t n_unique, uint32_t k, uint32_t usable_rows, const uint64_t beta[4], void* d_phi,
                                    h2mi_stream_t stream);
/* evaluate_h + vanishing division for the halo2-lib constraint systems [halo2-base shapes restated from memory]: gate
 * q (a + a(wX) a(w^2 X) - a(w^3 X)), permutation argument over n_perm <= 4 columns in chunks of chunk_len (= cs.degree()
 * - 2 = 1 .. 3), and — has_lookup (the Range builder, extended domain 4n) — one lookup in `table` of either
 * `lookup_selector` * a (halo2-base with a single advice column: a complex selector on the looked-up cells' own rows,
 * lookup degree 5, chunk_len 3) or, when `lookup_selector` is NULL, of the dedicated column `lookup_advice` (degree 4,
 * chunk_len 2); without has_lookup (the Gate builder: degree 3, chunk_len 1, extended domain 2n) the lookup pointers are
 * unused.  All vectors are extended-coset evaluations. */
typedef struct {
  const void* a;               /* the gate's advice column */
  const void* lookup_advice;   /* the lookup input column (NULL when lookup_selector is given) */
  const void* lookup_selector; /* q_lookup: the lookup input is q_lookup * a (NULL: lookup_advice) */
  const void* q;               /* gate selector */
  const void* table;           /* fixed lookup table */
  const void* perm_value[4];   /* equality-enabled columns in argument order */
  const void* perm_sigma[4];
  const void* perm_z[4];       /* ceil(n_perm / chunk_len) grand products */
  const void* lookup_permuted_input;
  const void* lookup_permuted_table;
  const void* lookup_z;
  const void* l0;
  const void* l_last;
  const void* l_active;
  uint32_t n_perm;
  uint32_t chunk_len;          /* 1, 2 or 3 */
  uint32_t has_lookup;         /* 0: gate + permutation terms only */
} h2mi_range_cosets;
int h2mi_plonk_evaluate_h_range_dev(const h2mi_range_cosets* cosets, const h2mi_quotient_scalars* scalars, void* d_h_out, h2mi_stream_t stream);

/* The general form of the halo2-base constraint systems (round 4; the column limits below from round 5): what
 * `builder.config(k, Some(minimum_rows))` (src/scaffold.rs:268) configures when the cells overflow ONE advice column — n_gates <=
 * H2MI_FLEX_MAX_GATES gate advice columns, each with its own selector and vertical gate; the permutation argument over n_perm <=
 * H2MI_FLEX_MAX_PERM columns (constants, the gate columns, the lookup-advice columns, the instance column) in chunks of chunk_len =
 * cs.degree() - 2; n_lookups <= H2MI_FLEX_MAX_LOOKUPS single-expression lookups
 * whose input is a lookup-advice column (lookup_input_b NULL) or the product of two columns (the single-column selector form).
 * Terms in evaluate_h's order: gates, permutation, lookups.  All vectors are extended-coset evaluations; t_inv as above.
 * Slower per point than the specialised entry above (every operand is converted to the multiplier's radix on load), and written
 * independently of its level bookkeeping: for a shape both accept the two must agree (tests/test_gpu_flex.py). */
#define H2MI_FLEX_MAX_GATES 32
#define H2MI_FLEX_MAX_PERM 64
#define H2MI_FLEX_MAX_LOOKUPS 8
typedef struct {
  uint32_t n_gates;
  const void* gate_a[H2MI_FLEX_MAX_GATES];
  const void* gate_q[H2MI_FLEX_MAX_GATES];
  uint32_t n_perm, chunk_len;
  const void* perm_value[H2MI_FLEX_MAX_PERM];
  const void* perm_sigma[H2MI_FLEX_MAX_PERM];
  const void* perm_z[H2MI_FLEX_MAX_PERM]; /* ceil(n_perm / chunk_len) grand products */
  uint32_t n_lookups;
  const void* lookup_input[H2MI_FLEX_MAX_LOOKUPS];
  const void* lookup_input_b[H2MI_FLEX_MAX_LOOKUPS]; /* NULL, or a second factor of the input expression */
  const void* lookup_table[H2MI_FLEX_MAX_LOOKUPS];
  const void* lookup_permuted_input[H2MI_FLEX_MAX_LOOKUPS];
  const void* lookup_permuted_table[H2MI_FLEX_MAX_LOOKUPS];
  const void* lookup_z[H2MI_FLEX_MAX_LOOKUPS];
  const void* l0;
  const void* l_last;
  const void* l_active;
} h2mi_flex_cosets;
int h2mi_plonk_evaluate_h_flex_dev(const h2mi_flex_cosets* cosets, const h2mi_quotient_scalars* scalars, void* d_h_out, h2mi_stream_t stream);

/* Gates given as DATA: the polynomials of `meta.create_gate(...)` (reference src/circuits/is_zero.rs, or.rs) as a postfix program that
 * one kernel interprets on the extended coset, in front of the permutation and lookup terms of the general form above.
 * One gate polynomial after another, each in postfix, in the order evaluate_h folds them with y (gates in create_gate order, a
 * gate's polynomials in the order of its Vec).  Expression<F> maps op for op; Scaled(e, c) is `e, CONSTANT c, MUL`, a selector is the
 * fixed query keygen substitutes for it. */
enum { H2MI_EXPR_ADVICE = 0, H2MI_EXPR_FIXED = 1, H2MI_EXPR_INSTANCE = 2,   /* = H2MI_COL_*: push column `index` at `rotation` */
       H2MI_EXPR_CONSTANT = 3,                                             /* push constants[index] */
       H2MI_EXPR_ADD, H2MI_EXPR_SUB, H2MI_EXPR_MUL, H2MI_EXPR_NEG,          /* on the top of the stack */
       H2MI_EXPR_END,                                                      /* the one value left is this polynomial */
       H2MI_EXPR_CHALLENGE };                                              /* push challenge `index` (rotation ignored): Expression::Challenge,
                                                                              degree 0.  index < the n_challenges of the call's record */
#define H2MI_MAX_EXPR_OPS 4096
#define H2MI_MAX_EXPR_CONSTANTS 256
#define H2MI_MAX_EXPR_STACK 8
#define H2MI_MAX_CHALLENGES 16    /* meta.challenge_usable_after(phase): values squeezed from the transcript between the advice phases */
#define H2MI_MAX_ADVICE_PHASES 3  /* FirstPhase .. ThirdPhase */
#define H2MI_EXPR_MAX_ADVICE 64 /* = H2MI_MAX_ADVICE / H2MI_MAX_FIXED of h2mi_prover.h */
#define H2MI_EXPR_MAX_FIXED 64
typedef struct { uint32_t op; uint32_t index; int32_t rotation; } h2mi_expr_op;
typedef struct {
  const h2mi_expr_op* ops;   uint32_t n_ops;        /* <= H2MI_MAX_EXPR_OPS */
  const uint64_t* constants; uint32_t n_constants;  /* n x 4 limbs, Montgomery; <= H2MI_MAX_EXPR_CONSTANTS */
} h2mi_gate_program;
/* h2mi_flex_cosets with the columns a program may query where gate_a / gate_q were.  A column the program does not read may be NULL;
 * n_perm == 0 and n_lookups == 0 are accepted (the gate terms alone). */
typedef struct {
  const void* advice[H2MI_EXPR_MAX_ADVICE];
  const void* fixed[H2MI_EXPR_MAX_FIXED];
  const void* instance;       /* instance column 0, or NULL; a circuit with several: h2mi_instance_cosets beside this struct (below) */
  uint32_t n_perm, chunk_len; /* chunk_len = cs.degree() - 2: any length */
  const void* perm_value[H2MI_FLEX_MAX_PERM];
  const void* perm_sigma[H2MI_FLEX_MAX_PERM];
  const void* perm_z[H2MI_FLEX_MAX_PERM];
  uint32_t n_lookups;
  const void* lookup_input[H2MI_FLEX_MAX_LOOKUPS];
  const void* lookup_input_b[H2MI_FLEX_MAX_LOOKUPS];
  const void* lookup_table[H2MI_FLEX_MAX_LOOKUPS];
  const void* lookup_permuted_input[H2MI_FLEX_MAX_LOOKUPS];
  const void* lookup_permuted_table[H2MI_FLEX_MAX_LOOKUPS];
  const void* lookup_z[H2MI_FLEX_MAX_LOOKUPS];
  const void* l0;
  const void* l_last;
  const void* l_active;
} h2mi_expr_cosets;
/* n_lookups | H2MI_LOOKUPS_LOGUP in an h2mi_expr_cosets: every lookup of the entry is a logUp argument.  lookup_permuted_input then holds
 * the multiplicity column M and lookup_z the running sum phi (extended-coset forms), lookup_permuted_table is not read (may be NULL),
 * and a lookup contributes three terms in the place of its five, Horner in y: l_0 phi, l_last phi, l_active ((phi(wX) - phi(X)) (A +
 * beta)(S + beta) - ((S + beta) - M (A + beta))); gamma is not read.  In a batch every entry states the same mode. */
#define H2MI_LOOKUPS_LOGUP 0x80000000u
/* Shuffle arguments of one circuit [RECALL halo2_proofs (PSE line) plonk/shuffle.rs, plonk/evaluation.rs — restated from memory, pinned
 * to DESIGN.md 4.5]: behind the circuit's lookup terms, per shuffle, l_0 (1 - z), l_last (z^2 - z), l_active (z(wX) (S + gamma) - z(X) (A +
 * gamma)), Horner in y; beta is not read.  input / shuffle: both sides compressed with theta on the extended coset
 * (h2mi_plonk_expr_compress_dev at domain_k = extended_k); z: the product's extended-coset form. */
#define H2MI_MAX_SHUFFLES 8
typedef struct {
  uint32_t n_shuffles;
  const void* input[H2MI_MAX_SHUFFLES];
  const void* shuffle[H2MI_MAX_SHUFFLES];
  const void* z[H2MI_MAX_SHUFFLES];
} h2mi_shuffle_cosets;
/* logUp lookups with SEVERAL INPUT SETS over one table [restated from memory, pinned to DESIGN.md 4.5 and tests/logup_sets_cases.py]:
 * per lookup the number K of input tuples, 1 .. H2MI_MAX_LOGUP_INPUTS.  lookup_input[l] then points at K CONSECUTIVE vectors (set j at
 * element j 2^extended_k), each compressed with theta, and the lookup's third term is l_active ((phi(wX) - phi(X)) D - N) with (N, D)
 * from the recurrence (N, D) = (-M, S + beta), then per input N <- N (A_j + beta) + D, D <- D (A_j + beta).  h2mi_expr_cosets keeps its
 * layout and the meaning of every field.  One struct holds for every circuit of a proof; counts beyond n_lookups are not read. */
typedef struct {
  uint32_t n_inputs[H2MI_FLEX_MAX_LOOKUPS];
} h2mi_logup_cosets;
/* The instance columns of one circuit (up to H2MI_MAX_INSTANCE: `meta.instance_column()` called more than once).  An H2MI_EXPR_INSTANCE
 * op carries the column's index as the advice and fixed queries do; the interpreter's pointer table holds instance column i behind the
 * advice and fixed columns, in slot H2MI_EXPR_MAX_ADVICE + H2MI_EXPR_MAX_FIXED + i.  A column the program does not read may be NULL. */
typedef struct {
  uint32_t n_instance;
  const void* column[H2MI_MAX_INSTANCE];
} h2mi_instance_cosets;
/* The circuits of one proof for the interpreting kernels.  circuits, gates: required.  The program, its constants and the challenges
 * are the proof's; an entry of `circuits` holds what belongs to one circuit (advice, instance, perm_value, perm_z, the six vectors of
 * each lookup).  What the circuits share — fixed, perm_sigma, l0, l_last, l_active — is stated in every entry: perm_sigma and the three
 * Lagrange cosets are read from entry 0 and must be the same pointers in the others; two entries may share any other pointer too (the
 * same advice twice is folded twice).
 *   shuffles    NULL (no shuffle: the same words as n_shuffles == 0 in every entry), or n_circuits entries with one n_shuffles
 *   logup       NULL (one input set per lookup: the same words as all ones), or one struct for the proof
 *   instances   NULL (circuits[i].instance is column 0 and the only one: the same words as {1, {circuits[i].instance}}), or n_circuits
 *               entries; circuits[i].instance is not read then
 *   challenges  n_challenges x 4 limbs, Montgomery, host, n_challenges <= H2MI_MAX_CHALLENGES; NULL with 0.  An H2MI_EXPR_CHALLENGE op
 *               pushes challenges[index] */
#define H2MI_MAX_CIRCUITS 8
typedef struct {
  const h2mi_expr_cosets* circuits;      uint32_t n_circuits;
  const h2mi_shuffle_cosets* shuffles;
  const h2mi_logup_cosets* logup;
  const h2mi_instance_cosets* instances;
  const h2mi_gate_program* gates;
  const uint64_t* challenges;            uint32_t n_challenges;
} h2mi_quotient_circuits;
/* The quotient of ONE circuit (k_evaluate_h_expr): n_circuits must be 1.  Terms in evaluate_h's order, Horner in y: the gate
 * polynomials, the permutation terms, the lookup terms, the shuffle terms; then the division by X^n - 1.  The column pointers, the
 * program, its constants and behind them the challenges (converted to the kernel's domain) travel in one device buffer written on
 * `stream`.
 * H2MI_EINVAL: a NULL record, a NULL required field or d_h_out; n_circuits != 1; a program that is malformed (unknown op, stack
 * underflow or deeper than H2MI_MAX_EXPR_STACK, not exactly one value at an END, no final END, empty), reads a NULL column, a constant
 * beyond n_constants, a challenge at or beyond n_challenges or an instance column at or beyond n_instance, or rotates by 2^k or more;
 * n_perm, n_lookups, n_shuffles, n_instance or n_challenges above its maximum; a NULL vector of a stated permutation column, lookup or
 * shuffle; a logUp count of 0 or above H2MI_MAX_LOGUP_INPUTS, or other than 1 without H2MI_LOOKUPS_LOGUP.  H2MI_ERANGE: the scalars'. */
int h2mi_plonk_evaluate_h_expr_dev(const h2mi_quotient_circuits* circuits, const h2mi_quotient_scalars* scalars, void* d_h_out,
                                   h2mi_stream_t stream);
/* The quotient of 1 .. H2MI_MAX_CIRCUITS circuits of one proof [RECALL halo2_proofs v2023_02_02 plonk/evaluation.rs evaluate_h]: ONE
 * accumulator walks circuits[0 .. n_circuits - 1] in order, per circuit acc = acc y + term over its gate polynomials, its permutation,
 * lookup and shuffle terms, and the division by X^n - 1 comes behind the last circuit — one launch and one pass over d_h_out whatever
 * n_circuits is.  The entries travel as consecutive records behind the program in the launch's one device buffer.  With n_circuits == 1
 * the words of d_h_out are those of h2mi_plonk_evaluate_h_expr_dev.
 * slice == H2MI_WHOLE_COSET: k_evaluate_h_expr_batch; every vector is an extended-coset evaluation.
 * 0 <= slice < rot = 2^(extended_k - k): k_evaluate_h_expr_slice, ONE COSET at a time (the quotient of a key made with
 * H2MI_KEYGEN_BY_COSET, include/h2mi_prover.h).  Extended-coset point slice + rot i is X = (zeta extended_omega^slice) omega^i, omega =
 * extended_omega^rot: the 2^extended_k evaluations of a polynomial of degree < 2^k are rot coset transforms of 2^k points, one per
 * shift.  Every column pointer of the record is then the 2^k-element slice `slice` of the extended-coset vector: element i the value at
 * extended-coset point slice + rot i, which for a column is h2mi_ntt_bn254_fr_oop_dev(coefficients, 2^k, out, k, omega, pre = zeta
 * extended_omega^slice).  A query at rotation r reads element (i + r) mod 2^k of the same slice; a compressed side is
 * h2mi_plonk_expr_compress_dev over the slices with domain_k = k; input set j of a logUp lookup lies j 2^k elements behind
 * lookup_input[l].  zeta, extended_omega and the rot values of t_inv stay the DOMAIN'S.  d_h_out is the whole vector of 2^extended_k
 * elements: the call writes elements slice + rot i, i < 2^k, each word for word what the whole-coset call stores there, and no other;
 * rot calls, one per slice, fill it.
 * H2MI_EINVAL: whatever the single call refuses, in any entry; n_circuits == 0 or > H2MI_MAX_CIRCUITS; entries that disagree in n_perm,
 * chunk_len, n_lookups or n_shuffles, or that name other sigma or Lagrange cosets than entry 0; slice < H2MI_WHOLE_COSET.
 * H2MI_ERANGE: the scalars'; slice >= rot. */
#define H2MI_WHOLE_COSET (-1)
int h2mi_plonk_evaluate_h_expr_batch_dev(const h2mi_quotient_circuits* circuits, const h2mi_quotient_scalars* scalars, int32_t slice, void* d_h_out,
                                         h2mi_stream_t stream);

/* The columns a program reads on one domain: the 2^k rows or the extended coset.  advice / fixed: n_advice <= H2MI_EXPR_MAX_ADVICE /
 * n_fixed <= H2MI_EXPR_MAX_FIXED column pointers (the arrays may be NULL with a count of 0; a column the program does not read may be
 * NULL); instances: the instance columns on the same points, whatever the struct's name says (NULL: none; one column: {1, {ptr}}, and
 * {1, {NULL}} for a program that reads none); program: required; challenges: as h2mi_quotient_circuits takes them; k: rotations are
 * modulo 2^k.  The same interpreter, the same uploader and the same refusals of a program as h2mi_plonk_evaluate_h_expr_dev. */
typedef struct {
  const void* const* advice; uint32_t n_advice;
  const void* const* fixed;  uint32_t n_fixed;
  const h2mi_instance_cosets* instances;
  const h2mi_gate_program* program;
  const uint64_t* challenges; uint32_t n_challenges;
  uint32_t k;
} h2mi_expr_columns;
/* A lookup's expressions compressed with theta (plonk/lookup/prover.rs compress_expressions): the program holds m polynomials e_0 ..
 * e_(m-1) and d_out[i] = sum_j e_j(i) theta^(m-1-j) — the fold acc theta + e_j — for the 2^domain_k points the columns are given on:
 * the Lagrange rows (domain_k = k) or the extended coset (domain_k = extended_k).  A query at rotation r reads point
 * (i + (r mod 2^k) 2^(domain_k-k)) mod 2^domain_k.  d_out must not be one of the columns.  Values are stored fully reduced, Montgomery.
 * H2MI_EINVAL: a NULL record, program, theta or d_out; H2MI_ERANGE: k == 0, domain_k < k, domain_k - k > 4, domain_k > H2MI_MAX_LOG_N. */
int h2mi_plonk_expr_compress_dev(const h2mi_expr_columns* columns, uint32_t domain_k, const uint64_t theta[4], void* d_out, h2mi_stream_t stream);

/* ---- the witness check on the rows (what MockProver::run(..).assert_satisfied() answers on the host): does a witness satisfy the
 * circuit, and where not?  Three calls over Lagrange-row columns; each returns when its report is on the host.  h2mi_prover_check
 * (h2mi_prover.h) runs them on the columns of a proof in flight.
 * Polynomials: the program holds n polynomials (columns on the 2^k rows, rotations modulo 2^k).  report_out receives, per polynomial in
 * program order, {the number of rows i < n_rows on which it is not zero modulo r, the smallest such row or 0xffffffff}: 2 uint32 per
 * polynomial, HOST memory, room for every END of the program; n_polys_out (may be NULL) their number.  n_rows in [1, 2^k]: rows at or
 * beyond it are not tested but are read by rotations.  A satisfied witness costs no atomic operation.
 * H2MI_EINVAL: a NULL record, program or report_out; H2MI_ERANGE: k == 0, k > H2MI_MAX_LOG_N, n_rows out of range. */
int h2mi_plonk_expr_check_dev(const h2mi_expr_columns* columns, uint32_t n_rows, uint32_t* report_out /* host, n_polys x 2 */, uint32_t* n_polys_out,
                              h2mi_stream_t stream);
/* Copy constraints: d_cells holds n_cells x 4 uint32 in DEVICE memory, {column, row, image column, image row} per cell that the
 * permutation moves, columns as indices into d_values (m <= H2MI_FLEX_MAX_PERM Lagrange-row columns, the permutation argument's order)
 * — trusted like the active rows of h2mi_plonk_permutation_products_sparse_dev: every column below m, every row inside its column.
 * report_out (host) = {cells whose value differs from their image's, the smallest index of such a cell in d_cells or 0xffffffff}. */
int h2mi_plonk_copy_check_dev(const void* const* d_values, uint32_t m, const void* d_cells, uint32_t n_cells, uint32_t report_out[2],
                              h2mi_stream_t stream);
/* Lookup membership: report_out (host) = {rows i < usable_rows whose d_input[i] (Montgomery) is none of the n_unique ascending
 * canonical values of d_table_sorted (h2mi_fr_sort_unique_dev's first output, or a key's table), the smallest such row or 0xffffffff}.
 * h2mi_plonk_lookup_permute_dev counts the same rows but cannot say which. */
int h2mi_plonk_lookup_member_dev(const void* d_input, const void* d_table_sorted, uint32_t n_unique, uint32_t usable_rows, uint32_t report_out[2],
                                 h2mi_stream_t stream);
/* Shuffle multiplicities: both sides sorted by h2mi_fr_sort_unique_dev (ascending canonical distinct values and their u32
 * multiplicities).  report_out (host) = {rows i < usable_rows whose d_input[i] (Montgomery) occurs more often among the inputs than on
 * the shuffle side — not at all included —, the smallest such row or 0xffffffff}.  Both sides hold usable_rows values, so unequal
 * multisets always report at least one row. */
int h2mi_plonk_shuffle_member_dev(const void* d_input, const void* d_input_sorted, const void* d_input_mult, uint32_t n_input_unique,
                                  const void* d_shuffle_sorted, const void* d_shuffle_mult, uint32_t n_shuffle_unique, uint32_t usable_rows,
                                  uint32_t report_out[2], h2mi_stream_t stream);

/* ---- SRS generation helper: ParamsKZG::setup's g[i] = s_i * G   ------------------
 * d_scalars: n Fr (Montgomery).  d_out_affine: n G1Affine.  Fixed-base windowed multiplication of the
 * generator (1, 2) with on-device normalisation. */
int h2mi_g1_fixed_base_mul_dev(const void* d_scalars, size_t n, void* d_out_affine, h2mi_stream_t stream);
/* out[i] = base^i for i < n (the powers-of-s vector of ParamsKZG::setup), Montgomery in and out */
int h2mi_fr_powers_dev(void* d_out, size_t n, const uint64_t base[4], h2mi_stream_t stream);
/* halo2_proofs::arithmetic::best_fft for G = bn256::G1 — the group-valued transform ParamsKZG::setup runs over the monomial SRS to get
 * the Lagrange one (reference examples/standard_plonk.rs:29; `best_fft(&mut g_lagrange_projective, root.invert(), k)` then a scaling by
 * n^-1): out[i] = post_scale * sum_j omega^(i j) * in[j], natural order in and out.  Points are G1Affine on both sides (n x 64 B, (0, 0) =
 * identity); in place allowed.  omega: a 2^log_n-th root of unity; post_scale (Montgomery) may be NULL.  Every butterfly multiplies a
 * point by a 254-bit twiddle, so the cost is (n / 2) log n scalar multiplications (seconds at DEGREE 20 - 22, where the crate takes
 * minutes): keygen-time work.  Uses 144 B x n of scratch for the call and synchronises `stream` before returning.  log_n <= 26. */
int h2mi_fft_bn254_g1_dev(const void* d_affine_in, void* d_affine_out, uint32_t log_n, const uint64_t omega[4], const uint64_t* post_scale_or_null,
                          h2mi_stream_t stream);

/* ---- wire encodings: what create_proof writes to the transcript (reference call sites:
 * Blake2bWrite::init / finalize around create_proof, examples/standard_plonk.rs:40-50 and src/scaffold.rs:190-200,
 * 321-332; Blake2bRead::init for verify_proof, examples/standard_plonk.rs:56, src/scaffold.rs:221,352) and what
 * ParamsKZG::{write,read} keep on disk (the SRS the scaffold obtains through gen_srs, src/scaffold.rs:119,174,271,
 * cached under params/, .gitignore:17-18).  Conventions restated from halo2curves 0.3.x [RECALL, see
 * csrc/h2mi_serde.hip]: field elements as 32 little-endian canonical bytes (Fr::to_repr); G1Affine as 32
 * bytes = x with flags in byte 31 (0x40: y odd, 0x80: point at infinity).  field: 0 = Fq, 1 = Fr.
 * The *_from_* / decompress forms report the number of invalid encodings (>= modulus, not on the curve,
 * inconsistent flags) through invalid_out — such entries decode to zero / the identity — and synchronise. */
int h2mi_fe_to_repr_dev(int field, const void* d_in, size_t n, void* d_out32, h2mi_stream_t stream);
int h2mi_fe_from_repr_dev(int field, const void* d_in32, size_t n, void* d_out, uint64_t* invalid_out);
int h2mi_g1_compress_dev(const void* d_affine, size_t n, void* d_out32, h2mi_stream_t stream);
int h2mi_g1_decompress_dev(const void* d_in32, size_t n, void* d_affine_out, uint64_t* invalid_out);
/* host-pointer forms (synchronous): G1Affine::to_bytes / from_bytes over n points */
int h2mi_g1_compress(const uint64_t* affine /* n*8 */, size_t n, uint8_t* out32 /* n*32 */);
int h2mi_g1_decompress(const uint8_t* in32 /* n*32 */, size_t n, uint64_t* affine_out /* n*8 */, uint64_t* invalid_out);

/* ---- profiling: per-kernel device time measured with HIP events on the launching stream ---------- */
int h2mi_profile_enable(int on);         /* 1 = record events around every kernel launch */
/* restrict event recording to kernels whose name starts with `prefix` (NULL or "" = all kernels) */
int h2mi_profile_filter(const char* prefix);
int h2mi_profile_reset(void);
/* total milliseconds and launch count for kernels whose name starts with `prefix`; synchronises */
int h2mi_profile_query(const char* prefix, double* total_ms, uint64_t* launches);
/* every recorded launch in order, one text line each: "<kernel> <start ms after the first recorded launch> <duration ms>";
 * needed_out (may be NULL) receives the buffer size the full text needs; synchronises */
int h2mi_profile_dump(char* buf, size_t cap, size_t* needed_out);

#ifdef __cplusplus
}
#endif
#endif /* H2MI_H */
