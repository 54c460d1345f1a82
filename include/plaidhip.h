/* plaidhip.h -- C ABI of the MI355X-native gene-set scoring hot path.
 *
 * Drop-in boundary for the R package bigomics/plaid (reference @ 2025-06-14).  The
 * reference has NO native interface (NAMESPACE:1-16 has no useDynLib, there is no src/);
 * the seam is therefore inside the R functions named below, whose BODIES are replaced by
 * `.Call()` into this library while their R signatures stay (see INTEGRATION.md and
 * r-pkg/).  Every entry point cites the reference code it replaces.
 *
 * Conventions
 *   - plain C, no R / torch / HIP types in any signature; `void*` device pointers.
 *   - matrices use R layout: column-major `double`; sparse = dgCMatrix slots
 *     (`p` int32[ncol+1], `i` int32[nnz] 0-based sorted, `x` double[nnz]).
 *   - every function returns a status code (0 = ok); the text of the last error of the
 *     calling thread is available from plaidhip_last_error_string().  Nothing throws.
 *   - element offsets are 64-bit: m*n may exceed 2^31-1 (the reason R/plaid.R:103-104
 *     chunks).
 *   - `host` entry points take caller-owned host buffers, stage them through HBM and
 *     synchronise before returning (R's .Call contract).  `dev` entry points take
 *     device pointers, enqueue on the context's stream and do NOT synchronise.
 */
#ifndef PLAIDHIP_H
#define PLAIDHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLAIDHIP_VERSION 200 /* 0.2.0 */

enum plaidhip_status {
  PLAIDHIP_OK = 0,
  PLAIDHIP_EINVAL = 1,       /* bad dimensions / arguments (R: stop())            */
  PLAIDHIP_ENOMEM = 2,       /* device or host allocation failed                  */
  PLAIDHIP_EHIP = 3,         /* a HIP runtime call or kernel failed               */
  PLAIDHIP_EUNSUPPORTED = 4, /* shape outside what the kernels cover              */
  PLAIDHIP_ENODEVICE = 5     /* no gfx950 device visible                          */
};

enum plaidhip_stat { PLAIDHIP_STAT_MEAN = 0, PLAIDHIP_STAT_SUM = 1 }; /* R/plaid.R:60 `stats` */
enum plaidhip_ties {                                                   /* R/plaid.R:593 `ties.method` */
  PLAIDHIP_TIES_AVERAGE = 0,
  PLAIDHIP_TIES_MIN = 1,
  PLAIDHIP_TIES_MAX = 2,
  /* passed through like the reference does (R/plaid.R:614-617 -> matrixStats::colRanks; :639-642 -> base::rank): ties in
   * order of their position / reverse position / without gaps ("dense": dense columns only, as in matrixStats).  Composed
   * from two or three passes of the min-rank kernels: exact, off the hot path, no fused power / column maximum, and the
   * CSC form reads Xp[n] back (not stream-ordered).                                                                     */
  PLAIDHIP_TIES_FIRST = 3,
  PLAIDHIP_TIES_LAST = 4,
  PLAIDHIP_TIES_DENSE = 5,
  PLAIDHIP_TIES_RANDOM = 6 /* legal in R, REFUSED here (PLAIDHIP_EUNSUPPORTED): not a function of the input */
};
enum plaidhip_ignore_zero { /* R/plaid.R:554 `ignore.zero`: NULL / FALSE / TRUE */
  PLAIDHIP_IGNORE_ZERO_AUTO = -1,
  PLAIDHIP_IGNORE_ZERO_FALSE = 0,
  PLAIDHIP_IGNORE_ZERO_TRUE = 1
};

/* `flags` arguments are device arrays of 4 uint32 words set to 0/1 by the SpMM epilogue /
 * plaidhip_dev_minflags (the caller zeroes them first): [0] a value < 0 was seen, [1] an exact
 * zero, [2] a NaN, [3] reserved (never written by the product library).  0/1 words so that a sample-sharded host can all-reduce(MAX)
 * them in place.  min(x, na.rm=TRUE) == 0  <=>  flags[1] && !flags[0]   (R/plaid.R:556-557).
 * The PLAIDHIP_FLAG_* bits are the in-kernel encoding (bit b <-> word b).                    */
#define PLAIDHIP_FLAG_HAS_NEG 1u
#define PLAIDHIP_FLAG_HAS_ZERO 2u
#define PLAIDHIP_FLAG_HAS_NAN 4u

typedef struct plaidhip_ctx plaidhip_ctx;         /* device, stream, workspace           */
typedef struct plaidhip_geneset plaidhip_geneset; /* device-resident prepared membership */

/* ---- lifecycle --------------------------------------------------------------------- */
int plaidhip_version(void);
const char* plaidhip_last_error_string(void);
int plaidhip_device_count(int* count);
/* `stream`: an existing hipStream_t to enqueue on (e.g. the host framework's current
 * stream) or NULL to create a private one. */
int plaidhip_init(int device, void* stream, plaidhip_ctx** out);
int plaidhip_finalize(plaidhip_ctx* ctx);
int plaidhip_synchronize(plaidhip_ctx* ctx);
/* Precision of the dense crossprod.  PLAIDHIP_PRECISION_F64 (default): fp64 storage and accumulation,
 * scores agree with the reference to ~1e-15.  PLAIDHIP_PRECISION_MIXED (opt-in): the sample columns are
 * staged as fp32 (2^-24 relative rounding of the inputs, ~6e-8 on the scores, inside the 1e-5 bar).
 * The sums are NOT fp64 throughout: the eight values a lane gathers per chunk are added as two four-term
 * fp32 partial sums, (v0 + v1) + (v2 + v3), and only those partials are accumulated in fp64.  For a set
 * of k genes with mag = sum |x| every raw sum is within
 *   3 * 2^-24 * (1 + 2^-22) * mag  +  (k + c) * 2^-53 * mag  +  k * 2^-149
 * of the exact sum (cast 2^-24, four-term fp32 sum 2 * 2^-24, the fp64 accumulation and the c roundings
 * of the epilogue, values below the fp32 normal range); tests/helpers/compact_ref.py derives it and
 * tests/test_gpu_compact_staging.py holds the kernel to it, cancelling data included.  The cast is the
 * IEEE one: NaN and +-Inf propagate to exactly the scores of their sets (flag words as in fp64), a
 * finite |x| >= 2^128 (1e39) becomes +-Inf in its sets, and |x| <= 2^-150 (1e-46) contributes 0.
 * Applies to dense X with 8,192 < genes <= 20,448, everything else keeps fp64.                        */
enum { PLAIDHIP_PRECISION_F64 = 0, PLAIDHIP_PRECISION_MIXED = 1 };
int plaidhip_set_precision(plaidhip_ctx* ctx, int mode);
/* Enqueue on `stream` (a hipStream_t) from now on; NULL means the device's null stream, e.g. the
 * default stream of a host framework (plaidhip_init treats NULL as "create a private stream", so a
 * caller that wants the null stream says so here).  A private stream created by init is destroyed. */
int plaidhip_set_stream(plaidhip_ctx* ctx, void* stream);
/* Kernel-selection knobs of one context (tests and tools use them to pin a path; the defaults choose
 * by shape).  Unknown option or value: PLAIDHIP_EINVAL.                                              */
enum plaidhip_option {
  PLAIDHIP_OPT_SPMM_DENSE_KERNEL = 1,  /* 0 auto (default) | 1 one-column kernel | 2 pair kernel wherever it applies |
                                          3 dense 0/1 G x bf16x3 split of X on MFMA (BASELINE config 4's "GEMM" form:
                                          ~145x the flops of the SpMM; measured beside it, never default).  NOT fp64 sums:
                                          each value is split into three bf16 terms (24 significant bits) and summed in
                                          fp32 on the matrix cores.  For a set of k nonzero terms with mag = sum |x| every
                                          raw sum is within
                                            3 k 2^-23 mag  +  (k + c) 2^-53 mag  +  3 k 2^-126
                                          of the exact sum (3 k fp32 additions of one ulp each, the split's 2^-24 inside
                                          them; the c fp64 roundings of the epilogue; fp32 / bf16 subnormals, which may be
                                          flushed); tests/helpers/mfma_ref.py derives it, tests/test_gpu_mfma.py holds the
                                          kernels to it.  Range: the fp32 sums overflow to +-Inf where a partial sum
                                          passes 3.4e38, so sum |x| over a set has to stay below 2^127.  NaN and +-Inf
                                          reach exactly the scores of the sets that hold their gene, as on the fp64
                                          kernels (flag words included; +Inf and -Inf in one set give NaN): they, and a
                                          finite |x| >= (2 - 2^-8) 2^127 = 3.39e38 whose bf16 head would be Inf, never
                                          enter the matrix core but are added to their sets' scores in fp64 by a kernel
                                          enqueued behind it -- such a finite value counts as the fp64 number it is, not
                                          as Inf.  No host synchronisation is added: the call stays capturable.
                                          Every dense scorer entry of the context takes this route while it is set |
                                          4 as 0, but the pair kernel always in its 1,024-thread form with the slice
                                          partial sums in a scratch, also where the collection qualifies for the
                                          768-thread form that keeps them in registers (more than 10,224 genes and at most
                                          6,144 sets): the same scores bit for bit; tests and A/B runs compare the two  */
  PLAIDHIP_OPT_SPMM_SPARSE_KERNEL = 2, /* 0 auto: by nnz(X) (default) | 1 scatter | 2 gather                        */
  PLAIDHIP_OPT_NT_STORE = 3,           /* -1 auto (default) | 0 plain stores of S | 1 streaming stores              */
  PLAIDHIP_OPT_RANKS_F32 = 4,          /* staging of RANK inputs in the crossprod, all three exact and bit-identical:
                                          2 (default) u16 (2 * rank), four samples per LDS entry, integer sums |
                                          1 fp32 staging | 0 the fp64 kernels                                        */
  PLAIDHIP_OPT_RANK_KERNEL = 5,        /* 0 auto (default) | 1 sorting network | 2 bucket ranker | 3 bucket ranker with
                                          512 threads x 40 keys for columns beyond 12,288 keys (default: 1,024 x 20)  */
  PLAIDHIP_OPT_SCATTER_FIXED = 6,      /* sparse-X scatter kernel, inputs declared bounded (rank weights): 1 (default) u64
                                          fixed-point accumulators: exact integer sums, bit-reproducible | 0 fp64 atomics  */
  PLAIDHIP_OPT_SCATTER_ORDER = 7,      /* sparse-X scatter kernel: 1 (default) all workgroups on one chunk of sets at a
                                          time (chunk, column order) | 0 column after column                              */
  PLAIDHIP_OPT_FUSED_MEDIANS = 8       /* plaidhip_dev_spmm_csc_fused_f64 and the host pipelines on a dgCMatrix: medians
                                          selected inside the crossprod launch 0 (default) from 1e9 scores on | 1 whenever
                                          the shapes allow | 2 never                                                      */
};
int plaidhip_set_option(plaidhip_ctx* ctx, int option, int value);
/* Size limits of the kernels a host has to route by (so that no binding repeats them as literals).  Unknown `which`:
 * PLAIDHIP_EINVAL.                                                                                                   */
enum plaidhip_limit_id {
  PLAIDHIP_LIMIT_SPARSE_RANK_COLUMN = 1, /* most stored values of a column plaidhip_dev_colranks_csc_dense_nz_f64 takes     */
  PLAIDHIP_LIMIT_LDS_GENES = 2           /* most genes the one-slice LDS-resident crossprod kernels take (u16 rank staging) */
};
int plaidhip_limit(int which, int64_t* value);
/* device memory helpers for hosts without a tensor library (R) */
int plaidhip_malloc(plaidhip_ctx* ctx, size_t bytes, void** dptr);
int plaidhip_free(plaidhip_ctx* ctx, void* dptr);
int plaidhip_memcpy_h2d(plaidhip_ctx* ctx, void* dst, const void* src, size_t bytes);
int plaidhip_memcpy_d2h(plaidhip_ctx* ctx, void* dst, const void* src, size_t bytes);

/* ---- gene-set membership G (replaces R/plaid.R:72-77 on `gmt2mat()` output,
 *      R/gmt-utils.R:19-66).  The caller passes the CSC pattern of the ALIGNED,
 *      binarised membership: column j lists the rows OF X (0-based, < g) that belong to
 *      set j, i.e. `matG[gg,] != 0` re-indexed into X's row space (R/plaid.R:65-73) --
 *      X itself is never row-gathered.  Explicit zeros must already be dropped.
 *      Set sizes (colSums(G), R/plaid.R:75) are the column lengths.
 *      A prepared gene-set collection is reused for every sample, chunk and call, but it owns
 *      per-launch device scratch: use it from ONE stream at a time (one per context is free). */
int plaidhip_geneset_create(plaidhip_ctx* ctx, int32_t g, int32_t m, const int32_t* Gp,
                            const int32_t* Gi, plaidhip_geneset** out);
int plaidhip_geneset_destroy(plaidhip_geneset* gs);
/* info[0]=g info[1]=m info[2]=z (nnz) info[3]=padded index slots info[4]=tiles
 * info[5]=1 if the LDS-resident column kernel is usable for f64 at this g             */
int plaidhip_geneset_info(const plaidhip_geneset* gs, int64_t info[8]);

/* ---- device-level hot path (pointers are device pointers) --------------------------- */

/* S = alpha * (G^T X) (.) w + beta * (k (.) w):  the crossprod of R/plaid.R:80,107 with
 * the column scaling of R/plaid.R:74-77 folded into the epilogue.  w_j = 1/(1e-8 + k_j)
 * for STAT_MEAN, 1 for STAT_SUM; k_j = size of set j.  alpha=1, beta=0 is plaid() itself;
 * (alpha, beta) = (1/nrow(X), -0.5) applied to raw ranks is replaid.sing (R/plaid.R:216),
 * (1/max(rX), -0.5) is replaid.ssgsea (R/plaid.R:251) -- by linearity of the crossprod.
 * X: g x n column-major, leading dimension ldx; S: m x n column-major, leading dim lds.
 * `alpha_div` (device double*, may be NULL): alpha is divided by *alpha_div on the device, so
 * the global max(rX) never visits the host.  `flags` (device uint32[4], may be NULL): see above. */
int plaidhip_dev_spmm_dense_f64(plaidhip_ctx* ctx, const plaidhip_geneset* gs, const void* X,
                                int64_t ldx, int32_t n, int stat, double alpha, const void* alpha_div,
                                double beta, void* S, int64_t lds, void* flags);
/* The same crossprod for an X that holds RANKS -- exactly what plaidhip_dev_colranks_dense_f64 writes with power = 1 and
 * is_signed = 0 (half-integers in [0.5, nrow(X)]), or such ranks after replaid.ucell's max - rank / pmin map: the rank
 * matrix of replaid.sing (R/plaid.R:215-217), replaid.ssgsea(alpha = 0) (:245-253), replaid.ucell (:277-279).  2 * rank
 * is staged as u16 (four sample columns per 8-byte LDS entry) and summed in integers: exact, order-independent and
 * bit-identical to plaidhip_dev_spmm_dense_f64 on the same input, at a quarter of its LDS bytes per score.  The launch is
 * speculative: a value that is not such a rank (NaN -- matrixStats::colRanks keeps NA --, +-Inf, a negative value, a double
 * >= 32,768, a value that is not a multiple of 1/2) is seen while staging, in whichever column of whichever pass, and the
 * fp64 kernel enqueued right behind it on the same stream then recomputes the scores (it returns at once otherwise), so
 * the result is plaidhip_dev_spmm_dense_f64's for ANY input, NaN propagation included.  Shapes the u16 kernel does not take (nrow(X) <= 8,192 or > 20,448) run the general kernels.             */
int plaidhip_dev_spmm_ranks_f64(plaidhip_ctx* ctx, const plaidhip_geneset* gs, const void* R,
                                int64_t ldr, int32_t n, int stat, double alpha, const void* alpha_div,
                                double beta, void* S, int64_t lds, void* flags);
/* same with X as CSC (dgCMatrix) -- sparse branch of Matrix::crossprod at R/plaid.R:107.
 * `nnz`: number of stored values of X when the caller knows it (Xp[n] on the host), else -1.  It picks
 * the kernel: sparse-aware scatter below 12.5 % stored values, column gather above; with -1 both are
 * enqueued and the one that does not apply returns at once (the value is then read on the device).
 * nnz is a hint only: what the kernels read is Xx[Xp[0] .. Xp[n]).
 * The scatter kernel sums in u64 fixed point -- scores that do not depend on the order in which its LDS atomics arrive,
 * bit-identical from run to run -- when a sweep over the stored values finds them all finite and >= 0 AND their dynamic
 * range small enough for every score to stay within 2^-40 (9.1e-13) relative of the exact sum: each value is rounded once
 * to a grid of 2^-(e+1) <= 2^-40 x (smallest stored value > 0), e = 63 bits minus those of the largest possible sum
 * ((largest set size) x (largest value), or -- where that is too coarse -- the largest sum of a column's values).  Anything else (a negative, NaN or infinite value, raw
 * counts next to values near 1, one huge outlier) takes fp64 atomics.  Decided on the device; both launches are enqueued. */
int plaidhip_dev_spmm_csc_f64(plaidhip_ctx* ctx, const plaidhip_geneset* gs, const void* Xp,
                              const void* Xi, const void* Xx, int32_t n, int64_t nnz, int stat, double alpha,
                              const void* alpha_div, double beta, void* S, int64_t lds, void* flags);

/* The sparse crossprod for RANK WEIGHTS: Rx is what plaidhip_dev_colranks_csc_f64 wrote (rank^power of the stored values,
 * so 0 <= Rx <= *rmax, rmax = their maximum on the device -- the max(rX) replaid.ssgsea divides by, R/plaid.R:251: alpha is
 * divided by it as by alpha_div).  The fixed-point grid of the scatter kernel then follows *rmax -- the maximum over the
 * WHOLE matrix -- so while the first bound applies ((largest set size) x *rmax: collections whose largest set has at most
 * 1,024 genes) every shard of a sharded call rounds alike and the scores do not depend on the sharding.  Collections with a
 * larger set fall back to the bound from the largest column sum OF THE SHARD (and the fixed-point / fp64 choice looks at the
 * shard's own smallest value): there the scores of different shardings agree to 2^-40 relative, not bit for bit.  Same
 * device-side guard as plaidhip_dev_spmm_csc_f64: a stored value outside [0, *rmax], a NaN (the rank weight of a NaN
 * input) or too wide a dynamic range takes the fp64 accumulators, which propagate it as the reference does.  rmax is
 * required.                                                                                                          */
int plaidhip_dev_spmm_csc_ranks_f64(plaidhip_ctx* ctx, const plaidhip_geneset* gs, const void* Xp,
                                    const void* Xi, const void* Rx, int32_t n, int64_t nnz, int stat, double alpha,
                                    const void* rmax, double beta, void* S, int64_t lds, void* flags);

/* chunked_crossprod(x, y) = t(x) %*% y (R/plaid.R:100-123, Matrix::crossprod at :107 / :117) for a GENERAL sparse x: the
 * stored values of x (@x) may differ inside a column -- signed or weighted gene sets -- which the prepared membership
 * of plaidhip_geneset_create cannot express.  x stays in its dgCMatrix slots (device pointers Wp: m + 1, Wi / Wx: Wp[m];
 * g rows, m columns); y is g x n dense (leading dimension ldy); S: m x n, leading dimension lds.  Every stored entry of x
 * is multiplied, explicit zeros included (0 * NaN is NaN, as in Matrix::crossprod); sums are fp64 in an order that
 * differs from a sequential one (16 partial sums per column of x).  plaid() itself never needs this entry: it builds
 * the column-scaled 0/1 matrix (:73-77), the path plaidhip_dev_spmm_dense_f64 is made for.                          */
int plaidhip_dev_crossprod_weighted_f64(plaidhip_ctx* ctx, const void* Wp, const void* Wi, const void* Wx, int32_t g,
                                        int32_t m, const void* Y, int64_t ldy, int32_t n, void* S, int64_t lds);
/* same with y a dgCMatrix (device pointers Yp: n + 1, Yi / Yx); S is dense                                           */
int plaidhip_dev_crossprod_weighted_csc_f64(plaidhip_ctx* ctx, const void* Wp, const void* Wi, const void* Wx, int32_t g,
                                            int32_t m, const void* Yp, const void* Yi, const void* Yx, int32_t n,
                                            void* S, int64_t lds);

/* colranks(), dense branch: t(matrixStats::colRanks(as.matrix(X), ties.method))
 * (R/plaid.R:611-619); `is_signed` = sign(X)*rank(|X|) (R/plaid.R:612-615).  Optional fused
 * power transform rank^power (R/plaid.R:249, power = 1+alpha; pass 1.0 for none).
 * R: g x n doubles (same layout as X).  colmax (device double[n], may be NULL) receives the
 * per-column maximum of the written values (feeds max(rX), R/plaid.R:251).              */
int plaidhip_dev_colranks_dense_f64(plaidhip_ctx* ctx, const void* X, int64_t ldx, int32_t g,
                                    int32_t n, int ties, int is_signed, double power, void* R,
                                    int64_t ldr, void* colmax);
/* sparse_colranks() (R/plaid.R:631-650): ranks of the stored non-zeros of each CSC column
 * among themselves; only @x is produced, pattern unchanged (R/plaid.R:645-646).          */
/* `max_col_nnz`: an upper bound on the number of stored values of any column (it sizes the workgroups
 * and their LDS; the number of rows of X is always valid, a tight bound is faster).  The call is
 * stream-ordered like every dev entry point: nothing is read back to size the launch.               */
int plaidhip_dev_colranks_csc_f64(plaidhip_ctx* ctx, const void* Xp, const void* Xx, int32_t n,
                                  int32_t max_col_nnz, int ties, int is_signed, double power, void* Rx,
                                  void* colmax);

/* colranks() on a dgCMatrix WITHOUT keep.zero (R/plaid.R:602-609 -> sparseMatrixStats::colRanks):
 * the zeros are ranked too and the result is DENSE g x n -- same numbers as the dense branch on
 * the densified matrix, computed from the CSC arrays on the device.                        */
int plaidhip_dev_colranks_csc_dense_f64(plaidhip_ctx* ctx, const void* Xp, const void* Xi, const void* Xx,
                                        int32_t g, int32_t n, int ties, int is_signed, double power,
                                        void* R, int64_t ldr, void* colmax);

/* The same dense ranks WITHOUT densifying the column: all zeros of a sparse column tie, so its dense ranks follow from the
 * ranks among the stored values (the sparse_colranks kernel) and the counts of negative and zero entries -- O(nnz) work plus
 * one dense write, for any nrow(X) (the densify-and-rank route leaves the fast rank kernel beyond 20,352 rows; a 10x
 * Genomics matrix has 33,538 or 36,601).  max_col_nnz: the longest column's stored values (<= 20,352, else EUNSUPPORTED);
 * Rx_scratch: Xp[n] doubles of device scratch.  Results are identical to plaidhip_dev_colranks_csc_dense_f64.          */
int plaidhip_dev_colranks_csc_dense_nz_f64(plaidhip_ctx* ctx, const void* Xp, const void* Xi, const void* Xx, int32_t g,
                                           int32_t n, int32_t max_col_nnz, int ties, int is_signed, double power,
                                           void* Rx_scratch, void* R, int64_t ldr, void* colmax);

/* replaid.ssgsea.exact's operand pass (kernels_walk.hip), stream-ordered, no read-back.  For the g x n columns of X (dense,
 * leading dimension ldx) it writes Q = rank(x, ties = "last") -- bit-identical to plaidhip_dev_colranks_dense_f64 with
 * PLAIDHIP_TIES_LAST -- and, when alpha != 0, W = rank(x, "average")^alpha and P = W * Q (leading dimension ldq).  W is
 * bit-identical to plaidhip_dev_colranks_dense_f64(PLAIDHIP_TIES_AVERAGE, power = alpha) wherever that call takes the
 * bucket or partitioned ranker (columns of more than 256 genes; a clustered column the bucket ranker hands to the sorting
 * network gets pow() there and 1/4-step roots here: each within its allowance of the exact power -- 3 u = 3 * 2^-53
 * relative for pow(), 0 to 5.5 u for the roots by the count in rank_bucket.h -- so at most 8.5 u apart).  colnan: n uint32, 1 for a column holding a NaN.
 * Two rank passes (average ranks, then min ranks of (2 r - 1) 2^26 + (g - 1 - i)); scratch: 2 ldq n doubles; g < 2^26. */
int plaidhip_dev_ssgsea_exact_operands_f64(plaidhip_ctx* ctx, const void* X, int64_t ldx, int32_t g, int32_t n, double alpha,
                                           void* Q, void* W, void* P, int64_t ldq, void* scratch, void* colnan);
/* the same for a dgCMatrix (device slots; rows increasing inside each column), with the results of its dense form: the
 * zeros are ranked, implicit zeros take their q from their row order inside the zero tie group.  nnz = Xp[n], max_col_nnz
 * the longest column (as for plaidhip_dev_colranks_csc_f64); scratch: 3 nnz doubles.  Two rank passes over the stored
 * values, then one dense write of Q (and W, P).                                                                        */
int plaidhip_dev_ssgsea_exact_operands_csc_f64(plaidhip_ctx* ctx, const void* Xp, const void* Xi, const void* Xx, int32_t g,
                                               int32_t n, int32_t max_col_nnz, int64_t nnz, double alpha, void* Q, void* W,
                                               void* P, int64_t ldq, void* scratch, void* colnan);

/* The walk of plaidhip_ssgsea_exact_ks on operands already on the device (what plaidhip_dev_ssgsea_exact_operands*_f64
 * wrote: Q, W with leading dimension ldq, colnan), stream-ordered, no read-back.  Gp (m + 1) / Gi (Gp[m]) are DEVICE
 * copies of the aligned pattern (row indices in 0..g-1, distinct inside a set).  W is not read at alpha = 0 and may be
 * NULL then.  S: m x n fp64, leading dimension lds; no norm (the caller divides).  For alpha != 0 the column's weights
 * are first scattered into walk order, into g n doubles of the context's workspace.  g <= PLAIDHIP_GSEA_KS_MAX_GENES,
 * else PLAIDHIP_EUNSUPPORTED with nothing launched.                                                                    */
int plaidhip_dev_gsea_ks_f64(plaidhip_ctx* ctx, const void* Q, const void* W, int64_t ldq, const void* colnan, int32_t g,
                             int32_t n, const void* Gp, const void* Gi, int32_t m, double alpha, int scale, void* S,
                             int64_t lds);

/* The walk of plaidhip_gsva_exact on last ranks already on the device (Q of plaidhip_dev_ssgsea_exact_operands*_f64 with
 * alpha = 0, applied to the row-transformed matrix v; colnan from the same call), stream-ordered, no read-back.  Gp / Gi
 * are DEVICE copies of the aligned pattern.  S: m x n fp64, leading dimension lds.  For tau != 0 the weight table (g
 * doubles) is built in the context's workspace first.  g <= PLAIDHIP_GSEA_KS_MAX_GENES, else PLAIDHIP_EUNSUPPORTED with
 * nothing launched.                                                                                                    */
int plaidhip_dev_gsva_ks_f64(plaidhip_ctx* ctx, const void* Q, int64_t ldq, const void* colnan, int32_t g, int32_t n,
                             const void* Gp, const void* Gi, int32_t m, double tau, int max_diff, void* S, int64_t lds);

/* The dispersion of plaidhip_sing_exact on ranks already on the device, stream-ordered, no read-back.  R: the min ranks of
 * the columns (plaidhip_dev_colranks_dense_f64, ties "min"), Q: their last ranks and colnan (plaidhip_dev_ssgsea_exact_
 * operands*_f64 with alpha = 0), both g x n fp64 with leading dimension ldq.  Gp / Gi are DEVICE copies of the aligned
 * pattern.  S: m x n fp64, leading dimension lds.  The ranks by position (g n u32) are built in the context's workspace
 * first.  g <= PLAIDHIP_GSEA_KS_MAX_GENES, else PLAIDHIP_EUNSUPPORTED with nothing launched.                              */
int plaidhip_dev_sing_mad_f64(plaidhip_ctx* ctx, const void* R, const void* Q, int64_t ldq, const void* colnan, int32_t g,
                              int32_t n, const void* Gp, const void* Gi, int32_t m, void* S, int64_t lds);

/* normalize_medians() (R/plaid.R:554-575) in three phases so that a sample-sharded host
 * can all-reduce between them:
 *   1. flags  : plaidhip_dev_minflags   (or the SpMM epilogue's `flags`)  -> ignore.zero
 *   2. medians: plaidhip_dev_col_medians  (zeros masked when ignore_zero, all-masked
 *               column -> 0, R/plaid.R:561-566).  ignore_zero = 0 / 1, or -1 to resolve
 *               min(x)==0 on the device from `flags`.  plaidhip_dev_sum -> {sum, #non-NaN}.
 *   3. shift  : x - med[col] + add  (R/plaid.R:572); with `red` (device double[2] = {sum,
 *               count}) non-NULL, add = red[0]/red[1] is taken on the device instead.
 * Nothing in the chain needs a host round trip.                                           */
int plaidhip_dev_minflags(plaidhip_ctx* ctx, const void* S, int64_t count, void* flags);
int plaidhip_dev_col_medians(plaidhip_ctx* ctx, const void* S, int64_t lds, int32_t m, int32_t n,
                             int ignore_zero, const void* flags, void* med);
/* The sparse crossprod that ALSO prepares normalize_medians (round 4).  plaidhip_dev_spmm_csc_fused_f64 is
 * plaidhip_dev_spmm_csc_f64 (rmax == NULL) or plaidhip_dev_spmm_csc_ranks_f64 (rmax != NULL) -- same S, same flags --
 * and, when the scatter kernel takes the input and the result has more than 6,144 sets per column, it classifies every
 * score it writes against a bracket around the column's median (predicted from the column's mean score, which is known from
 * X before the crossprod, and calibrated on the first 256 columns): counts below / zero / NaN and the 1-5 % of the scores
 * inside the bracket go to a scratch the context owns.  plaidhip_dev_col_medians_resume then is plaidhip_dev_col_medians
 * for that S: the medians are selected among the candidates -- the same two middle values, bit for bit -- and only columns
 * whose bracket missed (or everything, if the matrix turns out to follow the other ignore.zero rule than the calibration
 * columns) are read again by the standalone kernel.  The 40 GB second pass of config 3 is gone.  Call it after the flag
 * words are final (a sample-sharded host all-reduces them in between) and before S is changed; with any other S, or after
 * an ineligible crossprod, it simply is plaidhip_dev_col_medians.  nnz must be the caller's true count (>= 0) for the
 * fused form to apply.  Stream-ordered, no host round trip -- except that the context's candidate scratch is (re)allocated
 * when a call needs more than the last one did (hipStreamSynchronize + hipFree + hipMalloc: NOT capture-safe; make the
 * first call of a shape outside a stream capture).  Memory: 8 bytes per candidate slot, min(8,192, max(1,024, 0.16 m))
 * slots per column, + 16 bytes per (column, wavefront slice): at most 0.2 x the bytes of S, kept by the context until
 * plaidhip_dev_fused_medians_discard or plaidhip_destroy.  If that allocation fails the plain crossprod runs.             */
int plaidhip_dev_spmm_csc_fused_f64(plaidhip_ctx* ctx, const plaidhip_geneset* gs, const void* Xp, const void* Xi,
                                    const void* Xx, int32_t n, int64_t nnz, int stat, double alpha, const void* alpha_div,
                                    double beta, void* S, int64_t lds, void* flags, const void* rmax);
int plaidhip_dev_col_medians_resume(plaidhip_ctx* ctx, const void* S, int64_t lds, int32_t m, int32_t n, int ignore_zero,
                                    const void* flags, void* med);
/* The DENSE crossprod that also prepares normalize_medians (round 5): plaidhip_dev_spmm_dense_f64 -- same S, same flags --
 * and, when the fp64 pair kernel takes the input and the result has more than 6,144 sets per column and at least 1e9
 * scores (PLAIDHIP_OPT_FUSED_MEDIANS overrides the size rule), the workgroup of a column pair computes the pair's mean
 * scores from the X it stages (no extra pass over X), and the tile ends of the last gene slice classify the scores they
 * write against the bracket around (mean + calibrated offset) exactly like the sparse form above.  Finish with
 * plaidhip_dev_col_medians_resume (or ..._resume_token); with an ineligible call it is the plain crossprod.
 * Eligible means ALL of: PLAIDHIP_OPT_FUSED_MEDIANS != 2; m > 6,144; n >= 1,024 (four times the 256 calibration columns);
 * m * n >= 1e9 or PLAIDHIP_OPT_FUSED_MEDIANS == 1; flags != NULL; the fp64 pair kernel takes the input -- not the u16 / fp32
 * stagings of rank inputs (plaidhip_dev_spmm_ranks_f64, PLAIDHIP_OPT_RANKS_F32 >= 1 with a one-slice plan) or of
 * PLAIDHIP_PRECISION_MIXED, not the MFMA backend (PLAIDHIP_OPT_SPMM_DENSE_KERNEL == 3), not the one-column kernel.
 * Scratch, its memory cost and the capture caveat: as for plaidhip_dev_spmm_csc_fused_f64 above.                        */
int plaidhip_dev_spmm_dense_fused_f64(plaidhip_ctx* ctx, const plaidhip_geneset* gs, const void* X, int64_t ldx, int32_t n,
                                      int stat, double alpha, const void* alpha_div, double beta, void* S, int64_t lds,
                                      void* flags);
/* plaidhip_dev_col_medians_resume recognises "that S" by (pointer, lds, m, n) only: right for a caller that resumes directly
 * after the fused crossprod.  A caller that may free and re-allocate S in between (an allocator that reuses addresses)
 * takes the TOKEN of the fused launch (plaidhip_dev_fused_medians_info, info[3], right after the crossprod; 0 = the plain
 * route ran, nothing is pending) and resumes with it: the candidates are used only if they are still the pending ones of
 * exactly that launch; any other token (0, stale) runs plaidhip_dev_col_medians -- always correct -- and drops what was
 * pending.  plaidhip_dev_fused_medians_discard drops it explicitly (a caller that will not normalise after all) and
 * releases the candidate scratch (it waits for the context's stream first).                                             */
int plaidhip_dev_col_medians_resume_token(plaidhip_ctx* ctx, int64_t token, const void* S, int64_t lds, int32_t m, int32_t n,
                                          int ignore_zero, const void* flags, void* med);
int plaidhip_dev_fused_medians_discard(plaidhip_ctx* ctx);
/* what the last fused crossprod of this context left behind (tests, tools): info[0] = its number of columns (0: it ran the
 * plain route), info[1] = device pointer to int32 status[n] (after ..._resume: 1 = median selected from the candidates,
 * 0 = the standalone kernel computed it), info[2] = device pointer to the calibration {offset, half width, ignore-zero},
 * info[3] = the launch's token (> 0) while a resume is pending, else 0.                                               */
int plaidhip_dev_fused_medians_info(plaidhip_ctx* ctx, int64_t info[4]);
int plaidhip_dev_sum(plaidhip_ctx* ctx, const void* v, int64_t count, void* out /* double[2]: sum, #non-NaN */);
int plaidhip_dev_shift_columns(plaidhip_ctx* ctx, void* S, int64_t lds, int32_t m, int32_t n,
                               const void* med, double add, const void* red);
/* phase 3 fused with an fp64 -> fp32 cast into ANOTHER matrix (float out[ldo * n]): out = (float)((S - med[col]) + add), S left
 * as it is.  What a sample-sharded job sends to the root when the assembled result must be fp32 to fit one GPU (config 5:
 * 1e6 cells x 50,000 sets = 400 GB in fp64): one read of S and a half-size write instead of shift (read + write) followed by a
 * cast (read + half-size write).  Bit-identical to plaidhip_dev_shift_columns followed by a conversion to float.
 * R/plaid.R:572 (the sweep) and :110-119 (the chunks the reference assembles).                                          */
int plaidhip_dev_shift_columns_cast_f32(plaidhip_ctx* ctx, const void* S, int64_t lds, int32_t m, int32_t n, const void* med,
                                        double add, const void* red, void* out, int64_t ldo);
/* max over a device double vector (global max(rX), R/plaid.R:251) */
int plaidhip_dev_max(plaidhip_ctx* ctx, const void* v, int64_t count, void* out /* double[1] */);

/* ---- host-level entry points: what the R `.Call` shim binds (r-pkg/src/plaidhip_R.c) -- */

/* plaid(X, matG, stats, chunk=NULL, normalize) body, R/plaid.R:73-85, dense X.
 * S_out: m x n doubles, caller-allocated.                                               */
int plaidhip_plaid_dense(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n,
                         const int32_t* Gp, const int32_t* Gi, int32_t m, int stat, int normalize,
                         double* S_out);
/* same for a dgCMatrix X */
int plaidhip_plaid_csc(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx,
                       int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m,
                       int stat, int normalize, double* S_out);
/* chunked_crossprod(x, y) with a general sparse x (see plaidhip_dev_crossprod_weighted_f64), host pointers: x as
 * dgCMatrix slots, y dense g x n; S_out m x n, caller-allocated.  The caller's chunk loop (R/plaid.R:110-119) bounds n. */
int plaidhip_crossprod_weighted_dense(plaidhip_ctx* ctx, const int32_t* Wp, const int32_t* Wi, const double* Wx,
                                      int32_t g, int32_t m, const double* Y, int32_t n, double* S_out);
/* same for a dgCMatrix y */
int plaidhip_crossprod_weighted_csc(plaidhip_ctx* ctx, const int32_t* Wp, const int32_t* Wi, const double* Wx,
                                    int32_t g, int32_t m, const int32_t* Yp, const int32_t* Yi, const double* Yx,
                                    int32_t n, double* S_out);
/* normalize_medians(x, ignore.zero), R/plaid.R:554-575, in place; med_out (n) may be NULL */
int plaidhip_normalize_medians(plaidhip_ctx* ctx, double* S, int32_t m, int32_t n, int ignore_zero,
                               double* med_out);
/* colranks(X, signed, ties.method), dense branch R/plaid.R:611-619 */
int plaidhip_colranks_dense(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, int ties,
                            int is_signed, double* R_out);
/* sparse_colranks(X, signed, ties.method), R/plaid.R:631-650: Rx_out has Xp[n] entries */
int plaidhip_colranks_csc(plaidhip_ctx* ctx, const int32_t* Xp, const double* Xx, int32_t n,
                          int ties, int is_signed, double* Rx_out);
/* colranks(X sparse, keep.zero=FALSE), R/plaid.R:602-609: dense g x n result from CSC input */
int plaidhip_colranks_csc_dense(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx,
                                int32_t g, int32_t n, int ties, int is_signed, double* R_out);
/* replaid.sing body, R/plaid.R:215-217 (dense X; G aligned to X's rows as above)         */
int plaidhip_sing_dense(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n,
                        const int32_t* Gp, const int32_t* Gi, int32_t m, double* S_out);
/* replaid.sing body for a dgCMatrix X (zeros are ranked: colranks' sparse branch without keep.zero, R/plaid.R:602-609):
 * X goes to the device as its CSC slots; the reference (and R/plaid.R:215) densify it                                */
int plaidhip_sing_csc(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx, int32_t g, int32_t n,
                      const int32_t* Gp, const int32_t* Gi, int32_t m, double* S_out);
/* replaid.ssgsea body, R/plaid.R:245-253, dense X                                        */
int plaidhip_ssgsea_dense(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n,
                          const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha,
                          double* S_out);
/* replaid.ssgsea body for a dgCMatrix X (rank step = sparse_colranks, R/plaid.R:600-601)  */
int plaidhip_ssgsea_csc(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx,
                        int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m,
                        double alpha, double* S_out);

/* replaid.ssgsea.exact(X, matG, alpha, scale, norm): the original ssGSEA statistic (gao.ssgsea, single = TRUE) for any
 * alpha, where replaid.ssgsea (R/plaid.R:233-234, 247-248) is exact at alpha = 0 only.  Per sample column with N = g genes:
 * r = average ranks, q = rank(x, ties = "last") (order(r, decreasing = TRUE) keeps tied genes in row order), w = r^alpha;
 * per set with k members (G's column, aligned to X's rows): A = sum w q, B = sum w, C = sum q, T = N (N + 1) / 2, and
 * the scores, in fp64 and in exactly these operations (no other association, no contraction):
 *     d1 = A / B;  d2 = (T - C) / (double)(N - k);  es = d1 - d2;  scale: es = es / N;  norm: es = es / (max - min)
 * with max / min over the whole m x n result (one NaN makes every score NaN, as R's range does).  k = 0 and k = N give
 * NaN (0 / 0).  A sample column holding a NaN scores NaN for every set at every alpha (R's NA^0 == 1 would keep
 * gao.ssgsea finite at alpha = 0: a deliberate difference).  alpha must be finite.  At alpha = 0 (w = 1: A = C, B = k)
 * and alpha = 1 the sums are of integers and half-integers and the scores are exact.  X dense (Xp == NULL: X_or_x are
 * g x n doubles) or a dgCMatrix, scored as as.matrix(X) without densifying it on the host.  The result is fp64 in every
 * precision mode.  S_out: m x n doubles.                                                                             */
int plaidhip_ssgsea_exact(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                          const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha, int scale, int norm, double* S_out);

/* replaid.ssgsea.exact(..., single = FALSE): the running sum's value of LARGEST MAGNITUDE instead of its sum -- the classic
 * GSEA enrichment score (gao.ssgsea's second branch, experiments/R/functions.R:568-572).  Arguments, checks, NaN rules and
 * norm as for plaidhip_ssgsea_exact; r, q, w as there.  The walk visits the genes at pos = N + 1 - q (1 first).  For a set
 * with k aligned members sorted by pos ascending, t = 1..k, in fp64 and in exactly these operations:
 *     cw_t = w_1 + ... + w_t (cw_0 = 0);  B = cw_k;  miss_t = (double)(pos_t - t) / (double)(N - k)
 *     after_t  = cw_t / B - miss_t                          (the running sum at position pos_t)
 *     before_t = cw_{t-1} / B - miss_t   when pos_t >= 2    (the running sum at position pos_t - 1)
 *     scale: each candidate is divided by (double)N before any comparison
 * The running sum falls linearly between two hits, so its extremes are among these 2k candidates.  They are visited in
 * position order (before_1, after_1, before_2, ...); the best starts at 0 and a later candidate replaces it only when its
 * absolute value is strictly larger: step_cdf_diff[which.max(abs(step_cdf_diff))], first maximum and sign included.
 * norm divides by max - min over the whole m x n result.  k = 0 and k = N give NaN; a sample column holding a NaN scores
 * NaN for every set; alpha must be finite.  A candidate holds no product, so no contraction changes a bit.  At alpha = 0
 * (cw_t = t, B = k) and alpha = 1 every candidate is exact; for other alphas cw_t and B are summed in an order that
 * depends on k and the positions alone (never on the sharding).  One route for every k (a bitmap walk, kernels_ks.hip);
 * its map bounds nrow(X): g > PLAIDHIP_GSEA_KS_MAX_GENES returns PLAIDHIP_EUNSUPPORTED before any device work.        */
#define PLAIDHIP_GSEA_KS_MAX_GENES 131072
int plaidhip_ssgsea_exact_ks(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g,
                             int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha, int scale, int norm,
                             double* S_out);

/* replaid.gsva.exact(X, matG, tau, rowtf, max.diff): the random-walk statistic of GSVA (Haenzelmann et al. 2013), where
 * replaid.gsva (R/plaid.R:353-356) is a mean of transformed ranks.  rowtf: 0 "z", 1 "ecdf", 2 "none", 3 "gauss".
 *  1. Row transform v of X: "z" and "ecdf" are replaid.gsva's own (the launches of plaidhip_gsva_multi's z transform, of
 *     plaidhip_gsva / plaidhip_gsva_csc's ecdf; a dgCMatrix through the row view, the dense v built on the device);
 *     "none" takes X as it is, for a caller who brings their own per-gene CDF; "gauss" is GSVA's Gaussian kernel CDF
 *     estimate V of plaidhip_gsva_kcdf below (n >= 2, else PLAIDHIP_EINVAL before any device work), dense whatever X is.
 *  2. Per sample column with N = g genes: q = rank(v, ties = "last"), the walk visits the genes at pos = N + 1 - q.  This
 *     is order(v, decreasing = TRUE) with tied genes in row order.  No average ranks are needed.
 *  3. Weight of the gene at pos: w = |q - N / 2|^tau (GSVA's symmetric rank score abs(seq(N, 1) - N / 2) laid along the
 *     order), with 0^0 = 1.  N / 2 in fp64: integers for even N, half-integers for odd N.  The weight depends on the
 *     position alone: one table of N doubles serves every column and every set of the call.
 *  4. For a set with k aligned members sorted by pos, t = 1..k, in fp64 and in exactly these operations:
 *         cw_t = w_1 + ... + w_t (cw_0 = 0);  B = cw_k;  miss_t = (double)(pos_t - t) / (double)(N - k)
 *         after_t = cw_t / B - miss_t;  before_t = cw_{t-1} / B - miss_t  (only where pos_t >= 2)
 *         mx_pos = max(0, max_t after_t);  mx_neg = min(0, min_t before_t)
 *     The running sum rises only at a hit and ends at 0, so these hold its extremes.
 *  5. max_diff != 0: ES = mx_pos + mx_neg.  max_diff == 0: ES = mx_pos > |mx_neg| ? mx_pos : mx_neg (GSVA's rule: equal
 *     magnitudes return the negative one).
 *  6. k = 0, k = N and B == 0 (tau > 0 and even N: a set made only of the gene at q = N / 2) give NaN.  A column of v
 *     holding a NaN scores NaN for every set.  tau must be finite and >= 0, rowtf one of the three; both are refused
 *     before any device work, as is g > PLAIDHIP_GSEA_KS_MAX_GENES (PLAIDHIP_EUNSUPPORTED).
 *  7. At tau 0 (cw_t = t, B = k) and 1 every cw_t and B is an exact integer or half-integer sum, a candidate is two
 *     correctly rounded divisions and a subtraction with no product in it: the bits of the same operations on the host.
 *     For other tau, cw_t and B are summed in an order that depends on k and the positions only, never on the sharding.
 * Deliberate differences from the GSVA package: GSVA accumulates the running sum step by step (N roundings; this form
 * has three per candidate), its B == 0 case leaves whatever the walk held before the NaN, abs.ranking is not offered, and
 * of GSVA's kernel CDF estimates (kcdf) the Gaussian one is ("gauss"), the Poisson one is not.  No normalize_medians (GSVA
 * applies none).  X dense (Xp == NULL) or a dgCMatrix
 * (rows increasing inside a column), never densified on the host: with "none" its stored values are ranked as
 * plaidhip_ssgsea_exact ranks them.  fp64 in every precision mode.  S_out: m x n doubles.                              */
int plaidhip_gsva_exact(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                        const int32_t* Gp, const int32_t* Gi, int32_t m, double tau, int rowtf, int max_diff, double* S_out);

/* GSVA's Gaussian kernel CDF estimate (kcdf = "Gaussian": the row_d / precomputedCdf loop of its kernel_estimation.c), the
 * row transform "gauss" of plaidhip_gsva_exact, on its own.  Per gene row i of X (g x n, n >= 2), all in fp64, every sum
 * sequential in sample order k = 0, 1, ..., n - 1 and starting from 0.0, no product contracted into an add, every division
 * and the square root correctly rounded:
 *     mean = (x_0 + x_1 + ... + x_{n-1}) / (double) n
 *     ss   = sum_k d_k * d_k,  d_k = x_k - mean                      (the product rounded, then added)
 *     h    = sqrt(ss / (double)(n - 1)) / 4.0
 *     c(d) : v = d / h;  v < -10 -> 0.0;  v > 10 -> 1.0;
 *            else t = T[(int)(fabs(v) / 10.0 * 10000.0)];  v < 0 ? 1.0 - t : t
 *     V_ij = sum_k c(x_ij - x_ik)
 *     T[i] = Phi(10.0 * (double) i / 10000.0) = 0.5 * erfc(-t / sqrt(2.0)),  i = 0 ... 10000
 * T is built once on the host with the C library's erfc, made non-decreasing where that erfc is not (T[i] = max(T[i],
 * T[i - 1])), uploaded, and exported by plaidhip_gsva_kcdf_table so that a checker uses the device's own bits.
 * A row with h == 0 (v = 0 / 0) reads T[0] = 0.5 in every term: V_ij = n / 2 exactly (GSVA indexes its table with
 * (int) NaN there).  A row holding a NaN or an infinity has a NaN h and gives a NaN row of V (GSVA refuses such input), so
 * every column is NaN and scores NaN under plaidhip_gsva_exact.  The kernel may find the index from |d| (1 / h) 1000 where
 * that estimate is provably on the same side of every integer as the pinned expression, and runs the pinned operations
 * elsewhere: the index is the pinned one always.
 * Deliberate differences from the GSVA package: V is the sum itself, where GSVA divides by n and takes -log((1 - F) / F);
 * both are monotone, so a sample's order of genes is the same except where their rounding merges or splits neighbours.
 * GSVA's Poisson kernel (kcdf = "Poisson", for counts) is not offered.
 * X dense (Xp == NULL) or a dgCMatrix, expanded on the device into the dense form (its bits by construction), never
 * densified on the host.  n < 2: PLAIDHIP_EINVAL before any device work.  V_out: g x n doubles, column-major.            */
#define PLAIDHIP_GSVA_KCDF_TABLE 10001
int plaidhip_gsva_kcdf(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                       double* V_out);
/* out[PLAIDHIP_GSVA_KCDF_TABLE] <- T.  Needs no device. */
int plaidhip_gsva_kcdf_table(double* out);

/* replaid.sing.exact(X, matG, matD, center, dispersion): singscore's normalised score and its dispersion, where
 * replaid.sing (R/plaid.R:203-216) returns mean(rank) / N - 0.5, which only orders the samples as singscore does.  The
 * formulas follow singscore's rankGenes and singscoring (simpleScore) AS RECALLED: the package's source is not in this
 * tree, so the statistic is pinned here, operation for operation, and tested against these words.
 * Per sample column with N = g rows (all rows of X, before the alignment with the sets, as in replaid.sing), in fp64:
 *  1. r = rank(x, ties = "min"), integers 1..N: the ranks replaid.sing takes.  A down set is scored on d = N + 1 - r.
 *  2. Score of a set with k aligned members of ranks s:  mean = (double)(sum s) / (double)k  (the sum an exact integer;
 *     a down set's is k (N + 1) - sum r, formed in integers);  low = (k + 1) / 2,  high = (2 N - k + 1) / 2,  so
 *     high - low = N - k;  score = (mean - low) / (double)(N - k),  then - 0.5 when center != 0.  Two correctly rounded
 *     divisions and at most two subtractions; no product, nothing to contract.  k = 0 and k = N give NaN: 0 / 0, and for
 *     k = N in a column with ties, where the min ranks sum to less than N (N + 1) / 2 and the quotient would be -Inf, NaN
 *     by rule (high == low: the score is not defined).
 *  3. Dispersion:  med = median(s) (R's: the mean of the two middle values for even k, an exact half-integer);
 *     dev_i = |s_i - med|;  disp = 1.4826 * median(dev), the constant R's literal of mad().  median(dev) is an exact
 *     multiple of 0.25 (formed in integers as 4 median(dev), then * 0.25), so the product carries the one rounding.
 *     k = 0 gives NaN, k = N is finite.  The dispersion of a down set is that of its r (a reflection), bit for bit.
 *  4. Column j of the down sets (Dp / Di, aligned to X's rows as Gp / Gi are, m columns) pairs with column j of the up
 *     sets: total = up + down, one add each for score and dispersion; an empty down column makes that row NaN.
 *     Dp == NULL: up only; total, down, total_disp and down_disp must then be NULL (PLAIDHIP_EINVAL otherwise).
 *  5. A column of X holding a NaN gives NaN in every output.
 * Six nullable m x n outputs; what is NULL is not computed: without a dispersion output the per-pair kernel is not
 * launched and the launches are replaid.sing's and an epilogue.  Each column is ranked once whatever is asked for; the
 * dispersions add one rank pass over a tie-free column built from those ranks (the last ranks).  The totals are filled on
 * the device.  X dense (Xp == NULL) or a dgCMatrix (rows increasing inside a column), never densified on the host: its
 * zeros are ranked as colranks ranks them for replaid.sing, the result has the dense form's bits.  fp64 and integers in
 * every precision mode.  With a dispersion output g <= PLAIDHIP_GSEA_KS_MAX_GENES, else PLAIDHIP_EUNSUPPORTED before any
 * device work.  Not offered: knownDirection = FALSE, other dispersion functions, stable genes, permutation p-values.    */
int plaidhip_sing_exact(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                        const int32_t* Gp, const int32_t* Gi, const int32_t* Dp, const int32_t* Di, int32_t m, int center,
                        double* total, double* up, double* down, double* total_disp, double* up_disp, double* down_disp);

/* replaid.ucell.exact and replaid.aucell.exact: the statistics of UCell (ScoreSignatures_UCell) and of AUCell
 * (AUCell_calcAUC) on truncated ranks, where replaid.ucell is "near exact" (max(rX) - rX for the descending rank, plaid()'s
 * median normalisation and its 1e-8) and replaid.aucell a ramp with a factor of 1.08.  The formulas follow the two packages
 * AS RECALLED: their sources are not in this tree, so the statistics are pinned here, operation for operation, and tested
 * against these words.
 * Common to both, per sample column: N = g rows; all rows of X are ranked before the alignment with the sets, as in
 * replaid.ucell.  X dense (Xp == NULL) or a dgCMatrix (rows increasing inside a column) whose implicit zeros are ranked; it
 * is never expanded, on the host or on the device: no g x n buffer of any type is allocated for it, device memory is
 * O(nnz + n T + m n).  A column holding a NaN gives NaN in all of its outputs.  k: the aligned members of a set.  fp64 and
 * integers in every precision mode.
 *
 * plaidhip_ucell_exact, T = max_rank, an integer in 1..N:
 *  1. d = rank(-x, ties = "average") = N + 1 - colranks(x, "average"): half-integers.
 *  2. UCell's truncation, which is not pmin: c = (d <= T) ? d : T + 1.  Weight u = T + 1 - c: a half-integer >= 0, zero for
 *     every gene with d > T.  A tie group is weighted as a whole or not at all: the group at the boundary, with `a` strictly
 *     larger values and `c` members, has the average rank a + (c + 1) / 2 and is weighted exactly when that is <= T.
 *  3. K = k_full[j] when impute != 0 (UCell's missing_genes = "impute": absent members count with rank T + 1; k_full[j] an
 *     integer >= k), else K = k.  In integers: S2 = 2 sum u over the aligned members;
 *     U2 = 2 K (T + 1) - S2 - K (K + 1);  auc = 1.0 - (double)U2 / (double)(2 K T): one correctly rounded division and one
 *     subtraction, no product of doubles.  auc < 0 gives 0.0.  K = 0 gives NaN.
 *     2 N T >= 2^53 (or 2 K (T + 1) + K (K + 1) >= 2^53 for an imputed K): PLAIDHIP_EUNSUPPORTED before any device work.
 *  4. Down sets (Dp / Di, aligned to X's rows, m columns; their imputed sizes in k_full_down): column j pairs with column j
 *     of the up sets.  down = the same statistic on the down members;  total = up - w_neg * down: one multiplication and one
 *     subtraction, never contracted.  total < 0 gives 0.0.  An empty down column makes total NaN.  w_neg finite and >= 0.
 *     Three nullable m x n outputs; what is NULL is not computed.  Dp == NULL with total or down non-NULL: PLAIDHIP_EINVAL.
 *     impute != 0 with k_full == NULL (or, beside down sets, k_full_down == NULL): PLAIDHIP_EINVAL.
 *
 * plaidhip_aucell_exact, A = auc_max_rank, an integer in 1..N:
 *  1. AUCell breaks ties at random; here they are broken by row order, so that the result is a function of its input:
 *     pos = N + 1 - rank(x, ties = "last"), distinct integers, the earlier row of a tie taking the smaller pos.
 *  2. area = sum (A - pos) over the members with pos < A (strict, as AUCell's x < aucThreshold);  kk = min(k, A - 1);
 *     maxAUC = kk A - kk (kk + 1) / 2, both exact integers;  score = (double)area / (double)maxAUC: one division.
 *     k = 0 or A = 1 gives 0 / 0 = NaN.  2 N A >= 2^53: PLAIDHIP_EUNSUPPORTED before any device work.
 *  3. No normalize_medians.  Not offered: random ties, and AUCell's older normalisation (A k).                            */
int plaidhip_ucell_exact(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                         const int32_t* Gp, const int32_t* Gi, const int32_t* Dp, const int32_t* Di, int32_t m, double max_rank,
                         double w_neg, int impute, const double* k_full, const double* k_full_down, double* total, double* up,
                         double* down);
int plaidhip_aucell_exact(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                          const int32_t* Gp, const int32_t* Gi, int32_t m, double auc_max_rank, double* S_out);

/* The truncated-rank stage of the two on device operands, stream-ordered, no read-back: per column the compressed list
 * (row, weight) of the entries whose weight is not zero, rows ascending, as CSC slots Wp (n + 1), Wi, Wx (doubles) that
 * plaidhip_dev_spmm_csc_f64 takes (stat = sum gives S2 / 2, or the area).  mode PLAIDHIP_TRUNC_UCELL: weights u;
 * PLAIDHIP_TRUNC_AUCELL: A - pos for the first A - 1 positions.  T in 1..g, g < 2^26.  A count pass, an exclusive scan on
 * the device and a fill pass place the columns; `capacity` (entries of Wi / Wx) must cover what the columns can take:
 * n min(g, 2 T - 1) (UCell) or n min(g, T - 1) (AUCell), and for _csc nnz (UCell) or n min(g, T - 1) (AUCell); else
 * PLAIDHIP_EINVAL.  colnan: n words, 1 for a column holding a NaN (which gets no entries); counts: n words of scratch.
 * Dense: X g x n (leading dimension ldx), R_scratch g x n doubles.
 * _csc: the slots of a g x n matrix, rows increasing inside a column, Xp[0] = 0, nnz = Xp[n], max_col_nnz the longest
 * column; scratch 2 nnz doubles.  All zeros, stored and implicit, form one tie group.  UCell: where that group is weighted
 * it is not enumerated: u0[c] (n doubles) receives its weight and every stored non-zero entry the weight u - u0 (any
 * sign; entries whose shifted weight is zero are left out), so that sum u over a set = sum of its entries + k u0[c].
 * AUCell: u0 is zeroed, and the first zero rows in row order, implicit ones included, fill the positions the positive
 * values leave below A.                                                                                              */
#define PLAIDHIP_TRUNC_UCELL 0
#define PLAIDHIP_TRUNC_AUCELL 1
int plaidhip_dev_truncated_ranks_f64(plaidhip_ctx* ctx, const void* X, int64_t ldx, int32_t g, int32_t n, int mode, int64_t T,
                                     void* R_scratch, void* colnan, void* counts, void* Wp, void* Wi, void* Wx,
                                     int64_t capacity);
int plaidhip_dev_truncated_ranks_csc_f64(plaidhip_ctx* ctx, const void* Xp, const void* Xi, const void* Xx, int32_t g, int32_t n,
                                         int32_t max_col_nnz, int64_t nnz, int mode, int64_t T, void* scratch, void* colnan,
                                         void* counts, void* u0, void* Wp, void* Wi, void* Wx, int64_t capacity);

/* ---- several GPUs of one node from ONE host process (the R session): multi.cpp ----------------------
 * The sample columns are cut into ndev contiguous shards (plaidhip_shard_bounds); a host thread per device
 * moves its shard over its own PCIe link (pipelined through pinned staging), runs the same kernels, and the
 * three scalars that couple the samples -- max(rX) (R/plaid.R:251), min(x) == 0 (:556-557), mean(medx) (:572)
 * -- are combined on the host between the phases.  Nothing else crosses between devices (no RCCL).
 * `devices`: ndev distinct device ordinals, or NULL for 0 .. ndev-1.  X: dense g x n (Xp == NULL, X_or_x are
 * the doubles) or a dgCMatrix (Xp, Xi, X_or_x = @x).  The contexts are created on first use and kept by the
 * library until plaidhip_multi_finalize().  For dense X the results equal the single-device entry points bit
 * for bit (shards only change which device computes a column).  For a dgCMatrix every sharding takes the same
 * kernel (chosen from the density of the whole matrix); the sparse-aware scatter kernel adds in arrival order, so
 * its scores agree to the last bits only (~1e-16 relative), between shardings as between two runs.             */
int plaidhip_shard_bounds(int64_t n, int ndev, int k, int64_t* lo, int64_t* hi);   /* columns [lo, hi) of shard k */
int plaidhip_plaid_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                         int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, int stat,
                         int normalize, double* S_out);
int plaidhip_sing_multi(const int* devices, int ndev, const double* X, int32_t g, int32_t n, const int32_t* Gp,
                        const int32_t* Gi, int32_t m, double* S_out);
/* replaid.sing for a dgCMatrix X over several devices (see plaidhip_sing_csc) */
int plaidhip_sing_csc_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* Xx, int32_t g,
                            int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double* S_out);
int plaidhip_ssgsea_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                          int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha,
                          double* S_out);
/* replaid.ssgsea.exact over several devices: the arguments and results of plaidhip_ssgsea_exact, bit for bit for dense X
 * and for a dgCMatrix alike (per-column work only; norm's range is combined on the host).  The argument checks and the
 * device list's run before any device is touched.                                                                     */
int plaidhip_ssgsea_exact_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                                int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha, int scale,
                                int norm, double* S_out);
/* plaidhip_ssgsea_exact_ks over several devices, bit for bit (the walk is per column; norm's range is combined on the
 * host).  The argument checks, the bound on g among them, and the device list's run before any device is touched.     */
int plaidhip_ssgsea_exact_ks_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                                   int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha,
                                   int scale, int norm, double* S_out);
/* plaidhip_gsva_exact over several devices, sharded by sample column.  "none" has no coupling between the shards; "z"
 * chains the row moments as plaidhip_gsva_multi does (dense X: shards of whole 128-column blocks, the one-device bits;
 * a dgCMatrix: the rows' sums of stored values are added shard by shard, which is exact whenever those sums are);
 * "ecdf" ranks all samples of a gene together and returns PLAIDHIP_EINVAL when ndev > 1.  "gauss" is sharded by sample
 * too: every device receives all of X (each V_ij needs its gene's whole row) and computes V for its own columns, summing
 * over k in the one fixed order, so every sharding gives the one-device bits.  The walk is per column.  The argument
 * checks and the device list's run before any device is touched.                                                       */
int plaidhip_gsva_exact_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                              int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double tau, int rowtf,
                              int max_diff, double* S_out);
/* plaidhip_sing_exact over several devices, sharded by sample column.  Nothing couples the shards: every sharding returns
 * the one-device bits.  The argument checks and the device list's run before any device is touched.                     */
int plaidhip_sing_exact_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                              int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, const int32_t* Dp, const int32_t* Di,
                              int32_t m, int center, double* total, double* up, double* down, double* total_disp,
                              double* up_disp, double* down_disp);
/* plaidhip_ucell_exact and plaidhip_aucell_exact over several devices, sharded by sample column.  Nothing couples the
 * shards and every sum is exact: every sharding returns the one-device bits, dense and dgCMatrix.  Memory per shard (nloc =
 * its columns): dense X g x nloc and its ranks panel by panel; a dgCMatrix its slots, 2 nnz doubles and the compressed
 * weights.  The argument checks and the device list's run before any device is touched.                               */
int plaidhip_ucell_exact_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                               int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, const int32_t* Dp, const int32_t* Di,
                               int32_t m, double max_rank, double w_neg, int impute, const double* k_full,
                               const double* k_full_down, double* total, double* up, double* down);
int plaidhip_aucell_exact_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                                int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double auc_max_rank,
                                double* S_out);
/* replaid.ucell / aucell / scse / gsva over several devices: the arguments and results of plaidhip_ucell, plaidhip_aucell,
 * plaidhip_scse and plaidhip_gsva (rowtf = 0, "z"), X dense or a dgCMatrix as above.  The argument checks run before any
 * device is touched.  What couples the shards is combined on the host: max(rX) (R/plaid.R:278, 306, 354), the min / max
 * behind removeLog2 = NULL (:160-161, decided ONCE for the whole matrix; its implicit zeros count), the per-gene mean
 * and sd of the z row transform (:341-343, g values each), and the medians' flags and mean(medx).
 * Result contract: for dense X every sharding equals the single-device entry bit for bit, removed_log2 included.
 * replaid.gsva's row sums are chained: dense X is cut into shards of whole 128-column blocks (per = 128 *
 * ceil(ceil(n / 128) / ndev) columns, not plaidhip_shard_bounds), and each shard continues the previous shard's running
 * sums block by block, so the z transform adds exactly what the one-device call adds, in its order.  For a dgCMatrix
 * the results agree with the single-device entry to the last bits only (the sparse crossprod adds in arrival order,
 * the rows' moments of stored values are summed per shard) and are deterministic for a given sharding.
 * Memory per shard (nloc = its columns): ucell / aucell the shard's X and its g x nloc average ranks; scse its X;
 * gsva two g x nloc buffers (X or zX, ranks), plus, for a dgCMatrix, the shard's slots and their row view; every
 * method the m x nloc scores.  rowtf = 1 ("ecdf") ranks all samples of a gene together and is not sharded: the call
 * returns PLAIDHIP_EINVAL (use plaidhip_gsva / plaidhip_gsva_csc on one device).                                   */
int plaidhip_ucell_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                         int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m,
                         const double* k_full, double rmax, double* S_out);
int plaidhip_aucell_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                          int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double auc_max_rank,
                          double* S_out);
int plaidhip_scse_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                        int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, int remove_log2,
                        int score_mean, double* S_out, int* removed_log2);
int plaidhip_gsva_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                        int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double tau, int rowtf,
                        double* S_out);
/* plaid.test over several devices: the arguments, checks, error messages and `out` of plaidhip_plaid_test (X dense,
 * Xp == NULL) and plaidhip_plaid_test_csc (a dgCMatrix: Xp, Xi, X_or_x = @x), y / tests / metap_method / gsetX as there.
 * The checks run before any device is touched.  The shards are cut at whole 128-column blocks (as dense gsva above).
 * Everything plaid.test reduces is a row sum over the samples, so the scores never leave their devices and only
 * O(genes + sets) numbers cross between the shards: the two group sums of X (dense: chained from shard to shard in the
 * one-device block order; a dgCMatrix: each shard's stored values per group, added on the host in shard order), then on
 * shard 0 alone fc, fc^2 and Gt [fc, fc^2]; then the medians' flags and mean(medx) of plaid(X, G) (gsetX == NULL), and
 * the chained group sums and sums of squared deviations of the score rows, which are normalised on load (the shifted
 * scores are never written).  The p-values are computed on the host from those.
 * Result contract: for dense X every sharding equals plaidhip_plaid_test bit for bit, NaNs included, with or without
 * gsetX, for every `tests` and both metap_method values; for a dgCMatrix the sums are added in another order and the
 * result agrees with plaidhip_plaid_test_csc to ~1e-9 relative.
 * Memory per shard (nloc = its columns): dense X g x nloc, or the shard's slots and their row view; with "lm" the
 * m x nloc scores; O(g + m) besides.  No shard holds X and S of all samples.                                       */
int plaidhip_plaid_test_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                              int32_t g, int32_t n, const int32_t* y, const int32_t* Gp, const int32_t* Gi, int32_t m,
                              const double* gsetX, int tests, int metap_method, double* out);
/* precision of the dense crossprod on the library-owned contexts of the *_multi entry points (plaidhip_set_precision's
 * counterpart; default PLAIDHIP_PRECISION_F64) */
int plaidhip_multi_set_precision(int mode);
int plaidhip_multi_finalize(void);

/* ---- "next" rows of the scope table: thin callers of the same two kernels --------------- */

/* replaid.ucell(X, matG, rmax), R/plaid.R:276-282: rX = colranks(X, "average");
 * rX = pmin(max(rX) - rX, rmax + 1); S = plaid(rX, matG); S = 1 - S/rmax + (k_full + 1)/(2 rmax).
 * X dense (Xp == NULL: X_or_x is g x n doubles) or dgCMatrix (zeros are ranked, R/plaid.R:602-609).
 * k_full[m] = colSums(matG != 0) of the UN-aligned matrix, exactly as R/plaid.R:280 uses it.   */
int plaidhip_ucell(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                   int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m,
                   const double* k_full, double rmax, double* S_out);
/* replaid.aucell(X, matG, aucMaxRank), R/plaid.R:304-309:
 * ww = 1.08 * pmax((rX - (max(rX) - K)) / K, 0); plaid(ww, matG, stats = "mean").             */
int plaidhip_aucell(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                    int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m,
                    double auc_max_rank, double* S_out);
/* replaid.scse(X, matG, removeLog2, scoreMean), R/plaid.R:155-190.  remove_log2: -1 = NULL (auto:
 * min(X) == 0 && max(X) < 20, :160-161), 0, 1.  score_mean: 0 -> sum statistic, x100 (:180-182);
 * 1 -> mean statistic divided by colMeans(|X|) (:175-177).  removed_log2 (may be NULL): set to 1
 * when the 2**x transform ran -- the automatic decision is taken on the device; the host prints
 * the reference's message from it (:164).                                                       */
int plaidhip_scse(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                  int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m,
                  int remove_log2, int score_mean, double* S_out, int* removed_log2);

/* replaid.gsva(X, matG, tau, rowtf), R/plaid.R:338-363, dense X (a dgCMatrix: plaidhip_gsva_csc
 * below): row transform (rowtf = 0: "z", center + scale per gene; 1: "ecdf", the per-gene empirical
 * CDF), signed average ranks per sample,
 * / max|rank|, sign * |.|^(1 + tau) for tau > 0, then plaid(mean, normalised).  One device; the
 * z transform over several devices is plaidhip_gsva_multi (ecdf needs every sample of a gene on one
 * device and is not sharded).                                                                     */
int plaidhip_gsva(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, const int32_t* Gp,
                  const int32_t* Gi, int32_t m, double tau, int rowtf, double* S_out);

/* plaid.test(X, y, G, gsetX, tests, metap.method), R/plaid.R:392-474, for dense X and the aligned
 * pattern G.  y: 0 / 1 per sample.  gsetX: sets x samples scores, or NULL: plaid(X, G) is computed
 * and stays on the device (:424-427).  tests: bit mask 1 = "one" (one-sample t on logFC, :476-486),
 * 2 = "two" (:488-520), 4 = "lm" (Welch per set over the scores, Rfast::ttests, :429).
 * metap_method: 0 = fisher / sumlog, 1 = stouffer / sumz (:522-537).
 * out: sets x 6, column-major: gsetFC, p.one, p.two, p.lm, p.meta, q.meta -- in the column order of
 * G (the caller sorts, :469-471); columns of tests that were not asked for are NaN.               */
int plaidhip_plaid_test(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, const int32_t* y,
                        const int32_t* Gp, const int32_t* Gi, int32_t m, const double* gsetX, int tests,
                        int metap_method, double* out);

/* The same two calls for a dgCMatrix X (g x n, slots Xp / Xi / Xx): replaid.gsva(X, ...) and plaid.test(X, ...) with
 * the result of as.matrix(X) (R/plaid.R:341-343 / 365-370, 407-408 / 426), without a dense X on the host or the link.
 * The slots go to the device and are transposed there into a row view (CSR), whose rows are in ascending column
 * order whatever the scheduling; the row statistics sum each row in that order, with no floating-point atomics.
 *   plaidhip_gsva_csc: "z": per-gene mean / sd from the stored values and the implicit zeros; "ecdf": #{x <= x_i}
 *     per gene from the max-ranks of the stored values and the implicit zeros (integers: exact).  The dense zX is then
 *     built on the device and the rest is plaidhip_gsva's own launch sequence.  Device memory: the CSC slots, the row
 *     view (Rp, Rx, and for "ecdf" the CSC position of every entry: 12 or 16 bytes per stored value), two g x n doubles
 *     (zX and its ranks: every gene is ranked in every sample) and S; no g x n buffer on the host.
 *   plaidhip_plaid_test_csc: the logFC from the per-row group means of the row view, then plaidhip_plaid_test's
 *     crossprod and host tail; with "lm" and gsetX == NULL, plaid(X, G) is computed from the CSC slots with the
 *     kernels of plaidhip_plaid_csc (mean, normalised) and stays on the device.  Device memory: the CSC slots, the row
 *     view (Rp, Rx, column indices: 12 bytes per stored value) and m x n doubles of scores with "lm"; no g x n buffer
 *     anywhere.  Same y / tests / metap_method checks, messages and out as plaidhip_plaid_test.
 * Guarantees: the same inputs give the same bits from run to run; two genes with identical rows get identical row
 * statistics; "ecdf" gives the bits of plaidhip_gsva on as.matrix(X).  R: replaid.gsva / plaid.test with a dgCMatrix
 * (R_plaidhip_gsva_csc, R_plaidhip_plaid_test_csc).                                                                   */
int plaidhip_gsva_csc(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx, int32_t g, int32_t n,
                      const int32_t* Gp, const int32_t* Gi, int32_t m, double tau, int rowtf, double* S_out);
int plaidhip_plaid_test_csc(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx, int32_t g,
                            int32_t n, const int32_t* y, const int32_t* Gp, const int32_t* Gi, int32_t m,
                            const double* gsetX, int tests, int metap_method, double* out);

/* plaid.test over SAMPLE SHARDS (one process per GPU): the statistics of R/plaid.R:407-431 are row-wise sums over the
 * samples, so every shard reduces its own columns on the device and the caller adds the shards' results (an all-reduce
 * of 2 x rows doubles) before the host half runs once.  All pointers of the two _dev_ entries are device pointers;
 * stream-ordered, no synchronisation.
 *   plaidhip_dev_row_group_sums: sums[0 * rows + r] = sum of A[r, c] over the columns with y[c] == 0, sums[rows + r] over
 *     y[c] == 1 (rowMeans of :407-408 and :431 times the group size).  A: rows x n, column-major, leading dimension ld.
 *   plaidhip_dev_row_group_ssd: ssd[.] = sum of (A[r, c] - mean[group, r])^2 per group, mean: [2][rows] -- the caller
 *     passes the means of ALL shards, so the shards' results add up to the two-pass sums the one-device call computes
 *     (the group variances of Rfast::ttests, :429).
 *   plaidhip_plaid_test_finish (host only, no device): T = [2][m] per-set sums of fc and of fc^2 (crossprod of G with the
 *     two columns, :478-479), tot1 / tot2 = sums of fc and fc^2 over all g genes (:490-493), SM = [4][m] group-0 mean,
 *     group-1 mean, group-0 ssd, group-1 ssd of the score rows (NULL without the "lm" test), n0 / n1 the group sizes.
 *     Same `tests`, `metap_method` and `out` as plaidhip_plaid_test, which calls it.                                     */
int plaidhip_dev_row_group_sums(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n,
                                const int32_t* y, double* sums);
int plaidhip_dev_row_group_ssd(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n,
                               const int32_t* y, const double* mean, double* ssd);
int plaidhip_plaid_test_finish(int32_t g, int32_t m, const int32_t* Gp, const double* T, double tot1, double tot2,
                               const double* SM, int64_t n0, int64_t n1, int tests, int metap_method, double* out);

/* plaid.test.contrasts(X, Y, G, gsetX, tests, metap.method): plaid.test for every column of a contrast matrix in one pass
 * over the scores.  Y: n x C, int32, column-major, 0 / 1 per sample and -1 for NA: the sample takes no part in that
 * contrast.  Anything else is PLAIDHIP_EINVAL with a message naming the contrast and the sample (both counted from 1),
 * before any device is touched.  With sel_j = which(!is.na(Y[, j])), contrast j is the reference's
 *     plaid.test(X[, sel_j], Y[sel_j, j], G, gsetX = S_all[, sel_j], tests, metap.method)         (R/plaid.R:392-474)
 * where S_all is the gsetX given or, gsetX == NULL, plaid(X, G) over ALL samples (:424-427): the scores are computed and
 * normalised once (the constant mean(medx) cancels in the Welch test and in gsetFC).  A contrast without NA is therefore
 * plaidhip_plaid_test(X, Y[, j], ...) and has its bits, NaNs included; empty groups, groups of one and constant rows
 * behave as documented there.  A NaN or Inf in an excluded sample's column of X (given gsetX) or of gsetX does not reach
 * that contrast: an excluded column is added as +0.0.
 * out: m x 6 x C doubles, contrast j at out + j * 6 * m with plaidhip_plaid_test's six columns in G's order.  C == 0 or
 * m == 0: nothing is written.  tests / metap_method: as plaidhip_plaid_test.
 * How: the row moments are taken for PLAIDHIP_CONTRAST_TILE contrasts per read of the matrix (kernels_contrasts.hip), so
 * dense X is read ceil(C / tile) times for the logFC and the scores 2 ceil(C / tile) times for the Welch moments, not C
 * and 2 C times, and plaid(X, G) runs once.  Gt [fc_j, fc_j^2] is the dense crossprod of plaidhip_plaid_test, called per
 * contrast with its two columns; a dgCMatrix is uploaded and transposed once, its stored-value group sums run once per
 * contrast.  The host tail is plaidhip_plaid_test_finish per contrast with that contrast's group sizes.
 * Device memory: X (or its slots and row view) and, with "lm", the scores S once; the block partials
 * 2 * C * rows * ceil(n / 128) doubles for rows = g (dense X) and rows = m ("lm"), one buffer for both;
 * O(C * (g + m)) besides.
 *   plaidhip_plaid_test_contrasts: dense X.  plaidhip_plaid_test_contrasts_csc: the slots of a dgCMatrix.
 *   plaidhip_plaid_test_contrasts_multi: the sample columns sharded over devices exactly as plaidhip_plaid_test_multi
 *     (X dense with Xp == NULL, or the slots), the chained sums carried as [C][2][rows]; for dense X every sharding has the
 *     bits of the one-device call.  This is the single-process form; a process per GPU combines the two _dev_ entries
 *     below as plaid_amd/sharded.py does for plaid.test.
 *   plaidhip_dev_row_contrast_sums / _ssd: plaidhip_dev_row_group_sums / _ssd for C label columns at once.  Device
 *     pointers, stream-ordered.  Y: n x C int32 column-major (0, 1, anything else: excluded); sums, mean, ssd:
 *     [C][2][rows].  A contrast without an excluded sample has the bits of the one-label entries.                        */
#define PLAIDHIP_CONTRAST_TILE 8
int plaidhip_plaid_test_contrasts(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, const int32_t* Y, int32_t C,
                                  const int32_t* Gp, const int32_t* Gi, int32_t m, const double* gsetX, int tests,
                                  int metap_method, double* out);
int plaidhip_plaid_test_contrasts_csc(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx, int32_t g,
                                      int32_t n, const int32_t* Y, int32_t C, const int32_t* Gp, const int32_t* Gi,
                                      int32_t m, const double* gsetX, int tests, int metap_method, double* out);
int plaidhip_plaid_test_contrasts_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi,
                                        const double* X_or_x, int32_t g, int32_t n, const int32_t* Y, int32_t C,
                                        const int32_t* Gp, const int32_t* Gi, int32_t m, const double* gsetX, int tests,
                                        int metap_method, double* out);
int plaidhip_dev_row_contrast_sums(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n,
                                   const int32_t* Y, int32_t C, double* sums);
int plaidhip_dev_row_contrast_ssd(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n,
                                  const int32_t* Y, int32_t C, const double* mean, double* ssd);
int plaidhip_contrast_tile(void);   /* PLAIDHIP_CONTRAST_TILE of the built library */

/* plaid.gsea(stats, G, nperm, gseaParam): preranked GSEA with a permutation null -- ES, NES, pval and padj of every set for
 * every ranked list (a logFC vector, or one per contrast).  The form is fgsea's fgseaSimple with scoreType = "std" AS
 * RECALLED: the package's source is not in this tree, so the statistic is pinned here, operation for operation, and tested
 * against these words.
 * Operands, per ranked list (a column of stat, g x c, column-major, beside weight, g x c, all finite and >= 0):
 *     N = g genes.  The walk order is order(-stat), stable: tied genes go in row order.
 *     pos_obs[i] in 0..N-1 is gene i's place in that order (the second rank pass of plaidhip_sing_exact gives it).
 *     Wpos[pos_obs[i]] = weight[i].  The wrappers pass weight = |stat|^gseaParam, computed on the host: the device never
 *     calls pow.
 * A placement is an int32 vector pos[0..N) that is a permutation of 0..N-1.  The observed placement is pos_obs; null
 * placement b is column b of P (g x B) and is the same for every set and every list.
 * A set with k members has 1-based positions p_1 < ... < p_k, taken from pos[i] + 1 over its members i.  Then, in fp64:
 *     w_t = Wpos[p_t - 1];  cw_t = w_1 + ... + w_t;  B = cw_k
 *     if B == 0:  w_t = 1 for all t   (cw_t = t, B = k: the unweighted walk, as fgsea's calcGseaStat does for NR == 0)
 *     miss_t = (double)(p_t - t) / (double)(N - k)
 *     after_t = cw_t / B - miss_t;   before_t = cw_{t-1} / B - miss_t      (t = 1..k, cw_0 = 0)
 *     maxP = max_t after_t;  minP = min_t before_t
 *     ES = maxP > -minP ? maxP : (maxP < -minP ? minP : 0.0)
 * k = 0 or k = N gives NaN in every output column of that set, except `size`.  A list holding a NaN or an infinity in stat
 * gives NaN for that list.  A negative, NaN or infinite weight is an argument error before any device work.
 * Per (set, list), over the null scores es_b, b = 0..B-1 (B = nperm):
 *     nGeEs = #{es_b >= ES}   nLeEs = #{es_b <= ES}   nGeZero = #{es_b >= 0}   nLeZero = #{es_b <= 0}
 *     sumPos = sum max(es_b, 0)    sumNeg = sum min(es_b, 0)
 *     NES  = ES > 0 ? ES / (sumPos / nGeZero) : ES / fabs(sumNeg / nLeZero)
 *     pval = min((1 + nLeEs) / (1 + nLeZero), (1 + nGeEs) / (1 + nGeZero))
 *     nMoreExtreme = ES > 0 ? nGeEs : nLeEs
 * The two sums are taken in blocks of PLAIDHIP_GSEA_PERM_BLOCK consecutive permutations: inside a block sequentially in b
 * from 0.0, the block sums then sequentially in block order from 0.0.  No product is contracted anywhere; the divisions
 * follow IEEE, so a zero mean gives +-Inf or NaN as the form says.  Where every weight is an integer below 2^20 (or 1)
 * every cw_t is exact and all of this has the bits of the same operations on the host; for other weights cw_t and B are
 * summed in an order that depends on the positions alone, never on the sharding.
 * padj is Benjamini-Hochberg over the sets of one list that have a non-NaN pval (the host routine behind q.meta).
 * Permutations: perm != NULL is int32, g x nperm, every column checked on the device to be a permutation of 0..g-1 before
 * it is walked (PLAIDHIP_EINVAL otherwise).  The columns are checked slab by slab as they are uploaded, so a bad column may
 * be found after earlier slabs were walked: on any error out and null_out are unspecified.  perm == NULL generates the placements from seed: for gene i and permutation b,
 * Philox4x32-10 with counter (i, b, 0, 0) and key (seed & 0xffffffff, seed >> 32) gives words o0..o3;
 * r = ((uint64)o0 << 4) | (o1 >> 28) (36 bits);  y = (double)(r 2^17 + i), exact and free of ties because g <= 131,072;
 * P[., b] = (ascending min rank of y within column b) - 1.  The placement of (i, b) depends on nothing else: it is the same
 * under every sharding.  plaidhip_gsea_permutations returns these placements themselves (P_out: g x nperm int32).
 * out: m x 12 x c, column-major: ES, NES, pval, padj, nMoreExtreme, size, nGeEs, nLeEs, nGeZero, nLeZero, sumPos, sumNeg.
 * null_out (nullable): the m x nperm x c null scores.  Argument errors, in this order: nperm < 1, c < 1,
 * g > PLAIDHIP_GSEA_KS_MAX_GENES (PLAIDHIP_EUNSUPPORTED), a bad weight, then (on the device) a bad perm column.
 * plaidhip_gsea_multi shares the permutation blocks out over the devices in whole blocks; every device holds stat, weight
 * and G; the block partials are chained in block order and reduced once: every sharding returns the one-device bits.
 * Score types (plaidhip_gsea_scored; fgsea's scoreType, AS RECALLED like the rest): PLAIDHIP_GSEA_STD is everything above,
 * unchanged.  With maxP and minP as defined above, for the observed score and for every null score alike:
 *                     std (above)                                           pos                        neg
 *     ES              maxP > -minP ? maxP : (maxP < -minP ? minP : 0.0)     maxP                       minP
 *     NES             ES > 0 ? ES/(sumPos/nGeZero)                          ES/(sumPos/nGeZero)        ES/fabs(sumNeg/nLeZero)
 *                            : ES/fabs(sumNeg/nLeZero)
 *     pval            min((1+nLeEs)/(1+nLeZero), (1+nGeEs)/(1+nGeZero))     (1+nGeEs)/(1+nGeZero)      (1+nLeEs)/(1+nLeZero)
 *     nMoreExtreme    ES > 0 ? nGeEs : nLeEs                                nGeEs                      nLeEs
 * The six partials, their block order and the IEEE division rule are the same for all three types, and so are the NaN rules
 * (k = 0, k = N, a list with a NaN or an infinity).
 * Leading edge of (set j, list l), defined on the observed placement.  Let t_top be the smallest t with after_t == maxP
 * and t_bot the smallest t with before_t == minP: fp64 equality on the values the walk itself forms, the first occurrence
 * as R's which.max / which.min give it.
 *     top branch:     the members t = 1 .. t_top in walk order (decreasing stat); length t_top
 *     bottom branch:  the members t = k .. t_bot, from the end of the list backwards; length k - t_bot + 1
 *     std takes the top branch if maxP > -minP, the bottom branch if maxP < -minP, and is empty (length 0) if they tie;
 *     pos always takes the top branch and neg always the bottom branch, also where ES is 0.
 *     A NaN pair (k = 0, k = N, a NaN list) has length 0.
 * le_len is m x c int32 and le_idx is nnz x c int32, nnz = Gp[m]: the edge of (j, l) is le_idx[l nnz + Gp[j] + 0 .. len-1],
 * len = le_len[l m + j], row indices into stat (the numbering of Gi) in the order above; the rest of the set's segment is
 * -1.  An edge never exceeds k, so a set's own segment of G always holds it.  le_len and le_idx are passed both or neither.
 * plaidhip_gsea / plaidhip_gsea_multi are plaidhip_gsea_scored / _multi with PLAIDHIP_GSEA_STD and no edge buffers.  The
 * argument errors of plaidhip_gsea_scored, in this order: score_type outside 0..2, exactly one of le_len / le_idx null,
 * then those above.  Under plaidhip_gsea_scored_multi the edges are formed once, on the first device, after the reduction;
 * every sharding returns the one-device bits of out, null_out, le_len and le_idx.
 * Not offered: fgsea's multilevel p-values by these entries themselves (their smallest pval is 1 / (nperm + 1));
 * plaidhip_gsea_multilevel, below, adds them. */
#define PLAIDHIP_GSEA_PERM_BLOCK 64
#define PLAIDHIP_GSEA_STD 0
#define PLAIDHIP_GSEA_POS 1
#define PLAIDHIP_GSEA_NEG 2
int plaidhip_gsea(plaidhip_ctx* ctx, const double* stat, const double* weight, int32_t g, int32_t c, const int32_t* Gp,
                  const int32_t* Gi, int32_t m, const int32_t* perm, int32_t nperm, uint64_t seed, double* out,
                  double* null_out);
int plaidhip_gsea_multi(const int* devices, int ndev, const double* stat, const double* weight, int32_t g, int32_t c,
                        const int32_t* Gp, const int32_t* Gi, int32_t m, const int32_t* perm, int32_t nperm, uint64_t seed,
                        double* out, double* null_out);
int plaidhip_gsea_scored(plaidhip_ctx* ctx, const double* stat, const double* weight, int32_t g, int32_t c, const int32_t* Gp,
                         const int32_t* Gi, int32_t m, const int32_t* perm, int32_t nperm, uint64_t seed, int score_type,
                         double* out, double* null_out, int32_t* le_len, int32_t* le_idx);
int plaidhip_gsea_scored_multi(const int* devices, int ndev, const double* stat, const double* weight, int32_t g, int32_t c,
                               const int32_t* Gp, const int32_t* Gi, int32_t m, const int32_t* perm, int32_t nperm,
                               uint64_t seed, int score_type, double* out, double* null_out, int32_t* le_len,
                               int32_t* le_idx);
int plaidhip_gsea_permutations(plaidhip_ctx* ctx, int32_t g, int32_t nperm, uint64_t seed, int32_t* P_out);

/* plaid.gsea(multilevel = TRUE): p-values below 1 / (nperm + 1) by adaptive multilevel splitting with a one-gene Metropolis
 * move (the method of fgsea's multilevel routine, Korotkevich et al.).  fgsea's source is not in this tree: the estimator is
 * pinned here, operation for operation, and tested against these words and against exhaustive enumeration (DESIGN.md
 * section 23).  It has fgsea's reading -- pval, log2err -- not fgsea's bits.
 * Level function.  A RULER belongs to one (list l, side, set size k).  Positive side: ES > 0 under std, or pos; negative
 * side: ES < 0 under std, or neg.  A state is a k-subset S of the positions 0..N-1 of list l's observed placement; its
 * score h(S) is formed by the operations above over the list's Wpos (the B == 0 rule included):
 *     pos: maxP(S)     neg: -minP(S)     std, positive side: ES(S)     std, negative side: -ES(S)
 * The target of a set is gamma = |ES|.  A std set with ES == 0, or a NaN pair, has no ruler (its ml_out row is NaN).
 * Random numbers: Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (x, i, k, tag), i the sample slot and
 * tag = 0x80000000 | (l << 1) | side, l < 2^30: the high bit keeps the stream apart from the placements' counters
 * (i, b, 0, 0).  An integer in 0..R-1 from a word o is ((uint64)o * R) >> 32; a value's probability differs from 1 / R by
 * at most 2^-32, a relative bias of at most R / 2^32 (2^-15 at R = 131,072).
 * Initial states.  The sample size n is odd, 3 <= n <= PLAIDHIP_GSEA_ML_MAX_SAMPLE.  Draw d = 0, 1, ... of slot i is word
 * (d & 3) of the counter with x = 0x80000000 | (d >> 2), mapped to 0..N-1.  T0 = the first min(k, N - k) distinct values
 * of that sequence; S_i = T0 if 2 k <= N, otherwise its complement.
 * Stage l = 0, 1, ..., with P_0 = 1.0:
 *     1. m_l = the (n + 1) / 2-th smallest of h_0..h_{n-1};  2. s_l = #{h_i > m_l} (strictly: the levels rise strictly)
 *     3. the stage's n scores are recorded
 *     4. the ruler ends REACHED if m_l >= gamma_max, the largest target of its sets;  5. otherwise STALLED if s_l == 0
 *     6. otherwise P_{l+1} = P_l * ((double)s_l / (double)n), and it ends at the FLOOR if P_{l+1} < eps or
 *        l + 1 == PLAIDHIP_GSEA_ML_MAX_STAGES
 *     7. otherwise the j-th slot (in slot order) with h_i <= m_l takes a copy of the (j mod s_l)-th survivor in slot order
 *     8. every slot, survivors too, makes T = sweeps * k proposals (sweeps in 1..32).  Proposal `step` of slot i reads
 *        words o0, o1 of the counter with x = l * T + step (below 2^31):  a = (o0 * k) >> 32,  b = (o1 * N) >> 32.
 *        p_a = the a-th member of S_i in ascending position (0-based).  If bit b is set (b == p_a included) nothing moves;
 *        otherwise S' = S_i - {p_a} + {b} is taken iff h(S') > m_l.
 * Read-off of a set with target gamma: l* = the first stage with m_l >= gamma, or the last stage if there is none;
 * c = #{h_i of stage l* >= gamma}, c' = max(c, 1);
 *     qhat = P_{l*} * ((double)c' / (double)n)
 *     status = PLAIDHIP_GSEA_ML_ESTIMATED if a stage with m_l >= gamma existed, otherwise the ruler's end, _FLOOR or
 *              _STALLED, and qhat is then an upper bound
 *     log2err = sqrt(sum_{j < l*} (n - s_j) / ((double)n * s_j) + (n - c') / ((double)n * c')) / ln 2, the terms added
 *               in the order of j from 0.0, the last term last; formed on the host
 * A set's row depends on its own gamma, k, list, side and the seed, never on the sets that share its ruler.
 * The table: the permutation pass of plaidhip_gsea_scored runs unchanged (out, null_out, the edges), then
 *     denom = (1 + nGeZero) / (1 + nperm) on the positive side, (1 + nLeZero) / (1 + nperm) on the negative side
 *     pvalML = min(1, qhat / denom)
 *     pval (reported) = the permutation one where nMoreExtreme >= ml_min or the pair has no ruler, pvalML otherwise
 *     padj = Benjamini-Hochberg over the reported pval
 * ml_min = 0 returns plaidhip_gsea_scored's twelve columns bit for bit.
 * ml_out: m x 6 x c: pvalML, log2err, l*, status, qhat, denom.
 * plaidhip_gsea_ruler runs ONE ruler (one list: stat and weight are g long; k; the list's number l for the counter; side)
 * to the caller's gamma and returns its trace: *nstages, *end_status (PLAIDHIP_GSEA_ML_ESTIMATED for REACHED, _FLOOR,
 * _STALLED), m_out and s_out (PLAIDHIP_GSEA_ML_MAX_STAGES each) and h_out (MAX_STAGES x n, stage-major), filled for the
 * stages run.  It is to the chains what plaidhip_gsea_permutations is to the null.
 * Argument errors, in this order and before any device work: sample_size even or outside 3..PLAIDHIP_GSEA_ML_MAX_SAMPLE,
 * sweeps outside 1..32, eps not in [0, 1), ml_min < 0, c >= 2^30, a null ml_out, then plaidhip_gsea_scored's.
 * plaidhip_gsea_ruler: those of the first three, then side outside 0..1 (or against a pos / neg score type), l outside
 * 0..2^30-1, k outside 1..g-1, gamma NaN, then score_type, g and the weights as above.
 * plaidhip_gsea_multilevel_multi shares the rulers out as whole rulers (plaidhip_shard_bounds over the ruler list, which is
 * sorted by list, side and k); the read-off meets on the first device's thread: every sharding returns the one-device bits. */
#define PLAIDHIP_GSEA_ML_MAX_STAGES 256
#define PLAIDHIP_GSEA_ML_MAX_SAMPLE 1023
#define PLAIDHIP_GSEA_ML_ESTIMATED 0
#define PLAIDHIP_GSEA_ML_FLOOR 1
#define PLAIDHIP_GSEA_ML_STALLED 2
int plaidhip_gsea_multilevel(plaidhip_ctx* ctx, const double* stat, const double* weight, int32_t g, int32_t c,
                             const int32_t* Gp, const int32_t* Gi, int32_t m, const int32_t* perm, int32_t nperm, uint64_t seed,
                             int score_type, int32_t sample_size, int32_t sweeps, double eps, int32_t ml_min, double* out,
                             double* null_out, int32_t* le_len, int32_t* le_idx, double* ml_out);
int plaidhip_gsea_multilevel_multi(const int* devices, int ndev, const double* stat, const double* weight, int32_t g, int32_t c,
                                   const int32_t* Gp, const int32_t* Gi, int32_t m, const int32_t* perm, int32_t nperm,
                                   uint64_t seed, int score_type, int32_t sample_size, int32_t sweeps, double eps,
                                   int32_t ml_min, double* out, double* null_out, int32_t* le_len, int32_t* le_idx,
                                   double* ml_out);
int plaidhip_gsea_ruler(plaidhip_ctx* ctx, const double* stat, const double* weight, int32_t g, int32_t k, int32_t l, int side,
                        int score_type, double gamma, uint64_t seed, int32_t sample_size, int32_t sweeps, double eps,
                        int32_t* nstages, int32_t* end_status, double* m_out, int32_t* s_out, double* h_out);

/* plaid.fisher(sig, G): over-representation analysis -- Fisher's exact (hypergeometric) test of every list of significant
 * genes against every set, in three directions.  The form is fgsea::fora / fisher.test(alternative = "greater") AS
 * RECALLED: their source is not in this tree, so the statistic is pinned here, operation for operation, and tested against
 * these words and against exact rational arithmetic.
 * Operands: sig is g x c int8, column-major; sig[i, l] is -1 (gene i significant down in list l), 0 (not significant) or
 * +1 (significant up).  Any other value is PLAIDHIP_EINVAL, found on the host before any device work.  The universe is the
 * g rows: N = g.  The sets are Gp / Gi as everywhere else (rows of sig, 0-based).
 * Per list l:  nUp = #{i : sig[i, l] = +1},  nDn = #{i : sig[i, l] = -1}.  Per set j with k = Gp[j + 1] - Gp[j] members:
 * ovUp = #{members with sig = +1}, ovDn = #{members with sig = -1}.  All are exact integer counts.  Three directions:
 *     up:    K = nUp         x = ovUp
 *     down:  K = nDn         x = ovDn
 *     any:   K = nUp + nDn   x = ovUp + ovDn
 * Upper tail p = P(X >= x), X ~ Hypergeometric(N, K, k) (k draws from N genes of which K are marked), all in fp64, the
 * integers in 64 bits:
 *     lo = max(0, k + K - N);  hi = min(k, K)
 *     if x <= lo: p = 1.0;  if x > hi: p = 0.0;  otherwise
 *     t0 = clamp(floor((k + 1)(K + 1) / (N + 2)), lo, hi)                         (the mode: every other term is <= its own)
 *     u = 1.0;  total = 1.0;  upper = (t0 >= x) ? 1.0 : 0.0
 *     upwards, for t = t0 .. hi - 1 in order:
 *         u = (u * ((double)(K - t) * (double)(k - t))) / ((double)(t + 1) * (double)(N - K - k + t + 1))
 *         total += u;  upper += u if t + 1 >= x
 *     downwards, restart u = 1.0, for t = t0 .. lo + 1 descending:
 *         u = (u * ((double)t * (double)(N - K - k + t))) / ((double)(K - t + 1) * (double)(k - t + 1))
 *         total += u;  upper += u if t - 1 >= x
 *     p = upper / total
 * The integer products are exact (g <= PLAIDHIP_FISHER_MAX_GENES = 2^26, else PLAIDHIP_EUNSUPPORTED), so a step is one
 * rounded multiply and one rounded divide, and the additions run in exactly that order.  No product is contracted, and
 * there is no pow, lgamma or exp.  A term that underflows becomes 0 and stays 0 (adding it changes nothing, so a walk may
 * stop there).  Where the true p is at least 2^-900 the result lies within (4 n + 2) 2^-53 of it, relatively, n = hi - lo + 1
 * (DESIGN.md section 19 derives this); a true p below about 2^-900 may come back as any value in [0, 2^-890], including 0.
 * Odds ratio (the sample one, not fisher.test's conditional MLE): a = x, b = k - x, c' = K - x, d = N - k - K + x,
 *     OR = ((double)a * (double)d) / ((double)b * (double)c')          IEEE: x / 0 = Inf, 0 / 0 = NaN
 * NaN rule, as plaid.gsea's: k = 0 or k = N gives NaN in every column of that set except size, ovUp and ovDn.  K = 0 is not
 * special: x = 0, so p = 1.
 * padj is Benjamini-Hochberg per list and direction over the sets with a non-NaN p (the host routine behind plaid.gsea's
 * padj and q.meta).
 * out: m x 12 x c, column-major: size, ovUp, ovDn, pUp, pDn, pAny, padjUp, padjDn, padjAny, orUp, orDn, orAny.
 * tot_out: 2 x c doubles: nUp, nDn of every list.
 * ov_len (m x c int32) and ov_idx (nnz x c int32, nnz = Gp[m]) are passed both or neither, laid out as plaid.gsea's le_len /
 * le_idx: the overlap of (j, l) is ov_idx[l nnz + Gp[j] + 0 .. len-1], len = ov_len[l m + j] = ovUp + ovDn: the rows of set j
 * with sig != 0 in list l, in the set's own member order (the order of Gi); the rest of the set's segment is -1.
 * Argument errors, in this order: c < 1; bad dims or a null Gp; null sig or tot_out (or out, with m > 0); exactly one of
 * ov_len / ov_idx null; g > PLAIDHIP_FISHER_MAX_GENES (PLAIDHIP_EUNSUPPORTED); Gp not starting at 0 or decreasing, a null
 * Gi, or a Gi row outside 0..g-1; a bad sig value.  All are found on the host before any device is touched.  m = 0 returns
 * PLAIDHIP_OK with nothing written, as the other entries do.
 * plaidhip_fisher_multi shares the lists out over the devices (plaidhip_shard_bounds over c); a device takes the columns of
 * sig of its lists and all of G.  A list's results depend on that list alone and its counts are integers, so every
 * sharding, including ndev > c, returns the one-device bits of out, tot_out, ov_len and ov_idx.
 * plaidhip_hyper_tail is the tail above, the same inline function, on the host: no device is touched.  0 <= K, k <= N
 * (else PLAIDHIP_EINVAL), N <= PLAIDHIP_FISHER_MAX_GENES (else PLAIDHIP_EUNSUPPORTED), any x.  It applies no NaN rule.
 * Not offered: two-sided p-values and the conditional-MLE odds ratio. */
#define PLAIDHIP_FISHER_MAX_GENES (1 << 26)
#define PLAIDHIP_FISHER_LIST_TILE 8
int plaidhip_fisher(plaidhip_ctx* ctx, const int8_t* sig, int32_t g, int32_t c, const int32_t* Gp, const int32_t* Gi, int32_t m,
                    double* out, double* tot_out, int32_t* ov_len, int32_t* ov_idx);
int plaidhip_fisher_multi(const int* devices, int ndev, const int8_t* sig, int32_t g, int32_t c, const int32_t* Gp,
                          const int32_t* Gi, int32_t m, double* out, double* tot_out, int32_t* ov_len, int32_t* ov_idx);
int plaidhip_hyper_tail(int64_t N, int64_t K, int64_t k, int64_t x, double* p);

/* plaid.rankcor(stat, G): the Pearson correlation of a per-gene statistic, or of its ranks, with the 0/1 membership column
 * of every set -- the reference's gset.rankcor(fc, matG, compute.p = TRUE[, use.rank = FALSE]) (experiments/R/functions.R:
 * 183-237), one list (contrast, or sample) per column, with per-list missing values.
 * Operands: stat is g x c doubles, column-major; a NaN means "gene i takes no part in list l" (R's NA, na.last = "keep").
 * Per list: V = the rows that are not NaN, n = |V|.  Per set j: k = the number of its members (rows of Gi) in V.
 * RANK MODE (use_rank = 1).  r_i = the rank of stat[i] among V, ascending, +-Inf ordinary values, -0 == +0; ties is
 * PLAIDHIP_TIES_AVERAGE, _MIN or _MAX (the dense rank kernel's values, NaN kept).  The reference ranks with ties.method =
 * "random", which is no function of the input: the callers' default here is "average"; lists without ties are the same
 * under every method.  z_i = 2 r_i is an integer in 2 .. 2 n, and everything before the epilogue is exact integers:
 *     A = sum of z_i over the members in V;  T1 = sum of z_i over V;  T2 = sum of z_i^2 over V        (T2 <= 2^53)
 *     num = n A - k T1                               (|num| < 2^53: int64)
 *     P   = k (n - k) (n T2 - T1^2)                  (< 2^102: unsigned 128-bit)
 *     Q   = P - num^2                                (>= 0 by Cauchy-Schwarz; 128-bit)
 * The epilogue runs on the host in fp64; a 128-bit integer becomes a double by ONE rounding to nearest, ties to even:
 *     P == 0 (k = 0, k = n, an all-tied list, n <= 1): rho = t = p = NaN
 *     Q == 0: rho = +-1.0 (the sign of num), t = +-Inf, p = 0.0;  otherwise
 *     rho = (double)num / sqrt((double)P)
 *     tsq = ((double)(n - 2) * (double)(num^2)) / (double)Q;   t = copysign(sqrt(tsq), num);   p = 2.0 * pnorm_upper(|t|)
 *     n <= 2: t = p = NaN, whatever Q is.
 * pnorm_upper(x) = 0.5 * erfc(x / sqrt(2.0)), the routine behind every normal tail of this library.  rho lies within
 * 3 * 2^-53 of the exact value, relatively, and t within 4 * 2^-53 (DESIGN.md section 21 derives 2.5 and 3).
 * VALUE MODE (use_rank = 0).  A list whose V holds an infinity, or whose values over V are all equal (max == min), gives NaN
 * in rho, t, p and q.  mu = (the sum of stat over V) / (double)n, d_i = stat[i] - mu (one rounding each), and
 *     A = sum of d_i over the members in V;  T1 = sum of d_i over V;  T2 = sum of d_i * d_i over V
 *     num = A - ((double)k * T1) / (double)n
 *     den = sqrt((((double)k * (double)(n - k)) / (double)n) * (T2 - (T1 * T1) / (double)n))
 *     rho = num / den            (den == 0 or not finite, k = 0, k = n: NaN)
 *     w   = (1.0 - rho) * (1.0 + rho);   w <= 0: t = copysign(Inf, rho), p = 0.0;   otherwise
 *     t   = rho * sqrt((double)(n - 2) / w);   p = 2.0 * pnorm_upper(|t|);   n <= 2: t = p = NaN
 * This is the correlation for ANY shift mu (the centred two-pass form; never sum x^2 - n mu^2).  No product is contracted.
 * The order of every fp64 sum is fixed by the launch geometry alone, never by the sharding or the number of lists:
 *   over V (the sum for mu, then T1 and T2): thread h of 256 adds rows h, h + 256, ... in ascending order from 0.0 (a row
 *   outside V is skipped), and the 256 partials are added pairwise, partial[h] += partial[h + s] for s = 128, 64, ..., 1;
 *   over a set: lane h of 64 adds the members in V at positions h, h + 64, ... of the set's segment of Gi in ascending order
 *   from 0.0, and the lanes are added by the butterfly v += (v of lane h xor s) for s = 32, 16, 8, 4, 2, 1.
 * q.value is Benjamini-Hochberg per list over the sets with a non-NaN p (the host routine behind every padj here).
 * out: m x 5 x c doubles, column-major: size (k), rho, t, p.value, q.value.  tot_out: c doubles, n of every list.
 * Argument errors, in this order, all found on the host before any device is touched: c < 1; bad dims or a null Gp; null
 * stat or tot_out (or out, with m > 0); use_rank not 0 / 1 or ties not one of the three; g > PLAIDHIP_RANKCOR_MAX_GENES
 * (PLAIDHIP_EUNSUPPORTED); Gp not starting at 0 or decreasing, a set of more than g members, a null Gi, or a Gi row outside
 * 0..g-1.  m = 0 returns PLAIDHIP_OK with nothing written.
 * plaidhip_rankcor_multi shares the lists out over the devices (plaidhip_shard_bounds over c); a device takes its columns of
 * stat and all of G.  A list's results depend on that list alone, so every sharding, ndev > c included, returns the
 * one-device bits of out and tot_out.
 * plaidhip_rankcor_finish (host only, no device): the rank-mode epilogue and Benjamini-Hochberg on integer operands: n, T1,
 * T2: c each; k, A: m x c, list-major (set j of list l at l m + j); out as above.  Operands outside the ranges above
 * (n < 0, k outside 0..n, n > PLAIDHIP_RANKCOR_MAX_GENES, T1 < 0, T2 < 0, P < num^2) are PLAIDHIP_EINVAL.
 * Not offered: a dgCMatrix stat; ties = "random"; the reference's cor_sparse_matrix for a non-binary gset. */
#define PLAIDHIP_RANKCOR_MAX_GENES 131072
#define PLAIDHIP_RANKCOR_LIST_TILE 8
int plaidhip_rankcor(plaidhip_ctx* ctx, const double* stat, int32_t g, int32_t c, const int32_t* Gp, const int32_t* Gi, int32_t m,
                     int use_rank, int ties, double* out, double* tot_out);
int plaidhip_rankcor_multi(const int* devices, int ndev, const double* stat, int32_t g, int32_t c, const int32_t* Gp,
                           const int32_t* Gi, int32_t m, int use_rank, int ties, double* out, double* tot_out);
int plaidhip_rankcor_finish(int32_t m, int32_t c, const int64_t* n, const int64_t* T1, const int64_t* T2, const int64_t* k,
                            const int64_t* A, double* out);

/* replaid.zscore(X, G) and replaid.plage(X, G): the other two methods of GSVA::gsva(), the reference's
 * gset.gsva(X, geneSets, method = "zscore" | "plage") (experiments/R/functions.R:148-160); DESIGN.md section 22.
 * Operands: X is g x n doubles, column-major, or the slots of a dgCMatrix (sorted, distinct row indices), which is expanded
 * on the device and scored as its dense form: the same bits.  G is aligned to X's rows (Gp, Gi).  n >= 2.
 * STANDARDIZATION, per gene row over all n samples, fp64, GSVA's scale() (no 1e-8, unlike replaid.gsva):
 *     mean = (sum of x) / (double)n;   ss = sum of (x - mean)^2;   sd = sqrt(ss / (double)(n - 1));   z = (x - mean) / sd
 * Both sums run over the samples 0, 1, ..., n - 1 in that order from 0.0, one addition each (the order of
 * kcdf_row_moments_kernel, kernels_kcdf.hip); d = x - mean and d * d are rounded before they are added.
 *   sd == 0: a constant gene.  It is left out of every set, as GSVA's filter does: a set's effective size k counts its other
 *   members (a member listed twice counts twice).
 *   sd not finite (the row holds a NaN or an infinity, or its sum of squares overflows): the row stays a member, and every
 *   score of every set that contains it is NaN.  Other sets are untouched.
 * ZSCORE (Lee et al. 2008).  S[s, j] = (sum of z_ij over the kept members of s) / sqrt((double)k_s); the sum is the crossprod
 * of plaidhip_plaid_dense with stat = sum on Z (a constant row holds 0.0 there), the division and the square root are
 * correctly rounded.  k_s == 0 gives NaN.  size_out (nullable): the m effective sizes.
 * PLAGE (Tomfohr et al. 2005).  Z_s is the k x n block of the set's kept rows in G's own order, C = Z_s Z_s' (k x k; n - 1
 * times the genes' correlation matrix), u the unit eigenvector of C's largest eigenvalue lambda, and the score
 *     v_j = (sum over i of u_i z_ij) / sqrt(lambda)                 (svd(Z_s)$v[, 1] up to sign)
 * summed over the kept members in G's order from 0.0, each product rounded before it is added.  k == 0 gives a NaN row;
 * k == 1 gives u = (1), lambda = C_00 and v = z / sqrt(lambda).
 *   C.  C_ab = the sum over the samples 0, 1, ..., n - 1, in that order from 0.0, of the products z_aj z_bj, each ROUNDED
 *   before it is added (no fused operation; the rows are padded with zeros to a multiple of 16 samples, which adds exact
 *   zeros).  The order depends on nothing but n.  C_ab is computed once for a <= b and mirrored, so C is symmetric bit for
 *   bit, and two rows whose products cancel term by term (the orthogonal pair [1,-1,1,-1], [1,1,-1,-1]) give an exact 0.
 *   (The fp64 matrix instruction v_mfma_f64_16x16x4_f64 adds unrounded products and leaves a rounding residue there (1.9e-18 of
 *   lambda on that pair): the kernel built on it stays behind a test hook)
 *   Start.  u = the column of C with the largest squared 2-norm (sum over j = 0..k-1 in order of C_ji^2; the lowest index
 *   at a tie), divided by the square root of that sum.  (Never the all-ones vector: for k = 2 it is always an eigenvector,
 *   and for a negatively correlated pair the wrong one.)
 *   Step t = 1, 2, ...: y = C u (y_i = sum over j = 0..k-1 in order of C_ij u_j), lambda = u'y, r = ||y - lambda u||_2.
 *   Stop when r <= tol * lambda (converged = 1) or when t == maxit (converged = 0: the last iterate is returned);
 *   otherwise u = y / ||y||_2.  The returned u is the one lambda and r were computed for.
 *   The sums over i (u'y, the norms, and those of the orientation and the trace) run in one fixed tree: thread h of 256
 *   adds its elements h, h + 256, ... in ascending order from 0.0, then partial[h] += partial[h + w] for w = 128, 64, ..., 1.
 *   No product is contracted into an add anywhere.
 *   Orientation, part of the definition: s = sum of u_i, a = sum of |u_i|.  If |s| > 2^-20 a, u is oriented so that s > 0
 *   (the score rises when the set's genes rise on average).  Otherwise the first kept member in G's order with
 *   |u_i| >= max|u| / 2 is made positive (member 0 of a negatively correlated pair).
 *   info_out (nullable): m x 6 doubles, column-major: size (the effective k), lambda, explained = lambda / trace(C) (the
 *   trace summed from the computed diagonal), iterations (the steps taken), residual = r / lambda, converged.  A set with
 *   k == 0 or with a flagged member reports its size, NaN in lambda, explained and residual, and 0 in the other two.
 *   load_out (nullable): Gp[m] doubles, u in the set's own segment of G (the layout of plaidhip_gsea_scored's le_idx); the
 *   entry of a dropped constant member is 0.0, the kept members of a NaN set hold NaN.
 * tol (the callers' default 2^-40) and maxit (1000) are arguments, as in any eigensolver.
 * Argument errors, in this order, all found on the host before any device is touched: bad dims or a null Gp; n < 2;
 * (plage) tol not > 0 (a NaN included), maxit < 1; Gp not starting at 0 or decreasing; (plage) a set of more than
 * PLAIDHIP_PLAGE_MAX_SET members; with m > 0: a null X, S_out or Gi, a malformed dgCMatrix, a Gi row outside 0..g-1.
 * m = 0 returns PLAIDHIP_OK with nothing written.
 * The _multi forms send all of X to every device, as rowtf = "gauss" does: every device standardizes and (plage) forms C
 * and u of every set -- redundant by design, the same code in the same order, hence the same bits -- and then scores its
 * own sample columns (plaidhip_shard_bounds over n).  Every sharding, ndev > n included, returns the one-device bits.
 * Not offered: sets shared out over devices; sets above the cap; GSVA's Poisson kernel. */
#define PLAIDHIP_PLAGE_MAX_SET 4096
int plaidhip_plage(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m,
                   double tol, int32_t maxit, double* S_out, double* info_out, double* load_out);
int plaidhip_plage_csc(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx, int32_t g, int32_t n,
                       const int32_t* Gp, const int32_t* Gi, int32_t m, double tol, int32_t maxit, double* S_out, double* info_out,
                       double* load_out);
int plaidhip_plage_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g,
                         int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double tol, int32_t maxit, double* S_out,
                         double* info_out, double* load_out);
int plaidhip_zscore(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m,
                    double* S_out, double* size_out);
int plaidhip_zscore_csc(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx, int32_t g, int32_t n,
                        const int32_t* Gp, const int32_t* Gi, int32_t m, double* S_out, double* size_out);
int plaidhip_zscore_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g,
                          int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double* S_out, double* size_out);

/* plaid.limma(A, design, contrasts): limma's moderated t-test -- lmFit + eBayes + topTable -- of every row of A (the
 * single-sample scores of the sets, or the expression of the genes) for one or several designs.  The form is limma's AS
 * RECALLED: its source is not in this tree, so the statistic is pinned here and tested against these words in 50-digit
 * arithmetic and against an independent least-squares restatement.
 * Operands: A rows x n doubles, column-major, one row per set or gene.  nfit designs D_f, each n x p column-major, D_f at
 * design + f * n * p; p is the same for every fit, 1 <= p <= PLAIDHIP_LIMMA_MAX_COEF.  use: n x nfit int8, column-major,
 * 0 = the sample takes no part in fit f (NULL: every sample in every fit).  K: the contrasts, p x q column-major, shared
 * by the fits (NULL: the p unit vectors, and q must be p).  For fit f, sel are its used samples and n_f their number.
 * 1. The design, on the host in fp64.  Householder QR without pivoting of the rows sel of D_f, column k reflected by
 *    x - alpha e_1 with alpha = -sign(x_1) ||x||_2 (sign(0) = +1), R_kk = alpha: Q_f (n x p, thin, the rows of excluded
 *    samples zero) and R_f (p x p, upper).  Column k is rank-deficient when |R_kk| <= 1e-7 ||D_f[sel, k]||_2.
 *    For contrast j: v_j = R_f^-T K_j by forward substitution, u_j = sqrt(sum_k v_jk^2) in ascending k (limma's
 *    stdev.unscaled), and logFC = v_j' E = sum_k v_jk E_k by fma in ascending k from 0.0, on the host: no coefficient
 *    vector is formed.
 * 2. Per row, on the device (kernels_lmfit.hip), x_c = A[r, c], all in fp64 with no contracted product but the fma written:
 *      E_k = sum over c of (c in sel ? fma(x_c, Q_f[c, k], .) : unchanged)
 *      M   = the same with the weight 1.0 / (double)n_f for Q_f[c, k]                         (AveExpr)
 *      r_c = fma(-Q_f[c, p-1], E_{p-1}, ... fma(-Q_f[c, 0], E_0, x_c))                        (ascending k, from x_c)
 *      RSS = sum over c of (c in sel ? r_c * r_c : 0.0), from the reduced E of ALL samples; never sum x^2 - sum E^2
 *      s2  = RSS / (n_f - p)
 *    Every sum runs over the columns of a block of 128 in ascending order from 0.0, and the blocks are added in ascending
 *    order.  The select form matters: an excluded sample may hold NaN or Inf, and it does not reach a fit that left it out.
 * 3. eBayes per fit, on the host (squeezeVar / fitFDist; no trend, not robust), d = n_f - p:
 *      rows with a finite s2 are "ok", n_ok their number; the other rows get NaN in every column and take no part;
 *      x = max(s2, 1e-5 m), m = median(s2) over the ok rows (the mean of the middle two for an even count), m = 1 if it is 0;
 *      e = log x - digamma(d / 2) + log(d / 2);   ebar = mean(e);   v = sum (e - ebar)^2 / (n_ok - 1) - trigamma(d / 2);
 *      v > 0:  df.prior = 2 y with trigamma(y) = v,  s2.prior = exp(ebar + digamma(y) - log y);
 *      else:   df.prior = +Inf,  s2.prior = mean(x);
 *      n_ok < 2: df.prior = 0, s2.prior = NaN, and the test is the ordinary t;
 *      s2.post = (d s2 + d0 s0^2) / (d + d0), s0^2 when d0 is infinite, s2 when d0 is 0;   df.total = min(d + d0, n_ok d);
 *      t = logFC / (u_j sqrt(s2.post));   P.Value = 2 pt(-|t|, df.total) (the tail of plaid.test, a real df);
 *      adj.P.Val = Benjamini-Hochberg over the rows of each (fit, contrast), NaN rows apart.
 *    digamma and trigamma: the recurrence up to an argument >= 10, then the asymptotic series.  The root of trigamma(y) = v
 *    is pinned as a property (to a relative 1e-12 in y or better for 1e-6 <= v <= 1e7), not as an iteration; outside that
 *    range limma's own closed forms stand: y = 1 / sqrt(v) for v > 1e7 and y = 1 / v for v < 1e-6.
 * out: rows x 6 x q x nfit doubles, column-major: logFC, AveExpr, t, P.Value, adj.P.Val, sigma2 (the unmoderated s2), in
 * the row order of A; contrast j of fit f at out + (f * q + j) * 6 * rows.
 * hyper: nfit x 4 doubles, row-major per fit: df.residual, df.prior, s2.prior, n_ok.
 * rows == 0, nfit == 0 or q == 0: PLAIDHIP_OK with nothing written.
 * Argument errors, in this order, all PLAIDHIP_EINVAL and all found on the host before any device is touched: bad dims
 * (rows, n, nfit, q < 0, nfit > PLAIDHIP_LIMMA_MAX_FITS, n > PLAIDHIP_LIMMA_MAX_SAMPLES); p outside 1..PLAIDHIP_LIMMA_MAX_COEF; K == NULL with q != p; a null design; a null A, out or
 * hyper where something is to be written; a non-finite entry of K; then fit by fit: a non-finite entry of a used row of
 * D_f, n_f - p < 1, a rank-deficient column -- with a message naming the fit and the column (or sample), counted from 1.
 * A non-finite entry of an unused row of D_f is accepted.
 * How: the W = nfit (p + 1) weight columns of all fits (p columns of Q_f, then use / n_f) lie side by side and are cut into
 * tiles of PLAIDHIP_LIMMA_TILE; a thread owns two adjacent rows and keeps a tile's accumulators in registers, so A is read
 * ceil(W / tile) times for the effects and nfit times for the RSS.
 * plaidhip_limma_multi shards the SAMPLES over the devices at multiples of 128 columns.  The effects are handed from shard
 * to shard as [W][rows], then every shard takes the RSS of its columns from the full effects and hands it on as
 * [nfit][rows]; every sharding, with more shards than samples too, has the bits of the one-device call.
 *   plaidhip_dev_row_design_effects / _rss: the two passes on device pointers, stream-ordered.  A: rows x n, leading
 *     dimension ld.  Q: n x p x nfit doubles (Q_f column-major at Q + f n p), use: n x nfit int8 or NULL, invn: nfit doubles,
 *     1 / n_f.  E: [W][rows], fit f's p effects then its M at rows f (p + 1) ...  rss: [nfit][rows].  seed (NULL: zeros):
 *     the sums of the shards before this one, of the result's shape.  _rss takes the E of ALL shards, as
 *     plaidhip_dev_row_contrast_ssd takes the means of all shards.  The partials live in the context's workspace.
 *   plaidhip_limma_design (host only): step 1 for one design: Q (n x p), R (p x p column-major), v (p x q), u (q), *nf;
 *     each may be NULL.  `fit` is the number its messages name.
 *   plaidhip_limma_finish (host only): step 3 and the output from E ([W][rows]), rss ([nfit][rows]), nf (nfit), v
 *     (p x q x nfit) and u (q x nfit).  Tails and Benjamini-Hochberg are dealt to at most 8 host threads.
 * Not offered: trend = TRUE and robust = TRUE; the B-statistic and the F-statistic; a dgCMatrix input; fusing a scorer with
 * the test so that the scores never leave the device.  In plaidhip_limma a NaN in a used sample makes the row NaN;
 * plaidhip_limma_na (below) refits such a row on the samples it has; plaidhip_limma_w (below) takes array and observation
 * weights.
 *
 * plaidhip_limma_na / _na_multi: na = "fit", limma's handling of per-row missing values (lmFit refits a row with NA on the
 * samples it has) and gx.limma's max.na.  The operands of plaidhip_limma plus max_na, and dfres.  DESIGN.md section 24.
 * - Missing is NaN only (R's NA / NaN).  Inf is a value: a used Inf makes the row NaN, as above.
 * - max_na: a row whose share of NaN over ALL n columns, (double)count / (double)n, exceeds max_na is not fitted in any fit:
 *   NaN in every column, no part in eBayes (rowMeans(is.na(X)) <= max.na).  max_na = 0 refuses every row with a NaN.
 * - For fit f and row r: mis = the samples of sel that are NaN in the row, obs = sel \ mis.  E' and M' are step 2's sums
 *   with the select "c in sel and x_c == x_c", in the same order; a row without NaN in sel has the bits of plaidhip_limma,
 *   skips the solve (gamma = E exactly) and has the fit's u_j.
 * - An incomplete row: with q_c = row c of Q_f, for every pair (k, l <= k)
 *     s = sum over mis in ascending c of fma(q_ck, q_cl, .) from 0.0 -- one chain --,   H_kl = (k == l ? 1.0 : 0.0) - s.
 *   H = L L' by Cholesky without pivoting, row by row: L_kl = (H_kl - sum_{m<l} L_km L_lm) / L_ll, the pivot d_k = H_kk -
 *   sum_{m<k} L_km^2, L_kk = sqrt(d_k), every sum a chain of fma(-a, b, .) in ascending m from H_kl.  L y = E' forward and
 *   L' gamma = y backward, the sums likewise in ascending m (from E'_k, from y_k), then one division.  For contrast j:
 *   w = L^-1 v_j forward, u_j = sqrt(sum_k fma(w_k, w_k, .)) ascending from 0.0 (stdev.unscaled of the row), and logFC =
 *   sum_k v_jk gamma_k as in step 1.  AveExpr = (M' * (double)n_f) / (double)|obs|.  RSS is step 2's chain at gamma instead
 *   of E with the extended select; s2 = RSS / d_r, d_r = |obs| - p.  The chain's step, the factorisation with the
 *   substitutions, u_j and the mean are inline functions of csrc/lmfit_na.h, one copy for the device and for
 *   plaidhip_limma_na_solve (a GPU test holds the device to that entry bit for bit).  The chain runs over the row's own missing samples, so the result does not
 *   depend on the launch geometry or on the sharding.
 * - Estimability is a rule: row r is not estimable in fit f when a pivot d_k <= 1e-10 (or is NaN) or |obs| - p < 1.  Then it
 *   is NaN in that fit and not ok.  A pivot is 1 minus the leverage the missing samples hold on direction k, so 1e-10 would
 *   be a 1e10-fold variance inflation; rounding leaves about (|mis| + p) 2^-52 in a pivot that is exactly 0.  limma would
 *   still report the estimable coefficients of such a row (NA for the others); this does not.
 * - eBayes with unequal df: limma's classic moment estimator fitFDist with a vector df1 (newer limma releases fit unequal
 *   df by another route).  Over the ok rows (finite s2) of the fit, d_r as above:
 *     e_r = log x_r - digamma(d_r / 2) + log(d_r / 2);   v = sum (e - ebar)^2 / (n_ok - 1) - mean_r trigamma(d_r / 2)
 *     s2.post_r = (d_r s2_r + d0 s0^2) / (d_r + d0);   df.total_r = min(d_r + d0, df.pooled),  df.pooled = sum_r d_r
 *   with sums in ascending row order.  Where all ok rows share one d the mean of trigamma is trigamma(d / 2) itself and
 *   df.pooled is n_ok d: step 3 as it stands above, to the bit.
 * - dfres: rows x nfit doubles, column-major: d_r of every ok (row, fit), NaN for the others.  hyper: nfit x 5 row-major:
 *   the four of plaidhip_limma (df.residual = n_f - p, the complete rows') and df.pooled.
 * - p <= PLAIDHIP_LIMMA_NA_MAX_COEF: the lower triangle of H is held by the lanes of one wavefront.  gx.limma's designs are
 *   intercept + group + a few batch columns.
 * - Argument errors: those of plaidhip_limma in their order, with, after "p outside 1..PLAIDHIP_LIMMA_MAX_COEF": p >
 *   PLAIDHIP_LIMMA_NA_MAX_COEF, then max_na outside [0, 1] or NaN; and a null dfres after "a null A, out or hyper".
 * - How: a count pass (a thread per row and block of 128 columns: coalesced, and with the host's prefix sums over (row,
 *   block) a row's NaN columns come out ascending with no atomic; counts first, then the columns into space sized from the
 *   total) and per (fit, row) counts inside sel; the incomplete pairs form a work list; Gram and solve with one wavefront
 *   per pair (lane = one entry of the triangle, the sample's row of Q_f through LDS once), writing gamma where the RSS pass
 *   reads E.  _na_multi: sample shards at multiples of 128 columns; counts add, the lists concatenate in shard order, and
 *   one device runs the work list on the concatenated lists: every sharding, with more shards than samples too, has the
 *   one-device bits.  A failing shard reports and nothing is written.
 *   plaidhip_limma_na_solve (host only): one incomplete row.  qmis: nmis x p row-major, the rows q_c of its missing samples
 *     in ascending c; Ep: E' (p); nobs = |obs|; v: p x q.  Writes gamma (p), u (q), *ok and the pivots d_k (p, may be
 *     NULL; NaN past the pivot that broke the rule).
 *   plaidhip_limma_finish_na (host only): plaidhip_limma_finish with drow ([nfit][rows]: d_r, NaN for a row that is not
 *     fitted) and urow ([nfit q][rows]) in place of u, and hyper nfit x 5.
 *
 * plaidhip_limma_w / _w_multi: lmFit with precision weights -- limma's `weights` (observation weights: voom's, or quality
 * weights from upstream) and array weights -- then eBayes and topTable as above.  DESIGN.md section 28.  The operands of
 * plaidhip_limma_na plus Wt (rows x n doubles, column-major, may be NULL) and aw (n doubles, may be NULL); both NULL is
 * PLAIDHIP_EINVAL (plaidhip_limma and plaidhip_limma_na are the entries without weights).  The outputs are those of
 * plaidhip_limma_na: out, hyper (nfit x 5) and dfres.  A missing value is a weight of 0: this is the general case of na = "fit".
 * - Effective weight: omega_rc = Wt[r, c] * aw[c], one rounded product; a NULL operand counts as 1.0 and no product is taken.
 * - Live observations: (r, c) is live in fit f iff c is in sel_f, x_rc == x_rc, and 0 < omega_rc < +Inf.  As in limma, a
 *   weight that is zero, negative, NaN or infinite makes the observation missing.  A live +-Inf VALUE makes the row NaN in
 *   that fit, as above.
 * - max_na keeps its meaning: the share of NaN in x over all n columns; weights do not count.
 * - The basis: Q_f, R_f and v_j are exactly step 1 of plaidhip_limma, the UNWEIGHTED QR of the design; the weights enter
 *   per row.  Per fit, a table of n x p (p + 1) / 2 products pi_c,kl = q_ck * q_cl (l <= k), each rounded once.
 * - Per row, on the device (kernels_lmfit_w.hip); every sum runs over the columns of a block of 128 in ascending order from
 *   0.0 and the blocks are added in ascending order, the rule of step 2:
 *     H_kl = live ? fma(omega_rc, pi_c,kl, .) : unchanged                  (l <= k)
 *     b_k  = live ? fma(y_rc, q_ck, .) : unchanged,   y_rc = omega_rc * x_rc rounded once
 *     M'   = step 2's chain with the select "c in sel and x == x" and the weight 1 / n_f, IGNORING omega
 *     AveExpr = (M' * (double)n_f) / (double)count, count the size of that select
 *   (limma's rowMeans(y, na.rm = TRUE): a value with a zero weight still counts in AveExpr).
 * - The solve: H = L L', L y = b, L' gamma = y, u_j and logFC = v_j' gamma by the inline functions of csrc/lmfit_na.h that
 *   na = "fit" uses, in their order.  The pivot rule is RELATIVE here: the row is not estimable when a pivot d_k <=
 *   1e-10 * H_kk (one rounded product; H_kk the diagonal entry before elimination) or d_k is NaN.  H scales with the
 *   weights, and scaling all weights by a power of two commutes with every rounding, so it changes no logFC bit and no
 *   decision.  (na = "fit" keeps its absolute rule, to the bit: the factorisation takes the tolerance as a parameter.)
 * - Degrees of freedom: d_r = |live| - p; d_r < 1 is not estimable.  A pair that is not estimable, or whose row is above
 *   max_na, is NaN in that fit and not ok.
 * - Residuals: r_c is step 2's fma chain from x_c at gamma;  RSS = live ? fma(omega_rc, r_c * r_c, .) : unchanged, with
 *   r_c * r_c rounded first;  s2 = RSS / d_r.
 * - eBayes and the output: plaidhip_limma_finish_na as it stands, with drow = d_r and urow = the rows' u_j.
 * - All weights 1 with no NaN is NOT the bits of plaidhip_limma (H is summed, not taken as I); it agrees with it within the
 *   bound of DESIGN.md section 28, and the integers (dfres, n_ok, df.pooled) are equal.
 * - p <= PLAIDHIP_LIMMA_NA_MAX_COEF.
 * - Argument errors: those of plaidhip_limma_na in their order, with, after "max_na outside [0, 1] or NaN": Wt and aw both
 *   NULL, then nfit (p (p + 1) / 2 + p + 1) weight columns in more than 65,535 tiles of PLAIDHIP_LIMMA_TILE.  The entries of
 *   Wt and aw are not checked: what is not a positive finite number is a missing observation.
 * - How: a table kernel (the products and the masks), one fused pass that reads x and omega once per column and tile of 8
 *   of the nfit (p (p + 1) / 2 + p + 1) weight columns (pi, q and 1 / n_f are wave-uniform; the per-row factor is omega, y or
 *   x by the column's kind), a count pass (|live|, the mean's count and the row's NaN as exact doubles that take the road of
 *   the sums), the solve with one thread per (row, fit) and H in LDS, and the weighted RSS pass.  _w_multi: sample shards at
 *   multiples of 128 columns; the sums and counts are handed from shard to shard as seeds, one device solves, and the RSS is
 *   handed on likewise: every sharding, with more shards than samples too, has the one-device bits.  A failing shard reports
 *   and nothing is written.
 *   plaidhip_dev_limma_w_sums / _w_rss: the passes on device pointers, stream-ordered.  A and Wt: rows x n with the leading
 *     dimension ld (Wt may be NULL), aw: n or NULL, Q / use / invn as plaidhip_dev_row_design_effects.  S: [nfit Wc][rows], Wc
 *     = p (p + 1) / 2 + p + 1: fit f's triangle of H row by row, then b, then M'.  cnt (may be NULL): [2 nfit + 1][rows]:
 *     |live| and the mean's count of every fit, then the row's NaN.  seed / seed_cnt (NULL: zeros): the sums of the shards
 *     before this one.  _w_rss: rss [nfit][rows] at G ([nfit (p + 1)][rows]: gamma of every pair; the mean's row is not read).
 *   plaidhip_limma_w_solve (host only): one row from its sums, the one copy of the arithmetic the device runs
 *     (lmfit_w_row_solve).  Htri: H's lower triangle row by row (p (p + 1) / 2), b (p), nlive = |live|, v: p x q.  Writes
 *     gamma (p), u (q), *ok and the pivots d_k (p, may be NULL; NaN past the pivot that broke the rule).
 *   Both dev entries take Wt and aw both NULL as well (omega = 1.0 everywhere): they are passes, not the fit.
 * Not offered (out of scope): weights in plaid.camera, plaid.fry and plaid.roast; voomWithQualityWeights, arrayWeights and
 * duplicateCorrelation (estimating weights or correlations); trend and robust.
 *
 * plaidhip_voom / _voom_multi: plaid.voom(counts, design, lib.size = NULL, span = 0.5), limma's voom with normalize.method =
 * "none" AS RECALLED: counts to log2-CPM and a precision weight for every observation from the mean-variance trend, for one
 * design and all samples.  Its E and weights feed plaidhip_limma_w (limma's lmFit on an EList).  DESIGN.md section 28.
 * Operands: counts rows x n doubles, column-major; design n x p, 1 <= p <= PLAIDHIP_LIMMA_MAX_COEF; lib_size n doubles or NULL.
 * 1. The check, on the device before anything is written: every count is finite and >= 0, else PLAIDHIP_EINVAL.  Column
 *    sums: thread t of 256 adds the rows t, t + 256, ... of the column in ascending order from 0.0 and the 256 partials are
 *    folded in halves (s_t += s_{t + off}, off = 128, 64, ..., 1) -- exact for integer counts with sums < 2^53, whatever the
 *    order.  lib.size L_c = lib_size[c], or the column sum when NULL.  Row sums: over the columns of a block of 128 in
 *    ascending order from 0.0, the blocks added in ascending order; a row is "all zero" iff its row sum is 0.
 * 2. E_rc = log2(((counts_rc + 0.5) / (L_c + 1.0)) * 1e6), in that operation order, on the device (its log2).
 * 3. The unweighted fit of E on the design: steps 1 and 2 of plaidhip_limma give the effects E_k, the mean M and RSS;
 *    s2 = RSS / (n - p).
 * 4. Trend points, on the host: sx = M + (ml - log2(1e6)), ml = (sum over c ascending from 0.0 of log2(L_c + 1.0)) / n, and
 *    sy = sqrt(sqrt(s2)), over the rows that are not all zero and have a finite s2, sorted by sx, ties in row order.  No
 *    such row: PLAIDHIP_EINVAL.
 * 5. lowess(sx, sy, f = span, iter = 3, delta = 0.01 * (max - min)) on the host: plaidhip_lowess below.
 * 6. The knots are the anchor points of lowess's last pass -- where the local fit or a tie copy was made -- with their fitted
 *    values, one per distinct x (the first): at most PLAIDHIP_VOOM_MAX_KNOTS, else PLAIDHIP_EINVAL (with this delta there are
 *    at most 202: every second anchor lies more than delta beyond the one two back).  f(lambda): the end values outside the
 *    knots (rule = 2: Y_0 for lambda <= X_0, Y_last for lambda >= X_last); else bisection (lo = 0, hi = last; mid = (lo + hi)
 *    / 2 takes lo when X_mid <= lambda, else hi, until hi - lo = 1) finds the largest k with X_k <= lambda and
 *    f = Y_k + (Y_{k+1} - Y_k) * ((lambda - X_k) / (X_{k+1} - X_k)), which is exactly Y_k at a knot.
 * 7. Weights, on the device: mu_rc = the fma chain of Q[c, k] E_k in ascending k from 0.0; lambda_rc = mu_rc + offset_c with
 *    offset_c = log2(L_c + 1.0) - log2(1e6) made on the host and returned; w_rc = 1.0 / ((f * f) * (f * f)).  limma goes
 *    through 2^mu and back to the log scale; this stays on it (a stated deviation, a few ulp of lambda).  f <= 0 or NaN gives
 *    the weight NaN, which plaidhip_limma_w treats as a missing observation.
 * Outputs: E and W rows x n column-major; lib_out and offset n; knots_x and knots_y PLAIDHIP_VOOM_MAX_KNOTS doubles each (NaN
 * past *nknots).  rows == 0 or n == 0: PLAIDHIP_OK with nothing written.  Nothing is written before every device pass of
 * every shard is done.
 * Argument errors, in this order, PLAIDHIP_EINVAL before any device is touched: bad dims; p outside
 * 1..PLAIDHIP_LIMMA_MAX_COEF; span outside (0, 1] or NaN; a null design; a null counts or output; a lib_size entry that is not
 * finite and >= 0; then the design's own faults as plaidhip_limma reports them.  Then, on the device: a bad count.
 * plaidhip_voom_multi shards the SAMPLES at multiples of 128 columns: every pass is column-local except the check's flag, the
 * row sums and the fit's sums, which are handed from shard to shard in the order of the one-device call; one shard fits the
 * trend.  Every sharding, with more shards than samples too, has the one-device bits.
 *   plaidhip_dev_voom_weights: step 7 on device pointers, stream-ordered: Q n x p, offset n, Eff [p + 1][rows] (the effects;
 *     the last row is not read), the knots, W rows x n with leading dimension ldw.  nknots outside 1..PLAIDHIP_VOOM_MAX_KNOTS
 *     is PLAIDHIP_EINVAL with nothing written.
 *   plaidhip_lowess (host only): R's lowess AS RECALLED.  x ascending and finite, n >= 1; ys: n fitted values; anchor (may be
 *     NULL): n flags, 1 where the last pass made a local fit or a tie copy.  ns = max(2, min(n, floor(f n + 1e-7))); robustness
 *     weights start at 1; iter + 1 fitting passes.  A pass: i = 0, last = -1, window [nleft, nright] = [0, ns - 1]; while
 *     nright < n - 1 and x_i - x_nleft > x_(nright+1) - x_i the window moves right by one; ys_i is the local fit (y_i if it
 *     fails); the points between last and i get alpha ys_i + (1 - alpha) ys_last, alpha = (x_j - x_last) / (x_i - x_last);
 *     last = i, cut = x_last + delta; scan forward from last + 1 until x > cut, a point with x == x_last copies ys and becomes
 *     last; i = max(last + 1, stop - 1); the pass ends when last >= n - 1.  The local fit at xs: h = max(xs - x_nleft, x_nright
 *     - xs); for j from nleft upward with r = |x_j - xs| <= 0.999 h: w_j = 1 if r <= 0.001 h, else t = r / h, u = 1 - (t t) t,
 *     w_j = (u u) u, times the robustness weight from the second pass on; stop at the first x_j > xs outside 0.999 h; it fails
 *     if sum w <= 0; else w is normalised and, if h > 0: a = sum w x, c = sum w ((x - a)(x - a)), and if sqrt(c) > 0.001 (x_max
 *     - x_min): w_j *= ((xs - a) / c)(x_j - a) + 1; ys = sum w y.  After every pass but the last: res = y - ys; cmad = 6 median
 *     |res| (the mean of the middle two for even n); stop if cmad < 1e-7 mean|res|; the robustness weight is 1 for |res| <=
 *     0.001 cmad, (1 - (res / cmad)^2)^2 up to 0.999 cmad, 0 beyond.  Every sum ascending from 0.0, no fused operation.
 * Not offered (out of scope): normalize.method other than "none"; voomWithQualityWeights, arrayWeights, duplicateCorrelation;
 * trend and robust; a dgCMatrix of counts; weights in plaid.camera, plaid.fry and plaid.roast. */
#define PLAIDHIP_VOOM_MAX_KNOTS 256
#define PLAIDHIP_LIMMA_MAX_COEF 32
#define PLAIDHIP_LIMMA_NA_MAX_COEF 10         /* 10 * 11 / 2 = 55 entries of the triangle <= the 64 lanes of a wavefront */
#define PLAIDHIP_LIMMA_TILE 8
#define PLAIDHIP_LIMMA_MAX_FITS 15000         /* nfit (p + 1) / tile and nfit are launch grid extents, at most 65,535 each */
#define PLAIDHIP_LIMMA_MAX_SAMPLES 8388480    /* 65,535 column blocks of 128: a launch grid extent as well */
int plaidhip_limma(plaidhip_ctx* ctx, const double* A, int32_t rows, int32_t n, const double* design, int32_t p, int32_t nfit,
                   const int8_t* use, const double* K, int32_t q, double* out, double* hyper);
int plaidhip_limma_multi(const int* devices, int ndev, const double* A, int32_t rows, int32_t n, const double* design,
                         int32_t p, int32_t nfit, const int8_t* use, const double* K, int32_t q, double* out, double* hyper);
int plaidhip_dev_row_design_effects(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const double* Q,
                                    const int8_t* use, const double* invn, int32_t p, int32_t nfit, const double* seed,
                                    double* E);
int plaidhip_dev_row_design_rss(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const double* Q,
                                const int8_t* use, int32_t p, int32_t nfit, const double* E, const double* seed, double* rss);
int plaidhip_limma_design(const double* D, int32_t n, int32_t p, const int8_t* use, const double* K, int32_t q, int32_t fit,
                          double* Q, double* R, double* v, double* u, int64_t* nf);
int plaidhip_limma_finish(int32_t rows, int32_t p, int32_t nfit, int32_t q, const double* E, const double* rss,
                          const int64_t* nf, const double* v, const double* u, double* out, double* hyper);
int plaidhip_limma_tile(void);   /* PLAIDHIP_LIMMA_TILE of the built library */
int plaidhip_limma_na(plaidhip_ctx* ctx, const double* A, int32_t rows, int32_t n, const double* design, int32_t p, int32_t nfit,
                      const int8_t* use, const double* K, int32_t q, double max_na, double* out, double* hyper, double* dfres);
int plaidhip_limma_na_multi(const int* devices, int ndev, const double* A, int32_t rows, int32_t n, const double* design,
                            int32_t p, int32_t nfit, const int8_t* use, const double* K, int32_t q, double max_na, double* out,
                            double* hyper, double* dfres);
int plaidhip_limma_na_solve(int32_t p, int32_t nmis, const double* qmis, const double* Ep, int64_t nobs, const double* v,
                            int32_t q, double* gamma, double* u, double* pivots, int32_t* ok);
int plaidhip_limma_finish_na(int32_t rows, int32_t p, int32_t nfit, int32_t q, const double* E, const double* rss,
                             const int64_t* nf, const double* v, const double* drow, const double* urow, double* out,
                             double* hyper);
int plaidhip_limma_w(plaidhip_ctx* ctx, const double* A, const double* Wt, const double* aw, int32_t rows, int32_t n,
                     const double* design, int32_t p, int32_t nfit, const int8_t* use, const double* K, int32_t q, double max_na,
                     double* out, double* hyper, double* dfres);
int plaidhip_limma_w_multi(const int* devices, int ndev, const double* A, const double* Wt, const double* aw, int32_t rows,
                           int32_t n, const double* design, int32_t p, int32_t nfit, const int8_t* use, const double* K, int32_t q,
                           double max_na, double* out, double* hyper, double* dfres);
int plaidhip_dev_limma_w_sums(plaidhip_ctx* ctx, const double* A, const double* Wt, const double* aw, int64_t ld, int32_t rows,
                              int32_t n, const double* Q, const int8_t* use, const double* invn, int32_t p, int32_t nfit,
                              const double* seed, double* S, const double* seed_cnt, double* cnt);
int plaidhip_dev_limma_w_rss(plaidhip_ctx* ctx, const double* A, const double* Wt, const double* aw, int64_t ld, int32_t rows,
                             int32_t n, const double* Q, const int8_t* use, int32_t p, int32_t nfit, const double* G,
                             const double* seed, double* rss);
int plaidhip_limma_w_solve(int32_t p, const double* Htri, const double* b, int64_t nlive, const double* v, int32_t q,
                           double* gamma, double* u, double* pivots, int32_t* ok);
int plaidhip_voom(plaidhip_ctx* ctx, const double* counts, int32_t rows, int32_t n, const double* design, int32_t p,
                  const double* lib_size, double span, double* E, double* W, double* lib_out, double* offset, double* knots_x,
                  double* knots_y, int32_t* nknots);
int plaidhip_voom_multi(const int* devices, int ndev, const double* counts, int32_t rows, int32_t n, const double* design,
                        int32_t p, const double* lib_size, double span, double* E, double* W, double* lib_out, double* offset,
                        double* knots_x, double* knots_y, int32_t* nknots);
int plaidhip_dev_voom_weights(plaidhip_ctx* ctx, const double* Q, const double* offset, int32_t n, int32_t p, const double* Eff,
                              int32_t rows, const double* knots_x, const double* knots_y, int32_t nknots, double* W, int64_t ldw);
int plaidhip_lowess(const double* x, const double* y, int64_t n, double f, int32_t iter, double delta, double* ys,
                    int8_t* anchor);

/* plaid.camera(X, design, G, contrasts): limma's competitive gene-set test camera (Wu & Smyth 2012) for every set, contrast
 * and design -- the one common set test that corrects a set's p-value for the correlation between its genes.  The form is
 * limma's camera.default AS RECALLED: its source is not in this tree, so the statistic is pinned here and tested against
 * these words restated literally (a complete QR of the design, U = Q2'x / sigma) in 50-digit arithmetic.
 * Operands: X is g x n doubles, column-major, one row per gene; the designs D_f, use and the contrasts K are those of
 * plaidhip_limma; G is aligned to X's rows (Gp, Gi; a member listed twice counts twice).  d = n_f - p.
 * 1. The fit: steps 1 to 3 of plaidhip_limma, unchanged.  For (fit f, contrast j) the gene statistic is plaid.limma's t,
 *    t_g = logFC / (u_j sqrt(s2.post)) (camera's unscaledt / sqrt(var.post)).  A gene that is not ok in fit f (s2 not
 *    finite) leaves that fit's universe, as a NaN does in plaid.rankcor: G_f is the number of ok genes, the size m of a set
 *    counts its ok members only.  df.camera = min(d + df.prior, G_f - 2) -- not plaid.limma's df.total.
 * 2. Standardised residuals, per fit, on the device (kernels_camera.hip): r_gc is step 2's chain of plaidhip_limma from the
 *    reduced effects of ALL samples, fma(-Q_f[c, k], E_k, .) in ascending k from x_c, and
 *      z_gc = r_gc / sqrt(max(s2_g, 1e-8))  for a used sample and an ok gene,  0.0 otherwise,    s2_g = RSS_g / d:
 *    one square root per gene and one division per element, both correctly rounded; no reciprocal is formed.  The chain's
 *    step, the gene's divisor and the select are inline functions of csrc/camera.h, one copy for the device and for
 *    plaidhip_camera_residual_row (a GPU test holds the device to that entry bit for bit).
 * 3. The variance inflation factor of a set with m > 1.  limma forms U = Q2'x / sigma (g x d, Q2 an orthonormal basis of
 *    the residual space) and takes m * mean(colMeans(U[set, ])^2).  Every residual lies in the span of Q2, so that value is
 *      vif = || sum over the set's members of z_g ||^2 / (m d),
 *    the norm taken in sample space over the n samples: no n x n matrix and no second QR.  T = G'Z (m x n) is the dense
 *    crossprod of plaidhip_plaid_dense (stat = sum, fp64) applied to Z.  The squares t * t of a row of T, each rounded, are
 *    added over the columns of a block of 128 in ascending order from 0.0, and the blocks are added in ascending order: the
 *    order of the RSS pass.  correlation = (vif - 1) / (m - 1).  m = 1: vif = 1, correlation = NaN.  m = 0: both NaN.
 *    allow_neg_cor = 0 (limma's default) uses max(vif, 1) in the test; the reported VIF and correlation stay as estimated.
 * 4. A fixed correlation, inter_gene_cor = rho inside (-1, 1) (limma's current default is 0.01; NaN asks for step 3):
 *    vif = 1 + (m - 1) rho as it stands (no max), correlation = rho, for every set with m >= 1.  Steps 2 and 3 are skipped
 *    entirely: no Z is formed.
 * 5. The test of (fit, contrast, set), plaidhip_camera_finish: fp64 on the host, sums over the genes in ascending order
 *    from 0.0.  Over the ok genes' t: mean = sum / G; var = sum of (t - mean)^2 / (G - 1) (two passes).  m2 = G - m,
 *      delta  = (G / m2) * (sumt / m - mean)                    sumt: the member sum of t
 *      pooled = ((G - 1) var - ((delta delta) m m2) / G) / (G - 2)
 *      T_set  = delta / sqrt(pooled * (vif / m + 1 / m2))
 *      Down = pt(T_set, df.camera), Up the upper tail, from h = pt(-|T_set|, df.camera) (the tail of plaid.test, a real
 *      df) and 1 - h;  PValue = 2 min(Down, Up);  Direction = Up if Up < Down, else Down (the callers' column);
 *      FDR = Benjamini-Hochberg over the sets of each (fit, contrast), NaN rows apart.
 *    t, Down, Up, PValue and FDR are NaN when m = 0, m2 = 0, G < 3, pooled <= 0 or pooled * (vif / m + 1 / m2) <= 0 (a
 *    negative fixed rho on a large set); NGenes, Correlation and VIF are reported as in steps 3 and 4 all the same.
 *    The member sums of t and the counts m come from ONE crossprod of the membership with [the t columns | the ok
 *    indicators] (a gene that is not ok holds 0.0 in both); the counts are sums of 0 / 1 in fp64: exact.
 * out: m x 8 x q x nfit doubles, column-major: NGenes, Correlation, VIF, t, Down, Up, PValue, FDR; contrast j of fit f at
 * out + (f * q + j) * 8 * m.  hyper: nfit x 6 doubles, row-major per fit: plaid.limma's four (df.residual, df.prior,
 * s2.prior, n_ok), then G_f and df.camera.  g == 0, nfit == 0, q == 0 or m == 0: PLAIDHIP_OK with nothing written.
 * Argument errors, all PLAIDHIP_EINVAL and all found on the host before any device is touched: m < 0; those of
 * plaidhip_limma in their order (named "camera:"); then a null Gp, Gp not starting at 0 or decreasing, a set of more than g
 * members, a null Gi, a Gi row outside 0..g-1; then inter_gene_cor outside (-1, 1) unless it is NaN.
 * How: Z is materialised and the crossprod reused -- gathering the members' rows of X set by set would read X about twelve
 * times over at 5,000 sets of 50.  One fit's Z (g x n_shard) and T live in the context's buffers at a time.
 * plaidhip_camera_multi shards the SAMPLES at multiples of 128 columns as plaidhip_limma_multi does; after its two rounds a
 * third hands the sums of T^2 from shard to shard as [nfit][m].  T's columns do not depend on the sharding, the partial
 * sums are those of the one-device call: every sharding, with more shards than samples too, has the one-device bits.
 *   plaidhip_dev_camera_residuals: step 2 on device pointers, stream-ordered.  A: rows x n, leading dimension ld; Q, use as
 *     in plaidhip_dev_row_design_rss; E [nfit (p + 1)][rows] and rss [nfit][rows] of ALL samples; `fit` counted from 0;
 *     d = n_f - p; Z: rows x n, leading dimension ldz.  The masks live in the context's workspace.
 *   plaidhip_dev_camera_sumsq: out[s] = seed[s] (NULL: 0.0) + the block sums of T[s, c]^2 in ascending order; T: m x n,
 *     leading dimension ldt.  A thread owns one set and one block of 128 columns; the partials live in the workspace.
 *   plaidhip_camera_residual_row (host only): step 2 for one gene: x (n), Q (n x p column-major, Q_f), use (n, or NULL),
 *     E (p), the gene's rss and d; z (n).
 *   plaidhip_camera_finish (host only): step 5.  t: g x q x nfit; ok: g x nfit int8; sumt: m x q x nfit; cnt: m x nfit;
 *     ss: m x nfit, the sums of T^2 (NULL: the fixed inter_gene_cor); dfres, dfprior: nfit; gdf: nfit x 2 (G_f, df.camera).
 * Not offered: use.ranks = TRUE (the rank-sum form); trend.var; array or observation weights; a dgCMatrix X; na = "fit"
 * rows (limma's camera refuses NA; here such a gene leaves the universe); fry / roast. */
int plaidhip_camera(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, const double* design, int32_t p, int32_t nfit,
                    const int8_t* use, const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi, int32_t m,
                    double inter_gene_cor, int allow_neg_cor, double* out, double* hyper);
int plaidhip_camera_multi(const int* devices, int ndev, const double* X, int32_t g, int32_t n, const double* design, int32_t p,
                          int32_t nfit, const int8_t* use, const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi,
                          int32_t m, double inter_gene_cor, int allow_neg_cor, double* out, double* hyper);
int plaidhip_dev_camera_residuals(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const double* Q,
                                  const int8_t* use, int32_t p, int32_t nfit, int32_t fit, const double* E, const double* rss,
                                  double d, double* Z, int64_t ldz);
int plaidhip_dev_camera_sumsq(plaidhip_ctx* ctx, const double* T, int64_t ldt, int32_t m, int32_t n, const double* seed,
                              double* out);
int plaidhip_camera_residual_row(int32_t n, int32_t p, const double* x, const double* Q, const int8_t* use, const double* E,
                                 double rss, double d, double* z);
int plaidhip_camera_finish(int32_t g, int32_t m, int32_t nfit, int32_t q, const double* t, const int8_t* ok, const double* sumt,
                           const double* cnt, const double* ss, const double* dfres, const double* dfprior,
                           double inter_gene_cor, int allow_neg_cor, double* out, double* gdf);

/* plaid.fry(X, design, G, contrasts): limma's SELF-CONTAINED rotation gene-set test in closed form -- fry, the limit of
 * roast for infinitely many rotations (Wu et al. 2010; Giner & Smyth) -- for every set, contrast and design.  camera asks
 * whether a set moves more than the other genes; fry asks whether the set is differential at all.  It draws no random
 * number: the result is a pure function of the input.  The form is limma's fry.default / .fryEffects AS RECALLED: the source
 * is not in this tree, so the statistic is pinned here and tested against these words restated at 50 digits (DESIGN.md
 * section 26).  Operands as plaidhip_camera.  For fit f: d = n_f - p >= 1, contrast j has plaid.limma's v_j and u_j.
 * 1. The fit and the divisors: steps 1 to 3 of plaidhip_limma, unchanged.  s2_g = RSS_g / d; s2.post_g is eBayes' posterior
 *    variance with the prior (df.prior, s2.prior) of plaidhip_limma_finish, bit for bit (one function makes both).  The
 *    divisor c_g is sqrt(s2.post_g) for standardize = 0 ("posterior.sd", the default), sqrt(s2_g) for 1 ("residual.sd") and
 *    1.0 for 2 ("none"); "p2" is not offered.  A gene that is not ok in the fit (s2 not finite: a NaN or Inf in a used
 *    sample), or whose divisor is 0 or not finite, leaves the fit's universe -- a stated deviation: limma would divide by
 *    it.  Sets count their members inside the universe only: m.
 * 2. The standardised effects of gene g are the row F_g = [ e_gj | rho_g ] of length d + 1:
 *      e_gj  = logFC_gj / (u_j c_g)                       with the posterior sd exactly plaid.limma's moderated t
 *      z_gc  = r_gc / c_g for a used sample, else 0.0     r_gc: camera's chain, fma(-Q_f[c, k], E_k, .) ascending k from x_c
 *      rho_g = Q2' z_g                                    Q2: the n_f - p other columns of the full Householder Q of step 1
 *    (the reflectors applied, last first, to the identity's columns p .. n_f - 1, scattered to the used samples).  z comes
 *    from kernels_fry.hip's residual pass: camera's with c_g read instead of derived; the chain step and the select are
 *    inline functions of csrc/camera.h and csrc/fry.h, one copy for the device and for plaidhip_fry_residual_row.  rho is
 *    d more weight columns of plaid.limma's effects pass run over Z: rho_gk = sum over c of fma(z_gc, Q2[c, k], .) over the
 *    columns of a block of 128 ascending from 0.0, the blocks added ascending.  |sum_g rho_g| = |sum_g z_g| (Q2 is an
 *    isometry on the residual space).
 * 3. Directional, for every n:  T = G'Z by the dense crossprod, the sums of T^2 as in step 3 of plaidhip_camera, and
 *      t = (sum_g e_gj / m) / sqrt(|sum_g z_g|^2 / ((m m) d)),    PValue = 2 pt(-|t|, d)  -- the df is d, not d + df.prior.
 *    Direction is Down (-1) if t < 0, else Up (+1); NaN where t is NaN.  m = 0: NaN.  IEEE decides 0 / 0 and x / 0.
 * 4. Mixed, for fits with d + 1 <= PLAIDHIP_FRY_MIXED_MAX.  M_j = F_S' F_S ((d + 1) x (d + 1)) over the set's members,
 *    D = min(m, d + 1), lambda_1 >= ... >= lambda_D its D largest eigenvalues (limma's svd(EffectsSet)$d^2):
 *      SA = tr M_j,  SA2 = |M_j|_F^2,   den = lambda_1 - lambda_D
 *      Fobs = (sum_g e_gj^2 - lambda_D) / den
 *      bm = 1 / D,   bv = (D - 1) / (D D) / (D / 2 + 1)
 *      Fm = (SA bm - lambda_D) / den
 *      Fv = (bv SA2 - bv / (D - 1) (SA SA - SA2)) / (den den)
 *      ab = Fm (1 - Fm) / Fv - 1,   alpha = ab Fm,   beta = ab - alpha
 *      PValue.Mixed = pbeta(Fobs, alpha, beta, lower.tail = FALSE)
 *    m = 1: PValue.Mixed = PValue.  alpha or beta not finite or not positive (lambda_1 = lambda_D among them): NaN.
 *    On the device, on the first context: fry_gram_kernel (a workgroup per set) makes C = sum_g rho_g rho_g', and per
 *    contrast b_j = sum_g e_gj rho_g and a_j = sum_g e_gj^2 -- every entry one accumulator from 0.0 over the members in the
 *    order of Gi, the product rounded, then added -- and
 *      tr M_j = a_j + sum_i C_ii,    |M_j|_F^2 = (a_j a_j + 2 sum_i b_ji^2) + sum_i (sum_k C_ik^2),
 *    every sum ascending from 0.0 with rounded squares.  fry_eigen_kernel (a workgroup per (set, contrast)) holds
 *    M_j = [a_j, b_j'; b_j, C] in LDS and runs cyclic two-sided Jacobi in the round-robin tournament order, until the
 *    off-diagonal mass is at most 2^-53 |M_j|_F or 30 sweeps; lambda_D is picked BY INDEX from the sorted diagonal (for
 *    m < d + 1 the eigenvalues past m are rounding noise about 0 and are never picked).  The eigenvalues are pinned as a
 *    property -- within max(4 x LAPACK's own deviation, D 2^-53) lambda_1 of the exact spectrum of M_j -- not as bits.
 *    A fit above the cap has NaN in PValue.Mixed and FDR.Mixed and 0 in its hyper flag; its other columns are complete.
 * 5. FDR, FDR.Mixed: Benjamini-Hochberg over the sets of each (fit, contrast), NaN rows apart (plaidhip_fry_finish).
 * out: m x 7 x q x nfit doubles, column-major: NGenes, Direction, t, PValue, FDR, PValue.Mixed, FDR.Mixed; contrast j of
 * fit f at out + (f * q + j) * 7 * m.  hyper: nfit x 7 doubles, row-major per fit: plaid.limma's four (df.residual,
 * df.prior, s2.prior, n_ok), the universe's size, d + 1, and 1.0 / 0.0: the mixed test was offered.
 * g == 0, nfit == 0, q == 0 or m == 0: PLAIDHIP_OK with nothing written.
 * Argument errors, all PLAIDHIP_EINVAL and all found on the host before any device is touched: m < 0; those of
 * plaidhip_limma in their order (named "fry:"); the membership's as plaidhip_camera makes them; then standardize outside
 * 0..2; then q > PLAIDHIP_FRY_MAX_CONTRASTS.
 * plaidhip_fry_multi shards the SAMPLES at multiples of 128 columns: after plaid.limma's two rounds shard 0 makes the
 * divisors from the RSS of ALL samples, a third round chains the sums of T^2 and, fit by fit under the cap, a round
 * chains rho as [d + 1][g] (the last column, a mean, is not used).  Every partial sum is that of the one-device call, and
 * the Gram and eigen stages run once, after the chains: every sharding has the one-device bits.
 *   plaidhip_dev_fry_residuals: step 2's z on device pointers; plaidhip_dev_camera_residuals with cg ([nfit][rows]) in place
 *     of rss and d.
 *   plaidhip_dev_fry_residual_effects: rho [d + 1][rows] = seed (NULL: 0.0) + the block sums of Z Q2 (row d, the effects
 *     pass's mean column with weight 0.0, is not used); Z: rows x n, leading dimension ldz; Q2: n x d column-major; use: n
 *     or NULL; d <= PLAIDHIP_FRY_MIXED_MAX - 1.  Synchronises the stream before it returns.
 *   plaidhip_dev_fry_gram: rho: rows x d ROW-major, e: rows x q row-major (both 0.0 outside the universe), Gp / Gi device
 *     pointers; C: m x d x d, b: m x q x d, a, tr, fro: m x q.
 *   plaidhip_dev_fry_eigen: nprob matrices M (dim x dim each, symmetric), Dk (nprob int32, from 1): lam1, lamD, sweeps,
 *     converged per problem.
 *   plaidhip_fry_q2, _fry_divisors, _fry_residual_row, _fry_finish (host only): Q2 of one design (n x (n_f - p)); step 1's
 *     c_g [nfit][rows] (NaN: outside the universe) from rss [nfit][rows]; step 2's z for one gene; steps 3 to 5 from
 *     dres (nfit), cnt (m x nfit), sume (m x q x nfit), ss (m x nfit) and, mixed (nfit int8, may be NULL) saying where,
 *     sume2, lam1, lamD, trM, froM (m x q x nfit each).
 * Not offered: roast and mroast (random rotations); gene weights; array or observation weights; trend.var; robust; a
 * dgCMatrix X; na = "fit" rows; standardize = "p2". */
#define PLAIDHIP_FRY_MIXED_MAX 128            /* d + 1 effects: M in LDS with an odd row stride is 129 KiB of the CU's 160 */
#define PLAIDHIP_FRY_MAX_CONTRASTS 32
int plaidhip_fry(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, const double* design, int32_t p, int32_t nfit,
                 const int8_t* use, const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi, int32_t m,
                 int standardize, double* out, double* hyper);
int plaidhip_fry_multi(const int* devices, int ndev, const double* X, int32_t g, int32_t n, const double* design, int32_t p,
                       int32_t nfit, const int8_t* use, const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi,
                       int32_t m, int standardize, double* out, double* hyper);
int plaidhip_dev_fry_residuals(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const double* Q,
                               const int8_t* use, int32_t p, int32_t nfit, int32_t fit, const double* E, const double* cg,
                               double* Z, int64_t ldz);
int plaidhip_dev_fry_residual_effects(plaidhip_ctx* ctx, const double* Z, int64_t ldz, int32_t rows, int32_t n,
                                      const double* Q2, const int8_t* use, int32_t d, const double* seed, double* rho);
int plaidhip_dev_fry_gram(plaidhip_ctx* ctx, const double* rho, const double* e, int32_t rows, int32_t d, int32_t q,
                          const int32_t* Gp, const int32_t* Gi, int32_t m, double* C, double* b, double* a, double* tr,
                          double* fro);
int plaidhip_dev_fry_eigen(plaidhip_ctx* ctx, const double* M, int32_t dim, int64_t nprob, const int32_t* Dk, double* lam1,
                           double* lamD, int32_t* sweeps, int32_t* converged);
int plaidhip_fry_q2(const double* D, int32_t n, int32_t p, const int8_t* use, int32_t fit, double* Q2, int64_t* nf);
int plaidhip_fry_divisors(int32_t rows, int32_t p, int32_t nfit, const double* rss, const int64_t* nf, int standardize,
                          double* cg);
int plaidhip_fry_residual_row(int32_t n, int32_t p, const double* x, const double* Q, const int8_t* use, const double* E,
                              double c, double* z);
int plaidhip_fry_finish(int32_t m, int32_t nfit, int32_t q, const double* dres, const double* cnt, const double* sume,
                        const double* ss, const double* sume2, const double* lam1, const double* lamD, const double* trM,
                        const double* froM, const int8_t* mixed, double* out);

/* plaid.roast(X, design, G, contrasts): limma's rotation gene-set test with SAMPLED rotations (Wu et al. 2010) -- the test
 * that plaid.fry is the closed-form limit of -- for every set, contrast and design.  What it adds to plaid.fry: a mixed test
 * for any number of samples, and the set statistics mean50 (limma's default for roast), floormean and msq beside mean.  The
 * form is limma's roast / mroast AS RECALLED, pinned here: the source is not in this tree, so the tests hold the code to these
 * words restated at 50 digits.  Operands as plaidhip_fry.  For fit f: d = n_f - p >= 1; contrast j
 * has plaid.limma's logFC_gj, u_j (stdev.unscaled), the gene's RSS_g, and the prior (df0, s0^2) of plaidhip_limma_finish.
 * limma rotates a gene's effects [beta | rho] (rho = Q2' r, the d residual effects) by random unit vectors R of length
 * d + 1.  Here the rotation is taken in SAMPLE space: rho . R2 = r . w with w = Q2 R2, and a Gaussian R2 gives w the law of
 * (I - Q1 Q1') nu for a Gaussian n_f-vector nu; |[beta | rho]|^2 = beta^2 + RSS.  Neither rho, Q2 nor an n x n matrix is
 * ever made, so there is no cap on the samples.
 * 1. Universe: a gene that is not ok in the fit (s2 not finite: a NaN or Inf in a used sample) leaves it.  Sets count their
 *    members inside the universe only: m.
 * 2. Rotations k = 0 .. nrot - 1 of fit f (counted from 0), shared by every set and contrast of the fit (as romer shares
 *    them; mroast draws fresh ones per set -- a stated deviation).  Index i = 0 is nu_0, i = c + 1 the used sample c:
 *      (x0, x1, x2, x3) = Philox4x32-10(counter = (i, k, f, 0x726f6173), key = (seed mod 2^32, seed / 2^32))
 *      u1 = (((x0 2^32 + x1) >> 11) + 1) 2^-53,   u2 = ((x2 2^32 + x3) >> 11) 2^-53
 *      nu_i = sqrt(-2 log(u1)) cos(2 pi u2)                       (Box-Muller, the cosine branch)
 *      a_k = sum_c Q1[c, k] nu_c ascending c from 0.0;  wt_c = nu_c - (sum_k Q1[c, k] a_k ascending k from 0.0)
 *      s = sqrt(nu_0^2 + sum_c wt_c^2 ascending),   r0 = nu_0 / s,   w_c = wt_c / s;   0.0 on the samples the fit leaves out.
 *    The sum under the root is kept in double-double -- every square split exactly by an fma, the terms added by two-sum,
 *    fp64 operations only -- and s is sqrt(hi) corrected once by (hi - s s + lo) / (2 s): the rounded root of the sum, the
 *    same bits on every IEEE host.
 *    Q1 is plaid.limma's thin Q of the design.  A draw is a function of (seed, f, k, i) alone.  They are made on the host
 *    (plaidhip_roast_rotations); W is (n + 1) x nrot row-major: W[0][k] = r0, W[c + 1][k] = w_c.  Every entry also takes the
 *    caller's own W (rotations != NULL: nfit matrices), as they are.
 * 3. The rotated moderated statistic of gene g under rotation k, beta = logFC_gj / u_j (roast.h, one copy for all):
 *      B = beta r0 rounded, then fma(r_gc, w_c, .) over ALL samples c ascending (r_gc: plaid.fry's residual chain with a
 *          divisor of 1.0; 0.0 on a sample left out)
 *      s2r = (beta beta + RSS_g - B B) / d, and 0.0 unless that is > 0
 *      post = (df0 s0^2 + d s2r) / (df0 + d);   df0 infinite: s0^2;   df0 = 0 (fewer than two ok genes): s2r
 *      t = B / sqrt(post)                         IEEE decides x / 0
 *    The OBSERVED column is plaid.limma's moderated t itself, bit for bit -- not a rotation with r0 = 1.
 * 4. z-score on nu = min(df0 + d, 10,000) degrees of freedom (the winsorised df; also what makes an infinite df0 finite).
 *    zscore = 0 ("hill", the default), Hill's (1970) form: A = nu - 1/2, C = 48 A A, y = A log1p(t t / nu),
 *      z = sign(t) sqrt(y) (1 + ((y + 3) + (((-0.4 y - 3.3) y - 24) y - 85.5) / ((0.8 y y + 100) + C)) / C)
 *    every operation rounded on its own in this order.  zscore = 1 ("none"): z = t.  limma's exact qnorm(pt()) is not
 *    offered (an incomplete beta per element).  A gene outside the universe has beta = NaN and so z = NaN; no set reads it.
 * 5. The set statistic, four sides (down, up, upordown, mixed) over the m members' z; upordown = up if up > down, else
 *    down.  set_statistic 0 "mean": up = S / m, down = -S / m with S = sum z, mixed = sum |z| / m.  1 "floormean":
 *    down = sum max(-z, 0) / m, up = sum max(z, 0) / m, mixed = sum max(|z|, sqrt(q)) / m with q = qchisq(0.5, 1), sqrt(q) =
 *    0.67448975019608171.  2 "msq": down = sum over z < 0 of z z / m, up = sum over z > 0 of z z / m, mixed = sum z z / m.
 *    3 "mean50" (the default): h = floor(m / 2) + 1; up is the mean of the h largest z, down of the h largest -z, mixed of
 *    the h largest |z|, pinned without a sort: the keys are z + 0.0, (-z) + 0.0, |z| (no -0.0 among them), tau the h-th
 *    largest key, and the side is ((sum of the keys > tau in the set's own order) + (h - #{> tau}) tau) / h.  A NaN among a
 *    set's z makes its three mean50 sides NaN.  Every sum is ONE accumulator from 0.0 over the members in the order of
 *    Gi (the squares rounded first), so the sides are reproducible bit for bit from the z.  mean50 holds a set's z in LDS:
 *    a set with more than PLAIDHIP_ROAST_MEAN50_MAX members in the universe has NaN p-values under mean50 and raises the
 *    hyper flag; the other three statistics take any m.
 * 6. b = #{k : stat_k >= stat_obs} per side (exact integers), p = (b + 1) / (nrot + 1).  PropDown, PropUp: the shares of the
 *    members with observed z < -sqrt(2), z > sqrt(2).  Direction is Up (+1) where p_up < p_down, else Down (-1).  PValue is
 *    the upordown side, PValue.Mixed the mixed side.  FDR, FDR.Mixed: Benjamini-Hochberg over the sets of each (fit,
 *    contrast); with midp (the default) taken on p - 0.5 / (nrot + 1) and then raised to at least p.  m = 0: NaN but NGenes.
 * out: m x 8 x q x nfit doubles, column-major: NGenes, PropDown, PropUp, Direction, PValue, FDR, PValue.Mixed, FDR.Mixed;
 * contrast j of fit f at out + (f * q + j) * 8 * m.  hyper: nfit x 7 doubles: plaid.limma's four (df.residual, df.prior,
 * s2.prior, n_ok), the universe's size, nrot, and 1.0 where a set was above the mean50 cap (else 0.0).
 * g == 0, nfit == 0, q == 0 or m == 0: PLAIDHIP_OK with nothing written.
 * Argument errors, all PLAIDHIP_EINVAL and all found on the host before any device is touched: those of plaidhip_fry in
 * their order without its standardize (named "roast:"); then set_statistic outside 0..3; zscore outside 0..1; nrot < 1;
 * nrot > PLAIDHIP_ROAST_MAX_ROTATIONS.
 * On the device (kernels_roast.hip): roast_rotate_kernel fuses steps 3 and 4 and writes z as [tile of 64 rotations][g][64],
 * in chunks of whole tiles of at most PLAIDHIP_ROAST_Z_BYTES; roast_stat_kernel / roast_mean50_kernel make step 5 with a
 * lane per rotation and add b with integer atomics; the observed statistics come from the same kernels on a one-column z.
 * plaidhip_roast_multi shards the ROTATIONS in whole tiles of 64: device k of ndev takes tiles [T k / ndev, T (k + 1) / ndev)
 * of the T = ceil(nrot / 64).  Every device takes all of X and runs plaid.limma's two cheap passes itself, in the operations
 * and the order of the one-device call, so all hold the same effects, RSS and observed statistics; a z is made whole on one
 * device by one chain, and the int32 counts are added on the host: every sharding has the one-device bits.  The set sizes,
 * PropDown / PropUp and hyper come from the first device.  A device without a tile (ndev > T) does nothing.
 *   plaidhip_dev_roast_rotate: steps 3 and 4 on device pointers.  Rz: the raw residuals [n][ldz]; beta, rss: rows each; W:
 *     (n + 1) x ldw row-major with ldw a multiple of 16 that is >= nrot; chunk: rotations per launch (a multiple of 64; 0:
 *     all at once); Z: ceil(nrot / 64) x rows x 64 doubles, the padding of the last tile not written.
 *   plaidhip_dev_roast_stats: step 5 on device pointers from that Z.  Gp, Gi: the pattern of the members INSIDE the
 *     universe; stat: m x nrot x 4 (or NULL); obs: m x 4 and cnt: m x 4 int32, raised by b (both or neither).
 *   plaidhip_roast_rotations (host only): step 2 for one design and fit number `fit` (from 0): W, (n + 1) x nrot.
 *   plaidhip_roast_finish (host only): step 6 from cnt (int32, 4 x m x q x nfit), msize (m x nfit), ndown and nup (m x q x
 *     nfit: the members beyond -+sqrt(2)).
 * Not offered: per-set rotations (mroast's), gene or array weights, trend.var, robust, a dgCMatrix X, na = "fit" rows,
 * the exact z-score; romer is plaid.romer, below. */
#define PLAIDHIP_ROAST_MEAN50_MAX 16384        /* members: one rotation of z at an odd stride and 3 KiB beside it is 131 KiB of the CU's 160 */
#define PLAIDHIP_ROAST_MAX_ROTATIONS 1048576
#define PLAIDHIP_ROAST_Z_BYTES ((int64_t)256 << 20)
int plaidhip_roast(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, const double* design, int32_t p, int32_t nfit,
                   const int8_t* use, const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi, int32_t m,
                   int set_statistic, int zscore, int32_t nrot, uint64_t seed, int midp, const double* rotations, double* out,
                   double* hyper);
int plaidhip_roast_multi(const int* devices, int ndev, const double* X, int32_t g, int32_t n, const double* design, int32_t p,
                         int32_t nfit, const int8_t* use, const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi,
                         int32_t m, int set_statistic, int zscore, int32_t nrot, uint64_t seed, int midp,
                         const double* rotations, double* out, double* hyper);
int plaidhip_dev_roast_rotate(plaidhip_ctx* ctx, const double* Rz, int64_t ldz, int32_t rows, int32_t n, const double* beta,
                              const double* rss, const double* W, int64_t ldw, int32_t nrot, double d, double df0, double s02,
                              int zscore, int32_t chunk, double* Z);
int plaidhip_dev_roast_stats(plaidhip_ctx* ctx, const double* Z, int32_t rows, const int32_t* Gp, const int32_t* Gi, int32_t m,
                             int set_statistic, int32_t nrot, double* stat, const double* obs, int32_t* cnt);
int plaidhip_roast_rotations(const double* design, int32_t n, int32_t p, const int8_t* use, int32_t fit, int32_t nrot,
                             uint64_t seed, double* W);
int plaidhip_roast_finish(int32_t m, int32_t nfit, int32_t q, int32_t nrot, int set_statistic, int midp, const int32_t* cnt,
                          const double* msize, const double* ndown, const double* nup, double* out);

/* plaid.romer(X, design, G, contrasts): limma's rotation GSEA (romer: Majewski et al. 2010; Dorum et al. 2009) -- the
 * COMPETITIVE set test with a rotation null: GSEA on the ranks of the moderated t among all genes, whose null distribution
 * keeps the gene-gene correlation.  The form is limma's romer AS RECALLED, pinned here: the source is not in this tree, so the
 * tests hold the code to these words restated at 50 digits.  Operands, designs, use, K and the Gp / Gi
 * pattern as plaidhip_roast.  For fit f: d = n_f - p >= 1; contrast j has plaid.limma's logFC_gj, u = u_j (stdev.unscaled),
 * the gene's RSS_g, and the prior (df0, s0^2) of plaidhip_limma_finish.
 * 1. Universe: as plaidhip_roast, step 1; U is its size, and sets count their members inside it: m.  U = 0: every row is
 *    NaN but NGenes (0).  U <= PLAIDHIP_ROMER_MAX_GENES.
 * 2. Rotations: plaidhip_roast's step 2 exactly -- the same plaidhip_roast_rotations, the same counter tag -- shared by every
 *    set and contrast of a fit, as limma's romer shares them.  The caller's own W (rotations != NULL) is taken as it is.
 * 3. The observed statistic of a gene is plaid.limma's moderated t, bit for bit.
 * 4. The rotated statistic is plaidhip_roast's step 3 with beta' in place of beta and no z-score (ranks do not change under
 *    a monotone map, so roast's step 4 has no place here): B = beta' r0 rounded, then the fma chain over the residuals;
 *    s2r = (beta' beta' + RSS - B B) / d, and 0.0 unless that is > 0; post as in roast; t = B / sqrt(post).  roast.h's inline
 *    functions are the one copy of this arithmetic.
 * 5. Shrink: beta' = beta c_g with beta = logFC_gj / u.  shrink_resid = 0: c_g = 1.0 and beta' has beta's bits.  shrink_resid
 *    = 1 (limma's default): c_g = sqrt(u^2 / (u^2 + v0 ProbDE_g)), made on the host in fp64 (plaidhip_romer_shrink) per fit
 *    and contrast over the universe's moderated t (a NaN t counts as 0.0).  nu = df0 + d; for nu infinite or > 10^6 the
 *    normal limits are used: pnorm, qnorm, kernel = t^2 (1 - 1 / r) / 2.
 *      a. p_g = 2 P(T_nu > |t_g|).
 *      b. propTrueNull, method "lfdr": p sorted decreasing, i = U .. 1, q = min(U / i p, 1), pi0 = 2 sum i q / (U (U + 1)),
 *         pi = 1 - pi0.
 *      c. pi <= 0: every c_g = 1.0.  pi >= 1: ProbDE = 1 for every gene.
 *      d. tmixture.vector: ntarget = ceil(pi / 2 U), P = max(ntarget / U, pi); the ntarget largest |t| in decreasing order,
 *         r = 1 .. ntarget: p0 = 2 P(T_nu > |t|), ptarget = ((r - 0.5) / U - (1 - P) p0) / P; v0_r = u^2 ((|t| / q_r)^2 - 1)
 *         where ptarget > p0, with q_r the upper ptarget / 2 quantile of t_nu (a bisection on the t tail), else 0; each v0_r
 *         clamped to [0.01, 16] / s0^2; v0 their mean.
 *      e. r = (u^2 + v0) / u^2; kernel = (1 + nu) / 2 log((t^2 + nu) / (t^2 / r + nu)); lods = log(pi / (1 - pi)) - log(r) / 2
 *         + kernel; ProbDE = 1 / (1 + exp(-lods)), a NaN counts as 1.
 *    The squared length the rotation preserves is beta'^2 + RSS, the length of the shrunken effects themselves: B B cannot
 *    exceed it (Cauchy-Schwarz on the unit rotation), so it is the only choice that keeps s2r >= 0 under every rotation.
 *    Every entry also takes the caller's factors (shrink != NULL: g x q x nfit, a row's factor for contrast j of fit f at
 *    shrink[(f q + j) g + row]; rows outside the universe are not read), so the device path can be held with given factors.
 * 6. Keys.  x = t + 0.0 (no -0.0 reaches a ranker); a rotated t that is NaN (0 / 0, post = 0) is keyed as 0.0 and raises the
 *    hyper flag; -Inf < finite < +Inf.  set_statistic 0 "mean" (limma's default for romer) and 2 "mean50": key a = x, key
 *    c = |x|.  1 "floormean": key a = max(x, 0), key b = max(-x, 0) + 0.0, key c = max(|x|, 1).  Ranks are taken among the U
 *    genes of the universe, ascending, ties averaged, and held as 2 rank: an integer in [2, 2 U].  For statistics 0 and 2
 *    the "down" rank is 2 (U + 1) - 2 rank_a and is not ranked again.
 * 7. The set statistic: three sides (Up, Down, Mixed) as exact int64 sums of 2 rank over the m members -- no division, the
 *    sides are compared as integers, and being integers they do not depend on any order.
 *      mean:      Up = sum 2 r_a;   Down = 2 m (U + 1) - sum 2 r_a;   Mixed = sum 2 r_c
 *      floormean: Up = sum 2 r_a;   Down = sum 2 r_b;                  Mixed = sum 2 r_c
 *      mean50, h = floor(m / 2) + 1:  Up = the sum of the h largest 2 r_a;  Down = 2 h (U + 1) - the sum of the h smallest
 *                 2 r_a;  Mixed = the sum of the h largest 2 r_c.  mean50 holds a set's 2 r in LDS: a set with more than
 *                 PLAIDHIP_ROAST_MEAN50_MAX members in the universe has NaN p-values and raises the hyper flag.
 * 8. b = #{k : side_k >= side_obs} per side; p = (b + 1) / (nrot + 1).  FDR.*: Benjamini-Hochberg over the sets of each
 *    (fit, contrast).  m = 0: NaN but NGenes.
 * out: m x 7 x q x nfit doubles, column-major: NGenes, Up, Down, Mixed (limma's columns), FDR.Up, FDR.Down, FDR.Mixed;
 * contrast j of fit f at out + (f q + j) 7 m.  hyper: nfit x (8 + q) doubles: plaid.limma's four (df.residual, df.prior,
 * s2.prior, n_ok), U, nrot, 1.0 where a set was above the mean50 cap, 1.0 where a rotated or observed t was NaN, then pi of
 * every contrast (0.0 where not shrunk).
 * g == 0, nfit == 0, q == 0 or m == 0: PLAIDHIP_OK with nothing written.
 * Argument errors, all PLAIDHIP_EINVAL and all found on the host before any device is touched: those of plaidhip_roast in
 * their order up to the membership (named "romer:"); then set_statistic outside 0..2; nrot < 1; nrot >
 * PLAIDHIP_ROAST_MAX_ROTATIONS; then g > PLAIDHIP_ROMER_MAX_GENES (PLAIDHIP_EUNSUPPORTED).
 * On the device: roast_rotate_kernel (kernels_roast.hip, untouched) writes t as [tile of 64 rotations][g][64];
 * kernels_romer.hip: romer_key_kernel gathers the universe's rows of a tile by an index list, turns the tile through LDS and
 * writes the keys as columns [rotation][ldu]; the rank kernels of plaidhip_dev_colranks_dense_f64 rank every column (ties
 * average).  mean and floormean: the sums are the rank crossprod of plaidhip_dev_spmm_ranks_f64 on a collection prepared from
 * the pattern inside the universe (exact integer sums), and romer_count_kernel doubles them into the int64 sides and counts.
 * mean50: romer_mean50_kernel takes a wave per (set, rotation), selects over the 19 bits of 2 rank in LDS and adds b with
 * integer atomics.  The observed sides come from the same kernels on a one-column key matrix.  Chunks are whole tiles of 64 rotations; t, keys and ranks of a chunk together
 * stay inside PLAIDHIP_ROAST_Z_BYTES.
 * plaidhip_romer_multi shards the ROTATIONS in whole tiles of 64 exactly as plaidhip_roast_multi does; every device runs
 * the cheap fit and the host shrink itself from the same bits, and the int32 counts are added on the host: every sharding
 * has the one-device bits.
 *   plaidhip_dev_romer_keys: step 6 on device pointers.  Z: t as plaidhip_dev_roast_rotate writes it (zscore 1); uidx: the U
 *     rows of the universe; Ka, Kb (floormean only, else NULL), Kc: nrot x ldu doubles, ldu >= U, neither the tail of a column
 *     nor anything past the matrices written; flag: one uint32 set to 1 by a NaN (or NULL); chunk: rotations per launch (a
 *     multiple of 64; 0: all at once).
 *   plaidhip_dev_romer_sides: step 7 on device pointers from the AVERAGE RANKS of the key matrices, as
 *     plaidhip_dev_colranks_dense_f64 writes them (ties average, power 1): Ra, Rb (floormean only, else NULL), Rc, nrot x ldu
 *     doubles.  Gp, Gi: the pattern of the members by their PLACE in the universe (0 .. U - 1); stat: m x nrot x 3 int64 (or
 *     NULL), not written for a set without a member or above the mean50 cap; obs: m x 3 int64 and cnt: m x 3 int32, raised by
 *     b (both or neither); chunk as above.
 *   plaidhip_romer_shrink (host only): step 5 for one (fit, contrast): c (U) and *prop = pi from t (U), u, s0^2, nu.
 *   plaidhip_romer_finish (host only): step 8 from cnt (int32, 3 x m x q x nfit) and msize (m x nfit).
 * Not offered: array.weights, block / correlation, a dgCMatrix X, na = "fit" rows, gene weights, trend, robust. */
#define PLAIDHIP_ROMER_MAX_GENES 131072        /* 2 rank <= 2^18: 19 bits to select on */
int plaidhip_romer(plaidhip_ctx* ctx, const double* X, int32_t g, int32_t n, const double* design, int32_t p, int32_t nfit,
                   const int8_t* use, const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi, int32_t m,
                   int set_statistic, int32_t nrot, uint64_t seed, int shrink_resid, const double* shrink, const double* rotations,
                   double* out, double* hyper);
int plaidhip_romer_multi(const int* devices, int ndev, const double* X, int32_t g, int32_t n, const double* design, int32_t p,
                         int32_t nfit, const int8_t* use, const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi,
                         int32_t m, int set_statistic, int32_t nrot, uint64_t seed, int shrink_resid, const double* shrink,
                         const double* rotations, double* out, double* hyper);
int plaidhip_dev_romer_keys(plaidhip_ctx* ctx, const double* Z, int32_t rows, const int32_t* uidx, int32_t U, int64_t ldu,
                            int set_statistic, int32_t nrot, int32_t chunk, double* Ka, double* Kb, double* Kc, uint32_t* flag);
int plaidhip_dev_romer_sides(plaidhip_ctx* ctx, const double* Ra, const double* Rb, const double* Rc, int64_t ldu, int32_t U,
                             const int32_t* Gp, const int32_t* Gi, int32_t m, int set_statistic, int32_t nrot, int32_t chunk,
                             int64_t* stat, const int64_t* obs, int32_t* cnt);
int plaidhip_romer_shrink(int32_t U, const double* t, double u, double s02, double nu, double* c, double* prop);
int plaidhip_romer_finish(int32_t m, int32_t nfit, int32_t q, int32_t nrot, int set_statistic, const int32_t* cnt,
                          const double* msize, double* out);

/* ---- GMT text -> 0/1 membership matrix on the host (no device involved) --------------------------
 * Replaces read.gmt() R/gmt-utils.R:99-125 and gmt2mat() R/gmt-utils.R:19-66 (50.9 s for a 50k-set
 * collection in R, experiments/benchmark/benchmark-plaid.R:42).  Objects are owned by the library
 * until *_destroy; returned pointers stay valid until the next call on the same object.            */
typedef struct plaidhip_gmt plaidhip_gmt;         /* a named list of gene sets                        */
typedef struct plaidhip_gmtmat plaidhip_gmtmat;   /* genes x sets 0/1 dgCMatrix pattern + dimnames    */

/* read.gmt(gmt.file, add.source, nrows): '#' comments, tab fields name/source/genes, genes split on
 * ' ' or tab, "" / "NA" / repeats dropped.  nrows <= 0: all lines.                                 */
int plaidhip_gmt_read(const char* path, int add_source, int64_t nrows, plaidhip_gmt** out);
/* the same from memory.  raw != 0: exchange format for an in-memory list (one set per line,
 * name TAB source TAB gene TAB gene ...; nothing is filtered but empty tokens and repeats)         */
int plaidhip_gmt_parse(const char* text, int64_t nbytes, int raw, int add_source, int64_t nrows,
                       plaidhip_gmt** out);
int64_t plaidhip_gmt_nsets(const plaidhip_gmt* gmt);
const char* plaidhip_gmt_set_name(const plaidhip_gmt* gmt, int64_t j);
int64_t plaidhip_gmt_set_size(const plaidhip_gmt* gmt, int64_t j);
const char* plaidhip_gmt_set_gene(const plaidhip_gmt* gmt, int64_t j, int64_t k);
/* all sets as text, one line per set: name TAB gene TAB gene ... (bulk transfer to a host language) */
const char* plaidhip_gmt_text(plaidhip_gmt* gmt, int64_t* nbytes);
int plaidhip_gmt_destroy(plaidhip_gmt* gmt);

/* gmt2mat(gmt, max.genes, ntop, bg): sets by decreasing size, repeated names dropped, head(ntop);
 * rows = bg (nbg names) or, nbg == 0, the genes by decreasing count (ties in name order);
 * head(max.genes) (max_genes < 0: all); rows finally by decreasing number of sets (stable).        */
int plaidhip_gmt2mat(const plaidhip_gmt* gmt, int64_t max_genes, int64_t ntop, const char* const* bg,
                     int64_t nbg, plaidhip_gmtmat** out);
int plaidhip_gmtmat_dims(const plaidhip_gmtmat* mat, int64_t dims[3]);   /* genes, sets, memberships */
const int32_t* plaidhip_gmtmat_p(const plaidhip_gmtmat* mat);             /* @p, sets + 1              */
const int32_t* plaidhip_gmtmat_i(const plaidhip_gmtmat* mat);             /* @i, sorted rows per set   */
/* newline-joined dimnames: axis 0 = genes (rows), 1 = sets (columns)                                */
const char* plaidhip_gmtmat_names(plaidhip_gmtmat* mat, int axis, int64_t* nbytes);
int plaidhip_gmtmat_destroy(plaidhip_gmtmat* mat);

#ifdef __cplusplus
}
#endif
#endif /* PLAIDHIP_H */
