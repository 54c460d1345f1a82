// replaid.ssgsea.exact: the operands and the epilogue of the original single-sample GSEA statistic (gao.ssgsea with
// single = TRUE).  For one sample column with N genes, average ranks r (ties "average"), q = rank(x, ties = "last")
// (the position in order(r, decreasing = TRUE), counted from the bottom: q = N - pos + 1) and w = r^alpha, a set S
// with k members scores
//     ES = A / B - (T - C) / (N - k),   A = sum_S w q,  B = sum_S w,  C = sum_S q,  T = N (N + 1) / 2
// -- the walk's running sum, summed in closed form.  A, B and C are crossprods of the gene-set matrix with dense operand
// columns, which this file builds; the crossprods run on the existing SpMM kernels (multi.cpp: ssgsea_exact_worker).
//
// Operands with TWO rank passes (the rank kernels of colranks(), the only ranking code):
//   1. R = average ranks (power 1: half-integers, exact);
//   2. Q = min ranks of the tie-free column y_i = (2 R_i - 1) * 2^26 + (cnt - 1 - i): the tie groups keep their order
//      and a group's rows come last-first, so these are the "last" ranks (kernels_rank.hip: launch_last_ranks);
//   3. element-wise: w = R^alpha with the exponent routine the rank kernel of that column length applies (pow_quarters
//      when 4 alpha is an integer in 1..16 and the bucket / partitioned ranker takes the column, pow otherwise), P = w q.
// A dgCMatrix is ranked on its stored values only (both passes over nnz) and expanded into dense operand columns: the
// implicit zeros tie with the stored zeros, and inside that group q follows the row order.
// A sample column that holds a NaN is flagged; every set scores NaN in it.
#include <algorithm>

#include "common.h"
#include "device_sort.h"
#include "exact_common.h"
#include "rank_bucket.h"

namespace plaidhip {

namespace {

__device__ __forceinline__ double walk_pow(double r, double power, int pow_q4) {
  return power == 1.0 ? r : (pow_q4 > 0 ? pow_quarters(r, pow_q4) : PH_POW(r, power));
}

// dense columns: w = r^alpha and P = w q (need_w), the NaN flag of the column
__global__ void __launch_bounds__(256)
walk_finish_dense_kernel(RankCols t, const double* __restrict__ R, const double* __restrict__ Q, int need_w, double power,
                         int pow_q4, double* __restrict__ W, double* __restrict__ P, uint32_t* __restrict__ colnan) {
  for_each_rank_item(t, [&](const RankItem& it) {
    const double r = R[it.r];
    if (r != r) colnan[it.c] = 1u;
    if (need_w) {
      const double w = r == r ? walk_pow(r, power, pow_q4) : r;
      W[it.r] = w;
      P[it.r] = w * Q[it.r];
    }
  });
}

// CSC columns -> dense operand columns, one wavefront per column walking 64 rows at a time.  A row is a stored non-zero
// (its ranks among the stored values, moved up by the z implicit zeros when it is positive) or a zero -- stored or
// implicit, the zeros form one tie group [lb0 + 1, lb0 + e0 + z] in which q counts down in row order.  Rows must be
// strictly increasing inside a column (a dgCMatrix's are); anything else gives wrong operands, never an access outside
// the buffers.
__global__ void __launch_bounds__(256)
walk_expand_csc_kernel(const int32_t* __restrict__ Xp, const int32_t* __restrict__ Xi, const double* __restrict__ Xx,
                       const double* __restrict__ Rx, const double* __restrict__ Qx, int32_t g, int32_t n, int need_w, double power, int pow_q4, double* __restrict__ Q,
                       double* __restrict__ W, double* __restrict__ P, int64_t ld, uint32_t* __restrict__ colnan) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (int c = blockIdx.x * 4 + wave; c < n; c += gridDim.x * 4) {   // (c is uniform in the wavefront)
    const int32_t q0 = Xp[c], q1 = Xp[c + 1];
    const int64_t z = (int64_t)g - (q1 - q0);
    uint32_t neg = 0, e0 = 0, nn = 0;
    for (int32_t q = q0 + lane; q < q1; q += 64) {
      const double v = Xx[q];
      neg += (v < 0.0) ? 1u : 0u;
      e0 += (v == 0.0) ? 1u : 0u;
      nn += (v != v) ? 1u : 0u;
    }
    neg = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_u32(neg), 63);
    e0 = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_u32(e0), 63);
    nn = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_u32(nn), 63);
    if (nn != 0u && lane == 0) colnan[c] = 1u;
    const int64_t top0 = (int64_t)neg + e0 + z;                       // ub of the zero group
    const double r0 = 0.5 * (double)((int64_t)neg + 1 + top0);        // its average rank
    const double w0 = need_w ? walk_pow(r0, power, pow_q4) : 0.0;
    double* qc = Q + (int64_t)c * ld;
    double* wc = need_w ? W + (int64_t)c * ld : nullptr;
    double* pc = need_w ? P + (int64_t)c * ld : nullptr;
    int64_t nzb = 0;   // stored non-zeros in the rows already written
    int32_t qp = q0;   // next stored value
    for (int32_t row0 = 0; row0 < g; row0 += 64) {
      // the stored rows of this chunk as a 64-bit mask (OR over the wavefront): rows are increasing, so the stored value
      // of row0 + lane is entry qp + (stored rows below it)
      const int32_t j = qp + lane;
      const int32_t xi = j < q1 ? Xi[j] : -1;
      const bool inch = xi >= row0 && xi < row0 + 64;                 // (the earlier rows are consumed)
      unsigned long long rows = inch ? (1ull << (xi - row0)) : 0ull;
      for (int o = 32; o >= 1; o >>= 1) rows |= __shfl_xor(rows, o);
      const unsigned long long below = (1ull << lane) - 1ull;
      const int32_t idx = ((rows >> lane) & 1ull) ? qp + (int32_t)__popcll(rows & below) : -1;
      const int32_t row = row0 + lane;
      const double v = idx >= 0 ? Xx[idx] : 0.0;
      const bool nzs = idx >= 0 && v != 0.0;                          // (a NaN is not a zero)
      const uint64_t mnz = __ballot(nzs);
      const int64_t before = nzb + __popcll(mnz & below);
      double qv, wv = w0;
      if (!nzs) {
        qv = (double)(top0 - ((int64_t)row - before));
      } else if (v != v) {
        qv = nan;
        wv = nan;
      } else {
        const double off = v > 0.0 ? (double)z : 0.0;   // a positive value ranks above the z implicit zeros
        qv = Qx[idx] + off;
        if (need_w) wv = walk_pow(Rx[idx] + off, power, pow_q4);
      }
      if (row < g) {
        qc[row] = qv;
        if (need_w) { wc[row] = wv; pc[row] = wv * qv; }
      }
      nzb += __popcll(mnz);
      qp += __popcll(rows);
    }
  }
}

// the pinned epilogue (include/plaidhip.h): d1 = A / B, d2 = (T - C) / (N - k), es = d1 - d2, [es / N]; it holds no
// product, so no contraction can fuse anything.  A == nullptr: A = C and B = k (alpha = 0).  S holds C on entry.
// Block partials {min, max, any NaN} of the scores for norm.
__global__ void __launch_bounds__(256)
walk_epilogue_kernel(const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ S, int64_t lds,
                     int32_t m, int32_t n, const int32_t* __restrict__ kset, int64_t N, int scale,
                     const uint32_t* __restrict__ colnan, double* __restrict__ part) {
  const double T = (double)(N * (N + 1) / 2);
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double mn = INFINITY, mx = -INFINITY, nf = 0.0;
  for_each_score(m, n, lds, [&](int64_t c, int64_t j, int64_t at) {
    const int32_t k = kset[j];
    const double cv = S[at];
    const double av = A != nullptr ? A[at] : cv;
    const double bv = B != nullptr ? B[at] : (double)k;
    const double d1 = av / bv;
    const double d2 = (T - cv) / (double)(N - k);
    double es = d1 - d2;
    if (scale) es = es / (double)N;
    if (colnan[c]) es = nan;
    S[at] = es;
    score_range_take(es, mn, mx, nf);
  });
  score_range_block(mn, mx, nf, part);
}

// block partials {min, max, any NaN} of m x n scores (launch_score_range: the scores of single = FALSE, which no epilogue
// kernel passes over)
__global__ void __launch_bounds__(256)
gsea_ks_range_kernel(const double* __restrict__ S, int64_t lds, int32_t m, int32_t n, double* __restrict__ part) {
  double mn = INFINITY, mx = -INFINITY, nf = 0.0;
  for_each_score(m, n, lds, [&](int64_t, int64_t, int64_t at) { score_range_take(S[at], mn, mx, nf); });
  score_range_block(mn, mx, nf, part);
}

// {min, max, any NaN} over the block partials (min / max select: any order gives the same values)
__global__ void __launch_bounds__(64)
gsea_ks_range_final_kernel(const double* __restrict__ part, int nblocks, double* __restrict__ out) {
  double mn = INFINITY, mx = -INFINITY, nf = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 64) {
    mn = part[3 * b] < mn ? part[3 * b] : mn;
    mx = part[3 * b + 1] > mx ? part[3 * b + 1] : mx;
    nf = part[3 * b + 2] > nf ? part[3 * b + 2] : nf;
  }
  for (int o = 32; o >= 1; o >>= 1) {
    const double a = __shfl_xor(mn, o), b = __shfl_xor(mx, o), f = __shfl_xor(nf, o);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
    nf = f > nf ? f : nf;
  }
  if (threadIdx.x == 0) { out[0] = mn; out[1] = mx; out[2] = nf; }
}

__global__ void __launch_bounds__(256)
walk_norm_kernel(double* __restrict__ S, int64_t lds, int32_t m, int32_t n, double range) {
  for_each_score(m, n, lds, [&](int64_t, int64_t, int64_t at) { S[at] = S[at] / range; });
}

// the exponent routine of colranks(ties = "average", power = alpha) for columns of g keys
int walk_pow_q4(plaidhip_ctx* ctx, int32_t g, double power) {
  const double q4 = power * 4.0;
  const int pq = (power != 1.0 && q4 >= 1.0 && q4 <= 16.0 && q4 == (double)(int)q4) ? (int)q4 : 0;
  return colranks_uses_power_quarters(ctx, g) ? pq : 0;
}

}  // namespace

int score_part_blocks(plaidhip_ctx* ctx, int64_t count) {
  const int64_t b = (count + 255) / 256, cap = (int64_t)ctx->num_cu * 4;
  return (int)std::max<int64_t>(1, std::min(b, cap));
}

int launch_score_range(plaidhip_ctx* ctx, const double* S, int64_t lds, int32_t m, int32_t n, double* part, double* range_out) {
  if ((int64_t)m * n == 0) return PLAIDHIP_OK;
  const int blocks = score_part_blocks(ctx, (int64_t)m * n);
  hipLaunchKernelGGL(gsea_ks_range_kernel, dim3(blocks), dim3(256), 0, ctx->stream, S, lds, m, n, part);
  hipLaunchKernelGGL(gsea_ks_range_final_kernel, dim3(1), dim3(64), 0, ctx->stream, part, blocks, range_out);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_ssgsea_exact_operands(plaidhip_ctx* ctx, const double* X, int64_t ldx, const int32_t* Xp, const int32_t* Xi,
                                 int32_t g, int32_t n, int32_t max_col_nnz, int64_t nnz, double alpha, double* Q, double* W,
                                 double* P, int64_t ldq, double* scratch, uint32_t* colnan) {
  if (n == 0) return PLAIDHIP_OK;
  PH_HIP(hipMemsetAsync(colnan, 0, (size_t)n * 4, ctx->stream));
  if (g == 0) return PLAIDHIP_OK;
  const int need_w = alpha != 0.0 ? 1 : 0;
  const int pow_q4 = walk_pow_q4(ctx, g, alpha);
  int rc;
  if (Xp == nullptr) {
    double* R = scratch;
    double* Y = scratch + ldq * (int64_t)n;
    const RankCols t = dense_cols(g, n, ldq);
    rc = launch_colranks_dense_f64(ctx, X, ldx, g, n, PLAIDHIP_TIES_AVERAGE, 0, 1.0, R, ldq, nullptr);      // pass 1
    if (rc != PLAIDHIP_OK) return rc;
    rc = launch_last_ranks(ctx, t, R, Y, Q);                                                                 // pass 2
    if (rc != PLAIDHIP_OK) return rc;
    hipLaunchKernelGGL(walk_finish_dense_kernel, rank_cols_grid(t), dim3(256), 0, ctx->stream, t, R, Q, need_w, alpha, pow_q4, W, P,
                       colnan);
    PH_HIP(hipGetLastError());
    return PLAIDHIP_OK;
  }
  // dgCMatrix: the stored values' average and last ranks (nnz each), then the dense expansion
  double* Rx = scratch;
  double* Yx = scratch + nnz;
  double* Qx = scratch + 2 * nnz;
  if (max_col_nnz > 0) {
    rc = launch_colranks_csc_f64(ctx, Xp, X, n, max_col_nnz, PLAIDHIP_TIES_AVERAGE, 0, 1.0, Rx, nullptr);      // pass 1
    if (rc != PLAIDHIP_OK) return rc;
    rc = launch_last_ranks(ctx, csc_cols(Xp, max_col_nnz, n), Rx, Yx, Qx);                                     // pass 2
    if (rc != PLAIDHIP_OK) return rc;
  }
  const int cap = ctx->num_cu * 16;
  const int blocks = (n + 3) / 4;
  hipLaunchKernelGGL(walk_expand_csc_kernel, dim3(blocks < cap ? blocks : cap), dim3(256), 0, ctx->stream, Xp, Xi, X, Rx, Qx, g, n,
                     need_w, alpha, pow_q4, Q, W, P, ldq, colnan);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_ssgsea_exact_epilogue(plaidhip_ctx* ctx, const double* A, const double* B, double* S, int64_t lds, int32_t m,
                                 int32_t n, const int32_t* kset, int64_t N, int scale, const uint32_t* colnan, double* part,
                                 double* range_out) {
  if ((int64_t)m * n == 0) return PLAIDHIP_OK;
  const int blocks = score_part_blocks(ctx, (int64_t)m * n);
  hipLaunchKernelGGL(walk_epilogue_kernel, dim3(blocks), dim3(256), 0, ctx->stream, A, B, S, lds, m, n, kset, N, scale, colnan,
                     part);
  hipLaunchKernelGGL(gsea_ks_range_final_kernel, dim3(1), dim3(64), 0, ctx->stream, part, blocks, range_out);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_ssgsea_exact_norm(plaidhip_ctx* ctx, double* S, int64_t lds, int32_t m, int32_t n, double range) {
  if ((int64_t)m * n == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(walk_norm_kernel, dim3(score_part_blocks(ctx, (int64_t)m * n)), dim3(256), 0, ctx->stream, S, lds, m, n, range);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
