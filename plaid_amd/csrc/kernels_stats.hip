// Row-wise two-group moments for plaid.test() (R/plaid.R:392-474): the statistics are reduced
// on the device so that neither X (genes x samples) nor the score matrix (sets x samples) has
// to visit the host -- only O(rows) numbers do.
//
//   rowMeans(A[, y == 1]) , rowMeans(A[, y == 0])                       (R/plaid.R:407-408, 431)
//   per-row group variances for the Welch tests Rfast::ttests(t(gsetX), ina = y + 1)   (:429)
//
// A is column-major (rows contiguous), so a thread owns a row and a workgroup walks a block of
// columns: every load is coalesced.  Columns are cut into blocks of kRowColBlock (row_pair.h); a block writes its
// partial sums to [block][stat][row] and a second kernel adds the blocks in a fixed order
// (deterministic, no atomics).  Variances are two-pass (sum of squared deviations from the group
// mean), which is at least as accurate as the sum-of-squares formula of the reference.
#include "common.h"
#include "row_pair.h"

namespace plaidhip {

// pass 1: sums per group.  part: [nblk][2][rows]
__global__ void __launch_bounds__(256)
row_group_sums_kernel(const double* __restrict__ A, int64_t ld, int32_t rows, int32_t n,
                      const int32_t* __restrict__ y, double* __restrict__ part) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  const int c0 = blockIdx.y * kRowColBlock;
  const int c1 = c0 + kRowColBlock < n ? c0 + kRowColBlock : n;
  double s0 = 0.0, s1 = 0.0;
  if (r < rows) {
    for (int c = c0; c < c1; ++c) {
      const int lab = y[c];                       // wave-uniform
      const double v = A[(int64_t)c * ld + r];
      s0 += lab == 0 ? v : 0.0;
      s1 += lab == 1 ? v : 0.0;
    }
    double* p = part + (int64_t)blockIdx.y * 2 * rows;
    p[r] = s0;
    p[rows + r] = s1;
  }
}

// pass 2: sums of squared deviations from the group means.  mean: [2][rows]; part: [nblk][2][rows]
__global__ void __launch_bounds__(256)
row_group_ssd_kernel(const double* __restrict__ A, int64_t ld, int32_t rows, int32_t n,
                     const int32_t* __restrict__ y, const double* __restrict__ mean,
                     double* __restrict__ part) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  const int c0 = blockIdx.y * kRowColBlock;
  const int c1 = c0 + kRowColBlock < n ? c0 + kRowColBlock : n;
  if (r < rows) {
    const double m0 = mean[r], m1 = mean[rows + r];
    double q0 = 0.0, q1 = 0.0;
    for (int c = c0; c < c1; ++c) {
      const int lab = y[c];
      const double v = A[(int64_t)c * ld + r];
      const double d0 = v - m0, d1 = v - m1;
      q0 += lab == 0 ? d0 * d0 : 0.0;
      q1 += lab == 1 ? d1 * d1 : 0.0;
    }
    double* p = part + (int64_t)blockIdx.y * 2 * rows;
    p[r] = q0;
    p[rows + r] = q1;
  }
}

// out[s][r] = scale[s] * sum over blocks of part[b][s][r]   (blocks added in order)
__global__ void __launch_bounds__(256)
reduce_blocks_kernel(const double* __restrict__ part, int32_t rows, int32_t nblk, double scale0,
                     double scale1, double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;   // over 2 * rows
  if (i >= 2 * rows) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += part[(int64_t)b * 2 * rows + i];
  out[i] = s * (i < rows ? scale0 : scale1);
}

// out[r] = seed[r] (0 without a seed) + part[0][0][r] + part[1][0][r] + ..., the blocks added in order: group 0 of
// reduce_blocks_kernel, continued from where the previous column shard stopped.  A sample-sharded caller whose shards
// start on block boundaries (multiples of kRowColBlock columns) and that chains them in column order adds exactly what
// reduce_blocks_kernel adds over all columns, in the same order; the scale step stays with the caller.
__global__ void __launch_bounds__(256)
reduce_blocks_seeded_kernel(const double* __restrict__ part, int32_t rows, int32_t nblk, const double* __restrict__ seed,
                            double* __restrict__ out) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  double s = seed != nullptr ? seed[r] : 0.0;
  for (int b = 0; b < nblk; ++b) s += part[(int64_t)b * 2 * rows + r];
  out[r] = s;
}

// fc = m1 - m0 and fc^2 as the two columns of a rows x 2 matrix with leading dimension ld2
__global__ void __launch_bounds__(256)
fold_change_kernel(const double* __restrict__ mean, int32_t rows, int64_t ld2, double* __restrict__ F) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const double fc = mean[rows + r] - mean[r];
  F[r] = fc;
  F[ld2 + r] = fc * fc;
}

// replaid.gsva row transform, R/plaid.R:343: z = (x - rowMeans(X)) / (1e-8 + rowSds(X)), in place, over the `ncols`
// columns of A; n_sd: the number of samples the moments were taken over (ncols, or all columns of a sharded X)
__device__ __forceinline__ void row_ztransform_body(double* __restrict__ A, int64_t ld, int32_t rows, int32_t ncols,
                                                    int32_t n_sd, const double* __restrict__ mean,
                                                    const double* __restrict__ ssd) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  const int c0 = blockIdx.y * kRowColBlock;
  const int c1 = c0 + kRowColBlock < ncols ? c0 + kRowColBlock : ncols;
  if (r >= rows) return;
  const double mu = mean[r];
  const double den = 1e-8 + sqrt(ssd[r] / (double)(n_sd - 1));   // sd with n - 1 (NaN for a single sample, as in R)
  for (int c = c0; c < c1; ++c) {
    double* p = &A[(int64_t)c * ld + r];
    *p = (*p - mu) / den;   // a true division, as the reference does: ties between genes stay ties
  }
}

// mean, ssd: the group-0 means and sums of squared deviations of the rows (all samples in group 0), taken over the n_total
// columns of X, of which A holds a shard: the sd divides by n_total - 1
__global__ void __launch_bounds__(256)
row_ztransform_shard_kernel(double* __restrict__ A, int64_t ld, int32_t rows, int32_t ncols, int32_t n_total,
                            const double* __restrict__ mean, const double* __restrict__ ssd) {
  row_ztransform_body(A, ld, rows, ncols, n_total, mean, ssd);
}

int launch_row_ztransform_shard(plaidhip_ctx* ctx, double* A, int64_t ld, int32_t rows, int32_t ncols, int32_t n_total,
                                const double* d_mean, const double* d_ssd) {
  if (rows == 0 || ncols == 0) return PLAIDHIP_OK;
  const int nblk = (ncols + kRowColBlock - 1) / kRowColBlock;
  hipLaunchKernelGGL(row_ztransform_shard_kernel, dim3((rows + 255) / 256, nblk), dim3(256), 0, ctx->stream, A, ld, rows,
                     ncols, n_total, d_mean, d_ssd);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// B (cols x rows, ldb) = transpose of A (rows x cols, lda), both column-major; 32 x 32 tiles through LDS
// (+1 padding), coalesced on both sides.  Used by the ECDF row transform of replaid.gsva, which needs
// per-GENE ranks across samples (R/plaid.R:346): genes become columns, the column rank kernel does the rest.
__global__ void __launch_bounds__(256)
transpose_f64_kernel(const double* __restrict__ A, int64_t lda, int32_t rows, int32_t cols,
                     double* __restrict__ B, int64_t ldb) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  const int r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  for (int j = ty; j < 32; j += 8) {
    const int r = r0 + tx, c = c0 + j;
    if (r < rows && c < cols) tile[j][tx] = A[(int64_t)c * lda + r];
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int c = c0 + tx, r = r0 + j;
    if (r < rows && c < cols) B[(int64_t)r * ldb + c] = tile[tx][j];
  }
}

int launch_transpose_f64(plaidhip_ctx* ctx, const double* A, int64_t lda, int32_t rows, int32_t cols, double* B,
                         int64_t ldb) {
  if (rows == 0 || cols == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(transpose_f64_kernel, dim3((rows + 31) / 32, (cols + 31) / 32), dim3(256), 0, ctx->stream, A, lda,
                     rows, cols, B, ldb);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// Group means (and optionally sums of squared deviations) of every row of A.
// d_mean: [2][rows] (group 0, group 1); d_ssd: [2][rows] or null.  n0 / n1: group sizes.
// ws: scratch of at least 2 * rows * ceil(n / kRowColBlock) doubles.
int launch_row_group_moments(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n,
                             const int32_t* d_y, int64_t n0, int64_t n1, double* d_mean, double* d_ssd,
                             double* ws) {
  if (rows == 0) return PLAIDHIP_OK;
  const int nblk = (n + kRowColBlock - 1) / kRowColBlock;
  const dim3 grid((rows + 255) / 256, nblk > 0 ? nblk : 1);
  const int red_blocks = (2 * rows + 255) / 256;
  if (n > 0) hipLaunchKernelGGL(row_group_sums_kernel, grid, dim3(256), 0, ctx->stream, A, ld, rows, n, d_y, ws);
  hipLaunchKernelGGL(reduce_blocks_kernel, dim3(red_blocks), dim3(256), 0, ctx->stream, ws, rows, n > 0 ? nblk : 0,
                     n0 > 0 ? 1.0 / (double)n0 : __builtin_nan(""), n1 > 0 ? 1.0 / (double)n1 : __builtin_nan(""), d_mean);
  if (d_ssd != nullptr) {
    if (n > 0) hipLaunchKernelGGL(row_group_ssd_kernel, grid, dim3(256), 0, ctx->stream, A, ld, rows, n, d_y, d_mean, ws);
    hipLaunchKernelGGL(reduce_blocks_kernel, dim3(red_blocks), dim3(256), 0, ctx->stream, ws, rows, n > 0 ? nblk : 0,
                       1.0, 1.0, d_ssd);
  }
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// pass 2 alone: sums of squared deviations from GIVEN group means (a sample-sharded caller passes the means of all shards)
int launch_row_group_ssd(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const int32_t* d_y,
                         const double* d_mean, double* d_ssd, double* ws) {
  if (rows == 0) return PLAIDHIP_OK;
  const int nblk = (n + kRowColBlock - 1) / kRowColBlock;
  const dim3 grid((rows + 255) / 256, nblk > 0 ? nblk : 1);
  const int red_blocks = (2 * rows + 255) / 256;
  if (n > 0) hipLaunchKernelGGL(row_group_ssd_kernel, grid, dim3(256), 0, ctx->stream, A, ld, rows, n, d_y, d_mean, ws);
  hipLaunchKernelGGL(reduce_blocks_kernel, dim3(red_blocks), dim3(256), 0, ctx->stream, ws, rows, n > 0 ? nblk : 0, 1.0, 1.0,
                     d_ssd);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// the per-block partials of launch_row_group_moments over one column shard (sums; or, with d_mean, sums of squared
// deviations from it), left in ws ([nblk][2][rows], nblk = ceil(n / kRowColBlock))
int launch_row_group_partials(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const int32_t* d_y,
                              const double* d_mean, double* ws) {
  if (rows == 0 || n == 0) return PLAIDHIP_OK;
  const int nblk = (n + kRowColBlock - 1) / kRowColBlock;
  const dim3 grid((rows + 255) / 256, nblk);
  if (d_mean == nullptr)
    hipLaunchKernelGGL(row_group_sums_kernel, grid, dim3(256), 0, ctx->stream, A, ld, rows, n, d_y, ws);
  else
    hipLaunchKernelGGL(row_group_ssd_kernel, grid, dim3(256), 0, ctx->stream, A, ld, rows, n, d_y, d_mean, ws);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// d_out[r] = d_seed[r] (0 when null) + group 0 of the partials in ws, blocks in order (reduce_blocks_seeded_kernel)
int launch_reduce_blocks_seeded(plaidhip_ctx* ctx, const double* ws, int32_t rows, int32_t n, const double* d_seed,
                                double* d_out) {
  if (rows == 0) return PLAIDHIP_OK;
  const int nblk = (n + kRowColBlock - 1) / kRowColBlock;
  hipLaunchKernelGGL(reduce_blocks_seeded_kernel, dim3((rows + 255) / 256), dim3(256), 0, ctx->stream, ws, rows, nblk, d_seed,
                     d_out);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_fold_change(plaidhip_ctx* ctx, const double* d_mean, int32_t rows, int64_t ld2, double* d_F) {
  if (rows == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(fold_change_kernel, dim3((rows + 255) / 256), dim3(256), 0, ctx->stream, d_mean, rows, ld2, d_F);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// The block partials of row_group_sums_kernel (mean == nullptr) or of row_group_ssd_kernel (mean: [2][rows]) over the
// score shard of a sample-sharded plaid.test (multi.cpp), with normalize_medians' last step applied on load:
// v = (S[r, c] - med[c]) + add, shift_columns_kernel's expression and operand order (med == nullptr: v = S[r, c]).  Same
// column blocks, the same per-row additions in ascending column order and the same [nblk][2][rows] output as the two
// kernels above, so the seeded chain adds what the one-device entry adds after its in-place shift -- and the shifted S
// is never written: two streaming reads of S replace the shift's read + write and the two passes after it.
// A thread owns two adjacent rows: the walk of row_pair.h (kUn = 8).
template <bool kSsd, bool kWide>
__global__ void __launch_bounds__(256)
row_group_shifted_partials_kernel(const double* __restrict__ S, int64_t ld, int32_t rows, int32_t n,
                                  const int32_t* __restrict__ y, const double* __restrict__ med, double add,
                                  const double* __restrict__ mean, double* __restrict__ part) {
  const RowPair g = row_pair_block(rows, n);
  const int r = g.r;
  if (r >= rows) return;
  const bool two = g.two;
  const bool shift = med != nullptr;
  double m0a = 0.0, m1a = 0.0, m0b = 0.0, m1b = 0.0;
  if (kSsd) {
    m0a = mean[r];
    m1a = mean[rows + r];
    if (two) { m0b = mean[r + 1]; m1b = mean[rows + r + 1]; }
  }
  double s0a = 0.0, s1a = 0.0, s0b = 0.0, s1b = 0.0;
  auto accumulate = [&](int c, double xa, double xb) {
    const int lab = y[c];   // wave-uniform
    double va = xa, vb = xb;
    if (shift) {
      const double md = med[c];
      va = (xa - md) + add;
      vb = (xb - md) + add;
    }
    if (kSsd) {
      const double d0a = va - m0a, d1a = va - m1a, d0b = vb - m0b, d1b = vb - m1b;
      s0a += lab == 0 ? d0a * d0a : 0.0;
      s1a += lab == 1 ? d1a * d1a : 0.0;
      s0b += lab == 0 ? d0b * d0b : 0.0;
      s1b += lab == 1 ? d1b * d1b : 0.0;
    } else {
      s0a += lab == 0 ? va : 0.0;
      s1a += lab == 1 ? va : 0.0;
      s0b += lab == 0 ? vb : 0.0;
      s1b += lab == 1 ? vb : 0.0;
    }
  };
  row_pair_walk<kWide, 8>(S, ld, g, accumulate);
  double* p = part + (int64_t)blockIdx.y * 2 * rows;
  p[r] = s0a;
  p[rows + r] = s1a;
  if (two) {
    p[r + 1] = s0b;
    p[rows + r + 1] = s1b;
  }
}

int launch_row_group_shifted_partials(plaidhip_ctx* ctx, const double* S, int64_t ld, int32_t rows, int32_t n,
                                      const int32_t* d_y, const double* d_med, double add, const double* d_mean,
                                      double* ws) {
  if (rows == 0 || n == 0) return PLAIDHIP_OK;
  const int nblk = (n + kRowColBlock - 1) / kRowColBlock;
  const dim3 grid((rows + 511) / 512, nblk);
  dispatch_flag(d_mean != nullptr, [&](auto ssd) {
    dispatch_flag(row_pair_wide(rows, {ld}, {S}), [&](auto wide) {
      hipLaunchKernelGGL((row_group_shifted_partials_kernel<decltype(ssd)::value, decltype(wide)::value>), grid, dim3(256), 0,
                         ctx->stream, S, ld, rows, n, d_y, d_med, add, d_mean, ws);
    });
  });
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int64_t row_group_ws_doubles(int32_t rows, int32_t n) {
  const int64_t nblk = (n + kRowColBlock - 1) / kRowColBlock;
  return 2 * (int64_t)rows * (nblk > 0 ? nblk : 1);
}

}  // namespace plaidhip
