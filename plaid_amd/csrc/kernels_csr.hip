// Row view of a CSC matrix on the device, and the row-wise statistics replaid.gsva (R/plaid.R:338-363) and plaid.test
// (:392-474) take from it, so that a dgCMatrix is scored without a dense X on the host or on the PCIe link.
//
//   launch_csc_to_csr            stable transpose: Rp / Rj / Rx (+ perm, the CSC position of each CSR entry).  Within
//                                every row the entries are in ascending column order whatever the scheduling: the row
//                                reductions below sum in that order, so their results are run-to-run bit-identical and
//                                two genes with identical rows get identical statistics.
//   launch_csr_row_group_moments per-row group means / sums of squared deviations, implicit zeros included
//   launch_csr_row_ecdf          #{x <= x_i} per stored value and per row's implicit zero (rowtf = "ecdf")
//   launch_csc_expand            the dense column-major transformed matrix, row defaults + stored entries
//
// Integer atomics only (counts, cursors): no floating-point atomics anywhere, the sums are fixed-order.
#include <algorithm>

#include "common.h"

namespace plaidhip {

namespace {

constexpr int kCsrThreads = 256;
constexpr int kLongRow = 4096;                     // rows longer than this: a workgroup per row instead of a wavefront
constexpr size_t kCountBytes = (size_t)256 << 20;  // cap on the [column block][row] count table of the transpose

// butterfly sums: every lane ends with the same value (a + b == b + a in IEEE), fixed order for given lane inputs
__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over the W threads that share a row: W = 64 one wavefront, W = 256 the workgroup (waves added in order).
// W = 256 must be reached by every thread of the workgroup.
template <int W>
__device__ __forceinline__ double group_sum_f64(double v, double* sh) {
  v = wave_sum_f64(v);
  if (W == 64) return v;
  const int tid = threadIdx.x;
  __syncthreads();
  if ((tid & 63) == 0) sh[tid >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}
template <int W>
__device__ __forceinline__ int group_sum_i32(int v, int* sh) {
  v = wave_sum_i32(v);
  if (W == 64) return v;
  const int tid = threadIdx.x;
  __syncthreads();
  if ((tid & 63) == 0) sh[tid >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

// ---- transpose -------------------------------------------------------------------------------------------------------
// Columns are cut into nblk blocks of cpb consecutive columns (their entries are one contiguous range of the CSC).
// cnt[b][r]: entries of row r in block b; then, per row, the exclusive prefix over b; the fill walks its block's columns
// in order, one barrier per column, and takes slots from its own cursors -- so a row's entries land in column order.

__global__ void __launch_bounds__(kCsrThreads)
csc_block_count_kernel(const int32_t* __restrict__ Xp, const int32_t* __restrict__ Xi, int32_t n, int32_t g, int32_t cpb,
                       int32_t* __restrict__ cnt) {
  const int b = blockIdx.x;
  const int c0 = b * cpb, c1 = c0 + cpb < n ? c0 + cpb : n;
  const int q0 = Xp[c0], q1 = Xp[c1];
  int32_t* cb = cnt + (int64_t)b * g;
  for (int q = q0 + (int)threadIdx.x; q < q1; q += kCsrThreads) atomicAdd(&cb[Xi[q]], 1);
}

// per row: cnt[b][r] <- entries of row r in blocks before b; rowlen[r] <- the row's total
__global__ void __launch_bounds__(kCsrThreads)
csc_block_offsets_kernel(int32_t* __restrict__ cnt, int32_t nblk, int32_t g, int32_t* __restrict__ rowlen) {
  const int r = blockIdx.x * kCsrThreads + threadIdx.x;
  if (r >= g) return;
  int run = 0;
  for (int b = 0; b < nblk; ++b) {
    int32_t* p = cnt + (int64_t)b * g + r;
    const int t = *p;
    *p = run;
    run += t;
  }
  rowlen[r] = run;
}

// one workgroup of 1,024 threads: Rp[0..g) row lengths -> exclusive prefix in place, Rp[g] = total, *maxlen = longest row
__global__ void __launch_bounds__(1024)
row_pointer_scan_kernel(int32_t* __restrict__ Rp, int32_t g, int32_t* __restrict__ maxlen) {
  __shared__ int s_sum[1024];
  __shared__ int s_max[1024];
  const int t = threadIdx.x;
  const int chunk = (g + 1023) / 1024;
  const int r0 = t * chunk < g ? t * chunk : g;
  const int r1 = r0 + chunk < g ? r0 + chunk : g;
  int sum = 0, mx = 0;
  for (int r = r0; r < r1; ++r) {
    const int v = Rp[r];
    sum += v;
    mx = v > mx ? v : mx;
  }
  s_sum[t] = sum;
  s_max[t] = mx;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {   // Hillis-Steele inclusive scan of the chunk sums, max alongside
    const int a = t >= o ? s_sum[t - o] : 0;
    const int b = t >= o ? s_max[t - o] : 0;
    __syncthreads();
    s_sum[t] += a;
    s_max[t] = b > s_max[t] ? b : s_max[t];
    __syncthreads();
  }
  int run = s_sum[t] - sum;
  for (int r = r0; r < r1; ++r) {
    const int v = Rp[r];
    Rp[r] = run;
    run += v;
  }
  if (t == 1023) {
    Rp[g] = s_sum[1023];
    *maxlen = s_max[1023];
  }
}

__global__ void __launch_bounds__(kCsrThreads)
csc_block_fill_kernel(const int32_t* __restrict__ Xp, const int32_t* __restrict__ Xi, const double* __restrict__ Xx,
                      int32_t n, int32_t g, int32_t cpb, int32_t* __restrict__ cnt, const int32_t* __restrict__ Rp,
                      int32_t* __restrict__ Rj, double* __restrict__ Rx, int32_t* __restrict__ perm) {
  const int b = blockIdx.x;
  const int c0 = b * cpb, c1 = c0 + cpb < n ? c0 + cpb : n;
  int32_t* cb = cnt + (int64_t)b * g;
  for (int c = c0; c < c1; ++c) {
    const int q1 = Xp[c + 1];
    for (int q = Xp[c] + (int)threadIdx.x; q < q1; q += kCsrThreads) {
      const int r = Xi[q];
      // rows are distinct inside a canonical column, so the cursor is uncontended; the atomic keeps a column with a
      // repeated row index (not canonical) inside the row's slots
      const int pos = Rp[r] + atomicAdd(&cb[r], 1);
      Rx[pos] = Xx[q];
      if (Rj != nullptr) Rj[pos] = c;
      if (perm != nullptr) perm[pos] = q;
    }
    __syncthreads();   // every slot of column c is taken before column c + 1 takes any
  }
}

// ---- per-row statistics ------------------------------------------------------------------------------------------------
// W = 64: wavefront w of workgroup b owns row 4 b + w (rows longer than kLongRow are left to the W = 256 launch).
// W = 256: workgroups stride over the rows longer than kLongRow.  Entry k of a row goes to lane k % W either way, and the
// path depends on the row's length only: identical rows give identical bits.
template <int W, typename Body>
__device__ __forceinline__ void for_each_row(const int32_t* __restrict__ Rp, int32_t rows, Body body) {
  if (W == 64) {
    const int row = blockIdx.x * (kCsrThreads / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int p0 = Rp[row], len = Rp[row + 1] - p0;
    if (len > kLongRow) return;
    body(row, p0, len, (int)(threadIdx.x & 63));
  } else {
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
      const int p0 = Rp[row], len = Rp[row + 1] - p0;   // (uniform over the workgroup)
      if (len <= kLongRow) continue;
      body(row, p0, len, (int)threadIdx.x);
    }
  }
}

// mean[k][r] = (sum of the stored values of row r in group k) / n_k; ssd[k][r] = sum over the stored values of group k
// of (x - mean_k)^2 + (n_k - nnz_k) mean_k^2 (the implicit zeros).  y == nullptr: every column in group 0.
template <int W>
__global__ void __launch_bounds__(kCsrThreads)
csr_row_moments_kernel(const int32_t* __restrict__ Rp, const int32_t* __restrict__ Rj, const double* __restrict__ Rx,
                       int32_t rows, const int32_t* __restrict__ y, double n0, double n1, double* __restrict__ mean,
                       double* __restrict__ ssd) {
  __shared__ double sh_d[4];
  __shared__ int sh_i[4];
  for_each_row<W>(Rp, rows, [&](int row, int p0, int len, int lane) {
    double s0 = 0.0, s1 = 0.0;
    int k1 = 0;
    for (int k = lane; k < len; k += W) {
      const double v = Rx[p0 + k];
      const int lab = y != nullptr ? y[Rj[p0 + k]] : 0;
      s0 += lab == 0 ? v : 0.0;
      s1 += lab == 1 ? v : 0.0;
      k1 += lab;
    }
    s0 = group_sum_f64<W>(s0, sh_d);
    s1 = group_sum_f64<W>(s1, sh_d);
    k1 = group_sum_i32<W>(k1, sh_i);
    const double m0 = s0 / n0, m1 = s1 / n1;   // an empty group: 0 / 0 = NaN, as launch_row_group_moments
    if (lane == 0) {
      mean[row] = m0;
      mean[rows + row] = m1;
    }
    if (ssd == nullptr) return;
    double q0 = 0.0, q1 = 0.0;
    for (int k = lane; k < len; k += W) {
      const double v = Rx[p0 + k];
      const int lab = y != nullptr ? y[Rj[p0 + k]] : 0;
      const double d0 = v - m0, d1 = v - m1;
      q0 += lab == 0 ? d0 * d0 : 0.0;
      q1 += lab == 1 ? d1 * d1 : 0.0;
    }
    q0 = group_sum_f64<W>(q0, sh_d);
    q1 = group_sum_f64<W>(q1, sh_d);
    const double z0 = n0 - (double)(len - k1), z1 = n1 - (double)k1;   // implicit zeros per group
    if (lane == 0) {
      ssd[row] = z0 > 0.0 ? q0 + z0 * (m0 * m0) : q0;
      ssd[rows + row] = z1 > 0.0 ? q1 + z1 * (m1 * m1) : q1;
    }
  });
}

// the two passes of csr_row_moments_kernel (every column in group 0) over a column shard, apart: mean == nullptr:
// out[row] = the sum of the row's stored values; else out[row] = the sum over them of (x - mean[row])^2.  Same lanes and
// group sums as csr_row_moments_kernel.  The caller adds the shards and the implicit zeros' (n - nnz) mean^2.
template <int W>
__global__ void __launch_bounds__(kCsrThreads)
csr_row_stored_moment_kernel(const int32_t* __restrict__ Rp, const double* __restrict__ Rx, int32_t rows,
                             const double* __restrict__ mean, double* __restrict__ out) {
  __shared__ double sh_d[4];
  for_each_row<W>(Rp, rows, [&](int row, int p0, int len, int lane) {
    double s = 0.0;
    if (mean == nullptr) {
      for (int k = lane; k < len; k += W) s += Rx[p0 + k];
    } else {
      const double mu = mean[row];
      for (int k = lane; k < len; k += W) {
        const double d = Rx[p0 + k] - mu;
        s += d * d;
      }
    }
    s = group_sum_f64<W>(s, sh_d);
    if (lane == 0) out[row] = s;
  });
}

// the unscaled first pass of csr_row_moments_kernel over a column shard's rows: out[k][row] = the sum of the row's stored
// values in group k (y looked up through Rj, the shard's own column index).  Same lanes and group sums; the caller adds
// the shards and divides by the global group sizes.
template <int W>
__global__ void __launch_bounds__(kCsrThreads)
csr_row_group_stored_sums_kernel(const int32_t* __restrict__ Rp, const int32_t* __restrict__ Rj,
                                 const double* __restrict__ Rx, int32_t rows, const int32_t* __restrict__ y,
                                 double* __restrict__ out) {
  __shared__ double sh_d[4];
  for_each_row<W>(Rp, rows, [&](int row, int p0, int len, int lane) {
    double s0 = 0.0, s1 = 0.0;
    for (int k = lane; k < len; k += W) {
      const double v = Rx[p0 + k];
      const int lab = y[Rj[p0 + k]];
      s0 += lab == 0 ? v : 0.0;
      s1 += lab == 1 ? v : 0.0;
    }
    s0 = group_sum_f64<W>(s0, sh_d);
    s1 = group_sum_f64<W>(s1, sh_d);
    if (lane == 0) {
      out[row] = s0;
      out[rows + row] = s1;
    }
  });
}

// ecdf(x)(x_i) * n = #{x <= x_i} from the max-ranks of the stored values among themselves (Rrank) and the row's
// z0 = n - nnz implicit zeros, which lie below every stored value >= 0.  Stored values go to out[perm[p]] (CSC order);
// the implicit zero's value, #{stored <= 0} + z0, to dflt[row].  Integers throughout: exact.
template <int W>
__global__ void __launch_bounds__(kCsrThreads)
csr_row_ecdf_kernel(const int32_t* __restrict__ Rp, const double* __restrict__ Rx, const double* __restrict__ Rrank,
                    int32_t rows, int32_t n, const int32_t* __restrict__ perm, double* __restrict__ out,
                    double* __restrict__ dflt) {
  __shared__ int sh_i[4];
  for_each_row<W>(Rp, rows, [&](int row, int p0, int len, int lane) {
    const double z0 = (double)(n - len);
    int le0 = 0;
    for (int k = lane; k < len; k += W) {
      const double v = Rx[p0 + k];
      le0 += v <= 0.0 ? 1 : 0;
      out[perm[p0 + k]] = Rrank[p0 + k] + (v >= 0.0 ? z0 : 0.0);
    }
    le0 = group_sum_i32<W>(le0, sh_i);
    if (lane == 0) dflt[row] = (double)le0 + z0;
  });
}

// the z transform's value of an implicit zero, in the expression of row_ztransform_kernel (kernels_stats.hip)
__device__ __forceinline__ double ztransform(double x, double mu, double ssd, int32_t n) {
  const double den = 1e-8 + sqrt(ssd / (double)(n - 1));
  return (x - mu) / den;
}

__global__ void __launch_bounds__(kCsrThreads)
row_z_default_kernel(const double* __restrict__ mean, const double* __restrict__ ssd, int32_t rows, int32_t n,
                     double* __restrict__ dflt) {
  const int r = blockIdx.x * kCsrThreads + threadIdx.x;
  if (r < rows) dflt[r] = ztransform(0.0, mean[r], ssd[r], n);
}

// dense column-major out (g x n, leading dimension ld): row i of every column gets dflt[i] (the padding rows 0), then
// the stored entries their value -- vals[q] itself (ecdf), or its z transform when mean / ssd are given (moments over
// n_sd samples: n, or all columns of a sharded X).
__device__ __forceinline__ void csc_expand_body(const int32_t* __restrict__ Xp, const int32_t* __restrict__ Xi,
                                                const double* __restrict__ vals, int32_t g, int32_t n, int32_t n_sd,
                                                int64_t ld, const double* __restrict__ dflt,
                                                const double* __restrict__ mean, const double* __restrict__ ssd,
                                                double* __restrict__ out) {
  const int tid = threadIdx.x;
  for (int c = blockIdx.x; c < n; c += gridDim.x) {
    double* oc = out + (int64_t)c * ld;
    for (int i = tid; i < ld; i += kCsrThreads) oc[i] = i < g ? dflt[i] : 0.0;
    __syncthreads();   // the column is filled (this workgroup's stores are performed) before single rows are overwritten
    const int q1 = Xp[c + 1];
    for (int q = Xp[c] + tid; q < q1; q += kCsrThreads) {
      const int r = Xi[q];
      oc[r] = mean != nullptr ? ztransform(vals[q], mean[r], ssd[r], n_sd) : vals[q];
    }
  }
}

__global__ void __launch_bounds__(kCsrThreads)
csc_expand_kernel(const int32_t* __restrict__ Xp, const int32_t* __restrict__ Xi, const double* __restrict__ vals,
                  int32_t g, int32_t n, int64_t ld, const double* __restrict__ dflt, const double* __restrict__ mean,
                  const double* __restrict__ ssd, double* __restrict__ out) {
  csc_expand_body(Xp, Xi, vals, g, n, n, ld, dflt, mean, ssd, out);
}

__global__ void __launch_bounds__(kCsrThreads)
csc_expand_shard_kernel(const int32_t* __restrict__ Xp, const int32_t* __restrict__ Xi, const double* __restrict__ vals,
                        int32_t g, int32_t ncols, int32_t n_total, int64_t ld, const double* __restrict__ dflt,
                        const double* __restrict__ mean, const double* __restrict__ ssd, double* __restrict__ out) {
  csc_expand_body(Xp, Xi, vals, g, ncols, n_total, ld, dflt, mean, ssd, out);
}

}  // namespace

int launch_csc_to_csr(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* Xx, int32_t g, int32_t n,
                      int32_t* Rp, int32_t* Rj, double* Rx, int32_t* perm, int32_t* d_maxlen) {
  if (g <= 0) return PLAIDHIP_OK;
  // column blocks: about two per CU, fewer when the count table would pass kCountBytes
  int64_t nblk = std::min<int64_t>(n, 2 * (int64_t)ctx->num_cu);
  nblk = std::min<int64_t>(nblk, std::max<int64_t>(1, (int64_t)(kCountBytes / 4) / g));
  const int32_t cpb = n > 0 ? (int32_t)((n + nblk - 1) / nblk) : 1;
  if (n > 0) nblk = (n + cpb - 1) / cpb;
  const size_t cnt_bytes = (size_t)std::max<int64_t>(nblk, 1) * (size_t)g * 4;
  const int rc = ensure_workspace(ctx, cnt_bytes);
  if (rc != PLAIDHIP_OK) return rc;
  int32_t* cnt = static_cast<int32_t*>(ctx->ws);
  PH_HIP(hipMemsetAsync(cnt, 0, cnt_bytes, ctx->stream));
  if (nblk > 0)
    hipLaunchKernelGGL(csc_block_count_kernel, dim3((unsigned)nblk), dim3(kCsrThreads), 0, ctx->stream, Xp, Xi, n, g, cpb,
                       cnt);
  hipLaunchKernelGGL(csc_block_offsets_kernel, dim3((g + kCsrThreads - 1) / kCsrThreads), dim3(kCsrThreads), 0, ctx->stream,
                     cnt, (int32_t)nblk, g, Rp);
  hipLaunchKernelGGL(row_pointer_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, Rp, g, d_maxlen);
  if (nblk > 0)
    hipLaunchKernelGGL(csc_block_fill_kernel, dim3((unsigned)nblk), dim3(kCsrThreads), 0, ctx->stream, Xp, Xi, Xx, n, g, cpb,
                       cnt, Rp, Rj, Rx, perm);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_csr_row_group_moments(plaidhip_ctx* ctx, const int32_t* Rp, const int32_t* Rj, const double* Rx, int32_t rows,
                                 int32_t max_row_nnz, const int32_t* d_y, int64_t n0, int64_t n1, double* d_mean,
                                 double* d_ssd) {
  if (rows <= 0) return PLAIDHIP_OK;
  const int rows_per_block = kCsrThreads / 64;
  hipLaunchKernelGGL(csr_row_moments_kernel<64>, dim3((rows + rows_per_block - 1) / rows_per_block), dim3(kCsrThreads), 0,
                     ctx->stream, Rp, Rj, Rx, rows, d_y, (double)n0, (double)n1, d_mean, d_ssd);
  if (max_row_nnz > kLongRow)
    hipLaunchKernelGGL(csr_row_moments_kernel<256>, dim3(std::min(rows, 2 * ctx->num_cu)), dim3(kCsrThreads), 0, ctx->stream,
                       Rp, Rj, Rx, rows, d_y, (double)n0, (double)n1, d_mean, d_ssd);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_csr_row_stored_moment(plaidhip_ctx* ctx, const int32_t* Rp, const double* Rx, int32_t rows, int32_t max_row_nnz,
                                 const double* d_mean, double* d_out) {
  if (rows <= 0) return PLAIDHIP_OK;
  const int rows_per_block = kCsrThreads / 64;
  hipLaunchKernelGGL(csr_row_stored_moment_kernel<64>, dim3((rows + rows_per_block - 1) / rows_per_block), dim3(kCsrThreads),
                     0, ctx->stream, Rp, Rx, rows, d_mean, d_out);
  if (max_row_nnz > kLongRow)
    hipLaunchKernelGGL(csr_row_stored_moment_kernel<256>, dim3(std::min(rows, 2 * ctx->num_cu)), dim3(kCsrThreads), 0,
                       ctx->stream, Rp, Rx, rows, d_mean, d_out);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_csr_row_group_stored_sums(plaidhip_ctx* ctx, const int32_t* Rp, const int32_t* Rj, const double* Rx, int32_t rows,
                                     int32_t max_row_nnz, const int32_t* d_y, double* d_out) {
  if (rows <= 0) return PLAIDHIP_OK;
  const int rows_per_block = kCsrThreads / 64;
  hipLaunchKernelGGL(csr_row_group_stored_sums_kernel<64>, dim3((rows + rows_per_block - 1) / rows_per_block),
                     dim3(kCsrThreads), 0, ctx->stream, Rp, Rj, Rx, rows, d_y, d_out);
  if (max_row_nnz > kLongRow)
    hipLaunchKernelGGL(csr_row_group_stored_sums_kernel<256>, dim3(std::min(rows, 2 * ctx->num_cu)), dim3(kCsrThreads), 0,
                       ctx->stream, Rp, Rj, Rx, rows, d_y, d_out);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_csr_row_ecdf(plaidhip_ctx* ctx, const int32_t* Rp, const double* Rx, int32_t rows, int32_t n,
                        int32_t max_row_nnz, const int32_t* perm, double* Rrank, double* out, double* dflt) {
  if (rows <= 0) return PLAIDHIP_OK;
  // ranks of each row's stored values among themselves, ties = max (rows as the columns of the CSC rank kernels)
  const int rc = launch_colranks_csc_f64(ctx, Rp, Rx, rows, max_row_nnz, PLAIDHIP_TIES_MAX, 0, 1.0, Rrank, nullptr);
  if (rc != PLAIDHIP_OK) return rc;
  const int rows_per_block = kCsrThreads / 64;
  hipLaunchKernelGGL(csr_row_ecdf_kernel<64>, dim3((rows + rows_per_block - 1) / rows_per_block), dim3(kCsrThreads), 0,
                     ctx->stream, Rp, Rx, Rrank, rows, n, perm, out, dflt);
  if (max_row_nnz > kLongRow)
    hipLaunchKernelGGL(csr_row_ecdf_kernel<256>, dim3(std::min(rows, 2 * ctx->num_cu)), dim3(kCsrThreads), 0, ctx->stream,
                       Rp, Rx, Rrank, rows, n, perm, out, dflt);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_row_z_defaults(plaidhip_ctx* ctx, const double* d_mean, const double* d_ssd, int32_t rows, int32_t n,
                          double* dflt) {
  if (rows <= 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(row_z_default_kernel, dim3((rows + kCsrThreads - 1) / kCsrThreads), dim3(kCsrThreads), 0, ctx->stream,
                     d_mean, d_ssd, rows, n, dflt);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_csc_expand(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* vals, int32_t g, int32_t n,
                      int64_t ld, const double* dflt, const double* d_mean, const double* d_ssd, double* out) {
  if (g <= 0 || n <= 0) return PLAIDHIP_OK;
  const int cap = ctx->num_cu * 8;
  hipLaunchKernelGGL(csc_expand_kernel, dim3(n < cap ? n : cap), dim3(kCsrThreads), 0, ctx->stream, Xp, Xi, vals, g, n, ld,
                     dflt, d_mean, d_ssd, out);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_csc_expand_shard(plaidhip_ctx* ctx, const int32_t* Xp, const int32_t* Xi, const double* vals, int32_t g,
                            int32_t ncols, int32_t n_total, int64_t ld, const double* dflt, const double* d_mean,
                            const double* d_ssd, double* out) {
  if (g <= 0 || ncols <= 0) return PLAIDHIP_OK;
  const int cap = ctx->num_cu * 8;
  hipLaunchKernelGGL(csc_expand_shard_kernel, dim3(ncols < cap ? ncols : cap), dim3(kCsrThreads), 0, ctx->stream, Xp, Xi, vals,
                     g, ncols, n_total, ld, dflt, d_mean, d_ssd, out);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
