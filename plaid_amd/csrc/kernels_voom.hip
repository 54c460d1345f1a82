// plaid.voom: the device passes of include/plaidhip.h (plaidhip_voom) over a rows x n matrix of counts.
//   check      column sums, and a flag for any count that is not finite and >= 0 (one workgroup per column)
//   row sums   block partials [block of 128 columns][rows], added in ascending order (reduce_blocks_flat_kernel)
//   log-CPM    E = log2(((x + 0.5) / (L_c + 1)) * 1e6), in that operation order
//   weights    mu = the fma chain of q_ck E_k, lambda = mu + offset_c, f(lambda) by bisection in the knots (LDS) and linear
//              interpolation, w = 1 / ((f f) (f f)); a thread keeps its row's p effects in registers
// The unweighted fit between them is kernels_lmfit.hip's two passes.  Compiled with -ffp-contract=off (and says so below).
#include "common.h"
#include "row_pair.h"   // kRowColBlock: the one-row kernels below keep their own loops

#pragma clang fp contract(off)

namespace plaidhip {

namespace {
constexpr int kVKnots = PLAIDHIP_VOOM_MAX_KNOTS;
}  // namespace

// colsum[c] = sum over the rows of X[r, c]: thread t of 256 adds rows t, t + 256, ... in ascending order from 0.0, then the 256
// partials are folded in halves (s_t += s_{t + off}, off = 128, 64, ..., 1).  *bad |= 1 where a count is NaN, negative or +Inf.
__global__ void __launch_bounds__(256)
voom_check_kernel(const double* __restrict__ X, int64_t ld, int32_t rows, double* __restrict__ colsum, uint32_t* __restrict__ bad) {
  __shared__ double sh[256];
  const int t = threadIdx.x;
  const double* col = X + (int64_t)blockIdx.x * ld;
  double s = 0.0;
  bool b = false;
  for (int r = t; r < rows; r += 256) {
    const double v = col[r];
    b = b || !(v >= 0.0 && v < __builtin_inf());
    s = s + v;
  }
  sh[t] = s;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if (t < off) sh[t] = sh[t] + sh[t + off];
    __syncthreads();
  }
  if (t == 0) colsum[blockIdx.x] = sh[0];
  if (b) atomicOr(bad, 1u);
}

// part[block][r] = the sum of row r over the block's columns in ascending order from 0.0
__global__ void __launch_bounds__(256)
voom_rowsum_kernel(const double* __restrict__ X, int64_t ld, int32_t rows, int32_t n, double* __restrict__ part) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  const int c0 = blockIdx.y * kRowColBlock;
  const int c1 = c0 + kRowColBlock < n ? c0 + kRowColBlock : n;
  if (r >= rows) return;
  double s = 0.0;
  for (int c = c0; c < c1; ++c) s = s + X[(int64_t)c * ld + r];
  part[(int64_t)blockIdx.y * rows + r] = s;
}

// E[r, c] = log2(((x + 0.5) / (L_c + 1.0)) * 1e6); lib: the n library sizes
__global__ void __launch_bounds__(256)
voom_logcpm_kernel(const double* __restrict__ X, int64_t ld, int32_t rows, const double* __restrict__ lib, double* __restrict__ E,
                   int64_t lde) {
  const int r = blockIdx.y * 256 + threadIdx.x;
  const int c = blockIdx.x;
  if (r >= rows) return;
  const double l1 = lib[c] + 1.0;   // wave-uniform
  const double x = X[(int64_t)c * ld + r];
  E[(int64_t)c * lde + r] = log2(((x + 0.5) / l1) * 1e6);
}

// f(lambda) in the knots (kx ascending, nk >= 1): the end values outside, else the largest k with kx[k] <= lambda by
// bisection and ky[k] + (ky[k + 1] - ky[k]) * ((lambda - kx[k]) / (kx[k + 1] - kx[k])) -- exactly ky[k] at a knot
__device__ inline double voom_trend(const double* kx, const double* ky, int nk, double lam) {
  if (!(lam > kx[0])) return ky[0];
  if (lam >= kx[nk - 1]) return ky[nk - 1];
  int lo = 0, hi = nk - 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (kx[mid] <= lam) lo = mid;
    else hi = mid;
  }
  return ky[lo] + (ky[lo + 1] - ky[lo]) * ((lam - kx[lo]) / (kx[lo + 1] - kx[lo]));
}

// W[r, c] of a block of 128 columns; Eff: [p + 1][rows] (the mean's row is not read); Q: n x p; off: n; the knots go to LDS
// (2 x 256 doubles, 4 KB).  f <= 0 or NaN: the weight is NaN, which the weighted fit treats as a missing observation.
template <int kP>
__global__ void __launch_bounds__(256)
voom_weights_kernel(const double* __restrict__ Q, const double* __restrict__ off, int32_t n, int32_t p,
                    const double* __restrict__ Eff, int32_t rows, const double* __restrict__ knx, const double* __restrict__ kny,
                    int32_t nk, double* __restrict__ W, int64_t ldw) {
  __shared__ double kx[kVKnots], ky[kVKnots];
  for (int i = threadIdx.x; i < nk; i += 256) {
    kx[i] = knx[i];
    ky[i] = kny[i];
  }
  __syncthreads();
  const int r = blockIdx.x * 256 + threadIdx.x;
  const int c0 = blockIdx.y * kRowColBlock;
  const int c1 = c0 + kRowColBlock < n ? c0 + kRowColBlock : n;
  if (r >= rows) return;
  double e[kP];
#pragma unroll
  for (int k = 0; k < kP; ++k) e[k] = k < p ? Eff[(int64_t)k * rows + r] : 0.0;
  for (int c = c0; c < c1; ++c) {
    double mu = 0.0;
#pragma unroll
    for (int k = 0; k < kP; ++k)   // (no early exit: the unrolled loop keeps e[] in registers; Q's entry is wave-uniform)
      mu = k < p ? __builtin_fma(Q[(int64_t)k * n + c], e[k], mu) : mu;
    const double lam = mu + off[c];
    const double f = voom_trend(kx, ky, nk, lam);
    const double f2 = f * f;
    W[(int64_t)c * ldw + r] = f > 0.0 ? 1.0 / (f2 * f2) : __builtin_nan("");
  }
}

// ---- the launchers (common.h) -------------------------------------------------------------------------------------------------
int launch_voom_check(plaidhip_ctx* ctx, const double* X, int64_t ld, int32_t rows, int32_t n, double* d_colsum, uint32_t* d_bad) {
  if (n == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(voom_check_kernel, dim3((unsigned)n), dim3(256), 0, ctx->stream, X, ld, rows, d_colsum, d_bad);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// part: row_design_ws_doubles(rows, n, 1) doubles, [nblk][rows]
int launch_voom_rowsum(plaidhip_ctx* ctx, const double* X, int64_t ld, int32_t rows, int32_t n, double* part) {
  if (rows == 0 || n == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(voom_rowsum_kernel, dim3((rows + 255) / 256, (n + kRowColBlock - 1) / kRowColBlock), dim3(256), 0, ctx->stream, X,
                     ld, rows, n, part);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_voom_logcpm(plaidhip_ctx* ctx, const double* X, int64_t ld, int32_t rows, int32_t n, const double* d_lib, double* E,
                       int64_t lde) {
  if (rows == 0 || n == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(voom_logcpm_kernel, dim3((unsigned)n, (rows + 255) / 256), dim3(256), 0, ctx->stream, X, ld, rows, d_lib, E, lde);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_voom_weights(plaidhip_ctx* ctx, const double* d_Q, const double* d_off, int32_t n, int32_t p, const double* d_Eff,
                        int32_t rows, const double* d_kx, const double* d_ky, int32_t nk, double* W, int64_t ldw) {
  if (rows == 0 || n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(nk >= 1 && nk <= kVKnots, "voom: %d knots (1 <= knots <= %d)", nk, kVKnots);
  PH_REQUIRE(p >= 1 && p <= PLAIDHIP_LIMMA_MAX_COEF, "voom: p = %d coefficients (1 <= p <= %d)", p, PLAIDHIP_LIMMA_MAX_COEF);
  const dim3 grid((rows + 255) / 256, (n + kRowColBlock - 1) / kRowColBlock);
#define PH_VOOM_W(KP)                                                                                                        \
  hipLaunchKernelGGL((voom_weights_kernel<KP>), grid, dim3(256), 0, ctx->stream, d_Q, d_off, n, p, d_Eff, rows, d_kx, d_ky, nk, W, \
                     ldw)
  if (p <= 4) PH_VOOM_W(4);
  else if (p <= 8) PH_VOOM_W(8);
  else if (p <= 16) PH_VOOM_W(16);
  else PH_VOOM_W(32);
#undef PH_VOOM_W
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
