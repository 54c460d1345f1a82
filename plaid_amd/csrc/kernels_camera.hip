// plaid.camera: the two device passes behind the variance inflation factor of every set (include/plaidhip.h:
// plaidhip_camera, steps 2 and 3).
//
// camera_residual_kernel is the residual store of row_pair.h (row_pair_residual_store: row_design_rss_kernel's thread and row
// geometry, walk and chain with a store in place of the square) with z = r / sqrt(max(s2, 1e-8)) or 0.0: the gene's divisor
// is taken once per (thread, column block) from rss / d (camera.h).
// camera_sumsq_kernel squares T = G'Z: a thread owns one set and one block of 128 columns, adds t * t (rounded, then added)
// in ascending column order from 0.0 and leaves a block partial; consecutive threads read consecutive sets of a column of
// the set-major T, so every load is coalesced.  The blocks are added in ascending order from a seed by
// reduce_blocks_flat_kernel (kernels_contrasts.hip): the order of the RSS pass, whatever the sharding.
#include "common.h"
#include "camera.h"
#include "row_pair.h"

#pragma clang fp contract(off)

namespace plaidhip {

// Z[r, c] of fit f for the rows x n matrix A: E [W][rows] the effects of ALL samples, rss [nfit][rows] likewise, d = n_f - p.
// masks: launch_lmfit_masks of the same n and W (the bit of the fit's mean column says "used by fit f").
template <int kP, bool kWide>
__global__ void __launch_bounds__(256)
camera_residual_kernel(const double* __restrict__ A, int64_t ld, int32_t rows, int32_t n, const double* __restrict__ Q,
                       const uint32_t* __restrict__ masks, int32_t p, int32_t f, const double* __restrict__ E,
                       const double* __restrict__ rss, double d, double* __restrict__ Z, int64_t ldz) {
  const double* __restrict__ rf = rss + (int64_t)f * rows;
  row_pair_residual_store<kP, kWide>(
      A, ld, rows, n, Q, masks, p, f, E, Z, ldz, [&](int r) { return camera_gene_scale(rf[r], d); },
      [](double r, double scale, bool used) { return camera_standardise(r, scale, used); });
}

// part[block][set] = the sum over the block's columns of T[set, c]^2; T: m x n column-major, leading dimension ldt;
// `stride` doubles from one block's partials to the next (several fits' partials lie side by side)
__global__ void __launch_bounds__(256)
camera_sumsq_kernel(const double* __restrict__ T, int64_t ldt, int32_t m, int32_t n, double* __restrict__ part, int64_t stride) {
  constexpr int kUn = 8;
  const int s = blockIdx.x * 256 + threadIdx.x;
  const int c0 = blockIdx.y * kRowColBlock;
  const int c1 = c0 + kRowColBlock < n ? c0 + kRowColBlock : n;
  if (s >= m) return;
  double acc = 0.0;
  int c = c0;
  for (; c + kUn <= c1; c += kUn) {
    double t[kUn];
#pragma unroll
    for (int u = 0; u < kUn; ++u) t[u] = T[(int64_t)(c + u) * ldt + s];
#pragma unroll
    for (int u = 0; u < kUn; ++u) {
      const double sq = t[u] * t[u];
      acc += sq;
    }
  }
  for (; c < c1; ++c) {
    const double t = T[(int64_t)c * ldt + s];
    const double sq = t * t;
    acc += sq;
  }
  part[(int64_t)blockIdx.y * stride + s] = acc;
}

// Z (rows x n, leading dimension ldz >= rows) of fit f; d_Q: n x p x nfit, d_masks: launch_lmfit_masks of the same n and
// W = nfit (p + 1); d_E: [W][rows] and d_rss: [nfit][rows], both of ALL samples; d = n_f - p
int launch_camera_residuals(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const double* d_Q,
                            const void* d_masks, int32_t p, int32_t f, const double* d_E, const double* d_rss, double d, double* Z,
                            int64_t ldz) {
  if (rows == 0 || n == 0) return PLAIDHIP_OK;
  const int nblk = (n + kRowColBlock - 1) / kRowColBlock;
  const dim3 grid((rows + 511) / 512, nblk);
  const uint32_t* mk = static_cast<const uint32_t*>(d_masks);
  dispatch_p(p, [&](auto kp) {
    dispatch_flag(row_pair_wide(rows, {ld, ldz}, {A, Z}), [&](auto wide) {
      hipLaunchKernelGGL((camera_residual_kernel<decltype(kp)::value, decltype(wide)::value>), grid, dim3(256), 0, ctx->stream, A, ld,
                         rows, n, d_Q, mk, p, f, d_E, d_rss, d, Z, ldz);
    });
  });
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// doubles of the block partials [nblk][len]
int64_t camera_sumsq_ws_doubles(int32_t n, int64_t len) {
  const int64_t nblk = (n + kRowColBlock - 1) / kRowColBlock;
  return len * (nblk > 0 ? nblk : 1);
}

// part[block][set] for the m x n matrix T; reduced by launch_reduce_blocks_flat(part, stride, n, seed, out)
int launch_camera_sumsq(plaidhip_ctx* ctx, const double* T, int64_t ldt, int32_t m, int32_t n, double* part, int64_t stride) {
  if (m == 0 || n == 0) return PLAIDHIP_OK;
  const int nblk = (n + kRowColBlock - 1) / kRowColBlock;
  hipLaunchKernelGGL(camera_sumsq_kernel, dim3((m + 255) / 256, nblk), dim3(256), 0, ctx->stream, T, ldt, m, n, part, stride);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
