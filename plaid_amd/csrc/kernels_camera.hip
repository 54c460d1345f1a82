// plaid.camera: the two device passes behind the variance inflation factor of every set (include/plaidhip.h:
// plaidhip_camera, steps 2 and 3).
//
// camera_residual_kernel is row_design_rss_kernel (kernels_lmfit.hip) with a store in place of the square: the same thread
// and row geometry (a thread owns two adjacent rows and walks a block of 128 columns, the sample's row of Q_f and its "used"
// bit are wavefront-uniform, a thread's p effects live in registers), the same chain -- camera_chain_step (camera.h) in
// ascending k from x_c -- and then z = r / sqrt(max(s2, 1e-8)) or 0.0, written as genes x n column-major, the layout the
// dense crossprod reads.  The gene's divisor is taken once per (thread, column block) from rss / d.
// camera_sumsq_kernel squares T = G'Z: a thread owns one set and one block of 128 columns, adds t * t (rounded, then added)
// in ascending column order from 0.0 and leaves a block partial; consecutive threads read consecutive sets of a column of
// the set-major T, so every load is coalesced.  The blocks are added in ascending order from a seed by
// reduce_blocks_flat_kernel (kernels_contrasts.hip): the order of the RSS pass, whatever the sharding.
#include "common.h"
#include "camera.h"

#pragma clang fp contract(off)

namespace plaidhip {

constexpr int kCamColBlock = 128;   // kernels_lmfit.hip's column block (launch_reduce_blocks_flat counts in it)
constexpr int kCamTile = PLAIDHIP_LIMMA_TILE;

// Z[r, c] of fit f for the rows x n matrix A: E [W][rows] the effects of ALL samples, rss [nfit][rows] likewise, d = n_f - p.
// masks: launch_lmfit_masks of the same n and W (the bit of the fit's mean column says "used by fit f").
template <int kP, bool kWide>
__global__ void __launch_bounds__(256)
camera_residual_kernel(const double* __restrict__ A, int64_t ld, int32_t rows, int32_t n, const double* __restrict__ Q,
                       const uint32_t* __restrict__ masks, int32_t p, int32_t f, const double* __restrict__ E,
                       const double* __restrict__ rss, double d, double* __restrict__ Z, int64_t ldz) {
  typedef double f64x2_s __attribute__((ext_vector_type(2)));
  constexpr int kUn = 8;
  const int r = 2 * (blockIdx.x * 256 + threadIdx.x);
  const int c0 = blockIdx.y * kCamColBlock;
  const int c1 = c0 + kCamColBlock < n ? c0 + kCamColBlock : n;
  const int64_t jm = (int64_t)f * (p + 1) + p;
  const uint32_t* __restrict__ mk = masks + (jm / kCamTile) * n;
  const int bit = (int)(jm % kCamTile);
  const double* __restrict__ Qf = Q + (int64_t)f * p * n;
  if (r >= rows) return;
  const bool two = r + 1 < rows;   // (false only for the last row of an odd `rows`: never kWide)
  double ea[kP], eb[kP];
#pragma unroll
  for (int k = 0; k < kP; ++k) {
    ea[k] = eb[k] = 0.0;
    if (k < p) {
      const double* e = E + ((int64_t)f * (p + 1) + k) * rows;
      ea[k] = e[r];
      if (two) eb[k] = e[r + 1];
    }
  }
  const double* __restrict__ rf = rss + (int64_t)f * rows;
  const double sa = camera_gene_scale(rf[r], d);
  const double sb = two ? camera_gene_scale(rf[r + 1], d) : __builtin_nan("");
  auto residuals = [&](int c, double xa, double xb) {
    const bool in = ((mk[c] >> bit) & 1u) != 0;
    double ra = xa, rb = xb;
#pragma unroll
    for (int k = 0; k < kP; ++k) {
      if (k >= p) break;
      const double qk = Qf[(int64_t)k * n + c];
      ra = camera_chain_step(qk, ea[k], ra);
      rb = camera_chain_step(qk, eb[k], rb);
    }
    const double za = camera_standardise(ra, sa, in), zb = camera_standardise(rb, sb, in);
    double* o = Z + (int64_t)c * ldz + r;
    if (kWide) {
      f64x2_s v;
      v.x = za;
      v.y = zb;
      *reinterpret_cast<f64x2_s*>(o) = v;
    } else {
      o[0] = za;
      if (two) o[1] = zb;
    }
  };
  auto load = [&](int c, double& xa, double& xb) {
    const double* q = A + (int64_t)c * ld + r;
    if (kWide) {
      const f64x2_s v = __builtin_nontemporal_load(reinterpret_cast<const f64x2_s*>(q));
      xa = v.x;
      xb = v.y;
    } else {
      xa = __builtin_nontemporal_load(q);
      xb = two ? __builtin_nontemporal_load(q + 1) : 0.0;
    }
  };
  int c = c0;
  for (; c + kUn <= c1; c += kUn) {
    double xa[kUn], xb[kUn];
#pragma unroll
    for (int u = 0; u < kUn; ++u) load(c + u, xa[u], xb[u]);
#pragma unroll
    for (int u = 0; u < kUn; ++u) residuals(c + u, xa[u], xb[u]);
  }
  for (; c < c1; ++c) {
    double xa, xb;
    load(c, xa, xb);
    residuals(c, xa, xb);
  }
}

// part[block][set] = the sum over the block's columns of T[set, c]^2; T: m x n column-major, leading dimension ldt;
// `stride` doubles from one block's partials to the next (several fits' partials lie side by side)
__global__ void __launch_bounds__(256)
camera_sumsq_kernel(const double* __restrict__ T, int64_t ldt, int32_t m, int32_t n, double* __restrict__ part, int64_t stride) {
  constexpr int kUn = 8;
  const int s = blockIdx.x * 256 + threadIdx.x;
  const int c0 = blockIdx.y * kCamColBlock;
  const int c1 = c0 + kCamColBlock < n ? c0 + kCamColBlock : n;
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

template <int kP>
static void launch_residuals_p(plaidhip_ctx* ctx, bool wide, dim3 grid, const double* A, int64_t ld, int32_t rows, int32_t n,
                               const double* d_Q, const uint32_t* mk, int32_t p, int32_t f, const double* d_E, const double* d_rss,
                               double d, double* Z, int64_t ldz) {
  if (wide)
    hipLaunchKernelGGL((camera_residual_kernel<kP, true>), grid, dim3(256), 0, ctx->stream, A, ld, rows, n, d_Q, mk, p, f, d_E,
                       d_rss, d, Z, ldz);
  else
    hipLaunchKernelGGL((camera_residual_kernel<kP, false>), grid, dim3(256), 0, ctx->stream, A, ld, rows, n, d_Q, mk, p, f, d_E,
                       d_rss, d, Z, ldz);
}

// Z (rows x n, leading dimension ldz >= rows) of fit f; d_Q: n x p x nfit, d_masks: launch_lmfit_masks of the same n and
// W = nfit (p + 1); d_E: [W][rows] and d_rss: [nfit][rows], both of ALL samples; d = n_f - p
int launch_camera_residuals(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const double* d_Q,
                            const void* d_masks, int32_t p, int32_t f, const double* d_E, const double* d_rss, double d, double* Z,
                            int64_t ldz) {
  if (rows == 0 || n == 0) return PLAIDHIP_OK;
  const int nblk = (n + kCamColBlock - 1) / kCamColBlock;
  const dim3 grid((rows + 511) / 512, nblk);
  const uint32_t* mk = static_cast<const uint32_t*>(d_masks);
  const bool wide = (rows & 1) == 0 && (ld & 1) == 0 && (ldz & 1) == 0 && (reinterpret_cast<uintptr_t>(A) & 15u) == 0 &&
                    (reinterpret_cast<uintptr_t>(Z) & 15u) == 0;
  if (p <= 4) launch_residuals_p<4>(ctx, wide, grid, A, ld, rows, n, d_Q, mk, p, f, d_E, d_rss, d, Z, ldz);
  else if (p <= 8) launch_residuals_p<8>(ctx, wide, grid, A, ld, rows, n, d_Q, mk, p, f, d_E, d_rss, d, Z, ldz);
  else if (p <= 16) launch_residuals_p<16>(ctx, wide, grid, A, ld, rows, n, d_Q, mk, p, f, d_E, d_rss, d, Z, ldz);
  else launch_residuals_p<32>(ctx, wide, grid, A, ld, rows, n, d_Q, mk, p, f, d_E, d_rss, d, Z, ldz);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// doubles of the block partials [nblk][len]
int64_t camera_sumsq_ws_doubles(int32_t n, int64_t len) {
  const int64_t nblk = (n + kCamColBlock - 1) / kCamColBlock;
  return len * (nblk > 0 ? nblk : 1);
}

// part[block][set] for the m x n matrix T; reduced by launch_reduce_blocks_flat(part, stride, n, seed, out)
int launch_camera_sumsq(plaidhip_ctx* ctx, const double* T, int64_t ldt, int32_t m, int32_t n, double* part, int64_t stride) {
  if (m == 0 || n == 0) return PLAIDHIP_OK;
  const int nblk = (n + kCamColBlock - 1) / kCamColBlock;
  hipLaunchKernelGGL(camera_sumsq_kernel, dim3((m + 255) / 256, nblk), dim3(256), 0, ctx->stream, T, ldt, m, n, part, stride);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
