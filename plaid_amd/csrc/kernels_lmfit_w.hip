// plaid.limma with weights: the per-row weighted fit of include/plaidhip.h (plaidhip_limma_w).
//
// kernels_lmfit.hip with a second matrix beside A (row_pair.h: row_pair_walk2).  The basis stays the unweighted Q_f of the
// design; what a row needs of it with its own weights omega_c are the Gram sums H_kl = sum_c omega_c q_ck q_cl (l <= k),
// b_k = sum_c (omega_c x_c) q_ck and the mean's M', all over its live observations.  So fit f has Wc = p (p + 1) / 2 + p + 1
// weight columns
//     [ pi_c,kl = q_ck q_cl, row by row of the triangle | q_ck | 1 / n_f ]
// that are the same for every row -- wave-uniform, read through scalar loads -- and the per-row factor is omega, omega x or x
// by the column's kind.  The columns of all fits lie side by side and are cut into tiles of kTile as in kernels_lmfit.hip:
// a thread owns two adjacent rows, walks a block of 128 columns in ascending order and keeps the tile's accumulators in
// registers, so A and the weights are read ceil(nfit Wc / kTile) times for the sums and nfit times for the residuals.
//     acc = sel ? fma(factor, column, acc) : acc      sel: live (H, b) or "c in sel and x == x" (M')
//     part[block][column][row], blocks added in ascending order from an optional seed (reduce_blocks_flat_kernel)
// The solve of every (row, fit) is a thread of its own with H in LDS (lmfit_na.h: lmfit_w_row_solve).  Compiled with
// -ffp-contract=off (and says so below): the only fused operations are the fma written out.
#include "common.h"
#include "lmfit_na.h"
#include "row_pair.h"

#pragma clang fp contract(off)

namespace plaidhip {

namespace {

constexpr int kWTile = PLAIDHIP_LIMMA_TILE;
constexpr int kWP = PLAIDHIP_LIMMA_NA_MAX_COEF;
constexpr int kWFitTile = 8;      // the fits whose counts share one read of A and the weights

__host__ __device__ inline int64_t w_cols(int p) { return (int64_t)p * (p + 1) / 2 + p + 1; }

// omega of an observation: Wt * aw in one rounded product; an operand that is not there counts as 1.0 and no product is taken
__device__ inline double w_omega(bool has_wt, double wt, bool has_aw, double aw) {
  return has_wt ? (has_aw ? wt * aw : wt) : aw;
}
__device__ inline bool w_live(double x, double om) { return x == x && om > 0.0 && om < __builtin_inf(); }

}  // namespace

// masks[tile][c]: bit t = sample c is used by the fit of column tile * kTile + t; wt[tile][c][t]: that column's entry for the
// sample -- q_ck * q_cl rounded once, q_ck, or 1 / n_f; 0.0 for an excluded sample and past the last column.  lmfit_masks_kernel
// with the products.  Q: n x p x nfit, use: n x nfit or null, invn: nfit (null: 0.0, for a caller that reads the masks alone).
__global__ void __launch_bounds__(256)
lmfit_w_table_kernel(const double* __restrict__ Q, const int8_t* __restrict__ use, const double* __restrict__ invn, int32_t n,
                     int32_t p, int32_t nfit, uint32_t* __restrict__ masks, double* __restrict__ wt) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int tile = blockIdx.y;
  if (c >= n) return;
  const int64_t Wc = w_cols(p), W = nfit * Wc;
  const int T = p * (p + 1) / 2;
  uint32_t bits = 0;
  double* w = wt + ((int64_t)tile * n + c) * kWTile;
  for (int t = 0; t < kWTile; ++t) {
    const int64_t j = (int64_t)tile * kWTile + t;
    double v = 0.0;
    if (j < W) {
      const int64_t f = j / Wc;
      const int jj = (int)(j % Wc);
      if (use == nullptr || use[f * n + c] != 0) {
        bits |= 1u << t;
        const double* qf = Q + f * p * n + c;
        if (jj < T) {
          int k = 0, l = jj;   // jj -> (k, l): row k of the triangle starts at k (k + 1) / 2
          while (l > k) { l -= k + 1; ++k; }
          v = qf[(int64_t)k * n] * qf[(int64_t)l * n];
        } else {
          v = jj < T + p ? qf[(int64_t)(jj - T) * n] : invn != nullptr ? invn[f] : 0.0;
        }
      }
    }
    w[t] = v;
  }
  masks[(int64_t)tile * n + c] = bits;
}

// The block partials part[nblk][W][rows] of the W = nfit Wc weighted row sums, tile blockIdx.z.  row_design_effects_kernel's
// shape on the two-matrix walk of row_pair.h (kUn = 4; kWide: A and Wt 16-byte aligned) with the per-row factor chosen by the
// column's kind, which is wave-uniform: omega for a product column, y = omega * x (rounded once) for a column of Q, x for the mean's.
// kWt: the rows x n observation weights are there (same leading dimension as A); aw: the n array weights or null.
template <bool kWide, bool kWt>
__global__ void __launch_bounds__(256)
row_design_w_sums_kernel(const double* __restrict__ A, const double* __restrict__ Wt, const double* __restrict__ aw, int64_t ld,
                         int32_t rows, int32_t n, const uint32_t* __restrict__ masks, const double* __restrict__ wt, int32_t W,
                         int32_t p, double* __restrict__ part) {
  constexpr int T = kWTile;
  const RowPair g = row_pair_block(rows, n);
  const int r = g.r;
  const int j0 = blockIdx.z * T;
  const int nt = W - j0 < T ? W - j0 : T;
  const uint32_t* __restrict__ mk = masks + (int64_t)blockIdx.z * n;
  const double* __restrict__ wk = wt + (int64_t)blockIdx.z * n * T;
  if (r >= rows) return;
  const bool two = g.two;
  const int Wc = (int)w_cols(p), ntri = p * (p + 1) / 2;
  int kind[T];   // 0: a product column, 1: a column of Q, 2: the mean's (wave-uniform)
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int jj = (j0 + t) % Wc;
    kind[t] = jj < ntri ? 0 : jj < ntri + p ? 1 : 2;
  }
  double a[T], b[T];
#pragma unroll
  for (int t = 0; t < T; ++t) a[t] = b[t] = 0.0;
  const bool has_aw = aw != nullptr;
  auto accumulate = [&](int c, double xa, double xb, double wa, double wb) {
    const uint32_t k = mk[c];                         // wave-uniform, as the columns' entries
    const double* __restrict__ w = wk + (int64_t)c * T;
    const double awc = has_aw ? aw[c] : 1.0;
    const double oa = w_omega(kWt, wa, has_aw, awc), ob = w_omega(kWt, wb, has_aw, awc);
    const bool la = w_live(xa, oa), lb = w_live(xb, ob);
    const double ya = oa * xa, yb = ob * xb;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const bool in = ((k >> t) & 1u) != 0;
      const double wc = w[t];
      const double fa = kind[t] == 0 ? oa : kind[t] == 1 ? ya : xa;
      const double fb = kind[t] == 0 ? ob : kind[t] == 1 ? yb : xb;
      const bool ia = in && (kind[t] == 2 ? xa == xa : la), ib = in && (kind[t] == 2 ? xb == xb : lb);
      a[t] = ia ? __builtin_fma(fa, wc, a[t]) : a[t];
      b[t] = ib ? __builtin_fma(fb, wc, b[t]) : b[t];
    }
  };
  row_pair_walk2<kWide, 4, kWt>(A, Wt, ld, g, accumulate);
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (t >= nt) break;
    double* o = part + ((int64_t)blockIdx.y * W + (j0 + t)) * rows;
    o[r] = a[t];
    if (two) o[r + 1] = b[t];
  }
}

// The block partials part[nblk][2 nfit + 1][rows] of the counts, as doubles (exact integers, so that they take the road of the
// sums): column 2 f the live observations of fit f, 2 f + 1 the size of the mean's select "c in sel and x == x", and the last
// column the NaN of the row over ALL columns (max_na).  A thread owns a row and a block of 128 columns; kWFitTile fits share
// one read (blockIdx.z).  use: n x nfit or null.
template <bool kWt>
__global__ void __launch_bounds__(256)
lmfit_w_counts_kernel(const double* __restrict__ A, const double* __restrict__ Wt, const double* __restrict__ aw, int64_t ld,
                      int32_t rows, int32_t n, const int8_t* __restrict__ use, int32_t nfit, double* __restrict__ part) {
  constexpr int F = kWFitTile;
  const int r = blockIdx.x * 256 + threadIdx.x;
  const int c0 = blockIdx.y * kRowColBlock;
  const int c1 = c0 + kRowColBlock < n ? c0 + kRowColBlock : n;
  const int f0 = blockIdx.z * F;
  if (r >= rows) return;
  const bool has_aw = aw != nullptr;
  int32_t live[F], seen[F], nans = 0;
#pragma unroll
  for (int t = 0; t < F; ++t) live[t] = seen[t] = 0;
  for (int c = c0; c < c1; ++c) {
    const double x = __builtin_nontemporal_load(A + (int64_t)c * ld + r);
    const double wv = kWt ? __builtin_nontemporal_load(Wt + (int64_t)c * ld + r) : 1.0;
    const double om = w_omega(kWt, wv, has_aw, has_aw ? aw[c] : 1.0);
    const bool obs = x == x, lv = w_live(x, om);
    nans += obs ? 0 : 1;
#pragma unroll
    for (int t = 0; t < F; ++t) {
      const int f = f0 + t;
      const bool in = f < nfit && (use == nullptr || use[(int64_t)f * n + c] != 0);   // wave-uniform
      live[t] += in && lv ? 1 : 0;
      seen[t] += in && obs ? 1 : 0;
    }
  }
  const int64_t C = 2 * (int64_t)nfit + 1;
  double* o = part + (int64_t)blockIdx.y * C * rows + r;
#pragma unroll
  for (int t = 0; t < F; ++t) {
    const int f = f0 + t;
    if (f < nfit) {
      o[(int64_t)(2 * f) * rows] = (double)live[t];
      o[(int64_t)(2 * f + 1) * rows] = (double)seen[t];
    }
  }
  if (blockIdx.z == 0) o[(C - 1) * rows] = (double)nans;
}

// The solve of every (row, fit): a thread per pair, its H (p x p, leading dimension kWP), g and the scratch of u_j in a slice
// of LDS of its own, kWSlice doubles (odd, so that the lanes of a wavefront fall on different banks); the arithmetic is
// lmfit_w_row_solve (lmfit_na.h), the host's copy.  S: the reduced sums [nfit Wc][rows]; cnt: the reduced counts
// [2 nfit + 1][rows].  Writes G [nfit (p + 1)][rows] (gamma, then AveExpr = (M' n_f) / |seen|), drow [nfit][rows] (d_r = |live|
// - p) and urow [nfit q][rows]; NaN in all of them for a pair that is not estimable or whose row is above max_na.
// 64 threads: 64 * 121 * 8 = 61,952 bytes of LDS.
constexpr int kWSlice = kWP * kWP + 2 * kWP + 1;
__global__ void __launch_bounds__(64)
lmfit_w_solve_kernel(const double* __restrict__ S, const double* __restrict__ cnt, const double* __restrict__ v,
                     const double* __restrict__ nf, int32_t rows, int32_t n, int32_t p, int32_t nfit, int32_t q, double max_na,
                     double* __restrict__ G, double* __restrict__ drow, double* __restrict__ urow) {
  __shared__ double lds[64 * kWSlice];
  const int r = blockIdx.x * 64 + threadIdx.x;
  const int f = blockIdx.y;
  if (r >= rows) return;
  double* H = lds + threadIdx.x * kWSlice;
  double* g = H + kWP * kWP;
  double* w = g + kWP;
  const int64_t Wc = w_cols(p);
  const int T = p * (p + 1) / 2;
  const double* s = S + (int64_t)f * Wc * rows + r;
  for (int k = 0, j = 0; k < p; ++k)
    for (int l = 0; l <= k; ++l, ++j) H[k * kWP + l] = s[(int64_t)j * rows];
  for (int k = 0; k < p; ++k) g[k] = s[(int64_t)(T + k) * rows];
  const double Mp = s[(int64_t)(T + p) * rows];
  const double nlive = cnt[(int64_t)(2 * f) * rows + r], nseen = cnt[(int64_t)(2 * f + 1) * rows + r];
  const double nans = cnt[(int64_t)(2 * nfit) * rows + r];
  const bool fitted = nans / (double)n <= max_na;   // rowMeans(is.na(X)) <= max.na
  double* u = urow + (int64_t)f * q * rows + r;
  const bool ok = fitted && lmfit_w_row_solve(p, H, kWP, g, nlive, v + (int64_t)f * q * p, q, u, rows, w, nullptr);
  const double nan = __builtin_nan("");
  double* o = G + (int64_t)f * (p + 1) * rows + r;
  for (int k = 0; k < p; ++k) o[(int64_t)k * rows] = ok ? g[k] : nan;
  o[(int64_t)p * rows] = ok ? lmfit_na_mean(Mp, nf[f], nseen) : nan;
  drow[(int64_t)f * rows + r] = ok ? nlive - (double)p : nan;
  if (!ok)
    for (int j = 0; j < q; ++j) u[(int64_t)j * rows] = nan;
}

// The block partials part[nblk][nfit][rows] of the weighted residual sums of squares of fit blockIdx.z at gamma (G:
// [nfit (p + 1)][rows]): row_design_rss_kernel with omega and the live select,
//     r = x - sum_k Q[c, k] gamma_k (p chained fma from x),   RSS = live ? fma(omega, r * r, .) : unchanged (r * r rounded first).
template <int kP, bool kWide, bool kWt>
__global__ void __launch_bounds__(256)
row_design_w_rss_kernel(const double* __restrict__ A, const double* __restrict__ Wt, const double* __restrict__ aw, int64_t ld,
                        int32_t rows, int32_t n, const double* __restrict__ Q, const uint32_t* __restrict__ masks, int32_t p,
                        int32_t nfit, const double* __restrict__ G, double* __restrict__ part) {
  const RowPair g = row_pair_block(rows, n);
  const int r = g.r, f = blockIdx.z;
  const int64_t Wc = w_cols(p);
  const RowPairFitBit used = row_pair_fit_bit(masks, (int64_t)f * Wc + Wc - 1, n);   // the fit's mean column
  const double* __restrict__ Qf = Q + (int64_t)f * p * n;
  if (r >= rows) return;
  const bool has_aw = aw != nullptr;
  double ea[kP], eb[kP];
  row_pair_effects<kP>(G, f, p, rows, g, ea, eb);
  double sa = 0.0, sb = 0.0;
  auto accumulate = [&](int c, double xa, double xb, double wa, double wb) {
    const bool in = used(c);
    const double awc = has_aw ? aw[c] : 1.0;
    const double oa = w_omega(kWt, wa, has_aw, awc), ob = w_omega(kWt, wb, has_aw, awc);
    double ra = xa, rb = xb;
    row_pair_chain<kP>(Qf, n, c, p, ea, eb, ra, rb);
    const double qa = ra * ra, qb = rb * rb;
    sa = in && w_live(xa, oa) ? __builtin_fma(oa, qa, sa) : sa;
    sb = in && w_live(xb, ob) ? __builtin_fma(ob, qb, sb) : sb;
  };
  row_pair_walk2<kWide, 4, kWt>(A, Wt, ld, g, accumulate);
  double* o = part + ((int64_t)blockIdx.y * nfit + f) * rows;
  o[r] = sa;
  if (g.two) o[r + 1] = sb;
}

// ---- the launchers (common.h) -------------------------------------------------------------------------------------------------
int64_t lmfit_w_columns(int32_t p) { return w_cols(p); }

int launch_lmfit_w_table(plaidhip_ctx* ctx, const double* d_Q, const int8_t* d_use, const double* d_invn, int32_t n, int32_t p,
                         int32_t nfit, void* d_masks, double* d_wt) {
  if (n == 0 || nfit == 0) return PLAIDHIP_OK;
  const int64_t tiles = lmfit_tiles((int64_t)nfit * w_cols(p));
  PH_REQUIRE(p >= 1 && p <= kWP && tiles <= 65535, "limma_w: p = %d, %lld tiles of weight columns (at most 65535)", p,
             (long long)tiles);
  hipLaunchKernelGGL(lmfit_w_table_kernel, dim3((n + 255) / 256, (unsigned)tiles), dim3(256), 0, ctx->stream, d_Q, d_use, d_invn,
                     n, p, nfit, static_cast<uint32_t*>(d_masks), d_wt);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// ws: row_design_ws_doubles(rows, n, W) doubles, [nblk][W][rows], W = nfit lmfit_w_columns(p); d_masks / d_wt:
// launch_lmfit_w_table of the same n.  d_Wt: rows x n with A's leading dimension, or null; d_aw: n, or null.
int launch_row_design_w_sums(plaidhip_ctx* ctx, const double* A, const double* d_Wt, const double* d_aw, int64_t ld, int32_t rows,
                             int32_t n, const void* d_masks, const double* d_wt, int32_t p, int32_t nfit, double* ws) {
  if (rows == 0 || n == 0 || nfit == 0) return PLAIDHIP_OK;
  const int64_t W = (int64_t)nfit * w_cols(p), tiles = lmfit_tiles(W);
  PH_REQUIRE(p >= 1 && p <= kWP && tiles <= 65535 && W <= 2147483647, "limma_w: p = %d, %lld tiles of weight columns", p,
             (long long)tiles);
  const int nblk = (n + kRowColBlock - 1) / kRowColBlock;
  const dim3 grid((rows + 511) / 512, nblk, (unsigned)tiles);
  const uint32_t* mk = static_cast<const uint32_t*>(d_masks);
  dispatch_flag(row_pair_wide(rows, {ld}, {A, d_Wt}), [&](auto wide) {
    dispatch_flag(d_Wt != nullptr, [&](auto has) {
      hipLaunchKernelGGL((row_design_w_sums_kernel<decltype(wide)::value, decltype(has)::value>), grid, dim3(256), 0, ctx->stream, A,
                         d_Wt, d_aw, ld, rows, n, mk, d_wt, (int32_t)W, p, ws);
    });
  });
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// ws: row_design_ws_doubles(rows, n, 2 nfit + 1) doubles, [nblk][2 nfit + 1][rows]
int launch_lmfit_w_counts(plaidhip_ctx* ctx, const double* A, const double* d_Wt, const double* d_aw, int64_t ld, int32_t rows,
                          int32_t n, const int8_t* d_use, int32_t nfit, double* ws) {
  if (rows == 0 || n == 0 || nfit == 0) return PLAIDHIP_OK;
  const int nblk = (n + kRowColBlock - 1) / kRowColBlock;
  const dim3 grid((rows + 255) / 256, nblk, (nfit + kWFitTile - 1) / kWFitTile);
  if (d_Wt != nullptr)
    hipLaunchKernelGGL((lmfit_w_counts_kernel<true>), grid, dim3(256), 0, ctx->stream, A, d_Wt, d_aw, ld, rows, n, d_use, nfit, ws);
  else
    hipLaunchKernelGGL((lmfit_w_counts_kernel<false>), grid, dim3(256), 0, ctx->stream, A, d_Wt, d_aw, ld, rows, n, d_use, nfit, ws);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// d_S: [nfit Wc][rows], d_cnt: [2 nfit + 1][rows], d_v: p x q x nfit, d_nf: nfit doubles; d_G: [nfit (p + 1)][rows], d_drow:
// [nfit][rows], d_urow: [nfit q][rows]
int launch_lmfit_w_solve(plaidhip_ctx* ctx, const double* d_S, const double* d_cnt, const double* d_v, const double* d_nf,
                         int32_t rows, int32_t n, int32_t p, int32_t nfit, int32_t q, double max_na, double* d_G, double* d_drow,
                         double* d_urow) {
  if (rows == 0 || nfit == 0) return PLAIDHIP_OK;
  PH_REQUIRE(p >= 1 && p <= kWP && nfit <= 65535, "limma_w: p = %d, nfit = %d", p, nfit);
  hipLaunchKernelGGL(lmfit_w_solve_kernel, dim3((rows + 63) / 64, nfit), dim3(64), 0, ctx->stream, d_S, d_cnt, d_v, d_nf, rows, n,
                     p, nfit, q, max_na, d_G, d_drow, d_urow);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// ws: row_design_ws_doubles(rows, n, nfit) doubles, [nblk][nfit][rows]; d_G: [nfit (p + 1)][rows], gamma of every pair
int launch_row_design_w_rss(plaidhip_ctx* ctx, const double* A, const double* d_Wt, const double* d_aw, int64_t ld, int32_t rows,
                            int32_t n, const double* d_Q, const void* d_masks, int32_t p, int32_t nfit, const double* d_G,
                            double* ws) {
  if (rows == 0 || n == 0 || nfit == 0) return PLAIDHIP_OK;
  PH_REQUIRE(p >= 1 && p <= kWP && nfit <= 65535, "limma_w: p = %d, nfit = %d", p, nfit);
  const int nblk = (n + kRowColBlock - 1) / kRowColBlock;
  const dim3 grid((rows + 511) / 512, nblk, nfit);
  const uint32_t* mk = static_cast<const uint32_t*>(d_masks);
  dispatch_p<kWP>(p, [&](auto kp) {   // (4, 8 and kWP effects)
    dispatch_flag(row_pair_wide(rows, {ld}, {A, d_Wt}), [&](auto wide) {
      dispatch_flag(d_Wt != nullptr, [&](auto has) {
        hipLaunchKernelGGL((row_design_w_rss_kernel<decltype(kp)::value, decltype(wide)::value, decltype(has)::value>), grid,
                           dim3(256), 0, ctx->stream, A, d_Wt, d_aw, ld, rows, n, d_Q, mk, p, nfit, d_G, ws);
      });
    });
  });
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
