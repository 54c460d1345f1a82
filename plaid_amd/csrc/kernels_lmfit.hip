// plaid.limma: the per-row linear-model fit of include/plaidhip.h (plaidhip_limma), two passes over a rows x n matrix.
//
// kernels_contrasts.hip generalised from 0 / 1 labels to real weights.  A fit f is the thin Q_f of its design (n x p, made on
// the host) and its used samples; what a row needs of it are the effects E_k = sum_c x_c Q_f[c, k], the mean M (one more
// weight column, use / n_f) and then the residual sum of squares at the reduced effects.  The W = nfit (p + 1) weight
// columns of all fits lie side by side (fit f: columns f (p + 1) + 0 .. p - 1 are Q_f's, column f (p + 1) + p is the mean's)
// and are cut into tiles of kTile; the weights of a column of A and the bits "this sample is used by the fit that owns tile
// column t" are the same for every row -- wavefront-uniform, read through scalar loads.  A thread owns two adjacent rows,
// walks a block of kRowColBlock columns in ascending order (the walk of row_pair.h) and keeps the tile's accumulators in
// registers, so A is read ceil(W / kTile) times for the effects and nfit times for the residuals.  As in kernels_contrasts.hip:
//     acc = in ? fma(x, w, acc) : acc          per column of the block, ascending (RSS: acc += in ? r * r : 0.0)
//     part[block][column][row]
//     blocks added in ascending order, from an optional seed (reduce_blocks_flat_kernel)
// The select form matters: an excluded column leaves the accumulator alone whatever it holds (NaN, Inf).  The file is
// compiled with -ffp-contract=off (and says so below): the only fused operations are the fma written out.
#include "common.h"
#include "lmfit_na.h"
#include "row_pair.h"

#pragma clang fp contract(off)

namespace plaidhip {

constexpr int kLmTile = PLAIDHIP_LIMMA_TILE;

// masks[tile][c]: bit t = sample c is used by the fit of column tile * kTile + t (an 8-bit mask, kept in a 32-bit word so
// that it is one scalar load); wt[tile][c][t]: that column's weight for the sample -- Q_f[c, k], 1 / n_f for the mean's
// column, 0.0 for an excluded sample and past column W.  Q: n x p x nfit, use: n x nfit or null, invn: nfit.  wt == nullptr:
// the masks alone (the RSS pass reads no weight), and Q and invn are not read.
__global__ void __launch_bounds__(256)
lmfit_masks_kernel(const double* __restrict__ Q, const int8_t* __restrict__ use, const double* __restrict__ invn, int32_t n,
                   int32_t p, int32_t nfit, uint32_t* __restrict__ masks, double* __restrict__ wt) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int tile = blockIdx.y;
  if (c >= n) return;
  const int64_t W = (int64_t)nfit * (p + 1);
  uint32_t bits = 0;
  double* w = wt != nullptr ? wt + ((int64_t)tile * n + c) * kLmTile : nullptr;
  for (int t = 0; t < kLmTile; ++t) {
    const int64_t j = (int64_t)tile * kLmTile + t;
    double v = 0.0;
    if (j < W) {
      const int64_t f = j / (p + 1);
      const int k = (int)(j % (p + 1));
      if (use == nullptr || use[f * n + c] != 0) {
        bits |= 1u << t;
        if (w != nullptr) v = k < p ? Q[(f * p + k) * n + c] : invn[f];
      }
    }
    if (w != nullptr) w[t] = v;
  }
  masks[(int64_t)tile * n + c] = bits;
}

// The block partials part[nblk][W][rows] of the W weighted row sums, tile blockIdx.z: the geometry and the load of row_pair.h
// with the loop of row_pair_walk (kUn = 8) written out in the kernel, where it compiles to the code it had before the header.
// kNa (na = "fit"): a NaN takes no part either -- the select is "c in sel and x_c == x_c", per row.
template <bool kWide, bool kNa>
__global__ void __launch_bounds__(256)
row_design_effects_kernel(const double* __restrict__ A, int64_t ld, int32_t rows, int32_t n, const uint32_t* __restrict__ masks,
                          const double* __restrict__ wt, int32_t W, double* __restrict__ part) {
  constexpr int T = kLmTile;
  const RowPair g = row_pair_block(rows, n);
  const int r = g.r;
  const int j0 = blockIdx.z * T;                      // the tile's first column
  const int nt = W - j0 < T ? W - j0 : T;             // its live columns (the others' bits are 0, nothing is written)
  const uint32_t* __restrict__ mk = masks + (int64_t)blockIdx.z * n;
  const double* __restrict__ wk = wt + (int64_t)blockIdx.z * n * T;
  if (r >= rows) return;
  const bool two = g.two;
  double a[T], b[T];
#pragma unroll
  for (int t = 0; t < T; ++t) a[t] = b[t] = 0.0;
  auto accumulate = [&](int c, double xa, double xb) {
    const uint32_t k = mk[c];                         // wave-uniform, as the weights
    const double* __restrict__ w = wk + (int64_t)c * T;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const bool in = ((k >> t) & 1u) != 0;
      const double wc = w[t];
      const bool ia = kNa ? (in && xa == xa) : in, ib = kNa ? (in && xb == xb) : in;
      a[t] = ia ? __builtin_fma(xa, wc, a[t]) : a[t];
      b[t] = ib ? __builtin_fma(xb, wc, b[t]) : b[t];
    }
  };
  // row_pair_walk<kWide, 8>(A, ld, g, accumulate), written out
  constexpr int kUn = 8;
  int c = g.c0;
  for (; c + kUn <= g.c1; c += kUn) {
    double xa[kUn], xb[kUn];
#pragma unroll
    for (int u = 0; u < kUn; ++u) row_pair_load<kWide, true>(A + (int64_t)(c + u) * ld + r, two, xa[u], xb[u]);
#pragma unroll
    for (int u = 0; u < kUn; ++u) accumulate(c + u, xa[u], xb[u]);
  }
  for (; c < g.c1; ++c) {
    double xa, xb;
    row_pair_load<kWide, true>(A + (int64_t)c * ld + r, two, xa, xb);
    accumulate(c, xa, xb);
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (t >= nt) break;
    double* o = part + ((int64_t)blockIdx.y * W + (j0 + t)) * rows;
    o[r] = a[t];
    if (two) o[r + 1] = b[t];
  }
}

// The block partials part[nblk][nfit][rows] of the residual sums of squares of fit blockIdx.z at the reduced effects E
// ([W][rows]): r = x - sum_k Q[c, k] E_k as p chained fma in ascending k, starting from x; the sum takes in ? r * r : 0.0.
// A thread keeps its two rows' p effects in registers (kP: p rounded up to 4, 8, 16 or 32; DESIGN.md section 20 has the
// resource report that chose registers over an LDS tile).  Q's entries of a column are wave-uniform.
// kNa: the select extended by x_c == x_c, as in the effects.
template <int kP, bool kWide, bool kNa>
__global__ void __launch_bounds__(256)
row_design_rss_kernel(const double* __restrict__ A, int64_t ld, int32_t rows, int32_t n, const double* __restrict__ Q,
                      const uint32_t* __restrict__ masks, int32_t p, int32_t nfit, const double* __restrict__ E,
                      double* __restrict__ part) {
  const RowPair g = row_pair_block(rows, n);
  const int r = g.r, f = blockIdx.z;
  const RowPairFitBit used = row_pair_fit_bit(masks, (int64_t)f * (p + 1) + p, n);   // the fit's mean column
  const double* __restrict__ Qf = Q + (int64_t)f * p * n;
  if (r >= rows) return;
  double ea[kP], eb[kP];
  row_pair_effects<kP>(E, f, p, rows, g, ea, eb);
  double sa = 0.0, sb = 0.0;
  auto accumulate = [&](int c, double xa, double xb) {
    const bool in = used(c);
    double ra = xa, rb = xb;
    row_pair_chain<kP>(Qf, n, c, p, ea, eb, ra, rb);
    const double qa = ra * ra, qb = rb * rb;
    sa += (kNa ? (in && xa == xa) : in) ? qa : 0.0;
    sb += (kNa ? (in && xb == xb) : in) ? qb : 0.0;
  };
  row_pair_walk<kWide, 8>(A, ld, g, accumulate);
  double* o = part + ((int64_t)blockIdx.y * nfit + f) * rows;
  o[r] = sa;
  if (g.two) o[r + 1] = sb;
}

// ---- na = "fit" (include/plaidhip.h: plaidhip_limma_na) ---------------------------------------------------
constexpr int kNaP = PLAIDHIP_LIMMA_NA_MAX_COEF;
static_assert(kNaP >= 8 && kNaP * (kNaP + 1) / 2 <= 64, "the lower triangle of H is one wavefront's lanes");

// The count pass.  A thread owns one row and one block of 128 columns (blockIdx.y), so a column's loads are coalesced, the
// grid fills the device as the effects kernel's does, and a row's NaN come out in ascending column order with no atomic:
// within a block the thread walks ascending, and the blocks of a row are laid out one after the other by the prefix sums.
// off == nullptr: cnt[b][r] = the NaN of row r in block b.  Otherwise the second sweep: list[off[b][r] ..] = their column
// indices (off: the exclusive prefix sums of cnt taken row by row, block by block within a row).
__global__ void __launch_bounds__(256)
lmfit_nan_rows_kernel(const double* __restrict__ A, int64_t ld, int32_t rows, int32_t n, const int64_t* __restrict__ off,
                      int32_t* __restrict__ cnt, int32_t* __restrict__ list) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  const int c0 = blockIdx.y * kRowColBlock;
  const int c1 = c0 + kRowColBlock < n ? c0 + kRowColBlock : n;
  if (r >= rows) return;
  const int64_t slot = (int64_t)blockIdx.y * rows + r;
  int32_t k = 0;
  int32_t* o = off != nullptr ? list + off[slot] : nullptr;
  for (int c = c0; c < c1; ++c) {
    const double x = __builtin_nontemporal_load(A + (int64_t)c * ld + r);
    if (x != x) {
      if (o != nullptr) o[k] = c;
      ++k;
    }
  }
  if (off == nullptr) cnt[slot] = k;
}

// cnt[f][r] = the NaN of row r inside the used samples of fit f = blockIdx.y, from the row's list (use: n x nfit or null)
__global__ void __launch_bounds__(256)
lmfit_nan_pairs_kernel(const int64_t* __restrict__ off, const int32_t* __restrict__ list, const int8_t* __restrict__ use,
                       int32_t rows, int32_t n, int32_t* __restrict__ cnt) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  const int f = blockIdx.y;
  if (r >= rows) return;
  int32_t k = 0;
  for (int64_t i = off[r]; i < off[r + 1]; ++i) k += use == nullptr || use[(int64_t)f * n + list[i]] != 0 ? 1 : 0;
  cnt[(int64_t)f * rows + r] = k;
}

// Gram and solve: one wavefront per incomplete (row, fit) pair of the work list (pairs[2 i], pairs[2 i + 1]).  Lane t < p (p +
// 1) / 2 owns the entry (k, l <= k) of H and runs its chain over the pair's missing samples -- the row's list, ascending,
// without the samples the fit left out (a wave-uniform test); the sample's row of Q_f goes through LDS once for all lanes.
// Then the shared solve (lmfit_na.h) on lane 0, and the contrasts' u_j dealt to the lanes.  E ([W][rows]) holds E' and M'
// of the pair on entry, gamma and the mean over the observed samples on return; a pair that is not estimable gets NaN.
// LDS: 120 doubles and a flag, 968 bytes.
__global__ void __launch_bounds__(64)
lmfit_na_solve_kernel(const int32_t* __restrict__ pairs, const int64_t* __restrict__ off, const int32_t* __restrict__ list,
                      const double* __restrict__ Q, const int8_t* __restrict__ use, int32_t n, int32_t p, int32_t q,
                      const double* __restrict__ v, const int32_t* __restrict__ nobs, const double* __restrict__ nf,
                      int32_t rows, double* __restrict__ E, double* __restrict__ upair, int32_t* __restrict__ okpair) {
  __shared__ double qrow[kNaP];
  __shared__ double H[kNaP * kNaP];
  __shared__ double gam[kNaP];
  __shared__ int ok;
  const int lane = threadIdx.x;
  const int r = pairs[2 * (int64_t)blockIdx.x], f = pairs[2 * (int64_t)blockIdx.x + 1];
  const double* __restrict__ Qf = Q + (int64_t)f * p * n;
  const int8_t* __restrict__ uf = use != nullptr ? use + (int64_t)f * n : nullptr;
  int k = 0, l = lane;   // lane -> (k, l): row k of the triangle starts at k (k + 1) / 2
  while (l > k) { l -= k + 1; ++k; }
  const bool mine = k < p;
  double s = 0.0;
  for (int64_t i = off[r]; i < off[r + 1]; ++i) {
    const int c = list[i];
    if (uf != nullptr && uf[c] == 0) continue;
    __syncthreads();
    if (lane < p) qrow[lane] = Qf[(int64_t)lane * n + c];
    __syncthreads();
    if (mine) s = lmfit_na_gram_step(qrow[k], qrow[l], s);
  }
  if (mine) H[k * kNaP + l] = (k == l ? 1.0 : 0.0) - s;
  double* e = E + (int64_t)f * (p + 1) * rows + r;
  __syncthreads();
  if (lane == 0) {
    double ep[kNaP];
    for (int t = 0; t < p; ++t) ep[t] = e[(int64_t)t * rows];
    ok = lmfit_na_factor_solve(p, H, kNaP, ep, gam, nullptr, PLAIDHIP_LMNA_PIVOT_MIN, false) ? 1 : 0;
    const double nan = __builtin_nan("");
    for (int t = 0; t < p; ++t) e[(int64_t)t * rows] = ok ? gam[t] : nan;
    e[(int64_t)p * rows] = ok ? lmfit_na_mean(e[(int64_t)p * rows], nf[f], (double)nobs[blockIdx.x]) : nan;
    okpair[blockIdx.x] = ok;
  }
  __syncthreads();
  for (int j = lane; j < q; j += 64) {
    double w[kNaP];
    upair[(int64_t)blockIdx.x * q + j] =
        ok ? lmfit_na_unscaled(p, H, kNaP, v + ((int64_t)f * q + j) * p, w) : __builtin_nan("");
  }
}

int launch_lmfit_nan_rows(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const int64_t* d_off,
                          int32_t* d_cnt, int32_t* d_list) {
  if (rows == 0 || n == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(lmfit_nan_rows_kernel, dim3((rows + 255) / 256, (n + kRowColBlock - 1) / kRowColBlock), dim3(256), 0,
                     ctx->stream, A, ld, rows, n, d_off, d_cnt, d_list);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_lmfit_nan_pairs(plaidhip_ctx* ctx, const int64_t* d_off, const int32_t* d_list, const int8_t* d_use, int32_t rows,
                           int32_t n, int32_t nfit, int32_t* d_cnt) {
  if (rows == 0 || nfit == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(lmfit_nan_pairs_kernel, dim3((rows + 255) / 256, nfit), dim3(256), 0, ctx->stream, d_off, d_list, d_use,
                     rows, n, d_cnt);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// npairs work items; d_E: [nfit (p + 1)][rows], changed in place; d_u: npairs x q; d_ok: npairs
int launch_lmfit_na_solve(plaidhip_ctx* ctx, int64_t npairs, const int32_t* d_pairs, const int64_t* d_off, const int32_t* d_list,
                          const double* d_Q, const int8_t* d_use, int32_t n, int32_t p, int32_t q, const double* d_v,
                          const int32_t* d_nobs, const double* d_nf, int32_t rows, double* d_E, double* d_u, int32_t* d_ok) {
  if (npairs == 0) return PLAIDHIP_OK;
  PH_REQUIRE(p >= 1 && p <= kNaP && npairs <= 2147483647, "limma_na: p = %d, %lld pairs", p, (long long)npairs);
  hipLaunchKernelGGL(lmfit_na_solve_kernel, dim3((unsigned)npairs), dim3(64), 0, ctx->stream, d_pairs, d_off, d_list, d_Q, d_use,
                     n, p, q, d_v, d_nobs, d_nf, rows, d_E, d_u, d_ok);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int64_t lmfit_tiles(int64_t W) { return (W + kLmTile - 1) / kLmTile; }

// doubles of the block partials [nblk][cols][rows]
int64_t row_design_ws_doubles(int32_t rows, int32_t n, int64_t cols) {
  const int64_t nblk = (n + kRowColBlock - 1) / kRowColBlock;
  return (int64_t)rows * cols * (nblk > 0 ? nblk : 1);
}

// bytes of the masks of n columns and W weight columns, and of their weights (a multiple of 16 each)
int64_t lmfit_mask_bytes(int32_t n, int64_t W) { return (lmfit_tiles(W) * (int64_t)(n > 0 ? n : 1) * 4 + 15) / 16 * 16; }
int64_t lmfit_weight_bytes(int32_t n, int64_t W) { return lmfit_tiles(W) * (int64_t)(n > 0 ? n : 1) * kLmTile * 8; }

int launch_lmfit_masks(plaidhip_ctx* ctx, const double* d_Q, const int8_t* d_use, const double* d_invn, int32_t n, int32_t p,
                       int32_t nfit, void* d_masks, double* d_wt) {
  if (n == 0 || nfit == 0) return PLAIDHIP_OK;
  const int64_t W = (int64_t)nfit * (p + 1);
  hipLaunchKernelGGL(lmfit_masks_kernel, dim3((n + 255) / 256, (unsigned)lmfit_tiles(W)), dim3(256), 0, ctx->stream, d_Q, d_use,
                     d_invn, n, p, nfit, static_cast<uint32_t*>(d_masks), d_wt);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// ws: row_design_ws_doubles(rows, n, W) doubles, [nblk][W][rows]; d_masks / d_wt: launch_lmfit_masks of the same n and W
int launch_row_design_effects(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const void* d_masks,
                              const double* d_wt, int32_t W, double* ws, bool na) {
  if (rows == 0 || n == 0 || W == 0) return PLAIDHIP_OK;
  const int nblk = (n + kRowColBlock - 1) / kRowColBlock;
  const dim3 grid((rows + 511) / 512, nblk, (unsigned)lmfit_tiles(W));
  const uint32_t* mk = static_cast<const uint32_t*>(d_masks);
  dispatch_flag(row_pair_wide(rows, {ld}, {A}), [&](auto wide) {
    dispatch_flag(na, [&](auto kna) {
      hipLaunchKernelGGL((row_design_effects_kernel<decltype(wide)::value, decltype(kna)::value>), grid, dim3(256), 0, ctx->stream,
                         A, ld, rows, n, mk, d_wt, W, ws);
    });
  });
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

// ws: row_design_ws_doubles(rows, n, nfit) doubles, [nblk][nfit][rows]; d_E: [nfit (p + 1)][rows], the effects of all samples
int launch_row_design_rss(plaidhip_ctx* ctx, const double* A, int64_t ld, int32_t rows, int32_t n, const double* d_Q,
                          const void* d_masks, int32_t p, int32_t nfit, const double* d_E, double* ws, bool na) {
  if (rows == 0 || n == 0 || nfit == 0) return PLAIDHIP_OK;
  const int nblk = (n + kRowColBlock - 1) / kRowColBlock;
  const dim3 grid((rows + 511) / 512, nblk, nfit);
  const uint32_t* mk = static_cast<const uint32_t*>(d_masks);
  const bool wide = row_pair_wide(rows, {ld}, {A});
  auto launch = [&](auto kp, auto kna) {
    dispatch_flag(wide, [&](auto w) {
      hipLaunchKernelGGL((row_design_rss_kernel<decltype(kp)::value, decltype(w)::value, decltype(kna)::value>), grid, dim3(256), 0,
                         ctx->stream, A, ld, rows, n, d_Q, mk, p, nfit, d_E, ws);
    });
  };
  if (na) dispatch_p<16>(p, [&](auto kp) { launch(kp, std::true_type{}); });   // (p <= PLAIDHIP_LIMMA_NA_MAX_COEF)
  else dispatch_p(p, [&](auto kp) { launch(kp, std::false_type{}); });
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
