// replaid.ssgsea.exact(single = FALSE): the running sum's value of largest magnitude (the classic GSEA enrichment score,
// gao.ssgsea's second branch).  An extremum over a walk is not a sum, so no crossprod gives it: this file holds the walk's
// two kernels (the walk itself, which plaid.gsea and the dispersion kernel share: bitmap_walk.h).
//
// Per sample column with N genes (the statistic is pinned in include/plaidhip.h): q = last ranks,
// w = r^alpha, the walk visits the genes at pos = N + 1 - q.  With a set's k members sorted by pos (t = 1..k):
//     cw_t = w_1 + ... + w_t,  B = cw_k,  miss_t = (pos_t - t) / (N - k)
//     after_t = cw_t / B - miss_t,  before_t = cw_{t-1} / B - miss_t  (pos_t >= 2),  each / N with scale
// and the score is the candidate of largest |.|, the earliest one among equals, 0 when none exceeds 0.
//
// ONE route for every k in 0..N -- a bitmap walk, no sort.  The q of a column are distinct integers in 1..N, so one
// wavefront per (set, column) pair sets bit pos - 1 of an N-bit map in LDS for every member and scans the 64-bit words in
// order: the wavefront prefix sum of the popcounts gives t of every set bit, the bit's index gives pos.  At alpha = 0 that
// is the whole computation.  Otherwise w is found by position in Wpos, the column's weights scattered into walk order once
// per column (gsea_ks_scatter_kernel; all m sets share it), B is the sum of the members' w (lane partials, butterfly) and
// cw_t a wavefront prefix sum over the lanes' words.  Cost per pair: k + N / 64 LDS words, whatever the set size.
// The map bounds N: PLAIDHIP_GSEA_KS_MAX_GENES (four wavefronts' maps in 64 KB of LDS).
#include <algorithm>

#include "bitmap_walk.h"

namespace plaidhip {

namespace {

constexpr int kKsWaves = 4;       // wavefronts per workgroup, one (set, column) pair each at a time
constexpr int kKsColTile = 16;    // sample columns a workgroup scores for one set before it moves to the next set

// walk order of a column's weights: Wpos[pos - 1] = w of the gene at position pos.  A column holding a NaN is skipped
// (its q are no permutation; the walk kernel never reads its Wpos); a q outside 1..N is never followed.
__global__ void __launch_bounds__(256)
gsea_ks_scatter_kernel(const double* __restrict__ Q, const double* __restrict__ W, int64_t ldq, const uint32_t* __restrict__ colnan,
                       int32_t N, int32_t n, double* __restrict__ Wpos) {
  for (int c = blockIdx.y; c < n; c += gridDim.y) {
    if (colnan[c]) continue;
    const int64_t b0 = (int64_t)c * ldq;
    for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
      const int32_t b = N - (int32_t)Q[b0 + i];
      if ((uint32_t)b < (uint32_t)N) Wpos[b0 + b] = W[b0 + i];
    }
  }
}

// The tasks of the two walk kernels.  One wavefront per (set j, column c): a workgroup takes a set and a tile of kKsColTile
// columns (tasks ordered set-first, so the workgroups in flight share the tile's Q columns in L2) and calls
// pair(bm, lane, p0, k, c, out) for each of them, c uniform in the wavefront; a pair with an empty or full set or a NaN column is
// NaN and never reaches it.  The wavefront's map (nw64 words, bitmap_walk.h) is all zero on the way in and has to be on the
// way out.
template <typename Pair>
__device__ __forceinline__ void ks_for_each_pair(const uint32_t* __restrict__ colnan, int32_t N, int32_t n,
                                                 const int32_t* __restrict__ Gp, int32_t m, double* __restrict__ S, int64_t lds,
                                                 int32_t nw64, Pair pair) {
  extern __shared__ unsigned long long ks_map[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long* bm = ks_map + (size_t)wave * nw64;
  walk_zero_map(bm, nw64, lane);
  walk_wave_sync();
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int64_t tiles = ((int64_t)n + kKsColTile - 1) / kKsColTile;
  const int64_t tasks = tiles * m;
  for (int64_t task = blockIdx.x; task < tasks; task += gridDim.x) {
    const int64_t tile = task / m;
    const int32_t j = (int32_t)(task - tile * m);
    const int32_t p0 = Gp[j], k = Gp[j + 1] - p0;
    const int32_t c1 = (int32_t)std::min<int64_t>(n, (tile + 1) * kKsColTile);
    for (int32_t c = (int32_t)(tile * kKsColTile) + wave; c < c1; c += kKsWaves) {   // (c is uniform in the wavefront)
      double* out = S + (int64_t)c * lds + j;
      if (k <= 0 || k >= N || colnan[c] != 0u) {
        if (lane == 0) *out = nan;
        continue;
      }
      pair(bm, lane, p0, k, c, out);
      walk_wave_sync();   // the cleared words before the next pair's bits
    }
  }
}

// gsea.ssgsea's second branch.  B is the sum of the members' w in list order (lane partials, butterfly); the candidates of
// a hit are before_t (pos >= 2) and after_t, each / N with scale; the score is the one of largest |.|, the earliest among
// equals (its place in the visiting order: 2 pos - 1 before, 2 pos after).
template <bool WEIGHTED>
__global__ void __launch_bounds__(64 * kKsWaves)
gsea_ks_kernel(const double* __restrict__ Q, const double* __restrict__ W, const double* __restrict__ Wpos, int64_t ldq,
               const uint32_t* __restrict__ colnan, int32_t N, int32_t n, const int32_t* __restrict__ Gp,
               const int32_t* __restrict__ Gi, int32_t m, int scale, double* __restrict__ S, int64_t lds, int32_t nw64) {
  const double dN = (double)N;
  ks_for_each_pair(colnan, N, n, Gp, m, S, lds, nw64,
                   [&](unsigned long long* bm, int lane, int32_t p0, int32_t k, int32_t c, double* out) {
    const double* qc = Q + (int64_t)c * ldq;
    double B = 0.0;
    walk_set_bits(bm, Gi, p0, k, N, lane, [&](int32_t row) {
      if (WEIGHTED) B += W[(int64_t)c * ldq + row];
      return N - (int32_t)qc[row];   // pos - 1
    });
    if (WEIGHTED) {
      for (int o = 32; o >= 1; o >>= 1) B += __shfl_xor(B, o);
    } else {
      B = (double)k;
    }
    walk_wave_sync();
    const double dmiss = (double)(N - k);
    double best = 0.0;
    uint32_t bidx = 0u;
    walk_scan<WEIGHTED>(bm, nw64, WEIGHTED ? Wpos + (int64_t)c * ldq : nullptr, true, lane, nullptr,
                        [&](int32_t pos, uint32_t t, double cwprev, double cwt) {
      const double miss = (double)(pos - (int32_t)t) / dmiss;
      if (pos >= 2) {
        double v = cwprev / B - miss;
        if (scale) v = v / dN;
        if (fabs(v) > fabs(best)) { best = v; bidx = 2u * (uint32_t)pos - 1u; }
      }
      double v = cwt / B - miss;
      if (scale) v = v / dN;
      if (fabs(v) > fabs(best)) { best = v; bidx = 2u * (uint32_t)pos; }
    });
    // the largest |.| over the lanes, the earliest candidate among equals (a lane without one holds 0 at place 0)
    for (int o = 32; o >= 1; o >>= 1) {
      const double ov = __shfl_xor(best, o);
      const uint32_t oi = (uint32_t)__shfl_xor((int)bidx, o);
      const double a = fabs(ov), b = fabs(best);
      if (a > b || (a == b && oi < bidx)) { best = ov; bidx = oi; }
    }
    if (lane == 0) *out = best;
  });
}

// ---- replaid.gsva.exact: GSVA's random-walk statistic (include/plaidhip.h) ----------------------------
// The same bitmap walk with two differences.  The weight of a hit is a function of the walk position alone,
// w = |q - N / 2|^tau with q = N + 1 - pos: ONE table T[pos - 1] of N doubles serves every column and every set (no Wpos,
// no g x n weight matrix).  And the score needs the running sum's largest positive and largest negative excursion
// separately: every lane keeps max(after) and min(before), plain max / min butterflies combine them (no place-in-order
// tie-break: equal values are the same value).

// T[pos - 1] = |q - N / 2|^tau, q = N + 1 - pos (tau != 0; a zero distance weighs 0)
__global__ void __launch_bounds__(256)
gsva_ks_table_kernel(int32_t N, double tau, int pow_q4, double* __restrict__ T) {
  const double half = (double)N / 2.0;
  for (int32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < N; b += gridDim.x * blockDim.x) {
    const double d = fabs((double)(N - b) - half);   // exact: integers and half-integers
    T[b] = d == 0.0 ? 0.0 : (tau == 1.0 ? d : (pow_q4 > 0 ? pow_quarters(d, pow_q4) : PH_POW(d, tau)));
  }
}

// Tasks and map as gsea_ks_kernel.  WEIGHTED: B first, by walk_total_weight: B and every cw_t depend on the positions
// alone, not on the order of the set's member list.  Extremes from 0 (before_t at pos >= 2 only).
template <bool WEIGHTED>
__global__ void __launch_bounds__(64 * kKsWaves)
gsva_ks_kernel(const double* __restrict__ Q, const double* __restrict__ T, int64_t ldq, const uint32_t* __restrict__ colnan,
               int32_t N, int32_t n, const int32_t* __restrict__ Gp, const int32_t* __restrict__ Gi, int32_t m, int max_diff,
               double* __restrict__ S, int64_t lds, int32_t nw64) {
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  ks_for_each_pair(colnan, N, n, Gp, m, S, lds, nw64,
                   [&](unsigned long long* bm, int lane, int32_t p0, int32_t k, int32_t c, double* out) {
    const double* qc = Q + (int64_t)c * ldq;
    walk_set_bits(bm, Gi, p0, k, N, lane, [&](int32_t row) { return N - (int32_t)qc[row]; });   // pos - 1
    walk_wave_sync();
    double B = (double)k;
    if (WEIGHTED) {
      B = walk_total_weight(bm, nw64, T, lane);
      if (B == 0.0) {   // tau > 0, even N: the set is the gene at q = N / 2 alone
        walk_zero_map(bm, nw64, lane);
        if (lane == 0) *out = nan;
        return;
      }
    }
    const double dmiss = (double)(N - k);
    double mxp = 0.0, mxn = 0.0;
    walk_scan<WEIGHTED>(bm, nw64, T, true, lane, nullptr, [&](int32_t pos, uint32_t t, double cwprev, double cwt) {
      const double miss = (double)(pos - (int32_t)t) / dmiss;
      if (pos >= 2) {
        const double v = cwprev / B - miss;
        mxn = v < mxn ? v : mxn;
      }
      const double v = cwt / B - miss;
      mxp = v > mxp ? v : mxp;
    });
    for (int o = 32; o >= 1; o >>= 1) {
      const double a = __shfl_xor(mxp, o), b = __shfl_xor(mxn, o);
      mxp = a > mxp ? a : mxp;
      mxn = b < mxn ? b : mxn;
    }
    if (lane == 0) *out = max_diff ? mxp + mxn : (mxp > -mxn ? mxp : mxn);
  });
}

WalkLaunch ks_launch(plaidhip_ctx* ctx, int32_t g, int32_t n, int32_t m) {
  return walk_launch((((int64_t)n + kKsColTile - 1) / kKsColTile) * m, (int64_t)ctx->num_cu * 32, kKsWaves, g);
}

}  // namespace

int launch_gsea_ks(plaidhip_ctx* ctx, const double* Q, const double* W, double* Wpos, int64_t ldq, const uint32_t* colnan,
                   int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha, int scale, double* S,
                   int64_t lds) {
  if ((int64_t)m * n == 0) return PLAIDHIP_OK;
  if (const int rc = check_walk_genes("gsea_ks: nrow(X) = %d (the walk's bitmap takes at most %d genes)", g)) return rc;
  const bool weighted = alpha != 0.0;
  if (weighted) {
    const dim3 grid((unsigned)std::min<int64_t>(((int64_t)g + 255) / 256, 64), (unsigned)std::min(n, 16384));
    hipLaunchKernelGGL(gsea_ks_scatter_kernel, grid, dim3(256), 0, ctx->stream, Q, W, ldq, colnan, g, n, Wpos);
  }
  const WalkLaunch wl = ks_launch(ctx, g, n, m);
  if (weighted)
    hipLaunchKernelGGL(gsea_ks_kernel<true>, dim3(wl.blocks), dim3(64 * kKsWaves), wl.shmem, ctx->stream, Q, W, Wpos, ldq, colnan, g, n,
                       Gp, Gi, m, scale, S, lds, wl.nw64);
  else
    hipLaunchKernelGGL(gsea_ks_kernel<false>, dim3(wl.blocks), dim3(64 * kKsWaves), wl.shmem, ctx->stream, Q, W, Wpos, ldq, colnan, g, n,
                       Gp, Gi, m, scale, S, lds, wl.nw64);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_gsva_ks(plaidhip_ctx* ctx, const double* Q, int64_t ldq, const uint32_t* colnan, int32_t g, int32_t n,
                   const int32_t* Gp, const int32_t* Gi, int32_t m, double tau, int max_diff, double* T, double* S, int64_t lds) {
  if ((int64_t)m * n == 0) return PLAIDHIP_OK;
  if (const int rc = check_walk_genes("gsva_ks: nrow(X) = %d (the walk's bitmap takes at most %d genes)", g)) return rc;
  const bool weighted = tau != 0.0;
  if (weighted) {
    const double q4 = tau * 4.0;
    const int pq = (tau != 1.0 && q4 >= 1.0 && q4 <= 16.0 && q4 == (double)(int)q4) ? (int)q4 : 0;
    hipLaunchKernelGGL(gsva_ks_table_kernel, dim3((unsigned)std::min<int64_t>(((int64_t)g + 255) / 256, 64)), dim3(256), 0,
                       ctx->stream, g, tau, pq, T);
  }
  const WalkLaunch wl = ks_launch(ctx, g, n, m);
  if (weighted)
    hipLaunchKernelGGL(gsva_ks_kernel<true>, dim3(wl.blocks), dim3(64 * kKsWaves), wl.shmem, ctx->stream, Q, T, ldq, colnan, g, n, Gp, Gi,
                       m, max_diff, S, lds, wl.nw64);
  else
    hipLaunchKernelGGL(gsva_ks_kernel<false>, dim3(wl.blocks), dim3(64 * kKsWaves), wl.shmem, ctx->stream, Q, T, ldq, colnan, g, n, Gp,
                       Gi, m, max_diff, S, lds, wl.nw64);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
