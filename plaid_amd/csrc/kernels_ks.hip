// replaid.ssgsea.exact(single = FALSE): the running sum's value of largest magnitude (the classic GSEA enrichment score,
// gao.ssgsea's second branch).  An extremum over a walk is not a sum, so no crossprod gives it: this file holds the walk.
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

#include "common.h"
#include "rank_bucket.h"

namespace plaidhip {

namespace {

constexpr int kKsWaves = 4;       // wavefronts per workgroup, one (set, column) pair each at a time
constexpr int kKsColTile = 16;    // sample columns a workgroup scores for one set before it moves to the next set

__device__ __forceinline__ void ks_wave_sync() {   // LDS written by the wavefront's lanes is read by its other lanes
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

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

// One wavefront per (set j, column c).  A workgroup takes a set and a tile of kKsColTile columns (tasks ordered set-first,
// so the workgroups in flight share the tile's Q columns in L2).  nw64: 64-bit words of one wavefront's map, a multiple
// of 64.  The map is all zero between pairs: the scan clears the words it reads.
template <bool WEIGHTED>
__global__ void __launch_bounds__(64 * kKsWaves)
gsea_ks_kernel(const double* __restrict__ Q, const double* __restrict__ W, const double* __restrict__ Wpos, int64_t ldq,
               const uint32_t* __restrict__ colnan, int32_t N, int32_t n, const int32_t* __restrict__ Gp,
               const int32_t* __restrict__ Gi, int32_t m, int scale, double* __restrict__ S, int64_t lds, int32_t nw64) {
  extern __shared__ unsigned long long ks_map[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long* bm = ks_map + (size_t)wave * nw64;
  uint32_t* bm32 = reinterpret_cast<uint32_t*>(bm);
  for (int32_t i = lane; i < nw64; i += 64) bm[i] = 0ull;
  ks_wave_sync();
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double dN = (double)N;
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
      // ---- the members' bits; B -----------------------------------------------------------------------------------------
      const double* qc = Q + (int64_t)c * ldq;
      double B = 0.0;
      for (int32_t i = lane; i < k; i += 64) {
        const int32_t row = Gi[p0 + i];
        if ((uint32_t)row >= (uint32_t)N) continue;
        const int32_t b = N - (int32_t)qc[row];   // pos - 1
        if ((uint32_t)b < (uint32_t)N) atomicOr(&bm32[b >> 5], 1u << (b & 31));
        if (WEIGHTED) B += W[(int64_t)c * ldq + row];
      }
      if (WEIGHTED) {
        for (int o = 32; o >= 1; o >>= 1) B += __shfl_xor(B, o);
      } else {
        B = (double)k;
      }
      ks_wave_sync();
      // ---- the walk over the set bits, 64 words at a time ---------------------------------------------------------------
      const double* wp = WEIGHTED ? Wpos + (int64_t)c * ldq : nullptr;
      const double dmiss = (double)(N - k);
      uint32_t tbase = 0u;     // members in the words already walked
      double cwbase = 0.0;     // their weight
      double best = 0.0;
      uint32_t bidx = 0u;      // the best candidate's place in the visiting order (2 pos - 1: before, 2 pos: after)
      for (int32_t w0 = 0; w0 < nw64; w0 += 64) {
        unsigned long long word = bm[w0 + lane];
        if (__ballot(word != 0ull) == 0ull) continue;
        bm[w0 + lane] = 0ull;
        const uint32_t cnt = (uint32_t)__popcll(word);
        const uint32_t incl = wave_incl_scan_u32(cnt);
        uint32_t t = tbase + incl - cnt;
        tbase += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const int32_t pos0 = (w0 + lane) * 64;   // position - 1 of the word's bit 0
        double cw = 0.0;
        if (WEIGHTED) {
          double s = 0.0;
          for (unsigned long long wd = word; wd != 0ull; wd &= wd - 1ull) s += wp[pos0 + (__ffsll((long long)wd) - 1)];
          double inc = s;   // inclusive prefix sum over the lanes
          for (int o = 1; o < 64; o <<= 1) {
            const double up = __shfl_up(inc, o);
            if (lane >= o) inc += up;
          }
          const double excl = __shfl_up(inc, 1);
          cw = cwbase + (lane == 0 ? 0.0 : excl);
          cwbase += __shfl(inc, 63);
        }
        for (; word != 0ull; word &= word - 1ull) {
          const int32_t pos = pos0 + __ffsll((long long)word);
          const double cwprev = WEIGHTED ? cw : (double)t;
          t += 1u;
          if (WEIGHTED) cw += wp[pos - 1];
          const double cwt = WEIGHTED ? cw : (double)t;
          const double miss = (double)(pos - (int32_t)t) / dmiss;
          if (pos >= 2) {
            double v = cwprev / B - miss;
            if (scale) v = v / dN;
            if (fabs(v) > fabs(best)) { best = v; bidx = 2u * (uint32_t)pos - 1u; }
          }
          double v = cwt / B - miss;
          if (scale) v = v / dN;
          if (fabs(v) > fabs(best)) { best = v; bidx = 2u * (uint32_t)pos; }
        }
      }
      // the largest |.| over the lanes, the earliest candidate among equals (a lane without one holds 0 at place 0)
      for (int o = 32; o >= 1; o >>= 1) {
        const double ov = __shfl_xor(best, o);
        const uint32_t oi = (uint32_t)__shfl_xor((int)bidx, o);
        const double a = fabs(ov), b = fabs(best);
        if (a > b || (a == b && oi < bidx)) { best = ov; bidx = oi; }
      }
      if (lane == 0) *out = best;
      ks_wave_sync();   // the cleared words before the next pair's bits
    }
  }
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

// One wavefront per (set j, column c), tasks and map as gsea_ks_kernel.  WEIGHTED: B first, by a pass over the map that
// adds the words' weights as the walk below adds them to its base (the inclusive scan's last lane holds the sum tree of
// an ascending butterfly): B and every cw_t depend on the positions alone, not on the order of the set's member list.
template <bool WEIGHTED>
__global__ void __launch_bounds__(64 * kKsWaves)
gsva_ks_kernel(const double* __restrict__ Q, const double* __restrict__ T, int64_t ldq, const uint32_t* __restrict__ colnan,
               int32_t N, int32_t n, const int32_t* __restrict__ Gp, const int32_t* __restrict__ Gi, int32_t m, int max_diff,
               double* __restrict__ S, int64_t lds, int32_t nw64) {
  extern __shared__ unsigned long long ks_map[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long* bm = ks_map + (size_t)wave * nw64;
  uint32_t* bm32 = reinterpret_cast<uint32_t*>(bm);
  for (int32_t i = lane; i < nw64; i += 64) bm[i] = 0ull;
  ks_wave_sync();
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
      // ---- the members' bits ----------------------------------------------------------------------------------------------
      const double* qc = Q + (int64_t)c * ldq;
      for (int32_t i = lane; i < k; i += 64) {
        const int32_t row = Gi[p0 + i];
        if ((uint32_t)row >= (uint32_t)N) continue;
        const int32_t b = N - (int32_t)qc[row];   // pos - 1
        if ((uint32_t)b < (uint32_t)N) atomicOr(&bm32[b >> 5], 1u << (b & 31));
      }
      ks_wave_sync();
      // ---- B ----------------------------------------------------------------------------------------------------------------
      double B = (double)k;
      if (WEIGHTED) {
        B = 0.0;
        for (int32_t w0 = 0; w0 < nw64; w0 += 64) {
          const unsigned long long word = bm[w0 + lane];
          if (__ballot(word != 0ull) == 0ull) continue;
          const int32_t pos0 = (w0 + lane) * 64;
          double s = 0.0;
          for (unsigned long long wd = word; wd != 0ull; wd &= wd - 1ull) s += T[pos0 + (__ffsll((long long)wd) - 1)];
          for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
          B += __shfl(s, 63);
        }
        if (B == 0.0) {   // tau > 0, even N: the set is the gene at q = N / 2 alone
          for (int32_t i = lane; i < nw64; i += 64) bm[i] = 0ull;
          if (lane == 0) *out = nan;
          ks_wave_sync();
          continue;
        }
      }
      // ---- the walk over the set bits, 64 words at a time -----------------------------------------------------------------
      const double dmiss = (double)(N - k);
      uint32_t tbase = 0u;     // members in the words already walked
      double cwbase = 0.0;     // their weight
      double mxp = 0.0, mxn = 0.0;
      for (int32_t w0 = 0; w0 < nw64; w0 += 64) {
        unsigned long long word = bm[w0 + lane];
        if (__ballot(word != 0ull) == 0ull) continue;
        bm[w0 + lane] = 0ull;
        const uint32_t cnt = (uint32_t)__popcll(word);
        const uint32_t incl = wave_incl_scan_u32(cnt);
        uint32_t t = tbase + incl - cnt;
        tbase += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const int32_t pos0 = (w0 + lane) * 64;   // position - 1 of the word's bit 0
        double cw = 0.0;
        if (WEIGHTED) {
          double s = 0.0;
          for (unsigned long long wd = word; wd != 0ull; wd &= wd - 1ull) s += T[pos0 + (__ffsll((long long)wd) - 1)];
          double inc = s;   // inclusive prefix sum over the lanes
          for (int o = 1; o < 64; o <<= 1) {
            const double up = __shfl_up(inc, o);
            if (lane >= o) inc += up;
          }
          const double excl = __shfl_up(inc, 1);
          cw = cwbase + (lane == 0 ? 0.0 : excl);
          cwbase += __shfl(inc, 63);
        }
        for (; word != 0ull; word &= word - 1ull) {
          const int32_t pos = pos0 + __ffsll((long long)word);
          const double cwprev = WEIGHTED ? cw : (double)t;
          t += 1u;
          if (WEIGHTED) cw += T[pos - 1];
          const double cwt = WEIGHTED ? cw : (double)t;
          const double miss = (double)(pos - (int32_t)t) / dmiss;
          if (pos >= 2) {
            const double v = cwprev / B - miss;
            mxn = v < mxn ? v : mxn;
          }
          const double v = cwt / B - miss;
          mxp = v > mxp ? v : mxp;
        }
      }
      for (int o = 32; o >= 1; o >>= 1) {
        const double a = __shfl_xor(mxp, o), b = __shfl_xor(mxn, o);
        mxp = a > mxp ? a : mxp;
        mxn = b < mxn ? b : mxn;
      }
      if (lane == 0) *out = max_diff ? mxp + mxn : (mxp > -mxn ? mxp : mxn);
      ks_wave_sync();   // the cleared words before the next pair's bits
    }
  }
}

// block partials {min, max, any NaN} of the m x n scores for norm
__global__ void __launch_bounds__(256)
gsea_ks_range_kernel(const double* __restrict__ S, int64_t lds, int32_t m, int32_t n, double* __restrict__ part) {
  __shared__ double s_mn[4], s_mx[4], s_nf[4];
  double mn = INFINITY, mx = -INFINITY, nf = 0.0;
  const int64_t total = (int64_t)m * n;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = e / m, j = e - c * m;
    const double es = S[c * lds + j];
    if (es != es) nf = 1.0;
    else { mn = es < mn ? es : mn; mx = es > mx ? es : mx; }
  }
  for (int o = 32; o >= 1; o >>= 1) {
    const double a = __shfl_xor(mn, o), b = __shfl_xor(mx, o), f = __shfl_xor(nf, o);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
    nf = f > nf ? f : nf;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_mn[wave] = mn; s_mx[wave] = mx; s_nf[wave] = nf; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      mn = s_mn[w] < mn ? s_mn[w] : mn;
      mx = s_mx[w] > mx ? s_mx[w] : mx;
      nf = s_nf[w] > nf ? s_nf[w] : nf;
    }
    part[3 * (int64_t)blockIdx.x] = mn;
    part[3 * (int64_t)blockIdx.x + 1] = mx;
    part[3 * (int64_t)blockIdx.x + 2] = nf;
  }
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

}  // namespace

int launch_gsea_ks(plaidhip_ctx* ctx, const double* Q, const double* W, double* Wpos, int64_t ldq, const uint32_t* colnan,
                   int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha, int scale, double* S,
                   int64_t lds) {
  if ((int64_t)m * n == 0) return PLAIDHIP_OK;
  if (g > PLAIDHIP_GSEA_KS_MAX_GENES) {
    set_error("gsea_ks: nrow(X) = %d (the walk's bitmap takes at most %d genes)", g, PLAIDHIP_GSEA_KS_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  const bool weighted = alpha != 0.0;
  if (weighted) {
    const dim3 grid((unsigned)std::min<int64_t>(((int64_t)g + 255) / 256, 64), (unsigned)std::min(n, 16384));
    hipLaunchKernelGGL(gsea_ks_scatter_kernel, grid, dim3(256), 0, ctx->stream, Q, W, ldq, colnan, g, n, Wpos);
  }
  const int32_t nw64 = (int32_t)((((int64_t)g + 63) / 64 + 63) / 64 * 64);
  const size_t shmem = (size_t)kKsWaves * nw64 * 8;   // at most 64 KB at PLAIDHIP_GSEA_KS_MAX_GENES
  const int64_t tasks = (((int64_t)n + kKsColTile - 1) / kKsColTile) * m;
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(tasks, (int64_t)ctx->num_cu * 32));
  if (weighted)
    hipLaunchKernelGGL(gsea_ks_kernel<true>, dim3(blocks), dim3(64 * kKsWaves), shmem, ctx->stream, Q, W, Wpos, ldq, colnan, g, n,
                       Gp, Gi, m, scale, S, lds, nw64);
  else
    hipLaunchKernelGGL(gsea_ks_kernel<false>, dim3(blocks), dim3(64 * kKsWaves), shmem, ctx->stream, Q, W, Wpos, ldq, colnan, g, n,
                       Gp, Gi, m, scale, S, lds, nw64);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_gsva_ks(plaidhip_ctx* ctx, const double* Q, int64_t ldq, const uint32_t* colnan, int32_t g, int32_t n,
                   const int32_t* Gp, const int32_t* Gi, int32_t m, double tau, int max_diff, double* T, double* S, int64_t lds) {
  if ((int64_t)m * n == 0) return PLAIDHIP_OK;
  if (g > PLAIDHIP_GSEA_KS_MAX_GENES) {
    set_error("gsva_ks: nrow(X) = %d (the walk's bitmap takes at most %d genes)", g, PLAIDHIP_GSEA_KS_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  const bool weighted = tau != 0.0;
  if (weighted) {
    const double q4 = tau * 4.0;
    const int pq = (tau != 1.0 && q4 >= 1.0 && q4 <= 16.0 && q4 == (double)(int)q4) ? (int)q4 : 0;
    hipLaunchKernelGGL(gsva_ks_table_kernel, dim3((unsigned)std::min<int64_t>(((int64_t)g + 255) / 256, 64)), dim3(256), 0,
                       ctx->stream, g, tau, pq, T);
  }
  const int32_t nw64 = (int32_t)((((int64_t)g + 63) / 64 + 63) / 64 * 64);
  const size_t shmem = (size_t)kKsWaves * nw64 * 8;   // at most 64 KB at PLAIDHIP_GSEA_KS_MAX_GENES
  const int64_t tasks = (((int64_t)n + kKsColTile - 1) / kKsColTile) * m;
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(tasks, (int64_t)ctx->num_cu * 32));
  if (weighted)
    hipLaunchKernelGGL(gsva_ks_kernel<true>, dim3(blocks), dim3(64 * kKsWaves), shmem, ctx->stream, Q, T, ldq, colnan, g, n, Gp, Gi,
                       m, max_diff, S, lds, nw64);
  else
    hipLaunchKernelGGL(gsva_ks_kernel<false>, dim3(blocks), dim3(64 * kKsWaves), shmem, ctx->stream, Q, T, ldq, colnan, g, n, Gp,
                       Gi, m, max_diff, S, lds, nw64);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_gsea_ks_range(plaidhip_ctx* ctx, const double* S, int64_t lds, int32_t m, int32_t n, double* part, double* range_out) {
  if ((int64_t)m * n == 0) return PLAIDHIP_OK;
  const int blocks = ssgsea_exact_part_blocks(ctx, (int64_t)m * n);
  hipLaunchKernelGGL(gsea_ks_range_kernel, dim3(blocks), dim3(256), 0, ctx->stream, S, lds, m, n, part);
  hipLaunchKernelGGL(gsea_ks_range_final_kernel, dim3(1), dim3(64), 0, ctx->stream, part, blocks, range_out);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
