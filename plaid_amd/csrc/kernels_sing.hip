// replaid.sing.exact: singscore's normalised score and its dispersion, the MAD of a set's ranks in a sample
// (include/plaidhip.h: plaidhip_sing_exact).
//
// The score is a crossprod: C = sum of the set's min ranks r (the exact rank route of the SpMM kernels, integer sums),
// then sing_score_kernel's pinned epilogue -- two divisions and at most two subtractions, no product.
//
// The dispersion is a median of absolute deviations from a median per (set, column) pair: not a crossprod and not a walk
// extremum.  sing_mad_kernel takes the workgroup, tile and task order of kernels_ks.hip: ONE wavefront per pair sets the
// members' bits in an N-bit map in LDS (bitmap_walk.h), for every set size 0..N, without a sort.
//   * Min ranks tie, so the map is set over the tie-free last ranks q (bit q - 1); the order by q is an order by r.  Rpos,
//     built once per column and shared by all sets, gives r by position: Rpos[q - 1] = r (u32).
//   * One pass over the map leaves the number of members in each run of 64 words (a lane per run: at most 32 runs at
//     PLAIDHIP_GSEA_KS_MAX_GENES).  select(t), the position of the t-th member, is then a ballot over those counts, one
//     scan of the run's 64 popcounts and a ballot inside the word: s_t = Rpos[select(t)] for any t, s sorted.
//   * med = the middle s or the two middle ones; in integers M2 = 2 med.
//   * The j-th smallest |s_t - med| is min over l of max(med - s_l, s_{l+j-1} - med) (windows of j consecutive members).
//     The first term falls and the second rises with l, so the minimum sits where they cross: a binary search over l
//     for the first window with s_l + s_{l+j-1} >= M2, about log2(k) pairs of selects, then the smaller of that window's
//     second term and its predecessor's first.  Even k needs j = k / 2 and k / 2 + 1; the second crossing is the first
//     one or the window before it, one more test.
//   * 4 median(dev) is an integer; disp = 1.4826 * (that / 4): one rounding.
// Cost per pair: k atomics, 2 N / 64 LDS words, about 2 log2(k) + 6 dependent gathers from Rpos.
#include <algorithm>

#include "bitmap_walk.h"
#include "exact_common.h"

namespace plaidhip {

namespace {

constexpr int kMadWaves = 4;       // wavefronts per workgroup, one (set, column) pair each at a time
constexpr int kMadColTile = 16;    // sample columns a workgroup takes for one set before it moves to the next set

// Rpos[q - 1] = r of every row of a column (u32, leading dimension ldp).  A column holding a NaN is skipped (its q are
// no permutation; sing_mad_kernel never reads its Rpos); a q outside 1..g is never followed.
__global__ void __launch_bounds__(256)
sing_rpos_kernel(const double* __restrict__ R, const double* __restrict__ Q, int64_t ld, const uint32_t* __restrict__ colnan,
                 int32_t g, int32_t n, uint32_t* __restrict__ Rpos, int64_t ldp) {
  for (int c = blockIdx.y; c < n; c += gridDim.y) {
    if (colnan[c]) continue;
    const int64_t b = (int64_t)c * ld;
    for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < g; i += gridDim.x * blockDim.x) {
      const int32_t p = (int32_t)Q[b + i] - 1;
      if ((uint32_t)p < (uint32_t)g) Rpos[(int64_t)c * ldp + p] = (uint32_t)R[b + i];
    }
  }
}

// The pinned epilogue (include/plaidhip.h).  Cu / Cd hold the sums of the up / down set's min ranks (exact integers) on
// entry and the scores on return; Cd == nullptr: no down sets.  A down set is scored on d = N + 1 - r, whose sum
// kd (N + 1) - Cd is formed in integers.  tot (nullable) = up + down, one add.  No product anywhere: nothing to contract.
__global__ void __launch_bounds__(256)
sing_score_kernel(double* __restrict__ Cu, double* __restrict__ Cd, double* __restrict__ tot, int64_t lds, int32_t m, int32_t n,
                  const int32_t* __restrict__ ku, const int32_t* __restrict__ kd, int64_t N, int center,
                  const uint32_t* __restrict__ colnan) {
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for_each_score(m, n, lds, [&](int64_t c, int64_t j, int64_t at) {
    const bool bad = colnan[c] != 0u;
    double up, dn = 0.0;
    {
      const int64_t k = ku[j];
      const int64_t sum = bad ? 0 : (int64_t)Cu[at];
      const double mean = (double)sum / (double)k;
      const double low = (double)(k + 1) / 2.0;
      up = (mean - low) / (double)(N - k);
      if (center) up = up - 0.5;
      if (bad || k == N) up = nan;   // (k = N: 0 / 0 without ties, -x / 0 with them; NaN either way)
      Cu[at] = up;
    }
    if (Cd != nullptr) {
      const int64_t k = kd[j];
      const int64_t sum = bad ? 0 : k * (N + 1) - (int64_t)Cd[at];
      const double mean = (double)sum / (double)k;
      const double low = (double)(k + 1) / 2.0;
      dn = (mean - low) / (double)(N - k);
      if (center) dn = dn - 0.5;
      if (bad || k == N) dn = nan;
      Cd[at] = dn;
      if (tot != nullptr) tot[at] = up + dn;
    }
  });
}

// out = a + b over m x n (the total dispersion), one add
__global__ void __launch_bounds__(256)
sing_add_kernel(const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ out, int64_t lds, int32_t m,
                int32_t n) {
  for_each_score(m, n, lds, [&](int64_t, int64_t, int64_t at) { out[at] = A[at] + B[at]; });
}

// position (bit index in the map) of the t-th member, t in 0..k-1, uniform in the wavefront.  runincl: the lane's inclusive
// count of members up to and including run `lane` of 64 words (k for the lanes past the last run).
__device__ __forceinline__ int32_t mad_select(const unsigned long long* bm, uint32_t runincl, uint32_t runcnt, uint32_t t,
                                              int lane) {
  const int run = (int)__popcll(__ballot(runincl <= t));                 // runs wholly before the t-th member
  const uint32_t base = (uint32_t)__shfl((int)(runincl - runcnt), run);  // members before this run
  const unsigned long long word = bm[run * 64 + lane];
  const uint32_t cnt = (uint32_t)__popcll(word);
  const uint32_t incl = wave_incl_scan_u32(cnt);
  const uint32_t tt = t - base;
  const int wl = (int)__popcll(__ballot(incl <= tt));                    // the lane whose word holds it
  const uint32_t rem = tt - (uint32_t)__shfl((int)(incl - cnt), wl);     // its place among the word's bits
  const uint32_t wlo = (uint32_t)__shfl((int)(uint32_t)word, wl), whi = (uint32_t)__shfl((int)(uint32_t)(word >> 32), wl);
  const unsigned long long w = ((unsigned long long)whi << 32) | wlo;
  const unsigned long long below = (1ull << lane) - 1ull;
  const bool hit = ((w >> lane) & 1ull) != 0ull && (uint32_t)__popcll(w & below) == rem;
  const int bit = __ffsll((long long)__ballot(hit)) - 1;
  return (run * 64 + wl) * 64 + bit;
}

// One wavefront per (set j, column c).  A workgroup takes a set and a tile of kMadColTile columns (tasks ordered set-first,
// as gsea_ks_kernel's).  nw64: 64-bit words of one wavefront's map, a multiple of 64, at most 64 * 32.  The map is all zero
// between pairs.
__global__ void __launch_bounds__(64 * kMadWaves)
sing_mad_kernel(const double* __restrict__ Q, int64_t ldq, const uint32_t* __restrict__ Rpos, int64_t ldp,
                const uint32_t* __restrict__ colnan, int32_t N, int32_t n, const int32_t* __restrict__ Gp,
                const int32_t* __restrict__ Gi, int32_t m, double* __restrict__ S, int64_t lds, int32_t nw64) {
  extern __shared__ unsigned long long mad_map[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long* bm = mad_map + (size_t)wave * nw64;
  walk_zero_map(bm, nw64, lane);
  walk_wave_sync();
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int nruns = nw64 / 64;
  const int64_t tiles = ((int64_t)n + kMadColTile - 1) / kMadColTile;
  const int64_t tasks = tiles * m;
  for (int64_t task = blockIdx.x; task < tasks; task += gridDim.x) {
    const int64_t tile = task / m;
    const int32_t j = (int32_t)(task - tile * m);
    const int32_t p0 = Gp[j], kk = Gp[j + 1] - p0;
    const int32_t c1 = (int32_t)std::min<int64_t>(n, (tile + 1) * kMadColTile);
    for (int32_t c = (int32_t)(tile * kMadColTile) + wave; c < c1; c += kMadWaves) {   // (c is uniform in the wavefront)
      double* out = S + (int64_t)c * lds + j;
      if (kk <= 0 || colnan[c] != 0u) {
        if (lane == 0) *out = nan;
        continue;
      }
      // ---- the members' bits ------------------------------------------------------------------------------------------------
      const double* qc = Q + (int64_t)c * ldq;
      walk_set_bits(bm, Gi, p0, kk, N, lane, [&](int32_t row) { return (int32_t)qc[row] - 1; });
      walk_wave_sync();
      // ---- members per run of 64 words: lane `run` keeps the run's count --------------------------------------------------
      uint32_t runcnt = 0u;
      for (int run = 0; run < nruns; ++run) {
        const uint32_t cnt = (uint32_t)__popcll(bm[run * 64 + lane]);
        const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_u32(cnt), 63);
        if (lane == run) runcnt = tot;
      }
      const uint32_t runincl = wave_incl_scan_u32(runcnt);
      const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)runincl, 63);   // members present (every bit is < N)
      if (k == 0u) {
        if (lane == 0) *out = nan;
        continue;
      }
      const uint32_t* rp = Rpos + (int64_t)c * ldp;
      auto s_at = [&](uint32_t t) -> int64_t {   // (every lane reads the same word: the value is the wavefront's)
        return (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)rp[mad_select(bm, runincl, runcnt, t, lane)]);
      };
      // ---- M2 = 2 median(s) ---------------------------------------------------------------------------------------------------
      const int64_t M2 = (k & 1u) ? 2 * s_at(k / 2u) : s_at(k / 2u - 1u) + s_at(k / 2u);
      // ---- D2(jw) = 2 * (the jw-th smallest |s - med|): the crossing of the windows of jw members ---------------------------
      // first window l in [lo, hi] with s_l + s_{l+jw-1} >= M2 (hi: none below it), then the two candidates beside it
      auto crossing = [&](uint32_t jw, uint32_t lo, uint32_t hi, uint32_t* at) -> int64_t {
        const uint32_t W = k - jw + 1u;   // windows
        while (lo < hi) {
          const uint32_t mid = lo + (hi - lo) / 2u;
          if (s_at(mid) + s_at(mid + jw - 1u) >= M2) hi = mid;
          else lo = mid + 1u;
        }
        *at = lo;
        int64_t best = INT64_MAX;
        if (lo < W) best = 2 * s_at(lo + jw - 1u) - M2;
        if (lo > 0u) {
          const int64_t a = M2 - 2 * s_at(lo - 1u);
          best = a < best ? a : best;
        }
        return best;
      };
      int64_t md4;   // 4 * median(|s - med|)
      uint32_t l1 = 0u;
      if (k & 1u) {
        md4 = 2 * crossing((k + 1u) / 2u, 0u, k - (k + 1u) / 2u + 1u, &l1);
      } else {
        const uint32_t j1 = k / 2u, j2 = j1 + 1u;
        const int64_t d1 = crossing(j1, 0u, k - j1 + 1u, &l1);
        // windows one member longer cross at l1 or at the window before it
        uint32_t l2 = 0u;
        const uint32_t W2 = k - j2 + 1u;
        const int64_t d2 = crossing(j2, l1 > 0u ? l1 - 1u : 0u, l1 < W2 ? l1 : W2, &l2);
        md4 = d1 + d2;
      }
      if (lane == 0) *out = 1.4826 * ((double)md4 * 0.25);
      // ---- the map back to zero -----------------------------------------------------------------------------------------------
      walk_zero_map(bm, nw64, lane);
      walk_wave_sync();
    }
  }
}

}  // namespace

int launch_sing_rpos(plaidhip_ctx* ctx, const double* R, const double* Q, int64_t ld, const uint32_t* colnan, int32_t g,
                     int32_t n, uint32_t* Rpos, int64_t ldp) {
  if (n == 0 || g == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(sing_rpos_kernel, rank_cols_grid(dense_cols(g, n, ld)), dim3(256), 0, ctx->stream, R, Q, ld, colnan, g, n, Rpos, ldp);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_sing_score(plaidhip_ctx* ctx, double* Cu, double* Cd, double* tot, int64_t lds, int32_t m, int32_t n,
                      const int32_t* ku, const int32_t* kd, int32_t g, int center, const uint32_t* colnan) {
  if ((int64_t)m * n == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(sing_score_kernel, dim3(score_part_blocks(ctx, (int64_t)m * n)), dim3(256), 0, ctx->stream, Cu, Cd, tot, lds, m, n,
                     ku, kd, (int64_t)g, center, colnan);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_sing_add(plaidhip_ctx* ctx, const double* A, const double* B, double* out, int64_t lds, int32_t m, int32_t n) {
  if ((int64_t)m * n == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(sing_add_kernel, dim3(score_part_blocks(ctx, (int64_t)m * n)), dim3(256), 0, ctx->stream, A, B, out, lds, m, n);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_sing_mad(plaidhip_ctx* ctx, const double* Q, int64_t ldq, const uint32_t* Rpos, int64_t ldp, const uint32_t* colnan,
                    int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double* S, int64_t lds) {
  if ((int64_t)m * n == 0) return PLAIDHIP_OK;
  if (const int rc = check_walk_genes("sing_mad: nrow(X) = %d (the bitmap takes at most %d genes)", g)) return rc;
  const WalkLaunch wl = walk_launch((((int64_t)n + kMadColTile - 1) / kMadColTile) * m, (int64_t)ctx->num_cu * 32, kMadWaves, g);
  hipLaunchKernelGGL(sing_mad_kernel, dim3(wl.blocks), dim3(64 * kMadWaves), wl.shmem, ctx->stream, Q, ldq, Rpos, ldp, colnan, g, n, Gp,
                     Gi, m, S, lds, wl.nw64);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
