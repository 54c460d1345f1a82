// plaid.gsea: preranked GSEA with a permutation null (include/plaidhip.h: plaidhip_gsea).
//
// The observed enrichment score of a (set, list) pair and the B null scores of the set are the same walk: the bitmap walk
// of bitmap_walk.h over a PLACEMENT, an int32 permutation pos[0..N) of 0..N-1 that says where each gene stands in the
// walk.  The observed placement of a list is its order by decreasing stat (gsea_operand_kernel, from the last ranks); null
// placement b is column b of P and serves every set and every list.  The weight of a hit depends on the walk position
// alone: Wpos[pos] per list, scattered once.  So the null walks read 4-byte placements and one Wpos per list where
// gsea_ks_kernel reads an 8-byte Q and a Wpos per column.
//
// gsea_null_kernel: a workgroup takes one set and one block of 64 permutations (four wavefronts, 16 permutations each, an
// N-bit map per wavefront in LDS).  A permutation's bits are set once and walked once per list of the workgroup's list
// tile (the last walk clears the map); when every weight is 1 the score does not depend on the list and is walked once.
// The 64 null scores stay in LDS; one thread per list then forms the block's six partials against the observed score,
// sequentially in b.  gsea_null_reduce_kernel adds the blocks in order.
//
// The score type (std / pos / neg: which of the walk's two extremes is the score) is a template parameter of the walk and
// of the two kernels above, and an argument of the reduction.  gsea_edge_kernel walks the observed placement once more with
// the place of each extreme kept, and writes the leading edges.
//
// This file is compiled with fp contraction off (the pragma below): every product, quotient and difference of the pinned
// form is its own IEEE operation.
#include <algorithm>

#include "bitmap_walk.h"

#pragma clang fp contract(off)

#include "gsea_walk.h"

namespace plaidhip {

namespace {

constexpr int kGnWaves = 4;        // wavefronts per workgroup, one permutation each at a time
constexpr int kGnBlock = 64;       // permutations per block of partials (PLAIDHIP_GSEA_PERM_BLOCK)
constexpr int kGnListTile = 8;     // lists that share one setting of a permutation's bits
static_assert(kGnBlock == PLAIDHIP_GSEA_PERM_BLOCK, "the block of the pinned summation order");

// y = r 2^17 + i of gene i and permutation b0 + column: tie-free (g <= 2^17), exact (r < 2^36); Y: g x nb, leading dimension g
__global__ void __launch_bounds__(256)
gsea_philox_keys_kernel(int32_t g, int64_t b0, int32_t nb, uint32_t k0, uint32_t k1, double* __restrict__ Y) {
  for (int32_t col = blockIdx.y; col < nb; col += gridDim.y) {
    const uint32_t b = (uint32_t)(b0 + col);
    for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < g; i += gridDim.x * blockDim.x) {
      uint32_t o[4];
      philox4x32_10((uint32_t)i, b, 0u, 0u, k0, k1, o);
      const uint64_t r = ((uint64_t)o[0] << 4) | (uint64_t)(o[1] >> 28);
      Y[(int64_t)col * g + i] = (double)((r << 17) + (uint64_t)i);
    }
  }
}

// P = min rank - 1
__global__ void __launch_bounds__(256)
gsea_rank_to_placement_kernel(const double* __restrict__ R, int64_t count, int32_t* __restrict__ P) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x)
    P[e] = (int32_t)R[e] - 1;
}

// every column of P (g x nb) a permutation of 0..g-1, or bad[0] = 1 and bad[1] = the largest bad column + 1.  One workgroup
// per column, a g-bit map in LDS (g <= PLAIDHIP_GSEA_KS_MAX_GENES).
__global__ void __launch_bounds__(256)
gsea_check_perm_kernel(const int32_t* __restrict__ P, int32_t g, int32_t nb, int32_t col0, uint32_t* __restrict__ bad) {
  __shared__ uint32_t seen[PLAIDHIP_GSEA_KS_MAX_GENES / 32];
  const int32_t words = (g + 31) / 32;
  for (int32_t col = blockIdx.x; col < nb; col += gridDim.x) {
    for (int32_t i = threadIdx.x; i < words; i += blockDim.x) seen[i] = 0u;
    __syncthreads();
    bool is_bad = false;
    for (int32_t i = threadIdx.x; i < g; i += blockDim.x) {
      const int32_t v = P[(int64_t)col * g + i];
      if ((uint32_t)v >= (uint32_t)g) {
        is_bad = true;
      } else {
        const uint32_t bit = 1u << (v & 31);
        if (atomicOr(&seen[v >> 5], bit) & bit) is_bad = true;
      }
    }
    if (is_bad) {
      atomicOr(&bad[0], 1u);
      atomicMax(&bad[1], (uint32_t)(col0 + col) + 1u);
    }
    __syncthreads();
  }
}

// the observed placement of every list and its weights in walk order: pos_obs[i] = N - q_i (q the last ranks: the order by
// decreasing stat, tied genes in row order), Wpos[pos_obs[i]] = weight[i].  A list flagged in listnan is skipped.
__global__ void __launch_bounds__(256)
gsea_operand_kernel(const double* __restrict__ Q, const double* __restrict__ W, int64_t ld, const uint32_t* __restrict__ listnan,
                    int32_t N, int32_t c, int32_t* __restrict__ pos_obs, double* __restrict__ Wpos) {
  for (int l = blockIdx.y; l < c; l += gridDim.y) {
    if (listnan[l]) continue;
    const int64_t b0 = (int64_t)l * ld;
    for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
      const int32_t p = N - (int32_t)Q[b0 + i];
      pos_obs[(int64_t)l * N + i] = (uint32_t)p < (uint32_t)N ? p : 0;
      if ((uint32_t)p < (uint32_t)N) Wpos[(int64_t)l * N + p] = W[(int64_t)l * N + i];
    }
  }
}

// ---- the walk (one wavefront; bitmap_walk.h) ----------------------------------------------------------------------------------
// bit pos[i] of the map for every member i of the set
__device__ __forceinline__ void gn_set_bits(unsigned long long* bm, const int32_t* __restrict__ pos, const int32_t* __restrict__ Gi,
                                            int32_t p0, int32_t k, int32_t N, int lane) {
  walk_set_bits(bm, Gi, p0, k, N, lane, [&](int32_t row) { return pos[row]; });
}

// the same choice of walk with the extremes' places kept (the map stays set)
template <bool WEIGHTED>
__device__ __forceinline__ void gn_extremes(unsigned long long* bm, int32_t nw64, const double* __restrict__ wp, int32_t N,
                                            int32_t k, int lane, uint32_t* prefix, GnExtremes* ex) {
  if (WEIGHTED) {
    const double B = walk_total_weight(bm, nw64, wp, lane);
    if (B != 0.0) {
      gn_walk<true, PLAIDHIP_GSEA_STD, true>(bm, nw64, wp, B, N, k, false, lane, prefix, ex);
      return;
    }
  }
  gn_walk<false, PLAIDHIP_GSEA_STD, true>(bm, nw64, wp, (double)k, N, k, false, lane, prefix, ex);
}

// ES[l m + j] of every (set j, list l): one wavefront per pair, the placement pos_obs of the list
template <bool WEIGHTED, int ST>
__global__ void __launch_bounds__(64 * kGnWaves)
gsea_obs_kernel(const int32_t* __restrict__ pos_obs, const double* __restrict__ Wpos, const uint32_t* __restrict__ listnan,
                int32_t N, int32_t c, const int32_t* __restrict__ Gp, const int32_t* __restrict__ Gi, int32_t m,
                double* __restrict__ ES, int32_t nw64) {
  extern __shared__ unsigned long long gn_map[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long* bm = gn_map + (size_t)wave * nw64;
  walk_zero_map(bm, nw64, lane);
  walk_wave_sync();
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int64_t pairs = (int64_t)m * c;
  for (int64_t e = (int64_t)blockIdx.x * kGnWaves + wave; e < pairs; e += (int64_t)gridDim.x * kGnWaves) {
    const int32_t l = (int32_t)(e / m), j = (int32_t)(e - (int64_t)l * m);
    const int32_t p0 = Gp[j], k = Gp[j + 1] - p0;
    if (k <= 0 || k >= N || listnan[l] != 0u) {
      if (lane == 0) ES[e] = nan;
      continue;
    }
    gn_set_bits(bm, pos_obs + (int64_t)l * N, Gi, p0, k, N, lane);
    walk_wave_sync();
    const double es = gn_score<WEIGHTED, ST>(bm, nw64, Wpos + (int64_t)l * N, N, k, true, lane);
    if (lane == 0) ES[e] = es;
    walk_wave_sync();   // the cleared words before the next pair's bits
  }
}

// The leading edge of every (set j, list l) on the observed placement: one wavefront per pair, the map of gsea_obs_kernel
// and, beside it in LDS, 4 bytes per word for the words' exclusive member counts.  The walk keeps where maxP and minP were
// first met; the score type picks the branch (std: by the sign rule of ES, none on a tie).  Then every member finds its own
// walk index t from its position p -- prefix[p >> 6] + the word's bits below p -- and, if it is in the edge, writes its row
// to slot t - 1 (top branch: walk order) or members - t (bottom branch: from the end of the list backwards).  Each slot of
// the set's segment is written by exactly one lane: the edge's by its member, the rest (-1) by the fill.
// le_len: [c][m]; le_idx: [c][nnz], nnz = Gp[m], the segment of (j, l) at l nnz + Gp[j].
template <bool WEIGHTED>
__global__ void __launch_bounds__(64 * kGnWaves)
gsea_edge_kernel(const int32_t* __restrict__ pos_obs, const double* __restrict__ Wpos, const uint32_t* __restrict__ listnan,
                 int32_t N, int32_t c, const int32_t* __restrict__ Gp, const int32_t* __restrict__ Gi, int32_t m,
                 int score_type, int32_t* __restrict__ le_len, int32_t* __restrict__ le_idx, int32_t nw64) {
  extern __shared__ unsigned long long gn_map[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long* bm = gn_map + (size_t)wave * nw64;
  uint32_t* prefix = reinterpret_cast<uint32_t*>(gn_map + (size_t)kGnWaves * nw64) + (size_t)wave * nw64;
  walk_zero_map(bm, nw64, lane);
  walk_wave_sync();
  const int32_t nnz = Gp[m];
  const int64_t pairs = (int64_t)m * c;
  for (int64_t e = (int64_t)blockIdx.x * kGnWaves + wave; e < pairs; e += (int64_t)gridDim.x * kGnWaves) {
    const int32_t l = (int32_t)(e / m), j = (int32_t)(e - (int64_t)l * m);
    const int32_t p0 = Gp[j], k = Gp[j + 1] - p0;
    if (k <= 0 || p0 < 0 || k > nnz - p0) {   // no segment to write (the second and third: a pattern that is none)
      if (lane == 0) le_len[e] = 0;
      continue;
    }
    int32_t* seg = le_idx + (int64_t)l * nnz + p0;
    if (k >= N || listnan[l] != 0u) {
      for (int32_t i = lane; i < k; i += 64) seg[i] = -1;
      if (lane == 0) le_len[e] = 0;
      continue;
    }
    const int32_t* pos = pos_obs + (int64_t)l * N;
    gn_set_bits(bm, pos, Gi, p0, k, N, lane);
    walk_wave_sync();
    GnExtremes ex;
    gn_extremes<WEIGHTED>(bm, nw64, Wpos + (int64_t)l * N, N, k, lane, prefix, &ex);
    walk_wave_sync();   // the words' counts before other lanes read them
    const bool top = score_type == PLAIDHIP_GSEA_POS || (score_type == PLAIDHIP_GSEA_STD && ex.maxP > -ex.minP);
    const bool bot = score_type == PLAIDHIP_GSEA_NEG || (score_type == PLAIDHIP_GSEA_STD && ex.maxP < -ex.minP);
    const uint32_t kk = ex.members;   // k for a set of distinct rows in range; never more
    uint32_t len = top ? ex.t_top : (bot ? kk - ex.t_bot + 1u : 0u);
    if (kk == 0u || kk > (uint32_t)k || len > kk) len = 0u;
    if (len != 0u) {
      for (int32_t i = lane; i < k; i += 64) {
        const int32_t row = Gi[p0 + i];
        if ((uint32_t)row >= (uint32_t)N) continue;
        const int32_t p = pos[row];
        if ((uint32_t)p >= (uint32_t)N) continue;
        const unsigned long long word = bm[p >> 6];
        const uint32_t t = prefix[p >> 6] + (uint32_t)__popcll(word & ((1ull << (p & 63)) - 1ull)) + 1u;
        if (top) {
          if (t <= ex.t_top) seg[t - 1u] = row;
        } else if (t >= ex.t_bot && t <= kk) {
          seg[kk - t] = row;
        }
      }
    }
    for (int32_t i = (int32_t)len + lane; i < k; i += 64) seg[i] = -1;
    if (lane == 0) le_len[e] = (int32_t)len;
    walk_wave_sync();   // every lane has read the map
    walk_zero_map(bm, nw64, lane);
    walk_wave_sync();   // the cleared words before the next pair's bits
  }
}

// P: g x nbs placements of this launch (the permutations bglob0 .. bglob0 + nbs - 1 of Btot; bglob0 a multiple of 64).
// part: [block][c][6][m] from block blk_at0 of the buffer on; null_out (nullable): [c][nbs][m], this launch's columns.
// Tasks are ordered set-first inside a block of permutations, so the workgroups in flight share its 64 columns of P in L2.
template <bool WEIGHTED, int ST>
__global__ void __launch_bounds__(64 * kGnWaves)
gsea_null_kernel(const int32_t* __restrict__ P, int32_t nbs, const double* __restrict__ Wpos,
                 const uint32_t* __restrict__ listnan, const double* __restrict__ ES, int32_t N, int32_t c,
                 const int32_t* __restrict__ Gp, const int32_t* __restrict__ Gi, int32_t m, double* __restrict__ part,
                 int64_t blk_at0, double* __restrict__ null_out, int32_t nw64) {
  extern __shared__ unsigned long long gn_map[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long* bm = gn_map + (size_t)wave * nw64;
  double* s_es = reinterpret_cast<double*>(gn_map + (size_t)kGnWaves * nw64);   // [list of the tile][64]
  walk_zero_map(bm, nw64, lane);
  walk_wave_sync();
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int32_t ntile = WEIGHTED ? (c + kGnListTile - 1) / kGnListTile : 1;
  const int32_t nblk = (nbs + kGnBlock - 1) / kGnBlock;
  const int64_t per_blk = (int64_t)m * ntile;
  const int64_t tasks = per_blk * nblk;
  for (int64_t task = blockIdx.x; task < tasks; task += gridDim.x) {
    const int32_t blk = (int32_t)(task / per_blk);
    const int64_t rem = task - (int64_t)blk * per_blk;
    const int32_t tile = (int32_t)(rem / m), j = (int32_t)(rem - (int64_t)tile * m);
    const int32_t l0 = WEIGHTED ? tile * kGnListTile : 0;
    const int32_t nl = WEIGHTED ? std::min(kGnListTile, c - l0) : c;   // lists this task forms partials for
    const int32_t nwalk = WEIGHTED ? nl : 1;                           // ... and walks
    const int32_t p0 = Gp[j], k = Gp[j + 1] - p0;
    const bool valid = k > 0 && k < N;
    const int32_t nb = std::min(kGnBlock, nbs - blk * kGnBlock);
    for (int32_t pi = wave; pi < nb; pi += kGnWaves) {   // (pi is uniform in the wavefront)
      const int32_t col = blk * kGnBlock + pi;
      if (valid) {
        gn_set_bits(bm, P + (int64_t)col * N, Gi, p0, k, N, lane);
        walk_wave_sync();
      }
      for (int32_t li = 0; li < nwalk; ++li) {
        const int32_t l = l0 + li;
        const bool last = li == nwalk - 1;
        double es = nan;
        if (valid && (!WEIGHTED || listnan[l] == 0u)) {
          es = gn_score<WEIGHTED, ST>(bm, nw64, WEIGHTED ? Wpos + (int64_t)l * N : nullptr, N, k, last, lane);
        } else if (valid && last) {
          walk_zero_map(bm, nw64, lane);
        }
        if (lane == 0) s_es[li * kGnBlock + pi] = es;
      }
      walk_wave_sync();   // the cleared words before the next permutation's bits
    }
    __syncthreads();
    // ---- the block's six partials of every list, sequentially in b; the null scores themselves when asked for -----------
    for (int32_t li = threadIdx.x; li < nl; li += blockDim.x) {
      const int32_t l = l0 + li;
      const double* es_b = s_es + (WEIGHTED ? li : 0) * kGnBlock;
      const double es = ES[(int64_t)l * m + j];
      double n_ge = 0.0, n_le = 0.0, n_ge0 = 0.0, n_le0 = 0.0, sum_pos = 0.0, sum_neg = 0.0;
      for (int32_t b = 0; b < nb; ++b) {
        const double e = es_b[b];
        n_ge += e >= es ? 1.0 : 0.0;
        n_le += e <= es ? 1.0 : 0.0;
        n_ge0 += e >= 0.0 ? 1.0 : 0.0;
        n_le0 += e <= 0.0 ? 1.0 : 0.0;
        sum_pos += e > 0.0 ? e : 0.0;
        sum_neg += e < 0.0 ? e : 0.0;
      }
      double* o = part + (((blk_at0 + blk) * c + l) * 6) * (int64_t)m + j;
      o[0] = n_ge;
      o[(int64_t)m] = n_le;
      o[2 * (int64_t)m] = n_ge0;
      o[3 * (int64_t)m] = n_le0;
      o[4 * (int64_t)m] = sum_pos;
      o[5 * (int64_t)m] = sum_neg;
    }
    if (null_out != nullptr) {
      const bool bad_set = !valid;
      for (int32_t e = threadIdx.x; e < nl * nb; e += blockDim.x) {
        const int32_t li = e / nb, b = e - li * nb;
        const int32_t l = l0 + li;
        const double v = (bad_set || listnan[l] != 0u) ? nan : s_es[(WEIGHTED ? li : 0) * kGnBlock + b];
        null_out[((int64_t)l * nbs + blk * kGnBlock + b) * m + j] = v;
      }
    }
    __syncthreads();   // s_es is the next task's
  }
}

// the blocks in order; NES, pval, nMoreExtreme.  out: m x 12 x c (column 3, padj, is the host's)
__global__ void __launch_bounds__(256)
gsea_null_reduce_kernel(const double* __restrict__ part, int32_t nblk, const double* __restrict__ ES,
                        const int32_t* __restrict__ Gp, int32_t m, int32_t c, int score_type, double* __restrict__ out) {
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int64_t pairs = (int64_t)m * c;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < pairs; e += (int64_t)gridDim.x * blockDim.x) {
    const int32_t l = (int32_t)(e / m), j = (int32_t)(e - (int64_t)l * m);
    const double es = ES[e];
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int32_t blk = 0; blk < nblk; ++blk) {
      const double* p = part + (((int64_t)blk * c + l) * 6) * (int64_t)m + j;
      for (int q = 0; q < 6; ++q) acc[q] += p[(int64_t)q * m];
    }
    double* o = out + (int64_t)l * 12 * m + j;
    const double size = (double)(Gp[j + 1] - Gp[j]);
    if (es != es) {
      for (int q = 0; q < 12; ++q) o[(int64_t)q * m] = nan;
      o[5 * (int64_t)m] = size;
      continue;
    }
    const double n_ge = acc[0], n_le = acc[1], n_ge0 = acc[2], n_le0 = acc[3], sum_pos = acc[4], sum_neg = acc[5];
    // std: the side of ES; pos: the upper side; neg: the lower side
    const bool upper = score_type == PLAIDHIP_GSEA_POS || (score_type == PLAIDHIP_GSEA_STD && es > 0.0);
    const double nes = upper ? es / (sum_pos / n_ge0) : es / fabs(sum_neg / n_le0);
    const double pl = (1.0 + n_le) / (1.0 + n_le0), pg = (1.0 + n_ge) / (1.0 + n_ge0);
    o[0] = es;
    o[(int64_t)m] = nes;
    o[2 * (int64_t)m] = score_type == PLAIDHIP_GSEA_POS ? pg : (score_type == PLAIDHIP_GSEA_NEG ? pl : (pl < pg ? pl : pg));
    o[3 * (int64_t)m] = nan;
    o[4 * (int64_t)m] = upper ? n_ge : n_le;
    o[5 * (int64_t)m] = size;
    for (int q = 0; q < 6; ++q) o[(int64_t)(6 + q) * m] = acc[q];
  }
}

constexpr const char* kGnTooManyGenes = "gsea: %d genes (the walk's bitmap takes at most %d)";

// one wavefront per (set, list) pair
WalkLaunch gn_pair_launch(plaidhip_ctx* ctx, int32_t g, int64_t pairs, int extra) {
  return walk_launch((pairs + kGnWaves - 1) / kGnWaves, (int64_t)ctx->num_cu * 16, kGnWaves, g, extra);
}

}  // namespace

int launch_gsea_operands(plaidhip_ctx* ctx, const double* Q, const double* W, int64_t ld, const uint32_t* listnan, int32_t g,
                         int32_t c, int32_t* pos_obs, double* Wpos) {
  if (g == 0 || c == 0) return PLAIDHIP_OK;
  const dim3 grid((unsigned)std::min<int64_t>(((int64_t)g + 255) / 256, 64), (unsigned)std::min(c, 16384));
  hipLaunchKernelGGL(gsea_operand_kernel, grid, dim3(256), 0, ctx->stream, Q, W, ld, listnan, g, c, pos_obs, Wpos);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_gsea_placements(plaidhip_ctx* ctx, int32_t g, int64_t b0, int32_t nb, uint64_t seed, double* Y, double* R,
                           int32_t* P) {
  if (g == 0 || nb == 0) return PLAIDHIP_OK;
  const dim3 grid((unsigned)std::min<int64_t>(((int64_t)g + 255) / 256, 64), (unsigned)std::min(nb, 16384));
  hipLaunchKernelGGL(gsea_philox_keys_kernel, grid, dim3(256), 0, ctx->stream, g, b0, nb, (uint32_t)(seed & 0xffffffffull),
                     (uint32_t)(seed >> 32), Y);
  PH_HIP(hipGetLastError());
  const int rc = launch_colranks_dense_f64(ctx, Y, g, g, nb, PLAIDHIP_TIES_MIN, 0, 1.0, R, g, nullptr);
  if (rc != PLAIDHIP_OK) return rc;
  const int64_t count = (int64_t)g * nb;
  hipLaunchKernelGGL(gsea_rank_to_placement_kernel, dim3((unsigned)std::min<int64_t>((count + 255) / 256, 65536)), dim3(256), 0,
                     ctx->stream, R, count, P);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_gsea_check_perm(plaidhip_ctx* ctx, const int32_t* P, int32_t g, int32_t nb, int32_t col0, uint32_t* bad) {
  if (g == 0 || nb == 0) return PLAIDHIP_OK;
  if (const int rc = check_walk_genes(kGnTooManyGenes, g)) return rc;
  hipLaunchKernelGGL(gsea_check_perm_kernel, dim3((unsigned)std::min(nb, ctx->num_cu * 8)), dim3(256), 0, ctx->stream, P, g, nb,
                     col0, bad);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_gsea_obs(plaidhip_ctx* ctx, int weighted, int score_type, const int32_t* pos_obs, const double* Wpos,
                    const uint32_t* listnan, int32_t g, int32_t c, const int32_t* Gp, const int32_t* Gi, int32_t m, double* ES) {
  if ((int64_t)m * c == 0) return PLAIDHIP_OK;
  if (const int rc = check_walk_genes(kGnTooManyGenes, g)) return rc;
  const WalkLaunch wl = gn_pair_launch(ctx, g, (int64_t)m * c, 0);
#define PH_GSEA_OBS(W, ST)                                                                                                     \
  hipLaunchKernelGGL((gsea_obs_kernel<W, ST>), dim3(wl.blocks), dim3(64 * kGnWaves), wl.shmem, ctx->stream, pos_obs, Wpos, listnan, g, \
                     c, Gp, Gi, m, ES, wl.nw64)
  if (weighted) {
    if (score_type == PLAIDHIP_GSEA_POS) PH_GSEA_OBS(true, PLAIDHIP_GSEA_POS);
    else if (score_type == PLAIDHIP_GSEA_NEG) PH_GSEA_OBS(true, PLAIDHIP_GSEA_NEG);
    else PH_GSEA_OBS(true, PLAIDHIP_GSEA_STD);
  } else {
    if (score_type == PLAIDHIP_GSEA_POS) PH_GSEA_OBS(false, PLAIDHIP_GSEA_POS);
    else if (score_type == PLAIDHIP_GSEA_NEG) PH_GSEA_OBS(false, PLAIDHIP_GSEA_NEG);
    else PH_GSEA_OBS(false, PLAIDHIP_GSEA_STD);
  }
#undef PH_GSEA_OBS
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_gsea_edges(plaidhip_ctx* ctx, int weighted, int score_type, const int32_t* pos_obs, const double* Wpos,
                      const uint32_t* listnan, int32_t g, int32_t c, const int32_t* Gp, const int32_t* Gi, int32_t m,
                      int32_t* le_len, int32_t* le_idx) {
  if ((int64_t)m * c == 0) return PLAIDHIP_OK;
  if (const int rc = check_walk_genes(kGnTooManyGenes, g)) return rc;
  const WalkLaunch wl = gn_pair_launch(ctx, g, (int64_t)m * c, 4);   // the maps and the words' counts: at most 96 KB
  if (weighted) {
    PH_FULL_LDS(ctx, gsea_edge_kernel<true>);
    hipLaunchKernelGGL(gsea_edge_kernel<true>, dim3(wl.blocks), dim3(64 * kGnWaves), wl.shmem, ctx->stream, pos_obs, Wpos, listnan, g, c,
                       Gp, Gi, m, score_type, le_len, le_idx, wl.nw64);
  } else {
    PH_FULL_LDS(ctx, gsea_edge_kernel<false>);
    hipLaunchKernelGGL(gsea_edge_kernel<false>, dim3(wl.blocks), dim3(64 * kGnWaves), wl.shmem, ctx->stream, pos_obs, Wpos, listnan, g, c,
                       Gp, Gi, m, score_type, le_len, le_idx, wl.nw64);
  }
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_gsea_null(plaidhip_ctx* ctx, int weighted, int score_type, const int32_t* P, int32_t nbs, const double* Wpos,
                     const uint32_t* listnan, const double* ES, int32_t g, int32_t c, const int32_t* Gp, const int32_t* Gi,
                     int32_t m, double* part, int64_t blk_at0, double* null_out) {
  if ((int64_t)m * c == 0 || nbs == 0) return PLAIDHIP_OK;
  if (const int rc = check_walk_genes(kGnTooManyGenes, g)) return rc;
  const int32_t ntile = weighted ? (c + kGnListTile - 1) / kGnListTile : 1;
  const int64_t tasks = (int64_t)m * ntile * ((nbs + kGnBlock - 1) / kGnBlock);
  const WalkLaunch wl = walk_launch(tasks, (int64_t)ctx->num_cu * 16, kGnWaves, g);
  const size_t shmem = wl.shmem + (size_t)kGnListTile * kGnBlock * 8;   // the maps and a tile's null scores: at most 68 KB
#define PH_GSEA_NULL(W, ST)                                                                                                   \
  do {                                                                                                                        \
    PH_FULL_LDS(ctx, (gsea_null_kernel<W, ST>));                                                                              \
    hipLaunchKernelGGL((gsea_null_kernel<W, ST>), dim3(wl.blocks), dim3(64 * kGnWaves), shmem, ctx->stream, P, nbs, Wpos, listnan, \
                       ES, g, c, Gp, Gi, m, part, blk_at0, null_out, wl.nw64);                                                   \
  } while (0)
  if (weighted) {
    if (score_type == PLAIDHIP_GSEA_POS) PH_GSEA_NULL(true, PLAIDHIP_GSEA_POS);
    else if (score_type == PLAIDHIP_GSEA_NEG) PH_GSEA_NULL(true, PLAIDHIP_GSEA_NEG);
    else PH_GSEA_NULL(true, PLAIDHIP_GSEA_STD);
  } else {
    if (score_type == PLAIDHIP_GSEA_POS) PH_GSEA_NULL(false, PLAIDHIP_GSEA_POS);
    else if (score_type == PLAIDHIP_GSEA_NEG) PH_GSEA_NULL(false, PLAIDHIP_GSEA_NEG);
    else PH_GSEA_NULL(false, PLAIDHIP_GSEA_STD);
  }
#undef PH_GSEA_NULL
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_gsea_null_reduce(plaidhip_ctx* ctx, const double* part, int32_t nblk, const double* ES, const int32_t* Gp, int32_t m,
                            int32_t c, int score_type, double* out) {
  const int64_t pairs = (int64_t)m * c;
  if (pairs == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(gsea_null_reduce_kernel, dim3((unsigned)std::min<int64_t>((pairs + 255) / 256, 65536)), dim3(256), 0,
                     ctx->stream, part, nblk, ES, Gp, m, c, score_type, out);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
