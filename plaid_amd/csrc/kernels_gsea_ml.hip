// plaid.gsea's multilevel p-values (include/plaidhip.h: plaidhip_gsea_multilevel): adaptive multilevel
// splitting over k-subsets of one list's walk positions, with a one-gene Metropolis move.
//
// A RULER belongs to one (list, side, set size k) and serves every set of that list, side and size.  Its state lives in
// global memory between launches: n maps of ceil(N / 64) words (the n sample slots), their n scores, a small record
// (MlState) and the trace of levels.  No launch runs a ruler to its end: the host advances all unfinished rulers one stage
// at a time and reads back one counter, so a launch is bounded by one stage's work whatever the data.
//
// gsea_ml_init_kernel    one wavefront per (ruler, slot): the first-distinct-draws state in its LDS map, 64 draws at a
//                        time; the batch that would pass the target is taken back and finished in draw order.
// gsea_ml_stage_kernel   one workgroup per ruler: the median of the n scores by rank counting in LDS, the count above it,
//                        the trace, the read-off of every set whose target the level has reached (or of all that are left
//                        when the ruler ends), the end test, the copies of survivors over the slots at or below the level.
// gsea_ml_mutate_kernel  one wavefront per (ruler, slot): the slot's map in LDS, T = sweeps k proposals, each a select of
//                        the a-th member (popcounts and one wavefront scan per 64 words), two bit flips and one walk
//                        (gsea_walk.h: the walk behind the observed ES), taken back when the score does not pass the level.
//
// fp contraction is off as in kernels_gsea.hip: the scores are formed by the operations of the pinned form and no other.
#include <algorithm>

#include "bitmap_walk.h"

#pragma clang fp contract(off)

#include "gsea_walk.h"

namespace plaidhip {

namespace {

constexpr int kMlWaves = 4;      // wavefronts per workgroup of the init and mutate kernels, a map each
constexpr int kMlStageThreads = 256;
constexpr int kMlMaxSample = 1024;
static_assert(PLAIDHIP_GSEA_ML_MAX_SAMPLE < kMlMaxSample, "the stage kernel's LDS arrays");

// h(S) of the set in the map: ES by the score type, negated on the negative side (pos: maxP; neg: -minP)
template <bool WEIGHTED, int ST>
__device__ __forceinline__ double ml_h(unsigned long long* bm, int32_t nw64, const double* __restrict__ wp, int32_t N, int32_t k,
                                       int32_t side, int lane) {
  const double es = gn_score<WEIGHTED, ST>(bm, nw64, wp, N, k, false, lane);
  return side ? -es : es;
}

__device__ __forceinline__ uint32_t ml_tag(const GseaMlRuler& r) { return 0x80000000u | ((uint32_t)r.tag << 1) | (uint32_t)r.side; }

__device__ __forceinline__ uint32_t ml_below(uint32_t o, uint32_t R) { return (uint32_t)(((uint64_t)o * R) >> 32); }

// the position of the a-th member (0-based, ascending) of the map; a < members
__device__ __forceinline__ int32_t ml_select(const unsigned long long* bm, int32_t nw64, uint32_t a, int lane) {
  uint32_t base = 0u;
  for (int32_t w0 = 0; w0 < nw64; w0 += 64) {
    unsigned long long word = bm[w0 + lane];
    if (__ballot(word != 0ull) == 0ull) continue;
    const uint32_t cnt = (uint32_t)__popcll(word);
    const uint32_t incl = wave_incl_scan_u32(cnt);
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (a < base + total) {
      const uint32_t lo = base + incl - cnt;
      const bool mine = a >= lo && a < lo + cnt;
      int32_t pos = 0;
      if (mine) {
        for (uint32_t r = a - lo; r != 0u; --r) word &= word - 1ull;
        pos = (w0 + lane) * 64 + (__ffsll((long long)word) - 1);
      }
      const unsigned long long who = __ballot(mine);
      return __shfl(pos, __ffsll((long long)who) - 1);
    }
    base += total;
  }
  return -1;   // (a >= members: the callers never ask)
}

template <bool WEIGHTED, int ST>
__global__ void __launch_bounds__(64 * kMlWaves)
gsea_ml_init_kernel(const GseaMlRuler* __restrict__ rulers, int32_t nr, int32_t n, int32_t N, const double* __restrict__ Wpos,
                    uint32_t key0, uint32_t key1, unsigned long long* __restrict__ maps, double* __restrict__ H, int32_t nwg,
                    int32_t nw64) {
  extern __shared__ unsigned long long ml_map[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long* bm = ml_map + (size_t)wave * nw64;
  uint32_t* bm32 = reinterpret_cast<uint32_t*>(bm);
  const int64_t tasks = (int64_t)nr * n;
  const uint32_t cap = 64u * (uint32_t)N + 4096u;   // a guard no seed reaches: about 0.7 N draws fill half the positions
  for (int64_t e = (int64_t)blockIdx.x * kMlWaves + wave; e < tasks; e += (int64_t)gridDim.x * kMlWaves) {
    const int32_t r = (int32_t)(e / n), slot = (int32_t)(e - (int64_t)r * n);
    const GseaMlRuler ru = rulers[r];
    const int32_t k = ru.k;
    const uint32_t tag = ml_tag(ru);
    walk_zero_map(bm, nw64, lane);
    walk_wave_sync();
    const uint32_t target = (uint32_t)std::min(k, N - k);
    uint32_t count = 0u;
    for (uint32_t d0 = 0u; count < target && d0 < cap; d0 += 64u) {
      const uint32_t d = d0 + (uint32_t)lane;
      uint32_t o[4];
      philox4x32_10(0x80000000u | (d >> 2), (uint32_t)slot, (uint32_t)k, tag, key0, key1, o);
      const uint32_t v = ml_below(o[d & 3u], (uint32_t)N);
      const uint32_t bit = 1u << (v & 31u);
      const bool isnew = (atomicOr(&bm32[v >> 5], bit) & bit) == 0u;
      const uint32_t nnew = (uint32_t)__popcll(__ballot(isnew));
      if (count + nnew <= target) {
        count += nnew;
      } else {   // the batch passes the target: take it back, then draw by draw
        if (isnew) atomicAnd(&bm32[v >> 5], ~bit);
        walk_wave_sync();
        for (int j = 0; j < 64 && count < target; ++j) {
          const uint32_t vj = (uint32_t)__shfl((int)v, j);
          const uint32_t bj = 1u << (vj & 31u);
          if ((bm32[vj >> 5] & bj) == 0u) {
            if (lane == 0) bm32[vj >> 5] |= bj;
            count += 1u;
          }
          walk_wave_sync();
        }
      }
      walk_wave_sync();
    }
    if (2 * (int64_t)k > N) {   // the complement within the N positions
      for (int32_t w = lane; w < nwg; w += 64) {
        const int32_t tail = N - w * 64;
        const unsigned long long mask = tail >= 64 ? ~0ull : ((1ull << tail) - 1ull);
        bm[w] = ~bm[w] & mask;
      }
      walk_wave_sync();
    }
    const double h = ml_h<WEIGHTED, ST>(bm, nw64, WEIGHTED ? Wpos + (int64_t)ru.l * N : nullptr, N, k, ru.side, lane);
    unsigned long long* out = maps + (size_t)e * nwg;
    for (int32_t w = lane; w < nwg; w += 64) out[w] = bm[w];
    if (lane == 0) H[e] = h;
    walk_wave_sync();   // every lane has read the map
  }
}

template <bool WEIGHTED, int ST>
__global__ void __launch_bounds__(64 * kMlWaves)
gsea_ml_mutate_kernel(const GseaMlRuler* __restrict__ rulers, const GseaMlState* __restrict__ state, int32_t nr, int32_t n,
                      int32_t N, const double* __restrict__ Wpos, uint32_t key0, uint32_t key1, int32_t sweeps,
                      unsigned long long* __restrict__ maps, double* __restrict__ H, int32_t nwg, int32_t nw64) {
  extern __shared__ unsigned long long ml_map[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long* bm = ml_map + (size_t)wave * nw64;
  const int64_t tasks = (int64_t)nr * n;
  for (int32_t w = nwg + lane; w < nw64; w += 64) bm[w] = 0ull;   // (the words past the map stay empty)
  for (int64_t e = (int64_t)blockIdx.x * kMlWaves + wave; e < tasks; e += (int64_t)gridDim.x * kMlWaves) {
    const int32_t r = (int32_t)(e / n), slot = (int32_t)(e - (int64_t)r * n);
    const GseaMlState st = state[r];
    if (st.ended != 0) continue;   // (uniform in the wavefront)
    const GseaMlRuler ru = rulers[r];
    const int32_t k = ru.k, side = ru.side;
    const uint32_t tag = ml_tag(ru);
    const double* wp = WEIGHTED ? Wpos + (int64_t)ru.l * N : nullptr;
    unsigned long long* mine = maps + (size_t)e * nwg;
    for (int32_t w = lane; w < nwg; w += 64) bm[w] = mine[w];
    walk_wave_sync();
    double h = H[e];
    const double level = st.level;
    const uint32_t T = (uint32_t)sweeps * (uint32_t)k;
    const uint32_t x0 = (uint32_t)(st.stage - 1) * T;   // the stage just recorded
    for (uint32_t step = 0u; step < T; ++step) {
      uint32_t o[4];
      philox4x32_10(x0 + step, (uint32_t)slot, (uint32_t)k, tag, key0, key1, o);
      const uint32_t a = ml_below(o[0], (uint32_t)k), b = ml_below(o[1], (uint32_t)N);
      const unsigned long long bbit = 1ull << (b & 63u);
      if ((bm[b >> 6] & bbit) != 0ull) continue;   // (uniform: every lane reads the same word)
      const int32_t pa = ml_select(bm, nw64, a, lane);
      if (pa < 0) continue;
      const unsigned long long abit = 1ull << (pa & 63);
      if (lane == 0) {
        bm[pa >> 6] &= ~abit;
        bm[b >> 6] |= bbit;
      }
      walk_wave_sync();
      const double h2 = ml_h<WEIGHTED, ST>(bm, nw64, wp, N, k, side, lane);
      if (h2 > level) {
        h = h2;
      } else {
        walk_wave_sync();   // every lane has read the map
        if (lane == 0) {
          bm[b >> 6] &= ~bbit;
          bm[pa >> 6] |= abit;
        }
        walk_wave_sync();
      }
    }
    walk_wave_sync();
    for (int32_t w = lane; w < nwg; w += 64) mine[w] = bm[w];
    if (lane == 0) H[e] = h;
    walk_wave_sync();   // every lane has read the map
  }
}

// One stage of every unfinished ruler.  s_trace / m_trace: [nr][PLAIDHIP_GSEA_ML_MAX_STAGES]; h_trace (nullable):
// [nr][MAX_STAGES][n].  Per set of a ruler (gamma: its target): lstar (-1 until read off), cnt, est.
__global__ void __launch_bounds__(kMlStageThreads)
gsea_ml_stage_kernel(const GseaMlRuler* __restrict__ rulers, GseaMlState* __restrict__ state, int32_t n, double eps,
                     unsigned long long* __restrict__ maps, double* __restrict__ H, int32_t nwg, int32_t* __restrict__ s_trace,
                     double* __restrict__ m_trace, double* __restrict__ h_trace, const double* __restrict__ gamma,
                     int32_t* __restrict__ lstar, int32_t* __restrict__ cnt, int32_t* __restrict__ est,
                     uint32_t* __restrict__ unfinished) {
  __shared__ double sh[kMlMaxSample];
  __shared__ int32_t s_surv[kMlMaxSample], s_los[kMlMaxSample];
  __shared__ double s_med;
  __shared__ int32_t s_count;
  const int32_t r = blockIdx.x;
  const GseaMlState st = state[r];
  if (st.ended != 0) return;   // (uniform in the workgroup)
  const GseaMlRuler ru = rulers[r];
  const int tid = threadIdx.x;
  double* Hr = H + (size_t)r * n;
  for (int32_t i = tid; i < n; i += kMlStageThreads) sh[i] = Hr[i];
  if (tid == 0) s_count = 0;
  __syncthreads();
  // ---- the (n + 1) / 2-th smallest: the value with fewer than that many below it and at least that many at or below ------
  const int32_t rank = (n + 1) / 2;
  for (int32_t i = tid; i < n; i += kMlStageThreads) {
    const double v = sh[i];
    int32_t lt = 0, le = 0;
    for (int32_t j = 0; j < n; ++j) {
      lt += sh[j] < v ? 1 : 0;
      le += sh[j] <= v ? 1 : 0;
    }
    if (lt < rank && rank <= le) s_med = v;   // (every writer holds the same value)
  }
  __syncthreads();
  const double med = s_med;
  // ---- survivors and the slots at or below the level, both in slot order -----------------------------------------------------
  for (int32_t i = tid; i < n; i += kMlStageThreads) {
    const bool up = sh[i] > med;
    int32_t before = 0;   // slots before i on the same side of the level
    for (int32_t j = 0; j < i; ++j) before += (sh[j] > med) == up ? 1 : 0;
    if (up) {
      s_surv[before] = i;
      atomicAdd(&s_count, 1);
    } else {
      s_los[before] = i;
    }
  }
  __syncthreads();
  const int32_t s = s_count, stage = st.stage;
  const bool reached = med >= ru.gmax;
  const double Pnext = st.P * ((double)s / (double)n);
  const bool floor = !reached && s != 0 && (Pnext < eps || stage + 1 == PLAIDHIP_GSEA_ML_MAX_STAGES);
  const bool ends = reached || s == 0 || floor;
  const int32_t end_status = reached ? PLAIDHIP_GSEA_ML_ESTIMATED : (s == 0 ? PLAIDHIP_GSEA_ML_STALLED : PLAIDHIP_GSEA_ML_FLOOR);
  // ---- the trace ----------------------------------------------------------------------------------------------------------------
  if (tid == 0) {
    s_trace[(size_t)r * PLAIDHIP_GSEA_ML_MAX_STAGES + stage] = s;
    m_trace[(size_t)r * PLAIDHIP_GSEA_ML_MAX_STAGES + stage] = med;
  }
  if (h_trace != nullptr)
    for (int32_t i = tid; i < n; i += kMlStageThreads)
      h_trace[((size_t)r * PLAIDHIP_GSEA_ML_MAX_STAGES + stage) * n + i] = sh[i];
  // ---- the read-off of the sets this level reaches (all that are left when the ruler ends) -------------------------------------
  for (int32_t q = ru.set0 + tid; q < ru.set0 + ru.nset; q += kMlStageThreads) {
    if (lstar[q] >= 0) continue;
    const double ga = gamma[q];
    const bool got = med >= ga;
    if (!got && !ends) continue;
    int32_t c = 0;
    for (int32_t j = 0; j < n; ++j) c += sh[j] >= ga ? 1 : 0;
    lstar[q] = stage;
    cnt[q] = c;
    est[q] = got ? PLAIDHIP_GSEA_ML_ESTIMATED : end_status;
  }
  if (tid == 0) {
    GseaMlState nx;
    nx.stage = stage + 1;
    nx.ended = ends ? 1 : 0;
    nx.status = ends ? end_status : 0;
    nx.level = med;
    nx.P = ends ? st.P : Pnext;
    state[r] = nx;
    if (!ends) atomicAdd(unfinished, 1u);
  }
  if (ends) return;
  // ---- the j-th slot at or below the level takes the (j mod s)-th survivor ------------------------------------------------------
  const int32_t nlos = n - s;
  unsigned long long* Mr = maps + (size_t)r * n * nwg;
  const int64_t words = (int64_t)nlos * nwg;
  for (int64_t e = tid; e < words; e += kMlStageThreads) {
    const int32_t j = (int32_t)(e / nwg), w = (int32_t)(e - (int64_t)j * nwg);
    Mr[(size_t)s_los[j] * nwg + w] = Mr[(size_t)s_surv[j % s] * nwg + w];
  }
  for (int32_t j = tid; j < nlos; j += kMlStageThreads) Hr[s_los[j]] = sh[s_surv[j % s]];
}

constexpr const char* kMlTooManyGenes = "gsea_multilevel: %d genes (the walk's bitmap takes at most %d)";

}  // namespace

#define PH_GSEA_ML_PICK(LAUNCH)                                                   \
  do {                                                                            \
    if (weighted) {                                                               \
      if (score_type == PLAIDHIP_GSEA_POS) LAUNCH(true, PLAIDHIP_GSEA_POS);        \
      else if (score_type == PLAIDHIP_GSEA_NEG) LAUNCH(true, PLAIDHIP_GSEA_NEG);   \
      else LAUNCH(true, PLAIDHIP_GSEA_STD);                                       \
    } else {                                                                      \
      if (score_type == PLAIDHIP_GSEA_POS) LAUNCH(false, PLAIDHIP_GSEA_POS);       \
      else if (score_type == PLAIDHIP_GSEA_NEG) LAUNCH(false, PLAIDHIP_GSEA_NEG);  \
      else LAUNCH(false, PLAIDHIP_GSEA_STD);                                      \
    }                                                                             \
  } while (0)

int launch_gsea_ml_init(plaidhip_ctx* ctx, int weighted, int score_type, const GseaMlRuler* rulers, int32_t nr, int32_t n,
                        int32_t g, const double* Wpos, uint64_t seed, unsigned long long* maps, double* H) {
  if ((int64_t)nr * n == 0) return PLAIDHIP_OK;
  if (const int rc = check_walk_genes(kMlTooManyGenes, g)) return rc;
  const int64_t tasks = (int64_t)nr * n;
  const WalkLaunch wl = walk_launch((tasks + kMlWaves - 1) / kMlWaves, (int64_t)ctx->num_cu * 16, kMlWaves, g);
  const int32_t nwg = gsea_ml_map_words(g);
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32);
#define PH_ML_INIT(W, ST)                                                                                                       \
  do {                                                                                                                          \
    PH_FULL_LDS(ctx, (gsea_ml_init_kernel<W, ST>));                                                                             \
    hipLaunchKernelGGL((gsea_ml_init_kernel<W, ST>), dim3(wl.blocks), dim3(64 * kMlWaves), wl.shmem, ctx->stream, rulers, nr, n, g, \
                       Wpos, k0, k1, maps, H, nwg, wl.nw64);                                                                     \
  } while (0)
  PH_GSEA_ML_PICK(PH_ML_INIT);
#undef PH_ML_INIT
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_gsea_ml_mutate(plaidhip_ctx* ctx, int weighted, int score_type, const GseaMlRuler* rulers, const GseaMlState* state,
                          int32_t nr, int32_t n, int32_t g, const double* Wpos, uint64_t seed, int32_t sweeps,
                          unsigned long long* maps, double* H) {
  if ((int64_t)nr * n == 0) return PLAIDHIP_OK;
  if (const int rc = check_walk_genes(kMlTooManyGenes, g)) return rc;
  const int64_t tasks = (int64_t)nr * n;
  const WalkLaunch wl = walk_launch((tasks + kMlWaves - 1) / kMlWaves, (int64_t)ctx->num_cu * 16, kMlWaves, g);
  const int32_t nwg = gsea_ml_map_words(g);
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32);
#define PH_ML_MUTATE(W, ST)                                                                                                     \
  do {                                                                                                                          \
    PH_FULL_LDS(ctx, (gsea_ml_mutate_kernel<W, ST>));                                                                           \
    hipLaunchKernelGGL((gsea_ml_mutate_kernel<W, ST>), dim3(wl.blocks), dim3(64 * kMlWaves), wl.shmem, ctx->stream, rulers, state, \
                       nr, n, g, Wpos, k0, k1, sweeps, maps, H, nwg, wl.nw64);                                                   \
  } while (0)
  PH_GSEA_ML_PICK(PH_ML_MUTATE);
#undef PH_ML_MUTATE
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

int launch_gsea_ml_stage(plaidhip_ctx* ctx, const GseaMlRuler* rulers, GseaMlState* state, int32_t nr, int32_t n, int32_t g,
                         double eps, unsigned long long* maps, double* H, int32_t* s_trace, double* m_trace, double* h_trace,
                         const double* gamma, int32_t* lstar, int32_t* cnt, int32_t* est, uint32_t* unfinished) {
  if (nr == 0) return PLAIDHIP_OK;
  hipLaunchKernelGGL(gsea_ml_stage_kernel, dim3((unsigned)nr), dim3(kMlStageThreads), 0, ctx->stream, rulers, state, n, eps, maps,
                     H, gsea_ml_map_words(g), s_trace, m_trace, h_trace, gamma, lstar, cnt, est, unfinished);
  PH_HIP(hipGetLastError());
  return PLAIDHIP_OK;
}

}  // namespace plaidhip
