// The bitmap walk of the exact scorers, once: gsea_ks_kernel / gsva_ks_kernel (kernels_ks.hip), the
// plaid.gsea kernels (kernels_gsea.hip) and, for the map alone, sing_mad_kernel (kernels_sing.hip).
//
// One wavefront per (set, column) pair.  The positions of a column's genes are distinct integers in 0..N-1, so the wavefront
// sets bit `position` of an N-bit map in LDS for every member and scans the 64-bit words in order, 64 words at a time: the
// wavefront prefix sum of the popcounts gives t (the member's place in the walk) of every set bit, the bit's index gives
// pos = position + 1.  With weights, wp[position] is the weight of the gene that stands there and cw_t = w_1 + ... + w_t a
// wavefront prefix sum over the lanes' words.  Cost per pair: k + N / 64 LDS words, whatever the set size.
//
// A kernel supplies: the functor that places a member (walk_set_bits), the visitor that takes a hit (walk_scan) and what it
// makes of the candidates.  The candidates themselves -- cw / B - miss, / N -- are formed in the visitors, in the kernels'
// own files: those files differ in fp contraction, and this header holds no expression of the form a * b +- c, so it means
// the same under both.  The additions of walk_scan and walk_total_weight and their association are part of the pinned
// results: s per word in bit order, the inclusive lane scan, cwbase + exclusive, cwbase += the last lane's.
#pragma once

#include <algorithm>

#include "common.h"
#include "rank_bucket.h"

namespace plaidhip {

__device__ __forceinline__ void walk_wave_sync() {   // LDS written by the wavefront's lanes is read by its other lanes
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 64-bit words of one wavefront's map of g bits: a multiple of 64 (the scan's chunk), at most 64 * 32 at
// PLAIDHIP_GSEA_KS_MAX_GENES
inline int32_t walk_map_words(int32_t g) { return (int32_t)((((int64_t)g + 63) / 64 + 63) / 64 * 64); }

__device__ __forceinline__ void walk_zero_map(unsigned long long* bm, int32_t nw64, int lane) {
  for (int32_t i = lane; i < nw64; i += 64) bm[i] = 0ull;
}

// the bit bit_of(row) of the map for every member of the set Gi[p0 .. p0 + k) (in list order, a lane per member); a row or
// a bit outside 0..N-1 is passed over
template <typename BitOf>
__device__ __forceinline__ void walk_set_bits(unsigned long long* bm, const int32_t* __restrict__ Gi, int32_t p0, int32_t k,
                                              int32_t N, int lane, BitOf bit_of) {
  uint32_t* bm32 = reinterpret_cast<uint32_t*>(bm);
  for (int32_t i = lane; i < k; i += 64) {
    const int32_t row = Gi[p0 + i];
    if ((uint32_t)row >= (uint32_t)N) continue;
    const int32_t b = bit_of(row);
    if ((uint32_t)b < (uint32_t)N) atomicOr(&bm32[b >> 5], 1u << (b & 31));
  }
}

// B = the weight of the set's members, by a pass over the map that adds the words' weights as walk_scan adds them to its
// base (the inclusive scan's last lane holds the sum tree of an ascending butterfly): B depends on the positions alone,
// not on the order of the set's member list
__device__ __forceinline__ double walk_total_weight(const unsigned long long* bm, int32_t nw64, const double* __restrict__ wp,
                                                    int lane) {
  double B = 0.0;
  for (int32_t w0 = 0; w0 < nw64; w0 += 64) {
    const unsigned long long word = bm[w0 + lane];
    if (__ballot(word != 0ull) == 0ull) continue;
    const int32_t pos0 = (w0 + lane) * 64;
    double s = 0.0;
    for (unsigned long long wd = word; wd != 0ull; wd &= wd - 1ull) s += wp[pos0 + (__ffsll((long long)wd) - 1)];
    for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
    B += __shfl(s, 63);
  }
  return B;
}

// The walk over the set bits, 64 words at a time.  Every hit: visit(pos, t, cwprev, cwt) with pos the 1-based position, t
// the member's 1-based place, cwprev = cw_{t-1} and cwt = cw_t (t - 1 and t when not WEIGHTED; wp is not read then).
// clear: the words read are zeroed, so the map is empty again when the scan returns.  prefix (nullable): every word's
// exclusive member count, for the words of the chunks that hold a member.  Returns the members the map held.
template <bool WEIGHTED, typename Visit>
__device__ __forceinline__ uint32_t walk_scan(unsigned long long* bm, int32_t nw64, const double* __restrict__ wp, bool clear,
                                              int lane, uint32_t* prefix, Visit visit) {
  uint32_t tbase = 0u;     // members in the words already walked
  double cwbase = 0.0;     // their weight
  for (int32_t w0 = 0; w0 < nw64; w0 += 64) {
    unsigned long long word = bm[w0 + lane];
    if (__ballot(word != 0ull) == 0ull) continue;
    if (clear) bm[w0 + lane] = 0ull;
    const uint32_t cnt = (uint32_t)__popcll(word);
    const uint32_t incl = wave_incl_scan_u32(cnt);
    uint32_t t = tbase + incl - cnt;
    tbase += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (prefix != nullptr) prefix[w0 + lane] = t;
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
      visit(pos, t, cwprev, WEIGHTED ? cw : (double)t);
    }
  }
  return tbase;
}

// ---- host geometry -------------------------------------------------------------------------------------------------------
struct WalkLaunch {
  unsigned blocks;
  size_t shmem;    // `waves` maps, with `extra` bytes beside every word: at most 64 KB (96 KB with 4 extra bytes) at
  int32_t nw64;    // PLAIDHIP_GSEA_KS_MAX_GENES and four wavefronts
};

inline WalkLaunch walk_launch(int64_t tasks, int64_t max_blocks, int waves, int32_t g, int extra = 0) {
  const int32_t nw64 = walk_map_words(g);
  return WalkLaunch{(unsigned)std::max<int64_t>(1, std::min<int64_t>(tasks, max_blocks)), (size_t)waves * nw64 * (8 + extra), nw64};
}

// the map bounds the rows; `text`: the caller's refusal, with %d for g and for the bound
inline int check_walk_genes(const char* text, int32_t g) {
  if (g <= PLAIDHIP_GSEA_KS_MAX_GENES) return PLAIDHIP_OK;
  set_error(text, g, PLAIDHIP_GSEA_KS_MAX_GENES);
  return PLAIDHIP_EUNSUPPORTED;
}

}  // namespace plaidhip
