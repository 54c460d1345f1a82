// The walk of plaid.gsea over one wavefront's map and its Philox4x32-10, shared by kernels_gsea.hip
// (the observed scores, the permutation null, the leading edges) and kernels_gsea_ml.hip (the multilevel chains): one
// statement of the score, so a chain's h(S) has the bits of the observed ES of the same members.
//
// The pinned form holds no contracted product: include this header AFTER `#pragma clang fp contract(off)` (both files
// are also compiled with -ffp-contract=off).
#pragma once

#include "bitmap_walk.h"

namespace plaidhip {

// ---- Philox4x32-10 (Salmon et al., SC'11): counter (i, b, 0, 0), key (seed lo, seed hi) ------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t* o) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// where the walk met its extremes (the leading edge): t_top the smallest t with after_t == maxP, t_bot the smallest t with
// before_t == minP (both 1-based), and the members the map holds
struct GnExtremes {
  double maxP, minP;
  uint32_t t_top, t_bot, members;
};

// ES of the set whose bits are in the map: max(after), min(before) over the members, the choice between them that the score
// type ST pins (PLAIDHIP_GSEA_STD / _POS / _NEG; launch-uniform, a template parameter so that an instantiation carries the
// extreme it needs and no other).  EDGE: the walk also carries the t of each extreme -- (value, t) pairs, the smaller t on
// equal values -- leaves every word's exclusive member count in `prefix` (LDS, beside the map) and returns the extremes in
// *ex.  The values are formed by the same operations either way, so maxP / minP of an EDGE walk have the bits behind ES.
template <bool WEIGHTED, int ST, bool EDGE = false>
__device__ __forceinline__ double gn_walk(unsigned long long* bm, int32_t nw64, const double* __restrict__ wp, double B,
                                          int32_t N, int32_t k, bool clear, int lane, uint32_t* prefix = nullptr,
                                          GnExtremes* ex = nullptr) {
  const double dmiss = (double)(N - k);
  double mxp = -INFINITY, mnp = INFINITY;   // no pos >= 2 rule: before_1 = 0 takes part
  uint32_t tmx = 0xffffffffu, tmn = 0xffffffffu;   // (EDGE) a lane's t only grows, so a strict update keeps its first
  if constexpr (EDGE) __builtin_assume(prefix != nullptr);
  const uint32_t members = walk_scan<WEIGHTED>(bm, nw64, wp, clear, lane, EDGE ? prefix : nullptr,
                                               [&](int32_t pos, uint32_t t, double cwprev, double cwt) {
    const double miss = (double)(pos - (int32_t)t) / dmiss;
    const double before = cwprev / B - miss;
    const double after = cwt / B - miss;
    if constexpr (EDGE) {
      if (before < mnp) { mnp = before; tmn = t; }
      if (after > mxp) { mxp = after; tmx = t; }
    } else {
      mnp = before < mnp ? before : mnp;
      mxp = after > mxp ? after : mxp;
    }
  });
  if constexpr (EDGE) {
    // lanes own different words and the outer loop different chunks of 64 words, so equal values can sit in any two
    // lanes: the tie is settled here, by t, and every lane ends with the same pair
    for (int o = 32; o >= 1; o >>= 1) {
      const double a = __shfl_xor(mxp, o), b = __shfl_xor(mnp, o);
      const uint32_t ta = (uint32_t)__shfl_xor((int)tmx, o), tb = (uint32_t)__shfl_xor((int)tmn, o);
      if (a > mxp || (a == mxp && ta < tmx)) { mxp = a; tmx = ta; }
      if (b < mnp || (b == mnp && tb < tmn)) { mnp = b; tmn = tb; }
    }
    ex->maxP = mxp;
    ex->minP = mnp;
    ex->t_top = tmx;
    ex->t_bot = tmn;
    ex->members = members;
  } else {
    for (int o = 32; o >= 1; o >>= 1) {   // (an extreme the score type does not read is dropped by the compiler)
      const double a = __shfl_xor(mxp, o), b = __shfl_xor(mnp, o);
      mxp = a > mxp ? a : mxp;
      mnp = b < mnp ? b : mnp;
    }
  }
  if (ST == PLAIDHIP_GSEA_POS) return mxp;
  if (ST == PLAIDHIP_GSEA_NEG) return mnp;
  return mxp > -mnp ? mxp : (mxp < -mnp ? mnp : 0.0);
}

// the score of the set in the map under one list's weights; B == 0: the unweighted walk
template <bool WEIGHTED, int ST>
__device__ __forceinline__ double gn_score(unsigned long long* bm, int32_t nw64, const double* __restrict__ wp, int32_t N,
                                           int32_t k, bool clear, int lane) {
  if (WEIGHTED) {
    const double B = walk_total_weight(bm, nw64, wp, lane);
    if (B != 0.0) return gn_walk<true, ST>(bm, nw64, wp, B, N, k, clear, lane);
  }
  return gn_walk<false, ST>(bm, nw64, wp, (double)k, N, k, clear, lane);
}

}  // namespace plaidhip
