// plaid.fisher's upper hypergeometric tail and odds ratio as pinned in include/plaidhip.h (plaidhip_fisher), once, for the
// device (kernels_fisher.hip: fisher_tail_kernel) and the host (plaidhip_hyper_tail).  fp64 and 64-bit integers only: no
// pow, lgamma or exp, and no contracted product (the including file is also compiled with -ffp-contract=off).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define PH_TAIL_HD __host__ __device__
#else
#define PH_TAIL_HD
#endif

namespace plaidhip {

// p = P(X >= x), X ~ Hypergeometric(N, K, k): 0 <= K, k <= N <= 2^26, any x.  The terms are ratios to the term at t0 (near
// the mode), walked upwards then downwards; a term that underflows to 0 stays 0, so leaving a walk there adds the same bits.
PH_TAIL_HD inline double hyper_tail(int64_t N, int64_t K, int64_t k, int64_t x) {
#pragma clang fp contract(off)
  const int64_t lo = k + K - N > 0 ? k + K - N : 0;
  const int64_t hi = k < K ? k : K;
  if (x <= lo) return 1.0;
  if (x > hi) return 0.0;
  int64_t t0 = ((k + 1) * (K + 1)) / (N + 2);
  t0 = t0 < lo ? lo : (t0 > hi ? hi : t0);
  const int64_t r = N - K - k;   // (N - K - k + t >= 1 wherever it divides: t + 1 > lo)
  double u = 1.0, total = 1.0, upper = t0 >= x ? 1.0 : 0.0;
  for (int64_t t = t0; t < hi; ++t) {
    u = (u * ((double)(K - t) * (double)(k - t))) / ((double)(t + 1) * (double)(r + t + 1));
    if (u == 0.0) break;
    total += u;
    if (t + 1 >= x) upper += u;
  }
  u = 1.0;
  for (int64_t t = t0; t > lo; --t) {
    u = (u * ((double)t * (double)(r + t))) / ((double)(K - t + 1) * (double)(k - t + 1));
    if (u == 0.0) break;
    total += u;
    if (t - 1 >= x) upper += u;
  }
  return upper / total;
}

// the sample odds ratio (a d) / (b c') of the table a = x, b = k - x, c' = K - x, d = N - k - K + x; IEEE: x / 0 = Inf,
// 0 / 0 = NaN.  Both products are exact below 2^53.
PH_TAIL_HD inline double fisher_odds(int64_t N, int64_t K, int64_t k, int64_t x) {
#pragma clang fp contract(off)
  return ((double)x * (double)(N - k - K + x)) / ((double)(k - x) * (double)(K - x));
}

}  // namespace plaidhip
