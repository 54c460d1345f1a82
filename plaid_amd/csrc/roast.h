// plaid.roast: the rotated moderated statistic and its z-score of one (gene, rotation) as pinned in include/plaidhip.h
// (plaidhip_roast, steps 3 and 4), once, for the device (kernels_roast.hip) and for the host entries that restate them.
// fp64 only; the including files are compiled with -ffp-contract=off, so every operation below is rounded on its own and the
// only fused ones are the fma of the chain, written out.
#pragma once

#include "camera.h"

#define PLAIDHIP_ROAST_STAT_MEAN 0
#define PLAIDHIP_ROAST_STAT_FLOORMEAN 1
#define PLAIDHIP_ROAST_STAT_MSQ 2
#define PLAIDHIP_ROAST_STAT_MEAN50 3
#define PLAIDHIP_ROAST_ZSCORE_HILL 0
#define PLAIDHIP_ROAST_ZSCORE_NONE 1

namespace plaidhip {

// the fit's scalars of steps 3 and 4: d = n_f - p, the prior (df0, s0^2) of limma_squeeze_fit, nu = min(df0 + d, 10,000)
struct RoastFit { double d, df0, s02, nu; };

PH_CAM_HD inline RoastFit roast_fit(double d, double df0, double s02) {
  const double tot = df0 + d;
  return RoastFit{d, df0, s02, tot < 1e4 ? tot : 1e4};
}

// sqrt(q) for q = qchisq(0.5, 1) = 0.454936423119572...: floormean's floor of |z|
#define PLAIDHIP_ROAST_SQRT_Q 0.67448975019608171

// one step of B's chain: acc = fma(r_gc, w_c, acc), ascending c from beta r0
PH_CAM_HD inline double roast_chain_step(double r, double w, double acc) {
#pragma clang fp contract(off)
  return fma(r, w, acc);
}

// step 3 after the chain: the moderated t of the rotated effects from B, beta and the gene's RSS
PH_CAM_HD inline double roast_moderated_t(double B, double beta, double rss, const RoastFit& f) {
#pragma clang fp contract(off)
  const double bb = beta * beta;
  const double tot = bb + rss;
  const double BB = B * B;
  const double rest = tot - BB;
  const double q = rest / f.d;
  const double s2r = q > 0.0 ? q : 0.0;
  double post;
  if (!(f.df0 - f.df0 == 0.0)) {
    post = f.s02;                      // an infinite prior df
  } else if (f.df0 == 0.0) {
    post = s2r;                        // no prior (fewer than two ok genes), as limma_squeeze_fit
  } else {
    const double a = f.df0 * f.s02;
    const double b = f.d * s2r;
    const double num = a + b;
    post = num / (f.df0 + f.d);
  }
  return B / sqrt(post);
}

// step 4: Hill's (1970) normal score of a t on nu degrees of freedom
PH_CAM_HD inline double roast_hill_z(double t, double nu) {
#pragma clang fp contract(off)
  const double A = nu - 0.5;
  const double C = 48.0 * A * A;
  const double tt = t * t;
  const double y = A * log1p(tt / nu);
  double pol = -0.4 * y - 3.3;
  pol = pol * y - 24.0;
  pol = pol * y - 85.5;
  const double y2 = 0.8 * y * y;
  const double den = (y2 + 100.0) + C;
  const double in = (y + 3.0) + pol / den;
  const double mag = sqrt(y) * (1.0 + in / C);
  return t < 0.0 ? -mag : mag;
}

PH_CAM_HD inline double roast_zscore(double t, double nu, int zscore) {
  return zscore == PLAIDHIP_ROAST_ZSCORE_HILL ? roast_hill_z(t, nu) : t;
}

// mean50 on the device: the sets run in three size classes, so that the small ones do not pay for the LDS of the large.
// Class 0: at most 40 members, 1: at most 128, 2: up to PLAIDHIP_ROAST_MEAN50_MAX (and the sets above it, which get NaN).
// A class's LDS holds z of up to 64 rotations at an odd stride of its largest set.
inline int roast_mean50_class(int32_t members) { return members <= 40 ? 0 : members <= 128 ? 1 : 2; }
inline int32_t roast_mean50_class_doubles(int cls) { return cls == 0 ? 64 * 41 : cls == 1 ? 64 * 129 : 16384 + 1; }

// a double as an unsigned key with the order of the doubles (-0.0 below +0.0, NaN of either sign at the ends), and back
PH_CAM_HD inline uint64_t roast_order_key(double x) {
  uint64_t u;
  __builtin_memcpy(&u, &x, 8);
  return (u >> 63) != 0 ? ~u : u ^ 0x8000000000000000ull;
}
PH_CAM_HD inline double roast_key_value(uint64_t k) {
  const uint64_t u = (k >> 63) != 0 ? k ^ 0x8000000000000000ull : ~k;
  double x;
  __builtin_memcpy(&x, &u, 8);
  return x;
}

// mean50's key of side 0 (up), 1 (down), 2 (mixed); the added 0.0 turns -0.0 into +0.0, so that equal keys have equal bits
PH_CAM_HD inline double roast_mean50_key(double z, int side) {
#pragma clang fp contract(off)
  // selects of values, no branch on `side`: (|z| or z) times (-1 or 1), both exact, then the added 0.0
  const double v = side == 2 ? fabs(z) : z;
  const double sg = side == 1 ? -1.0 : 1.0;
  return v * sg + 0.0;
}

}  // namespace plaidhip
