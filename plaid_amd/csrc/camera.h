// plaid.camera: the standardised residual of one (gene, sample), as pinned in include/plaidhip.h (plaidhip_camera, step 2),
// once, for the device (kernels_camera.hip: camera_residual_kernel) and the host (plaidhip_camera_residual_row).  fp64 only;
// the only fused operation is the fma written out (the including files are also compiled with -ffp-contract=off), one
// IEEE square root per gene and one IEEE division per element -- never a multiplication by a reciprocal.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PH_CAM_HD __host__ __device__
#else
#define PH_CAM_HD
#endif

#define PLAIDHIP_CAMERA_S2_FLOOR 1e-8   // z = r / sqrt(max(s2, floor)): a gene that fits exactly has z = r * 1e4, not Inf

namespace plaidhip {

// One step of the residual's chain: r = fma(-Q_f[c, k], E_k, r), run in ascending k from x_c (step 2 of plaidhip_limma).
PH_CAM_HD inline double camera_chain_step(double qck, double ek, double r) {
#pragma clang fp contract(off)
  return fma(-qck, ek, r);
}

// The gene's divisor from its residual sum of squares and d = n_f - p: s2 = rss / d, then sqrt(max(s2, floor)).  A gene that
// is not ok in the fit (s2 not finite) returns NaN: every z of it is 0.0.
PH_CAM_HD inline double camera_gene_scale(double rss, double d) {
  const double s2 = rss / d;
  if (!(s2 - s2 == 0.0)) return s2 - s2;   // (NaN for NaN and for +-Inf)
  return sqrt(s2 > PLAIDHIP_CAMERA_S2_FLOOR ? s2 : PLAIDHIP_CAMERA_S2_FLOOR);
}

// z_gc: `used` = the sample takes part in the fit; scale = camera_gene_scale of the gene
PH_CAM_HD inline double camera_standardise(double r, double scale, bool used) { return used && scale == scale ? r / scale : 0.0; }

}  // namespace plaidhip
