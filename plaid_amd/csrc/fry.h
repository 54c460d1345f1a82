// plaid.fry: the standardised residual of one (gene, sample) as pinned in include/plaidhip.h (plaidhip_fry, step 2), once,
// for the device (kernels_fry.hip: fry_residual_kernel) and the host (plaidhip_fry_residual_row).  The chain is camera's
// (camera.h: camera_chain_step); the divisor c_g is given, not derived: the posterior sd needs the prior of ALL genes, which
// the host makes after the RSS chain (stats.cpp: fry_divisors).  One IEEE division per element, no reciprocal.
#pragma once

#include "camera.h"

#define PLAIDHIP_FRY_STANDARDIZE_POSTERIOR 0
#define PLAIDHIP_FRY_STANDARDIZE_RESIDUAL 1
#define PLAIDHIP_FRY_STANDARDIZE_NONE 2

namespace plaidhip {

// is the gene inside the fit's universe: a divisor that is finite and not 0 (fry_divisors writes NaN for every other gene)
PH_CAM_HD inline bool fry_in_universe(double c) { return c - c == 0.0 && c != 0.0; }

// z'_gc: `used` = the sample takes part in the fit; c = the gene's divisor
PH_CAM_HD inline double fry_standardise(double r, double c, bool used) { return used && fry_in_universe(c) ? r / c : 0.0; }

}  // namespace plaidhip
