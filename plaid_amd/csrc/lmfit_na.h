// plaid.limma with na = "fit": the refit of one row on the samples it has, as pinned in include/plaidhip.h
// (plaidhip_limma_na), once, for the device (kernels_lmfit.hip: lmfit_na_solve_kernel) and the host
// (plaidhip_limma_na_solve).  In the coordinates gamma = R_f beta the row's least-squares problem is H gamma = E' with
// H = I - sum over its missing samples of q_c q_c' (DESIGN.md section 24).  fp64 only, every product inside an fma that is
// written out, and no contracted one (the including file is also compiled with -ffp-contract=off).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PH_LMNA_HD __host__ __device__
#else
#define PH_LMNA_HD
#endif

#define PLAIDHIP_LMNA_PIVOT_MIN 1e-10   // a Cholesky pivot at or below it: the row is not estimable in the fit
#define PLAIDHIP_LMW_PIVOT_REL 1e-10    // the weighted fit (plaidhip_limma_w): at or below it times H_kk, the diagonal before elimination

namespace plaidhip {

// One step of an entry's chain of the downdate: s = fma(q_ck, q_cl, s).  The device runs it lane by lane over a pair's missing
// samples (kernels_lmfit.hip), the host through lmfit_na_gram_chain.
PH_LMNA_HD inline double lmfit_na_gram_step(double qk, double ql, double s) {
#pragma clang fp contract(off)
  return fma(qk, ql, s);
}

// One entry of the downdate: the chain from 0.0 over the missing samples in the order given; qk / ql point at entry k / l
// of the first missing sample's row of Q_f, `stride` doubles from row to row.
PH_LMNA_HD inline double lmfit_na_gram_chain(const double* qk, const double* ql, int64_t stride, int64_t nmis) {
  double s = 0.0;
  for (int64_t i = 0; i < nmis; ++i) s = lmfit_na_gram_step(qk[i * stride], ql[i * stride], s);
  return s;
}

// H (p x p, row-major with leading dimension ld; the lower triangle is read) -> L in its place, H = L L', Cholesky without
// pivoting, row by row, every inner sum in ascending order; then L y = e and L' gamma = y.  e: p values; gamma: p values
// (may be e).  Returns false -- and leaves gamma unwritten -- when a pivot d_k is <= the threshold or NaN.  The threshold is
// `tol` itself (relative == false: na = "fit", whose H is I minus a downdate) or tol * H_kk, one rounded product with the
// diagonal entry before elimination (relative == true: the weighted fit, whose H scales with the weights).  piv (may be
// null): the pivots d_k as far as the factorisation went.
PH_LMNA_HD inline bool lmfit_na_factor_solve(int p, double* H, int ld, const double* e, double* gamma, double* piv, double tol,
                                             bool relative) {
#pragma clang fp contract(off)
  for (int k = 0; k < p; ++k) {
    for (int l = 0; l < k; ++l) {
      double s = H[k * ld + l];
      for (int m = 0; m < l; ++m) s = fma(-H[k * ld + m], H[l * ld + m], s);
      H[k * ld + l] = s / H[l * ld + l];
    }
    const double hkk = H[k * ld + k];
    double d = hkk;
    for (int m = 0; m < k; ++m) d = fma(-H[k * ld + m], H[k * ld + m], d);
    if (piv != nullptr) piv[k] = d;
    const double least = relative ? tol * hkk : tol;
    if (!(d > least)) return false;
    H[k * ld + k] = sqrt(d);
  }
  for (int k = 0; k < p; ++k) {   // forward: y in gamma
    double s = e[k];
    for (int m = 0; m < k; ++m) s = fma(-H[k * ld + m], gamma[m], s);
    gamma[k] = s / H[k * ld + k];
  }
  for (int k = p - 1; k >= 0; --k) {   // back, the sum over m > k ascending
    double s = gamma[k];
    for (int m = k + 1; m < p; ++m) s = fma(-H[m * ld + k], gamma[m], s);
    gamma[k] = s / H[k * ld + k];
  }
  return true;
}

// stdev.unscaled of one contrast of the row: w = L^-1 v_j by forward substitution, u = sqrt(sum_k w_k^2) ascending from 0.0.
// L as lmfit_na_factor_solve left it; w: p doubles of scratch.
PH_LMNA_HD inline double lmfit_na_unscaled(int p, const double* L, int ld, const double* vj, double* w) {
#pragma clang fp contract(off)
  double s2 = 0.0;
  for (int k = 0; k < p; ++k) {
    double s = vj[k];
    for (int m = 0; m < k; ++m) s = fma(-L[k * ld + m], w[m], s);
    w[k] = s / L[k * ld + k];
    s2 = fma(w[k], w[k], s2);
  }
  return sqrt(s2);
}

// AveExpr of an incomplete row: the mean over its observed samples from M' = sum over them of x_c * (1 / n_f)
PH_LMNA_HD inline double lmfit_na_mean(double Mp, double nf, double nobs) {
#pragma clang fp contract(off)
  return (Mp * nf) / nobs;
}

// The weighted fit of one (row, fit) pair (include/plaidhip.h: plaidhip_limma_w), once for the device (kernels_lmfit_w.hip:
// lmfit_w_solve_kernel) and the host (plaidhip_limma_w_solve).  H: p x p with leading dimension ld, its lower triangle holds
// the weighted Gram sums on entry and L on return; g: b on entry, gamma on return; nlive: the live observations.  u[j *
// ustride] takes stdev.unscaled of contrast j (v: p x q); w: p doubles of scratch.  Not estimable (a pivot at or below
// PLAIDHIP_LMW_PIVOT_REL H_kk or NaN, or nlive - p < 1): false; u is not written, and g holds nothing to be used (gamma where only the
// degrees of freedom were missing, b otherwise): the callers write NaN.
PH_LMNA_HD inline bool lmfit_w_row_solve(int p, double* H, int ld, double* g, double nlive, const double* v, int q, double* u,
                                         int64_t ustride, double* w, double* piv) {
  const bool ok = lmfit_na_factor_solve(p, H, ld, g, g, piv, PLAIDHIP_LMW_PIVOT_REL, true) && nlive - (double)p >= 1.0;
  if (!ok) return false;
  for (int j = 0; j < q; ++j) u[j * ustride] = lmfit_na_unscaled(p, H, ld, v + (int64_t)j * p, w);
  return true;
}

}  // namespace plaidhip
