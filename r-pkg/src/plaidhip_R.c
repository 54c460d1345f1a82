/* .Call() shim between R and the C ABI of include/plaidhip.h.
 *
 * Argument unpacking only: every number is produced by libplaidhip.so.  Not compiled in the
 * build container (R is absent there); it needs only R's headers and -lplaidhip.
 * Error contract: the C ABI never throws or longjmps; a non-zero status is turned into
 * Rf_error() here, after the library call has returned (no C++ frames to unwind).
 * Threading: .Call arrives on R's main thread; the library synchronises before returning.
 */
#include <R.h>
#include <Rinternals.h>
#include <R_ext/Rdynload.h>

#include <string.h>

#include "plaidhip.h"

static plaidhip_ctx* g_ctx = NULL;
static int g_device = 0;

static plaidhip_ctx* ctx(void) {
  if (g_ctx == NULL) {
    int rc = plaidhip_init(g_device, NULL, &g_ctx);
    if (rc != PLAIDHIP_OK) Rf_error("plaidhip: %s", plaidhip_last_error_string());
  }
  return g_ctx;
}

static void check(int rc) {
  if (rc != PLAIDHIP_OK) Rf_error("plaidhip: %s", plaidhip_last_error_string());
}

/* options(plaidhip.device, plaidhip.precision): called by every R wrapper before its .Call.  A changed device
 * closes the session context (the next call opens one on the new device). */
SEXP R_plaidhip_session(SEXP device, SEXP precision) {
  const int d = Rf_asInteger(device);
  if (d != g_device && g_ctx != NULL) { plaidhip_finalize(g_ctx); g_ctx = NULL; }
  g_device = d;
  check(plaidhip_set_precision(ctx(), Rf_asInteger(precision)));
  check(plaidhip_multi_set_precision(Rf_asInteger(precision)));   /* options(plaidhip.devices) with several GPUs */
  return R_NilValue;
}

/* plaid(): X numeric matrix g x n; Gp/Gi integer vectors = aligned membership pattern in
 * X's row space (built in R/plaid-hip.R); returns an m x n numeric matrix. */
SEXP R_plaidhip_plaid_dense(SEXP X, SEXP Gp, SEXP Gi, SEXP stat, SEXP normalize) {
  const int g = Rf_nrows(X), n = Rf_ncols(X), m = LENGTH(Gp) - 1;
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, n));
  check(plaidhip_plaid_dense(ctx(), REAL(X), g, n, INTEGER(Gp), INTEGER(Gi), m, Rf_asInteger(stat),
                             Rf_asLogical(normalize), REAL(S)));
  UNPROTECT(1);
  return S;
}

/* same for a dgCMatrix: slots @p, @i, @x and nrow */
SEXP R_plaidhip_plaid_csc(SEXP Xp, SEXP Xi, SEXP Xx, SEXP g, SEXP Gp, SEXP Gi, SEXP stat, SEXP normalize) {
  const int n = LENGTH(Xp) - 1, m = LENGTH(Gp) - 1;
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, n));
  check(plaidhip_plaid_csc(ctx(), INTEGER(Xp), INTEGER(Xi), REAL(Xx), Rf_asInteger(g), n, INTEGER(Gp),
                           INTEGER(Gi), m, Rf_asInteger(stat), Rf_asLogical(normalize), REAL(S)));
  UNPROTECT(1);
  return S;
}

/* chunked_crossprod(x, y) with a general sparse x (stored values differ inside a column): x as its dgCMatrix slots,
 * y a numeric matrix (R/plaid.R:107, :117: Matrix::crossprod(x, y[, jj])) */
SEXP R_plaidhip_crossprod_weighted_dense(SEXP Wp, SEXP Wi, SEXP Wx, SEXP Y) {
  const int g = Rf_nrows(Y), n = Rf_ncols(Y), m = LENGTH(Wp) - 1;
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, n));
  check(plaidhip_crossprod_weighted_dense(ctx(), INTEGER(Wp), INTEGER(Wi), REAL(Wx), g, m, REAL(Y), n, REAL(S)));
  UNPROTECT(1);
  return S;
}

/* same for a dgCMatrix y: slots @p, @i, @x and nrow */
SEXP R_plaidhip_crossprod_weighted_csc(SEXP Wp, SEXP Wi, SEXP Wx, SEXP Yp, SEXP Yi, SEXP Yx, SEXP g) {
  const int n = LENGTH(Yp) - 1, m = LENGTH(Wp) - 1;
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, n));
  check(plaidhip_crossprod_weighted_csc(ctx(), INTEGER(Wp), INTEGER(Wi), REAL(Wx), Rf_asInteger(g), m, INTEGER(Yp),
                                        INTEGER(Yi), REAL(Yx), n, REAL(S)));
  UNPROTECT(1);
  return S;
}

/* replaid.sing for a dgCMatrix: slots @p, @i, @x and nrow (no as.matrix(X) on the host) */
SEXP R_plaidhip_sing_csc(SEXP Xp, SEXP Xi, SEXP Xx, SEXP g, SEXP Gp, SEXP Gi) {
  const int n = LENGTH(Xp) - 1, m = LENGTH(Gp) - 1;
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, n));
  check(plaidhip_sing_csc(ctx(), INTEGER(Xp), INTEGER(Xi), REAL(Xx), Rf_asInteger(g), n, INTEGER(Gp), INTEGER(Gi), m,
                          REAL(S)));
  UNPROTECT(1);
  return S;
}

/* normalize_medians(x, ignore.zero): ignore_zero = NA (NULL in R) / FALSE / TRUE */
SEXP R_plaidhip_normalize_medians(SEXP x, SEXP ignore_zero) {
  const int m = Rf_nrows(x), n = Rf_ncols(x);
  SEXP S = PROTECT(Rf_duplicate(x));
  const int iz = Rf_asLogical(ignore_zero);
  check(plaidhip_normalize_medians(ctx(), REAL(S), m, n, iz == NA_LOGICAL ? PLAIDHIP_IGNORE_ZERO_AUTO : iz, NULL));
  UNPROTECT(1);
  return S;
}

SEXP R_plaidhip_colranks_dense(SEXP X, SEXP ties, SEXP is_signed) {
  const int g = Rf_nrows(X), n = Rf_ncols(X);
  SEXP R = PROTECT(Rf_allocMatrix(REALSXP, g, n));
  check(plaidhip_colranks_dense(ctx(), REAL(X), g, n, Rf_asInteger(ties), Rf_asLogical(is_signed), REAL(R)));
  UNPROTECT(1);
  return R;
}

/* sparse_colranks(): returns the new @x vector; the caller keeps @i/@p (R/plaid.R:645-646) */
SEXP R_plaidhip_colranks_csc(SEXP Xp, SEXP Xx, SEXP ties, SEXP is_signed) {
  const int n = LENGTH(Xp) - 1;
  SEXP R = PROTECT(Rf_allocVector(REALSXP, XLENGTH(Xx)));
  check(plaidhip_colranks_csc(ctx(), INTEGER(Xp), REAL(Xx), n, Rf_asInteger(ties), Rf_asLogical(is_signed), REAL(R)));
  UNPROTECT(1);
  return R;
}

/* colranks(sparse X, keep.zero = FALSE): dense g x n ranks from the CSC slots (R/plaid.R:602-609) */
SEXP R_plaidhip_colranks_csc_dense(SEXP Xp, SEXP Xi, SEXP Xx, SEXP g, SEXP ties, SEXP is_signed) {
  const int n = LENGTH(Xp) - 1, gg = Rf_asInteger(g);
  SEXP R = PROTECT(Rf_allocMatrix(REALSXP, gg, n));
  check(plaidhip_colranks_csc_dense(ctx(), INTEGER(Xp), INTEGER(Xi), REAL(Xx), gg, n, Rf_asInteger(ties),
                                    Rf_asLogical(is_signed), REAL(R)));
  UNPROTECT(1);
  return R;
}

SEXP R_plaidhip_sing_dense(SEXP X, SEXP Gp, SEXP Gi) {
  const int g = Rf_nrows(X), n = Rf_ncols(X), m = LENGTH(Gp) - 1;
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, n));
  check(plaidhip_sing_dense(ctx(), REAL(X), g, n, INTEGER(Gp), INTEGER(Gi), m, REAL(S)));
  UNPROTECT(1);
  return S;
}

SEXP R_plaidhip_ssgsea_dense(SEXP X, SEXP Gp, SEXP Gi, SEXP alpha) {
  const int g = Rf_nrows(X), n = Rf_ncols(X), m = LENGTH(Gp) - 1;
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, n));
  check(plaidhip_ssgsea_dense(ctx(), REAL(X), g, n, INTEGER(Gp), INTEGER(Gi), m, Rf_asReal(alpha), REAL(S)));
  UNPROTECT(1);
  return S;
}

SEXP R_plaidhip_ssgsea_csc(SEXP Xp, SEXP Xi, SEXP Xx, SEXP g, SEXP Gp, SEXP Gi, SEXP alpha) {
  const int n = LENGTH(Xp) - 1, m = LENGTH(Gp) - 1;
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, n));
  check(plaidhip_ssgsea_csc(ctx(), INTEGER(Xp), INTEGER(Xi), REAL(Xx), Rf_asInteger(g), n, INTEGER(Gp),
                            INTEGER(Gi), m, Rf_asReal(alpha), REAL(S)));
  UNPROTECT(1);
  return S;
}

/* X: numeric matrix or NULL; for a dgCMatrix pass Xp/Xi/Xx (else R_NilValue) */
static const int* int_or_null(SEXP x) { return Rf_isNull(x) ? NULL : INTEGER(x); }

/* several GPUs from the one R process: `devices` integer vector of ordinals (plaidhip_*_multi, a host thread per
 * device inside the library) */
SEXP R_plaidhip_plaid_multi(SEXP devices, SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Gp, SEXP Gi, SEXP stat,
                            SEXP normalize) {
  const int m = LENGTH(Gp) - 1, nn = Rf_asInteger(n);
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, nn));
  check(plaidhip_plaid_multi(INTEGER(devices), LENGTH(devices), int_or_null(Xp), int_or_null(Xi), REAL(Xv), Rf_asInteger(g),
                             nn, INTEGER(Gp), INTEGER(Gi), m, Rf_asInteger(stat), Rf_asLogical(normalize), REAL(S)));
  UNPROTECT(1);
  return S;
}

SEXP R_plaidhip_sing_csc_multi(SEXP devices, SEXP Xp, SEXP Xi, SEXP Xx, SEXP g, SEXP Gp, SEXP Gi) {
  const int n = LENGTH(Xp) - 1, m = LENGTH(Gp) - 1;
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, n));
  check(plaidhip_sing_csc_multi(INTEGER(devices), LENGTH(devices), INTEGER(Xp), INTEGER(Xi), REAL(Xx), Rf_asInteger(g), n,
                                INTEGER(Gp), INTEGER(Gi), m, REAL(S)));
  UNPROTECT(1);
  return S;
}

SEXP R_plaidhip_sing_multi(SEXP devices, SEXP X, SEXP Gp, SEXP Gi) {
  const int g = Rf_nrows(X), n = Rf_ncols(X), m = LENGTH(Gp) - 1;
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, n));
  check(plaidhip_sing_multi(INTEGER(devices), LENGTH(devices), REAL(X), g, n, INTEGER(Gp), INTEGER(Gi), m, REAL(S)));
  UNPROTECT(1);
  return S;
}

SEXP R_plaidhip_ssgsea_multi(SEXP devices, SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Gp, SEXP Gi, SEXP alpha) {
  const int m = LENGTH(Gp) - 1, nn = Rf_asInteger(n);
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, nn));
  check(plaidhip_ssgsea_multi(INTEGER(devices), LENGTH(devices), int_or_null(Xp), int_or_null(Xi), REAL(Xv),
                              Rf_asInteger(g), nn, INTEGER(Gp), INTEGER(Gi), m, Rf_asReal(alpha), REAL(S)));
  UNPROTECT(1);
  return S;
}

SEXP R_plaidhip_ucell_multi(SEXP devices, SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Gp, SEXP Gi, SEXP kfull,
                            SEXP rmax) {
  const int m = LENGTH(Gp) - 1, nn = Rf_asInteger(n);
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, nn));
  check(plaidhip_ucell_multi(INTEGER(devices), LENGTH(devices), int_or_null(Xp), int_or_null(Xi), REAL(Xv), Rf_asInteger(g),
                             nn, INTEGER(Gp), INTEGER(Gi), m, REAL(kfull), Rf_asReal(rmax), REAL(S)));
  UNPROTECT(1);
  return S;
}

SEXP R_plaidhip_aucell_multi(SEXP devices, SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Gp, SEXP Gi, SEXP auc_max_rank) {
  const int m = LENGTH(Gp) - 1, nn = Rf_asInteger(n);
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, nn));
  check(plaidhip_aucell_multi(INTEGER(devices), LENGTH(devices), int_or_null(Xp), int_or_null(Xi), REAL(Xv),
                              Rf_asInteger(g), nn, INTEGER(Gp), INTEGER(Gi), m, Rf_asReal(auc_max_rank), REAL(S)));
  UNPROTECT(1);
  return S;
}

SEXP R_plaidhip_scse_multi(SEXP devices, SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Gp, SEXP Gi, SEXP remove_log2,
                           SEXP score_mean) {
  const int m = LENGTH(Gp) - 1, nn = Rf_asInteger(n);
  const int rl = Rf_asLogical(remove_log2);
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, nn));
  int removed = 0;
  check(plaidhip_scse_multi(INTEGER(devices), LENGTH(devices), int_or_null(Xp), int_or_null(Xi), REAL(Xv), Rf_asInteger(g),
                            nn, INTEGER(Gp), INTEGER(Gi), m, rl == NA_LOGICAL ? -1 : rl, Rf_asLogical(score_mean), REAL(S),
                            &removed));
  Rf_setAttrib(S, Rf_install("removedLog2"), Rf_ScalarLogical(removed));   /* as R_plaidhip_scse */
  UNPROTECT(1);
  return S;
}

SEXP R_plaidhip_gsva_multi(SEXP devices, SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Gp, SEXP Gi, SEXP tau, SEXP rowtf) {
  const int m = LENGTH(Gp) - 1, nn = Rf_asInteger(n);
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, nn));
  check(plaidhip_gsva_multi(INTEGER(devices), LENGTH(devices), int_or_null(Xp), int_or_null(Xi), REAL(Xv), Rf_asInteger(g),
                            nn, INTEGER(Gp), INTEGER(Gi), m, Rf_asReal(tau), Rf_asInteger(rowtf), REAL(S)));
  UNPROTECT(1);
  return S;
}

SEXP R_plaidhip_ssgsea_exact(SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Gp, SEXP Gi, SEXP alpha, SEXP scale, SEXP norm) {
  const int m = LENGTH(Gp) - 1, nn = Rf_asInteger(n);
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, nn));
  check(plaidhip_ssgsea_exact(ctx(), int_or_null(Xp), int_or_null(Xi), REAL(Xv), Rf_asInteger(g), nn, INTEGER(Gp),
                              INTEGER(Gi), m, Rf_asReal(alpha), Rf_asLogical(scale), Rf_asLogical(norm), REAL(S)));
  UNPROTECT(1);
  return S;
}

SEXP R_plaidhip_ssgsea_exact_multi(SEXP devices, SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Gp, SEXP Gi, SEXP alpha,
                                   SEXP scale, SEXP norm) {
  const int m = LENGTH(Gp) - 1, nn = Rf_asInteger(n);
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, nn));
  check(plaidhip_ssgsea_exact_multi(INTEGER(devices), LENGTH(devices), int_or_null(Xp), int_or_null(Xi), REAL(Xv),
                                    Rf_asInteger(g), nn, INTEGER(Gp), INTEGER(Gi), m, Rf_asReal(alpha), Rf_asLogical(scale),
                                    Rf_asLogical(norm), REAL(S)));
  UNPROTECT(1);
  return S;
}

/* replaid.ssgsea.exact(single = FALSE): the walk's value of largest magnitude */
SEXP R_plaidhip_ssgsea_exact_ks(SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Gp, SEXP Gi, SEXP alpha, SEXP scale,
                                SEXP norm) {
  const int m = LENGTH(Gp) - 1, nn = Rf_asInteger(n);
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, nn));
  check(plaidhip_ssgsea_exact_ks(ctx(), int_or_null(Xp), int_or_null(Xi), REAL(Xv), Rf_asInteger(g), nn, INTEGER(Gp),
                                 INTEGER(Gi), m, Rf_asReal(alpha), Rf_asLogical(scale), Rf_asLogical(norm), REAL(S)));
  UNPROTECT(1);
  return S;
}

SEXP R_plaidhip_ssgsea_exact_ks_multi(SEXP devices, SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Gp, SEXP Gi, SEXP alpha,
                                      SEXP scale, SEXP norm) {
  const int m = LENGTH(Gp) - 1, nn = Rf_asInteger(n);
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, nn));
  check(plaidhip_ssgsea_exact_ks_multi(INTEGER(devices), LENGTH(devices), int_or_null(Xp), int_or_null(Xi), REAL(Xv),
                                       Rf_asInteger(g), nn, INTEGER(Gp), INTEGER(Gi), m, Rf_asReal(alpha),
                                       Rf_asLogical(scale), Rf_asLogical(norm), REAL(S)));
  UNPROTECT(1);
  return S;
}

/* replaid.gsva.exact: GSVA's random-walk statistic; rowtf 0 "z", 1 "ecdf", 2 "none", 3 "gauss" */
SEXP R_plaidhip_gsva_exact(SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Gp, SEXP Gi, SEXP tau, SEXP rowtf, SEXP max_diff) {
  const int m = LENGTH(Gp) - 1, nn = Rf_asInteger(n);
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, nn));
  check(plaidhip_gsva_exact(ctx(), int_or_null(Xp), int_or_null(Xi), REAL(Xv), Rf_asInteger(g), nn, INTEGER(Gp), INTEGER(Gi),
                            m, Rf_asReal(tau), Rf_asInteger(rowtf), Rf_asLogical(max_diff), REAL(S)));
  UNPROTECT(1);
  return S;
}

SEXP R_plaidhip_gsva_exact_multi(SEXP devices, SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Gp, SEXP Gi, SEXP tau,
                                 SEXP rowtf, SEXP max_diff) {
  const int m = LENGTH(Gp) - 1, nn = Rf_asInteger(n);
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, nn));
  check(plaidhip_gsva_exact_multi(INTEGER(devices), LENGTH(devices), int_or_null(Xp), int_or_null(Xi), REAL(Xv),
                                  Rf_asInteger(g), nn, INTEGER(Gp), INTEGER(Gi), m, Rf_asReal(tau), Rf_asInteger(rowtf),
                                  Rf_asLogical(max_diff), REAL(S)));
  UNPROTECT(1);
  return S;
}

/* replaid.sing.exact: a list of six m x n matrices (total, up, down score; total, up, down dispersion), NULL where not
 * computed: Dp of length 0 means no down sets, dispersion FALSE no dispersions.  devices of length 0: the session's context */
SEXP R_plaidhip_sing_exact(SEXP devices, SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Gp, SEXP Gi, SEXP Dp, SEXP Di,
                           SEXP center, SEXP dispersion) {
  const int m = LENGTH(Gp) - 1, nn = Rf_asInteger(n);
  const int down = LENGTH(Dp) > 0, disp = Rf_asLogical(dispersion) != 0;
  const int want[6] = {down, 1, down, down && disp, disp, down && disp};
  double* out[6];
  SEXP res = PROTECT(Rf_allocVector(VECSXP, 6));
  for (int o = 0; o < 6; ++o) {
    out[o] = NULL;
    if (want[o]) {
      SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, nn));
      SET_VECTOR_ELT(res, o, S);
      UNPROTECT(1);
      out[o] = REAL(S);
    }
  }
  if (LENGTH(devices) > 0)
    check(plaidhip_sing_exact_multi(INTEGER(devices), LENGTH(devices), int_or_null(Xp), int_or_null(Xi), REAL(Xv),
                                    Rf_asInteger(g), nn, INTEGER(Gp), INTEGER(Gi), down ? INTEGER(Dp) : NULL,
                                    down ? INTEGER(Di) : NULL, m, Rf_asLogical(center), out[0], out[1], out[2], out[3], out[4],
                                    out[5]));
  else
    check(plaidhip_sing_exact(ctx(), int_or_null(Xp), int_or_null(Xi), REAL(Xv), Rf_asInteger(g), nn, INTEGER(Gp), INTEGER(Gi),
                              down ? INTEGER(Dp) : NULL, down ? INTEGER(Di) : NULL, m, Rf_asLogical(center), out[0], out[1],
                              out[2], out[3], out[4], out[5]));
  UNPROTECT(1);
  return res;
}

/* replaid.ucell.exact: a list of three m x n matrices (total, up, down), NULL where not computed: Dp of length 0 means no
 * down sets, kfull of length 0 no imputation.  devices of length 0: the session's context */
SEXP R_plaidhip_ucell_exact(SEXP devices, SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Gp, SEXP Gi, SEXP Dp, SEXP Di,
                            SEXP max_rank, SEXP w_neg, SEXP kfull, SEXP kfull_down) {
  const int m = LENGTH(Gp) - 1, nn = Rf_asInteger(n);
  const int down = LENGTH(Dp) > 0, impute = LENGTH(kfull) > 0;
  const int want[3] = {down, 1, down};
  double* out[3];
  SEXP res = PROTECT(Rf_allocVector(VECSXP, 3));
  for (int o = 0; o < 3; ++o) {
    out[o] = NULL;
    if (want[o]) {
      SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, nn));
      SET_VECTOR_ELT(res, o, S);
      UNPROTECT(1);
      out[o] = REAL(S);
    }
  }
  const double* kf = impute ? REAL(kfull) : NULL;
  const double* kd = impute && LENGTH(kfull_down) > 0 ? REAL(kfull_down) : NULL;
  if (LENGTH(devices) > 0)
    check(plaidhip_ucell_exact_multi(INTEGER(devices), LENGTH(devices), int_or_null(Xp), int_or_null(Xi), REAL(Xv),
                                     Rf_asInteger(g), nn, INTEGER(Gp), INTEGER(Gi), down ? INTEGER(Dp) : NULL,
                                     down ? INTEGER(Di) : NULL, m, Rf_asReal(max_rank), Rf_asReal(w_neg), impute, kf, kd, out[0],
                                     out[1], out[2]));
  else
    check(plaidhip_ucell_exact(ctx(), int_or_null(Xp), int_or_null(Xi), REAL(Xv), Rf_asInteger(g), nn, INTEGER(Gp), INTEGER(Gi),
                               down ? INTEGER(Dp) : NULL, down ? INTEGER(Di) : NULL, m, Rf_asReal(max_rank), Rf_asReal(w_neg),
                               impute, kf, kd, out[0], out[1], out[2]));
  UNPROTECT(1);
  return res;
}

SEXP R_plaidhip_aucell_exact(SEXP devices, SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Gp, SEXP Gi, SEXP auc_max_rank) {
  const int m = LENGTH(Gp) - 1, nn = Rf_asInteger(n);
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, nn));
  if (LENGTH(devices) > 0)
    check(plaidhip_aucell_exact_multi(INTEGER(devices), LENGTH(devices), int_or_null(Xp), int_or_null(Xi), REAL(Xv),
                                      Rf_asInteger(g), nn, INTEGER(Gp), INTEGER(Gi), m, Rf_asReal(auc_max_rank), REAL(S)));
  else
    check(plaidhip_aucell_exact(ctx(), int_or_null(Xp), int_or_null(Xi), REAL(Xv), Rf_asInteger(g), nn, INTEGER(Gp), INTEGER(Gi),
                                m, Rf_asReal(auc_max_rank), REAL(S)));
  UNPROTECT(1);
  return S;
}

SEXP R_plaidhip_ucell(SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Gp, SEXP Gi, SEXP kfull, SEXP rmax) {
  const int m = LENGTH(Gp) - 1, nn = Rf_asInteger(n);
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, nn));
  check(plaidhip_ucell(ctx(), int_or_null(Xp), int_or_null(Xi), REAL(Xv), Rf_asInteger(g), nn, INTEGER(Gp),
                       INTEGER(Gi), m, REAL(kfull), Rf_asReal(rmax), REAL(S)));
  UNPROTECT(1);
  return S;
}

SEXP R_plaidhip_aucell(SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Gp, SEXP Gi, SEXP auc_max_rank) {
  const int m = LENGTH(Gp) - 1, nn = Rf_asInteger(n);
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, nn));
  check(plaidhip_aucell(ctx(), int_or_null(Xp), int_or_null(Xi), REAL(Xv), Rf_asInteger(g), nn, INTEGER(Gp),
                        INTEGER(Gi), m, Rf_asReal(auc_max_rank), REAL(S)));
  UNPROTECT(1);
  return S;
}

SEXP R_plaidhip_scse(SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Gp, SEXP Gi, SEXP remove_log2, SEXP score_mean) {
  const int m = LENGTH(Gp) - 1, nn = Rf_asInteger(n);
  const int rl = Rf_asLogical(remove_log2);
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, nn));
  int removed = 0;
  check(plaidhip_scse(ctx(), int_or_null(Xp), int_or_null(Xi), REAL(Xv), Rf_asInteger(g), nn, INTEGER(Gp),
                      INTEGER(Gi), m, rl == NA_LOGICAL ? -1 : rl, Rf_asLogical(score_mean), REAL(S), &removed));
  /* whether 2**x ran (decided on the device when removeLog2 = NULL): the R wrapper prints R/plaid.R:164's message */
  Rf_setAttrib(S, Rf_install("removedLog2"), Rf_ScalarLogical(removed));
  UNPROTECT(1);
  return S;
}


/* gmt2mat(read.gmt(file)) in one native call: returns list(p, i, Dim, rownames, colnames); the R side
 * wraps it with new("dgCMatrix", ...).  (R/gmt-utils.R:19-66, 99-125)                             */
static SEXP split_lines(const char* txt, int64_t nbytes, int64_t count) {
  SEXP out = PROTECT(Rf_allocVector(STRSXP, (R_xlen_t)count));
  int64_t b = 0, k = 0;
  for (int64_t e = 0; e <= nbytes && k < count; ++e)
    if (e == nbytes || txt[e] == '\n') {
      SET_STRING_ELT(out, (R_xlen_t)k++, Rf_mkCharLenCE(txt + b, (int)(e - b), CE_UTF8));
      b = e + 1;
    }
  UNPROTECT(1);
  return out;
}

SEXP R_plaidhip_gmt2mat_file(SEXP path, SEXP add_source, SEXP nrows, SEXP max_genes, SEXP ntop, SEXP bg) {
  plaidhip_gmt* gmt = NULL;
  plaidhip_gmtmat* mat = NULL;
  if (plaidhip_gmt_read(CHAR(STRING_ELT(path, 0)), Rf_asLogical(add_source), (int64_t)Rf_asReal(nrows), &gmt) != PLAIDHIP_OK)
    Rf_error("plaidhip: %s", plaidhip_last_error_string());
  const int64_t nbg = Rf_isNull(bg) ? 0 : (int64_t)XLENGTH(bg);
  const char** bgp = nbg ? (const char**)R_alloc((size_t)nbg, sizeof(char*)) : NULL;
  for (int64_t k = 0; k < nbg; ++k) bgp[k] = Rf_translateCharUTF8(STRING_ELT(bg, (R_xlen_t)k));
  const int rc = plaidhip_gmt2mat(gmt, (int64_t)Rf_asReal(max_genes), (int64_t)Rf_asReal(ntop), bgp, nbg, &mat);
  plaidhip_gmt_destroy(gmt);
  if (rc != PLAIDHIP_OK) Rf_error("plaidhip: %s", plaidhip_last_error_string());
  /* everything R needs is copied into R_alloc() memory (released by R itself, also on error) and `mat` is freed
   * BEFORE the first R allocation that could longjmp: an allocation failure cannot leak the native object */
  int64_t dims[3], nb_r = 0, nb_c = 0;
  plaidhip_gmtmat_dims(mat, dims);
  int* cp = (int*)R_alloc((size_t)dims[1] + 1, sizeof(int));
  int* ci = (int*)R_alloc((size_t)(dims[2] > 0 ? dims[2] : 1), sizeof(int));
  memcpy(cp, plaidhip_gmtmat_p(mat), sizeof(int) * (size_t)(dims[1] + 1));
  if (dims[2]) memcpy(ci, plaidhip_gmtmat_i(mat), sizeof(int) * (size_t)dims[2]);
  const char* rn0 = plaidhip_gmtmat_names(mat, 0, &nb_r);
  char* rn = (char*)R_alloc((size_t)nb_r + 1, 1);
  memcpy(rn, rn0, (size_t)nb_r);
  const char* cn0 = plaidhip_gmtmat_names(mat, 1, &nb_c);
  char* cn = (char*)R_alloc((size_t)nb_c + 1, 1);
  memcpy(cn, cn0, (size_t)nb_c);
  plaidhip_gmtmat_destroy(mat);
  SEXP out = PROTECT(Rf_allocVector(VECSXP, 5));
  SEXP p = PROTECT(Rf_allocVector(INTSXP, (R_xlen_t)dims[1] + 1));
  SEXP i = PROTECT(Rf_allocVector(INTSXP, (R_xlen_t)dims[2]));
  memcpy(INTEGER(p), cp, sizeof(int) * (size_t)(dims[1] + 1));
  if (dims[2]) memcpy(INTEGER(i), ci, sizeof(int) * (size_t)dims[2]);
  SEXP dim = PROTECT(Rf_allocVector(INTSXP, 2));
  INTEGER(dim)[0] = (int)dims[0];
  INTEGER(dim)[1] = (int)dims[1];
  SEXP rnames = PROTECT(split_lines(rn, nb_r, dims[0]));
  SEXP cnames = PROTECT(split_lines(cn, nb_c, dims[1]));
  SET_VECTOR_ELT(out, 0, p);
  SET_VECTOR_ELT(out, 1, i);
  SET_VECTOR_ELT(out, 2, dim);
  SET_VECTOR_ELT(out, 3, rnames);
  SET_VECTOR_ELT(out, 4, cnames);
  UNPROTECT(6);
  return out;
}


/* plaid.test(): sets x 6 matrix (gsetFC, p.one, p.two, p.lm, p.meta, q.meta) in G's column order */
SEXP R_plaidhip_plaid_test(SEXP X, SEXP y, SEXP Gp, SEXP Gi, SEXP gsetX, SEXP tests, SEXP metap) {
  const int g = Rf_nrows(X), n = Rf_ncols(X), m = LENGTH(Gp) - 1;
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, m, 6));
  int rc = plaidhip_plaid_test(ctx(), REAL(X), g, n, INTEGER(y), INTEGER(Gp), INTEGER(Gi), m,
                               Rf_isNull(gsetX) ? NULL : REAL(gsetX), Rf_asInteger(tests), Rf_asInteger(metap), REAL(out));
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  UNPROTECT(1);
  return out;
}


SEXP R_plaidhip_gsva(SEXP X, SEXP Gp, SEXP Gi, SEXP tau, SEXP rowtf) {
  const int g = Rf_nrows(X), n = Rf_ncols(X), m = LENGTH(Gp) - 1;
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, n));
  int rc = plaidhip_gsva(ctx(), REAL(X), g, n, INTEGER(Gp), INTEGER(Gi), m, Rf_asReal(tau), Rf_asInteger(rowtf), REAL(S));
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  UNPROTECT(1);
  return S;
}

/* plaid.test() over several devices (plaidhip_plaid_test_multi): dense X (Xp, Xi NULL, Xv the matrix) or a dgCMatrix's
 * slots; the same result as R_plaidhip_plaid_test / R_plaidhip_plaid_test_csc and the same error messages */
SEXP R_plaidhip_plaid_test_multi(SEXP devices, SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP y, SEXP Gp, SEXP Gi,
                                 SEXP gsetX, SEXP tests, SEXP metap) {
  const int m = LENGTH(Gp) - 1;
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, m, 6));
  int rc = plaidhip_plaid_test_multi(INTEGER(devices), LENGTH(devices), int_or_null(Xp), int_or_null(Xi), REAL(Xv),
                                     Rf_asInteger(g), Rf_asInteger(n), INTEGER(y), INTEGER(Gp), INTEGER(Gi), m,
                                     Rf_isNull(gsetX) ? NULL : REAL(gsetX), Rf_asInteger(tests), Rf_asInteger(metap),
                                     REAL(out));
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  UNPROTECT(1);
  return out;
}

/* plaid.test.contrasts(): an m x 6C matrix, columns 6 j + 1 .. 6 j + 6 the matrix of R_plaidhip_plaid_test for contrast j
 * (the caller gives it dim m x 6 x C).  Y: n x C
 * integers, -1 for NA.  Dense X (Xp, Xi NULL, Xv the matrix) or a dgCMatrix's slots; several devices: the _multi entry */
SEXP R_plaidhip_plaid_test_contrasts(SEXP devices, SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Y, SEXP Gp, SEXP Gi,
                                     SEXP gsetX, SEXP tests, SEXP metap) {
  const int m = LENGTH(Gp) - 1, C = Rf_ncols(Y);
  const double* gx = Rf_isNull(gsetX) ? NULL : REAL(gsetX);
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, m, 6 * C));
  int rc;
  if (LENGTH(devices) > 1)
    rc = plaidhip_plaid_test_contrasts_multi(INTEGER(devices), LENGTH(devices), int_or_null(Xp), int_or_null(Xi), REAL(Xv),
                                             Rf_asInteger(g), Rf_asInteger(n), INTEGER(Y), C, INTEGER(Gp), INTEGER(Gi), m, gx,
                                             Rf_asInteger(tests), Rf_asInteger(metap), REAL(out));
  else if (!Rf_isNull(Xp))
    rc = plaidhip_plaid_test_contrasts_csc(ctx(), INTEGER(Xp), INTEGER(Xi), REAL(Xv), Rf_asInteger(g), Rf_asInteger(n),
                                           INTEGER(Y), C, INTEGER(Gp), INTEGER(Gi), m, gx, Rf_asInteger(tests),
                                           Rf_asInteger(metap), REAL(out));
  else
    rc = plaidhip_plaid_test_contrasts(ctx(), REAL(Xv), Rf_asInteger(g), Rf_asInteger(n), INTEGER(Y), C, INTEGER(Gp),
                                       INTEGER(Gi), m, gx, Rf_asInteger(tests), Rf_asInteger(metap), REAL(out));
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  UNPROTECT(1);
  return out;
}

/* the same two calls for a dgCMatrix: its slots, no dense X (plaidhip_plaid_test_csc / plaidhip_gsva_csc) */
SEXP R_plaidhip_plaid_test_csc(SEXP Xp, SEXP Xi, SEXP Xx, SEXP g, SEXP y, SEXP Gp, SEXP Gi, SEXP gsetX, SEXP tests,
                               SEXP metap) {
  const int n = LENGTH(Xp) - 1, m = LENGTH(Gp) - 1;
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, m, 6));
  int rc = plaidhip_plaid_test_csc(ctx(), INTEGER(Xp), INTEGER(Xi), REAL(Xx), Rf_asInteger(g), n, INTEGER(y), INTEGER(Gp),
                                   INTEGER(Gi), m, Rf_isNull(gsetX) ? NULL : REAL(gsetX), Rf_asInteger(tests),
                                   Rf_asInteger(metap), REAL(out));
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  UNPROTECT(1);
  return out;
}

SEXP R_plaidhip_gsva_csc(SEXP Xp, SEXP Xi, SEXP Xx, SEXP g, SEXP Gp, SEXP Gi, SEXP tau, SEXP rowtf) {
  const int n = LENGTH(Xp) - 1, m = LENGTH(Gp) - 1;
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, n));
  int rc = plaidhip_gsva_csc(ctx(), INTEGER(Xp), INTEGER(Xi), REAL(Xx), Rf_asInteger(g), n, INTEGER(Gp), INTEGER(Gi), m,
                             Rf_asReal(tau), Rf_asInteger(rowtf), REAL(S));
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  UNPROTECT(1);
  return S;
}

/* plaid.gsea(): an m x 12c matrix, columns 12 l + 1 .. 12 l + 12 the columns of plaidhip_gsea for list l (the caller gives
 * it dim m x 12 x c).  stat, weight: g x c doubles; perm: NULL (the placements generated from seed, two 32-bit halves in a
 * double each) or a g x nperm integer matrix of 0-based placements; several devices: the _multi entry */
SEXP R_plaidhip_gsea(SEXP devices, SEXP stat, SEXP weight, SEXP Gp, SEXP Gi, SEXP perm, SEXP nperm, SEXP seed_lo,
                     SEXP seed_hi) {
  const int g = Rf_nrows(stat), c = Rf_ncols(stat), m = LENGTH(Gp) - 1;
  const int B = Rf_isNull(perm) ? Rf_asInteger(nperm) : Rf_ncols(perm);
  const uint64_t seed = ((uint64_t)(uint32_t)Rf_asReal(seed_hi) << 32) | (uint64_t)(uint32_t)Rf_asReal(seed_lo);
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, m, 12 * c));
  int rc;
  if (LENGTH(devices) > 1)
    rc = plaidhip_gsea_multi(INTEGER(devices), LENGTH(devices), REAL(stat), REAL(weight), g, c, INTEGER(Gp), INTEGER(Gi), m,
                             int_or_null(perm), B, seed, REAL(out), NULL);
  else
    rc = plaidhip_gsea(ctx(), REAL(stat), REAL(weight), g, c, INTEGER(Gp), INTEGER(Gi), m, int_or_null(perm), B, seed,
                       REAL(out), NULL);
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  UNPROTECT(1);
  return out;
}

/* plaid.gsea(scoreType =, leadingEdge =): list(out, le_len, le_idx) of plaidhip_gsea_scored -- out as R_plaidhip_gsea
 * returns it; le_len (m x c integer) and le_idx (Gp[m] x c integer, 0-based rows of stat, -1 behind a set's edge), or NULL
 * for both when no edges are asked for */
SEXP R_plaidhip_gsea_scored(SEXP devices, SEXP stat, SEXP weight, SEXP Gp, SEXP Gi, SEXP perm, SEXP nperm, SEXP seed_lo,
                            SEXP seed_hi, SEXP score_type, SEXP edges) {
  const int g = Rf_nrows(stat), c = Rf_ncols(stat), m = LENGTH(Gp) - 1;
  const int B = Rf_isNull(perm) ? Rf_asInteger(nperm) : Rf_ncols(perm);
  const uint64_t seed = ((uint64_t)(uint32_t)Rf_asReal(seed_hi) << 32) | (uint64_t)(uint32_t)Rf_asReal(seed_lo);
  const int want = Rf_asLogical(edges) == 1, st = Rf_asInteger(score_type);
  SEXP res = PROTECT(Rf_allocVector(VECSXP, 3));
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, m, 12 * c));
  SET_VECTOR_ELT(res, 0, out);
  int32_t *le_len = NULL, *le_idx = NULL;
  if (want) {
    SEXP len = PROTECT(Rf_allocMatrix(INTSXP, m, c));
    SEXP idx = PROTECT(Rf_allocMatrix(INTSXP, INTEGER(Gp)[m], c));
    SET_VECTOR_ELT(res, 1, len);
    SET_VECTOR_ELT(res, 2, idx);
    le_len = INTEGER(len);
    le_idx = INTEGER(idx);
    UNPROTECT(2);
  }
  int rc;
  if (LENGTH(devices) > 1)
    rc = plaidhip_gsea_scored_multi(INTEGER(devices), LENGTH(devices), REAL(stat), REAL(weight), g, c, INTEGER(Gp), INTEGER(Gi),
                                    m, int_or_null(perm), B, seed, st, REAL(out), NULL, le_len, le_idx);
  else
    rc = plaidhip_gsea_scored(ctx(), REAL(stat), REAL(weight), g, c, INTEGER(Gp), INTEGER(Gi), m, int_or_null(perm), B, seed, st,
                              REAL(out), NULL, le_len, le_idx);
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  UNPROTECT(2);
  return res;
}

/* plaid.gsea(multilevel = TRUE): list(out, le_len, le_idx, ml) of plaidhip_gsea_multilevel -- the first three as
 * R_plaidhip_gsea_scored returns them (out with the reported pval and padj), ml an m x 6c matrix (columns 6 l + 1 .. 6 l + 6:
 * pvalML, log2err, stage, status, qhat, denom of list l).  ml_par: c(sampleSize, sweeps, eps, mlMin) */
SEXP R_plaidhip_gsea_multilevel(SEXP devices, SEXP stat, SEXP weight, SEXP Gp, SEXP Gi, SEXP perm, SEXP nperm, SEXP seed_lo,
                                SEXP seed_hi, SEXP score_type, SEXP edges, SEXP ml_par) {
  const int g = Rf_nrows(stat), c = Rf_ncols(stat), m = LENGTH(Gp) - 1;
  const int B = Rf_isNull(perm) ? Rf_asInteger(nperm) : Rf_ncols(perm);
  const uint64_t seed = ((uint64_t)(uint32_t)Rf_asReal(seed_hi) << 32) | (uint64_t)(uint32_t)Rf_asReal(seed_lo);
  const int want = Rf_asLogical(edges) == 1, st = Rf_asInteger(score_type);
  if (LENGTH(ml_par) != 4) Rf_error("plaid.gsea: ml_par must be c(sampleSize, sweeps, eps, mlMin)");
  const double* par = REAL(ml_par);
  SEXP res = PROTECT(Rf_allocVector(VECSXP, 4));
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, m, 12 * c));
  SEXP ml = PROTECT(Rf_allocMatrix(REALSXP, m, 6 * c));
  SET_VECTOR_ELT(res, 0, out);
  SET_VECTOR_ELT(res, 3, ml);
  int32_t *le_len = NULL, *le_idx = NULL;
  if (want) {
    SEXP len = PROTECT(Rf_allocMatrix(INTSXP, m, c));
    SEXP idx = PROTECT(Rf_allocMatrix(INTSXP, INTEGER(Gp)[m], c));
    SET_VECTOR_ELT(res, 1, len);
    SET_VECTOR_ELT(res, 2, idx);
    le_len = INTEGER(len);
    le_idx = INTEGER(idx);
    UNPROTECT(2);
  }
  int rc;
  if (LENGTH(devices) > 1)
    rc = plaidhip_gsea_multilevel_multi(INTEGER(devices), LENGTH(devices), REAL(stat), REAL(weight), g, c, INTEGER(Gp),
                                        INTEGER(Gi), m, int_or_null(perm), B, seed, st, (int32_t)par[0], (int32_t)par[1], par[2],
                                        (int32_t)par[3], REAL(out), NULL, le_len, le_idx, REAL(ml));
  else
    rc = plaidhip_gsea_multilevel(ctx(), REAL(stat), REAL(weight), g, c, INTEGER(Gp), INTEGER(Gi), m, int_or_null(perm), B, seed,
                                  st, (int32_t)par[0], (int32_t)par[1], par[2], (int32_t)par[3], REAL(out), NULL, le_len, le_idx,
                                  REAL(ml));
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  UNPROTECT(3);
  return res;
}

/* plaid.fisher(): list(out, tot, ov_len, ov_idx) of plaidhip_fisher -- out an m x 12c matrix (columns 12 l + 1 .. 12 l + 12
 * the columns of list l; the caller gives it dim m x 12 x c), tot 2 x c (nUp, nDn); ov_len (m x c integer) and ov_idx
 * (Gp[m] x c integer, 0-based rows of sig, -1 behind a set's overlap), or NULL for both when no overlap lists are asked for.
 * sig: a g x c integer matrix of -1 / 0 / 1 (R has no 8-bit integer: it is narrowed here; NA is refused); several
 * devices: the _multi entry */
SEXP R_plaidhip_fisher(SEXP devices, SEXP sig, SEXP Gp, SEXP Gi, SEXP overlap) {
  const int g = Rf_nrows(sig), c = Rf_ncols(sig), m = LENGTH(Gp) - 1;
  const int want = Rf_asLogical(overlap) == 1;
  const size_t count = (size_t)g * (size_t)c;
  int8_t* s8 = (int8_t*)R_alloc(count > 0 ? count : 1, 1);
  const int* s = INTEGER(sig);
  for (size_t e = 0; e < count; ++e) {
    if (s[e] < -1 || s[e] > 1) Rf_error("plaid.fisher: sig holds a value that is not -1, 0 or 1 (or NA)");
    s8[e] = (int8_t)s[e];
  }
  SEXP res = PROTECT(Rf_allocVector(VECSXP, 4));
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, m, 12 * c));
  SEXP tot = PROTECT(Rf_allocMatrix(REALSXP, 2, c));
  SET_VECTOR_ELT(res, 0, out);
  SET_VECTOR_ELT(res, 1, tot);
  int32_t *ov_len = NULL, *ov_idx = NULL;
  if (want) {
    SEXP len = PROTECT(Rf_allocMatrix(INTSXP, m, c));
    SEXP idx = PROTECT(Rf_allocMatrix(INTSXP, INTEGER(Gp)[m], c));
    SET_VECTOR_ELT(res, 2, len);
    SET_VECTOR_ELT(res, 3, idx);
    ov_len = INTEGER(len);
    ov_idx = INTEGER(idx);
    UNPROTECT(2);
  }
  int rc;
  if (LENGTH(devices) > 1)
    rc = plaidhip_fisher_multi(INTEGER(devices), LENGTH(devices), s8, g, c, INTEGER(Gp), INTEGER(Gi), m, REAL(out), REAL(tot),
                               ov_len, ov_idx);
  else
    rc = plaidhip_fisher(ctx(), s8, g, c, INTEGER(Gp), INTEGER(Gi), m, REAL(out), REAL(tot), ov_len, ov_idx);
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  UNPROTECT(3);
  return res;
}

/* plaid.limma(): list(out, hyper) of plaidhip_limma -- out a rows x (6 q nfit) matrix (the caller gives it dim rows x 6 x q x
 * nfit), hyper 4 x nfit (df.residual, df.prior, s2.prior, n.ok down a column).  A: rows x n doubles; design: n x (p nfit)
 * doubles, the fits' designs side by side; use: NULL or an n x nfit integer matrix (0 or NA: the sample takes no part; R has
 * no 8-bit integer: it is narrowed here); K: NULL (every coefficient) or p x q doubles; several devices: the _multi entry */
SEXP R_plaidhip_limma(SEXP devices, SEXP A, SEXP design, SEXP nfit_, SEXP use, SEXP K) {
  const int rows = Rf_nrows(A), n = Rf_ncols(A), nfit = Rf_asInteger(nfit_);
  if (nfit < 1 || Rf_nrows(design) != n || Rf_ncols(design) % nfit != 0)
    Rf_error("plaid.limma: design must have one row per sample and the same number of columns for every fit");
  const int p = Rf_ncols(design) / nfit;
  const int q = Rf_isNull(K) ? p : Rf_ncols(K);
  if (!Rf_isNull(K) && Rf_nrows(K) != p) Rf_error("plaid.limma: contrasts must have one row per coefficient");
  int8_t* u8 = NULL;
  if (!Rf_isNull(use)) {
    if (Rf_nrows(use) != n || Rf_ncols(use) != nfit) Rf_error("plaid.limma: use must be samples x fits");
    const size_t count = (size_t)n * (size_t)nfit;
    const int* u = INTEGER(use);
    u8 = (int8_t*)R_alloc(count > 0 ? count : 1, 1);
    for (size_t e = 0; e < count; ++e) u8[e] = (int8_t)(u[e] != 0 && u[e] != NA_INTEGER);
  }
  SEXP res = PROTECT(Rf_allocVector(VECSXP, 2));
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, rows, 6 * q * nfit));
  SEXP hyper = PROTECT(Rf_allocMatrix(REALSXP, 4, nfit));
  SET_VECTOR_ELT(res, 0, out);
  SET_VECTOR_ELT(res, 1, hyper);
  const double* Kp = Rf_isNull(K) ? NULL : REAL(K);
  int rc;
  if (LENGTH(devices) > 1)
    rc = plaidhip_limma_multi(INTEGER(devices), LENGTH(devices), REAL(A), rows, n, REAL(design), p, nfit, u8, Kp, q, REAL(out),
                              REAL(hyper));
  else
    rc = plaidhip_limma(ctx(), REAL(A), rows, n, REAL(design), p, nfit, u8, Kp, q, REAL(out), REAL(hyper));
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  UNPROTECT(3);
  return res;
}

/* plaid.camera(): list(out, hyper) of plaidhip_camera -- out an m x (8 q nfit) matrix (the caller gives it dim m x 8 x q x
 * nfit: NGenes, Correlation, VIF, t, Down, Up, PValue, FDR), hyper 6 x nfit (plaid.limma's four, n.genes, df.camera down a
 * column).  X, design, use, K: as R_plaidhip_limma; Gp, Gi: the sets' pattern over the rows of X; rho: the fixed inter-gene
 * correlation, NA to estimate every set's variance inflation factor; several devices: the _multi entry */
SEXP R_plaidhip_camera(SEXP devices, SEXP X, SEXP design, SEXP nfit_, SEXP use, SEXP K, SEXP Gp, SEXP Gi, SEXP rho_,
                       SEXP allow_neg_) {
  const int g = Rf_nrows(X), n = Rf_ncols(X), nfit = Rf_asInteger(nfit_), m = LENGTH(Gp) - 1;
  if (nfit < 1 || Rf_nrows(design) != n || Rf_ncols(design) % nfit != 0)
    Rf_error("plaid.camera: design must have one row per sample and the same number of columns for every fit");
  if (m < 0) Rf_error("plaid.camera: an empty column pointer");
  const int p = Rf_ncols(design) / nfit;
  const int q = Rf_isNull(K) ? p : Rf_ncols(K);
  if (!Rf_isNull(K) && Rf_nrows(K) != p) Rf_error("plaid.camera: contrasts must have one row per coefficient");
  int8_t* u8 = NULL;
  if (!Rf_isNull(use)) {
    if (Rf_nrows(use) != n || Rf_ncols(use) != nfit) Rf_error("plaid.camera: use must be samples x fits");
    const size_t count = (size_t)n * (size_t)nfit;
    const int* u = INTEGER(use);
    u8 = (int8_t*)R_alloc(count > 0 ? count : 1, 1);
    for (size_t e = 0; e < count; ++e) u8[e] = (int8_t)(u[e] != 0 && u[e] != NA_INTEGER);
  }
  const double rho = Rf_asReal(rho_);   /* (NA_real_ is a NaN: the library takes any NaN as "estimate") */
  const int allow_neg = Rf_asLogical(allow_neg_) == 1;
  SEXP res = PROTECT(Rf_allocVector(VECSXP, 2));
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, m, 8 * q * nfit));
  SEXP hyper = PROTECT(Rf_allocMatrix(REALSXP, 6, nfit));
  SET_VECTOR_ELT(res, 0, out);
  SET_VECTOR_ELT(res, 1, hyper);
  const double* Kp = Rf_isNull(K) ? NULL : REAL(K);
  int rc;
  if (LENGTH(devices) > 1)
    rc = plaidhip_camera_multi(INTEGER(devices), LENGTH(devices), REAL(X), g, n, REAL(design), p, nfit, u8, Kp, q, INTEGER(Gp),
                               INTEGER(Gi), m, rho, allow_neg, REAL(out), REAL(hyper));
  else
    rc = plaidhip_camera(ctx(), REAL(X), g, n, REAL(design), p, nfit, u8, Kp, q, INTEGER(Gp), INTEGER(Gi), m, rho, allow_neg,
                         REAL(out), REAL(hyper));
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  UNPROTECT(3);
  return res;
}

/* plaid.fry(): list(out, hyper) of plaidhip_fry -- out an m x (7 q nfit) matrix (the caller gives it dim m x 7 x q x nfit:
 * NGenes, Direction, t, PValue, FDR, PValue.Mixed, FDR.Mixed), hyper 7 x nfit (plaid.limma's four, n.genes, n.effects, mixed
 * down a column).  X, design, use, K, Gp, Gi: as R_plaidhip_camera; standardize: 0 posterior.sd, 1 residual.sd, 2 none */
SEXP R_plaidhip_fry(SEXP devices, SEXP X, SEXP design, SEXP nfit_, SEXP use, SEXP K, SEXP Gp, SEXP Gi, SEXP standardize_) {
  const int g = Rf_nrows(X), n = Rf_ncols(X), nfit = Rf_asInteger(nfit_), m = LENGTH(Gp) - 1;
  if (nfit < 1 || Rf_nrows(design) != n || Rf_ncols(design) % nfit != 0)
    Rf_error("plaid.fry: design must have one row per sample and the same number of columns for every fit");
  if (m < 0) Rf_error("plaid.fry: an empty column pointer");
  const int p = Rf_ncols(design) / nfit;
  const int q = Rf_isNull(K) ? p : Rf_ncols(K);
  if (!Rf_isNull(K) && Rf_nrows(K) != p) Rf_error("plaid.fry: contrasts must have one row per coefficient");
  int8_t* u8 = NULL;
  if (!Rf_isNull(use)) {
    if (Rf_nrows(use) != n || Rf_ncols(use) != nfit) Rf_error("plaid.fry: use must be samples x fits");
    const size_t count = (size_t)n * (size_t)nfit;
    const int* u = INTEGER(use);
    u8 = (int8_t*)R_alloc(count > 0 ? count : 1, 1);
    for (size_t e = 0; e < count; ++e) u8[e] = (int8_t)(u[e] != 0 && u[e] != NA_INTEGER);
  }
  const int standardize = Rf_asInteger(standardize_);
  SEXP res = PROTECT(Rf_allocVector(VECSXP, 2));
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, m, 7 * q * nfit));
  SEXP hyper = PROTECT(Rf_allocMatrix(REALSXP, 7, nfit));
  SET_VECTOR_ELT(res, 0, out);
  SET_VECTOR_ELT(res, 1, hyper);
  const double* Kp = Rf_isNull(K) ? NULL : REAL(K);
  int rc;
  if (LENGTH(devices) > 1)
    rc = plaidhip_fry_multi(INTEGER(devices), LENGTH(devices), REAL(X), g, n, REAL(design), p, nfit, u8, Kp, q, INTEGER(Gp),
                            INTEGER(Gi), m, standardize, REAL(out), REAL(hyper));
  else
    rc = plaidhip_fry(ctx(), REAL(X), g, n, REAL(design), p, nfit, u8, Kp, q, INTEGER(Gp), INTEGER(Gi), m, standardize,
                      REAL(out), REAL(hyper));
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  UNPROTECT(3);
  return res;
}

/* plaid.roast(): list(out, hyper) of plaidhip_roast -- out an m x (8 q nfit) matrix (the caller gives it dim m x 8 x q x nfit:
 * NGenes, PropDown, PropUp, Direction, PValue, FDR, PValue.Mixed, FDR.Mixed), hyper 7 x nfit (plaid.limma's four, n.genes, nrot,
 * mean50.capped down a column).  X, design, use, K, Gp, Gi: as R_plaidhip_fry; opts: integer (set statistic 0..3, z-score 0..1,
 * nrot, midp); seed: a whole number below 2^53; rotations: NULL (generated) or nrot x (n + 1) x nfit doubles, i.e. every
 * fit's (n + 1) x nrot matrix row by row */
SEXP R_plaidhip_roast(SEXP devices, SEXP X, SEXP design, SEXP nfit_, SEXP use, SEXP K, SEXP Gp, SEXP Gi, SEXP opts, SEXP seed_,
                      SEXP rotations) {
  const int g = Rf_nrows(X), n = Rf_ncols(X), nfit = Rf_asInteger(nfit_), m = LENGTH(Gp) - 1;
  if (nfit < 1 || Rf_nrows(design) != n || Rf_ncols(design) % nfit != 0)
    Rf_error("plaid.roast: design must have one row per sample and the same number of columns for every fit");
  if (m < 0) Rf_error("plaid.roast: an empty column pointer");
  if (LENGTH(opts) != 4) Rf_error("plaid.roast: opts must be (set statistic, z-score, nrot, midp)");
  const int p = Rf_ncols(design) / nfit;
  const int q = Rf_isNull(K) ? p : Rf_ncols(K);
  if (!Rf_isNull(K) && Rf_nrows(K) != p) Rf_error("plaid.roast: contrasts must have one row per coefficient");
  int8_t* u8 = NULL;
  if (!Rf_isNull(use)) {
    if (Rf_nrows(use) != n || Rf_ncols(use) != nfit) Rf_error("plaid.roast: use must be samples x fits");
    const size_t count = (size_t)n * (size_t)nfit;
    const int* u = INTEGER(use);
    u8 = (int8_t*)R_alloc(count > 0 ? count : 1, 1);
    for (size_t e = 0; e < count; ++e) u8[e] = (int8_t)(u[e] != 0 && u[e] != NA_INTEGER);
  }
  const int stat = INTEGER(opts)[0], zscore = INTEGER(opts)[1], nrot = INTEGER(opts)[2], midp = INTEGER(opts)[3];
  const double seed = Rf_asReal(seed_);
  if (!(seed >= 0.0 && seed < 9007199254740992.0)) Rf_error("plaid.roast: seed must be a whole number in [0, 2^53)");
  const double* rot = NULL;
  if (!Rf_isNull(rotations)) {
    if (nrot < 1 || (double)XLENGTH(rotations) != (double)nrot * ((double)n + 1.0) * (double)nfit)
      Rf_error("plaid.roast: rotations must be (samples + 1) x nrot for every fit");
    rot = REAL(rotations);
  }
  SEXP res = PROTECT(Rf_allocVector(VECSXP, 2));
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, m, 8 * q * nfit));
  SEXP hyper = PROTECT(Rf_allocMatrix(REALSXP, 7, nfit));
  SET_VECTOR_ELT(res, 0, out);
  SET_VECTOR_ELT(res, 1, hyper);
  const double* Kp = Rf_isNull(K) ? NULL : REAL(K);
  int rc;
  if (LENGTH(devices) > 1)
    rc = plaidhip_roast_multi(INTEGER(devices), LENGTH(devices), REAL(X), g, n, REAL(design), p, nfit, u8, Kp, q, INTEGER(Gp),
                              INTEGER(Gi), m, stat, zscore, nrot, (uint64_t)seed, midp, rot, REAL(out), REAL(hyper));
  else
    rc = plaidhip_roast(ctx(), REAL(X), g, n, REAL(design), p, nfit, u8, Kp, q, INTEGER(Gp), INTEGER(Gi), m, stat, zscore, nrot,
                        (uint64_t)seed, midp, rot, REAL(out), REAL(hyper));
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  UNPROTECT(3);
  return res;
}

/* plaid.romer(): list(out, hyper) of plaidhip_romer -- out an m x (7 q nfit) matrix (the caller gives it dim m x 7 x q x nfit:
 * NGenes, Up, Down, Mixed, FDR.Up, FDR.Down, FDR.Mixed), hyper (8 + q) x nfit (plaid.limma's four, n.genes, nrot, mean50.capped,
 * nan.t, then pi of every contrast down a column).  X, design, use, K, Gp, Gi: as R_plaidhip_roast; opts: integer (set statistic
 * 0..2, nrot, shrink.resid); seed: a whole number below 2^53; rotations: NULL (generated) or nrot x (n + 1) x nfit doubles, i.e.
 * every fit's (n + 1) x nrot matrix row by row */
SEXP R_plaidhip_romer(SEXP devices, SEXP X, SEXP design, SEXP nfit_, SEXP use, SEXP K, SEXP Gp, SEXP Gi, SEXP opts, SEXP seed_,
                      SEXP rotations) {
  const int g = Rf_nrows(X), n = Rf_ncols(X), nfit = Rf_asInteger(nfit_), m = LENGTH(Gp) - 1;
  if (nfit < 1 || Rf_nrows(design) != n || Rf_ncols(design) % nfit != 0)
    Rf_error("plaid.romer: design must have one row per sample and the same number of columns for every fit");
  if (m < 0) Rf_error("plaid.romer: an empty column pointer");
  if (LENGTH(opts) != 3) Rf_error("plaid.romer: opts must be (set statistic, nrot, shrink.resid)");
  const int p = Rf_ncols(design) / nfit;
  const int q = Rf_isNull(K) ? p : Rf_ncols(K);
  if (!Rf_isNull(K) && Rf_nrows(K) != p) Rf_error("plaid.romer: contrasts must have one row per coefficient");
  int8_t* u8 = NULL;
  if (!Rf_isNull(use)) {
    if (Rf_nrows(use) != n || Rf_ncols(use) != nfit) Rf_error("plaid.romer: use must be samples x fits");
    const size_t count = (size_t)n * (size_t)nfit;
    const int* u = INTEGER(use);
    u8 = (int8_t*)R_alloc(count > 0 ? count : 1, 1);
    for (size_t e = 0; e < count; ++e) u8[e] = (int8_t)(u[e] != 0 && u[e] != NA_INTEGER);
  }
  const int stat = INTEGER(opts)[0], nrot = INTEGER(opts)[1], shrink = INTEGER(opts)[2];
  const double seed = Rf_asReal(seed_);
  if (!(seed >= 0.0 && seed < 9007199254740992.0)) Rf_error("plaid.romer: seed must be a whole number in [0, 2^53)");
  const double* rot = NULL;
  if (!Rf_isNull(rotations)) {
    if (nrot < 1 || (double)XLENGTH(rotations) != (double)nrot * ((double)n + 1.0) * (double)nfit)
      Rf_error("plaid.romer: rotations must be (samples + 1) x nrot for every fit");
    rot = REAL(rotations);
  }
  SEXP res = PROTECT(Rf_allocVector(VECSXP, 2));
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, m, 7 * q * nfit));
  SEXP hyper = PROTECT(Rf_allocMatrix(REALSXP, 8 + q, nfit));
  SET_VECTOR_ELT(res, 0, out);
  SET_VECTOR_ELT(res, 1, hyper);
  const double* Kp = Rf_isNull(K) ? NULL : REAL(K);
  int rc;
  if (LENGTH(devices) > 1)
    rc = plaidhip_romer_multi(INTEGER(devices), LENGTH(devices), REAL(X), g, n, REAL(design), p, nfit, u8, Kp, q, INTEGER(Gp),
                              INTEGER(Gi), m, stat, nrot, (uint64_t)seed, shrink, NULL, rot, REAL(out), REAL(hyper));
  else
    rc = plaidhip_romer(ctx(), REAL(X), g, n, REAL(design), p, nfit, u8, Kp, q, INTEGER(Gp), INTEGER(Gi), m, stat, nrot,
                        (uint64_t)seed, shrink, NULL, rot, REAL(out), REAL(hyper));
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  UNPROTECT(3);
  return res;
}

/* plaid.limma(na = "fit"): list(out, hyper, dfres) of plaidhip_limma_na -- R_plaidhip_limma's operands and max_na; hyper 5 x
 * nfit (df.pooled last), dfres rows x nfit (the df.residual of every fitted row, NaN for the others) */
SEXP R_plaidhip_limma_na(SEXP devices, SEXP A, SEXP design, SEXP nfit_, SEXP use, SEXP K, SEXP max_na_) {
  const int rows = Rf_nrows(A), n = Rf_ncols(A), nfit = Rf_asInteger(nfit_);
  const double max_na = Rf_asReal(max_na_);
  if (nfit < 1 || Rf_nrows(design) != n || Rf_ncols(design) % nfit != 0)
    Rf_error("plaid.limma: design must have one row per sample and the same number of columns for every fit");
  const int p = Rf_ncols(design) / nfit;
  const int q = Rf_isNull(K) ? p : Rf_ncols(K);
  if (!Rf_isNull(K) && Rf_nrows(K) != p) Rf_error("plaid.limma: contrasts must have one row per coefficient");
  int8_t* u8 = NULL;
  if (!Rf_isNull(use)) {
    if (Rf_nrows(use) != n || Rf_ncols(use) != nfit) Rf_error("plaid.limma: use must be samples x fits");
    const size_t count = (size_t)n * (size_t)nfit;
    const int* u = INTEGER(use);
    u8 = (int8_t*)R_alloc(count > 0 ? count : 1, 1);
    for (size_t e = 0; e < count; ++e) u8[e] = (int8_t)(u[e] != 0 && u[e] != NA_INTEGER);
  }
  SEXP res = PROTECT(Rf_allocVector(VECSXP, 3));
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, rows, 6 * q * nfit));
  SEXP hyper = PROTECT(Rf_allocMatrix(REALSXP, 5, nfit));
  SEXP dfres = PROTECT(Rf_allocMatrix(REALSXP, rows, nfit));
  SET_VECTOR_ELT(res, 0, out);
  SET_VECTOR_ELT(res, 1, hyper);
  SET_VECTOR_ELT(res, 2, dfres);
  const double* Kp = Rf_isNull(K) ? NULL : REAL(K);
  int rc;
  if (LENGTH(devices) > 1)
    rc = plaidhip_limma_na_multi(INTEGER(devices), LENGTH(devices), REAL(A), rows, n, REAL(design), p, nfit, u8, Kp, q, max_na,
                                 REAL(out), REAL(hyper), REAL(dfres));
  else
    rc = plaidhip_limma_na(ctx(), REAL(A), rows, n, REAL(design), p, nfit, u8, Kp, q, max_na, REAL(out), REAL(hyper),
                           REAL(dfres));
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  UNPROTECT(4);
  return res;
}

/* plaid.limma(weights = ): list(out, hyper, dfres) of plaidhip_limma_w -- R_plaidhip_limma_na's operands with Wt (a rows x n
 * double matrix of observation weights, or NULL) and aw (n array weights, or NULL) after A; the R wrapper sends at least one */
SEXP R_plaidhip_limma_w(SEXP devices, SEXP A, SEXP Wt, SEXP aw, SEXP design, SEXP nfit_, SEXP use, SEXP K, SEXP max_na_) {
  const int rows = Rf_nrows(A), n = Rf_ncols(A), nfit = Rf_asInteger(nfit_);
  const double max_na = Rf_asReal(max_na_);
  if (nfit < 1 || Rf_nrows(design) != n || Rf_ncols(design) % nfit != 0)
    Rf_error("plaid.limma: design must have one row per sample and the same number of columns for every fit");
  const int p = Rf_ncols(design) / nfit;
  const int q = Rf_isNull(K) ? p : Rf_ncols(K);
  if (!Rf_isNull(K) && Rf_nrows(K) != p) Rf_error("plaid.limma: contrasts must have one row per coefficient");
  if (!Rf_isNull(Wt) && (Rf_nrows(Wt) != rows || Rf_ncols(Wt) != n)) Rf_error("plaid.limma: a matrix of weights has the shape of S");
  if (!Rf_isNull(aw) && LENGTH(aw) != n) Rf_error("plaid.limma: a vector of weights has one entry per sample");
  int8_t* u8 = NULL;
  if (!Rf_isNull(use)) {
    if (Rf_nrows(use) != n || Rf_ncols(use) != nfit) Rf_error("plaid.limma: use must be samples x fits");
    const size_t count = (size_t)n * (size_t)nfit;
    const int* u = INTEGER(use);
    u8 = (int8_t*)R_alloc(count > 0 ? count : 1, 1);
    for (size_t e = 0; e < count; ++e) u8[e] = (int8_t)(u[e] != 0 && u[e] != NA_INTEGER);
  }
  SEXP res = PROTECT(Rf_allocVector(VECSXP, 3));
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, rows, 6 * q * nfit));
  SEXP hyper = PROTECT(Rf_allocMatrix(REALSXP, 5, nfit));
  SEXP dfres = PROTECT(Rf_allocMatrix(REALSXP, rows, nfit));
  SET_VECTOR_ELT(res, 0, out);
  SET_VECTOR_ELT(res, 1, hyper);
  SET_VECTOR_ELT(res, 2, dfres);
  const double* Kp = Rf_isNull(K) ? NULL : REAL(K);
  const double* Wp = Rf_isNull(Wt) ? NULL : REAL(Wt);
  const double* ap = Rf_isNull(aw) ? NULL : REAL(aw);
  int rc;
  if (LENGTH(devices) > 1)
    rc = plaidhip_limma_w_multi(INTEGER(devices), LENGTH(devices), REAL(A), Wp, ap, rows, n, REAL(design), p, nfit, u8, Kp, q,
                                max_na, REAL(out), REAL(hyper), REAL(dfres));
  else
    rc = plaidhip_limma_w(ctx(), REAL(A), Wp, ap, rows, n, REAL(design), p, nfit, u8, Kp, q, max_na, REAL(out), REAL(hyper),
                          REAL(dfres));
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  UNPROTECT(4);
  return res;
}

/* plaid.voom(): list(E, weights, lib.size, offset, knots.x, knots.y) of plaidhip_voom -- counts a double genes x samples matrix,
 * design samples x p, lib_size a double vector over the samples or NULL (the column sums), span the lowess span; several
 * devices: the _multi entry */
SEXP R_plaidhip_voom(SEXP devices, SEXP counts, SEXP design, SEXP lib_size, SEXP span_) {
  const int rows = Rf_nrows(counts), n = Rf_ncols(counts), p = Rf_ncols(design);
  const double span = Rf_asReal(span_);
  if (Rf_nrows(design) != n) Rf_error("plaid.voom: design must have one row per column of counts");
  if (!Rf_isNull(lib_size) && LENGTH(lib_size) != n) Rf_error("plaid.voom: lib.size must have one entry per sample");
  SEXP res = PROTECT(Rf_allocVector(VECSXP, 6));
  SEXP E = PROTECT(Rf_allocMatrix(REALSXP, rows, n));
  SEXP W = PROTECT(Rf_allocMatrix(REALSXP, rows, n));
  SEXP lib = PROTECT(Rf_allocVector(REALSXP, n));
  SEXP off = PROTECT(Rf_allocVector(REALSXP, n));
  double* kx = (double*)R_alloc(PLAIDHIP_VOOM_MAX_KNOTS, sizeof(double));
  double* ky = (double*)R_alloc(PLAIDHIP_VOOM_MAX_KNOTS, sizeof(double));
  int32_t nk = 0;
  const double* lp = Rf_isNull(lib_size) ? NULL : REAL(lib_size);
  int rc;
  if (LENGTH(devices) > 1)
    rc = plaidhip_voom_multi(INTEGER(devices), LENGTH(devices), REAL(counts), rows, n, REAL(design), p, lp, span, REAL(E), REAL(W),
                             REAL(lib), REAL(off), kx, ky, &nk);
  else
    rc = plaidhip_voom(ctx(), REAL(counts), rows, n, REAL(design), p, lp, span, REAL(E), REAL(W), REAL(lib), REAL(off), kx, ky, &nk);
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  SEXP kxs = PROTECT(Rf_allocVector(REALSXP, nk));
  SEXP kys = PROTECT(Rf_allocVector(REALSXP, nk));
  for (int i = 0; i < nk; ++i) {
    REAL(kxs)[i] = kx[i];
    REAL(kys)[i] = ky[i];
  }
  SET_VECTOR_ELT(res, 0, E);
  SET_VECTOR_ELT(res, 1, W);
  SET_VECTOR_ELT(res, 2, lib);
  SET_VECTOR_ELT(res, 3, off);
  SET_VECTOR_ELT(res, 4, kxs);
  SET_VECTOR_ELT(res, 5, kys);
  UNPROTECT(7);
  return res;
}

/* plaid.rankcor(): list(out, tot) of plaidhip_rankcor -- out an m x 5c matrix (columns 5 l + 1 .. 5 l + 5 the columns of list
 * l; the caller gives it dim m x 5 x c), tot the c universe sizes.  stat: a g x c double matrix, NA / NaN: the gene takes no
 * part in that list; ties: 0 average, 1 min, 2 max; several devices: the _multi entry */
SEXP R_plaidhip_rankcor(SEXP devices, SEXP stat, SEXP Gp, SEXP Gi, SEXP use_rank, SEXP ties) {
  const int g = Rf_nrows(stat), c = Rf_ncols(stat), m = LENGTH(Gp) - 1;
  const int ur = Rf_asLogical(use_rank) == 1, tm = Rf_asInteger(ties);
  SEXP res = PROTECT(Rf_allocVector(VECSXP, 2));
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, m, 5 * c));
  SEXP tot = PROTECT(Rf_allocVector(REALSXP, c));
  SET_VECTOR_ELT(res, 0, out);
  SET_VECTOR_ELT(res, 1, tot);
  int rc;
  if (LENGTH(devices) > 1)
    rc = plaidhip_rankcor_multi(INTEGER(devices), LENGTH(devices), REAL(stat), g, c, INTEGER(Gp), INTEGER(Gi), m, ur, tm,
                                REAL(out), REAL(tot));
  else
    rc = plaidhip_rankcor(ctx(), REAL(stat), g, c, INTEGER(Gp), INTEGER(Gi), m, ur, tm, REAL(out), REAL(tot));
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  UNPROTECT(3);
  return res;
}

/* replaid.plage(): list(S, info, loadings) of plaidhip_plage -- S m x n, info m x 6 (size, lambda, explained, iterations,
 * residual, converged), loadings Gp[m] doubles in the sets' own segments of G (NULL unless asked).  Xp / Xi NULL: a dense
 * X.  One device: plaidhip_plage or plaidhip_plage_csc on the session's context; several: the _multi entry */
SEXP R_plaidhip_plage(SEXP devices, SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Gp, SEXP Gi, SEXP tol, SEXP maxit,
                      SEXP loadings) {
  const int m = LENGTH(Gp) - 1, nn = Rf_asInteger(n), gg = Rf_asInteger(g), want = Rf_asLogical(loadings) == 1;
  SEXP res = PROTECT(Rf_allocVector(VECSXP, 3));
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, nn));
  SEXP info = PROTECT(Rf_allocMatrix(REALSXP, m, 6));
  SEXP load = PROTECT(want ? Rf_allocVector(REALSXP, INTEGER(Gp)[m]) : R_NilValue);
  SET_VECTOR_ELT(res, 0, S);
  SET_VECTOR_ELT(res, 1, info);
  SET_VECTOR_ELT(res, 2, load);
  double* L = want ? REAL(load) : NULL;
  int rc;
  if (LENGTH(devices) > 1)
    rc = plaidhip_plage_multi(INTEGER(devices), LENGTH(devices), int_or_null(Xp), int_or_null(Xi), REAL(Xv), gg, nn, INTEGER(Gp),
                              INTEGER(Gi), m, Rf_asReal(tol), Rf_asInteger(maxit), REAL(S), REAL(info), L);
  else if (int_or_null(Xp) != NULL)
    rc = plaidhip_plage_csc(ctx(), INTEGER(Xp), int_or_null(Xi), REAL(Xv), gg, nn, INTEGER(Gp), INTEGER(Gi), m, Rf_asReal(tol),
                            Rf_asInteger(maxit), REAL(S), REAL(info), L);
  else
    rc = plaidhip_plage(ctx(), REAL(Xv), gg, nn, INTEGER(Gp), INTEGER(Gi), m, Rf_asReal(tol), Rf_asInteger(maxit), REAL(S),
                        REAL(info), L);
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  UNPROTECT(4);
  return res;
}

/* replaid.zscore(): the m x n scores of plaidhip_zscore; the dispatch of R_plaidhip_plage */
SEXP R_plaidhip_zscore(SEXP devices, SEXP Xp, SEXP Xi, SEXP Xv, SEXP g, SEXP n, SEXP Gp, SEXP Gi) {
  const int m = LENGTH(Gp) - 1, nn = Rf_asInteger(n), gg = Rf_asInteger(g);
  SEXP S = PROTECT(Rf_allocMatrix(REALSXP, m, nn));
  int rc;
  if (LENGTH(devices) > 1)
    rc = plaidhip_zscore_multi(INTEGER(devices), LENGTH(devices), int_or_null(Xp), int_or_null(Xi), REAL(Xv), gg, nn, INTEGER(Gp),
                               INTEGER(Gi), m, REAL(S), NULL);
  else if (int_or_null(Xp) != NULL)
    rc = plaidhip_zscore_csc(ctx(), INTEGER(Xp), int_or_null(Xi), REAL(Xv), gg, nn, INTEGER(Gp), INTEGER(Gi), m, REAL(S), NULL);
  else
    rc = plaidhip_zscore(ctx(), REAL(Xv), gg, nn, INTEGER(Gp), INTEGER(Gi), m, REAL(S), NULL);
  if (rc != PLAIDHIP_OK) Rf_error("%s", plaidhip_last_error_string());
  UNPROTECT(1);
  return S;
}

static const R_CallMethodDef call_methods[] = {
    {"R_plaidhip_session", (DL_FUNC)&R_plaidhip_session, 2},
    {"R_plaidhip_plaid_dense", (DL_FUNC)&R_plaidhip_plaid_dense, 5},
    {"R_plaidhip_plaid_csc", (DL_FUNC)&R_plaidhip_plaid_csc, 8},
    {"R_plaidhip_crossprod_weighted_dense", (DL_FUNC)&R_plaidhip_crossprod_weighted_dense, 4},
    {"R_plaidhip_crossprod_weighted_csc", (DL_FUNC)&R_plaidhip_crossprod_weighted_csc, 7},
    {"R_plaidhip_sing_csc", (DL_FUNC)&R_plaidhip_sing_csc, 6},
    {"R_plaidhip_sing_csc_multi", (DL_FUNC)&R_plaidhip_sing_csc_multi, 7},
    {"R_plaidhip_normalize_medians", (DL_FUNC)&R_plaidhip_normalize_medians, 2},
    {"R_plaidhip_colranks_dense", (DL_FUNC)&R_plaidhip_colranks_dense, 3},
    {"R_plaidhip_colranks_csc", (DL_FUNC)&R_plaidhip_colranks_csc, 4},
    {"R_plaidhip_colranks_csc_dense", (DL_FUNC)&R_plaidhip_colranks_csc_dense, 6},
    {"R_plaidhip_plaid_multi", (DL_FUNC)&R_plaidhip_plaid_multi, 10},
    {"R_plaidhip_sing_multi", (DL_FUNC)&R_plaidhip_sing_multi, 4},
    {"R_plaidhip_ssgsea_multi", (DL_FUNC)&R_plaidhip_ssgsea_multi, 9},
    {"R_plaidhip_sing_dense", (DL_FUNC)&R_plaidhip_sing_dense, 3},
    {"R_plaidhip_ssgsea_dense", (DL_FUNC)&R_plaidhip_ssgsea_dense, 4},
    {"R_plaidhip_ssgsea_csc", (DL_FUNC)&R_plaidhip_ssgsea_csc, 7},
    {"R_plaidhip_ucell_multi", (DL_FUNC)&R_plaidhip_ucell_multi, 10},
    {"R_plaidhip_aucell_multi", (DL_FUNC)&R_plaidhip_aucell_multi, 9},
    {"R_plaidhip_scse_multi", (DL_FUNC)&R_plaidhip_scse_multi, 10},
    {"R_plaidhip_gsva_multi", (DL_FUNC)&R_plaidhip_gsva_multi, 10},
    {"R_plaidhip_sing_exact", (DL_FUNC)&R_plaidhip_sing_exact, 12},
    {"R_plaidhip_ucell_exact", (DL_FUNC)&R_plaidhip_ucell_exact, 14},
    {"R_plaidhip_aucell_exact", (DL_FUNC)&R_plaidhip_aucell_exact, 9},
    {"R_plaidhip_gsva_exact", (DL_FUNC)&R_plaidhip_gsva_exact, 10},
    {"R_plaidhip_gsva_exact_multi", (DL_FUNC)&R_plaidhip_gsva_exact_multi, 11},
    {"R_plaidhip_ssgsea_exact", (DL_FUNC)&R_plaidhip_ssgsea_exact, 10},
    {"R_plaidhip_ssgsea_exact_multi", (DL_FUNC)&R_plaidhip_ssgsea_exact_multi, 11},
    {"R_plaidhip_ssgsea_exact_ks", (DL_FUNC)&R_plaidhip_ssgsea_exact_ks, 10},
    {"R_plaidhip_ssgsea_exact_ks_multi", (DL_FUNC)&R_plaidhip_ssgsea_exact_ks_multi, 11},
    {"R_plaidhip_ucell", (DL_FUNC)&R_plaidhip_ucell, 9},
    {"R_plaidhip_aucell", (DL_FUNC)&R_plaidhip_aucell, 8},
    {"R_plaidhip_scse", (DL_FUNC)&R_plaidhip_scse, 9},
    {"R_plaidhip_gmt2mat_file", (DL_FUNC)&R_plaidhip_gmt2mat_file, 6},
    {"R_plaidhip_plaid_test", (DL_FUNC)&R_plaidhip_plaid_test, 7},
    {"R_plaidhip_gsva", (DL_FUNC)&R_plaidhip_gsva, 5},
    {"R_plaidhip_plaid_test_csc", (DL_FUNC)&R_plaidhip_plaid_test_csc, 10},
    {"R_plaidhip_plaid_test_multi", (DL_FUNC)&R_plaidhip_plaid_test_multi, 12},
    {"R_plaidhip_plaid_test_contrasts", (DL_FUNC)&R_plaidhip_plaid_test_contrasts, 12},
    {"R_plaidhip_gsva_csc", (DL_FUNC)&R_plaidhip_gsva_csc, 8},
    {"R_plaidhip_gsea", (DL_FUNC)&R_plaidhip_gsea, 9},
    {"R_plaidhip_gsea_scored", (DL_FUNC)&R_plaidhip_gsea_scored, 11},
    {"R_plaidhip_gsea_multilevel", (DL_FUNC)&R_plaidhip_gsea_multilevel, 12},
    {"R_plaidhip_fisher", (DL_FUNC)&R_plaidhip_fisher, 5},
    {"R_plaidhip_limma", (DL_FUNC)&R_plaidhip_limma, 6},
    {"R_plaidhip_limma_na", (DL_FUNC)&R_plaidhip_limma_na, 7},
    {"R_plaidhip_limma_w", (DL_FUNC)&R_plaidhip_limma_w, 9},
    {"R_plaidhip_voom", (DL_FUNC)&R_plaidhip_voom, 5},
    {"R_plaidhip_camera", (DL_FUNC)&R_plaidhip_camera, 10},
    {"R_plaidhip_fry", (DL_FUNC)&R_plaidhip_fry, 9},
    {"R_plaidhip_roast", (DL_FUNC)&R_plaidhip_roast, 11},
    {"R_plaidhip_romer", (DL_FUNC)&R_plaidhip_romer, 11},
    {"R_plaidhip_rankcor", (DL_FUNC)&R_plaidhip_rankcor, 6},
    {"R_plaidhip_plage", (DL_FUNC)&R_plaidhip_plage, 11},
    {"R_plaidhip_zscore", (DL_FUNC)&R_plaidhip_zscore, 8},
    {NULL, NULL, 0}};

void R_init_plaidhip(DllInfo* dll) {
  R_registerRoutines(dll, NULL, call_methods, NULL, NULL);
  R_useDynamicSymbols(dll, FALSE);
}

void R_unload_plaidhip(DllInfo* dll) {
  (void)dll;
  if (g_ctx) { plaidhip_finalize(g_ctx); g_ctx = NULL; }
  plaidhip_multi_finalize();
}
