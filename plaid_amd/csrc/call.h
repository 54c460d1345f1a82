// One host-level scorer call: what it computes (Call), where it runs (Target), and the one way in (dispatch, multi.cpp).
// Host only: api.cpp, multi.cpp and the sharded engine (shard.h, shard.cpp, shard_*.cpp).
#pragma once

#include <vector>

#include "common.h"

namespace plaidhip {

// the ordinals are what the test hooks plaidhip_debug_sharded_on_one_device / _scorer_sharded_on_one_device take
enum Method : int {
  kPlaid = 0, kSing = 1, kSsgsea = 2, kUcell = 3, kAucell = 4, kScse = 5, kGsva = 6, kPlaidTest = 7, kSsgseaExact = 8,
  kGsvaExact = 9, kSingExact = 10, kUcellExact = 11, kAucellExact = 12, kPlaidTestContrasts = 13, kGsea = 14, kFisher = 15,
  kLimma = 16, kRankcor = 17, kPlage = 18, kZscore = 19, kGseaMultilevel = 20, kCamera = 21, kFry = 22, kRoast = 23,
  kVoom = 24, kRomer = 25
};
inline bool is_rank_sum(int method) { return method >= kPlaid && method <= kSsgsea; }   // shard_worker's three
inline bool is_scorer(int method) { return method >= kUcell && method <= kGsva; }       // scorer_worker's own four

// the matrix and the aligned set collection every scorer takes: X dense (Xp == nullptr) or the slots of a dgCMatrix
struct Operands {
  const int32_t* Xp;
  const int32_t* Xi;
  const double* X;   // dense values or CSC @x
  int32_t g, n;
  const int32_t* Gp;
  const int32_t* Gi;
  int32_t m;
};

struct Call : Operands {
  int method = kPlaid;
  int stat = PLAIDHIP_STAT_MEAN, normalize = 1;
  double alpha = 0.0;
  double* S_out = nullptr;
  const double* k_full = nullptr;   // ucell: set sizes
  double rmax = 0.0;                // ucell
  double auc_max_rank = 0.0;        // aucell
  int remove_log2 = -1;             // scse: < 0 decided from min / max of X
  int score_mean = 0;               // scse
  double tau = 0.0;                 // gsva
  int rowtf = 0;                    // gsva: 0 z, 1 ecdf (one shard); gsva.exact: 0 z, 1 ecdf (one shard), 2 none, 3 gauss
                                    // (every shard takes all of X)
  int max_diff = 1;                 // gsva.exact
  int* removed_log2 = nullptr;      // scse output (may be null)
  int scale = 1;                    // ssgsea.exact (its norm is `normalize`)
  int single = 1;                   // ssgsea.exact: 1 the walk's sum (closed form), 0 its value of largest magnitude (kernels_ks.hip)
  // plaid.test: the arguments of plaidhip_plaid_test and the group sizes of y (counted by check_call)
  const int32_t* y = nullptr;
  const double* gsetX = nullptr;
  int tests = 0, metap_method = 0;
  int64_t n0 = 0, n1 = 0;
  double* out = nullptr;
  // plaid.test.contrasts: y is Y (n x C, column-major, -1: the sample takes no part), out m x 6 x C; the group sizes of
  // every contrast (counted by check_call)
  int32_t ncontrast = 0;
  std::vector<int64_t> cn0, cn1;
  // sing.exact: the down sets (null: none), center, and the six nullable results (total, up, down score; total, up, down
  // dispersion)
  const int32_t* Dp = nullptr;
  const int32_t* Di = nullptr;
  int center = 1;
  double* sx_out[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // ucell.exact: maxRank (aucell.exact: aucMaxRank), w_neg, the down sets (Dp / Di), the imputed set sizes (k_full for the up
  // sets, k_full_down; null: the aligned sizes) and the nullable results sx_out[0..2] (total, up, down); aucell.exact: S_out
  double max_rank = 0.0;
  double w_neg = 1.0;
  const double* k_full_down = nullptr;
  // plaid.gsea: X is stat (g x n, n = the ranked lists, dense), out m x 12 x n; the weights beside stat, the caller's
  // placements (null: generated from seed), the permutations, the nullable m x nperm x n null scores; whether any weight
  // differs from 1 and which lists hold a NaN or an infinity (both found by check_call)
  const double* weight = nullptr;
  const int32_t* perm = nullptr;
  int32_t nperm = 0;
  uint64_t seed = 0;
  double* null_out = nullptr;
  int score_type = PLAIDHIP_GSEA_STD;   // the choice between the walk's extremes
  int32_t* le_len = nullptr;            // the leading edges (both null: none): m x n lengths,
  int32_t* le_idx = nullptr;            // Gp[m] x n rows of stat, a set's edge in its own segment of G
  int gsea_weighted = 0;
  std::vector<uint32_t> listnan;
  // plaid.gsea's multilevel p-values (kGseaMultilevel): plaid.gsea's fields and the sample size, the sweeps, eps, ml_min and
  // ml_out (m x 6 x n).  ml_ruler: ONE ruler instead (plaidhip_gsea_ruler) -- X / weight are one list, no sets; its size,
  // list number, side and target, and where its trace goes
  int32_t ml_sample = 0, ml_sweeps = 0, ml_min = 0;
  double ml_eps = 0.0;
  double* ml_out = nullptr;
  int ml_ruler = 0;
  int32_t ml_k = 0, ml_l = 0, ml_side = 0;
  double ml_gamma = 0.0;
  int32_t* ml_nstages = nullptr;
  int32_t* ml_end = nullptr;
  double* ml_m = nullptr;
  int32_t* ml_s = nullptr;
  double* ml_h = nullptr;
  // plaid.fisher: sig (g x n int8, n = the lists; X stays null), out m x 12 x n, the 2 x n list totals, and the overlap
  // lists in le_len / le_idx (both null: none)
  const int8_t* sig = nullptr;
  double* tot_out = nullptr;
  // plaid.rankcor: X is stat (g x n, n = the lists, dense; NaN: the gene takes no part in the list), out m x 5 x n, tot_out
  // the n universe sizes; ranks (with their ties) or values
  int use_rank = 1, ties = PLAIDHIP_TIES_AVERAGE;
  // replaid.plage: the stop test and the step cap of the power iteration, out m x 6 (the per-set statistics, nullable),
  // load_out Gp[m] loadings (nullable); replaid.zscore: out the m effective sizes (nullable)
  double tol = 0.0;
  int32_t maxit = 0;
  double* load_out = nullptr;
  // plaid.limma: X is A (g rows x n samples; no sets: Gp stays null, m = 0), the nfit designs (n x p each), use (n x nfit,
  // null: all), K (p x q, null: the unit vectors), out g x 6 x q x nfit and hyper nfit x 4; what check_call makes of the
  // designs: Q (n x p x nfit), 1 / n_f, n_f, v (p x q x nfit) and u (q x nfit)
  const double* design = nullptr;
  const int8_t* use = nullptr;
  const double* K = nullptr;
  int32_t ncoef = 0, nfit = 0, nq = 0;
  double* hyper = nullptr;
  std::vector<double> lm_Q, lm_invn, lm_v, lm_u;
  std::vector<int64_t> lm_nf;
  // plaid.limma with na = "fit" (plaidhip_limma_na): rows with at most max_na of their n values NaN are refitted on the
  // samples they have; dfres g x nfit, hyper nfit x 5
  int na_fit = 0;
  double max_na = 0.0;
  double* dfres = nullptr;
  // plaid.limma with weights (plaidhip_limma_w): Wt rows x n observation weights and / or aw, n array weights (one of them
  // may be null); max_na, dfres and hyper nfit x 5 as na = "fit"
  int weighted = 0;
  const double* Wt = nullptr;
  const double* aw = nullptr;
  // plaid.voom (kVoom): X is the counts (g rows x n samples), one design (n x ncoef), the library sizes (n, null: the column
  // sums) and the span of the trend; E and W (g x n each), the library sizes used and the offsets (n each), the trend's
  // knots (PLAIDHIP_VOOM_MAX_KNOTS each) and their number
  const double* voom_lib = nullptr;
  double voom_span = 0.5;
  double* voom_E = nullptr;
  double* voom_W = nullptr;
  double* voom_lib_out = nullptr;
  double* voom_off = nullptr;
  double* voom_kx = nullptr;
  double* voom_ky = nullptr;
  int32_t* voom_nk = nullptr;
  // plaid.camera (kCamera): plaid.limma's operands (X genes x n, designs, use, K) and the sets; the fixed inter-gene
  // correlation (NaN: estimated from the residuals), allow.neg.cor; out m x 8 x q x nfit, hyper nfit x 6
  double inter_gene_cor = 0.0;
  int allow_neg_cor = 0;
  // plaid.fry (kFry): plaid.camera's operands; standardize (PLAIDHIP_FRY_STANDARDIZE_*, fry.h); out m x 7 x q x nfit, hyper
  // nfit x 7; what check_call adds to plaid.limma's: Q2 of every fit under the cap (n x (n_f - p) at lm_Q2_off[f], -1: above)
  int standardize = 0;
  std::vector<double> lm_Q2;
  std::vector<int64_t> lm_Q2_off;
  // plaid.roast (kRoast): plaid.camera's operands; the set statistic and z-score (roast.h), nrot, seed, midp, the caller's
  // rotations (nfit x (n + 1) x nrot, or null: generated); out m x 8 x q x nfit, hyper nfit x 7
  int set_statistic = 0, zscore = 0, midp = 1;
  int32_t nrot = 0;
  uint64_t roast_seed = 0;
  const double* rotations = nullptr;
  // plaid.romer (kRomer): plaid.roast's operands (set_statistic 0..2 of romer.h, nrot, roast_seed, rotations); shrink_resid,
  // the caller's factors (g x q x nfit, or null: computed where shrink_resid is set); out m x 7 x q x nfit, hyper nfit x (8 + q)
  int shrink_resid = 1;
  const double* shrink = nullptr;
};

// ---- one builder per scorer: its own parameters, nothing else ----------------------------------------------------------
inline Call make_call(int method, const Operands& x, double* S_out) {
  Call c;
  static_cast<Operands&>(c) = x;
  c.method = method;
  c.S_out = S_out;
  return c;
}
// plaid / sing / ssgsea by ordinal: the hook's form, and its alone
inline Call rank_sum_call(int method, const Operands& x, int stat, int normalize, double alpha, double* S_out) {
  Call c = make_call(method, x, S_out);
  c.stat = stat;
  c.normalize = normalize;
  c.alpha = alpha;
  return c;
}
inline Call plaid_call(const Operands& x, int stat, int normalize, double* S_out) {
  Call c = make_call(kPlaid, x, S_out);
  c.stat = stat;
  c.normalize = normalize;
  return c;
}
// rX = colranks(X, ties.method="min") / nrow(X) - 0.5 ; plaid(rX, normalize=FALSE)  (R/plaid.R:215-217)
inline Call sing_call(const Operands& x, double* S_out) {
  Call c = make_call(kSing, x, S_out);
  c.normalize = 0;
  return c;
}
// rX = colranks(X, ties="average")^(1+alpha) ; rX/max(rX) - 0.5 ; plaid(mean, normalize=TRUE)  (R/plaid.R:245-253)
inline Call ssgsea_call(const Operands& x, double alpha, double* S_out) {
  Call c = make_call(kSsgsea, x, S_out);
  c.alpha = alpha;
  return c;
}
// ucell / aucell / scse / gsva by ordinal: the hook's form, and its alone; the parameters a method does not take are ignored
inline Call scorer_call(int method, const Operands& x, const double* k_full, double rmax, double auc_max_rank, int remove_log2,
                        int score_mean, double tau, int rowtf, double* S_out, int* removed_log2) {
  Call c = make_call(method, x, S_out);
  c.k_full = k_full;
  c.rmax = rmax;
  c.auc_max_rank = auc_max_rank;
  c.remove_log2 = remove_log2;
  c.score_mean = score_mean;
  c.tau = tau;
  c.rowtf = rowtf;
  c.removed_log2 = removed_log2;
  return c;
}
// pmin(max(rX) - rX, rmax + 1) of the average ranks, plaid(), 1 - S / rmax + (k + 1) / (2 rmax)   (R/plaid.R:278-280)
inline Call ucell_call(const Operands& x, const double* k_full, double rmax, double* S_out) {
  Call c = make_call(kUcell, x, S_out);
  c.k_full = k_full;
  c.rmax = rmax;
  return c;
}
// pmax(aucMaxRank - (max(rX) - rX), 0) of the average ranks, plaid()   (R/plaid.R:306-307)
inline Call aucell_call(const Operands& x, double auc_max_rank, double* S_out) {
  Call c = make_call(kAucell, x, S_out);
  c.auc_max_rank = auc_max_rank;
  return c;
}
// removeLog2 (< 0: decided from min / max of X, R/plaid.R:160-161), sX / (colMeans|X| + 1e-8) or its sum form (:176-182)
inline Call scse_call(const Operands& x, int remove_log2, int score_mean, double* S_out, int* removed_log2) {
  Call c = make_call(kScse, x, S_out);
  c.remove_log2 = remove_log2;
  c.score_mean = score_mean;
  c.removed_log2 = removed_log2;
  return c;
}
// zX = (X - rowMeans(X)) / (1e-8 + rowSds(X)) ("z", R/plaid.R:341-343) or t(apply(X, 1, function(x) ecdf(x)(x))) ("ecdf",
// :346), the signed average ranks of its columns, plaid()
inline Call gsva_call(const Operands& x, double tau, int rowtf, double* S_out) {
  Call c = make_call(kGsva, x, S_out);
  c.tau = tau;
  c.rowtf = rowtf;
  return c;
}
inline Call plaid_test_call(const Operands& x, const int32_t* y, const double* gsetX, int tests, int metap_method, double* out) {
  Call c = make_call(kPlaidTest, x, nullptr);
  c.y = y;
  c.gsetX = gsetX;
  c.tests = tests;
  c.metap_method = metap_method;
  c.out = out;
  return c;
}
// plaid.test(X[, sel_j], Y[sel_j, j], G, gsetX = S_all[, sel_j]) for every column j of Y, sel_j = which(!is.na(Y[, j]))
inline Call plaid_test_contrasts_call(const Operands& x, const int32_t* Y, int32_t C, const double* gsetX, int tests,
                                      int metap_method, double* out) {
  Call c = make_call(kPlaidTestContrasts, x, nullptr);
  c.y = Y;
  c.ncontrast = C;
  c.gsetX = gsetX;
  c.tests = tests;
  c.metap_method = metap_method;
  c.out = out;
  return c;
}
inline Call ssgsea_exact_call(const Operands& x, double alpha, int scale, int norm, double* S_out, int single) {
  Call c = make_call(kSsgseaExact, x, S_out);
  c.stat = PLAIDHIP_STAT_SUM;
  c.normalize = norm ? 1 : 0;
  c.alpha = alpha;
  c.scale = scale ? 1 : 0;
  c.single = single ? 1 : 0;
  return c;
}
inline Call gsva_exact_call(const Operands& x, double tau, int rowtf, int max_diff, double* S_out) {
  Call c = make_call(kGsvaExact, x, S_out);
  c.stat = PLAIDHIP_STAT_SUM;
  c.normalize = 0;
  c.tau = tau;
  c.rowtf = rowtf;
  c.max_diff = max_diff ? 1 : 0;
  return c;
}
inline Call sing_exact_call(const Operands& x, const int32_t* Dp, const int32_t* Di, int center, double* total, double* up,
                            double* down, double* total_disp, double* up_disp, double* down_disp) {
  Call c = make_call(kSingExact, x, nullptr);
  c.stat = PLAIDHIP_STAT_SUM;
  c.normalize = 0;
  c.Dp = Dp;
  c.Di = Di;
  c.center = center ? 1 : 0;
  double* const out[6] = {total, up, down, total_disp, up_disp, down_disp};
  for (int o = 0; o < 6; ++o) c.sx_out[o] = out[o];
  return c;
}
// maxRank = T; K = k_full (null: the aligned size); total = up - w_neg * down (include/plaidhip.h: plaidhip_ucell_exact)
inline Call ucell_exact_call(const Operands& x, const int32_t* Dp, const int32_t* Di, double max_rank, double w_neg,
                             const double* k_full, const double* k_full_down, double* total, double* up, double* down) {
  Call c = make_call(kUcellExact, x, nullptr);
  c.stat = PLAIDHIP_STAT_SUM;
  c.normalize = 0;
  c.Dp = Dp;
  c.Di = Di;
  c.max_rank = max_rank;
  c.w_neg = w_neg;
  c.k_full = k_full;
  c.k_full_down = k_full_down;
  c.sx_out[0] = total;
  c.sx_out[1] = up;
  c.sx_out[2] = down;
  return c;
}
inline Call aucell_exact_call(const Operands& x, double auc_max_rank, double* S_out) {
  Call c = make_call(kAucellExact, x, S_out);
  c.stat = PLAIDHIP_STAT_SUM;
  c.normalize = 0;
  c.max_rank = auc_max_rank;
  return c;
}
// fgseaSimple as pinned in include/plaidhip.h: plaidhip_gsea (std, no edges) and plaidhip_gsea_scored
inline Call gsea_call(const double* stat, const double* weight, int32_t g, int32_t c, const int32_t* Gp, const int32_t* Gi,
                      int32_t m, const int32_t* perm, int32_t nperm, uint64_t seed, double* out, double* null_out,
                      int score_type = PLAIDHIP_GSEA_STD, int32_t* le_len = nullptr, int32_t* le_idx = nullptr) {
  Call k = make_call(kGsea, {nullptr, nullptr, stat, g, c, Gp, Gi, m}, nullptr);
  k.weight = weight;
  k.perm = perm;
  k.nperm = nperm;
  k.seed = seed;
  k.out = out;
  k.null_out = null_out;
  k.score_type = score_type;
  k.le_len = le_len;
  k.le_idx = le_idx;
  return k;
}
// plaid.gsea with multilevel p-values as pinned in include/plaidhip.h: plaidhip_gsea_multilevel; one ruler's trace:
// plaidhip_gsea_ruler
inline Call gsea_multilevel_call(const double* stat, const double* weight, int32_t g, int32_t c, const int32_t* Gp,
                                 const int32_t* Gi, int32_t m, const int32_t* perm, int32_t nperm, uint64_t seed, int score_type,
                                 int32_t sample_size, int32_t sweeps, double eps, int32_t ml_min, double* out, double* null_out,
                                 int32_t* le_len, int32_t* le_idx, double* ml_out) {
  Call k = gsea_call(stat, weight, g, c, Gp, Gi, m, perm, nperm, seed, out, null_out, score_type, le_len, le_idx);
  k.method = kGseaMultilevel;
  k.ml_sample = sample_size;
  k.ml_sweeps = sweeps;
  k.ml_eps = eps;
  k.ml_min = ml_min;
  k.ml_out = ml_out;
  return k;
}
inline Call gsea_ruler_call(const double* stat, const double* weight, int32_t g, int32_t k, int32_t l, int side, int score_type,
                            double gamma, uint64_t seed, int32_t sample_size, int32_t sweeps, double eps, int32_t* nstages,
                            int32_t* end_status, double* m_out, int32_t* s_out, double* h_out) {
  Call c = make_call(kGseaMultilevel, {nullptr, nullptr, stat, g, 1, nullptr, nullptr, 0}, nullptr);
  c.weight = weight;
  c.seed = seed;
  c.score_type = score_type;
  c.ml_sample = sample_size;
  c.ml_sweeps = sweeps;
  c.ml_eps = eps;
  c.ml_ruler = 1;
  c.ml_k = k;
  c.ml_l = l;
  c.ml_side = side;
  c.ml_gamma = gamma;
  c.ml_nstages = nstages;
  c.ml_end = end_status;
  c.ml_m = m_out;
  c.ml_s = s_out;
  c.ml_h = h_out;
  return c;
}
// over-representation tests as pinned in include/plaidhip.h: plaidhip_fisher
inline Call fisher_call(const int8_t* sig, int32_t g, int32_t c, const int32_t* Gp, const int32_t* Gi, int32_t m, double* out,
                        double* tot_out, int32_t* ov_len, int32_t* ov_idx) {
  Call k = make_call(kFisher, {nullptr, nullptr, nullptr, g, c, Gp, Gi, m}, nullptr);
  k.sig = sig;
  k.out = out;
  k.tot_out = tot_out;
  k.le_len = ov_len;
  k.le_idx = ov_idx;
  return k;
}

// correlation of statistics or ranks with every set as pinned in include/plaidhip.h: plaidhip_rankcor
inline Call rankcor_call(const double* stat, int32_t g, int32_t c, const int32_t* Gp, const int32_t* Gi, int32_t m, int use_rank,
                         int ties, double* out, double* tot_out) {
  Call k = make_call(kRankcor, {nullptr, nullptr, stat, g, c, Gp, Gi, m}, nullptr);
  k.use_rank = use_rank;
  k.ties = ties;
  k.out = out;
  k.tot_out = tot_out;
  return k;
}

// GSVA's "plage" and "zscore" as pinned in include/plaidhip.h: plaidhip_plage, plaidhip_zscore
inline Call plage_call(const Operands& x, double tol, int32_t maxit, double* S_out, double* info_out, double* load_out) {
  Call k = make_call(kPlage, x, S_out);
  k.tol = tol;
  k.maxit = maxit;
  k.out = info_out;
  k.load_out = load_out;
  return k;
}
inline Call zscore_call(const Operands& x, double* S_out, double* size_out) {
  Call k = make_call(kZscore, x, S_out);
  k.stat = PLAIDHIP_STAT_SUM;
  k.normalize = 0;
  k.out = size_out;
  return k;
}

// lmFit + eBayes + topTable as pinned in include/plaidhip.h: plaidhip_limma
inline Call limma_call(const double* A, int32_t rows, int32_t n, const double* design, int32_t p, int32_t nfit, const int8_t* use,
                       const double* K, int32_t q, double* out, double* hyper) {
  Call k = make_call(kLimma, {nullptr, nullptr, A, rows, n, nullptr, nullptr, 0}, nullptr);
  k.design = design;
  k.ncoef = p;
  k.nfit = nfit;
  k.use = use;
  k.K = K;
  k.nq = q;
  k.out = out;
  k.hyper = hyper;
  return k;
}

// plaid.limma with na = "fit" as pinned in include/plaidhip.h: plaidhip_limma_na
inline Call limma_na_call(const double* A, int32_t rows, int32_t n, const double* design, int32_t p, int32_t nfit,
                          const int8_t* use, const double* K, int32_t q, double max_na, double* out, double* hyper,
                          double* dfres) {
  Call k = limma_call(A, rows, n, design, p, nfit, use, K, q, out, hyper);
  k.na_fit = 1;
  k.max_na = max_na;
  k.dfres = dfres;
  return k;
}

// plaid.limma with observation and / or array weights as pinned in include/plaidhip.h: plaidhip_limma_w
inline Call limma_w_call(const double* A, const double* Wt, const double* aw, int32_t rows, int32_t n, const double* design,
                         int32_t p, int32_t nfit, const int8_t* use, const double* K, int32_t q, double max_na, double* out,
                         double* hyper, double* dfres) {
  Call k = limma_call(A, rows, n, design, p, nfit, use, K, q, out, hyper);
  k.weighted = 1;
  k.Wt = Wt;
  k.aw = aw;
  k.max_na = max_na;
  k.dfres = dfres;
  return k;
}

// limma's voom (normalize.method = "none") as pinned in include/plaidhip.h: plaidhip_voom
inline Call voom_call(const double* counts, int32_t rows, int32_t n, const double* design, int32_t p, const double* lib_size,
                      double span, double* E, double* W, double* lib_out, double* offset, double* knots_x, double* knots_y,
                      int32_t* nknots) {
  Call k = limma_call(counts, rows, n, design, p, 1, nullptr, nullptr, p, nullptr, nullptr);
  k.method = kVoom;
  k.voom_lib = lib_size;
  k.voom_span = span;
  k.voom_E = E;
  k.voom_W = W;
  k.voom_lib_out = lib_out;
  k.voom_off = offset;
  k.voom_kx = knots_x;
  k.voom_ky = knots_y;
  k.voom_nk = nknots;
  return k;
}

// limma's competitive set test as pinned in include/plaidhip.h: plaidhip_camera
inline Call camera_call(const double* X, int32_t g, int32_t n, const double* design, int32_t p, int32_t nfit, const int8_t* use,
                        const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi, int32_t m, double inter_gene_cor,
                        int allow_neg_cor, double* out, double* hyper) {
  Call k = limma_call(X, g, n, design, p, nfit, use, K, q, out, hyper);
  k.method = kCamera;
  k.Gp = Gp;
  k.Gi = Gi;
  k.m = m;
  k.inter_gene_cor = inter_gene_cor;
  k.allow_neg_cor = allow_neg_cor ? 1 : 0;
  return k;
}

// limma's self-contained set test in closed form as pinned in include/plaidhip.h: plaidhip_fry
inline Call fry_call(const double* X, int32_t g, int32_t n, const double* design, int32_t p, int32_t nfit, const int8_t* use,
                     const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi, int32_t m, int standardize, double* out,
                     double* hyper) {
  Call k = limma_call(X, g, n, design, p, nfit, use, K, q, out, hyper);
  k.method = kFry;
  k.Gp = Gp;
  k.Gi = Gi;
  k.m = m;
  k.standardize = standardize;
  return k;
}

// limma's rotation set test with sampled rotations as pinned in include/plaidhip.h: plaidhip_roast
inline Call roast_call(const double* X, int32_t g, int32_t n, const double* design, int32_t p, int32_t nfit, const int8_t* use,
                       const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi, int32_t m, int set_statistic,
                       int zscore, int32_t nrot, uint64_t seed, int midp, const double* rotations, double* out, double* hyper) {
  Call k = limma_call(X, g, n, design, p, nfit, use, K, q, out, hyper);
  k.method = kRoast;
  k.Gp = Gp;
  k.Gi = Gi;
  k.m = m;
  k.set_statistic = set_statistic;
  k.zscore = zscore;
  k.nrot = nrot;
  k.roast_seed = seed;
  k.midp = midp;
  k.rotations = rotations;
  return k;
}

// limma's rotation GSEA on the ranks of the rotated moderated t as pinned in include/plaidhip.h: plaidhip_romer
inline Call romer_call(const double* X, int32_t g, int32_t n, const double* design, int32_t p, int32_t nfit, const int8_t* use,
                       const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi, int32_t m, int set_statistic,
                       int32_t nrot, uint64_t seed, int shrink_resid, const double* shrink, const double* rotations, double* out,
                       double* hyper) {
  Call k = roast_call(X, g, n, design, p, nfit, use, K, q, Gp, Gi, m, set_statistic, 1, nrot, seed, 0, rotations, out, hyper);
  k.method = kRomer;
  k.shrink_resid = shrink_resid;
  k.shrink = shrink;
  return k;
}

// ---- where a call runs -------------------------------------------------------------------------------------------------
struct Target {
  enum Kind { kContext, kDevices, kHook } kind;
  plaidhip_ctx* ctx;            // kContext: the caller's context (one shard)
  const int* devices;           // kDevices: plaidhip_*_multi's list (null: the first ndev devices)
  int device, ndev, fail_shard; // kHook: ndev contexts on `device`, shard fail_shard (>= 0) fails in its crossprod phase
};
inline Target on_context(plaidhip_ctx* ctx) { return Target{Target::kContext, ctx, nullptr, 0, 1, -1}; }
inline Target on_devices(const int* devices, int ndev) { return Target{Target::kDevices, nullptr, devices, 0, ndev, -1}; }
inline Target on_hook(int device, int nshards, int fail_shard) {
  return Target{Target::kHook, nullptr, nullptr, device, nshards, fail_shard};
}

// The one way in (multi.cpp): the device list's (or the hook's) own checks, check_call, a null context, the empty result,
// the contexts, run_call (shard.cpp).  Nothing before the contexts touches a device.
int dispatch(const Target& t, Call c);
// the argument checks of every method, which touch no device.  multi: a plaidhip_*_multi entry, which refuses replaid.gsva's
// rowtf = "ecdf" whatever the device count; the others take it on one shard.  Counts plaid.test's groups into c.n0 / c.n1.
int check_call(Call& c, int ndev, bool multi);

}  // namespace plaidhip
