// The way into the host engine (shard.cpp: one thread per device, the sample columns cut into shards): the shard bounds,
// the argument checks of every method (check_call, which touch no device), the contexts of the plaidhip_*_multi entries,
// dispatch, and every extern "C" multi-device entry and test hook.  What a method runs -- its worker, what it shares
// between the shards, its host half -- is route's (shard.cpp) and the worker families' (shard_*.cpp).
#include "shard.h"

using namespace plaidhip;

extern "C" int plaidhip_shard_bounds(int64_t n, int ndev, int k, int64_t* lo, int64_t* hi) try {
  PH_REQUIRE(n >= 0 && ndev > 0 && k >= 0 && k < ndev && lo && hi, "shard_bounds: bad arguments n=%lld ndev=%d k=%d",
             (long long)n, ndev, k);
  const int64_t per = (n + ndev - 1) / ndev;
  *lo = std::min(n, (int64_t)k * per);
  *hi = std::min(n, *lo + per);
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

namespace plaidhip {

// the bound of the walk kernel's bitmap (kernels_ks.hip), checked before a device is touched
int check_gsea_ks_genes(int32_t g) {
  if (g > PLAIDHIP_GSEA_KS_MAX_GENES) {
    set_error("ssgsea_exact_ks: nrow(X) = %d (at most %d rows with single = FALSE)", g, PLAIDHIP_GSEA_KS_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  return PLAIDHIP_OK;
}

}  // namespace plaidhip

// ---- the argument checks of every method: check_call.  None touches a device. -----------------------------------------------
namespace {

// plaid / sing / ssgsea
int check_rank_sum_call(const Call& c) {
  PH_TRY(check_host_common(c.Gp, c.g, c.n, c.m));
  if ((int64_t)c.m * c.n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(c.X != nullptr || (c.Xp != nullptr && c.Xp[c.n] == 0), "null X");
  PH_REQUIRE(c.S_out != nullptr, "null S_out");
  if (c.Xp != nullptr) PH_TRY(check_host_csc(c.Xp, c.Xi, c.g, c.n));
  return PLAIDHIP_OK;
}

// replaid.ssgsea.exact; replaid.gsva.exact and replaid.sing.exact (alpha 0) run it inside theirs.  S_out: the result, or
// any one of sing.exact's
int check_ssgsea_exact_call(const Call& c, const double* S_out) {
  PH_REQUIRE(std::isfinite(c.alpha), "ssgsea_exact: alpha must be finite (got %g)", c.alpha);
  PH_TRY(check_host_common(c.Gp, c.g, c.n, c.m));
  PH_REQUIRE(c.g < (1 << 26), "ssgsea_exact: nrow(X) = %d (at most 2^26 - 1 rows)", c.g);
  if ((int64_t)c.m * c.n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(c.Gi != nullptr || c.Gp[c.m] == 0, "ssgsea_exact: null Gi");
  PH_REQUIRE(c.X != nullptr || (c.Xp != nullptr && c.Xp[c.n] == 0), "ssgsea_exact: null X");
  PH_REQUIRE(S_out != nullptr, "ssgsea_exact: null S_out");
  if (c.Xp != nullptr) {
    const int32_t* Xp = c.Xp;
    const int32_t* Xi = c.Xi;
    PH_TRY(check_host_csc(Xp, Xi, c.g, c.n));
    PH_REQUIRE(Xp[c.n] == 0 || Xi != nullptr, "ssgsea_exact: null Xi");
    for (int32_t j = 0; j < c.n; ++j)   // the expansion walks the rows of a column in order (kernels_walk.hip)
      for (int32_t q = Xp[j] + 1; q < Xp[j + 1]; ++q)
        PH_REQUIRE(Xi[q] > Xi[q - 1], "ssgsea_exact: row indices of column %d are not increasing (Xi[%d] = %d after %d)", j, q,
                   Xi[q], Xi[q - 1]);
  }
  return PLAIDHIP_OK;
}

int check_gsva_exact_call(const Call& c, int ndev) {
  PH_REQUIRE(std::isfinite(c.tau) && c.tau >= 0.0, "gsva_exact: tau must be finite and >= 0 (got %g)", c.tau);
  PH_REQUIRE(c.rowtf >= 0 && c.rowtf <= 3, "Error: unknown row transform %d", c.rowtf);                     // R/plaid.R:348
  PH_REQUIRE(c.rowtf != 3 || c.n >= 2, "gsva_exact: rowtf = \"gauss\" needs at least 2 samples (got %d)", c.n);
  PH_REQUIRE(c.rowtf != 1 || ndev == 1, "gsva_exact_multi: rowtf = \"ecdf\" ranks all samples of a gene together and is not "
                                        "sharded by sample; score it on one device (plaidhip_gsva_exact)");
  PH_TRY(check_ssgsea_exact_call(c, c.S_out));
  if (c.g > PLAIDHIP_GSEA_KS_MAX_GENES) {
    set_error("gsva_exact: nrow(X) = %d (at most %d rows)", c.g, PLAIDHIP_GSEA_KS_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  return PLAIDHIP_OK;
}

int check_sing_exact_call(const Call& c) {
  double* const* out = c.sx_out;
  const double* any = nullptr;
  for (int o = 0; o < 6; ++o) any = any ? any : out[o];
  PH_REQUIRE((int64_t)c.m * c.n == 0 || any != nullptr, "sing_exact: no output requested");
  PH_TRY(check_ssgsea_exact_call(c, any));
  if (c.Dp != nullptr) {
    PH_TRY(check_host_common(c.Dp, c.g, c.n, c.m));
    PH_REQUIRE((int64_t)c.m * c.n == 0 || c.Di != nullptr || c.Dp[c.m] == 0, "sing_exact: null Di");
  } else {
    PH_REQUIRE(!out[0] && !out[2] && !out[3] && !out[5], "sing_exact: total and down results need the down sets");
  }
  if ((out[3] || out[4] || out[5]) && c.g > PLAIDHIP_GSEA_KS_MAX_GENES) {
    set_error("sing_exact: nrow(X) = %d (at most %d rows with the dispersion)", c.g, PLAIDHIP_GSEA_KS_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  return PLAIDHIP_OK;
}

// replaid.ucell.exact / replaid.aucell.exact.  The order is part of the contract: the rank bound and the 2^53 bound of the
// integer epilogue come before anything reads X.
int check_truncated_exact_call(const Call& c) {
  const bool ucell = c.method == kUcellExact;
  const char* who = ucell ? "ucell_exact" : "aucell_exact";
  const char* what = ucell ? "maxRank" : "aucMaxRank";
  const double* any = ucell ? nullptr : c.S_out;
  if (ucell) {
    for (int o = 0; o < 3; ++o) any = any ? any : c.sx_out[o];
    PH_REQUIRE(std::isfinite(c.w_neg) && c.w_neg >= 0.0, "ucell_exact: w_neg must be finite and >= 0 (got %g)", c.w_neg);
  }
  PH_TRY(check_host_common(c.Gp, c.g, c.n, c.m));
  if (ucell && c.Dp != nullptr) PH_TRY(check_host_common(c.Dp, c.g, c.n, c.m));
  if (ucell && c.Dp == nullptr)
    PH_REQUIRE(!c.sx_out[0] && !c.sx_out[2], "ucell_exact: total and down results need the down sets");
  if ((int64_t)c.m * c.n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(c.max_rank >= 1.0 && c.max_rank <= (double)c.g && c.max_rank == std::floor(c.max_rank),
             "%s: %s must be an integer in 1..nrow(X) = %d (got %g)", who, what, c.g, c.max_rank);
  if (2.0 * (double)c.g * c.max_rank >= 0x1p53) {
    set_error("%s: 2 nrow(X) %s = 2 x %d x %.0f does not stay below 2^53", who, what, c.g, c.max_rank);
    return PLAIDHIP_EUNSUPPORTED;
  }
  PH_REQUIRE(any != nullptr, "%s: no output requested", who);
  PH_TRY(check_ssgsea_exact_call(c, any));
  if (ucell && c.Dp != nullptr) PH_REQUIRE(c.Di != nullptr || c.Dp[c.m] == 0, "ucell_exact: null Di");
  if (ucell && c.k_full != nullptr) {
    PH_REQUIRE(c.Dp == nullptr || c.k_full_down != nullptr, "ucell_exact: impute needs k_full_down beside the down sets");
    for (int pass = 0; pass < (c.Dp != nullptr ? 2 : 1); ++pass) {
      const double* K = pass ? c.k_full_down : c.k_full;
      const int32_t* P = pass ? c.Dp : c.Gp;
      for (int32_t j = 0; j < c.m; ++j) {
        PH_REQUIRE(std::isfinite(K[j]) && K[j] == std::floor(K[j]) && K[j] >= (double)(P[j + 1] - P[j]),
                   "ucell_exact: k_full%s[%d] = %g is no integer >= the %d aligned members", pass ? "_down" : "", j, K[j],
                   P[j + 1] - P[j]);
        if (2.0 * K[j] * (c.max_rank + 1.0) + K[j] * (K[j] + 1.0) >= 0x1p53) {
          set_error("ucell_exact: k_full%s[%d] = %g with maxRank = %.0f does not stay below 2^53", pass ? "_down" : "", j, K[j],
                    c.max_rank);
          return PLAIDHIP_EUNSUPPORTED;
        }
      }
    }
  }
  return PLAIDHIP_OK;
}

// replaid.ucell / aucell / scse / gsva
int check_scorer_call(const Call& c, int ndev, bool multi) {
  if (c.method == kScse && c.removed_log2 != nullptr) *c.removed_log2 = c.remove_log2 > 0 ? 1 : 0;
  PH_REQUIRE(is_scorer(c.method), "scorer: bad method %d", c.method);
  PH_TRY(check_host_common(c.Gp, c.g, c.n, c.m));
  if (c.method == kUcell) PH_REQUIRE(c.rmax > 0, "ucell: rmax must be positive");
  if (c.method == kAucell) PH_REQUIRE(c.auc_max_rank > 0, "aucell: aucMaxRank must be positive");
  if (c.method == kGsva) {
    PH_REQUIRE(c.rowtf == 0 || c.rowtf == 1, "Error: unknown row transform %d", c.rowtf);              // R/plaid.R:348
    PH_REQUIRE(c.rowtf == 0 || (!multi && ndev == 1), "gsva: rowtf = \"ecdf\" ranks all samples of a gene together and is "
               "not sharded by sample; score it on one device (plaidhip_gsva / plaidhip_gsva_csc)");
  }
  if ((int64_t)c.m * c.n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(c.X != nullptr || (c.Xp != nullptr && c.Xp[c.n] == 0), "null X");
  PH_REQUIRE(c.S_out != nullptr, "null S_out");
  if (c.method == kUcell) PH_REQUIRE(c.k_full != nullptr, "ucell: null k_full");
  if (c.Xp != nullptr) {
    PH_TRY(check_host_csc(c.Xp, c.Xi, c.g, c.n));
    PH_REQUIRE(c.Xp[c.n] == 0 || c.Xi != nullptr, "null Xi");
    // (the ranks of the rows' stored values use a g x n buffer as scratch: a column repeating a row index could pass it)
    if (c.method == kGsva)
      PH_REQUIRE((int64_t)c.Xp[c.n] <= (int64_t)c.g * c.n, "gsva: %d stored values in a %d x %d matrix (repeated row "
                 "indices?)", c.Xp[c.n], c.g, c.n);
  }
  return PLAIDHIP_OK;
}

// plaid.test, and their messages; counts the groups of y into c.n0 / c.n1
int check_plaid_test_call(Call& c) {
  PH_TRY(check_host_common(c.Gp, c.g, c.n, c.m));
  PH_REQUIRE(c.m == 0 || c.out, "plaid_test: null out");
  PH_REQUIRE(c.n == 0 || ((c.Xp != nullptr || c.X != nullptr) && c.y != nullptr), "plaid_test: null X / y");
  PH_REQUIRE((c.tests & 7) != 0 && (c.tests & ~7) == 0, "plaid_test: tests is a bit mask of 1 (one), 2 (two), 4 (lm)");
  PH_REQUIRE(c.metap_method == 0 || c.metap_method == 1, "Invalid method: %d", c.metap_method);   // R/plaid.R:533
  c.n0 = c.n1 = 0;
  for (int32_t j = 0; j < c.n; ++j) {
    PH_REQUIRE(c.y[j] == 0 || c.y[j] == 1, "elements of y must be 0 or 1");                        // R/plaid.R:394
    if (c.y[j]) ++c.n1; else ++c.n0;
  }
  if (c.Xp != nullptr) {
    PH_TRY(check_host_csc(c.Xp, c.Xi, c.g, c.n));
    PH_REQUIRE(c.Xp[c.n] == 0 || (c.Xi && c.X), "plaid_test: null Xi/Xx");
  }
  return PLAIDHIP_OK;
}

// plaid.test.contrasts: plaid.test's checks with Y (n x C; 0, 1, -1 = NA) for y; counts every contrast's groups
int check_plaid_test_contrasts_call(Call& c) {
  PH_TRY(check_host_common(c.Gp, c.g, c.n, c.m));
  PH_REQUIRE(c.ncontrast >= 0 && c.ncontrast <= 65535, "plaid_test_contrasts: C = %d (0 <= C <= 65535)", c.ncontrast);
  PH_REQUIRE(c.m == 0 || c.ncontrast == 0 || c.out, "plaid_test_contrasts: null out");
  PH_REQUIRE(c.n == 0 || c.Xp != nullptr || c.X != nullptr, "plaid_test_contrasts: null X");
  PH_REQUIRE(c.n == 0 || c.ncontrast == 0 || c.y != nullptr, "plaid_test_contrasts: null Y");
  PH_REQUIRE((c.tests & 7) != 0 && (c.tests & ~7) == 0, "plaid_test: tests is a bit mask of 1 (one), 2 (two), 4 (lm)");
  PH_REQUIRE(c.metap_method == 0 || c.metap_method == 1, "Invalid method: %d", c.metap_method);   // R/plaid.R:533
  c.cn0.assign((size_t)c.ncontrast, 0);
  c.cn1.assign((size_t)c.ncontrast, 0);
  for (int32_t j = 0; j < c.ncontrast; ++j)
    for (int32_t i = 0; i < c.n; ++i) {
      const int32_t lab = c.y[(size_t)j * c.n + i];
      PH_REQUIRE(lab == 0 || lab == 1 || lab == -1, "elements of Y must be 0, 1 or NA (-1): contrast %d, sample %d is %d",
                 j + 1, i + 1, lab);
      if (lab == 1) ++c.cn1[(size_t)j];
      else if (lab == 0) ++c.cn0[(size_t)j];
    }
  if (c.Xp != nullptr) {
    PH_TRY(check_host_csc(c.Xp, c.Xi, c.g, c.n));
    PH_REQUIRE(c.Xp[c.n] == 0 || (c.Xi && c.X), "plaid_test_contrasts: null Xi/Xx");
  }
  return PLAIDHIP_OK;
}

// plaid.gsea; the order is part of the contract (include/plaidhip.h).  Finds whether any weight differs from 1 and the lists
// that hold a NaN or an infinity
int check_gsea_call(Call& c) {
  PH_REQUIRE(c.score_type >= PLAIDHIP_GSEA_STD && c.score_type <= PLAIDHIP_GSEA_NEG, "gsea: score_type = %d (0 std, 1 pos, 2 neg)",
             c.score_type);
  PH_REQUIRE((c.le_len == nullptr) == (c.le_idx == nullptr), "gsea: le_len and le_idx are passed both or neither");
  PH_REQUIRE(c.nperm >= 1, "gsea: nperm = %d (at least 1)", c.nperm);
  PH_REQUIRE(c.n >= 1, "gsea: %d ranked lists (at least 1)", c.n);
  PH_TRY(check_host_common(c.Gp, c.g, c.n, c.m));
  if (c.g > PLAIDHIP_GSEA_KS_MAX_GENES) {
    set_error("gsea: %d genes (at most %d)", c.g, PLAIDHIP_GSEA_KS_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  PH_REQUIRE(c.X != nullptr && c.weight != nullptr, "gsea: null stat / weight");
  c.gsea_weighted = 0;
  for (int64_t e = 0; e < (int64_t)c.g * c.n; ++e) {
    const double w = c.weight[e];
    PH_REQUIRE(std::isfinite(w) && w >= 0.0, "gsea: weight[%lld] = %g (weights are finite and >= 0)", (long long)e, w);
    if (w != 1.0) c.gsea_weighted = 1;
  }
  c.listnan.assign((size_t)c.n, 0u);
  for (int32_t l = 0; l < c.n; ++l)
    for (int32_t i = 0; i < c.g; ++i)
      if (!std::isfinite(c.X[(int64_t)l * c.g + i])) { c.listnan[(size_t)l] = 1u; break; }
  if (c.m == 0) return PLAIDHIP_OK;
  PH_REQUIRE(c.Gi != nullptr || c.Gp[c.m] == 0, "gsea: null Gi");
  PH_REQUIRE(c.out != nullptr, "gsea: null out");
  return PLAIDHIP_OK;
}

// the chains' own parameters, in the order of include/plaidhip.h
int check_gsea_ml_params(const Call& c, const char* who) {
  PH_REQUIRE(c.ml_sample >= 3 && c.ml_sample <= PLAIDHIP_GSEA_ML_MAX_SAMPLE && (c.ml_sample & 1) == 1,
             "%s: sample_size = %d (odd, 3..%d)", who, c.ml_sample, PLAIDHIP_GSEA_ML_MAX_SAMPLE);
  PH_REQUIRE(c.ml_sweeps >= 1 && c.ml_sweeps <= 32, "%s: sweeps = %d (1..32)", who, c.ml_sweeps);
  PH_REQUIRE(c.ml_eps >= 0.0 && c.ml_eps < 1.0, "%s: eps = %g (0 <= eps < 1)", who, c.ml_eps);
  return PLAIDHIP_OK;
}

// plaid.gsea with multilevel p-values, or one ruler; the order is part of the contract (include/plaidhip.h)
int check_gsea_multilevel_call(Call& c) {
  if (!c.ml_ruler) {
    PH_TRY(check_gsea_ml_params(c, "gsea_multilevel"));
    PH_REQUIRE(c.ml_min >= 0, "gsea_multilevel: ml_min = %d (at least 0)", c.ml_min);
    PH_REQUIRE(c.n < (1 << 30), "gsea_multilevel: %d ranked lists (below 2^30)", c.n);
    PH_REQUIRE(c.ml_out != nullptr || c.m == 0, "gsea_multilevel: null ml_out");
    return check_gsea_call(c);
  }
  PH_TRY(check_gsea_ml_params(c, "gsea_ruler"));
  PH_REQUIRE(c.ml_side == 0 || c.ml_side == 1, "gsea_ruler: side = %d (0 positive, 1 negative)", c.ml_side);
  PH_REQUIRE(c.ml_l >= 0 && c.ml_l < (1 << 30), "gsea_ruler: list number %d (0..2^30 - 1)", c.ml_l);
  PH_REQUIRE(c.g >= 2 && c.ml_k >= 1 && c.ml_k < c.g, "gsea_ruler: k = %d of %d genes (1..g - 1)", c.ml_k, c.g);
  PH_REQUIRE(c.ml_gamma == c.ml_gamma, "gsea_ruler: gamma is NaN");
  PH_REQUIRE(c.score_type >= PLAIDHIP_GSEA_STD && c.score_type <= PLAIDHIP_GSEA_NEG, "gsea_ruler: score_type = %d (0 std, 1 pos, 2 neg)",
             c.score_type);
  PH_REQUIRE(c.score_type == PLAIDHIP_GSEA_STD || c.ml_side == (c.score_type == PLAIDHIP_GSEA_NEG ? 1 : 0),
             "gsea_ruler: side = %d does not go with score_type = %d", c.ml_side, c.score_type);
  if (c.g > PLAIDHIP_GSEA_KS_MAX_GENES) {
    set_error("gsea_ruler: %d genes (at most %d)", c.g, PLAIDHIP_GSEA_KS_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  PH_REQUIRE(c.X != nullptr && c.weight != nullptr, "gsea_ruler: null stat / weight");
  PH_REQUIRE(c.ml_nstages && c.ml_end && c.ml_m && c.ml_s && c.ml_h, "gsea_ruler: null output");
  c.gsea_weighted = 0;
  for (int32_t i = 0; i < c.g; ++i) {
    const double w = c.weight[i];
    PH_REQUIRE(std::isfinite(w) && w >= 0.0, "gsea_ruler: weight[%d] = %g (weights are finite and >= 0)", i, w);
    PH_REQUIRE(std::isfinite(c.X[i]), "gsea_ruler: stat[%d] is not finite", i);
    if (w != 1.0) c.gsea_weighted = 1;
  }
  return PLAIDHIP_OK;
}

// plaid.fisher; the order is part of the contract (include/plaidhip.h)
int check_fisher_call(const Call& c) {
  PH_REQUIRE(c.n >= 1, "fisher: %d lists (at least 1)", c.n);
  PH_TRY(check_host_common(c.Gp, c.g, c.n, c.m));
  PH_REQUIRE(c.sig != nullptr && c.tot_out != nullptr && (c.out != nullptr || c.m == 0), "fisher: null sig / out / tot_out");
  PH_REQUIRE((c.le_len == nullptr) == (c.le_idx == nullptr), "fisher: ov_len and ov_idx are passed both or neither");
  if (c.g > PLAIDHIP_FISHER_MAX_GENES) {
    set_error("fisher: %d genes (at most %d)", c.g, PLAIDHIP_FISHER_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  PH_REQUIRE(c.Gp[0] == 0, "fisher: Gp[0] = %d (a column pointer starts at 0)", c.Gp[0]);
  for (int32_t j = 0; j < c.m; ++j)
    PH_REQUIRE(c.Gp[j + 1] >= c.Gp[j], "fisher: Gp[%d] = %d after %d (a column pointer does not decrease)", j + 1, c.Gp[j + 1],
               c.Gp[j]);
  PH_REQUIRE(c.Gi != nullptr || c.Gp[c.m] == 0, "fisher: null Gi");
  for (int32_t e = 0; e < c.Gp[c.m]; ++e)
    PH_REQUIRE(c.Gi[e] >= 0 && c.Gi[e] < c.g, "fisher: Gi[%d] = %d (rows are 0..%d)", e, c.Gi[e], c.g - 1);
  for (int64_t e = 0; e < (int64_t)c.g * c.n; ++e)
    PH_REQUIRE(c.sig[e] >= -1 && c.sig[e] <= 1, "fisher: sig[%lld] = %d (-1 down, 0, +1 up)", (long long)e, (int)c.sig[e]);
  return PLAIDHIP_OK;
}

// plaid.rankcor; the order is part of the contract (include/plaidhip.h)
int check_rankcor_call(const Call& c) {
  PH_REQUIRE(c.n >= 1, "rankcor: %d lists (at least 1)", c.n);
  PH_TRY(check_host_common(c.Gp, c.g, c.n, c.m));
  PH_REQUIRE(c.X != nullptr && c.tot_out != nullptr && (c.out != nullptr || c.m == 0), "rankcor: null stat / out / tot_out");
  PH_REQUIRE(c.use_rank == 0 || c.use_rank == 1, "rankcor: use_rank = %d (0 values, 1 ranks)", c.use_rank);
  PH_REQUIRE(c.ties == PLAIDHIP_TIES_AVERAGE || c.ties == PLAIDHIP_TIES_MIN || c.ties == PLAIDHIP_TIES_MAX,
             "rankcor: ties = %d (0 average, 1 min, 2 max)", c.ties);
  if (c.g > PLAIDHIP_RANKCOR_MAX_GENES) {
    set_error("rankcor: %d genes (at most %d)", c.g, PLAIDHIP_RANKCOR_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  PH_REQUIRE(c.Gp[0] == 0, "rankcor: Gp[0] = %d (a column pointer starts at 0)", c.Gp[0]);
  for (int32_t j = 0; j < c.m; ++j) {
    PH_REQUIRE(c.Gp[j + 1] >= c.Gp[j], "rankcor: Gp[%d] = %d after %d (a column pointer does not decrease)", j + 1, c.Gp[j + 1],
               c.Gp[j]);
    PH_REQUIRE(c.Gp[j + 1] - c.Gp[j] <= c.g, "rankcor: set %d has %d members (at most the %d genes)", j + 1,
               c.Gp[j + 1] - c.Gp[j], c.g);
  }
  PH_REQUIRE(c.Gi != nullptr || c.Gp[c.m] == 0, "rankcor: null Gi");
  for (int32_t e = 0; e < c.Gp[c.m]; ++e)
    PH_REQUIRE(c.Gi[e] >= 0 && c.Gi[e] < c.g, "rankcor: Gi[%d] = %d (rows are 0..%d)", e, c.Gi[e], c.g - 1);
  return PLAIDHIP_OK;
}

// replaid.plage and replaid.zscore; the order is part of the contract (include/plaidhip.h)
int check_plage_call(const Call& c) {
  const bool plage = c.method == kPlage;
  const char* who = plage ? "plage" : "zscore";
  PH_TRY(check_host_common(c.Gp, c.g, c.n, c.m));
  PH_REQUIRE(c.n >= 2, "%s: %d samples (at least 2)", who, c.n);
  if (plage) {
    PH_REQUIRE(c.tol > 0.0, "plage: tol = %g (a positive number)", c.tol);   // (a NaN is refused here too)
    PH_REQUIRE(c.maxit >= 1, "plage: maxit = %d (at least 1)", c.maxit);
  }
  PH_REQUIRE(c.Gp[0] == 0, "%s: Gp[0] = %d (a column pointer starts at 0)", who, c.Gp[0]);
  for (int32_t j = 0; j < c.m; ++j) {
    PH_REQUIRE(c.Gp[j + 1] >= c.Gp[j], "%s: Gp[%d] = %d after %d (a column pointer does not decrease)", who, j + 1, c.Gp[j + 1],
               c.Gp[j]);
    PH_REQUIRE(!plage || c.Gp[j + 1] - c.Gp[j] <= PLAIDHIP_PLAGE_MAX_SET, "plage: set %d has %d members (at most %d)", j + 1,
               c.Gp[j + 1] - c.Gp[j], PLAIDHIP_PLAGE_MAX_SET);
  }
  if (c.m == 0) return PLAIDHIP_OK;
  PH_REQUIRE(c.X != nullptr || (c.Xp != nullptr && c.Xp[c.n] == 0), "%s: null X", who);
  PH_REQUIRE(c.S_out != nullptr, "%s: null S_out", who);
  PH_REQUIRE(c.Gi != nullptr || c.Gp[c.m] == 0, "%s: null Gi", who);
  if (c.Xp != nullptr) {
    PH_TRY(check_host_csc(c.Xp, c.Xi, c.g, c.n));
    PH_REQUIRE(c.Xp[c.n] == 0 || c.Xi != nullptr, "%s: null Xi", who);
    for (int32_t j = 0; j < c.n; ++j)   // (the expansion takes a column's rows as sorted and distinct)
      for (int32_t q = c.Xp[j] + 1; q < c.Xp[j + 1]; ++q)
        PH_REQUIRE(c.Xi[q] > c.Xi[q - 1], "%s: row indices of column %d are not increasing (Xi[%d] = %d after %d)", who, j, q,
                   c.Xi[q], c.Xi[q - 1]);
  }
  for (int32_t e = 0; e < c.Gp[c.m]; ++e)
    PH_REQUIRE(c.Gi[e] >= 0 && c.Gi[e] < c.g, "%s: Gi[%d] = %d (rows are 0..%d)", who, e, c.Gi[e], c.g - 1);
  return PLAIDHIP_OK;
}

// plaid.limma; the order is part of the contract (include/plaidhip.h).  Makes every fit's Q, v, u and n_f: the designs are
// decomposed here, on the host, so that a design that cannot be fitted is refused before any device is touched
int check_limma_call(Call& c) {
  const char* who = c.method == kCamera ? "camera" : c.method == kFry ? "fry" : c.method == kRoast ? "roast" : c.method == kRomer ? "romer" : "limma";
  const bool sets = (c.method != kCamera && c.method != kFry && c.method != kRoast && c.method != kRomer) || c.m != 0;   // (plaid.camera without sets writes nothing)
  const int32_t rows = c.g, n = c.n, p = c.ncoef, nfit = c.nfit, q = c.nq;
  PH_REQUIRE(rows >= 0 && n >= 0 && n <= PLAIDHIP_LIMMA_MAX_SAMPLES && nfit >= 0 && nfit <= PLAIDHIP_LIMMA_MAX_FITS && q >= 0,
             "%s: bad dims rows=%d n=%d nfit=%d q=%d (n <= %d, nfit <= %d)", who, rows, n, nfit, q, PLAIDHIP_LIMMA_MAX_SAMPLES,
             PLAIDHIP_LIMMA_MAX_FITS);
  PH_REQUIRE(p >= 1 && p <= PLAIDHIP_LIMMA_MAX_COEF, "%s: p = %d coefficients (1 <= p <= %d)", who, p, PLAIDHIP_LIMMA_MAX_COEF);
  if (c.na_fit) {
    PH_REQUIRE(p <= PLAIDHIP_LIMMA_NA_MAX_COEF, "%s: p = %d coefficients with na = \"fit\" (p <= %d)", who, p,
               PLAIDHIP_LIMMA_NA_MAX_COEF);
    PH_REQUIRE(c.max_na >= 0.0 && c.max_na <= 1.0, "%s: max_na = %g (a share, 0 <= max_na <= 1)", who, c.max_na);
  }
  if (c.weighted) {
    PH_REQUIRE(p <= PLAIDHIP_LIMMA_NA_MAX_COEF, "%s: p = %d coefficients with weights (p <= %d)", who, p,
               PLAIDHIP_LIMMA_NA_MAX_COEF);
    PH_REQUIRE(c.max_na >= 0.0 && c.max_na <= 1.0, "%s: max_na = %g (a share, 0 <= max_na <= 1)", who, c.max_na);
    PH_REQUIRE(c.Wt != nullptr || c.aw != nullptr, "%s: weights: Wt and aw are both null (plaidhip_limma takes no weights)", who);
    PH_REQUIRE(lmfit_tiles((int64_t)nfit * lmfit_w_columns(p)) <= 65535,
               "%s: nfit = %d fits of p = %d coefficients with weights: %lld tiles of weight columns (at most 65535)", who, nfit,
               p, (long long)lmfit_tiles((int64_t)nfit * lmfit_w_columns(p)));
  }
  PH_REQUIRE(c.K != nullptr || q == p, "%s: q = %d without K (the p = %d unit vectors)", who, q, p);
  PH_REQUIRE(c.design != nullptr || nfit == 0, "%s: null design", who);
  PH_REQUIRE(rows == 0 || nfit == 0 || q == 0 || !sets || (c.X != nullptr && c.out != nullptr && c.hyper != nullptr),
             "%s: null A / out / hyper", who);
  PH_REQUIRE((!c.na_fit && !c.weighted) || rows == 0 || nfit == 0 || q == 0 || c.dfres != nullptr, "%s: null dfres", who);
  if (c.K != nullptr)
    for (int64_t e = 0; e < (int64_t)p * q; ++e)
      PH_REQUIRE(std::isfinite(c.K[e]), "%s: K[%lld] = %g (the contrasts are finite)", who, (long long)e, c.K[e]);
  c.lm_Q.assign((size_t)n * p * nfit, 0.0);
  c.lm_v.assign((size_t)p * q * nfit, 0.0);
  c.lm_u.assign((size_t)q * nfit, 0.0);
  c.lm_nf.assign((size_t)nfit, 0);
  c.lm_invn.assign((size_t)nfit, 0.0);
  // plaid.fry: the same decomposition also gives Q2 (n x d at lm_Q2_off[f]) of every fit with 1 <= d and d + 1 effects
  // under the cap; d is known from the count of used samples
  c.lm_Q2_off.assign((size_t)nfit, -1);
  if (c.method == kFry && rows != 0 && q != 0 && c.m > 0) {
    size_t total = 0;
    for (int32_t f = 0; f < nfit; ++f) {
      int64_t nf = n;
      if (c.use != nullptr) nf = std::count_if(c.use + (size_t)f * n, c.use + (size_t)(f + 1) * n, [](int8_t u) { return u != 0; });
      const int64_t d = nf - p;
      if (d < 1 || d + 1 > PLAIDHIP_FRY_MIXED_MAX) continue;
      c.lm_Q2_off[(size_t)f] = (int64_t)total;
      total += (size_t)n * (size_t)d;
    }
    c.lm_Q2.assign(total, 0.0);
  }
  for (int32_t f = 0; f < nfit; ++f) {
    PH_TRY(limma_design(who, c.design + (size_t)f * n * p, n, p, c.use != nullptr ? c.use + (size_t)f * n : nullptr, c.K, q,
                        f + 1, c.lm_Q.data() + (size_t)f * n * p, nullptr, c.lm_v.data() + (size_t)f * p * q,
                        c.lm_u.data() + (size_t)f * q, &c.lm_nf[(size_t)f],
                        c.lm_Q2_off[(size_t)f] >= 0 ? c.lm_Q2.data() + c.lm_Q2_off[(size_t)f] : nullptr));
    c.lm_invn[(size_t)f] = 1.0 / (double)c.lm_nf[(size_t)f];
  }
  return PLAIDHIP_OK;
}

// plaid.voom; the order is part of the contract (include/plaidhip.h).  The design is decomposed here, as plaid.limma's
int check_voom_call(Call& c) {
  const int32_t rows = c.g, n = c.n, p = c.ncoef;
  PH_REQUIRE(rows >= 0 && n >= 0 && n <= PLAIDHIP_LIMMA_MAX_SAMPLES, "voom: bad dims rows=%d n=%d (n <= %d)", rows, n,
             PLAIDHIP_LIMMA_MAX_SAMPLES);
  PH_REQUIRE(p >= 1 && p <= PLAIDHIP_LIMMA_MAX_COEF, "voom: p = %d coefficients (1 <= p <= %d)", p, PLAIDHIP_LIMMA_MAX_COEF);
  PH_REQUIRE(c.voom_span > 0.0 && c.voom_span <= 1.0, "voom: span = %g (0 < span <= 1)", c.voom_span);
  PH_REQUIRE(c.design != nullptr, "voom: null design");
  if (rows == 0 || n == 0) return PLAIDHIP_OK;
  PH_REQUIRE(c.X && c.voom_E && c.voom_W && c.voom_lib_out && c.voom_off && c.voom_kx && c.voom_ky && c.voom_nk,
             "voom: null counts / E / weights / lib.size / offset / knots");
  if (c.voom_lib != nullptr)
    for (int32_t s = 0; s < n; ++s)
      PH_REQUIRE(std::isfinite(c.voom_lib[s]) && c.voom_lib[s] >= 0.0, "voom: lib.size[%d] = %g (finite and >= 0)", s + 1,
                 c.voom_lib[s]);
  c.lm_Q.assign((size_t)n * p, 0.0);
  c.lm_v.assign((size_t)p * p, 0.0);
  c.lm_u.assign((size_t)p, 0.0);
  c.lm_nf.assign(1, 0);
  PH_TRY(limma_design("voom", c.design, n, p, nullptr, nullptr, p, 1, c.lm_Q.data(), nullptr, c.lm_v.data(), c.lm_u.data(),
                      &c.lm_nf[0], nullptr));
  c.lm_invn.assign(1, 1.0 / (double)c.lm_nf[0]);
  return PLAIDHIP_OK;
}

// plaid.camera; the order is part of the contract (include/plaidhip.h): plaid.limma's checks in their order (the designs are
// decomposed there), then the membership's as plaid.rankcor makes them, then the fixed correlation
int check_camera_call(Call& c) {
  const char* who = c.method == kFry ? "fry" : c.method == kRoast ? "roast" : c.method == kRomer ? "romer" : "camera";
  PH_REQUIRE(c.m >= 0, "%s: bad dims m=%d", who, c.m);
  PH_TRY(check_limma_call(c));
  PH_REQUIRE(c.Gp != nullptr, "%s: null Gp", who);
  PH_REQUIRE(c.Gp[0] == 0, "%s: Gp[0] = %d (a column pointer starts at 0)", who, c.Gp[0]);
  for (int32_t j = 0; j < c.m; ++j) {
    PH_REQUIRE(c.Gp[j + 1] >= c.Gp[j], "%s: Gp[%d] = %d after %d (a column pointer does not decrease)", who, j + 1,
               c.Gp[j + 1], c.Gp[j]);
    PH_REQUIRE(c.Gp[j + 1] - c.Gp[j] <= c.g, "%s: set %d has %d members (at most the %d genes)", who, j + 1,
               c.Gp[j + 1] - c.Gp[j], c.g);
  }
  PH_REQUIRE(c.Gi != nullptr || c.Gp[c.m] == 0, "%s: null Gi", who);
  for (int32_t e = 0; e < c.Gp[c.m]; ++e)
    PH_REQUIRE(c.Gi[e] >= 0 && c.Gi[e] < c.g, "%s: Gi[%d] = %d (rows are 0..%d)", who, e, c.Gi[e], c.g - 1);
  if (c.method == kFry || c.method == kRoast || c.method == kRomer) return PLAIDHIP_OK;
  PH_REQUIRE(std::isnan(c.inter_gene_cor) || (c.inter_gene_cor > -1.0 && c.inter_gene_cor < 1.0),
             "camera: inter_gene_cor = %g (a correlation inside (-1, 1), or NaN to estimate it)", c.inter_gene_cor);
  return PLAIDHIP_OK;
}

// plaid.fry; the order is part of the contract (include/plaidhip.h): plaid.camera's checks of the fit and of the membership,
// then standardize and the number of contrasts.  Q2 of every fit under the cap comes out of plaid.limma's one decomposition
// (check_limma_call)
int check_fry_call(Call& c) {
  PH_TRY(check_camera_call(c));
  PH_REQUIRE(c.standardize >= 0 && c.standardize <= 2, "fry: standardize = %d (0 posterior.sd, 1 residual.sd, 2 none)",
             c.standardize);
  PH_REQUIRE(c.nq <= PLAIDHIP_FRY_MAX_CONTRASTS, "fry: q = %d contrasts (at most %d)", c.nq, PLAIDHIP_FRY_MAX_CONTRASTS);
  return PLAIDHIP_OK;
}

// plaid.roast; the order is part of the contract (include/plaidhip.h): plaid.camera's checks of the fit and of the membership,
// then the set statistic, the z-score and the number of rotations
int check_roast_call(Call& c) {
  PH_TRY(check_camera_call(c));
  PH_REQUIRE(c.set_statistic >= 0 && c.set_statistic <= 3, "roast: set_statistic = %d (0 mean, 1 floormean, 2 msq, 3 mean50)",
             c.set_statistic);
  PH_REQUIRE(c.zscore >= 0 && c.zscore <= 1, "roast: zscore = %d (0 hill, 1 none)", c.zscore);
  PH_REQUIRE(c.nrot >= 1, "roast: nrot = %d rotations (at least 1)", c.nrot);
  PH_REQUIRE(c.nrot <= PLAIDHIP_ROAST_MAX_ROTATIONS, "roast: nrot = %d rotations (at most %d)", c.nrot,
             PLAIDHIP_ROAST_MAX_ROTATIONS);
  return PLAIDHIP_OK;
}

// plaid.romer; the order is part of the contract (include/plaidhip.h): plaid.roast's checks of the fit and of the membership,
// then the set statistic and the number of rotations
int check_romer_call(Call& c) {
  PH_TRY(check_camera_call(c));
  PH_REQUIRE(c.set_statistic >= 0 && c.set_statistic <= 2, "romer: set_statistic = %d (0 mean, 1 floormean, 2 mean50)",
             c.set_statistic);
  PH_REQUIRE(c.nrot >= 1, "romer: nrot = %d rotations (at least 1)", c.nrot);
  PH_REQUIRE(c.nrot <= PLAIDHIP_ROAST_MAX_ROTATIONS, "romer: nrot = %d rotations (at most %d)", c.nrot,
             PLAIDHIP_ROAST_MAX_ROTATIONS);
  if (c.g > PLAIDHIP_ROMER_MAX_GENES) {
    set_error("romer: %d genes (at most %d)", c.g, PLAIDHIP_ROMER_MAX_GENES);
    return PLAIDHIP_EUNSUPPORTED;
  }
  return PLAIDHIP_OK;
}

std::mutex g_multi_mu;
std::vector<plaidhip_ctx*> g_multi_ctx;  // one lazily created context per device, owned by the library
int g_multi_precision = PLAIDHIP_PRECISION_F64;   // plaidhip_multi_set_precision: applies to these contexts

// the device list's own checks, which touch no device
int check_devices(const int* devices, int ndev) {
  PH_REQUIRE(ndev >= 1 && ndev <= 64, "multi: ndev = %d", ndev);
  if (devices != nullptr)
    for (int k = 0; k < ndev; ++k)
      for (int q = 0; q < k; ++q) PH_REQUIRE(devices[q] != devices[k], "multi: device %d listed twice", devices[k]);
  return PLAIDHIP_OK;
}

int multi_contexts(const int* devices, int ndev, std::vector<plaidhip_ctx*>& out) {
  int count = 0;
  PH_TRY(plaidhip_device_count(&count));
  std::lock_guard<std::mutex> lk(g_multi_mu);
  if ((int)g_multi_ctx.size() < count) g_multi_ctx.resize((size_t)count, nullptr);
  out.clear();
  for (int k = 0; k < ndev; ++k) {
    const int d = devices ? devices[k] : k;
    PH_REQUIRE(d >= 0 && d < count, "multi: device %d out of range [0, %d)", d, count);
    if (g_multi_ctx[(size_t)d] == nullptr) PH_TRY(plaidhip_init(d, nullptr, &g_multi_ctx[(size_t)d]));
    g_multi_ctx[(size_t)d]->precision = g_multi_precision;
    out.push_back(g_multi_ctx[(size_t)d]);
  }
  return PLAIDHIP_OK;
}

// The test hooks' engine: `nshards` contexts on ONE device -- worker threads, rendezvous, cross-shard scalars and the
// failure path are what a 1-GPU box can exercise of plaidhip_*_multi.  fail_shard >= 0: that shard fails in its crossprod
// phase (the call must return an error, not hang).  The error text of the call outlives the contexts' release.
int run_on_one_device(int device, int nshards, int fail_shard, const Call& c) {
  std::vector<plaidhip_ctx*> ctxs((size_t)nshards, nullptr);
  int rc = PLAIDHIP_OK;
  for (int k = 0; k < nshards && rc == PLAIDHIP_OK; ++k) {
    rc = plaidhip_init(device, nullptr, &ctxs[(size_t)k]);
    if (rc == PLAIDHIP_OK && k == fail_shard) ctxs[(size_t)k]->debug_fail_crossprod = 1;
  }
  if (rc == PLAIDHIP_OK) rc = run_call(ctxs.data(), nshards, c);
  const std::string err = rc != PLAIDHIP_OK ? std::string(last_error_cstr()) : std::string();
  for (plaidhip_ctx* x : ctxs)
    if (x) plaidhip_finalize(x);
  if (rc != PLAIDHIP_OK) set_error("%s", err.c_str());
  return rc;
}

}  // namespace

namespace plaidhip {

int check_call(Call& c, int ndev, bool multi) {
  if (is_rank_sum(c.method)) return check_rank_sum_call(c);
  switch (c.method) {
    case kPlaidTest: return check_plaid_test_call(c);
    case kPlaidTestContrasts: return check_plaid_test_contrasts_call(c);
    case kGsea: return check_gsea_call(c);
    case kGseaMultilevel: return check_gsea_multilevel_call(c);
    case kFisher: return check_fisher_call(c);
    case kRankcor: return check_rankcor_call(c);
    case kPlage:
    case kZscore: return check_plage_call(c);
    case kLimma: return check_limma_call(c);
    case kCamera: return check_camera_call(c);
    case kFry: return check_fry_call(c);
    case kRoast: return check_roast_call(c);
    case kRomer: return check_romer_call(c);
    case kVoom: return check_voom_call(c);
    case kSsgseaExact:
      PH_TRY(check_ssgsea_exact_call(c, c.S_out));
      return c.single ? PLAIDHIP_OK : check_gsea_ks_genes(c.g);
    case kGsvaExact: return check_gsva_exact_call(c, ndev);
    case kSingExact: return check_sing_exact_call(c);
    case kUcellExact:
    case kAucellExact: return check_truncated_exact_call(c);
    default: return check_scorer_call(c, ndev, multi);   // (which refuses what is no method at all)
  }
}

int dispatch(const Target& t, Call c) {
  // (the shard count first: check_call reads it.  A null context after the arguments: tests reach the checks without one)
  if (t.kind == Target::kDevices) PH_TRY(check_devices(t.devices, t.ndev));
  if (t.kind == Target::kHook) PH_REQUIRE(t.ndev >= 1 && t.ndev <= 64, "debug_sharded: nshards = %d", t.ndev);
  PH_TRY(check_call(c, t.ndev, t.kind == Target::kDevices));
  if (t.kind == Target::kContext) PH_REQUIRE(t.ctx != nullptr, "null plaidhip_ctx");
  if (route(c).empty(c)) return PLAIDHIP_OK;
  if (t.kind == Target::kHook) return run_on_one_device(t.device, t.ndev, t.fail_shard, c);
  std::vector<plaidhip_ctx*> ctxs(1, t.ctx);
  if (t.kind == Target::kContext)
    PH_HIP(hipSetDevice(t.ctx->device));
  else
    PH_TRY(multi_contexts(t.devices, t.ndev, ctxs));
  return run_call(ctxs.data(), t.ndev, c);
}

}  // namespace plaidhip

// ---- multi-device entry points (include/plaidhip.h) and the test hooks: build the Call, dispatch ------------------------------
extern "C" {

int plaidhip_multi_set_precision(int mode) try {
  PH_REQUIRE(mode == PLAIDHIP_PRECISION_F64 || mode == PLAIDHIP_PRECISION_MIXED, "multi_set_precision: bad mode %d", mode);
  std::lock_guard<std::mutex> lk(g_multi_mu);
  g_multi_precision = mode;
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_multi_finalize(void) try {
  std::lock_guard<std::mutex> lk(g_multi_mu);
  for (plaidhip_ctx*& c : g_multi_ctx)
    if (c) { plaidhip_finalize(c); c = nullptr; }
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

// Each plaidhip_*_multi entry; then the test hooks (not part of include/plaidhip.h): the same calls on `nshards` contexts of
// one device (run_on_one_device), so a hook's signature is its entry's with (device, nshards, fail_shard) for (devices,
// ndev).  Two hooks serve several entries by Method ordinal: plaid / sing / ssgsea (0 - 2) and ucell / aucell / scse /
// gsva (3 - 6; the parameters a method does not take are ignored).

int plaidhip_plaid_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g,
                         int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, int stat, int normalize, double* S_out) try {
  PH_REQUIRE(stat == PLAIDHIP_STAT_MEAN || stat == PLAIDHIP_STAT_SUM, "plaid_multi: bad stat %d", stat);
  return dispatch(on_devices(devices, ndev), plaid_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, stat, normalize, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_sing_multi(const int* devices, int ndev, const double* X, int32_t g, int32_t n, const int32_t* Gp,
                        const int32_t* Gi, int32_t m, double* S_out) try {
  return dispatch(on_devices(devices, ndev), sing_call({nullptr, nullptr, X, g, n, Gp, Gi, m}, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_sing_csc_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* Xx, int32_t g,
                            int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double* S_out) try {
  PH_REQUIRE(Xp != nullptr, "sing_csc_multi: null Xp");
  return dispatch(on_devices(devices, ndev), sing_call({Xp, Xi, Xx, g, n, Gp, Gi, m}, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_ssgsea_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g,
                          int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha, double* S_out) try {
  return dispatch(on_devices(devices, ndev), ssgsea_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, alpha, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_ucell_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g,
                         int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, const double* k_full, double rmax,
                         double* S_out) try {
  return dispatch(on_devices(devices, ndev), ucell_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, k_full, rmax, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_aucell_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g,
                          int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double auc_max_rank, double* S_out) try {
  return dispatch(on_devices(devices, ndev), aucell_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, auc_max_rank, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_scse_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g,
                        int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, int remove_log2, int score_mean,
                        double* S_out, int* removed_log2) try {
  return dispatch(on_devices(devices, ndev),
                  scse_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, remove_log2, score_mean, S_out, removed_log2));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_gsva_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g,
                        int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double tau, int rowtf, double* S_out) try {
  return dispatch(on_devices(devices, ndev), gsva_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, tau, rowtf, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_plaid_test_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                              int32_t g, int32_t n, const int32_t* y, const int32_t* Gp, const int32_t* Gi, int32_t m,
                              const double* gsetX, int tests, int metap_method, double* out) try {
  return dispatch(on_devices(devices, ndev),
                  plaid_test_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, y, gsetX, tests, metap_method, out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_plaid_test_contrasts_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi,
                                        const double* X_or_x, int32_t g, int32_t n, const int32_t* Y, int32_t C,
                                        const int32_t* Gp, const int32_t* Gi, int32_t m, const double* gsetX, int tests,
                                        int metap_method, double* out) try {
  return dispatch(on_devices(devices, ndev),
                  plaid_test_contrasts_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, Y, C, gsetX, tests, metap_method, out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_ssgsea_exact_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                                int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha, int scale,
                                int norm, double* S_out) try {
  return dispatch(on_devices(devices, ndev), ssgsea_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, alpha, scale, norm, S_out, 1));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_ssgsea_exact_ks_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                                   int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha,
                                   int scale, int norm, double* S_out) try {
  return dispatch(on_devices(devices, ndev), ssgsea_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, alpha, scale, norm, S_out, 0));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_gsva_exact_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                              int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double tau, int rowtf,
                              int max_diff, double* S_out) try {
  return dispatch(on_devices(devices, ndev), gsva_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, tau, rowtf, max_diff, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_sing_exact_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                              int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, const int32_t* Dp, const int32_t* Di,
                              int32_t m, int center, double* total, double* up, double* down, double* total_disp,
                              double* up_disp, double* down_disp) try {
  return dispatch(on_devices(devices, ndev), sing_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, Dp, Di, center, total, up, down,
                                                             total_disp, up_disp, down_disp));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_sharded_on_one_device(int device, int nshards, int fail_shard, int method, const int32_t* Xp,
                                         const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n, const int32_t* Gp,
                                         const int32_t* Gi, int32_t m, int stat, int normalize, double alpha, double* S_out) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  rank_sum_call(method, {Xp, Xi, X_or_x, g, n, Gp, Gi, m}, stat, normalize, alpha, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_scorer_sharded_on_one_device(int device, int nshards, int fail_shard, int method, const int32_t* Xp,
                                                const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                                                const int32_t* Gp, const int32_t* Gi, int32_t m, const double* k_full,
                                                double rmax, double auc_max_rank, int remove_log2, int score_mean, double tau,
                                                int rowtf, double* S_out, int* removed_log2) try {
  PH_REQUIRE(is_scorer(method), "scorer: bad method %d", method);   // (the ordinal picks the checks: none but these four)
  return dispatch(on_hook(device, nshards, fail_shard),
                  scorer_call(method, {Xp, Xi, X_or_x, g, n, Gp, Gi, m}, k_full, rmax, auc_max_rank, remove_log2, score_mean, tau,
                              rowtf, S_out, removed_log2));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_plaid_test_sharded_on_one_device(int device, int nshards, int fail_shard, const int32_t* Xp,
                                                    const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                                                    const int32_t* y, const int32_t* Gp, const int32_t* Gi, int32_t m,
                                                    const double* gsetX, int tests, int metap_method, double* out) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  plaid_test_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, y, gsetX, tests, metap_method, out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_plaid_test_contrasts_sharded_on_one_device(int device, int nshards, int fail_shard, const int32_t* Xp,
                                                              const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                                                              const int32_t* Y, int32_t C, const int32_t* Gp,
                                                              const int32_t* Gi, int32_t m, const double* gsetX, int tests,
                                                              int metap_method, double* out) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  plaid_test_contrasts_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, Y, C, gsetX, tests, metap_method, out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_ssgsea_exact_sharded_on_one_device(int device, int nshards, int fail_shard, const int32_t* Xp,
                                                      const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                                                      const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha, int scale,
                                                      int norm, double* S_out) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  ssgsea_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, alpha, scale, norm, S_out, 1));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_ssgsea_exact_ks_sharded_on_one_device(int device, int nshards, int fail_shard, const int32_t* Xp,
                                                         const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                                                         const int32_t* Gp, const int32_t* Gi, int32_t m, double alpha,
                                                         int scale, int norm, double* S_out) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  ssgsea_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, alpha, scale, norm, S_out, 0));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_gsva_exact_sharded_on_one_device(int device, int nshards, int fail_shard, const int32_t* Xp,
                                                    const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                                                    const int32_t* Gp, const int32_t* Gi, int32_t m, double tau, int rowtf,
                                                    int max_diff, double* S_out) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  gsva_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, tau, rowtf, max_diff, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_sing_exact_sharded_on_one_device(int device, int nshards, int fail_shard, const int32_t* Xp, const int32_t* Xi,
                                                    const double* X_or_x, int32_t g, int32_t n, const int32_t* Gp,
                                                    const int32_t* Gi, const int32_t* Dp, const int32_t* Di, int32_t m,
                                                    int center, double* total, double* up, double* down, double* total_disp,
                                                    double* up_disp, double* down_disp) try {
  return dispatch(on_hook(device, nshards, fail_shard), sing_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, Dp, Di, center, total,
                                                                         up, down, total_disp, up_disp, down_disp));
} catch (...) { return plaidhip::on_exception(); }

// impute != 0: K = k_full (k_full_down for the down sets), which must be given; impute == 0: they are not read
int plaidhip_ucell_exact_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                               int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, const int32_t* Dp, const int32_t* Di,
                               int32_t m, double max_rank, double w_neg, int impute, const double* k_full,
                               const double* k_full_down, double* total, double* up, double* down) try {
  PH_REQUIRE(!impute || k_full != nullptr || m == 0, "ucell_exact: impute needs k_full");
  return dispatch(on_devices(devices, ndev),
                  ucell_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, Dp, Di, max_rank, w_neg, impute ? k_full : nullptr,
                                   impute ? k_full_down : nullptr, total, up, down));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_aucell_exact_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x,
                                int32_t g, int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double auc_max_rank,
                                double* S_out) try {
  return dispatch(on_devices(devices, ndev), aucell_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, auc_max_rank, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_ucell_exact_sharded_on_one_device(int device, int nshards, int fail_shard, const int32_t* Xp,
                                                     const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                                                     const int32_t* Gp, const int32_t* Gi, const int32_t* Dp, const int32_t* Di,
                                                     int32_t m, double max_rank, double w_neg, int impute, const double* k_full,
                                                     const double* k_full_down, double* total, double* up, double* down) try {
  PH_REQUIRE(!impute || k_full != nullptr || m == 0, "ucell_exact: impute needs k_full");
  return dispatch(on_hook(device, nshards, fail_shard),
                  ucell_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, Dp, Di, max_rank, w_neg, impute ? k_full : nullptr,
                                   impute ? k_full_down : nullptr, total, up, down));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_aucell_exact_sharded_on_one_device(int device, int nshards, int fail_shard, const int32_t* Xp,
                                                      const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n,
                                                      const int32_t* Gp, const int32_t* Gi, int32_t m, double auc_max_rank,
                                                      double* S_out) try {
  return dispatch(on_hook(device, nshards, fail_shard), aucell_exact_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, auc_max_rank, S_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_gsea_multi(const int* devices, int ndev, const double* stat, const double* weight, int32_t g, int32_t c,
                        const int32_t* Gp, const int32_t* Gi, int32_t m, const int32_t* perm, int32_t nperm, uint64_t seed,
                        double* out, double* null_out) try {
  return dispatch(on_devices(devices, ndev), gsea_call(stat, weight, g, c, Gp, Gi, m, perm, nperm, seed, out, null_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_gsea_scored_multi(const int* devices, int ndev, const double* stat, const double* weight, int32_t g, int32_t c,
                               const int32_t* Gp, const int32_t* Gi, int32_t m, const int32_t* perm, int32_t nperm,
                               uint64_t seed, int score_type, double* out, double* null_out, int32_t* le_len,
                               int32_t* le_idx) try {
  return dispatch(on_devices(devices, ndev),
                  gsea_call(stat, weight, g, c, Gp, Gi, m, perm, nperm, seed, out, null_out, score_type, le_len, le_idx));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_gsea_scored_sharded_on_one_device(int device, int nshards, int fail_shard, const double* stat,
                                                     const double* weight, int32_t g, int32_t c, const int32_t* Gp,
                                                     const int32_t* Gi, int32_t m, const int32_t* perm, int32_t nperm,
                                                     uint64_t seed, int score_type, double* out, double* null_out,
                                                     int32_t* le_len, int32_t* le_idx) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  gsea_call(stat, weight, g, c, Gp, Gi, m, perm, nperm, seed, out, null_out, score_type, le_len, le_idx));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_gsea_multilevel_multi(const int* devices, int ndev, const double* stat, const double* weight, int32_t g, int32_t c,
                                   const int32_t* Gp, const int32_t* Gi, int32_t m, const int32_t* perm, int32_t nperm,
                                   uint64_t seed, int score_type, int32_t sample_size, int32_t sweeps, double eps,
                                   int32_t ml_min, double* out, double* null_out, int32_t* le_len, int32_t* le_idx,
                                   double* ml_out) try {
  return dispatch(on_devices(devices, ndev),
                  gsea_multilevel_call(stat, weight, g, c, Gp, Gi, m, perm, nperm, seed, score_type, sample_size, sweeps, eps,
                                       ml_min, out, null_out, le_len, le_idx, ml_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_gsea_multilevel_sharded_on_one_device(int device, int nshards, int fail_shard, const double* stat,
                                                         const double* weight, int32_t g, int32_t c, const int32_t* Gp,
                                                         const int32_t* Gi, int32_t m, const int32_t* perm, int32_t nperm,
                                                         uint64_t seed, int score_type, int32_t sample_size, int32_t sweeps,
                                                         double eps, int32_t ml_min, double* out, double* null_out,
                                                         int32_t* le_len, int32_t* le_idx, double* ml_out) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  gsea_multilevel_call(stat, weight, g, c, Gp, Gi, m, perm, nperm, seed, score_type, sample_size, sweeps, eps,
                                       ml_min, out, null_out, le_len, le_idx, ml_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_fisher_multi(const int* devices, int ndev, const int8_t* sig, int32_t g, int32_t c, const int32_t* Gp,
                          const int32_t* Gi, int32_t m, double* out, double* tot_out, int32_t* ov_len, int32_t* ov_idx) try {
  return dispatch(on_devices(devices, ndev), fisher_call(sig, g, c, Gp, Gi, m, out, tot_out, ov_len, ov_idx));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_limma_multi(const int* devices, int ndev, const double* A, int32_t rows, int32_t n, const double* design,
                         int32_t p, int32_t nfit, const int8_t* use, const double* K, int32_t q, double* out,
                         double* hyper) try {
  return dispatch(on_devices(devices, ndev), limma_call(A, rows, n, design, p, nfit, use, K, q, out, hyper));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_limma_sharded_on_one_device(int device, int nshards, int fail_shard, const double* A, int32_t rows, int32_t n,
                                               const double* design, int32_t p, int32_t nfit, const int8_t* use, const double* K,
                                               int32_t q, double* out, double* hyper) try {
  return dispatch(on_hook(device, nshards, fail_shard), limma_call(A, rows, n, design, p, nfit, use, K, q, out, hyper));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_limma_na_multi(const int* devices, int ndev, const double* A, int32_t rows, int32_t n, const double* design,
                            int32_t p, int32_t nfit, const int8_t* use, const double* K, int32_t q, double max_na, double* out,
                            double* hyper, double* dfres) try {
  return dispatch(on_devices(devices, ndev), limma_na_call(A, rows, n, design, p, nfit, use, K, q, max_na, out, hyper, dfres));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_voom_multi(const int* devices, int ndev, const double* counts, int32_t rows, int32_t n, const double* design,
                        int32_t p, const double* lib_size, double span, double* E, double* W, double* lib_out, double* offset,
                        double* knots_x, double* knots_y, int32_t* nknots) try {
  return dispatch(on_devices(devices, ndev),
                  voom_call(counts, rows, n, design, p, lib_size, span, E, W, lib_out, offset, knots_x, knots_y, nknots));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_voom_sharded_on_one_device(int device, int nshards, int fail_shard, const double* counts, int32_t rows,
                                              int32_t n, const double* design, int32_t p, const double* lib_size, double span,
                                              double* E, double* W, double* lib_out, double* offset, double* knots_x,
                                              double* knots_y, int32_t* nknots) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  voom_call(counts, rows, n, design, p, lib_size, span, E, W, lib_out, offset, knots_x, knots_y, nknots));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_limma_w_multi(const int* devices, int ndev, const double* A, const double* Wt, const double* aw, int32_t rows,
                           int32_t n, const double* design, int32_t p, int32_t nfit, const int8_t* use, const double* K, int32_t q,
                           double max_na, double* out, double* hyper, double* dfres) try {
  return dispatch(on_devices(devices, ndev), limma_w_call(A, Wt, aw, rows, n, design, p, nfit, use, K, q, max_na, out, hyper, dfres));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_limma_w_sharded_on_one_device(int device, int nshards, int fail_shard, const double* A, const double* Wt,
                                                 const double* aw, int32_t rows, int32_t n, const double* design, int32_t p,
                                                 int32_t nfit, const int8_t* use, const double* K, int32_t q, double max_na,
                                                 double* out, double* hyper, double* dfres) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  limma_w_call(A, Wt, aw, rows, n, design, p, nfit, use, K, q, max_na, out, hyper, dfres));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_limma_na_sharded_on_one_device(int device, int nshards, int fail_shard, const double* A, int32_t rows,
                                                  int32_t n, const double* design, int32_t p, int32_t nfit, const int8_t* use,
                                                  const double* K, int32_t q, double max_na, double* out, double* hyper,
                                                  double* dfres) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  limma_na_call(A, rows, n, design, p, nfit, use, K, q, max_na, out, hyper, dfres));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_camera_multi(const int* devices, int ndev, const double* X, int32_t g, int32_t n, const double* design, int32_t p,
                          int32_t nfit, const int8_t* use, const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi,
                          int32_t m, double inter_gene_cor, int allow_neg_cor, double* out, double* hyper) try {
  return dispatch(on_devices(devices, ndev),
                  camera_call(X, g, n, design, p, nfit, use, K, q, Gp, Gi, m, inter_gene_cor, allow_neg_cor, out, hyper));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_camera_sharded_on_one_device(int device, int nshards, int fail_shard, const double* X, int32_t g, int32_t n,
                                                const double* design, int32_t p, int32_t nfit, const int8_t* use,
                                                const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi, int32_t m,
                                                double inter_gene_cor, int allow_neg_cor, double* out, double* hyper) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  camera_call(X, g, n, design, p, nfit, use, K, q, Gp, Gi, m, inter_gene_cor, allow_neg_cor, out, hyper));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_fry_multi(const int* devices, int ndev, const double* X, int32_t g, int32_t n, const double* design, int32_t p,
                       int32_t nfit, const int8_t* use, const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi,
                       int32_t m, int standardize, double* out, double* hyper) try {
  return dispatch(on_devices(devices, ndev), fry_call(X, g, n, design, p, nfit, use, K, q, Gp, Gi, m, standardize, out, hyper));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_fry_sharded_on_one_device(int device, int nshards, int fail_shard, const double* X, int32_t g, int32_t n,
                                             const double* design, int32_t p, int32_t nfit, const int8_t* use, const double* K,
                                             int32_t q, const int32_t* Gp, const int32_t* Gi, int32_t m, int standardize,
                                             double* out, double* hyper) try {
  return dispatch(on_hook(device, nshards, fail_shard),
                  fry_call(X, g, n, design, p, nfit, use, K, q, Gp, Gi, m, standardize, out, hyper));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_roast_multi(const int* devices, int ndev, const double* X, int32_t g, int32_t n, const double* design, int32_t p,
                         int32_t nfit, const int8_t* use, const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi,
                         int32_t m, int set_statistic, int zscore, int32_t nrot, uint64_t seed, int midp,
                         const double* rotations, double* out, double* hyper) try {
  return dispatch(on_devices(devices, ndev), roast_call(X, g, n, design, p, nfit, use, K, q, Gp, Gi, m, set_statistic, zscore,
                                                        nrot, seed, midp, rotations, out, hyper));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_roast_sharded_on_one_device(int device, int nshards, int fail_shard, const double* X, int32_t g, int32_t n,
                                               const double* design, int32_t p, int32_t nfit, const int8_t* use,
                                               const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi, int32_t m,
                                               int set_statistic, int zscore, int32_t nrot, uint64_t seed, int midp,
                                               const double* rotations, double* out, double* hyper) try {
  return dispatch(on_hook(device, nshards, fail_shard), roast_call(X, g, n, design, p, nfit, use, K, q, Gp, Gi, m, set_statistic,
                                                                    zscore, nrot, seed, midp, rotations, out, hyper));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_romer_multi(const int* devices, int ndev, const double* X, int32_t g, int32_t n, const double* design, int32_t p,
                         int32_t nfit, const int8_t* use, const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi,
                         int32_t m, int set_statistic, int32_t nrot, uint64_t seed, int shrink_resid, const double* shrink,
                         const double* rotations, double* out, double* hyper) try {
  return dispatch(on_devices(devices, ndev), romer_call(X, g, n, design, p, nfit, use, K, q, Gp, Gi, m, set_statistic, nrot, seed,
                                                        shrink_resid, shrink, rotations, out, hyper));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_romer_sharded_on_one_device(int device, int nshards, int fail_shard, const double* X, int32_t g, int32_t n,
                                               const double* design, int32_t p, int32_t nfit, const int8_t* use,
                                               const double* K, int32_t q, const int32_t* Gp, const int32_t* Gi, int32_t m,
                                               int set_statistic, int32_t nrot, uint64_t seed, int shrink_resid,
                                               const double* shrink, const double* rotations, double* out, double* hyper) try {
  return dispatch(on_hook(device, nshards, fail_shard), romer_call(X, g, n, design, p, nfit, use, K, q, Gp, Gi, m, set_statistic,
                                                                    nrot, seed, shrink_resid, shrink, rotations, out, hyper));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_fisher_sharded_on_one_device(int device, int nshards, int fail_shard, const int8_t* sig, int32_t g, int32_t c,
                                                const int32_t* Gp, const int32_t* Gi, int32_t m, double* out, double* tot_out,
                                                int32_t* ov_len, int32_t* ov_idx) try {
  return dispatch(on_hook(device, nshards, fail_shard), fisher_call(sig, g, c, Gp, Gi, m, out, tot_out, ov_len, ov_idx));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_rankcor_multi(const int* devices, int ndev, const double* stat, int32_t g, int32_t c, const int32_t* Gp,
                           const int32_t* Gi, int32_t m, int use_rank, int ties, double* out, double* tot_out) try {
  return dispatch(on_devices(devices, ndev), rankcor_call(stat, g, c, Gp, Gi, m, use_rank, ties, out, tot_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_rankcor_sharded_on_one_device(int device, int nshards, int fail_shard, const double* stat, int32_t g,
                                                 int32_t c, const int32_t* Gp, const int32_t* Gi, int32_t m, int use_rank,
                                                 int ties, double* out, double* tot_out) try {
  return dispatch(on_hook(device, nshards, fail_shard), rankcor_call(stat, g, c, Gp, Gi, m, use_rank, ties, out, tot_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_plage_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g,
                         int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double tol, int32_t maxit, double* S_out,
                         double* info_out, double* load_out) try {
  return dispatch(on_devices(devices, ndev), plage_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, tol, maxit, S_out, info_out, load_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_zscore_multi(const int* devices, int ndev, const int32_t* Xp, const int32_t* Xi, const double* X_or_x, int32_t g,
                          int32_t n, const int32_t* Gp, const int32_t* Gi, int32_t m, double* S_out, double* size_out) try {
  return dispatch(on_devices(devices, ndev), zscore_call({Xp, Xi, X_or_x, g, n, Gp, Gi, m}, S_out, size_out));
} catch (...) { return plaidhip::on_exception(); }

// which Gram kernel replaid.plage launches: 0 the product's (rounded products), 1 the MFMA form
int plaidhip_debug_plage_gram(int mode) try {
  PH_REQUIRE(mode == 0 || mode == 1, "debug_plage_gram: mode = %d", mode);
  plaidhip::debug_plage_set_gram(mode);
  return PLAIDHIP_OK;
} catch (...) { return plaidhip::on_exception(); }

// method: kPlage (18) or kZscore (19), which takes no tol / maxit / load_out and the sizes in info_out
int plaidhip_debug_plage_sharded_on_one_device(int device, int nshards, int fail_shard, int method, const int32_t* Xp,
                                               const int32_t* Xi, const double* X_or_x, int32_t g, int32_t n, const int32_t* Gp,
                                               const int32_t* Gi, int32_t m, double tol, int32_t maxit, double* S_out,
                                               double* info_out, double* load_out) try {
  PH_REQUIRE(method == kPlage || method == kZscore, "debug_plage_sharded: method = %d", method);
  const Operands x{Xp, Xi, X_or_x, g, n, Gp, Gi, m};
  return dispatch(on_hook(device, nshards, fail_shard),
                  method == kPlage ? plage_call(x, tol, maxit, S_out, info_out, load_out) : zscore_call(x, S_out, info_out));
} catch (...) { return plaidhip::on_exception(); }

int plaidhip_debug_gsea_sharded_on_one_device(int device, int nshards, int fail_shard, const double* stat, const double* weight,
                                              int32_t g, int32_t c, const int32_t* Gp, const int32_t* Gi, int32_t m,
                                              const int32_t* perm, int32_t nperm, uint64_t seed, double* out,
                                              double* null_out) try {
  return dispatch(on_hook(device, nshards, fail_shard), gsea_call(stat, weight, g, c, Gp, Gi, m, perm, nperm, seed, out, null_out));
} catch (...) { return plaidhip::on_exception(); }

}  // extern "C"
