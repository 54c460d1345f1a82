// Sanitizer run of the library's host code (ASan / UBSan on the CPU build): the index planners
// of geneset.cpp (tile schedules, edge colouring, pair slices, scatter segments -- 840 lines of index arithmetic),
// the GMT parser and gmt2mat of gmt.cpp, and the p-value tails and plaid.limma's host half of stats.cpp.  Built and run by
// `make -C plaid_amd/csrc host-asan`; any sanitizer report aborts with a non-zero status.
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../plaid_amd/csrc/common.h"

extern "C" int plaidhip_debug_pair_plan_check(int32_t g, int32_t m, const int32_t* Gp, const int32_t* Gi, int32_t waves,
                                              int64_t out[8]);

#define REQUIRE(cond)                                                          \
  do {                                                                         \
    if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
  } while (0)

static void random_sets(std::mt19937_64& rng, int32_t g, int32_t m, int kmin, int kmax, bool sorted, std::vector<int32_t>& Gp,
                        std::vector<int32_t>& Gi) {
  std::vector<int32_t> sizes(m);
  std::uniform_real_distribution<double> u(std::log((double)kmin), std::log((double)kmax));
  for (auto& k : sizes) k = std::min<int32_t>(g, std::max<int32_t>(0, (int32_t)std::lround(std::exp(u(rng))) - (rng() % 11 == 0 ? 1000000 : 0)));
  if (sorted) std::sort(sizes.rbegin(), sizes.rend());
  Gp.assign(1, 0);
  Gi.clear();
  std::vector<int32_t> perm(g);
  for (int32_t i = 0; i < g; ++i) perm[i] = i;
  for (int32_t j = 0; j < m; ++j) {
    const int32_t k = std::max<int32_t>(0, sizes[j]);
    for (int32_t t = 0; t < k; ++t) std::swap(perm[t], perm[t + rng() % (g - t)]);
    std::vector<int32_t> mem(perm.begin(), perm.begin() + k);
    std::sort(mem.begin(), mem.end());
    Gi.insert(Gi.end(), mem.begin(), mem.end());
    Gp.push_back((int32_t)Gi.size());
  }
}

static void plans() {
  std::mt19937_64 rng(7);
  struct Case { int32_t g, m; int kmin, kmax; bool sorted; };
  const Case cases[] = {{37, 3, 1, 30, true},      {1000, 70, 1, 200, false},  {10224, 130, 5, 300, true},
                        {10226, 129, 5, 300, false}, {20000, 700, 15, 500, true}, {20448, 65, 1, 2000, false},
                        {20449, 64, 15, 500, true}, {45000, 300, 15, 500, false}, {1, 5, 1, 1, true},
                        {20000, 5000, 15, 500, true}, {20000, 50000, 15, 500, true}, {10225, 6144, 15, 40, true},
                        {30001, 6145, 15, 40, false}};
  plaidhip_ctx ctx;
  for (const Case& c : cases) {
    std::vector<int32_t> Gp, Gi;
    random_sets(rng, c.g, c.m, c.kmin, c.kmax, c.sorted, Gp, Gi);
    int64_t out[8] = {0};
    REQUIRE(plaidhip_debug_pair_plan_check(c.g, c.m, Gp.data(), Gi.data(), 16, out) == PLAIDHIP_OK);
    REQUIRE(out[2] == (int64_t)Gi.size());   // every membership scheduled exactly once
    REQUIRE(out[4] == 0);                    // none for the wrong set, twice, or outside its slice
    // more than one slice and at most 12 x 8 tiles: dealt to 12 wavefronts, no more than 8 tiles each (register partials)
    REQUIRE(out[5] == ((c.g > plaidhip::kMaxLdsGenesPair && (c.m + 63) / 64 <= plaidhip::kPairRegWaves * plaidhip::kPairRegPartials) ? 1 : 0));
    if (out[5]) REQUIRE(out[6] <= plaidhip::kPairRegPartials && out[7] == plaidhip::kPairRegWaves);
    plaidhip_geneset* gs = nullptr;
    REQUIRE(plaidhip_geneset_create(&ctx, c.g, c.m, Gp.data(), Gi.data(), &gs) == PLAIDHIP_OK);
    int64_t info[8];
    REQUIRE(plaidhip_geneset_info(gs, info) == PLAIDHIP_OK);
    REQUIRE(info[0] == c.g && info[1] == c.m && info[2] == (int64_t)Gi.size() && info[3] >= info[2]);
    REQUIRE(plaidhip_geneset_destroy(gs) == PLAIDHIP_OK);
    printf("  plan g=%d m=%d z=%zu: pair slices %" PRId64 ", padded slots %" PRId64 " (one-column) / %" PRId64 " (pair)\n", c.g, c.m,
           Gi.size(), out[0], info[3], info[7]);
  }
  // rejected inputs: a decreasing pointer array, an index out of range
  {
    plaidhip_geneset* gs = nullptr;
    const int32_t badp[] = {0, 3, 2}, gi[] = {0, 1, 2};
    REQUIRE(plaidhip_geneset_create(&ctx, 5, 2, badp, gi, &gs) == PLAIDHIP_EINVAL);
    const int32_t p2[] = {0, 2}, gi2[] = {0, 9};
    REQUIRE(plaidhip_geneset_create(&ctx, 5, 1, p2, gi2, &gs) == PLAIDHIP_EINVAL);
  }
}

static void gmt() {
  std::mt19937_64 rng(11);
  for (int rep = 0; rep < 40; ++rep) {
    // random GMT text: comments, blank lines, empty fields, "NA", repeats, spaces inside the gene field, CRLF, no
    // trailing newline, very long lines
    std::string text;
    const int nsets = (int)(rng() % 60);
    for (int j = 0; j < nsets; ++j) {
      if (rng() % 9 == 0) text += "# comment\tline\n";
      if (rng() % 13 == 0) text += "\n";
      text += "SET_" + std::to_string(rng() % 40) + "\t" + (rng() % 3 ? "src" : "") ;
      const int k = (int)(rng() % (rep == 7 ? 20000 : 50));
      for (int t = 0; t < k; ++t) {
        text += (rng() % 7 == 0) ? " " : "\t";
        const int r = (int)(rng() % 10);
        text += r == 0 ? "NA" : (r == 1 ? "" : "G" + std::to_string(rng() % 300));
      }
      text += (rng() % 5 == 0) ? "\r\n" : "\n";
    }
    if (!text.empty() && rng() % 2) text.pop_back();
    for (int raw = 0; raw < 2; ++raw) {
      plaidhip_gmt* gm = nullptr;
      REQUIRE(plaidhip_gmt_parse(text.data(), (int64_t)text.size(), raw, (int)(rng() % 2), rng() % 4 == 0 ? 5 : 0, &gm) == PLAIDHIP_OK);
      const int64_t ns = plaidhip_gmt_nsets(gm);
      int64_t total = 0;
      for (int64_t j = 0; j < ns; ++j) {
        REQUIRE(plaidhip_gmt_set_name(gm, j) != nullptr);
        const int64_t k = plaidhip_gmt_set_size(gm, j);
        for (int64_t t = 0; t < k; ++t) total += (int64_t)strlen(plaidhip_gmt_set_gene(gm, j, t));
      }
      int64_t nb = 0;
      REQUIRE(plaidhip_gmt_text(gm, &nb) != nullptr || ns == 0);
      plaidhip_gmtmat* mat = nullptr;
      const char* bg[] = {"G1", "G2", "G299", "nope"};
      REQUIRE(plaidhip_gmt2mat(gm, rep % 3 == 0 ? 25 : -1, rep % 4 == 0 ? 7 : -1, rep % 5 == 0 ? bg : nullptr, rep % 5 == 0 ? 4 : 0, &mat) == PLAIDHIP_OK);
      int64_t dims[3];
      REQUIRE(plaidhip_gmtmat_dims(mat, dims) == PLAIDHIP_OK);
      const int32_t* p = plaidhip_gmtmat_p(mat);
      const int32_t* ii = plaidhip_gmtmat_i(mat);
      for (int64_t j = 0; j < dims[1]; ++j)
        for (int32_t q = p[j]; q < p[j + 1]; ++q) REQUIRE(ii[q] >= 0 && ii[q] < dims[0] && (q == p[j] || ii[q - 1] < ii[q]));
      REQUIRE(dims[1] == 0 || p[dims[1]] == dims[2]);
      for (int axis = 0; axis < 2; ++axis) {
        int64_t bytes = 0;
        const char* names = plaidhip_gmtmat_names(mat, axis, &bytes);
        REQUIRE(names != nullptr || dims[axis] == 0);
      }
      REQUIRE(plaidhip_gmtmat_destroy(mat) == PLAIDHIP_OK);
      REQUIRE(plaidhip_gmt_destroy(gm) == PLAIDHIP_OK);
      (void)total;
    }
  }
  printf("  gmt: 80 random texts parsed, listed and turned into matrices\n");
}

static void tails() {
  using namespace plaidhip;
  std::mt19937_64 rng(3);
  std::normal_distribution<double> N(0.0, 1.0);
  std::vector<double> p;
  for (int rep = 0; rep < 2000; ++rep) {
    const double k = 1 + (double)(rng() % 400), s1 = N(rng) * k, s2 = s1 * s1 / k + std::fabs(N(rng)) * k;
    double mean = 0, diff = 0;
    const double a = onesample_p(k, s1, s2, &mean);
    const double b = twosample_p(5000.0, k, s1, s2, N(rng) * 5000, 7000.0 + std::fabs(N(rng)) * 100, &diff);
    const double c = welch_p(N(rng), N(rng), std::fabs(N(rng)), std::fabs(N(rng)), 2 + (double)(rng() % 30), 2 + (double)(rng() % 30));
    for (double v : {a, b, c}) REQUIRE(std::isnan(v) || (v >= 0.0 && v <= 1.0));
    const double q[3] = {clamp_p(a), clamp_p(b), clamp_p(c)};
    for (int method = 0; method < 2; ++method) {
      const double m = combine_p(q, 3, method);
      REQUIRE(std::isnan(m) || (m >= 0.0 && m <= 1.0));
    }
    p.push_back(rep % 50 == 0 ? NAN : q[rep % 3]);
  }
  // degenerate inputs: zero variance, one observation, empty
  double tmp;
  (void)onesample_p(1.0, 3.0, 9.0, &tmp);
  (void)onesample_p(0.0, 0.0, 0.0, &tmp);
  (void)welch_p(1.0, 1.0, 0.0, 0.0, 2.0, 2.0);
  std::vector<double> q(p.size());
  p_adjust_fdr(p.data(), (int64_t)p.size(), q.data());
  p_adjust_fdr(p.data(), 0, q.data());
  for (size_t i = 0; i < p.size(); ++i) REQUIRE(std::isnan(p[i]) ? std::isnan(q[i]) : (q[i] >= p[i] - 1e-15 && q[i] <= 1.0));
  printf("  stats: 2000 random moment sets through the t / chi^2 / normal tails, combine_p and BH\n");
}

// plaid.limma's host half: designs that fit and designs that are refused through plaidhip_limma_design, and
// plaidhip_limma_finish on both sides of its thread threshold, with rows that are not ok
static void limma() {
  std::mt19937_64 rng(7);
  std::normal_distribution<double> N(0.0, 1.0);
  for (int p : {1, 2, 3, 32}) {
    const int n = p + 1 + (int)(rng() % 9), q = p;
    std::vector<double> D((size_t)n * p), Q((size_t)n * p), R((size_t)p * p), v((size_t)p * q), u((size_t)q);
    std::vector<int8_t> use((size_t)n + 3, 1);
    for (auto& x : D) x = N(rng);
    for (int c = 0; c < n; ++c) D[(size_t)c] = 1.0;
    int64_t nf = 0;
    REQUIRE(plaidhip_limma_design(D.data(), n, p, nullptr, nullptr, q, 1, Q.data(), R.data(), v.data(), u.data(), &nf) == PLAIDHIP_OK);
    REQUIRE(nf == n);
    for (int j = 0; j < q; ++j) REQUIRE(u[(size_t)j] > 0.0);
    // three more samples that take no part and hold NaN; nothing but u asked for
    std::vector<double> D2((size_t)(n + 3) * p, NAN);
    for (int k = 0; k < p; ++k)
      for (int c = 0; c < n; ++c) D2[(size_t)k * (n + 3) + c + (c >= 2 ? 3 : 0)] = D[(size_t)k * n + c];
    use[2] = use[3] = use[4] = 0;
    std::vector<double> u2((size_t)q);
    REQUIRE(plaidhip_limma_design(D2.data(), n + 3, p, use.data(), nullptr, q, 2, nullptr, nullptr, nullptr, u2.data(), &nf) == PLAIDHIP_OK);
    REQUIRE(nf == n);
    for (int j = 0; j < q; ++j) REQUIRE(std::fabs(u2[(size_t)j] - u[(size_t)j]) <= 1e-12 * u[(size_t)j]);
    if (p >= 2) {   // a duplicated column, n_f = p
      for (int c = 0; c < n; ++c) D[(size_t)(p - 1) * n + c] = D[(size_t)c];
      REQUIRE(plaidhip_limma_design(D.data(), n, p, nullptr, nullptr, q, 1, Q.data(), nullptr, nullptr, nullptr, nullptr) == PLAIDHIP_EINVAL);
      REQUIRE(plaidhip_limma_design(D.data(), p, p, nullptr, nullptr, q, 1, nullptr, nullptr, nullptr, nullptr, nullptr) == PLAIDHIP_EINVAL);
    }
  }
  for (int rows : {1, 3, 500, 70001}) {
    const int p = 2, nfit = 2, q = 2;
    std::vector<double> E((size_t)nfit * (p + 1) * rows), rss((size_t)nfit * rows), v((size_t)p * q * nfit), u((size_t)q * nfit, 0.5);
    std::vector<double> out((size_t)rows * 6 * q * nfit), hyper((size_t)nfit * 4);
    for (auto& x : E) x = N(rng);
    for (auto& x : v) x = N(rng);
    for (auto& x : rss) { const double z = N(rng); x = z * z; }
    if (rows >= 3) { rss[1] = NAN; rss[(size_t)rows + 2] = INFINITY; rss[0] = 0.0; }
    const int64_t nf[2] = {9, 3};
    REQUIRE(plaidhip_limma_finish(rows, p, nfit, q, E.data(), rss.data(), nf, v.data(), u.data(), out.data(), hyper.data()) == PLAIDHIP_OK);
    for (size_t e = 0; e < (size_t)rows; ++e) {
      const double pv = out[3 * (size_t)rows + e];
      REQUIRE(std::isnan(pv) || (pv >= 0.0 && pv <= 1.0));
    }
    REQUIRE(hyper[3] == (double)(rows >= 3 ? rows - 1 : rows));
    // na = "fit": the rows' own df.residual (three values, NaN for a row that is not fitted) and u
    std::vector<double> drow((size_t)nfit * rows), urow((size_t)nfit * q * rows, 0.5), hyper5((size_t)nfit * 5);
    for (size_t e = 0; e < drow.size(); ++e) drow[e] = (double)(1 + e % 3);
    if (rows >= 3) drow[2] = NAN;
    REQUIRE(plaidhip_limma_finish_na(rows, p, nfit, q, E.data(), rss.data(), nf, v.data(), drow.data(), urow.data(), out.data(),
                                     hyper5.data()) == PLAIDHIP_OK);
    REQUIRE(hyper5[3] == (double)(rows >= 3 ? rows - 2 : rows));
    REQUIRE(rows < 3 || std::isnan(out[2]));
  }
  // one incomplete row through the shared solve (csrc/lmfit_na.h) at every p: the rows of an orthonormal Q that are missing
  for (int p = 1; p <= PLAIDHIP_LIMMA_NA_MAX_COEF; ++p) {
    const int n = 24, q = 2;
    std::vector<double> D((size_t)n * p), Q((size_t)n * p), R((size_t)p * p), v((size_t)p * q), u((size_t)q), K((size_t)p * q);
    for (auto& x : D) x = N(rng);
    for (auto& x : K) x = N(rng);
    int64_t nf = 0;
    REQUIRE(plaidhip_limma_design(D.data(), n, p, nullptr, K.data(), q, 1, Q.data(), R.data(), v.data(), u.data(), &nf) == PLAIDHIP_OK);
    for (int nmis : {0, 1, 5, n - p}) {   // (n - p missing: no residual degree of freedom)
      std::vector<double> qmis((size_t)(nmis > 0 ? nmis : 1) * p), Ep((size_t)p), gamma((size_t)p), uu((size_t)q), piv((size_t)p);
      for (int i = 0; i < nmis; ++i)
        for (int k = 0; k < p; ++k) qmis[(size_t)i * p + k] = Q[(size_t)k * n + i];
      for (auto& x : Ep) x = N(rng);
      int32_t ok = -1;
      REQUIRE(plaidhip_limma_na_solve(p, nmis, qmis.data(), Ep.data(), n - nmis, v.data(), q, gamma.data(), uu.data(), piv.data(),
                                      &ok) == PLAIDHIP_OK);
      REQUIRE(ok == (nmis < n - p ? 1 : 0));
      if (ok) for (int j = 0; j < q; ++j) REQUIRE(uu[(size_t)j] >= u[(size_t)j] * (1.0 - 1e-12));   // missing samples never shrink it
      if (nmis == 0) for (int k = 0; k < p; ++k) REQUIRE(gamma[(size_t)k] == Ep[(size_t)k]);
    }
  }
  printf("  limma: designs of 1, 2, 3 and 32 coefficients, refused ones, the finish step up to 70,001 rows on host threads, with\n"
         "         per-row df, and the refit of an incomplete row at 1 .. %d coefficients\n", PLAIDHIP_LIMMA_NA_MAX_COEF);
}

// plaid.rankcor's host half: plaidhip_rankcor_finish on tie-free lists at the integer limits (n = 131,072: 128-bit products),
// on the degenerate tables and on operands it must refuse
static void rankcor() {
  for (int64_t n : {2, 3, 10, 1000, 131072}) {
    const int32_t m = 6;
    // z = 2, 4, ..., 2n: T1 = n (n + 1), T2 = 2 n (n + 1) (2n + 1) / 3; a set of the k highest ranks has A = k (2n - k + 1)
    const int64_t T1 = n * (n + 1), T2 = 2 * n * (n + 1) * (2 * n + 1) / 3;
    const int64_t ks[m] = {0, 1, n / 2, n - 1, n, 1};
    std::vector<int64_t> k(ks, ks + m), A((size_t)m);
    for (int j = 0; j < m; ++j) A[(size_t)j] = k[(size_t)j] * (2 * n - k[(size_t)j] + 1);
    A[5] = 2;   // the lowest rank alone
    std::vector<double> out((size_t)m * 5, -7.0);
    REQUIRE(plaidhip_rankcor_finish(m, 1, &n, &T1, &T2, k.data(), A.data(), out.data()) == PLAIDHIP_OK);
    for (int j = 0; j < m; ++j) {
      const double rho = out[(size_t)m + j], pv = out[3 * (size_t)m + j];
      REQUIRE(out[(size_t)j] == (double)k[(size_t)j]);
      REQUIRE((k[(size_t)j] == 0 || k[(size_t)j] == n) ? std::isnan(rho) : (rho >= -1.0 && rho <= 1.0));
      REQUIRE(std::isnan(pv) || (pv >= 0.0 && pv <= 1.0));
    }
    REQUIRE(n < 3 || (out[(size_t)m + 1] > 0.0 && out[(size_t)m + 5] < 0.0));
    const int64_t bad = n + 1;
    REQUIRE(plaidhip_rankcor_finish(1, 1, &n, &T1, &T2, &bad, A.data(), out.data()) == PLAIDHIP_EINVAL);
  }
  printf("  rankcor: the finish step at n = 2 .. 131,072, k = 0 .. n, and refused operands\n");
}

// plaid.camera's host half: plaidhip_camera_residual_row with samples left out and genes that are not ok, and
// plaidhip_camera_finish with estimated and fixed correlations over sets of 0 .. G ok members and universes of 0 .. 3 genes
static void camera() {
  std::mt19937_64 rng(11);
  std::normal_distribution<double> N(0.0, 1.0);
  for (int p : {1, 4, 32}) {
    const int n = p + 5;
    std::vector<double> x((size_t)n), Q((size_t)n * p), E((size_t)p), z((size_t)n, -7.0);
    std::vector<int8_t> use((size_t)n, 1);
    use[1] = 0;
    for (auto& v : x) v = N(rng);
    for (auto& v : Q) v = N(rng);
    for (auto& v : E) v = N(rng);
    x[1] = NAN;
    REQUIRE(plaidhip_camera_residual_row(n, p, x.data(), Q.data(), use.data(), E.data(), 2.5, 4.0, z.data()) == PLAIDHIP_OK);
    REQUIRE(z[1] == 0.0);
    for (int c = 0; c < n; ++c) REQUIRE(std::isfinite(z[(size_t)c]));
    REQUIRE(plaidhip_camera_residual_row(n, p, x.data(), Q.data(), nullptr, E.data(), NAN, 4.0, z.data()) == PLAIDHIP_OK);
    for (int c = 0; c < n; ++c) REQUIRE(z[(size_t)c] == 0.0);
    REQUIRE(plaidhip_camera_residual_row(n, p, x.data(), Q.data(), nullptr, E.data(), 0.0, 4.0, z.data()) == PLAIDHIP_OK);   // the floor
    REQUIRE(std::isnan(z[1]) && std::isfinite(z[0]));
  }
  for (int g : {0, 1, 2, 3, 400}) {
    const int m = 5, nfit = 2, q = 2;
    std::vector<double> t((size_t)g * q * nfit), sumt((size_t)m * q * nfit), cnt((size_t)m * nfit), ss((size_t)m * nfit);
    std::vector<int8_t> ok((size_t)g * nfit, 1);
    for (auto& v : t) v = N(rng);
    if (g >= 3) { ok[1] = 0; t[1] = NAN; }
    const int G0 = g >= 3 ? g - 1 : g;
    const int sizes[m] = {0, 1, G0 / 2, G0 > 0 ? G0 - 1 : 0, G0};
    for (int f = 0; f < nfit; ++f)
      for (int s = 0; s < m; ++s) {
        cnt[(size_t)f * m + s] = (double)std::min(sizes[s], f == 0 ? G0 : g);
        ss[(size_t)f * m + s] = std::fabs(N(rng)) * 10.0 * (sizes[s] + 1);
        for (int j = 0; j < q; ++j) sumt[((size_t)f * q + j) * m + s] = N(rng) * sizes[s];
      }
    const double dres[2] = {6.0, 1.0}, dprior[2] = {3.5, INFINITY};
    std::vector<double> out((size_t)m * 8 * q * nfit, -7.0), gdf((size_t)nfit * 2, -7.0);
    for (int mode = 0; mode < 3; ++mode) {
      REQUIRE(plaidhip_camera_finish(g, m, nfit, q, t.data(), ok.data(), sumt.data(), cnt.data(), mode == 2 ? nullptr : ss.data(), dres,
                                     dprior, mode == 2 ? -0.05 : NAN, mode == 1, out.data(), gdf.data()) == PLAIDHIP_OK);
      REQUIRE(gdf[0] == (double)G0 && gdf[2] == (double)g);
      for (size_t col = 0; col < (size_t)q * nfit; ++col)
        for (int s = 0; s < m; ++s) {
          const double* o = out.data() + col * 8 * m;
          const double pv = o[6 * m + s], fdr = o[7 * m + s];
          REQUIRE(o[s] == cnt[(col / q) * m + s]);
          REQUIRE(std::isnan(pv) ? std::isnan(fdr) : (pv >= 0.0 && pv <= 1.0 && fdr >= pv - 1e-15 && fdr <= 1.0));
          REQUIRE(g >= 3 || std::isnan(pv));
        }
    }
    REQUIRE(plaidhip_camera_finish(g, m, nfit, q, t.data(), ok.data(), sumt.data(), cnt.data(), nullptr, dres, dprior, 1.0, 0, out.data(),
                                   gdf.data()) == PLAIDHIP_EINVAL);
  }
  printf("  camera: the residual row at 1, 4 and 32 coefficients, the finish step over universes of 0 .. 400 genes, refused operands\n");
}

// plaid.romer's host half: the shrink over universes of 0 .. 400 genes (no non-null gene, a few, all; t with NaN and +-Inf;
// finite and infinite df), and the tables from counts (empty sets, a set above the mean50 cap)
static void romer() {
  std::mt19937_64 rng(29);
  std::normal_distribution<double> N(0.0, 1.0);
  for (int U : {0, 1, 2, 3, 60, 400})
    for (int kind = 0; kind < 4; ++kind) {
      std::vector<double> t((size_t)U), c((size_t)U, -7.0);
      for (int i = 0; i < U; ++i) t[(size_t)i] = N(rng) * (kind == 0 ? 0.2 : 1.0) + (kind >= 2 && i % (kind == 3 ? 1 : 4) == 0 ? 6.0 : 0.0);
      if (U >= 3 && kind == 1) { t[0] = NAN; t[1] = INFINITY; t[2] = -INFINITY; }
      double prop = -7.0;
      const double nu = kind == 1 ? INFINITY : 9.5;
      REQUIRE(plaidhip_romer_shrink(U, t.data(), 0.5, 1.25, nu, c.data(), &prop) == PLAIDHIP_OK);
      REQUIRE(prop >= 0.0 || U > 0);
      for (int i = 0; i < U; ++i) REQUIRE(c[(size_t)i] > 0.0 && c[(size_t)i] <= 1.0);
    }
  double prop = 0.0, one = 1.0;
  REQUIRE(plaidhip_romer_shrink(1, &one, 0.0, 1.0, 5.0, &one, &prop) == PLAIDHIP_EINVAL);
  REQUIRE(plaidhip_romer_shrink(1, nullptr, 1.0, 1.0, 5.0, &one, &prop) == PLAIDHIP_EINVAL);
  for (int m : {0, 1, 7, 300}) {
    const int nfit = 2, q = 2, nrot = 99;
    std::vector<int32_t> cnt((size_t)3 * m * q * nfit);
    std::vector<double> msize((size_t)m * nfit), out((size_t)m * 7 * q * nfit, -7.0);
    for (auto& v : cnt) v = (int32_t)(rng() % (nrot + 1));
    for (auto& v : msize) v = (double)(rng() % 40);
    if (m >= 7) msize[3] = 16385.0;
    for (int stat = 0; stat < 3; ++stat) {
      REQUIRE(plaidhip_romer_finish(m, nfit, q, nrot, stat, cnt.data(), msize.data(), out.data()) == PLAIDHIP_OK);
      for (size_t col = 0; col < (size_t)q * nfit; ++col)
        for (int s = 0; s < m; ++s) {
          const double* o = out.data() + col * 7 * m;
          const double mm = msize[(col / q) * m + s];
          REQUIRE(o[s] == mm);
          for (int e = 0; e < 3; ++e) {
            const double pv = o[(1 + e) * m + s], fdr = o[(4 + e) * m + s];
            REQUIRE(std::isnan(pv) == (mm < 1.0 || (stat == 2 && mm > 16384.0)));
            REQUIRE(std::isnan(pv) ? std::isnan(fdr) : (pv > 0.0 && pv <= 1.0 && fdr >= pv - 1e-15 && fdr <= 1.0));
          }
        }
    }
    REQUIRE(plaidhip_romer_finish(m, nfit, q, 0, 0, cnt.data(), msize.data(), out.data()) == PLAIDHIP_EINVAL);
  }
  printf("  romer: the shrink over universes of 0 .. 400 genes, the tables from counts, refused operands\n");
}

int main() {
  printf("[host-asan] planners\n");
  plans();
  printf("[host-asan] GMT parser / gmt2mat\n");
  gmt();
  printf("[host-asan] p-value tails\n");
  tails();
  printf("[host-asan] plaid.limma's design and finish\n");
  limma();
  printf("[host-asan] plaid.rankcor's finish\n");
  rankcor();
  printf("[host-asan] plaid.camera's residual row and finish\n");
  camera();
  printf("[host-asan] plaid.romer's shrink and finish\n");
  romer();
  printf("[host-asan] ok\n");
  return 0;
}
